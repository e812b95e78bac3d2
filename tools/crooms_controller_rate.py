"""Kernel time of the C-ROOMS closed-loop rollouts (csrc/crooms.hip crooms_rollout_ctrl) against the open loop
(crooms_rollout) in one session on one build: layout "4", rng_mode philox, 2^21 envs, K = 128 steps per launch, the
default action noise and failure probability.

  open loop:   rollout_plan on uniform random actions, same action type and obs as the closed-loop row it is paired
               with;
  closed loop: a uniform controller,
                 cardinal actions with the `hansen` obs (80 obs values: the table is staged in LDS), M = 1 and M = 4
                 nodes, storing all six outputs and storing nothing (pure policy evaluation);
                 ordinal actions with the `hansen8` obs (2,304 obs values: 72 KB at M = 1, read from global memory),
                 M = 1, all six outputs.

Each measurement: two warm-up launches, then 5 launches timed by the handle's hipEvent pairs around the kernel. Each
closed-loop row is paired with the open loop: one discarded pair, then two alternated pairs (open, closed, open,
closed); `ratio_to_open_loop` is the mean of its two closed-loop measurements over the mean of its two open-loop ones.
`frac_hbm`: algorithmic bytes per env-step over the kernel time, as a fraction of 8 TB/s. The ratios are recorded, not
gated.

Usage (GPU box): python tools/crooms_controller_rate.py [out.json] -> one JSON line per row (also written to out.json).
"""
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-po-taxi_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import CRoomsEnv  # noqa: E402

HBM = 8e12
B, K, REPS, PAIRS = 1 << 21, 128, 5, 2
FULL = ("obs", "actions", "nodes", "rew", "term", "trunc")
NBYTES = {"obs": 4, "actions": 4, "nodes": 1, "rew": 4, "term": 1, "trunc": 1}


def make_env(action_type, obs_type):
    env = CRoomsEnv(B, layout="4", action_type=action_type, obs_type=obs_type, rng_mode="philox")
    env.reset(seed=0)
    return env


def timed(env, launch):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    env.set_profiling(True)
    env.profile_read()
    for _ in range(REPS):
        launch()
    ms, n = env.profile_read()
    env.set_profiling(False)
    return ms * 1e3 / (n * K)


def open_loop_launcher(env):
    g = torch.Generator(device=env.device).manual_seed(1)
    acts = torch.randint(0, int(env.single_action_space.n), (K, B), device=env.device, generator=g, dtype=torch.int32)
    run, _ = env.rollout_plan(acts)
    return run


def closed_loop_row(what, action_type, obs_type, M, store, open_env, open_run):
    env = make_env(action_type, obs_type)
    n_obs, A = int(env.single_observation_space.n), int(env.single_action_space.n)
    env.set_controller(probs=np.full((M, n_obs, A, M), 1.0 / (A * M)))
    env.reset(seed=0)
    out = env.rollout_controller(K, store=store)  # (allocates the buffers every timed launch reuses)
    out = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in out.items()}
    closed_run = lambda: env.rollout_controller(K, out=out, store=store)  # noqa: E731
    timed(open_env, open_run)  # the discarded pair
    timed(env, closed_run)
    us_open, us_closed = [], []
    for _ in range(PAIRS):
        us_open.append(timed(open_env, open_run))
        us_closed.append(timed(env, closed_run))
    o, c = float(np.mean(us_open)), float(np.mean(us_closed))
    closed_bytes, open_bytes = sum(NBYTES[s] for s in store), 4 + 4 + 4 + 2  # open: actions in; obs, reward, 2 flags out
    return {"what": what, "mode": "philox", "env": f"crooms_4_{action_type}_{obs_type}", "num_envs": B, "K": K,
            "launches_per_measurement": REPS, "nodes": M, "stored": list(store),
            "table_bytes": M * n_obs * A * M * 4, "table_in_lds": env.query("controller_lds"),
            "closed_loop_us_per_step": us_closed, "open_loop_us_per_step": us_open,
            "closed_loop_us_per_step_mean": c, "open_loop_us_per_step_mean": o, "ratio_to_open_loop": c / o,
            "closed_loop_bytes_per_env_step": closed_bytes, "open_loop_bytes_per_env_step": open_bytes,
            "closed_loop_frac_hbm": closed_bytes * B / (c * 1e-6) / HBM,
            "open_loop_frac_hbm": open_bytes * B / (o * 1e-6) / HBM,
            "episodes": env.metrics()["episodes"], "persist_blocks_open_loop": env.query("persist_blocks"),
            "persist_occupancy_open_loop": env.query("persist_occupancy")}


def main():
    rows = []
    open_env = make_env("cardinal", "hansen")
    open_run = open_loop_launcher(open_env)
    for M in (1, 4):
        rows.append(closed_loop_row(f"closed_loop_all_outputs_m{M}", "cardinal", "hansen", M, FULL, open_env, open_run))
        rows.append(closed_loop_row(f"closed_loop_no_outputs_m{M}", "cardinal", "hansen", M, (), open_env, open_run))
    del open_run, open_env
    open_env = make_env("ordinal", "hansen8")
    open_run = open_loop_launcher(open_env)
    rows.append(closed_loop_row("closed_loop_all_outputs_m1_global_table", "ordinal", "hansen8", 1, FULL, open_env,
                                open_run))
    for r in rows:
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
