"""Kernel time of the grid Heaven-Hell rollouts (csrc/heavenhell.hip hh_rollout) in one session on one build: the
default 10 x 16 maze, action_failure_probability 1/3, rng_mode philox, 2^21 envs, K = 128 steps per launch, uniform
random actions.

  (a) open loop: rollout_plan on random actions (measured before and after the other rows), obs cell_signal;
  (b) the yardstick of the same 14 B per env-step and the same geometry, which does strictly more per step: the
      Ant-Tag index-obs philox open loop (anttag_rollout_idx), measured right after the first (a) row and right before
      the last one;
  (c) closed loop storing all six outputs, M = 1 and M = 4 nodes, a uniform controller, for both obs types;
  (d) closed loop storing nothing (pure policy evaluation), M = 1 and M = 4, for both obs types.

Each row: two warm-up launches, then `reps` launches timed by the handle's hipEvent pairs around the kernel.
`frac_hbm`: algorithmic bytes per env-step over the kernel time, as a fraction of 8 TB/s. `ratio_to_open_loop` of the
(c) and (d) rows is their us/step over the mean of the two (a) rows; `ratio_to_yardstick` of the (a) rows is their
us/step over the mean of the two (b) rows (expected at most 1.05, the spread of one build between boxes).

Usage (GPU box): python tools/heavenhell_rate.py [out.json] -> one JSON line per row (also written to out.json).
"""
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-po-taxi_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import AntTagGridEnv, HeavenHellGridEnv  # noqa: E402

HBM = 8e12
B, K, REPS = 1 << 21, 128, 5
FULL = ("obs", "actions", "nodes", "rew", "term", "trunc")


def make_heavenhell(obs_type="cell_signal"):
    env = HeavenHellGridEnv(B, obs_type=obs_type, action_failure_probability=1 / 3)
    env.reset(seed=0)
    return env


def make_anttag():
    env = AntTagGridEnv(B, obs_type="index", rng_mode="philox")
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
    return ms * 1e3 / (n * K), n


def row(what, name, env, us, n, bytes_per_env_step, **extra):
    r = {"what": what, "mode": "philox", "env": name, "num_envs": B, "K": K, "launches": n,
         "us_per_step_kernel": us, "bytes_per_env_step": bytes_per_env_step,
         "frac_hbm": bytes_per_env_step * B / (us * 1e-6) / HBM, "episodes": env.metrics()["episodes"],
         "persist_blocks": env.query("persist_blocks"), "persist_occupancy": env.query("persist_occupancy")}
    r.update(extra)
    return r


def open_loop(what, name, env):
    g = torch.Generator(device=env.device).manual_seed(1)
    acts = torch.randint(0, int(env.single_action_space.n), (K, B), device=env.device, generator=g, dtype=torch.int32)
    run, _ = env.rollout_plan(acts)
    us, n = timed(env, run)
    return row(what, name, env, us, n, 4 + 4 + 4 + 2)  # actions in; obs, reward, 2 flags out


def closed_loop(what, obs_type, M, store):
    env = make_heavenhell(obs_type)
    n_obs, A = int(env.single_observation_space.n), int(env.single_action_space.n)
    env.set_controller(probs=np.full((M, n_obs, A, M), 1.0 / (A * M)))
    env.reset(seed=0)
    out = env.rollout_controller(K, store=store)  # (allocates the buffers every timed launch reuses)
    out = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in out.items()}
    us, n = timed(env, lambda: env.rollout_controller(K, out=out, store=store))
    nbytes = {"obs": 4, "actions": 4, "nodes": 1, "rew": 4, "term": 1, "trunc": 1}
    return row(what, "heavenhell_" + obs_type, env, us, n, sum(nbytes[s] for s in store), nodes=M,
               table_bytes=M * n_obs * A * M * 4, table_in_lds=env.query("controller_lds"), stored=list(store))


def main():
    rows = [open_loop("a_open_loop_before", "heavenhell_cell_signal", make_heavenhell()),
            open_loop("b_anttag_index_open_loop_before", "anttag_index_10x10", make_anttag())]
    for obs_type in ("cell_signal", "hansen_signal"):
        for M in (1, 4):
            rows.append(closed_loop(f"c_closed_loop_all_outputs_m{M}", obs_type, M, FULL))
            rows.append(closed_loop(f"d_closed_loop_no_outputs_m{M}", obs_type, M, ()))
    rows.append(open_loop("b_anttag_index_open_loop_after", "anttag_index_10x10", make_anttag()))
    rows.append(open_loop("a_open_loop_after", "heavenhell_cell_signal", make_heavenhell()))
    mean = lambda p: float(np.mean([r["us_per_step_kernel"] for r in rows if r["what"].startswith(p)]))  # noqa: E731
    a, b = mean("a_"), mean("b_")
    for r in rows:
        if r["what"].startswith("a_"):
            r["ratio_to_yardstick"] = r["us_per_step_kernel"] / b
        elif not r["what"].startswith("b_"):
            r["ratio_to_open_loop"] = r["us_per_step_kernel"] / a
    rows.append({"what": "summary", "open_loop_us_per_step": a, "yardstick_us_per_step": b,
                 "open_loop_over_yardstick": a / b, "expected_at_most": 1.05})
    for r in rows:
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
