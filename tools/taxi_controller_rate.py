"""Kernel time of the Taxi rollouts, open loop (csrc/taxi.hip taxi_rollout) against closed loop (taxi_rollout_ctrl), in
one session on one build: the 5 x 5 Hansen Taxi, rng_mode philox, 2^22 envs; K = 128 steps per launch with the scalar obs,
K = 4 with the one-hot obs (bench.py's chunk: a [128, 2^22, 320] uint8 obs buffer would take 172 GB).

  (a) scalar obs, open loop: rollout_plan on uniform random actions (measured before and after the other rows);
  (b) one-hot obs, open loop: the same (bench.py's Taxi config);
  (c) scalar obs, closed loop storing all six outputs, a uniform controller of M = 1 and M = 4 nodes;
  (d) one-hot obs, the same;
  (e) scalar obs, closed loop storing nothing (pure policy evaluation), M = 1 and M = 4;
  (f) M = 1, all six outputs, scalar obs: the table staged in LDS (the default) against ctrl_lds_max = 0 (global
      memory), two alternated pairs.

Each row: two warm-up launches, then `reps` launches timed by the handle's hipEvent pairs around the kernel.
`frac_hbm`: algorithmic bytes per env-step over the kernel time, as a fraction of 8 TB/s. `ratio_to_open_loop` of a
closed-loop row is its us/step over the open-loop row of the same obs layout (for the scalar rows the mean of the two
(a) rows).

Usage (GPU box): python tools/taxi_controller_rate.py [out.json] -> one JSON line per row (also written to out.json).
"""
import contextlib
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-po-taxi_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import HansenTaxiVecEnv  # noqa: E402
from gym_po_amd._lib import debug_knobs  # noqa: E402

HBM = 8e12
B, REPS, A = 1 << 22, 5, 5
STEPS = {False: 128, True: 4}  # steps per launch by one_hot
FULL = ("obs", "actions", "nodes", "rew", "term", "trunc")


def make_env(one_hot):
    env = HansenTaxiVecEnv(B, one_hot=one_hot)
    env.reset(seed=0)
    return env


def timed(env, launch, K):
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


def row(what, one_hot, env, us, n, bytes_per_env_step, **extra):
    K = STEPS[one_hot]
    r = {"what": what, "mode": "philox", "env": "hansen_taxi_5x5_" + ("one_hot" if one_hot else "scalar"),
         "num_envs": B, "K": K, "launches": n, "us_per_step_kernel": us, "bytes_per_env_step": bytes_per_env_step,
         "frac_hbm": bytes_per_env_step * B / (us * 1e-6) / HBM, "episodes": env.metrics()["episodes"],
         "persist_blocks": env.query("persist_blocks")}
    r.update(extra)
    return r


def open_loop(what, one_hot):
    env, K = make_env(one_hot), STEPS[one_hot]
    g = torch.Generator(device=env.device).manual_seed(1)
    acts = torch.randint(0, A, (K, B), device=env.device, generator=g, dtype=torch.int32)
    run, _ = env.rollout_plan(acts)
    us, n = timed(env, run, K)
    return row(what, one_hot, env, us, n, 4 + (env.no if one_hot else 4) + 4 + 2)  # actions in; obs, reward, 2 flags out


def closed_loop(what, one_hot, M, store, lds_max=None):
    env, K = make_env(one_hot), STEPS[one_hot]
    with debug_knobs(ctrl_lds_max=lds_max) if lds_max is not None else contextlib.nullcontext():
        env.set_controller(probs=np.full((M, env.no, A, M), 1.0 / (A * M)))
    env.reset(seed=0)
    out = env.rollout_controller(K, store=store)  # (allocates the buffers every timed launch reuses)
    out = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in out.items()}
    us, n = timed(env, lambda: env.rollout_controller(K, out=out, store=store), K)
    nbytes = {"obs": env.no if one_hot else 4, "actions": 4, "nodes": 1, "rew": 4, "term": 1, "trunc": 1}
    return row(what, one_hot, env, us, n, sum(nbytes[s] for s in store), nodes=M,
               table_bytes=M * env.no * ((A * M + 3) // 4 * 4) * 4, table_in_lds=env.query("controller_lds"),
               controller_blocks=env.query("controller_blocks"), stored=list(store))


def main():
    rows = [open_loop("a_scalar_open_loop_before", False)]
    rows.append(open_loop("b_one_hot_open_loop", True))
    rows.append(closed_loop("c_scalar_closed_loop_all_outputs_m1", False, 1, FULL))
    rows.append(closed_loop("c_scalar_closed_loop_all_outputs_m4", False, 4, FULL))
    rows.append(closed_loop("d_one_hot_closed_loop_all_outputs_m1", True, 1, FULL))
    rows.append(closed_loop("d_one_hot_closed_loop_all_outputs_m4", True, 4, FULL))
    rows.append(closed_loop("e_scalar_closed_loop_no_outputs_m1", False, 1, ()))
    rows.append(closed_loop("e_scalar_closed_loop_no_outputs_m4", False, 4, ()))
    for pair in (1, 2):
        rows.append(closed_loop(f"f_m1_table_in_lds_pair{pair}", False, 1, FULL))
        rows.append(closed_loop(f"f_m1_table_in_global_memory_pair{pair}", False, 1, FULL, lds_max=0))
    rows.append(open_loop("a_scalar_open_loop_after", False))
    scalar = 0.5 * (rows[0]["us_per_step_kernel"] + rows[-1]["us_per_step_kernel"])
    one_hot = rows[1]["us_per_step_kernel"]
    for r in rows[2:-1]:
        r["ratio_to_open_loop"] = r["us_per_step_kernel"] / (one_hot if r["env"].endswith("one_hot") else scalar)
    for r in rows:
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
