"""Kernel time of the grid Ant-Tag rollouts (csrc/anttag.hip anttag_rollout / anttag_rollout_idx) in one session on
one build: 10 x 10 arena, rng_mode philox, 2^21 envs, K = 128 steps per launch.

  (a) vector obs, open loop: rollout_plan on uniform random actions (measured before and after the other rows);
  (b) index obs, open loop: the same actions;
  (c) index obs, closed loop storing all six outputs, M = 1 and M = 4 nodes, a uniform controller;
  (d) closed loop storing nothing (pure policy evaluation), M = 1 and M = 4.

Each row: two warm-up launches, then `reps` launches timed by the handle's hipEvent pairs around the kernel.
`frac_hbm`: algorithmic bytes per env-step over the kernel time, as a fraction of 8 TB/s. `ratio_to_vector_open_loop`
of the (b) row is its us/step over the mean of the two (a) rows; `ratio_to_index_open_loop` of the (c) and (d) rows is
theirs over (b).

Usage (GPU box): python tools/anttag_controller_rate.py [out.json] -> one JSON line per row (also written to out.json).
"""
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-po-taxi_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import AntTagGridEnv  # noqa: E402

HBM = 8e12
B, K, REPS, SIZE = 1 << 21, 128, 5, 10


def make_env(obs_type):
    env = AntTagGridEnv(B, size=SIZE, obs_type=obs_type)
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


def row(what, obs_type, env, us, n, bytes_per_env_step, **extra):
    r = {"what": what, "mode": "philox", "env": f"anttag_{SIZE}x{SIZE}_{obs_type}", "num_envs": B, "K": K,
         "launches": n, "us_per_step_kernel": us, "bytes_per_env_step": bytes_per_env_step,
         "frac_hbm": bytes_per_env_step * B / (us * 1e-6) / HBM, "episodes": env.metrics()["episodes"],
         "persist_blocks": env.query("persist_blocks")}
    r.update(extra)
    return r


def open_loop(what, obs_type):
    env = make_env(obs_type)
    g = torch.Generator(device=env.device).manual_seed(1)
    acts = torch.randint(0, 5, (K, B), device=env.device, generator=g, dtype=torch.int32)
    run, _ = env.rollout_plan(acts)
    us, n = timed(env, run)
    obs_bytes = 16 if obs_type == "vector" else 4
    return row(what, obs_type, env, us, n, 4 + obs_bytes + 4 + 2)  # actions in; obs, reward, 2 flags out


def closed_loop(what, M, store):
    env = make_env("index")
    n_obs = int(env.single_observation_space.n)
    env.set_controller(probs=np.full((M, n_obs, 5, M), 1.0 / (5 * M)))
    env.reset(seed=0)
    out = env.rollout_controller(K, store=store)  # (allocates the buffers every timed launch reuses)
    out = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in out.items()}
    us, n = timed(env, lambda: env.rollout_controller(K, out=out, store=store))
    nbytes = {"obs": 4, "actions": 4, "nodes": 1, "rew": 4, "term": 1, "trunc": 1}
    return row(what, "index", env, us, n, sum(nbytes[s] for s in store), nodes=M,
               table_bytes=M * n_obs * ((5 * M + 3) // 4 * 4) * 4, table_in_lds=env.query("controller_lds"),
               stored=list(store))


def main():
    full = ("obs", "actions", "nodes", "rew", "term", "trunc")
    rows = [open_loop("a_vector_open_loop_before", "vector")]
    rows.append(open_loop("b_index_open_loop", "index"))
    rows.append(closed_loop("c_closed_loop_all_outputs_m1", 1, full))
    rows.append(closed_loop("c_closed_loop_all_outputs_m4", 4, full))
    rows.append(closed_loop("d_closed_loop_no_outputs_m1", 1, ()))
    rows.append(closed_loop("d_closed_loop_no_outputs_m4", 4, ()))
    rows.append(open_loop("a_vector_open_loop_after", "vector"))
    a = 0.5 * (rows[0]["us_per_step_kernel"] + rows[-1]["us_per_step_kernel"])
    b = rows[1]["us_per_step_kernel"]
    rows[1]["ratio_to_vector_open_loop"] = b / a
    for r in rows[2:-1]:
        r["ratio_to_index_open_loop"] = r["us_per_step_kernel"] / b
    for r in rows:
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
