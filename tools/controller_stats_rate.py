"""Time of the controller statistics (csrc/ctrl_stats.hip ctrl_stats, NativeVecEnv.controller_statistics) against the
launch that wrote its planes and against what a user writes in torch, in one session on one build.

Per workload (a uniform controller, rng_mode philox, K = 128 stored steps, gamma = 0.99):
  (a) the rollout_controller launch that wrote the six planes (the handle's hipEvent pairs around the kernel): the
      statistics read the same 15 B per env-step that launch wrote;
  (b) controller_statistics on those planes into zeroed tables: on the path it takes by default, and with the knob
      stats_lds_max = 0, which forces the global-atomics path (device events around the call: one launch);
  (c) the same statistics in plain torch on the same planes: a backward loop over the K steps (elementwise float32
      return-to-go, the cell index, the fixed-point value) with index_put_(accumulate=True) into int64 tables per
      step (device events around the whole loop). Whether its tables equal (b)'s bit for bit is recorded.
(a), (b) and (c) are alternated: each of REPS rounds runs them one after the other; the medians are reported, with
the ratios b / a, b_global / a and c / b.

Workloads: FourRooms Hansen-4, 2^20 envs, M = 1 and M = 4; Heaven-Hell Hansen obs, M = 3, 2^21 envs.

Usage (GPU box): python tools/controller_stats_rate.py [out.json] -> one JSON line per row (also written to out.json,
default profiles/controller_stats_rate.json).
"""
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-po-taxi_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import HeavenHellGridEnv, MultistoryFourRoomsEnv  # noqa: E402
from gym_po_amd._lib import debug_knobs  # noqa: E402

K, REPS, GAMMA = 128, 5, 0.99
WORKLOADS = [
    ("fourrooms_hansen4_m1", lambda: MultistoryFourRoomsEnv(1 << 20, grid_z=1, obs_type="hansen", rng_mode="philox"), 1),
    ("fourrooms_hansen4_m4", lambda: MultistoryFourRoomsEnv(1 << 20, grid_z=1, obs_type="hansen", rng_mode="philox"), 4),
    ("heavenhell_hansen_m3", lambda: HeavenHellGridEnv(1 << 21, obs_type="hansen_signal",
                                                       action_failure_probability=1 / 3), 3),
]


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_statistics(planes, obs0, next_nodes, gamma, M, n_obs, A):
    """What a user writes today: K dependent elementwise steps backwards and a scatter-add per step."""
    obs, act, nodes, rew = planes["obs"], planes["actions"], planes["nodes"], planes["rew"]
    ended = planes["term"] | planes["trunc"]
    T = M * n_obs * A * (M + 1)
    counts = torch.zeros(T, dtype=torch.int64, device=obs.device)
    ret_q = torch.zeros(T, dtype=torch.int64, device=obs.device)
    g = torch.zeros_like(rew[0])
    nn = next_nodes.long()
    one = torch.ones_like(nn)
    gam = torch.tensor(gamma, dtype=torch.float32, device=obs.device)
    for k in range(obs.shape[0] - 1, -1, -1):
        g = torch.where(ended[k], rew[k], rew[k] + gam * g)
        o = (obs[k - 1] if k else obs0).long()
        n = nodes[k].long()
        last = torch.where(ended[k], torch.full_like(nn, M), nn)
        cell = ((n * n_obs + o) * A + act[k].long()) * (M + 1) + last
        q = torch.round(g.double() * 2.0 ** 20).long()
        counts.index_put_((cell,), one, accumulate=True)
        ret_q.index_put_((cell,), q, accumulate=True)
        nn = n
    return counts, ret_q


def measure(name, make, M):
    env = make()
    B = env.num_envs
    n_obs, A = int(env.single_observation_space.n), int(env.single_action_space.n)
    env.set_controller(probs=np.full((M, n_obs, A, M), 1.0 / (A * M)))
    r = env.reset(seed=0)
    obs0 = (r[0] if isinstance(r, tuple) else r).clone()
    out = env.rollout_controller(K)
    raw = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in out.items()}
    into = {n: torch.zeros((M, n_obs, A, M + 1), dtype=torch.int64, device=env.device) for n in ("counts", "ret_q")}

    def stats():
        into["counts"].zero_()
        into["ret_q"].zero_()
        nn = env.controller_nodes
        return device_ms(lambda: env.controller_statistics(out, obs0, next_nodes=nn, gamma=GAMMA, into=into))[0]

    def rollout():  # obs0 of the planes in `out` after this launch: the last obs row before it
        obs0.copy_(out["obs"][-1])
        env.set_profiling(True)
        env.profile_read()
        env.rollout_controller(K, out=raw)
        ms, _ = env.profile_read()
        env.set_profiling(False)
        return ms

    rollout(), stats()  # warm-up of every shape
    with debug_knobs(stats_lds_max=0):
        stats()
    torch_statistics(out, obs0, env.controller_nodes, GAMMA, M, n_obs, A)
    t = {"a": [], "b": [], "b_global": [], "c": []}
    same = {"paths": True, "torch": True}  # bit equality of the two paths' tables, and of torch's with them
    for _ in range(REPS):
        t["a"].append(rollout())
        t["b"].append(stats())
        path = env.query("stats_lds")
        mine = (into["counts"].clone(), into["ret_q"].clone())
        with debug_knobs(stats_lds_max=0):
            t["b_global"].append(stats())
        same["paths"] &= (env.query("stats_lds") == 0 and torch.equal(mine[0], into["counts"])
                          and torch.equal(mine[1], into["ret_q"]))
        nn = env.controller_nodes
        ms, theirs = device_ms(lambda: torch_statistics(out, obs0, nn, GAMMA, M, n_obs, A))
        t["c"].append(ms)
        same["torch"] &= torch.equal(theirs[0], mine[0].reshape(-1)) and torch.equal(theirs[1], mine[1].reshape(-1))
    env.check()
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"what": name, "num_envs": B, "K": K, "nodes": M, "n_obs": n_obs, "actions": A,
            "table_cells": M * n_obs * A * (M + 1), "default_path": "lds" if path else "global", "rounds": REPS,
            "a_rollout_controller_ms": med["a"], "b_controller_stats_ms": med["b"],
            "b_controller_stats_global_path_ms": med["b_global"], "c_torch_ms": med["c"],
            "b_over_a": med["b"] / med["a"], "b_global_over_a": med["b_global"] / med["a"],
            "c_over_b": med["c"] / med["b"], "global_path_tables_equal": same["paths"], "torch_tables_equal": same["torch"],
            "bytes_read_per_env_step": 15,
            "b_read_rate_TBps": 15 * B * K / (med["b"] * 1e-3) / 1e12, "all_ms": t}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "controller_stats_rate.json")
    rows = []
    for name, make, M in WORKLOADS:
        rows.append(measure(name, make, M))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
