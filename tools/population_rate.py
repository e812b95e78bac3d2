"""Kernel time of a controller population's closed-loop rollout (csrc/grid.hip grid_rollout_population) beside the
single-controller rollout it extends (grid_rollout_controller), in one session on one build: FourRooms Hansen-4,
rng_mode philox, 2^20 envs, K = 128 steps per launch.

  P in {1, 16, 1024} controllers (groups of 2^20, 65,536 and 1,024 envs), M in {1, 4} nodes, storing all six outputs
  and storing nothing. Controller p has its own random table; the single-controller launch of the pair runs table 0.

Each row is one alternated pair sequence single, population, single, population after one discarded pair: every entry
two warm-up launches, then `REPS` launches timed by the handle's hipEvent pairs around the kernel (the recipe of
tools/controller_rate.py). `ratio` is the population's mean us/step over the single controller's mean of the same row; `pair_ratios` are the two
within-pair ratios, the ones to read (box-to-box spread is about +-5%).

Usage (GPU box): python tools/population_rate.py [out.json] -> one JSON line per row (also written to out.json).
"""
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-po-taxi_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import MultistoryFourRoomsEnv, population_thresholds  # noqa: E402

B, K, REPS, PAIRS = 1 << 20, 128, 5, 2
FULL = ("obs", "actions", "nodes", "rew", "term", "trunc")


def make_env():
    env = MultistoryFourRoomsEnv(B, grid_z=1, obs_type="hansen", rng_mode="philox")
    env.reset(seed=0)
    return env


def random_tables(P, M, n_obs, A):
    rng = np.random.default_rng(7)
    p = rng.random((P, M, n_obs, A, M)) + 0.05
    return population_thresholds(p / p.sum((-1, -2), keepdims=True))


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


def prepared(env, store):
    env.reset(seed=0)
    out = env.rollout_controller(K, store=store)  # (allocates the buffers every timed launch reuses)
    out = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in out.items()}
    return lambda: env.rollout_controller(K, out=out, store=store)


def row(P, M, store):
    single, pop = make_env(), make_env()
    n_obs, A = int(single.single_observation_space.n), int(single.single_action_space.n)
    thr = random_tables(P, M, n_obs, A)
    single.set_controller(thresholds=thr[0])
    pop.set_controller_population(thresholds=thr, group_envs=B // P, gamma=0.95)
    run_s, run_p = prepared(single, store), prepared(pop, store)
    us_s, us_p = [], []
    timed(single, run_s), timed(pop, run_p)  # one untimed pair first: the first entry of a row reads slow
    for _ in range(PAIRS):
        us_s.append(timed(single, run_s))
        us_p.append(timed(pop, run_p))
    scores = pop.controller_scores()
    assert int(scores["env_steps"].sum()) == int(pop.metrics()["env_steps"])
    return {"what": f"population_p{P}_m{M}_{'all' if store else 'no'}_outputs", "mode": "philox",
            "env": "fourrooms_hansen4", "num_envs": B, "K": K, "launches_per_entry": REPS, "controllers": P,
            "group_envs": B // P, "nodes": M, "stored": list(store), "table_bytes_per_controller": int(thr[0].nbytes),
            "table_bytes_total": int(thr.nbytes), "table_in_lds": pop.query("controller_lds"),
            "single_table_in_lds": single.query("controller_lds"), "us_per_step_single": us_s,
            "us_per_step_population": us_p, "pair_ratios": [p / s for p, s in zip(us_p, us_s)],
            "ratio": float(np.mean(us_p) / np.mean(us_s))}


def main():
    rows = []
    for store in (FULL, ()):
        for M in (1, 4):
            for P in (1, 16, 1024):
                rows.append(row(P, M, store))
                print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
