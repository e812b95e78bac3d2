"""Kernel time of the tabular POMDP rollouts (csrc/pomdp.hip pd_rollout) in one session on one build: rng_mode philox,
2^21 envs, K = 128 steps per launch, uniform random actions (open loop) and a uniform controller storing all six
outputs (closed loop, M = 1 and M = 4 nodes).

  (a) Tiger from its text (S = 2, A = 3, O = 2): the model blob, 304 B, in LDS;
  (b) the default grid Heaven-Hell maze at action_failure_probability 1/3 lowered to tables by heaven_hell_pomdp
      (S = 320, A = 4, O = 480; T alone is 1.6 MB): the blob in global memory, read through the caches;
  (n) the yardstick of what generality costs: the native HeavenHellGridEnv on the same maze and probability
      (csrc/heavenhell.hip), open and closed loop.
(b) and (n) alternate, five rounds; every figure is the median over the rounds of the kernel time per step, each round
being two warm-up launches and then `REPS` launches timed by the handle's hipEvent pairs around the kernel. (a) is
measured before and after them.

`frac_hbm`: algorithmic bytes per env-step (the planes read and written; the tables are not counted) over the kernel
time, as a fraction of 8 TB/s. `ratio_to_native`: a (b) row's median over the matching (n) row's.

Usage (GPU box): python tools/pomdp_rate.py [out.json] -> one JSON line per row (also written to out.json; default
profiles/pomdp_rate.json).
"""
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-po-taxi_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv, heaven_hell_pomdp  # noqa: E402

HBM = 8e12
B, K, REPS, ROUNDS = 1 << 21, 128, 5, 5
FULL = ("obs", "actions", "nodes", "rew", "term", "trunc")
OPEN_BYTES = 4 + 4 + 4 + 2  # actions in; obs, reward, 2 flags out
FULL_BYTES = 4 + 4 + 1 + 4 + 1 + 1

TIGER = """discount: 0.95
values: reward
states: tiger-left tiger-right
actions: listen open-left open-right
observations: hear-left hear-right
start: uniform
T: listen
identity
T: open-left
uniform
T: open-right
uniform
O: listen
0.85 0.15
0.15 0.85
O: open-left
uniform
O: open-right
uniform
R: listen : * : * : * -1
R: open-left : tiger-left : * : * -100
R: open-left : tiger-right : * : * 10
R: open-right : tiger-left : * : * 10
R: open-right : tiger-right : * : * -100
"""


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


class Case:
    """One env and one way of running it; `measure()` appends a round's us/step."""

    def __init__(self, what, name, env, M):
        self.what, self.name, self.env, self.M, self.us = what, name, env, M, []
        A = int(env.single_action_space.n)
        if M == 0:
            g = torch.Generator(device=env.device).manual_seed(1)
            acts = torch.randint(0, A, (K, B), device=env.device, generator=g, dtype=torch.int32)
            env.reset(seed=0)
            self.launch, _ = env.rollout_plan(acts)
            self.bytes = OPEN_BYTES
        else:
            n_obs = int(env.single_observation_space.n)
            env.set_controller(probs=np.full((M, n_obs, A, M), 1.0 / (A * M)))
            env.reset(seed=0)
            out = env.rollout_controller(K, store=FULL)  # (allocates the buffers every timed launch reuses)
            out = {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in out.items()}
            self.launch = lambda: env.rollout_controller(K, out=out, store=FULL)
            self.bytes = FULL_BYTES

    def measure(self):
        self.us.append(timed(self.env, self.launch))

    def row(self):
        us = float(np.median(self.us))
        env = self.env
        r = {"what": self.what, "mode": "philox", "env": self.name, "loop": "open" if self.M == 0 else "closed",
             "nodes": self.M, "num_envs": B, "K": K, "rounds": len(self.us), "launches_per_round": REPS,
             "us_per_step_kernel": us, "us_per_step_rounds": self.us, "bytes_per_env_step": self.bytes,
             "frac_hbm": self.bytes * B / (us * 1e-6) / HBM, "persist_blocks": env.query("persist_blocks"),
             "persist_occupancy": env.query("persist_occupancy")}
        if isinstance(env, TabularPOMDPEnv):
            r.update(model_bytes=env.query("pomdp_model_bytes"), model_in_lds=env.query("pomdp_lds"))
        if self.M:
            r.update(table_in_lds=env.query("controller_lds"))
        return r


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pomdp_rate.json")
    loops = (0, 1, 4)  # open loop, closed loop M = 1, M = 4
    tiger = [Case("a_tiger", "tiger", TabularPOMDPEnv.from_pomdp(TIGER, B), M) for M in loops]
    for c in tiger:
        c.measure()
    native0 = HeavenHellGridEnv(8, action_failure_probability=1 / 3)
    model = heaven_hell_pomdp(native0)
    T, Z, R, start, terminal, reset_obs = model
    lowered = [Case("b_heavenhell_as_tables", "heavenhell_cell_signal_as_tables",
                    TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs), M) for M in loops]
    native = [Case("n_heavenhell_native", "heavenhell_cell_signal",
                   HeavenHellGridEnv(B, action_failure_probability=1 / 3), M) for M in loops]
    for _ in range(ROUNDS):
        for lo, na in zip(lowered, native):  # alternating, loop kind by loop kind
            lo.measure()
            na.measure()
    for c in tiger:
        c.measure()
    rows = [c.row() for c in tiger + lowered + native]
    for lo, na in zip(rows[3:6], rows[6:9]):
        lo["ratio_to_native"] = lo["us_per_step_kernel"] / na["us_per_step_kernel"]
    for r in rows:
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
