"""Kernel time of the belief filter and the closed-loop belief rollout of the tabular POMDP (csrc/pomdp.hip
pd_belief_filter, pd_rollout_belief) in one session on one build: rng_mode philox, 2^21 envs, K = 128
steps per launch.

Models:
  tiger       Tiger from its text (S = 2): the beliefs stay on chip (LDS) across a launch;
  heavenhell  the default grid Heaven-Hell maze at action_failure_probability 1/3 lowered to tables by
              heaven_hell_pomdp (S = 320, A = 4, O = 480): the beliefs in the global planes; Tf has at most four
              nonzero entries per column and Zf is 0 / 1, which is where column skipping pays.
Rows, per model:
  (a) rollout_controller with a uniform M = 1 controller storing all six outputs: what a closed loop without a belief
      costs;
  (b) rollout_belief under QMDP vectors (N = A) storing all seven outputs;
  (c) belief_filter alone over the planes (b) stored;
  (d) a plain torch float32 filter (a gather of Zf, one mat-vec batch per action) over the first KT of the same
      planes, timed with torch events, per step; compared with the device's beliefs by allclose, not bitwise.
The rows of a model alternate, ROUNDS rounds; every figure is the median over the rounds of the time per step, each
round being two warm-up launches and then REPS timed ones ((a)-(c): the handle's hipEvent pairs around the kernel). A
model whose K-step launch takes more than two seconds gets two rounds of two launches instead; its rows say so.
Ratios: b / a, c / a, d / c.

Usage (GPU box): python tools/belief_rate.py [out.json] -> one JSON line per row (also written to out.json; default
profiles/belief_rate.json).
"""
import json
import os
import time
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-po-taxi_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv, float_laws, heaven_hell_pomdp, parse_pomdp, qmdp_vectors  # noqa: E402
from pomdp_rate import TIGER  # noqa: E402

B, K, KT, REPS, ROUNDS = 1 << 21, 128, 16, 5, 5
CTRL = ("obs", "actions", "nodes", "rew", "term", "trunc")
BEL = ("obs", "actions", "vec", "value", "rew", "term", "trunc")


def kernel_us(env, launch, steps, reps=None):
    reps = reps or REPS
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    env.set_profiling(True)
    env.profile_read()
    for _ in range(reps):
        launch()
    ms, n = env.profile_read()
    env.set_profiling(False)
    return ms * 1e3 / (n * steps)


def event_us(launch, steps, reps=None):
    reps = reps or REPS
    for _ in range(2):
        launch()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        launch()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (reps * steps)


class TorchFilter:
    """The filter in plain torch float32 on the device: per step a gather of Zf[a, :, o], one [n_a, S] x [S, S]
    product per action, the terminal mask, the reset rule on ended rows, a row normalisation."""

    def __init__(self, env):
        dev = env.device
        lw = float_laws(env)
        self.Tf = torch.from_numpy(lw["Tf"]).to(dev).permute(1, 0, 2).contiguous()  # [A, S, S']
        self.Zf = torch.from_numpy(lw["Zf"]).to(dev)                                # [A, S', O]
        self.Rf = torch.from_numpy(lw["Rf"]).to(dev)                                # [S, O]
        self.prior = torch.from_numpy(lw["prior"]).to(dev)
        self.live = torch.from_numpy(1.0 - env.terminal.astype(np.float32)).to(dev)
        self.A = env.n_actions

    def run(self, b, acts, obs, term, trunc):
        for k in range(acts.shape[0]):
            a, o = acts[k].long(), obs[k].long()
            acc = torch.empty_like(b)
            for x in range(self.A):
                idx = (a == x).nonzero(as_tuple=True)[0]
                acc[idx] = b[idx] @ self.Tf[x]
            u = self.Zf[a, :, o] * acc * self.live
            ended = (term[k] | trunc[k]).bool()
            u = torch.where(ended[:, None], self.prior[None, :] * self.Rf[:, o].T, u)
            b = u / u.sum(-1, keepdim=True)
        return b


class Model:
    """Three handles of one model, so that no row disturbs another: (a) a controller, no belief; (b) the filter and the
    policy, whose state and beliefs advance together; (c) the filter alone, put back to the beliefs (b) started from
    before every launch (set_belief is not inside the timed kernel) and run over the planes (b) stored first."""

    def __init__(self, name, make_env, alpha):
        self.name = name
        u8 = lambda d: {k: (v.view(torch.uint8) if v.dtype == torch.bool else v) for k, v in d.items()}  # noqa: E731
        self.env_a = make_env()
        A, n_obs = self.env_a.n_actions, self.env_a.n_obs
        self.env_a.set_controller(probs=np.full((n_obs, A), 1.0 / A))
        self.env_a.reset(seed=0)
        self.ctrl_out = u8(self.env_a.rollout_controller(K, store=CTRL))
        self.env = env = make_env()
        env.reset(seed=0)
        env.enable_belief()
        env.set_belief_policy(alpha)
        self.b0 = env.belief
        torch.cuda.synchronize()
        t = time.perf_counter()
        self.bel_out = u8(env.rollout_belief(K, store=BEL))
        torch.cuda.synchronize()
        # a model whose launch takes seconds is measured with fewer launches (said in its rows)
        self.rounds, self.reps = (ROUNDS, REPS) if time.perf_counter() - t < 2.0 else (2, 2)
        self.planes = tuple(self.bel_out[n].clone() for n in ("actions", "obs", "term", "trunc"))
        self.bel_scratch = {k: torch.empty_like(v) for k, v in self.bel_out.items()}
        self.env_c = make_env()
        self.env_c.reset(seed=0)
        self.env_c.enable_belief()
        # the torch filter against the device's, from the same beliefs over the same KT planes
        self.tf = TorchFilter(env)
        self.env_c.set_belief(self.b0)
        self.env_c.belief_filter(*(x[:KT] for x in self.planes))
        dev_b = self.env_c.belief
        tor_b = self.tf.run(self.b0, *(x[:KT] for x in self.planes))
        self.max_diff = float((dev_b - tor_b).abs().max())
        self.allclose = bool(torch.allclose(dev_b, tor_b, rtol=1e-4, atol=1e-6))
        self.us = {"a": [], "b": [], "c": [], "d": []}

    def filter_launch(self):
        self.env_c.set_belief(self.b0)
        self.env_c.belief_filter(*self.planes)

    def measure(self):
        a, b, c = self.env_a, self.env, self.env_c
        self.us["a"].append(kernel_us(a, lambda: a.rollout_controller(K, out=self.ctrl_out, store=CTRL), K, self.reps))
        self.us["b"].append(kernel_us(b, lambda: b.rollout_belief(K, out=self.bel_scratch, store=BEL), K, self.reps))
        self.us["c"].append(kernel_us(c, self.filter_launch, K, self.reps))
        self.us["d"].append(event_us(lambda: self.tf.run(self.b0, *(x[:KT] for x in self.planes)), KT, self.reps))
        print(json.dumps({"progress": self.name, **{k: v[-1] for k, v in self.us.items()}}), flush=True)

    def check(self):
        for e in (self.env_a, self.env, self.env_c):  # (no degenerate filter step, no clamped value)
            e.check()

    def rows(self):
        env = self.env
        med = {k: float(np.median(v)) for k, v in self.us.items()}
        what = {"a": "rollout_controller M=1", "b": "rollout_belief qmdp", "c": "belief_filter", "d": "torch filter"}
        base = {"env": self.name, "mode": "philox", "num_envs": B, "K": K, "S": env.n_states, "A": env.n_actions,
                "O": env.n_obs, "belief_onchip": env.query("belief_onchip"), "model_in_lds": env.query("pomdp_lds"),
                "rounds": len(self.us["a"]), "launches_per_round": self.reps}
        rows = [dict(base, what=f"{k}_{what[k]}", us_per_step=med[k], us_per_step_rounds=self.us[k],
                     steps_per_launch=KT if k == "d" else K, timer="torch events" if k == "d" else "hipEvent kernel")
                for k in "abcd"]
        rows[1]["ratio_b_over_a"] = med["b"] / med["a"]
        rows[2]["ratio_c_over_a"] = med["c"] / med["a"]
        rows[3].update(ratio_d_over_c=med["d"] / med["c"], allclose_to_device=self.allclose,
                       max_abs_diff_to_device=self.max_diff)
        return rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "belief_rate.json")
    m = parse_pomdp(TIGER)
    tiger = Model("tiger", lambda: TabularPOMDPEnv.from_pomdp(TIGER, B), qmdp_vectors(m["T"], m["R"], None, 0.95, 1000))
    print(json.dumps({"progress": "tiger built", "allclose": tiger.allclose, "max_diff": tiger.max_diff}), flush=True)
    T, Z, R, start, terminal, reset_obs = heaven_hell_pomdp(HeavenHellGridEnv(8, action_failure_probability=1 / 3))
    hh = Model("heavenhell_cell_signal_as_tables",
               lambda: TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs),
               qmdp_vectors(T, R, terminal, 0.95, 300))
    print(json.dumps({"progress": "heavenhell built", "allclose": hh.allclose, "max_diff": hh.max_diff}), flush=True)
    for r in range(ROUNDS):
        for mdl in (tiger, hh):
            if r < mdl.rounds:
                mdl.measure()
    tiger.check()
    hh.check()
    rows = tiger.rows() + hh.rows()
    for r in rows:
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
