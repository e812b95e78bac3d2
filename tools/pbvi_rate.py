"""Time of one point-based backup sweep of the tabular POMDP (csrc/pomdp_backup.hip, gp_belief_backup)
against a dense torch float32 backup of the same mathematics on the same device, in one session on one build.

Models:
  tiger       Tiger from its text (S = 2, A = 3, O = 2): P = 4,096 points, N = 64 vectors;
  heavenhell  the default grid Heaven-Hell maze at action_failure_probability 1/3 lowered to tables by
              heaven_hell_pomdp (S = 320, A = 4, O = 480): P = 1,024 points, N = 64 vectors. Tf has at most four
              nonzero entries per row and Zf is 0 / 1: the device walks compressed tables, torch multiplies dense ones.
Points: the beliefs of P envs after WALK steps of uniform random actions (what collect_beliefs gathers, duplicates
kept). Vectors: seeded normal draws (the cost does not depend on their values).
Rows, per model:
  (a) gp_belief_backup through the C ABI on prepared device buffers: the copy of the vectors, the four launches;
  (b) TabularPOMDPEnv.point_backup: (a) plus the validation of the points and the allocation of the outputs;
  (c) the dense torch backup: per action one [P, S] x [S, O N] product for the scores, an argmax, a one-hot
      [P, O N] x [O N, S] product for w, one [P, S] x [S, S] product for h; compared with (a) by allclose on the
      values (bitwise equality is not expected: torch's sums are blocked and fused).
Every figure is a host clock around REPS calls that end in a device synchronise, per call; the rows of a model
alternate over ROUNDS rounds after two warm-up calls each, and the median over the rounds is reported.

Usage (GPU box): python tools/pbvi_rate.py [out.json] -> one JSON line per row (also written to out.json; default
profiles/pbvi_rate.json).
"""
import ctypes
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

REPS, ROUNDS, WALK, GAMMA = 50, 5, 12, 0.95


class TorchBackup:
    """The backup in plain dense torch float32 (`laws`: gym_po_amd.float_laws of the env; reward [S, A, S]; terminal
    [S])."""

    def __init__(self, laws, reward, terminal, device):
        self.Tf = torch.from_numpy(laws["Tf"]).to(device).permute(1, 0, 2).contiguous()  # [A, S, S']
        live = torch.from_numpy(1.0 - np.asarray(terminal).astype(np.float32)).to(device)
        self.Zl = torch.from_numpy(laws["Zf"]).to(device) * live[None, :, None]          # [A, S', O], terminal rows 0
        rw = torch.from_numpy(np.asarray(reward, dtype=np.float32)).to(device).permute(1, 0, 2)
        self.r = (self.Tf * rw).sum(-1)                                                   # [A, S]
        self.A, self.S, self.O = self.Zl.shape[0], self.Zl.shape[1], self.Zl.shape[2]

    def run(self, b, alpha, gamma):
        P, N = b.shape[0], alpha.shape[0]
        vals, betas = [], []
        for a in range(self.A):
            acc = b @ self.Tf[a]                                                    # [P, S']
            za = (self.Zl[a][:, :, None] * alpha.T[:, None, :]).reshape(self.S, self.O * N)  # [S', (o, j)]
            jst = (acc @ za).view(P, self.O, N).argmax(-1)                          # [P, O]
            hot = torch.nn.functional.one_hot(jst, N).to(torch.float32).view(P, self.O * N)
            w = hot @ za.T                                                          # [P, S']
            beta = self.r[a][None, :] + gamma * (w @ self.Tf[a].T)                  # [P, S]
            betas.append(beta)
            vals.append((b * beta).sum(-1))
        v = torch.stack(vals, -1)
        a_star = v.argmax(-1)
        beta = torch.stack(betas, 1)[torch.arange(P, device=b.device), a_star]
        return beta, a_star.to(torch.int32), v.max(-1).values


def clock_us(call, reps=REPS):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / reps


class Model:
    def __init__(self, name, make_env, P, N):
        from gym_po_amd import _lib, float_laws
        self.name, self.P, self.N = name, P, N
        env = self.env = make_env(P)
        env.reset(seed=0)
        env.enable_belief()
        gen = torch.Generator(device="cpu").manual_seed(1)
        for _ in range(WALK):
            a = torch.randint(0, env.n_actions, (1, P), generator=gen, dtype=torch.int32)
            o, _, tm, tr = env.rollout(a)
            env.belief_filter(a, o, tm, tr)
        self.points = env.belief
        S = env.n_states
        self.alpha = np.ascontiguousarray(np.random.default_rng(2).normal(size=(N, S)).astype(np.float32))
        self.alpha_dev = torch.from_numpy(self.alpha).to(env.device)
        self.out = {"alpha": torch.empty((P, S), dtype=torch.float32, device=env.device),
                    "actions": torch.empty(P, dtype=torch.int32, device=env.device),
                    "value": torch.empty(P, dtype=torch.float32, device=env.device)}
        fn = _lib.lib().gp_belief_backup
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

        def raw():
            _lib.check(fn(env._handle, P, ptr(self.points), N, ctypes.c_void_p(self.alpha.ctypes.data), GAMMA,
                          ptr(self.out["alpha"]), ptr(self.out["actions"]), ptr(self.out["value"]), env._stream()),
                       "gp_belief_backup")
        self.raw = raw
        self.tb = TorchBackup(float_laws(env), env.reward, env.terminal, env.device)
        raw()
        beta, act, val = self.tb.run(self.points, self.alpha_dev, GAMMA)
        torch.cuda.synchronize()
        self.value_allclose = bool(torch.allclose(val, self.out["value"], rtol=1e-4, atol=1e-4))
        self.value_max_diff = float((val - self.out["value"]).abs().max())
        self.actions_equal = float((act == self.out["actions"]).float().mean())
        same = act == self.out["actions"]
        self.alpha_max_diff_same_action = float((beta - self.out["alpha"])[same].abs().max()) if bool(same.any()) else 0.0
        self.distinct_points = int(torch.unique(self.points.view(torch.int32), dim=0).shape[0])
        self.us = {"a": [], "b": [], "c": []}

    def measure(self):
        calls = {"a": self.raw, "b": lambda: self.env.point_backup(self.points, self.alpha, GAMMA),
                 "c": lambda: self.tb.run(self.points, self.alpha_dev, GAMMA)}
        for k, call in calls.items():
            for _ in range(2):
                call()
            self.us[k].append(clock_us(call))
        print(json.dumps({"progress": self.name, **{k: v[-1] for k, v in self.us.items()}}), flush=True)

    def rows(self):
        env = self.env
        med = {k: float(np.median(v)) for k, v in self.us.items()}
        what = {"a": "gp_belief_backup (C ABI, prepared buffers)", "b": "TabularPOMDPEnv.point_backup",
                "c": "torch dense float32 backup"}
        base = {"env": self.name, "S": env.n_states, "A": env.n_actions, "O": env.n_obs, "P": self.P, "N": self.N,
                "gamma": GAMMA, "distinct_points": self.distinct_points, "rounds": len(self.us["a"]),
                "calls_per_round": REPS, "timer": "host clock around calls ending in a device synchronise",
                "backup_scratch_bytes": env.query("backup_scratch_bytes")}
        rows = [dict(base, what=f"{k}_{what[k]}", us_per_sweep=med[k], us_per_sweep_rounds=self.us[k]) for k in "abc"]
        rows[2].update(ratio_c_over_a=med["c"] / med["a"], ratio_c_over_b=med["c"] / med["b"],
                       value_allclose_to_device=self.value_allclose, value_max_abs_diff=self.value_max_diff,
                       actions_equal_share=self.actions_equal,
                       alpha_max_abs_diff_where_actions_agree=self.alpha_max_diff_same_action)
        return rows


def main():
    from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv, heaven_hell_pomdp
    from pomdp_rate import TIGER
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pbvi_rate.json")
    tiger = Model("tiger", lambda B: TabularPOMDPEnv.from_pomdp(TIGER, B, time_limit=25), 4096, 64)
    T, Z, R, start, terminal, reset_obs = heaven_hell_pomdp(HeavenHellGridEnv(8, action_failure_probability=1 / 3))
    hh = Model("heavenhell_cell_signal_as_tables",
               lambda B: TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs), 1024, 64)
    for _ in range(ROUNDS):
        for mdl in (tiger, hh):
            mdl.measure()
    for mdl in (tiger, hh):
        mdl.env.check()
    rows = tiger.rows() + hh.rows()
    for r in rows:
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
