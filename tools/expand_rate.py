"""Time of one belief-set expansion of the tabular POMDP (csrc/pomdp_expand.hip, gp_belief_expand)
against a dense torch float32 statement of the same mathematics on the same device, in one session on one build.

Models:
  tiger       Tiger from its text (S = 2, A = 3, O = 2): P = Q = 4,096;
  heavenhell  the default grid Heaven-Hell maze at action_failure_probability 1/3 lowered to tables by
              heaven_hell_pomdp (S = 320, A = 4, O = 480): P = Q = 1,024. Zf is 0 / 1, so few of the 1,920 candidates
              of a point are live: the device forms and measures the live ones only, torch all of them.
Points: the beliefs of P envs after WALK steps of uniform random actions (what collect_beliefs gathers, duplicates
kept); the reference set is the points themselves, passed explicitly (ref != NULL), so Q = P.
Rows, per model:
  (a) gp_belief_expand through the C ABI on prepared device buffers: the five launches, nothing else;
  (b) TabularPOMDPEnv.expand_beliefs: (a) plus the validation of points and ref and the allocation of the outputs;
  (c) the dense torch statement: per action the batched filter step of every obs ([P, O, S] successors), then
      torch.cdist(p=1) against the reference set, a min over it and an argmax over the candidates. Compared with (a):
      act / obs must agree wherever the best dist beats the runner-up candidate's by more than 1e-5, and dist by
      allclose (bitwise equality is not expected: torch's sums are blocked and fused).
Every figure is a host clock around REPS calls that end in a device synchronise, per call; the rows of a model
alternate over ROUNDS rounds after two warm-up calls each, and the median over the rounds is reported.

Usage (GPU box): python tools/expand_rate.py [out.json] -> one JSON line per row (also written to out.json; default
profiles/expand_rate.json). python tools/expand_rate.py --kernels N: N calls of row (a) per model and nothing else, for
a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/expand_rate.py --kernels 20): in it the Tiger launches
of a kernel are the first N + 1 and the Heaven-Hell launches the last N + 1.
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

REPS = {"a": 20, "b": 20, "c": 2}
ROUNDS, WALK, MARGIN = 5, 12, 1e-5
CDIST_CELLS = 1 << 22


class TorchExpand:
    """The expansion in plain dense torch float32 (`laws`: gym_po_amd.float_laws of the env; terminal [S])."""

    def __init__(self, laws, terminal, device):
        self.Tf = torch.from_numpy(laws["Tf"]).to(device).permute(1, 0, 2).contiguous()  # [A, S, S']
        live = torch.from_numpy(1.0 - np.asarray(terminal).astype(np.float32)).to(device)
        self.Zl = (torch.from_numpy(laws["Zf"]).to(device) * live[None, :, None]).permute(0, 2, 1).contiguous()  # [A, O, S']
        self.A, self.O, self.S = self.Zl.shape

    def run(self, b, ref):
        """-> dist [P, A O] of every candidate (-1: dead) and mass [P, A O]."""
        P = b.shape[0]
        dist, mass = [], []
        for a in range(self.A):
            u = (b @ self.Tf[a])[:, None, :] * self.Zl[a][None]          # [P, O, S']
            n = u.sum(-1)                                                # [P, O]
            bp = u / n.clamp_min(1e-30)[..., None]
            rows = bp.view(P * self.O, self.S)
            step = max(1, CDIST_CELLS // ref.shape[0])  # (cdist launches a block per cell: keep the grid in 32 bits)
            d = torch.cat([torch.cdist(rows[i:i + step], ref, p=1.0).min(-1).values
                           for i in range(0, rows.shape[0], step)]).view(P, self.O)
            dist.append(torch.where(n > 0, d, torch.full_like(d, -1.0)))
            mass.append(n)
        return torch.cat(dist, -1), torch.cat(mass, -1)

    def pick(self, b, ref):
        dist, mass = self.run(b, ref)
        best = dist.argmax(-1)
        return dist, mass, best


def clock_us(call, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / reps


class Model:
    def __init__(self, name, make_env, P, compare=True):
        from gym_po_amd import _lib, float_laws
        self.name, self.P = name, P
        env = self.env = make_env(P)
        env.reset(seed=0)
        env.enable_belief()
        gen = torch.Generator(device="cpu").manual_seed(1)
        for _ in range(WALK):
            a = torch.randint(0, env.n_actions, (1, P), generator=gen, dtype=torch.int32)
            o, _, tm, tr = env.rollout(a)
            env.belief_filter(a, o, tm, tr)
        self.points = env.belief
        self.ref = self.points.clone()
        S, O = env.n_states, env.n_obs
        dev = env.device
        self.out = {"succ": torch.empty((P, S), dtype=torch.float32, device=dev),
                    "dist": torch.empty(P, dtype=torch.float32, device=dev),
                    "actions": torch.empty(P, dtype=torch.int32, device=dev),
                    "obs": torch.empty(P, dtype=torch.int32, device=dev),
                    "mass": torch.empty(P, dtype=torch.float32, device=dev)}
        fn = _lib.lib().gp_belief_expand
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

        def raw():
            _lib.check(fn(env._handle, P, ptr(self.points), P, ptr(self.ref), ptr(self.out["succ"]),
                          ptr(self.out["dist"]), ptr(self.out["actions"]), ptr(self.out["obs"]), ptr(self.out["mass"]),
                          env._stream()), "gp_belief_expand")
        self.raw = raw
        self.tx = TorchExpand(float_laws(env), env.terminal, dev)
        raw()
        self.us = {"a": [], "b": [], "c": []}
        if not compare:
            return
        dist, mass, best = self.tx.pick(self.points, self.ref)
        torch.cuda.synchronize()
        dev_dist, dev_c = self.out["dist"], (self.out["actions"].long() * O + self.out["obs"].long())
        top2 = dist.topk(2, dim=-1).values
        clear = ((top2[:, 0] - top2[:, 1]) > MARGIN) & (top2[:, 0] >= 0)
        self.clear_share = float(clear.float().mean())
        self.pick_agrees_where_clear = bool((best == dev_c)[clear].all())
        self.pick_equal_share = float((best == dev_c).float().mean())
        top = top2[:, 0].clamp_min(0.0)  # (a point without a live candidate: the device answers dist 0)
        self.dist_allclose = bool(torch.allclose(top, dev_dist, rtol=1e-4, atol=1e-5))
        self.dist_max_diff = float((top - dev_dist).abs().max())
        pa = torch.arange(P, device=dev)
        self.mass_max_diff = float((mass[pa, dev_c.clamp_min(0)] - self.out["mass"]).abs().max())
        self.live_per_point = float((dist >= 0).float().sum(-1).mean())
        self.open_share = float((dev_dist > 0).float().mean())
        self.distinct_points = int(torch.unique(self.points.view(torch.int32), dim=0).shape[0])

    def measure(self):
        calls = {"a": self.raw, "b": lambda: self.env.expand_beliefs(self.points, self.ref),
                 "c": lambda: self.tx.pick(self.points, self.ref)}
        for k, call in calls.items():
            for _ in range(2):
                call()
            self.us[k].append(clock_us(call, REPS[k]))
        print(json.dumps({"progress": self.name, **{k: v[-1] for k, v in self.us.items()}}), flush=True)

    def rows(self):
        env = self.env
        med = {k: float(np.median(v)) for k, v in self.us.items()}
        what = {"a": "gp_belief_expand (C ABI, prepared buffers)", "b": "TabularPOMDPEnv.expand_beliefs",
                "c": "torch dense float32: batched filter, cdist(p=1), argmax"}
        base = {"env": self.name, "S": env.n_states, "A": env.n_actions, "O": env.n_obs, "P": self.P, "Q": self.P,
                "distinct_points": self.distinct_points, "live_candidates_per_point": self.live_per_point,
                "share_of_points_with_dist_above_0": self.open_share, "rounds": len(self.us["a"]),
                "timer": "host clock around calls ending in a device synchronise",
                "expand_scratch_bytes": env.query("expand_scratch_bytes")}
        rows = [dict(base, what=f"{k}_{what[k]}", calls_per_round=REPS[k], us_per_expansion=med[k],
                     us_per_expansion_rounds=self.us[k]) for k in "abc"]
        rows[2].update(ratio_c_over_a=med["c"] / med["a"], ratio_c_over_b=med["c"] / med["b"],
                       margin=MARGIN, share_of_points_with_a_clear_best=self.clear_share,
                       act_obs_agree_where_clear=self.pick_agrees_where_clear, act_obs_equal_share=self.pick_equal_share,
                       dist_allclose_to_device=self.dist_allclose, dist_max_abs_diff=self.dist_max_diff,
                       mass_max_abs_diff=self.mass_max_diff)
        return rows


def main():
    from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv, heaven_hell_pomdp
    from pomdp_rate import TIGER
    kernels = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--kernels" else 0
    out_path = sys.argv[1] if len(sys.argv) > 1 and not kernels else os.path.join(ROOT, "profiles", "expand_rate.json")
    tiger = Model("tiger", lambda B: TabularPOMDPEnv.from_pomdp(TIGER, B, time_limit=25), 4096, compare=not kernels)
    T, Z, R, start, terminal, reset_obs = heaven_hell_pomdp(HeavenHellGridEnv(8, action_failure_probability=1 / 3))
    hh = Model("heavenhell_cell_signal_as_tables",
               lambda B: TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs), 1024,
               compare=not kernels)
    if kernels:  # row (a) alone, `kernels` calls per model: what a kernel trace of this command shows
        for mdl in (tiger, hh):
            for _ in range(kernels):
                mdl.raw()
            torch.cuda.synchronize()
            mdl.env.check()
        return
    for _ in range(ROUNDS):
        for mdl in (tiger, hh):
            mdl.measure()
    for mdl in (tiger, hh):
        mdl.env.check()
    rows = tiger.rows() + hh.rows()
    for r in rows:
        print(json.dumps(r), flush=True)
    ok = all(m.pick_agrees_where_clear and m.dist_allclose for m in (tiger, hh))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    if not ok:
        sys.exit("the torch statement disagrees with the device (see act_obs_agree_where_clear / dist_allclose_to_device)")


if __name__ == "__main__":
    main()
