"""Record the Car-Flag golden fixtures from the reference (gym_po.envs.car_flag, loaded by refload.load()).

    python tests/golden/make_golden_carflag.py

Writes tests/golden/carflag_*.npz and tests/golden/carflag_index.json: DATA only (seeds, the action recipe, the
reference's per-step outputs, its final state and final PCG64 state, and the draws its resets took). The draws
are recorded by running a second numpy Generator from the same seed through the same calls and checking that it
reproduces the reference's reset values. A fixture that lacks one of the event classes it is meant to pin is
refused.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import refload  # noqa: E402
from carflag_oracle import bits_equal, dynamics, make_actions, reset_position  # noqa: E402
from fixtures import digest  # noqa: E402

CASES = {
    "carflag_f32_b64": dict(env="CarVecEnv", num_envs=64, steps=400, time_limit=160, seed=11, action_seed=1,
                            recipe="bias", period=50, action_dtype="float32"),
    "carflag_f32_tl40_b63": dict(env="CarVecEnv", num_envs=63, steps=200, time_limit=40, seed=12, action_seed=2,
                                 recipe="bias", period=50, action_dtype="float32"),
    "carflag_f64_b64": dict(env="CarVecEnv", num_envs=64, steps=400, time_limit=160, seed=11, action_seed=1,
                            recipe="bias", period=50, action_dtype="float64"),
    "carflag_disc5_b64": dict(env="DiscreteActionCarVecEnv", num_envs=64, steps=300, time_limit=160, seed=13,
                              action_seed=3, recipe="held", period=40, action_dtype="int64", num_actions=5),
}


def rng_meta(gen):
    st = gen.bit_generator.state
    return {"state": str(st["state"]["state"]), "inc": str(st["state"]["inc"]), "has_uint32": int(st["has_uint32"]),
            "uinteger": int(st["uinteger"])}


def record(name, meta, car_flag):
    B, T = meta["num_envs"], meta["steps"]
    if meta["env"] == "CarVecEnv":
        env = car_flag.CarVecEnv(B, time_limit=meta["time_limit"])
    else:
        env = car_flag.DiscreteActionCarVecEnv(meta["num_actions"], B, time_limit=meta["time_limit"])
    shadow = np.random.default_rng(meta["seed"])  # the same stream, drawn through the same calls
    acts = make_actions(meta)
    k53 = np.zeros((T + 1, B), np.uint64)
    hidx = np.zeros((T + 1, B), np.int8)
    pidx = np.zeros((T + 1, B), np.int8)

    def shadow_draw(row, mask):
        b = int(mask.sum())
        if b == 0:
            return
        k = (shadow.random(b) * float(1 << 53)).astype(np.uint64)
        h, p = shadow.choice(2, b), shadow.choice(2, b)
        assert np.array_equal(reset_position(k), env.s[mask, 0]), "shadow stream: reset position"
        assert np.array_equal(np.where(h > 0, 1, -1), env.heavens[mask]), "shadow stream: heavens"
        assert np.array_equal(np.where(p > 0, 0.5, -0.5), env.priests[mask]), "shadow stream: priests"
        k53[row, mask], hidx[row, mask], pidx[row, mask] = k, h, p

    obs0, _ = env.reset(seed=meta["seed"])
    obs0 = obs0.copy()
    shadow_draw(0, np.ones(B, bool))
    obs = np.zeros((T, B, 3), np.float32)
    rew = np.zeros((T, B), np.float32)
    term = np.zeros((T, B), bool)
    trunc = np.zeros((T, B), bool)
    for t in range(T):
        o, r, d, tr, _ = env.step(acts[t].reshape(B, 1) if meta["env"] == "CarVecEnv" else acts[t])
        obs[t], rew[t], term[t], trunc[t] = o, r, d, tr
        shadow_draw(t + 1, d | tr)
    assert env.np_random.bit_generator.state == shadow.bit_generator.state
    assert obs.dtype == np.float32 and env.s.dtype == np.float32
    # every event class this fixture is meant to pin
    events = {"term_plus": int(((rew > 0) & term).sum()), "term_minus": int(((rew < 0) & term).sum()),
              "trunc_only": int((trunc & ~term).sum()), "dir_plus": int((obs[:, :, 2] > 0).sum()),
              "dir_minus": int((obs[:, :, 2] < 0).sum())}
    if meta["recipe"] == "bias":
        events["clipped_actions"] = int((np.abs(acts) > 1).sum())
    for k, v in events.items():
        if v == 0:
            raise SystemExit(f"{name}: no {k} event in the recording; not written")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), obs0=obs0, obs=obs, rew=rew, term=term, trunc=trunc,
                        final_s=env.s, final_heavens=env.heavens, final_priests=env.priests,
                        final_elapsed=env.elapsed.astype(np.int64), k53=k53, hidx=hidx, pidx=pidx)
    out = dict(meta)
    out.update(file=name + ".npz", events=events, final_rng=rng_meta(env.np_random),
               digest={"obs": str(digest(obs)), "rew": str(digest(rew)), "term": str(digest(term)),
                       "trunc": str(digest(trunc)), "actions": str(digest(acts))})
    return out


def record_render(car_flag):
    """8 frames of env 0 with the state they were drawn from."""
    env = car_flag.CarVecEnv(2, time_limit=160, render_mode="rgb_array")
    env.reset(seed=21)
    rng = np.random.default_rng(5)
    frames, s0, hv, pr = [], [], [], []
    taken = {}  # (direction shown, heaven side) -> frames so far: two of each of the four combinations
    t = 0
    while len(frames) < 8:
        if t % 60 == 0:
            bias = rng.choice([-1.0, 1.0], 2)
        env.step(np.clip(bias + rng.uniform(-1, 1, 2), -1, 1).astype(np.float32))
        t += 1
        key = (bool(env.s[0, 2] != 0), bool(env.heavens[0] > 0))
        if taken.get(key, 0) < 2 and t % 7 == 0:
            taken[key] = taken.get(key, 0) + 1
            frames.append(env.render().copy())
            s0.append(env.s[0].copy())
            hv.append(env.heavens[0])
            pr.append(env.priests[0])
        if t > 20000:
            raise SystemExit(f"carflag_render: only {taken} after {t} steps; not written")
    hv = np.array(hv, np.float32)
    np.savez_compressed(os.path.join(HERE, "carflag_render.npz"), frames=np.stack(frames), s0=np.stack(s0),
                        heavens=hv, priests=np.array(pr, np.float64))
    return dict(file="carflag_render.npz", frames=8, seed=21)


# ---------------------------------------------------------------- one-step tables ----
# Each table is ONE reference step of an env whose rows (state, old direction, heaven, priest, elapsed) were planted
# after a seeded reset. time_limit 7; elapsed in {0, 5, 6}: not truncated, one short of it, truncated.
F32 = np.float32
TABLE_TL = 7
TABLES = {
    "carflag_table_f32": dict(env="CarVecEnv", action_dtype="float32", seed=31),
    "carflag_table_f64": dict(env="CarVecEnv", action_dtype="float64", seed=32),
    "carflag_table_disc2": dict(env="DiscreteActionCarVecEnv", action_dtype="int64", num_actions=2, seed=33),
    "carflag_table_disc4": dict(env="DiscreteActionCarVecEnv", action_dtype="int64", num_actions=4, seed=34),
    "carflag_table_disc5": dict(env="DiscreteActionCarVecEnv", action_dtype="int64", num_actions=5, seed=35),
}
MAX_TABLE_BYTES, MAX_TABLE_ROWS = 384 * 1024, 16384
G_LANDING, G_FORCE, G_PRODUCT, G_SPLIT, G_CANCEL, G_TABLE32, G_EDGE = range(7)
GROUPS = ("landing", "force", "product", "path_split", "cancel", "table_f32", "zone_edge")
LANDING_CONSTS = (0.0, 0.2, 0.3, 0.5, 0.7, 1.0, 1.03, 1.1)
COMBOS = ((-1.0, -0.5), (-1.0, 0.5), (1.0, -0.5), (1.0, 0.5))  # (heaven, priest)
ELAPSED = (0, TABLE_TL - 2, TABLE_TL - 1)


def neighbours(c, dtype=F32):
    """(the value below, c, the value above) in `dtype`."""
    c = dtype(c)
    return [np.nextafter(c, dtype(-np.inf)), c, np.nextafter(c, dtype(np.inf))]


def _uniq(vals, dtype):
    """Distinct by bits (keeps -0.0 next to 0.0, and one NaN), in order."""
    u = {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
    seen, out = set(), []
    for v in vals:
        b = int(np.array(v, dtype).view(u))
        if b not in seen:
            seen.add(b)
            out.append(dtype(v))
    return out


def landing_positions():
    xs = []
    for c in LANDING_CONSTS:
        xs += neighbours(c) + neighbours(-c)
    return _uniq(xs + [F32(-0.0)], F32)


def float_actions(dtype):
    fi = np.finfo(dtype)
    vals = []
    for c in (0.0, 0.5, 1.0, 1.5):
        vals += neighbours(c, dtype) + neighbours(-c, dtype)
    tiny, big = fi.smallest_subnormal, dtype(fi.max / 2)
    vals += [dtype(-0.0), dtype(np.inf), dtype(-np.inf), dtype(np.nan), tiny, -tiny, big, -big]
    return _uniq(vals, dtype)


class Rows:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.r = []

    def add(self, group, x, v, a, combo=None, elapsed=None, old=None):
        """One row; what is not given is drawn (old direction: 0, heaven's sign or its opposite)."""
        h, p = COMBOS[self.rng.integers(4)] if combo is None else combo
        el = ELAPSED[self.rng.integers(3)] if elapsed is None else elapsed
        old = (0.0, h, -h)[self.rng.integers(3)] if old is None else old
        self.r.append((group, F32(x), F32(v), F32(old), h, p, el, a))

    def arrays(self, act_dtype):
        g, x, v, o, h, p, el, a = zip(*self.r)
        return dict(group=np.array(g, np.uint8), s0=np.stack([np.array(x, F32), np.array(v, F32), np.array(o, F32)], 1),
                    heavens0=np.array(h, F32), priests0=np.array(p, np.float64), elapsed0=np.array(el, np.int64),
                    act=np.array(a, act_dtype))


def _one(x, v, a, h=1.0, p=0.5, **kw):
    """dynamics() of a single row."""
    s = np.array([[x, v, 0.0]], F32)
    return [r[0] for r in dynamics(s, np.array([h], F32), np.array([p]), np.array([a]), **kw)]


def split_rows():
    """(x, v, priest) at which the float32 and the float64 arithmetic of a = 0 give different flags: x' one
    float64 step inside |x| = 1 or inside a zone edge, the float32 sum rounded onto or across it. Found by
    trying the float32 neighbours of v; the first two families are x = 1 - 2^-k, v = 2^-k - 2^(-k-24)."""
    seeds = [(1 - 2.0 ** -k, 2.0 ** -k, 0.5) for k in (4, 5, 6)]       # |x'| >= 1
    seeds += [(0.6875, 0.0125, 0.5), (0.65, 0.05, 0.5), (0.25, 0.05, 0.5), (0.28125, 0.01875, 0.5)]  # 0.7 and 0.3 edges
    out = []
    for x, v0, p in seeds:
        v = F32(v0)
        for _ in range(8):
            v = np.nextafter(v, F32(-np.inf))
        for _ in range(17):
            a, b = _one(x, v, F32(0)), _one(x, v, np.float64(0))
            if a[2] != b[2] or (not a[2] and not b[2] and a[4] != b[4]):
                out += [(F32(x), v, p), (F32(-x), -v, -p)]  # and the mirror image
            v = np.nextafter(v, F32(np.inf))
    return out


def fused(v, f, c):
    """v + f * c rounded ONCE (what a fused multiply-add gives): exact in rationals, non-finite inputs as they are."""
    from fractions import Fraction
    plain = v + f * c
    out = plain.copy()
    for i in np.flatnonzero(np.isfinite(plain)):
        exact = Fraction(float(v[i])) + Fraction(float(f[i])) * Fraction(float(c))
        if exact:  # an exact zero keeps the sign the two-step sum gives it (the same rule for both)
            out[i] = plain.dtype.type(float(exact)) if plain.dtype != F32 else F32(_round_f32(exact))
    return out


def _round_f32(q):
    """A rational rounded ONCE to float32 (through float64 it would be rounded twice)."""
    from fractions import Fraction
    d = float(q)
    a = F32(d)
    if Fraction(float(a)) == q:
        return a
    lo, hi = (np.nextafter(a, F32(-np.inf)), a) if Fraction(float(a)) > q else (a, np.nextafter(a, F32(np.inf)))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return a
    mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
    if q != mid:
        return lo if q < mid else hi
    return lo if (int(np.array(lo).view(np.uint32)) & 1) == 0 else hi


def cancel_rows(dtype):
    """(v, a) where v nearly cancels a * 0.0015, so that the rounding of the product survives into the stored
    velocity: rows on which one rounding (an FMA) and two roundings differ."""
    out = []
    for a in [dtype(x) for x in (0.3, 0.7, 0.9, -0.3, -0.7, -0.9, 1 / 3, -1 / 3)] + neighbours(1.0, dtype)[:1]:
        c = F32(0.0015) if dtype == F32 else 0.0015
        v = F32(-(a * c))
        for _ in range(32):
            v = np.nextafter(v, F32(-np.inf))
        found = 0
        for _ in range(65):
            if found < 6 and F32(_one(0.1, v, a)[0]) != F32(_one(0.1, v, a, madd=fused)[0]):  # the STORED velocity
                out.append((v, a))
                found += 1
            v = np.nextafter(v, F32(np.inf))
    if dtype == np.float64:
        # In float64 the product's rounding error (2^-65 here) shows in the stored float32 only where the float32 v
        # cancels the product to far below its own ulp: take the forces, of 2^18 random ones, whose product lies
        # closest to a float32.
        a = np.random.default_rng(64).uniform(-1.0, 1.0, 1 << 18)
        v = (-(a * 0.0015)).astype(F32)
        found = 0
        for i in np.argsort(np.abs(a * 0.0015 + v.astype(np.float64)))[:256]:
            if found < 12 and F32(_one(0.1, v[i], a[i])[0]) != F32(_one(0.1, v[i], a[i], madd=fused)[0]):
                out.append((v[i], np.float64(a[i])))
                found += 1
    return out


def edge_rows():
    """float64 path only: (x, v, a, priest) whose x' IS the double 0.3 or 0.7 (no float32 is, so a = 0 cannot land
    there): v' = d = edge - x exactly, reached as v + a * 0.0015 by trying the doubles around a = (d - v) / 0.0015."""
    out = []
    for edge, x in ((0.3, 0.25), (0.7, 0.65), (0.3, 0.26), (0.7, 0.66)):
        x = float(F32(x))
        d = edge - x
        assert x + d == edge
        found = 0
        for v in np.arange(0.0485, 0.0499, 0.0001).astype(F32):
            a = (d - float(v)) / 0.0015
            for _ in range(8):
                a = np.nextafter(a, -np.inf)
            for _ in range(17):
                if float(v) + a * 0.0015 == d and found < 2:
                    out += [(F32(x), v, np.float64(a), 0.5), (F32(-x), -v, np.float64(-a), -0.5)]
                    found += 1
                a = np.nextafter(a, np.inf)
        assert found, edge
    return out


def table32_rows(n, want=32):
    """(v, index) at which the step with the action table rounded to float32 stores another velocity than the step
    with the float64 table (np.linspace(-1, 1, 4) holds +-1/3): searched over random v."""
    table = np.linspace(-1.0, 1.0, n)
    t32 = table.astype(F32).astype(np.float64)
    rng = np.random.default_rng(n)
    out = []
    for idx in np.flatnonzero(table != t32):
        v = rng.uniform(-0.06, 0.06, 1 << 16).astype(F32)
        s = np.stack([np.full_like(v, 0.1), v, np.zeros_like(v)], 1)
        hv, pr = np.ones(len(v), F32), np.full(len(v), 0.5)
        a = dynamics(s, hv, pr, np.full(len(v), table[idx]))[0].astype(F32)
        b = dynamics(s, hv, pr, np.full(len(v), t32[idx]))[0].astype(F32)
        out += [(x, int(idx)) for x in v[a != b][:want]]
    return out


def table_rows(name, meta):
    n = meta.get("num_actions")
    dtype = {"float32": F32, "float64": np.float64}.get(meta["action_dtype"])
    rows = Rows(meta["seed"])
    acts0 = [dtype(0)] if n is None else list(range(-n, n))
    for x in landing_positions():  # a = 0, v = 0: x' = x (discrete: every index)
        for combo in COMBOS:
            for el in ELAPSED:
                for a in acts0:
                    rows.add(G_LANDING, x, 0.0, a, combo, el)
    vel = []
    for c in (0.0, 0.0015, 0.0685, 0.07):
        vel += neighbours(c) + neighbours(-c)
    vel = _uniq(vel, F32)
    if n is None:
        for x in (0.1, 0.95, -0.95, 0.27, -0.73):
            for v in vel:
                for a in float_actions(dtype):
                    rows.add(G_FORCE, x, v, a)
    else:
        for x in (0.1, 0.95, -0.95, 0.27, -0.73):
            for v in vel:
                for a in range(-n, n):
                    rows.add(G_FORCE, x, v, a)
    pos = (-1.09, -1.0, -0.97, -0.93, -0.7, -0.5, -0.3, -0.2, -0.05, 0.0, 0.05, 0.2, 0.3, 0.5, 0.7, 0.93, 0.97, 1.0,
           1.09)
    vels = (-0.07, -0.05, -0.03, -0.0015, 0.0, 0.0015, 0.03, 0.05, 0.07)
    acts = [dtype(a) for a in (-1.5, -1.0, -0.6, -0.3, 0.0, 0.3, 0.6, 1.0, 1.5)] if n is None else list(range(-n, n))
    for x in pos:
        for v in vels:
            for a in acts:
                for combo in (COMBOS if n is None else COMBOS[:1]):
                    rows.add(G_PRODUCT, x, v, a, None if n else combo)
    if n is None:
        for x, v, p in split_rows():  # the same f32 inputs in both float tables
            for h in (-1.0, 1.0):
                for el in ELAPSED:
                    rows.add(G_SPLIT, x, v, dtype(0), (h, p), el, old=h)
        for v, a in cancel_rows(dtype):
            rows.add(G_CANCEL, 0.1, v, a, elapsed=0)
        if dtype == np.float64:
            for x, v, a, p in edge_rows():
                for h in (-1.0, 1.0):
                    rows.add(G_EDGE, x, v, a, (h, p), 0, old=0.0)
    else:
        for v, idx in table32_rows(n):
            rows.add(G_TABLE32, 0.1, v, idx, elapsed=0)
            rows.add(G_TABLE32, 0.1, v, idx - n, elapsed=0)
    return rows.arrays(np.int64 if n else dtype)


# Five wrong variants of the rules (carflag_oracle.dynamics with one piece swapped): a table must hold rows that
# tell each of them from the reference.
VARIANTS = {
    "gt_for_ge": dict(term_of=lambda x: np.abs(x) > 1.0),
    "strict_zone": dict(zone_of=lambda xd, pr: (xd > pr - 0.2) & (xd < pr + 0.2)),
    "zone_in_f32": dict(zone_of=lambda xd, pr: (xd.astype(F32) >= (pr - 0.2).astype(F32))
                        & (xd.astype(F32) <= (pr + 0.2).astype(F32))),
    "fma": dict(madd=fused),
    "reward_by_old_side": dict(side_of=lambda x0, x: np.sign(x0)),
}
MIN_VARIANT_ROWS = 4


def variant_requirement(meta, variant):
    """Rows of a table that must tell `variant` from the reference: MIN_VARIANT_ROWS, 0 where the variant computes
    the same function (asserted to be exactly 0), None where it is only counted.
      float32 path: x' is a float32 and neither 0.5 -+ 0.2 (the doubles 0.3, 0.7) is one, so x' never sits ON a zone
        edge (strict edges change nothing), and no float32 lies between 0.3 and f32(0.3) or f32(0.7) and 0.7 (the
        compare in float32 changes nothing). Both are mutations of the float64 path only.
      discrete tables: the float64 path with the force from a table. Without a zero force (n even) x' = x + v' is
        never exactly +-1 from float32 x, v, and an exact edge or a one-rounding difference needs a searched double
        action, which an index cannot give: there the float64 table is the one that pins the shared cf_dyn<true>."""
    n = meta.get("num_actions")
    if variant == "reward_by_old_side":
        # every path: a reward needs |x'| >= 1 and |x' - x| <= 0.07, so x and x' lie on the same side; asserted 0
        return 0
    if meta["action_dtype"] == "float32":
        return 0 if variant in ("strict_zone", "zone_in_f32") else MIN_VARIANT_ROWS
    if n is None:
        return MIN_VARIANT_ROWS
    if variant == "gt_for_ge" and n % 2:
        return MIN_VARIANT_ROWS
    return None


def table_actions(meta, d):
    """The float actions of a table's rows (discrete: the float64 table's values)."""
    n = meta.get("num_actions")
    return d["act"] if n is None else np.linspace(-1.0, 1.0, n)[d["act"]]


def rows_differing(meta, d, **variant):
    """Rows on which dynamics(**variant) disagrees with the recorded step in term, reward or, where the row did not
    end, in the stored state."""
    v, x, term, rew, direction = dynamics(d["s0"], d["heavens0"], d["priests0"], table_actions(meta, d), **variant)
    stay = ~(d["term"] | d["trunc"])
    s = np.stack([x.astype(F32), v.astype(F32), direction], 1)
    bad = (term != d["term"]) | ~bits_equal(rew, d["rew"])
    return bad | (stay & ~term & ~bits_equal(s, d["final_s"]).all(1))


def table_coverage(meta, d):
    """Every count a table is accepted on, from its arrays alone."""
    term, trunc, rew = d["term"], d["trunc"], d["rew"]
    stay = ~(term | trunc)
    fs, old = d["final_s"], d["s0"][:, 2]
    v, x = dynamics(d["s0"], d["heavens0"], d["priests0"], table_actions(meta, d))[:2]
    cov = {
        "rows": int(len(term)), "term_plus": int((term & (rew > 0)).sum()), "term_minus": int((term & (rew < 0)).sum()),
        "trunc_only": int((trunc & ~term).sum()), "term_and_trunc": int((term & trunc).sum()),
        "dir_plus": int((stay & (fs[:, 2] > 0)).sum()), "dir_minus": int((stay & (fs[:, 2] < 0)).sum()),
        "dir_cleared": int((stay & (old != 0) & (fs[:, 2] == 0)).sum()),
        "speed_clipped": int((stay & (np.abs(fs[:, 1]) == F32(0.07))).sum()),
        "position_clipped": int((np.abs(x) == (F32(1.1) if x.dtype == F32 else 1.1)).sum()),
        "nan_rows": int(np.isnan(fs[:, 0]).sum()),
        "groups": {g: int((d["group"] == i).sum()) for i, g in enumerate(GROUPS)},
        "variants": {k: int(rows_differing(meta, d, **kw).sum()) for k, kw in VARIANTS.items()},
    }
    if meta.get("num_actions"):
        t32 = np.linspace(-1.0, 1.0, meta["num_actions"]).astype(F32).astype(np.float64)[d["act"]]
        v32, x32 = dynamics(d["s0"], d["heavens0"], d["priests0"], t32)[:2]
        cov["table_f32_rows"] = int((stay & ((v32.astype(F32) != fs[:, 1]) | (x32.astype(F32) != fs[:, 0]))).sum())
    return cov


def landing_pattern(meta, d):
    """For every landing constant c and sign: (terminated, direction shown) at the f32 below c, at c and above it,
    on the rows with elapsed 0, a = 0 and the priest on c's side; {"+0.3": [[t, t, t], [z, z, z]], ...}."""
    n = meta.get("num_actions")
    a0 = (table_actions(meta, d) == 0) & (d["group"] == G_LANDING) & (d["elapsed0"] == 0)
    out = {}
    for c in LANDING_CONSTS[1:]:
        for sg in (1.0, -1.0):
            t, z = [], []
            for xv in neighbours(sg * c):
                m = a0 & (d["s0"][:, 0] == xv) & (d["priests0"] == sg * 0.5)
                if n is not None and not m.any():
                    continue  # a discrete table without a zero action lands nowhere
                assert m.sum() >= 2 and len(set(d["term"][m])) == 1, (c, sg, xv)
                t.append(int(d["term"][m][0]))
                shown = d["final_s"][m, 2] != 0
                assert len(set(shown)) == 1
                z.append(int(shown[0]))
            out[("+" if sg > 0 else "-") + str(c)] = [t, z]
    return out


# what the rules say at the three f32 around each constant (0.5 -+ 0.2 are the doubles 0.3 and 0.7: f32(0.3) lies
# above 0.3 and f32(0.7) below 0.7, so both are inside the zone)
LANDING_WANT = {
    "+0.2": [[0, 0, 0], [0, 0, 0]], "-0.2": [[0, 0, 0], [0, 0, 0]],
    "+0.3": [[0, 0, 0], [0, 1, 1]], "-0.3": [[0, 0, 0], [1, 1, 0]],
    "+0.5": [[0, 0, 0], [1, 1, 1]], "-0.5": [[0, 0, 0], [1, 1, 1]],
    "+0.7": [[0, 0, 0], [1, 1, 0]], "-0.7": [[0, 0, 0], [0, 1, 1]],
    "+1.0": [[0, 1, 1], [0, 0, 0]], "-1.0": [[1, 1, 0], [0, 0, 0]],
    "+1.03": [[1, 1, 1], [0, 0, 0]], "-1.03": [[1, 1, 1], [0, 0, 0]],
    "+1.1": [[1, 1, 1], [0, 0, 0]], "-1.1": [[1, 1, 1], [0, 0, 0]],
}


def check_table(name, meta, d, cov, nbytes):
    """Refuse a table that does not pin what it is meant to (tests/test_carflag_table_cpu.py repeats this)."""
    def need(ok, what):
        if not ok:
            raise SystemExit(f"{name}: {what}; not written")
    need(nbytes <= MAX_TABLE_BYTES and cov["rows"] <= MAX_TABLE_ROWS, f"{nbytes} bytes, {cov['rows']} rows")
    for k in ("term_plus", "term_minus", "trunc_only", "term_and_trunc", "dir_plus", "dir_minus", "dir_cleared",
              "speed_clipped", "position_clipped"):
        need(cov[k] > 0, f"no {k} row")
    n = meta.get("num_actions")
    pat = landing_pattern(meta, d)
    if n is None or n % 2:
        need(pat == LANDING_WANT, f"landing pattern {pat}")
    for k, c in cov["variants"].items():
        want = variant_requirement(meta, k)
        need(want is None or (c == 0 if want == 0 else c >= want),
             f"variant {k} differs on {c} rows, wanted {want or 'none'}")
    if n == 4:
        need(cov["table_f32_rows"] >= 16, f"{cov['table_f32_rows']} rows tell the float32-rounded table apart")


def record_table(name, meta, car_flag):
    d = table_rows(name, meta)
    B = len(d["act"])
    if meta["env"] == "CarVecEnv":
        env = car_flag.CarVecEnv(B, time_limit=TABLE_TL)
    else:
        env = car_flag.DiscreteActionCarVecEnv(meta["num_actions"], B, time_limit=TABLE_TL)
    env.reset(seed=meta["seed"])
    env.s[:] = d["s0"]
    env.elapsed[:] = d["elapsed0"]
    env.heavens[:] = d["heavens0"]
    env.hells[:] = -d["heavens0"]
    env.priests[:] = d["priests0"]
    before = rng_meta(env.np_random)
    shadow = np.random.Generator(np.random.PCG64())
    shadow.bit_generator.state = env.np_random.bit_generator.state
    with np.errstate(all="ignore"):
        o, r, tm, tr, _ = env.step(d["act"].reshape(B, 1) if meta["env"] == "CarVecEnv" else d["act"])
    mask = tm | tr
    b = int(mask.sum())
    k = (shadow.random(b) * float(1 << 53)).astype(np.uint64)
    h, p = shadow.choice(2, b), shadow.choice(2, b)
    assert np.array_equal(reset_position(k), env.s[mask, 0]), "shadow stream: reset position"
    assert np.array_equal(np.where(h > 0, 1, -1), env.heavens[mask]), "shadow stream: heavens"
    assert np.array_equal(np.where(p > 0, 0.5, -0.5), env.priests[mask]), "shadow stream: priests"
    assert env.np_random.bit_generator.state == shadow.bit_generator.state
    assert o.dtype == np.float32 and r.dtype == np.float32 and env.priests.dtype == np.float64
    k53, hidx, pidx = np.zeros(B, np.uint64), np.zeros(B, np.int8), np.zeros(B, np.int8)
    k53[mask], hidx[mask], pidx[mask] = k, h, p
    d.update(obs=o.copy(), rew=r, term=tm, trunc=tr, final_s=env.s.copy(), final_heavens=env.heavens.copy(),
             final_priests=env.priests.copy(), final_elapsed=env.elapsed.astype(np.int64), k53=k53, hidx=hidx,
             pidx=pidx)
    out = dict(meta)
    out.update(file=name + ".npz", rows=B, time_limit=TABLE_TL, rng_before=before, rng_after=rng_meta(env.np_random))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path + ".tmp.npz", **d)
    cov = table_coverage(out, d)
    try:
        check_table(name, out, d, cov, os.path.getsize(path + ".tmp.npz"))
    except SystemExit:
        os.remove(path + ".tmp.npz")
        raise
    os.replace(path + ".tmp.npz", path)
    out["coverage"] = cov
    out["landing"] = landing_pattern(out, d)
    return out


def check_path_split(tables):
    """The two float tables hold the same f32 inputs in their path-split rows and disagree there."""
    a, b = (dict(np.load(os.path.join(HERE, tables[n]["file"]))) for n in ("carflag_table_f32", "carflag_table_f64"))
    ma, mb = a["group"] == G_SPLIT, b["group"] == G_SPLIT
    for k in ("s0", "heavens0", "priests0", "elapsed0"):
        assert np.array_equal(a[k][ma], b[k][mb]), k
    stay = ~(a["term"][ma] | a["trunc"][ma] | b["term"][mb] | b["trunc"][mb])
    n_term = int((a["term"][ma] != b["term"][mb]).sum())
    n_dir = int((stay & (a["final_s"][ma, 2] != b["final_s"][mb, 2])).sum())
    if n_term < 2 or n_dir < 2:
        raise SystemExit(f"path split: {n_term} rows differ in term, {n_dir} in direction")
    return {"term": n_term, "direction": n_dir}


def main():
    refload.load()
    import gym_po.envs.car_flag as car_flag
    cases = {name: record(name, meta, car_flag) for name, meta in CASES.items()}
    tables = {name: record_table(name, meta, car_flag) for name, meta in TABLES.items()}
    index = {"numpy_version": np.__version__, "cases": cases, "carflag_render": record_render(car_flag),
             "tables": tables, "path_split": check_path_split(tables)}
    with open(os.path.join(HERE, "carflag_index.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, c in cases.items():
        print(name, c["events"])
    for name, t in tables.items():
        print(name, t["coverage"])
    print("path_split", index["path_split"])


if __name__ == "__main__":
    main()
