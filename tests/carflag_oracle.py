"""TEST INFRASTRUCTURE — NumPy restatement of the Car-Flag envs (the rules of gym_po/envs/car_flag.py:50-144 and
:286-303, in our own words) with pluggable reset draws. Only tests and the fixture generator import this; the
product (gym-po-taxi_amd/) never does.

Draw sources (what a reset of the envs `idx`, ascending, gets):
  NumpyDraws(gen)   the reference's own stream: gen.random(b) for uniform(-0.2, 0.2, (b, 1)), then two
                    gen.choice(2, b) for the heaven and priest picks (the calls car_flag.py:100-110 make)
  ReplayDraws       per-env k53 / heaven index / priest index arrays set before each step (`.set(k, h, p)`)
  FollowDraws       reset values decided elsewhere (read back from the device): `.set(x, heavens, priests)`
"""
import numpy as np

F32 = np.float32
TWO53 = float(1 << 53)


def reset_position(k53):
    """uniform(-0.2, 0.2) for next_double = k53 * 2**-53: loc + scale * u in float64, then float32."""
    u = np.asarray(k53, dtype=np.uint64).astype(np.float64) * (1.0 / TWO53)
    return (-0.2 + 0.4 * u).astype(F32)


class NumpyDraws:
    def __init__(self, gen):
        self.gen = gen

    def draw(self, idx):
        b = len(idx)
        k = (self.gen.random(b) * TWO53).astype(np.uint64)  # exact: random() is k * 2**-53
        h = self.gen.choice(2, b)
        p = self.gen.choice(2, b)
        return k, h, p

    def values(self, idx):
        k, h, p = self.draw(idx)
        self.last = (k, h, p)
        return reset_position(k), np.where(h > 0, 1.0, -1.0).astype(F32), np.where(p > 0, 0.5, -0.5)


class ReplayDraws:
    def set(self, k, h, p):
        self.k, self.h, self.p = np.asarray(k, np.uint64), np.asarray(h), np.asarray(p)

    def values(self, idx):
        return (reset_position(self.k[idx]), np.where(self.h[idx] != 0, 1.0, -1.0).astype(F32),
                np.where(self.p[idx] != 0, 0.5, -0.5))


class FollowDraws:
    def set(self, x, heavens, priests):
        self.x, self.hv, self.pr = np.asarray(x, F32), np.asarray(heavens, F32), np.asarray(priests, np.float64)

    def values(self, idx):
        return self.x[idx], self.hv[idx], self.pr[idx]


def dynamics(s, heavens, priests, a, madd=lambda v, f, c: v + f * c, term_of=lambda x: np.abs(x) >= 1.0,
             zone_of=lambda xd, pr: (xd >= pr - 0.2) & (xd <= pr + 0.2), side_of=lambda x0, x: np.sign(x)):
    """The arithmetic of one step from the state s [B, 3] (elapsed and the reset excluded): (v', x', terminated,
    reward, direction). float32 actions: float32 arithmetic with the constants rounded to float32; anything else
    (float64, or values of the float64 table): float64 arithmetic from the f32 state, rounded when stored. The four
    keyword pieces are the rules themselves; the table generator swaps one at a time for a wrong one to count the
    rows that would notice (tests/golden/make_golden_carflag.py VARIANTS)."""
    if a.dtype == F32:
        f = np.minimum(np.maximum(a, F32(-1.0)), F32(1.0))
        v = np.minimum(np.maximum(madd(s[:, 1], f, F32(0.0015)), F32(-0.07)), F32(0.07))
        x = np.minimum(np.maximum(s[:, 0] + v, F32(-1.1)), F32(1.1))
        assert v.dtype == F32 and x.dtype == F32
    else:
        f = np.minimum(np.maximum(a.astype(np.float64), -1.0), 1.0)
        v = np.minimum(np.maximum(madd(s[:, 1].astype(np.float64), f, 0.0015), -0.07), 0.07)
        x = np.minimum(np.maximum(s[:, 0].astype(np.float64) + v, -1.1), 1.1)
    term = term_of(x)
    side = side_of(s[:, 0], x).astype(F32)
    rew = np.where(term, np.where(side == heavens, F32(1), F32(-1)), F32(0)).astype(F32)
    direction = np.where(zone_of(x.astype(np.float64), priests), heavens, F32(0)).astype(F32)
    return v, x, term, rew, direction


PHILOX_TAG = 0x63666c31  # 'cfl1'


class PhiloxDraws:
    """rng_mode="philox" predicted from the key alone: the reset of env e at counter c takes the four words of the
    Philox block (e, c, tag 'cfl1'): k53 = (w1 << 32 | w0) >> 11, heaven = w2 >> 31, priest = w3 >> 31. `reset(seed)`
    uses counter 0; every step and every further `reset()` the next one. The caller sets `.counter` before the
    oracle call that may reset (`PhiloxDraws(philox_key(seed))`, oracle.philox)."""

    def __init__(self, key):
        self.key, self.counter = key, 0

    def draw(self, idx):
        from oracle.philox import env_step_words
        w0, w1, w2, w3 = (w[idx] for w in env_step_words(int(idx[-1]) + 1, self.counter, PHILOX_TAG, self.key))
        k = ((w1.astype(np.uint64) << np.uint64(32)) | w0.astype(np.uint64)) >> np.uint64(11)
        return k, (w2 >> np.uint32(31)).astype(np.int64), (w3 >> np.uint32(31)).astype(np.int64)

    def values(self, idx):
        k, h, p = self.draw(idx)
        self.last = (k, h, p)
        return reset_position(k), np.where(h > 0, 1.0, -1.0).astype(F32), np.where(p > 0, 0.5, -0.5)


class CarFlagOracle:
    def __init__(self, num_envs, time_limit=160, num_actions=None, draws=None):
        self.B = num_envs
        self.time_limit = time_limit
        self.table = None if num_actions is None else np.linspace(-1.0, 1.0, num_actions)
        self.draws = draws
        self.s = np.zeros((num_envs, 3), F32)
        self.elapsed = np.zeros(num_envs, np.int64)
        self.heavens = np.ones(num_envs, F32)
        self.priests = np.full(num_envs, 0.5)
        self.episodes = 0
        self.return_sum = 0.0
        self.length_sum = 0
        self.env_steps = 0
        self.last_reset = np.zeros(num_envs, bool)

    def _reset(self, mask):
        self.last_reset = mask.copy()
        idx = np.flatnonzero(mask)
        if len(idx) == 0:
            return
        x, hv, pr = self.draws.values(idx)
        self.s[idx, 0] = x
        self.s[idx, 1:] = 0
        self.elapsed[idx] = 0
        self.heavens[idx] = hv
        self.priests[idx] = pr

    def reset(self):
        self.episodes = self.length_sum = self.env_steps = 0
        self.return_sum = 0.0
        self._reset(np.ones(self.B, bool))
        return self.s.copy()

    def step(self, actions):
        """One step of every env (see `dynamics`), then the same-step reset of the finished ones."""
        a = np.asarray(actions).reshape(-1)
        if self.table is not None:
            a = self.table[a]
        self.elapsed += 1
        v, x, term, rew, direction = dynamics(self.s, self.heavens, self.priests, a)
        trunc = self.elapsed >= self.time_limit
        keep = ~term
        self.s[keep, 0] = x[keep].astype(F32)
        self.s[keep, 1] = v[keep].astype(F32)
        self.s[keep, 2] = direction[keep]
        done = term | trunc
        self.env_steps += self.B
        self.return_sum += float(rew.sum())
        self.episodes += int(done.sum())
        self.length_sum += int(self.elapsed[done].sum())
        self._reset(done)
        return self.s.copy(), rew, term, trunc


def frame(s0, heaven, priest):
    """The number-line frame of one env (uint8 [48, 600, 3]); see car_flag.py:156-178."""
    def px(x):
        return np.floor(np.interp(x, [-1.1, 1.1], [0, 596])).astype(int)
    img = np.zeros((48, 600, 3), np.uint8)
    img[:, :4] = 255
    img[:, -4:] = 255
    ends = px([-1, 1])
    hea, hell = (ends[1], ends[0]) if heaven > 0 else (ends[0], ends[1])
    img[:, hea:hea + 4, 1] = 255
    img[:, hell:hell + 4, 0] = 255
    car = px(s0[0])
    img[24:, car:car + 4] = 255 if s0[2] != 0 else 128
    lo, mid, hi = px([priest - 0.2, priest, priest + 0.2])
    img[:, lo:lo + 4, 2] = 128
    img[:, hi:hi + 4, 2] = 128
    img[:, mid:mid + 4, 2] = 255
    return img


# ---------------------------------------------------------------- action recipes of the fixtures ----
def make_actions(meta):
    """The action sequence [T, B] a carflag fixture was recorded with (carflag_index.json `recipe`)."""
    T, B = meta["steps"], meta["num_envs"]
    rng = np.random.default_rng(meta["action_seed"])
    out = []
    if meta["recipe"] == "bias":  # a per-env push of +-1 redrawn every `period` steps, plus uniform noise
        for t in range(T):
            if t % meta["period"] == 0:
                bias = rng.choice([-1.0, 1.0], B)
            out.append(np.clip(bias + rng.uniform(-1.0, 1.0, B), -1.5, 1.5))
        a = np.stack(out).astype(F32)
        return a.astype(np.float64) if meta["action_dtype"] == "float64" else a
    if meta["recipe"] == "held":  # a held discrete action redrawn every `period` steps, 30% uniform ones mixed in
        n = meta["num_actions"]
        for t in range(T):
            if t % meta["period"] == 0:
                hold = rng.choice([0, n - 1], B)
            out.append(np.where(rng.random(B) < 0.3, rng.integers(0, n, B), hold))
        return np.stack(out).astype(np.int64)
    raise ValueError(meta["recipe"])


# ---------------------------------------------------------------- fixtures ----
def load_index():
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "carflag_index.json")) as f:
        return here, json.load(f)


def load_case(name):
    """(meta, arrays) of one recorded case of tests/golden/carflag_index.json."""
    import os
    here, idx = load_index()
    meta = idx["cases"][name]
    return meta, np.load(os.path.join(here, meta["file"]), allow_pickle=False)


def load_render():
    import os
    here, idx = load_index()
    return np.load(os.path.join(here, idx["carflag_render"]["file"]), allow_pickle=False)


def rng_state(r):
    """A recorded PCG64 state ({state, inc, has_uint32, uinteger}, the big integers as strings) as numpy's
    bit_generator.state dict."""
    return {"bit_generator": "PCG64", "state": {"state": int(r["state"]), "inc": int(r["inc"])},
            "has_uint32": r["has_uint32"], "uinteger": r["uinteger"]}


def final_rng_state(meta):
    """The recorded final PCG64 state as numpy's bit_generator.state dict."""
    return rng_state(meta["final_rng"])


# ---------------------------------------------------------------- one-step tables ----
TABLE_NAMES = ("carflag_table_f32", "carflag_table_f64", "carflag_table_disc2", "carflag_table_disc4",
               "carflag_table_disc5")


def load_table(name):
    """(meta, arrays) of one one-step table (carflag_index.json `tables`): ONE reference step of a B-row env whose
    rows were planted (s0, elapsed0, heavens0, priests0) after a seeded reset, with the action `act`, the reference's
    obs / rew / term / trunc, its state after the step (final_*) and the draws of the rows that reset."""
    import os
    here, idx = load_index()
    meta = idx["tables"][name]
    return meta, dict(np.load(os.path.join(here, meta["file"]), allow_pickle=False))


def table_oracle(meta, d, draws):
    """The oracle with a table's rows planted."""
    ora = CarFlagOracle(meta["rows"], meta["time_limit"], meta.get("num_actions"), draws)
    ora.s[:] = d["s0"]
    ora.elapsed[:] = d["elapsed0"]
    ora.heavens[:] = d["heavens0"]
    ora.priests[:] = d["priests0"]
    return ora


def bits_equal(got, want):
    """Elementwise: the same bits, or a NaN where `want` (the reference) holds a NaN. float32 / float64 by their
    bits (so -0.0 != 0.0), everything else by value."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype.kind != "f":
        return got == want
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return np.where(np.isnan(want), np.isnan(got), got.view(u) == want.view(u))


CASE_NAMES = ("carflag_f32_b64", "carflag_f32_tl40_b63", "carflag_f64_b64", "carflag_disc5_b64")
