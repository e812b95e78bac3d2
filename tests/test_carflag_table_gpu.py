"""The Car-Flag one-step tables (tests/golden/carflag_table_*.npz: one reference step over rows planted on every
threshold, one ulp either side of it, and on non-finite and denormal actions) through every kernel path of
csrc/carflag.hip that can execute them: replay, numpy and philox mode, `step` and fused `rollout`, with the rows in
their recorded order, permuted, and padded to every batch size modulo 4. Everything is compared by bits; an element
that is NaN in the reference must be NaN (tests/test_carflag_table_cpu.py pins the oracle used for the permuted
orders and for the steps after the first to the same tables)."""
import numpy as np
import pytest

from carflag_oracle import (TABLE_NAMES, NumpyDraws, PhiloxDraws, ReplayDraws, bits_equal, load_table,
                            reset_position, rng_state, table_oracle)
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

ORDERS = ("recorded", "permuted", "pad0", "pad1", "pad3")


def _np(x):
    return x.cpu().numpy()


def _same(got, want, what):
    got = _np(got) if hasattr(got, "cpu") else np.asarray(got)
    if got.dtype != want.dtype:
        assert got.dtype.kind == want.dtype.kind or want.dtype.kind in "iu", (what, got.dtype, want.dtype)
        got = got.astype(want.dtype)
    bad = np.argwhere(~bits_equal(got, want))
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


def _rows(d, order):
    """Row indices of the table in the order they are planted: recorded, permuted by a fixed seed (every row in
    another lane slot and tile), or padded with copies of row 0 to B = 4 k + r."""
    n = len(d["term"])
    if order == "recorded":
        return np.arange(n)
    if order == "permuted":
        return np.random.default_rng(20).permutation(n)
    r = int(order[3:])
    idx = np.concatenate([np.arange(n), np.zeros((r - n) % 4 + 4, np.int64)])
    assert len(idx) % 4 == r
    return idx


def _make(meta, B, rng_mode):
    from gym_po_amd import CarVecEnv, DiscreteActionCarVecEnv
    if meta["env"] == "DiscreteActionCarVecEnv":
        return DiscreteActionCarVecEnv(meta["num_actions"], B, time_limit=meta["time_limit"], rng_mode=rng_mode)
    return CarVecEnv(B, time_limit=meta["time_limit"], rng_mode=rng_mode, action_dtype=meta["action_dtype"])


def _setup(name, order, draws):
    meta, d = load_table(name)
    idx = _rows(d, order)
    sub = {k: v[idx] for k, v in d.items()}
    ora = table_oracle(dict(meta, rows=len(idx)), sub, draws)
    return meta, sub, ora, order == "recorded"


def _plant(env, sub):
    env.set_state(s=sub["s0"], elapsed=sub["elapsed0"], heavens=sub["heavens0"], priests=sub["priests0"])
    s = _np(env.get_state()[0])
    _same(s, sub["s0"], "planted s (old direction included)")


def _check_step(out, want, sub, first=True, what=""):
    """Device outputs of one step against the oracle's, and (the table's own step) against the recorded rows."""
    for got, w, key in zip(out, want, ("obs", "rew", "term", "trunc")):
        _same(got, w, f"{what} {key}")
    if first:
        for got, key in zip(out[1:], ("rew", "term", "trunc")):
            _same(got, sub[key], f"{what} table {key}")
        stay = ~(sub["term"] | sub["trunc"])
        _same(_np(out[0])[stay], sub["obs"][stay], f"{what} table obs of the rows that go on")


def _check_state(env, ora, sub=None, what=""):
    s, el, hv, pr = env.get_state()
    _same(s, ora.s, what + " s")
    _same(el, ora.elapsed, what + " elapsed")
    _same(hv, ora.heavens, what + " heavens")
    _same(pr, ora.priests, what + " priests")
    if sub is not None:  # the recorded order with the recorded draws: the table's own final state
        for got, key in ((s, "final_s"), (el, "final_elapsed"), (hv, "final_heavens"), (pr, "final_priests")):
            _same(got, sub[key], what + " table " + key)
    m = env.metrics()
    assert (m["episodes"], m["length_sum"], m["env_steps"], m["return_sum"]) == (
        ora.episodes, ora.length_sum, ora.env_steps, ora.return_sum), what
    env.check()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_table_replay(name, order, gpu_device):
    dr = ReplayDraws()
    meta, sub, ora, _ = _setup(name, order, dr)
    dr.set(sub["k53"], sub["hidx"], sub["pidx"])
    env = _make(meta, len(sub["term"]), "replay")
    env.set_replay(sub["k53"], sub["hidx"], sub["pidx"])
    env.reset()
    _plant(env, sub)
    out = env.step(sub["act"])[:4]
    _check_step(out, ora.step(sub["act"]), sub)
    _same(out[0], sub["obs"], "table obs")  # the recorded draws: every row, the reset ones included
    _check_state(env, ora, sub)


@pytest.mark.parametrize("order,buffered", [("recorded", False), ("recorded", True), ("permuted", False),
                                            ("pad0", True), ("pad1", True), ("pad3", False)])
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_table_numpy(name, order, buffered, gpu_device):
    """From the recorded PCG64 state (`buffered`: with a 32-bit half planted in the stream's buffer, which the heaven
    picks take first): the resetting rows share the stream by rank, whatever order they are in."""
    gen = np.random.Generator(np.random.PCG64())
    meta, sub, ora, recorded = _setup(name, order, NumpyDraws(gen))
    st = rng_state(meta["rng_before"])
    if buffered:
        st.update(has_uint32=1, uinteger=0x80000001)
    gen.bit_generator.state = st
    env = _make(meta, len(sub["term"]), "numpy")
    env.reset(seed=0)
    _plant(env, sub)
    env.rng_state = st
    out = env.step(sub["act"])[:4]
    _check_step(out, ora.step(sub["act"]), sub)
    exact = recorded and not buffered
    if exact:
        _same(out[0], sub["obs"], "table obs")
        assert env.rng_state == rng_state(meta["rng_after"])
    assert env.rng_state == gen.bit_generator.state
    _check_state(env, ora, sub if exact else None)


def _more_actions(meta, sub, K):
    """[K, B] actions whose first row is the table's."""
    B = len(sub["act"])
    rng = np.random.default_rng(B)
    n = meta.get("num_actions")
    if n is not None:
        more = rng.integers(-n, n, (K - 1, B))
    else:
        more = rng.uniform(-1.5, 1.5, (K - 1, B)).astype(sub["act"].dtype)
    return np.concatenate([sub["act"][None], more])


@pytest.mark.parametrize("order,via", [("recorded", "step"), ("recorded", "rollout1"), ("recorded", "rollout3"),
                                       ("permuted", "rollout3"), ("pad0", "rollout3"), ("pad1", "rollout3"),
                                       ("pad3", "rollout3"), ("pad1", "step")])
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_table_philox(name, order, via, gpu_device):
    """The fused cf_rollout<ACT, philox> of every action kind: rows that go on against the table, rows that reset
    against the draws predicted from the seed (block (env, counter), counter 0 for reset(seed), then one per step).
    K = 3: the table is the first step of one launch; with B = 4 k + 1 / 3 its later rows start off 16 bytes."""
    seed = 77
    dr = PhiloxDraws(philox_key(seed))
    meta, sub, ora, _ = _setup(name, order, dr)
    B = len(sub["term"])
    env = _make(meta, B, "philox")
    obs0 = env.reset(seed=seed)[0]
    k, h, p = dr.draw(np.arange(B))
    _same(obs0[:, 0], reset_position(k), "reset(seed) positions at counter 0")
    _same(env.get_state()[2], np.where(h > 0, 1.0, -1.0).astype(np.float32), "reset(seed) heavens")
    _same(env.get_state()[3], np.where(p > 0, 0.5, -0.5).astype(np.float32), "reset(seed) priests")
    _plant(env, sub)
    K = 3 if via == "rollout3" else 1
    acts = _more_actions(meta, sub, K)
    if via == "step":
        out = [x[None] for x in env.step(acts[0])[:4]]
    else:
        out = env.rollout(acts)
    assert tuple(out[0].shape) == (K, B, 3)
    for t in range(K):
        dr.counter = 1 + t
        with np.errstate(invalid="ignore"):
            want = ora.step(acts[t])
        _check_step([x[t] for x in out], want, sub, first=t == 0, what=f"t={t}")
    _check_state(env, ora)
