"""GPU parity of the Car-Flag backend (csrc/carflag.hip) with the fixtures recorded from the reference
(tests/golden/carflag_*.npz) and with the NumPy restatement (tests/carflag_oracle.py), in numpy, replay and
philox mode. Everything is compared bit for bit (float32 by value on finite data and by digest of the bits)."""
import numpy as np
import pytest

from carflag_oracle import (CASE_NAMES, CarFlagOracle, FollowDraws, NumpyDraws, PhiloxDraws, ReplayDraws,
                            final_rng_state, load_case, load_render, make_actions)
from fixtures import digest
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy()


def _eq(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    if a.dtype == np.float32 or b.dtype == np.float32:
        assert a.dtype == b.dtype, what
        assert digest(a) == digest(b), what  # the f32 bits (also tells -0.0 from 0.0)
    np.testing.assert_array_equal(a, b, err_msg=what)


def _make(meta, rng_mode, **kw):
    from gym_po_amd import CarVecEnv, DiscreteActionCarVecEnv
    if meta["env"] == "DiscreteActionCarVecEnv":
        return DiscreteActionCarVecEnv(meta["num_actions"], meta["num_envs"], time_limit=meta["time_limit"],
                                       rng_mode=rng_mode, **kw)
    return CarVecEnv(meta["num_envs"], time_limit=meta["time_limit"], rng_mode=rng_mode,
                     action_dtype=meta["action_dtype"], **kw)


def _check_final(env, meta, d):
    s, el, hv, pr = (_np(x) for x in env.get_state())
    _eq(s, d["final_s"], "final s")
    _eq(el.astype(np.int64), d["final_elapsed"], "final elapsed")
    _eq(hv, d["final_heavens"], "final heavens")
    _eq(pr.astype(np.float64), d["final_priests"], "final priests")
    done = d["term"] | d["trunc"]
    m = env.metrics()
    assert m["episodes"] == done.sum() and m["env_steps"] == done.size
    assert m["return_sum"] == float(d["rew"].astype(np.float64).sum())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_numpy_mode_steps_reproduce_fixture_from_seed(name, gpu_device):
    meta, d = load_case(name)
    env = _make(meta, "numpy")
    acts = make_actions(meta)
    B = meta["num_envs"]
    _eq(_np(env.reset(seed=meta["seed"])[0]), d["obs0"], "reset obs")
    for t in range(meta["steps"]):
        a = acts[t].reshape(B, 1) if meta["env"] == "CarVecEnv" and t % 2 else acts[t]  # the space's [B, 1] too
        o, r, tm, tr, _ = env.step(a)
        _eq(_np(o), d["obs"][t], f"obs t={t}")
        _eq(_np(r), d["rew"][t], f"rew t={t}")
        _eq(_np(tm), d["term"][t], f"term t={t}")
        _eq(_np(tr), d["trunc"][t], f"trunc t={t}")
    _check_final(env, meta, d)
    assert env.rng_state == final_rng_state(meta)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_numpy_mode_one_rollout_reproduces_fixture_from_seed(name, gpu_device):
    meta, d = load_case(name)
    env = _make(meta, "numpy")
    _eq(_np(env.reset(seed=meta["seed"])[0]), d["obs0"], "reset obs")
    o, r, tm, tr = env.rollout(make_actions(meta))
    _eq(_np(o), d["obs"], "obs")
    _eq(_np(r), d["rew"], "rew")
    _eq(_np(tm), d["term"], "term")
    _eq(_np(tr), d["trunc"], "trunc")
    _check_final(env, meta, d)
    assert env.rng_state == final_rng_state(meta)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_replay_mode_reproduces_fixture_from_recorded_draws(name, gpu_device):
    meta, d = load_case(name)
    env = _make(meta, "replay")
    acts = make_actions(meta)
    env.set_replay(d["k53"][0], d["hidx"][0], d["pidx"][0])
    _eq(_np(env.reset()[0]), d["obs0"], "reset obs")
    for t in range(meta["steps"]):
        env.set_replay(d["k53"][t + 1], d["hidx"][t + 1], d["pidx"][t + 1])
        o, r, tm, tr, _ = env.step(acts[t])
        _eq(_np(o), d["obs"][t], f"obs t={t}")
        _eq(_np(r), d["rew"][t], f"rew t={t}")
        _eq(_np(tm), d["term"][t], f"term t={t}")
        _eq(_np(tr), d["trunc"][t], f"trunc t={t}")
    _check_final(env, meta, d)


def test_f32_and_f64_action_paths_differ_and_match_their_fixtures(gpu_device):
    """One arithmetic path silently serving both dtypes would make the two runs equal."""
    out = {}
    for name in ("carflag_f32_b64", "carflag_f64_b64"):
        meta, d = load_case(name)
        env = _make(meta, "numpy")
        env.reset(seed=meta["seed"])
        out[name] = _np(env.rollout(make_actions(meta))[0])
        _eq(out[name], d["obs"], name)
    a, b = out.values()
    assert (a.view(np.uint32) != b.view(np.uint32)).sum() > 1000


@pytest.mark.parametrize("buffered", [False, True], ids=["empty", "buffered_half"])
@pytest.mark.parametrize("B", [1, 63, 1000, 70001])
def test_numpy_mode_vs_oracle_across_blocks(B, buffered, gpu_device):
    """45 steps at time_limit 20: every env truncates in lockstep at step 20 (a reset of all B envs from a step);
    at step 22 the elapsed counters are staggered, so that afterwards a sparse, changing subset resets each step
    and the rank scan crosses tiles. `buffered`: the stream starts with one 32-bit half buffered."""
    from gym_po_amd import CarVecEnv
    T, tl = 45, 20
    env = CarVecEnv(B, time_limit=tl)
    if buffered:
        gen = np.random.default_rng(7)
        gen.integers(0, 2)
        assert gen.bit_generator.state["has_uint32"] == 1
        env.np_random = gen
        o = env.reset()[0]
    else:
        gen = np.random.default_rng(7)
        o = env.reset(seed=7)[0]
    ora = CarFlagOracle(B, tl, None, NumpyDraws(gen))
    _eq(_np(o), ora.reset(), "reset obs")
    assert env.rng_state == gen.bit_generator.state
    rng = np.random.default_rng(B)
    for t in range(T):
        if t == 22:
            el = rng.integers(0, tl, B)
            env.set_state(elapsed=el)
            ora.elapsed[:] = el
        a = rng.uniform(-1.5, 1.5, B).astype(np.float32)
        o, r, tm, tr, _ = env.step(a)
        oo, ro, tmo, tro = ora.step(a)
        _eq(_np(o), oo, f"obs t={t}")
        _eq(_np(r), ro, f"rew t={t}")
        _eq(_np(tm), tmo, f"term t={t}")
        _eq(_np(tr), tro, f"trunc t={t}")
        if t in (19, 20, 30):
            assert env.rng_state == gen.bit_generator.state, f"t={t}"
    s, el, hv, pr = (_np(x) for x in env.get_state())
    _eq(s, ora.s)
    _eq(el.astype(np.int64), ora.elapsed)
    _eq(hv, ora.heavens)
    _eq(pr.astype(np.float64), ora.priests)
    assert env.rng_state == gen.bit_generator.state
    m = env.metrics()
    assert (m["episodes"], m["length_sum"], m["env_steps"], m["return_sum"]) == (
        ora.episodes, ora.length_sum, ora.env_steps, ora.return_sum)
    assert ora.episodes > B  # the lockstep reset and the sparse ones both happened


KINDS = ("float32", "float64", "disc4")


def _make_kind(kind, B, tl, rng_mode="philox"):
    """(env, num_actions of the oracle) of an action kind: "float32", "float64" or "disc<n>"."""
    from gym_po_amd import CarVecEnv, DiscreteActionCarVecEnv
    if kind.startswith("disc"):
        n = int(kind[4:])
        return DiscreteActionCarVecEnv(n, B, time_limit=tl, rng_mode=rng_mode), n
    return CarVecEnv(B, time_limit=tl, rng_mode=rng_mode, action_dtype=kind), None


def _kind_actions(kind, rng, K, B):
    """[K, B] actions that push every env one way most of the time (so that both ends are reached)."""
    if kind.startswith("disc"):
        n = int(kind[4:])
        hold = rng.choice([0, n - 1], B)
        return np.where(rng.random((K, B)) < 0.3, rng.integers(-n, n, (K, B)), hold)
    a = rng.choice([-1.0, 1.0], B) + rng.uniform(-1.0, 1.0, (K, B))
    return a.astype(np.float32) if kind == "float32" else a


def _check_state_and_metrics(env, ora, what=""):
    s, el, hv, pr = (_np(x) for x in env.get_state())
    _eq(s, ora.s, what + " s")
    _eq(el.astype(np.int64), ora.elapsed, what + " elapsed")
    _eq(hv, ora.heavens, what + " heavens")
    _eq(pr.astype(np.float64), ora.priests, what + " priests")
    m = env.metrics()
    assert (m["episodes"], m["length_sum"], m["env_steps"], m["return_sum"]) == (
        ora.episodes, ora.length_sum, ora.env_steps, ora.return_sum), what


def _philox_rollout_equals_steps_and_oracle(kind, B, gpu_device):
    import torch
    K, tl, seed = 37, 20, 5
    (a, n), (b, _) = _make_kind(kind, B, tl), _make_kind(kind, B, tl)
    dr = PhiloxDraws(philox_key(seed))  # the oracle: every draw predicted from the seed
    ora = CarFlagOracle(B, tl, n, dr)
    fd = FollowDraws()                  # the cross-check: an oracle fed the device's reset values
    chk = CarFlagOracle(B, tl, n, fd)
    want0 = ora.reset()  # counter 0, before the device has run
    o0 = _np(a.reset(seed=seed)[0])
    _eq(o0, _np(b.reset(seed=seed)[0]))
    _eq(o0, want0, "reset obs")
    rng = np.random.default_rng(B + 1)
    el = rng.integers(0, tl, B)  # staggered: resets at every step, all B within the launch
    a.set_state(elapsed=el)
    b.set_state(elapsed=el)

    def follow():
        s, _, hv, pr = (_np(x) for x in b.get_state())
        fd.set(s[:, 0], hv, pr)
        return s, hv, pr

    _, hv, pr = follow()
    _eq(hv, ora.heavens, "reset heavens")
    _eq(pr.astype(np.float64), ora.priests, "reset priests")
    chk.reset()
    ora.elapsed[:] = el
    chk.elapsed[:] = el
    acts = _kind_actions(kind, rng, K, B)
    # a quarter of the envs start near an end, so that terminations (both rewards) happen inside 37 steps
    near = rng.random(B) < 0.25
    s0 = ora.s.copy()
    s0[near, 0] = rng.choice([-0.9, 0.9], int(near.sum())).astype(np.float32)
    for e in (a, b):
        e.set_state(s=s0)
    ora.s[:] = s0
    chk.s[:] = s0
    # the whole run on the CPU first
    want = []
    for t in range(K):
        dr.counter = 1 + t
        want.append(ora.step(acts[t]) + (ora.last_reset,))
    dev_acts = torch.as_tensor(acts.astype(np.int32) if n else acts, device=gpu_device)
    ro, rr, rd, rt = a.rollout(dev_acts)
    nreset = 0
    for t in range(K):
        o, r, d, tr, _ = b.step(acts[t])
        assert torch.equal(o, ro[t]) and torch.equal(r, rr[t]) and torch.equal(d, rd[t]) and torch.equal(tr, rt[t]), t
        s, hv, pr = follow()
        for oo, ro_, do_, to_ in (want[t][:4], chk.step(acts[t])):
            _eq(_np(o), oo, f"obs t={t}")
            _eq(_np(r), ro_, f"rew t={t}")
            _eq(_np(d), do_, f"term t={t}")
            _eq(_np(tr), to_, f"trunc t={t}")
        m = chk.last_reset
        assert np.array_equal(m, want[t][4])
        nreset += int(m.sum())
        assert (np.abs(s[m, 0]) <= np.float32(0.2)).all() and not s[m, 1:].any()
        assert np.isin(hv[m], (-1.0, 1.0)).all() and np.isin(pr[m], (-0.5, 0.5)).all()
    for x, y in zip(a.get_state(), b.get_state()):
        assert torch.equal(x, y)
    assert nreset >= B and (_np(rr) > 0).any() and (_np(rr) < 0).any()
    ma, mb = a.metrics(), b.metrics()
    assert ma == mb and ma["episodes"] == ora.episodes and ma["length_sum"] == ora.length_sum
    _check_state_and_metrics(a, ora)
    a.check()


@pytest.mark.parametrize("B", [1000, 70001])
def test_philox_rollout_equals_steps_and_oracle(B, gpu_device):
    """One fused K = 37 launch == 37 single steps == the oracle run ahead of the device from the seed alone
    (PhiloxDraws: every reset draw predicted on the CPU; dynamics, rewards, flags and reset values bit-exact). The
    reset values read back through get_state feed a second oracle as a cross-check and are checked against their
    law."""
    _philox_rollout_equals_steps_and_oracle("float32", B, gpu_device)


@pytest.mark.parametrize("B", [1000, 4099])
@pytest.mark.parametrize("kind", ["float64", "disc4"])
def test_philox_rollout_equals_steps_and_oracle_f64_and_discrete(kind, B, gpu_device):
    """The same for cf_rollout<ACT_F64, philox> and cf_rollout<ACT_DISC, philox> (double2 / int4 action loads; at
    B = 4099 every row after the first starts off its 16-byte boundary: the scalar fallback)."""
    _philox_rollout_equals_steps_and_oracle(kind, B, gpu_device)


def test_philox_counters_across_resets_and_rollouts(gpu_device):
    """reset(seed) is counter 0; rollout(K1), rollout(K2), a second reset() without a seed and a step after it take
    the counters that follow, one each."""
    B, tl, seed, K1, K2 = 1027, 2, 9, 3, 2
    env, _ = _make_kind("float32", B, tl)
    dr = PhiloxDraws(philox_key(seed))
    ora = CarFlagOracle(B, tl, None, dr)
    _eq(_np(env.reset(seed=seed)[0]), ora.reset(), "reset(seed)")
    rng = np.random.default_rng(3)
    c = 0
    for K in (K1, K2):
        acts = rng.uniform(-1.5, 1.5, (K, B)).astype(np.float32)
        out = [_np(x) for x in env.rollout(acts)]
        for t in range(K):
            c += 1
            dr.counter = c
            for got, want, key in zip([x[t] for x in out], ora.step(acts[t]), ("obs", "rew", "term", "trunc")):
                _eq(got, want, f"{key} counter={c}")
    assert c == K1 + K2 and ora.episodes >= 2 * B
    _check_state_and_metrics(env, ora, "after two rollouts")
    dr.counter = c + 1
    _eq(_np(env.reset()[0]), ora.reset(), "second reset()")
    _check_state_and_metrics(env, ora, "after the second reset")
    a = rng.uniform(-1.5, 1.5, B).astype(np.float32)
    dr.counter = c + 2
    for got, want in zip(env.step(a)[:4], ora.step(a)):
        _eq(_np(got), want, "step after the second reset")
    dr.counter = c + 3
    for got, want in zip(env.step(a)[:4], ora.step(a)):  # tl = 2: every env truncates and resets here
        _eq(_np(got), want, "second step after the second reset")
    assert ora.last_reset.all()
    _check_state_and_metrics(env, ora, "end")


def test_reset_position_rounds_twice(gpu_device):
    """-0.2 + 0.4 u with the product rounded before the sum, as the reference does it. Around u = 1/2 the sum
    cancels to a few units of 2^-55 and the product's rounding IS the result, so a fused multiply-add (one rounding)
    gives another float32 on most of these draws; random draws would need about 2^29 tries to show it. Replay mode
    feeds the draws: through reset() (cf_reset) and through the same-step reset of a step (cf_rollout)."""
    from fractions import Fraction
    from carflag_oracle import reset_position
    from gym_po_amd import CarVecEnv
    B = 1027
    k = (np.int64(1) << 52) + np.arange(B, dtype=np.int64) - B // 2
    want = reset_position(k.astype(np.uint64))
    fused = np.array([float(Fraction(-0.2) + Fraction(0.4) * Fraction(int(x), 1 << 53)) for x in k]).astype(np.float32)
    assert (fused != want).sum() > B // 2 and np.abs(want).max() < 1e-12
    hp = np.zeros(B, np.int32)
    env = CarVecEnv(B, time_limit=1, rng_mode="replay")
    env.set_replay(k.astype(np.uint64), hp, hp)
    _eq(_np(env.reset()[0])[:, 0], want, "reset()")
    env.set_replay(k[::-1].astype(np.uint64).copy(), hp, hp)
    o = env.step(np.zeros(B, np.float32))[0]  # time_limit 1: every env resets in the step
    _eq(_np(o)[:, 0], want[::-1].copy(), "the reset inside a step")


# ------------------------------------------------------------------ launch shapes and store paths ----
def test_blocks_looping_over_several_tiles(gpu_device):
    """persist_bpc = 1: one block per CU, each looping over two tiles (block 0 over a third, ragged one): the state
    reload per tile, the action prefetch across tiles, metrics summed across tiles and, in numpy mode, the
    pending-reset count of every tile."""
    import torch
    from gym_po_amd import CarVecEnv
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B, K, tl, seed = 2 * 1024 * cus + 5, 6, 3, 3
    with debug_knobs(persist_bpc=1):
        env = CarVecEnv(B, time_limit=tl, rng_mode="philox")
        envn = CarVecEnv(B, time_limit=tl, rng_mode="numpy")
    for e in (env, envn):
        assert e.query("persist_blocks") == cus and (B + 1023) // 1024 == 2 * cus + 1
    dr = PhiloxDraws(philox_key(seed))
    ora = CarFlagOracle(B, tl, None, dr)
    _eq(_np(env.reset(seed=seed)[0]), ora.reset(), "reset obs")
    rng = np.random.default_rng(seed)
    x0 = ora.s.copy()
    x0[:, 0] = rng.choice([-0.95, 0.0, 0.95], B).astype(np.float32)  # terminations among the truncations
    x0[:, 1] = np.float32(0.0625) * np.sign(x0[:, 0])
    el = rng.integers(0, tl, B)
    env.set_state(s=x0, elapsed=el)
    ora.s[:] = x0
    ora.elapsed[:] = el
    acts = rng.uniform(-1.5, 1.5, (K, B)).astype(np.float32)
    out = [_np(x) for x in env.rollout(acts)]
    for t in range(K):
        dr.counter = 1 + t
        for got, want, key in zip([x[t] for x in out], ora.step(acts[t]), ("obs", "rew", "term", "trunc")):
            _eq(got, want, f"{key} t={t}")
    assert ora.episodes >= B and (out[1] > 0).any() and (out[1] < 0).any()
    _check_state_and_metrics(env, ora, "philox")
    env.check()
    # numpy mode, three steps: sparse resets, then (t = 2) a reset of every env left
    gen = np.random.default_rng(seed)
    oran = CarFlagOracle(B, tl, None, NumpyDraws(gen))
    _eq(_np(envn.reset(seed=seed)[0]), oran.reset(), "numpy reset obs")
    envn.set_state(s=x0)
    oran.s[:] = x0
    for t in range(3):
        for got, want, key in zip(envn.step(acts[t])[:4], oran.step(acts[t]), ("obs", "rew", "term", "trunc")):
            _eq(_np(got), want, f"numpy {key} t={t}")
        assert envn.rng_state == gen.bit_generator.state, t
    assert oran.episodes >= B
    _check_state_and_metrics(envn, oran, "numpy")


def _offset_view(torch, dtype, shape, offset, device):
    """A contiguous tensor of `shape` that starts `offset` elements into a larger allocation."""
    n = int(np.prod(shape))
    v = torch.zeros(n + 8, dtype=dtype, device=device)[offset:offset + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


@pytest.mark.parametrize("kind", KINDS)
def test_misaligned_caller_buffers(kind, gpu_device):
    """act / obs / rew / term / trunc views that start off their 16-byte (flags: 4-byte) boundaries take the scalar
    load and store paths, all together and each alone (the kernel chooses per buffer); float64 actions 8 bytes off.
    Written in place, equal to the aligned run and to the oracle."""
    import torch
    B, K, tl, seed = 1027, 5, 3, 4
    adt = {"float32": torch.float32, "float64": torch.float64}.get(kind, torch.int32)
    rng = np.random.default_rng(1)
    acts = _kind_actions(kind, rng, K, B)
    dev = torch.as_tensor(acts, device=gpu_device).to(adt)
    el = rng.integers(0, tl, B)
    x0 = rng.choice([-0.95, 0.0, 0.95], B).astype(np.float32)

    def fresh():
        env, n = _make_kind(kind, B, tl)
        o = _np(env.reset(seed=seed)[0])
        s = np.stack([x0, np.float32(0.0625) * np.sign(x0), np.zeros(B, np.float32)], 1)  # the ends are reached
        env.set_state(s=s, elapsed=el)
        return env, n, o, s

    env, n, o0, s = fresh()
    dr = PhiloxDraws(philox_key(seed))
    ora = CarFlagOracle(B, tl, n, dr)
    _eq(o0, ora.reset(), "reset obs")
    ora.s[:] = s
    ora.elapsed[:] = el
    ref = [_np(x) for x in env.rollout(dev)]
    for t in range(K):
        dr.counter = 1 + t
        for got, want, key in zip([x[t] for x in ref], ora.step(acts[t]), ("obs", "rew", "term", "trunc")):
            _eq(got, want, f"aligned {key} t={t}")
    _check_state_and_metrics(env, ora, "aligned")
    assert ora.episodes >= B and ref[2].any()
    # offsets in elements of (act, obs, rew, term, trunc)
    for offs in ((1, 3, 1, 1, 3), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 2, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 2)):
        env = fresh()[0]
        act = _offset_view(torch, adt, (K, B), offs[0], gpu_device)
        act.copy_(dev)
        out = (_offset_view(torch, torch.float32, (K, B, 3), offs[1], gpu_device),
               _offset_view(torch, torch.float32, (K, B), offs[2], gpu_device),
               _offset_view(torch, torch.uint8, (K, B), offs[3], gpu_device),
               _offset_view(torch, torch.uint8, (K, B), offs[4], gpu_device))
        got = env.rollout(act, out=out)
        assert [x.data_ptr() for x in got] == [x.data_ptr() for x in out]  # written in place, not into copies
        for g, want, key in zip(got, ref, ("obs", "rew", "term", "trunc")):
            _eq(_np(g), want, f"{key} offsets={offs}")
        _check_state_and_metrics(env, ora, f"offsets={offs}")
        env.check()


# ------------------------------------------------------------------ limits and errors ----
@pytest.mark.parametrize("mode", ["philox", "numpy"])
@pytest.mark.parametrize("planted", [1, 2], ids=["tl-1", "tl-2"])
@pytest.mark.parametrize("B", [8, 1029])
def test_largest_time_limit(B, planted, mode, gpu_device):
    """time_limit = 2^29 (the largest accepted) with every env one or two steps short of it: the truncation
    compare, the 30-bit elapsed field, and a length sum of B * 2^29 (2^32 at B = 8) kept exact."""
    from gym_po_amd import CarVecEnv
    tl, seed = 2 ** 29, 6
    env = CarVecEnv(B, time_limit=tl, rng_mode=mode)
    if mode == "philox":
        dr = PhiloxDraws(philox_key(seed))
        dr.counter = 1
    else:
        gen = np.random.default_rng(seed)
        dr = NumpyDraws(gen)
    ora = CarFlagOracle(B, tl, None, dr)
    env.reset(seed=seed)
    el = np.full(B, tl - planted)
    s = np.zeros((B, 3), np.float32)
    hv, pr = np.ones(B, np.float32), np.full(B, 0.5)
    env.set_state(s=s, elapsed=el, heavens=hv, priests=pr)
    ora.s[:], ora.elapsed[:], ora.heavens[:], ora.priests[:] = s, el, hv, pr
    if mode == "numpy":
        dr.draw(np.arange(B))  # the reset(seed) of the device took these
        assert env.rng_state == gen.bit_generator.state
    a = np.zeros(B, np.float32)
    o, r, tm, tr, _ = env.step(a)
    for got, want, key in zip((o, r, tm, tr), ora.step(a), ("obs", "rew", "term", "trunc")):
        _eq(_np(got), want, key)
    assert _np(tr).all() == (planted == 1) and _np(tr).any() == (planted == 1) and not _np(tm).any()
    _eq(_np(env.get_state()[1]).astype(np.int64), np.full(B, 0 if planted == 1 else tl - 1), "elapsed")
    m = env.metrics()
    want = (B, B * tl) if planted == 1 else (0, 0)
    assert (ora.episodes, ora.length_sum) == want
    assert (int(m["episodes"]), int(m["length_sum"])) == want and m["length_sum"] == float(want[1])
    if mode == "numpy":
        assert env.rng_state == gen.bit_generator.state


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["philox", "numpy", "replay"])
def test_time_limit_one_resets_every_env_every_step(mode, kind, gpu_device):
    """time_limit = 1: all B envs reset at every one of 5 steps (the resolver gets the full batch every call)."""
    B, seed, T = 1029, 8, 5
    env, n = _make_kind(kind, B, 1, rng_mode=mode)
    rng = np.random.default_rng(2)
    if mode == "philox":
        dr = PhiloxDraws(philox_key(seed))
    elif mode == "numpy":
        gen = np.random.default_rng(seed)
        dr = NumpyDraws(gen)
    else:
        dr = ReplayDraws()
        draws = [(rng.integers(0, 1 << 53, B).astype(np.uint64), rng.integers(0, 2, B), rng.integers(0, 2, B))
                 for _ in range(T + 1)]
        dr.set(*draws[0])
        env.set_replay(*draws[0])
    ora = CarFlagOracle(B, 1, n, dr)
    _eq(_np(env.reset(seed=seed)[0]), ora.reset(), "reset obs")
    acts = _kind_actions(kind, rng, T, B)
    for t in range(T):
        if mode == "philox":
            dr.counter = 1 + t
        elif mode == "replay":
            dr.set(*draws[t + 1])
            env.set_replay(*draws[t + 1])
        for got, want, key in zip(env.step(acts[t])[:4], ora.step(acts[t]), ("obs", "rew", "term", "trunc")):
            _eq(_np(got), want, f"{key} t={t}")
        assert ora.last_reset.all()
        if mode == "numpy":
            assert env.rng_state == gen.bit_generator.state, t
    assert ora.episodes == T * B and ora.length_sum == T * B
    _check_state_and_metrics(env, ora)
    env.check()


def test_limits_and_misuse_raise(gpu_device):
    from gym_po_amd import CarVecEnv, DiscreteActionCarVecEnv
    from gym_po_amd._lib import GymPoError
    for tl in (0, 2 ** 29 + 1):
        with pytest.raises(GymPoError):
            CarVecEnv(8, time_limit=tl, rng_mode="philox")
    CarVecEnv(8, time_limit=2 ** 29, rng_mode="philox")
    with pytest.raises(ValueError):
        DiscreteActionCarVecEnv(1, 8, rng_mode="philox")
    env = CarVecEnv(8, rng_mode="replay")
    with pytest.raises(GymPoError):
        env.reset()  # a replay reset without draws
    with pytest.raises(GymPoError):
        env.step(np.zeros(8, np.float32))  # step before reset
    env.set_state(elapsed=np.zeros(8, np.int32))  # a planted state stands for a reset
    with pytest.raises(GymPoError):
        env.step(np.zeros(8, np.float32))  # a replay step without draws
    env = CarVecEnv(8, rng_mode="philox")
    with pytest.raises(GymPoError):
        env.step(np.zeros(8, np.float32))  # step before reset
    env.reset(seed=1)
    with pytest.raises(GymPoError):
        env.rng_state
    with pytest.raises(GymPoError):
        env.rng_state = np.random.default_rng(1).bit_generator.state


def test_philox_reset_choices_are_uniform(gpu_device):
    from gym_po_amd import CarVecEnv
    N = 1 << 16
    env = CarVecEnv(N, rng_mode="philox")
    env.reset(seed=123)
    s, el, hv, pr = (_np(x) for x in env.get_state())
    assert (np.abs(s[:, 0]) <= np.float32(0.2)).all() and not s[:, 1:].any() and not el.any()
    assert -0.01 < float(s[:, 0].mean()) < 0.01 and len(np.unique(s[:, 0])) > N // 2
    sd = np.sqrt(N * 0.25 * 0.75)
    for h in (-1.0, 1.0):
        for p in (-0.5, 0.5):
            n = int(((hv == h) & (pr == p)).sum())
            assert abs(n - N / 4) <= 5 * sd, (h, p, n)


def test_discrete_action_out_of_range_flags_and_negative_wraps(gpu_device):
    import torch
    from gym_po_amd import DiscreteActionCarVecEnv
    from gym_po_amd._lib import GymPoError
    B = 8
    a, b = (DiscreteActionCarVecEnv(5, B, rng_mode="philox") for _ in range(2))
    assert a.action_names == ["<<:", "<:", ":", ":>", ":>>"] and a.single_action_space.n == 5
    a.reset(seed=1)
    b.reset(seed=1)
    oa = a.step(torch.full((B,), -1, dtype=torch.int32, device=gpu_device))[0]
    ob = b.step(torch.full((B,), 4, dtype=torch.int32, device=gpu_device))[0]
    assert torch.equal(oa, ob)
    a.check()
    with pytest.raises(IndexError):
        a.step(np.full(B, 5))
    a.step(torch.full((B,), 5, dtype=torch.int32, device=gpu_device))
    with pytest.raises(GymPoError):
        a.check()


def test_state_round_trip(gpu_device):
    import torch
    from gym_po_amd import CarVecEnv
    B = 1027
    a, b = CarVecEnv(B, time_limit=30, rng_mode="philox"), CarVecEnv(B, time_limit=30, rng_mode="philox")
    a.reset(seed=2)
    b.reset(seed=2)
    acts = torch.rand((25, B), device=gpu_device) * 3 - 1.5
    a.rollout(acts)
    b.rollout(acts)
    st = a.get_state()
    assert (_np(st[1]) > 0).all() and st[0].dtype == torch.float32 and tuple(st[0].shape) == (B, 3)
    b.set_state(s=torch.zeros_like(st[0]), elapsed=torch.zeros_like(st[1]), heavens=-st[2], priests=-st[3])
    b.set_state(*st)
    for x, y in zip(st, b.get_state()):
        assert torch.equal(x, y)
    ra, rb = a.rollout(acts), b.rollout(acts)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)


def test_render_matches_recorded_frames(gpu_device):
    from gym_po_amd import CarVecEnv
    d = load_render()
    env = CarVecEnv(2, render_mode="rgb_array", rng_mode="philox")
    env.reset(seed=0)
    for i in range(len(d["frames"])):
        env.set_state(s=np.stack([d["s0"][i], np.zeros(3, np.float32)]), heavens=[d["heavens"][i], 1.0],
                      priests=[d["priests"][i], 0.5])
        img = env.render()
        assert isinstance(img, np.ndarray) and img.dtype == np.uint8
        np.testing.assert_array_equal(img, d["frames"][i], err_msg=f"frame {i}")
    with pytest.raises(NotImplementedError):
        CarVecEnv(2, rng_mode="philox").render()
