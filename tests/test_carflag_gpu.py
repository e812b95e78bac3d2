"""GPU parity of the Car-Flag backend (csrc/carflag.hip) with the fixtures recorded from the reference
(tests/golden/carflag_*.npz) and with the NumPy restatement (tests/carflag_oracle.py), in numpy, replay and
philox mode. Everything is compared bit for bit (float32 by value on finite data and by digest of the bits)."""
import numpy as np
import pytest

from carflag_oracle import (CASE_NAMES, CarFlagOracle, FollowDraws, NumpyDraws, final_rng_state, load_case,
                            load_render, make_actions)
from fixtures import digest

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


@pytest.mark.parametrize("B", [1000, 70001])
def test_philox_rollout_equals_steps_and_oracle(B, gpu_device):
    """One fused K = 37 launch == 37 single steps == the oracle fed the device's reset values (dynamics, rewards
    and flags bit-exact; the reset values read back through get_state and checked against their law)."""
    import torch
    from gym_po_amd import CarVecEnv
    K, tl = 37, 20
    a, b = CarVecEnv(B, time_limit=tl, rng_mode="philox"), CarVecEnv(B, time_limit=tl, rng_mode="philox")
    fd = FollowDraws()
    ora = CarFlagOracle(B, tl, None, fd)
    _eq(_np(a.reset(seed=5)[0]), _np(b.reset(seed=5)[0]))
    rng = np.random.default_rng(B + 1)
    el = rng.integers(0, tl, B)  # staggered: resets at every step, all B within the launch
    a.set_state(elapsed=el)
    b.set_state(elapsed=el)

    def follow():
        s, _, hv, pr = (_np(x) for x in b.get_state())
        fd.set(s[:, 0], hv, pr)
        return s, hv, pr

    follow()
    ora.reset()
    ora.elapsed[:] = el
    acts = (rng.choice([-1.0, 1.0], B) + rng.uniform(-1.0, 1.0, (K, B))).astype(np.float32)
    # a quarter of the envs start near an end, so that terminations (both rewards) happen inside 37 steps
    near = rng.random(B) < 0.25
    s0 = ora.s.copy()
    s0[near, 0] = rng.choice([-0.9, 0.9], int(near.sum())).astype(np.float32)
    for e in (a, b):
        e.set_state(s=s0)
    ora.s[:] = s0
    ro, rr, rd, rt = a.rollout(torch.as_tensor(acts, device=gpu_device))
    nreset = 0
    for t in range(K):
        o, r, d, tr, _ = b.step(acts[t])
        assert torch.equal(o, ro[t]) and torch.equal(r, rr[t]) and torch.equal(d, rd[t]) and torch.equal(tr, rt[t]), t
        s, hv, pr = follow()
        oo, ro_, do_, to_ = ora.step(acts[t])
        _eq(_np(o), oo, f"obs t={t}")
        _eq(_np(r), ro_, f"rew t={t}")
        _eq(_np(d), do_, f"term t={t}")
        _eq(_np(tr), to_, f"trunc t={t}")
        m = ora.last_reset
        nreset += int(m.sum())
        assert (np.abs(s[m, 0]) <= np.float32(0.2)).all() and not s[m, 1:].any()
        assert np.isin(hv[m], (-1.0, 1.0)).all() and np.isin(pr[m], (-0.5, 0.5)).all()
    for x, y in zip(a.get_state(), b.get_state()):
        assert torch.equal(x, y)
    assert nreset >= B and (_np(rr) > 0).any() and (_np(rr) < 0).any()
    ma, mb = a.metrics(), b.metrics()
    assert ma == mb and ma["episodes"] == ora.episodes and ma["length_sum"] == ora.length_sum


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
