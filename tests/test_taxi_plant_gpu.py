"""Taxi exact mode (rng_mode="numpy", csrc/taxi.hip) on maps whose location count is no power of two, and on planted
draws that no seed reaches. Comparator: the oracle (oracle/taxi.py) on numpy's Generator in the same PCG64 state;
tolerance: none. tests/test_stream_plant_cpu.py asserts for every planted case that numpy takes the rare branch.

Part 1, L = 6 and L = 3 locations (L (L + 1) states per cell; `integers(L)` has a Lemire threshold of 4 / 1, while the
shipped maps' L = 4 rejects nothing): seeded baselines in numpy mode on both kernels, scalar and Hansen obs, and in
philox mode; then planted passenger / destination rejections: np_pd_parallel gives up on any rejected half-word and
np_draws walks the stream serially (np_integers, the `while d == p` redraw rounds), in the one-workgroup kernel and in
taxi_npg_draws.

Part 2, the default map: the word 2^64 - 1 planted as the double of one category of one multinomial row, where
random_binomial_inversion runs past its bound and restarts with one more double. That moves the row's deficit by -1
in the speculative chain of np_reset_rows (64 rows x 16 deficits per round) and in the windowed candidate chain of
taxi_npg_rows (1024 rows x 64 starts per round).
"""
import numpy as np
import pytest

import plant_cases as pc
import stream_plant as sp
from oracle.draws import ReplayDraws
from oracle.taxi import TaxiOracle

pytestmark = pytest.mark.gpu


def _make_env(B, kw, knobs, gpu_device, **extra):
    from gym_po_amd import TaxiVecEnv
    from gym_po_amd._lib import debug_knobs
    with debug_knobs(**knobs):
        return TaxiVecEnv(B, **kw, device=gpu_device, **extra)


def _np4(x):
    return [v.cpu().numpy() for v in x[:4]]


def _check_step(got, want, tag):
    o, r, d, t = got
    oo, ro, do, to = want
    np.testing.assert_array_equal(o.astype(np.int64), np.asarray(oo).astype(np.int64), err_msg="obs " + tag)
    np.testing.assert_array_equal(r, ro, err_msg="rew " + tag)
    np.testing.assert_array_equal(d.astype(bool), do, err_msg="term " + tag)
    np.testing.assert_array_equal(t.astype(bool), to, err_msg="trunc " + tag)


def _check_state(env, ora):
    s, el, nd = (x.cpu().numpy() for x in env.get_state())
    np.testing.assert_array_equal(s, ora.s, err_msg="s")
    np.testing.assert_array_equal(el, ora.elapsed, err_msg="elapsed")
    np.testing.assert_array_equal(nd, ora.n_dropoffs_completed, err_msg="n_dropoffs")
    env.check()  # no GP_DERR_* flag
    assert sp.rng6(env.rng_state) == sp.rng6(ora.gen.bit_generator.state)


def _ordinary_steps(env, ora, steps, seed):
    acts = np.random.default_rng(seed).integers(0, 5, (steps, env.num_envs))
    for t in range(steps):
        _check_step(_np4(env.step(acts[t])), ora.step_seeded(acts[t]), f"after the plant, t={t}")


# ------------------------------------------------------------------- part 1: L not a power of two ----
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("hansen", [False, True])
@pytest.mark.parametrize("knobs", [{}, {"taxi_npg_min": 0}], ids=["one_workgroup", "grid_wide"])
@pytest.mark.parametrize("mapname", ["six", "three"])
def test_numpy_mode_baseline_on_non_power_of_two_maps(mapname, knobs, hansen, K, gpu_device):
    import torch
    B, T = 256, 40
    kw = dict(map=pc.TAXI_MAPS[mapname], num_passengers=2, time_limit=15, hansen_obs=hansen)
    env = _make_env(B, kw, knobs, gpu_device, rng_mode="numpy")
    ora = TaxiOracle(B, **kw)
    assert env.ns == ora.ns and env.no == ora.no and env.nlocs == ora.nlocs
    o0, _ = env.reset(seed=17)
    np.testing.assert_array_equal(o0.cpu().numpy().astype(np.int64), np.asarray(ora.reset_seed(17)).astype(np.int64))
    acts = np.random.default_rng(18).integers(0, 5, (T, B))
    eps = tasks = 0
    for t0 in range(0, T, K):
        k = min(K, T - t0)
        a = torch.as_tensor(acts[t0:t0 + k].astype(np.int32), device=env.device)
        got = [x[None] for x in _np4(env.step(a[0]))] if k == 1 else _np4(env.rollout(a))
        for j in range(k):
            want = ora.step_seeded(acts[t0 + j])
            _check_step([g[j] for g in got], want, f"t={t0 + j}")
            eps += int((want[2] | want[3]).sum())
            tasks += int((want[1] == ora.GOAL_MOVE).sum())
        _check_state(env, ora)
    assert eps >= B and tasks > 0  # resets (multinomial rows) and completions (integers(L)) both happened
    m = env.metrics()
    assert m["episodes"] == eps and m["env_steps"] == T * B


@pytest.mark.parametrize("hansen", [False, True])
@pytest.mark.parametrize("mapname", ["six", "three"])
def test_philox_mode_steps_follow_the_oracle_on_non_power_of_two_maps(mapname, hansen, gpu_device):
    """Philox mode draws its own start states and passenger / destination pairs; everything else is the step's. Each
    step the oracle starts from the device's state and is handed the states the device landed in as replay draws
    (as test_taxi_gpu.py's replay runs do in the other direction): obs, reward and flags must agree, every drawn
    start state must be a valid one, and every redrawn pair must have d != p."""
    B, T = 4099, 40
    kw = dict(map=pc.TAXI_MAPS[mapname], num_passengers=2, time_limit=15, hansen_obs=hansen)
    env = _make_env(B, kw, {}, gpu_device, rng_mode="philox")
    ora = TaxiOracle(B, **kw)
    L, lpl = ora.nlocs, ora.nlocs * (ora.nlocs + 1)
    env.reset(seed=3)
    valid = set(int(v) for v in ora.valid_states)
    acts = np.random.default_rng(4).integers(0, 5, (T, B))
    for t in range(T):
        s, el, nd = (x.cpu().numpy() for x in env.get_state())
        if t == 0:
            assert set(int(v) for v in s) <= valid
        ora.s, ora.elapsed, ora.n_dropoffs_completed = s.astype(int), el.astype(int), nd.astype(np.float64)
        got = _np4(env.step(acts[t]))
        s2 = env.get_state()[0].cpu().numpy().astype(int)
        want = ora.step(acts[t], ReplayDraws({"reset_state": s2, "pd": s2 % lpl}))
        _check_step(got, want, f"t={t}")
        np.testing.assert_array_equal(ora.s, s2)
        reset = want[2] | want[3]
        assert set(int(v) for v in s2[reset]) <= valid
        task = (want[1] == ora.GOAL_MOVE) & ~reset
        p, d = (s2[task] % lpl) // L, s2[task] % L
        assert (p < L).all() and (p != d).all()


@pytest.mark.parametrize("case", pc.taxi_pd_cases(), ids=pc.taxi_pd_id)
def test_planted_passenger_destination_rejection_vs_oracle(case, gpu_device):
    import torch
    c = pc.taxi_pd_build(case)
    env = _make_env(c.B, c.kw, c.knobs, gpu_device, rng_mode="numpy")
    ora = c.ora
    env.reset(seed=2)
    env.set_state(s=c.s, elapsed=np.zeros(c.B, np.int32), n_dropoffs=np.zeros(c.B, np.int32))
    env.rng_state = c.st
    a = torch.as_tensor(c.actions.astype(np.int32), device=env.device)
    got = [x[None] for x in _np4(env.step(a[0]))] if c.mode == "step" else _np4(env.rollout(a))
    for k in range(c.actions.shape[0]):
        want = ora.step_seeded(c.actions[k])
        _check_step([g[k] for g in got], want, f"step {k} (planted: {c.planted_step})")
        assert int((want[1] == ora.GOAL_MOVE).sum()) == (case[2] if k == c.planted_step else 0)
    _check_state(env, ora)
    _ordinary_steps(env, ora, 5, seed=c.h)
    _check_state(env, ora)


# --------------------------------------------------------------------- part 2: inversion restart ----
@pytest.mark.parametrize("case", pc.taxi_row_cases(), ids=pc.taxi_row_id)
def test_planted_inversion_restart_vs_oracle(case, gpu_device):
    path, place, row, what = case
    c = pc.taxi_row_build(case)
    env = _make_env(c.B, c.kw, c.knobs, gpu_device, rng_mode="numpy")
    ora = c.ora
    if place == "reset":
        env.rng_state = c.info["state"]
        o, _ = env.reset()
        from oracle.draws import NumpyDraws
        oo = ora.reset(NumpyDraws(ora.gen))
        np.testing.assert_array_equal(o.cpu().numpy().astype(np.int64), np.asarray(oo).astype(np.int64))
    else:
        env.reset(seed=2)
        env.set_state(s=c.s, elapsed=np.full(c.B, c.kw["time_limit"], np.int32), n_dropoffs=np.zeros(c.B, np.int32))
        env.rng_state = c.info["state"]
        want = ora.step_seeded(c.actions)
        assert want[3].all() and not want[2].any()
        _check_step(_np4(env.step(c.actions)), want, "planted step")
    _check_state(env, ora)  # the start states, no GP_DERR_* flag, the RNG state
    _ordinary_steps(env, ora, 3, seed=row)
    _check_state(env, ora)
