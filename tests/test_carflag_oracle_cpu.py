"""The NumPy restatement of Car-Flag (tests/carflag_oracle.py) against the fixtures recorded from the reference
(tests/golden/carflag_*.npz): every output bit for bit from the seed, the final PCG64 state, and the frames."""
import numpy as np
import pytest

from carflag_oracle import (CASE_NAMES, CarFlagOracle, NumpyDraws, ReplayDraws, final_rng_state, frame, load_case,
                            load_index, load_render, make_actions)
from fixtures import digest


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if digest(a) != digest(b) or not np.array_equal(a, b):  # the digest takes f32 by its bits
        bad = np.argwhere((a != b) if a.dtype != np.float32 else (a.view(np.uint32) != b.view(np.uint32)))
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}")


def test_index_lists_every_case():
    _, idx = load_index()
    assert set(CASE_NAMES) <= set(idx["cases"])
    for name in CASE_NAMES:
        ev = idx["cases"][name]["events"]
        assert all(v > 0 for v in ev.values()), (name, ev)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_reproduces_fixture_from_seed(name):
    meta, d = load_case(name)
    gen = np.random.default_rng(meta["seed"])
    ora = CarFlagOracle(meta["num_envs"], meta["time_limit"], meta.get("num_actions"), NumpyDraws(gen))
    acts = make_actions(meta)
    assert str(digest(acts)) == meta["digest"]["actions"]
    _same(ora.reset(), d["obs0"], "reset obs")
    k53, hidx, pidx = d["k53"], d["hidx"], d["pidx"]
    out = []
    for t in range(meta["steps"]):
        out.append(ora.step(acts[t]))
        m = ora.last_reset
        if m.any():
            k, h, p = ora.draws.last
            assert np.array_equal(k53[t + 1][m], k) and np.array_equal(hidx[t + 1][m], h), t
            assert np.array_equal(pidx[t + 1][m], p), t
    for i, key in enumerate(("obs", "rew", "term", "trunc")):
        _same(np.stack([o[i] for o in out]), d[key], key)
    _same(ora.s, d["final_s"], "final s")
    _same(ora.heavens, d["final_heavens"], "final heavens")
    _same(ora.priests, d["final_priests"], "final priests")
    _same(ora.elapsed, d["final_elapsed"], "final elapsed")
    assert gen.bit_generator.state == final_rng_state(meta)
    for key in ("obs", "rew", "term", "trunc"):
        assert str(digest(d[key])) == meta["digest"][key]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_replay_of_recorded_draws(name):
    meta, d = load_case(name)
    dr = ReplayDraws()
    ora = CarFlagOracle(meta["num_envs"], meta["time_limit"], meta.get("num_actions"), dr)
    acts = make_actions(meta)
    dr.set(d["k53"][0], d["hidx"][0], d["pidx"][0])
    _same(ora.reset(), d["obs0"], "reset obs")
    out = []
    for t in range(meta["steps"]):
        dr.set(d["k53"][t + 1], d["hidx"][t + 1], d["pidx"][t + 1])
        out.append(ora.step(acts[t]))
    for i, key in enumerate(("obs", "rew", "term", "trunc")):
        _same(np.stack([o[i] for o in out]), d[key], key)


def test_f32_and_f64_fixtures_differ():
    (_, a), (_, b) = load_case("carflag_f32_b64"), load_case("carflag_f64_b64")
    assert (a["obs"].view(np.uint32) != b["obs"].view(np.uint32)).sum() > 1000


def test_frames_match_recorded():
    d = load_render()
    shown = 0
    for i in range(len(d["frames"])):
        img = frame(d["s0"][i], d["heavens"][i], d["priests"][i])
        assert img.dtype == np.uint8 and img.shape == (48, 600, 3)
        np.testing.assert_array_equal(img, d["frames"][i], err_msg=f"frame {i}")
        shown += int(d["s0"][i][2] != 0)
    assert 0 < shown < len(d["frames"])


def test_product_frame_matches_recorded():
    """The product's host-side frame builder (CarVecEnv.frame; no GPU needed)."""
    from gym_po_amd.envs.car_flag import CarVecEnv
    d = load_render()
    for i in range(len(d["frames"])):
        np.testing.assert_array_equal(CarVecEnv.frame(d["s0"][i], d["heavens"][i], d["priests"][i]), d["frames"][i])
