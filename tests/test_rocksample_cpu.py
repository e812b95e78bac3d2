"""CPU tests of RockSample's host side: the numpy oracle of the build-defined rules (tests/rocksample_oracle.py)
against its own scalar one-env statement over every transition of three small grids, the sensor table lowered by
`rocksample_sensor_thresholds`, the default layout, and the package export. No GPU is touched."""
import numpy as np
import pytest

from rocksample_oracle import RockSampleOracle, Spec, scalar_step

TOP = 1 << 31
DYADIC = dict(exit_reward=4.0, good_reward=2.0, bad_reward=-2.0, empty_reward=-1.0, check_reward=-0.25,
              step_reward=-0.5, wall_reward=-0.75)


def _layout(H, W, k):
    """k distinct rock cells spread over the grid (the last cell among them when k > 1), an off-centre start."""
    nc = H * W
    cells = sorted({(i * (nc - 1)) // max(k - 1, 1) for i in range(k)}) if k > 1 else [0]
    assert len(cells) == k
    return [(c // W, c % W) for c in cells], ((H - 1) // 2, W // 3)


@pytest.mark.parametrize("H,W,k", [(1, 1, 1), (2, 3, 2), (4, 4, 4)])
@pytest.mark.parametrize("obs_type", ["cell_sensor", "sensor"])
def test_vectorised_oracle_equals_the_scalar_statement(H, W, k, obs_type):
    from gym_po_amd import rocksample_sensor_thresholds
    rocks, init_pos = _layout(H, W, k)
    thr = rocksample_sensor_thresholds((H, W), rocks, 1.5)
    tl = 7
    sp = Spec((H, W), rocks, init_pos, thr, obs_type, tl, **DYADIC)
    A = 5 + k
    cell, mask, act, el, cor = (x.ravel() for x in np.meshgrid(np.arange(H * W), np.arange(1 << k),
                                                               np.arange(-A, A), np.array([0, tl - 1]),
                                                               np.arange(2), indexing="ij"))
    B = cell.size
    i = np.clip(np.where(act < 0, act + A, act) - 5, 0, k - 1)
    t = thr[cell, i].astype(np.int64)
    y = np.where(cor == 1, t - 1, np.minimum(t, TOP - 1))  # a draw just below / at the threshold of the checked rock
    reset_mask = np.random.default_rng(H * W + k).integers(0, 1 << 32, B)  # the whole word: the oracle keeps k bits
    ora = RockSampleOracle(B, sp)
    ora.agent[:], ora.mask[:], ora.elapsed[:] = cell, mask, el
    o, r, d, tr = ora.step(act, dict(y=y, mask=reset_mask & ((1 << k) - 1)))
    assert r.dtype == np.float32 and o.dtype == np.int32
    seen = set()
    for b in range(B):
        want = scalar_step(sp, int(cell[b]), int(mask[b]), int(el[b]), int(act[b]), int(y[b]), int(reset_mask[b]))
        got = (int(ora.agent[b]), int(ora.mask[b]), int(ora.elapsed[b]), int(o[b]), r[b], bool(d[b]), bool(tr[b]))
        assert got == want, (b, cell[b], mask[b], el[b], act[b], cor[b], got, want)
        seen.add((float(r[b]), bool(d[b]), bool(tr[b])))
    # every reward of the config and both flags occurred
    assert {x[0] for x in seen} >= ({4.0, 2.0, -2.0, -0.25} | ({-1.0, -0.5, -0.75} if H * W > 1 else {-0.75}))
    assert d.any() and tr.any() and not tr.all()
    if obs_type == "sensor":
        assert set(np.unique(o)) == {0, 1, 2}


def test_sensor_thresholds():
    from gym_po_amd import rocksample_sensor_thresholds
    from gym_po_amd.envs.rocksample import DEFAULT_ROCKS
    t = rocksample_sensor_thresholds((5, 5), DEFAULT_ROCKS, 20.0)
    assert t.shape == (25, 5) and t.dtype == np.uint32
    for i, (y, x) in enumerate(DEFAULT_ROCKS):
        assert t[y * 5 + x, i] == TOP  # a check on the rock's own cell is always right
    # p = 0.5 * (1 + 2^-1) = 0.75 exactly at distance d0
    t = rocksample_sensor_thresholds((1, 4), ((0, 0),), 3.0)
    assert int(t[3, 0]) == 3 * (1 << 29) and int(t[0, 0]) == TOP
    # nonincreasing in distance, never below 1/2
    H, W, rock = 16, 16, (3, 11)
    t = rocksample_sensor_thresholds((H, W), (rock,), 2.0)[:, 0].astype(np.int64)
    yy, xx = np.divmod(np.arange(H * W), W)
    d2 = (yy - rock[0]) ** 2 + (xx - rock[1]) ** 2
    order = np.argsort(d2, kind="stable")
    assert (np.diff(t[order]) <= 0).all() and (t >= 1 << 30).all() and (t <= TOP).all()
    assert len(np.unique(t)) > 20  # (not a constant table)
    for a, b in zip(*np.nonzero(d2[:, None] == d2[None, :])):
        assert t[a] == t[b]  # equal distance, equal threshold


def test_default_layout_and_rocks_required_elsewhere():
    from gym_po_amd import RockSample
    from gym_po_amd.envs.rocksample import DEFAULT_ROCKS, resolve_rocks
    assert DEFAULT_ROCKS == ((0, 2), (2, 0), (2, 3), (3, 4), (4, 1))
    assert resolve_rocks((5, 5), None) == DEFAULT_ROCKS
    assert resolve_rocks((7, 7), [(1, 2), (3, 4)]) == ((1, 2), (3, 4))
    with pytest.raises(ValueError, match="rocks must be given"):
        resolve_rocks((7, 7), None)
    with pytest.raises(ValueError, match="rocks must be given"):  # raised before anything touches the GPU
        RockSample(4, map_size=(7, 7))
    with pytest.raises(ValueError, match="obs_type"):
        RockSample(4, obs_type="hansen")


def test_exported():
    import gym_po_amd
    assert "RockSample" in gym_po_amd.__all__ and "rocksample_sensor_thresholds" in gym_po_amd.__all__
    assert gym_po_amd.RockSample.__name__ == "RockSample"
    from gym_po_amd import _lib
    assert _lib.GP_KIND_ROCKSAMPLE == 6
