"""The index obs of grid Ant-Tag on the CPU: the pure-numpy helpers of gym_po_amd.envs (ant_tag_obs_index,
ant_tag_obs_vector) against the independent statement of the law in tests/anttag_index_oracle.py, over every
(ant cell, target cell) pair of arenas 2, 3, 10 and 16."""
import numpy as np
import pytest

from anttag_index_oracle import IndexObs, index_obs
from gym_po_amd.envs import ant_tag_obs_index, ant_tag_obs_vector
from oracle.anttag import AntTagOracle

SIZES = [2, 3, 10, 16]


def every_pair(size, visible_radius2=9):
    nc = size * size
    ant, tgt = (x.ravel() for x in np.meshgrid(np.arange(nc), np.arange(nc), indexing="ij"))
    ora = AntTagOracle(ant.size, size=size, visible_radius2=visible_radius2, min_start_dist2=0)
    ora.ant[:], ora.target[:] = ant, tgt
    return ora


@pytest.mark.parametrize("size", SIZES)
def test_helper_equals_the_wrapper_and_inverts(size):
    nc = size * size
    ora = every_pair(size)
    vec, idx = ora.obs(), index_obs(ora)
    assert idx.dtype == np.int32 and idx.shape == (nc * nc,)
    got = ant_tag_obs_index(vec, size)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, idx)
    back = ant_tag_obs_vector(idx, size)
    assert back.dtype == np.int32
    np.testing.assert_array_equal(back, vec)
    # a bijection between the vectors that occur and the indices that occur
    assert len(np.unique(idx)) == len(np.unique(vec, axis=0))
    assert idx.min() >= 0 and idx.max() < nc * (nc + 1)
    hidden = vec[:, 2] < 0
    assert (hidden == (vec[:, 3] < 0)).all()
    np.testing.assert_array_equal(idx[hidden] % (nc + 1), nc)  # hidden targets all map to nc
    assert (idx[~hidden] % (nc + 1) < nc).all()
    np.testing.assert_array_equal(idx // (nc + 1), ora.ant)
    if size >= 4:
        assert hidden.any() and (~hidden).any()
    else:
        assert not hidden.any()  # no two cells of a 2 x 2 or 3 x 3 arena are 3 apart


@pytest.mark.parametrize("size", SIZES)
def test_largest_value(size):
    nc = size * size
    # the last ant cell with the target hidden (visible_radius2 = 0 hides it everywhere, its own cell included)
    ora = every_pair(size, visible_radius2=0)
    idx = index_obs(ora)
    assert idx.max() == nc * (nc + 1) - 1
    np.testing.assert_array_equal(ant_tag_obs_index(ora.obs(), size), idx)
    np.testing.assert_array_equal(idx % (nc + 1), nc)
    # every target visible: the largest is the last ant cell seeing the target on the last cell
    ora = every_pair(size, visible_radius2=10 ** 6)
    assert index_obs(ora).max() == nc * (nc + 1) - 2
    np.testing.assert_array_equal(ant_tag_obs_index(ora.obs(), size), index_obs(ora))


def test_helpers_keep_leading_shapes():
    ora = every_pair(10)
    vec = ora.obs().reshape(100, 100, 4)
    idx = ant_tag_obs_index(vec, 10)
    assert idx.shape == (100, 100)
    assert ant_tag_obs_vector(idx, 10).shape == (100, 100, 4)
    np.testing.assert_array_equal(ant_tag_obs_vector(idx, 10), vec)


def test_wrapper_steps_as_the_oracle_does():
    """The wrapper's reset / step change nothing but the obs."""
    B = 257
    rng = np.random.default_rng(0)
    a, b = AntTagOracle(B, size=6, min_start_dist2=9, time_limit=7), AntTagOracle(B, size=6, min_start_dist2=9,
                                                                                 time_limit=7)
    w = IndexObs(b)

    def draws():
        return dict(choose=rng.integers(0, 4, B), ant=rng.integers(0, 36, B), tgt=rng.integers(0, 30, B))

    dr = draws()
    np.testing.assert_array_equal(w.reset(dr), ant_tag_obs_index(a.reset(dr), 6))
    for _ in range(30):
        act, dr = rng.integers(0, 5, B), draws()
        o, r, d, t = a.step(act, dr)
        wo, wr, wd, wt = w.step(act, dr)
        np.testing.assert_array_equal(wo, ant_tag_obs_index(o, 6))
        np.testing.assert_array_equal(wr, r)
        np.testing.assert_array_equal(wd, d)
        np.testing.assert_array_equal(wt, t)
        np.testing.assert_array_equal(a.ant, b.ant)
        np.testing.assert_array_equal(a.target, b.target)
        np.testing.assert_array_equal(a.elapsed, b.elapsed)
