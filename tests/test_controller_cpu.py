"""CPU tests of the closed-loop rollouts' host side: the threshold tables `controller_thresholds` builds and the
choice rule of the numpy restatement (tests/controller_oracle.py). No GPU."""
import numpy as np
import pytest

from controller_oracle import TAG_CTRL, choose
from gym_po_amd.controller import TAG_CTRL as PKG_TAG_CTRL
from gym_po_amd.controller import controller_thresholds

TOP = 1 << 31


def test_tag_is_distinct_from_the_env_draws():
    assert PKG_TAG_CTRL == TAG_CTRL == 0x67706F63
    assert TAG_CTRL != 0x67706F21


def test_deterministic_row_gives_all_mass_to_one_choice():
    M, n_obs, A = 2, 3, 4
    p = np.zeros((M, n_obs, A, M))
    p[:, :, 2, 1] = 1.0  # action 2, next node 1: j = 2 * M + 1 = 5
    t = controller_thresholds(p)
    assert t.dtype == np.uint32 and t.shape == (M, n_obs, A * M)
    row = t[1, 2].astype(np.int64)
    assert list(row) == [0] * 5 + [TOP] * 3
    widths = np.diff(np.concatenate(([0], row)))
    assert list(widths) == [0] * 5 + [TOP] + [0] * 2  # every other interval is empty
    for y in (0, 1, TOP // 2, TOP - 1):
        assert choose(y, row) == 5


def test_tables_are_monotone_and_end_at_2_31():
    rng = np.random.default_rng(0)
    p = rng.random((3, 7, 8, 3)) ** 3 * (rng.random((3, 7, 8, 3)) > 0.4)
    p[..., 0, 0] += 1e-3
    p /= p.sum((-1, -2), keepdims=True)
    t = controller_thresholds(p).astype(np.int64)
    assert np.all(np.diff(t, axis=-1) >= 0)
    assert np.all(t <= TOP) and np.all(t[..., -1] == TOP)
    # zero-probability choices have empty intervals, and the thresholds are floor(cumsum * 2^31) below the forced tail
    rows = p.reshape(3, 7, 24)
    widths = np.diff(np.concatenate((np.zeros((3, 7, 1), dtype=np.int64), t), -1), axis=-1)
    assert np.all(widths[rows == 0] == 0)
    want = np.floor(np.cumsum(rows, -1) * float(TOP)).astype(np.int64)
    last = 23 - np.argmax(rows[..., ::-1] > 0, -1)
    below = np.arange(24) < last[..., None]
    assert np.array_equal(t[below], want[below])
    assert np.all(t[~below] == TOP)


def test_memoryless_shorthand():
    p = np.array([[0.25, 0.25, 0.5, 0.0], [0.0, 1.0, 0.0, 0.0]])
    t = controller_thresholds(p)
    assert t.shape == (1, 2, 4)
    assert np.array_equal(t, controller_thresholds(p[None, :, :, None]))
    assert list(t[0, 0]) == [TOP // 4, TOP // 2, TOP, TOP]
    assert list(t[0, 1]) == [0, TOP, TOP, TOP]


@pytest.mark.parametrize("bad", [
    np.array([[0.5, 0.6, -0.1, 0.0]]),          # a negative entry
    np.array([[0.5, 0.25, 0.25, 1e-5]]),        # sums to 1 + 1e-5
    np.array([[0.5, 0.25, 0.25 - 1e-5, 0.0]]),  # sums to 1 - 1e-5
    np.array([[0.0, 0.0, 0.0, 0.0]]),
    np.array([[0.5, np.nan, 0.5, 0.0]]),
    np.ones((2, 3, 4, 3)) / 12,                 # node axes disagree
    np.ones((9, 1, 4, 9)) / 36,                 # more than 8 nodes
])
def test_bad_rows_raise(bad):
    with pytest.raises(ValueError):
        controller_thresholds(bad)


def test_row_sum_tolerance_is_1e_6():
    t = controller_thresholds(np.array([[0.5, 0.25, 0.25 + 5e-7, 0.0]]))  # off by 5e-7: accepted
    assert t[0, 0, -1] == TOP and t[0, 0, 2] == TOP


def test_choice_changes_exactly_at_the_thresholds():
    """Over all 2^31 values of y the choice of a 3-entry row changes exactly at T_i: y = T_i - 1 and y = T_i."""
    t = controller_thresholds(np.array([[0.3, 0.45, 0.25]]))[0, 0].astype(np.int64)
    assert t[0] == int(np.floor(0.3 * TOP)) and t[1] == int(np.floor((0.3 + 0.45) * TOP)) and t[2] == TOP
    assert choose(0, t) == 0
    for i in range(2):
        assert choose(t[i] - 1, t) == i
        assert choose(t[i], t) == i + 1
    assert choose(TOP - 1, t) == 2  # the largest y: j <= L - 1 always
    # and piecewise constant in between (sampled)
    ys = np.random.default_rng(1).integers(0, TOP, 10000)
    assert np.array_equal(choose(ys, np.broadcast_to(t, (10000, 3))), np.searchsorted(t, ys, side="right"))
