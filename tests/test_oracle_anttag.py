"""CPU checks of the grid Ant-Tag oracle (oracle/anttag.py) against an independent scalar statement of the spec.

`scalar_step` below is written from the prose of the spec (the header of csrc/anttag.hip and DESIGN.md section 6b),
one env at a time, with explicit branches on (y, x) coordinates. The vectorised oracle, which the GPU tests pin the
kernel to, must agree with it on EVERY (ant cell, target cell, action, choose) of an arena, so the rules the random
trajectories of the GPU tests reach rarely or never (contact states, walls and corners for both bodies, the
|vy| == |vx| diagonal, v == 0, a tag on the truncation step) are all compared.
"""
import math

import numpy as np
import pytest

from oracle.anttag import AntTagOracle
from oracle.philox import philox_key


# ---------------------------------------------------------------------------------- the scalar model ----
def admissible_targets(N, min_start_dist2):
    """Per ant cell, the cells farther than sqrt(min_start_dist2) from it, ascending (brute force)."""
    lists = []
    for ant in range(N * N):
        ay, ax = ant // N, ant % N
        lst = []
        for tgt in range(N * N):
            ty, tx = tgt // N, tgt % N
            if (ay - ty) * (ay - ty) + (ax - tx) * (ax - tx) > min_start_dist2:
                lst.append(tgt)
        lists.append(lst)
    return lists


def scalar_obs(N, vis_r2, ant, tgt):
    ay, ax, ty, tx = ant // N, ant % N, tgt // N, tgt % N
    if (ay - ty) ** 2 + (ax - tx) ** 2 < vis_r2:
        return (ay, ax, ty, tx)
    return (ay, ax, -1, -1)


def scalar_step(N, tag_r2, vis_r2, time_limit, tag_reward, step_reward, lists, ant, tgt, elapsed, action, choose,
                reset_ant, reset_k):
    """One env-step. Returns (obs, reward, term, trunc, ant, target, elapsed, notes); `notes` names the corner cases
    the step went through."""
    notes = set()
    ay, ax, ty, tx = ant // N, ant % N, tgt // N, tgt % N
    # the ant: N, E, S, W, stay; a move off the arena leaves it in place
    if action == 0:
        ny, nx = ay - 1, ax
    elif action == 1:
        ny, nx = ay, ax + 1
    elif action == 2:
        ny, nx = ay + 1, ax
    elif action == 3:
        ny, nx = ay, ax - 1
    else:
        ny, nx = ay, ax
    if 0 <= ny < N and 0 <= nx < N:
        ay, ax = ny, nx
    else:
        notes.add("ant_wall")
    # the target, after the ant: away / the two orthogonals / stay, in (y, x) order
    dy, dx = ay - ty, ax - tx
    if choose == 0:
        vy, vx = -dy, -dx
    elif choose == 1:
        vy, vx = -dx, dy
    elif choose == 2:
        vy, vx = dx, -dy
    else:
        vy, vx = 0, 0
    # rounded to one grid step: the dominant axis, the diagonal on a tie, nothing when v = 0
    if vy == 0 and vx == 0:
        sy, sx = 0, 0
        notes.add("v_zero")
    elif abs(vy) > abs(vx):
        sy, sx = (1 if vy > 0 else -1), 0
    elif abs(vx) > abs(vy):
        sy, sx = 0, (1 if vx > 0 else -1)
    else:
        sy, sx = (1 if vy > 0 else -1), (1 if vx > 0 else -1)
        notes.add("tie")
    my, mx = ty + sy, tx + sx
    if 0 <= my < N and 0 <= mx < N:
        ty, tx = my, mx
    else:  # a step leaving the cage is not taken
        notes.add("cage")
    elapsed += 1
    term = (ay - ty) ** 2 + (ax - tx) ** 2 <= tag_r2
    trunc = elapsed >= time_limit
    reward = tag_reward if term else step_reward
    ant, tgt = ay * N + ax, ty * N + tx
    if term and trunc:
        notes.add("term_and_trunc")
    if term or trunc:  # same-step reset from the env's reset draws; an index past the list takes its last cell
        ant = reset_ant
        lst = lists[ant]
        tgt = lst[reset_k] if reset_k < len(lst) else lst[-1]
        elapsed = 0
    return scalar_obs(N, vis_r2, ant, tgt), reward, term, trunc, ant, tgt, elapsed, notes


def _cross_product(nc):
    ant, tgt, act, cho = np.meshgrid(np.arange(nc), np.arange(nc), np.arange(5), np.arange(4), indexing="ij")
    return ant.ravel(), tgt.ravel(), act.ravel(), cho.ravel()


# ---------------------------------------------------------------------------------- exhaustive one step ----
@pytest.mark.parametrize("size,kw", [(5, dict(min_start_dist2=4, time_limit=7)), (10, dict())])
@pytest.mark.parametrize("last_step", [False, True])
def test_oracle_step_matches_scalar_model_exhaustively(size, kw, last_step):
    nc = size * size
    ant, tgt, act, cho = _cross_product(nc)
    B = ant.size
    ora = AntTagOracle(B, size=size, **kw)
    lists = admissible_targets(size, ora.min_r2)
    el0 = ora.time_limit - 1 if last_step else 0
    rng = np.random.default_rng(size + 100 * last_step)
    dr = dict(choose=cho, ant=rng.integers(0, nc, B), tgt=rng.integers(0, nc + 8, B))  # tgt often past the list
    assert (dr["tgt"] >= np.array([len(lists[a]) for a in dr["ant"]])).any()
    ora.ant[:], ora.target[:], ora.elapsed[:] = ant, tgt, el0
    obs, rew, term, trunc = ora.step(act, dr)
    seen = dict(tie=0, v_zero=0, cage=0, ant_wall=0, term_and_trunc=0)
    r_tag, r_step = float(ora.tag_reward), float(ora.step_reward)
    want = [scalar_step(size, ora.tag_r2, ora.vis_r2, ora.time_limit, r_tag, r_step, lists, int(ant[i]), int(tgt[i]),
                        el0, int(act[i]), int(cho[i]), int(dr["ant"][i]), int(dr["tgt"][i])) for i in range(B)]
    for w in want:
        for n in w[7]:
            seen[n] += 1
    np.testing.assert_array_equal(obs, np.array([w[0] for w in want], np.int32))
    np.testing.assert_array_equal(rew, np.array([w[1] for w in want], np.float32))
    np.testing.assert_array_equal(term, np.array([w[2] for w in want]))
    np.testing.assert_array_equal(trunc, np.array([w[3] for w in want]))
    np.testing.assert_array_equal(ora.ant, np.array([w[4] for w in want]))
    np.testing.assert_array_equal(ora.target, np.array([w[5] for w in want]))
    np.testing.assert_array_equal(ora.elapsed, np.array([w[6] for w in want]))
    # the cases a kernel can get wrong are all in the set
    for name in ("tie", "v_zero", "cage", "ant_wall"):
        assert seen[name] > 0, name
    assert (seen["term_and_trunc"] > 0) == last_step
    assert trunc.all() == last_step and term.any() and not term.all()


def test_oracle_wraps_negative_actions_like_numpy_indexing():
    size, nc = 5, 25
    ant, tgt, act, cho = _cross_product(nc)
    a, b = (AntTagOracle(ant.size, size=size, min_start_dist2=4) for _ in range(2))
    dr = dict(choose=cho, ant=ant, tgt=np.zeros_like(ant))
    for o in (a, b):
        o.ant[:], o.target[:] = ant, tgt
    for x, y in zip(a.step(act, dr), b.step(act - 5, dr)):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------------------------- admissible targets ----
@pytest.mark.parametrize("size", range(2, 17))
def test_valid_targets_match_brute_force(size):
    checked = 0
    for md2 in (0, 1, 4, 25, (size - 1) ** 2, 2 * (size - 1) ** 2 - 1):
        lists = admissible_targets(size, md2)
        if min(len(v) for v in lists) == 0:  # the device refuses these (GP_E_INVALID); so does the oracle
            with pytest.raises(ValueError, match="no target cell"):
                AntTagOracle(1, size=size, min_start_dist2=md2)
            continue
        ora = AntTagOracle(1, size=size, min_start_dist2=md2)
        assert [list(v) for v in ora.valid_targets] == lists
        checked += 1
    assert checked >= 2  # md2 = 0 and 1 leave every cell a target at every size


def test_default_distance_needs_size_8():
    for size in range(2, 8):
        with pytest.raises(ValueError, match="no target cell"):
            AntTagOracle(1, size=size)
    AntTagOracle(1, size=8)


# ---------------------------------------------------------------------------------- the reset law ----
def wilson_hilferty(p, df):
    """Wilson-Hilferty cube approximation of the p-quantile of chi-square(df)."""
    lo, hi = -10.0, 10.0  # the standard normal quantile of p, by bisection on erfc
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > 1.0 - p:
            lo = mid
        else:
            hi = mid
    z = 0.5 * (lo + hi)
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi2_quantile(p, df):
    """The p-quantile of chi-square(df): scipy's where scipy is importable, else Wilson-Hilferty."""
    try:
        from scipy.stats import chi2
    except ImportError:
        return wilson_hilferty(p, df)
    return float(chi2.ppf(p, df))


def test_chi2_quantile_forms_agree():
    # the upper 1e-6 quantile at the reset test's degrees of freedom, to 7 digits (tables / scipy.stats.chi2.ppf)
    df, exact = 5043, 5534.859
    assert abs(wilson_hilferty(1 - 1e-6, df) / exact - 1.0) < 1e-4
    assert abs(chi2_quantile(1 - 1e-6, df) / exact - 1.0) < 1e-4


def test_reset_law_uniform_over_admissible_pairs():
    """Reset: the ant uniform over the cells, the target uniform over the ant cell's admissible list. Every draw must
    lie in the list, and the counts of the (ant cell, list index) buckets must pass a chi-square test against the
    uniform expectation B / (ncells * len(list)): one bucket per admissible pair, so
    df = (number of admissible pairs) - 1, at a false-alarm level of 1e-6. (The seed is fixed: the test is
    deterministic; the level says how surprising a failure of a correct law would have been.)"""
    B, N = 1 << 16, 10
    ora = AntTagOracle(B)
    lists = admissible_targets(N, 25)
    ora.reset(ora.philox_draws(0, philox_key(2024)))
    assert ora.ant.min() >= 0 and ora.ant.max() < N * N and (ora.elapsed == 0).all()
    observed, expected = [], []
    for a in range(N * N):
        t = ora.target[ora.ant == a]
        assert np.isin(t, lists[a]).all(), f"ant cell {a}: a target outside its admissible list"
        pos = np.searchsorted(lists[a], t)
        observed.extend(np.bincount(pos, minlength=len(lists[a])).tolist())
        expected.extend([B / (N * N * len(lists[a]))] * len(lists[a]))
    observed, expected = np.array(observed, np.float64), np.array(expected)
    n_pairs = sum(len(v) for v in lists)
    assert observed.size == n_pairs and observed.sum() == B and expected.min() > 5.0
    df = n_pairs - 1
    stat = float(((observed - expected) ** 2 / expected).sum())
    bound = chi2_quantile(1.0 - 1e-6, df)
    assert stat < bound, f"chi-square {stat:.1f} over df={df} exceeds the 1e-6 bound {bound:.1f}"
    # and not suspiciously regular either (a counter used as the draw would give stat ~ 0)
    assert stat > chi2_quantile(1e-6, df)
