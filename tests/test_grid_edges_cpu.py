"""CPU twin of tests/test_grid_edges_gpu.py: the rows at the action-failure thresholds and the planted PCG64 words,
checked against numpy itself (no device)."""
import numpy as np
import pytest

from grid_table_oracle import (EDGE_PS, K_MAX, generator_at, plant_word, planted_words, rng6, threshold_rows,
                               thresholds)
from oracle.gridworld import action_probability_matrix, sample_effective_action


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("p", EDGE_PS)
def test_threshold_rows_and_what_is_dropped(n, p):
    act, k, dropped = threshold_rows(n, p)
    # only k = 2^53 - 1 rows may be dropped, at most n of them
    assert all(x == K_MAX for _, x in dropped) and len(dropped) <= n
    cs = action_probability_matrix(n, p).cumsum(axis=1)
    below = int((cs[:, -1] < 1.0 - 2.0 ** -53).sum())
    assert len(dropped) == below
    assert below == {(8, 0.5): 3, (8, 1.0): 8}.get((n, p), 0)
    # the integer form the device uses, k > floor(cumsum_j * 2^53), is the reference's formula on every row
    t = np.array(thresholds(n, p), dtype=object)
    want = sample_effective_action(action_probability_matrix(n, p)[act], k.astype(np.float64) * 2.0 ** -53)
    got = np.array([sum(int(kk) > tj for tj in t[a]) for a, kk in zip(act, k)])
    np.testing.assert_array_equal(got, want)
    # every threshold below 2^53 - 1 is straddled: k = t and k = t + 1 give different counts
    for a in range(n):
        for j in range(n - 1):
            tj = t[a][j]
            if 0 <= tj < K_MAX:
                e = {int(kk): int(w) for aa, kk, w in zip(act, k, want) if aa == a}
                assert tj + 1 not in e or e[tj + 1] > e[tj], (a, j)  # (k = 2^53 - 1 may be a dropped row)
    assert (k[act > 0] == 0).any() and ((k == K_MAX).sum() == n - len(dropped))
    if p == 0.0:  # u = 0.0 yields action 0 whatever was intended
        assert (want[(k == 0)] == 0).all()


@pytest.mark.parametrize("n,p", [(4, 1.0 / 3), (4, 0.2), (8, 1.0 / 3), (8, 0.2)])
def test_planted_words_straddle_each_threshold_in_numpy(n, p):
    B = 4096
    words = planted_words(n, p)
    assert len(words) == 2 * n * (n - 1)
    m = action_probability_matrix(n, p)
    inc = generator_at(rng6(np.random.PCG64(3).state)).bit_generator.state["state"]["inc"]
    for i, (a, j, w) in enumerate(words):
        pos = (0, 63, 64, B - 1)[i % 4]
        gen = np.random.Generator(np.random.PCG64())
        gen.bit_generator.state = plant_word(inc, pos, w, seed=i)
        u = gen.random(B)
        assert u[pos] == (w >> 11) * 2.0 ** -53
        eff = int(sample_effective_action(m[[a]], u[[pos]])[0])
        lower = (w & 0x7FF) == 0x7FF  # the largest word that must not exceed threshold j
        assert (eff <= j) if lower else (eff >= j + 1), (a, j, hex(w), eff)
        if i % 2:  # the pair differs by one in the 64-bit draw and by one threshold in the count
            assert w == words[i - 1][2] + 1
