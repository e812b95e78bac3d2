"""CPU tests of the controller statistics' host side: the numpy restatement (tests/controller_stats_oracle.py) on a
stream small enough to compute by hand, the pure-numpy consumers in gym_po_amd.controller (stats_returns, q_estimate,
policy_gradient) against a brute-force per-visit sum, and the presence of the C entry point. No GPU compute."""
import ctypes
import os
import re

import numpy as np
import pytest

from controller_stats_oracle import SCALE, controller_stats, returns_to_go
from gym_po_amd.controller import policy_gradient, q_estimate, stats_returns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_hand_computed_stream():
    """2 envs, 3 steps, M = 2, n_obs = 3, A = 2, gamma = 0.5, every value dyadic.
    env 0: no step ends; bootstrap 8.   G_2 = 1 + 0.5 * 8 = 5, G_1 = -2 + 2.5 = 0.5, G_0 = 0.25 + 0.25 = 0.5
    env 1: step 1 terminates; bootstrap 4. G_2 = 3 + 2 = 5, G_1 = -1 (ended), G_0 = 2 - 0.5 = 1.5"""
    planes = dict(obs=np.array([[1, 2], [2, 0], [0, 1]]), actions=np.array([[0, 1], [1, 0], [1, 1]]),
                  nodes=np.array([[0, 0], [1, 1], [0, 0]], dtype=np.uint8),
                  rew=np.array([[0.25, 2.0], [-2.0, -1.0], [1.0, 3.0]], dtype=np.float32),
                  term=np.array([[0, 0], [0, 1], [0, 0]], dtype=bool), trunc=np.zeros((3, 2), dtype=bool))
    obs0, next_nodes, boot = np.array([0, 1]), np.array([1, 0], dtype=np.uint8), np.array([8.0, 4.0], dtype=np.float32)
    G = returns_to_go(planes["rew"], planes["term"], planes["trunc"], 0.5, boot)
    assert np.array_equal(G, np.array([[0.5, 1.5], [0.5, -1.0], [5.0, 5.0]], dtype=np.float32))
    counts, ret_q, flagged = controller_stats(2, 3, 2, obs0, planes, next_nodes, 0.5, boot)
    assert not flagged and counts.shape == (2, 3, 2, 3)
    # (node, obs before, action, next node or 2 = ended) -> G
    want = {(0, 0, 0, 1): 0.5, (1, 1, 1, 0): 0.5, (0, 2, 1, 1): 5.0,   # env 0: steps 0, 1, 2
            (0, 1, 1, 1): 1.5, (1, 2, 0, 2): -1.0, (0, 0, 1, 0): 5.0}  # env 1: step 1 ended -> column M = 2
    wc, wq = np.zeros_like(counts), np.zeros_like(ret_q)
    for cell, g in want.items():
        wc[cell] += 1
        wq[cell] += int(g * SCALE)
    assert np.array_equal(counts, wc) and np.array_equal(ret_q, wq)
    assert np.array_equal(stats_returns(ret_q), wq / SCALE)


def test_oracle_skips_bad_visits_and_adds_into():
    planes = dict(obs=np.zeros((2, 3), dtype=np.int32), actions=np.array([[0, 5, 0], [0, 0, 0]]),
                  nodes=np.zeros((2, 3), dtype=np.uint8), rew=np.array([[1, 1, 1], [1, 1, np.inf]], dtype=np.float32),
                  term=np.zeros((2, 3), dtype=bool), trunc=np.zeros((2, 3), dtype=bool))
    c, q, flagged = controller_stats(1, 1, 2, np.zeros(3, dtype=np.int32), planes, np.zeros(3, dtype=np.uint8))
    assert flagged
    assert c.sum() == 3 and c[0, 0, 0, 0] == 3  # env 1's action 5 and both of env 2's infinite returns are absent
    assert q[0, 0, 0, 0] == int((2 + 1 + 1) * SCALE)  # env 0: G = 2, 1; env 1: the G = 1 of its good step
    c2, q2, _ = controller_stats(1, 1, 2, np.zeros(3, dtype=np.int32), planes, np.zeros(3, dtype=np.uint8),
                                 counts=c.copy(), ret_q=q.copy())
    assert np.array_equal(c2, 2 * c) and np.array_equal(q2, 2 * q)


def brute_force_gradient(probs, visits):
    """sum over visits of G * d log pi(choice) / d z[n, o], z the joint softmax logits of row (n, o): for a visit with
    a known next node the choice is (a, n'); for one that ended the episode it is the action alone (its marginal)."""
    M, n_obs, A, _ = probs.shape
    grad = np.zeros_like(probs)
    for n, o, a, nx, g in visits:
        pi = probs[n, o]
        if nx < M:
            d = -pi.copy()
            d[a, nx] += 1.0
        else:
            pa = pi[a].sum()
            d = -pi.copy()
            d[a] += pi[a] / pa
        grad[n, o] += g * d
    return grad


@pytest.mark.parametrize("M,n_obs,A", [(1, 3, 4), (2, 3, 2), (3, 2, 5)])
def test_policy_gradient_against_brute_force(M, n_obs, A):
    rng = np.random.default_rng(M * 100 + A)
    probs = rng.random((M, n_obs, A, M)) + 0.05
    probs /= probs.sum((-1, -2), keepdims=True)
    K, B = 9, 7
    planes = dict(obs=rng.integers(0, n_obs, (K, B)), actions=rng.integers(0, A, (K, B)),
                  nodes=rng.integers(0, M, (K, B)).astype(np.uint8),
                  rew=rng.integers(-8, 9, (K, B)).astype(np.float32) / 4,
                  term=rng.random((K, B)) < 0.2, trunc=rng.random((K, B)) < 0.1)
    obs0, nn = rng.integers(0, n_obs, B), rng.integers(0, M, B).astype(np.uint8)
    counts, ret_q, flagged = controller_stats(M, n_obs, A, obs0, planes, nn, 0.5)
    assert not flagged
    # the same float64 terms as the table holds: each visit's G rounded to 2^-20 (exact here: dyadic rewards)
    G = returns_to_go(planes["rew"], planes["term"], planes["trunc"], 0.5)
    ended = planes["term"] | planes["trunc"]
    visits = []
    for k in range(K):
        for e in range(B):
            o = obs0[e] if k == 0 else planes["obs"][k - 1, e]
            nx = M if ended[k, e] else (planes["nodes"][k + 1, e] if k + 1 < K else nn[e])
            visits.append((planes["nodes"][k, e], o, planes["actions"][k, e], nx,
                           float(np.rint(float(G[k, e]) * SCALE) / SCALE)))
    want = brute_force_gradient(probs, visits)
    got = policy_gradient(probs, counts, ret_q)
    assert got.shape == probs.shape
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # a leading population axis: each controller on its own
    got2 = policy_gradient(np.stack([probs, probs]), np.stack([counts, 2 * counts]), np.stack([ret_q, 2 * ret_q]))
    np.testing.assert_allclose(got2[0], got, rtol=1e-13, atol=1e-12 * np.abs(want).max())
    np.testing.assert_allclose(got2[1], 2 * got, rtol=1e-13, atol=1e-12 * np.abs(want).max())


def test_policy_gradient_memoryless_reduction():
    """M = 1: both columns collapse to S[a] - pi[a] * sum S, S the return sum of action a wherever the visit led."""
    rng = np.random.default_rng(3)
    n_obs, A = 4, 3
    pi = rng.random((n_obs, A)) + 0.1
    pi /= pi.sum(-1, keepdims=True)
    ret_q = rng.integers(-2 ** 30, 2 ** 30, (1, n_obs, A, 2))
    counts = np.ones_like(ret_q)
    S = stats_returns(ret_q).sum(-1)[0]
    want = S - pi * S.sum(-1, keepdims=True)
    got = policy_gradient(pi, counts, ret_q)
    assert got.shape == (n_obs, A)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(policy_gradient(pi[None, :, :, None], counts, ret_q)[0, :, :, 0], want, rtol=1e-12,
                               atol=1e-9)
    np.testing.assert_allclose(got.sum(-1), 0, atol=1e-6)  # a softmax gradient sums to 0 over a row


def test_policy_gradient_zero_marginal_and_shapes():
    probs = np.zeros((1, 1, 2, 1))
    probs[0, 0, 0, 0] = 1.0
    ret_q = np.zeros((1, 1, 2, 2), dtype=np.int64)
    ret_q[0, 0, 0, 1] = 1 << 20  # one ended visit of action 0, G = 1
    g = policy_gradient(probs, np.ones_like(ret_q), ret_q)
    assert np.array_equal(g, np.zeros_like(probs))  # 1 * pi / pi_a - pi * 1 = 0; action 1: 0 / 0 -> 0
    with pytest.raises(ValueError):
        policy_gradient(np.ones((2, 3, 4, 2)), np.ones((2, 3, 4, 2)), np.ones((2, 3, 4, 2)))


def test_q_estimate_nan_on_empty_cells():
    counts = np.array([[[[2, 0]]]])
    ret_q = np.array([[[[3 << 20, 0]]]])
    q = q_estimate(counts, ret_q)
    assert q.shape == counts.shape and q[0, 0, 0, 0] == 1.5 and np.isnan(q[0, 0, 0, 1])
    assert stats_returns(np.array([-(1 << 19)]))[0] == -0.5


def test_symbol_and_signature_present():
    from gym_po_amd import _lib as L
    assert hasattr(L.lib(), "gp_controller_stats")
    res, args = L.SIGNATURES["gp_controller_stats"]
    assert res is ctypes.c_int and len(args) == 15 and args[11] is ctypes.c_float
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gym_po_amd.h")).read(), flags=re.S)
    decl = re.search(r"int\s+gp_controller_stats\s*\(([^)]*)\)", src).group(1)
    assert len(decl.split(",")) == 15 and "float gamma" in decl and "int64_t* counts" in decl
    assert L.lib().gp_abi_version() == 1
