"""CPU tests of the controller populations' host side: `population_thresholds`, the two C symbols and their ctypes
bindings, and the numpy restatement of the per-controller scores (tests/population_oracle.py) on a stream small enough
to check by hand. Nothing here touches the GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_po_amd.controller import controller_thresholds, population_thresholds
from population_oracle import FIELDS, discounted_terms, population_scores, weight_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gym_po_amd.h")


def random_probs(M, n_obs, A, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, rng.integers(A), rng.integers(M)] += 1e-2
    return p / p.sum((-1, -2), keepdims=True)


def test_population_thresholds_is_controller_thresholds_per_controller():
    P, M, n_obs, A = 3, 2, 7, 4
    probs = np.stack([random_probs(M, n_obs, A, seed=20 + p) for p in range(P)])
    t = population_thresholds(probs)
    assert t.dtype == np.uint32 and t.shape == (P, M, n_obs, A * M)
    for p in range(P):
        assert np.array_equal(t[p], controller_thresholds(probs[p]))
    assert not np.array_equal(t[0], t[1])
    # 2-D / 4-D input keeps its meaning: a single controller, not a population
    assert controller_thresholds(probs[0]).shape == (M, n_obs, A * M)
    with pytest.raises(ValueError):
        population_thresholds(probs[0])


def test_population_thresholds_names_the_controller_of_a_bad_row():
    P, M, n_obs, A = 3, 2, 5, 4
    probs = np.stack([random_probs(M, n_obs, A, seed=30 + p) for p in range(P)])
    probs[2, 1, 3] *= 0.5  # controller 2, node 1, obs 3 sums to 0.5
    with pytest.raises(ValueError, match=r"controller 2: .*node 1, obs 3"):
        population_thresholds(probs)
    probs = np.stack([random_probs(M, n_obs, A, seed=30 + p) for p in range(P)])
    probs[1, 0, 0, 0, 0] = -0.1
    with pytest.raises(ValueError, match="controller 1"):
        population_thresholds(probs)


def test_header_declares_and_lib_binds_both_symbols():
    from gym_po_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("gp_set_controller_population", "gp_controller_scores"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    res, args = L.SIGNATURES["gp_set_controller_population"]
    assert res is ctypes.c_int and args[2] is ctypes.c_int64 and args[5] is ctypes.c_float and len(args) == 7
    res, args = L.SIGNATURES["gp_controller_scores"]
    assert res is ctypes.c_int and args[1] == ctypes.POINTER(ctypes.c_double) and len(args) == 4
    assert L.lib().gp_abi_version() == 1  # additive: the version stays


def test_weight_table_is_the_sequential_float32_product():
    g = np.float32(0.95)
    W = weight_table(0.95, 32)
    assert W.dtype == np.float32 and W[0] == np.float32(1.0) and W[1] == g
    assert W[2] == np.float32(g * g)
    w = np.float32(1.0)
    for _ in range(20):
        w = np.float32(w * g)
    assert W[20] == w
    # not the correctly rounded power: the sequential products drift from it by a few ulps
    assert abs(float(W[20]) - float(g) ** 20) <= 20 * 2.0 ** -24 * float(g) ** 20
    assert np.array_equal(weight_table(1.0, 8), np.ones(8, dtype=np.float32))
    assert len(weight_table(0.5, 70000)) == 70000 and weight_table(0.5)[-1] == 0.0  # 65,536 entries; underflows to 0


def test_oracle_on_a_hand_checked_stream():
    """2 groups of 2 envs, 6 steps, gamma = 0.5 (every product exact, so the expected values are plain arithmetic)."""
    #          env0   env1   env2   env3
    rew = np.array([[1.0, 0.0, 2.0, -1.0],
                    [1.0, 0.0, 2.0, -1.0],
                    [1.0, 4.0, 2.0, -1.0],
                    [1.0, 0.0, 2.0, -1.0],
                    [1.0, 0.0, 2.0, -1.0],
                    [1.0, 8.0, 2.0, -1.0]], dtype=np.float32)
    term = np.zeros((6, 4), dtype=bool)
    trunc = np.zeros((6, 4), dtype=bool)
    term[2, 1] = True   # env1 ends its first episode at step 2 (length 3), its second runs on
    term[5, 1] = True   # ... and ends at step 5 (length 3)
    trunc[1, 2] = True  # env2 started at elapsed 3: the episode ends at step 1 with length 5
    elapsed0 = np.array([0, 0, 3, 1])
    terms, w = discounted_terms(rew, term, trunc, elapsed0, 0.5)
    assert terms.dtype == np.float32
    assert np.array_equal(w[:, 0], 0.5 ** np.arange(6))
    assert np.array_equal(w[:, 1], [1, 0.5, 0.25, 1, 0.5, 0.25])
    assert np.array_equal(w[:, 2], [0.125, 0.0625, 1, 0.5, 0.25, 0.125])
    assert np.array_equal(w[:, 3], 0.5 ** np.arange(1, 7))
    s = population_scores(rew, term, trunc, elapsed0, group_envs=2, gamma=0.5)
    assert list(s["episodes"]) == [2, 1]
    assert list(s["length_sum"]) == [6, 5]
    assert list(s["env_steps"]) == [12, 12]
    assert list(s["return_sum"]) == [6.0 + 12.0, 12.0 - 6.0]
    d0 = (1 + 0.5 + 0.25 + 0.125 + 0.0625 + 0.03125) + (0.25 * 4 + 0.25 * 8)
    d2 = 2 * (0.125 + 0.0625 + 1 + 0.5 + 0.25 + 0.125)
    d3 = -(0.5 + 0.25 + 0.125 + 0.0625 + 0.03125 + 0.015625)
    assert list(s["discounted_return_sum"]) == [d0, d2 + d3]
    assert s["episodes"].dtype == np.int64 and s["return_sum"].dtype == np.float64
    assert all(f in s for f in FIELDS)
    # the summation bound: n * 2^-52 * sum|term|
    assert s["return_bound"][1] == 12 * 2.0 ** -52 * 18.0
    # gamma = 1: the discounted sum is the return; a short last group
    s1 = population_scores(rew[:, :3], term[:, :3], trunc[:, :3], elapsed0[:3], group_envs=2, gamma=1.0)
    assert np.array_equal(s1["discounted_return_sum"], s1["return_sum"])
    assert list(s1["env_steps"]) == [12, 6] and list(s1["return_sum"]) == [18.0, 12.0]
