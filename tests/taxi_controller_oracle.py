"""Test helper of test_taxi_controller_cpu.py / test_taxi_controller_gpu.py: the stochastic, goal-directed policy the
directed closed-loop case runs on the Hansen Taxi, built from the Taxi oracle (oracle/taxi.py) alone.

A Hansen obs does not tell the taxi's cell, only the walls around it, so the greedy pickup -> dropoff policy over
states (taxi_table_oracle.greedy_policy) is no function of the obs. Its marginal over the states behind each obs is:

    probs[obs, a]  ~  #{s < ns : obs_of[s] == obs and greedy[s] == a}        over all ns states,

with a uniform row for the obs values no state maps to. The controller's own actions and nodes are checked with the
env-agnostic tests/controller_oracle.py.
"""
import functools

import numpy as np

from taxi_table_oracle import greedy_policy, make_oracle, set_rows

A = 5


def obs_table(kw):
    """(obs_of [ns], n_obs): the oracle's obs of every state."""
    ns = make_oracle(kw, 1).ns
    ora = make_oracle(kw, ns)
    set_rows(ora, np.arange(ns), np.zeros(ns), np.zeros(ns))
    return np.asarray(ora.obs()).astype(np.int64), int(ora.no)


def _freeze(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _marginal(frozen):
    kw = dict(frozen)
    obs_of, n_obs = obs_table(kw)
    greedy = greedy_policy(kw)
    counts = np.zeros((n_obs, A))
    np.add.at(counts, (obs_of, greedy), 1.0)
    empty = counts.sum(1) == 0
    counts[empty] = 1.0
    return counts / counts.sum(1, keepdims=True)


def marginal_greedy_probs(kw):
    """float64 [n_obs, 5]: the memoryless policy above (rows sum to 1 up to rounding)."""
    return _marginal(_freeze(kw)).copy()


def policy_rollout_sampled(kw, B, seed, K, probs, policy_seed):
    """The oracle on numpy's own stream from `seed` for K steps, its actions sampled from `probs[obs]` with a numpy
    Generator of `policy_seed` (inverse CDF of one uniform per env-step): the stacked (obs, rew, term, trunc)."""
    ora = make_oracle(kw, B)
    obs = np.asarray(ora.reset_seed(seed))
    gen = np.random.default_rng(policy_seed)
    cdf = np.cumsum(probs, -1)
    outs = []
    for _ in range(K):
        a = np.minimum((gen.random(B)[:, None] >= cdf[obs]).sum(-1), A - 1)
        o, r, d, tr = ora.step_seeded(a)
        obs = np.asarray(o)
        outs.append((obs, r, d, tr))
    return ora, [np.stack(x) for x in zip(*outs)]
