"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the per-controller scores of a controller population
(include/gym_po_amd.h, controller populations; gp_controller_scores).

The env and the controllers are not restated here: the rew / term / trunc planes a run emitted go in with the elapsed
count every env had before the first step, the group size G and the discount gamma; the five counters per group come
out. Env e belongs to group e // G. The discount weight of an env is gamma^elapsed by sequential float32 products
(W[0] = 1, W[t] = fl32(W[t-1] * gamma)): W[elapsed] before the first step, then 1 after a step that ended the episode,
else fl32(w * gamma). A discounted term is the float32 product fl32(w * rew); the sums are float64.
"""
import math

import numpy as np

FIELDS = ("episodes", "return_sum", "length_sum", "env_steps", "discounted_return_sum")
W_ENTRIES = 65536


def weight_table(gamma, n=W_ENTRIES):
    """W[0] = 1, W[t] = fl32(W[t-1] * gamma) for t < n, gamma taken as float32."""
    g = np.float32(gamma)
    W = np.empty(n, dtype=np.float32)
    w = np.float32(1.0)
    for t in range(n):
        W[t] = w
        w = np.float32(w * g)
    return W


def discounted_terms(rew, term, trunc, elapsed0, gamma, W=None):
    """fl32(w * rew) per env-step, float32 [K, B], for rew float32 [K, B], term / trunc [K, B] and elapsed0 [B], the
    elapsed counts before the first step. Also returns the weights w [K, B] each step was taken under."""
    rew = np.asarray(rew, dtype=np.float32)
    done = np.asarray(term, dtype=bool) | np.asarray(trunc, dtype=bool)
    K, B = rew.shape
    g = np.float32(gamma)
    if W is None:
        W = weight_table(gamma, int(np.max(elapsed0, initial=0)) + 1)
    w = W[np.asarray(elapsed0, dtype=np.int64)].astype(np.float32)
    terms = np.empty((K, B), dtype=np.float32)
    weights = np.empty((K, B), dtype=np.float32)
    for k in range(K):
        weights[k] = w
        terms[k] = w * rew[k]  # float32 * float32 -> float32: one rounding
        w = np.where(done[k], np.float32(1.0), (w * g).astype(np.float32)).astype(np.float32)
    return terms, weights


def population_scores(rew, term, trunc, elapsed0, group_envs, gamma, W=None):
    """The five counters per group as a dict of arrays [P] (counts int64, sums float64), and the two bounds of
    gp_controller_scores' own double summation, n * 2^-52 * sum|term| per group, n the group's term count, for
    return_sum and discounted_return_sum (`return_bound`, `discounted_bound`)."""
    rew = np.asarray(rew, dtype=np.float32)
    done = np.asarray(term, dtype=bool) | np.asarray(trunc, dtype=bool)
    K, B = rew.shape
    G = int(group_envs)
    P = -(-B // G)
    terms, _ = discounted_terms(rew, term, trunc, elapsed0, gamma, W)
    # episode lengths: the elapsed count a step reaches, where it ends the episode
    el = np.asarray(elapsed0, dtype=np.int64).copy()
    length = np.zeros((K, B), dtype=np.int64)
    for k in range(K):
        el = el + 1
        length[k] = np.where(done[k], el, 0)
        el = np.where(done[k], 0, el)
    out = {f: np.zeros(P, dtype=np.float64 if f in ("return_sum", "discounted_return_sum") else np.int64)
           for f in FIELDS}
    out["return_bound"] = np.zeros(P)
    out["discounted_bound"] = np.zeros(P)
    for p in range(P):
        sl = slice(p * G, min((p + 1) * G, B))
        n = K * (sl.stop - sl.start)
        out["episodes"][p] = int(done[:, sl].sum())
        out["length_sum"][p] = int(length[:, sl].sum())
        out["env_steps"][p] = n
        out["return_sum"][p] = math.fsum(rew[:, sl].astype(np.float64).ravel())  # correctly rounded
        out["discounted_return_sum"][p] = math.fsum(terms[:, sl].astype(np.float64).ravel())
        out["return_bound"][p] = n * 2.0 ** -52 * np.abs(rew[:, sl].astype(np.float64)).sum()
        out["discounted_bound"][p] = n * 2.0 ** -52 * np.abs(terms[:, sl].astype(np.float64)).sum()
    return out
