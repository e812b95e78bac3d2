"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of gp_controller_stats (include/gym_po_amd.h, controller
statistics): per controller table cell (node, obs, action, next node) the visit count and the fixed-point sum of the
float32 returns-to-go that followed the choice, over K stored closed-loop steps.

The backward loop runs in np.float32 with two roundings per step (a product, then a sum: numpy never fuses them), the
fixed point is np.rint(G.astype(float64) * 2**20) (G * 2^20 is exact in float64, rint rounds to nearest even as the
device's conversion does), and np.add.at accumulates into int64. A visit outside the table, or with |G| not below
2^31 (NaN and infinity included), is skipped and reported through the "flagged" bool; the G chain goes on through it.
"""
import numpy as np

SCALE = 2.0 ** 20


def returns_to_go(rew, term, trunc, gamma, bootstrap=None):
    """G [K, B] float32: G_k = rew_k where the step ended the episode, else fl32(rew_k + fl32(gamma * G_{k+1})), with
    G_K = bootstrap (or 0)."""
    rew = np.asarray(rew, dtype=np.float32)
    K, B = rew.shape
    ended = np.asarray(term, dtype=bool) | np.asarray(trunc, dtype=bool)
    g = np.zeros(B, dtype=np.float32) if bootstrap is None else np.asarray(bootstrap, dtype=np.float32).copy()
    gam = np.float32(gamma)
    G = np.empty((K, B), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(K - 1, -1, -1):
            prod = (gam * g).astype(np.float32)          # first rounding
            g = np.where(ended[k], rew[k], (rew[k] + prod).astype(np.float32))  # second rounding
            G[k] = g
    return G


def controller_stats(M, n_obs, A, obs0, planes, next_nodes, gamma=1.0, bootstrap=None, P=1, G_envs=None,
                     counts=None, ret_q=None):
    """planes: dict of numpy arrays obs / actions / nodes / rew / term / trunc [K, B]. Returns (counts, ret_q,
    flagged): int64 [P, M, n_obs, A, M + 1] (the leading axis dropped for P = 1 without G_envs), added into `counts` /
    `ret_q` if given."""
    obs = np.asarray(planes["obs"], dtype=np.int64)
    K, B = obs.shape
    act = np.asarray(planes["actions"], dtype=np.int64)
    nodes = np.asarray(planes["nodes"], dtype=np.int64)
    ended = np.asarray(planes["term"], dtype=bool) | np.asarray(planes["trunc"], dtype=bool)
    single = G_envs is None
    shape = (P, M, n_obs, A, M + 1)
    if counts is None:
        counts = np.zeros(shape[1:] if single else shape, dtype=np.int64)
        ret_q = np.zeros(shape[1:] if single else shape, dtype=np.int64)
    c5, q5 = counts.reshape(shape), ret_q.reshape(shape)
    flagged = False
    if K == 0:
        return counts, ret_q, flagged
    G = returns_to_go(planes["rew"], planes["term"], planes["trunc"], gamma, bootstrap)
    before = np.concatenate([np.asarray(obs0, dtype=np.int64)[None], obs[:-1]], axis=0)    # the obs conditioning step k
    after = np.concatenate([nodes[1:], np.asarray(next_nodes, dtype=np.int64)[None]], axis=0)  # the node after step k
    p = np.zeros(B, dtype=np.int64) if single else np.arange(B, dtype=np.int64) // int(G_envs)
    with np.errstate(all="ignore"):
        ok = ((nodes >= 0) & (nodes < M) & (before >= 0) & (before < n_obs) & (act >= 0) & (act < A)
              & (ended | (after < M)) & (np.abs(G) < np.float32(2.0 ** 31)))
    flagged = bool((~ok).any())
    last = np.where(ended, M, after)
    k_idx, e_idx = np.nonzero(ok)
    cell = (p[e_idx], nodes[k_idx, e_idx], before[k_idx, e_idx], act[k_idx, e_idx], last[k_idx, e_idx])
    q = np.rint(G[k_idx, e_idx].astype(np.float64) * SCALE).astype(np.int64)
    np.add.at(c5, cell, 1)
    np.add.at(q5, cell, q)
    return counts, ret_q, flagged
