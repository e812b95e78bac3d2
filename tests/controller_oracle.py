"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the closed-loop rollouts' controller alone.

The env itself is not restated here: the obs stream a run emitted (and its terminated / truncated flags) go in, the
actions and nodes the controller must have chosen come out. Per env-step (include/gym_po_amd.h, closed-loop
rollouts): one Philox4x32-10 block with counter (env, step_lo, step_hi, TAG_CTRL) under the env's key, y = x0 >> 1,
j = #{i : y >= thr[node, obs, i]}, action = j // M, and after the step node = j % M, or 0 where the step ended the
episode. The obs conditioning step k is the obs the env is in before it: the reset obs for k = 0, else obs[k - 1].
"""
import numpy as np

from oracle.philox import philox4x32_10

TAG_CTRL = 0x67706F63


def choose(y, rows):
    """j = #{i : y >= rows[..., i]} for y [...] (31-bit) and threshold rows [..., L]."""
    return (np.asarray(y, dtype=np.int64)[..., None] >= np.asarray(rows, dtype=np.int64)).sum(-1)


def controller_draws(B, step, key):
    """y = x0 >> 1 of the controller's block of global step `step`, for env 0..B-1."""
    env = np.arange(B, dtype=np.uint64)
    x0 = philox4x32_10(env, step & 0xFFFFFFFF, step >> 32, TAG_CTRL, *key)[0]
    return (x0 >> np.uint32(1)).astype(np.int64)


def controller_rollout(obs0, obs, term, trunc, thr, key, step0, nodes0=None):
    """obs0 [B]: the obs before the first step; obs / term / trunc [K, B]: what the K steps emitted; thr uint32
    [M, n_obs, L]; key = philox_key(seed); step0: the global step index of the first step; nodes0 [B] (default 0).
    Returns (actions int32 [K, B], nodes uint8 [K, B], final nodes uint8 [B])."""
    obs = np.asarray(obs, dtype=np.int64)
    K, B = obs.shape
    M = thr.shape[0]
    node = np.zeros(B, dtype=np.int64) if nodes0 is None else np.asarray(nodes0, dtype=np.int64).copy()
    o = np.asarray(obs0, dtype=np.int64)
    done = np.asarray(term, dtype=bool) | np.asarray(trunc, dtype=bool)
    actions = np.empty((K, B), dtype=np.int32)
    nodes = np.empty((K, B), dtype=np.uint8)
    for k in range(K):
        j = choose(controller_draws(B, int(step0) + k, key), thr[node, o])
        actions[k] = j // M
        nodes[k] = node
        node = np.where(done[k], 0, j % M)
        o = obs[k]
    return actions, nodes, node.astype(np.uint8)
