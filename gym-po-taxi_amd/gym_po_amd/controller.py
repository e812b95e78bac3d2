"""Tabular controllers for the closed-loop rollouts (`NativeVecEnv.set_controller` / `rollout_controller`).

A controller is a finite-state machine with M nodes (M = 1: a memoryless policy). In node n, seeing the scalar obs o,
it draws the joint choice (action a, next node n') from `probs[n, o, a, n']`. The device evaluates it with integers
only: one Philox4x32-10 block per env-step, counter (env, step_lo, step_hi, TAG_CTRL) under the env's own key, gives
y = x0 >> 1 (31 bits); the choice is j = #{i : y >= thr[n, o, i]} with j = a * M + n', where `thr` is the table built
here: the row's cumulative probabilities scaled to 2^31. Pure numpy: nothing here touches the GPU.
"""
import numpy as np

TAG_CTRL = 0x67706F63  # 4th counter word of the controller's draw (the env's own draws carry 0x67706f21)
MAX_NODES = 8
TOP = 1 << 31


def controller_thresholds(probs):
    """float probs [M, n_obs, A, M] (or [n_obs, A] for M = 1) -> uint32 thresholds [M, n_obs, A * M].

    Entry j = a * M + n' of a row is T_j = floor(C_j * 2^31), C the float64 sequential cumulative sum of the row,
    and T_j = 2^31 from the row's last nonzero entry onward, so that every row ends at exactly 2^31 and a choice of
    probability zero has an empty interval [T_{j-1}, T_j) and is never drawn. Raises ValueError for negative (or
    NaN) entries and for rows whose sum is off 1 by more than 1e-6."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim == 2:
        p = p[None, :, :, None]
    if p.ndim != 4 or p.shape[0] != p.shape[3]:
        raise ValueError(f"probs must be [M, n_obs, A, M] (or [n_obs, A] for M = 1), got shape {np.shape(probs)}")
    M, n_obs, A, _ = p.shape
    if not 1 <= M <= MAX_NODES:
        raise ValueError(f"a controller has 1 to {MAX_NODES} nodes, got {M}")
    if n_obs < 1 or A < 1:
        raise ValueError(f"probs needs at least one obs and one action, got shape {p.shape}")
    if not np.all(p >= 0):  # (NaN fails the comparison too)
        raise ValueError("probs has negative (or NaN) entries")
    rows = np.ascontiguousarray(p).reshape(M, n_obs, A * M)  # j = a * M + n'
    off = np.abs(rows.sum(-1) - 1.0)
    if not np.all(off <= 1e-6):
        n, o = np.unravel_index(int(np.argmax(off)), off.shape)
        raise ValueError(f"probs row (node {n}, obs {o}) sums to {rows[n, o].sum()!r}, not 1")
    c = np.cumsum(rows, axis=-1)  # sequential float64 adds, in index order
    t = np.minimum(np.floor(c * float(TOP)), float(TOP)).astype(np.uint64)
    L = A * M
    last = (L - 1) - np.argmax(rows[..., ::-1] > 0, axis=-1)  # the last nonzero entry of each row
    t[np.arange(L) >= last[..., None]] = TOP
    return t.astype(np.uint32)


STATS_SCALE_BITS = 20  # ret_q of NativeVecEnv.controller_statistics counts returns in units of 2^-20


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def stats_returns(ret_q):
    """int64 fixed-point return sums `ret_q` of `NativeVecEnv.controller_statistics` -> float64 sums (x 2^-20; exact
    below 2^53 units)."""
    return _host(ret_q).astype(np.float64) * 2.0 ** -STATS_SCALE_BITS


def q_estimate(counts, ret_q):
    """The mean return-to-go per table cell [..., M, n_obs, A, M + 1] (the Monte Carlo estimate of the value of
    making that choice), NaN where a cell was never visited."""
    c = _host(counts).astype(np.float64)
    s = stats_returns(ret_q)
    return np.divide(s, c, out=np.full(s.shape, np.nan), where=c > 0)


def policy_gradient(probs, counts, ret_q):
    """The unnormalised likelihood-ratio gradient sum over visits of G * d log pi / d logits, with respect to the
    per-row joint softmax logits z[n, o, a, n'] (pi[n, o] = softmax of z[n, o] over the A * M joint choices).

    probs float [M, n_obs, A, M] (or [n_obs, A] for M = 1), counts / ret_q int64 [M, n_obs, A, M + 1] from
    `NativeVecEnv.controller_statistics`; all three may carry a leading population axis P. With S =
    stats_returns(ret_q), C = S[..., :M] (visits whose next node is known), E = S[..., M] (visits that ended the
    episode, scored by the action marginal pi_a = sum over n' of pi), and sums over a row's (a, n'):

        grad[n, o, a, n'] = C[n, o, a, n'] - pi[n, o, a, n'] * sum C[n, o]
                            + E[n, o, a] * pi[n, o, a, n'] / pi_a[n, o, a] - pi[n, o, a, n'] * sum E[n, o]

    the third term being 0 where pi_a is 0. Returns float64 shaped like probs. `counts` fixes the shape only (divide
    by counts.sum() for a per-visit mean)."""
    p = np.asarray(probs, dtype=np.float64)
    s = stats_returns(ret_q)
    flat = p.ndim == s.ndim - 2  # [n_obs, A] (or [P, n_obs, A]) for M = 1
    if flat:
        p = p[..., None, :, :, None]
    if p.ndim not in (4, 5) or p.shape[-1] != p.shape[-4] or s.shape != p.shape[:-1] + (p.shape[-1] + 1,) \
            or np.shape(_host(counts)) != s.shape:
        raise ValueError(f"probs {np.shape(probs)} must be [(P,) M, n_obs, A, M] and counts / ret_q [(P,) M, n_obs, A, "
                         f"M + 1], got {np.shape(_host(counts))} / {s.shape}")
    M = p.shape[-1]
    C, E = s[..., :M], s[..., M]
    pa = p.sum(-1)
    ratio = np.divide(p, pa[..., None], out=np.zeros_like(p), where=pa[..., None] > 0)
    sum_c = C.sum((-1, -2))[..., None, None]
    sum_e = E.sum(-1)[..., None, None]
    g = C - p * sum_c + E[..., None] * ratio - p * sum_e
    return g[..., 0, :, :, 0] if flat else g


def population_thresholds(probs):
    """float probs [P, M, n_obs, A, M], P controllers of one shape -> uint32 thresholds [P, M, n_obs, A * M] for
    `NativeVecEnv.set_controller_population`: `controller_thresholds` applied to each controller. Raises ValueError
    as it does, the message naming the controller first."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 5 or p.shape[0] < 1:
        raise ValueError(f"probs must be [P, M, n_obs, A, M] with P >= 1, got shape {np.shape(probs)}")
    out = []
    for c in range(p.shape[0]):
        try:
            out.append(controller_thresholds(p[c]))
        except ValueError as e:
            raise ValueError(f"controller {c}: {e}") from None
    return np.stack(out)
