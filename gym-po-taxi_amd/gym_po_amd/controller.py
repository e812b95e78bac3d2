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
