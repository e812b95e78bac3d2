"""Belief-space helpers of the tabular POMDP env (pure numpy, nothing here touches the device): the float32 laws the
on-device Bayes filter multiplies, QMDP alpha-vectors, and a reader of `pomdp-solve`'s `.alpha` files.
`TabularPOMDPEnv.set_belief_policy` takes the vectors these return.
"""
import numpy as np

TOP = 1 << 31


def threshold_law(thr):
    """Threshold rows (last axis) -> float32 laws by the filter's rule: p[i] = (float32)(thr[i] - thr[i-1]) * 2^-31
    with thr[-1] = 0: one round-to-nearest conversion, then an exact scale."""
    t = np.asarray(thr).astype(np.int64)
    return np.diff(t, axis=-1, prepend=0).astype(np.float32) * np.float32(2.0 ** -31)


def float_laws(env):
    """The float32 tables the filter of `env` (a TabularPOMDPEnv, or anything with its integer tables as attributes)
    works with: a dict of Tf [S, A, S] (s, a, s'), Zf [A, S, O] (a, s', o), Rf [S, O] (the reset obs law) and prior [S]
    (the start law), each from the integer thresholds by `threshold_law`."""
    return {"Tf": threshold_law(env.trans_thr), "Zf": threshold_law(env.obs_thr),
            "Rf": threshold_law(env.reset_obs_thr), "prior": threshold_law(env.start_thr)}


def normalise_belief(b):
    """Rows of `b` (last axis) divided by their sum, in float32 with the sum taken sequentially in ascending index
    from +0 (the filter's own rule). Raises ValueError for entries that are negative or not finite and for a row whose
    sum is not positive."""
    b = np.array(b, dtype=np.float32, ndmin=1)
    if not np.all(np.isfinite(b)) or not np.all(b >= 0):
        raise ValueError("belief entries must be finite and >= 0")
    n = np.zeros(b.shape[:-1], dtype=np.float32)
    for s in range(b.shape[-1]):
        n = (n + b[..., s]).astype(np.float32)
    if not (np.all(n > 0) and np.all(np.isfinite(n))):
        raise ValueError("a belief row must have a positive finite sum")
    return (np.abs(b) / n[..., None]).astype(np.float32)  # (abs: a -0 entry becomes +0)


def qmdp_vectors(T, R, terminal=None, gamma=0.95, iters=1000):
    """QMDP (Littman, Cassandra & Kaelbling 1995): float64 value iteration on the underlying MDP,
        Q(s, a) = sum_s' T[s, a, s'] (R[s, a, s'] + gamma * [s' not terminal] * max_a' Q(s', a')),
    `iters` sweeps from Q = 0. T [S, A, S]; R [S, A] or [S, A, S]; terminal bool [S] (None: none). Returns
    alpha [A, S] float64 with alpha[a, s] = Q(s, a): one vector per action, vector a belonging to action a."""
    T = np.asarray(T, dtype=np.float64)
    S, A, _ = T.shape
    R = np.asarray(R, dtype=np.float64)
    if R.shape == (S, A):
        R = np.broadcast_to(R[:, :, None], (S, A, S))
    if T.shape != (S, A, S) or R.shape != (S, A, S):
        raise ValueError(f"T must be [S, A, S] and R [S, A] or [S, A, S], got {T.shape} and {R.shape}")
    live = np.ones(S) if terminal is None else 1.0 - np.asarray(terminal).astype(bool).astype(np.float64)
    if live.shape != (S,):
        raise ValueError(f"terminal must be [S] = [{S}]")
    if not 0.0 <= gamma <= 1.0:
        raise ValueError(f"gamma must be in [0, 1], got {gamma}")
    r = (T * R).sum(-1)
    Q = np.zeros((S, A))
    for _ in range(int(iters)):
        Q = r + gamma * (T @ (live * Q.max(-1)))
    return np.ascontiguousarray(Q.T)


def parse_alpha(text, S):
    """`pomdp-solve`'s `.alpha` text: per vector one line with the action's index, then S coefficients (on one line or
    spread over several); blank lines and `#` comments are skipped. Returns (alpha float64 [N, S], actions int64 [N]).
    Anything else (an action that is no non-negative integer, a coefficient that is no finite number, too many or too
    few coefficients, no vector at all) raises ValueError naming the line."""
    S = int(S)
    if S < 1:
        raise ValueError(f"S must be >= 1, got {S}")
    vectors, actions = [], []
    cur, cur_line = None, 0  # the coefficients of the vector being read, and the line of its action
    for n, raw in enumerate(text.splitlines(), 1):
        toks = raw.split("#", 1)[0].split()
        if not toks:
            continue
        if cur is None:
            if len(toks) != 1:
                raise ValueError(f"line {n}: expected an action index alone on the line, got {' '.join(toks)!r}")
            try:
                a = int(toks[0])
            except ValueError:
                raise ValueError(f"line {n}: the action {toks[0]!r} is not an integer") from None
            if a < 0:
                raise ValueError(f"line {n}: the action {a} is negative")
            actions.append(a)
            cur, cur_line = [], n
            continue
        for tok in toks:
            try:
                v = float(tok)
            except ValueError:
                raise ValueError(f"line {n}: the coefficient {tok!r} is not a number") from None
            if not np.isfinite(v):
                raise ValueError(f"line {n}: the coefficient {tok!r} is not finite")
            cur.append(v)
        if len(cur) > S:
            raise ValueError(f"line {n}: {len(cur)} coefficients for the vector of line {cur_line}, expected {S}")
        if len(cur) == S:
            vectors.append(cur)
            cur = None
    if cur is not None:
        raise ValueError(f"line {cur_line}: the vector has {len(cur)} coefficients at the end of the text, expected {S}")
    if not vectors:
        raise ValueError("line 1: no vector in the text")
    return np.asarray(vectors, dtype=np.float64), np.asarray(actions, dtype=np.int64)
