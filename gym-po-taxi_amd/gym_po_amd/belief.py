"""Belief-space helpers of the tabular POMDP env: the float32 laws the on-device Bayes filter multiplies (DESIGN.md
§6r), QMDP alpha-vectors, a reader of `pomdp-solve`'s `.alpha` files (pure numpy), and the drivers of the on-device
point-based backup: `collect_beliefs` steps an env and gathers its beliefs, `pbvi` iterates
`TabularPOMDPEnv.point_backup` (or any backup given) over a fixed point set; and the drivers of the on-device
belief-set expansion: `reset_points` are the beliefs an episode starts with, `expand_points` grows a
set by every point's farthest successor (`TabularPOMDPEnv.expand_beliefs`, or any expansion given), `is_closed` says
whether a set holds all its successors, and `pbvi_expanding` alternates `pbvi` and `expand_points` from the reset
beliefs alone. `TabularPOMDPEnv.set_belief_policy` takes the vectors these return.
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


def _host(x):
    """A numpy array of a torch tensor (any device) or of anything numpy takes."""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def distinct_rows(b):
    """The bitwise-distinct rows of float32 `b` [E, S] in lexicographic order of their bit patterns (for rows >= 0:
    of their values), float32 [P, S]. -0 and +0 are different bits."""
    b = np.ascontiguousarray(_host(b), dtype=np.float32)
    if b.ndim != 2:
        raise ValueError(f"rows must be [E, S], got shape {b.shape}")
    return np.unique(b.view(np.uint32), axis=0).view(np.float32)


def collect_beliefs(env, actions, K=None):
    """The beliefs a run of `env` (a TabularPOMDPEnv after reset() and enable_belief()) passes through: the env is
    stepped one step at a time and `env.belief` is gathered before every step. `actions`: an int [K, B] plane, stepped
    by rollout() of one row and belief_filter() (reproducible on the numpy restatements), or the string "policy" with
    `K`: K steps of rollout_belief(1) under the installed policy. Returns the bitwise-distinct rows among the K B
    gathered beliefs, float32 [P, S] (numpy), in the order of `distinct_rows`. The env is left K steps further."""
    seen = []
    if isinstance(actions, str):
        if actions != "policy":
            raise ValueError(f"collect_beliefs: actions must be an int [K, B] plane or 'policy', got {actions!r}")
        if K is None or int(K) < 1:
            raise ValueError("collect_beliefs: 'policy' needs K >= 1")
        for _ in range(int(K)):
            seen.append(distinct_rows(env.belief))
            env.rollout_belief(1, store=())
    else:
        a = _host(actions)
        if a.ndim != 2 or a.shape[1] != env.num_envs or a.dtype.kind not in "iu" or a.shape[0] < 1:
            raise ValueError(f"collect_beliefs: actions must be integers [K, B] = [K, {env.num_envs}] with K >= 1, got "
                             f"{a.dtype} {a.shape}")
        if K is not None and int(K) != a.shape[0]:
            raise ValueError(f"collect_beliefs: K = {K} but the plane has {a.shape[0]} rows")
        a = a.astype(np.int32)
        for k in range(a.shape[0]):
            seen.append(distinct_rows(env.belief))
            o, _, tm, tr = env.rollout(a[k:k + 1])
            env.belief_filter(a[k:k + 1], o, tm, tr)
    return distinct_rows(np.concatenate(seen))


def pbvi(env, points, gamma, sweeps, backup=None):
    """Point-based value iteration (Pineau, Gordon & Thrun 2003) over the fixed belief set `points` [P, S]. Starts from
    the single vector min(0, min reward) / (1 - gamma) in every state (float64, then float32): a lower bound of every
    policy's value, so the value at every point never decreases. Each of the `sweeps` sweeps backs up every point
    against the current set (`backup(points, alpha, gamma)` -> a dict of alpha [P, S], actions [P], value [P]; None:
    `env.point_backup`) and replaces the set by the bitwise-distinct new vectors, keeping the first occurrence in point
    order. Needs 0 <= gamma < 1. Returns (alpha float32 [N, S], actions int64 [N], values float32 [sweeps, P]): the
    first two are what `set_belief_policy` takes."""
    gamma = float(gamma)
    if not 0.0 <= gamma < 1.0:
        raise ValueError(f"pbvi: gamma must be in [0, 1), got {gamma}")
    sweeps = int(sweeps)
    if sweeps < 1:
        raise ValueError(f"pbvi: sweeps must be >= 1, got {sweeps}")
    S = int(env.n_states)
    pts = points if hasattr(points, "detach") else np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != S or pts.shape[0] < 1:
        raise ValueError(f"pbvi: points must be [P, S] = [P, {S}] with P >= 1, got {tuple(pts.shape)}")
    if backup is None:
        backup = env.point_backup
    floor = min(0.0, float(np.min(env.reward))) / (1.0 - gamma)
    alpha = np.full((1, S), floor, dtype=np.float32)
    actions = np.zeros(1, dtype=np.int64)
    values = []
    for _ in range(sweeps):
        out = backup(pts, alpha, gamma)
        new = np.ascontiguousarray(_host(out["alpha"]), dtype=np.float32)
        _, first = np.unique(new.view(np.uint32), axis=0, return_index=True)
        first = np.sort(first)
        alpha, actions = new[first], _host(out["actions"]).astype(np.int64)[first]
        values.append(_host(out["value"]).astype(np.float32))
    return alpha, actions, np.stack(values)


def reset_points(env, prior=None):
    """The beliefs an episode can start with: for every reset obs o the filter's ended rule on the prior,
    u(s) = fl(prior[s] Rf[s][o]), n = sum_s u(s) (sequential, ascending, from +0), b(s) = fl(u(s) / n), in float32 from
    `float_laws(env)` (pure numpy). `prior` None: the env's start law, enable_belief()'s default; an env enabled with
    `enable_belief(prior)` takes the same `prior` here (normalised as there, by `normalise_belief`), else these are not
    the beliefs its filter resets to. An obs with !(n > 0) or n not finite never opens an episode and is left out.
    Returns the `distinct_rows` of the rest, float32 [P, S]: the seed set of `pbvi_expanding` (which uses the start
    law: pass `points=reset_points(env, prior)` for another), and the successors through an episode end that
    `expand_beliefs` leaves out."""
    lw = float_laws(env)
    if prior is not None:
        prior = normalise_belief(prior)
        if prior.shape != lw["prior"].shape:
            raise ValueError(f"prior must be [S] = [{lw['prior'].shape[0]}], got shape {prior.shape}")
        lw["prior"] = prior
    u = (lw["prior"][None, :] * lw["Rf"].T).astype(np.float32)  # [O, S]
    n = np.zeros(u.shape[0], dtype=np.float32)
    for s in range(u.shape[1]):
        n = (n + u[:, s]).astype(np.float32)
    live = (n > 0) & np.isfinite(n)
    return distinct_rows((u[live] / n[live, None]).astype(np.float32))


def _expansion(env, points, expand):
    pts = points if hasattr(points, "detach") else np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != int(env.n_states) or pts.shape[0] < 1:
        raise ValueError(f"points must be [P, S] = [P, {int(env.n_states)}] with P >= 1, got {tuple(pts.shape)}")
    out = (env.expand_beliefs if expand is None else expand)(pts)
    return pts, np.ascontiguousarray(_host(out["succ"]), dtype=np.float32), _host(out["dist"]).astype(np.float32)


def expand_points(env, points, expand=None):
    """One expansion of the belief set `points` [P, S] (Pineau, Gordon & Thrun 2003): every point proposes its
    farthest successor (`expand(points)` -> a dict with succ [P, S] and dist [P]; None: `env.expand_beliefs`, measured
    against the points themselves), the successors with dist > 0 are kept, and the `distinct_rows` of the points and
    the kept successors are returned, float32 (numpy): the set at most doubles."""
    pts, succ, dist = _expansion(env, points, expand)
    return distinct_rows(np.concatenate((np.ascontiguousarray(_host(pts), dtype=np.float32), succ[dist > 0])))


def is_closed(env, points, expand=None):
    """True iff every successor of positive probability of every point of `points` [P, S] that does not pass through an
    episode end is itself a point, bit for bit: one expansion in which every dist is 0. With `reset_points` among the
    points the set is then closed under the filter, which is where point-based value iteration improves monotonically
    (DESIGN.md §6s)."""
    return bool(np.all(_expansion(env, points, expand)[2] == 0))


def pbvi_expanding(env, gamma, rounds, sweeps, points=None, backup=None, expand=None):
    """Point-based value iteration with its belief-set expansion: `rounds` rounds of `pbvi(env, points, gamma, sweeps,
    backup)` (each from pbvi's own start vector, not from the round before's vectors: pbvi keeps its signature, at the
    price of rounds x sweeps backups), with one `expand_points` between two rounds. `points` None: start from
    `reset_points(env)`. Stops early, after the round on it, once an expansion adds no point (the set is closed).
    Returns (alpha, actions, points, values_per_round): the vectors and actions of the last round (what
    `set_belief_policy` takes), the final point set float32 [P, S], and per round the float32 [sweeps, P_round] values
    of pbvi."""
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError(f"pbvi_expanding: rounds must be >= 1, got {rounds}")
    pts = reset_points(env) if points is None else distinct_rows(points)
    if pts.shape[0] < 1:
        raise ValueError("pbvi_expanding: no point to start from")
    values = []
    for r in range(rounds):
        alpha, actions, v = pbvi(env, pts, gamma, sweeps, backup)
        values.append(v)
        if r + 1 == rounds:
            break
        grown = expand_points(env, pts, expand)
        if grown.shape[0] == pts.shape[0]:
            break
        pts = grown
    return alpha, actions, pts, values


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
