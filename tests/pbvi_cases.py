"""TEST INFRASTRUCTURE — the inputs and the CPU pipeline shared by tests/test_pbvi_cpu.py and tests/test_pbvi_gpu.py
(DESIGN.md §6s): the models, the special points and vectors of the parity tests, and the detour-maze demonstration run
entirely on the numpy restatements (pomdp_oracle, belief_oracle, pbvi_oracle), so that the CPU run predicts the GPU
run exactly. Everything is made once and left unchanged.
"""
import numpy as np

import belief_oracle as bo
import pbvi_oracle as po
from oracle.philox import philox_key
from pomdp_oracle import TIGER, PomdpOracle, Spec, random_model

F = np.float32
MODELS = {"tiger": None, "m5": (5, 2, 3), "m37": (37, 3, 21), "m300": (300, 2, 70)}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def tables(name):
    """(T, Z, R, start, terminal, reset_obs): those of tests/test_pomdp_gpu.py."""
    def make():
        if name == "tiger":
            from gym_po_amd import parse_pomdp
            m = parse_pomdp(TIGER)
            return (m["T"], m["Z"], m["R"].astype(np.float32), m["start"], np.zeros(2, dtype=bool), np.full((2, 2), 0.5))
        S, A, O = MODELS[name]
        return random_model(S, A, O, seed=S, n_terminal=max(1, S // 8))
    return cached(("tables", name), make)


def spec(name, time_limit=7):
    def make():
        from gym_po_amd import row_thresholds
        T, Z, R, start, terminal, reset_obs = tables(name)
        return Spec(row_thresholds(T), row_thresholds(Z), row_thresholds(start), row_thresholds(reset_obs), R, terminal,
                    time_limit)
    return cached(("spec", name, time_limit), make)


def model(name):
    return cached(("model", name), lambda: po.Model(spec(name)))


def special_inputs(name, P, N, seed=0):
    """Points [P, S] and vectors [N, S] with the cases the rule has to get right: one-hot, sparse and unnormalised
    points (a one-hot point makes some obs impossible where Z has zeros); mixed-sign vectors; for N >= 6 two exact
    duplicates (4 of 1, N - 1 of 0) and a vector (3) that equals vector 1 except in the last state, which ties with it
    wherever the last state carries no weight (it is terminal in the random models)."""
    md = model(name)
    S = md.S
    rng = np.random.default_rng(1000 * seed + 31 * P + N + S)
    b = rng.random((P, S)) * (rng.random((P, S)) > 0.5)
    b[np.arange(P), rng.integers(0, S, P)] += 0.1
    b = b / b.sum(-1, keepdims=True)
    b[0] = 0.0
    b[0, 0] = 1.0  # one-hot
    if P > 1:
        b[1] = 0.0
        b[1, S - 1] = 1.0  # (on (5,2,3): obs 2 has probability zero from here under action 0)
    b[2::5] *= 3.0  # unnormalised
    alpha = rng.normal(size=(N, S)) * 4.0
    if N >= 6:
        alpha[4] = alpha[1]
        alpha[N - 1] = alpha[0]
        alpha[3] = alpha[1]
        alpha[3, S - 1] += 1.0
    return b.astype(F), alpha.astype(F)


def reference(name, P, N, gamma=0.95):
    """The oracle's backup of special_inputs(name, P, N): computed once, shared."""
    def make():
        b, al = special_inputs(name, P, N)
        return b, al, po.backup(model(name), b, al, gamma)
    return cached(("ref", name, P, N, gamma), make)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


# ------------------------------------------------------------------ the detour maze ----
DETOUR = ("L.R", "#.#", "#S#", "#.#", "#P#")  # start in the middle, the areas at the top, the priest below: a detour
DETOUR_TL, DETOUR_GAMMA, DETOUR_SWEEPS = 30, 0.95, 25
DETOUR_B, DETOUR_K, DETOUR_SEED = 2048, 40, 5
EVAL_K, EVAL_SEED = 64, 9


def detour_spec(obs_type):
    """The detour maze lowered by the product's heaven_hell_pomdp (p = 0, default rewards), as integer tables."""
    def make():
        from gym_po_amd import heaven_hell_pomdp, row_thresholds
        from test_pomdp_cpu import hh_stand_in
        env = hh_stand_in(DETOUR, obs_type, 0.0, dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=0.0,
                                                       wall_reward=0.0))
        T, Z, R, start, terminal, reset_obs = heaven_hell_pomdp(env)
        return Spec(row_thresholds(T), row_thresholds(Z), row_thresholds(start), row_thresholds(reset_obs), R, terminal,
                    DETOUR_TL)
    return cached(("detour", obs_type), make)


def detour_plane():
    """The fixed uniform action plane the beliefs are collected under."""
    return cached("plane", lambda: np.random.default_rng(DETOUR_SEED).integers(0, 4, (DETOUR_K, DETOUR_B)).astype(
        np.int32))


def collect_on_oracle(sp, plane, seed):
    """gym_po_amd.belief.collect_beliefs on the numpy env and the numpy filter: the same seed and plane give the
    device's beliefs bit for bit."""
    from gym_po_amd.belief import distinct_rows
    lw = bo.Laws(sp)
    key = philox_key(seed)
    ora = PomdpOracle(plane.shape[1], sp)
    b, bad = bo.reset_beliefs(lw, ora.reset(ora.philox_draws(0, key)))
    assert not bad.any()
    seen = []
    for k in range(plane.shape[0]):
        seen.append(distinct_rows(b))
        o, _, tm, tr = ora.step(plane[k], ora.philox_draws(1 + k, key))
        b, bad = bo.filter_step(lw, b, plane[k], o, tm | tr)
        assert not bad.any()
    return distinct_rows(np.concatenate(seen))


def closed_loop_on_oracle(sp, alpha, vec_action, B, K, seed):
    """K closed-loop steps of B numpy envs under the alpha-vector policy from reset(seed). -> dict(episodes,
    terminated, truncated, returns: the return of every finished episode in order of finishing)."""
    lw = bo.Laws(sp)
    key = philox_key(seed)
    ora = PomdpOracle(B, sp)
    b, _ = bo.reset_beliefs(lw, ora.reset(ora.philox_draws(0, key)))
    run = np.zeros(B, dtype=np.float64)
    returns, n_term, n_trunc = [], 0, 0
    for k in range(K):
        a = bo.policy(alpha, vec_action, b)[0]
        o, r, tm, tr = ora.step(a, ora.philox_draws(1 + k, key))
        run += r
        fin = tm | tr
        returns.append(run[fin].copy())
        run[fin] = 0.0
        n_term += int(tm.sum())
        n_trunc += int((tr & ~tm).sum())
        b, bad = bo.filter_step(lw, b, a, o, fin)
        assert not bad.any()
    returns = np.concatenate(returns)
    return dict(episodes=len(returns), terminated=n_term, truncated=n_trunc, returns=returns)


def detour_pipeline(obs_type):
    """The demonstration on the CPU: collect under the plane, 25 sweeps of pbvi on the oracle's backup, the closed loop
    under the result and under the QMDP vectors. Made once."""
    def make():
        from gym_po_amd.belief import pbvi, qmdp_vectors
        sp = detour_spec(obs_type)
        md = po.Model(sp)
        points = collect_on_oracle(sp, detour_plane(), DETOUR_SEED)
        alpha, actions, values = pbvi(md, points, DETOUR_GAMMA, DETOUR_SWEEPS,
                                      backup=lambda p, a, g: po.backup(md, p, a, g))
        l64 = bo.Laws64(sp)
        qmdp = qmdp_vectors(l64.Tf, sp.reward.astype(np.float64), sp.terminal, DETOUR_GAMMA, 1000)
        return dict(sp=sp, md=md, points=points, alpha=alpha, actions=actions, values=values, qmdp=qmdp,
                    run_pbvi=closed_loop_on_oracle(sp, alpha, actions, DETOUR_B, EVAL_K, EVAL_SEED),
                    run_qmdp=closed_loop_on_oracle(sp, qmdp.astype(F), np.arange(4), DETOUR_B, EVAL_K, EVAL_SEED))
    return cached(("pipeline", obs_type), make)
