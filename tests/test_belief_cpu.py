"""CPU tests of the belief filter's numpy restatement (tests/belief_oracle.py) and of the pure-numpy
helpers in gym_po_amd.belief. No GPU.

The vectorised restatement equals the scalar one-env statement; Tiger by hand; the degenerate rule; the float32 rule
against a float64 Bayes filter from the exact integer law (a bound of 1e-4 whose sole job is to catch a wrong rule: a
wrong rule shows at 1e-1, the measured gap is 1e-7); qmdp_vectors against a brute-force Bellman fixed point; parse_alpha;
symbols and signatures; and the calibration test on the numpy env with its Philox draws, which knows nothing of the
rule text, with three wrong filters that it must reject.
"""
import os
import re

import numpy as np
import pytest

import belief_oracle as bo
from oracle.philox import philox_key
from pomdp_oracle import TIGER, PomdpOracle, Spec, random_model

F = np.float32
MODELS = {"tiger": None, "m5": (5, 2, 3), "m37": (37, 3, 21)}
_SPECS = {}


def spec(name, time_limit=7):
    """The lowered tables of a model (those of tests/test_pomdp_gpu.py): made once, left unchanged."""
    if (name, time_limit) not in _SPECS:
        from gym_po_amd import parse_pomdp, row_thresholds
        if name == "tiger":
            m = parse_pomdp(TIGER)
            T, Z, R, start, terminal, reset_obs = (m["T"], m["Z"], m["R"].astype(np.float32), m["start"],
                                                   np.zeros(2, dtype=bool), np.full((2, 2), 0.5))
        else:
            S, A, O = MODELS[name]
            T, Z, R, start, terminal, reset_obs = random_model(S, A, O, seed=S, n_terminal=max(1, S // 8))
        _SPECS[name, time_limit] = Spec(row_thresholds(T), row_thresholds(Z), row_thresholds(start),
                                        row_thresholds(reset_obs), R, terminal, time_limit)
    return _SPECS[name, time_limit]


def random_beliefs(rng, E, S, zero=0.3):
    b = rng.random((E, S)) * (rng.random((E, S)) > zero)
    b[np.arange(E), rng.integers(0, S, E)] += 0.1
    return (b / b.sum(-1, keepdims=True)).astype(F)


# ------------------------------------------------------------------ the restatement ----
def test_float_laws_rule():
    from gym_po_amd.belief import float_laws, threshold_law
    sp = spec("m37")
    lw = bo.Laws(sp)
    fl = float_laws(sp)
    for name, x in (("Tf", lw.Tf), ("Zf", lw.Zf), ("Rf", lw.Rf), ("prior", lw.prior)):
        assert fl[name].dtype == np.float32 and np.array_equal(fl[name], x), name
    # one rounding of the integer difference, then an exact scale; rows sum to 1 within the roundings
    t = np.array([3, 3, 2 ** 31 - 129, 2 ** 31], dtype=np.uint32)
    want = [F(3) * F(2.0 ** -31), F(0), F(2 ** 31 - 132) * F(2.0 ** -31), F(129) * F(2.0 ** -31)]
    assert threshold_law(t).tolist() == [float(x) for x in want]
    assert np.abs(lw.Tf.astype(np.float64).sum(-1) - 1).max() < 37 * 2.0 ** -24


@pytest.mark.parametrize("name", sorted(MODELS))
def test_vectorised_equals_scalar(name):
    sp = spec(name)
    lw = bo.Laws(sp)
    rng = np.random.default_rng(lw.S)
    E = 64 if lw.S > 8 else 256
    b = random_beliefs(rng, E, lw.S)
    a, o = rng.integers(0, lw.A, E), rng.integers(0, lw.O, E)
    ended = rng.random(E) < 0.4
    got, bad = bo.filter_step(lw, b, a, o, ended)
    n_bad = 0
    for e in range(E):
        want, wbad = bo.scalar_filter_step(lw, b[e], int(a[e]), int(o[e]), bool(ended[e]))
        assert bool(bad[e]) == wbad
        assert np.array_equal(got[e].view(np.uint32), np.asarray(want, dtype=F).view(np.uint32)), e
        n_bad += wbad
    assert ended.any() and not ended.all() and n_bad < E // 2
    alpha = rng.normal(size=(5, lw.S)).astype(F)
    alpha[3] = alpha[1]  # an exact tie: the first wins
    va = rng.integers(0, lw.A, 5)
    act, j, v = bo.policy(alpha, va, got)
    for e in range(E):
        wa, wj, wv = bo.scalar_policy(alpha, va, got[e])
        assert (int(act[e]), int(j[e])) == (wa, wj) and F(v[e]).view(np.uint32) == F(wv).view(np.uint32)
    assert 3 not in set(j.tolist())


def test_tiger_by_hand():
    lw = bo.Laws(spec("tiger"))
    LISTEN, HEAR_LEFT = 0, 0
    b0 = np.array([[0.5, 0.5]], dtype=F)
    b1, bad = bo.filter_step(lw, b0, [LISTEN], [HEAR_LEFT], [False])
    assert not bad.any() and b1[0].tolist() == [float(F(0.85)), float(F(0.15))]
    b2, bad = bo.filter_step(lw, b1, [LISTEN], [HEAR_LEFT], [False])
    assert not bad.any() and abs(float(b2[0, 0]) - 0.85 ** 2 / (0.85 ** 2 + 0.15 ** 2)) < 1e-6
    assert f"{float(b2[0, 0]):.4f}" == "0.9698"
    # opening a door moves the tiger uniformly and tells nothing: back to (0.5, 0.5)
    b3, _ = bo.filter_step(lw, b2, [1], [1], [False])
    assert b3[0].tolist() == [0.5, 0.5]
    # an episode end: the prior times the reset obs law (uniform here)
    b4, _ = bo.filter_step(lw, b2, [LISTEN], [HEAR_LEFT], [True])
    assert b4[0].tolist() == [0.5, 0.5]


def test_degenerate_step_gives_the_prior_and_the_flag():
    """A belief on a state that the obs excludes: n = 0, so b' = prior and the step is flagged."""
    T = np.eye(2)[:, None, :]
    Z = np.eye(2)[None]  # state s shows obs s
    from gym_po_amd import row_thresholds
    sp = Spec(row_thresholds(T), row_thresholds(Z), row_thresholds([0.25, 0.75]), row_thresholds(np.full((2, 2), 0.5)),
              np.zeros((2, 1, 2), dtype=np.float32), np.zeros(2, dtype=bool), 7)
    lw = bo.Laws(sp)
    b = np.array([[1, 0], [1, 0], [0.5, 0.5]], dtype=F)
    got, bad = bo.filter_step(lw, b, [0, 0, 0], [1, 0, 1], [False] * 3)
    assert bad.tolist() == [True, False, False]
    assert got.tolist() == [[0.25, 0.75], [1.0, 0.0], [0.0, 1.0]]
    want, wbad = bo.scalar_filter_step(lw, b[0], 0, 1, False)
    assert wbad and [float(x) for x in want] == [0.25, 0.75]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_float32_rule_against_float64_bayes(name):
    """12 steps of the numpy env under random actions: the float32 beliefs against a float64 Bayes filter from the exact
    integer law. Measured gap at most 1.5e-7; the bound only has to catch a wrong rule."""
    sp = spec(name)
    lw, l64 = bo.Laws(sp), bo.Laws64(sp)
    E, K, key = 4096, 12, philox_key(3)
    ora = PomdpOracle(E, sp)
    rng = np.random.default_rng(1)
    obs = ora.reset(ora.philox_draws(0, key))
    b32, bad = bo.reset_beliefs(lw, obs)
    b64 = bo.filter_step64(l64, b32.astype(np.float64), np.zeros(E, dtype=np.int64), obs, np.ones(E, dtype=bool))
    gap = np.abs(b32 - b64).max()
    for k in range(K):
        a = rng.integers(0, lw.A, E)
        o, _, tm, tr = ora.step(a, ora.philox_draws(1 + k, key))
        b32, bad = bo.filter_step(lw, b32, a, o, tm | tr)
        assert not bad.any()
        b64 = bo.filter_step64(l64, b64, a, o, tm | tr)
        gap = max(gap, np.abs(b32 - b64).max())
    print(f"{name}: max |b32 - b64| over {K} steps of {E} envs = {gap:.3g}")
    assert gap < 1e-4


# ------------------------------------------------------------------ helpers of the package ----
def test_qmdp_vectors_against_brute_force_fixed_point():
    from gym_po_amd import parse_pomdp, qmdp_vectors
    m = parse_pomdp(TIGER)
    T, R, g = m["T"], m["R"], 0.95
    S, A, _ = T.shape
    alpha = qmdp_vectors(T, R, None, g, 2000)
    assert alpha.shape == (A, S) and alpha.dtype == np.float64
    # brute force: V = max_a sum_s' T (R + g V) solved by plain iteration in Python floats
    V = [0.0] * S
    for _ in range(3000):
        V = [max(sum(T[s][a][t] * (R[s][a][t] + g * V[t]) for t in range(S)) for a in range(A)) for s in range(S)]
    for a in range(A):
        for s in range(S):
            q = sum(T[s][a][t] * (R[s][a][t] + g * V[t]) for t in range(S))
            assert abs(alpha[a][s] - q) < 1e-9
    # listening forever is worth -1 / (1 - g) = -20; the right door 10 + g V
    assert abs(alpha[0][0] - (-1 + g * V[0])) < 1e-9 and V[0] > 100
    # a terminal state is worth nothing afterwards
    al = qmdp_vectors(np.array([[[0.0, 1.0]], [[0.0, 1.0]]]), np.array([[1.0], [5.0]]), [False, True], 0.9, 50)
    assert al.tolist() == [[1.0, 5.0]]
    with pytest.raises(ValueError):
        qmdp_vectors(T, R[:, :1], None, g, 1)


def test_parse_alpha():
    from gym_po_amd import parse_alpha
    al, act = parse_alpha("0\n-1.5 2e1\n\n# a comment\n2\n3\n4 # trailing\n", 2)
    assert al.tolist() == [[-1.5, 20.0], [3.0, 4.0]] and act.tolist() == [0, 2]
    assert al.dtype == np.float64 and act.dtype == np.int64
    al, act = parse_alpha("1\n0.5 0.25 0.125", 3)
    assert al.tolist() == [[0.5, 0.25, 0.125]] and act.tolist() == [1]
    for text, line, what in (("0\n1 2 3\n", 2, "3 coefficients"), ("0 1\n1 2\n", 1, "alone"), ("x\n1 2\n", 1, "integer"),
                             ("-1\n1 2\n", 1, "negative"), ("0\n1 nan\n", 2, "finite"), ("0\n1 b\n", 2, "number"),
                             ("0\n1 2\n1\n3\n", 3, "1 coefficients"), ("\n# nothing\n", 1, "no vector"),
                             ("0\n1 2\n1.5\n1 2\n", 3, "integer")):
        with pytest.raises(ValueError, match=f"line {line}: .*{what}"):
            parse_alpha(text, 2)


def test_normalise_belief():
    from gym_po_amd.belief import normalise_belief
    b = normalise_belief([1, 2, 1])
    assert b.dtype == np.float32 and b.tolist() == [0.25, 0.5, 0.25]
    for bad in ([1, -1, 1], [0, 0, 0], [1, np.nan, 0], [np.inf, 1, 0]):
        with pytest.raises(ValueError):
            normalise_belief(bad)


def test_symbols_and_signatures():
    import gym_po_amd
    from gym_po_amd import TabularPOMDPEnv, _lib
    names = ("gp_belief_enable", "gp_belief_disable", "gp_belief_get", "gp_belief_set", "gp_belief_filter",
             "gp_set_belief_policy", "gp_rollout_belief")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gym_po_amd.h")).read()
    L = _lib.lib()
    for n in names:
        assert re.search(rf"\bint {n}\(", header), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    assert len(_lib.SIGNATURES["gp_rollout_belief"][1]) == 10 and len(_lib.SIGNATURES["gp_belief_filter"][1]) == 7
    for n in ("float_laws", "qmdp_vectors", "parse_alpha"):
        assert n in gym_po_amd.__all__ and hasattr(gym_po_amd, n)
    for n in ("enable_belief", "disable_belief", "belief", "set_belief", "belief_filter", "set_belief_policy",
              "rollout_belief"):
        assert hasattr(TabularPOMDPEnv, n), n
    assert "GP_DERR_BELIEF 128u" in open(os.path.join(os.path.dirname(__file__), "..", "gym-po-taxi_amd", "csrc",
                                                      "gp_common.h")).read()
    assert "belief tracking" not in open(os.path.join(os.path.dirname(__file__), "..", "DESIGN.md")).read().split(
        "### 6p")[1].split("### 6q")[0]


# ------------------------------------------------------------------ calibration ----
B_CAL, K_CAL, TL_CAL = 1 << 16, 12, 7


def greedy_alpha(sp):
    """QMDP vectors of the model's exact law: a policy that depends on the belief."""
    from gym_po_amd.belief import qmdp_vectors
    l64 = bo.Laws64(sp)
    return qmdp_vectors(l64.Tf, sp.reward.astype(np.float64), sp.terminal, 0.95, 200).astype(F)


def simulate(sp, mode, step_fn, seed=17):
    """The numpy env with its Philox draws under `mode` ('uniform' actions or the 'greedy' alpha policy on the tracked
    belief), the belief tracked by step_fn(b, a, o, ended) -> b'. Yields (beliefs, states) after the reset and after
    each of the K steps."""
    lw = bo.Laws(sp)
    key = philox_key(seed)
    ora = PomdpOracle(B_CAL, sp)
    rng = np.random.default_rng(seed)
    alpha = greedy_alpha(sp) if mode == "greedy" else None
    obs = ora.reset(ora.philox_draws(0, key))
    b, _ = bo.reset_beliefs(lw, obs)
    yield b, ora.state.copy()
    for k in range(K_CAL):
        a = rng.integers(0, lw.A, B_CAL) if alpha is None else bo.policy(alpha, np.arange(lw.A), b)[0]
        o, _, tm, tr = ora.step(a, ora.philox_draws(1 + k, key))
        b = step_fn(b, a, o, tm | tr)
        yield b, ora.state.copy()


@pytest.mark.parametrize("mode", ["uniform", "greedy"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_calibration(name, mode):
    sp = spec(name, TL_CAL)
    lw = bo.Laws(sp)

    def step(b, a, o, ended):
        b, bad = bo.filter_step(lw, b, a, o, ended)
        assert not bad.any(), "a degenerate step"
        return b
    bo.assert_calibrated(simulate(sp, mode, step), f"{name} {mode}")


@pytest.mark.parametrize("wrong", ["z_by_s", "no_terminal_mask", "kept_across_end"])
def test_calibration_rejects_wrong_filters(wrong):
    """Teeth: three plausible mistakes, each a float64 filter on m37 under uniform actions, must each break the bound
    (|z| above 6 in some cell, or a true state given belief 0)."""
    sp = spec("m37", TL_CAL)
    l = bo.Laws64(sp)

    def step(b, a, o, ended):
        b = b.astype(np.float64)
        if wrong == "z_by_s":  # Z indexed by the state left, not the state entered
            u = np.where(l.terminal[None, :], 0.0, bo.predict64(l, b * l.Zf[a, :, o], a))
        else:
            u = l.Zf[a, :, o] * bo.predict64(l, b, a)
            if wrong != "no_terminal_mask":
                u = np.where(l.terminal[None, :], 0.0, u)
        if wrong == "kept_across_end":
            n = u.sum(-1, keepdims=True)
            u = np.where(n > 0, u, l.prior[None, :])  # (where the obs excludes the kept belief: the prior)
        else:
            u = np.where(ended[:, None], l.prior[None, :] * l.Rf[:, o].T, u)
        return u / u.sum(-1, keepdims=True)
    zmax, zero = 0.0, False
    for b, s in simulate(sp, "uniform", step):
        c = bo.calibration(b, s)
        zmax, zero = max(zmax, float(c["z"].max())), zero or c["min_true"] == 0
        if zmax > 6.0 or zero:  # rejected (over all 13 steps: |z| 5.0 with a belief of 0 / 44.1 / 195.2)
            break
    print(f"wrong filter {wrong}: max |z| {zmax:.1f}, belief 0 on a true state: {zero}")
    assert zmax > 6.0 or zero
