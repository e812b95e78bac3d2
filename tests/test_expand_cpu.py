"""CPU tests of the belief-set expansion's numpy restatement (tests/expand_oracle.py) and of the drivers
in gym_po_amd.belief (reset_points, expand_points, is_closed, pbvi_expanding). No GPU. Every equality is on bit
patterns.

The vectorised restatement equals the scalar statement written from the rule text; live successors and their
probabilities against a float64 filter on the exact integer laws, which knows nothing of the rule's order of
operations, within 1e-4 and within a derived rounding bound, with three wrong expansions that the comparisons must
reject; the detour maze (the collected set is closed, no point of it can be left out, the closure of the reset beliefs
is that set, pbvi_expanding from the reset beliefs alone reaches the pipeline's policy); the drivers' rules; symbols and
signatures.
"""
import inspect
import os
import re

import numpy as np
import pytest

import belief_oracle as bo
import expand_cases as xc
import expand_oracle as xo
import pbvi_cases as pc

F = np.float32
bits = xc.bits


def assert_same(got, want, msg=""):
    assert set(got) == set(xc.OUTPUTS)
    for k in xc.OUTPUTS:
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=f"{k} {msg}")


# ------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("name,P,Q", [("tiger", 24, 6), ("tiger", 5, None), ("hand", 7, 4), ("hand", 7, None),
                                      ("m5", 16, 9), ("m5", 3, 1), ("m5", 12, None), ("m37", 4, 5), ("m37", 3, None)])
def test_vectorised_equals_scalar(name, P, Q):
    lw = xc.laws(name)
    b, q, out = xc.reference(name, P, Q)
    assert out["succ"].dtype == F and out["actions"].dtype == np.int32 and out["obs"].dtype == np.int32
    for p in range(P):
        succ, dist, a, o, mass = xo.scalar_expand(lw, b[p], b if q is None else q)
        assert (int(out["actions"][p]), int(out["obs"][p])) == (a, o), p
        assert F(out["dist"][p]).view(np.uint32) == F(dist).view(np.uint32), p
        assert F(out["mass"][p]).view(np.uint32) == F(mass).view(np.uint32), p
        assert np.array_equal(bits(out["succ"][p]), bits(np.asarray(succ, dtype=F))), p
    # the inputs hold what they claim: one-hot, sparse and unnormalised points; duplicate reference rows
    assert ((b > 0).sum(-1) == 1).any() and ((b == 0).sum(-1) > 0).any()
    if P > 2:
        assert (b.sum(-1) > 2).any()
    if q is not None and Q >= 4:
        assert np.array_equal(q[Q - 1], q[0]) and np.array_equal(q[2], q[1])
    if q is None:  # against themselves the points are at distance 0 only where a successor is a point
        assert (out["dist"] >= 0).all()


def test_dead_points_ties_and_impossible_obs_by_hand():
    """The hand model (expand_cases.hand_tables), dyadic throughout. From (1, 0, 0): action 0 gives acc = (1/2, 1/4,
    1/4), n(0, 0) = 3/4 1/2 + 1/4 1/4 = 7/16 with b' = (6/7, 1/7, 0), n(0, 1) = 1/4 1/2 + 3/4 1/4 = 5/16 with
    b' = (2/5, 3/5, 0); action 1 stays in state 0 and both obs give b' = (1, 0, 0) with n = 1/2. Obs 2 never occurs.
    Against the single reference row (1, 0, 0): L1 = 2/7, 6/5, 0, 0: the farthest is (0, 1). Against (2/5, 3/5, 0)
    (float32): (0, 0) at 32/35 loses to (1, 0) at 6/5, which ties with (1, 1): the first wins."""
    lw = xc.laws("hand")
    b = np.array([[1, 0, 0], [0, 0.25, 0.75], [0, 0, 1], [0, 1, 0]], dtype=F)
    n = xo.masses(lw, b)
    assert n[0].tolist() == [[0.4375, 0.3125, 0.0], [0.5, 0.5, 0.0]] and not n[1:].any()
    out = xo.expand(lw, b, np.array([[1, 0, 0]], dtype=F))
    assert out["actions"].tolist() == [0, -1, -1, -1] and out["obs"].tolist() == [1, -1, -1, -1]
    assert out["mass"].tolist() == [0.3125, 0, 0, 0] and not out["succ"][1:].any() and not out["dist"][1:].any()
    assert not np.signbit(out["succ"]).any() and not np.signbit(out["dist"]).any() and not np.signbit(out["mass"]).any()
    assert out["succ"][0].tolist() == [F(0.125) / F(0.3125), F(0.1875) / F(0.3125), 0.0]
    far = xo.expand(lw, b[:1], out["succ"][:1])
    assert (int(far["actions"][0]), int(far["obs"][0])) == (1, 0) and far["succ"][0].tolist() == [1.0, 0.0, 0.0]
    assert far["mass"][0] == 0.5


def test_tiger_uniform_belief_under_listen_picks_the_first_obs():
    """Tiger's uniform belief: listen's two successors (0.85, 0.15) and (0.15, 0.85) are mirror images and the
    reference sets of expand_cases are symmetric, so both are equally far: obs 0 wins. Opening a door resets the
    problem: its successor is the uniform belief itself."""
    lw = xc.laws("tiger")
    for P, Q in ((67, 65), (257, 1027)):
        b, q, out = xc.reference("tiger", P, Q)
        assert b[0].tolist() == [0.5, 0.5]
        cand = {}
        for o in (0, 1):
            bp, bad = bo.filter_step(lw, b[:1], [0], [o], [False])
            assert not bad.any()
            cand[o] = xo.l1_to_set(bp, q)[0]
        assert cand[0] == cand[1] > 0
        assert (int(out["actions"][0]), int(out["obs"][0])) == (0, 0) and out["dist"][0] == cand[0]


# ------------------------------------------------------------------ the independent statement ----
def candidates(lw, b, wrong=None):
    """Every candidate of every point in float32, vectorised another way than expand_oracle.expand: n [P, A, O] and
    b' [P, A, O, S]. `wrong` names one of two plausible mistakes of the law."""
    P, S = b.shape
    term = np.zeros(S, dtype=bool) if wrong == "no_terminal_mask" else lw.terminal
    u = np.zeros((P, lw.A, lw.O, S), dtype=F)
    if wrong == "z_by_s":  # Z indexed by the state left, not the state entered
        for a in range(lw.A):
            for o in range(lw.O):
                acc = np.zeros((P, S), dtype=F)
                for s in range(S):
                    seen = (b[:, s] * lw.Zf[a, s, o]).astype(F)
                    acc = (acc + (seen[:, None] * lw.Tf[s, a][None]).astype(F)).astype(F)
                u[:, a, o] = np.where(term[None], F(0), acc)
    else:
        for a in range(lw.A):
            acc = np.zeros((P, S), dtype=F)
            for s in range(S):
                acc = (acc + (b[:, s, None] * lw.Tf[s, a][None]).astype(F)).astype(F)
            u[:, a] = np.where(term[None, None], F(0), (lw.Zf[a].T[None] * acc[:, None, :]).astype(F))
    n = np.zeros((P, lw.A, lw.O), dtype=F)
    for s1 in range(S):
        n = (n + u[..., s1]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return n, (u / n[..., None]).astype(F)


def select(n, bp, ref, last=False):
    """Step 3 and 4 on the candidates; last=True: the mistake of replacing on >= (the last maximiser)."""
    P, A, O, S = bp.shape
    out = {"succ": np.zeros((P, S), dtype=F), "dist": np.zeros(P, dtype=F), "actions": np.full(P, -1, dtype=np.int32),
           "obs": np.full(P, -1, dtype=np.int32), "mass": np.zeros(P, dtype=F)}
    for p in range(P):
        for a in range(A):
            for o in range(O):
                if not (n[p, a, o] > 0 and np.isfinite(n[p, a, o])):
                    continue
                d = xo.l1_to_set(bp[p, a, o][None], ref)[0]
                if out["actions"][p] < 0 or (d >= out["dist"][p] if last else d > out["dist"][p]):
                    out["succ"][p], out["dist"][p], out["mass"][p] = bp[p, a, o], d, n[p, a, o]
                    out["actions"][p], out["obs"][p] = a, o
    return out


def float64_errors(name, b, n, bp):
    """(the largest |b' - float64 filter| over the live candidates, the largest |n - float64 n| / bound)."""
    sp = xc.spec(name)
    l64 = bo.Laws64(sp)
    S = b.shape[1]
    n64 = xo.masses64(l64, b)
    live = (n > 0) & np.isfinite(n)
    assert np.array_equal(live, n64 > 0)
    worst_b = 0.0
    for a in range(n.shape[1]):
        for o in range(n.shape[2]):
            m = live[:, a, o]
            if m.any():
                want = bo.filter_step64(l64, b[m].astype(np.float64), np.full(m.sum(), a), np.full(m.sum(), o),
                                        np.zeros(m.sum(), dtype=bool))
                worst_b = max(worst_b, float(np.abs(bp[m, a, o].astype(np.float64) - want).max()))
    ratio = np.abs(n.astype(np.float64) - n64)[live] / (xo.mass_bound(S) * n64[live])
    return worst_b, float(ratio.max())


@pytest.mark.parametrize("name,P", [("tiger", 24), ("hand", 12), ("m5", 40), ("m37", 24)])
def test_successors_and_masses_against_the_float64_filter(name, P):
    """Live successors within the 1e-4 that tests/test_belief_cpu.py asserts of the filter; mass within
    expand_oracle.mass_bound(S) n (derived there). The candidates made here equal the restatement's, so the two
    comparisons cover what `expand` returns."""
    lw = xc.laws(name)
    b = xc.points(name, P)
    assert b[b > 0].min() > 2.0 ** -40  # (mass_bound's no-underflow premise)
    n, bp = candidates(lw, b)
    np.testing.assert_array_equal(bits(n), bits(xo.masses(lw, b)))
    for Q in (None, 5):
        _, q, want = xc.reference(name, P, Q)
        assert_same(select(n, bp, b if q is None else q), want, f"Q {Q}")
    worst_b, ratio = float64_errors(name, b, n, bp)
    print(f"{name}: largest |b' - float64| {worst_b:.3g}, largest mass error / bound {ratio:.3g}")
    assert worst_b <= 1e-4 and ratio <= 1.0
    pick = want["actions"] >= 0
    assert pick.any() and (want["mass"][pick] > 0).all()


@pytest.mark.parametrize("name", ["hand", "m5", "m37"])
@pytest.mark.parametrize("wrong", ["no_terminal_mask", "z_by_s"])
def test_the_float64_filter_rejects_wrong_laws(name, wrong):
    """Teeth: each wrong law breaks a bound of the test above (a successor off by more than 1e-4, a mass outside its
    bound, or a candidate alive that the exact law says is dead)."""
    lw = xc.laws(name)
    b = xc.points(name, 24)
    n, bp = candidates(lw, b, wrong)
    try:
        worst_b, ratio = float64_errors(name, b, n, bp)
    except AssertionError:
        return  # the set of live candidates itself is wrong
    print(f"{name} {wrong}: largest |b' - float64| {worst_b:.3g}, largest mass error / bound {ratio:.3g}")
    assert worst_b > 1e-4 or ratio > 1.0


@pytest.mark.parametrize("name,P,Q", [("tiger", 67, 65), ("hand", 7, 4)])
def test_the_scalar_statement_rejects_the_last_maximiser(name, P, Q):
    """Teeth: on a tie (Tiger's mirror successors; the hand model's action 1, whose two obs give one successor) taking
    the last maximiser changes the obs, and the scalar statement says which is right."""
    lw = xc.laws(name)
    b, q, want = xc.reference(name, P, Q)
    n, bp = candidates(lw, b)
    assert_same(select(n, bp, q), want)
    wrong = select(n, bp, q, last=True)
    differ = np.flatnonzero((wrong["obs"] != want["obs"]) | (wrong["actions"] != want["actions"]))
    assert len(differ) > 0
    for p in differ[:4]:
        _, dist, a, o, _ = xo.scalar_expand(lw, b[p], q)
        assert (a, o) == (int(want["actions"][p]), int(want["obs"][p]))
        assert F(dist) == wrong["dist"][p] == want["dist"][p]


# ------------------------------------------------------------------ the detour maze ----
@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_detour_set_is_closed_and_no_point_can_be_left_out(obs_type):
    """The 14 collected points: every dist is 0 (the closure that DESIGN §6s's monotonicity argument needs, stated by
    the library instead of a loop in a test). With any one non-reset point removed, some remaining point's farthest
    successor is that very point, at a positive distance."""
    from gym_po_amd.belief import is_closed, reset_points
    d = pc.detour_pipeline(obs_type)
    env = xo.CpuEnv(d["sp"])
    pts = d["points"]
    assert pts.shape[0] == 14
    out = env.expand_beliefs(pts)
    assert not out["dist"].any() and is_closed(env, pts)
    resets = {r.tobytes() for r in bits(reset_points(env))}
    assert 1 <= len(resets) < 14 and all(r in {x.tobytes() for x in bits(pts)} for r in resets)
    removed = 0
    for i in range(14):
        if bits(pts[i]).tobytes() in resets:
            continue
        rest = np.delete(pts, i, axis=0)
        o = env.expand_beliefs(rest)
        hit = [p for p in range(13) if o["dist"][p] > 0 and np.array_equal(bits(o["succ"][p]), bits(pts[i]))]
        assert hit, f"point {i} is nobody's farthest successor"
        assert not is_closed(env, rest)
        removed += 1
    assert removed == 14 - len(resets)


@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_closure_of_the_reset_beliefs_is_the_collected_set(obs_type):
    """expand_points from reset_points until nothing is added gives the 14 collected points as a set. Why it must: (1)
    the 14 are closed under the successors of steps that do not end (the test above) and contain the reset beliefs, and
    every point expand_points adds is such a successor of a member, so by induction the closure is a subset of the 14;
    (2) the closure's fixed point has every dist == 0, so it holds every successor of every member, and each of the 14
    was held by an env of the collecting run: it is reached from a reset belief by filter steps that each had positive
    probability under the integer laws (p = 0: all laws are 0 / 1 but the start side), every one of them a candidate
    of step 2 or a reset belief. The set at most doubles per round."""
    from gym_po_amd.belief import expand_points, is_closed, reset_points
    d = pc.detour_pipeline(obs_type)
    env = xo.CpuEnv(d["sp"])
    pts = reset_points(env)
    sizes = [len(pts)]
    for _ in range(32):
        grown = expand_points(env, pts)
        assert len(pts) <= len(grown) <= 2 * len(pts)
        if len(grown) == len(pts):
            break
        pts = grown
        sizes.append(len(pts))
    print(f"{obs_type}: sizes {sizes}")
    assert is_closed(env, pts)
    np.testing.assert_array_equal(bits(pts), bits(d["points"]))  # (both in distinct_rows' order)


@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_pbvi_expanding_from_the_reset_beliefs_reaches_the_pipeline(obs_type):
    """Without a collecting walk: pbvi_expanding from the reset beliefs alone ends on the 14 points with the vectors
    and actions of detour_pipeline (bit for bit), hence its episodes: every one a termination with +1."""
    from gym_po_amd.belief import pbvi_expanding
    d = pc.detour_pipeline(obs_type)
    env = xo.CpuEnv(d["sp"])
    alpha, actions, pts, values = pbvi_expanding(env, pc.DETOUR_GAMMA, 32, pc.DETOUR_SWEEPS)
    np.testing.assert_array_equal(bits(pts), bits(d["points"]))
    np.testing.assert_array_equal(bits(alpha), bits(d["alpha"]))
    np.testing.assert_array_equal(actions, d["actions"])
    np.testing.assert_array_equal(bits(values[-1]), bits(d["values"]))
    assert 1 < len(values) < 32 and [v.shape for v in values][-1] == (pc.DETOUR_SWEEPS, 14)
    assert all(v.shape[1] <= w.shape[1] for v, w in zip(values, values[1:]))
    run = pc.closed_loop_on_oracle(d["sp"], alpha, actions, pc.DETOUR_B, pc.EVAL_K, pc.EVAL_SEED)
    want = d["run_pbvi"]
    assert run["episodes"] == want["episodes"] and run["terminated"] == want["terminated"] == run["episodes"]
    assert run["truncated"] == 0 and np.array_equal(run["returns"], want["returns"]) and (run["returns"] == 1.0).all()


# ------------------------------------------------------------------ the drivers ----
class FakeEnv:
    n_states = 2
    reward = np.array([[0.0]], dtype=F)


def test_reset_points_rule():
    """The ended rule per reset obs, in float32 with a sequential sum; an obs that opens no episode is left out; equal
    rows collapse, in distinct_rows' order."""
    from gym_po_amd import row_thresholds
    from gym_po_amd.belief import float_laws, reset_points

    class E:
        trans_thr = row_thresholds(np.eye(3)[:, None, :])
        obs_thr = row_thresholds(np.full((1, 3, 4), 0.25))
        start_thr = row_thresholds([0.5, 0.25, 0.25])
        # obs 0: states 0 and 1; obs 1: state 2 only; obs 2: never; obs 3: as obs 0 (a duplicate row)
        reset_obs_thr = row_thresholds([[0.5, 0, 0, 0.5], [0.5, 0, 0, 0.5], [0, 1.0, 0, 0]])
        terminal = np.zeros(3, dtype=bool)
    got = reset_points(E)
    assert got.dtype == F and got.tolist() == [[0.0, 0.0, 1.0], [F(0.25) / F(0.375), F(0.125) / F(0.375), 0.0]]
    lw = float_laws(E)
    for o, row in ((1, 0), (0, 1), (3, 1)):
        want, bad = bo.scalar_filter_step(bo.Laws(E, lw["prior"]), None, 0, o, True)
        assert not bad and got[row].tolist() == [float(x) for x in want]
    assert bo.scalar_filter_step(bo.Laws(E), None, 0, 2, True)[1]  # the obs left out is the degenerate one
    # another prior (what enable_belief(prior) would hold): normalised by the filter's sequential sum, then the same rule
    other = reset_points(E, prior=[0.0, 3.0, 1.0])
    pr = np.array([0.0, 0.75, 0.25], dtype=F)
    assert other.tolist() == [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]
    for o, row in ((1, 0), (0, 1)):
        want, bad = bo.scalar_filter_step(bo.Laws(E, pr), None, 0, o, True)
        assert not bad and other[row].tolist() == [float(x) for x in want]
    for bad_prior, match in (([0.5, 0.5], "prior must be"), ([0.0, 0.0, 0.0], "positive"), ([1.0, -1.0, 1.0], ">= 0")):
        with pytest.raises(ValueError, match=match):
            reset_points(E, prior=bad_prior)


def test_expand_drivers_rules():
    from gym_po_amd.belief import expand_points, is_closed, pbvi_expanding
    pts = np.array([[0.5, 0.5], [1.0, 0.0], [0.25, 0.75]], dtype=F)
    calls = []

    def expand(points):
        calls.append(np.array(points))
        succ = np.array([[0.0, 1.0], [0.5, 0.5], [-0.0, 1.0]], dtype=F)
        return {"succ": succ, "dist": np.array([0.5, 0.0, 1.0], dtype=F)}
    got = expand_points(FakeEnv, pts, expand)
    # the successors with dist > 0 join, the one with dist == 0 does not; distinct_rows' order; -0 is other bits
    assert got.dtype == F and got.tolist() == [[0.0, 1.0], [0.25, 0.75], [0.5, 0.5], [1.0, 0.0], [-0.0, 1.0]]
    assert np.signbit(got[4, 0]) and calls[0].dtype == F and calls[0].tolist() == pts.tolist()
    assert not is_closed(FakeEnv, pts, expand)
    assert is_closed(FakeEnv, pts, lambda p: {"succ": np.zeros_like(p), "dist": np.zeros(len(p), dtype=F)})
    # a kept successor that is already a point adds nothing; duplicates among the points collapse
    same = expand_points(FakeEnv, np.concatenate((pts, pts[:1])),
                         lambda p: {"succ": p[::-1].copy(), "dist": np.ones(len(p), dtype=F)})
    assert same.tolist() == [[0.25, 0.75], [0.5, 0.5], [1.0, 0.0]]
    for bad in (np.zeros((2, 3), dtype=F), np.zeros((0, 2), dtype=F), np.zeros(2, dtype=F)):
        with pytest.raises(ValueError, match="points must be"):
            expand_points(FakeEnv, bad, expand)
        with pytest.raises(ValueError, match="points must be"):
            is_closed(FakeEnv, bad, expand)
    # pbvi_expanding: rounds of pbvi with one expansion between two, the early stop, the refusals
    log = []

    def backup(points, alpha, gamma):
        log.append(len(points))
        P = len(points)
        return {"alpha": np.tile(np.array([[1.0, 2.0]], dtype=F), (P, 1)), "actions": np.zeros(P, dtype=np.int32),
                "value": np.full(P, float(P), dtype=F)}

    def grow(points):  # every point proposes one new point until there are four
        n = len(points)
        succ = np.tile(np.array([[n / 8.0, 1.0 - n / 8.0]], dtype=F), (n, 1))
        return {"succ": succ, "dist": np.full(n, 1.0 if n < 4 else 0.0, dtype=F)}
    alpha, actions, out, values = pbvi_expanding(FakeEnv, 0.5, 10, 2, points=pts[:2], backup=backup, expand=grow)
    assert log == [2, 2, 3, 3, 4, 4]  # two sweeps on 2, 3 and 4 points; closed at 4: rounds 4..10 are not run
    assert out.shape == (4, 2) and [v.shape for v in values] == [(2, 2), (2, 3), (2, 4)]
    assert alpha.tolist() == [[1.0, 2.0]] and actions.tolist() == [0] and actions.dtype == np.int64
    log.clear()
    _, _, out, values = pbvi_expanding(FakeEnv, 0.5, 2, 1, points=pts[:2], backup=backup, expand=grow)
    assert log == [2, 3] and out.shape == (3, 2) and len(values) == 2  # no expansion after the last round
    with pytest.raises(ValueError, match="rounds"):
        pbvi_expanding(FakeEnv, 0.5, 0, 1, points=pts, backup=backup, expand=grow)
    with pytest.raises(ValueError, match="sweeps"):
        pbvi_expanding(FakeEnv, 0.5, 1, 0, points=pts, backup=backup, expand=grow)
    with pytest.raises(ValueError, match="gamma"):
        pbvi_expanding(FakeEnv, 1.0, 1, 1, points=pts, backup=backup, expand=grow)


def test_pbvi_keeps_its_signature():
    from gym_po_amd.belief import expand_points, is_closed, pbvi, pbvi_expanding, reset_points
    assert list(inspect.signature(pbvi).parameters) == ["env", "points", "gamma", "sweeps", "backup"]
    assert list(inspect.signature(pbvi_expanding).parameters) == "env gamma rounds sweeps points backup expand".split()
    assert list(inspect.signature(expand_points).parameters) == ["env", "points", "expand"]
    assert list(inspect.signature(is_closed).parameters) == ["env", "points", "expand"]
    assert list(inspect.signature(reset_points).parameters) == ["env", "prior"]
    assert inspect.signature(reset_points).parameters["prior"].default is None


def test_symbols_and_signature():
    import ctypes
    import gym_po_amd
    from gym_po_amd import TabularPOMDPEnv, _lib
    root = os.path.join(os.path.dirname(__file__), "..")
    header = open(os.path.join(root, "include", "gym_po_amd.h")).read()
    assert re.search(r"\bint gp_belief_expand\(gp_env\* env, int n_points, const float\* points, int n_ref, "
                     r"const float\* ref, float\* succ_out,\s+float\* dist_out, int32_t\* act_out, int32_t\* obs_out, "
                     r"float\* mass_out, void\* stream\);", header)
    L = _lib.lib()
    assert hasattr(L, "gp_belief_expand")
    res, args = _lib.SIGNATURES["gp_belief_expand"]
    assert res is ctypes.c_int and len(args) == 11 and args[1] is ctypes.c_int and args[3] is ctypes.c_int
    for n in ("reset_points", "expand_points", "is_closed", "pbvi_expanding"):
        assert n in gym_po_amd.__all__ and hasattr(gym_po_amd, n)
    assert hasattr(TabularPOMDPEnv, "expand_beliefs")
    assert list(inspect.signature(TabularPOMDPEnv.expand_beliefs).parameters) == ["self", "points", "ref", "out"]
    csrc = os.path.join(root, "gym-po-taxi_amd", "csrc")
    kernel = open(os.path.join(csrc, "pomdp_expand.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and os.path.exists(os.path.join(csrc, "pomdp_expand.h"))
    # the rule text stands in the header, the kernel file and DESIGN alike
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "### 6t" in design
    squeeze = lambda t: re.sub(r"[\s*/]+", " ", t)  # noqa: E731
    for line in ("u(s') = terminal[s'] ? +0 : fl(Zf[a][s'][o] acc_a(s'))", "L1 = sum_s |fl(b'[s] - q[s])|",
                 "the first live candidate of the largest dist, a ascending, then o ascending",
                 "act = obs = -1, dist = mass = +0"):
        for text in (header, kernel, design.split("### 6t")[1]):
            assert line in squeeze(text), line
