"""CPU tests of the point-based value backup's numpy restatement (tests/pbvi_oracle.py) and of the
driver in gym_po_amd.belief (collect_beliefs' dedupe, pbvi). No GPU.

The vectorised restatement equals the scalar statement written from the rule text, bit for bit; the backup against a
float64 exhaustive enumeration of the exact value function's vectors (Monahan), which knows nothing of the backup's
order of operations, within a derived rounding bound, with three wrong backups that the comparison must reject; the
bounds (monotone from the lower bound on a belief set closed under the filter, below the QMDP value everywhere); the
driver's rules; symbols and signatures; and the demonstration on the detour maze: the PBVI policy visits the priest
and always reaches heaven where the QMDP policy never finishes an episode.
"""
import os
import re

import numpy as np
import pytest

import belief_oracle as bo
import pbvi_cases as pc
import pbvi_oracle as po

F = np.float32
bits = pc.bits


# ------------------------------------------------------------------ the restatement ----
@pytest.mark.parametrize("gamma", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("name,P,N", [("tiger", 24, 6), ("tiger", 5, 3), ("m5", 16, 6), ("m5", 3, 1), ("m37", 4, 6)])
def test_vectorised_equals_scalar(name, P, N, gamma):
    md = pc.model(name)
    b, al = pc.special_inputs(name, P, N, seed=1)
    out = po.backup(md, b, al, gamma)
    assert out["alpha"].dtype == F and out["actions"].dtype == np.int32 and out["value"].dtype == F
    for p in range(P):
        beta, a, v = po.scalar_backup(md, b[p], al, gamma)
        assert int(out["actions"][p]) == a, p
        assert F(out["value"][p]).view(np.uint32) == F(v).view(np.uint32), p
        assert np.array_equal(bits(out["alpha"][p]), bits(np.asarray(beta, dtype=F))), p
    # the inputs hold what they claim: one-hot, sparse and unnormalised points, mixed signs, duplicates
    assert (b[0] > 0).sum() == 1 and ((b == 0).sum(-1) > 0).any() and (b.sum(-1) > 2).any()
    assert (al > 0).any() and (al < 0).any()
    if N >= 6:
        assert np.array_equal(al[4], al[1]) and np.array_equal(al[N - 1], al[0]) and not np.array_equal(al[3], al[1])
    if name == "m5":  # an obs of probability zero: from the second one-hot point under action 0 every u(s') is 0
        pr = np.einsum("s,sat,ato->ao", b[1].astype(np.float64), md.Tf.astype(np.float64),
                       md.Zf.astype(np.float64) * (~md.terminal)[None, :, None])
        assert (pr == 0).any() and (pr > 0).any()


def test_first_maximiser_and_terminal_rule_by_hand():
    """Two states, state 1 terminal; one action that moves 0 -> 1 with probability 1/2; obs 0 always. Reward 1 on every
    move. With alpha = (4, 100): w(0) = 4, w(1) = +0 (terminal: its 100 never counts), beta(0) = 1 + g (1/2) 4,
    beta(1) = 1 + g 0 (state 1 loops onto itself)."""
    from gym_po_amd import row_thresholds
    from pomdp_oracle import Spec
    T = np.array([[[0.5, 0.5]], [[0.0, 1.0]]])
    Z = np.array([[[1.0, 0.0], [1.0, 0.0]]])  # a second obs that never occurs: it adds +0 everywhere
    sp = Spec(row_thresholds(T), row_thresholds(Z), row_thresholds([1.0, 0.0]), row_thresholds(Z[0]),
              np.ones((2, 1, 2), dtype=F), [False, True], 7)
    md = po.Model(sp)
    out = po.backup(md, np.array([[1.0, 0.0], [0.25, 0.75]], dtype=F), np.array([[4.0, 100.0], [4.0, 100.0]], dtype=F),
                    0.5)
    assert out["alpha"].tolist() == [[2.0, 1.0], [2.0, 1.0]] and out["value"].tolist() == [2.0, 1.25]
    assert out["actions"].tolist() == [0, 0]


# ------------------------------------------------------------------ the independent statement ----
def enumerated(name, gamma=0.95, horizon=3):
    return pc.cached(("monahan", name, gamma, horizon), lambda: po.monahan(po.Model64(pc.spec(name)), gamma, horizon))


def random_points(S, P, seed):
    rng = np.random.default_rng(seed)
    b = rng.random((P, S)) * (rng.random((P, S)) > 0.3)
    b[np.arange(P), rng.integers(0, S, P)] += 0.1
    b[:S] = np.eye(S)[:min(S, P)]  # the corners too
    return (b / b.sum(-1, keepdims=True)).astype(F)


def backup64(m, b, alpha, gamma, wrong=None):
    """The value of a backup in float64 with numpy's own sums; `wrong` names one of three plausible mistakes."""
    live = np.ones(m.S) if wrong == "no_terminal_mask" else m.live
    best = None
    for a in range(m.A):
        r = (m.T[:, a, :] * m.R[:, a, :]).sum(-1)
        tot = 0.0
        for o in range(m.O):
            if wrong == "z_by_s":  # Z indexed by the state left, not the state entered
                g = m.Z[a, :, o][None, :] * ((alpha * live[None, :]) @ m.T[:, a, :].T)
            else:
                g = (alpha * (m.Z[a, :, o] * live)[None, :]) @ m.T[:, a, :].T  # [N, S]
            tot = tot + (b @ g.T).max(-1)
        v = (gamma * (b @ r) if wrong == "gamma_on_r" else b @ r) + gamma * tot
        best = v if best is None else np.maximum(best, v)
    return best


@pytest.mark.parametrize("name", ["tiger", "m5"])
def test_backup_against_exhaustive_enumeration(name):
    """point_backup(b, Gamma_{h-1}) has the value max over Gamma_h of b . alpha, and its vector is a member of Gamma_h,
    h = 1..3 (Tiger 3 / 27 / 2,187 vectors; (5,2,3) 2 / 16 / 8,192), within pbvi_oracle.abs_bound. Largest observed
    error / bound: Tiger value 1.35e-6 / 2.6e-4 (h = 3), vector entry 3.05e-6 / 8.1e-5 (h = 2); (5,2,3) value
    1.48e-7 / 6.2e-6, vector entry 1.39e-7 / 2.3e-6."""
    gamma = 0.95
    sets = enumerated(name, gamma)
    md, m64 = pc.model(name), po.Model64(pc.spec(name))
    assert [len(g) for g in sets] == {"tiger": [1, 3, 27, 2187], "m5": [1, 2, 16, 8192]}[name]
    b = random_points(md.S, 200, seed=md.S)
    b64 = b.astype(np.float64)
    for h in (1, 2, 3):
        out = po.backup(md, b, sets[h - 1].astype(F), gamma)
        v_bound, beta_bound = po.abs_bound(md, b, sets[h - 1], gamma)
        want = (b64 @ sets[h].T).max(-1)
        err = np.abs(out["value"].astype(np.float64) - want)
        # the vector: a member of Gamma_h (the one of its own choices), entry by entry
        dist = np.array([np.abs(sets[h] - out["alpha"][p].astype(np.float64)[None, :]).max(-1).min() for p in range(len(b))])
        print(f"{name} h={h}: value error max {err.max():.3g} (bound {v_bound.min():.3g}..{v_bound.max():.3g}), "
              f"vector entry error max {dist.max():.3g} (bound {beta_bound:.3g})")
        assert (err <= v_bound).all()
        assert (dist <= beta_bound).all()
        # the float64 statement of the same rule agrees with the enumeration far inside the bound
        assert np.abs(backup64(m64, b64, sets[h - 1], gamma) - want).max() < 1e-9


@pytest.mark.parametrize("name,wrong", [("m5", "no_terminal_mask"), ("m5", "z_by_s"), ("m5", "gamma_on_r"),
                                        ("tiger", "gamma_on_r")])
def test_enumeration_rejects_wrong_backups(name, wrong):
    """Teeth: each wrong backup breaks the bound of the test above at some point of some horizon."""
    gamma = 0.95
    sets = enumerated(name, gamma)
    md, m64 = pc.model(name), po.Model64(pc.spec(name))
    b = random_points(md.S, 200, seed=md.S)
    b64 = b.astype(np.float64)
    worst = 0.0
    for h in (1, 2, 3):
        v_bound, _ = po.abs_bound(md, b, sets[h - 1], gamma)
        err = np.abs(backup64(m64, b64, sets[h - 1], gamma, wrong) - (b64 @ sets[h].T).max(-1))
        worst = max(worst, float((err / v_bound).max()))
    print(f"{name} {wrong}: largest error / bound {worst:.3g}")
    assert worst > 1.0


# ------------------------------------------------------------------ bounds ----
def successors(sp, points):
    """Every belief the filter reaches in one step that does not end from `points`, over every action and every obs of
    positive probability."""
    lw = bo.Laws(sp)
    out = []
    for a in range(lw.A):
        for o in range(lw.O):
            E = len(points)
            nb, bad = bo.filter_step(lw, points, np.full(E, a), np.full(E, o), np.zeros(E, dtype=bool))
            out.append(nb[~bad])
    return np.concatenate(out)


@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_values_rise_from_the_lower_bound_and_stay_below_qmdp(obs_type):
    """From the driver's starting vector every sweep's value at every point is >= the previous sweep's and <= the QMDP
    value, within abs_bound. The first holds in exact arithmetic where the point set is closed under the filter's
    successors (H V_n >= H V_{n-1} at a point needs V_n >= V_{n-1} at its successors, and the driver drops the old
    vectors): the collected set of the detour maze is, which is asserted first. The second holds for any set: every
    vector is the value of a policy tree."""
    from gym_po_amd.belief import distinct_rows
    d = pc.detour_pipeline(obs_type)
    sp, md, pts, values = d["sp"], d["md"], d["points"], d["values"]
    have = {r.tobytes() for r in bits(pts)}
    live = pts[(pts[:, ~sp.terminal].sum(-1) > 0)]
    assert all(r.tobytes() in have for r in bits(distinct_rows(successors(sp, live))))
    assert values.shape == (pc.DETOUR_SWEEPS, len(pts))
    floor = np.full((1, md.S), min(0.0, float(md.reward.min())) / (1 - pc.DETOUR_GAMMA), dtype=F)
    bound, _ = po.abs_bound(md, pts, np.maximum(np.abs(d["qmdp"]).max(), np.abs(floor).max()) * np.ones((1, md.S)),
                            pc.DETOUR_GAMMA)
    v0 = (pts.astype(np.float64) @ floor[0].astype(np.float64))
    prev = v0
    for k in range(len(values)):
        v = values[k].astype(np.float64)
        assert (v >= prev - bound).all(), f"sweep {k}"
        prev = v
    upper = (pts.astype(np.float64) @ d["qmdp"].T).max(-1)
    assert (values.astype(np.float64) <= upper[None, :] + bound[None, :]).all()
    assert (values[-1] > values[0]).any()


@pytest.mark.parametrize("name", ["tiger", "m5", "m37"])
def test_values_stay_below_qmdp_on_random_points(name):
    from gym_po_amd.belief import pbvi, qmdp_vectors
    sp, md = pc.spec(name), pc.model(name)
    gamma = 0.95
    pts = random_points(md.S, 40, seed=3)
    alpha, actions, values = pbvi(md, pts, gamma, 8, backup=lambda p, a, g: po.backup(md, p, a, g))
    l64 = bo.Laws64(sp)
    q = qmdp_vectors(l64.Tf, sp.reward.astype(np.float64), sp.terminal, gamma, 2000)
    M = max(np.abs(q).max(), abs(min(0.0, float(md.reward.min())) / (1 - gamma)))
    bound, _ = po.abs_bound(md, pts, M * np.ones((1, md.S)), gamma)
    upper = (pts.astype(np.float64) @ q.T).max(-1)
    assert (values.astype(np.float64) <= upper[None, :] + bound[None, :]).all()
    # the first sweep never falls below the starting vector (H V_0 >= V_0 for a uniform lower bound)
    v0 = pts.astype(np.float64).sum(-1) * (min(0.0, float(md.reward.min())) / (1 - gamma))
    assert (values[0].astype(np.float64) >= v0 - bound).all()


# ------------------------------------------------------------------ the driver ----
class FakeModel:
    n_states = 3
    reward = np.array([[-2.0, 1.0]], dtype=F)


def test_pbvi_driver_rules():
    from gym_po_amd.belief import pbvi
    calls = []
    vecs = np.array([[1, 2, 3], [4, 5, 6], [1, 2, 3], [0.0, 5, 6], [-0.0, 5, 6], [4, 5, 6]], dtype=F)

    def backup(points, alpha, gamma):
        calls.append((np.array(alpha), gamma))
        return {"alpha": vecs if len(calls) == 1 else vecs + 1, "actions": np.array([5, 4, 3, 2, 1, 0], dtype=np.int32),
                "value": np.arange(6, dtype=F) * len(calls)}
    pts = np.eye(3, dtype=F)[[0, 1, 2, 0, 1, 2]]
    alpha, actions, values = pbvi(FakeModel, pts, 0.75, 2, backup=backup)
    # the starting vector: min(0, min reward) / (1 - gamma) in every state; then the distinct vectors of the last sweep
    assert calls[0][0].dtype == F and calls[0][0].tolist() == [[-8.0, -8.0, -8.0]] and calls[0][1] == 0.75
    # bitwise duplicates leave, the first occurrence stays, in point order; -0 and +0 are different vectors
    assert calls[1][0].tolist() == vecs[[0, 1, 3, 4]].tolist() and np.signbit(calls[1][0][3, 0])
    assert alpha.tolist() == (vecs + 1)[[0, 1, 3]].tolist() and actions.tolist() == [5, 4, 2]
    assert alpha.dtype == F and actions.dtype == np.int64
    assert values.dtype == F and values.tolist() == [[0, 1, 2, 3, 4, 5], [0, 2, 4, 6, 8, 10]]

    class Pos(FakeModel):
        reward = np.array([[2.0, 1.0]], dtype=F)
    calls.clear()
    pbvi(Pos, pts, 0.5, 1, backup=backup)
    assert calls[0][0].tolist() == [[0.0, 0.0, 0.0]]
    for kw, match in ((dict(gamma=1.0), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma=float("nan")), "gamma"),
                      (dict(sweeps=0), "sweeps"), (dict(points=np.zeros((2, 4), dtype=F)), "points"),
                      (dict(points=np.zeros((0, 3), dtype=F)), "points")):
        args = dict(points=pts, gamma=0.5, sweeps=1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            pbvi(FakeModel, args["points"], args["gamma"], args["sweeps"], backup=backup)


def test_distinct_rows_order():
    from gym_po_amd.belief import distinct_rows
    b = np.array([[0.5, 0.5], [0.0, 1.0], [0.5, 0.5], [1.0, 0.0], [0.25, 0.75], [-0.0, 1.0]], dtype=F)
    got = distinct_rows(b)
    assert got.dtype == F and got.tolist() == [[0.0, 1.0], [0.25, 0.75], [0.5, 0.5], [1.0, 0.0], [-0.0, 1.0]]
    assert np.signbit(got[4, 0]) and not np.signbit(got[0, 0])
    with pytest.raises(ValueError):
        distinct_rows(np.zeros(3, dtype=F))


def test_symbols_and_signature():
    import ctypes
    import gym_po_amd
    from gym_po_amd import TabularPOMDPEnv, _lib
    root = os.path.join(os.path.dirname(__file__), "..")
    header = open(os.path.join(root, "include", "gym_po_amd.h")).read()
    assert re.search(r"\bint gp_belief_backup\(gp_env\* env, int n_points, const float\* points, int n_vectors, "
                     r"const float\* alpha, float gamma,\s+float\* alpha_out, int32_t\* act_out, float\* value_out, "
                     r"void\* stream\);", header)
    L = _lib.lib()
    assert hasattr(L, "gp_belief_backup")
    res, args = _lib.SIGNATURES["gp_belief_backup"]
    assert res is ctypes.c_int and len(args) == 10 and args[1] is ctypes.c_int and args[3] is ctypes.c_int
    assert args[5] is ctypes.c_float
    for n in ("collect_beliefs", "pbvi"):
        assert n in gym_po_amd.__all__ and hasattr(gym_po_amd, n)
    assert hasattr(TabularPOMDPEnv, "point_backup")
    kernel = open(os.path.join(root, "gym-po-taxi_amd", "csrc", "pomdp_backup.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "### 6s" in design
    assert "point-based solvers on the device" not in design.split("### 6r")[1].split("### 6s")[0]


# ------------------------------------------------------------------ the demonstration ----
@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_detour_maze_pbvi_reaches_heaven_where_qmdp_dithers(obs_type):
    """The detour maze, p = 0, gamma 0.95, default rewards, time_limit 30, entirely on the numpy restatements: beliefs
    collected under a fixed uniform plane (14 distinct ones), 25 sweeps. Under the PBVI policy every finished episode
    is a termination with return +1; the QMDP policy walks to the junction and dithers: no episode of it terminates
    (mean return 0 per finished episode, all of them truncations)."""
    d = pc.detour_pipeline(obs_type)
    assert d["points"].shape == (14, 30) and d["alpha"].shape[1] == 30 and len(d["alpha"]) == len(d["actions"])
    good, base = d["run_pbvi"], d["run_qmdp"]
    print(f"{obs_type}: PBVI {good['episodes']} episodes, {good['truncated']} truncated, mean return "
          f"{good['returns'].mean():.3f}; QMDP {base['episodes']} episodes, {base['terminated']} terminated, mean return "
          f"{base['returns'].mean():.3f}")
    assert good["episodes"] >= 4 * pc.DETOUR_B and good["truncated"] == 0 and good["terminated"] == good["episodes"]
    assert (good["returns"] == 1.0).all()
    assert base["episodes"] >= pc.DETOUR_B and base["returns"].mean() < 0.5
