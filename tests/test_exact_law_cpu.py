"""CPU tests of the exact-law reference (tests/exact_law.py) and of the scheme built on it.

1. The forward and backward passes equal a brute-force enumeration of every path of a tiny problem.
2. The lowerings from probabilities to thresholds (`row_thresholds`, `controller_thresholds`) keep every entry within
   2^-30, every zero exactly zero and every row sum exactly 1.
3. The numpy oracles of the three kernels, run closed loop with the controller oracle's draws, stay inside every bound
   of `assert_law` on every case of tests/exact_law_cases.py, at the device's (seed, B, K): 2 to 3 s per case. The
   device equals these oracles bit for bit (asserted elsewhere), so this is the device's test made in advance, and it
   exercises the rules' statement itself: nothing in `exact_law` knows which Philox word decides what.
4. Teeth: four deliberately wrong closed loops are rejected.
"""
import numpy as np
import pytest

import exact_law
from exact_law_cases import CASES, GAMMA, SEED, controller

MUTANTS = ("obs_from_y0", "node_kept", "ctrl_is_env_y0", "frozen_step")


def closed_loop(case, B, mutant=None):
    """K closed-loop steps of the case's numpy oracle after reset(SEED), the controller evaluated as
    tests/controller_oracle.py states it. -> (hist int64 [K, cells], metrics, {"counts", "ret_q"}).

    Mutants (built here, around the draws and the loop; the oracles stay as they are):
      obs_from_y0     the obs of a step that goes on is drawn with the word that drew s' (tabular oracle only)
      node_kept       the node survives an episode end
      ctrl_is_env_y0  the controller's draw is the env block's y0 of the same step
      frozen_step     the step index of every draw stays at the first step's"""
    from controller_oracle import choose, controller_draws
    from controller_stats_oracle import controller_stats
    from oracle.philox import philox_key
    assert mutant is None or mutant in MUTANTS
    ora = case.oracle(B)
    thr = case.thr.astype(np.int64)
    M, O, L = thr.shape
    A, K = L // M, case.K
    key = philox_key(SEED)
    obs0 = ora.reset(ora.philox_draws(0, key)).astype(np.int64)
    obs, node = obs0, np.zeros(B, dtype=np.int64)
    planes = {n: [] for n in ("obs", "actions", "nodes", "rew", "term", "trunc")}
    m = dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)
    hist = np.zeros((K, M * O * A * (M + 1)), dtype=np.int64)
    for k in range(K):
        step = 1 if mutant == "frozen_step" else 1 + k
        d = ora.philox_draws(step, key)
        y = controller_draws(B, step, key)
        if mutant == "ctrl_is_env_y0":
            y = d["y"] if isinstance(d, dict) else d[0]
        if mutant == "obs_from_y0":
            d = (d[0], d[0], d[2], d[3])
        j = choose(y, thr[node, obs])
        a = j // M
        el0 = ora.elapsed.copy()
        o, r, term, trunc = ora.step(a, d)
        fin = term | trunc
        m["episodes"] += int(fin.sum())
        m["length_sum"] += int((el0[fin] + 1).sum())
        m["return_sum"] += float(r.astype(np.float64).sum())
        m["env_steps"] += B
        for name, x in zip(planes, (o, a.astype(np.int32), node.astype(np.uint8), r, term, trunc)):
            planes[name].append(x)
        nxt = j % M if mutant == "node_kept" else np.where(fin, 0, j % M)
        cell = ((node * O + obs) * A + a) * (M + 1) + np.where(fin, M, nxt)
        hist[k] = np.bincount(cell, minlength=hist.shape[1])
        obs, node = o.astype(np.int64), nxt
    planes = {n: np.stack(x) for n, x in planes.items()}
    counts, ret_q, flagged = controller_stats(M, O, A, obs0, planes, node, GAMMA)
    assert not flagged
    return hist, m, dict(counts=counts, ret_q=ret_q)


# ------------------------------------------------------------------ 1. brute force ----
def enumerate_paths(model, C, K, gamma, boot):
    """Every path (choice, s', o' or the reset's (s0, o0)) of K steps with its probability, in plain Python: the same
    outputs as `exact_law.evaluate`, as dense arrays."""
    S, A, O, TL = model.S, model.A, model.O, model.time_limit
    M = C.shape[0]
    out = dict(p=np.zeros((K, M, O, A, M + 1)), g1=np.zeros((K, M, O, A, M + 1)), g2=np.zeros((K, M, O, A, M + 1)),
               r1=np.zeros(K), r2=np.zeros(K), end=np.zeros(K), len1=np.zeros(K), len2=np.zeros(K))
    starts = [(model.start[s] * model.reset_obs[s, o], s, o) for s in range(S) for o in range(O)
              if model.start[s] * model.reset_obs[s, o] > 0]

    def leaf(prob, s, hist):
        G = boot[s]
        for k in range(K - 1, -1, -1):
            cell, rew, ended, length = hist[k]
            G = rew if ended else rew + gamma * G
            out["p"][(k,) + cell] += prob
            out["g1"][(k,) + cell] += prob * G
            out["g2"][(k,) + cell] += prob * G * G
            out["r1"][k] += prob * rew
            out["r2"][k] += prob * rew * rew
            if ended:
                out["end"][k] += prob
                out["len1"][k] += prob * length
                out["len2"][k] += prob * length * length

    def walk(prob, s, e, o, n, hist):
        if len(hist) == K:
            return leaf(prob, s, hist)
        for a in range(A):
            for n1 in range(M):
                pc = C[n, o, a, n1]
                for s1 in range(S):
                    pt = pc * model.T[s, a, s1]
                    if pt == 0:
                        continue
                    rew = model.R[s, a, s1]
                    if model.terminal[s1] or e + 1 >= TL:
                        for q, s0, o0 in starts:
                            walk(prob * pt * q, s0, 0, o0, 0, hist + [((n, o, a, M), rew, True, e + 1)])
                    else:
                        for o1 in range(O):
                            pz = model.Z[a, s1, o1]
                            if pz > 0:
                                walk(prob * pt * pz, s1, e + 1, o1, n1, hist + [((n, o, a, n1), rew, False, 0)])

    for q, s0, o0 in starts:
        walk(q, s0, 0, o0, 0, [])
    return out


@pytest.mark.parametrize("terminal,boot", [((False, False), None), ((False, True), (3.0, -7.0))],
                         ids=["tiger", "tiger_terminal_bootstrap"])
def test_passes_equal_brute_force_enumeration(terminal, boot):
    """Tiger, M = 2, K = 3, time_limit = 2: as it is (every episode is truncated), and with the second state terminal
    and a bootstrap value per state, so that terminations and G_K enter."""
    from gym_po_amd import row_thresholds
    from exact_law_cases import pomdp_tables
    T, Z, R, start, _, reset_obs = pomdp_tables("tiger")
    if terminal[1]:
        start = np.array([1.0, 0.0])
        T = T.copy()
        T[0, 0] = (0.75, 0.25)  # listening can now end the episode
    model = exact_law.Model(row_thresholds(T), row_thresholds(Z), row_thresholds(start), row_thresholds(reset_obs), R,
                            terminal, 2)
    thr = controller(2, 2, 3, seed=1)
    K, gamma = 3, 0.95
    ex = exact_law.evaluate(model, thr, K, gamma, boot)
    want = enumerate_paths(model, exact_law.integer_law(thr).reshape(2, 2, 3, 2), K, gamma,
                           np.zeros(2) if boot is None else np.asarray(boot))
    assert abs(want["p"].sum(axis=(1, 2, 3, 4)) - 1.0).max() < 1e-12 and want["end"].max() > 0
    assert (want["end"].min() > 0) == terminal[1]  # without a terminal state only the time limit ends an episode
    for name in ("p", "g1", "g2", "r1", "r2", "end", "len1", "len2"):
        np.testing.assert_allclose(getattr(ex, name), want[name], rtol=0, atol=1e-12 * max(1.0, abs(want[name]).max()),
                                   err_msg=name)
    assert np.array_equal(ex.p == 0, want["p"] == 0)  # a cell is impossible in both or in neither
    # E[G_0] two ways: through the cells and through V_0 under the reset law
    assert abs(ex.g1[0].sum() - (ex.law[0] * ex.V0).sum()) < 1e-12
    assert abs(ex.g2[0].sum() - (ex.law[0] * ex.W0).sum()) < 1e-9


# ------------------------------------------------------------------ 2. lowerings ----
def random_rows(shape, seed):
    rng = np.random.default_rng(seed)
    p = rng.random(shape) ** 3 * (rng.random(shape) > 0.4)
    p[..., 1] += 0.01  # no all-zero row; first and last entries are zero in some rows
    return p


def test_lowerings_keep_the_law_within_two_units():
    from gym_po_amd import row_thresholds
    from gym_po_amd.controller import controller_thresholds
    p = random_rows((500, 23), seed=0)
    p /= p.sum(-1, keepdims=True)
    q = exact_law.integer_law(row_thresholds(p))
    assert (p == 0).any() and (p[:, 0] == 0).any() and (p[:, -1] == 0).any()
    assert np.abs(q - p).max() <= 2.0 ** -30 and (q[p == 0] == 0).all() and (q[p >= 2.0 ** -30] > 0).all()
    assert (q.sum(-1) == 1.0).all()  # exact: multiples of 2^-31
    c = random_rows((4, 50, 5, 4), seed=1)
    c /= c.sum((-1, -2), keepdims=True)
    qc = exact_law.integer_law(controller_thresholds(c)).reshape(c.shape)
    assert np.abs(qc - c).max() <= 2.0 ** -30 and (qc[c == 0] == 0).all() and (qc.sum((-1, -2)) == 1.0).all()
    with pytest.raises(AssertionError):
        exact_law.integer_law(np.array([5, 3, 1 << 31]))
    with pytest.raises(AssertionError):
        exact_law.integer_law(np.array([5, 7, (1 << 31) - 1]))


def test_rocksample_tables_state_the_scalar_rule():
    """`rocksample_tables` against the one-env statement of the rules (rocksample_oracle.scalar_step), for every
    state and action at the two ends of the check draw and on both sides of the sensor threshold: the same next state,
    reward and termination, and the same reading law. (The law, not the draw's intervals: the rule reads GOOD on a bad
    rock for the draws at or above the threshold, a table row counts thresholds from 0 up.)"""
    from rocksample_oracle import BAD, GOOD, scalar_step
    top = 1 << 31
    for name in ("rs_cell", "rs_sensor"):
        sp, model = CASES[name].spec, CASES[name].model
        n_mask = 1 << sp.k
        trans, obs_thr = model.tables[0].astype(np.int64), model.tables[1].astype(np.int64)
        assert model.S == sp.H * sp.W * n_mask + 1 and model.A == 5 + sp.k and model.terminal.sum() == 1
        assert len(set(sp.rewards.values())) == 7
        for cell in range(sp.H * sp.W):
            for mask in range(n_mask):
                s = cell * n_mask + mask
                for a in range(model.A):
                    t = int(sp.thr[cell, a - 5]) if a >= 5 else top
                    n_good = 0  # the number of draws that read GOOD, from the rule's two intervals [0, t), [t, 2^31)
                    for lo, hi in ((0, t), (t, top)):
                        if lo == hi:
                            continue
                        seen = set()
                        for y in (lo, hi - 1):
                            c1, m1, _, obs, rew, term, trunc = scalar_step(sp, cell, mask, 0, a, y, 0)
                            s1 = int((y >= trans[s, a]).sum())
                            assert not trunc and term == bool(model.terminal[s1])
                            assert model.R[s, a, s1] == rew
                            if not term:
                                assert s1 == c1 * n_mask + m1
                                base = c1 * 3 if sp.obs_cell else 0
                                assert obs - base in ((GOOD, BAD) if a >= 5 else (0,))
                                seen.add(obs - base)
                        assert len(seen) <= 1  # one reading per interval
                        n_good += (hi - lo) * (seen == {GOOD})
                    if s1 != model.S - 1:
                        law = np.diff(obs_thr[a, s1], prepend=0)
                        want = np.zeros(model.O, dtype=np.int64)
                        want[base:base + 3] = (top, 0, 0) if a < 5 else (0, n_good, top - n_good)
                        assert np.array_equal(law, want), (cell, mask, a)
        assert model.start.sum() == 1.0 and (model.start[model.start > 0] == 1.0 / n_mask).all()
        assert np.flatnonzero(model.start).tolist() == [sp.init_cell * n_mask + i for i in range(n_mask)]
        init_obs = sp.init_cell * 3 if sp.obs_cell else 0
        assert (model.reset_obs[:, init_obs] == 1.0).all()


# ------------------------------------------------------------------ 3. the oracles, closed loop ----
# "m5_global" differs from "m5" in the device's memory paths only: the oracle has one run for both
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if not CASES[n].knobs])
def test_oracle_closed_loop_samples_the_exact_law(name):
    case = CASES[name]
    hist, metrics, stats = closed_loop(case, case.B)
    B = case.B
    assert np.array_equal(stats["counts"].reshape(-1), hist.sum(0)) and stats["counts"].sum() == B * case.K
    rep = exact_law.assert_law(hist, metrics, stats, case.exact(), B)
    print(f"\n{name}: B = {B}, " + ", ".join(f"{k} {v:.3g}" for k, v in rep.items()))
    assert rep["cells"] >= 100 and metrics["episodes"] > 0


# ------------------------------------------------------------------ 4. teeth ----
# Every mutant is rejected on Tiger; the other pairs show that the native kinds' tests bite too. RockSample under
# "ctrl_is_env_y0" is left out because it is not rejected (largest |z| 5.3): the word only decides whether a CHECK reads
# right, and under a fair mask the reading itself stays a fair coin whatever the word, so the error shows only through
# the agreement of repeated checks and the SAMPLE rewards after them, which a random controller hardly uses.
TEETH = [(m, "tiger") for m in MUTANTS] + [
    ("obs_from_y0", "m5"), ("ctrl_is_env_y0", "m5"), ("node_kept", "rs_cell"), ("frozen_step", "rs_cell"),
    ("ctrl_is_env_y0", "hh_hansen_p13")]


@pytest.mark.parametrize("mutant,name", TEETH)
def test_wrong_closed_loops_are_rejected(mutant, name):
    case = CASES[name]
    hist, metrics, stats = closed_loop(case, case.B, mutant)
    with pytest.raises(AssertionError) as e:
        exact_law.assert_law(hist, metrics, stats, case.exact(), case.B)
    print(f"\n{mutant} on {name}: {str(e.value)[:200]}")
