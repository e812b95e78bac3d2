"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the build-defined belief filter and alpha-vector policy of the
tabular POMDP (csrc/pomdp.hip, include/gym_po_amd.h). The device is pinned to `filter_step` / `policy`
bit for bit, and these to the scalar one-env statements `scalar_filter_step` / `scalar_policy` in plain Python floats
cast through np.float32 at every operation (tests/test_belief_cpu.py). The restatement is dense: every entry of every
law takes part, zeros included.

Also here: a float64 Bayes filter from the exact integer law (the yardstick for the float32 rule's error) and the
calibration statistic that knows nothing of the rule text: among the envs whose belief gives state s probability p,
a fraction p must be in s.
"""
import numpy as np

from exact_law import integer_law

F = np.float32
SCALE = F(2.0 ** -31)


def threshold_law(thr):
    """p[i] = (float32)(uint32)(thr[i] - thr[i-1]) * 2^-31, thr[-1] = 0: one rounding, then an exact scale."""
    return np.diff(np.asarray(thr).astype(np.int64), axis=-1, prepend=0).astype(F) * SCALE


class Laws:
    """The float32 laws of a Spec / env (anything with the integer tables as attributes)."""

    def __init__(self, sp, prior=None):
        self.Tf, self.Zf = threshold_law(sp.trans_thr), threshold_law(sp.obs_thr)
        self.Rf = threshold_law(sp.reset_obs_thr)
        self.prior = threshold_law(sp.start_thr) if prior is None else np.asarray(prior, dtype=F)
        self.terminal = np.asarray(sp.terminal).astype(bool)
        self.S, self.A, _ = self.Tf.shape
        self.O = self.Zf.shape[2]


def wrap_actions(a, A):
    a = np.asarray(a, dtype=np.int64)
    a = np.where(a < 0, a + A, a)
    return np.clip(a, 0, A - 1)


def filter_step(lw, b, a, o, ended):
    """One filter step of E envs at once: b float32 [E, S], a (already wrapped) and o int [E], ended bool [E] ->
    (b' float32 [E, S], degenerate bool [E]). The loops over s are explicit, ascending, in float32."""
    b = np.asarray(b, dtype=F)
    a, o, ended = np.asarray(a, dtype=np.int64), np.asarray(o, dtype=np.int64), np.asarray(ended).astype(bool)
    E, S = b.shape
    # not ended: acc(s') = sum_s fl(b[s] Tf[s][a][s']), u = terminal ? +0 : fl(Zf[a][s'][o] acc)
    acc = np.zeros((E, S), dtype=F)
    for s in range(S):
        acc = (acc + (b[:, s, None] * lw.Tf[s][a]).astype(F)).astype(F)  # Tf[s][a]: [E, S'] rows of state s
    u_go = (lw.Zf[a, :, o] * acc).astype(F)
    u_go = np.where(lw.terminal[None, :], F(0), u_go).astype(F)
    # ended: u(s) = fl(prior[s] Rf[s][o])
    u_end = (lw.prior[None, :] * lw.Rf[:, o].T).astype(F)
    u = np.where(ended[:, None], u_end, u_go).astype(F)
    n = np.zeros(E, dtype=F)
    for s in range(S):
        n = (n + u[:, s]).astype(F)
    bad = ~((n > 0) & np.isfinite(n))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (u / n[:, None]).astype(F)
    out[bad] = lw.prior
    return out, bad


def policy(alpha, vec_action, b):
    """The piecewise-linear policy on beliefs b [E, S]: v_j = sum_s fl(b[s] alpha[j][s]) (ascending, float32), j* the
    first maximiser (replaced only on a strict >) -> (action, j*, v_j*)."""
    alpha = np.asarray(alpha, dtype=F)
    b = np.asarray(b, dtype=F)
    E, S = b.shape
    v = np.zeros((E, alpha.shape[0]), dtype=F)  # every vector at once; the sum over s stays sequential
    for s in range(S):
        v = (v + (b[:, s, None] * alpha[None, :, s]).astype(F)).astype(F)
    best_j = np.zeros(E, dtype=np.int64)
    best_v = v[:, 0].copy()
    for j in range(1, alpha.shape[0]):
        better = v[:, j] > best_v
        best_v = np.where(better, v[:, j], best_v).astype(F)
        best_j = np.where(better, j, best_j)
    return np.asarray(vec_action, dtype=np.int64)[best_j], best_j, best_v


def scalar_filter_step(lw, b, a, o, ended):
    """One env, one step, following the rule's wording: every product, sum and quotient is a Python float operation
    on float32 values cast back through np.float32 (a double operation on two float32 operands rounded to float32 is
    the correctly rounded float32 operation). -> (b' list of np.float32, degenerate)."""
    S = lw.S
    u = []
    if ended:
        for s in range(S):
            u.append(F(float(lw.prior[s]) * float(lw.Rf[s][o])))
    else:
        for s1 in range(S):
            acc = F(0.0)
            for s in range(S):
                acc = F(float(acc) + float(F(float(b[s]) * float(lw.Tf[s][a][s1]))))
            u.append(F(0.0) if lw.terminal[s1] else F(float(lw.Zf[a][s1][o]) * float(acc)))
    n = F(0.0)
    for s in range(S):
        n = F(float(n) + float(u[s]))
    if not (float(n) > 0.0) or not np.isfinite(n):
        return [F(x) for x in lw.prior], True
    return [F(float(u[s]) / float(n)) for s in range(S)], False


def scalar_policy(alpha, vec_action, b):
    best_j, best_v = 0, None
    for j in range(len(alpha)):
        v = F(0.0)
        for s in range(len(b)):
            v = F(float(v) + float(F(float(b[s]) * float(F(alpha[j][s])))))
        if best_v is None or float(v) > float(best_v):
            best_j, best_v = j, v
    return int(vec_action[best_j]), best_j, best_v


def reset_beliefs(lw, obs):
    """The beliefs after reset() / enable_belief(): the ended rule on each env's stored obs."""
    E = len(obs)
    return filter_step(lw, np.zeros((E, lw.S), dtype=F), np.zeros(E, dtype=np.int64), obs, np.ones(E, dtype=bool))


def filter_planes(lw, b, acts, obs, term, trunc):
    """filter_step over K stored steps of planes [K, E] -> (b', any degenerate step)."""
    bad_any = False
    for k in range(len(acts)):
        b, bad = filter_step(lw, b, wrap_actions(acts[k], lw.A), obs[k], np.asarray(term[k]).astype(bool)
                             | np.asarray(trunc[k]).astype(bool))
        bad_any |= bool(bad.any())
    return b, bad_any


# ------------------------------------------------------------------ float64 yardstick ----
class Laws64:
    """The exact integer laws as float64 (exact_law.integer_law): what a float64 Bayes filter multiplies."""

    def __init__(self, sp):
        self.Tf, self.Zf = integer_law(sp.trans_thr), integer_law(sp.obs_thr)
        self.Rf, self.prior = integer_law(sp.reset_obs_thr), integer_law(sp.start_thr)
        self.terminal = np.asarray(sp.terminal).astype(bool)


def predict64(lw, w, a):
    """sum_s w[e, s] T[s, a_e, s'] in float64 -> [E, S'] (a loop over s: no [E, S, S'] array)."""
    acc = np.zeros(w.shape, dtype=np.float64)
    for s in range(w.shape[1]):
        acc += w[:, s, None] * lw.Tf[s][a]
    return acc


def filter_step64(lw, b, a, o, ended):
    """The same Bayes step in float64 with numpy's own sums (no degenerate rule: the caller asserts n > 0)."""
    acc = predict64(lw, b, a)
    u_go = np.where(lw.terminal[None, :], 0.0, lw.Zf[a, :, o] * acc)
    u_end = lw.prior[None, :] * lw.Rf[:, o].T
    u = np.where(np.asarray(ended)[:, None], u_end, u_go)
    n = u.sum(-1)
    assert (n > 0).all()
    return u / n[:, None]


# ------------------------------------------------------------------ calibration ----
def calibration(beliefs, states):
    """The calibration statistic of one step: beliefs [E, S] (any float dtype), true states int [E]. Per state s the
    count #{e : state_e = s} against its mean sum_e b_e(s) and variance sum_e b_e(s)(1 - b_e(s)) under the claim that
    each env's state is drawn from its belief. Cells with variance >= 25 are tested alone, the rest pooled into one
    cell. -> dict(z: |count - mean| / sqrt(var) of every tested cell, cells, mass_alone: the share of the E envs'
    probability mass carried by the cells tested alone, min_true: the smallest belief any env holds on its own state)."""
    b = np.asarray(beliefs, dtype=np.float64)
    E, S = b.shape
    cnt = np.bincount(np.asarray(states, dtype=np.int64), minlength=S).astype(np.float64)
    mean, var = b.sum(0), (b * (1.0 - b)).sum(0)
    alone = var >= 25.0
    z = list(np.abs(cnt[alone] - mean[alone]) / np.sqrt(var[alone]))
    # the pooled cell: the count of envs in any pooled state; per env a Bernoulli of probability q_e = its pooled mass
    q = b[:, ~alone].sum(-1)
    pv = (q * (1.0 - q)).sum()
    if pv > 0:
        z.append(abs(cnt[~alone].sum() - q.sum()) / np.sqrt(pv))
    else:
        assert cnt[~alone].sum() == round(q.sum()), "a pooled cell without variance must be met exactly"
    return dict(z=np.asarray(z), cells=len(z), mass_alone=float(mean[alone].sum() / E),
                min_true=float(b[np.arange(E), np.asarray(states, dtype=np.int64)].min()))


def assert_calibrated(steps, what=""):
    """`steps`: (beliefs [E, S], states [E]) per step. Asserts the calibration bound of DESIGN.md §6r on every cell:
    |count - mean| <= 6 sqrt(var) (fewer than 10^4 cells over the whole suite, Gaussian tail 2e-9: §6q's derivation),
    the cells tested alone carry >= 85 % of the mass, and no env holds belief 0 on its true state. Prints and returns
    the figures."""
    zmax, cells, mass, mtrue = 0.0, 0, 1.0, 1.0
    for k, (b, s) in enumerate(steps):
        c = calibration(b, s)
        zmax, cells = max(zmax, float(c["z"].max())), cells + c["cells"]
        mass, mtrue = min(mass, c["mass_alone"]), min(mtrue, c["min_true"])
        assert c["min_true"] > 0, f"{what} step {k}: an env holds belief 0 on its true state"
        assert c["mass_alone"] >= 0.85, f"{what} step {k}: the cells tested alone carry {c['mass_alone']:.3f} of the mass"
        assert c["z"].max() <= 6.0, f"{what} step {k}: |z| = {c['z'].max():.2f} over {c['cells']} cells"
    print(f"calibration {what}: max |z| {zmax:.2f} over {cells} cells, least mass alone {mass:.3f}, "
          f"least belief on the true state {mtrue:.3g}")
    return dict(zmax=zmax, cells=cells, mass=mass, min_true=mtrue)
