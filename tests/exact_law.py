"""REFERENCE / TEST INFRASTRUCTURE — exact policy evaluation of a finite POMDP under a finite-state controller, and
the statistical comparison of a closed-loop rollout against it.

Plain numpy, float64. Nothing here is imported from the numpy oracles of the kernels, and nothing here knows which
Philox word decides what: the only inputs are the integer threshold tables a handle is configured with and the
controller's threshold table. From them the law of every stored plane at every step of `rollout_controller`, and the
expectation and variance of every entry of `controller_statistics` and `metrics`, are small linear-algebra
computations. A kernel (or an oracle) whose draws are reused, correlated, stuck or skewed samples another chain.

The chain. The joint state is x = (s, elapsed, last obs, node). After reset() its law is start x reset_obs with
elapsed 0 and node 0. A step draws the choice (a, n') from the controller's row of (node, obs), then s' from T[s, a];
the step ends iff terminal[s'] or elapsed + 1 >= time_limit; if it ended, x is redrawn from the reset law (node 0),
else x = (s', elapsed + 1, o' ~ Z[a, s'], n').

Sizes. The largest arrays are the joint of a step, [S, TL, O, M, A, M] doubles, and the branch on the next state,
[S, TL, A, M, S] doubles (TL = time_limit). For the largest model used (S = 37, A = 3, O = 21, M = 2, TL = 9) that is
83,916 and 73,926 doubles; Heaven-Hell's "t3" maze under the Hansen obs (S = 18, O = 48, M = 2, A = 4, TL = 8) has
110,592 and 20,736. Every model of the tests stays four orders of magnitude below 10^7 doubles, so the obs is kept as
a coordinate even where it is a function of the state.
"""
import numpy as np

TOP = 1 << 31


def integer_law(thr):
    """Threshold rows (last axis; nondecreasing, ending at 2^31) -> the law the device samples from them: a 31-bit
    draw y picks #{i : y >= thr[i]}, so outcome i has the y of [thr[i - 1], thr[i]), thr[-1] = 0. The first
    differences are taken in int64; the division by 2^31 is exact in float64."""
    t = np.asarray(thr).astype(np.int64)
    d = np.diff(t, axis=-1, prepend=0)
    assert (d >= 0).all() and (t[..., -1] == TOP).all(), "not a threshold row"
    return d / float(TOP)


class Model:
    """The integer tables of a handle as float64 laws: T [S, A, S], Z [A, S, O], start [S], reset_obs [S, O], R
    [S, A, S], terminal bool [S], time_limit."""

    def __init__(self, trans_thr, obs_thr, start_thr, reset_obs_thr, reward, terminal, time_limit):
        self.tables = (np.asarray(trans_thr), np.asarray(obs_thr), np.asarray(start_thr), np.asarray(reset_obs_thr))
        self.T, self.Z = integer_law(trans_thr), integer_law(obs_thr)
        self.start, self.reset_obs = integer_law(start_thr), integer_law(reset_obs_thr)
        self.R = np.asarray(reward, dtype=np.float64)
        self.terminal = np.asarray(terminal).astype(bool)
        self.time_limit = int(time_limit)
        self.S, self.A, _ = self.T.shape
        self.O = self.Z.shape[2]
        assert self.Z.shape == (self.A, self.S, self.O) and self.start.shape == (self.S,)
        assert self.reset_obs.shape == (self.S, self.O) and self.R.shape == (self.S, self.A, self.S)
        assert self.terminal.shape == (self.S,) and self.time_limit >= 1


class Exact:
    """What `evaluate` returns, for k = 0..K-1 (cells: [M, O, A, M + 1], the last column = the step ended the episode):
    p [K, cells]      P(an env is in the cell at step k)
    g1, g2 [K, cells] E[G_k 1[cell at k]], E[G_k^2 1[cell at k]]
    r1, r2 [K]        E[r_k], E[r_k^2]
    end [K]           P(step k ends an episode)
    len1, len2 [K]    E[L 1[ended]], E[L^2 1[ended]], L = the length credited (elapsed + 1)
    gmax              the largest |G| the rewards allow over K steps (the bootstrap included)
    law [K]           the law of x before step k, [S, TL, O, M] (kept for the brute-force pin)."""


def evaluate(model, ctrl_thr, K, gamma=1.0, bootstrap=None):
    """Forward pass (the cell laws, the reward moments, the episode ends) and backward pass (V_k(x) = E[G_k | x],
    W_k(x) = E[G_k^2 | x] with G_k = r + gamma [not ended] G_{k+1} and G_K = bootstrap[s] or 0) of K closed-loop steps
    after reset(). ctrl_thr: the controller's thresholds [M, O, A * M], entry j = a * M + n'."""
    m = model
    S, A, O, TL = m.S, m.A, m.O, m.time_limit
    ctrl_thr = np.asarray(ctrl_thr)
    M = ctrl_thr.shape[0]
    assert ctrl_thr.shape == (M, O, A * M)
    C = integer_law(ctrl_thr).reshape(M, O, A, M)  # [n, o, a, n']
    Ca = C.sum(3)
    T, Z, R = m.T, m.Z, m.R
    # go[e, s']: the step from elapsed e into s' does not end the episode. Entries of T are multiples of 2^-31, so the
    # sums of T against 0 / 1 weights below are exact: a probability that is 0 or 1 is so exactly.
    go = np.outer((np.arange(TL) + 1 < TL).astype(np.float64), (~m.terminal).astype(np.float64))
    p_go = np.einsum("sat,et->sea", T, go)
    p_end = np.einsum("sat,et->sea", T, 1.0 - go)
    reset = np.zeros((S, TL, O, M))
    reset[:, 0, :, 0] = m.start[:, None] * m.reset_obs
    r1_sa, r2_sa = (T * R).sum(2), (T * R * R).sum(2)
    length = np.arange(TL) + 1.0

    ex = Exact()
    ex.K, ex.M, ex.O, ex.A, ex.gamma = K, M, O, A, float(gamma)
    ex.p = np.zeros((K, M, O, A, M + 1))
    ex.r1, ex.r2, ex.end, ex.len1, ex.len2 = (np.zeros(K) for _ in range(5))
    ex.law = []
    mu = reset.copy()
    for k in range(K):
        ex.law.append(mu)
        w = np.einsum("seon,noam->seonam", mu, C)  # the joint of x and the choice
        u = w.sum((2, 3))  # [s, e, a, n']
        ex.p[k, ..., :M] = np.einsum("seonam,sea->noam", w, p_go)
        ex.p[k, ..., M] = np.einsum("seonam,sea->noa", w, p_end)
        usa = u.sum((1, 3))
        ex.r1[k], ex.r2[k] = (usa * r1_sa).sum(), (usa * r2_sa).sum()
        ended = (u.sum(3) * p_end).sum((0, 2))  # by elapsed
        ex.end[k], ex.len1[k], ex.len2[k] = ended.sum(), (ended * length).sum(), (ended * length ** 2).sum()
        x = np.einsum("seam,sat->seamt", u, T)  # branch on s'
        cont = np.einsum("seamt,et,ato->teom", x, go, Z)
        mu = ex.end[k] * reset
        mu[:, 1:] += cont[:, :-1]  # elapsed + 1 (the last elapsed never goes on)

    boot = np.zeros(S) if bootstrap is None else np.asarray(bootstrap, dtype=np.float64)
    assert boot.shape == (S,)
    V = np.broadcast_to(boot[:, None, None, None], (S, TL, O, M))
    W = V * V
    g = float(gamma)
    ex.g1, ex.g2 = np.zeros_like(ex.p), np.zeros_like(ex.p)
    tgo, tend = np.einsum("sat,et->seat", T, go), np.einsum("sat,et->seat", T, 1.0 - go)
    qe1, qe2 = np.einsum("seat,sat->sea", tend, R), np.einsum("seat,sat->sea", tend, R * R)
    qr1, qr2 = np.einsum("seat,sat->sea", tgo, R), np.einsum("seat,sat->sea", tgo, R * R)
    for k in range(K - 1, -1, -1):
        # the value of going on into (s', e + 1) under next node n', the obs integrated out: [a, n', s', e]
        EV, EW = np.zeros((A, M, S, TL)), np.zeros((A, M, S, TL))
        EV[..., :-1] = np.einsum("ato,teom->amte", Z, V)[..., 1:]
        EW[..., :-1] = np.einsum("ato,teom->amte", Z, W)[..., 1:]
        qc1 = qr1[..., None] + g * np.einsum("seat,amte->seam", tgo, EV)
        qc2 = (qr2[..., None] + 2.0 * g * np.einsum("seat,sat,amte->seam", tgo, R, EV)
               + g * g * np.einsum("seat,amte->seam", tgo, EW))
        mu = ex.law[k]
        ex.g1[k, ..., :M] = np.einsum("seon,noam,seam->noam", mu, C, qc1)
        ex.g2[k, ..., :M] = np.einsum("seon,noam,seam->noam", mu, C, qc2)
        ex.g1[k, ..., M] = np.einsum("seon,noa,sea->noa", mu, Ca, qe1)
        ex.g2[k, ..., M] = np.einsum("seon,noa,sea->noa", mu, Ca, qe2)
        V = np.einsum("noam,seam->seon", C, qc1) + np.einsum("noa,sea->seon", Ca, qe1)
        W = np.einsum("noam,seam->seon", C, qc2) + np.einsum("noa,sea->seon", Ca, qe2)
    ex.V0, ex.W0 = V, W
    ex.gmax = float(np.abs(R).max() * sum(g ** j for j in range(K)) + g ** K * np.abs(boot).max())
    return ex


# ---------------------------------------------------------------------------------------------------------------
# The comparison. Envs are independent, so the histogram of step k over the cells is Multinomial(B, p_k) and every
# statistic is a sum over envs of i.i.d. bounded variables whose mean and variance `evaluate` gives.
#
# Z = 6 is derived, not measured: a case tests 10^3 to 10^5 cells, the Gaussian tail beyond 6 sigma is 2e-9 per cell,
# and the floor of 100 expected visits keeps the Poisson skew negligible at that distance. Per step, the cells below
# the floor are pooled into one cell that is tested the same way, so nothing is left out. Sums over the K steps use
# sigma(sum X_k) <= sum sigma(X_k), which needs no covariance between steps.
Z_BOUND = 6.0
FLOOR = 100.0
COVERAGE = 0.85


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _check(name, got, mean, sd, extra=0.0):
    """|got - mean| <= Z_BOUND sd + extra, elementwise. Returns the largest |z| = |got - mean| / sd (0 where sd is 0:
    there the test is |got - mean| <= extra)."""
    got, mean, sd = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (got, mean, sd))
    dev = np.abs(got - mean)
    ok = dev <= Z_BOUND * sd + extra
    z = np.divide(dev, sd, out=np.zeros_like(dev), where=sd > 0)
    if not ok.all():
        i = int(np.argmax(np.where(ok, -1.0, z + 1.0)))
        raise AssertionError(f"{name}: entry {i} is {got[i]:.10g}, the exact law gives {mean[i]:.10g} with sigma "
                             f"{sd[i]:.6g} (|z| = {z[i]:.2f} > {Z_BOUND}); {int((~ok).sum())} of {ok.size} entries "
                             "fail")
    return float(z.max()) if z.size else 0.0


def _with_pool(big, x):
    """The entries of x (last axis) where `big`, then the sum of the others."""
    return np.append(x[big], x[~big].sum())


def assert_law(hist_k, metrics, stats, exact, B):
    """hist_k int [K, cells]: per step the number of envs in each controller table cell ((n O + o) A + a) (M + 1) + c;
    metrics: the dict of metrics() after the K steps since reset(); stats: {"counts", "ret_q"} of
    controller_statistics over the K planes with gamma = exact.gamma and no bootstrap; exact: `evaluate`'s result.
    Raises AssertionError naming the first statistic outside its bound; returns the largest |z| seen per family."""
    from gym_po_amd.controller import stats_returns
    K = exact.K
    p = exact.p.reshape(K, -1)
    g1, g2 = exact.g1.reshape(K, -1), exact.g2.reshape(K, -1)
    hist = _host(hist_k).astype(np.int64).reshape(K, -1)
    assert hist.shape == p.shape, (hist.shape, p.shape)
    assert (hist.sum(1) == B).all(), "a step's histogram does not hold every env"
    rep = {}
    # impossible cells
    bad = (p == 0) & (hist > 0)
    assert not bad.any(), (f"{int(bad.sum())} (step, cell) pairs of probability 0 were visited, the first: step, cell "
                           f"= {tuple(int(i[0]) for i in np.nonzero(bad))}")
    # the per-step law
    rep["cells"], rep["step"], rep["coverage"] = 0, 0.0, 1.0
    for k in range(K):
        big = B * p[k] >= FLOOR
        cov = float(p[k][big].sum())
        rep["coverage"] = min(rep["coverage"], cov)
        assert cov >= COVERAGE, f"step {k}: the individually tested cells carry {cov:.3f} of the mass, below {COVERAGE}"
        pk, hk = _with_pool(big, p[k]), _with_pool(big, hist[k])
        rep["step"] = max(rep["step"], _check(f"step {k} cell counts", hk, B * pk, np.sqrt(B * pk * (1.0 - pk))))
        rep["cells"] += int(big.sum()) + 1
    # the summed tables, every cell (the step-wise sigmas add up to a bound wide enough for the rare cells too: the
    # largest |z| of a cell below the floor was 1.6 over all cases)
    counts = _host(stats["counts"]).astype(np.int64).reshape(-1)
    ret = stats_returns(stats["ret_q"]).reshape(-1)
    assert counts.shape == p[0].shape and (counts >= 0).all()
    rep["counts"] = _check("summed counts", counts, B * p.sum(0), np.sqrt(B * p * (1.0 - p)).sum(0))
    # the return-to-go sums, with the rounding allowance of the device's arithmetic per visit: rint at 2^-20 (half a
    # unit) and K float32 steps of two roundings each on magnitudes up to gmax
    allowance = counts * (2.0 ** -21 + K * 2.0 ** -23 * exact.gmax)
    rep["returns"] = _check("return-to-go sums", ret, B * g1.sum(0),
                            np.sqrt(B * np.maximum(g2 - g1 * g1, 0.0)).sum(0), allowance)
    assert not ret[p.sum(0) == 0].any()
    # the metrics
    assert metrics["env_steps"] == B * K
    rep["episodes"] = _check("episodes", metrics["episodes"], B * exact.end.sum(),
                             np.sqrt(B * exact.end * (1.0 - exact.end)).sum())
    rep["length_sum"] = _check("length_sum", metrics["length_sum"], B * exact.len1.sum(),
                               np.sqrt(B * np.maximum(exact.len2 - exact.len1 ** 2, 0.0)).sum())
    rep["return_sum"] = _check("return_sum", metrics["return_sum"], B * exact.r1.sum(),
                               np.sqrt(B * np.maximum(exact.r2 - exact.r1 ** 2, 0.0)).sum())
    return rep
