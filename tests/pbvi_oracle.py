"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the build-defined point-based value backup of the tabular POMDP
(csrc/pomdp_backup.hip, include/gym_po_amd.h gp_belief_backup). The device is pinned to `backup` bit for
bit, and `backup` to the scalar one-point statement `scalar_backup`, written line by line from the rule text in plain
Python floats cast through np.float32 at every operation (tests/test_pbvi_cpu.py). Both are dense: every entry of
every law takes part, zeros and terminal states included.

Also here: a float64 exhaustive enumeration of the exact value function's vectors (Monahan 1982) from the integer
thresholds, which knows nothing of the backup's order of operations, and the error bound its comparison uses.
"""
import numpy as np

from belief_oracle import Laws, Laws64

F = np.float32


class Model:
    """What the backup reads of a Spec / env: the filter's float32 laws, the rewards, the terminal flags."""

    def __init__(self, sp):
        lw = Laws(sp)
        self.Tf, self.Zf, self.terminal = lw.Tf, lw.Zf, lw.terminal
        self.reward = np.asarray(sp.reward, dtype=F)
        self.S, self.A, self.O = lw.S, lw.A, lw.O
        self.n_states = self.S


def first_max(v):
    """The first maximiser along the last axis, replaced only on a strict >: (index, value)."""
    best_i = np.zeros(v.shape[:-1], dtype=np.int64)
    best_v = v[..., 0].copy()
    for i in range(1, v.shape[-1]):
        better = v[..., i] > best_v
        best_v = np.where(better, v[..., i], best_v)
        best_i = np.where(better, i, best_i)
    return best_i, best_v


def backup(md, points, alpha, gamma):
    """The backup of P points at once: points float32 [P, S], alpha float32 [N, S], gamma -> a dict of alpha [P, S],
    actions int32 [P], value float32 [P]. The loops over every summed index are explicit, ascending, in float32; the
    rest is vectorised."""
    b = np.asarray(points, dtype=F)
    al = np.asarray(alpha, dtype=F)
    g = F(gamma)
    P, S = b.shape
    A, O, N = md.A, md.O, al.shape[0]
    term = md.terminal
    # 1. acc_a(s') = sum_s fl(b[s] Tf[s][a][s'])
    acc = np.zeros((P, A, S), dtype=F)
    for s in range(S):
        acc = (acc + (b[:, s, None, None] * md.Tf[s][None]).astype(F)).astype(F)
    # 2. u(s') = terminal ? +0 : fl(Zf[a][s'][o] acc_a(s')); score_j = sum_s' fl(u(s') alpha[j][s']); j* first maximiser
    jst = np.zeros((P, A, O), dtype=np.int64)
    for a in range(A):
        u = (md.Zf[a][None] * acc[:, a, :, None]).astype(F)  # [P, S', O]
        u = np.where(term[None, :, None], F(0), u).astype(F)
        score = np.zeros((P, O, N), dtype=F)
        for s1 in range(S):
            score = (score + (u[:, s1, :, None] * al[None, None, :, s1]).astype(F)).astype(F)
        jst[:, a] = first_max(score)[0]
    # 3. w_a(s') = terminal ? +0 : sum_o fl(Zf[a][s'][o] alpha[j*(a, o)][s'])
    w = np.zeros((P, A, S), dtype=F)
    cols = np.arange(S)
    for o in range(O):
        w = (w + (md.Zf[None, :, :, o] * al[jst[:, :, o][:, :, None], cols[None, None, :]]).astype(F)).astype(F)
    w = np.where(term[None, None, :], F(0), w).astype(F)
    # 4. r_a(s) = sum_s' fl(Tf reward); h_a(s) = sum_s' fl(Tf w_a(s')); beta_a(s) = fl(r + fl(gamma h))
    Ta = md.Tf.transpose(1, 0, 2)  # [A, S, S']
    Ra = md.reward.transpose(1, 0, 2)
    r = np.zeros((A, S), dtype=F)
    h = np.zeros((P, A, S), dtype=F)
    for s1 in range(S):
        r = (r + (Ta[:, :, s1] * Ra[:, :, s1]).astype(F)).astype(F)
        h = (h + (Ta[None, :, :, s1] * w[:, :, None, s1]).astype(F)).astype(F)
    beta = (r[None] + (g * h).astype(F)).astype(F)
    # 5. v_a = sum_s fl(b[s] beta_a(s)); a* first maximiser
    v = np.zeros((P, A), dtype=F)
    for s in range(S):
        v = (v + (b[:, s, None] * beta[:, :, s]).astype(F)).astype(F)
    a_star, v_star = first_max(v)
    return {"alpha": beta[np.arange(P), a_star].astype(F), "actions": a_star.astype(np.int32), "value": v_star.astype(F)}


def scalar_backup(md, b, alpha, gamma):
    """One point, following the rule's wording: every product and sum is a Python float operation on float32 values
    cast back through np.float32 (a double operation on two float32 operands rounded to float32 is the correctly
    rounded float32 operation). -> (beta list of np.float32, a*, v)."""
    S, A, O, N = md.S, md.A, md.O, len(alpha)
    mul = lambda x, y: F(float(x) * float(y))  # noqa: E731
    add = lambda x, y: F(float(x) + float(y))  # noqa: E731
    g = F(gamma)
    best_a, best_v, best_beta = 0, None, None
    for a in range(A):
        acc = []
        for s1 in range(S):
            t = F(0.0)
            for s in range(S):
                t = add(t, mul(b[s], md.Tf[s][a][s1]))
            acc.append(t)
        jstar = []
        for o in range(O):
            u = [F(0.0) if md.terminal[s1] else mul(md.Zf[a][s1][o], acc[s1]) for s1 in range(S)]
            bj, bs = 0, None
            for j in range(N):
                score = F(0.0)
                for s1 in range(S):
                    score = add(score, mul(u[s1], F(alpha[j][s1])))
                if bs is None or float(score) > float(bs):
                    bj, bs = j, score
            jstar.append(bj)
        w = []
        for s1 in range(S):
            t = F(0.0)
            if not md.terminal[s1]:
                for o in range(O):
                    t = add(t, mul(md.Zf[a][s1][o], F(alpha[jstar[o]][s1])))
            w.append(t)
        beta = []
        for s in range(S):
            r, h = F(0.0), F(0.0)
            for s1 in range(S):
                r = add(r, mul(md.Tf[s][a][s1], md.reward[s][a][s1]))
                h = add(h, mul(md.Tf[s][a][s1], w[s1]))
            beta.append(add(r, mul(g, h)))
        v = F(0.0)
        for s in range(S):
            v = add(v, mul(b[s], beta[s]))
        if best_v is None or float(v) > float(best_v):
            best_a, best_v, best_beta = a, v, beta
    return best_beta, best_a, best_v


# ------------------------------------------------------------------ the independent statement ----
class Model64:
    """The exact integer laws as float64, the rewards and the terminal mask."""

    def __init__(self, sp):
        lw = Laws64(sp)
        self.T, self.Z, self.live = lw.Tf, lw.Zf, 1.0 - lw.terminal.astype(np.float64)
        self.R = np.asarray(sp.reward, dtype=np.float64)
        self.S, self.A, _ = self.T.shape
        self.O = self.Z.shape[2]


def monahan(m, gamma, horizon):
    """Gamma_0 = {0}, Gamma_h = {r_a + gamma sum_o g_{a,o}^{j_o}} over every action and every choice of one vector of
    Gamma_{h-1} per obs, with g_{a,o}^j(s) = sum_s' T[s, a, s'] Z[a, s', o] live[s'] alpha_j(s'): every vector of the
    exact h-step value function, unpruned, in float64 with numpy's own sums. -> [Gamma_0, ..., Gamma_horizon]."""
    sets = [np.zeros((1, m.S))]
    r = (m.T * m.R).sum(-1)  # [S, A]
    for _ in range(horizon):
        prev = sets[-1]
        new = []
        for a in range(m.A):
            # g[o, j, s]
            g = np.einsum("st,to,jt->ojs", m.T[:, a, :], m.Z[a] * m.live[:, None], prev)
            tot = np.zeros((1, m.S))
            for o in range(m.O):  # the cross sum over the obs
                tot = (tot[:, None, :] + g[o][None, :, :]).reshape(-1, m.S)
            new.append(r[:, a][None, :] + gamma * tot)
        sets.append(np.concatenate(new))
    return sets


def abs_bound(md, points, alpha, gamma):
    """The a-priori bound on |float32 backup - exact arithmetic on the integer laws| -> (float64 [P]:
    on the value at each point; float64: on every entry of the vector against the exact vector of the same choices).
    The standard bound of a sequential sum (Higham 2002, §3.1, §4.2): a float32 sum of n terms that each carry k
    roundings of their own is off by at most g(n - 1 + k) sum |terms|, g(m) = m u / (1 - m u), u = 2^-24. A float law
    is the exact law with one rounding; `alpha` given as float64 is rounded once on its way in. Composed over the five
    steps with every magnitude replaced by its upper bound: laws sum to <= `one`, |alpha| <= M, |reward| <= Rm."""
    u = 2.0 ** -24
    S, O = md.S, md.O
    g = lambda k: k * u / (1.0 - k * u)  # noqa: E731
    M = float(np.abs(np.asarray(alpha, dtype=np.float64)).max())
    Rm = float(np.abs(md.reward.astype(np.float64)).max())
    b1 = np.abs(np.asarray(points, dtype=np.float64)).sum(-1)
    one = 1.0 + g(S + O)  # the row sum of a float32 law
    # 3. w_a(s') = sum_o fl(Zf alpha[j*]): O - 1 additions; per term the law, alpha's cast, the product
    w_mag = M * one
    w_err = g(O + 2) * w_mag
    # 4. h_a(s) = sum_s' fl(Tf w): the error of w under weights that sum to <= one, S - 1 additions, law and product;
    #    r_a(s) the same with exact rewards
    h_err = w_err * one + g(S + 1) * (w_mag + w_err) * one
    r_err = g(S + 1) * Rm * one
    #    beta = fl(r + fl(gamma h)): two roundings more
    beta_mag = (Rm + gamma * w_mag * one) * one
    beta_err = r_err + gamma * h_err + g(2) * (beta_mag + r_err + gamma * h_err)
    # 5. v_a = sum_s fl(b[s] beta_a(s)): S - 1 additions and the product
    v_err = (beta_err + g(S) * (beta_mag + beta_err)) * b1
    # 2. j*(a, o) is chosen on float32 scores: against the exact maximiser the chosen vector loses at most twice a
    #    score's error. score_j = sum_s' fl(fl(Zf acc(s')) alpha_j(s')) with acc(s') itself a sum of S products: at most
    #    (S - 1) + (S - 1) additions and 2 + 2 + 2 roundings in the factors of a term; sum over o of sum |terms| is at
    #    most M one^2 |b|_1. It enters the value through gamma.
    pick_err = gamma * 2.0 * g(2 * S + 4) * M * one * one * b1
    return v_err + pick_err, beta_err
