"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the build-defined tabular POMDP rules (csrc/pomdp.hip header,
include/gym_po_amd.h gp_pomdp_config). There is no reference env: the device is pinned to this
restatement bit for bit, and this restatement to the scalar one-env statement `scalar_step` below
(tests/test_pomdp_cpu.py).

Draws: one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, TAG); with y_i = x_i >> 1, y0 picks the
next state from trans_thr[s][a], y1 the obs from obs_thr[a][s'] if the episode goes on; if the step ended it, y2 picks
the start state from start_thr and y3 the obs from reset_obs_thr[s0]. A pick is the count of thresholds <= y.
"""
import numpy as np

from oracle.philox import env_step_words, philox_key  # noqa: F401  (philox_key(seed): the key the draws take)

TAG = 0x706F6D64
TOP = 1 << 31

TIGER = """\
# The tiger problem (Kaelbling, Littman & Cassandra 1998), written out for these tests.
discount: 0.95
values: reward
states: tiger-left tiger-right
actions: listen open-left open-right
observations: hear-left hear-right

start: uniform

T: listen
identity
T: open-left
uniform
T: open-right
uniform

O: listen
0.85 0.15
0.15 0.85
O: open-left
uniform
O: open-right
uniform

R: listen : * : * : * -1
R: open-left : tiger-left : * : * -100
R: open-left : tiger-right : * : * 10
R: open-right : tiger-left : * : * 10
R: open-right : tiger-right : * : * -100
"""


class Spec:
    """What a handle is configured with: the integer tables, the rewards, the terminal flags, time_limit."""

    def __init__(self, trans_thr, obs_thr, start_thr, reset_obs_thr, reward, terminal, time_limit):
        self.trans_thr = np.asarray(trans_thr, dtype=np.int64)
        self.obs_thr = np.asarray(obs_thr, dtype=np.int64)
        self.start_thr = np.asarray(start_thr, dtype=np.int64)
        self.reset_obs_thr = np.asarray(reset_obs_thr, dtype=np.int64)
        self.reward = np.asarray(reward, dtype=np.float32)
        self.terminal = np.asarray(terminal).astype(bool)
        self.time_limit = int(time_limit)
        self.S, self.A, _ = self.trans_thr.shape
        self.O = self.obs_thr.shape[2]
        assert self.obs_thr.shape == (self.A, self.S, self.O) and self.start_thr.shape == (self.S,)
        assert self.reset_obs_thr.shape == (self.S, self.O) and self.reward.shape == (self.S, self.A, self.S)

    @classmethod
    def of_env(cls, env):
        return cls(env.trans_thr, env.obs_thr, env.start_thr, env.reset_obs_thr, env.reward, env.terminal,
                   env.time_limit)


def scalar_count(row, y):
    """#{i : y >= row[i]} in plain integers, one entry after the other."""
    n = 0
    for t in row:
        if y >= int(t):
            n += 1
    return n


def scalar_step(sp, s, elapsed, action, x0, x1, x2, x3):
    """One env, one step, in plain Python integers, following the rules' wording line by line; x0..x3 are the four
    words of the step's block. -> (state, elapsed, obs, reward, terminated, truncated)."""
    if action < 0:
        action += sp.A
    assert 0 <= action < sp.A
    y0, y1, y2, y3 = x0 >> 1, x1 >> 1, x2 >> 1, x3 >> 1
    s1 = min(scalar_count(sp.trans_thr[s][action], y0), sp.S - 1)
    reward = sp.reward[s][action][s1]
    terminated = bool(sp.terminal[s1])
    truncated = elapsed + 1 >= sp.time_limit
    if terminated or truncated:
        s0 = min(scalar_count(sp.start_thr, y2), sp.S - 1)
        obs = min(scalar_count(sp.reset_obs_thr[s0], y3), sp.O - 1)
        return s0, 0, obs, np.float32(reward), terminated, truncated
    obs = min(scalar_count(sp.obs_thr[action][s1], y1), sp.O - 1)
    return s1, elapsed + 1, obs, np.float32(reward), terminated, truncated


def count(rows, y):
    """#{i : y >= rows[..., i]} for y [...] and rows [..., L]."""
    return (np.asarray(y, dtype=np.int64)[..., None] >= rows).sum(-1)


class PomdpOracle:
    """B envs at once. State: state, elapsed, obs (the last observation), int64 [B]."""

    def __init__(self, B, spec):
        self.B, self.sp = B, spec
        self.state = np.zeros(B, dtype=np.int64)
        self.elapsed = np.zeros(B, dtype=np.int64)
        self.obs = np.zeros(B, dtype=np.int64)

    def philox_draws(self, step, key):
        return self.draws_of_words(*env_step_words(self.B, step, TAG, key))

    @staticmethod
    def draws_of_words(x0, x1, x2, x3):
        return tuple((np.asarray(x, dtype=np.uint64) >> np.uint64(1)).astype(np.int64) for x in (x0, x1, x2, x3))

    def _reset_draw(self, y2, y3):
        sp = self.sp
        s0 = np.minimum(count(sp.start_thr[None, :], y2), sp.S - 1)
        return s0, np.minimum(count(sp.reset_obs_thr[s0], y3), sp.O - 1)

    def reset(self, draws):
        self.state, self.obs = self._reset_draw(draws[2], draws[3])
        self.elapsed = np.zeros(self.B, dtype=np.int64)
        return self.obs.astype(np.int32)

    def step(self, actions, draws):
        sp = self.sp
        y0, y1, y2, y3 = draws
        a = np.asarray(actions, dtype=np.int64)
        a = np.where(a < 0, a + sp.A, a)
        assert ((a >= 0) & (a < sp.A)).all()
        s1 = np.minimum(count(sp.trans_thr[self.state, a], y0), sp.S - 1)
        rew = sp.reward[self.state, a, s1]
        term = sp.terminal[s1]
        el = self.elapsed + 1
        trunc = el >= sp.time_limit
        done = term | trunc
        s0, o0 = self._reset_draw(y2, y3)
        o1 = np.minimum(count(sp.obs_thr[a, s1], y1), sp.O - 1)
        self.state = np.where(done, s0, s1)
        self.obs = np.where(done, o0, o1)
        self.elapsed = np.where(done, 0, el)
        return self.obs.astype(np.int32), rew.astype(np.float32), term, trunc


def oracle_rollout(ora, acts, draws):
    """len(acts) oracle steps with draws(k): the stacked (obs, rew, term, trunc) and the four metrics the device
    accumulates (length_sum: the length of every episode that ended, i.e. its elapsed before the same-step reset)."""
    outs, m = [], dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)
    for k in range(len(acts)):
        el0 = ora.elapsed.copy()
        o, r, d, tr = ora.step(acts[k], draws(k))
        fin = d | tr
        m["episodes"] += int(fin.sum())
        m["length_sum"] += int((el0[fin] + 1).sum())
        m["return_sum"] += float(r.astype(np.float64).sum())
        m["env_steps"] += ora.B
        outs.append((o, r, d, tr))
    return [np.stack(x) for x in zip(*outs)], m


def random_model(S, A, O, seed, zero=0.35, n_terminal=1, dyadic=True):
    """(T, Z, R, start, terminal, reset_obs) of a random model: about `zero` of the entries of every law are exactly 0
    (the last entry of a row among them for some rows, so zero tails occur), rewards multiples of 0.25 in [-2, 2]
    (exact sums in any order), the last `n_terminal` states terminal and never start states."""
    rng = np.random.default_rng(seed)

    def law(*shape):
        p = rng.random(shape) ** 2 * (rng.random(shape) > zero)
        p[..., 0] += 0.05  # no all-zero row
        return p / p.sum(-1, keepdims=True)

    T, Z, reset_obs = law(S, A, S), law(A, S, O), law(S, O)
    terminal = np.zeros(S, dtype=bool)
    if n_terminal:
        terminal[S - n_terminal:] = True
    start = law(S)
    start[terminal] = 0.0
    start /= start.sum()
    R = rng.integers(-8, 9, (S, A, S)) * 0.25 if dyadic else rng.normal(size=(S, A, S))
    return T, Z, R.astype(np.float32), start, terminal, reset_obs
