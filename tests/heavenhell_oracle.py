"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the build-defined grid Heaven-Hell rules (csrc/heavenhell.hip
header, include/gym_po_amd.h gp_heavenhell_config). The reference's env is a MuJoCo ant
(gym_po/envs/ant_heaven_hell.py), which this build does not restate, so there is no reference parity to pin: the device
is pinned to this restatement bit for bit, and this restatement to the scalar one-env statement `scalar_step` below
(tests/test_heavenhell_cpu.py).

Draws: one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, TAG): y = x0 >> 1 decides whether the
action slips (y >= keep_thr), x1 picks the action it slips to, x2 the start cell of a reset, x3 & 1 its heaven side.
"""
import numpy as np

from oracle.philox import env_step_words, philox_key  # noqa: F401  (philox_key(seed): the key the draws take)

TAG = 0x6868656C
FREE, LEFT, RIGHT, PRIEST, START = 1, 2, 4, 8, 16
CHAR_FLAGS = {"#": 0, ".": FREE, "S": FREE | START, "L": FREE | LEFT, "R": FREE | RIGHT, "P": FREE | PRIEST}
N, E, S, W_ = 0, 1, 2, 3
TOP = 1 << 31
DEFAULT_REWARDS = dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=0.0, wall_reward=0.0)
T3 = ("LPR",
      "#.#",
      "#S#")


def hansen_code(H, W, flags, cell):
    """sum 2^i [neighbour i of `cell` is a free cell of the grid], i = N, E, S, W — one cell, plain integers."""
    row, col = divmod(cell, W)
    code = 0
    for i, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
        r, c = row + dr, col + dc
        if 0 <= r < H and 0 <= c < W and flags[r * W + c] & FREE:
            code |= 1 << i
    return code


class Spec:
    """What a handle is configured with: the maze in characters, the obs type, keep_thr, time_limit, the rewards."""

    def __init__(self, maze, obs_type="cell_signal", keep_thr=TOP, time_limit=500, **rewards):
        rows = [str(r) for r in maze]
        self.H, self.W = len(rows), len(rows[0])
        self.flags = [CHAR_FLAGS[c] for r in rows for c in r]
        self.starts = [c for c, f in enumerate(self.flags) if f & START]
        self.free_cells = [c for c, f in enumerate(self.flags) if f & FREE]
        self.hansen = {"cell_signal": False, "hansen_signal": True}[obs_type]
        self.base = [hansen_code(self.H, self.W, self.flags, c) if self.hansen else c
                     for c in range(self.H * self.W)]
        self.n_obs = (16 if self.hansen else self.H * self.W) * 3
        self.keep_thr = int(keep_thr)
        self.time_limit = int(time_limit)
        unknown = set(rewards) - set(DEFAULT_REWARDS)
        assert not unknown, unknown
        self.rewards = {**DEFAULT_REWARDS, **rewards}

    @classmethod
    def of_env(cls, env):
        return cls(env.maze, env.obs_type, env.keep_thr, env.time_limit, **env.rewards)


def scalar_obs(sp, cell, side):
    signal = (1 if side == 0 else 2) if sp.flags[cell] & PRIEST else 0
    return sp.base[cell] * 3 + signal


def scalar_step(sp, cell, side, elapsed, action, x0, x1, x2, x3):
    """One env, one step, in plain Python integers, following the rules' wording line by line; x0..x3 are the four
    words of the step's block. -> (cell, side, elapsed, obs, reward, terminated, truncated)."""
    r = sp.rewards
    if action < 0:
        action += 4
    assert 0 <= action < 4
    y = x0 >> 1
    if y >= sp.keep_thr:  # the action slips to one of the three others
        action = (action + 1 + ((x1 * 3) >> 32)) & 3
    row, col = divmod(cell, sp.W)
    nrow, ncol = {N: (row - 1, col), E: (row, col + 1), S: (row + 1, col), W_: (row, col - 1)}[action]
    if 0 <= nrow < sp.H and 0 <= ncol < sp.W and sp.flags[nrow * sp.W + ncol] & FREE:
        cell, reward = nrow * sp.W + ncol, r["step_reward"]
    else:
        reward = r["wall_reward"]
    terminated = bool(sp.flags[cell] & (LEFT | RIGHT))
    if terminated:
        in_heaven = (sp.flags[cell] & LEFT and side == 0) or (sp.flags[cell] & RIGHT and side == 1)
        reward = r["heaven_reward"] if in_heaven else r["hell_reward"]
    truncated = elapsed + 1 >= sp.time_limit
    elapsed += 1
    if terminated or truncated:
        cell = sp.starts[(x2 * len(sp.starts)) >> 32]
        side = x3 & 1
        elapsed = 0
    return cell, side, elapsed, scalar_obs(sp, cell, side), np.float32(reward), terminated, truncated


class HeavenHellOracle:
    """B envs at once. State: agent (cell), side, elapsed, int64 [B]."""

    def __init__(self, B, spec):
        self.B, self.sp = B, spec
        self.agent = np.zeros(B, dtype=np.int64)
        self.side = np.zeros(B, dtype=np.int64)
        self.elapsed = np.zeros(B, dtype=np.int64)
        self.flags = np.array(spec.flags, dtype=np.int64)
        self.base = np.array(spec.base, dtype=np.int64)
        self.starts = np.array(spec.starts, dtype=np.int64)

    def philox_draws(self, step, key):
        w = env_step_words(self.B, step, TAG, key)
        return self.draws_of_words(*w)

    def draws_of_words(self, x0, x1, x2, x3):
        x0, x1, x2, x3 = (np.asarray(x, dtype=np.uint64) for x in (x0, x1, x2, x3))
        return dict(y=(x0 >> np.uint64(1)).astype(np.int64),
                    slip_to=((x1 * np.uint64(3)) >> np.uint64(32)).astype(np.int64),
                    start=self.starts[((x2 * np.uint64(len(self.starts))) >> np.uint64(32)).astype(np.int64)],
                    side=(x3 & np.uint64(1)).astype(np.int64))

    def obs(self):
        priest = (self.flags[self.agent] & PRIEST) != 0
        return (self.base[self.agent] * 3 + np.where(priest, 1 + self.side, 0)).astype(np.int32)

    def reset(self, draws):
        self.agent = draws["start"].copy()
        self.side = draws["side"].copy()
        self.elapsed[:] = 0
        return self.obs()

    def step(self, actions, draws):
        sp, r = self.sp, self.sp.rewards
        a = np.asarray(actions, dtype=np.int64)
        a = np.where(a < 0, a + 4, a)
        assert ((a >= 0) & (a < 4)).all()
        a = np.where(draws["y"] >= sp.keep_thr, (a + 1 + draws["slip_to"]) & 3, a)
        row, col = np.divmod(self.agent, sp.W)
        nrow = row + np.array([-1, 0, 1, 0])[a]
        ncol = col + np.array([0, 1, 0, -1])[a]
        inside = (nrow >= 0) & (nrow < sp.H) & (ncol >= 0) & (ncol < sp.W)
        target = np.where(inside, nrow * sp.W + ncol, self.agent)
        moved = inside & ((self.flags[target] & FREE) != 0)
        agent = np.where(moved, target, self.agent)
        rew = np.where(moved, r["step_reward"], r["wall_reward"])
        f = self.flags[agent]
        term = (f & (LEFT | RIGHT)) != 0
        heaven = np.where(self.side == 0, (f & LEFT) != 0, (f & RIGHT) != 0)
        rew = np.where(term, np.where(heaven, r["heaven_reward"], r["hell_reward"]), rew)
        el = self.elapsed + 1
        trunc = el >= sp.time_limit
        done = term | trunc
        self.agent = np.where(done, draws["start"], agent)
        self.side = np.where(done, draws["side"], self.side)
        self.elapsed = np.where(done, 0, el)
        return self.obs(), rew.astype(np.float32), term, trunc


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


def enumeration(sp, time_limit):
    """One env per (free cell, side, action in -4..3, elapsed first / last): int64 arrays (cell, side, act, el)."""
    return tuple(x.ravel() for x in np.meshgrid(np.array(sp.free_cells), np.arange(2), np.arange(-4, 4),
                                                np.array([0, time_limit - 1]), indexing="ij"))
