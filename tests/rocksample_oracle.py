"""ORACLE / TEST INFRASTRUCTURE — numpy restatement of the build-defined RockSample rules (csrc/rocksample.hip header,
include/gym_po_amd.h gp_rocksample_config). The reference has no program text for this env (only the
Obs / ACTION enums and a constructor signature), so there is no reference parity to pin: the device is pinned to this
restatement bit for bit, and this restatement to the scalar one-env statement `scalar_step` below
(tests/test_rocksample_cpu.py).

Draws: one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, TAG): y = x0 >> 1 decides a CHECK,
x1 & (2^k - 1) is the good mask of a reset.
"""
import numpy as np

from oracle.philox import env_step_words, philox_key  # noqa: F401  (philox_key(seed): the key the draws take)

TAG = 0x726F636B
NULL, GOOD, BAD = 0, 1, 2
N, E, S, W_, SAMPLE, CHECK0 = 0, 1, 2, 3, 4, 5
DEFAULT_REWARDS = dict(exit_reward=10.0, good_reward=10.0, bad_reward=-10.0, empty_reward=-10.0, check_reward=0.0,
                       step_reward=0.0, wall_reward=0.0)


class Spec:
    """What a handle is configured with. rocks / init_pos are (y, x); thr is the uint32 [H * W, k] sensor table."""

    def __init__(self, map_size, rocks, init_pos, thr, obs_type="cell_sensor", time_limit=200, **rewards):
        self.H, self.W = map_size
        self.rock_cells = [y * self.W + x for y, x in rocks]
        self.k = len(self.rock_cells)
        self.A = 5 + self.k
        self.init_cell = init_pos[0] * self.W + init_pos[1]
        self.thr = np.asarray(thr, dtype=np.int64).reshape(self.H * self.W, self.k)
        self.obs_cell = {"cell_sensor": True, "sensor": False}[obs_type]
        self.time_limit = time_limit
        unknown = set(rewards) - set(DEFAULT_REWARDS)
        assert not unknown, unknown
        self.rewards = {**DEFAULT_REWARDS, **rewards}

    @classmethod
    def of_env(cls, env, **rewards):
        return cls(env.map_size, env.rocks, env.init_pos, env.sensor_thresholds, env.obs_type, env.time_limit,
                   **rewards)


def scalar_step(sp, cell, mask, elapsed, action, y, reset_mask):
    """One env, one step, in plain Python integers, following the rules' wording line by line.
    -> (cell, mask, elapsed, obs, reward, terminated, truncated)."""
    r = sp.rewards
    if action < 0:
        action += sp.A
    assert 0 <= action < sp.A
    elapsed += 1
    reading = NULL
    terminated = False
    row, col = cell // sp.W, cell % sp.W
    if action in (N, S, W_):
        nrow, ncol = {N: (row - 1, col), S: (row + 1, col), W_: (row, col - 1)}[action]
        if 0 <= nrow < sp.H and 0 <= ncol < sp.W:
            cell, reward = nrow * sp.W + ncol, r["step_reward"]
        else:
            reward = r["wall_reward"]
    elif action == E:
        if col == sp.W - 1:
            terminated, reward = True, r["exit_reward"]
        else:
            cell, reward = cell + 1, r["step_reward"]
    elif action == SAMPLE:
        if cell in sp.rock_cells:
            i = sp.rock_cells.index(cell)
            reward = r["good_reward"] if (mask >> i) & 1 else r["bad_reward"]
            mask &= ~(1 << i)
        else:
            reward = r["empty_reward"]
    else:
        i = action - CHECK0
        reward = r["check_reward"]
        correct = y < int(sp.thr[cell, i])
        reading = GOOD if bool((mask >> i) & 1) == correct else BAD
    truncated = elapsed >= sp.time_limit
    if terminated or truncated:
        cell, mask, elapsed, reading = sp.init_cell, reset_mask & ((1 << sp.k) - 1), 0, NULL
    obs = cell * 3 + reading if sp.obs_cell else reading
    return cell, mask, elapsed, obs, np.float32(reward), terminated, truncated


class RockSampleOracle:
    """B envs at once. State: agent (cell), mask, elapsed, int64 [B]."""

    def __init__(self, B, spec):
        self.B, self.sp = B, spec
        self.agent = np.zeros(B, dtype=np.int64)
        self.mask = np.zeros(B, dtype=np.int64)
        self.elapsed = np.zeros(B, dtype=np.int64)
        self.rock_at = np.full(spec.H * spec.W, -1, dtype=np.int64)
        self.rock_at[spec.rock_cells] = np.arange(spec.k)

    def philox_draws(self, step, key):
        w = env_step_words(self.B, step, TAG, key)
        return dict(y=(w[0] >> np.uint32(1)).astype(np.int64),
                    mask=(w[1] & np.uint32((1 << self.sp.k) - 1)).astype(np.int64))

    def obs(self, reading):
        return (self.agent * 3 + reading if self.sp.obs_cell else reading + 0 * self.agent).astype(np.int32)

    def reset(self, draws):
        self.agent[:] = self.sp.init_cell
        self.mask[:] = draws["mask"]
        self.elapsed[:] = 0
        return self.obs(NULL)

    def step(self, actions, draws):
        sp, r = self.sp, self.sp.rewards
        a = np.asarray(actions, dtype=np.int64)
        a = np.where(a < 0, a + sp.A, a)
        assert ((a >= 0) & (a < sp.A)).all()
        el = self.elapsed + 1
        row, col = np.divmod(self.agent, sp.W)
        move = a < SAMPLE
        am = np.where(move, a, 0)
        nrow = row + np.array([-1, 0, 1, 0])[am]
        ncol = col + np.array([0, 1, 0, -1])[am]
        term = (a == E) & (col == sp.W - 1)
        moved = move & ~term & (nrow >= 0) & (nrow < sp.H) & (ncol >= 0) & (ncol < sp.W)
        rew = np.where(term, r["exit_reward"], np.where(moved, r["step_reward"], r["wall_reward"]))
        agent = np.where(moved, nrow * sp.W + ncol, self.agent)
        # SAMPLE
        rk = self.rock_at[self.agent]
        on = (a == SAMPLE) & (rk >= 0)
        rks = np.where(on, rk, 0)
        good = (self.mask >> rks) & 1
        rew = np.where(a == SAMPLE, np.where(on, np.where(good == 1, r["good_reward"], r["bad_reward"]),
                                             r["empty_reward"]), rew)
        mask = np.where(on, self.mask & ~(1 << rks), self.mask)
        # CHECK
        chk = a >= CHECK0
        i = np.where(chk, a - CHECK0, 0)
        correct = draws["y"] < sp.thr[self.agent, i]
        reading = np.where(chk, np.where((((self.mask >> i) & 1) == 1) == correct, GOOD, BAD), NULL)
        rew = np.where(chk, r["check_reward"], rew)
        trunc = el >= sp.time_limit
        done = term | trunc
        self.agent = np.where(done, sp.init_cell, agent)
        self.mask = np.where(done, draws["mask"], mask)
        self.elapsed = np.where(done, 0, el)
        return self.obs(np.where(done, NULL, reading)), rew.astype(np.float32), term, trunc


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
