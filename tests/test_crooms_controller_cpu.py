"""CPU tests behind the C-ROOMS closed-loop rollouts (no GPU): the threshold tables of its two action sets, and the
breadth-first controller of the GPU task test, whose cell-level prediction (tests/crooms_controller_task.py) is held
against the numpy restatement of the reference (oracle/crooms.py) stepped with the controller's own actions.
"""
import numpy as np
import pytest

from controller_oracle import choose
from crooms_controller_task import (GOAL, LAYOUT, REWARDS, TIME_LIMIT as TL, TRUNC, UNDETERMINED, bfs_actions,
                                    bfs_distance, controller_probs, predict, task_grid)
from gym_po_amd.controller import controller_thresholds
from oracle.crooms import CRoomsOracle
from oracle.draws import ReplayDraws
from oracle.gridworld import discrete_states

TOP = 1 << 31


# ------------------------------------------------------------------ threshold tables ----
@pytest.mark.parametrize("A", [4, 8])
@pytest.mark.parametrize("M", [1, 3, 8])
def test_threshold_tables(A, M):
    """C-ROOMS has 4 (cardinal) or 8 (ordinal) actions: L = A M is a whole number of 16-B quads, at most 64."""
    n_obs, L = 5, A * M
    rng = np.random.default_rng(100 * A + M)
    p = rng.random((M, n_obs, A, M)) * (rng.random((M, n_obs, A, M)) > 0.3)
    p[:, :, A - 1, M - 1] += 0.05
    p /= p.sum((-1, -2), keepdims=True)
    p[0, 0] = 1.0 / L                       # a uniform row
    p[0, 1] = 0.0                           # half on choice 0, nothing on choice 1, half on choice 2
    p[0, 1].reshape(-1)[[0, 2]] = 0.5
    t = controller_thresholds(p)
    assert t.shape == (M, n_obs, L) and t.dtype == np.uint32 and L % 4 == 0 and L <= 64
    t64 = t.astype(np.int64)
    assert (np.diff(t64, axis=-1) >= 0).all() and (t64[..., -1] == TOP).all() and (t64 >= 0).all()
    # the uniform row: T_j = floor((j + 1) 2^31 / L); y below T_0 -> 0, y = T_k - 1 -> k, y = T_k -> k + 1
    row = t64[0, 0]
    # (exactly when L is a power of two; else the float64 cumulative sum may fall just below an integer: one less)
    exact = (np.arange(1, L + 1) * TOP) // L
    assert np.array_equal(row, exact) if L & (L - 1) == 0 else (np.abs(row - exact) <= 1).all()
    assert choose(0, row) == 0 and choose(row[0] - 1, row) == 0 and choose(row[0], row) == 1
    assert choose(TOP - 1, row) == L - 1
    for k in (1, L // 2 - 1, L - 2):
        assert choose(row[k] - 1, row) == k and choose(row[k], row) == k + 1
    # the row with a choice of probability 0: its interval is empty, so it is never drawn
    row = t64[0, 1]
    assert row[0] == row[1] == TOP // 2 and (row[2:] == TOP).all()
    assert choose(0, row) == 0 and choose(TOP // 2 - 1, row) == 0
    assert choose(TOP // 2, row) == 2 and choose(TOP - 1, row) == 2
    # action and next node of a choice: j = a M + n'
    ys = np.array([0, TOP // 3, TOP // 2, TOP - 1])
    j = choose(ys[:, None, None], t64[None])  # [4, M, n_obs]
    assert j.min() >= 0 and j.max() <= L - 1 and (j // M < A).all() and (j % M < M).all()
    # the device's j / M: (j * ceil(2^16 / M)) >> 16 is exact for every j < L (M = 8, A = 8 sits at its limit)
    inv_m = (65536 + M - 1) // M
    assert all((jj * inv_m) >> 16 == jj // M for jj in range(L))


# ------------------------------------------------------------------ the breadth-first controller ----
def _oracle(n):
    return CRoomsOracle(n, layout=LAYOUT, time_limit=TL, obs_type="mdp", action_failure_probability=0.0,
                        action_type="cardinal", action_std=0.0, **REWARDS)


def _first_episodes(act, steps):
    """One env per valid cell of the layout, started on that cell's centre and stepped with act[its cell] read
    through the obs, as the memoryless controller does. Returns per env (first-episode length or 0, its last reward,
    terminated, truncated, any wall hit during it)."""
    grid, goal = task_grid()
    n, sg = discrete_states(grid)
    act_of_obs = np.zeros(n, dtype=int)
    act_of_obs[sg[grid >= 0]] = act[grid >= 0]
    ora = _oracle(n)
    draws = ReplayDraws(dict(uniform=np.full(n, 0.5), agent=np.arange(n), wall_noise=np.zeros((n, 2))))
    obs = ora.reset(draws)
    assert np.array_equal(obs, np.arange(n))  # env i stands on valid cell i, whose obs is i
    assert np.array_equal(ora.goal, np.full((n, 2), goal) + 0.5)
    length = np.zeros(n, dtype=int)
    last = np.zeros(n, dtype=np.float32)
    term1, trunc1, wall = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    for k in range(1, steps + 1):
        obs, r, d, tr = ora.step(act_of_obs[obs], draws)
        running = length == 0
        wall |= running & (r == REWARDS["wall_reward"])
        ends = running & (d | tr)
        length[ends], last[ends], term1[ends], trunc1[ends] = k, r[ends], d[ends], tr[ends]
    return length, last, term1, trunc1, wall


def test_breadth_first_prediction_equals_the_oracle():
    grid, goal = task_grid()
    free = grid >= 0
    assert grid[goal] >= 0 and grid[goal[0] + 1, goal[1]] < 0 and grid[goal[0], goal[1] + 1] < 0  # walls S and E of it
    dist = bfs_distance(grid, goal)
    assert (dist[free] >= 0).all() and dist.max() < TL
    act = bfs_actions(grid, goal)
    p = controller_probs(grid, act)
    assert p.shape == (int(free.sum()), 4)
    length, ending, walls = predict(grid, goal, act, TL)
    # the walk is the breadth-first distance; from the goal cell itself one move out and one back
    assert np.array_equal(length[free], np.where(dist[free] > 0, dist[free], 2))
    assert (ending[free] == GOAL).all() and not walls.any()
    got, last, term, trunc, wall = _first_episodes(act, int(length.max()))
    assert np.array_equal(got, length[free])  # every env ends after exactly the predicted number of steps,
    assert term.all() and not trunc.any() and (last == np.float32(REWARDS["goal_reward"])).all()  # on the goal,
    assert not wall.any()  # and no move hit a wall


def test_rotated_controller_prediction_equals_the_oracle():
    """Every action turned by two walks away from the goal: no first episode reaches it before the time limit, except
    from the goal cell itself: the turned action there points at the map's border, the clip to gridshape - 1 - 1e-6
    leaves the agent 0.499999 from the centre, inside the threshold: terminated after one step. No start is left
    undetermined by the wall noise (no walk enters the goal cell after a wall hit)."""
    grid, goal = task_grid()
    free = grid >= 0
    act = bfs_actions(grid, goal, rotate=True)
    assert np.array_equal((act[free] + 2) % 4, bfs_actions(grid, goal)[free])
    length, ending, walls = predict(grid, goal, act, TL)
    assert not (ending == UNDETERMINED).any()
    reach = ending == GOAL
    assert reach.sum() == 1 and reach[goal] and length[goal] == 1 and walls[goal] == 0
    rest = free & ~reach
    assert (ending[rest] == TRUNC).all() and (length[rest] == TL + 1).all()
    got, last, term, trunc, wall = _first_episodes(act, TL + 1)
    assert np.array_equal(got, length[free]) and np.array_equal(term, reach[free])
    assert np.array_equal(trunc, ~reach[free]) and np.array_equal(wall, walls[free] > 0) and wall.any()
