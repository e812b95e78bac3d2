"""TEST INFRASTRUCTURE — the breadth-first controller of the C-ROOMS closed-loop task test and its cell-level
prediction, shared by tests/test_crooms_controller_cpu.py (which pins the prediction to oracle/crooms.py) and
tests/test_crooms_controller_gpu.py (which holds the device to it).

The task: layout "4", cardinal moves (0 N, 1 E, 2 S, 3 W: ACTIONS_CARDINAL), obs_type "mdp" (the obs is the index of
the agent's cell among the valid cells), no action failures, no action noise, the fixed default goal. Every reset
puts the agent on the centre of a valid cell, a move shifts it by exactly one cell, and the episode ends when it
stands on the goal cell's centre (distance 0 <= goal_threshold 0.5; one cell away the distance is 1).

Rules of `simulate` (crooms.py:276-331 for this configuration):
  * a move into a free cell takes the agent there;
  * a move from the last row or column of cells towards the map's border is clipped to gridshape - 1 - 1e-6, which
    still lies in the agent's cell: no wall hit, the agent stays in its cell at that (known) coordinate;
  * any other move into a wall leaves it in its cell, at a position the wall noise picks inside that cell (clipped
    to [c - 0.5, c + 0.5 - 1e-8] per axis): from then on its position within the cell is unknown; later moves
    still shift it by exactly one cell;
  * with a known position: terminated iff its distance to the goal cell's centre is <= 0.5, evaluated as the
    reference does. With an unknown position: in the goal cell the distance may fall on either side of 0.5
    (undetermined); in any other cell it exceeds 0.5: the goal's free neighbours lie north and west of it (the CPU
    test asserts that), where the clip's upper bound keeps the agent at least 0.5 + 1e-8 away;
  * truncated when the elapsed steps exceed time_limit, i.e. at step time_limit + 1.
"""
import numpy as np

from oracle.gridworld import ACTIONS_CARDINAL, discrete_states, load_maps

LAYOUT = "4"
TIME_LIMIT = 40  # above the longest walk to the goal (28 moves; the CPU test asserts it)
REWARDS = dict(step_reward=-0.25, wall_reward=-0.5, goal_reward=1.0)  # dyadic: the metrics' float64 sums are exact
GOAL, TRUNC, UNDETERMINED = 1, 2, 3


def task_grid():
    maps = load_maps()
    grid = np.array(maps["rooms_layouts"][LAYOUT])
    goal = tuple(reversed(maps["rooms_ends_xy"][LAYOUT]))  # goal_xy = (0, 0) is a wall: the layout's end cell
    return grid, (int(goal[0]), int(goal[1]))


def bfs_distance(grid, goal):
    """Moves to the goal cell through free cells, int [H, W] (-1: a wall)."""
    H, W = grid.shape
    dist = np.full((H, W), -1)
    dist[goal] = 0
    frontier = [goal]
    while frontier:
        nxt = []
        for (r, q) in frontier:
            for dy, dx in ACTIONS_CARDINAL:
                n = (r + dy, q + dx)
                if 0 <= n[0] < H and 0 <= n[1] < W and grid[n] >= 0 and dist[n] < 0:
                    dist[n] = dist[r, q] + 1
                    nxt.append(n)
        frontier = nxt
    return dist


def bfs_actions(grid, goal, rotate=False):
    """int [H, W]: per free cell the first of N, E, S, W that lowers the distance to the goal (on the goal cell: the
    first that leads into a free cell); -1 on walls. rotate: every action turned by two (N <-> S, E <-> W)."""
    H, W = grid.shape
    dist = bfs_distance(grid, goal)
    act = np.full((H, W), -1)
    for r in range(H):
        for q in range(W):
            if grid[r, q] < 0:
                continue
            for a, (dy, dx) in enumerate(ACTIONS_CARDINAL):
                n = (r + dy, q + dx)
                if grid[n] >= 0 and ((r, q) == goal or dist[n] < dist[r, q]):
                    act[r, q] = a
                    break
    assert (act[grid >= 0] >= 0).all()
    return np.where(act >= 0, (act + 2) % 4, -1) if rotate else act


def controller_probs(grid, act):
    """float [n_obs, 4] over the mdp obs: the memoryless deterministic controller that plays act[cell]."""
    n, sg = discrete_states(grid)
    p = np.zeros((n, 4))
    free = grid >= 0
    p[sg[free], act[free]] = 1.0
    assert (p.sum(-1) == 1.0).all()
    return p


def simulate(grid, goal, act, start, time_limit, goal_threshold=0.5):
    """The first episode from the centre of cell `start` under act[cell]: (length, how it ends, wall hits)."""
    H, W = grid.shape
    hi = np.array(grid.shape) - 1 - 1e-6
    centre = np.array(goal) + 0.5
    cell, pos, known, walls = tuple(start), np.array(start) + 0.5, True, 0
    for k in range(1, time_limit + 2):
        d = ACTIONS_CARDINAL[act[cell]]
        n = (cell[0] + d[0], cell[1] + d[1])
        if n[0] == H - 1 or n[1] == W - 1:
            pos = np.minimum(pos + d, hi)
        elif grid[n] >= 0:
            cell, pos = n, pos + d
        else:
            known, walls = False, walls + 1
        if known:
            assert tuple(np.floor(pos).astype(int)) == cell
            if np.linalg.norm(pos - centre, 2) <= goal_threshold:
                return k, GOAL, walls
        elif cell == goal:
            return k, UNDETERMINED, walls
        if k > time_limit:
            return k, TRUNC, walls
    raise AssertionError("unreachable")


def predict(grid, goal, act, time_limit):
    """(length [H, W], ending [H, W], wall hits [H, W]) of `simulate` per start cell (0 on walls)."""
    out = np.zeros((3,) + grid.shape, dtype=int)
    for r, q in zip(*np.nonzero(grid >= 0)):
        out[:, r, q] = simulate(grid, goal, act, (r, q), time_limit)
    return out
