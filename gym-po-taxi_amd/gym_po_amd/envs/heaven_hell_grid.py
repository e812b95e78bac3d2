"""Grid Heaven-Hell — a build-defined grid restatement of the task of `gym_po.envs.ant_heaven_hell.AntHeavenHellEnv`
(ant_heaven_hell.py:35-40, :99-137; the reference env is a MuJoCo ant in a T-maze, registered with
max_episode_steps=500). The ant is out of scope here, so parity with the reference is unpinned by construction, as
grid Ant-Tag's is: the device is pinned to the numpy restatement of the rules under tests/.

The task is the canonical memory task: the agent starts in the stem of a T, one arm of which holds heaven (+1) and
the other hell (-1), a fair coin per episode. Only near the priest, between the arms, does the obs say which arm is
which; no memoryless policy can carry that to the arm, a finite-state controller (set_controller) can.

Rules (csrc/heavenhell.hip header): an H x W maze (sides 1..16), cell = row * W + col. Actions 0 N, 1 E,
2 S, 3 W; with `action_failure_probability` the action is replaced by one of the other three, uniformly. A move into
a wall or off the grid leaves the agent in place and pays wall_reward, any other move step_reward. A cell of the left or
right area ends the episode with heaven_reward or hell_reward. Truncation at time_limit steps (gymnasium TimeLimit).
An episode end resets the env in the same step: a uniform start cell, a fair coin for the heaven side.
Observation: base * 3 + signal, signal 0 outside the priest area, inside it 1 = heaven left, 2 = heaven right; base is
the cell (`obs_type="cell_signal"`, the default) or the cell's Hansen-4 code sum 2^i [neighbour i is free] over N, E, S,
W (`"hansen_signal"`: the reference's position-free obs plus this project's wall sensor).
"""
import ctypes

import numpy as np

from .. import _lib
from ..core import NativeVecEnv, _torch
from ..spaces import Discrete, batch_space

ACTION_NAMES = ["N", "E", "S", "W"]
OBS_TYPES = ("cell_signal", "hansen_signal")
MAZE_CHARS = "#.SLRP"
FLAG_FREE, FLAG_LEFT, FLAG_RIGHT, FLAG_PRIEST, FLAG_START = 1, 2, 4, 8, 16
_CHAR_FLAGS = {"#": 0, ".": FLAG_FREE, "S": FLAG_FREE | FLAG_START, "L": FLAG_FREE | FLAG_LEFT,
               "R": FLAG_FREE | FLAG_RIGHT, "P": FLAG_FREE | FLAG_PRIEST}
MAX_SIDE = 16
TOP = 1 << 31
# ant_heaven_hell.py:35-40
DEFAULT_HEAVEN_HELL = ((-6.25, 6.0), (6.25, 6.0))
DEFAULT_PRIEST_POS = (0.0, 6.0)
DEFAULT_TERMINATION_RADIUS = 2.0
# the arena of assets/ant_heaven_hell.xml:72-100 at 1 m cells: 10 rows x 16 columns, cell (r, c) centred at
# (x, y) = (c - 7.5, 7.5 - r); the bar and the stem as open boxes (x0, x1, y0, y1); the start box of
# ant_heaven_hell.py:74 as a closed one
ARENA_SHAPE = (10, 16)
ARENA_FREE_BOXES = ((-8.0, 8.0, 4.0, 8.0), (-2.0, 2.0, -2.0, 4.0))
ARENA_START_BOX = (-1.0, 1.0, 0.0, 1.0)


def heaven_hell_maze(heaven_hell=DEFAULT_HEAVEN_HELL, priest_pos=DEFAULT_PRIEST_POS,
                     termination_radius=DEFAULT_TERMINATION_RADIUS):
    """The reference's arena as a tuple of strings over `# . S L R P` (wall, free, start, left area, right area,
    priest area): a free cell is in an area iff its centre is within `termination_radius` of that area's point
    (float64; with the defaults every quantity is a dyadic rational and no centre lies on a circle). `heaven_hell` =
    (left point, right point), (x, y) each. Raises ValueError where two areas overlap or an area covers a start cell:
    one character per cell cannot say that."""
    H, W = ARENA_SHAPE
    r, c = np.divmod(np.arange(H * W), W)
    x, y = c - 7.5, 7.5 - r
    free = np.zeros(H * W, dtype=bool)
    for x0, x1, y0, y1 in ARENA_FREE_BOXES:
        free |= (x0 < x) & (x < x1) & (y0 < y) & (y < y1)
    x0, x1, y0, y1 = ARENA_START_BOX
    start = free & (x0 <= x) & (x <= x1) & (y0 <= y) & (y <= y1)
    r2 = float(termination_radius) ** 2
    points = (tuple(heaven_hell[0]), tuple(heaven_hell[1]), tuple(priest_pos))
    areas = [free & ((x - float(px)) ** 2 + (y - float(py)) ** 2 <= r2) for px, py in points]
    if (areas[0] & areas[1]).any() or (areas[0] & areas[2]).any() or (areas[1] & areas[2]).any():
        raise ValueError("heaven_hell_maze: the left, right and priest areas overlap")
    if (start & (areas[0] | areas[1] | areas[2])).any():
        raise ValueError("heaven_hell_maze: an area covers a start cell")
    ch = np.where(free, ".", "#")
    for a, name in zip(areas, "LRP"):
        ch = np.where(a, name, ch)
    ch = np.where(start, "S", ch)
    return tuple("".join(ch[i * W:(i + 1) * W]) for i in range(H))


def parse_maze(maze):
    """(H, W, flags uint8 [H * W]) of a maze given as strings over `# . S L R P` (a sequence of rows, or one string
    with newlines). Raises ValueError naming the fault: rows of unequal length, a side outside [1, 16], a character
    outside the set, no start cell. (A start cell in the left or right area has no character; a flag table that holds
    one is refused by `check_flags`.)"""
    rows = [r for r in maze.strip().splitlines()] if isinstance(maze, str) else [str(r) for r in maze]
    rows = [r.strip() for r in rows]
    H = len(rows)
    W = len(rows[0]) if H else 0
    if any(len(r) != W for r in rows):
        raise ValueError("maze: rows of unequal length")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"maze: {H} x {W} has a side outside [1, {MAX_SIDE}] (cells are kept in 8 bits)")
    for i, r in enumerate(rows):
        for j, c in enumerate(r):
            if c not in _CHAR_FLAGS:
                raise ValueError(f"maze: character {c!r} at row {i}, col {j} is outside the set {MAZE_CHARS!r}")
    flags = np.array([_CHAR_FLAGS[c] for r in rows for c in r], dtype=np.uint8)
    check_flags(H, W, flags)
    return H, W, flags


def check_flags(H, W, flags):
    """The refusals of a flag table (the library states the same ones): ValueError naming the fault."""
    flags = np.asarray(flags)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"maze: {H} x {W} has a side outside [1, {MAX_SIDE}] (cells are kept in 8 bits)")
    start = (flags & FLAG_START) != 0
    if not start.any():
        raise ValueError("maze: no start cell")
    bad = start & ((flags & (FLAG_LEFT | FLAG_RIGHT)) != 0)
    if bad.any():
        c = int(np.flatnonzero(bad)[0])
        raise ValueError(f"maze: start cell {c} (row {c // W}, col {c % W}) lies in the left or right area")


def hansen_codes(H, W, flags):
    """int32 [H * W]: sum 2^i [neighbour i is a free cell of the grid] over i = N, E, S, W (ROOMS' binary Hansen-4)."""
    free = ((np.asarray(flags) & FLAG_FREE) != 0).reshape(H, W)
    p = np.pad(free, 1)
    code = p[:-2, 1:-1] * 1 + p[1:-1, 2:] * 2 + p[2:, 1:-1] * 4 + p[1:-1, :-2] * 8
    return code.reshape(-1).astype(np.int32)


def keep_threshold(action_failure_probability):
    """floor((1 - p) * 2^31) in float64: an action slips iff its 31-bit draw is at or above it."""
    p = float(action_failure_probability)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"action_failure_probability must be in [0, 1], got {action_failure_probability!r}")
    return int(np.floor((1.0 - p) * float(TOP)))


class HeavenHellGridEnv(NativeVecEnv):
    """`maze=None` builds the reference's arena from (heaven_hell, priest_pos, termination_radius) with
    `heaven_hell_maze`; a maze given in the characters `# . S L R P` replaces it (the three geometry arguments are
    then unused). rng_mode: 'philox' only (there is no reference stream to follow or replay)."""
    metadata = {"render_modes": [], "name": "HeavenHellGrid"}

    def __init__(self, num_envs, heaven_hell=DEFAULT_HEAVEN_HELL, priest_pos=DEFAULT_PRIEST_POS,
                 termination_radius=DEFAULT_TERMINATION_RADIUS, maze=None, obs_type="cell_signal",
                 action_failure_probability=0.0, time_limit=500, heaven_reward=1.0, hell_reward=-1.0, step_reward=0.0,
                 wall_reward=0.0, device=None, rng_mode="philox"):
        if obs_type not in OBS_TYPES:
            raise ValueError(f"obs_type must be one of {OBS_TYPES}, got {obs_type!r}")
        if maze is None:
            maze = heaven_hell_maze(heaven_hell, priest_pos, termination_radius)
        self.maze = tuple(maze.strip().splitlines()) if isinstance(maze, str) else tuple(str(r) for r in maze)
        H, W, flags = parse_maze(self.maze)
        self.map_size = (H, W)
        self.flags = flags
        self.start_cells = np.flatnonzero(flags & FLAG_START).astype(np.int32)
        self.obs_type = obs_type
        self.obs_base = (np.arange(H * W, dtype=np.int32) if obs_type == "cell_signal" else hansen_codes(H, W, flags))
        self.obs_base_n = H * W if obs_type == "cell_signal" else 16
        self.action_failure_probability = float(action_failure_probability)
        self.keep_thr = keep_threshold(action_failure_probability)
        self.time_limit = int(time_limit)
        self.rewards = dict(heaven_reward=float(heaven_reward), hell_reward=float(hell_reward),
                            step_reward=float(step_reward), wall_reward=float(wall_reward))
        self.num_envs = num_envs
        self.is_vector_env = True
        self.single_action_space = Discrete(len(ACTION_NAMES))
        self.action_space = batch_space(self.single_action_space, num_envs)
        self.single_observation_space = Discrete(self.obs_base_n * 3)
        self.observation_space = batch_space(self.single_observation_space, num_envs)
        base = np.ascontiguousarray(self.obs_base, dtype=np.int32)
        cfg = _lib.HeavenHellConfig()
        cfg.height, cfg.width = H, W
        cfg.flags = flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        cfg.obs_base = base.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        cfg.obs_base_n = self.obs_base_n
        cfg.keep_thr = self.keep_thr
        cfg.time_limit = self.time_limit
        cfg.heaven_reward, cfg.hell_reward = self.rewards["heaven_reward"], self.rewards["hell_reward"]
        cfg.step_reward, cfg.wall_reward = self.rewards["step_reward"], self.rewards["wall_reward"]
        self._create(_lib.GP_KIND_HEAVENHELL, cfg, num_envs, device, rng_mode)

    def reset(self, *, seed=None, options=None):
        return self._reset_impl(seed), {}

    def get_state(self):
        """(agent cell, heaven side, elapsed) int32 [B] (cell = row * W + col; side 0: heaven is the left area)."""
        torch = _torch()
        a, h, e = (torch.empty(self.num_envs, dtype=torch.int32, device=self.device) for _ in range(3))
        self._get_state_raw([a, h, e])
        return a, h, e

    def set_state(self, agent=None, heaven=None, elapsed=None):
        """Replace the given fields (None leaves one alone): the cell is clamped to the grid, elapsed to [0, 65535],
        the side keeps its low bit."""
        torch = _torch()
        conv = lambda x: None if x is None else torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, device=self.device).to(torch.int32).contiguous()  # noqa: E731
        self._set_state_raw([conv(agent), conv(heaven), conv(elapsed)])
        torch.cuda.current_stream(self.device).synchronize()
