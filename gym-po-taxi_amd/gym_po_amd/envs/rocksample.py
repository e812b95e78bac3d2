"""RockSample (Smith & Simmons, 2004) — the env `gym_po.envs.rocksample.rocksample` names and never builds: the
reference holds only the `Obs` enum (NULL / GOOD / BAD), the `ACTION` enum (NORTH, EAST, SOUTH, WEST, SAMPLE) and the
constructor signature `RockSample(num_envs, map_size=(5, 5), init_pos=(1, 1), render_mode=None)`; every body is `...`.
The rules, the default rock layout and every default below are therefore BUILD-DEFINED, as grid Ant-Tag's are.

Rules (csrc/rocksample.hip header): an H x W grid (sides 1..16) with k rocks (1..16), each good or bad
per env; the agent starts on `init_pos`. Actions: 0 N, 1 E, 2 S, 3 W (a move off the grid leaves the agent in place and
pays wall_reward, except E from the last column, which exits: terminated, exit_reward), 4 SAMPLE (good_reward /
bad_reward on a rock's cell, and the rock turns bad; empty_reward elsewhere), 5 + i CHECK rock i (check_reward; the
reading is the rock's quality with probability 0.5 * (1 + 2^(-d / half_efficiency_distance)), d the Euclidean distance
in cells, else its opposite). Truncation at time_limit steps (gymnasium TimeLimit). An episode end resets the env in the
same step: every rock good with probability 1/2.
Observation: the reading NULL (0) / GOOD (1) / BAD (2) of the step (`obs_type="sensor"`), or cell * 3 + reading
(`"cell_sensor"`, the default), cell = y * W + x.
"""
import ctypes

import numpy as np

from .. import _lib
from ..core import NativeVecEnv, _torch
from ..spaces import Discrete, batch_space

ACTION_NAMES = ["NORTH", "EAST", "SOUTH", "WEST", "SAMPLE"]  # then CHECK_0 .. CHECK_{k-1}
OBS_NAMES = ["NULL", "GOOD", "BAD"]
DEFAULT_MAP_SIZE = (5, 5)
DEFAULT_ROCKS = ((0, 2), (2, 0), (2, 3), (3, 4), (4, 1))  # (y, x), build-defined
OBS_TYPES = ("sensor", "cell_sensor")
TOP = 1 << 31


def rocksample_sensor_thresholds(map_size, rocks, d0=20.0):
    """uint32 [H * W, k]: thr[cell, i] = floor(p * 2^31) with p = 0.5 * (1 + 2^(-d / d0)), d the float64 Euclidean
    distance in cells between `cell` = y * W + x and rock i at `rocks[i]` = (y, x). A CHECK is right iff its 31-bit
    draw is below the entry: always on the rock's own cell (2^31), with probability -> 1/2 far from it. The device
    and the tests' numpy restatement read this one table."""
    H, W = (int(v) for v in map_size)
    r = np.asarray(rocks, dtype=np.float64).reshape(-1, 2)
    if not float(d0) > 0:
        raise ValueError(f"half_efficiency_distance must be > 0, got {d0!r}")
    yy, xx = np.divmod(np.arange(H * W, dtype=np.float64), float(W))
    d = np.sqrt((yy[:, None] - r[None, :, 0]) ** 2 + (xx[:, None] - r[None, :, 1]) ** 2)
    p = 0.5 * (1.0 + np.exp2(-d / float(d0)))
    return np.minimum(np.floor(p * float(TOP)), float(TOP)).astype(np.uint32)


def resolve_rocks(map_size, rocks):
    """The rock layout of a constructor call: `rocks` as given, the build's default on the default map."""
    if rocks is None:
        if tuple(int(v) for v in map_size) != DEFAULT_MAP_SIZE:
            raise ValueError(f"rocks must be given for map_size {tuple(map_size)} (the default layout is for "
                             f"{DEFAULT_MAP_SIZE})")
        rocks = DEFAULT_ROCKS
    return tuple((int(y), int(x)) for y, x in rocks)


class RockSample(NativeVecEnv):
    """Every default (layout, rewards, time_limit, half_efficiency_distance) is build-defined: the reference has
    none. rng_mode: 'philox' only (there is no reference stream to follow or replay)."""
    metadata = {"render_modes": [], "name": "RockSample"}

    def __init__(self, num_envs, map_size=(5, 5), init_pos=(1, 1), render_mode=None, rocks=None,
                 obs_type="cell_sensor", half_efficiency_distance=20.0, time_limit=200, exit_reward=10.0,
                 good_reward=10.0, bad_reward=-10.0, empty_reward=-10.0, check_reward=0.0, step_reward=0.0,
                 wall_reward=0.0, device=None, rng_mode="philox"):
        if obs_type not in OBS_TYPES:
            raise ValueError(f"obs_type must be one of {OBS_TYPES}, got {obs_type!r}")
        if render_mode is not None:
            raise ValueError("RockSample has no render modes")
        H, W = (int(v) for v in map_size)
        self.map_size = (H, W)
        self.rocks = resolve_rocks(map_size, rocks)
        self.init_pos = (int(init_pos[0]), int(init_pos[1]))
        self.render_mode = render_mode
        self.obs_type = obs_type
        self.time_limit = int(time_limit)
        self.num_envs = num_envs
        self.is_vector_env = True
        k = len(self.rocks)
        self.single_action_space = Discrete(5 + k)
        self.action_space = batch_space(self.single_action_space, num_envs)
        self.single_observation_space = Discrete(max(H * W, 1) * 3 if obs_type == "cell_sensor" else 3)
        self.observation_space = batch_space(self.single_observation_space, num_envs)
        self.sensor_thresholds = rocksample_sensor_thresholds((H, W), self.rocks, half_efficiency_distance)

        def cell(y, x):  # a position off the grid becomes -1: the library refuses it by name
            return y * W + x if 0 <= y < H and 0 <= x < W else -1

        rock_cells = np.array([cell(y, x) for y, x in self.rocks], dtype=np.int32)
        thr = np.ascontiguousarray(self.sensor_thresholds)
        cfg = _lib.RockSampleConfig()
        cfg.height, cfg.width, cfg.n_rocks = H, W, k
        cfg.rocks = rock_cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        cfg.init_cell = cell(*self.init_pos)
        cfg.sensor_thr = thr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        cfg.obs_cell = int(obs_type == "cell_sensor")
        cfg.time_limit = self.time_limit
        cfg.exit_reward, cfg.good_reward, cfg.bad_reward = float(exit_reward), float(good_reward), float(bad_reward)
        cfg.empty_reward, cfg.check_reward = float(empty_reward), float(check_reward)
        cfg.step_reward, cfg.wall_reward = float(step_reward), float(wall_reward)
        self._create(_lib.GP_KIND_ROCKSAMPLE, cfg, num_envs, device, rng_mode)

    def reset(self, *, seed=None, options=None):
        return self._reset_impl(seed), {}

    def get_state(self):
        """(agent cell, good-rock mask, elapsed) int32 [B] (cell = y * W + x; bit i of the mask: rock i is good)."""
        torch = _torch()
        a, m, e = (torch.empty(self.num_envs, dtype=torch.int32, device=self.device) for _ in range(3))
        self._get_state_raw([a, m, e])
        return a, m, e

    def set_state(self, agent=None, rocks=None, elapsed=None):
        """Replace the given fields (None leaves one alone). The reading part of the obs becomes NULL."""
        torch = _torch()
        conv = lambda x: None if x is None else torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, device=self.device).to(torch.int32).contiguous()  # noqa: E731
        self._set_state_raw([conv(agent), conv(rocks), conv(elapsed)])
        torch.cuda.current_stream(self.device).synchronize()
