"""Car-Flag vector envs — drop-ins for `gym_po.envs.car_flag.CarVecEnv` / `DiscreteActionCarVecEnv`
(car_flag.py:23-144, :286-303): the 1-D heaven/hell POMDP.

A car on the line [-1.1, 1.1] is pushed by a force in [-1, 1]. One end (+-1) is heaven (+1, terminal), the
other hell (-1, terminal); which is which is revealed (observation component 2 = heaven's sign) only while the
car is within 0.2 of the priest at +-0.5. Observation float32 [B, 3] = (position, velocity, direction).
Episodes truncate at `elapsed >= time_limit`; terminated or truncated envs reset in the same step and the
returned observation is the state after that reset.

The step, the resets and their random draws run on the GPU (csrc/carflag.hip). `rng_mode="numpy"` consumes
the reference's own PCG64 stream draw for draw; "philox" fuses K-step rollouts in one launch; "replay" takes the
draws from the caller. `action_dtype` picks the arithmetic the reference would use for actions of that dtype:
"float32" (the action space's dtype) computes in float32 throughout, "float64" computes the new velocity and
position in float64 and rounds them to float32 when stored; the discrete env's action table is float64.
"""
import ctypes

import numpy as np

from .. import _lib
from ..core import NativeVecEnv, _torch
from ..spaces import Box, Discrete, batch_space


class CarVecEnv(NativeVecEnv):
    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 10, "name": "CarFlag"}
    # physics and task parameters
    MAX_POS = 1.1
    MIN_POS = -MAX_POS
    POS_RANGE = MAX_POS - MIN_POS
    MAX_SPEED = 0.07
    MIN_ACT = -1.0
    MAX_ACT = 1.0
    PRIEST = 0.5
    PRIEST_THRESHOLD = 0.2
    POWER = 0.0015
    # number-line frame
    SCREEN_WIDTH = 600
    SCREEN_HEIGHT = 400
    SCALE = SCREEN_WIDTH / (MAX_POS - MIN_POS)
    HEIGHT = 0.55
    PIXEL_WIDTH = 4
    PIXEL_HEIGHT = 24
    START_PIXEL_RANGE = SCREEN_WIDTH - PIXEL_WIDTH

    def __init__(self, num_envs, time_limit=160, render_mode=None, device=None, rng_mode="numpy",
                 action_dtype="float32", *, _num_actions=None):
        self.num_envs = num_envs
        self.is_vector_env = True
        self.render_mode = render_mode
        self.time_limit = time_limit
        self.single_observation_space = Box(np.array([self.MIN_POS, -self.MAX_SPEED, -1.0]),
                                            np.array([self.MAX_POS, self.MAX_SPEED, 1.0]), dtype=np.float32)
        self.observation_space = batch_space(self.single_observation_space, num_envs)
        self.single_action_space = Box(self.MIN_ACT, self.MAX_ACT, (1,), dtype=np.float32)
        self.action_space = batch_space(self.single_action_space, num_envs)
        cfg = _lib.CarFlagConfig()
        cfg.time_limit = int(time_limit)
        self._table = None
        if _num_actions is None:
            if action_dtype not in ("float32", "float64"):
                raise ValueError("action_dtype must be 'float32' or 'float64'")
            self._action_dtype = action_dtype
            cfg.action_kind = 0 if action_dtype == "float32" else 1
            cfg.action_table = None
        else:
            if int(_num_actions) < 2:
                raise ValueError("DiscreteActionCarVecEnv needs num_actions >= 2")
            self._action_dtype = "int32"
            self._table = np.ascontiguousarray(np.linspace(self.MIN_ACT, self.MAX_ACT, int(_num_actions)), np.float64)
            cfg.action_kind = int(_num_actions)
            cfg.action_table = self._table.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self._create(_lib.GP_KIND_CARFLAG, cfg, num_envs, device, rng_mode)

    def reset(self, *, seed=None, options=None):
        return self._reset_impl(seed), {}

    # ------------------------------------------------------------------ state / replay ----
    def get_state(self):
        """(s float32 [B,3], elapsed int32 [B], heavens float32 [B] (+-1), priests float32 [B] (+-0.5))."""
        torch = _torch()
        s = torch.empty((self.num_envs, 3), dtype=torch.float32, device=self.device)
        el = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        h = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        p = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        self._get_state_raw([s, el, h, p])
        return s, el, h, p

    def set_state(self, s=None, elapsed=None, heavens=None, priests=None):
        """Overwrite the given parts of the state (heavens / priests are taken by sign)."""
        torch = _torch()

        def conv(x, dt):
            if x is None:
                return None
            x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
            return x.to(device=self.device, dtype=dt).contiguous()
        bufs = [conv(s, torch.float32), conv(elapsed, torch.int32), conv(heavens, torch.float32),
                conv(priests, torch.float32)]
        if bufs[0] is not None and tuple(bufs[0].shape) != (self.num_envs, 3):
            raise ValueError(f"s must have shape ({self.num_envs}, 3)")
        for b in bufs[1:]:
            if b is not None and b.numel() != self.num_envs:
                raise ValueError(f"elapsed / heavens / priests must have {self.num_envs} elements")
        self._set_state_raw(bufs)
        torch.cuda.current_stream(self.device).synchronize()

    def set_replay(self, u=None, heaven_idx=None, priest_idx=None):
        """rng_mode='replay': per-env draws of the next reset. u: the integer k (< 2**53) with
        Generator.random() == k * 2**-53 behind uniform(-0.2, 0.2); heaven_idx / priest_idx: the indices
        choice() drew into (-1, 1) / (-0.5, 0.5)."""
        torch = _torch()

        def conv(x, dt):
            if x is None:
                return None
            if not isinstance(x, torch.Tensor):
                x = np.asarray(x)
                x = torch.as_tensor(x.view(np.int64) if x.dtype == np.uint64 else x)
            return x.to(device=self.device, dtype=dt).contiguous()
        super().set_replay(u=conv(u, torch.int64), i0=conv(heaven_idx, torch.int32), i1=conv(priest_idx, torch.int32))

    # ------------------------------------------------------------------ rendering ----
    @classmethod
    def _pixel(cls, x):
        return np.floor(np.interp(x, xp=[cls.MIN_POS, cls.MAX_POS], fp=[0, cls.START_PIXEL_RANGE])).astype(int)

    @classmethod
    def frame(cls, s0, heaven, priest):
        """The number-line frame (uint8 [48, 600, 3]) of one env: s0 = its (position, velocity, direction),
        heaven = +-1, priest = +-0.5 (car_flag.py:156-178). White end posts; heaven's end (+-1) green, hell's
        red; the car a 4-pixel bar on the lower half, bright while the direction is shown; the priest a blue bar
        with dimmer bars at the edges of its zone."""
        W, PH = cls.PIXEL_WIDTH, cls.PIXEL_HEIGHT
        img = np.zeros((2 * PH, cls.SCREEN_WIDTH, 3), dtype=np.uint8)
        img[:, :W] = 255
        img[:, -W:] = 255
        flags = cls._pixel([-1, 1])
        hea = flags[0 if heaven < 0 else 1]
        hell = flags[1 if heaven < 0 else 0]
        img[:, hea:hea + 4, 1] = 255
        img[:, hell:hell + 4, 0] = 255
        car = cls._pixel(s0[0])
        img[-PH:, car:car + 4] = 255 if s0[2] else 128
        priest = float(priest)
        lo, mid, hi = cls._pixel([priest - cls.PRIEST_THRESHOLD, priest, priest + cls.PRIEST_THRESHOLD])
        img[:, lo:lo + W, 2] = 128
        img[:, hi:hi + W, 2] = 128
        img[:, mid:mid + W, 2] = 255
        return img

    def render(self):
        """render_mode='rgb_array': the number-line frame of env 0 as a host uint8 [48, 600, 3] array, drawn on
        the host from env 0's state (syncs). The reference's 'human' mode opens a pygame window; not offered."""
        if self.render_mode != "rgb_array":
            raise NotImplementedError("CarVecEnv.render(): only render_mode='rgb_array' is available")
        s, _, h, p = self.get_state()
        return self.frame(s[0].cpu().numpy(), float(h[0].item()), float(p[0].item()))


class DiscreteActionCarVecEnv(CarVecEnv):
    """Car-Flag with `num_actions` evenly spaced forces over [-1, 1] (car_flag.py:286-303)."""

    def __init__(self, num_actions, *args, **kwargs):
        if "action_dtype" in kwargs or len(args) > 5:
            raise TypeError("DiscreteActionCarVecEnv takes no action_dtype (its force table is float64)")
        super().__init__(*args, _num_actions=int(num_actions), **kwargs)
        self._actions = self._table
        half = num_actions // 2
        self.action_names = (["<" * i + ":" for i in range(half, 0, -1)] + ([":"] if num_actions % 2 else [])
                             + [":" + ">" * i for i in range(1, half + 1)])
        self.single_action_space = Discrete(num_actions)
        self.action_space = batch_space(self.single_action_space, self.num_envs)
