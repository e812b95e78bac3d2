"""Shared host-side plumbing of the drop-in vector envs: handle lifetime, seeding with the
reference's semantics, device output allocation, reset/step/rollout through the C ABI.

The reference's vector envs are `gymnasium.Env` subclasses with `is_vector_env=True` whose
`reset(*, seed, options)` re-seeds `np_random = Generator(PCG64(SeedSequence(seed)))` when a seed
is given and whose `step(actions)` returns `(obs, rew, terminated, truncated, {})` with
same-step autoreset (msrooms.py:369-413, rooms.py:177-222, extended_taxi.py:232-287,
crooms.py:251-298). Here the state and the RNG live on the GPU; outputs are torch-ROCm tensors.
"""
import ctypes
import secrets

import numpy as np

from . import _lib
from ._lib import check, lib


def _torch():
    import torch
    return torch


class _PlanKeep:
    """Owns a gp_plan (freed with the run closure) and keeps its buffers alive."""

    def __init__(self, plan, bufs):
        self.plan, self.bufs = plan, bufs

    def __del__(self):
        try:
            if self.plan is not None:
                lib().gp_plan_destroy(self.plan)
        except Exception:  # noqa: BLE001
            pass


class NativeVecEnv:
    """Base class: one C-ABI handle, one device, one stream (the torch current stream)."""
    is_vector_env = True
    metadata = {"render_modes": [], "name": "gym_po_amd"}
    _action_dtype = "int32"
    _action_tail = ()

    def _create(self, kind, cfg, num_envs, device=None, rng_mode="numpy"):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.GymPoError("gym_po_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
        self._handle = None
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("gym_po_amd envs run on a GPU device")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        if rng_mode not in _lib.RNG_MODES:
            raise ValueError(f"rng_mode must be one of {list(_lib.RNG_MODES)}")
        self.rng_mode = rng_mode
        self.num_envs = int(num_envs)
        h = ctypes.c_void_p()
        check(lib().gp_create(kind, ctypes.byref(cfg), self.num_envs, self.device.index, _lib.RNG_MODES[rng_mode],
                              ctypes.byref(h)), "gp_create")
        self._handle = h
        dt, w = ctypes.c_int(), ctypes.c_int()
        check(lib().gp_obs_info(h, ctypes.byref(dt), ctypes.byref(w)), "gp_obs_info")
        self._obs_dtype = {0: torch.int32, 1: torch.uint8, 2: torch.float32, 3: torch.float64}[dt.value]
        self._obs_width = w.value
        self._seeded = False
        self._replay_keep = None

    # ------------------------------------------------------------------ lifetime ----
    def close(self):
        if getattr(self, "_handle", None):
            lib().gp_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ------------------------------------------------------------------ helpers ----
    def _stream(self):
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _obs_shape(self):
        return (self.num_envs,) if self._obs_width == 1 else (self.num_envs, self._obs_width)

    def _alloc_outputs(self, K=None):
        torch = _torch()
        lead = (self.num_envs,) if K is None else (K, self.num_envs)
        oshape = self._obs_shape() if K is None else (K,) + self._obs_shape()
        obs = torch.empty(oshape, dtype=self._obs_dtype, device=self.device)
        rew = torch.empty(lead, dtype=torch.float32, device=self.device)
        term = torch.empty(lead, dtype=torch.uint8, device=self.device)
        trunc = torch.empty(lead, dtype=torch.uint8, device=self.device)
        return obs, rew, term, trunc

    def _as_actions(self, actions, K=None):
        torch = _torch()
        dt = {"int32": torch.int32, "float32": torch.float32, "float64": torch.float64}[self._action_dtype]
        shape = ((self.num_envs,) if K is None else (K, self.num_envs)) + self._action_tail
        if isinstance(actions, torch.Tensor):
            if actions.device.type == "cpu":
                self._check_host_actions(actions.numpy())
            a = actions.to(device=self.device, dtype=dt)
        else:
            an = np.asarray(actions)
            self._check_host_actions(an)
            a = torch.as_tensor(an, device=self.device).to(dt)
        if tuple(a.shape) != shape:
            a = a.reshape(shape)
        return a.contiguous()

    def _check_host_actions(self, a):
        """Host-resident discrete actions are range-checked before upload, raising the reference's own error:
        numpy's IndexError from `action_matrix[action]` (msrooms.py:400, rooms.py:208) / `ACTIONS_YX[actions]`
        (extended_taxi.py:248); negatives in [-n, 0) wrap as numpy indexing does. Device tensors are checked
        on the device instead (GP_DERR_ACTION -> GymPoError from check() / metrics()), without a sync."""
        n = getattr(getattr(self, "single_action_space", None), "n", None)
        if n is None or self._action_dtype != "int32":
            return
        if a.dtype.kind not in "iub":  # numpy refuses non-integer index arrays (before any bounds check)
            raise IndexError("arrays used as indices must be of integer (or boolean) type")
        if a.size == 0:
            return
        lo, hi = a.min(), a.max()
        if hi >= n or lo < -n:
            flat = a.reshape(-1)
            bad = int(flat[np.flatnonzero((flat >= n) | (flat < -n))[0]])  # numpy names the first in index order
            raise IndexError(f"index {bad} is out of bounds for axis 0 with size {n}")

    def _post_obs(self, obs):
        # obs_dtype="reference" (grid envs): the reference's own dtype, cast on the device after the kernel (the
        # kernels and rollout_plan's buffers keep the compact native layout)
        cast = getattr(self, "_obs_cast", None)
        return obs if cast is None else obs.to(cast)

    # ------------------------------------------------------------------ seeding ----
    def _seed(self, seed, spawn_key=()):
        words = _lib.int_to_u32_words(int(seed))
        ent = (ctypes.c_uint32 * len(words))(*words)
        sk = (ctypes.c_uint32 * max(len(spawn_key), 1))(*(list(spawn_key) or [0]))
        check(lib().gp_seed_words(self._handle, ent, len(words), sk, len(spawn_key)), "gp_seed_words")
        self._seeded = True

    def seed(self, seed=None, spawn_key=()):
        """numpy/gymnasium seeding: SeedSequence(seed[, spawn_key]); None draws fresh OS entropy."""
        if seed is None:
            seed = secrets.randbits(128)
        self._seed(seed, spawn_key)
        return seed

    @property
    def rng_state(self):
        """The device RNG state as numpy's `PCG64.state` dict (syncs)."""
        st = (ctypes.c_uint64 * 6)()
        check(lib().gp_get_rng_state(self._handle, st), "gp_get_rng_state")
        return {"bit_generator": "PCG64", "state": {"state": (st[0] << 64) | st[1], "inc": (st[2] << 64) | st[3]},
                "has_uint32": int(st[4]), "uinteger": int(st[5])}

    @rng_state.setter
    def rng_state(self, s):
        m = (1 << 64) - 1
        v = [s["state"]["state"] >> 64, s["state"]["state"] & m, s["state"]["inc"] >> 64, s["state"]["inc"] & m,
             s.get("has_uint32", 0), s.get("uinteger", 0)]
        st = (ctypes.c_uint64 * 6)(*v)
        check(lib().gp_set_rng_state(self._handle, st), "gp_set_rng_state")
        self._seeded = True

    @property
    def np_random(self):
        """A numpy Generator positioned where the device stream is (snapshot; syncs)."""
        bg = np.random.PCG64()
        bg.state = self.rng_state
        return np.random.Generator(bg)

    @np_random.setter
    def np_random(self, gen):
        self.rng_state = gen.bit_generator.state

    # ------------------------------------------------------------------ hot path ----
    def _reset_impl(self, seed=None):
        if seed is not None:
            self._seed(seed)
        elif not self._seeded:
            self.seed(None)
        obs, _, _, _ = self._alloc_outputs()
        check(lib().gp_reset(self._handle, ctypes.c_void_p(obs.data_ptr()), self._stream()), "gp_reset")
        return self._post_obs(obs)

    def _step_impl(self, actions):
        a = self._as_actions(actions)
        obs, rew, term, trunc = self._alloc_outputs()
        check(lib().gp_step(self._handle, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(obs.data_ptr()),
                            ctypes.c_void_p(rew.data_ptr()), ctypes.c_void_p(term.data_ptr()),
                            ctypes.c_void_p(trunc.data_ptr()), self._stream()), "gp_step")
        return self._post_obs(obs), rew, term.view(_torch().bool), trunc.view(_torch().bool)

    def step(self, actions):
        obs, rew, term, trunc = self._step_impl(actions)
        return obs, rew, term, trunc, {}

    def rollout(self, actions, out=None):
        """K steps in one call: actions [K, B(,2)] -> obs [K, B, ...], rew/term/trunc [K, B].

        Philox mode, and numpy mode on the grid envs (persistent kernel with a per-step grid
        exchange), run the K steps in ONE fused launch with the env state in registers; C-ROOMS
        numpy mode runs a few multi-workgroup stream kernels per step (csrc/crooms.hip xg_*), Taxi
        numpy mode one single-workgroup launch for the K steps (the stream walk); replay mode issues
        K step launches on the stream. `out` may supply preallocated buffers
        (obs, rew, term(uint8), trunc(uint8)) shaped like `_alloc_outputs(K)`: they are checked
        for shape, dtype, device and contiguity (ValueError otherwise)."""
        torch = _torch()
        K = int(actions.shape[0])
        a = self._as_actions(actions, K)
        if out is None:
            out = self._alloc_outputs(K)
        else:
            self._check_out(out, K)
        obs, rew, term, trunc = out
        check(lib().gp_rollout(self._handle, K, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(obs.data_ptr()),
                               ctypes.c_void_p(rew.data_ptr()), ctypes.c_void_p(term.data_ptr()),
                               ctypes.c_void_p(trunc.data_ptr()), self._stream()), "gp_rollout")
        return self._post_obs(obs), rew, term.view(torch.bool), trunc.view(torch.bool)

    def _check_out(self, out, K):
        torch = _torch()
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise ValueError("out must be (obs, rew, term, trunc)")
        want = (((K,) + self._obs_shape(), self._obs_dtype), ((K, self.num_envs), torch.float32),
                ((K, self.num_envs), torch.uint8), ((K, self.num_envs), torch.uint8))
        for name, t, (shape, dt) in zip(("obs", "rew", "term", "trunc"), out, want):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"out {name}: expected a torch tensor")
            if tuple(t.shape) != shape or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"out {name}: need a contiguous {dt} tensor of shape {shape} on {self.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device} (contiguous={t.is_contiguous()})")

    def rollout_plan(self, actions, out=None):
        """A prepared K-step rollout: validates `actions` [K, B(,2)] (already the env's action dtype, on its
        device, contiguous) and the output buffers once, and returns a callable that enqueues the K steps on
        the stream current at plan time (or the hipStream_t handle it is given) with no further Python work (the agent loop's allocation-free hot path; the
        buffers are reused by every call). Returns (run, (obs, rew, term, trunc))."""
        torch = _torch()
        K = int(actions.shape[0])
        a = self._as_actions(actions, K)
        if a.data_ptr() != actions.data_ptr():
            raise ValueError("rollout_plan: actions must already be a contiguous device tensor of the action dtype")
        if out is None:
            out = self._alloc_outputs(K)
        else:
            self._check_out(out, K)
        L, h = lib(), self._handle
        args = [ctypes.c_void_p(x.data_ptr()) for x in (a,) + tuple(out)]
        stream0 = torch.cuda.current_stream(self.device).cuda_stream
        fn = L.gp_rollout
        if hasattr(L, "gp_plan_create"):
            plan = ctypes.c_void_p()
            check(L.gp_plan_create(h, K, *args, stream0, ctypes.byref(plan)), "gp_plan_create")
            keep = _PlanKeep(plan, (a, out))
            fn_plan = L.gp_plan_run
        else:  # an older library chosen through GYM_PO_AMD_LIB (in-call A/B tooling)
            keep = _PlanKeep(None, (a, out))
            fn_plan = lambda _p: fn(h, K, *args, stream0)  # noqa: E731

        def run(stream=None):
            # the bound plan: one pointer across ctypes (another stream: the plain call with its arguments)
            rc = fn_plan(keep.plan) if stream is None else fn(h, K, *args, stream)
            if rc:
                check(rc, "gp_rollout")
            return keep.bufs
        return run, (out[0], out[1], out[2].view(torch.bool), out[3].view(torch.bool))

    # ------------------------------------------------------------------ closed loop ----
    _CTRL_OUTPUTS = ("obs", "actions", "nodes", "rew", "term", "trunc")

    def _ctrl_fn(self, name):
        fn = getattr(lib(), name, None)
        if fn is None:  # an older library chosen through GYM_PO_AMD_LIB
            raise _lib.GymPoError(f"{_lib.LIB_PATH} has no {name}: closed-loop rollouts need a current build")
        return fn

    def _controller_n_obs(self):
        """The number of scalar observations a controller table must cover (None: not checked on the host). Envs whose
        observation space does not carry it as `.n` (a one-hot encoding of a scalar obs) override this."""
        return getattr(getattr(self, "single_observation_space", None), "n", None)

    def set_controller(self, probs=None, thresholds=None):
        """Install the tabular controller of the closed-loop rollouts (FourRooms / ROOMS with a scalar obs in
        rng_mode='philox', RockSample, where A * M may not exceed 64, AntTagGridEnv with obs_type='index' in
        rng_mode='philox', TaxiVecEnv with hansen_obs=True in rng_mode='philox', scalar or one-hot: the table is
        indexed by the scalar Hansen obs either way, HeavenHellGridEnv with either obs_type, TabularPOMDPEnv (any
        model; A * M may not exceed 64; the obs conditioning a step is the env's stored last obs), and CRoomsEnv with
        action_type 'cardinal' (A = 4) or 'ordinal' (A = 8) and a scalar obs_type (hansen, hansen8, mdp, mdp_goal,
        room, room_goal) in rng_mode='philox'; its 'yx' actions, vector / grid obs and numpy / replay modes raise
        GymPoError naming the condition), or remove it when both arguments are None. `probs`: float [M, n_obs, A, M], the joint probability of (action, next node) given
        (node, obs), or [n_obs, A] for a memoryless policy; lowered by `controller.controller_thresholds`. `thresholds`: that uint32
        [M, n_obs, A * M] table itself. n_obs is `single_observation_space.n` (a one-hot Taxi's row width `no`), A the
        action count, M <= 8. Every env's node becomes 0. Raises GymPoError for a table that does not fit the env or
        is not monotone up to 2^31, and for envs without closed-loop rollouts."""
        fn = self._ctrl_fn("gp_set_controller")
        if probs is not None and thresholds is not None:
            raise ValueError("set_controller takes probs or thresholds, not both")
        if probs is None and thresholds is None:
            check(fn(self._handle, 0, 0, None), "gp_set_controller")
            return
        if probs is not None:
            from .controller import controller_thresholds
            thresholds = controller_thresholds(probs)
        t = np.ascontiguousarray(thresholds)
        if t.dtype != np.uint32 or t.ndim != 3:
            raise ValueError(f"thresholds must be a uint32 array [M, n_obs, A * M], got {t.dtype} {t.shape}")
        M, n_obs, L = t.shape
        A = getattr(getattr(self, "single_action_space", None), "n", None)
        if A is None or self._action_dtype != "int32":
            raise _lib.GymPoError("set_controller: the env has no discrete action space")
        if L != int(A) * M:
            raise _lib.GymPoError(f"set_controller: rows of a {M}-node controller over {int(A)} actions have "
                                  f"{int(A) * M} entries, got {L}")
        n_space = self._controller_n_obs()
        if n_space is not None and n_obs != int(n_space):
            raise _lib.GymPoError(f"set_controller: the table has n_obs = {n_obs}, the env's observation space "
                                  f"{int(n_space)}")
        check(fn(self._handle, M, n_obs, ctypes.c_void_p(t.ctypes.data)), "gp_set_controller")

    _SCORE_FIELDS = ("episodes", "return_sum", "length_sum", "env_steps", "discounted_return_sum")

    def set_controller_population(self, probs=None, thresholds=None, group_envs=None, gamma=1.0):
        """Install P controllers side by side (FourRooms / ROOMS with a scalar obs in rng_mode='philox'; every other
        env, HeavenHellGridEnv and CRoomsEnv included, raises GymPoError), or remove
        whatever controller is installed when `probs` and `thresholds` are both None. Env e is driven by controller
        e // group_envs; `controller_scores()` then gives one score row per controller, its discounted return under
        `gamma` (float32, in (0, 1]) included. `probs`: float [P, M, n_obs, A, M], lowered by
        `controller.population_thresholds`; `thresholds`: that uint32 [P, M, n_obs, A * M] table itself.
        `group_envs` must be a multiple of query('controller_group_multiple') (1024) that splits the envs into exactly
        P groups, the last one possibly short; None takes ceil(num_envs / P) rounded up to such a multiple and raises
        GymPoError if that does not give P groups. Replaces a controller installed by set_controller (and is replaced
        by it); every node and score becomes 0. rollout_controller() runs it like a single controller."""
        fn = self._ctrl_fn("gp_set_controller_population")
        if probs is not None and thresholds is not None:
            raise ValueError("set_controller_population takes probs or thresholds, not both")
        if probs is None and thresholds is None:
            check(fn(self._handle, 0, 0, 0, 0, 1.0, None), "gp_set_controller_population")
            return
        if probs is not None:
            from .controller import population_thresholds
            thresholds = population_thresholds(probs)
        t = np.ascontiguousarray(thresholds)
        if t.dtype != np.uint32 or t.ndim != 4 or t.shape[0] < 1:
            raise ValueError(f"thresholds must be a uint32 array [P, M, n_obs, A * M], got {t.dtype} {t.shape}")
        P, M, n_obs, L = t.shape
        A = getattr(getattr(self, "single_action_space", None), "n", None)
        if A is None or self._action_dtype != "int32":
            raise _lib.GymPoError("set_controller_population: the env has no discrete action space")
        if L != int(A) * M:
            raise _lib.GymPoError(f"set_controller_population: rows of a {M}-node controller over {int(A)} actions "
                                  f"have {int(A) * M} entries, got {L}")
        n_space = self._controller_n_obs()
        if n_space is not None and n_obs != int(n_space):
            raise _lib.GymPoError(f"set_controller_population: the tables have n_obs = {n_obs}, the env's observation "
                                  f"space {int(n_space)}")
        if group_envs is None:
            mult = 1024  # gp_query "controller_group_multiple" (asked below where the handle answers it)
            try:
                mult = self.query("controller_group_multiple")
            except _lib.GymPoError:
                pass  # another env kind: the call below says that populations are unsupported there
            per_group = -(-self.num_envs // P)  # ceil
            group_envs = -(-per_group // mult) * mult
            if -(-self.num_envs // group_envs) != P:
                raise _lib.GymPoError(f"set_controller_population: {self.num_envs} envs in groups of {group_envs} (the "
                                      f"next multiple of {mult}) do not make {P} groups; pass group_envs")
        check(fn(self._handle, P, int(group_envs), M, n_obs, float(gamma), ctypes.c_void_p(t.ctypes.data)),
              "gp_set_controller_population")

    def controller_scores(self, clear=False):
        """The per-controller scores of the installed population since reset() / the last clear (syncs): a dict of
        numpy arrays [P]: episodes, length_sum, env_steps (int64), return_sum and discounted_return_sum (float64).
        clear=True zeroes them after reading. Raises GymPoError without a population, or if a device-side failure
        invalidated the run (see check())."""
        fn = self._ctrl_fn("gp_controller_scores")
        try:
            P = self.query("controller_population")
        except _lib.GymPoError:
            P = 0  # another env kind: the call below says that populations are unsupported there
        buf = (ctypes.c_double * (5 * max(P, 1)))()
        check(fn(self._handle, buf, max(P, 1), int(bool(clear))), "gp_controller_scores")
        a = np.array(buf[:5 * P], dtype=np.float64).reshape(P, 5)
        sums = ("return_sum", "discounted_return_sum")  # float64; the three counts are exact integers
        return {name: (a[:, i].copy() if name in sums else a[:, i].astype(np.int64))
                for i, name in enumerate(self._SCORE_FIELDS)}

    def rollout_controller(self, K, out=None, store=_CTRL_OUTPUTS):
        """K closed-loop steps in ONE launch: each env's action is drawn on the device by the installed controller
        from the env's current observation and controller node (set_controller). Returns a dict of the outputs
        named in `store`: obs [K, B] (the env's obs dtype; uint8 [K, B, n_obs] for a one-hot Taxi), actions int32
        [K, B] (the actions taken), nodes uint8
        [K, B] (the node each action was chosen in), rew float32 [K, B], term / trunc bool [K, B]. Outputs left out
        of `store` are not written at all (store=() is a pure policy evaluation, read through metrics()). `out`
        may supply preallocated buffers as a dict by name (term / trunc as uint8), checked for shape, dtype, device
        and contiguity (ValueError otherwise). Feeding `actions` to rollout() on a twin env of the same seed
        reproduces obs, rew, term and trunc bit for bit (CRoomsEnv: the float64 positions and velocities of
        get_state() too)."""
        torch = _torch()
        fn = self._ctrl_fn("gp_rollout_controller")
        K = int(K)
        if K < 0:
            raise ValueError("K must be >= 0")
        store = tuple(store)
        for name in store:
            if name not in self._CTRL_OUTPUTS:
                raise ValueError(f"store: unknown output {name!r} (one of {self._CTRL_OUTPUTS})")
        lead = (K, self.num_envs)
        want = {"obs": ((K,) + self._obs_shape(), self._obs_dtype), "actions": (lead, torch.int32),
                "nodes": (lead, torch.uint8), "rew": (lead, torch.float32), "term": (lead, torch.uint8),
                "trunc": (lead, torch.uint8)}
        if out is not None and not isinstance(out, dict):
            raise ValueError("out must be a dict of tensors by output name")
        bufs = {}
        for name in store:
            shape, dt = want[name]
            t = None if out is None else out.get(name)
            if t is None:
                t = torch.empty(shape, dtype=dt, device=self.device)
            elif not isinstance(t, torch.Tensor):
                raise ValueError(f"out {name}: expected a torch tensor")
            elif tuple(t.shape) != shape or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"out {name}: need a contiguous {dt} tensor of shape {shape} on {self.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device} (contiguous={t.is_contiguous()})")
            bufs[name] = t
        ptr = lambda name: ctypes.c_void_p(bufs[name].data_ptr()) if name in bufs else None  # noqa: E731
        check(fn(self._handle, K, ptr("obs"), ptr("actions"), ptr("nodes"), ptr("rew"), ptr("term"), ptr("trunc"),
                 self._stream()), "gp_rollout_controller")
        res = dict(bufs)
        if "obs" in res:
            res["obs"] = self._post_obs(res["obs"])
        for name in ("term", "trunc"):
            if name in res:
                res[name] = res[name].view(torch.bool)
        return res

    @property
    def controller_nodes(self):
        """The controller node of every env, uint8 [B] on the device (a copy). Assigning an array-like [B] replaces
        them (values below the controller's node count); reset() and set_controller() zero them; step(), rollout()
        and CRoomsEnv.set_state() leave them alone."""
        torch = _torch()
        t = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        check(self._ctrl_fn("gp_controller_nodes")(self._handle, ctypes.c_void_p(t.data_ptr()), None, self._stream()),
              "gp_controller_nodes")
        return t

    @controller_nodes.setter
    def controller_nodes(self, nodes):
        torch = _torch()
        fn = self._ctrl_fn("gp_controller_nodes")
        if not isinstance(nodes, torch.Tensor) or nodes.device.type == "cpu":
            n = np.asarray(nodes.numpy() if isinstance(nodes, torch.Tensor) else nodes)
            M = self.query("controller_nodes")
            if n.size and M and (n.min() < 0 or n.max() >= M):
                raise ValueError(f"controller_nodes: values must be in [0, {M})")
            nodes = torch.as_tensor(n)
        t = nodes.to(device=self.device, dtype=torch.uint8).contiguous()
        if tuple(t.shape) != (self.num_envs,):
            raise ValueError(f"controller_nodes: need {self.num_envs} values, got shape {tuple(t.shape)}")
        check(fn(self._handle, None, ctypes.c_void_p(t.data_ptr()), self._stream()), "gp_controller_nodes")

    def _stats_plane(self, name, t, shape, dtypes, cast=None):
        """A plane of controller_statistics as a contiguous device tensor: `dtypes` are accepted as they are (a view
        at any storage offset included), `cast` = (kinds, dtype) converts those dtype kinds; ValueError otherwise."""
        torch = _torch()
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"controller_statistics: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        if t.dtype not in dtypes:
            if cast is None or not (t.dtype.is_floating_point or t.dtype in cast[0]):
                raise ValueError(f"controller_statistics: {name} must be {' or '.join(map(str, dtypes))}, got {t.dtype}")
            t = t.to(cast[1])
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        return t.to(self.device).contiguous()

    def controller_statistics(self, planes, obs0, next_nodes=None, gamma=1.0, bootstrap=None, into=None):
        """Visit counts and return-to-go sums per controller table cell over K stored closed-loop steps, accumulated
        on the device in ONE launch as exact integers (bit-reproducible: no float atomics): the sufficient statistics
        of a policy-gradient, Monte Carlo policy-iteration or EM step (`controller.q_estimate`, `policy_gradient`).

        `planes`: the dict rollout_controller(K) returned, all six entries (obs, actions, nodes, rew, term, trunc).
        obs must be a scalar [K, B] plane (a one-hot Taxi plane is a ValueError; other integer or float obs dtypes are
        cast to int32). `obs0` [B]: the obs before the first of the K steps (what reset() or the previous rollout's
        last obs row gave). `next_nodes` uint8 [B]: the controller nodes after the K-th step; None reads
        `controller_nodes` NOW, which is correct only when called right after the rollout that wrote `planes`, before
        any other closed-loop rollout, reset() or node assignment. `gamma`: float32 in (0, 1]. `bootstrap` float32 [B]
        or None (0): the value after the K-th step. `into`: a dict {"counts", "ret_q"} of int64 device tensors to
        accumulate into (the call adds); None makes fresh zeroed ones.

        Returns {"counts", "ret_q"}: int64 [M, n_obs, A, M + 1] ([P, ...] with a population; env e belongs to
        controller e // group_envs). The cell of step k is (nodes[k], the obs before it, actions[k], next node), the
        next node being nodes[k + 1] (next_nodes after the last step), or column M when the step ended the episode
        (terminated or truncated; the return stops there too). G_k = rew[k] + gamma * G_{k+1} in float32, two
        roundings; ret_q sums rint(G_k * 2^20) (`controller.stats_returns` scales back). An entry overflows once the
        sum of |G| over its visits reaches 2^43. A visit outside the table, or with |G| not below 2^31 (NaN included),
        is skipped and flags the handle: check() raises until the next seed. Raises GymPoError without an installed
        controller and on envs without closed-loop rollouts. Needs no reset(): only the planes are read."""
        torch = _torch()
        fn = self._ctrl_fn("gp_controller_stats")
        # the shape of what is installed (first: its errors say that the kind has no controllers, or that none is set)
        n_obs, A, M = (self.query(k) for k in ("controller_n_obs", "controller_actions", "controller_nodes"))
        if not isinstance(planes, dict) or any(n not in planes for n in self._CTRL_OUTPUTS):
            raise ValueError(f"controller_statistics: planes must be a dict with all of {self._CTRL_OUTPUTS}")
        obs = planes["obs"]
        if not isinstance(obs, torch.Tensor):
            obs = torch.as_tensor(np.asarray(obs))
        if obs.ndim != 2:
            raise ValueError(f"controller_statistics: obs must be a scalar [K, B] plane, got shape {tuple(obs.shape)} "
                             "(a one-hot obs plane is not supported: create the env with the scalar obs)")
        K, B = int(obs.shape[0]), self.num_envs
        ints = (torch.int64, torch.int16, torch.int8, torch.uint8)
        lead = (K, B)
        obs = self._stats_plane("obs", obs, lead, (torch.int32,), (ints, torch.int32))
        act = self._stats_plane("actions", planes["actions"], lead, (torch.int32,))
        nodes = self._stats_plane("nodes", planes["nodes"], lead, (torch.uint8,))
        rew = self._stats_plane("rew", planes["rew"], lead, (torch.float32,))
        term = self._stats_plane("term", planes["term"], lead, (torch.bool, torch.uint8))
        trunc = self._stats_plane("trunc", planes["trunc"], lead, (torch.bool, torch.uint8))
        o0 = self._stats_plane("obs0", obs0, (B,), (torch.int32,), (ints, torch.int32))
        if next_nodes is None:
            next_nodes = self.controller_nodes
        nn = self._stats_plane("next_nodes", next_nodes, (B,), (torch.uint8,))
        boot = None if bootstrap is None else self._stats_plane("bootstrap", bootstrap, (B,), (torch.float32,))
        try:
            P = self.query("controller_population")
        except _lib.GymPoError:
            P = 0  # a kind without populations
        shape = ((P,) if P else ()) + (M, n_obs, A, M + 1)
        if into is None:
            into = {n: torch.zeros(shape, dtype=torch.int64, device=self.device) for n in ("counts", "ret_q")}
        else:
            if not isinstance(into, dict) or any(n not in into for n in ("counts", "ret_q")):
                raise ValueError("controller_statistics: into must be a dict with 'counts' and 'ret_q'")
            for n in ("counts", "ret_q"):
                t = into[n]
                if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.int64
                        or t.device != self.device or not t.is_contiguous()):
                    raise ValueError(f"controller_statistics: into[{n!r}] must be a contiguous int64 tensor of shape "
                                     f"{shape} on {self.device}")
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        check(fn(self._handle, K, ptr(o0), ptr(obs), ptr(act), ptr(nodes), ptr(nn), ptr(rew), ptr(term), ptr(trunc),
                 ptr(boot), float(gamma), ptr(into["counts"]), ptr(into["ret_q"]), self._stream()),
              "gp_controller_stats")
        return {"counts": into["counts"], "ret_q": into["ret_q"]}

    def autotune(self, K=20, reps=5):
        """Pick, on this device, the faster of the handle's interchangeable kernels for launches of K steps
        (numpy-mode FourRooms/ROOMS: the windowed and the fused kernel, bit-identical results) by timing `reps`
        launches of each on scratch state; the env's own state, stream position and metrics are left exactly as
        they were. Returns 1 (windowed), 0 (fused) or -1 (nothing to choose). After reset(); syncs."""
        chosen = ctypes.c_int(-1)
        check(lib().gp_autotune(self._handle, int(K), int(reps), ctypes.byref(chosen)), "gp_autotune")
        return chosen.value

    def check(self):
        """Sync and raise GymPoError if a device-side failure hit any launch since the last seed (the
        asynchronous step/rollout calls cannot report it themselves; metrics() and rng_state check too)."""
        check(lib().gp_check(self._handle), "gp_check")

    def query(self, key):
        """Handle introspection (gp_query), e.g. 'fused_blocks', 'fused_staged'."""
        v = ctypes.c_int64()
        check(lib().gp_query(self._handle, key.encode(), ctypes.byref(v)), "gp_query")
        return v.value

    def step_raw(self, a, obs, rew, term, trunc, stream=None):
        """Allocation-free step into caller buffers (all device tensors; term/trunc uint8)."""
        st = self._stream() if stream is None else ctypes.c_void_p(stream)
        check(lib().gp_step(self._handle, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(obs.data_ptr()),
                            ctypes.c_void_p(rew.data_ptr()), ctypes.c_void_p(term.data_ptr()),
                            ctypes.c_void_p(trunc.data_ptr()), st), "gp_step")

    # ------------------------------------------------------------------ state / replay ----
    def _get_state_raw(self, bufs):
        ptrs = [ctypes.c_void_p(b.data_ptr()) if b is not None else None for b in bufs]
        ptrs += [None] * (4 - len(ptrs))
        check(lib().gp_get_state(self._handle, *ptrs, self._stream()), "gp_get_state")

    def _set_state_raw(self, bufs):
        """gp_set_state from device tensors (the dtypes of get_state(), None leaves a field alone): asynchronous on the
        current stream. The envs' public set_state(...) wrappers accept host arrays, so they upload, call this and then
        synchronise the current stream before they return (Streams)."""
        ptrs = [ctypes.c_void_p(b.data_ptr()) if b is not None else None for b in bufs]
        ptrs += [None] * (4 - len(ptrs))
        check(lib().gp_set_state(self._handle, *ptrs, self._stream()), "gp_set_state")

    def set_replay(self, u=None, i0=None, i1=None, f0=None, f1=None):
        """Pre-decided per-env draws for the next step/reset (rng_mode='replay')."""
        keep = [x for x in (u, i0, i1, f0, f1) if x is not None]
        self._replay_keep = keep  # keep the tensors alive until the step is enqueued
        ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
        check(lib().gp_set_replay(self._handle, ptr(u), ptr(i0), ptr(i1), ptr(f0), ptr(f1)), "gp_set_replay")

    def valid_cells(self, which):
        buf = (ctypes.c_int32 * 65536)()
        n = lib().gp_valid_cells(self._handle, which, buf, 65536)
        return np.array(buf[:n], dtype=np.int64)

    def metrics(self):
        """{episodes, return_sum, length_sum, env_steps} accumulated on device since reset (syncs; raises
        GymPoError if a device-side failure invalidated the run, see check())."""
        out = (ctypes.c_double * 4)()
        check(lib().gp_metrics(self._handle, out), "gp_metrics")
        return dict(episodes=out[0], return_sum=out[1], length_sum=out[2], env_steps=out[3])

    def set_profiling(self, enable=True):
        check(lib().gp_set_profiling(self._handle, int(bool(enable))), "gp_set_profiling")

    def profile_read(self):
        """(summed step-kernel ms, launches) since the last read (syncs)."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        check(lib().gp_profile_read(self._handle, ctypes.byref(ms), ctypes.byref(n)), "gp_profile_read")
        return ms.value, n.value

    def profile_read_resolver(self):
        """(summed reset-resolver-kernel ms, launches) since the last read (syncs; numpy mode)."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        check(lib().gp_profile_read_resolver(self._handle, ctypes.byref(ms), ctypes.byref(n)),
              "gp_profile_read_resolver")
        return ms.value, n.value

    def render(self):
        """The reference renders none of the grid / continuous envs (msrooms.py:430-432 raises, RoomsEnv and
        CRoomsEnv inherit gymnasium's NotImplementedError); TaxiVecEnv overrides this."""
        raise NotImplementedError("render() is not implemented for this env (nor in the reference)")
