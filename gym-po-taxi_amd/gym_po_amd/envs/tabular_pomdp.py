"""Tabular POMDP — a finite POMDP given as its tables (Cassandra's T / O / R), run by one kernel whose dynamics are the
tables themselves (csrc/pomdp.hip). Build-defined: there is no reference env, the device is pinned to the
numpy restatement of the rules under tests/. Every feature of the on-device finite-state controllers (set_controller,
rollout_controller, controller_statistics, q_estimate, policy_gradient) works on it, so any finite POMDP (Tiger,
Hallway, Tag, ...) runs closed loop without a kernel of its own.

Rules: in state s under action a the next state s' is drawn from T[s, a], the reward is R[s, a, s'], the episode
terminates iff terminal[s'] and is truncated after time_limit steps (gymnasium TimeLimit); if it goes on, the obs is
drawn from Z[a, s']. An episode end resets the env in the same step: s0 from `start`, the obs from reset_obs[s0]. The
probabilities are lowered to integers on the host (`row_thresholds`: cumulative sums scaled to 2^31) and the device
compares 31-bit Philox draws against them: no float arithmetic decides an outcome.
"""
import ctypes

import numpy as np

from .. import _lib
from ..core import NativeVecEnv, _torch
from ..spaces import Discrete, batch_space

TOP = 1 << 31
MAX_STATES, MAX_ACTIONS, MAX_OBS = 65536, 64, 65536


def row_thresholds(p):
    """Float rows along the last axis -> uint32 thresholds of the same shape, by `controller_thresholds`' rule: entry j
    of a row is floor(C_j * 2^31), C the float64 sequential cumulative sum of the row, and 2^31 from the row's last
    nonzero entry on, so that every row ends at exactly 2^31 and an outcome of probability zero has an empty interval.
    Raises ValueError, naming the row, for negative (or NaN) entries and for a row whose sum is off 1 by more than
    1e-6."""
    p = np.asarray(p, dtype=np.float64)
    if p.ndim < 1 or p.shape[-1] < 1 or p.size == 0:
        raise ValueError(f"rows need at least one entry, got shape {p.shape}")
    ok = p >= 0  # (NaN fails the comparison too)
    if not np.all(ok):
        row = np.unravel_index(int(np.argmin(ok.all(-1))), p.shape[:-1])
        raise ValueError(f"row {tuple(int(i) for i in row)} has negative (or NaN) entries")
    off = np.abs(p.sum(-1) - 1.0)
    if not np.all(off <= 1e-6):
        row = np.unravel_index(int(np.argmax(off)), off.shape)
        raise ValueError(f"row {tuple(int(i) for i in row)} sums to {float(p[row].sum())!r}, not 1")
    c = np.cumsum(p, axis=-1)  # sequential float64 adds, in index order
    t = np.minimum(np.floor(c * float(TOP)), float(TOP)).astype(np.uint64)
    L = p.shape[-1]
    last = (L - 1) - np.argmax(p[..., ::-1] > 0, axis=-1)  # the last nonzero entry of each row
    t[np.arange(L) >= last[..., None]] = TOP
    return t.astype(np.uint32)


def _named(name, fn, x):
    try:
        return fn(x)
    except ValueError as e:
        raise ValueError(f"{name}: {e}") from None


class TabularPOMDPEnv(NativeVecEnv):
    """T float [S, A, S] (s, a, s'), Z float [A, S, O] (a, s', o: Cassandra's `O: a : s' : o`), R [S, A] (the same for
    every s') or [S, A, S]; start [S] (None: uniform), terminal bool [S] (None: no terminal state), reset_obs [S, O]
    (the law of an episode's first obs given its start state; None: uniform over O, which carries no information).
    1 <= S <= 65,536, 1 <= A <= 64, 1 <= O <= 65,536, time_limit in [1, 65,535]. rng_mode: 'philox' only (there is no
    reference stream to follow or replay). The lowered integer tables are kept as attributes (trans_thr, obs_thr,
    start_thr, reset_obs_thr, reward, terminal)."""
    metadata = {"render_modes": [], "name": "TabularPOMDP"}

    def __init__(self, num_envs, T, Z, R, start=None, terminal=None, reset_obs=None, time_limit=500, device=None,
                 rng_mode="philox"):
        T = np.asarray(T, dtype=np.float64)
        if T.ndim != 3 or T.shape[0] != T.shape[2] or T.shape[0] < 1 or T.shape[1] < 1:
            raise ValueError(f"T must be [S, A, S], got shape {T.shape}")
        S, A, _ = T.shape
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 3 or Z.shape[:2] != (A, S) or Z.shape[2] < 1:
            raise ValueError(f"Z must be [A, S, O] = [{A}, {S}, O], got shape {Z.shape}")
        O = Z.shape[2]
        if S > MAX_STATES or A > MAX_ACTIONS or O > MAX_OBS:
            raise ValueError(f"T, Z: sizes (S {S}, A {A}, O {O}) above ({MAX_STATES}, {MAX_ACTIONS}, {MAX_OBS})")
        R = np.asarray(R, dtype=np.float32)
        if R.shape == (S, A):
            R = np.broadcast_to(R[:, :, None], (S, A, S))
        if R.shape != (S, A, S):
            raise ValueError(f"R must be [S, A] or [S, A, S] = [{S}, {A}(, {S})], got shape {R.shape}")
        start = np.full(S, 1.0 / S) if start is None else np.asarray(start, dtype=np.float64)
        if start.shape != (S,):
            raise ValueError(f"start must be [S] = [{S}], got shape {start.shape}")
        terminal = np.zeros(S, dtype=bool) if terminal is None else np.asarray(terminal)
        if terminal.shape != (S,):
            raise ValueError(f"terminal must be [S] = [{S}], got shape {terminal.shape}")
        reset_obs = np.full((S, O), 1.0 / O) if reset_obs is None else np.asarray(reset_obs, dtype=np.float64)
        if reset_obs.shape != (S, O):
            raise ValueError(f"reset_obs must be [S, O] = [{S}, {O}], got shape {reset_obs.shape}")
        time_limit = int(time_limit)
        if not 1 <= time_limit <= 65535:
            raise ValueError(f"time_limit must be in [1, 65535], got {time_limit}")
        self._build(num_envs, _named("T", row_thresholds, T), _named("Z", row_thresholds, Z),
                    _named("start", row_thresholds, start), _named("reset_obs", row_thresholds, reset_obs), R, terminal,
                    time_limit, device, rng_mode)

    @classmethod
    def from_thresholds(cls, num_envs, trans_thr, obs_thr, start_thr, reset_obs_thr, reward, terminal, time_limit=500,
                        device=None, rng_mode="philox"):
        """An env from the integer tables themselves (uint32 [S, A, S], [A, S, O], [S], [S, O]; reward float32
        [S, A, S]; terminal [S]): what `__init__` lowers its probabilities to. The library validates the rows
        (GymPoError naming the table and the row)."""
        env = cls.__new__(cls)
        t = [np.asarray(x) for x in (trans_thr, obs_thr, start_thr, reset_obs_thr)]
        if t[0].ndim != 3 or t[0].shape[0] != t[0].shape[2]:
            raise ValueError(f"trans_thr must be [S, A, S], got shape {t[0].shape}")
        S, A, _ = t[0].shape
        if t[1].ndim != 3 or t[1].shape[:2] != (A, S):
            raise ValueError(f"obs_thr must be [A, S, O] = [{A}, {S}, O], got shape {t[1].shape}")
        O = t[1].shape[2]
        if t[2].shape != (S,) or t[3].shape != (S, O) or np.shape(reward) != (S, A, S) or np.shape(terminal) != (S,):
            raise ValueError(f"start_thr, reset_obs_thr, reward, terminal must be [{S}], [{S}, {O}], [{S}, {A}, {S}], "
                             f"[{S}], got {t[2].shape}, {t[3].shape}, {np.shape(reward)}, {np.shape(terminal)}")
        env._build(num_envs, *t, np.asarray(reward), np.asarray(terminal), int(time_limit), device, rng_mode)
        return env

    def _build(self, num_envs, trans_thr, obs_thr, start_thr, reset_obs_thr, reward, terminal, time_limit, device,
               rng_mode):
        S, A, O = trans_thr.shape[0], trans_thr.shape[1], obs_thr.shape[2]
        self.n_states, self.n_actions, self.n_obs = S, A, O
        self.trans_thr = np.ascontiguousarray(trans_thr, dtype=np.uint32)
        self.obs_thr = np.ascontiguousarray(obs_thr, dtype=np.uint32)
        self.start_thr = np.ascontiguousarray(start_thr, dtype=np.uint32)
        self.reset_obs_thr = np.ascontiguousarray(reset_obs_thr, dtype=np.uint32)
        self.reward = np.ascontiguousarray(reward, dtype=np.float32)
        self.terminal = np.ascontiguousarray(terminal.astype(bool).astype(np.uint8))
        self.time_limit = time_limit
        self.num_envs = num_envs
        self.is_vector_env = True
        self.single_action_space = Discrete(A)
        self.action_space = batch_space(self.single_action_space, num_envs)
        self.single_observation_space = Discrete(O)
        self.observation_space = batch_space(self.single_observation_space, num_envs)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        cfg = _lib.PomdpConfig()
        cfg.n_states, cfg.n_actions, cfg.n_obs, cfg.time_limit = S, A, O, time_limit
        cfg.trans_thr = self.trans_thr.ctypes.data_as(u32p)
        cfg.obs_thr = self.obs_thr.ctypes.data_as(u32p)
        cfg.start_thr = self.start_thr.ctypes.data_as(u32p)
        cfg.reset_obs_thr = self.reset_obs_thr.ctypes.data_as(u32p)
        cfg.reward = self.reward.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        cfg.terminal = self.terminal.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        self._create(_lib.GP_KIND_POMDP, cfg, num_envs, device, rng_mode)

    @classmethod
    def from_pomdp(cls, text, num_envs, terminal=None, **kw):
        """An env from a model in Cassandra's text format (`pomdp_file.parse_pomdp`: the accepted subset). The format
        has no terminal states: `terminal` (bool [S]) names them. The parsed dict is kept as `.model`."""
        from ..pomdp_file import parse_pomdp
        m = parse_pomdp(text)
        env = cls(num_envs, m["T"], m["Z"], m["R"], start=m["start"], terminal=terminal, **kw)
        env.model = m
        return env

    def reset(self, *, seed=None, options=None):
        return self._reset_impl(seed), {}

    def get_state(self):
        """(state, elapsed, last obs) int32 [B]."""
        torch = _torch()
        s, e, o = (torch.empty(self.num_envs, dtype=torch.int32, device=self.device) for _ in range(3))
        self._get_state_raw([s, e, o])
        return s, e, o

    def set_state(self, state=None, elapsed=None, obs=None):
        """Replace the given fields (None leaves one alone): the state is clamped to [0, S), elapsed to [0, 65535], the
        obs to [0, O)."""
        torch = _torch()
        conv = lambda x: None if x is None else torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, device=self.device).to(torch.int32).contiguous()  # noqa: E731
        self._set_state_raw([conv(state), conv(elapsed), conv(obs)])
        torch.cuda.current_stream(self.device).synchronize()

    # ------------------------------------------------------------------ belief filter ----
    # An exact Bayes filter kept per env on the device and a piecewise-linear (alpha-vector) policy over it
    # (csrc/pomdp.hip; the rules are stated in include/gym_po_amd.h). reset() sets every belief from
    # the prior and the reset obs; step(), rollout(), rollout_controller() and set_state() leave the beliefs alone, as
    # they leave controller nodes alone: belief_filter() advances them over the planes those calls wrote.
    _BELIEF_OUTPUTS = ("obs", "actions", "vec", "value", "rew", "term", "trunc")

    def enable_belief(self, prior=None):
        """Start tracking a belief [S] per env. `prior` [S]: the law of an episode's start state as the agent knows it
        (validated: finite, >= 0, a positive sum; then normalised in float32 by the filter's sequential sum); None: the
        env's start law as the filter's float32 law. Every belief is set from the prior and the env's stored obs, as
        reset() does from then on. S <= 4,096. Calling it again replaces the prior."""
        from ..belief import normalise_belief
        fn = self._ctrl_fn("gp_belief_enable")
        if prior is None:
            _lib.check(fn(self._handle, None), "gp_belief_enable")
            return
        p = np.asarray(prior)
        if p.shape != (self.n_states,):
            raise ValueError(f"prior must be [S] = [{self.n_states}], got shape {p.shape}")
        p = np.ascontiguousarray(_named("prior", normalise_belief, p))
        _lib.check(fn(self._handle, ctypes.c_void_p(p.ctypes.data)), "gp_belief_enable")

    def disable_belief(self):
        """Stop tracking beliefs and free them (an installed policy stays)."""
        _lib.check(self._ctrl_fn("gp_belief_disable")(self._handle), "gp_belief_disable")

    @property
    def belief(self):
        """The belief of every env, float32 [B, S] on the device (a copy)."""
        torch = _torch()
        t = torch.empty((self.num_envs, self.n_states), dtype=torch.float32, device=self.device)
        _lib.check(self._ctrl_fn("gp_belief_get")(self._handle, ctypes.c_void_p(t.data_ptr()), self._stream()),
                   "gp_belief_get")
        return t

    def set_belief(self, b):
        """Replace the beliefs by `b` [B, S] (float32 values are stored as given). ValueError for entries that are
        negative or not finite and for a row whose sum is not positive."""
        torch = _torch()
        t = b if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b, dtype=np.float32))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(t.shape) != (self.num_envs, self.n_states):
            raise ValueError(f"set_belief: need [B, S] = [{self.num_envs}, {self.n_states}], got {tuple(t.shape)}")
        if not bool((torch.isfinite(t) & (t >= 0)).all()) or not bool((t.sum(-1) > 0).all()):
            raise ValueError("set_belief: entries must be finite and >= 0, and every row needs a positive sum")
        _lib.check(self._ctrl_fn("gp_belief_set")(self._handle, ctypes.c_void_p(t.data_ptr()), self._stream()),
                   "gp_belief_set")
        torch.cuda.current_stream(self.device).synchronize()

    def belief_filter(self, actions, obs=None, term=None, trunc=None):
        """Advance the stored beliefs over K stored steps: `actions` int32 [K, B], `obs` int32 [K, B] (the obs after
        each step), `term` / `trunc` bool or uint8 [K, B], whoever wrote them (rollout(), rollout_controller(), a
        replay); or, as the only argument, the dict rollout_controller() / rollout_belief() returned. A pure function
        of the planes and the stored beliefs: the env's state is not read. Actions wrap and clamp as in step(), obs
        values outside [0, O) are clamped; both are flagged (check())."""
        torch = _torch()
        if isinstance(actions, dict):
            d = actions
            if obs is not None or term is not None or trunc is not None:
                raise ValueError("belief_filter: a dict of planes is the only argument")
            missing = [n for n in ("actions", "obs", "term", "trunc") if n not in d]
            if missing:
                raise ValueError(f"belief_filter: the dict lacks {missing}")
            actions, obs, term, trunc = d["actions"], d["obs"], d["term"], d["trunc"]
        elif obs is None or term is None or trunc is None:
            raise ValueError("belief_filter: needs actions, obs, term and trunc")

        def plane(name, x, dt):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
            if dt is torch.uint8 and t.dtype == torch.bool:
                t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
            t = t.to(device=self.device, dtype=dt).contiguous()
            if t.dim() != 2 or t.shape[1] != self.num_envs:
                raise ValueError(f"belief_filter: {name} must be [K, B] = [K, {self.num_envs}], got {tuple(t.shape)}")
            return t
        a, o = plane("actions", actions, torch.int32), plane("obs", obs, torch.int32)
        tm, tr = plane("term", term, torch.uint8), plane("trunc", trunc, torch.uint8)
        K = a.shape[0]
        if not (o.shape[0] == tm.shape[0] == tr.shape[0] == K):
            raise ValueError("belief_filter: the planes differ in K")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(self._ctrl_fn("gp_belief_filter")(self._handle, K, ptr(a), ptr(o), ptr(tm), ptr(tr), self._stream()),
                   "gp_belief_filter")

    def set_belief_policy(self, alpha=None, actions=None):
        """Install a piecewise-linear policy over the belief: `alpha` [N, S] (finite, |alpha| <= 1e30; stored as
        float32) and `actions` int [N] in [0, A), the action of each vector (None: arange(N), which needs N == A, the
        layout of `belief.qmdp_vectors`). The action of a step is that of the first vector that attains
        max_j sum_s b[s] alpha[j, s] on the belief before the step. N <= 4,096 and N * S <= 2^22. alpha=None removes
        the policy."""
        fn = self._ctrl_fn("gp_set_belief_policy")
        if alpha is None:
            _lib.check(fn(self._handle, 0, None, None), "gp_set_belief_policy")
            return
        al = np.ascontiguousarray(np.asarray(alpha, dtype=np.float32))
        if al.ndim != 2 or al.shape[1] != self.n_states or al.shape[0] < 1:
            raise ValueError(f"alpha must be [N, S] = [N, {self.n_states}], got shape {al.shape}")
        N = al.shape[0]
        if actions is None:
            if N != self.n_actions:
                raise ValueError(f"set_belief_policy: {N} vectors and {self.n_actions} actions: name each vector's action")
            actions = np.arange(N)
        va = np.asarray(actions)
        if va.shape != (N,) or va.dtype.kind not in "iu":
            raise ValueError(f"actions must be integers [N] = [{N}], got {va.dtype} {va.shape}")
        va = np.ascontiguousarray(va.astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32))
        _lib.check(fn(self._handle, N, ctypes.c_void_p(al.ctypes.data), ctypes.c_void_p(va.ctypes.data)),
                   "gp_set_belief_policy")

    def rollout_belief(self, K, out=None, store=_BELIEF_OUTPUTS):
        """K closed-loop steps in ONE launch: each env's action is chosen on the device by the installed alpha-vector
        policy from the env's belief, the env steps, and the belief is updated from the action and the new obs.
        Returns a dict of the outputs named in `store`: obs int32 [K, B], actions int32 [K, B], vec int32 [K, B] (the
        index of the maximising vector), value float32 [K, B] (its value on the belief before the step), rew float32
        [K, B], term / trunc bool [K, B]. `out`, `store`, dtypes and the bool views follow rollout_controller(). No
        random draw is spent on the choice: rollout() of `actions` on a twin env of the same seed reproduces every
        output, the state and the metrics bit for bit."""
        torch = _torch()
        fn = self._ctrl_fn("gp_rollout_belief")
        K = int(K)
        if K < 0:
            raise ValueError("K must be >= 0")
        store = tuple(store)
        for name in store:
            if name not in self._BELIEF_OUTPUTS:
                raise ValueError(f"store: unknown output {name!r} (one of {self._BELIEF_OUTPUTS})")
        lead = (K, self.num_envs)
        want = {"obs": (lead, torch.int32), "actions": (lead, torch.int32), "vec": (lead, torch.int32),
                "value": (lead, torch.float32), "rew": (lead, torch.float32), "term": (lead, torch.uint8),
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
        _lib.check(fn(self._handle, K, ptr("obs"), ptr("actions"), ptr("vec"), ptr("value"), ptr("rew"), ptr("term"),
                      ptr("trunc"), self._stream()), "gp_rollout_belief")
        res = dict(bufs)
        for name in ("term", "trunc"):
            if name in res:
                res[name] = res[name].view(torch.bool)
        return res

    # ------------------------------------------------------------------ point-based backup ----
    _BACKUP_OUTPUTS = ("alpha", "actions", "value")

    def point_backup(self, points, alpha, gamma=0.95, out=None):
        """One point-based value backup (csrc/pomdp_backup.hip; the rule is stated in
        include/gym_po_amd.h): for every belief point the best one-step look-ahead vector over the set `alpha`.
        `points` [P, S] (validated as set_belief validates beliefs: finite, >= 0, a positive sum per row; not
        normalised), `alpha` [N, S] (finite, |alpha| <= 1e30; taken as float32), `gamma` in [0, 1]. Returns a dict of
        alpha float32 [P, S], actions int32 [P] and value float32 [P] on the device; `out` may hold contiguous tensors
        of these shapes to write into. Needs enable_belief() (the float laws live there); reads the model only."""
        torch = _torch()
        fn = self._ctrl_fn("gp_belief_backup")
        S = self.n_states
        t = points if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points, dtype=np.float32))
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if t.dim() != 2 or t.shape[1] != S:
            raise ValueError(f"point_backup: points must be [P, S] = [P, {S}], got {tuple(t.shape)}")
        if t.shape[0] and (not bool((torch.isfinite(t) & (t >= 0)).all()) or not bool((t.sum(-1) > 0).all())):
            raise ValueError("point_backup: points must be finite and >= 0, and every row needs a positive sum")
        al = np.ascontiguousarray(np.asarray(alpha.cpu() if isinstance(alpha, torch.Tensor) else alpha,
                                             dtype=np.float32))
        if al.ndim != 2 or al.shape[1] != S or al.shape[0] < 1:
            raise ValueError(f"point_backup: alpha must be [N, S] = [N, {S}] with N >= 1, got shape {al.shape}")
        P = t.shape[0]
        want = {"alpha": ((P, S), torch.float32), "actions": ((P,), torch.int32), "value": ((P,), torch.float32)}
        if out is not None and not isinstance(out, dict):
            raise ValueError("out must be a dict of tensors by output name")
        bufs = {}
        for name in self._BACKUP_OUTPUTS:
            shape, dt = want[name]
            b = None if out is None else out.get(name)
            if b is None:
                b = torch.empty(shape, dtype=dt, device=self.device)
            elif not isinstance(b, torch.Tensor):
                raise ValueError(f"out {name}: expected a torch tensor")
            elif tuple(b.shape) != shape or b.dtype != dt or b.device != self.device or not b.is_contiguous():
                raise ValueError(f"out {name}: need a contiguous {dt} tensor of shape {shape} on {self.device}, got "
                                 f"{b.dtype} {tuple(b.shape)} on {b.device} (contiguous={b.is_contiguous()})")
            bufs[name] = b
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        _lib.check(fn(self._handle, P, ptr(t), al.shape[0], ctypes.c_void_p(al.ctypes.data), float(gamma),
                      ptr(bufs["alpha"]), ptr(bufs["actions"]), ptr(bufs["value"]), self._stream()),
                   "gp_belief_backup")
        # (the launches read `t` on the current stream: the caching allocator hands its memory out again only to
        # work queued behind them on that stream)
        return bufs

    # ------------------------------------------------------------------ belief-set expansion ----
    _EXPAND_OUTPUTS = ("succ", "dist", "actions", "obs", "mass")

    def expand_beliefs(self, points, ref=None, out=None):
        """One belief-set expansion (csrc/pomdp_expand.hip; the rule is stated in
        include/gym_po_amd.h): for every belief point the successor b' under the filter, over every action and obs of
        positive probability, whose L1 distance to the nearest row of `ref` is largest (the first such, actions then
        obs ascending). `points` [P, S] and `ref` [Q, S] with Q >= 1 (None: the points themselves) are validated as
        point_backup validates points (finite, >= 0, a positive sum per row) and not normalised. Returns a dict of succ
        float32 [P, S], dist float32 [P], actions int32 [P], obs int32 [P] and mass float32 [P] (the probability of
        that obs) on the device; `out` may hold contiguous tensors of these shapes to write into. A point without a
        successor of positive probability gives actions = obs = -1, dist = mass = 0 and a row of zeros. dist == 0
        everywhere says that the set is closed under the filter's successors. Needs enable_belief(); reads the model
        only; asynchronous on the current stream."""
        torch = _torch()
        fn = self._ctrl_fn("gp_belief_expand")
        S = self.n_states

        def rows(name, n, x):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
            if t.dim() != 2 or t.shape[1] != S:
                raise ValueError(f"expand_beliefs: {name} must be [{n}, S] = [{n}, {S}], got {tuple(t.shape)}")
            if t.shape[0] and (not bool((torch.isfinite(t) & (t >= 0)).all()) or not bool((t.sum(-1) > 0).all())):
                raise ValueError(f"expand_beliefs: {name} must be finite and >= 0, and every row needs a positive sum")
            return t
        t = rows("points", "P", points)
        q = None if ref is None else rows("ref", "Q", ref)
        if q is not None and q.shape[0] < 1:
            raise ValueError("expand_beliefs: ref must have at least one row (None: the points themselves)")
        P = t.shape[0]
        want = {"succ": ((P, S), torch.float32), "dist": ((P,), torch.float32), "actions": ((P,), torch.int32),
                "obs": ((P,), torch.int32), "mass": ((P,), torch.float32)}
        if out is not None and not isinstance(out, dict):
            raise ValueError("out must be a dict of tensors by output name")
        bufs = {}
        for name in self._EXPAND_OUTPUTS:
            shape, dt = want[name]
            b = None if out is None else out.get(name)
            if b is None:
                b = torch.empty(shape, dtype=dt, device=self.device)
            elif not isinstance(b, torch.Tensor):
                raise ValueError(f"out {name}: expected a torch tensor")
            elif tuple(b.shape) != shape or b.dtype != dt or b.device != self.device or not b.is_contiguous():
                raise ValueError(f"out {name}: need a contiguous {dt} tensor of shape {shape} on {self.device}, got "
                                 f"{b.dtype} {tuple(b.shape)} on {b.device} (contiguous={b.is_contiguous()})")
            bufs[name] = b
        ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        _lib.check(fn(self._handle, P, ptr(t), 0 if q is None else q.shape[0], None if q is None else ptr(q),
                      ptr(bufs["succ"]), ptr(bufs["dist"]), ptr(bufs["actions"]), ptr(bufs["obs"]), ptr(bufs["mass"]),
                      self._stream()), "gp_belief_expand")
        # (the launches read `t` and `q` on the current stream: the caching allocator hands their memory out again
        # only to work queued behind them on that stream)
        return bufs


def heaven_hell_pomdp(env):
    """(T, Z, R, start, terminal, reset_obs) of a `HeavenHellGridEnv`: the same task as tables. S = 2 H W with state =
    side * H W + cell, A = 4, O = the env's obs count. Under action a the move made is a with probability 1 - p and
    each of the three others with p / 3 (p = action_failure_probability). The reward is a function of (s, s'): entering
    (or staying in) the left or right area pays heaven_reward or hell_reward by the side, staying put anywhere else
    wall_reward, any other move step_reward. Z and reset_obs are 0 / 1 rows of the env's obs; the start law is uniform
    over start cells x sides. Wall cells are states no episode reaches: they loop onto themselves."""
    from .heaven_hell_grid import FLAG_FREE, FLAG_LEFT, FLAG_PRIEST, FLAG_RIGHT
    H, W = env.map_size
    n = H * W
    flags = np.asarray(env.flags, dtype=np.int64)
    base = np.asarray(env.obs_base, dtype=np.int64)
    p = float(env.action_failure_probability)
    r = env.rewards
    S, A, O = 2 * n, 4, int(env.obs_base_n) * 3
    free = (flags & FLAG_FREE) != 0
    row, col = np.divmod(np.arange(n), W)
    target = np.empty((n, A), dtype=np.int64)  # the cell a move ends in
    for a, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
        rr, cc = row + dr, col + dc
        inside = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
        t = np.where(inside, rr * W + cc, np.arange(n))
        target[:, a] = np.where(free & inside & free[t], t, np.arange(n))
    keep = np.zeros((S, A, S), dtype=np.int64)  # 1 where the intended move lands
    slip = np.zeros((S, A, S), dtype=np.int64)  # how many of the three other moves land there
    for side in range(2):
        s = side * n + np.arange(n)
        for a in range(A):
            keep[s, a, side * n + target[:, a]] += 1
            for b in range(A):
                if b != a:
                    np.add.at(slip, (s, a, side * n + target[:, b]), 1)
    T = keep * (1.0 - p) + slip * (p / 3.0)
    cell = np.arange(S) % n
    side = np.arange(S) // n
    in_left, in_right = (flags[cell] & FLAG_LEFT) != 0, (flags[cell] & FLAG_RIGHT) != 0
    terminal = in_left | in_right
    arrive = np.where(terminal, np.where(np.where(side == 0, in_left, in_right), r["heaven_reward"], r["hell_reward"]),
                      r["step_reward"])  # by s'
    R = np.broadcast_to(arrive[None, None, :], (S, A, S)).astype(np.float32).copy()
    stay = np.arange(S)
    R[stay, :, stay] = np.where(terminal, arrive, r["wall_reward"]).astype(np.float32)[:, None]
    obs = base[cell] * 3 + np.where((flags[cell] & FLAG_PRIEST) != 0, 1 + side, 0)
    reset_obs = np.zeros((S, O))
    reset_obs[np.arange(S), obs] = 1.0
    Z = np.broadcast_to(reset_obs[None], (A, S, O)).copy()
    starts = np.asarray(env.start_cells, dtype=np.int64)
    start = np.zeros(S)
    start[np.concatenate((starts, n + starts))] = 1.0 / (2 * len(starts))
    return T, Z, R, start, terminal, reset_obs
