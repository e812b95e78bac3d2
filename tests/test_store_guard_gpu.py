"""Every entry point writes exactly the documented bytes, whatever the pointer's alignment and whatever B.

A caller's buffer is a torch tensor that the caching allocator places next to other live tensors: a store a few bytes
outside the documented shape faults nowhere and shows in no value comparison. Here every buffer handed to the library is
a view cut from a larger allocation (tests/store_guard.py): guard bytes (0xA5) on both sides, each at least one [B, ...]
plane long, the view itself pre-filled with poison (0x5A), its address a chosen number of bytes past a 16-B boundary.
After the call the guards must be intact, the view must equal a same-seed twin handle that ran the same call on
ordinary aligned allocations (the values the rest of the suite pins to the oracles), bit for bit through the byte view,
and no expected element may carry the poison pattern, so that equality implies that every element was stored. Inputs
are guarded and shifted too and must be unchanged. State (get_state), metrics, the RNG position, controller nodes and
beliefs must equal the twin's after every case. There is no tolerance anywhere. Every pointer is valid for the
documented shape: the guards only observe.

Shapes: the 23 backends of tests/test_stream_order_gpu.py (B = 1027, so every k * B plane changes its alignment with k;
K = 6), the numpy-mode FourRooms handles also at B = 8196 (a multiple of 4 but not of 16 or 512), one philox backend per
.hip file at B = 3, and the wide observation planes (GRID Hansen vectors, windows and coordinates; C-ROOMS window, Hansen
vector, scalar and float obs, in philox, numpy and replay mode) at B = 1027 (C-ROOMS' one-workgroup numpy path holds at
most 1,024 envs: B = 1023 there).

A call that refuses an alignment (Ant-Tag's vector obs off 16 B, C-ROOMS' action / obs buffers in rollout and its pair
stores in rollout_controller) must say so with GP_E_INVALID and its message, leave every view poison and every guard
intact, and not advance the handle: the next aligned call equals the twin.

Which kernel a numpy-mode FourRooms launch took is read from gp_query "launches_windowed" / "launches_fused" /
"launches_step" before and after every case and must be the one the KERNELS table below states per shift.

Closed loop: GRID philox, ROCKSAMPLE, ANTTAG index, TAXI Hansen (scalar, one-hot, and a one-node table, the only one
Taxi stages in LDS), HEAVENHELL (cell and Hansen obs), CROOMS cardinal, POMDP Tiger and m37, and a ROOMS population of
P = 2 (B = 1027 + 1024), with the table in LDS and in global memory wherever `ctrl_lds_max` switches the placement
(ROCKSAMPLE and ANTTAG always read global memory; Heaven-Hell's cell-obs table, Taxi's three-node tables exceed the 60 KB
cap). gp_get_state is not called with NULL fields: the header documents NULL for gp_set_state only.

Measured on an MI355X: 276 tests, 17,274 guarded buffers checked, 8.0 - 8.8 s for the module, the slowest test 0.47 s
(rollout(out=) on the one-workgroup numpy-mode Taxi). Kernels selected, as read from the launch counters (shifts of
actions, obs, rew, term, trunc in bytes; K = 6):
  fourrooms_wgrid (B = 8192): all aligned and actions at 4 / 8 / 12: the windowed kernel; term or trunc at 4 / 8: the
    fused kernel; obs or rew at 4 / 8 / 12, term or trunc at 1 / 2 / 3, and the all-together cases: 6 x the step kernels.
    rollout_plan and step_raw alike: (4,0,0,0,0) windowed, (0,0,0,4,8) fused, all together the step kernels.
  fourrooms_fused (B = 8192, no_wgrid) and both handles at B = 8196 (not eligible for the windowed kernel: wgrid = 0):
    all aligned and term / trunc at 4 / 8: the fused kernel; every other shift, actions included: the step kernels.
  B = 1027 (wide obs, numpy mode): K single steps; with everything aligned (and term / trunc at 4 / 8) steps 0 and 4
    (whose planes sit on 16 B; the windows: one step, step 4 with the obs at 4) take the fused kernel as one-step
    launches, the others the step kernels; every other shift: 6 x the step kernels.
Table placement (`controller_lds` at ctrl_lds_max = 61,440 / 0): 1 / 0 for rooms_philox, rooms_population,
taxi_one_node, heavenhell_hansen, crooms_hansen, pomdp_tiger, pomdp_m37; 0 for rocksample, anttag_index, heavenhell,
taxi_philox, taxi_onehot. Beliefs: on chip for Tiger, in the global planes for m37.

One case failed on the library as it stood: test_crooms_wide_obs[*-replay] for the four obs kinds whose [B, ...] plane
is no multiple of 16 B at B = 1027 (float32 [B,2], the Hansen vector, the window, the scalar obs). A replay rollout is K
single steps, and each step repeated the 16-B check of the obs base on its own plane: the rollout was refused at step 1
("crooms: misaligned action / obs / reward buffer") on aligned allocations, after step 0 had written and advanced. The
bases are now checked once per call. The reference of every belief, backup and statistics case is a twin handle of its
own. The planes run alone in the closed-loop cases take every shift of their kind; the statistics inputs run the full
shift cases.

Out of scope: the multi-process shard (its buffers are the same calls per process), gp_autotune (its scratch is
internal), the profiling reads (host scalars), and gp_set_replay inputs (read by later steps; the replay backends run
here with aligned replay planes).
"""
import ctypes
import re

import numpy as np
import pytest

import store_guard as sg
import stream_order as so
import test_stream_order_gpu as tso
from test_stream_order_gpu import BACKENDS, CTRL_BACKENDS, K, SEED, actions_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATHS = {}       # numpy-mode FourRooms: {(backend, entry, shifts): the kernel the documented gates select}
PLACEMENT = {}   # closed loop: {(backend, ctrl_lds_max): controller_lds}

CROOMS_OPEN = r"failed \(-1\): crooms: misaligned action / obs / reward buffer"
CROOMS_CTRL = r"failed \(-1\): crooms: misaligned obs / action / reward \(8 B\) or node / flag \(2 B\) buffer"
ANTTAG_OBS = r"failed \(-1\): anttag: obs buffer must be 16-B aligned"


def _t():
    import torch
    return torch


def _err():
    from gym_po_amd._lib import GymPoError
    return GymPoError


def host(x):
    torch = _t()
    x = x.detach().cpu().contiguous()
    return (x.view(torch.uint8) if x.dtype == torch.bool else x).numpy()


def G(dtype, shape, shift, lead=1):
    """A guarded buffer; `lead` leading axes (K) come before the [B, ...] plane whose size sets the guards."""
    torch = _t()
    shape = tuple(int(s) for s in shape)
    plane = int(np.prod(shape[lead:], dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return sg.guarded(torch, dtype, shape, shift, DEV, plane)


def filled(x, shift, lead=1):
    """A guarded, shifted input buffer holding the host array `x`."""
    torch = _t()
    t = torch.as_tensor(np.ascontiguousarray(x))
    buf = G(t.dtype, t.shape, shift, lead)
    buf[0].copy_(t)
    return buf


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def same_env(ref_env, env, what):
    bad = so.differing(ref_env, so.env_snapshot(env))
    assert not bad, f"{what}: the handle differs from the twin's in {bad}"


def same_bytes(got, want, what):
    assert np.array_equal(sg._bytes(got), sg._bytes(want)), f"{what}: differs from the twin"


def closing(env):
    _t().cuda.synchronize()
    env.close()


# ------------------------------------------------------------------ backends ----
def _mk(cls, *a, **kw):
    import gym_po_amd
    return getattr(gym_po_amd, cls)(*a, **kw)


EXTRA = {  # numpy-mode FourRooms at a multiple of 4 that is no multiple of 16 or 512
    "fourrooms_wgrid_8196": lambda: tso._fourrooms_numpy(8196),
    "fourrooms_fused_8196": lambda: tso._fourrooms_numpy(8196, no_wgrid=1),
}
SMALL = {  # one philox backend per .hip file at B = 3: a single ragged quad
    "rooms_philox_b3": lambda: _mk("RoomsEnv", 3, layout="4", obs_type="hansen", time_limit=5, rng_mode="philox"),
    "taxi_philox_b3": lambda: tso._taxi(3, "philox"),
    "crooms_philox_b3": lambda: tso._crooms(3, "philox"),
    "anttag_index_b3": lambda: _mk("AntTagGridEnv", 3, size=4, min_distance=2.0, time_limit=5, obs_type="index"),
    "carflag_f32_b3": lambda: _mk("CarVecEnv", 3, time_limit=5, rng_mode="philox"),
    "rocksample_b3": lambda: _mk("RockSample", 3, time_limit=5),
    "heavenhell_b3": lambda: _mk("HeavenHellGridEnv", 3, action_failure_probability=0.25, time_limit=5),
    "pomdp_tiger_b3": lambda: tso._pomdp("tiger", 3),
}


def _grid_wide(kind, mode):
    f = {"hansen_vec4": lambda: _mk("MultistoryFourRoomsEnv", 1027, grid_z=1, obs_type="vector_hansen", time_limit=5,
                                    rng_mode=mode),
         "hansen_vec8": lambda: _mk("MultistoryFourRoomsEnv", 1027, grid_z=1, obs_type="vector_hansen8", time_limit=5,
                                    rng_mode=mode),
         "window3": lambda: _mk("RoomsEnv", 1027, layout="4", obs_type="grid", obs_n=3, time_limit=5, rng_mode=mode),
         "window5": lambda: _mk("RoomsEnv", 1027, layout="4", obs_type="grid", obs_n=5, time_limit=5, rng_mode=mode),
         "coords": lambda: _mk("MultistoryFourRoomsEnv", 1027, grid_z=3, obs_type="vector_mdp", time_limit=5,
                               rng_mode=mode),
         "coords_goal": lambda: _mk("MultistoryFourRoomsEnv", 1027, grid_z=3, obs_type="vector_mdp_goal", time_limit=5,
                                    rng_mode=mode)}
    return f[kind]


GRID_WIDE = ("hansen_vec4", "hansen_vec8", "window3", "window5", "coords", "coords_goal")
GRID_ORACLE = {"hansen_vec4": ("FourRoomsOracle", dict(grid_z=1, obs_type="vector_hansen")),
               "hansen_vec8": ("FourRoomsOracle", dict(grid_z=1, obs_type="vector_hansen8")),
               "window3": ("RoomsOracle", dict(layout="4", obs_type="grid", obs_n=3)),
               "window5": ("RoomsOracle", dict(layout="4", obs_type="grid", obs_n=5)),
               "coords": ("FourRoomsOracle", dict(grid_z=3, obs_type="vector_mdp")),
               "coords_goal": ("FourRoomsOracle", dict(grid_z=3, obs_type="vector_mdp_goal"))}
CROOMS_WIDE = {"window": dict(obs_type="grid", obs_m=3), "hansen_vec": dict(obs_type="vector_hansen"),
               "f32x2": dict(obs_type="vector_mdp"), "f32x4": dict(obs_type="vector_mdp_goal"),
               "f64x2": dict(obs_type="vector_mdp", f64=True), "scalar": dict(obs_type="hansen")}
CROOMS_MODES = {"philox": (1027, "philox", {}), "numpy_wg": (1023, "numpy", {}),
                "numpy_grid": (1027, "numpy", dict(xg_min_envs=0, xg_graph=0)),
                "replay": (1027, "replay", {})}  # (K step launches, each on the planes of its own step)


def _crooms_wide(kind, mode):
    def make():
        torch = _t()
        kw = dict(CROOMS_WIDE[kind])
        dt = torch.float64 if kw.pop("f64", False) else torch.float32
        B, rng, knobs = CROOMS_MODES[mode]
        if rng == "replay":
            kw["goal_xy"] = None
        with tso._knobs(**knobs):
            env = _mk("CRoomsEnv", B, time_limit=5, rng_mode=rng, dtype=dt, **kw)
        if rng == "replay":  # (the draws of tso.mk_crooms_replay)
            g = np.random.default_rng(5)
            env.set_replay(u=g.integers(0, 1 << 53, B, dtype=np.int64).astype(np.uint64),
                           goal_idx=g.integers(0, max(len(env.valid_cells(0)), 1), B).astype(np.int32),
                           agent_idx=g.integers(0, max(len(env.valid_cells(1)), 1), B).astype(np.int32),
                           noise=g.normal(0, 0.2, (B, 2)), wall_noise=g.normal(0, 0.5, (B, 2)))
            torch.cuda.synchronize()
        return env
    return make


_ACTS = {}


def acts_of(name, make, k=K):
    """Host actions [k, B(, 2)] of a backend (those of the stream-order module where it has the backend)."""
    if name in BACKENDS:
        return actions_of(name, k)[0]
    if (name, k) not in _ACTS:
        env = make()
        try:
            rng = np.random.default_rng(11)
            shape = (k, env.num_envs) + tuple(env._action_tail)
            if env._action_dtype == "int32":
                a = rng.integers(0, int(env.single_action_space.n), shape).astype(np.int32)
            else:
                a = rng.uniform(-1, 1, shape).astype(np.float32 if env._action_dtype == "float32" else np.float64)
        finally:
            closing(env)
        _ACTS[(name, k)] = a
    return _ACTS[(name, k)]


# ------------------------------------------------------------------ (a) open loop ----
_REF = {}


def open_ref(name, make, acts):
    """The aligned twin: reset obs, the outputs of one rollout of `acts`, and the handle afterwards."""
    key = (name, acts.shape[0])
    if key not in _REF:
        env = make()
        try:
            obs0 = so.reset(env, SEED)
            outs = env.rollout(tso._dev(acts))
            _t().cuda.synchronize()
            _REF[key] = {"obs0": host(obs0), "outs": [host(x) for x in outs], "env": so.env_snapshot(env)}
        finally:
            closing(env)
    return _REF[key]


def refusal_open(env, act, obs):
    """The documented refusal of gp_step / gp_rollout for these pointers (a regex of the error), or None."""
    kind = type(env).__name__
    if kind == "CRoomsEnv":
        need = {"float64": 16, "float32": 8, "int32": 4}[env._action_dtype]
        if act.data_ptr() % need or obs.data_ptr() % 16:
            return CROOMS_OPEN
    if kind == "AntTagGridEnv" and env._obs_width != 1 and obs.data_ptr() % 16:
        return ANTTAG_OBS
    return None


PATH_KEYS = ("launches_windowed", "launches_fused", "launches_step")


def numpy_grid(env):
    return type(env).__name__ in ("MultistoryFourRoomsEnv", "RoomsEnv") and env.rng_mode == "numpy"


# The kernel each shift of (actions, obs, rew, term, trunc) selects on the numpy-mode FourRooms handles, as
# include/gym_po_amd.h documents the fall-back; every shift not listed takes the step kernels (one launch per step).
_ACTIONS_ONLY = {(0, 0, 0, 0, 0), (4, 0, 0, 0, 0), (8, 0, 0, 0, 0), (12, 0, 0, 0, 0)}
_FLAGS_ON_4 = {(0, 0, 0, 4, 0), (0, 0, 0, 8, 0), (0, 0, 0, 0, 4), (0, 0, 0, 0, 8), (0, 0, 0, 4, 8)}
_FUSED_ONLY = {"fused": {(0, 0, 0, 0, 0)} | _FLAGS_ON_4}
KERNELS = {"fourrooms_wgrid": {"windowed": _ACTIONS_ONLY, "fused": _FLAGS_ON_4},
           "fourrooms_fused": _FUSED_ONLY,
           "fourrooms_wgrid_8196": _FUSED_ONLY,  # (B = 8196 is not eligible for the windowed kernel: wgrid = 0)
           "fourrooms_fused_8196": _FUSED_ONLY}


def launches(env):
    return [env.query(key) for key in PATH_KEYS]


def note_path(name, env, entry, k, shifts, before):
    """The kernels the call launched, read from the handle's launch counters. The FourRooms handles are held to the
    KERNELS table; the odd-B handles of the wide obs planes run K single steps, each of which takes the fused kernel
    when its own planes happen to sit on 16 B, else the step kernels (recorded, and held to K steps in all)."""
    ran = [b - a for a, b in zip(before, launches(env))]
    one = 1 if entry == "step" else k
    took = {(1, 0, 0): "windowed", (0, 1, 0): "fused", (0, 0, one): "step kernels"}.get(
        tuple(ran), f"single steps: {ran[0]} windowed, {ran[1]} fused, {ran[2]} step kernels")
    if name in KERNELS:
        want = next((kern for kern, cases in KERNELS[name].items() if tuple(shifts) in cases), "step kernels")
        assert took == want, (f"{name}/{entry} shifts={tuple(shifts)}: launches {dict(zip(PATH_KEYS, ran))}, "
                              f"documented: {want}")
    else:
        assert ran[0] == 0 and ran[1] + ran[2] == one, f"{name}/{entry} shifts={tuple(shifts)}: launches {ran}"
    PATHS[(name, entry, tuple(shifts))] = took


def run_open(name, env, ref, acts, shifts, entry):
    """One guarded call of `entry` (rollout, plan or step) after reset(SEED), held to the twin `ref`."""
    torch = _t()
    B, k = env.num_envs, acts.shape[0]
    step = entry == "step"
    lead, pre = (0, ()) if step else (1, (k,))
    a_np = acts[0] if step else acts
    specs = [(getattr(torch, env._action_dtype), a_np.shape), (env._obs_dtype, pre + tuple(env._obs_shape())),
             (torch.float32, pre + (B,)), (torch.uint8, pre + (B,)), (torch.uint8, pre + (B,))]
    so.reset(env, SEED)
    bufs = [G(dt, shp, sh, lead) for (dt, shp), sh in zip(specs, shifts)]
    views = [b[0] for b in bufs]
    a_dev = tso._dev(a_np)
    views[0].copy_(a_dev)
    expect = refusal_open(env, views[0], views[1])
    before = launches(env) if numpy_grid(env) else None
    what = f"{name}/{entry} shifts={tuple(shifts)}"
    refused = None
    try:
        if entry == "rollout":
            env.rollout(views[0], out=tuple(views[1:]))
        elif entry == "plan":
            run, _ = env.rollout_plan(views[0], out=tuple(views[1:]))
            run()
        else:
            env.step_raw(*views)
    except _err() as e:
        refused = str(e)
    torch.cuda.synchronize()
    names = ("actions", "obs", "rew", "term", "trunc")
    if expect or refused:
        assert refused and expect and re.search(expect, refused), f"{what}: expected {expect!r}, got {refused!r}"
        for nm, b in zip(names[1:], bufs[1:]):
            sg.check_untouched(*b, f"{what} {nm}")
        sg.check_input(*bufs[0], a_np, f"{what} actions")
        outs = env.step(a_dev)[:4] if step else env.rollout(a_dev)  # the refused call advanced nothing
        for nm, x, w in zip(names[1:], outs, ref["outs"]):
            same_bytes(host(x), w, f"{what} {nm} of the aligned call after the refusal")
    else:
        for nm, b, w in zip(names[1:], bufs[1:], ref["outs"]):
            sg.check(*b, w, f"{what} {nm}")
        sg.check_input(*bufs[0], a_np, f"{what} actions")
        if before is not None:
            note_path(name, env, entry, k, shifts, before)
    same_env(ref["env"], env, what)
    return refused is not None


def open_kinds(env):
    torch = _t()
    return (torch.empty((), dtype=getattr(torch, env._action_dtype)).element_size(),
            torch.empty((), dtype=env._obs_dtype).element_size(), 4, 1, 1)


OPEN = dict(BACKENDS, **EXTRA, **SMALL)


@pytest.mark.parametrize("backend", sorted(OPEN))
def test_rollout_out(backend, gpu_device):
    """rollout(out=): each of actions, obs, rew, term, trunc alone at each of its shifts, then all together."""
    make = OPEN[backend]
    acts = acts_of(backend, make)
    ref = open_ref(backend, make, acts)
    env = make()
    try:
        ran = 0
        for shifts in [(0,) * 5] + sg.shift_cases(open_kinds(env)):
            ran += not run_open(backend, env, ref, acts, shifts, "rollout")
        assert ran >= 12  # (rew, term and trunc are accepted anywhere by every backend)
        env.check()
    finally:
        closing(env)


@pytest.mark.parametrize("entry", ["plan", "step"])
@pytest.mark.parametrize("backend", sorted(OPEN))
def test_plan_and_step(backend, entry, gpu_device):
    """rollout_plan(out=) and step_raw with every buffer off its boundary (and once with the refusing ones on it)."""
    make = OPEN[backend]
    acts = acts_of(backend, make)
    acts = acts[:1] if entry == "step" else acts
    ref = open_ref(backend, make, acts)
    env = make()
    try:
        kinds = open_kinds(env)
        cases = sg.together_cases(kinds)
        cases += [(0, 0) + c[2:] for c in cases[:1]]  # kinds that refuse an action / obs shift: the other three shifted
        cases += [(kinds[0] if kinds[0] > 1 else 4, 0, 0, 0, 0), (0, 0, 0, 4, 8)]  # numpy-mode GRID: windowed, fused
        for shifts in cases:
            run_open(backend, env, ref, acts, shifts, entry)
        env.check()
    finally:
        closing(env)


@pytest.mark.parametrize("backend", sorted(OPEN))
def test_reset_into_guarded_obs(backend, gpu_device):
    """Raw gp_reset into a guarded obs [B, ...] at every shift of its element size."""
    from gym_po_amd import _lib
    make = OPEN[backend]
    acts = acts_of(backend, make)
    ref = open_ref(backend, make, acts)
    env = make()
    try:
        size = _t().empty((), dtype=env._obs_dtype).element_size()
        if (backend, "reset2") not in _REF:
            t = make()
            try:
                so.reset(t, SEED)
                _REF[(backend, "reset2")] = {"obs": host(so.reset(t, None)), "env": so.env_snapshot(t)}
            finally:
                closing(t)
        twin = _REF[(backend, "reset2")]
        for shift in (0,) + sg.SHIFTS[size]:
            so.reset(env, SEED)  # seeds; the raw reset below draws what a second reset() of the twin draws
            buf = G(env._obs_dtype, env._obs_shape(), shift, lead=0)
            _lib.check(_lib.lib().gp_reset(env._handle, ptr(buf[0]), env._stream()), "gp_reset")
            _t().cuda.synchronize()
            sg.check(*buf, twin["obs"], f"{backend}/gp_reset shift={shift}")
            same_env(twin["env"], env, f"{backend}/gp_reset shift={shift}")
        assert ref["obs0"].shape == twin["obs"].shape
    finally:
        closing(env)


@pytest.mark.parametrize("entry", ["rollout", "plan", "step"])
@pytest.mark.parametrize("backend", sorted(KERNELS))
def test_numpy_fourrooms_kernels(backend, entry, gpu_device):
    """What a numpy-mode FourRooms handle is eligible for, and one shifted call per kernel it can select (run_open
    holds the launch counters to the KERNELS table): every kernel of the handle is reached through every entry."""
    make = OPEN[backend]
    acts = acts_of(backend, make)
    acts = acts[:1] if entry == "step" else acts
    ref = open_ref(backend, make, acts)
    env = make()
    try:
        assert env.query("wgrid") == (1 if backend == "fourrooms_wgrid" else 0) and env.query("fused_blocks") > 0
        for shifts in ((0, 0, 0, 0, 0), (4, 0, 0, 0, 0), (0, 0, 0, 4, 8), (0, 4, 0, 0, 0), (0, 0, 0, 1, 0)):
            run_open(backend, env, ref, acts, shifts, entry)
        seen = {PATHS[(backend, entry, sh)] for sh in ((0, 0, 0, 0, 0), (4, 0, 0, 0, 0), (0, 0, 0, 4, 8), (0, 4, 0, 0, 0),
                                                       (0, 0, 0, 1, 0))}
        assert seen == set(KERNELS[backend]) | {"step kernels"}, seen
    finally:
        closing(env)


# ------------------------------------------------------------------ (b) wide obs planes ----
def _oracle_check(ref, acts, ora, f32):
    o = np.asarray(ora.reset_seed(SEED))
    cast = (lambda x: np.asarray(x).astype(np.float32)) if f32 else (lambda x: np.asarray(x).astype(np.float64))
    got0 = ref["obs0"] if f32 else ref["obs0"].astype(np.float64)
    assert np.array_equal(got0.reshape(o.shape), cast(o)), "reset obs against the oracle"
    for k in range(acts.shape[0]):
        oo, rr, dd, tt = ora.step_seeded(acts[k].astype(np.float64) if acts.dtype.kind == "f" else acts[k])
        g = ref["outs"][0][k] if f32 else ref["outs"][0][k].astype(np.float64)
        assert np.array_equal(g.reshape(np.asarray(oo).shape), cast(oo)), f"obs of step {k} against the oracle"
        assert np.array_equal(ref["outs"][1][k], rr), f"rew of step {k} against the oracle"
        assert np.array_equal(ref["outs"][2][k].astype(bool), dd) and np.array_equal(ref["outs"][3][k].astype(bool), tt)


@pytest.mark.parametrize("mode", ["philox", "numpy"])
@pytest.mark.parametrize("kind", GRID_WIDE)
def test_grid_wide_obs(kind, mode, gpu_device):
    """GRID's Hansen vectors (4, 8 B per env), windows (9, 25 B) and coordinates (12, 24 B) at B = 1027: every k * B
    plane starts at another alignment, and the obs shifts come on top. numpy mode: odd B selects K single steps, and
    the aligned twin is the oracle's run of the same seed."""
    name = f"grid_{kind}_{mode}"
    make = _grid_wide(kind, mode)
    acts = acts_of(name, make)
    ref = open_ref(name, make, acts)
    if mode == "numpy":
        import oracle.gridworld as og
        cls, kw = GRID_ORACLE[kind]
        _oracle_check(ref, acts, getattr(og, cls)(1027, time_limit=5, **kw), False)
    env = make()
    try:
        for shifts in [(0,) * 5] + sg.shift_cases(open_kinds(env)):
            assert not run_open(name, env, ref, acts, shifts, "rollout")
        env.check()
    finally:
        closing(env)


@pytest.mark.parametrize("mode", sorted(CROOMS_MODES))
@pytest.mark.parametrize("kind", sorted(CROOMS_WIDE))
def test_crooms_wide_obs(kind, mode, gpu_device):
    """C-ROOMS' window (9 B per env), Hansen vector (4 B), float32 [B,2] / [B,4] and float64 [B,2] obs on an odd B, in
    philox mode and on both numpy-mode paths. The obs and action bases must sit on 16 / 8 B (refused otherwise: those
    cases hold the refusal); the planes of steps k > 0 do not, and rew / term / trunc go anywhere."""
    name = f"crooms_{kind}_{mode}"
    make = _crooms_wide(kind, mode)
    acts = acts_of(name, make)
    ref = open_ref(name, make, acts)
    if mode == "numpy_grid":
        from oracle.crooms import CRoomsOracle
        kw = dict(CROOMS_WIDE[kind])
        f64 = kw.pop("f64", False)
        _oracle_check(ref, acts, CRoomsOracle(CROOMS_MODES[mode][0], time_limit=5, **kw),
                      not f64 and CROOMS_WIDE[kind]["obs_type"].startswith("vector_mdp"))
    env = make()
    try:
        ran = sum(not run_open(name, env, ref, acts, shifts, "rollout")
                  for shifts in [(0,) * 5] + sg.shift_cases(open_kinds(env)))
        assert ran >= 12
        env.check()
    finally:
        closing(env)


# ------------------------------------------------------------------ (c) closed loop ----
CTRL_NAMES = ("obs", "actions", "nodes", "rew", "term", "trunc")


def mk_taxi_onehot():
    return tso._taxi(1027, "philox", one_hot=True)


def mk_population():  # (ROOMS' binary Hansen obs: one controller's table fits the LDS budget)
    return _mk("RoomsEnv", 1027 + 1024, layout="4", obs_type="hansen", time_limit=5, rng_mode="philox")


def install_one_node(env):  # (Taxi stages the table in LDS beside its maps only for M = 1)
    n_obs, A = int(env._controller_n_obs()), int(env.single_action_space.n)
    env.set_controller(probs=tso.random_probs(1, n_obs, A, 5))


def install_population(env):
    n_obs, A = int(env._controller_n_obs()), int(env.single_action_space.n)
    env.set_controller_population(probs=np.stack([tso.random_probs(tso.M_NODES, n_obs, A, 20 + i) for i in range(2)]),
                                  group_envs=2048, gamma=0.875)
    assert env.query("controller_population") == 2


CTRL = {k: (v, tso.install) for k, v in CTRL_BACKENDS.items()}
CTRL["taxi_onehot"] = (mk_taxi_onehot, tso.install)
CTRL["taxi_one_node"] = (tso.mk_taxi_ctrl, install_one_node)
CTRL["rooms_population"] = (mk_population, install_population)
# the tables whose placement `ctrl_lds_max` switches (ROCKSAMPLE, ANTTAG: always global memory; Heaven-Hell's cell obs
# and Taxi's M = 3 tables exceed the 60 KB cap)
LDS_KINDS = ("rooms_philox", "taxi_one_node", "heavenhell_hansen", "crooms_hansen", "pomdp_tiger", "pomdp_m37",
             "rooms_population")
CTRL_CASES = [(b, lds) for b in sorted(CTRL) for lds in ((61440, 0) if b in LDS_KINDS else (-1,))]


def ctrl_env(backend, lds_max):
    make, setup = CTRL[backend]
    env = make()
    so.reset(env, SEED)
    with tso._knobs(ctrl_lds_max=lds_max):
        setup(env)
    PLACEMENT[(backend, lds_max)] = env.query("controller_lds")
    if backend in LDS_KINDS:
        assert env.query("controller_lds") == (1 if lds_max else 0), f"{backend}: ctrl_lds_max={lds_max}"
    return env


def ctrl_ref(backend):
    """The aligned twin (default table placement): the six planes of K closed-loop steps and the handle afterwards."""
    key = (backend, "ctrl")
    if key not in _REF:
        env = ctrl_env(backend, -1)
        try:
            so.reset(env, SEED)
            out = env.rollout_controller(K)
            _t().cuda.synchronize()
            snap = so.env_snapshot(env)
            if backend == "rooms_population":
                snap["scores"] = so.raw(env.controller_scores())
            _REF[key] = {"outs": {n: host(out[n]) for n in CTRL_NAMES}, "env": snap}
        finally:
            closing(env)
    return _REF[key]


def refusal_ctrl(env, views):
    if type(env).__name__ != "CRoomsEnv":
        return None
    need = {"obs": 8, "actions": 8, "rew": 8, "nodes": 2, "term": 2, "trunc": 2}
    return CROOMS_CTRL if any(v.data_ptr() % need[n] for n, v in views.items()) else None


def run_ctrl(backend, env, ref, shifts):
    """rollout_controller into guarded planes; `shifts`: {name: shift}, a name left out is passed as NULL."""
    torch = _t()
    B = env.num_envs
    dts = {"obs": env._obs_dtype, "actions": torch.int32, "nodes": torch.uint8, "rew": torch.float32,
           "term": torch.uint8, "trunc": torch.uint8}
    so.reset(env, SEED)
    bufs = {n: G(dts[n], (K,) + (tuple(env._obs_shape()) if n == "obs" else (B,)), sh) for n, sh in shifts.items()}
    views = {n: b[0] for n, b in bufs.items()}
    expect = refusal_ctrl(env, views)
    what = f"{backend}/rollout_controller shifts={shifts}"
    refused = None
    try:
        env.rollout_controller(K, out=views, store=tuple(views))
    except _err() as e:
        refused = str(e)
    torch.cuda.synchronize()
    if expect or refused:
        assert refused and expect and re.search(expect, refused), f"{what}: expected {expect!r}, got {refused!r}"
        for n, b in bufs.items():
            sg.check_untouched(*b, f"{what} {n}")
        out = env.rollout_controller(K)
        for n in CTRL_NAMES:
            same_bytes(host(out[n]), ref["outs"][n], f"{what} {n} of the aligned call after the refusal")
    else:
        for n, b in bufs.items():
            sg.check(*b, ref["outs"][n], f"{what} {n}")
    snap = so.env_snapshot(env)
    if "scores" in ref["env"]:
        snap["scores"] = so.raw(env.controller_scores())
    bad = so.differing(ref["env"], snap)
    assert not bad, f"{what}: the handle differs from the twin's in {bad}"
    return refused is not None


def ctrl_kinds(env):
    return (_t().empty((), dtype=env._obs_dtype).element_size(), 4, 1, 4, 1, 1)


@pytest.mark.parametrize("backend,lds_max", CTRL_CASES)
def test_rollout_controller_planes(backend, lds_max, gpu_device):
    """All six planes guarded over the shift cases, then each plane alone with the other five NULL, with the
    controller table in LDS (the budget raised to its 60 KB cap) and in global memory (0); PLACEMENT records what
    `controller_lds` answered."""
    ref = ctrl_ref(backend)
    env = ctrl_env(backend, lds_max)
    try:
        kinds = ctrl_kinds(env)
        ran = 0
        for shifts in [(0,) * 6] + sg.shift_cases(kinds):
            ran += not run_ctrl(backend, env, ref, dict(zip(CTRL_NAMES, shifts)))
        for i, n in enumerate(CTRL_NAMES):
            for sh in (0,) + sg.SHIFTS[kinds[i]]:
                ran += not run_ctrl(backend, env, ref, {n: sh})
        run_ctrl(backend, env, ref, {})  # nothing stored: a pure policy evaluation
        assert ran >= 16
        env.check()
    finally:
        closing(env)


@pytest.mark.parametrize("backend", sorted(set(CTRL) - {"taxi_one_node"}))  # (its nodes are all 0)
def test_controller_nodes(backend, gpu_device):
    """gp_controller_nodes: get into a guarded uint8 [B] at shifts 0..3, set from a shifted input; the closed-loop
    rollout that follows equals the twin's that set the same nodes from an aligned buffer."""
    from gym_po_amd import _lib
    fn = _lib.lib().gp_controller_nodes
    env = ctrl_env(backend, -1)
    try:
        B = env.num_envs
        nodes = tso._nodes(B)[0]["nodes"]
        key = (backend, "nodes")
        if key not in _REF:
            twin = ctrl_env(backend, -1)
            try:
                twin.controller_nodes = nodes
                out = twin.rollout_controller(K)
                _t().cuda.synchronize()
                _REF[key] = {"outs": {n: host(out[n]) for n in CTRL_NAMES}, "env": so.env_snapshot(twin)}
            finally:
                closing(twin)
        ref = _REF[key]
        for shift, src_shift in ((0, 1), (1, 2), (2, 3), (3, 8)):
            so.reset(env, SEED)
            src = filled(nodes, src_shift, lead=0)
            _lib.check(fn(env._handle, None, ptr(src[0]), env._stream()), "gp_controller_nodes")
            dst = G(_t().uint8, (B,), shift, lead=0)
            _lib.check(fn(env._handle, ptr(dst[0]), None, env._stream()), "gp_controller_nodes")
            _t().cuda.synchronize()
            sg.check(*dst, nodes, f"{backend}/controller_nodes get shift={shift}")
            sg.check_input(*src, nodes, f"{backend}/controller_nodes set")
            out = env.rollout_controller(K)
            for n in CTRL_NAMES:
                same_bytes(host(out[n]), ref["outs"][n], f"{backend}/rollout after set nodes: {n}")
            same_env(ref["env"], env, f"{backend}/controller_nodes shift={shift}")
    finally:
        closing(env)


# ------------------------------------------------------------------ (d) state ----
STATE_KINDS = ["rooms_philox", "taxi_philox", "crooms_philox", "anttag_index", "carflag_f32", "rocksample", "heavenhell",
               "pomdp_tiger"]


def _np_state(ref):
    out = []
    for dt, shape, b in ref["env"]["state"]:
        out.append(np.frombuffer(b, dtype=np.dtype(dt.replace("torch.", ""))).reshape(shape).copy())
    return out


@pytest.mark.parametrize("backend", STATE_KINDS)
def test_get_state_into_guarded_buffers(backend, gpu_device):
    make = BACKENDS[backend]
    acts = acts_of(backend, make)
    ref = open_ref(backend, make, acts)
    env = make()
    try:
        so.reset(env, SEED)
        env.rollout(tso._dev(acts))
        want = _np_state(ref)
        protos = env.get_state()
        kinds = tuple(t.element_size() for t in protos)
        for shifts in [(0,) * len(kinds)] + sg.shift_cases(kinds):
            bufs = [G(t.dtype, t.shape, sh, lead=0) for t, sh in zip(protos, shifts)]
            env._get_state_raw([b[0] for b in bufs])
            _t().cuda.synchronize()
            for i, (b, w) in enumerate(zip(bufs, want)):
                sg.check(*b, w, f"{backend}/get_state field {i} shifts={shifts}")
        same_env(ref["env"], env, f"{backend}/get_state")
    finally:
        closing(env)


@pytest.mark.parametrize("backend", STATE_KINDS)
def test_set_state_from_shifted_inputs(backend, gpu_device):
    """gp_set_state from shifted, guarded inputs, then K steps: outputs and handle equal the twin's, which set the
    same state from aligned buffers."""
    make = BACKENDS[backend]
    acts = acts_of(backend, make)
    state = _np_state(open_ref(backend, make, acts))
    key = (backend, "set_state")
    if key not in _REF:
        twin = make()
        try:
            so.reset(twin, SEED + 1)
            twin._set_state_raw([tso._dev(x) for x in state])
            outs = twin.rollout(tso._dev(acts))
            _t().cuda.synchronize()
            _REF[key] = {"outs": [host(x) for x in outs], "env": so.env_snapshot(twin)}
        finally:
            closing(twin)
    ref = _REF[key]
    env = make()
    try:
        kinds = tuple(x.dtype.itemsize for x in state)
        for shifts in sg.shift_cases(kinds):
            so.reset(env, SEED + 1)
            bufs = [filled(x, sh, lead=0) for x, sh in zip(state, shifts)]
            env._set_state_raw([b[0] for b in bufs])
            outs = env.rollout(tso._dev(acts))
            _t().cuda.synchronize()
            for nm, x, w in zip(("obs", "rew", "term", "trunc"), outs, ref["outs"]):
                same_bytes(host(x), w, f"{backend}/set_state shifts={shifts}: {nm}")
            for i, (b, x) in enumerate(zip(bufs, state)):
                sg.check_input(*b, x, f"{backend}/set_state field {i}")
            same_env(ref["env"], env, f"{backend}/set_state shifts={shifts}")
    finally:
        closing(env)


# ------------------------------------------------------------------ (e) beliefs ----
MODELS = {"tiger": 2, "m37": 37}


def belief_env(model, policy=False):
    env = tso._pomdp(model)
    so.reset(env, SEED)
    (tso.enable_belief_policy if policy else tso.enable_belief)(env)
    return env


def belief_twin(key, model, policy, fn):
    """`fn(env)` on a same-seed twin handle of its own (aligned allocations), cached: the reference of a case."""
    if key not in _REF:
        twin = belief_env(model, policy)
        try:
            _REF[key] = fn(twin)
            _t().cuda.synchronize()
        finally:
            closing(twin)
    return _REF[key]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_belief_get_and_set(model, gpu_device):
    from gym_po_amd import _lib
    S = MODELS[model]
    b0 = belief_twin((model, "belief0"), model, False, lambda twin: host(twin.belief))
    env = belief_env(model)
    try:
        B = env.num_envs
        bt = tso._beliefs(model)[0]
        for shift in (0, 4, 8, 12):
            dst = G(_t().float32, (B, S), shift, lead=0)
            _lib.check(_lib.lib().gp_belief_get(env._handle, ptr(dst[0]), env._stream()), "gp_belief_get")
            _t().cuda.synchronize()
            sg.check(*dst, b0, f"pomdp_{model}/belief_get shift={shift}")
        for shift in (4, 8, 12):
            src = filled(bt, shift, lead=0)
            tso.raw_belief_set(env, src[0])
            dst = G(_t().float32, (B, S), 16 - shift, lead=0)
            _lib.check(_lib.lib().gp_belief_get(env._handle, ptr(dst[0]), env._stream()), "gp_belief_get")
            _t().cuda.synchronize()
            sg.check(*dst, bt, f"pomdp_{model}/belief_set shift={shift}")
            sg.check_input(*src, bt, f"pomdp_{model}/belief_set input")
            tso.raw_belief_set(env, tso._dev(b0))
    finally:
        closing(env)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_belief_filter_from_shifted_planes(model, gpu_device):
    planes = tso.open_planes(model, SEED)
    bt = tso._beliefs(model)[0]
    names = ("actions", "obs", "term", "trunc")

    def aligned(twin):
        tso.raw_belief_set(twin, tso._dev(bt))
        twin.belief_filter(*(tso._dev(planes[n]) for n in names))
        return host(twin.belief)
    want = belief_twin((model, "filter"), model, False, aligned)
    assert not np.array_equal(want, bt)
    env = belief_env(model)
    try:
        for shifts in sg.shift_cases((4, 4, 1, 1)):
            tso.raw_belief_set(env, tso._dev(bt))
            bufs = [filled(planes[n], sh) for n, sh in zip(names, shifts)]
            env.belief_filter(*(b[0] for b in bufs))
            same_bytes(host(env.belief), want, f"pomdp_{model}/belief_filter shifts={shifts}")
            for n, b in zip(names, bufs):
                sg.check_input(*b, planes[n], f"pomdp_{model}/belief_filter {n}")
        env.check()
    finally:
        closing(env)


BELIEF_NAMES = ("obs", "actions", "vec", "value", "rew", "term", "trunc")
BELIEF_KINDS = (4, 4, 4, 4, 4, 1, 1)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_rollout_belief_planes(model, gpu_device):
    """The seven planes of gp_rollout_belief together over the shift cases and each alone, beliefs on chip (Tiger) and
    in the global planes (m37)."""
    torch = _t()

    def aligned(twin):
        out = twin.rollout_belief(K)
        torch.cuda.synchronize()
        return {n: host(out[n]) for n in BELIEF_NAMES}, so.env_snapshot(twin)
    want, ref_env = belief_twin((model, "rollout_belief"), model, True, aligned)
    env = belief_env(model, policy=True)
    try:
        B = env.num_envs
        assert env.query("belief_onchip") == (1 if model == "tiger" else 0)
        dts = dict(zip(BELIEF_NAMES, (torch.int32, torch.int32, torch.int32, torch.float32, torch.float32,
                                      torch.uint8, torch.uint8)))
        cases = [dict(zip(BELIEF_NAMES, s)) for s in [(0,) * 7] + sg.shift_cases(BELIEF_KINDS)]
        cases += [{n: sg.SHIFTS[k][-1]} for n, k in zip(BELIEF_NAMES, BELIEF_KINDS)] + [{}]
        for shifts in cases:
            so.reset(env, SEED)
            bufs = {n: G(dts[n], (K, B), sh) for n, sh in shifts.items()}
            env.rollout_belief(K, out={n: b[0] for n, b in bufs.items()}, store=tuple(bufs))
            torch.cuda.synchronize()
            for n, b in bufs.items():
                sg.check(*b, want[n], f"pomdp_{model}/rollout_belief {n} shifts={shifts}")
            same_env(ref_env, env, f"pomdp_{model}/rollout_belief shifts={shifts}")
        env.check()
    finally:
        closing(env)


@pytest.mark.parametrize("P", [1, 1027])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_belief_backup(model, P, gpu_device):
    """gp_belief_backup: guarded alpha_out [P,S], act_out [P] and value_out [P], shifted points [P,S]."""
    torch = _t()
    S = MODELS[model]
    rng = np.random.default_rng(29)
    pts = rng.random((P, S)).astype(np.float32) + np.float32(0.01)
    alpha = tso.ALPHA if model == "tiger" else rng.normal(size=(5, S)).astype(np.float32)

    def aligned(twin):
        before = so.env_snapshot(twin)
        ref = {n: host(v) for n, v in twin.point_backup(pts, alpha).items()}
        assert not so.differing(before, so.env_snapshot(twin))
        return ref, before
    ref, b0 = belief_twin((model, "backup", P), model, False, aligned)
    env = belief_env(model)
    try:
        dts = {"alpha": (torch.float32, (P, S)), "actions": (torch.int32, (P,)), "value": (torch.float32, (P,))}
        for shifts in [(0,) * 4] + sg.shift_cases((4, 4, 4, 4)):
            src = filled(pts, shifts[0], lead=0)
            bufs = {n: G(*dts[n], sh, lead=0) for n, sh in zip(("alpha", "actions", "value"), shifts[1:])}
            env.point_backup(src[0], alpha, out={n: b[0] for n, b in bufs.items()})
            torch.cuda.synchronize()
            for n, b in bufs.items():
                sg.check(*b, ref[n], f"pomdp_{model}/point_backup P={P} {n} shifts={shifts}")
            sg.check_input(*src, pts, f"pomdp_{model}/point_backup points")
        same_env(b0, env, f"pomdp_{model}/point_backup")  # beliefs, state, step counter, metrics: untouched
    finally:
        closing(env)


# ------------------------------------------------------------------ (f) statistics ----
STAT_INPUTS = ("obs0", "obs", "actions", "nodes", "next_nodes", "rew", "term", "trunc")
STAT_KINDS = (4, 4, 4, 1, 1, 4, 1, 1)


@pytest.mark.parametrize("lds_max,path", [(-1, 1), (0, 0)], ids=["lds", "global"])
@pytest.mark.parametrize("backend", ["heavenhell_hansen", "pomdp_tiger"])
def test_controller_stats(backend, lds_max, path, gpu_device):
    """gp_controller_stats adds into guarded int64 tables at 8-byte shifts (zeroed, as the caller must), from eight
    input planes over the shift cases (each alone at each of its shifts, then all together), on the LDS-histogram path
    and on the global-atomics path; the reference is a twin handle's call on aligned planes."""
    torch = _t()
    planes = tso.planes_of(backend, SEED)

    def call(env, p, into=None):
        with tso._knobs(stats_lds_max=lds_max):
            out = env.controller_statistics({n: p[n] for n in CTRL_NAMES}, p["obs0"], next_nodes=p["next_nodes"],
                                            gamma=0.875, into=into)
        assert env.query("stats_lds") == path
        return out
    key = (backend, "stats", path)
    if key not in _REF:  # the twin handle: aligned planes, fresh tables
        twin = CTRL_BACKENDS[backend]()
        try:
            tso.install(twin)
            _REF[key] = {n: host(v) for n, v in call(twin, {n: tso._dev(planes[n]) for n in STAT_INPUTS}).items()}
        finally:
            closing(twin)
    ref = _REF[key]
    env = CTRL_BACKENDS[backend]()
    try:
        tso.install(env)
        assert ref["counts"].sum() == K * env.num_envs
        shape = ref["counts"].shape
        for i, shifts in enumerate([(0,) * 8] + sg.shift_cases(STAT_KINDS)):
            t_shift = 8 * ((i + 1) % 2)
            bufs = {n: filled(planes[n], sh, lead=0 if planes[n].ndim == 1 else 1)
                    for n, sh in zip(STAT_INPUTS, shifts)}
            tabs = {n: G(torch.int64, shape, t_shift, lead=0) for n in ("counts", "ret_q")}
            for b in tabs.values():
                b[0].zero_()
            call(env, {n: b[0] for n, b in bufs.items()}, into={n: b[0] for n, b in tabs.items()})
            torch.cuda.synchronize()
            for n, b in tabs.items():
                sg.check(*b, ref[n], f"{backend}/controller_stats {n} shifts={shifts}")
            for n, b in bufs.items():
                sg.check_input(*b, planes[n], f"{backend}/controller_stats {n}")
        env.check()
    finally:
        closing(env)


# ------------------------------------------------------------------ (g) render and diagnostics ----
@pytest.mark.parametrize("n", [1, 3, 5])
def test_taxi_render_into_guarded_frame(n, gpu_device):
    """gp_taxi_render tiles n frames ceil(sqrt(n)) wide: n = 3 and 5 leave zero-padding tiles, which are written too."""
    from gym_po_amd import _lib
    torch = _t()
    fn = _lib.lib().gp_taxi_render
    dims = (ctypes.c_int32 * 4)()
    env = tso.mk_taxi_philox()
    try:
        so.reset(env, SEED)
        _lib.check(fn(env._handle, n, 1, None, dims, None), "gp_taxi_render")
        rows, cols = dims[0], dims[1]
        ref = torch.empty((rows, cols, 3), dtype=torch.uint8, device=DEV)
        _lib.check(fn(env._handle, n, 1, ptr(ref), dims, env._stream()), "gp_taxi_render")
        ref = host(ref)
        assert (ref == 0).any() and (ref != 0).any()
        for shift in (0, 1, 2, 3):
            buf = G(torch.uint8, (rows, cols, 3), shift, lead=0)
            _lib.check(fn(env._handle, n, 1, ptr(buf[0]), dims, env._stream()), "gp_taxi_render")
            torch.cuda.synchronize()
            sg.check(*buf, ref, f"taxi_render n={n} shift={shift}")
    finally:
        closing(env)


@pytest.mark.parametrize("shape", [(7, 11, 176, 112), (5, 3, 64, 9), (13, 13, 13, 13)])
def test_resize_area_leaves_the_pitch_gap(shape, gpu_device):
    """gp_resize_area_u8 with dst_pitch = dw * ch + 5: the 5 gap bytes of every row still hold the poison, the pixels
    are the restatement's (source values <= 80, so no pixel can be the poison byte)."""
    from gym_po_amd import _lib
    from oracle import render
    torch = _t()
    sh, sw, dh, dw = shape
    src = np.random.default_rng(sum(shape)).integers(0, 81, (sh, sw, 3), dtype=np.uint8)
    want = render.resize_area_u8(src, dh, dw)
    assert not (want == sg.POISON).any()
    pitch = dw * 3 + 5
    for shift in (0, 1, 2, 3):
        s = filled(src, (shift + 2) % 4, lead=0)
        buf = G(torch.uint8, (dh, pitch), shift, lead=0)
        rc = _lib.lib().gp_resize_area_u8(ptr(s[0]), sh, sw, 3, ptr(buf[0]), dh, dw, pitch, None)
        assert rc == 0, _lib.lib().gp_last_error()
        torch.cuda.synchronize()
        before, after = sg.guards_intact(*buf)
        assert before and after, f"resize shift={shift}: a byte outside the frame was written"
        got = host(buf[0])
        assert np.array_equal(got[:, :dw * 3].reshape(dh, dw, 3), want), f"resize shift={shift}"
        assert (got[:, dw * 3:] == sg.POISON).all(), f"resize shift={shift}: the pitch gap was written"
        sg.check_input(*s, src, "resize src")
        sg.STATS["buffers"] += 1


def test_standard_normal_words_into_guarded_output(gpu_device):
    from gym_po_amd import _lib
    torch = _t()
    n, seed = 1000, 4242
    want = np.random.Generator(np.random.PCG64(seed)).standard_normal(n)
    words = np.random.PCG64(seed).random_raw(2 * n).view(np.int64)
    for w_shift, o_shift in ((0, 0), (8, 0), (0, 8), (8, 8)):
        src = filled(words, w_shift, lead=0)
        out = G(torch.float64, (n,), o_shift, lead=0)
        used = ctypes.c_int64()
        _lib.check(_lib.lib().gp_standard_normal_words(ptr(src[0]), len(words), ptr(out[0]), n, ctypes.byref(used),
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "gp_standard_normal_words")
        torch.cuda.synchronize()
        sg.check(*out, want, f"standard_normal_words shifts={(w_shift, o_shift)}")
        sg.check_input(*src, words, "standard_normal_words words")


# ------------------------------------------------------------------ (h) refusals ----
@pytest.mark.parametrize("backend,shifts,msg", [
    ("anttag_vector", (0, 4, 0, 0, 0), ANTTAG_OBS), ("anttag_vector", (0, 8, 0, 0, 0), ANTTAG_OBS),
    ("crooms_philox", (8, 0, 0, 0, 0), CROOMS_OPEN), ("crooms_philox", (0, 8, 0, 0, 0), CROOMS_OPEN),
    ("crooms_numpy_wg", (0, 8, 0, 0, 0), CROOMS_OPEN), ("crooms_numpy_grid", (8, 0, 0, 0, 0), CROOMS_OPEN),
    ("crooms_replay", (0, 8, 0, 0, 0), CROOMS_OPEN)])
@pytest.mark.parametrize("entry", ["rollout", "plan", "step"])
def test_open_loop_refusals(backend, shifts, msg, entry, gpu_device):
    """The documented alignment refusals of gp_step / gp_rollout: GP_E_INVALID with its message, nothing written,
    nothing advanced (run_open holds all of it; here the refusal itself is required)."""
    make = BACKENDS[backend]
    acts = acts_of(backend, make)
    acts = acts[:1] if entry == "step" else acts
    ref = open_ref(backend, make, acts)
    env = make()
    try:
        assert run_open(backend, env, ref, acts, shifts, entry), "the call was not refused"
    finally:
        closing(env)


@pytest.mark.parametrize("shifts", [{"obs": 4}, {"actions": 12}, {"rew": 4}, {"nodes": 1}, {"term": 3}, {"trunc": 1},
                                    dict(zip(CTRL_NAMES, (4, 4, 1, 4, 1, 1)))])
def test_crooms_controller_refusals(shifts, gpu_device):
    """C-ROOMS' closed-loop kernel stores pairs: 8 B of 4-byte elements, 2 B of flags; other addresses are refused."""
    ref = ctrl_ref("crooms_hansen")
    env = ctrl_env("crooms_hansen", -1)
    try:
        assert run_ctrl("crooms_hansen", env, ref, shifts), "the call was not refused"
    finally:
        closing(env)


def test_zz_report(gpu_device):
    """What the module checked (printed for the record in the module docstring)."""
    print(f"[store-guard] guarded buffers checked: {sg.STATS['buffers']}")
    by = {}
    for (name, entry, shifts), path in sorted(PATHS.items()):
        by.setdefault((name, entry, path), []).append(shifts)
    for key, shifts in sorted(by.items()):
        print(f"[store-guard] path {key}: {shifts}")
    for key in sorted(PLACEMENT):
        print(f"[store-guard] placement {key}: controller_lds={PLACEMENT[key]}")
