"""GPU parity of the C-ROOMS kernels (csrc/crooms.hip) with the `crooms_table` fixtures: one reference step over rows
aimed at the lines where a step decides something (tests/golden/fixtures.py crooms_table_inputs; the fixtures
themselves are pinned to the oracle and to a scalar restatement in test_crooms_table_cpu.py).

  * exact mode (rng_mode="numpy"): the recorded PCG64 state set, the rows set, one step: everything equals the
    fixture bit for bit, the post-step state and the stream position included -- on the default path, through the
    grid-wide draw calls and through the one-workgroup kernel;
  * replay mode, fed the draws of the oracle's run of the same step: float64 I/O equals the fixture bit for bit,
    float32 I/O gives the fixture's float observations rounded once to float32 and its integer observations;
  * philox mode (the generic rollout kernel and crooms_rollout<GP_OBS_F32, false, 1>): with action_std = 0 a row
    that hits no wall and ends no episode draws nothing that matters, so on those rows the kernels must give the
    reference's values; on every row the flags and the reward must agree with each other;
  * agent_xy (a fixed start cell, no reference fixture: the reference raises there) against the oracle;
  * cell_size < 1 is refused at creation.

Tolerance: none. Every comparison is equality of bits, or equality after one float32 rounding of the reference value.
"""
import numpy as np
import pytest

from crooms_table_oracle import (RecordingDraws, ctor_kwargs, replay_args, rng6, state_of_rng6, table_oracle_step)
from fixtures import load_crooms_table, load_index
from oracle.crooms import CRoomsOracle

pytestmark = pytest.mark.gpu

TABLES = sorted(load_index()["crooms_table"])
_CACHE = {}


def _table(name):
    """(meta, recorded arrays, the oracle's recorded draws of the step): computed once, never written to."""
    if name not in _CACHE:
        meta, data = load_crooms_table(name)
        _, _, rd = table_oracle_step(meta, data)
        for v in list(data.values()) + list(rd.rec.values()):
            v.setflags(write=False)
        _CACHE[name] = (meta, data, rd.rec)
    return _CACHE[name]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _make(meta, **extra):
    from gym_po_amd import CRoomsEnv
    return CRoomsEnv(meta["num_envs"], **ctor_kwargs(meta["kwargs"]), **extra)


def _set_rows(env, meta, data):
    goal = None if meta["kwargs"]["goal_xy"] is not None else data["in_goal_cell"].astype(np.int32)
    env.set_state(agent_yx=data["in_agent"].copy(), goal_cell_yx=goal, velocity=data["in_velocity"].copy(),
                  elapsed=data["in_elapsed"].copy())


def _actions(data, dtype):
    import torch
    a = data["in_action"]
    return torch.as_tensor(a.copy()).to(dtype) if a.dtype.kind == "f" else a.copy()


def _outputs(out):
    return [x.cpu().numpy() for x in out[:4]]


def _state(env):
    return [x.cpu().numpy() for x in env.get_state()]


def _assert_obs(o, data, f32):
    ref = data["obs"]
    if o.dtype.kind == "f":
        if f32:
            assert o.dtype == np.float32
            np.testing.assert_array_equal(o.view(np.uint32), ref.astype(np.float32).view(np.uint32))
        else:
            np.testing.assert_array_equal(_bits(o), _bits(ref))
    else:
        np.testing.assert_array_equal(o.astype(np.int64), ref.astype(np.int64))


def _assert_all_rows(env, got, data, f32):
    o, r, d, tr = got
    _assert_obs(o, data, f32)
    np.testing.assert_array_equal(r.view(np.uint32), data["rew"].view(np.uint32))
    np.testing.assert_array_equal(d.astype(bool), data["term"])
    np.testing.assert_array_equal(tr.astype(bool), data["trunc"])
    a, g, v, e = _state(env)
    np.testing.assert_array_equal(_bits(a), _bits(data["agent"]))
    np.testing.assert_array_equal(g, data["goal_cell"])
    np.testing.assert_array_equal(_bits(v), _bits(data["velocity"]))
    np.testing.assert_array_equal(e, data["elapsed"])


@pytest.mark.parametrize("xg_min", [None, 0, 4096], ids=["default", "grid_wide", "one_workgroup"])
@pytest.mark.parametrize("name", TABLES)
def test_exact_mode_reproduces_table(name, xg_min, gpu_device):
    import torch
    from gym_po_amd._lib import debug_knobs
    meta, data, _ = _table(name)
    if xg_min is None:
        env = _make(meta, rng_mode="numpy", dtype=torch.float64)
    else:
        with debug_knobs(xg_min_envs=xg_min):
            env = _make(meta, rng_mode="numpy", dtype=torch.float64)
    env.reset(seed=meta["seed"])
    assert rng6(env.np_random) == [int(v) for v in data["pre_rng_state"]]
    _set_rows(env, meta, data)
    env.rng_state = state_of_rng6(data["pre_rng_state"])
    got = _outputs(env.step(_actions(data, torch.float64)))
    _assert_all_rows(env, got, data, False)
    assert rng6(env.np_random) == [int(v) for v in data["rng_state"]]  # has_uint32 and uinteger included


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", TABLES)
def test_replay_mode_reproduces_table(name, f32, gpu_device):
    import torch
    meta, data, rec = _table(name)
    B, dtype = meta["num_envs"], torch.float32 if f32 else torch.float64
    env = _make(meta, rng_mode="replay", dtype=dtype)
    env.set_replay(**replay_args({}, B))
    env.reset()
    _set_rows(env, meta, data)
    env.set_replay(**replay_args({k: v.copy() for k, v in rec.items()}, B))
    got = _outputs(env.step(_actions(data, dtype)))
    _assert_all_rows(env, got, data, f32)


def _philox_cases():
    for name in TABLES:
        for f32 in (True, False):
            for how in ("step", "rollout"):
                yield pytest.param(name, f32, how, False, id=f"{name}-{'f32' if f32 else 'f64'}-{how}")
    for how in ("step", "rollout"):  # the specialised kernel's shape through the generic kernel
        yield pytest.param("crooms_table_yx_vmdp_spec", True, how, True,
                           id=f"crooms_table_yx_vmdp_spec-f32-{how}-generic")


@pytest.mark.parametrize("name,f32,how,generic", list(_philox_cases()))
def test_philox_mode_deterministic_rows(name, f32, how, generic, gpu_device):
    """With float32 I/O, a fixed goal, continuous actions and no velocity (yx_vmdp_spec, yx_vgmdp, thr*) the launch is
    crooms_rollout<GP_OBS_F32, false, 1>; `generic_kernels` forces the generic kernel on the same rows. The cardinal
    table's effective action comes from the stream (action_failure_probability), so it has no deterministic row in
    philox mode: it takes the checks that hold on every row."""
    import torch
    from gym_po_amd._lib import debug_knobs
    meta, data, _ = _table(name)
    kw = meta["kwargs"]
    B, dtype = meta["num_envs"], torch.float32 if f32 else torch.float64
    if generic:
        with debug_knobs(generic_kernels=1):
            env = _make(meta, dtype=dtype)
    else:
        env = _make(meta, dtype=dtype)
    env.reset(seed=meta["seed"])
    _set_rows(env, meta, data)
    a = _actions(data, dtype)
    if how == "step":
        o, r, d, tr = _outputs(env.step(a))
    else:
        a = torch.as_tensor(a)
        o, r, d, tr = (x[0] for x in _outputs(env.rollout(a[None])))
    d, tr = d.astype(bool), tr.astype(bool)
    ag, g, v, e = _state(env)
    cardinal = kw.get("action_type", "yx") == "cardinal"
    oob = data["oob"]
    # every row
    np.testing.assert_array_equal(tr, data["trunc"])
    rs, rw, rg = (np.float32(kw[k]) for k in ("step_reward", "wall_reward", "goal_reward"))
    assert (r[d] == rg).all()
    if cardinal:
        assert np.isin(r[~d], [rs, rw]).all()
    else:
        np.testing.assert_array_equal(r[~d], np.where(oob, rw, rs)[~d])
        # a wall hit that ends no episode: resampled inside the start cell, velocity dropped
        hit = oob & ~d & ~tr
        assert int(hit.sum()) >= (100 if (data["in_family"] == 0).any() else 0)
        cell = float(kw.get("cell_size", 1.0))
        c = np.floor(data["in_agent"] / cell) * cell + cell / 2
        assert (ag[hit] >= (c - cell / 2)[hit]).all() and (ag[hit] <= (c + cell / 2 - 1e-8)[hit]).all()
        assert (v[hit] == 0.0).all()
        # the deterministic rows: the reference's values
        det = ~(oob | data["term"] | data["trunc"])
        assert 2 * int(det.sum()) >= B
        assert not d[det].any()
        if o.dtype.kind == "f":
            ref = data["obs"].astype(np.float32) if f32 else data["obs"]
            assert o.dtype == ref.dtype
            np.testing.assert_array_equal(_bits(o[det]), _bits(ref[det]))
        else:
            np.testing.assert_array_equal(o[det].astype(np.int64), data["obs"][det].astype(np.int64))
        np.testing.assert_array_equal(r[det].view(np.uint32), data["rew"][det].view(np.uint32))
        np.testing.assert_array_equal(_bits(ag[det]), _bits(data["agent"][det]))
        np.testing.assert_array_equal(g[det], data["goal_cell"][det])
        np.testing.assert_array_equal(_bits(v[det]), _bits(data["velocity"][det]))
        np.testing.assert_array_equal(e[det], data["elapsed"][det])
    # elapsed: reset to 0 where the episode ended, one more than the input elsewhere
    np.testing.assert_array_equal(e, np.where(d | tr, 0, data["in_elapsed"] + 1))


AGENT_XY = [((3, 2), 1.0), ((8, 3), 1.0), ((3, 2), 2.0)]  # a walkable cell; a wall (-> rooms_starts_xy); cell_size 2


@pytest.mark.parametrize("mode", ["numpy", "replay"])
@pytest.mark.parametrize("agent_xy,cell_size", AGENT_XY)
def test_fixed_agent_cell_vs_oracle(agent_xy, cell_size, mode, gpu_device):
    """agent_xy: every env goes back to the fixed cell's centre, cell * cell_size + cell_size / 2, at each of its four
    time-limit resets (and at the goal); device == oracle at every step."""
    import torch
    from gym_po_amd import CRoomsEnv
    B, steps = 1027, 40
    kw = dict(obs_type="vector_mdp", agent_xy=agent_xy, cell_size=cell_size, time_limit=10, wall_reward=-0.5)
    acts = np.random.default_rng(6).uniform(-1, 1, (steps, B, 2)).astype(np.float32).astype(np.float64)
    ora = CRoomsOracle(B, **kw)
    env = CRoomsEnv(B, **kw, rng_mode=mode, dtype=torch.float64)
    ora.gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(31)))
    rd = RecordingDraws(ora.gen, B, ora.valid)
    o_ref = ora.reset(rd)
    if mode == "replay":
        env.set_replay(**replay_args(rd.rec, B))
        o = env.reset()
    else:
        o = env.reset(seed=31)
    start = np.asarray(o_ref).copy()
    assert (start == start[0]).all()
    np.testing.assert_array_equal(_bits(o.cpu().numpy()), _bits(o_ref))
    resets = np.zeros(B, int)
    for t in range(steps):
        rd = RecordingDraws(ora.gen, B, ora.valid)
        ro, rr, rdn, rt = ora.step(acts[t], rd)
        if mode == "replay":
            env.set_replay(**replay_args(rd.rec, B))
        o, r, d, tr = _outputs(env.step(torch.as_tensor(acts[t])))
        np.testing.assert_array_equal(_bits(o), _bits(ro), err_msg=f"t={t}")
        np.testing.assert_array_equal(r, rr, err_msg=f"t={t}")
        np.testing.assert_array_equal(d.astype(bool), rdn, err_msg=f"t={t}")
        np.testing.assert_array_equal(tr.astype(bool), rt, err_msg=f"t={t}")
        fin = rdn | rt
        assert (o[fin] == start[0]).all()
        resets += fin
    assert resets.min() >= 3  # elapsed passes time_limit = 10 at steps 11, 22 and 33
    a, _, v, e = _state(env)
    np.testing.assert_array_equal(_bits(a), _bits(ora.agent))
    np.testing.assert_array_equal(e, ora.elapsed)
    if mode == "numpy":
        assert rng6(env.np_random) == rng6(ora.gen)


@pytest.mark.parametrize("cell_size", [0.5, 0.999, 0.0, -1.0, float("nan")])
def test_cell_size_below_one_is_rejected(cell_size, gpu_device):
    from gym_po_amd import CRoomsEnv
    from gym_po_amd._lib import GymPoError
    with pytest.raises(GymPoError, match="cell_size"):
        CRoomsEnv(8, cell_size=cell_size)
