"""FourRooms / ROOMS (csrc/grid.hip, csrc/wgrid.hip) against the reference's one-step tables.

A grid step exists several times on the device: the fused persistent kernel (plain, LDS-staged, and staged with the
single-call "SPW" reset), the two-kernel path (streaming step + reset resolver), the windowed kernel (wgrid.hip), the
counter kernels of philox / replay mode and the closed-loop kernel's transition(). Random walks hardly meet the rows
where they can differ, so every (agent cell, intended action) row of the `grid_table` fixtures
(tests/golden/make_golden.py GRID_TABLES: goals on the destination, on every neighbour, on stairs and on the agent's
own cell; elapsed 0, time_limit - 1 and time_limit) goes through each of them in ONE launch from the recorded pre-step
stream state: the four outputs, get_state(), the final PCG64 state and the four metrics, all compared with ==.

return_sum: the rewards are 2, -1 and -0.25 and the device sums them (or counts times rewards) in float64 from the
thread on: every partial sum is a multiple of 0.25 far below 2^53 / 4, hence exact in any order, and equal to the
float64 sum of the fixture's rewards. (Rewards that are no short binary fractions: tests/test_metrics_precision_gpu.py.)
"""
import contextlib
import functools

import numpy as np
import pytest

from fixtures import grid_table_inputs, load_grid_table, load_index
from grid_table_oracle import (flat, metrics_of_step, new_metrics, replay_indices, rng6, rng_dict, set_rows,
                               step_uniforms, table_oracle)

pytestmark = pytest.mark.gpu

INDEX = load_index()["grid_table"]
TABLES = sorted(INDEX)


def _is_fixed(name):
    kw = INDEX[name]["kwargs"]
    return not (kw.get("goal_xyz", 0) is None or kw.get("goal_xy", 0) is None)


def _is_scalar(name):
    ot = INDEX[name]["kwargs"]["obs_type"]
    return not ("vector" in ot or "grid" in ot)


FIXED = [n for n in TABLES if _is_fixed(n)]          # fixed goal, scalar Hansen obs: the windowed kernel's configs
RANDOM = [n for n in TABLES if not _is_fixed(n)]
P0 = [n for n in TABLES if INDEX[n]["kwargs"]["action_failure_probability"] == 0.0]
assert len(FIXED) == 2 and len(P0) == 2 and all(_is_scalar(n) for n in FIXED + P0)


@functools.lru_cache(maxsize=None)
def _table(name):
    meta, data = load_grid_table(name)
    inp = grid_table_inputs(meta)
    ora = table_oracle(meta, inp)
    cells = dict(agent=flat(ora, inp["agent"]), goal=flat(ora, inp["goal"]), post_agent=flat(ora, data["agent"]),
                 post_goal=flat(ora, data["goal"]))
    return meta, data, inp, cells


def _env(name, device, **extra):
    from gym_po_amd import MultistoryFourRoomsEnv, RoomsEnv
    meta = INDEX[name]
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["kwargs"].items()}
    cls = MultistoryFourRoomsEnv if meta["kind"] == "fourrooms" else RoomsEnv
    return cls(meta["num_envs"], **kw, device=device, **extra)


def _knob_env(name, device, knobs, **extra):
    from gym_po_amd._lib import debug_knobs
    with debug_knobs(**knobs) if knobs else contextlib.nullcontext():
        return _env(name, device, **extra)


def _np(x):
    return x.cpu().numpy()


def _set_rows(env, name):
    """set_state must read back unchanged through get_state (a fixed goal is the configuration's own)."""
    meta, data, inp, cells = _table(name)
    goal = None if _is_fixed(name) else cells["goal"].astype(np.int32)
    env.set_state(agent_cells=cells["agent"].astype(np.int32), goal_cells=goal,
                  elapsed=inp["elapsed"].astype(np.int32))
    a, g, e = (_np(x).astype(np.int64) for x in env.get_state())
    np.testing.assert_array_equal(a, cells["agent"])
    np.testing.assert_array_equal(g, cells["goal"])
    np.testing.assert_array_equal(e, inp["elapsed"])


def _one_step(env, name, through):
    import torch
    inp = _table(name)[2]
    if through == "step":
        return env.step(inp["action"])[:4]
    acts = torch.as_tensor(inp["action"][None].astype(np.int32), device=env.device)
    return tuple(x[0] for x in env.rollout(acts))


def _assert_outputs(out, data, rows=None, msg=""):
    rows = slice(None) if rows is None else rows
    for k, x in zip(("obs", "rew", "term", "trunc"), out):
        got, ref = _np(x), data[k]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if k == "rew":
            assert got.dtype == np.float32 and ref.dtype == np.float32
        else:
            got, ref = got.astype(np.int64), ref.astype(np.int64)
        np.testing.assert_array_equal(got[rows], ref[rows], err_msg=f"{k} {msg}")


def _assert_state(env, name, msg=""):
    meta, data, inp, cells = _table(name)
    a, g, e = (_np(x).astype(np.int64) for x in env.get_state())
    np.testing.assert_array_equal(a, cells["post_agent"], err_msg=f"agent {msg}")
    np.testing.assert_array_equal(g, cells["post_goal"], err_msg=f"goal {msg}")
    np.testing.assert_array_equal(e, data["elapsed"].astype(np.int64), err_msg=f"elapsed {msg}")


def _table_metrics(name):
    meta, data, inp, _ = _table(name)
    m = metrics_of_step(new_metrics(), inp["elapsed"], data["rew"], data["term"], data["trunc"])
    return {k: float(v) for k, v in m.items()}


def _numpy_table(name, device, knobs, through, expect):
    """Numpy mode from the recorded stream alone; `expect`: the env.query values that name the path taken."""
    meta, data, inp, cells = _table(name)
    env = _knob_env(name, device, knobs)
    got = {k: env.query(k) for k in expect}
    for k, want in expect.items():
        assert (got[k] > 0) == want if isinstance(want, bool) else got[k] == want, (name, knobs, got)
    env.reset(seed=meta["seed"])  # the device's own reset burst reaches the recorded pre-step stream
    assert rng6(env.rng_state) == [int(v) for v in data["pre_rng_state"]]
    env.rng_state = rng_dict(data["pre_rng_state"])
    _set_rows(env, name)
    out = _one_step(env, name, through)
    msg = f"{name} {knobs} {through}"
    _assert_outputs(out, data, msg=msg)
    _assert_state(env, name, msg)
    env.check()
    assert rng6(env.rng_state) == [int(v) for v in data["rng_state"]], msg
    assert env.metrics() == _table_metrics(name), msg
    env.close()


def _fused_expect(staged, spw):
    return dict(fused_blocks=True, fused_staged=int(staged), fused_spw=int(spw))


# ------------------------------------------------------------------ numpy mode, the fused and two-kernel paths ----
@pytest.mark.parametrize("name", RANDOM)
def test_table_numpy_default(name, gpu_device):
    """Default routing: the staged fused kernel for a scalar obs (whole 512-env tiles), the plain one for a vector
    obs; two reset calls (random goal and random agent: no SPW)."""
    _numpy_table(name, gpu_device, {}, "step", dict(_fused_expect(_is_scalar(name), False), wgrid=0))


@pytest.mark.parametrize("name", RANDOM)
def test_table_numpy_unstaged(name, gpu_device):
    _numpy_table(name, gpu_device, dict(no_staging=1), "step", dict(_fused_expect(False, False), wgrid=0))


@pytest.mark.parametrize("name", RANDOM)
def test_table_numpy_no_spw(name, gpu_device):
    _numpy_table(name, gpu_device, dict(no_spw=1), "step", dict(_fused_expect(_is_scalar(name), False), wgrid=0))


@pytest.mark.parametrize("name", TABLES)
def test_table_numpy_two_kernel(name, gpu_device):
    """The streaming step kernel + the reset resolver."""
    _numpy_table(name, gpu_device, dict(disable_fused=1), "step", dict(fused_blocks=0, wgrid=0))


# ------------------------------------------------------------------ numpy mode, the fixed-goal scalar tables ----
@pytest.mark.parametrize("through", ["step", "rollout"])
@pytest.mark.parametrize("name", FIXED)
def test_table_windowed(name, through, gpu_device):
    """The windowed kernel (wgrid.hip) at its default launch-length split (512-env blocks: every length)."""
    _numpy_table(name, gpu_device, {}, through, dict(wgrid=1, wgrid_kmax=1 << 30, wgrid_block_envs=512))


@pytest.mark.parametrize("through", ["step", "rollout"])
@pytest.mark.parametrize("knobs,staged,spw", [({}, 1, 1), (dict(no_spw=1), 1, 0), (dict(no_staging=1), 0, 0)],
                         ids=["spw", "no_spw", "unstaged"])
@pytest.mark.parametrize("name", FIXED)
def test_table_fixed_goal_fused(name, knobs, staged, spw, through, gpu_device):
    """wg_kmax = 0 hands every launch of the same handle to the fused kernel: staged with the single-call SPW reset
    (a fixed goal, random agents), staged with SPW off, and unstaged."""
    _numpy_table(name, gpu_device, dict(knobs, wg_kmax=0), through,
                 dict(_fused_expect(staged, spw), wgrid=1, wgrid_kmax=0))


# ------------------------------------------------------------------ replay mode ----
@pytest.mark.parametrize("through", ["step", "rollout"])
@pytest.mark.parametrize("name", TABLES)
def test_table_replay(name, through, gpu_device):
    """counter_env_step with pre-decided draws: k = u * 2^53 of the recorded stream (exact), and the recorded
    post-state as the reset indices."""
    import torch
    meta, data, inp, cells = _table(name)
    env = _env(name, gpu_device, rng_mode="replay")
    ora = table_oracle(meta, inp)
    _, k = step_uniforms(data["pre_rng_state"], meta["num_envs"])
    gi, ai = replay_indices(ora, data["agent"], data["goal"])
    dev = gpu_device
    i0, i1 = torch.as_tensor(gi, device=dev), torch.as_tensor(ai, device=dev)
    env.set_replay(i0=i0, i1=i1)
    env.reset()
    _set_rows(env, name)
    env.set_replay(u=torch.as_tensor(k.view(np.int64), device=dev), i0=i0, i1=i1)
    out = _one_step(env, name, through)
    _assert_outputs(out, data, msg=name)
    _assert_state(env, name, name)
    env.check()
    assert env.metrics() == _table_metrics(name)
    env.close()


# ------------------------------------------------------------------ philox mode (the p = 0 tables) ----
def _assert_philox(env, name, out, rows):
    """`rows`: the rows this launch is judged on. Rows without an episode end: everything is the reference's; rows
    that end: reward and flags are, elapsed == 0, and the device's own draws land in the valid sets (obs: the oracle's
    obs function on the device's post-state)."""
    meta, data, inp, cells = _table(name)
    ora = table_oracle(meta, inp)
    fin = (data["term"] | data["trunc"]).astype(bool)
    keep = rows & ~fin
    assert keep.any() and (rows & fin).any()
    _assert_outputs(out, data, rows=keep, msg=name)
    for k, x in zip(("rew", "term", "trunc"), out[1:]):
        np.testing.assert_array_equal(_np(x).astype(np.float64)[rows], data[k].astype(np.float64)[rows], err_msg=k)
    a, g, e = (_np(x).astype(np.int64) for x in env.get_state())
    np.testing.assert_array_equal(a[keep], cells["post_agent"][keep])
    np.testing.assert_array_equal(g[keep], cells["post_goal"][keep])
    np.testing.assert_array_equal(e[keep], data["elapsed"].astype(np.int64)[keep])
    ended = rows & fin
    assert (e[ended] == 0).all()
    assert np.isin(a[ended], ora.valid_agent).all() and np.isin(g[ended], ora.valid_goal).all()
    za, zg = (np.array(np.unravel_index(x, ora.grid.shape)).T for x in (a, g))
    np.testing.assert_array_equal(_np(out[0]).astype(np.int64)[rows],
                                  np.asarray(ora.obs_fn(za, zg)).astype(np.int64)[rows], err_msg="obs of post-state")


@pytest.mark.parametrize("through", ["step", "rollout"])
@pytest.mark.parametrize("name", P0)
def test_table_philox(name, through, gpu_device):
    """The counter kernels on their own draws: with p = 0 the effective action is the intended one whatever is drawn
    (k > 0 = t_j for j < a, k <= 2^53 = t_j from a on; k = 0 has probability 2^-53)."""
    meta, data, inp, cells = _table(name)
    env = _env(name, gpu_device, rng_mode="philox")
    env.reset(seed=meta["seed"])
    _set_rows(env, name)
    out = _one_step(env, name, through)
    _assert_philox(env, name, out, np.ones(meta["num_envs"], bool))
    env.check()
    m, want = env.metrics(), _table_metrics(name)
    assert m == want  # (rewards, ends and lengths do not depend on the reset draws)
    env.close()


@pytest.mark.parametrize("name", P0)
def test_table_philox_closed_loop(name, gpu_device):
    """rollout_controller's transition() on the same rows: a one-node controller that plays action a for every obs,
    one launch per action (rows of one obs differ in their action), judged on the rows whose intended action is a."""
    meta, data, inp, cells = _table(name)
    env = _env(name, gpu_device, rng_mode="philox")
    n_obs, A = int(env.single_observation_space.n), int(env.single_action_space.n)
    for a in range(A):
        probs = np.zeros((n_obs, A))
        probs[:, a] = 1.0
        env.set_controller(probs=probs)
        env.reset(seed=meta["seed"])
        _set_rows(env, name)
        res = env.rollout_controller(1)
        rows = inp["action"] == a
        np.testing.assert_array_equal(_np(res["actions"][0]).astype(np.int64), np.full(meta["num_envs"], a))
        _assert_philox(env, name, (res["obs"][0], res["rew"][0], res["term"][0], res["trunc"][0]), rows)
        env.check()
    env.close()
