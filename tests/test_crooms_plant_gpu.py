"""C-ROOMS exact mode (rng_mode="numpy", csrc/crooms.hip) on planted Lemire rejections of choice().

A half-word of `rng.choice(valid_states, n)` is rejected with probability ~ n_valid / 2^32 (about 5e-8 for layout
"4"): no seeded trajectory of the suite reaches the paths that handle one -- the candidate ranks after the rejected
half, the per-block counts and prefixes, the last candidate consumed (has_uint32 / uinteger and the state jump) and
the extra word when the n-th draw is rejected. Here the PCG64 state is set (tests/stream_plant.py) so that a chosen
half-word of a chosen call is a rejected one, and the device is compared with the oracle (oracle/crooms.py) on numpy's
Generator holding the same state: obs, reward and flags of every step, get_state(), and the final rng_state with
has_uint32 / uinteger. Float64 I/O; tolerance: none. tests/test_stream_plant_cpu.py asserts for every case that numpy
does reject that half-word.

Placements: reset() without a seed after `env.rng_state = planted` (the stream starts at the choice call; with
goal_xy=None there are two calls, the plant in either), and a step whose word count before the call is exact
(cardinal actions, action_std=0, every agent on the centre of a cell with four free neighbours: B uniforms, no
normals; `elapsed` picks the envs that truncate). Paths: the one-workgroup kernel (x_choices) at 600 envs and across
a 1024-word window at 3000, the grid-wide fused calls (xg_cho_fused) at 1500 envs and in one partial block at 64,
the two-launch calls (xg_cho_count / xg_cho_write) at 1500, and a replayed hipGraph of the fused calls.
"""
import numpy as np
import pytest

import plant_cases as pc
import stream_plant as sp

pytestmark = pytest.mark.gpu


def _make_env(c, gpu_device, **knobs):
    import torch
    from gym_po_amd import CRoomsEnv
    from gym_po_amd._lib import debug_knobs
    with debug_knobs(**dict(c.knobs, **knobs)):
        return CRoomsEnv(c.B, **c.kw, rng_mode="numpy", dtype=torch.float64, device=gpu_device)


def _check_state(env, ora):
    a, g, v, e = (x.cpu().numpy() for x in env.get_state())
    np.testing.assert_array_equal(a, ora.agent, err_msg="agent")
    np.testing.assert_array_equal(g + 0.5, ora.goal, err_msg="goal")
    np.testing.assert_array_equal(v, ora.velocity, err_msg="velocity")
    np.testing.assert_array_equal(e, ora.elapsed, err_msg="elapsed")
    env.check()
    assert sp.rng6(env.rng_state) == sp.rng6(ora.gen.bit_generator.state)


def _check_step(got, want, tag):
    o, r, d, t = got
    oo, ro, do, to = want
    np.testing.assert_array_equal(np.asarray(o, dtype=np.float64), np.asarray(oo, dtype=np.float64),
                                  err_msg="obs " + tag)
    np.testing.assert_array_equal(r, ro, err_msg="rew " + tag)
    np.testing.assert_array_equal(np.asarray(d).astype(bool), do, err_msg="term " + tag)
    np.testing.assert_array_equal(np.asarray(t).astype(bool), to, err_msg="trunc " + tag)


def _set_step_state(env, c):
    goal = c.goal_cell if c.kw.get("goal_xy", 0) is None else None  # (a fixed goal stays the constructor's)
    env.set_state(agent_yx=c.agent, goal_cell_yx=goal, velocity=np.zeros((c.B, 2)), elapsed=c.elapsed)
    env.rng_state = c.st


def _ordinary_steps(env, ora, steps, seed):
    acts = np.random.default_rng(seed).integers(0, 4, (steps, env.num_envs))
    for t in range(steps):
        got = [x.cpu().numpy() for x in env.step(acts[t])[:4]]
        _check_step(got, ora.step_seeded(acts[t]), f"after the plant, t={t}")


@pytest.mark.parametrize("case", pc.crooms_cases(), ids=pc.crooms_id)
def test_planted_choice_rejection_vs_oracle(case, gpu_device):
    path, place, n, h, buffered, call, calls = case
    c = pc.crooms_build(case)
    env = _make_env(c, gpu_device)
    if place == "reset":
        env.rng_state = c.st
        o = env.reset().cpu().numpy()
        (oo, _, _, _), _ = pc.crooms_oracle_planted(c)
        np.testing.assert_array_equal(o.astype(np.float64), np.asarray(oo, dtype=np.float64), err_msg="reset obs")
    else:
        env.reset(seed=1)
        _set_step_state(env, c)
        got = [x.cpu().numpy() for x in env.step(c.actions)[:4]]
        want, _ = pc.crooms_oracle_planted(c)  # (asserts the precondition: no wall-noise normal was drawn)
        _check_step(got, want, "planted step")
    _check_state(env, c.ora)
    _ordinary_steps(env, c.ora, 2, seed=n + h)
    _check_state(env, c.ora)


GRAPH_CASES = [("fused1500", "step", n, h, b, call, calls) for n, h, b, call, calls in (
    (1, 0, True, 0, 1), (2, 1, False, 0, 1), (301, 0, False, 0, 1), (301, 300, True, 0, 1), (1500, 511, False, 0, 1),
    (1500, 512, False, 0, 1), (1500, 1499, False, 0, 1), (301, 300, False, 0, 2), (301, 0, False, 1, 2))]


@pytest.mark.parametrize("case", GRAPH_CASES, ids=pc.crooms_id)
def test_planted_choice_rejection_in_replayed_graph(case, gpu_device):
    """xg_graph=1: the K = 2 launch sequence is captured on the plan's first run() and replayed from then on. The
    plant is set before the third run(), whose first step is the planted one: a replayed graph meets the
    rejection."""
    import torch
    path, place, n, h, buffered, call, calls = case
    c = pc.crooms_build(case)
    env = _make_env(c, gpu_device, xg_graph=1)
    K = 2
    free = pc.CRoomsOracle(c.B, **c.kw)  # the two launches before the plant, from a seed
    np.testing.assert_array_equal(env.reset(seed=5).cpu().numpy().astype(np.float64),
                                  np.asarray(free.reset_seed(5), dtype=np.float64))
    a = torch.zeros((K, c.B), dtype=torch.int32, device=env.device)
    run, bufs = env.rollout_plan(a)
    acts = np.random.default_rng(6).integers(0, 4, (3 * K, c.B))
    acts[2 * K] = c.actions
    ora = free
    for launch in range(3):
        if launch == 2:
            _set_step_state(env, c)
            ora = c.ora
        a.copy_(torch.as_tensor(acts[launch * K:(launch + 1) * K].astype(np.int32)))
        run()
        got = [x.cpu().numpy() for x in bufs]
        for k in range(K):
            if launch == 2 and k == 0:
                want, _ = pc.crooms_oracle_planted(c)
            else:
                want = ora.step_seeded(acts[launch * K + k])
            _check_step([g[k] for g in got], want, f"launch {launch} step {k}")
        _check_state(env, ora)
