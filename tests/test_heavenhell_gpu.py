"""GPU parity of the grid Heaven-Hell backend (csrc/heavenhell.hip) against the numpy oracle of the build-defined rules
(tests/heavenhell_oracle.py, itself pinned to a scalar statement by tests/test_heavenhell_cpu.py): bit-exact on obs,
reward, both flags, the state afterwards, the four metrics and the philox step index.

One-step tables over every (free cell, side, action in -4..3, elapsed first / last) of a 3 x 3 T and of the default
maze at three slip probabilities and both obs types, with the draws predicted on the CPU for each env index; rollouts
over three 1,024-env tiles with a ragged tail, split launches, single steps and a prepared plan, a 3-env batch, blocks
of a forced grid, blocks that loop over several tiles, caller buffers off their boundaries, the reset law, the state
round trip and the errors.
"""
import ctypes

import numpy as np
import pytest

from heavenhell_oracle import (FREE, LEFT, RIGHT, START, T3, HeavenHellOracle, Spec, enumeration, oracle_rollout)
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

# Dyadic rewards: every partial sum of the kernel's float64 accumulation (per thread over K steps x 4 envs x tiles,
# then 64 lanes, then 4 waves, then the slots) is a multiple of 0.25 far below 2^53 / 4 and therefore exact in any
# order, so return_sum compares with == against the float64 sum of the oracle's rewards. (Rewards that are no short
# binary fractions: tests/test_metrics_precision_gpu.py.)
DYADIC = dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=-0.25, wall_reward=-0.5)
# a T small enough that uniformly random actions reach both arms within 20 steps; two start cells
MID = ("L..P..R",
       "L.PPP.R",
       "##...##",
       "##.S.##",
       "##S..##")


def _np(x):
    return x.cpu().numpy()


def make(B, maze=None, obs_type="cell_signal", p=1 / 3, time_limit=20, **kw):
    """An env with dyadic rewards, and its oracle."""
    from gym_po_amd import HeavenHellGridEnv
    env = HeavenHellGridEnv(B, maze=maze, obs_type=obs_type, action_failure_probability=p, time_limit=time_limit,
                            **DYADIC, **kw)
    return env, HeavenHellOracle(B, Spec.of_env(env))


def assert_outputs(dev, want, msg=""):
    for name, x, y in zip(("obs", "rew", "term", "trunc"), dev, want):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def assert_state(env, ora, msg=""):
    for name, x, y in zip(("agent", "side", "elapsed"), env.get_state(), (ora.agent, ora.side, ora.elapsed)):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def assert_metrics(env, want):
    got = env.metrics()
    for k in ("episodes", "return_sum", "length_sum", "env_steps"):
        assert got[k] == want[k], f"{k}: device {got[k]} oracle {want[k]}"


# ------------------------------------------------------------------ one-step tables ----
@pytest.mark.parametrize("p", [0.0, 1 / 3, 1.0], ids=["p0", "p1_3", "p1"])
@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
@pytest.mark.parametrize("maze", [T3, None], ids=["t3", "default"])
def test_one_step_tables(maze, obs_type, p, gpu_device):
    tl, seed = 9, 5
    from gym_po_amd import heaven_hell_maze
    cell, side, act, el = enumeration(Spec(maze or heaven_hell_maze(), obs_type, time_limit=tl), tl)
    B = cell.size
    assert B == (2816 if maze is None else 160)
    env, ora = make(B, maze, obs_type, p, tl)
    assert env.single_action_space.n == 4 and env.single_observation_space.n == ora.sp.n_obs
    assert ora.sp.n_obs == (48 if obs_type == "hansen_signal" else ora.sp.H * ora.sp.W * 3)
    env.seed(seed)
    key = philox_key(seed)
    step = env.query("philox_step")
    assert step == 0
    env.set_state(agent=cell, heaven=side, elapsed=el)
    ora.agent[:], ora.side[:], ora.elapsed[:] = cell, side, el
    assert_state(env, ora, "after set_state")
    o, r, d, tr, _ = env.step(act)
    draws = ora.philox_draws(step, key)  # predicted on the CPU for each env index
    slipped = draws["y"] >= ora.sp.keep_thr
    assert slipped.all() if p == 1.0 else (not slipped.any() if p == 0.0 else (slipped.any() and not slipped.all()))
    want, m = oracle_rollout(ora, act[None], lambda k: draws)
    assert_outputs((o[None], r[None], d[None], tr[None]), want)
    assert_state(env, ora)
    assert_metrics(env, m)
    assert env.query("philox_step") == 1
    assert want[2].any() and not want[2].all() and (want[3][0] == (el == tl - 1)).all()
    assert set(np.unique(want[1])) == {1.0, -1.0, -0.25, -0.5}
    assert set(np.unique(want[0] % 3)) == {0, 1, 2}
    env.check()


# ------------------------------------------------------------------ rollouts ----
B0, K0, TL0, SEED0 = 2051, 48, 20, 12345
_REF = {}


def reference_run(obs_type="cell_signal"):
    """The oracle's 48-step run from the seed (the 5 x 7 T, p = 1/3): computed once, shared, left unchanged."""
    if obs_type not in _REF:
        env, ora = make(B0, MID, obs_type)
        env.close()
        key = philox_key(SEED0)
        obs0 = ora.reset(ora.philox_draws(0, key))
        state0 = (ora.agent.copy(), ora.side.copy())
        acts = np.random.default_rng(2).integers(0, 4, (K0, B0)).astype(np.int32)
        want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
        assert (want[2] | want[3]).sum(0).min() >= 2 and want[2].any() and want[3].any()
        assert set(np.unique(want[1])) == {1.0, -1.0, -0.25, -0.5} and set(np.unique(want[0] % 3)) == {0, 1, 2}
        _REF[obs_type] = dict(obs0=obs0, state0=state0, acts=acts, want=want, metrics=m, ora=ora)
    return _REF[obs_type]


def fresh(obs_type="cell_signal", seed=SEED0):
    env, _ = make(B0, MID, obs_type)
    obs0 = _np(env.reset(seed=seed)[0])
    return env, obs0


@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_rollout_from_the_seed_vs_oracle(obs_type, gpu_device):
    ref = reference_run(obs_type)
    env, obs0 = fresh(obs_type)
    np.testing.assert_array_equal(obs0, ref["obs0"])
    agent, side, el = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(agent, ref["state0"][0])
    np.testing.assert_array_equal(side, ref["state0"][1])
    assert not el.any() and set(np.unique(agent)) == {24, 30} and set(np.unique(side)) == {0, 1}
    assert_outputs(env.rollout(ref["acts"]), ref["want"])
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    assert env.query("philox_step") == 1 + K0
    env.check()


def test_split_launches_single_steps_and_plan(gpu_device):
    import torch
    ref = reference_run()
    env, _ = fresh()
    acts = torch.from_numpy(ref["acts"]).to(gpu_device)
    parts = [env.rollout(acts[a:b]) for a, b in ((0, 20), (20, 21), (21, 48))]
    assert_outputs([torch.cat([p[i] for p in parts]) for i in range(4)], ref["want"], "20 + 1 + 27")
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    assert env.query("philox_step") == 1 + K0
    env, _ = fresh()
    steps = [env.step(acts[k])[:4] for k in range(K0)]
    assert_outputs([torch.stack([s[i] for s in steps]) for i in range(4)], ref["want"], "48 steps")
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    assert env.query("philox_step") == 1 + K0
    env, _ = fresh()
    run, out = env.rollout_plan(acts)
    run()
    assert_outputs(out, ref["want"], "plan")
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    assert env.query("philox_step") == 1 + K0
    env.check()


def _short_run(B, maze, seed, K, tl):
    env, ora = make(B, maze, "hansen_signal", time_limit=tl)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(seed).integers(0, 4, (K, B))
    dev = env.rollout(acts)
    want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    assert_outputs(dev, want)
    assert_state(env, ora)
    assert_metrics(env, m)
    assert env.query("philox_step") == 1 + K
    env.check()
    return env, m


def test_three_envs(gpu_device):
    _, m = _short_run(3, MID, 31, 9, 4)
    assert m["episodes"] >= 2 * 3 and m["env_steps"] == 27


def test_forced_blocks_per_cu(gpu_device):
    """B = 9,221 is 10 tiles, the last with 5 envs. The knob forces the blocks per CU; on a device with more CUs than
    tiles the grid is then still one block per tile (the next test makes blocks loop)."""
    import torch
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    with debug_knobs(persist_bpc=1):
        env, m = _short_run(9221, None, 3, 12, 5)
    assert env.query("persist_blocks") == min(cus, 10)
    assert m["episodes"] >= 2 * 9221


def test_blocks_looping_over_several_tiles(gpu_device):
    import torch
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B = 2 * 1024 * cus + 5
    with debug_knobs(persist_bpc=1):
        env, m = _short_run(B, MID, 3, 6, 3)
    assert env.query("persist_blocks") == cus and (B + 1023) // 1024 == 2 * cus + 1
    assert m["episodes"] >= B


def _offset_view(torch, dtype, shape, offset, device):
    """A contiguous tensor of `shape` that starts `offset` elements into a larger allocation."""
    n = int(np.prod(shape))
    v = torch.zeros(n + 8, dtype=dtype, device=device)[offset:offset + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def test_buffers_offset_by_one_element(gpu_device):
    """act / obs / rew / term / trunc views that start one element off their 16-B (4-B for the flags) boundaries take
    the element-wise load and store paths at every step, all together and each alone."""
    import torch
    ref = reference_run()
    acts = torch.from_numpy(ref["acts"]).to(gpu_device)
    for offs in ((1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)):
        env, _ = fresh()
        act = _offset_view(torch, torch.int32, (K0, B0), offs[0], gpu_device)
        act.copy_(acts)
        out = (_offset_view(torch, torch.int32, (K0, B0), offs[1], gpu_device),
               _offset_view(torch, torch.float32, (K0, B0), offs[2], gpu_device),
               _offset_view(torch, torch.uint8, (K0, B0), offs[3], gpu_device),
               _offset_view(torch, torch.uint8, (K0, B0), offs[4], gpu_device))
        got = env.rollout(act, out=out)
        assert [x.data_ptr() for x in got] == [x.data_ptr() for x in out]  # written in place, not into copies
        assert_outputs(got, ref["want"], f"offsets={offs}")
        assert_state(env, ref["ora"])
        assert_metrics(env, ref["metrics"])
        env.check()


# ------------------------------------------------------------------ reset, state, errors ----
def test_reset_law_and_seeds(gpu_device):
    B = 4099
    env, ora = make(B)  # the default maze: start cells 119 and 120
    runs = []
    for seed in (7, 7, 8):
        obs0 = _np(env.reset(seed=seed)[0])
        agent, side, el = (_np(x) for x in env.get_state())
        d = ora.philox_draws(0, philox_key(seed))
        np.testing.assert_array_equal(agent, d["start"])
        np.testing.assert_array_equal(side, d["side"])
        assert not el.any() and (obs0 == agent * 3).all()
        runs.append((agent, side))
    assert all(np.array_equal(x, y) for x, y in zip(runs[0], runs[1]))
    assert not np.array_equal(runs[0][1], runs[2][1])
    for x, values in ((runs[0][0], (119, 120)), (runs[0][1], (0, 1))):  # fair coins: B / 2 +- 5 sigma
        assert set(np.unique(x)) == set(values) and abs((x == values[0]).sum() - B / 2) < 5 * np.sqrt(B) / 2
    # a second reset without a seed goes on in the stream: the draws of step index 1
    env.reset()
    np.testing.assert_array_equal(_np(env.get_state()[1]), ora.philox_draws(1, philox_key(8))["side"])
    assert env.query("philox_step") == 2 and env.query("num_envs") == B and env.query("rng_mode") == 1
    assert env.query("persist_blocks") >= 1 and env.query("persist_occupancy") >= 1
    assert env.query("controller_nodes") == 0 and env.query("controller_lds") == 0


def test_state_round_trip_and_actions(gpu_device):
    import torch
    from gym_po_amd._lib import GymPoError
    B = 1003
    env, _ = make(B)
    with pytest.raises(NotImplementedError):
        env.render()
    with pytest.raises(GymPoError, match="before reset"):
        env.step(np.zeros(B, dtype=np.int64))
    env.reset(seed=1)
    with pytest.raises(IndexError):
        env.step(np.full(B, 4))
    with pytest.raises(IndexError):
        env.step(np.full(B, -5))
    env.check()
    rng = np.random.default_rng(0)
    free = np.flatnonzero(env.flags & FREE)
    # action -k is action 4 - k
    twin, _ = make(B)
    twin.reset(seed=1)
    st = dict(agent=rng.choice(free, B), heaven=rng.integers(0, 2, B), elapsed=rng.integers(0, 19, B))
    env.set_state(**st)
    twin.set_state(**st)
    neg = rng.integers(-4, 0, B)
    for x, y in zip(env.step(neg)[:4], twin.step(neg + 4)[:4]):
        assert torch.equal(x, y)
    for x, y in zip(env.get_state(), twin.get_state()):
        assert torch.equal(x, y)
    # None leaves a field alone
    cur = dict(agent=rng.integers(0, 160, B), heaven=rng.integers(0, 2, B), elapsed=rng.integers(0, 65536, B))
    env.set_state(**cur)
    for given in ((), ("agent",), ("heaven",), ("elapsed",), ("agent", "elapsed")):
        new = dict(agent=rng.integers(0, 160, B), heaven=rng.integers(0, 2, B), elapsed=rng.integers(0, 65536, B))
        env.set_state(**{k: new[k] for k in given})
        cur.update({k: new[k] for k in given})
        for name, x in zip(("agent", "heaven", "elapsed"), env.get_state()):
            np.testing.assert_array_equal(_np(x), cur[name], err_msg=f"{name} after set_state{given}")
    # out-of-range values are clamped (cell, elapsed) or keep their low bit (side), as RockSample's are
    cells = np.resize(np.array([-1, -2 ** 31, 160, 255, 256, 2 ** 31 - 1, 0, 159]), B)
    env.set_state(agent=cells, heaven=np.resize(np.array([2, 3, -1, 1 << 20]), B),
                  elapsed=np.resize(np.array([-1, 65536, 65535, 2 ** 31 - 1]), B))
    a, h, e = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(a, np.clip(cells, 0, 159))
    np.testing.assert_array_equal(h, np.resize(np.array([0, 1, 1, 0]), B))
    np.testing.assert_array_equal(e, np.resize(np.array([0, 65535, 65535, 65535]), B))
    env.check()
    # a device tensor with action 4 is clamped on the device and flags the handle
    env.reset(seed=2)
    env.step(torch.full((B,), 4, dtype=torch.int32, device=gpu_device))
    with pytest.raises(GymPoError, match="action"):
        env.check()


def test_rng_modes_refused(gpu_device):
    from gym_po_amd import HeavenHellGridEnv
    from gym_po_amd._lib import GymPoError
    for mode in ("numpy", "replay"):
        with pytest.raises(GymPoError, match=r"\(-3\).*philox"):
            HeavenHellGridEnv(8, rng_mode=mode)


def _create_raw(H, W, flags, base=None, base_n=None, keep_thr=1 << 31, time_limit=10):
    from gym_po_amd import _lib
    flags = np.asarray(flags, dtype=np.uint8)
    base = np.arange(flags.size, dtype=np.int32) if base is None else np.asarray(base, dtype=np.int32)
    cfg = _lib.HeavenHellConfig()
    cfg.height, cfg.width, cfg.obs_base_n = H, W, flags.size if base_n is None else base_n
    cfg.flags = flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    cfg.obs_base = base.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cfg.keep_thr, cfg.time_limit = keep_thr, time_limit
    h = ctypes.c_void_p()
    rc = _lib.lib().gp_create(_lib.GP_KIND_HEAVENHELL, ctypes.byref(cfg), 8, 0, _lib.GP_RNG_PHILOX, ctypes.byref(h))
    msg = _lib.lib().gp_last_error().decode()
    if rc == 0:
        _lib.lib().gp_destroy(h)
    return rc, msg


def test_the_library_refuses_a_bad_config_by_name(gpu_device):
    S, L, R, F = FREE | START, FREE | LEFT, FREE | RIGHT, FREE
    assert _create_raw(1, 3, [L, S, R])[0] == 0
    for args, kw, match in [
        ((1, 3, [L, F, R]), {}, "no start cell"),
        ((1, 3, [L | START, S, R]), {}, "lies in the left area"),
        ((1, 3, [L, S, R | START]), {}, "lies in the right area"),
        ((1, 17, [S] * 17), {}, "per side"),
        ((17, 1, [S] * 17), {}, "per side"),
        ((0, 3, [S] * 3), {}, "per side"),
        ((1, 3, [L, S, 32 | FREE]), {}, "outside the set"),
        ((1, 3, [L, S, START]), {}, "outside the set"),       # a wall that is a start cell
        ((1, 3, [L | RIGHT, S, R]), {}, "outside the set"),   # two areas in one cell
        ((1, 3, [L, S, R]), dict(time_limit=0), "time_limit"),
        ((1, 3, [L, S, R]), dict(time_limit=65536), "time_limit"),
        ((1, 3, [L, S, R]), dict(keep_thr=(1 << 31) + 1), "keep_thr"),
        ((1, 3, [L, S, R]), dict(base=[0, 3, 1]), "obs_base"),
        ((1, 3, [L, S, R]), dict(base_n=257), "obs_base_n"),
    ]:
        rc, msg = _create_raw(*args, **kw)
        assert rc == -1 and match in msg, (args, kw, rc, msg)
