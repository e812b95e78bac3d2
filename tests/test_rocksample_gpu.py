"""GPU parity of the RockSample backend (csrc/rocksample.hip) against the numpy oracle of the build-defined rules
(tests/rocksample_oracle.py, itself pinned to a scalar statement by tests/test_rocksample_cpu.py): bit-exact on obs,
reward, both flags, the state afterwards and the four metrics.

Every (cell, mask, action) transition of three small grids at the first and the last step of an episode, random
states of the largest grid (16 x 16, 16 rocks: the 16 KB sensor table), rollouts over three 1,024-env tiles with a
ragged tail, split launches, single steps, batch sizes around the 4-env quads and the tiles, caller buffers off their
16-B boundaries, blocks that loop over several tiles, the reset law, the sensor on a rock's own cell, and the errors.
"""
import numpy as np
import pytest

from oracle.philox import philox_key
from rocksample_oracle import BAD, GOOD, RockSampleOracle, Spec, oracle_rollout

pytestmark = pytest.mark.gpu

# Dyadic rewards: every partial sum of the kernel's float64 accumulation (per thread over K steps x 4 envs x tiles,
# then 64 lanes, then 4 waves, then the slots) is a multiple of 0.25 far below 2^53 / 4 and therefore exact in any
# order, so return_sum compares with == against the float64 sum of the oracle's rewards. (Rewards that are no short
# binary fractions: tests/test_metrics_precision_gpu.py.)
DYADIC = dict(exit_reward=4.0, good_reward=2.0, bad_reward=-2.0, empty_reward=-1.0, check_reward=-0.25,
              step_reward=-0.5, wall_reward=-0.75)
ROCKS_232 = ((0, 1), (1, 2))
ROCKS_444 = ((0, 0), (1, 2), (3, 1), (3, 3))
ROCKS_578 = ((0, 0), (0, 6), (1, 3), (2, 2), (2, 5), (3, 0), (4, 4), (4, 6))
ROCKS_16 = tuple(((5 * i + 3) % 16, (11 * i + i // 4) % 16) for i in range(16))


def _np(x):
    return x.cpu().numpy()


def make(B, map_size=(5, 5), rocks=None, init_pos=(1, 1), obs_type="cell_sensor", time_limit=20, d0=1.5, **kw):
    """An env with dyadic rewards and a short-range sensor (wrong readings are common), and its oracle."""
    from gym_po_amd import RockSample
    env = RockSample(B, map_size=map_size, init_pos=init_pos, rocks=rocks, obs_type=obs_type, time_limit=time_limit,
                     half_efficiency_distance=d0, **DYADIC, **kw)
    return env, RockSampleOracle(B, Spec.of_env(env, **DYADIC))


def assert_outputs(dev, want, msg=""):
    for name, x, y in zip(("obs", "rew", "term", "trunc"), dev, want):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def assert_state(env, ora, msg=""):
    for name, x, y in zip(("agent", "mask", "elapsed"), env.get_state(), (ora.agent, ora.mask, ora.elapsed)):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def assert_metrics(env, want):
    got = env.metrics()
    for k in ("episodes", "return_sum", "length_sum", "env_steps"):
        assert got[k] == want[k], f"{k}: device {got[k]} oracle {want[k]}"


def add(total, m):
    for k in m:
        total[k] = total.get(k, 0) + m[k]


def one_step_from(env, ora, key, agent, mask, elapsed, act, total):
    """set_state, one step on both sides with the draws of the handle's step index, compare everything."""
    step = env.query("philox_step")
    env.set_state(agent=agent, rocks=mask, elapsed=elapsed)
    ora.agent[:], ora.mask[:], ora.elapsed[:] = agent, mask, elapsed
    assert_state(env, ora, "after set_state")
    o, r, d, tr, _ = env.step(act)
    want, m = oracle_rollout(ora, act[None], lambda k: ora.philox_draws(step, key))
    assert_outputs((o[None], r[None], d[None], tr[None]), want)
    assert_state(env, ora)
    add(total, m)
    return want


# ------------------------------------------------------------------ every transition ----
@pytest.mark.parametrize("obs_type", ["cell_sensor", "sensor"])
@pytest.mark.parametrize("H,W,rocks,init_pos", [(2, 3, ROCKS_232, (1, 0)), (4, 4, ROCKS_444, (2, 1)),
                                                (5, 7, ROCKS_578, (3, 1))])
def test_every_transition_one_step_vs_oracle(H, W, rocks, init_pos, obs_type, gpu_device):
    k, tl, seed = len(rocks), 9, 5
    A = 5 + k
    cell, mask, act = (x.ravel() for x in np.meshgrid(np.arange(H * W), np.arange(1 << k), np.arange(A),
                                                      indexing="ij"))
    B = cell.size
    env, ora = make(B, (H, W), rocks, init_pos, obs_type, tl)
    assert env.single_action_space.n == A
    assert env.single_observation_space.n == (H * W * 3 if obs_type == "cell_sensor" else 3)
    env.seed(seed)
    key = philox_key(seed)
    total = {}
    for el0 in (0, tl - 1):
        want = one_step_from(env, ora, key, cell, mask, np.full(B, el0), act, total)
        assert want[2].any() and want[3].all() == (el0 > 0) and want[3].any() == (el0 > 0)
        if el0 == 0:
            readings = want[0] % 3
            assert (readings[0][act >= 5] > 0).all() and not readings[0][act < 5].any()
            truth = np.where((mask >> np.clip(act - 5, 0, k - 1)) & 1, GOOD, BAD)
            wrong = (readings[0] != truth) & (act >= 5)
            assert wrong.any() and wrong.sum() < (act >= 5).sum() // 2  # the sensor errs, less than half the time
    assert_metrics(env, total)  # the second step counts terminated & truncated together as one episode each
    env.check()


@pytest.mark.parametrize("obs_type", ["cell_sensor", "sensor"])
def test_random_states_of_the_largest_grid(obs_type, gpu_device):
    B, tl, seed = 8192, 300, 9
    assert len(set(ROCKS_16)) == 16
    env, ora = make(B, (16, 16), ROCKS_16, (15, 15), obs_type, tl, d0=3.0)
    env.seed(seed)
    key = philox_key(seed)
    rng = np.random.default_rng(seed)
    total = {}
    for _ in range(2):
        want = one_step_from(env, ora, key, rng.integers(0, 256, B), rng.integers(0, 1 << 16, B),
                             rng.choice([0, 7, tl - 1], B), rng.integers(0, 21, B), total)
        assert want[2].any() and want[3].any() and not want[3].all() and len(np.unique(want[1])) == 7
    assert_metrics(env, total)
    env.check()


# ------------------------------------------------------------------ rollouts ----
B0, K0, TL0, SEED0 = 2051, 48, 20, 12345
_REF = {}


def reference_run(obs_type="cell_sensor"):
    """The oracle's 48-step run from the seed (7 x 7, 8 rocks): computed once, shared, left unchanged."""
    if obs_type not in _REF:
        env, ora = make(B0, (7, 7), ROCKS_578, (3, 1), obs_type, TL0)
        env.close()
        key = philox_key(SEED0)
        obs0 = ora.reset(ora.philox_draws(0, key))
        mask0 = ora.mask.copy()
        acts = np.random.default_rng(2).integers(0, 13, (K0, B0)).astype(np.int32)
        want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
        assert (want[2] | want[3]).sum(0).min() >= 2 and want[2].any() and want[3].any()
        _REF[obs_type] = dict(obs0=obs0, mask0=mask0, acts=acts, want=want, metrics=m, ora=ora)
    return _REF[obs_type]


def fresh(obs_type="cell_sensor", seed=SEED0, **kw):
    env, _ = make(B0, (7, 7), ROCKS_578, (3, 1), obs_type, TL0, **kw)
    obs0 = _np(env.reset(seed=seed)[0])
    return env, obs0


@pytest.mark.parametrize("obs_type", ["cell_sensor", "sensor"])
def test_rollout_from_the_seed_vs_oracle(obs_type, gpu_device):
    ref = reference_run(obs_type)
    env, obs0 = fresh(obs_type)
    np.testing.assert_array_equal(obs0, ref["obs0"])
    np.testing.assert_array_equal(_np(env.get_state()[1]), ref["mask0"])
    assert_outputs(env.rollout(ref["acts"]), ref["want"])
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    assert env.query("philox_step") == 1 + K0
    env.check()


def test_split_launches_and_single_steps(gpu_device):
    import torch
    ref = reference_run()
    env, _ = fresh()
    acts = torch.from_numpy(ref["acts"]).to(gpu_device)
    parts = [env.rollout(acts[a:b]) for a, b in ((0, 1), (1, 8), (8, 48))]
    assert_outputs([torch.cat([p[i] for p in parts]) for i in range(4)], ref["want"], "1 + 7 + 40")
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    env, _ = fresh()
    steps = [env.step(acts[k])[:4] for k in range(K0)]
    assert_outputs([torch.stack([s[i] for s in steps]) for i in range(4)], ref["want"], "48 steps")
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])


@pytest.mark.parametrize("B", [1, 3, 64, 1025])
def test_batch_shapes_one_rollout_vs_oracle(B, gpu_device):
    K, seed = 9, 31
    env, ora = make(B, (7, 7), ROCKS_578, (3, 1), time_limit=4)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(B).integers(0, 13, (K, B))
    dev = env.rollout(acts)
    want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    assert_outputs(dev, want)
    assert_state(env, ora)
    assert m["episodes"] >= 2 * B
    assert_metrics(env, m)


def _offset_view(torch, dtype, shape, offset, device):
    """A contiguous tensor of `shape` that starts `offset` elements into a larger allocation."""
    n = int(np.prod(shape))
    v = torch.zeros(n + 8, dtype=dtype, device=device)[offset:offset + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def test_misaligned_caller_buffers(gpu_device):
    """act / obs / rew / term / trunc views that start off their 16-B (4-B for the flags) boundaries take the scalar
    load and store paths at every step, all together and each alone (the kernel chooses per buffer and per step)."""
    import torch
    ref = reference_run()
    acts = torch.from_numpy(ref["acts"]).to(gpu_device)
    # offsets in elements of (act, obs, rew, term, trunc)
    for offs in ((1, 3, 1, 1, 3), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 2, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 2)):
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


def test_blocks_looping_over_several_tiles(gpu_device):
    import torch
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B, K, seed = 2 * 1024 * cus + 5, 6, 3
    with debug_knobs(persist_bpc=1):
        env, ora = make(B, (7, 7), ROCKS_578, (3, 1), time_limit=3)
    assert env.query("persist_blocks") == cus and (B + 1023) // 1024 == 2 * cus + 1
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(seed).integers(0, 13, (K, B))
    dev = env.rollout(acts)
    want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    assert_outputs(dev, want)
    assert_state(env, ora)
    assert m["episodes"] >= B
    assert_metrics(env, m)


# ------------------------------------------------------------------ reset and sensor ----
def test_reset_masks_and_seeds(gpu_device):
    import torch
    B = 4099
    env, ora = make(B, (7, 7), ROCKS_578, (3, 1))
    runs = []
    for seed in (7, 7, 8):
        obs0 = _np(env.reset(seed=seed)[0])
        agent, mask, el = (_np(x) for x in env.get_state())
        want = ora.philox_draws(0, philox_key(seed))["mask"]
        np.testing.assert_array_equal(mask, want)
        assert (agent == 3 * 7 + 1).all() and not el.any() and (obs0 == (3 * 7 + 1) * 3).all()
        acts = torch.from_numpy(np.random.default_rng(1).integers(0, 13, (30, B)).astype(np.int32)).to(gpu_device)
        runs.append([_np(x) for x in env.rollout(acts)] + [mask])
    for x, y in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(runs[0][4], runs[2][4]) and not np.array_equal(runs[0][0], runs[2][0])
    # every rock good with probability 1/2, independently: each of the 8 bits is set in 4099 / 2 +- 5 sigma envs
    bits = (runs[0][4][:, None] >> np.arange(8)) & 1
    assert (np.abs(bits.sum(0) - B / 2) < 5 * np.sqrt(B) / 2).all()
    # a second reset without a seed goes on in the stream: the masks of step index 1 + 30
    env.reset()
    np.testing.assert_array_equal(_np(env.get_state()[1]), ora.philox_draws(31, philox_key(8))["mask"])


def test_check_on_the_rocks_own_cell_reads_the_truth(gpu_device):
    B = 4096
    env, _ = make(B, (7, 7), ROCKS_578, (3, 1), obs_type="sensor", d0=0.25)
    assert (env.sensor_thresholds < (1 << 31)).sum() == 49 * 8 - 8  # (every other cell can read wrong)
    env.seed(4)
    rng = np.random.default_rng(4)
    rock = np.arange(B) % 8
    mask = rng.integers(0, 256, B)
    cells = np.array([y * 7 + x for y, x in ROCKS_578])
    env.set_state(agent=cells[rock], rocks=mask, elapsed=np.zeros(B))
    o, r, d, tr, _ = env.step(5 + rock)
    np.testing.assert_array_equal(_np(o), np.where((mask >> rock) & 1, GOOD, BAD))
    assert (_np(r) == -0.25).all() and not _np(d).any() and not _np(tr).any()
    # one cell away the same sensor errs
    env.set_state(agent=(cells[rock] + 7) % 49, rocks=mask, elapsed=np.zeros(B))
    o = _np(env.step(5 + rock)[0])
    assert (o != np.where((mask >> rock) & 1, GOOD, BAD)).sum() > B // 8


# ------------------------------------------------------------------ errors and API ----
@pytest.mark.parametrize("kw,match", [
    (dict(map_size=(0, 5), rocks=((0, 0),)), "per side"),
    (dict(map_size=(5, 17), rocks=((0, 0),)), "per side"),
    (dict(rocks=()), "rocks outside"),
    (dict(map_size=(5, 5), rocks=tuple((i // 5, i % 5) for i in range(17))), "rocks outside"),
    (dict(rocks=((0, 1), (2, 2), (0, 1))), "share cell"),
    (dict(rocks=((0, 1), (5, 0))), "off the"),
    (dict(rocks=((0, 1), (0, -1))), "off the"),
    (dict(init_pos=(1, 5)), "init_cell"),
    (dict(init_pos=(-1, 0)), "init_cell"),
    (dict(time_limit=0), "time_limit"),
    (dict(time_limit=65536), "time_limit"),
])
def test_invalid_configs_raise(kw, match, gpu_device):
    from gym_po_amd import RockSample
    from gym_po_amd._lib import GymPoError
    with pytest.raises(GymPoError, match=match):
        RockSample(8, **kw)


def test_sensor_table_entries_are_validated(gpu_device):
    import ctypes

    from gym_po_amd import _lib
    rocks = np.array([3], dtype=np.int32)
    thr = np.full((4, 1), 1 << 31, dtype=np.uint32)
    thr[2, 0] += 1
    cfg = _lib.RockSampleConfig()
    cfg.height, cfg.width, cfg.n_rocks, cfg.init_cell, cfg.obs_cell, cfg.time_limit = 2, 2, 1, 0, 1, 10
    cfg.rocks = rocks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cfg.sensor_thr = thr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    h = ctypes.c_void_p()
    rc = _lib.lib().gp_create(_lib.GP_KIND_ROCKSAMPLE, ctypes.byref(cfg), 8, 0, _lib.GP_RNG_PHILOX, ctypes.byref(h))
    assert rc == -1 and b"above 2^31" in _lib.lib().gp_last_error()
    thr[2, 0] -= 1
    assert _lib.lib().gp_create(_lib.GP_KIND_ROCKSAMPLE, ctypes.byref(cfg), 8, 0, _lib.GP_RNG_PHILOX,
                                ctypes.byref(h)) == 0
    _lib.lib().gp_destroy(h)


def test_rng_modes_actions_and_state_round_trip(gpu_device):
    import torch
    from gym_po_amd import RockSample
    from gym_po_amd._lib import GymPoError
    for mode in ("numpy", "replay"):
        with pytest.raises(GymPoError, match="philox"):
            RockSample(8, rng_mode=mode)
    B, A = 1003, 10
    env, ora = make(B)
    with pytest.raises(NotImplementedError):
        env.render()
    with pytest.raises(GymPoError, match="before reset"):
        env.step(np.zeros(B, dtype=np.int64))
    env.reset(seed=1)
    # a host array out of range raises as numpy indexing would; the env stays usable
    with pytest.raises(IndexError):
        env.step(np.full(B, A))
    with pytest.raises(IndexError):
        env.step(np.full(B, -A - 1))
    env.check()
    # action -1 is action A - 1
    twin, _ = make(B)
    twin.reset(seed=1)
    rng = np.random.default_rng(0)
    st = dict(agent=rng.integers(0, 25, B), rocks=rng.integers(0, 32, B), elapsed=rng.integers(0, 19, B))
    env.set_state(**st)
    twin.set_state(**st)
    neg = rng.integers(-A, 0, B)
    for x, y in zip(env.step(neg)[:4], twin.step(neg + A)[:4]):
        assert torch.equal(x, y)
    for x, y in zip(env.get_state(), twin.get_state()):
        assert torch.equal(x, y)
    env.check()
    # get_state / set_state round trip; None leaves a field alone; out-of-range values are clamped / masked
    cur = dict(agent=rng.integers(0, 25, B), rocks=rng.integers(0, 32, B), elapsed=rng.integers(0, 65536, B))
    env.set_state(**cur)
    for given in ((), ("agent",), ("rocks",), ("elapsed",), ("agent", "elapsed")):
        new = dict(agent=rng.integers(0, 25, B), rocks=rng.integers(0, 32, B), elapsed=rng.integers(0, 65536, B))
        env.set_state(**{k: new[k] for k in given})
        cur.update({k: new[k] for k in given})
        for name, x in zip(("agent", "rocks", "elapsed"), env.get_state()):
            np.testing.assert_array_equal(_np(x), cur[name], err_msg=f"{name} after set_state{given}")
    cells = np.resize(np.array([-1, -2 ** 31, 25, 255, 256, 2 ** 31 - 1, 0, 24]), B)
    env.set_state(agent=cells, rocks=np.resize(np.array([32, 63, -1, 1 << 20 | 5]), B),
                  elapsed=np.resize(np.array([-1, 65536, 65535, 2 ** 31 - 1]), B))
    a, m, e = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(a, np.clip(cells, 0, 24))
    np.testing.assert_array_equal(m, np.resize(np.array([0, 31, 31, 5]), B))
    np.testing.assert_array_equal(e, np.resize(np.array([0, 65535, 65535, 65535]), B))
    # a device tensor with action A is clamped on the device and flags the handle
    env.reset(seed=2)
    env.step(torch.full((B,), A, dtype=torch.int32, device=gpu_device))
    with pytest.raises(GymPoError, match="action"):
        env.check()
