"""GPU tests of grid Ant-Tag's scalar index obs (obs_type="index": csrc/anttag.hip anttag_rollout_idx /
anttag_reset_idx) against the numpy oracle (oracle/anttag.py under tests/anttag_index_oracle.py) and against a
vector-obs twin given the same draws: only the obs plane may differ.

Every (ant, target, action, choose) of arenas 2, 5 and 16 goes through set_state + a replay step(), at the first and
at the last step of an episode. The philox rollouts run B = 2,051 envs (three 1,024-env tiles, the last one ragged)
for K = 48 steps under time_limit = 20 on a 6 x 6 arena (min_distance 3) and a 4 x 4 arena (min_distance 2); the
reference of each is computed once and shared, unchanged, by the tests that read it."""
import numpy as np
import pytest

from anttag_index_oracle import IndexObs
from oracle.anttag import AntTagOracle
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

B0, K0, SEED, TL = 2051, 48, 11, 20
CASES = {"size6": dict(size=6, min_distance=3.0), "size4": dict(size=4, min_distance=2.0)}
# Dyadic rewards: every partial sum of the kernel's float64 accumulation is a multiple of 0.25 far below 2^53 / 4 and
# therefore exact, so return_sum compares with == (tests/test_anttag_gpu.py; other rewards:
# tests/test_metrics_precision_gpu.py).
DYADIC = dict(tag_reward=2.0, step_reward=-0.25)


def _np(x):
    return x.cpu().numpy()


def make_env(num_envs, obs_type="index", **kw):
    from gym_po_amd import AntTagGridEnv
    kw = {**DYADIC, **kw}
    return AntTagGridEnv(num_envs, obs_type=obs_type, **kw)


def oracle_for(env, num_envs):
    return IndexObs(AntTagOracle(num_envs, size=env.size, tag_radius2=env.tag_radius2,
                                 visible_radius2=env.visible_radius2, min_start_dist2=env.min_start_dist2,
                                 time_limit=env.time_limit, **DYADIC))


def oracle_rollout(ora, acts, draws):
    """len(acts) oracle steps with draws(k): the stacked outputs and the four metrics the device accumulates."""
    outs, m = [], dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)
    for k in range(len(acts)):
        el0 = ora.elapsed.copy()
        o, r, d, tr = ora.step(acts[k], draws(k))
        fin = d | tr
        m["episodes"] += int(fin.sum())
        m["length_sum"] += int((el0[fin] + 1).sum())
        m["return_sum"] += float(r.astype(np.float64).sum())
        m["env_steps"] += ora.B
        outs.append((o, r, d, tr))
    return [np.stack(x) for x in zip(*outs)], m


def assert_outputs(dev, want, msg=""):
    for name, x, y in zip(("obs", "rew", "term", "trunc"), dev, want):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def assert_state(env, ora, msg=""):
    a, tg, e = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(a, ora.ant, err_msg=f"ant {msg}")
    np.testing.assert_array_equal(tg, ora.target, err_msg=f"target {msg}")
    np.testing.assert_array_equal(e, ora.elapsed, err_msg=f"elapsed {msg}")


def assert_metrics(env, want):
    got = env.metrics()
    for k in ("episodes", "return_sum", "length_sum", "env_steps"):
        assert got[k] == want[k], f"{k}: device {got[k]} oracle {want[k]}"


def fresh(case, num_envs=B0, obs_type="index", seed=SEED):
    """A reset env of `case` and the obs its reset returned."""
    env = make_env(num_envs, obs_type=obs_type, time_limit=TL, **CASES[case])
    return env, env.reset(seed=seed)[0]


_REFS = {}


def reference_run(case):
    """The oracle's K0-step rollout of `case` from SEED under uniform random actions (computed once, left unchanged):
    the reset is philox step 0, the env steps are steps 1..K0."""
    if case not in _REFS:
        env = make_env(8, time_limit=TL, **CASES[case])  # (only its squared radii are read)
        ora = oracle_for(env, B0)
        key = philox_key(SEED)
        obs0 = ora.reset(ora.philox_draws(0, key))
        acts = np.random.default_rng(SEED).integers(0, 5, (K0, B0)).astype(np.int32)

        def draws(k):
            return ora.philox_draws(k + 1, key)

        want, m = oracle_rollout(ora, acts, draws)
        nc = env.size ** 2
        hidden = want[0] % (nc + 1) == nc
        _REFS[case] = dict(obs0=obs0, acts=acts, want=want, metrics=m, ora=ora, hidden=hidden)
    return _REFS[case]


@pytest.fixture(params=sorted(CASES))
def case(request, gpu_device):
    return request.param


# ------------------------------------------------------------------ spaces ----
def test_spaces_and_obs_type(gpu_device):
    import torch
    from gym_po_amd import AntTagGridEnv
    env = make_env(7, size=5, min_distance=2.0)
    assert env.single_observation_space.n == 25 * 26 and env.obs_type == "index"
    o = env.reset(seed=1)[0]
    assert o.dtype == torch.int32 and tuple(o.shape) == (7,)
    o, r, d, t, _ = env.step(np.zeros(7, dtype=np.int64))
    assert o.dtype == torch.int32 and tuple(o.shape) == (7,)
    assert tuple(env.rollout(np.zeros((3, 7), dtype=np.int64))[0].shape) == (3, 7)
    vec = AntTagGridEnv(7, size=5, min_distance=2.0)  # the default stays the vector obs
    assert vec.obs_type == "vector" and vec.single_observation_space.shape == (4,)
    assert tuple(vec.reset(seed=1)[0].shape) == (7, 4)
    assert tuple(AntTagGridEnv(7, size=5, min_distance=2.0, obs_type="vector").reset(seed=1)[0].shape) == (7, 4)
    for bad in ("scalar", "", "Index"):
        with pytest.raises(NotImplementedError, match="Observation type not recognized"):
            AntTagGridEnv(7, obs_type=bad)
    # the queries of the closed-loop contract answer on every Ant-Tag handle: a reset, a step and 3 steps; a reset
    assert env.query("philox_step") == 5 and vec.query("philox_step") == 1
    for e in (env, vec):
        assert e.query("controller_nodes") == 0 and e.query("controller_lds") == 0
        assert e.query("num_envs") == 7


# ------------------------------------------------------------------ every transition ----
@pytest.mark.parametrize("size,min_distance", [(2, 0.0), (5, 2.0), (16, 5.0)])
def test_every_transition_one_step_vs_oracle_and_vector_twin(size, min_distance, gpu_device):
    import torch
    from gym_po_amd import ant_tag_obs_index
    nc = size * size
    ant, tgt, act, cho = (x.ravel() for x in np.meshgrid(np.arange(nc), np.arange(nc), np.arange(5), np.arange(4),
                                                         indexing="ij"))
    B = ant.size
    env = make_env(B, size=size, min_distance=min_distance, rng_mode="replay")
    twin = make_env(B, obs_type="vector", size=size, min_distance=min_distance, rng_mode="replay")
    ora = oracle_for(env, B)
    assert env.query("persist_occupancy") >= 1 and env.query("persist_blocks") >= 1
    rng = np.random.default_rng(size)
    want_m = dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)
    for el0 in (0, env.time_limit - 1):  # the first and the last step of an episode (truncation, same-step reset)
        dr = dict(choose=cho, ant=rng.integers(0, nc, B), tgt=rng.integers(0, nc + 8, B))
        ora.ant[:], ora.target[:], ora.elapsed[:] = ant, tgt, el0
        dev = []
        for e in (env, twin):
            e.set_replay(choose=dr["choose"], ant=dr["ant"], target_idx=dr["tgt"])
            e.set_state(ant, tgt, np.full(B, el0))
            dev.append(e.step(act)[:4])
        want, m = oracle_rollout(ora, act[None], lambda k: dr)
        assert_outputs([x[None] for x in dev[0]], want, msg=f"elapsed={el0}")
        assert_state(env, ora, msg=f"elapsed={el0}")
        for name, x, y in zip(("rew", "term", "trunc"), dev[0][1:], dev[1][1:]):
            assert torch.equal(x, y), f"{name} differs from the vector-obs twin, elapsed={el0}"
        for x, y in zip(env.get_state(), twin.get_state()):
            assert torch.equal(x, y)
        np.testing.assert_array_equal(ant_tag_obs_index(_np(dev[1][0]), size), want[0][0])
        assert want[2].any() and want[3].all() == (el0 > 0)
        for k in want_m:
            want_m[k] += m[k]
    assert_metrics(env, want_m)
    assert env.metrics() == twin.metrics()
    env.check()


# ------------------------------------------------------------------ philox rollouts from the seed ----
def test_reference_exercises_both_branches_and_episode_ends(case):
    """What the rollouts below rely on, asserted and not assumed: every env ends at least 2 episodes, both
    terminations and truncations occur, and the target is visible on some env-steps and hidden on others."""
    ref = reference_run(case)
    _, _, term, trunc = ref["want"]
    assert (term | trunc).sum(0).min() >= 2
    assert term.any() and trunc.any()
    vis = 1.0 - ref["hidden"].mean()
    assert 0.02 < vis < 0.98
    assert ref["metrics"]["episodes"] >= 2 * B0 and ref["metrics"]["env_steps"] == K0 * B0


def test_philox_rollout_vs_oracle_and_vector_twin(case):
    import torch
    from gym_po_amd import ant_tag_obs_index
    ref = reference_run(case)
    env, obs0 = fresh(case)
    np.testing.assert_array_equal(_np(obs0), ref["obs0"])  # the reset() obs
    assert env.query("philox_step") == 1
    dev = env.rollout(ref["acts"])
    assert env.query("philox_step") == 1 + K0
    assert dev[0].dtype == torch.int32 and tuple(dev[0].shape) == (K0, B0)
    assert_outputs(dev, ref["want"])
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    twin, tobs0 = fresh(case, obs_type="vector")
    np.testing.assert_array_equal(ant_tag_obs_index(_np(tobs0), env.size), ref["obs0"])
    tdev = twin.rollout(ref["acts"])
    np.testing.assert_array_equal(ant_tag_obs_index(_np(tdev[0]), env.size), ref["want"][0])
    for name, x, y in zip(("rew", "term", "trunc"), dev[1:], tdev[1:]):
        assert torch.equal(x, y), name
    for x, y in zip(env.get_state(), twin.get_state()):
        assert torch.equal(x, y)
    assert env.metrics() == twin.metrics()
    env.check()


def test_split_launches_equal_one_launch(case):
    import torch
    ref = reference_run(case)
    env, _ = fresh(case)
    acts = torch.from_numpy(ref["acts"]).to(env.device)
    parts = [env.rollout(acts[:20]), env.rollout(acts[20:21]), env.rollout(acts[21:])]  # 48 = 20 + 1 + 27
    whole = [torch.cat([p[i] for p in parts]) for i in range(4)]
    assert_outputs(whole, ref["want"])
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])
    assert env.query("philox_step") == 1 + K0


def test_step_equals_rollout_of_one(case):
    import torch
    ref = reference_run(case)
    env, _ = fresh(case)
    acts = torch.from_numpy(ref["acts"]).to(env.device)
    steps = [env.step(acts[k])[:4] for k in range(K0)]
    assert tuple(steps[0][0].shape) == (B0,)
    assert_outputs([torch.stack([s[i] for s in steps]) for i in range(4)], ref["want"])
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])


def test_rollout_plan(case):
    import torch
    ref = reference_run(case)
    env, _ = fresh(case)
    acts = torch.from_numpy(ref["acts"]).to(env.device)
    run, out = env.rollout_plan(acts)
    run()
    assert_outputs(out, ref["want"])
    assert_state(env, ref["ora"])
    assert_metrics(env, ref["metrics"])


# ------------------------------------------------------------------ batch shapes, store paths ----
@pytest.mark.parametrize("B", [1, 3, 5, 1024 * 3 + 1])
def test_batch_shapes_one_rollout_vs_oracle(B, gpu_device):
    from gym_po_amd._lib import debug_knobs
    K, seed = 9, 31
    with debug_knobs(persist_bpc=1):
        env = make_env(B, time_limit=4)
    ora = oracle_for(env, B)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(B).integers(0, 5, (K, B))
    dev = env.rollout(acts)
    want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    assert_outputs(dev, want)
    assert_state(env, ora)
    assert m["episodes"] >= 2 * B
    assert_metrics(env, m)


def test_blocks_looping_over_several_tiles(gpu_device):
    """One block per CU and more than two tiles per CU: every block loops over 2 tiles, block 0 over a third, ragged
    one (persist_bpc cannot give fewer blocks than CUs, so the batch has to exceed 1,024 envs per CU)."""
    import torch
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B, K, seed = 2 * 1024 * cus + 5, 6, 3
    with debug_knobs(persist_bpc=1):
        env = make_env(B, time_limit=3)
    assert env.query("persist_blocks") == cus and (B + 1023) // 1024 == 2 * cus + 1
    ora = oracle_for(env, B)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(seed).integers(0, 5, (K, B))
    dev = env.rollout(acts)
    want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    assert_outputs(dev, want)
    assert_state(env, ora)
    assert m["episodes"] >= B
    assert_metrics(env, m)


def _offset_view(torch, dtype, shape, offset, device):
    """A contiguous tensor of `shape` that starts `offset` elements into a larger allocation."""
    n = int(np.prod(shape))
    v = torch.zeros(n + 8, dtype=dtype, device=device)[offset:offset + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def test_misaligned_caller_buffers(gpu_device):
    """act / obs / rew views 4 B off their 16-B boundary and flag views 1 B off their 4-B boundary take the
    element-wise load and store paths at every step, all together and each alone (the kernel chooses per buffer and
    per step): the same values. The index obs has no alignment requirement."""
    import torch
    ref = reference_run("size6")
    acts = torch.from_numpy(ref["acts"]).to(gpu_device)
    # offsets in elements of (act, obs, rew, term, trunc)
    for offs in ((1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)):
        env, _ = fresh("size6")
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


# ------------------------------------------------------------------ replay mode ----
def test_replay_reset_step_and_rollout(gpu_device):
    """Replay mode: reset(), step() and a K > 1 rollout (the generic per-step path: K launches reading the installed
    draws), against the oracle and a vector-obs twin."""
    import torch
    B, K = 2049, 3
    a, b = (make_env(B, time_limit=2, min_distance=0, rng_mode="replay") for _ in range(2))
    twin = make_env(B, obs_type="vector", time_limit=2, min_distance=0, rng_mode="replay")
    ora = oracle_for(a, B)
    rng = np.random.default_rng(17)
    dr = dict(choose=rng.integers(0, 4, B), ant=rng.integers(0, 100, B), tgt=rng.integers(0, 120, B))
    want0 = ora.reset(dr)
    for env in (a, b, twin):
        env.set_replay(choose=dr["choose"], ant=dr["ant"], target_idx=dr["tgt"])
        o = env.reset()[0]
        if env is not twin:
            np.testing.assert_array_equal(_np(o), want0)
    acts = rng.integers(-5, 5, (K, B))
    whole = a.rollout(acts)
    steps = [b.step(acts[k])[:4] for k in range(K)]
    for i, name in enumerate(("obs", "rew", "term", "trunc")):
        assert torch.equal(whole[i], torch.stack([s[i] for s in steps])), name
    want, m = oracle_rollout(ora, acts, lambda k: dr)
    assert_outputs(whole, want)
    for env in (a, b):
        assert_state(env, ora)
        assert_metrics(env, m)
    tw = twin.rollout(acts)
    for name, x, y in zip(("rew", "term", "trunc"), whole[1:], tw[1:]):
        assert torch.equal(x, y), name
    assert twin.metrics() == a.metrics()
    assert m["episodes"] >= B and want[2].any()
    # a prepared rollout (one step: the draws are those of the step)
    c = make_env(B, time_limit=2, min_distance=0, rng_mode="replay")
    c.set_replay(choose=dr["choose"], ant=dr["ant"], target_idx=dr["tgt"])
    c.reset()
    run, out = c.rollout_plan(torch.from_numpy(acts[:1].astype(np.int32)).to(c.device))
    run()
    assert_outputs(out, [w[:1] for w in want])
