"""The ordering contract of include/gym_po_amd.h on a side stream: "All calls are asynchronous on the given hipStream_t".

Every other GPU test runs on the null stream, where every kernel and copy is serialised with every other. Here each
entry point and backend runs on a non-blocking side stream behind a busy-wait, with device inputs that hold poison until
a copy queued behind that busy-wait replaces them (tests/stream_order.py). The result must equal, bit for bit, a twin env
that ran the true inputs on the null stream (the values the rest of the suite pins to the oracles); a twin that ran the
poison must differ (else the case is vacuous and fails); and every call the header does not document as waiting must
return while the busy-wait is still running (`still`). Only one stream has work at a time, the null stream is idle; the
one exception is the positive control, which launches on a second stream on purpose and must read the poison.

Shapes are the smallest at which each kernel path is still the one selected (asserted through query() where a key
exists), K <= 8 steps.

Measured on an MI355X (three runs of the whole module): the busy-wait is calibrated to 100.0 ms (accepted between 50
and 200 ms). `still` held for all 171 asynchronous cases in every run; the longest enqueue of a call under test was
25.5 ms (one run: the first numpy-mode FourRooms launch of the fused kernel on a fresh handle; 2.6 ms in the others),
then 16.6 ms (two Ant-Tag rollouts, every run), every other case under 3.5 ms: the delay is four times the longest. The
25 cases of documented waiting calls returned after 99.4 - 108.5 ms, i.e. when the delay ended. 197 tests, 27 - 30 s in
all, the slowest 0.4 s.
"""
import ctypes

import numpy as np
import pytest

import stream_order as so

pytestmark = pytest.mark.gpu

K, SEED = 6, 7
DYADIC_TAXI = dict(reward_goal=1.0, reward_bad=-0.5, reward_any=-0.0625)  # (sums of dyadic rewards are exact in any order)


def _knobs(**kw):
    from gym_po_amd._lib import debug_knobs
    return debug_knobs(**kw)


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


# ------------------------------------------------------------------ backends ----
def _fourrooms_numpy(B, **knobs):
    from gym_po_amd import MultistoryFourRoomsEnv
    with _knobs(**knobs):
        return MultistoryFourRoomsEnv(B, grid_z=1, obs_type="hansen", time_limit=5)


def mk_rooms_philox():
    from gym_po_amd import RoomsEnv
    return RoomsEnv(1027, layout="4", obs_type="hansen", time_limit=5, rng_mode="philox")


def mk_fourrooms_philox():
    from gym_po_amd import MultistoryFourRoomsEnv
    return MultistoryFourRoomsEnv(1027, grid_z=1, obs_type="hansen", time_limit=5, rng_mode="philox")


def mk_fourrooms_fused():
    env = _fourrooms_numpy(8192, no_wgrid=1)
    assert env.query("wgrid") == 0 and env.query("fused_blocks") > 0
    return env


def mk_fourrooms_wgrid():
    env = _fourrooms_numpy(8192)  # the smallest B of test_wgrid_gpu.py's block-size cases
    assert env.query("wgrid") == 1 and env.query("wgrid_block_envs") == 512
    return env


def mk_rooms_replay():
    import torch
    from gym_po_amd import RoomsEnv
    B = 1027
    env = RoomsEnv(B, layout="4", obs_type="hansen", time_limit=5, goal_xy=None, rng_mode="replay")
    rng = np.random.default_rng(3)
    u = _dev(rng.integers(0, 1 << 53, B, dtype=np.int64))
    i0 = _dev(rng.integers(0, max(len(env.valid_cells(0)), 1), B).astype(np.int32))
    i1 = _dev(rng.integers(0, max(len(env.valid_cells(1)), 1), B).astype(np.int32))
    torch.cuda.synchronize()
    env.set_replay(u=u, i0=i0, i1=i1)
    return env


def _taxi(B, rng_mode, **kw):
    from gym_po_amd import TaxiVecEnv
    return TaxiVecEnv(B, time_limit=5, hansen_obs=True, rng_mode=rng_mode, **DYADIC_TAXI, **kw)


def mk_taxi_philox():
    return _taxi(1027, "philox")


def mk_taxi_replay():
    import torch
    env = _taxi(1027, "replay")
    rs = np.random.default_rng(4).choice(env.valid_states, env.num_envs).astype(np.int32)
    env.set_replay(reset_states=rs, pd=rs % (env.nlocs * (env.nlocs + 1)))
    torch.cuda.synchronize()
    return env


def mk_taxi_numpy_wg():
    return _taxi(512, "numpy")  # up to 1,024 envs: taxi_np_kernel, one workgroup


def mk_taxi_numpy_grid():
    with _knobs(taxi_npg_min=0):  # the grid-wide taxi_npg_* launches, forced as test_taxi_numpy_gpu.py forces them
        return _taxi(64, "numpy")


def _crooms(B, rng_mode, **kw):
    import torch
    from gym_po_amd import CRoomsEnv
    return CRoomsEnv(B, obs_type="vector_mdp", time_limit=5, rng_mode=rng_mode, dtype=torch.float64, **kw)


def mk_crooms_philox():
    return _crooms(1027, "philox")


def mk_crooms_replay():
    import torch
    B = 1027
    env = _crooms(B, "replay", goal_xy=None)
    rng = np.random.default_rng(5)
    env.set_replay(u=rng.integers(0, 1 << 53, B, dtype=np.int64).astype(np.uint64),
                   goal_idx=rng.integers(0, max(len(env.valid_cells(0)), 1), B).astype(np.int32),
                   agent_idx=rng.integers(0, max(len(env.valid_cells(1)), 1), B).astype(np.int32),
                   noise=rng.normal(0, 0.2, (B, 2)), wall_noise=rng.normal(0, 0.5, (B, 2)))
    torch.cuda.synchronize()
    return env


def mk_crooms_numpy_wg():
    return _crooms(257, "numpy")  # B <= 1,024: crooms_numpy_rollout, one workgroup


def mk_crooms_numpy_grid():
    with _knobs(xg_min_envs=0, xg_graph=0):  # the grid-wide xg_* draw calls, launched eagerly
        return _crooms(257, "numpy")


def mk_crooms_numpy_graph():
    with _knobs(xg_min_envs=0, xg_graph=1):  # the same as a hipGraph from the first call
        return _crooms(257, "numpy")


def mk_anttag_vector():
    from gym_po_amd import AntTagGridEnv
    return AntTagGridEnv(1027, size=4, min_distance=2.0, time_limit=5, obs_type="vector")


def mk_anttag_index():
    from gym_po_amd import AntTagGridEnv
    return AntTagGridEnv(1027, size=4, min_distance=2.0, time_limit=5, obs_type="index")


def mk_carflag_f32():
    from gym_po_amd import CarVecEnv
    return CarVecEnv(1027, time_limit=5, rng_mode="philox")


def mk_carflag_numpy():
    from gym_po_amd import CarVecEnv
    return CarVecEnv(1027, time_limit=5)  # the default rng_mode: numpy's stream


def mk_carflag_discrete():
    from gym_po_amd import DiscreteActionCarVecEnv
    return DiscreteActionCarVecEnv(7, 1027, time_limit=5, rng_mode="philox")


def mk_rocksample():
    from gym_po_amd import RockSample
    return RockSample(1027, time_limit=5)


def mk_heavenhell():
    from gym_po_amd import HeavenHellGridEnv
    return HeavenHellGridEnv(1027, action_failure_probability=0.25, time_limit=5)


def _pomdp(model, B=1027):
    from gym_po_amd import TabularPOMDPEnv
    from test_pomdp_gpu import tables
    T, Z, R, start, terminal, reset_obs = tables(model)
    return TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs, time_limit=5)


def mk_pomdp_tiger():
    env = _pomdp("tiger")
    assert env.query("pomdp_lds") == 1
    return env


def mk_pomdp_m37():
    env = _pomdp("m37")
    assert env.query("pomdp_lds") == 0  # the 48,608 B blob stays in global memory
    return env


BACKENDS = {f.__name__[3:]: f for f in (
    mk_rooms_philox, mk_fourrooms_philox, mk_fourrooms_fused, mk_fourrooms_wgrid, mk_rooms_replay,
    mk_taxi_philox, mk_taxi_replay, mk_taxi_numpy_wg, mk_taxi_numpy_grid,
    mk_crooms_philox, mk_crooms_replay, mk_crooms_numpy_wg, mk_crooms_numpy_grid, mk_crooms_numpy_graph,
    mk_anttag_vector, mk_anttag_index, mk_carflag_f32, mk_carflag_numpy, mk_carflag_discrete, mk_rocksample, mk_heavenhell,
    mk_pomdp_tiger, mk_pomdp_m37)}

_ACTIONS = {}


def actions_of(backend, k):
    """(true, poison) host action planes [k, B(, 2)] of a backend: every poison action differs from the true one."""
    if (backend, k) not in _ACTIONS:
        import torch
        env = BACKENDS[backend]()
        rng = np.random.default_rng(11)
        shape = (k, env.num_envs) + tuple(env._action_tail)
        if env._action_dtype == "int32":
            n = int(env.single_action_space.n)
            a = rng.integers(0, n, shape).astype(np.int32)
            p = ((a + rng.integers(1, n, shape)) % n).astype(np.int32)
        else:
            dt = np.float32 if env._action_dtype == "float32" else np.float64
            a = rng.uniform(-1, 1, shape).astype(dt)
            p = (-a).astype(dt)
        torch.cuda.synchronize()
        env.close()
        _ACTIONS[(backend, k)] = (a, p)
    return _ACTIONS[(backend, k)]


def _named(o):
    return dict(zip(("obs", "rew", "term", "trunc"), o))


def call_step(env, b):
    return _named(env.step(b["a"][0])[:4])


def call_rollout(env, b):
    return _named(env.rollout(b["a"]))


def call_rollout_out(env, b):
    out = env._alloc_outputs(int(b["a"].shape[0]))
    return _named(env.rollout(b["a"], out=out))


def call_plan(env, b):
    run, outs = env.rollout_plan(b["a"])
    run()
    return _named(outs)


THROUGH = {"step": call_step, "rollout": call_rollout, "rollout_out": call_rollout_out, "rollout_plan": call_plan}


# ------------------------------------------------------------------ late actions ----
@pytest.mark.parametrize("through", sorted(THROUGH))
@pytest.mark.parametrize("backend", sorted(BACKENDS))
def test_late_actions(backend, through, gpu_device):
    k = 1 if through == "step" else K
    a, p = actions_of(backend, k)
    so.run_case(f"{backend}/{through}", BACKENDS[backend], SEED, THROUGH[through], {"a": a}, {"a": p},
                ref_key=f"{backend}/{'step' if k == 1 else 'rollout'}",
                ref_call=call_step if k == 1 else call_rollout)


def test_crooms_graph_replay_on_side_stream(gpu_device):
    """Three calls of one plan with the same buffers: under xg_graph=1 the first captures the launch sequence (on the
    handle's private capture stream) and every call is a hipGraphLaunch on the caller's stream; the third is a replay
    of an existing graph. All three sit behind the delay and read the late actions."""
    def call(env, b):
        run, outs = env.rollout_plan(b["a"])
        res = {}
        for i in range(3):
            run()
            res[i] = so.clone_outputs(_named(outs))
        return res
    a, p = actions_of("crooms_numpy_graph", 3)
    so.run_case("crooms_numpy_graph/3 calls", mk_crooms_numpy_graph, SEED, call, {"a": a}, {"a": p})


# ------------------------------------------------------------------ chained launches ----
def call_two_rollouts(env, b):
    import torch
    k = int(b["a"].shape[0]) // 2
    o1, o2 = env.rollout(b["a"][:k]), env.rollout(b["a"][k:])
    return _named([torch.cat((x, y)) for x, y in zip(o1, o2)])


@pytest.mark.parametrize("backend", sorted(BACKENDS))
def test_chained_launches(backend, gpu_device):
    """Two K-step rollouts back to back behind one delay equal one 2K-step rollout of the reference: the hand-off of
    env state, metric slots, window and tag state and the philox step between launches happens on the stream."""
    a, p = actions_of(backend, 2 * K)
    so.run_case(f"{backend}/2 x rollout", BACKENDS[backend], SEED, call_two_rollouts, {"a": a}, {"a": p},
                ref_key=f"{backend}/rollout2K", ref_call=call_rollout)


# ------------------------------------------------------------------ late state ----
_STATES = {}
STATE_BACKENDS = ["rooms_philox", "fourrooms_wgrid", "taxi_philox", "taxi_numpy_wg", "crooms_philox", "crooms_numpy_grid",
                  "anttag_index", "carflag_f32", "rocksample", "heavenhell", "pomdp_tiger"]


def states_of(backend):
    """Two valid states of a backend (host arrays in get_state order): after some steps from two seeds."""
    if backend not in _STATES:
        import torch
        a, p = actions_of(backend, K)
        got = []
        for seed, acts in ((SEED + 1, a), (SEED + 2, p)):
            env = BACKENDS[backend]()
            so.reset(env, seed)
            env.rollout(_dev(acts))
            got.append([x.cpu().numpy() for x in env.get_state()])
            torch.cuda.synchronize()
            env.close()
        _STATES[backend] = got
    return _STATES[backend]


def _state_inputs(backend):
    t, p = states_of(backend)
    return ({f"s{i}": x for i, x in enumerate(t)}, {f"s{i}": x for i, x in enumerate(p)})


def call_set_state(env, b):
    env._set_state_raw([b[f"s{i}"] for i in range(len(b))])
    return {"state": tuple(env.get_state())}


@pytest.mark.parametrize("backend", STATE_BACKENDS)
def test_late_state(backend, gpu_device):
    t, p = _state_inputs(backend)
    so.run_case(f"{backend}/set_state", BACKENDS[backend], SEED, call_set_state, t, p)


@pytest.mark.parametrize("backend", STATE_BACKENDS)
def test_late_state_then_rollout(backend, gpu_device):
    """The launch after a late set_state starts from the state the copy brought, not from the one before it."""
    t, p = _state_inputs(backend)
    a, _ = actions_of(backend, K)

    def call(env, b):
        env._set_state_raw([b[f"s{i}"] for i in range(len(b) - 1)])
        return call_rollout(env, b)
    so.run_case(f"{backend}/set_state+rollout", BACKENDS[backend], SEED, call, dict(t, a=a), dict(p, a=a))


def test_taxi_render_after_late_state(gpu_device):
    """gp_taxi_render is asynchronous, gp_resize_area_u8 synchronises the stream (its coefficient buffers are freed on
    return): render() waits, and shows the late state."""
    t, p = _state_inputs("taxi_philox")

    def call(env, b):
        env._set_state_raw([b[f"s{i}"] for i in range(len(b))])
        return {"frame": env.render(idx=np.arange(4))}
    so.run_case("taxi_philox/render", mk_taxi_philox, SEED, call, t, p, expect_async=False)


# ------------------------------------------------------------------ controllers ----
def random_probs(M, n_obs, A, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, A - 1, M - 1] += 0.05
    return p / p.sum((-1, -2), keepdims=True)


def mk_crooms_ctrl():
    from gym_po_amd import CRoomsEnv
    return CRoomsEnv(1027, obs_type="hansen", action_type="cardinal", time_limit=5, rng_mode="philox")


def mk_heavenhell_hansen():
    from gym_po_amd import HeavenHellGridEnv  # 48 obs values: the statistics tables of 3 nodes fit the LDS budget
    return HeavenHellGridEnv(1027, obs_type="hansen_signal", action_failure_probability=0.25, time_limit=5)


def mk_taxi_ctrl():
    return _taxi(1027, "philox")


CTRL_BACKENDS = {"rooms_philox": mk_rooms_philox, "rocksample": mk_rocksample, "anttag_index": mk_anttag_index,
                 "taxi_philox": mk_taxi_ctrl, "heavenhell": mk_heavenhell, "pomdp_tiger": mk_pomdp_tiger,
                 "pomdp_m37": mk_pomdp_m37, "crooms_hansen": mk_crooms_ctrl, "heavenhell_hansen": mk_heavenhell_hansen}
M_NODES = 3


def install(env, seed=5):
    n_obs, A = int(env._controller_n_obs()), int(env.single_action_space.n)
    env.set_controller(probs=random_probs(M_NODES, n_obs, A, seed))


def _nodes(B, M=M_NODES):
    t = np.random.default_rng(13).integers(0, M, B).astype(np.uint8)
    return {"nodes": t}, {"nodes": ((t + 1) % M).astype(np.uint8)}


def call_nodes_rollout(env, b):
    env.controller_nodes = b["nodes"]
    back = env.controller_nodes  # the read-back is queued behind the late copy too
    return dict(env.rollout_controller(K), nodes_back=back)


@pytest.mark.parametrize("backend", sorted(CTRL_BACKENDS))
def test_late_controller_nodes(backend, gpu_device):
    make = CTRL_BACKENDS[backend]
    t, p = _nodes(1027)
    so.run_case(f"{backend}/controller_nodes+rollout_controller", make, SEED, call_nodes_rollout, t, p, setup=install)


def mk_fourrooms_population():
    from gym_po_amd import MultistoryFourRoomsEnv
    return MultistoryFourRoomsEnv(2048 + 1024 - 5, grid_z=1, obs_type="hansen", time_limit=5, rng_mode="philox")


def install_population(env):
    n_obs, A = int(env._controller_n_obs()), int(env.single_action_space.n)
    env.set_controller_population(probs=np.stack([random_probs(M_NODES, n_obs, A, 20 + i) for i in range(3)]),
                                  group_envs=1024, gamma=0.875)
    assert env.query("controller_population") == 3


def test_late_controller_nodes_population(gpu_device):
    t, p = _nodes(2048 + 1024 - 5)

    def call(env, b):
        out = call_nodes_rollout(env, b)
        out["scores"] = env.controller_scores()  # waits for the stream
        return out
    so.run_case("fourrooms_population/rollout_controller", mk_fourrooms_population, SEED, call, t, p,
                setup=install_population, expect_async=False)


_PLANES = {}


def planes_of(backend, seed):
    """The planes a closed-loop rollout wrote (host arrays), with obs0 and the final nodes."""
    if (backend, seed) not in _PLANES:
        import torch
        env = CTRL_BACKENDS[backend]()
        obs0 = so.reset(env, seed)
        install(env)
        out = env.rollout_controller(K)
        d = {k: v.cpu().numpy().view(np.uint8) if v.dtype == torch.bool else v.cpu().numpy() for k, v in out.items()}
        d["obs0"], d["next_nodes"] = obs0.cpu().numpy().astype(np.int32), env.controller_nodes.cpu().numpy()
        d["obs"] = d["obs"].astype(np.int32)
        torch.cuda.synchronize()
        env.close()
        _PLANES[(backend, seed)] = d
    return _PLANES[(backend, seed)]


@pytest.mark.parametrize("lds_max,path", [(-1, 1), (0, 0)], ids=["lds", "global"])
@pytest.mark.parametrize("backend", ["heavenhell_hansen", "pomdp_tiger"])
def test_controller_stats_late_planes(backend, lds_max, path, gpu_device):
    t, p = planes_of(backend, SEED), planes_of(backend, SEED + 1)

    def call(env, b):
        with _knobs(stats_lds_max=lds_max):
            planes = {k: b[k] for k in ("obs", "actions", "nodes", "rew", "term", "trunc")}
            out = env.controller_statistics(planes, b["obs0"], next_nodes=b["next_nodes"], gamma=0.875)
        assert env.query("stats_lds") == path
        return out
    so.run_case(f"{backend}/controller_stats/{'lds' if path else 'global'}", CTRL_BACKENDS[backend], SEED, call, t, p,
                setup=install)


# ------------------------------------------------------------------ beliefs ----
def raw_belief_set(env, t):
    """gp_belief_set without the wrapper's host-side validation (which reads the tensor, so waits for it)."""
    from gym_po_amd import _lib
    _lib.check(_lib.lib().gp_belief_set(env._handle, ctypes.c_void_p(t.data_ptr()), env._stream()), "gp_belief_set")


def _beliefs(model, B=1027):
    S = {"tiger": 2, "m37": 37}[model]
    rng = np.random.default_rng(17)
    t = rng.random((B, S)).astype(np.float32) + np.float32(0.01)
    p = rng.random((B, S)).astype(np.float32) + np.float32(0.01)
    return t / t.sum(-1, keepdims=True), p / p.sum(-1, keepdims=True)


def enable_belief(env):
    env.enable_belief()
    assert env.query("belief") == 1


def enable_belief_policy(env):
    enable_belief(env)
    rng = np.random.default_rng(19)
    N = 5
    env.set_belief_policy(rng.normal(size=(N, env.n_states)).astype(np.float32), rng.integers(0, env.n_actions, N))


_OPEN = {}


def open_planes(model, seed):
    """actions / obs / term / trunc planes of an open-loop rollout (host arrays)."""
    if (model, seed) not in _OPEN:
        import torch
        env = _pomdp(model)
        so.reset(env, seed)
        a = np.random.default_rng(seed).integers(0, env.n_actions, (K, env.num_envs)).astype(np.int32)
        o, _, tm, tr = env.rollout(_dev(a))
        _OPEN[(model, seed)] = {"actions": a, "obs": o.cpu().numpy().astype(np.int32),
                                "term": tm.cpu().numpy().view(np.uint8), "trunc": tr.cpu().numpy().view(np.uint8)}
        torch.cuda.synchronize()
        env.close()
    return _OPEN[(model, seed)]


@pytest.mark.parametrize("model", ["tiger", "m37"])
def test_late_belief_and_filter_planes(model, gpu_device):
    bt, bp = _beliefs(model)
    t, p = dict(open_planes(model, SEED), belief=bt), dict(open_planes(model, SEED + 1), belief=bp)

    def call(env, b):
        raw_belief_set(env, b["belief"])
        back = env.belief
        env.belief_filter(b["actions"], b["obs"], b["term"], b["trunc"])
        return {"belief_back": back, "belief": env.belief}
    so.run_case(f"pomdp_{model}/belief_set+belief_filter", lambda: _pomdp(model), SEED, call, t, p, setup=enable_belief)


@pytest.mark.parametrize("model", ["tiger", "m37"])
def test_rollout_belief_from_late_belief(model, gpu_device):
    bt, bp = _beliefs(model)

    def call(env, b):
        raw_belief_set(env, b["belief"])
        return env.rollout_belief(K)
    so.run_case(f"pomdp_{model}/rollout_belief", lambda: _pomdp(model), SEED, call, {"belief": bt}, {"belief": bp},
                setup=enable_belief_policy)


def test_set_belief_wrapper_waits_for_the_stream(gpu_device):
    """set_belief() validates its tensor on the host and synchronises the stream: it waits, and stores the late values."""
    bt, bp = _beliefs("tiger")

    def call(env, b):
        env.set_belief(b["belief"])
        return {"belief": env.belief}
    so.run_case("pomdp_tiger/set_belief wrapper", mk_pomdp_tiger, SEED, call, {"belief": bt}, {"belief": bp},
                setup=enable_belief, expect_async=False)


def _points(P, S=2, seed=23):
    rng = np.random.default_rng(seed)
    t = rng.random((P, S)).astype(np.float32) + np.float32(0.01)
    return t, t[:, ::-1].copy() * np.float32(0.5)


ALPHA = np.array([[1.0, -2.0], [-3.0, 0.5], [0.25, 0.25]], dtype=np.float32)


def test_point_backup_late_points(gpu_device):
    """gp_belief_backup waits for the stream's earlier work (documented), and the wrapper validates the points on the
    host: the call blocks, and computes from the late points."""
    t, p = _points(64)
    so.run_case("pomdp_tiger/point_backup", mk_pomdp_tiger, SEED, lambda env, b: env.point_backup(b["pts"], ALPHA),
                {"pts": t}, {"pts": p}, setup=enable_belief, expect_async=False)


def test_point_backup_grows_its_scratch_under_queued_work(gpu_device):
    t, p = _points(512)

    def call(env, b):
        first = env.point_backup(b["pts"][:8], ALPHA)   # queued behind the delay; scratch for 8 points
        n0 = env.query("backup_scratch_bytes")
        second = env.point_backup(b["pts"], ALPHA)      # reallocates the scratch the first call's kernels used
        assert env.query("backup_scratch_bytes") > n0
        return {"first": first, "second": second}
    so.run_case("pomdp_tiger/point_backup grows", mk_pomdp_tiger, SEED, call, {"pts": t}, {"pts": p},
                setup=enable_belief, expect_async=False)


# ------------------------------------------------------------------ host-synchronous calls ----
@pytest.mark.parametrize("backend", ["heavenhell", "fourrooms_wgrid", "crooms_numpy_grid"])
def test_metrics_and_check_wait_for_the_stream(backend, gpu_device):
    a, p = actions_of(backend, K)

    def call(env, b):
        out = call_rollout(env, b)
        m = env.metrics()
        env.check()
        return dict(out, metrics=m)
    so.run_case(f"{backend}/metrics+check", BACKENDS[backend], SEED, call, {"a": a}, {"a": p}, expect_async=False)


@pytest.mark.parametrize("backend", ["fourrooms_fused", "fourrooms_wgrid", "taxi_numpy_wg", "taxi_numpy_grid",
                                     "crooms_numpy_wg", "crooms_numpy_grid"])
def test_rng_state_waits_for_the_stream(backend, gpu_device):
    a, p = actions_of(backend, K)

    def call(env, b):
        out = call_rollout(env, b)
        st = env.rng_state
        gen = env.np_random
        return dict(out, rng_state=st, next_word=int(gen.bit_generator.random_raw()))
    so.run_case(f"{backend}/rng_state", BACKENDS[backend], SEED, call, {"a": a}, {"a": p}, expect_async=False)


def test_controller_scores_clear_then_rollout(gpu_device):
    t, p = _nodes(2048 + 1024 - 5)

    def call(env, b):
        first = call_nodes_rollout(env, b)
        s1 = env.controller_scores(clear=True)   # waits, reads, zeroes the slots
        second = env.rollout_controller(K)       # adds into the zeroed slots, on the stream
        return {"first": first, "s1": s1, "second": second, "s2": env.controller_scores()}
    so.run_case("fourrooms_population/controller_scores(clear)", mk_fourrooms_population, SEED, call, t, p,
                setup=install_population, expect_async=False)


@pytest.mark.parametrize("backend", ["heavenhell", "fourrooms_wgrid", "taxi_numpy_grid"])
def test_seed_after_queued_work(backend, gpu_device):
    a, p = actions_of(backend, K)

    def call(env, b):
        first = call_rollout(env, b)
        env.seed(99)
        return {"first": first, "second": call_rollout(env, b)}
    so.run_case(f"{backend}/seed", BACKENDS[backend], SEED, call, {"a": a}, {"a": p}, expect_async=False)


@pytest.mark.parametrize("backend", ["heavenhell", "rooms_philox", "taxi_philox"])
def test_set_controller_replaces_a_table_a_queued_launch_reads(backend, gpu_device):
    t, p = _nodes(1027)

    def call(env, b):
        first = call_nodes_rollout(env, b)
        install(env, seed=6)  # frees / overwrites the table: it has to wait for the queued launch
        return {"first": first, "second": env.rollout_controller(K)}
    so.run_case(f"{backend}/set_controller", CTRL_BACKENDS[backend], SEED, call, t, p, setup=install, expect_async=False)


def test_belief_disable_and_enable_after_queued_work(gpu_device):
    bt, bp = _beliefs("tiger")

    def call(env, b):
        raw_belief_set(env, b["belief"])
        first = env.rollout_belief(K)  # reads and writes the belief planes that disable frees
        env.disable_belief()
        env.enable_belief()            # every belief from the prior and the stored obs of the state after the rollout
        return {"first": first, "belief": env.belief}
    so.run_case("pomdp_tiger/belief_disable+enable", mk_pomdp_tiger, SEED, call, {"belief": bt}, {"belief": bp},
                setup=enable_belief_policy, expect_async=False)


@pytest.mark.parametrize("backend", ["heavenhell", "taxi_numpy_wg", "crooms_philox"])
def test_set_state_wrapper_waits_for_the_stream(backend, gpu_device):
    """The Python set_state() wrappers upload host arrays and synchronise the current stream before they return."""
    a, p = actions_of(backend, K)
    state = states_of(backend)[0]

    def call(env, b):
        first = call_rollout(env, b)
        env.set_state(*state)
        return {"first": first, "state": tuple(env.get_state())}
    so.run_case(f"{backend}/set_state wrapper", BACKENDS[backend], SEED, call, {"a": a}, {"a": p}, expect_async=False)


@pytest.mark.parametrize("backend", ["heavenhell", "fourrooms_wgrid", "fourrooms_fused", "taxi_numpy_grid",
                                     "crooms_numpy_grid", "pomdp_tiger"])
def test_reset_between_queued_rollouts(backend, gpu_device):
    """reset() without a seed is a launch like any other: rollout, reset, rollout queued behind one delay."""
    a, p = actions_of(backend, K)

    def call(env, b):
        first = call_rollout(env, b)
        obs = so.reset(env, None)
        return {"first": first, "reset_obs": obs, "second": call_rollout(env, b)}
    so.run_case(f"{backend}/reset", BACKENDS[backend], SEED, call, {"a": a}, {"a": p})


# ------------------------------------------------------------------ rollout_plan binding, hand-over ----
@pytest.mark.parametrize("backend", ["heavenhell", "fourrooms_wgrid", "crooms_numpy_graph"])
def test_plan_runs_on_the_stream_of_plan_time(backend, gpu_device):
    """A plan made under `s` and run while the null stream is current still orders after s's delay and late actions."""
    import torch
    a, p = actions_of(backend, K)

    def call(env, b):
        run, outs = env.rollout_plan(b["a"])
        with torch.cuda.stream(torch.cuda.default_stream()):
            run()
        return _named(outs)
    so.run_case(f"{backend}/plan bound to s", BACKENDS[backend], SEED, call, {"a": a}, {"a": p},
                ref_key=f"{backend}/rollout", ref_call=call_rollout)


@pytest.mark.parametrize("backend", ["heavenhell", "fourrooms_wgrid"])
def test_plan_run_with_an_explicit_stream(backend, gpu_device):
    """run(stream=t.cuda_stream) orders after t, whatever stream the plan was bound to and whichever is current."""
    import torch
    a, p = actions_of(backend, K)

    def call(env, b):
        t = torch.cuda.current_stream()  # the stream that carries the delay and the late copy
        with torch.cuda.stream(torch.cuda.Stream()):
            run, outs = env.rollout_plan(b["a"])  # bound to an idle third stream
        with torch.cuda.stream(torch.cuda.default_stream()):
            run(stream=t.cuda_stream)
        return _named(outs)
    so.run_case(f"{backend}/run(stream=t)", BACKENDS[backend], SEED, call, {"a": a}, {"a": p},
                ref_key=f"{backend}/rollout", ref_call=call_rollout)


@pytest.mark.parametrize("backend", ["heavenhell", "fourrooms_wgrid", "taxi_numpy_grid", "crooms_numpy_grid",
                                     "pomdp_m37"])
def test_hand_over_between_streams(backend, gpu_device):
    """Half the steps on s1 (behind its delay), s2.wait_stream(s1), the other half on s2: equal to one stream."""
    import torch
    a, p = actions_of(backend, 2 * K)

    def call(env, b):
        s1, s2 = torch.cuda.current_stream(), torch.cuda.Stream()
        o1 = env.rollout(b["a"][:K])
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            o2 = env.rollout(b["a"][K:])
        s1.wait_stream(s2)  # the runner clones the outputs and reads the env on s1
        return _named([torch.cat((x, y)) for x, y in zip(o1, o2)])
    so.run_case(f"{backend}/hand-over", BACKENDS[backend], SEED, call, {"a": a}, {"a": p},
                ref_key=f"{backend}/rollout2K", ref_call=call_rollout)


# ------------------------------------------------------------------ positive control ----
def test_positive_control_launch_on_another_stream_reads_the_poison(gpu_device):
    """The pattern detects a launch on the wrong stream: the late producer is queued on `s`, the step is issued on a
    second side stream `t` (step_raw's stream argument). It runs at once, while s is still in its delay, and computes
    from the poison. Heaven-Hell's kernels have no cross-block wait; both action sets are valid."""
    import torch
    a, p = actions_of("heavenhell", 1)
    poison = so.null_run(mk_heavenhell, SEED, call_step, {"a": p})
    ref = so.null_run(mk_heavenhell, SEED, call_step, {"a": a})
    assert so.differing(ref["outs"], poison["outs"])
    s, t = torch.cuda.Stream(), torch.cuda.Stream()
    env = None
    try:
        with torch.cuda.stream(s):
            env = mk_heavenhell()
            so.reset(env, SEED)
            buf, src = _dev(p).clone(), _dev(a)
            obs, rew, term, trunc = env._alloc_outputs()
            torch.cuda.synchronize()
            ev = so.delay(s)
            so.late(buf, src)
            env.step_raw(buf[0], obs, rew, term, trunc, stream=t.cuda_stream)
            t.synchronize()
            assert not ev.query(), "the delay on s ended before the step on t did: nothing is shown"
            got = so.raw(_named((obs, rew, term, trunc)))
        torch.cuda.synchronize()
        assert not so.differing(got, poison["outs"]), "the step on t did not read the poison"
        assert so.differing(got, ref["outs"])
    finally:
        torch.cuda.synchronize()
        if env is not None:
            env.close()
