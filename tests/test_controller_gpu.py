"""GPU tests of the closed-loop rollouts (set_controller / rollout_controller / controller_nodes): a K-step launch
whose actions the device draws from a tabular finite-state controller must equal the open-loop rollout() of those
same actions on a twin env bit for bit, and the actions and nodes it emits must equal the numpy restatement of the
controller (tests/controller_oracle.py) run over the obs stream it emitted.

Shapes: B = 2051 envs = three 1024-env blocks, the last one ragged, with a thread that owns 3 live envs of its 4;
K = 48 steps under time_limit = 20 end at least two episodes in every env (truncations and the node reset to 0
included).
Rows of up to 16 thresholds are scanned whole (FourRooms: 12 and 16 entries, the table obs: 8), longer rows
searched by quads: ROOMS Hansen-8 has 8 actions, so M = 4, 5, 8 give rows of 8, 10 and 16 quads. Small tables
(FourRooms Hansen-4 with M = 1, 2) are staged in LDS, the others read from global memory; the knob `ctrl_lds_max`
sends a small table down the global-memory path too."""
import numpy as np
import pytest

from controller_oracle import controller_rollout
from fixtures import load_index
from gym_po_amd.controller import controller_thresholds
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

B, K, SEED = 2051, 48, 11
INDEX = load_index()["cases"]

# name -> (fixture config, kwargs on top of it, controller nodes)
CASES = {
    "fr_hansen4_m1": ("fr_hansen_tl20", {}, 1),                                    # 6.5 KB table: staged in LDS
    "fr_hansen4_m2": ("fr_hansen_tl20", {}, 2),                                    # 26 KB table: staged in LDS
    "fr_hansen4_m3": ("fr_hansen_tl20", {}, 3),                                    # 58 KB: read from global memory
    "fr_hansen8_ordinal_m2": ("fr_hansen8_ordinal", dict(time_limit=20), 2),
    "rooms_table_randgoal_m1": ("rooms_2_goal_mdp_randgoal", {}, 1),
    "rooms_hansen8_m4": ("rooms_4_hansen8", dict(time_limit=20), 4),               # the large-table path
    "rooms_hansen8_m5": ("rooms_4_hansen8", dict(time_limit=20), 5),               # rows of 10 quads
    "rooms_hansen8_m8": ("rooms_4_hansen8", dict(time_limit=20), 8),               # rows of 16 quads
}


def make_env(config, extra=None, num_envs=B, rng_mode="philox"):
    from gym_po_amd import MultistoryFourRoomsEnv, RoomsEnv
    meta = INDEX[config]
    kw = dict(meta["kwargs"])
    kw.update(extra or {})
    if meta["kind"] == "fourrooms":
        if kw.get("goal_xyz") is not None:
            kw["goal_xyz"] = tuple(kw["goal_xyz"])
        return MultistoryFourRoomsEnv(num_envs, **kw, rng_mode=rng_mode)
    return RoomsEnv(num_envs, **kw, rng_mode=rng_mode)


def random_probs(M, n_obs, A, seed):
    """Dirichlet-like rows (gamma-ish weights, normalised) in which about a third of the entries are exactly 0."""
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, rng.integers(A), rng.integers(M)] += 1e-2  # no all-zero row
    return p / p.sum((-1, -2), keepdims=True)


def reset_obs(env, seed=SEED):
    r = env.reset(seed=seed)
    return (r[0] if isinstance(r, tuple) else r).cpu().numpy()


def host(x):
    return x.cpu().numpy()


class Run:
    """One case, run once and shared (left unchanged) by the tests that read it."""

    def __init__(self, name):
        config, extra, M = CASES[name]
        self.config, self.extra, self.M = config, extra, M
        e1 = make_env(config, extra)
        self.n_obs, self.A = int(e1.single_observation_space.n), int(e1.single_action_space.n)
        self.thr = controller_thresholds(random_probs(M, self.n_obs, self.A, seed=5))
        e1.set_controller(thresholds=self.thr)
        self.staged = e1.query("controller_lds")
        self.obs0 = reset_obs(e1)
        self.step0 = e1.query("philox_step")
        out = e1.rollout_controller(K)
        self.out = {k: host(v) for k, v in out.items()}
        self.state = [host(x) for x in e1.get_state()]
        self.metrics = e1.metrics()
        self.final_nodes = host(e1.controller_nodes)
        self.step1 = e1.query("philox_step")
        self.actions_dev = out["actions"]

    def twin(self):
        e = make_env(self.config, self.extra)
        e.set_controller(thresholds=self.thr)
        assert np.array_equal(reset_obs(e), self.obs0)
        return e


_RUNS = {}


def get_run(name):
    if name not in _RUNS:
        _RUNS[name] = Run(name)
    return _RUNS[name]


@pytest.fixture(params=sorted(CASES))
def run(request, gpu_device):
    return get_run(request.param)


@pytest.fixture
def run_fr(gpu_device):
    return get_run("fr_hansen4_m3")


def test_closed_loop_equals_open_loop(run):
    import torch
    assert run.out["obs"].shape == (K, B) and run.out["actions"].dtype == np.int32
    assert run.out["nodes"].dtype == np.uint8
    assert run.step1 == run.step0 + K  # the counter advanced by K
    if run.config != "rooms_2_goal_mdp_randgoal":  # (its time_limit is 60; the others' 20: elapsed > 20 truncates)
        assert (run.out["term"] | run.out["trunc"]).sum(0).min() >= 2 and run.out["trunc"].any()
    e2 = make_env(run.config, run.extra)
    assert np.array_equal(reset_obs(e2), run.obs0)
    obs, rew, term, trunc = e2.rollout(run.actions_dev)
    for name, t in (("obs", obs), ("rew", rew), ("term", term), ("trunc", trunc)):
        assert torch.equal(t.cpu(), torch.from_numpy(run.out[name])), name
    for a, b in zip(e2.get_state(), run.state):
        assert np.array_equal(host(a), b)
    assert e2.metrics() == run.metrics
    assert run.metrics["env_steps"] == K * B


def test_actions_and_nodes_equal_the_oracle(run):
    assert (run.thr == 0).any()  # rows with exact zeros
    acts, nodes, final = controller_rollout(run.obs0, run.out["obs"], run.out["term"], run.out["trunc"], run.thr,
                                            philox_key(SEED), run.step0)
    assert np.array_equal(run.out["actions"], acts)
    assert np.array_equal(run.out["nodes"], nodes)
    assert np.array_equal(run.final_nodes, final)
    assert 0 <= run.out["actions"].min() and run.out["actions"].max() < run.A
    assert run.out["nodes"].max() < run.M
    if run.M > 1:
        ended = run.out["term"][:-1] | run.out["trunc"][:-1]
        assert ended.any() and not run.out["nodes"][1:][ended].any()  # node 0 after every episode end
        assert run.out["nodes"].any()


def test_table_in_lds_equals_table_in_global_memory(gpu_device):
    """Which path a table takes is a matter of its size; both give the same rollout."""
    from gym_po_amd._lib import debug_knobs
    staged = {name: get_run(name).staged for name in ("fr_hansen4_m1", "fr_hansen4_m2", "fr_hansen4_m3",
                                                      "rooms_hansen8_m4")}
    assert staged == {"fr_hansen4_m1": 1, "fr_hansen4_m2": 1, "fr_hansen4_m3": 0, "rooms_hansen8_m4": 0}
    for name in ("fr_hansen4_m1", "fr_hansen4_m2"):  # the same tables read from global memory
        run = get_run(name)
        e = make_env(run.config, run.extra)
        with debug_knobs(ctrl_lds_max=0):
            e.set_controller(thresholds=run.thr)
        assert e.query("controller_lds") == 0
        assert np.array_equal(reset_obs(e), run.obs0)
        out = e.rollout_controller(K)
        for k, v in out.items():
            assert np.array_equal(host(v), run.out[k]), (name, k)
        assert e.metrics() == run.metrics
        assert np.array_equal(host(e.controller_nodes), run.final_nodes)


def test_split_launches_equal_one_launch(run_fr):
    run = run_fr
    e = run.twin()
    a = {k: host(v) for k, v in e.rollout_controller(17).items()}
    _, _, nodes17 = controller_rollout(run.obs0, a["obs"], a["term"], a["trunc"], run.thr, philox_key(SEED), run.step0)
    assert np.array_equal(host(e.controller_nodes), nodes17)
    b = {k: host(v) for k, v in e.rollout_controller(31).items()}
    for name in ("obs", "actions", "nodes", "rew", "term", "trunc"):
        assert np.array_equal(np.concatenate((a[name], b[name])), run.out[name]), name
    for x, y in zip(e.get_state(), run.state):
        assert np.array_equal(host(x), y)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)


def test_optional_outputs(run_fr):
    run = run_fr
    e = run.twin()
    assert e.rollout_controller(K, store=()) == {}
    assert e.metrics() == run.metrics
    for x, y in zip(e.get_state(), run.state):
        assert np.array_equal(host(x), y)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)
    e = run.twin()
    out = e.rollout_controller(K, store=("actions",))
    assert sorted(out) == ["actions"]
    assert np.array_equal(host(out["actions"]), run.out["actions"])
    # caller buffers are used as given
    import torch
    e = run.twin()
    buf = torch.empty((K, B), dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(K, out={"nodes": buf}, store=("nodes", "rew"))
    assert out["nodes"].data_ptr() == buf.data_ptr()
    assert np.array_equal(host(buf), run.out["nodes"]) and np.array_equal(host(out["rew"]), run.out["rew"])
    with pytest.raises(ValueError):
        e.rollout_controller(K, out={"nodes": buf[:, :-1]}, store=("nodes",))


def test_deterministic_controller_and_chosen_start_nodes(gpu_device):
    M = 3
    e = make_env("fr_hansen_tl20")
    n_obs, A = int(e.single_observation_space.n), int(e.single_action_space.n)
    p = np.zeros((M, n_obs, A, M))
    for n in range(M):
        p[n, :, 2, (n + 1) % M] = 1.0  # always action 2; the node cycles 0 -> 1 -> 2 -> 0
    e.set_controller(probs=p)
    reset_obs(e)
    assert not host(e.controller_nodes).any()  # reset zeroes them
    start = (np.arange(B) * 7 % M).astype(np.uint8)
    e.controller_nodes = start
    out = {k: host(v) for k, v in e.rollout_controller(25).items()}
    assert (out["actions"] == 2).all()
    assert np.array_equal(out["nodes"][0], start)  # honoured at step 0
    ended = out["term"] | out["trunc"]
    want = start.astype(np.int64)
    for k in range(25):
        assert np.array_equal(out["nodes"][k], want), k
        want = np.where(ended[k], 0, (want + 1) % M)
    # explicit-action calls leave the nodes alone; reset zeroes them again
    before = host(e.controller_nodes)
    e.step(np.zeros(B, dtype=np.int64))
    assert np.array_equal(host(e.controller_nodes), before)
    reset_obs(e)
    assert not host(e.controller_nodes).any()
    with pytest.raises(ValueError):
        e.controller_nodes = np.full(B, M)
    e.check()


def test_errors(gpu_device):
    from gym_po_amd import RoomsEnv, TaxiVecEnv
    from gym_po_amd._lib import GymPoError
    e = make_env("fr_hansen_tl20", num_envs=64)
    n_obs, A = int(e.single_observation_space.n), int(e.single_action_space.n)
    uniform = np.full((n_obs, A), 1.0 / A)
    reset_obs(e)
    with pytest.raises(GymPoError):
        e.rollout_controller(4)  # before set_controller
    e.set_controller(probs=uniform)
    e.rollout_controller(4)
    e.set_controller()  # removed again
    with pytest.raises(GymPoError):
        e.rollout_controller(4)
    with pytest.raises(GymPoError):
        e.set_controller(probs=np.full((n_obs + 1, A), 1.0 / A))  # wrong n_obs
    with pytest.raises(GymPoError):
        e.set_controller(probs=np.full((n_obs, 2 * A), 0.5 / A))  # wrong action count
    bad = controller_thresholds(uniform)
    bad[0, 7, 1], bad[0, 7, 2] = bad[0, 7, 2], bad[0, 7, 1]  # a non-monotone row
    with pytest.raises(GymPoError):
        e.set_controller(thresholds=bad)
    bad = controller_thresholds(uniform)
    bad[0, 3, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError):
        e.set_controller(thresholds=bad)
    e2 = make_env("fr_hansen_tl20", num_envs=64)
    e2.set_controller(probs=uniform)
    with pytest.raises(GymPoError):
        e2.rollout_controller(4)  # before reset
    taxi = TaxiVecEnv(64, rng_mode="philox")
    with pytest.raises(GymPoError):
        taxi.set_controller(probs=np.full((int(taxi.single_observation_space.n), int(taxi.single_action_space.n)),
                                          1.0 / int(taxi.single_action_space.n)))
    with pytest.raises(GymPoError):
        taxi.rollout_controller(4)
    npy = make_env("fr_hansen_tl20", num_envs=64, rng_mode="numpy")
    with pytest.raises(GymPoError):
        npy.set_controller(probs=uniform)
    reset_obs(npy)
    with pytest.raises(GymPoError):
        npy.rollout_controller(4)
    vec = RoomsEnv(64, layout="1", obs_type="vector_hansen", rng_mode="philox")
    with pytest.raises(GymPoError):
        vec.set_controller(probs=np.full((16, 4), 0.25))
    reset_obs(vec)
    with pytest.raises(GymPoError):
        vec.rollout_controller(4)


def test_undersized_table_is_clamped_and_flagged(gpu_device):
    """The C ABI takes any n_obs: an obs beyond the table is clamped on the device and flags the handle."""
    import ctypes

    from gym_po_amd import _lib
    from gym_po_amd._lib import GymPoError
    e = make_env("fr_hansen_tl20", num_envs=300)
    A = int(e.single_action_space.n)
    t = controller_thresholds(np.full((2, A), 1.0 / A))  # n_obs = 2: nearly every obs lies beyond it
    _lib.check(_lib.lib().gp_set_controller(e._handle, 1, 2, ctypes.c_void_p(t.ctypes.data)), "gp_set_controller")
    reset_obs(e)
    out = e.rollout_controller(8)
    assert 0 <= int(out["actions"].min()) and int(out["actions"].max()) < A
    with pytest.raises(GymPoError):
        e.check()
