"""GPU tests of the closed-loop rollouts on grid Ant-Tag (index obs, philox mode): a K-step launch whose actions the
device draws from a tabular finite-state controller must equal the open-loop rollout() of those actions on a twin env
bit for bit (outputs, final state, metrics), and the actions and nodes it emits must equal the numpy restatement of the
controller (tests/controller_oracle.py, which is not env-specific) run over the obs stream it emitted.

A = 5 is no multiple of 4, so the library pads each uploaded row to 16-B quads with 2^31. On the 4 x 4 arena M = 1, 2, 3
give rows of 5 -> 8, 10 -> 12 and 15 -> 16 entries (the scanned path: up to 4 quads); on the 6 x 6 arena M = 4 and 8
give 20 and 40 entries (5 and 10 quads: the searched path). The 16 x 16 arena with M = 1 has a table of 65,792 rows
(2.1 MB). Every row puts nonzero probability on the last real joint choice: a padding entry that was counted would show
as action 5. B = 2051 envs = three 1,024-env tiles, the last one ragged; K = 48 steps under time_limit = 20 end at least
two episodes in every env."""
import numpy as np
import pytest

from controller_oracle import controller_rollout
from gym_po_amd.controller import controller_thresholds
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

B, K, SEED, TL = 2051, 48, 11, 20
A = 5
# name -> (size, min_distance, controller nodes)
CASES = {
    "s4_m1": (4, 2.0, 1),
    "s4_m2": (4, 2.0, 2),
    "s4_m3": (4, 2.0, 3),
    "s6_m4": (6, 3.0, 4),
    "s6_m8": (6, 3.0, 8),
    "s16_m1": (16, 5.0, 1),
}


def make_env(name, num_envs=B, **kw):
    from gym_po_amd import AntTagGridEnv
    size, min_distance, _ = CASES[name]
    kw = {"obs_type": "index", **kw}
    return AntTagGridEnv(num_envs, size=size, min_distance=min_distance, time_limit=TL, tag_reward=2.0,
                         step_reward=-0.25, **kw)


def random_probs(M, n_obs, A, seed):
    """Rows in which about a third of the entries are exactly 0 and the last joint choice never is."""
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, A - 1, M - 1] += 0.05
    return p / p.sum((-1, -2), keepdims=True)


def reset_obs(env, seed=SEED):
    return env.reset(seed=seed)[0].cpu().numpy()


def host(x):
    return x.cpu().numpy()


class Run:
    """One case, run once and shared (left unchanged) by the tests that read it."""

    def __init__(self, name):
        self.name, self.M = name, CASES[name][2]
        e1 = make_env(name)
        self.size = e1.size
        self.n_obs = int(e1.single_observation_space.n)
        assert int(e1.single_action_space.n) == A and self.n_obs == self.size ** 2 * (self.size ** 2 + 1)
        self.thr = controller_thresholds(random_probs(self.M, self.n_obs, A, seed=5))
        e1.set_controller(thresholds=self.thr)
        assert e1.query("controller_lds") == 0 and e1.query("controller_nodes") == self.M
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
        e = make_env(self.name)
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


@pytest.fixture(params=["s4_m3", "s6_m8"])  # a scanned and a searched row
def run_split(request, gpu_device):
    return get_run(request.param)


def test_closed_loop_equals_open_loop(run):
    import torch
    assert run.thr.shape == (run.M, run.n_obs, A * run.M)
    assert run.out["obs"].shape == (K, B) and run.out["obs"].dtype == np.int32
    assert run.out["actions"].dtype == np.int32 and run.out["nodes"].dtype == np.uint8
    assert run.step1 == run.step0 + K  # the counter advanced by K
    assert (run.out["term"] | run.out["trunc"]).sum(0).min() >= 2
    assert run.out["trunc"].any()
    if run.size < 16:  # (on the 16 x 16 arena the pairs start more than 5 cells apart: no random walk of 20 steps tags)
        assert run.out["term"].any()
    for obs_type in ("index", "vector"):  # the open loop of the emitted actions, on either obs kind
        e2 = make_env(run.name, obs_type=obs_type)
        obs0 = reset_obs(e2)
        obs, rew, term, trunc = e2.rollout(run.actions_dev)
        if obs_type == "index":
            assert np.array_equal(obs0, run.obs0)
            assert torch.equal(obs.cpu(), torch.from_numpy(run.out["obs"]))
        else:
            from gym_po_amd import ant_tag_obs_index
            assert np.array_equal(ant_tag_obs_index(host(obs), run.size), run.out["obs"])
        for name, t in (("rew", rew), ("term", term), ("trunc", trunc)):
            assert torch.equal(t.cpu(), torch.from_numpy(run.out[name])), name
        for a, b in zip(e2.get_state(), run.state):
            assert np.array_equal(host(a), b)
        assert e2.metrics() == run.metrics
        assert e2.query("philox_step") == run.step1
        e2.check()
    assert run.metrics["env_steps"] == K * B and run.metrics["episodes"] >= 2 * B


def test_actions_and_nodes_equal_the_oracle(run):
    t = run.thr.astype(np.int64)
    assert (np.diff(t, axis=-1, prepend=0) == 0).any()  # choices of probability exactly 0: empty intervals
    acts, nodes, final = controller_rollout(run.obs0, run.out["obs"], run.out["term"], run.out["trunc"], run.thr,
                                            philox_key(SEED), run.step0)
    assert np.array_equal(run.out["actions"], acts)
    assert np.array_equal(run.out["nodes"], nodes)
    assert np.array_equal(run.final_nodes, final)
    # the last real action is drawn; nothing beyond it ever is (a counted padding entry would give 5 or more)
    assert run.out["actions"].min() >= 0 and run.out["actions"].max() == A - 1
    assert run.out["nodes"].max() < run.M
    nc = run.size ** 2
    hidden = run.out["obs"] % (nc + 1) == nc
    assert hidden.any() and (~hidden).any() and run.out["obs"].max() < run.n_obs  # both obs branches conditioned on
    if run.M > 1:
        ended = run.out["term"][:-1] | run.out["trunc"][:-1]
        assert ended.any() and not run.out["nodes"][1:][ended].any()  # node 0 after every episode end
        assert run.out["nodes"].any()


def test_split_launches_equal_one_launch(run_split):
    run = run_split
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
    assert e.metrics() == run.metrics


def test_open_loop_steps_then_closed_loop(run_split):
    """17 explicit-action steps, then 31 closed-loop ones: the obs comes from the state, whoever stepped it."""
    import torch
    run = run_split
    e = run.twin()
    first = e.rollout(run.actions_dev[:17])
    assert torch.equal(first[0].cpu(), torch.from_numpy(run.out["obs"][:17]))
    assert not host(e.controller_nodes).any()  # rollout() leaves the nodes alone
    e.controller_nodes = run.out["nodes"][17]
    b = {k: host(v) for k, v in e.rollout_controller(31).items()}
    for name in ("obs", "actions", "nodes", "rew", "term", "trunc"):
        assert np.array_equal(b[name], run.out[name][17:]), name
    assert e.metrics() == run.metrics


def test_optional_outputs(run_split):
    import torch
    run = run_split
    e = run.twin()
    assert e.rollout_controller(K, store=()) == {}
    assert e.metrics() == run.metrics
    for x, y in zip(e.get_state(), run.state):
        assert np.array_equal(host(x), y)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)
    for name in ("obs", "actions", "nodes", "rew", "term", "trunc"):  # every output alone
        e = run.twin()
        out = e.rollout_controller(K, store=(name,))
        assert sorted(out) == [name]
        assert np.array_equal(host(out[name]), run.out[name]), name
        assert e.metrics() == run.metrics
    e = run.twin()
    buf = torch.empty((K, B), dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(K, out={"nodes": buf}, store=("nodes", "rew"))
    assert out["nodes"].data_ptr() == buf.data_ptr()
    assert np.array_equal(host(buf), run.out["nodes"]) and np.array_equal(host(out["rew"]), run.out["rew"])


def test_deterministic_controller_and_chosen_start_nodes(gpu_device):
    M = 3
    e = make_env("s6_m4")
    n_obs = int(e.single_observation_space.n)
    p = np.zeros((M, n_obs, A, M))
    for n in range(M):
        p[n, :, A - 1, (n + 1) % M] = 1.0  # always the last action (stay); the node cycles 0 -> 1 -> 2 -> 0
    e.set_controller(probs=p)
    reset_obs(e)
    assert not host(e.controller_nodes).any()  # reset zeroes them
    start = (np.arange(B) * 7 % M).astype(np.uint8)
    e.controller_nodes = start
    assert np.array_equal(host(e.controller_nodes), start)
    out = {k: host(v) for k, v in e.rollout_controller(25).items()}
    assert (out["actions"] == A - 1).all()
    ended = out["term"] | out["trunc"]
    assert ended.any()
    want = start.astype(np.int64)
    for k in range(25):
        assert np.array_equal(out["nodes"][k], want), k
        want = np.where(ended[k], 0, (want + 1) % M)
    assert np.array_equal(host(e.controller_nodes), want)
    # explicit-action calls leave the nodes alone; reset zeroes them again, and so does set_controller
    before = host(e.controller_nodes)
    assert before.any()
    e.step(np.zeros(B, dtype=np.int64))
    assert np.array_equal(host(e.controller_nodes), before)
    reset_obs(e)
    assert not host(e.controller_nodes).any()
    e.controller_nodes = start
    e.set_controller(probs=p)
    assert not host(e.controller_nodes).any()
    with pytest.raises(ValueError):
        e.controller_nodes = np.full(B, M)
    e.check()


def test_undersized_table_is_clamped_and_flagged(gpu_device):
    """The C ABI takes any n_obs: an obs beyond the table is clamped on the device and flags the handle."""
    import ctypes

    from gym_po_amd import _lib
    from gym_po_amd._lib import GymPoError
    e = make_env("s4_m1", num_envs=300)
    t = controller_thresholds(np.full((2, A), 1.0 / A))  # n_obs = 2: nearly every obs lies beyond it
    _lib.check(_lib.lib().gp_set_controller(e._handle, 1, 2, ctypes.c_void_p(t.ctypes.data)), "gp_set_controller")
    reset_obs(e)
    out = e.rollout_controller(8)
    assert 0 <= int(out["actions"].min()) and int(out["actions"].max()) < A
    with pytest.raises(GymPoError):
        e.check()


def test_node_beyond_the_controller_is_clamped_and_flagged(gpu_device):
    """A node >= M written from a device tensor (not range-checked on the host) is clamped and flags the handle."""
    import torch
    from gym_po_amd._lib import GymPoError
    e = make_env("s4_m2", num_envs=300)
    e.set_controller(probs=np.full((2, int(e.single_observation_space.n), A, 2), 0.1))
    reset_obs(e)
    e.controller_nodes = torch.full((300,), 2, dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(4)
    assert int(out["nodes"].max()) < 2 and int(out["actions"].max()) < A
    with pytest.raises(GymPoError):
        e.check()


def test_errors(gpu_device):
    from gym_po_amd._lib import GymPoError
    e = make_env("s4_m1", num_envs=64)
    n_obs = int(e.single_observation_space.n)
    uniform = np.full((n_obs, A), 1.0 / A)
    reset_obs(e)
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(4)
    with pytest.raises(GymPoError, match="without a controller"):
        e.controller_nodes
    e.set_controller(probs=np.full((8, n_obs, A, 8), 1.0 / (8 * A)))  # M = 8, the most: A * M = 40
    out = e.rollout_controller(4)
    assert int(out["actions"].max()) < A
    e.set_controller()  # removed again
    with pytest.raises(GymPoError):
        e.rollout_controller(4)
    with pytest.raises(GymPoError):
        e.set_controller(probs=np.full((n_obs + 1, A), 1.0 / A))  # wrong n_obs
    with pytest.raises(GymPoError):
        e.set_controller(probs=np.full((n_obs, A + 1), 1.0 / (A + 1)))  # wrong action count
    bad = controller_thresholds(uniform)
    bad[0, 7, 1], bad[0, 7, 2] = bad[0, 7, 2], bad[0, 7, 1]  # a non-monotone row
    with pytest.raises(GymPoError, match="not nondecreasing"):
        e.set_controller(thresholds=bad)
    bad = controller_thresholds(uniform)
    bad[0, 3, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError, match="not 2\\^31"):
        e.set_controller(thresholds=bad)
    e2 = make_env("s4_m1", num_envs=64)
    e2.set_controller(probs=uniform)
    with pytest.raises(GymPoError, match="before reset"):
        e2.rollout_controller(4)
    # a vector-obs handle and a replay handle take no controller, from any of the three entry points
    vec = make_env("s4_m1", num_envs=64, obs_type="vector")
    rep = make_env("s4_m1", num_envs=64, rng_mode="replay")
    thr = controller_thresholds(uniform)
    for env in (vec, rep):
        with pytest.raises(GymPoError, match=r"\(-3\)"):
            env.set_controller(thresholds=thr)
        with pytest.raises(GymPoError, match=r"\(-3\)"):
            env.rollout_controller(4)
        with pytest.raises(GymPoError, match=r"\(-3\)"):
            env.controller_nodes
    reset_obs(vec)
    vec.check()
