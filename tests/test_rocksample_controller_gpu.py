"""GPU tests of the closed-loop rollouts on RockSample: a K-step launch whose actions the device draws from a tabular
finite-state controller must equal the open-loop rollout() of those actions on a twin env bit for bit (outputs, final
state, metrics), and the actions and nodes it emits must equal the numpy restatement of the controller
(tests/controller_oracle.py, which is not grid-specific) run over the obs stream it emitted.

A = 5 + k actions is no multiple of 4 in general, so the library pads each uploaded row to 16-B quads with 2^31.
k = 3 (A = 8): M = 1, 2 give rows of 8 and 16 entries, no padding. k = 8 (A = 13): M = 1 gives 13 entries padded to 16
(the scanned path), M = 2 gives 26 padded to 28 and M = 4 gives 52 (13 quads; the searched paths). Every row puts
nonzero probability on the last real joint choice: a padding entry that was counted would show as an action >= A.
B = 2051 envs = three 1,024-env tiles, the last one ragged; K = 48 steps under time_limit = 20 end at least two
episodes in every env."""
import numpy as np
import pytest

from controller_oracle import controller_rollout
from gym_po_amd.controller import controller_thresholds
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

B, K, SEED, TL = 2051, 48, 11, 20
ROCKS_3 = ((0, 3), (2, 1), (3, 2))
ROCKS_8 = ((0, 0), (0, 6), (1, 3), (2, 2), (2, 5), (3, 0), (4, 4), (4, 6))
# name -> (map_size, rocks, init_pos, obs_type, controller nodes)
CASES = {
    "k3_m1_cell": ((4, 4), ROCKS_3, (1, 0), "cell_sensor", 1),
    "k3_m2_sensor": ((4, 4), ROCKS_3, (1, 0), "sensor", 2),
    "k8_m1_cell": ((7, 7), ROCKS_8, (3, 1), "cell_sensor", 1),
    "k8_m1_sensor": ((7, 7), ROCKS_8, (3, 1), "sensor", 1),
    "k8_m2_sensor": ((7, 7), ROCKS_8, (3, 1), "sensor", 2),
    "k8_m2_cell": ((7, 7), ROCKS_8, (3, 1), "cell_sensor", 2),
    "k8_m4_cell": ((7, 7), ROCKS_8, (3, 1), "cell_sensor", 4),
}


def make_env(name, num_envs=B):
    from gym_po_amd import RockSample
    map_size, rocks, init_pos, obs_type, _ = CASES[name]
    return RockSample(num_envs, map_size=map_size, rocks=rocks, init_pos=init_pos, obs_type=obs_type, time_limit=TL,
                      half_efficiency_distance=1.5, exit_reward=4.0, good_reward=2.0, bad_reward=-2.0,
                      empty_reward=-1.0, check_reward=-0.25, step_reward=-0.5, wall_reward=-0.75)


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
        self.name, self.M = name, CASES[name][4]
        e1 = make_env(name)
        self.n_obs, self.A = int(e1.single_observation_space.n), int(e1.single_action_space.n)
        self.thr = controller_thresholds(random_probs(self.M, self.n_obs, self.A, seed=5))
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


@pytest.fixture
def run_split(gpu_device):
    return get_run("k8_m2_sensor")  # the obs is the reading alone: it must survive between launches


def test_closed_loop_equals_open_loop(run):
    import torch
    assert run.thr.shape[-1] == run.A * run.M
    assert run.out["obs"].shape == (K, B) and run.out["actions"].dtype == np.int32
    assert run.out["nodes"].dtype == np.uint8
    assert run.step1 == run.step0 + K  # the counter advanced by K
    assert (run.out["term"] | run.out["trunc"]).sum(0).min() >= 2 and run.out["trunc"].any()
    e2 = make_env(run.name)
    assert np.array_equal(reset_obs(e2), run.obs0)
    obs, rew, term, trunc = e2.rollout(run.actions_dev)
    for name, t in (("obs", obs), ("rew", rew), ("term", term), ("trunc", trunc)):
        assert torch.equal(t.cpu(), torch.from_numpy(run.out[name])), name
    for a, b in zip(e2.get_state(), run.state):
        assert np.array_equal(host(a), b)
    assert e2.metrics() == run.metrics
    assert run.metrics["env_steps"] == K * B and run.metrics["episodes"] >= 2 * B
    e2.check()


def test_actions_and_nodes_equal_the_oracle(run):
    t = run.thr.astype(np.int64)
    assert (np.diff(t, axis=-1, prepend=0) == 0).any()  # choices of probability exactly 0: empty intervals
    acts, nodes, final = controller_rollout(run.obs0, run.out["obs"], run.out["term"], run.out["trunc"], run.thr,
                                            philox_key(SEED), run.step0)
    assert np.array_equal(run.out["actions"], acts)
    assert np.array_equal(run.out["nodes"], nodes)
    assert np.array_equal(run.final_nodes, final)
    # the last real action is drawn; nothing beyond it ever is (a counted padding entry would give A or more)
    assert run.out["actions"].min() >= 0 and run.out["actions"].max() == run.A - 1
    assert run.out["nodes"].max() < run.M
    assert (run.out["obs"] % 3).max() == 2 and run.out["obs"].max() < run.n_obs  # readings occur and are conditioned on
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
    assert a["obs"][-1].any()  # readings are pending when the second launch starts
    b = {k: host(v) for k, v in e.rollout_controller(31).items()}
    for name in ("obs", "actions", "nodes", "rew", "term", "trunc"):
        assert np.array_equal(np.concatenate((a[name], b[name])), run.out[name]), name
    for x, y in zip(e.get_state(), run.state):
        assert np.array_equal(host(x), y)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)
    assert e.metrics() == run.metrics


def test_open_loop_steps_leave_the_reading_for_the_controller(run_split):
    """17 explicit-action steps, then 31 closed-loop ones: the first of them conditions on the obs the last explicit
    step emitted."""
    import torch
    run = run_split
    e = run.twin()
    first = e.rollout(run.actions_dev[:17])
    assert torch.equal(first[0].cpu(), torch.from_numpy(run.out["obs"][:17]))
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
    e = run.twin()
    out = e.rollout_controller(K, store=("actions",))
    assert sorted(out) == ["actions"]
    assert np.array_equal(host(out["actions"]), run.out["actions"])
    e = run.twin()
    buf = torch.empty((K, B), dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(K, out={"nodes": buf}, store=("nodes", "rew"))
    assert out["nodes"].data_ptr() == buf.data_ptr()
    assert np.array_equal(host(buf), run.out["nodes"]) and np.array_equal(host(out["rew"]), run.out["rew"])


def test_deterministic_controller_and_chosen_start_nodes(gpu_device):
    M = 3
    e = make_env("k8_m1_cell")
    n_obs, A = int(e.single_observation_space.n), int(e.single_action_space.n)
    p = np.zeros((M, n_obs, A, M))
    for n in range(M):
        p[n, :, A - 1, (n + 1) % M] = 1.0  # always the last action (CHECK 7); the node cycles 0 -> 1 -> 2 -> 0
    e.set_controller(probs=p)
    reset_obs(e)
    assert not host(e.controller_nodes).any()  # reset zeroes them
    start = (np.arange(B) * 7 % M).astype(np.uint8)
    e.controller_nodes = start
    out = {k: host(v) for k, v in e.rollout_controller(25).items()}
    assert (out["actions"] == A - 1).all()
    ended = out["term"] | out["trunc"]
    assert ended[TL - 1].all() and ended.sum() == B  # checks never terminate: one truncation each
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
    from gym_po_amd import RockSample
    from gym_po_amd._lib import GymPoError
    e = make_env("k8_m1_cell", num_envs=64)
    n_obs, A = int(e.single_observation_space.n), int(e.single_action_space.n)
    uniform = np.full((n_obs, A), 1.0 / A)
    reset_obs(e)
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(4)
    e.set_controller(probs=np.full((4, n_obs, A, 4), 0.25 / A))  # A * M = 52
    e.rollout_controller(4)
    with pytest.raises(GymPoError, match="more than 64"):
        e.set_controller(probs=np.full((5, n_obs, A, 5), 0.2 / A))  # A * M = 65
    big = RockSample(64, map_size=(5, 5), rocks=tuple((i // 5, i % 5) for i in range(16)))
    with pytest.raises(GymPoError, match="more than 64"):
        big.set_controller(probs=np.full((4, 75, 21, 4), 0.25 / 21))  # A * M = 84
    big.set_controller(probs=np.full((3, 75, 21, 3), 1.0 / 63))  # A * M = 63
    reset_obs(big)
    out = big.rollout_controller(8)
    assert 0 <= int(out["actions"].min()) and int(out["actions"].max()) == 20
    big.check()
    e.set_controller()  # removed again
    with pytest.raises(GymPoError):
        e.rollout_controller(4)
    with pytest.raises(GymPoError):
        e.set_controller(probs=np.full((n_obs + 1, A), 1.0 / A))  # wrong n_obs
    bad = controller_thresholds(uniform)
    bad[0, 7, 1], bad[0, 7, 2] = bad[0, 7, 2], bad[0, 7, 1]  # a non-monotone row
    with pytest.raises(GymPoError):
        e.set_controller(thresholds=bad)
    bad = controller_thresholds(uniform)
    bad[0, 3, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError):
        e.set_controller(thresholds=bad)
    e2 = make_env("k8_m1_cell", num_envs=64)
    e2.set_controller(probs=uniform)
    with pytest.raises(GymPoError, match="before reset"):
        e2.rollout_controller(4)
