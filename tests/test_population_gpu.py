"""GPU tests of the controller populations (set_controller_population / controller_scores): P controllers run side by
side in one closed-loop launch, env e driven by controller e // G, with one score row per controller.

The main oracle is the twin: the draws are keyed by (env, step), so the trajectory of env e under a population equals
its trajectory on a same-seed handle with thr[e // G] installed by set_controller. The scores are checked against the
numpy restatement in tests/population_oracle.py, computed from the planes the run emitted.

Shapes: B = 3075 = 3 * 1024 + 3 envs with G = 1024, so P = 4: every group is one whole block, the last a ragged block
whose one live thread owns 3 of its 4 envs. B = 4099 with G = 2048 (P = 3) has groups that span two blocks.
K = 48 steps under time_limit = 20 end at least two episodes in every env, truncations included.
FourRooms Hansen-4 tables with M = 1, 2 are staged in LDS per controller, M = 3 is read from global memory; ROOMS
Hansen-8 with M = 5 has searched rows of 10 quads; the table obs with random goals has 8-entry rows.

Sum bounds: the device adds float terms into doubles (per thread, then per block, then per group on the host), so its
sum differs from the correctly rounded one by at most (n - 1) * 2^-53 * sum|term|; the tests allow
n * 2^-52 * sum|term|, n the group's term count (population_oracle computes it)."""
import numpy as np
import pytest

from controller_oracle import controller_rollout
from fixtures import load_index
from gym_po_amd.controller import controller_thresholds, population_thresholds
from oracle.philox import philox_key
from population_oracle import population_scores

pytestmark = pytest.mark.gpu

B, G, K, SEED, GAMMA = 3075, 1024, 48, 11, 0.95
INDEX = load_index()["cases"]
PLANES = ("obs", "actions", "nodes", "rew", "term", "trunc")
COUNTS = ("episodes", "length_sum", "env_steps")

# name -> (fixture config, kwargs on top of it, controller nodes, num_envs, group_envs)
CASES = {
    "fr_hansen4_m1": ("fr_hansen_tl20", {}, 1, B, G),                        # per-controller table staged in LDS
    "fr_hansen4_m2": ("fr_hansen_tl20", {}, 2, B, G),                        # staged in LDS
    "fr_hansen4_m3": ("fr_hansen_tl20", {}, 3, B, G),                        # 58 KB per controller: global memory
    "rooms_hansen8_m5": ("rooms_4_hansen8", dict(time_limit=20), 5, B, G),   # searched rows of 10 quads
    "rooms_table_randgoal_m1": ("rooms_2_goal_mdp_randgoal", {}, 1, B, G),   # table obs, random goals
    "fr_hansen4_m2_two_block_groups": ("fr_hansen_tl20", {}, 2, 4099, 2048),  # P = 3, groups of two blocks
}
STAGED = {"fr_hansen4_m1": 1, "fr_hansen4_m2": 1, "fr_hansen4_m3": 0, "rooms_hansen8_m5": 0,
          "fr_hansen4_m2_two_block_groups": 1}


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


def host_out(out):
    return {k: host(v) for k, v in out.items()}


def state_of(env):
    return [host(x) for x in env.get_state()]


def assert_scores_match(got, want, what=""):
    """Counts exact; the two sums within the double-summation bound of their group."""
    for f in COUNTS:
        assert got[f].dtype == np.int64 and np.array_equal(got[f], want[f]), (what, f, got[f], want[f])
    for f, b in (("return_sum", "return_bound"), ("discounted_return_sum", "discounted_bound")):
        err = np.abs(got[f] - want[f])
        print(what, f, "device", got[f], "oracle", want[f], "err", err, "bound", want[b])
        assert got[f].dtype == np.float64 and np.all(err <= want[b]), (what, f, err, want[b])


class Run:
    """One case, run once and shared (left unchanged) by the tests that read it."""

    def __init__(self, name):
        config, extra, M, nb, g = CASES[name]
        self.name, self.config, self.extra, self.M, self.B, self.G = name, config, extra, M, nb, g
        self.P = -(-nb // g)
        e1 = make_env(config, extra, nb)
        self.n_obs, self.A = int(e1.single_observation_space.n), int(e1.single_action_space.n)
        self.probs = np.stack([random_probs(M, self.n_obs, self.A, seed=50 + p) for p in range(self.P)])
        self.thr = population_thresholds(self.probs)
        e1.set_controller_population(thresholds=self.thr, group_envs=g, gamma=GAMMA)
        self.queries = {k: e1.query(k) for k in ("controller_population", "controller_group_envs",
                                                 "controller_group_multiple", "controller_lds", "controller_nodes")}
        self.obs0 = reset_obs(e1)
        self.step0 = e1.query("philox_step")
        self.elapsed0 = state_of(e1)[2]
        out = e1.rollout_controller(K)
        self.actions_dev = out["actions"]
        self.out = host_out(out)
        self.state = state_of(e1)
        self.metrics = e1.metrics()
        self.scores = e1.controller_scores()
        self.final_nodes = host(e1.controller_nodes)
        self.step1 = e1.query("philox_step")

    def cols(self, p):
        return slice(p * self.G, min((p + 1) * self.G, self.B))

    def population_twin(self, gamma=GAMMA):
        e = make_env(self.config, self.extra, self.B)
        e.set_controller_population(thresholds=self.thr, group_envs=self.G, gamma=gamma)
        assert np.array_equal(reset_obs(e), self.obs0)
        return e

    def oracle_scores(self, gamma=GAMMA):
        return population_scores(self.out["rew"], self.out["term"], self.out["trunc"], self.elapsed0, self.G, gamma)


_RUNS = {}


def get_run(name):
    if name not in _RUNS:
        _RUNS[name] = Run(name)
    return _RUNS[name]


@pytest.fixture(params=sorted(CASES))
def run(request, gpu_device):
    return get_run(request.param)


@pytest.fixture
def run_m1(gpu_device):
    return get_run("fr_hansen4_m1")


@pytest.fixture
def run_m3(gpu_device):
    return get_run("fr_hansen4_m3")


# ---- 1
def test_population_equals_per_controller_twins(run):
    assert run.queries["controller_population"] == run.P and run.queries["controller_group_envs"] == run.G
    assert run.queries["controller_group_multiple"] == 1024 and run.queries["controller_nodes"] == run.M
    if run.name in STAGED:
        assert run.queries["controller_lds"] == STAGED[run.name]
    if run.config != "rooms_2_goal_mdp_randgoal":  # (its time_limit is 60; the others' 20: elapsed > 20 truncates)
        assert (run.out["term"] | run.out["trunc"]).sum(0).min() >= 2 and run.out["trunc"].any()
    assert any(not np.array_equal(run.thr[0], run.thr[p]) for p in range(1, run.P))
    for p in range(run.P):
        e = make_env(run.config, run.extra, run.B)
        e.set_controller(thresholds=run.thr[p])
        assert e.query("controller_population") == 0
        assert np.array_equal(reset_obs(e), run.obs0)
        out = host_out(e.rollout_controller(K))
        c = run.cols(p)
        for name in PLANES:
            assert np.array_equal(out[name][:, c], run.out[name][:, c]), (p, name)
        for a, b in zip(state_of(e), run.state):
            assert np.array_equal(a[c], b[c]), p
        assert np.array_equal(host(e.controller_nodes)[c], run.final_nodes[c]), p
    # the groups do differ: group 0's columns under the last controller are another trajectory
    assert not np.array_equal(out["actions"][:, run.cols(0)], run.out["actions"][:, run.cols(0)])


# ---- 2
def test_closed_loop_equals_open_loop_and_the_controller_oracle(run):
    import torch
    assert run.out["obs"].shape == (K, run.B) and run.out["actions"].dtype == np.int32
    assert run.out["nodes"].dtype == np.uint8
    assert run.step1 == run.step0 + K
    e2 = make_env(run.config, run.extra, run.B)
    assert np.array_equal(reset_obs(e2), run.obs0)
    obs, rew, term, trunc = e2.rollout(run.actions_dev)
    for name, t in (("obs", obs), ("rew", rew), ("term", term), ("trunc", trunc)):
        assert torch.equal(t.cpu(), torch.from_numpy(run.out[name])), name
    for a, b in zip(state_of(e2), run.state):
        assert np.array_equal(a, b)
    assert e2.metrics() == run.metrics
    assert run.metrics["env_steps"] == K * run.B
    for p in range(run.P):  # the oracle over every column with table p, read on group p's columns
        acts, nodes, final = controller_rollout(run.obs0, run.out["obs"], run.out["term"], run.out["trunc"],
                                                run.thr[p], philox_key(SEED), run.step0)
        c = run.cols(p)
        assert np.array_equal(run.out["actions"][:, c], acts[:, c]), p
        assert np.array_equal(run.out["nodes"][:, c], nodes[:, c]), p
        assert np.array_equal(run.final_nodes[c], final[c]), p
    assert run.out["nodes"].max() < run.M and (run.M == 1 or run.out["nodes"].any())


# ---- 3
@pytest.mark.parametrize("nb,g", [(B, G), (4099, 2048)])
def test_deterministic_controllers_mark_their_groups(nb, g, gpu_device):
    e = make_env("fr_hansen_tl20", num_envs=nb)
    n_obs, A = int(e.single_observation_space.n), int(e.single_action_space.n)
    P = -(-nb // g)
    probs = np.zeros((P, 1, n_obs, A, 1))
    for p in range(P):
        probs[p, 0, :, p % A, 0] = 1.0
    e.set_controller_population(probs=probs, group_envs=g)
    reset_obs(e)
    acts = host(e.rollout_controller(12, store=("actions",))["actions"])
    assert np.array_equal(acts, np.broadcast_to((np.arange(nb) // g) % A, (12, nb)))
    e.check()


# ---- 4
def test_scores_match_the_oracle(run):
    want = run.oracle_scores()
    assert_scores_match(run.scores, want, run.name)
    assert sorted(run.scores) == sorted(COUNTS + ("return_sum", "discounted_return_sum"))
    assert all(v.shape == (run.P,) for v in run.scores.values())
    assert np.array_equal(run.scores["env_steps"], [K * (run.cols(p).stop - run.cols(p).start) for p in range(run.P)])
    if run.config != "rooms_2_goal_mdp_randgoal":
        assert (run.scores["discounted_return_sum"] != run.scores["return_sum"]).any()
    for f in COUNTS:  # the groups partition the batch: their counts sum to metrics(), ragged last block included
        print(run.name, f, "groups", run.scores[f], "sum", int(run.scores[f].sum()), "metrics()", run.metrics[f])
        assert int(run.scores[f].sum()) == run.metrics[f], (f, run.scores[f], run.metrics[f])


def test_group_counts_sum_to_metrics_on_whole_blocks(gpu_device):
    e = make_env("fr_hansen_tl20", num_envs=4096)
    n_obs, A = int(e.single_observation_space.n), int(e.single_action_space.n)
    probs = np.stack([random_probs(2, n_obs, A, seed=70 + p) for p in range(2)])
    e.set_controller_population(probs=probs, group_envs=2048, gamma=GAMMA)
    reset_obs(e)
    out = host_out(e.rollout_controller(K, store=("rew", "term", "trunc")))
    s, m = e.controller_scores(), e.metrics()
    assert_scores_match(s, population_scores(out["rew"], out["term"], out["trunc"], np.zeros(4096, dtype=np.int64),
                                             2048, GAMMA), "whole blocks")
    for f in COUNTS:
        assert int(s[f].sum()) == m[f], (f, s[f], m[f])
    assert s["episodes"].min() >= 2 * 2048


def test_scores_with_gamma_one_and_without_outputs(run_m1, run_m3):
    for run in (run_m1, run_m3):
        e = run.population_twin(gamma=1.0)
        assert e.rollout_controller(K, store=()) == {}  # all six outputs omitted
        s = e.controller_scores()
        want = run.oracle_scores(gamma=1.0)
        assert_scores_match(s, want, run.name + " gamma=1")
        assert np.all(np.abs(s["discounted_return_sum"] - s["return_sum"]) <= want["return_bound"])
        for f in COUNTS + ("return_sum",):  # the scores do not depend on what is stored, nor (these four) on gamma
            assert np.array_equal(s[f], run.scores[f]), f
        assert e.metrics() == run.metrics
        for a, b in zip(state_of(e), run.state):
            assert np.array_equal(a, b)
    e = run_m3.population_twin()  # gamma = 0.95 again, nothing stored
    e.rollout_controller(K, store=())
    s = e.controller_scores()
    for f in s:
        assert np.array_equal(s[f], run_m3.scores[f]), f


# ---- 5
def test_split_launches_equal_one_launch(run_m1, run_m3):
    for run in (run_m1, run_m3):
        e = run.population_twin()
        a = host_out(e.rollout_controller(17))
        mid = state_of(e)[2]
        assert 0 < mid.max() <= 17 and (mid > 0).mean() > 0.5  # the second launch starts mid-episode nearly everywhere
        b = host_out(e.rollout_controller(31))
        for name in PLANES:
            assert np.array_equal(np.concatenate((a[name], b[name])), run.out[name]), name
        for x, y in zip(state_of(e), run.state):
            assert np.array_equal(x, y)
        assert np.array_equal(host(e.controller_nodes), run.final_nodes)
        s = e.controller_scores()
        assert_scores_match(s, run.oracle_scores(), run.name + " split 17 + 31")
        m = e.metrics()  # the aggregate's counts too do not depend on how the steps are split
        assert all(m[f] == run.metrics[f] for f in COUNTS)


# ---- 6
def test_set_state_elapsed_is_the_discount_exponent(run_m1):
    run = run_m1
    e = run.population_twin()
    e.set_state(elapsed=np.full(run.B, 7, dtype=np.int32))
    elapsed0 = state_of(e)[2]
    assert (elapsed0 == 7).all()
    out = host_out(e.rollout_controller(5))
    s = e.controller_scores()
    want = population_scores(out["rew"], out["term"], out["trunc"], elapsed0, run.G, GAMMA)
    assert_scores_match(s, want, "elapsed 7")
    if np.abs(out["rew"]).sum() > 0:  # weighed from gamma^7 on, not from 1
        from_zero = population_scores(out["rew"], out["term"], out["trunc"], np.zeros(run.B, dtype=np.int64), run.G,
                                      GAMMA)
        assert not np.array_equal(from_zero["discounted_return_sum"], want["discounted_return_sum"])


# ---- 7
@pytest.mark.parametrize("M", [1, 3])
def test_population_of_one_equals_the_single_controller(M, gpu_device):
    e1, e2 = make_env("fr_hansen_tl20"), make_env("fr_hansen_tl20")
    n_obs, A = int(e1.single_observation_space.n), int(e1.single_action_space.n)
    thr = controller_thresholds(random_probs(M, n_obs, A, seed=9))
    e1.set_controller_population(thresholds=thr[None], group_envs=4096)
    e2.set_controller(thresholds=thr)
    assert e1.query("controller_population") == 1 and e1.query("controller_lds") == e2.query("controller_lds")
    assert np.array_equal(reset_obs(e1), reset_obs(e2))
    a, b = host_out(e1.rollout_controller(K)), host_out(e2.rollout_controller(K))
    for name in PLANES:
        assert np.array_equal(a[name], b[name]), name
    for x, y in zip(state_of(e1), state_of(e2)):
        assert np.array_equal(x, y)
    assert np.array_equal(host(e1.controller_nodes), host(e2.controller_nodes))
    assert e1.metrics() == e2.metrics()
    # group_envs=None: ceil(B / P) rounded up to a multiple of 1024 (P = 1: 3075 -> 4096)
    e1.set_controller_population(thresholds=thr[None])
    assert e1.query("controller_group_envs") == 4096


# ---- 8
def test_table_in_lds_equals_table_in_global_memory(run_m1):
    from gym_po_amd._lib import debug_knobs
    run = run_m1
    assert run.queries["controller_lds"] == 1
    e = make_env(run.config, run.extra, run.B)
    with debug_knobs(ctrl_lds_max=0):  # gp_debug_set; gp_debug_reset on exit
        e.set_controller_population(thresholds=run.thr, group_envs=run.G, gamma=GAMMA)
    assert e.query("controller_lds") == 0
    assert np.array_equal(reset_obs(e), run.obs0)
    out = host_out(e.rollout_controller(K))
    for name in PLANES:
        assert np.array_equal(out[name], run.out[name]), name
    for x, y in zip(state_of(e), run.state):
        assert np.array_equal(x, y)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)
    assert e.metrics() == run.metrics
    s = e.controller_scores()
    for f in s:
        assert np.array_equal(s[f], run.scores[f]), f


# ---- 9
def test_lifecycle(run_m1):
    run = run_m1
    e = run.population_twin()
    e.rollout_controller(K, store=())
    s = e.controller_scores(clear=True)  # read, then zeroed
    for f in s:
        assert np.array_equal(s[f], run.scores[f]), f
    z = e.controller_scores()
    assert all(not v.any() for v in z.values())
    e.rollout_controller(3, store=())
    assert (e.controller_scores()["env_steps"] == 3 * np.diff(np.r_[np.arange(0, run.B, run.G), run.B])).all()
    assert host(e.controller_nodes).shape == (run.B,)
    reset_obs(e)  # zeroes scores and nodes
    assert all(not v.any() for v in e.controller_scores().values())
    assert not host(e.controller_nodes).any()
    # a single controller replaces the population
    e.set_controller(thresholds=run.thr[1])
    assert e.query("controller_population") == 0 and e.query("controller_group_envs") == 0
    from gym_po_amd._lib import GymPoError
    with pytest.raises(GymPoError, match=r"\(-4\).*population"):
        e.controller_scores()
    fresh = make_env(run.config, run.extra, run.B)
    fresh.set_controller(thresholds=run.thr[1])
    assert np.array_equal(reset_obs(e), reset_obs(fresh))
    a, b = host_out(e.rollout_controller(K)), host_out(fresh.rollout_controller(K))
    for name in PLANES:
        assert np.array_equal(a[name], b[name]), name
    assert e.metrics() == fresh.metrics()
    # and a population replaces a single controller; removing leaves neither
    e.set_controller_population(thresholds=run.thr, group_envs=run.G)
    assert e.query("controller_population") == run.P
    e.set_controller_population()
    assert e.query("controller_population") == 0 and e.query("controller_nodes") == 0
    with pytest.raises(GymPoError):
        e.rollout_controller(4)


# ---- 10
def test_errors(gpu_device):
    from gym_po_amd import AntTagGridEnv, RockSample, RoomsEnv, TaxiVecEnv
    from gym_po_amd._lib import GymPoError
    INVALID, UNSUPPORTED, STATE = r"\(-1\)", r"\(-3\)", r"\(-4\)"
    e = make_env("fr_hansen_tl20")
    n_obs, A = int(e.single_observation_space.n), int(e.single_action_space.n)
    uniform = np.full((4, 1, n_obs, A, 1), 1.0 / A)
    thr = population_thresholds(uniform)
    with pytest.raises(GymPoError, match=STATE):
        e.controller_scores()  # no population
    with pytest.raises(GymPoError, match=INVALID + ".*multiple of 1024"):
        e.set_controller_population(thresholds=thr, group_envs=1000)
    with pytest.raises(GymPoError, match=INVALID + ".*groups"):
        e.set_controller_population(thresholds=thr[:3], group_envs=1024)  # ceil(3075 / 1024) = 4, not 3
    with pytest.raises(GymPoError, match=INVALID + ".*groups"):
        e.set_controller_population(thresholds=thr, group_envs=2048)  # 2 groups, not 4
    with pytest.raises(GymPoError, match="do not make 3 groups"):
        e.set_controller_population(thresholds=thr[:3])  # group_envs=None: 1025 -> 2048 gives 2 groups
    for gamma in (0.0, 1.5, float("nan"), -0.5):
        with pytest.raises(GymPoError, match=INVALID + ".*gamma"):
            e.set_controller_population(thresholds=thr, group_envs=1024, gamma=gamma)
    bad = thr.copy()
    bad[2, 0, 5, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError, match=INVALID + ".*controller 2.*node 0, obs 5"):
        e.set_controller_population(thresholds=bad, group_envs=1024)
    bad = thr.copy()
    bad[3, 0, 7, 1], bad[3, 0, 7, 2] = thr[3, 0, 7, 2], thr[3, 0, 7, 1]  # a non-monotone row
    with pytest.raises(GymPoError, match=INVALID + ".*controller 3.*node 0, obs 7"):
        e.set_controller_population(thresholds=bad, group_envs=1024)
    with pytest.raises(GymPoError):
        e.set_controller_population(thresholds=population_thresholds(uniform[:, :, :-1]), group_envs=1024)  # n_obs
    assert e.query("controller_population") == 0  # nothing was installed by any of these
    reset_obs(e)
    with pytest.raises(GymPoError):
        e.rollout_controller(4)
    e.set_controller_population(thresholds=thr, group_envs=1024, gamma=1.0)  # gamma = 1 is inside (0, 1]
    with pytest.raises(GymPoError, match=INVALID):
        e.set_controller_population(thresholds=bad, group_envs=1024)
    assert e.query("controller_population") == 4  # an invalid table leaves the installed one
    e.rollout_controller(4, store=())
    e.check()
    # kinds, modes and obs kinds without populations: GP_E_UNSUPPORTED with a message
    npy = make_env("fr_hansen_tl20", rng_mode="numpy")
    with pytest.raises(GymPoError, match=UNSUPPORTED + ".*philox"):
        npy.set_controller_population(thresholds=thr, group_envs=1024)
    with pytest.raises(GymPoError, match=UNSUPPORTED + ".*philox"):
        npy.controller_scores()
    vec = RoomsEnv(64, layout="1", obs_type="vector_hansen", rng_mode="philox")
    with pytest.raises(GymPoError, match=UNSUPPORTED + ".*scalar obs"):
        av = int(vec.single_action_space.n)
        vec.set_controller_population(probs=np.full((1, 1, 16, av, 1), 1.0 / av), group_envs=1024)
    rock = RockSample(64, map_size=(5, 5), rocks=((1, 1), (3, 3), (2, 4)), init_pos=(2, 0))
    ant = AntTagGridEnv(64, size=6, min_distance=3.0, obs_type="index")
    taxi = TaxiVecEnv(64, hansen_obs=True, rng_mode="philox")
    for env in (rock, ant, taxi):
        n, a = env._controller_n_obs(), int(env.single_action_space.n)
        with pytest.raises(GymPoError, match=UNSUPPORTED + ".*not supported"):
            env.set_controller_population(probs=np.full((1, 1, int(n), a, 1), 1.0 / a), group_envs=1024)
        with pytest.raises(GymPoError, match=UNSUPPORTED + ".*not supported"):
            env.controller_scores()
