"""GPU tests of the closed-loop rollouts on C-ROOMS (cardinal / ordinal actions, a scalar obs): a K-step launch whose
actions the device draws from a tabular finite-state controller must equal the open-loop rollout() of those actions
on a same-seed twin bit for bit (outputs, the float64 state, metrics), and the actions and nodes it emits must equal
the numpy restatement of the controller (tests/controller_oracle.py) run over the obs stream it emitted.

The shape: layout "1", time_limit = 20, B = 1,027 envs = two full 512-env tiles and a ragged one with three live envs
(its last live thread holds one env); B is odd, so k B is odd on every other step, which takes the element-wise
stores. K = 48 steps cross two truncations per env, and so node resets. A = 4 / 8 and M = 1, 3, 8 give rows of L = 4
to 64 entries: the counted path of the row search (up to 4 quads) and the searched one.

One of the four configurations leaves its observation space: with cell_size = 2 the `mdp_goal` obs indexes the
state grid at coordinates / 2, where agents that start in the first row or column of cells, and goals there, fall on
wall cells, whose state index is -1 (the reference computes the same values). Such an obs has no row in the table:
the device clamps it to the last row and flags the handle, as documented, so in that configuration check() raises;
everything else is compared as in the others (the metrics through the raw call, which fills them in before it
reports the flag), and the oracle is fed the obs clamped by the same rule.
"""
import ctypes

import numpy as np
import pytest

from controller_oracle import choose, controller_draws, controller_rollout
from crooms_controller_task import (GOAL, LAYOUT, REWARDS, TIME_LIMIT, TRUNC, UNDETERMINED, bfs_actions,
                                    controller_probs, predict, task_grid)
from gym_po_amd.controller import controller_thresholds
from oracle.crooms import crooms_obs_fn
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

B, K, SEED, TL = 1027, 48, 11, 20
DYADIC = dict(step_reward=-0.25, wall_reward=-0.5, goal_reward=1.0)  # float64 sums are exact in any order
OUTPUTS = ("obs", "actions", "nodes", "rew", "term", "trunc")
CONFIGS = {
    "card_hansen": dict(action_type="cardinal", obs_type="hansen"),  # the fixed default goal
    "ord_hansen8": dict(action_type="ordinal", obs_type="hansen8", goal_xy=None, use_velocity=True),
    "card_mdpgoal": dict(action_type="cardinal", obs_type="mdp_goal", goal_xy=None, cell_size=2.0),  # has_t2
    "ord_room": dict(action_type="ordinal", obs_type="room"),
}
GP_E_UNSUPPORTED, GP_E_DEVICE = -3, -5


def make_env(cfg, num_envs=B, **kw):
    from gym_po_amd import CRoomsEnv
    args = dict(layout="1", time_limit=TL, **DYADIC)
    args.update(CONFIGS[cfg] if isinstance(cfg, str) else cfg)
    args.update(kw)
    return CRoomsEnv(num_envs, **args)


def random_probs(M, n_obs, A, seed):
    """Rows in which about a third of the entries are exactly 0 and the last joint choice never is."""
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, A - 1, M - 1] += 0.05
    return p / p.sum((-1, -2), keepdims=True)


def host(x):
    return x.cpu().numpy()


def reset_obs(env, seed=SEED):
    return host(env.reset(seed=seed))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def raw_metrics(env):
    """(return code, metrics): gp_metrics fills the four sums in before it reports a flagged handle."""
    from gym_po_amd import _lib
    out = (ctypes.c_double * 4)()
    rc = _lib.lib().gp_metrics(env._handle, out)
    return rc, dict(episodes=out[0], return_sum=out[1], length_sum=out[2], env_steps=out[3])


def set_controller(env, thr, lds_max=None):
    """Install the table, under the ctrl_lds_max knob if given (gp_set_controller reads it)."""
    from gym_po_amd._lib import debug_knobs
    if lds_max is None:
        env.set_controller(thresholds=thr)
    else:
        with debug_knobs(ctrl_lds_max=lds_max):
            env.set_controller(thresholds=thr)


def clamp_obs(o, n_obs):
    """The header's rule for an obs outside the table: the last row."""
    o = np.asarray(o, dtype=np.int64)
    return np.where((o < 0) | (o >= n_obs), n_obs - 1, o)


class Run:
    """One case, run once and shared (left unchanged) by the tests that read it."""

    def __init__(self, cfg, M, lds_max=None, num_envs=B, steps=K, knobs=None):
        from gym_po_amd._lib import debug_knobs
        self.cfg, self.M, self.lds_max, self.B, self.K, self.knobs = cfg, M, lds_max, num_envs, steps, knobs or {}
        with debug_knobs(**self.knobs):
            e1 = make_env(cfg, num_envs)
            self.n_obs, self.A = int(e1.single_observation_space.n), int(e1.single_action_space.n)
            self.thr = controller_thresholds(random_probs(M, self.n_obs, self.A, seed=5))
            set_controller(e1, self.thr, lds_max)
        self.lds = e1.query("controller_lds")
        self.blocks = e1.query("persist_blocks")
        assert e1.query("controller_nodes") == M
        self.obs0 = reset_obs(e1)
        self.step0 = e1.query("philox_step")
        out = e1.rollout_controller(steps)
        self.out = {k: host(v) for k, v in out.items()}
        self.state = [host(x) for x in e1.get_state()]
        self.rc, self.metrics = raw_metrics(e1)
        self.final_nodes = host(e1.controller_nodes)
        self.step1 = e1.query("philox_step")
        self.actions_dev = out["actions"]
        seen = np.concatenate((self.obs0[None], self.out["obs"]))
        self.outside = bool(((seen < 0) | (seen >= self.n_obs)).any())  # an obs without a row: clamped and flagged

    def twin(self):
        from gym_po_amd._lib import debug_knobs
        with debug_knobs(**self.knobs):
            e = make_env(self.cfg, self.B)
            set_controller(e, self.thr, self.lds_max)
        assert np.array_equal(reset_obs(e), self.obs0)
        return e

    def same_as(self, e, metrics=True):
        for x, y in zip(e.get_state(), self.state):
            assert np.array_equal(bits(host(x)), bits(y))
        if metrics:
            assert raw_metrics(e)[1] == self.metrics


_RUNS = {}


def get_run(cfg, M, lds_max=None, **kw):
    key = (cfg, M, lds_max, repr(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = Run(cfg, M, lds_max, **kw)
    return _RUNS[key]


@pytest.fixture(params=[(c, m) for c in CONFIGS for m in (1, 3, 8)], ids=lambda p: f"{p[0]}_m{p[1]}")
def run(request, gpu_device):
    return get_run(*request.param)


@pytest.fixture
def run_split(gpu_device):
    return get_run("ord_hansen8", 3)


def check_against_open_loop(run):
    """rollout() of the emitted actions on a same-seed twin: every output, the state as bits, the metrics."""
    import torch
    from gym_po_amd._lib import debug_knobs
    with debug_knobs(**run.knobs):
        e2 = make_env(run.cfg, run.B)
    assert np.array_equal(reset_obs(e2), run.obs0)
    obs, rew, term, trunc = e2.rollout(run.actions_dev)
    for name, t in (("obs", obs), ("rew", rew), ("term", term), ("trunc", trunc)):
        assert torch.equal(t.cpu(), torch.from_numpy(run.out[name])), name
    run.same_as(e2)
    e2.check()


def check_against_oracle(run):
    acts, nodes, final = controller_rollout(clamp_obs(run.obs0, run.n_obs), clamp_obs(run.out["obs"], run.n_obs),
                                            run.out["term"], run.out["trunc"], run.thr, philox_key(SEED), run.step0)
    assert np.array_equal(run.out["actions"], acts)
    assert np.array_equal(run.out["nodes"], nodes)
    assert np.array_equal(run.final_nodes, final)


# ------------------------------------------------------------------ 1, 2: the open loop and the oracle ----
def test_closed_loop_equals_open_loop(run):
    assert run.thr.shape == (run.M, run.n_obs, run.A * run.M)
    assert run.out["obs"].shape == (K, B) and run.out["actions"].dtype == np.int32
    assert run.out["nodes"].dtype == np.uint8 and run.out["obs"].dtype == np.int32
    assert run.step1 == run.step0 + K  # the counter advanced by K
    assert (run.out["term"] | run.out["trunc"]).sum(0).min() >= 2 and run.out["trunc"].any()
    check_against_open_loop(run)
    assert run.metrics["env_steps"] == K * B and run.metrics["episodes"] >= 2 * B
    # an obs outside the observation space (see the module docstring) is the one thing that flags a run
    assert run.outside == (run.cfg == "card_mdpgoal")
    assert run.rc == (GP_E_DEVICE if run.outside else 0)


def test_actions_and_nodes_equal_the_oracle(run):
    t = run.thr.astype(np.int64)
    assert (np.diff(t, axis=-1, prepend=0) == 0).any()  # choices of probability exactly 0: empty intervals
    check_against_oracle(run)
    assert run.out["actions"].min() >= 0 and run.out["actions"].max() < run.A and run.out["nodes"].max() < run.M
    if run.n_obs > 1:  # (the one-room layout's `room` obs has a single value: a table of M rows)
        assert run.out["actions"].min() == 0 and run.out["actions"].max() == run.A - 1
        assert run.out["nodes"].max() == run.M - 1 and len(np.unique(run.out["obs"])) > 1
    if run.M > 1:
        ended = run.out["term"][:-1] | run.out["trunc"][:-1]
        assert ended.any() and not run.out["nodes"][1:][ended].any()  # node 0 after every episode end


# ------------------------------------------------------------------ 3: the obs the controller conditions on ----
# (y, x) on layout "1" (cells 1..11 per axis): a cell centre, y exactly on a cell boundary (3.0 is cell row 3), x on
# one, the last row and column, and the two cells next to the fixed goal (11, 11), off-centre so that the move of
# the twin's step does not end the episode under goal_threshold = 0.125
POSITIONS = np.array([[1.5, 1.5], [3.0, 4.25], [5.5, 7.0], [11.75, 11.25], [10.25, 11.75], [11.25, 10.75],
                      [11.0, 1.0], [6.5, 6.5]])
# the move that brings each position about from a free cell: 0 N, 1 E, 2 S, 3 W (cardinal)
ARRIVE = np.array([3, 2, 1, 2, 2, 1, 2, 0])
MOVES = np.array([[-1, 0], [0, 1], [1, 0], [0, -1]])


@pytest.mark.parametrize("obs_type", ["hansen", "mdp", "mdp_goal", "room_goal"])
def test_controller_conditions_on_the_obs_of_the_state(obs_type, gpu_device):
    n = len(POSITIONS)
    cfg = dict(action_type="cardinal", obs_type=obs_type, action_failure_probability=0.0, action_std=0.0,
               goal_threshold=0.125)
    grid = np.array(make_env(cfg, n).grid)
    # write_obs's value of each position: the obs of the step that arrives there on an open-loop twin
    twin = make_env(cfg, n)
    reset_obs(twin)
    before = POSITIONS - MOVES[ARRIVE]
    assert (grid[tuple(np.floor(before).astype(int).T)] >= 0).all()
    twin.set_state(agent_yx=before, elapsed=np.zeros(n, dtype=np.int32))
    obs_w, rew, term, trunc, _ = twin.step(ARRIVE)
    assert not host(term).any() and not host(trunc).any() and (host(rew) == DYADIC["step_reward"]).all()
    assert np.array_equal(bits(host(twin.get_state()[0])), bits(POSITIONS))
    obs_w = host(obs_w)
    goal = host(twin.get_state()[1]).astype(np.float64) + 0.5
    want = crooms_obs_fn(obs_type, grid, 3, 1.0)(POSITIONS, goal)  # the reference's obs function, restated
    assert np.array_equal(obs_w, np.asarray(want).astype(np.int64))
    if obs_type == "hansen":
        assert obs_w[4] % 3 == 0 and obs_w[5] % 2 == 0 and obs_w[4] != obs_w[5]  # the goal's multiplier: S = 3, E = 2
    # a deterministic 8-node controller whose joint choice j = action * 8 + next node spells digit d of the obs in
    # base 32; the env it drives stands in the positions through set_state, after a reset elsewhere
    env = make_env(cfg, n)
    n_obs = int(env.single_observation_space.n)
    A, M = 4, 8
    decoded = np.zeros(n, dtype=np.int64)
    for d in range(3):
        p = np.zeros((M, n_obs, A, M))
        digit = (np.arange(n_obs) // 32 ** d) % 32
        p[:, np.arange(n_obs), digit // M, digit % M] = 1.0
        env.set_controller(probs=p)
        reset_obs(env)
        env.set_state(agent_yx=POSITIONS, elapsed=np.zeros(n, dtype=np.int32))
        out = env.rollout_controller(1)
        assert not host(out["term"]).any() and not host(out["trunc"]).any()
        j = host(out["actions"])[0].astype(np.int64) * M + host(env.controller_nodes)
        decoded += j * 32 ** d
    assert n_obs <= 32 ** 3 and np.array_equal(decoded, obs_w)
    # and under a random table the first action is the oracle's choice for that obs
    thr = controller_thresholds(random_probs(3, n_obs, A, seed=9))
    env.set_controller(thresholds=thr)
    reset_obs(env)
    env.set_state(agent_yx=POSITIONS, elapsed=np.zeros(n, dtype=np.int32))
    step0 = env.query("philox_step")
    out = env.rollout_controller(1)
    j = choose(controller_draws(n, step0, philox_key(SEED)), thr[0, obs_w])
    assert np.array_equal(host(out["actions"])[0], j // 3)
    assert np.array_equal(host(env.controller_nodes), j % 3)
    env.check()


# ------------------------------------------------------------------ 4: LDS and global memory ----
@pytest.mark.parametrize("cfg,M,lds_max,lds", [("card_hansen", 3, 0, 0),            # 11.25 KB: staged by default
                                               ("ord_room", 8, 0, 0),               # 2 KB
                                               ("card_hansen", 6, 60 * 1024, 1),    # 45 KB: above the default 32 KB
                                               ("card_hansen", 3, 8 * 1024, 0)])    # a budget below the table
def test_lds_staged_equals_global_memory(cfg, M, lds_max, lds, gpu_device):
    """The same table under another ctrl_lds_max lands in the other memory: every output, the state, the nodes and
    the metrics are the same bits."""
    base, other = get_run(cfg, M), get_run(cfg, M, lds_max)
    assert other.lds == lds and base.lds != other.lds
    for k in OUTPUTS:
        assert np.array_equal(base.out[k], other.out[k]), k
    for x, y in zip(base.state, other.state):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(base.final_nodes, other.final_nodes) and base.metrics == other.metrics
    assert base.rc == 0 and other.rc == 0


def test_default_budget_by_table_size(gpu_device):
    """Layout "4" under the default budget: Hansen-4 at M = 1 (1.25 KB) is staged; Hansen-8 with 8 actions (72 KB)
    and mdp_goal (40,000 obs values) are read from global memory."""
    for cfg, n_obs, lds in ((dict(action_type="cardinal", obs_type="hansen"), 80, 1),
                            (dict(action_type="ordinal", obs_type="hansen8"), 2304, 0),
                            (dict(action_type="cardinal", obs_type="mdp_goal"), 40000, 0)):
        e = make_env(dict(cfg, layout="4"), 64)
        A = int(e.single_action_space.n)
        assert int(e.single_observation_space.n) == n_obs
        e.set_controller(probs=np.full((n_obs, A), 1.0 / A))
        assert e.query("controller_lds") == lds and e.query("controller_nodes") == 1


# ------------------------------------------------------------------ 5: split launches, optional outputs ----
def test_split_launches_equal_one_launch(run_split):
    run = run_split
    e = run.twin()
    a = {k: host(v) for k, v in e.rollout_controller(17).items()}
    _, _, nodes17 = controller_rollout(run.obs0, a["obs"], a["term"], a["trunc"], run.thr, philox_key(SEED), run.step0)
    assert np.array_equal(host(e.controller_nodes), nodes17)
    b = {k: host(v) for k, v in e.rollout_controller(31).items()}
    for name in OUTPUTS:
        assert np.array_equal(np.concatenate((a[name], b[name])), run.out[name]), name
    run.same_as(e)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)
    e.check()


def test_optional_outputs(run_split):
    import torch
    run = run_split
    e = run.twin()
    assert e.rollout_controller(K, store=()) == {}
    run.same_as(e)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)
    for name in OUTPUTS:  # each output alone
        e = run.twin()
        out = e.rollout_controller(K, store=(name,))
        assert sorted(out) == [name]
        assert np.array_equal(host(out[name]), run.out[name]), name
        run.same_as(e)
    e = run.twin()
    buf = torch.empty((K, B), dtype=torch.uint8, device=e.device)
    abuf = torch.empty((K, B), dtype=torch.int32, device=e.device)
    out = e.rollout_controller(K, out={"nodes": buf, "actions": abuf}, store=("nodes", "rew", "actions"))
    assert out["nodes"].data_ptr() == buf.data_ptr() and out["actions"].data_ptr() == abuf.data_ptr()
    assert np.array_equal(host(buf), run.out["nodes"]) and np.array_equal(host(out["rew"]), run.out["rew"])
    assert np.array_equal(host(abuf), run.out["actions"])
    e.check()


# ------------------------------------------------------------------ 6: nodes ----
def test_node_get_set_reset(gpu_device):
    M, A = 3, 4
    e = make_env("card_hansen")
    n_obs = int(e.single_observation_space.n)
    p = np.zeros((M, n_obs, A, M))
    for n in range(M):
        p[n, :, A - 1, (n + 1) % M] = 1.0  # always W; the node cycles 0 -> 1 -> 2 -> 0
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
    assert np.array_equal(host(e.controller_nodes), want) and want.any()
    # explicit-action calls and set_state leave the nodes alone; reset and set_controller zero them again
    before = host(e.controller_nodes)
    e.step(np.zeros(B, dtype=np.int64))
    assert np.array_equal(host(e.controller_nodes), before)
    e.rollout(np.zeros((3, B), dtype=np.int64))
    assert np.array_equal(host(e.controller_nodes), before)
    e.set_state(agent_yx=np.full((B, 2), 6.5), elapsed=np.zeros(B, dtype=np.int32))
    assert np.array_equal(host(e.controller_nodes), before)
    reset_obs(e)
    assert not host(e.controller_nodes).any()
    e.controller_nodes = start
    e.set_controller(probs=p)
    assert not host(e.controller_nodes).any()
    with pytest.raises(ValueError):
        e.controller_nodes = np.full(B, M)
    e.check()


# ------------------------------------------------------------------ 7: clamps ----
def test_undersized_table_is_clamped_and_flagged(gpu_device):
    """The C ABI takes any n_obs: an obs beyond the table is clamped on the device and flags the handle."""
    from gym_po_amd import _lib
    from gym_po_amd._lib import GymPoError
    A = 4
    e = make_env("card_hansen", num_envs=300)
    t = controller_thresholds(np.full((2, A), 1.0 / A))  # n_obs = 2: the obs of every free cell lies beyond it
    _lib.check(_lib.lib().gp_set_controller(e._handle, 1, 2, ctypes.c_void_p(t.ctypes.data)), "gp_set_controller")
    assert reset_obs(e).min() >= 2
    out = e.rollout_controller(8)
    assert 0 <= int(out["actions"].min()) and int(out["actions"].max()) < A
    with pytest.raises(GymPoError, match=r"\(-5\)"):
        e.check()
    with pytest.raises(GymPoError, match=r"\(-5\)"):
        e.metrics()


def test_node_beyond_the_controller_is_clamped_and_flagged(gpu_device):
    """A node >= M written from a device tensor (not range-checked on the host) is clamped and flags the handle."""
    import torch
    from gym_po_amd._lib import GymPoError
    A = 4
    e = make_env("card_hansen", num_envs=300)
    e.set_controller(probs=np.full((2, int(e.single_observation_space.n), A, 2), 0.125))
    reset_obs(e)
    e.controller_nodes = torch.full((300,), 2, dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(4)
    assert int(out["nodes"].max()) < 2 and int(out["actions"].max()) < A
    with pytest.raises(GymPoError, match=r"\(-5\)"):
        e.check()


# ------------------------------------------------------------------ 8: tiles per block ----
def test_several_tiles_per_block(gpu_device):
    """persist_bpc = 1: one block per CU. With B = 2 * 512 * CUs + 5 every block takes two tiles and block 0 a third
    (ragged: five live envs), each with its state reloaded and its nodes stored."""
    import torch
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    run = get_run("card_hansen", 3, num_envs=2 * 512 * cus + 5, steps=6, knobs=dict(persist_bpc=1))
    assert run.blocks == cus and run.lds == 1
    assert run.out["obs"].shape == (6, run.B)
    check_against_open_loop(run)
    check_against_oracle(run)
    assert run.rc == 0 and run.metrics["env_steps"] == 6 * run.B


def test_three_envs(gpu_device):
    run = get_run("ord_hansen8", 3, num_envs=3)
    assert run.out["actions"].shape == (K, 3)
    check_against_open_loop(run)
    check_against_oracle(run)
    assert run.rc == 0


# ------------------------------------------------------------------ 9: refusals ----
def test_refusals_by_name(gpu_device):
    from gym_po_amd import _lib
    from gym_po_amd._lib import GymPoError

    def raw_set(e, n_obs, A):
        t = controller_thresholds(np.full((n_obs, A), 1.0 / A))
        return _lib.check(_lib.lib().gp_set_controller(e._handle, 1, n_obs, ctypes.c_void_p(t.ctypes.data)),
                          "gp_set_controller")

    uniform4 = np.full((80, 4), 0.25)
    e = make_env(dict(action_type="yx", obs_type="hansen"), 64)
    with pytest.raises(GymPoError, match="no discrete action space"):
        e.set_controller(probs=uniform4)
    with pytest.raises(GymPoError, match=r"\(-3\).*no discrete action space"):  # the C ABI says the same
        raw_set(e, 80, 4)
    for mode in ("numpy", "replay"):
        e = make_env("card_hansen", 64, rng_mode=mode)
        with pytest.raises(GymPoError, match=rf"\(-3\).*philox.*{mode} mode"):
            e.set_controller(probs=uniform4)
    for obs_type in ("vector_hansen", "grid", "vector_mdp"):
        e = make_env(dict(action_type="cardinal", obs_type=obs_type), 64)
        with pytest.raises(GymPoError, match=r"\(-3\).*scalar obs"):
            e.set_controller(probs=uniform4)
    # populations stay GRID-only
    e = make_env("card_hansen", 64)
    with pytest.raises(GymPoError, match=r"\(-3\).*GRID only"):
        e.set_controller_population(probs=np.full((2, 1, 80, 4, 1), 0.25), group_envs=1024)
    with pytest.raises(GymPoError, match=r"\(-3\).*GRID only"):
        e.controller_scores()
    # tables that do not fit the env
    reset_obs(e)
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(4)
    with pytest.raises(GymPoError, match="without a controller"):
        e.controller_nodes
    with pytest.raises(GymPoError, match="n_obs = 81"):
        e.set_controller(probs=np.full((81, 4), 0.25))
    with pytest.raises(GymPoError, match="over 4 actions"):
        e.set_controller(probs=np.full((80, 8), 0.125))  # the ordinal action count on a cardinal env
    with pytest.raises(GymPoError, match=r"n_nodes must be in \[1, 8\]"):
        e.set_controller(thresholds=np.full((9, 80, 36), 1 << 31, dtype=np.uint32))
    bad = controller_thresholds(uniform4)
    bad[0, 7, 1], bad[0, 7, 2] = bad[0, 7, 2], bad[0, 7, 1]  # a non-monotone row
    with pytest.raises(GymPoError, match="not nondecreasing"):
        e.set_controller(thresholds=bad)
    bad = controller_thresholds(uniform4)
    bad[0, 3, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError, match="not 2\\^31"):
        e.set_controller(thresholds=bad)
    assert e.query("controller_nodes") == 0  # none of them installed anything
    e.set_controller(probs=uniform4)
    e.rollout_controller(4)
    e.set_controller()  # removed again
    assert e.query("controller_nodes") == 0 and e.query("controller_lds") == 0
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(4)
    e2 = make_env("card_hansen", 64)
    e2.set_controller(probs=uniform4)
    with pytest.raises(GymPoError, match="before reset"):
        e2.rollout_controller(4)
    e.check()


# ------------------------------------------------------------------ 10: the task ----
def _task_env():
    from gym_po_amd import CRoomsEnv
    return CRoomsEnv(B, layout=LAYOUT, time_limit=TIME_LIMIT, obs_type="mdp", action_type="cardinal",
                     action_failure_probability=0.0, action_std=0.0, **REWARDS)


def _first_episode(out):
    ended = out["term"] | out["trunc"]
    assert ended.any(0).all()
    return ended.argmax(0)  # the step index at which each env's first episode ends


def test_breadth_first_controller_solves_the_task(gpu_device):
    grid, goal = task_grid()
    act = bfs_actions(grid, goal)
    length, ending, walls = predict(grid, goal, act, TIME_LIMIT)  # pinned to oracle/crooms.py by the CPU test
    env = _task_env()
    assert np.array_equal(np.array(env.grid), grid)
    env.set_controller(probs=controller_probs(grid, act))
    assert env.query("controller_lds") == 1  # 200 obs x 16 B
    reset_obs(env)
    start = np.floor(host(env.get_state()[0])).astype(int)
    assert np.array_equal(host(env.get_state()[1]), np.full((B, 2), goal))
    out = {k: host(v) for k, v in env.rollout_controller(K).items()}
    term, rew = out["term"], out["rew"]
    assert not out["trunc"].any() and term.any(0).all()
    assert (rew[term] == REWARDS["goal_reward"]).all()  # every episode ends on the goal,
    assert (rew[~term] == REWARDS["step_reward"]).all()  # and every other step is a move: no wall is hit
    first = _first_episode(out)
    assert np.array_equal(first + 1, length[tuple(start.T)])  # the first episode lasts the predicted number of steps
    assert len(np.unique(first)) > 20
    env.check()


def test_rotated_controller_does_not(gpu_device):
    """The same table with every action turned by two. The expectation per start cell is the simulation's: the
    time limit, except where it says otherwise (the goal cell itself: see the CPU test)."""
    grid, goal = task_grid()
    act = bfs_actions(grid, goal, rotate=True)
    length, ending, walls = predict(grid, goal, act, TIME_LIMIT)
    env = _task_env()
    env.set_controller(probs=controller_probs(grid, act))
    reset_obs(env)
    start = tuple(np.floor(host(env.get_state()[0])).astype(int).T)
    out = {k: host(v) for k, v in env.rollout_controller(K).items()}
    first = _first_episode(out)
    env_ids = np.arange(B)
    decided = ending[start] != UNDETERMINED
    assert decided.all() and (ending[start] == TRUNC).sum() > 0.9 * B
    assert np.array_equal(first[decided] + 1, length[start][decided])
    assert np.array_equal(out["term"][first, env_ids][decided], ending[start][decided] == GOAL)
    assert np.array_equal(out["trunc"][first, env_ids][decided], ending[start][decided] == TRUNC)
    reached = ending[start] == GOAL
    assert (length[start][~reached] == TIME_LIMIT + 1).all()  # no other first episode is shorter than the time limit
    assert (np.array(start).T[reached] == np.array(goal)).all()  # the goal cell itself
    env.check()
