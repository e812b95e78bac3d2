"""GPU tests of the closed-loop rollouts on grid Heaven-Hell: a K-step launch whose actions the device draws from a
tabular finite-state controller must equal the open-loop rollout() of those actions on a twin env bit for bit (outputs,
final state, metrics), and the actions and nodes it emits must equal the numpy restatement of the controller
(tests/controller_oracle.py, which is not env-specific) run over the obs stream it emitted.

A = 4, so rows hold L = 4 M entries, whole 16-B quads: M = 1, 2, 3 take the scanned path of the row search (up to 4
quads), M = 8 the searched one (8 quads). The table is staged in LDS when it fits the budget (32 KB by default) behind
the env's tables, else read from global memory; both must give the same bits. B = 2051 envs = three 1,024-env tiles,
the last one ragged; K = 48 steps under time_limit = 20 end at least two episodes in every env.

The task itself, on the default maze without slips: a 3-node controller that walks to the priest, takes the node the
signal names and walks to that arm earns +1 in every episode; with the two nodes swapped it earns -1 in every one.
"""
import numpy as np
import pytest

from controller_oracle import controller_rollout
from gym_po_amd.controller import controller_thresholds
from heavenhell_oracle import FREE, LEFT, PRIEST, RIGHT, HeavenHellOracle, Spec, oracle_rollout
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu

B, K, SEED, TL, A = 2051, 48, 11, 20, 4
DYADIC = dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=-0.25, wall_reward=-0.5)
MID = ("L..P..R",
       "L.PPP.R",
       "##...##",
       "##.S.##",
       "##S..##")
# name -> (obs_type, controller nodes, the table is staged in LDS under the default budget)
CASES = {
    "cell_m1": ("cell_signal", 1, 1), "cell_m2": ("cell_signal", 2, 1), "cell_m3": ("cell_signal", 3, 1),
    "cell_m8": ("cell_signal", 8, 0),  # 105 obs x 8 x 8 x 16 B = 105 KB
    "hansen_m1": ("hansen_signal", 1, 1), "hansen_m2": ("hansen_signal", 2, 1), "hansen_m3": ("hansen_signal", 3, 1),
    "hansen_m8": ("hansen_signal", 8, 0),  # 48 KB: above the default budget, below the knob's 60 KB
}


def make_env(name, num_envs=B, **kw):
    from gym_po_amd import HeavenHellGridEnv
    return HeavenHellGridEnv(num_envs, maze=MID, obs_type=CASES[name][0], action_failure_probability=1 / 3,
                             time_limit=TL, **DYADIC, **kw)


def random_probs(M, n_obs, seed):
    """Rows in which about a third of the entries are exactly 0 and the last joint choice never is."""
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, A - 1, M - 1] += 0.05
    return p / p.sum((-1, -2), keepdims=True)


def reset_obs(env, seed=SEED):
    return env.reset(seed=seed)[0].cpu().numpy()


def host(x):
    return x.cpu().numpy()


def set_controller(env, thr, lds_max=None):
    """Install the table, under the ctrl_lds_max knob if given (gp_set_controller reads it)."""
    from gym_po_amd._lib import debug_knobs
    if lds_max is None:
        env.set_controller(thresholds=thr)
    else:
        with debug_knobs(ctrl_lds_max=lds_max):
            env.set_controller(thresholds=thr)


class Run:
    """One case, run once and shared (left unchanged) by the tests that read it."""

    def __init__(self, name, lds_max=None):
        self.name, self.M, self.lds_max = name, CASES[name][1], lds_max
        e1 = make_env(name)
        self.n_obs = int(e1.single_observation_space.n)
        self.thr = controller_thresholds(random_probs(self.M, self.n_obs, seed=5))
        set_controller(e1, self.thr, lds_max)
        self.lds = e1.query("controller_lds")
        assert e1.query("controller_nodes") == self.M
        self.obs0 = reset_obs(e1)
        self.step0 = e1.query("philox_step")
        out = e1.rollout_controller(K)
        self.out = {k: host(v) for k, v in out.items()}
        self.state = [host(x) for x in e1.get_state()]
        self.metrics = e1.metrics()
        self.final_nodes = host(e1.controller_nodes)
        self.step1 = e1.query("philox_step")
        self.actions_dev = out["actions"]
        e1.check()

    def twin(self):
        e = make_env(self.name)
        set_controller(e, self.thr, self.lds_max)
        assert np.array_equal(reset_obs(e), self.obs0)
        return e


_RUNS = {}


def get_run(name, lds_max=None):
    if (name, lds_max) not in _RUNS:
        _RUNS[name, lds_max] = Run(name, lds_max)
    return _RUNS[name, lds_max]


@pytest.fixture(params=sorted(CASES))
def run(request, gpu_device):
    return get_run(request.param)


@pytest.fixture
def run_split(gpu_device):
    return get_run("hansen_m2")


def test_closed_loop_equals_open_loop(run):
    import torch
    assert run.thr.shape == (run.M, run.n_obs, A * run.M) and run.lds == CASES[run.name][2]
    assert run.out["obs"].shape == (K, B) and run.out["actions"].dtype == np.int32
    assert run.out["nodes"].dtype == np.uint8
    assert run.step1 == run.step0 + K  # the counter advanced by K
    assert (run.out["term"] | run.out["trunc"]).sum(0).min() >= 2 and run.out["trunc"].any() and run.out["term"].any()
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
    assert run.out["actions"].min() == 0 and run.out["actions"].max() == A - 1
    assert run.out["nodes"].max() == run.M - 1
    assert (run.out["obs"] % 3).max() == 2 and run.out["obs"].max() < run.n_obs  # the signal occurs
    if run.M > 1:
        ended = run.out["term"][:-1] | run.out["trunc"][:-1]
        assert ended.any() and not run.out["nodes"][1:][ended].any()  # node 0 after every episode end


@pytest.mark.parametrize("name,lds_max,lds", [("hansen_m2", 0, 0), ("cell_m3", 0, 0), ("hansen_m8", 60 * 1024, 1),
                                              ("hansen_m3", 4096, 0)])
def test_lds_staged_equals_global_memory(name, lds_max, lds, gpu_device):
    """The same table under another ctrl_lds_max lands in the other memory: every output, the state, the nodes and the
    metrics are the same bits."""
    base, other = get_run(name), get_run(name, lds_max)
    assert other.lds == lds and base.lds == CASES[name][2] and base.lds != other.lds
    for k in ("obs", "actions", "nodes", "rew", "term", "trunc"):
        assert np.array_equal(base.out[k], other.out[k]), k
    for x, y in zip(base.state, other.state):
        assert np.array_equal(x, y)
    assert np.array_equal(base.final_nodes, other.final_nodes) and base.metrics == other.metrics


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


def test_optional_outputs(run_split):
    import torch
    run = run_split
    e = run.twin()
    assert e.rollout_controller(K, store=()) == {}
    assert e.metrics() == run.metrics
    for x, y in zip(e.get_state(), run.state):
        assert np.array_equal(host(x), y)
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)
    for name in ("obs", "actions", "nodes", "rew", "term", "trunc"):  # each output alone
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
    e.check()


def test_node_get_set_reset(gpu_device):
    M = 3
    e = make_env("cell_m1")
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
    assert np.array_equal(host(e.controller_nodes), want)
    # explicit-action calls leave the nodes alone; reset and set_controller zero them again
    before = host(e.controller_nodes)
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
    e = make_env("cell_m1", num_envs=300)
    t = controller_thresholds(np.full((2, A), 1.0 / A))  # n_obs = 2: every obs of a free cell lies beyond it
    _lib.check(_lib.lib().gp_set_controller(e._handle, 1, 2, ctypes.c_void_p(t.ctypes.data)), "gp_set_controller")
    reset_obs(e)
    out = e.rollout_controller(8)
    assert 0 <= int(out["actions"].min()) and int(out["actions"].max()) < A
    with pytest.raises(GymPoError, match=r"\(-5\)"):
        e.check()


def test_node_beyond_the_controller_is_clamped_and_flagged(gpu_device):
    """A node >= M written from a device tensor (not range-checked on the host) is clamped and flags the handle."""
    import torch
    from gym_po_amd._lib import GymPoError
    e = make_env("hansen_m2", num_envs=300)
    e.set_controller(probs=np.full((2, int(e.single_observation_space.n), A, 2), 0.125))
    reset_obs(e)
    e.controller_nodes = torch.full((300,), 2, dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(4)
    assert int(out["nodes"].max()) < 2 and int(out["actions"].max()) < A
    with pytest.raises(GymPoError, match=r"\(-5\)"):
        e.check()


def test_errors_and_populations_unsupported(gpu_device):
    from gym_po_amd._lib import GymPoError
    e = make_env("hansen_m1", num_envs=64)
    n_obs = int(e.single_observation_space.n)
    uniform = np.full((n_obs, A), 1.0 / A)
    reset_obs(e)
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(4)
    with pytest.raises(GymPoError, match="without a controller"):
        e.controller_nodes
    e.set_controller(probs=uniform)
    e.rollout_controller(4)
    e.set_controller()  # removed again
    assert e.query("controller_nodes") == 0 and e.query("controller_lds") == 0
    with pytest.raises(GymPoError):
        e.rollout_controller(4)
    with pytest.raises(GymPoError):
        e.set_controller(probs=np.full((n_obs + 1, A), 1.0 / A))  # wrong n_obs
    with pytest.raises(GymPoError):
        e.set_controller(probs=np.full((n_obs, A + 1), 1.0 / (A + 1)))  # wrong action count
    with pytest.raises(GymPoError, match=r"n_nodes must be in \[1, 8\]"):
        e.set_controller(thresholds=np.full((9, n_obs, A * 9), 1 << 31, dtype=np.uint32))
    bad = controller_thresholds(uniform)
    bad[0, 7, 1], bad[0, 7, 2] = bad[0, 7, 2], bad[0, 7, 1]  # a non-monotone row
    with pytest.raises(GymPoError, match="not nondecreasing"):
        e.set_controller(thresholds=bad)
    bad = controller_thresholds(uniform)
    bad[0, 3, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError, match="not 2\\^31"):
        e.set_controller(thresholds=bad)
    e2 = make_env("hansen_m1", num_envs=64)
    e2.set_controller(probs=uniform)
    with pytest.raises(GymPoError, match="before reset"):
        e2.rollout_controller(4)
    # controller populations stay GRID-only
    with pytest.raises(GymPoError, match=r"\(-3\).*GRID only"):
        e.set_controller_population(probs=np.full((2, 1, n_obs, A, 1), 1.0 / A), group_envs=1024)
    with pytest.raises(GymPoError, match=r"\(-3\).*GRID only"):
        e.controller_scores()
    e.check()


# ------------------------------------------------------------------ the task ----
def _bfs(H, W, passable, targets):
    """Moves to the nearest target cell through passable cells, int [H * W] (-1: unreachable)."""
    dist = np.full(H * W, -1)
    frontier = [c for c in targets]
    for c in frontier:
        dist[c] = 0
    while frontier:
        nxt = []
        for c in frontier:
            r, q = divmod(c, W)
            for rr, qq in ((r - 1, q), (r, q + 1), (r + 1, q), (r, q - 1)):
                n = rr * W + qq
                if 0 <= rr < H and 0 <= qq < W and passable[n] and dist[n] < 0:
                    dist[n] = dist[c] + 1
                    nxt.append(n)
        frontier = nxt
    return dist


def _descend(H, W, dist, cell):
    """The first action of N, E, S, W that lowers `dist` from `cell` (0 where none does)."""
    r, q = divmod(cell, W)
    for a, (rr, qq) in enumerate(((r - 1, q), (r, q + 1), (r + 1, q), (r, q - 1))):
        if 0 <= rr < H and 0 <= qq < W and 0 <= dist[rr * W + qq] < dist[cell]:
            return a
    return 0


def _memory_controller(sp, swap=False):
    """probs [3, n_obs, 4, 3] over the cell_signal obs: node 0 walks to the priest area and, there, takes the node
    the signal names (1: heaven left, 2: heaven right; swapped: the other one) with the first move towards that arm;
    nodes 1 / 2 walk to the left / right area. Returns the table and the three distance maps."""
    H, W = sp.H, sp.W
    f = np.array(sp.flags)
    free = (f & FREE) != 0
    arms = (f & (LEFT | RIGHT)) != 0
    d_priest = _bfs(H, W, free & ~arms, np.flatnonzero(f & PRIEST))
    d_left = _bfs(H, W, free & ((f & RIGHT) == 0), np.flatnonzero(f & LEFT))
    d_right = _bfs(H, W, free & ((f & LEFT) == 0), np.flatnonzero(f & RIGHT))
    d_arm = (None, d_left, d_right)
    p = np.zeros((3, sp.n_obs, A, 3))
    p[:, :, 0, 0] = 1.0  # rows of obs that never occur (walls, a signal outside the priest area): any valid row
    for c in np.flatnonzero(free):
        for sig in range(3):
            o = c * 3 + sig
            p[:, o] = 0.0
            node = 0 if sig == 0 else ((3 - sig) if swap else sig)
            p[0, o, _descend(H, W, d_priest if sig == 0 else d_arm[node], c), node] = 1.0
            p[1, o, _descend(H, W, d_left, c), 1] = 1.0
            p[2, o, _descend(H, W, d_right, c), 2] = 1.0
    return p, d_priest, d_left, d_right


@pytest.mark.parametrize("swap", [False, True], ids=["memory", "swapped"])
def test_the_memory_controller_solves_the_task(swap, gpu_device):
    from gym_po_amd import HeavenHellGridEnv
    env = HeavenHellGridEnv(B, obs_type="cell_signal", **DYADIC)  # the default maze, p = 0, time_limit 500
    sp = Spec.of_env(env)
    p, d_priest, d_left, d_right = _memory_controller(sp, swap)
    env.set_controller(probs=p)
    assert env.query("controller_nodes") == 3 and env.query("controller_lds") == 0  # 3 x 480 x 48 B = 67.5 KB
    obs0 = reset_obs(env)
    out = {k: host(v) for k, v in env.rollout_controller(K).items()}
    term, rew = out["term"], out["rew"]
    assert not out["trunc"].any() and term.sum(0).min() >= 3  # every env ends at least three episodes in 48 steps
    assert (rew[term] == (-1.0 if swap else 1.0)).all()
    assert (rew[~term] == -0.25).all()  # every other step is a move: the controller never bumps a wall
    # the oracle, fed the emitted actions from the same seed, ends every episode at the same step
    ora = HeavenHellOracle(B, sp)
    key = philox_key(SEED)
    assert np.array_equal(ora.reset(ora.philox_draws(0, key)), obs0)
    start0, side0 = ora.agent.copy(), ora.side.copy()
    want, m = oracle_rollout(ora, out["actions"], lambda k: ora.philox_draws(k + 1, key))
    for name, y in zip(("obs", "rew", "term", "trunc"), want):
        assert np.array_equal(out[name], y), name
    got = env.metrics()
    assert {k: got[k] for k in m} == m and m["episodes"] == int(term.sum())
    # the first episode of every env lasts the breadth-first distances: start -> priest area -> the arm walked to
    first = term.argmax(0) + 1
    entry = {119: 55, 120: 56}  # the priest cell straight above each start cell, 4 moves away
    assert d_priest[119] == d_priest[120] == 4
    walks_left = (side0 == 0) != swap
    arm = np.where(walks_left, d_left[[entry[s] for s in start0]], d_right[[entry[s] for s in start0]])
    assert np.array_equal(first, 4 + arm) and set(np.unique(first)) == {9, 10}  # the near arm and the far one
    # the nodes: 0 until the priest area, then the node the signal named until the episode's end
    nodes = out["nodes"]
    assert not nodes[:5].any()
    named = np.where(walks_left, 1, 2)
    assert (nodes[5] == named).all() and (nodes[8] == named).all()
    env.check()
