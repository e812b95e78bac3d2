"""GPU tests of the closed-loop rollouts on the tabular POMDP (csrc/pomdp.hip pd_rollout<true, ., .>): a K-step launch
whose actions the device draws from a tabular finite-state controller must equal the open-loop rollout() of those
actions on a twin env bit for bit (outputs, final state, metrics), and the actions and nodes it emits must equal the
numpy restatement of the controller (tests/controller_oracle.py, which is not env-specific) run over the obs stream it
emitted; the env itself equals tests/pomdp_oracle.py fed the emitted actions.

A = 3 (Tiger, m37): rows of L = 3 M entries are padded to 16-B quads; M = 1, 3, 8. A M = 64 is accepted, 65 refused. The
controller table in LDS or in global memory, with the model blob in LDS or in global memory: all four kernel instances
give the same bits. B = 1,027 envs = two 1,024-env tiles, the last one ragged; K = 40 steps under time_limit = 7.

Use: grid Heaven-Hell's default maze lowered to tables by `heaven_hell_pomdp`, under the 3-node breadth-first controller
of tests/test_heavenhell_controller_gpu.py, earns +1 in every finished episode, its node-swapped twin -1; Tiger under
"listen twice, open on agreement", written by hand.
"""
import ctypes

import numpy as np
import pytest

from controller_oracle import controller_rollout
from controller_stats_oracle import controller_stats
from gym_po_amd.controller import controller_thresholds
from oracle.philox import philox_key
from pomdp_oracle import PomdpOracle, Spec, oracle_rollout, random_model
from test_pomdp_gpu import tables

pytestmark = pytest.mark.gpu

B, K, SEED, TL = 1027, 40, 11, 7
_EXTRA = {"a8": (2, 8, 2), "a13": (2, 13, 2)}
# name -> (model, controller nodes, the model blob is in LDS, the table is staged in LDS; under the default budgets)
CASES = {
    "tiger_m1": ("tiger", 1, 1, 1), "tiger_m3": ("tiger", 3, 1, 1), "tiger_m8": ("tiger", 8, 1, 1),
    "m5_m3": ("m5", 3, 1, 1),
    "m37_m3": ("m37", 3, 0, 1),    # the blob (48,608 B) stays in global memory; the table, 3 KB, is staged at offset 0
    "m300_m8": ("m300", 8, 0, 0),  # 8 x 70 rows of 16 entries = 35,840 B: above the 32 KB budget
    "a8_m8": ("a8", 8, 1, 1),      # A M = 64: the j / M multiply's limit
}


def model_tables(model):
    if model in _EXTRA:
        S, A, O = _EXTRA[model]
        return random_model(S, A, O, seed=A, n_terminal=0)
    return tables(model)


def make_env(name, num_envs=B, **knobs):
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import debug_knobs
    T, Z, R, start, terminal, reset_obs = model_tables(CASES[name][0])
    with debug_knobs(**knobs):
        return TabularPOMDPEnv(num_envs, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs, time_limit=TL)


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


def set_controller(env, thr, lds_max=None):
    """Install the table, under the ctrl_lds_max knob if given (gp_set_controller reads it)."""
    from gym_po_amd._lib import debug_knobs
    if lds_max is None:
        env.set_controller(thresholds=thr)
    else:
        with debug_knobs(ctrl_lds_max=lds_max):
            env.set_controller(thresholds=thr)


class Run:
    """One case, run once and shared (left unchanged) by the tests that read it. `model_lds_max` / `ctrl_lds_max`: the
    knobs pomdp_lds_max (read at gp_create) and ctrl_lds_max (read by gp_set_controller), None = the defaults."""

    def __init__(self, name, model_lds_max=None, ctrl_lds_max=None):
        self.name, self.M = name, CASES[name][1]
        self.env_knobs = {} if model_lds_max is None else dict(pomdp_lds_max=model_lds_max)
        self.ctrl_lds_max = ctrl_lds_max
        e1 = make_env(name, **self.env_knobs)
        self.n_obs, self.A = int(e1.single_observation_space.n), int(e1.single_action_space.n)
        self.thr = controller_thresholds(random_probs(self.M, self.n_obs, self.A, seed=5))
        set_controller(e1, self.thr, ctrl_lds_max)
        self.model_lds, self.lds = e1.query("pomdp_lds"), e1.query("controller_lds")
        assert e1.query("controller_nodes") == self.M
        self.obs0 = reset_obs(e1)
        self.step0 = e1.query("philox_step")
        self.out_dev = e1.rollout_controller(K)
        self.out = {k: host(v) for k, v in self.out_dev.items()}
        self.state = [host(x) for x in e1.get_state()]
        self.metrics = e1.metrics()
        self.final_nodes = host(e1.controller_nodes)
        self.step1 = e1.query("philox_step")
        self.env = e1
        e1.check()

    def twin(self):
        e = make_env(self.name, **self.env_knobs)
        set_controller(e, self.thr, self.ctrl_lds_max)
        assert np.array_equal(reset_obs(e), self.obs0)
        return e


_RUNS = {}


def get_run(name, model_lds_max=None, ctrl_lds_max=None):
    k = (name, model_lds_max, ctrl_lds_max)
    if k not in _RUNS:
        _RUNS[k] = Run(*k)
    return _RUNS[k]


@pytest.fixture(params=sorted(CASES))
def run(request, gpu_device):
    return get_run(request.param)


@pytest.fixture
def run_split(gpu_device):
    return get_run("m37_m3")


def test_closed_loop_equals_open_loop(run):
    import torch
    A, M = run.A, run.M
    assert run.thr.shape == (M, run.n_obs, A * M)
    assert (run.model_lds, run.lds) == CASES[run.name][2:]
    assert run.out["obs"].shape == (K, B) and run.out["actions"].dtype == np.int32
    assert run.out["nodes"].dtype == np.uint8
    assert run.step1 == run.step0 + K  # the counter advanced by K
    assert (run.out["term"] | run.out["trunc"]).sum(0).min() >= 5 and run.out["trunc"].any()
    e2 = make_env(run.name)
    assert np.array_equal(reset_obs(e2), run.obs0)
    obs, rew, term, trunc = e2.rollout(run.out_dev["actions"])
    for name, t in (("obs", obs), ("rew", rew), ("term", term), ("trunc", trunc)):
        assert torch.equal(t.cpu(), torch.from_numpy(run.out[name])), name
    for a, b in zip(e2.get_state(), run.state):
        assert np.array_equal(host(a), b)
    assert e2.metrics() == run.metrics
    assert run.metrics["env_steps"] == K * B and run.metrics["episodes"] >= 5 * B
    e2.check()
    # and the env is the oracle's, fed the emitted actions
    ora = PomdpOracle(B, Spec.of_env(e2))
    key = philox_key(SEED)
    assert np.array_equal(ora.reset(ora.philox_draws(0, key)), run.obs0)
    want, m = oracle_rollout(ora, run.out["actions"], lambda k: ora.philox_draws(k + 1, key))
    for name, y in zip(("obs", "rew", "term", "trunc"), want):
        assert np.array_equal(run.out[name], y), name
    assert {k: run.metrics[k] for k in m} == m


def test_actions_and_nodes_equal_the_oracle(run):
    A, M = run.A, run.M
    t = run.thr.astype(np.int64)
    assert (np.diff(t, axis=-1, prepend=0) == 0).any()  # choices of probability exactly 0: empty intervals
    acts, nodes, final = controller_rollout(run.obs0, run.out["obs"], run.out["term"], run.out["trunc"], run.thr,
                                            philox_key(SEED), run.step0)
    assert np.array_equal(run.out["actions"], acts)
    assert np.array_equal(run.out["nodes"], nodes)
    assert np.array_equal(run.final_nodes, final)
    assert run.out["actions"].min() == 0 and run.out["actions"].max() == A - 1
    assert run.out["nodes"].max() == M - 1 and run.out["obs"].max() < run.n_obs
    if M > 1:
        ended = run.out["term"][:-1] | run.out["trunc"][:-1]
        assert ended.any() and not run.out["nodes"][1:][ended].any()  # node 0 after every episode end


@pytest.mark.parametrize("name", ["m5_m3", "tiger_m8"])
def test_the_four_memory_combinations_agree(name, gpu_device):
    """Model blob in LDS / global memory (pomdp_lds_max) x controller table in LDS / global memory (ctrl_lds_max): one
    kernel instance each; every output, the state, the nodes and the metrics are the same bits."""
    base = get_run(name)
    assert (base.model_lds, base.lds) == (1, 1)
    for model_max, ctrl_max, want in ((0, None, (0, 1)), (None, 0, (1, 0)), (0, 0, (0, 0))):
        other = get_run(name, model_max, ctrl_max)
        assert (other.model_lds, other.lds) == want
        for k in ("obs", "actions", "nodes", "rew", "term", "trunc"):
            assert np.array_equal(base.out[k], other.out[k]), (want, k)
        for x, y in zip(base.state, other.state):
            assert np.array_equal(x, y)
        assert np.array_equal(base.final_nodes, other.final_nodes) and base.metrics == other.metrics


def test_table_behind_a_large_model_in_lds(gpu_device):
    """m37's blob in LDS (pomdp_lds_max raised to 60 KB) leaves the default ctrl_lds_max budget no room: the table is
    read from global memory; with ctrl_lds_max raised too it is staged behind the blob. Same bits as the default."""
    base = get_run("m37_m3")
    for ctrl_max, want in ((None, (1, 0)), (60 * 1024, (1, 1))):
        other = get_run("m37_m3", 60 * 1024, ctrl_max)
        assert (other.model_lds, other.lds) == want
        for k in ("obs", "actions", "nodes", "rew", "term", "trunc"):
            assert np.array_equal(base.out[k], other.out[k]), (want, k)
        assert np.array_equal(base.final_nodes, other.final_nodes) and base.metrics == other.metrics


def test_sixty_five_joint_choices_are_refused(gpu_device):
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import GymPoError
    T, Z, R, start, terminal, ro = model_tables("a13")
    e = TabularPOMDPEnv(64, T, Z, R, start=start, terminal=terminal, reset_obs=ro, time_limit=TL)
    with pytest.raises(GymPoError, match=r"13 actions x 5 nodes = 65 joint choices, more than 64"):
        e.set_controller(probs=np.full((5, 2, 13, 5), 1.0 / 65))
    assert e.query("controller_nodes") == 0
    e.set_controller(probs=np.full((4, 2, 13, 4), 1.0 / 52))  # 52: accepted
    assert e.query("controller_nodes") == 4 and e.query("controller_actions") == 13


def test_split_launches_equal_one_launch(run_split):
    run = run_split
    e = run.twin()
    a = {k: host(v) for k, v in e.rollout_controller(17).items()}
    _, _, nodes17 = controller_rollout(run.obs0, a["obs"], a["term"], a["trunc"], run.thr, philox_key(SEED), run.step0)
    assert np.array_equal(host(e.controller_nodes), nodes17)
    b = {k: host(v) for k, v in e.rollout_controller(23).items()}
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
    assert e.rollout_controller(K, store=()) == {}  # every output NULL
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
    M, A = 3, 2
    e = make_env("m5_m3")
    n_obs = int(e.single_observation_space.n)
    p = np.zeros((M, n_obs, A, M))
    for n in range(M):
        p[n, :, A - 1, (n + 1) % M] = 1.0  # always the last action; the node cycles 0 -> 1 -> 2 -> 0
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
    from gym_po_amd import _lib
    from gym_po_amd._lib import GymPoError
    e = make_env("m5_m3", num_envs=300)
    A = 2
    t = controller_thresholds(np.full((1, A), 1.0 / A))  # n_obs = 1: the obs 1 and 2 lie beyond it
    _lib.check(_lib.lib().gp_set_controller(e._handle, 1, 1, ctypes.c_void_p(t.ctypes.data)), "gp_set_controller")
    assert reset_obs(e).max() > 0
    out = e.rollout_controller(8)
    assert 0 <= int(out["actions"].min()) and int(out["actions"].max()) < A
    with pytest.raises(GymPoError, match=r"\(-5\)"):
        e.check()


def test_node_beyond_the_controller_is_clamped_and_flagged(gpu_device):
    """A node >= M written from a device tensor (not range-checked on the host) is clamped and flags the handle."""
    import torch
    from gym_po_amd._lib import GymPoError
    e = make_env("tiger_m3", num_envs=300)
    e.set_controller(probs=np.full((2, 2, 3, 2), 1.0 / 6))
    reset_obs(e)
    e.controller_nodes = torch.full((300,), 2, dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(4)
    assert int(out["nodes"].max()) < 2 and int(out["actions"].max()) < 3
    with pytest.raises(GymPoError, match=r"\(-5\)"):
        e.check()


def test_errors_and_populations_unsupported(gpu_device):
    from gym_po_amd._lib import GymPoError
    e = make_env("tiger_m1", num_envs=64)
    n_obs, A = 2, 3
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
    bad[0, 1, 1], bad[0, 1, 0] = bad[0, 1, 0], bad[0, 1, 1]  # a non-monotone row
    with pytest.raises(GymPoError, match=r"gp_set_controller: row \(node 0, obs 1\) is not nondecreasing"):
        e.set_controller(thresholds=bad)
    bad = controller_thresholds(uniform)
    bad[0, 1, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError, match=r"gp_set_controller: row \(node 0, obs 1\) ends at 2147483647, not 2\^31"):
        e.set_controller(thresholds=bad)
    e2 = make_env("tiger_m1", num_envs=64)
    e2.set_controller(probs=uniform)
    with pytest.raises(GymPoError, match="before reset"):
        e2.rollout_controller(4)
    # controller populations stay GRID-only
    with pytest.raises(GymPoError, match=r"\(-3\).*GRID only"):
        e.set_controller_population(probs=np.full((2, 1, n_obs, A, 1), 1.0 / A), group_envs=1024)
    with pytest.raises(GymPoError, match=r"\(-3\).*GRID only"):
        e.controller_scores()
    e.check()


def test_controller_statistics_on_the_planes(gpu_device):
    import torch
    run = get_run("m37_m3")
    stats = run.env.controller_statistics(run.out_dev, torch.from_numpy(run.obs0).to(run.env.device),
                                          torch.from_numpy(run.final_nodes).to(run.env.device), gamma=0.95)
    wc, wq, flagged = controller_stats(run.M, run.n_obs, run.A, run.obs0.astype(np.int64), run.out, run.final_nodes,
                                       0.95)
    assert not flagged
    assert np.array_equal(host(stats["counts"]), wc) and np.array_equal(host(stats["ret_q"]), wq)
    ended = run.out["term"] | run.out["trunc"]
    assert wc.sum() == K * B and wc[..., run.M].sum() == ended.sum()
    from gym_po_amd.controller import q_estimate
    q = q_estimate(stats["counts"], stats["ret_q"])
    assert q.shape == (run.M, run.n_obs, run.A, run.M + 1) and np.isfinite(q[wc > 0]).all()


# ------------------------------------------------------------------ use ----
DYADIC = dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=-0.25, wall_reward=-0.5)


@pytest.mark.parametrize("swap", [False, True], ids=["memory", "swapped"])
def test_heaven_hell_as_tables_under_the_memory_controller(swap, gpu_device):
    """The default maze at p = 0 lowered to tables (S = 320, O = 480): the 3-node controller that walks to the priest,
    takes the node the signal names and walks to that arm earns +1 in every finished episode, its node-swapped twin
    -1; the first episode lasts the breadth-first distances, as on the native env."""
    import heavenhell_oracle as hh
    from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv, heaven_hell_pomdp
    from test_heavenhell_controller_gpu import _memory_controller
    native = HeavenHellGridEnv(8, obs_type="cell_signal", **DYADIC)  # the default maze, p = 0, time_limit 500
    T, Z, R, start, terminal, ro = heaven_hell_pomdp(native)
    assert T.shape == (320, 4, 320) and Z.shape == (4, 320, 480)
    env = TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=ro, time_limit=500)
    sp = hh.Spec.of_env(native)
    p, d_priest, d_left, d_right = _memory_controller(sp, swap)
    env.set_controller(probs=p)
    assert env.query("controller_nodes") == 3 and env.query("controller_lds") == 0 and env.query("pomdp_lds") == 0
    obs0 = reset_obs(env)
    state0 = host(env.get_state()[0]).astype(np.int64)
    out = {k: host(v) for k, v in env.rollout_controller(48).items()}
    term, rew = out["term"].astype(bool), out["rew"]
    assert not out["trunc"].any() and term.sum(0).min() >= 3  # every env ends at least three episodes in 48 steps
    assert (rew[term] == (-1.0 if swap else 1.0)).all()
    assert (rew[~term] == -0.25).all()  # every other step is a move: the controller never bumps a wall
    # the oracle of the tables, fed the emitted actions from the same seed
    ora = PomdpOracle(B, Spec.of_env(env))
    key = philox_key(SEED)
    assert np.array_equal(ora.reset(ora.philox_draws(0, key)), obs0) and np.array_equal(ora.state, state0)
    want, m = oracle_rollout(ora, out["actions"], lambda k: ora.philox_draws(k + 1, key))
    for name, y in zip(("obs", "rew", "term", "trunc"), want):
        assert np.array_equal(out[name], y), name
    got = env.metrics()
    assert {k: got[k] for k in m} == m and m["episodes"] == int(term.sum())
    # the first episode of every env: start -> priest area (4 moves) -> the arm walked to
    cell0, side0 = state0 % 160, state0 // 160
    assert set(np.unique(cell0)) == {119, 120} and set(np.unique(side0)) == {0, 1}
    assert np.array_equal(obs0, cell0 * 3)
    first = term.argmax(0) + 1
    entry = {119: 55, 120: 56}
    walks_left = (side0 == 0) != swap
    arm = np.where(walks_left, d_left[[entry[int(s)] for s in cell0]], d_right[[entry[int(s)] for s in cell0]])
    assert np.array_equal(first, 4 + arm) and set(np.unique(first)) == {9, 10}
    nodes = out["nodes"]
    named = np.where(walks_left, 1, 2)
    assert not nodes[:5].any() and (nodes[5] == named).all() and (nodes[8] == named).all()
    env.check()


def test_tiger_listen_twice_open_on_agreement(gpu_device):
    """Tiger from its text, under a 4-node controller written by hand. Node 0: nothing heard (the obs is the reset's or
    the noise after a door): listen. Node 1: the obs is a first hearing: listen, and remember it (node 2: left, node 3:
    right). Node 2 / 3: the obs is a second hearing: if it agrees, open the other door (back to node 0), else listen
    again with this hearing as the first (node 2 or 3 by it)."""
    from gym_po_amd import TabularPOMDPEnv
    from pomdp_oracle import TIGER
    LISTEN, OPEN_LEFT, OPEN_RIGHT, LEFT, RIGHT = 0, 1, 2, 0, 1
    p = np.zeros((4, 2, 3, 4))
    p[0, :, LISTEN, 1] = 1.0
    p[1, LEFT, LISTEN, 2] = p[1, RIGHT, LISTEN, 3] = 1.0
    p[2, LEFT, OPEN_RIGHT, 0] = p[2, RIGHT, LISTEN, 3] = 1.0
    p[3, RIGHT, OPEN_LEFT, 0] = p[3, LEFT, LISTEN, 2] = 1.0
    env = TabularPOMDPEnv.from_pomdp(TIGER, B, time_limit=25)
    env.set_controller(probs=p)
    assert env.query("pomdp_lds") == 1 and env.query("controller_lds") == 1
    obs0 = reset_obs(env)
    out = {k: host(v) for k, v in env.rollout_controller(K).items()}
    acts, nodes, final = controller_rollout(obs0, out["obs"], out["term"], out["trunc"], controller_thresholds(p),
                                            philox_key(SEED), 1)
    assert np.array_equal(out["actions"], acts) and np.array_equal(out["nodes"], nodes)
    assert np.array_equal(host(env.controller_nodes), final)
    ora = PomdpOracle(B, Spec.of_env(env))
    key = philox_key(SEED)
    assert np.array_equal(ora.reset(ora.philox_draws(0, key)), obs0)
    tiger0 = ora.state.copy()
    tigers = [tiger0]
    want, m = oracle_rollout(ora, out["actions"], lambda k: (tigers.append(ora.state.copy()), ora.philox_draws(k + 1, key))[1])
    for name, y in zip(("obs", "rew", "term", "trunc"), want):
        assert np.array_equal(out[name], y), name
    assert {k: env.metrics()[k] for k in m} == m
    # a door is opened only on two agreeing hearings in a row, and it is the other door; the reward is the table's
    a, o, r = out["actions"], out["obs"], out["rew"]
    opened = a != LISTEN
    assert opened.any() and not opened[:2].any()
    ks, es = np.nonzero(opened)
    assert (a[ks - 1, es] == LISTEN).all() and (a[ks - 2, es] == LISTEN).all()
    assert (o[ks - 1, es] == o[ks - 2, es]).all()
    assert (a[ks, es] == np.where(o[ks - 1, es] == LEFT, OPEN_RIGHT, OPEN_LEFT)).all()
    tiger = np.stack(tigers[1:])  # the state each step started in (the list's first entry is the reset's, again)
    door = np.where(a[ks, es] == OPEN_LEFT, LEFT, RIGHT)
    assert np.array_equal(r[ks, es], np.where(door == tiger[ks, es], -100.0, 10.0).astype(np.float32))
    assert (r[~opened] == -1.0).all() and {-100.0, 10.0} <= set(np.unique(r))
