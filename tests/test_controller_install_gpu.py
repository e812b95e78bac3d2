"""GPU tests of what the six kinds with closed-loop rollouts share (csrc/gp_ctrl.h CtrlHost and the device helpers;
csrc/gp_common.h load4 / store4): installing, refusing and removing a controller, the node plane, and the pick itself
under a deterministic controller, the same checks for GRID, RockSample, Ant-Tag, Taxi, Heaven-Hell and C-ROOMS.

B = 1029 envs = one full 1,024-env tile and a ragged 5, so that both the quad path and the element path of the 4-env
accesses run and every uint8 plane of step k >= 1 starts off a 4-byte boundary; K = 3 steps; M = 2 nodes. RockSample
(A = 13), Ant-Tag and Taxi (A = 5) have rows of L = A M entries that are no multiple of 4, which the library pads;
the other three have whole 16-B quads. time_limit = 2 truncates every episode inside the K steps.

The controller is deterministic: row (node, obs) puts all its mass on one joint choice j = J[node, obs], so whatever
the draw, action = j // M and next node = j % M (0 once the episode ended). That needs no oracle and holds in every
kind; it is run with the table read from global memory (ctrl_lds_max = 0) and at the default budget (staged in LDS by
the kinds that stage), and both runs must agree bit for bit.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, K, M, TL, SEED = 1029, 3, 2, 2, 7
TOP = 1 << 31
GP_E_INVALID = -1
NAMES = ("obs", "actions", "nodes", "rew", "term", "trunc")
ROCKS_8 = ((0, 0), (0, 6), (1, 3), (2, 2), (2, 5), (3, 0), (4, 4), (4, 6))
# kind -> (the rows are padded to 16-B quads by the library, this table is staged in LDS at the default budget).
# RockSample and Ant-Tag never stage; Taxi's M = 2 table (320 obs x 2 nodes x 12 entries = 30,720 B after padding) and
# its own tables exceed the 32 KB budget together, so it reads this table from global memory under both settings.
KINDS = {"grid": (0, 1), "rocksample": (1, 0), "anttag": (1, 0), "taxi": (1, 0), "heavenhell": (0, 1), "crooms": (0, 1)}


def make_env(kind):
    import gym_po_amd as g
    if kind == "grid":
        return g.MultistoryFourRoomsEnv(B, obs_type="hansen", time_limit=TL, rng_mode="philox")
    if kind == "rocksample":
        return g.RockSample(B, map_size=(7, 7), rocks=ROCKS_8, init_pos=(3, 1), obs_type="sensor", time_limit=TL)
    if kind == "anttag":
        return g.AntTagGridEnv(B, size=4, min_distance=2.0, time_limit=TL, obs_type="index")
    if kind == "taxi":
        return g.TaxiVecEnv(B, hansen_obs=True, time_limit=TL, rng_mode="philox")
    if kind == "heavenhell":
        return g.HeavenHellGridEnv(B, time_limit=TL)
    return g.CRoomsEnv(B, layout="1", action_type="cardinal", obs_type="hansen", time_limit=TL)


def joint_choice(n_obs, A):
    """J[node, obs]: the one joint choice of each row, covering every action and both next nodes."""
    n, o = np.meshgrid(np.arange(M), np.arange(n_obs), indexing="ij")
    return (3 * n + 5 * o + 1) % (A * M)


def deterministic_thresholds(J, L):
    """Row entries below j are 0 (every draw reaches them), the others 2^31 (none does): the count is j."""
    return np.where(np.arange(L)[None, None, :] < J[:, :, None], 0, TOP).astype(np.uint32)


def host(x):
    return x.cpu().numpy()


class Run:
    """One kind under one table placement, run once and shared (left unchanged) by the tests that read it."""

    def __init__(self, kind, lds_max):
        from gym_po_amd._lib import debug_knobs
        self.env = e = make_env(kind)
        self.A, self.n_obs = int(e.single_action_space.n), int(e._controller_n_obs())
        self.J = joint_choice(self.n_obs, self.A)
        self.thr = deterministic_thresholds(self.J, self.A * M)
        if lds_max is None:
            e.set_controller(thresholds=self.thr)
        else:
            with debug_knobs(ctrl_lds_max=lds_max):
                e.set_controller(thresholds=self.thr)
        self.staged = e.query("controller_lds")
        self.nodes_installed = host(e.controller_nodes)
        first = e.reset(seed=SEED)
        self.obs0 = host(first[0] if isinstance(first, tuple) else first)  # (CRoomsEnv.reset returns the obs alone)
        self.out = {k: host(v) for k, v in e.rollout_controller(K).items()}
        self.final_nodes = host(e.controller_nodes)
        e.check()


_RUNS = {}


def get_run(kind, lds_max=None):
    if (kind, lds_max) not in _RUNS:
        _RUNS[kind, lds_max] = Run(kind, lds_max)
    return _RUNS[kind, lds_max]


@pytest.fixture(params=sorted(KINDS))
def kind(request, gpu_device):
    return request.param


def test_rows_and_placements_cover_the_shared_paths(kind):
    padded, stages = KINDS[kind]
    run = get_run(kind)
    assert ((run.A * M) % 4 != 0) == bool(padded)
    assert run.staged == stages and get_run(kind, 0).staged == 0
    assert run.env.query("controller_nodes") == M


@pytest.mark.parametrize("lds_max", [0, None], ids=["global", "default"])
def test_deterministic_controller_picks_its_choice(kind, lds_max):
    run = get_run(kind, lds_max)
    o = run.out
    assert o["actions"].shape == (K, B) and o["nodes"].shape == (K, B) and o["obs"].shape == (K, B)
    assert not run.nodes_installed.any()  # set_controller: every node 0
    assert not o["nodes"][0].any()  # reset() left them 0
    obs_before = np.concatenate([run.obs0[None], o["obs"][:-1]]).astype(np.int64)
    assert obs_before.min() >= 0 and obs_before.max() < run.n_obs
    j = run.J[o["nodes"].astype(np.int64), obs_before]
    assert np.array_equal(o["actions"], j // M)
    done = o["term"] | o["trunc"]
    assert done.any() and not done.all()
    nxt = np.where(done, 0, j % M)
    assert np.array_equal(o["nodes"][1:], nxt[:-1])
    assert np.array_equal(run.final_nodes, nxt[-1])
    assert nxt.any()  # (node 1 is reached: the next-node half of j is exercised)


def test_table_placements_agree(kind):
    a, b = get_run(kind, 0), get_run(kind)
    assert np.array_equal(a.obs0, b.obs0)
    for name in NAMES:
        assert np.array_equal(a.out[name], b.out[name]), name
    assert np.array_equal(a.final_nodes, b.final_nodes)


def test_refused_tables_leave_the_controller(kind):
    from gym_po_amd import _lib
    run = get_run(kind)
    e, L = run.env, run.A * M
    fn = _lib.lib().gp_set_controller

    def refused(n_nodes, thr):
        thr = np.ascontiguousarray(thr, dtype=np.uint32)
        assert fn(e._handle, n_nodes, run.n_obs, ctypes.c_void_p(thr.ctypes.data)) == GP_E_INVALID
        return _lib.lib().gp_last_error().decode()

    for n_nodes in (0, 9):
        assert refused(n_nodes, run.thr) == (f"gp_set_controller: n_nodes must be in [1, 8] and n_obs in [1, 2^24] "
                                             f"(got {n_nodes}, {run.n_obs})")
    down = run.thr.copy()
    down[1, 2, :] = TOP
    down[1, 2, 1] = 5  # after a first entry of 2^31
    assert refused(M, down) == ("gp_set_controller: row (node 1, obs 2) is not nondecreasing within [0, 2^31] at "
                                "entry 1")
    short = run.thr.copy()
    short[0, 1, :] = 5
    assert refused(M, short) == "gp_set_controller: row (node 0, obs 1) ends at 5, not 2^31"
    assert e.query("controller_nodes") == M  # what was installed stays
    assert np.array_equal(host(e.controller_nodes), run.final_nodes)


def test_node_plane_round_trip_reset_and_removal(kind):
    from gym_po_amd._lib import GymPoError
    e = make_env(kind)
    run = get_run(kind)
    e.set_controller(thresholds=run.thr)
    want = (np.arange(B) % M).astype(np.uint8)
    e.controller_nodes = want
    assert np.array_equal(host(e.controller_nodes), want)
    e.reset(seed=SEED)
    assert not host(e.controller_nodes).any()
    e.set_controller()
    assert e.query("controller_nodes") == 0
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(1)
