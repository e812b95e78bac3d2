"""GPU tests of the controller statistics (NativeVecEnv.controller_statistics / gp_controller_stats): visit counts and
fixed-point return-to-go sums per controller table cell, accumulated on the device in one launch. Every equality is
exact (int64 arrays, array_equal) against the numpy restatement tests/controller_stats_oracle.py.

The kernel reads only planes, so the extremes come from a numpy generator: B = 3,075 envs = three full 1,024-env tiles
and one with a single live thread holding 3 envs; B is odd, so the 16-B accesses alternate with the element-wise
ones from row to row, and buffers offset by one element take the misaligned path in every row. Rewards are
full-mantissa random float32 of both signs (a contracted multiply-add would show as a mismatch), -0.0 and denormals.
The real planes come from rollout_controller(48) under time_limit = 20: at least two episode ends per env.
"""
import contextlib
import ctypes

import numpy as np
import pytest

from controller_stats_oracle import controller_stats, returns_to_go
from fixtures import load_index
from gym_po_amd.controller import q_estimate

pytestmark = pytest.mark.gpu

INDEX = load_index()["cases"]
NAMES = ("obs", "actions", "nodes", "rew", "term", "trunc")
STATE, INVALID, UNSUPPORTED, DEVICE = r"\(-4\)", r"\(-1\)", r"\(-3\)", r"\(-5\)"
MID = ("L..P..R",
       "L.PPP.R",
       "##...##",
       "##.S.##",
       "##S..##")
ROCKS_3 = ((0, 3), (2, 1), (3, 2))


# ------------------------------------------------------------------ envs ----
def fourrooms(num_envs, **kw):
    from gym_po_amd import MultistoryFourRoomsEnv
    args = dict(INDEX["fr_hansen_tl20"]["kwargs"])
    args.update(kw)
    return MultistoryFourRoomsEnv(num_envs, **args, rng_mode="philox")


def heavenhell(num_envs, obs_type="hansen_signal"):
    from gym_po_amd import HeavenHellGridEnv
    return HeavenHellGridEnv(num_envs, maze=MID, obs_type=obs_type, action_failure_probability=1 / 3, time_limit=20,
                             heaven_reward=1.0, hell_reward=-1.0, step_reward=-0.1, wall_reward=-0.3)


def rocksample(num_envs):
    from gym_po_amd import RockSample
    return RockSample(num_envs, map_size=(4, 4), rocks=ROCKS_3, init_pos=(1, 0), time_limit=20)


def taxi(num_envs, **kw):
    from gym_po_amd import TaxiVecEnv
    return TaxiVecEnv(num_envs, hansen_obs=True, time_limit=20, rng_mode="philox", **kw)


def crooms(num_envs):
    from gym_po_amd import CRoomsEnv
    return CRoomsEnv(num_envs, layout="1", time_limit=20, action_type="cardinal", obs_type="hansen",
                     step_reward=-0.1, wall_reward=-0.3, goal_reward=1.0)


def shape_of(env):
    return int(env._controller_n_obs()), int(env.single_action_space.n)


def install_uniform(env, M):
    n_obs, A = shape_of(env)
    env.set_controller(probs=np.full((M, n_obs, A, M), 1.0 / (A * M)))
    return n_obs, A


def random_probs(M, n_obs, A, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, A - 1, M - 1] += 0.05
    return p / p.sum((-1, -2), keepdims=True)


def host(x):
    return x.cpu().numpy()


def reset_obs(env, seed=11):
    r = env.reset(seed=seed)
    return r[0] if isinstance(r, tuple) else r


def dev(a, off=0):
    """The array on the device, as a view `off` elements into its allocation (off = 1: off every 4- and 16-B
    boundary the allocation has)."""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    flat[off:] = t.reshape(-1).to("cuda")
    return flat[off:].view(t.shape)


@contextlib.contextmanager
def lds_knob(value):
    from gym_po_amd._lib import debug_knobs
    if value is None:
        yield
    else:
        with debug_knobs(stats_lds_max=value):
            yield


# ------------------------------------------------------------------ synthetic planes ----
def random_rewards(rng, shape):
    """Full-mantissa float32 of both signs with magnitudes in [2^-20, 2^9), 5 % -0.0 and 5 % denormals."""
    sign = rng.integers(0, 2, shape).astype(np.uint32) << np.uint32(31)
    expo = rng.integers(127 - 20, 127 + 9, shape).astype(np.uint32) << np.uint32(23)
    mant = rng.integers(0, 1 << 23, shape).astype(np.uint32)
    pick = rng.random(shape)
    bits = np.where(pick < 0.05, np.uint32(0x80000000), np.where(pick < 0.10, sign | mant, sign | expo | mant))
    return bits.astype(np.uint32).view(np.float32)


def synth(seed, K, B, M, n_obs, A, ended="mixed", bootstrap=True):
    rng = np.random.default_rng(seed)
    planes = dict(obs=rng.integers(0, n_obs, (K, B)).astype(np.int32),
                  actions=rng.integers(0, A, (K, B)).astype(np.int32),
                  nodes=rng.integers(0, M, (K, B)).astype(np.uint8), rew=random_rewards(rng, (K, B)))
    if ended == "all":
        planes["term"], planes["trunc"] = rng.random((K, B)) < 0.5, np.ones((K, B), dtype=bool)
    elif ended == "none":
        planes["term"], planes["trunc"] = np.zeros((K, B), dtype=bool), np.zeros((K, B), dtype=bool)
    else:
        planes["term"], planes["trunc"] = rng.random((K, B)) < 0.1, rng.random((K, B)) < 0.1
    obs0 = rng.integers(0, n_obs, B).astype(np.int32)
    nn = rng.integers(0, M, B).astype(np.uint8)
    boot = random_rewards(rng, B) if bootstrap else None
    return planes, obs0, nn, boot


def device_stats(env, planes, obs0, nn, gamma, boot, off=0, into=None, knob=None):
    with lds_knob(knob):
        out = env.controller_statistics({k: dev(planes[k], off) for k in NAMES}, dev(obs0, off), dev(nn, off),
                                        gamma=gamma, bootstrap=None if boot is None else dev(boot, off), into=into)
    return host(out["counts"]), host(out["ret_q"])


_ENVS = {}


def syn_env(name):
    """(env with a uniform controller installed and never reset, M, n_obs, A), made once."""
    if name not in _ENVS:
        make, M = {"rocksample": (lambda: rocksample(3075), 3),
                   "heavenhell": (lambda: heavenhell(3075, "cell_signal"), 2),
                   "hh64": (lambda: heavenhell(64), 2), "fr_m1": (lambda: fourrooms(2051), 1),
                   "fr_m4": (lambda: fourrooms(2051), 4), "hh_m2": (lambda: heavenhell(2051), 2)}[name]
        env = make()
        n_obs, A = install_uniform(env, M)
        _ENVS[name] = (env, M, n_obs, A)
    return _ENVS[name]


@pytest.mark.parametrize("ended,bootstrap,gamma,off", [("all", True, 0.95, 1), ("none", False, 1.0, 0),
                                                        ("none", True, 0.95, 1), ("mixed", True, 0.95, 0),
                                                        ("mixed", False, 1.0, 1), ("mixed", True, 1.0, 1)])
@pytest.mark.parametrize("name", ["rocksample", "heavenhell"])
def test_synthetic_planes(gpu_device, name, ended, bootstrap, gamma, off):
    env, M, n_obs, A = syn_env(name)
    assert A == {"rocksample": 8, "heavenhell": 4}[name]
    K, B = 37, 3075
    planes, obs0, nn, boot = synth(7, K, B, M, n_obs, A, ended, bootstrap)
    counts, ret_q = device_stats(env, planes, obs0, nn, gamma, boot, off)
    wc, wq, flagged = controller_stats(M, n_obs, A, obs0, planes, nn, gamma, boot)
    assert not flagged
    assert counts.shape == (M, n_obs, A, M + 1) and counts.dtype == np.int64 and ret_q.dtype == np.int64
    assert np.array_equal(counts, wc)
    assert np.array_equal(ret_q, wq)
    assert counts.sum() == K * B
    if ended == "all":
        assert counts[..., :M].sum() == 0
    env.check()


def test_one_step_and_no_step(gpu_device):
    env, M, n_obs, A = syn_env("hh64")
    planes, obs0, nn, boot = synth(3, 1, 64, M, n_obs, A, "mixed", True)  # K = 1: only obs0 and next_nodes are read
    planes["obs"][:] = -7  # the obs after the last step is never read
    counts, ret_q = device_stats(env, planes, obs0, nn, 0.95, boot)
    ok_planes = dict(planes, obs=np.zeros_like(planes["obs"]))
    wc, wq, flagged = controller_stats(M, n_obs, A, obs0, ok_planes, nn, 0.95, boot)
    assert not flagged and np.array_equal(counts, wc) and np.array_equal(ret_q, wq) and counts.sum() == 64
    empty, obs0, nn, boot = synth(3, 0, 64, M, n_obs, A)
    c0, q0 = device_stats(env, empty, obs0, nn, 0.95, boot)
    assert c0.shape == counts.shape and not c0.any() and not q0.any()
    env.check()


# ------------------------------------------------------------------ the two paths ----
@pytest.mark.parametrize("name,default_lds,cells", [("hh_m2", 1, 2 * 48 * 4 * 3), ("fr_m1", 1, 405 * 4 * 2),
                                                     ("fr_m4", 0, 4 * 405 * 4 * 5)])
def test_lds_path_equals_global_path(gpu_device, name, default_lds, cells):
    """hh_m2 (13.5 KiB of LDS) and fr_m1 (38 KiB) fit the default budget of 40 KiB, FourRooms Hansen-4 with M = 4
    (380 KiB) fits no budget: the knob's 60 KB included."""
    env, M, n_obs, A = syn_env(name)
    assert M * n_obs * A * (M + 1) == cells
    K, B = 16, 2051
    planes, obs0, nn, boot = synth(9, K, B, M, n_obs, A)
    want = controller_stats(M, n_obs, A, obs0, planes, nn, 0.95, boot)[:2]
    got = {}
    for knob, lds in ((None, default_lds), (0, 0), (12 * cells - 1, 0), (12 * cells, int(12 * cells <= 60 * 1024)),
                      (1 << 20, default_lds)):
        got[knob] = device_stats(env, planes, obs0, nn, 0.95, boot, knob=knob)
        assert env.query("stats_lds") == lds, knob
        assert np.array_equal(got[knob][0], want[0]) and np.array_equal(got[knob][1], want[1]), knob
    env.check()


# ------------------------------------------------------------------ real planes ----
REAL = {"fr_m1": (lambda: fourrooms(2051), 1), "fr_m3": (lambda: fourrooms(2051), 3),
        "hh_m3": (lambda: heavenhell(2051), 3), "taxi_m2": (lambda: taxi(2051), 2), "crooms_m2": (lambda: crooms(1027), 2)}


class Run:
    """One closed-loop run of 48 steps, made once and shared (left unchanged) by the tests that read it."""
    K = 48

    def __init__(self, name):
        make, self.M = REAL[name]
        self.env = env = make()
        self.n_obs, self.A = shape_of(env)
        env.set_controller(probs=random_probs(self.M, self.n_obs, self.A, seed=5))
        self.obs0_dev = reset_obs(env)
        self.out_dev = env.rollout_controller(self.K)
        stats = env.controller_statistics(self.out_dev, self.obs0_dev, gamma=0.95)  # next_nodes: the nodes now
        self.counts, self.ret_q = host(stats["counts"]), host(stats["ret_q"])
        self.final_nodes = host(env.controller_nodes)
        self.obs0 = host(self.obs0_dev).astype(np.int64)
        self.out = {k: host(v) for k, v in self.out_dev.items()}
        env.check()


_RUNS = {}


def get_run(name):
    if name not in _RUNS:
        _RUNS[name] = Run(name)
    return _RUNS[name]


@pytest.mark.parametrize("name", sorted(REAL))
def test_real_planes(gpu_device, name):
    r = get_run(name)
    M, K, B = r.M, r.K, r.env.num_envs
    wc, wq, flagged = controller_stats(M, r.n_obs, r.A, r.obs0, r.out, r.final_nodes, 0.95)
    assert not flagged
    assert np.array_equal(r.counts, wc)
    assert np.array_equal(r.ret_q, wq)
    ended = r.out["term"] | r.out["trunc"]
    assert ended.sum() >= 2 * B  # time_limit = 20 inside 48 steps
    assert r.counts.sum() == K * B
    assert r.counts[..., M].sum() == ended.sum()
    hist = np.zeros((M, r.n_obs, r.A), dtype=np.int64)
    before = np.concatenate([r.obs0[None], r.out["obs"][:-1].astype(np.int64)])
    np.add.at(hist, (r.out["nodes"].astype(np.int64), before, r.out["actions"].astype(np.int64)), 1)
    assert np.array_equal(r.counts.sum(axis=-1), hist)


def test_split_equals_whole(gpu_device):
    """Two calls on the halves of the run, the later half first, into the same tables: the earlier half's bootstrap
    is the later half's return-to-go at its first step, and its next_nodes the nodes plane's row 24."""
    r = get_run("hh_m3")
    H = r.K // 2
    G = returns_to_go(r.out["rew"], r.out["term"], r.out["trunc"], 0.95)
    later = {k: v[H:] for k, v in r.out.items()}
    earlier = {k: v[:H] for k, v in r.out.items()}
    import torch
    into = {n: torch.zeros(r.counts.shape, dtype=torch.int64, device="cuda") for n in ("counts", "ret_q")}
    device_stats(r.env, later, r.out["obs"][H - 1], r.final_nodes, 0.95, None, into=into)
    counts, ret_q = device_stats(r.env, earlier, r.obs0.astype(np.int32), r.out["nodes"][H], 0.95, G[H], into=into)
    assert np.array_equal(counts, r.counts)
    assert np.array_equal(ret_q, r.ret_q)
    r.env.check()


# ------------------------------------------------------------------ populations ----
@pytest.mark.parametrize("B,G,M,lds", [(3075, 1024, 1, 1), (3075, 1024, 2, 0), (4099, 2048, 1, 1)])
def test_population_tables(gpu_device, B, G, M, lds):
    """GRID populations: env e belongs to controller e // G. B = 3,075 with G = 1,024: four controllers, the last
    block with one live thread. Table p equals the single-controller statistics of that group's slice."""
    env = fourrooms(B)
    n_obs, A = shape_of(env)
    P = -(-B // G)
    env.set_controller_population(probs=np.stack([random_probs(M, n_obs, A, seed=40 + p) for p in range(P)]),
                                  group_envs=G, gamma=0.95)
    obs0 = reset_obs(env)
    out = env.rollout_controller(24)
    stats = env.controller_statistics(out, obs0, gamma=0.95)
    assert env.query("stats_lds") == lds
    counts, ret_q = host(stats["counts"]), host(stats["ret_q"])
    assert counts.shape == (P, M, n_obs, A, M + 1)
    o, obs0, nn = {k: host(v) for k, v in out.items()}, host(obs0), host(env.controller_nodes)
    for p in range(P):
        s = slice(p * G, min((p + 1) * G, B))
        wc, wq, flagged = controller_stats(M, n_obs, A, obs0[s], {k: v[:, s] for k, v in o.items()}, nn[s], 0.95)
        assert not flagged and wc.sum() == 24 * (s.stop - s.start)
        assert np.array_equal(counts[p], wc), p
        assert np.array_equal(ret_q[p], wq), p
    wc, wq, _ = controller_stats(M, n_obs, A, obs0, o, nn, 0.95, P=P, G_envs=G)
    assert np.array_equal(counts, wc) and np.array_equal(ret_q, wq)
    env.check()


# ------------------------------------------------------------------ bad visits ----
BAD = {"obs_high": ("obs", 1, "n_obs"), "obs_negative": ("obs", 1, -1), "action_high": ("actions", 2, "A"),
       "action_negative": ("actions", 2, -3), "node": ("nodes", 0, "M"), "next_node": ("next_nodes", None, "M"),
       "inf": ("rew", 3, np.inf), "nan": ("rew", 3, np.nan), "huge": ("rew", 3, 1e38)}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_visits_are_skipped_and_flagged(gpu_device, case):
    from gym_po_amd._lib import GymPoError
    env, M, n_obs, A = syn_env("hh64")
    K, B, e = 5, 64, 37
    planes, obs0, nn, boot = synth(21, K, B, M, n_obs, A, "mixed", True)
    planes["term"][:, e] = planes["trunc"][:, e] = False  # env e: no step ends, so every visit has a next node
    clean_c, clean_q, flagged = controller_stats(M, n_obs, A, obs0, planes, nn, 0.95, boot)
    assert not flagged
    what, k, value = BAD[case]
    value = {"n_obs": n_obs, "A": A, "M": M}.get(value, value)
    if what == "next_nodes":
        nn[e] = value
    else:
        planes[what][k, e] = value
    env.seed(5)
    env.check()
    counts, ret_q = device_stats(env, planes, obs0, nn, 0.95, boot)
    wc, wq, flagged = controller_stats(M, n_obs, A, obs0, planes, nn, 0.95, boot)
    assert flagged
    assert np.array_equal(counts, wc) and np.array_equal(ret_q, wq)
    gone = clean_c - counts
    if what in ("obs", "actions", "next_nodes"):  # exactly that visit is absent, every other cell is unchanged
        assert gone.sum() == 1 and gone.min() == 0 and gone.max() == 1
        kv = k + 1 if what == "obs" else (K - 1 if k is None else k)  # obs[k] conditions step k + 1
        before = obs0[e] if kv == 0 else synth(21, K, B, M, n_obs, A, "mixed", True)[0]["obs"][kv - 1, e]
        assert gone[int(planes["nodes"][kv, e]), int(before)].sum() == 1
    elif what == "nodes":  # step 0 has no predecessor whose next node it would be
        assert gone.sum() == 1
    else:  # the return-to-go of step 3 and of every step before it in that env (none ends) is not below 2^31
        assert gone.sum() == 4 and (gone >= 0).all()
    others = np.ones(B, dtype=bool)
    others[e] = False
    sub = {k_: v[:, others] for k_, v in planes.items()}
    oc, oq, _ = controller_stats(M, n_obs, A, obs0[others], sub, nn[others], 0.95, boot[others])
    assert (counts - oc).sum() == K - gone.sum() and ((counts - oc) >= 0).all()  # the other envs' cells are whole
    with pytest.raises(GymPoError, match=DEVICE):
        env.check()
    env.seed(6)  # a re-seed clears the flag
    env.check()


# ------------------------------------------------------------------ errors ----
def raw_call(env, K, B, gamma=1.0, counts_off=0, shape=None):
    """gp_controller_stats through ctypes with valid zeroed planes; counts offset by `counts_off` bytes."""
    import torch
    from gym_po_amd._lib import lib
    z = lambda dt, *s: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    bufs = [z(torch.int32, B), z(torch.int32, K, B), z(torch.int32, K, B), z(torch.uint8, K, B), z(torch.uint8, B),
            z(torch.float32, K, B), z(torch.uint8, K, B), z(torch.uint8, K, B)]
    n = int(np.prod(shape)) if shape else 16
    counts, ret_q = z(torch.int64, n + 1), z(torch.int64, n + 1)
    p = [ctypes.c_void_p(b.data_ptr()) for b in bufs]
    rc = lib().gp_controller_stats(env._handle, K, *p, None, gamma, ctypes.c_void_p(counts.data_ptr() + counts_off),
                                   ctypes.c_void_p(ret_q.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, counts


def test_errors(gpu_device):
    import torch
    from gym_po_amd import CarVecEnv
    from gym_po_amd._lib import GymPoError
    K, B = 4, 64
    env = heavenhell(B)
    planes, obs0, nn, boot = synth(1, K, B, 2, 48, 4)
    d = {k: dev(v) for k, v in planes.items()}
    with pytest.raises(GymPoError, match=STATE):  # no controller installed
        env.controller_statistics(d, dev(obs0), dev(nn))
    assert raw_call(env, K, B)[0] == -4
    M, (n_obs, A) = 2, install_uniform(env, 2)
    shape = (M, n_obs, A, M + 1)
    rc, counts = raw_call(env, K, B, shape=shape)
    assert rc == 0 and int(counts.sum()) == K * B
    for gamma in (0.0, 1.5, -0.5, float("nan")):
        with pytest.raises(GymPoError, match=INVALID + ".*gamma"):
            env.controller_statistics(d, dev(obs0), dev(nn), gamma=gamma)
        assert raw_call(env, K, B, gamma=gamma, shape=shape)[0] == -1
    rc, counts = raw_call(env, K, B, counts_off=4, shape=shape)  # misaligned tables
    assert rc == -1 and int(counts.sum()) == 0
    car = CarVecEnv(B)
    assert raw_call(car, K, B)[0] == -3
    with pytest.raises(GymPoError, match=UNSUPPORTED):
        car.controller_statistics(d, dev(obs0), dev(nn))
    # Python-side argument checks
    bad = [dict(d, actions=d["actions"][:, :-1]), dict(d, actions=d["actions"].long()),
           dict(d, nodes=d["nodes"].int()), dict(d, rew=d["rew"].double()), dict(d, term=d["term"].float()),
           {k: v for k, v in d.items() if k != "trunc"}, dict(d, obs=d["obs"][:, :, None].expand(K, B, 3))]
    for p in bad:
        with pytest.raises(ValueError):
            env.controller_statistics(p, dev(obs0), dev(nn))
    with pytest.raises(ValueError):
        env.controller_statistics(d, dev(obs0)[:-1], dev(nn))
    with pytest.raises(ValueError):
        env.controller_statistics(d, dev(obs0), dev(nn).int())
    with pytest.raises(ValueError):
        env.controller_statistics(d, dev(obs0), dev(nn), bootstrap=dev(boot).double())
    with pytest.raises(ValueError):
        env.controller_statistics(d, dev(obs0), dev(nn), into={"counts": torch.zeros(shape, dtype=torch.int64,
                                                                                     device="cuda")})
    with pytest.raises(ValueError):
        z = torch.zeros((M, n_obs, A, M), dtype=torch.int64, device="cuda")
        env.controller_statistics(d, dev(obs0), dev(nn), into={"counts": z, "ret_q": z.clone()})
    # integer and float obs of another dtype are cast
    got = env.controller_statistics(dict(d, obs=d["obs"].double()), dev(obs0).long(), dev(nn))
    want = env.controller_statistics(d, dev(obs0), dev(nn))
    assert torch.equal(got["counts"], want["counts"]) and int(want["counts"].sum()) == K * B
    # a one-hot Taxi obs plane
    hot = taxi(B, one_hot=True)
    install_uniform(hot, 1)
    obs0h = reset_obs(hot)
    out = hot.rollout_controller(3)
    assert out["obs"].ndim == 3
    with pytest.raises(ValueError, match="one-hot"):
        hot.controller_statistics(out, obs0h)
    env.check()


# ------------------------------------------------------------------ use ----
def test_monte_carlo_policy_improvement(gpu_device):
    """One step of Monte Carlo policy improvement from the statistics of a uniform memoryless policy: the greedy
    policy ends episodes sooner and more often at the goal. Measured: mean episode length 87.76 ->
    11.77, terminated share of the episode ends 0.2103 -> 0.9786."""
    from gym_po_amd import RoomsEnv
    B, K = 4096, 256

    def run(probs):
        env = RoomsEnv(B, layout="1", obs_type="mdp", action_type="cardinal", action_failure_probability=0.0,
                       time_limit=100, rng_mode="philox")
        env.set_controller(probs=probs)
        obs0 = reset_obs(env, seed=2)
        out = env.rollout_controller(K)
        stats = env.controller_statistics(out, obs0, gamma=0.99)
        m = env.metrics()
        term, ended = host(out["term"]), host(out["term"] | out["trunc"])
        return stats, m["length_sum"] / m["episodes"], term.sum() / ended.sum(), env

    probe = RoomsEnv(1, layout="1", obs_type="mdp", action_type="cardinal", rng_mode="philox")
    n_obs, A = shape_of(probe)
    uniform = np.full((n_obs, A), 1.0 / A)
    stats, len_u, share_u, _ = run(uniform)
    counts, ret_q = host(stats["counts"]), host(stats["ret_q"])
    assert counts.shape == (1, n_obs, A, 2) and counts.sum() == K * B
    q = q_estimate(counts.sum(-1), ret_q.sum(-1))[0]  # [n_obs, A]: both columns of a choice together
    greedy = uniform.copy()
    seen = ~np.isnan(q).any(-1)  # cells never visited keep the uniform row
    greedy[seen] = np.eye(A)[np.argmax(q[seen], axis=-1)]
    _, len_g, share_g, env = run(greedy)
    print(f"mean episode length {len_u:.3f} -> {len_g:.3f}, terminated share {share_u:.4f} -> {share_g:.4f}")
    assert len_g < len_u and share_g > share_u
    env.check()
