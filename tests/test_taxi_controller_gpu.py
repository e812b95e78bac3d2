"""GPU tests of the closed-loop rollouts on the Hansen Taxi (csrc/taxi.hip taxi_rollout_ctrl; philox mode, scalar and
one-hot obs): a K-step launch whose actions the device draws from a tabular finite-state controller must equal the
open-loop rollout() of those actions on a twin env bit for bit (outputs, final state, metrics), and the actions and
nodes it emits must equal the numpy restatement of the controller (tests/controller_oracle.py, not env-specific) run
over the scalar obs stream.

A = 5 is no multiple of 4, so the library pads each uploaded row to 16-B quads with 2^31. M = 1, 2, 3 give rows of
5 -> 8, 10 -> 12 and 15 -> 16 entries (the scanned path: up to 4 quads), M = 4 and 8 give 20 and 40 entries (5 and 10
quads: the searched path). Every random row puts nonzero probability on the last real joint choice: a padding entry
that was counted would show as action 5. On the 5 x 5 map the M = 1 table (10,240 B) is staged in LDS behind the env's
tables by default; larger tables, and every table on the 8 x 8 map, are read from global memory.

B = 2,051 envs = three 1,024-env tiles, the last one holding 3 live envs in one thread's quad. K = 48 steps under
time_limit = 20: an episode lasts at most 21 steps, so every env ends at least two, and an env that never terminates
ends exactly two by truncation. Everything is compared with ==; the rewards are dyadic (multiples of 0.25, |r| <= 2),
so the float64 sums of the metrics are exact in any order (other rewards: tests/test_metrics_precision_gpu.py).
"""
import contextlib
import functools

import numpy as np
import pytest

from controller_oracle import controller_rollout
from gym_po_amd.controller import controller_thresholds
from oracle.philox import philox_key
from taxi_controller_oracle import marginal_greedy_probs
from taxi_table_oracle import make_oracle, per_tile_floor, rare_rows

pytestmark = pytest.mark.gpu

B, K, SEED, TL = 2051, 48, 11, 20
A = 5
DYADIC = dict(reward_goal=2.0, reward_bad=-1.0, reward_any=-0.25)
DIRECTED = dict(map="TAXI", hansen_obs=True, num_passengers=2, time_limit=24, **DYADIC)
NAMES = ("obs", "actions", "nodes", "rew", "term", "trunc")
# name -> (map, controller nodes, num_passengers)
CASES = {
    "t5_m1": ("TAXI", 1, 1),
    "t5_m2": ("TAXI", 2, 2),
    "t5_m3": ("TAXI", 3, 1),
    "t5_m4": ("TAXI", 4, 2),
    "t5_m8": ("TAXI", 8, 2),
    "e8_m1": ("EXTENDED", 1, 2),
}


def taxi_env(kw, num_envs=B, **extra):
    from gym_po_amd import TaxiVecEnv
    from gym_po_amd.maps import EXTENDED_TAXI_MAP, TAXI_MAP
    kw = dict(kw)
    m = kw.pop("map", "TAXI")
    return TaxiVecEnv(num_envs, map=TAXI_MAP if m == "TAXI" else EXTENDED_TAXI_MAP, **kw, **extra)


def make_env(name, num_envs=B, **kw):
    m, _, npass = CASES[name]
    base = dict(map=m, hansen_obs=True, num_passengers=npass, time_limit=TL, **DYADIC)
    base.update(kw)
    return taxi_env(base, num_envs)


def random_probs(M, n_obs, A, seed):
    """Rows in which about a third of the entries are exactly 0 and the last joint choice never is."""
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, A - 1, M - 1] += 0.05
    return p / p.sum((-1, -2), keepdims=True)


@functools.lru_cache(maxsize=None)
def case_thresholds(name):
    M = CASES[name][1]
    n_obs = make_env(name, num_envs=1).no
    return controller_thresholds(random_probs(M, n_obs, A, seed=5))


def host(x):
    return x.cpu().numpy()


def scalar_obs(env, o):
    """int64 numpy obs indices of an obs tensor: the scalar obs itself, or the hot index of each one-hot row (every
    row checked on the device to hold exactly one 1)."""
    import torch
    if not env.one_hot:
        return host(o).astype(np.int64)
    assert o.shape[-1] == env.no and int(o.max()) == 1 and bool((o.sum(-1, dtype=torch.int32) == 1).all())
    return host(o.argmax(-1)).astype(np.int64)


def reset_obs(env, seed=SEED):
    return scalar_obs(env, env.reset(seed=seed)[0])


def assert_same_outputs(a, b, names=NAMES, msg=""):
    import torch
    for nm in names:
        assert torch.equal(a[nm], b[nm]), f"{nm} {msg}"


def snapshot(env):
    return dict(state=[host(x) for x in env.get_state()], nodes=host(env.controller_nodes), metrics=env.metrics(),
                step=env.query("philox_step"))


def assert_same_snapshot(env, snap, msg=""):
    for x, y in zip(env.get_state(), snap["state"]):
        assert np.array_equal(host(x), y), f"state {msg}"
    assert np.array_equal(host(env.controller_nodes), snap["nodes"]), f"nodes {msg}"
    assert env.metrics() == snap["metrics"], f"metrics {msg}"
    assert env.query("philox_step") == snap["step"], f"philox_step {msg}"


class Run:
    """One case, run once and shared (left unchanged) by the tests that read it."""

    def __init__(self, name, one_hot):
        self.name, self.one_hot, self.M = name, one_hot, CASES[name][1]
        self.thr = case_thresholds(name)
        e1 = make_env(name, one_hot=one_hot)
        self.n_obs = e1.no
        assert int(e1.single_action_space.n) == A and self.thr.shape == (self.M, self.n_obs, A * self.M)
        e1.set_controller(thresholds=self.thr)
        assert e1.query("controller_nodes") == self.M
        self.lds = e1.query("controller_lds")
        self.obs0 = reset_obs(e1)
        self.step0 = e1.query("philox_step")
        self.dev = e1.rollout_controller(K)  # device tensors, never written again
        self.obs = scalar_obs(e1, self.dev["obs"])
        self.out = {k: host(v) for k, v in self.dev.items() if k != "obs"}
        self.snap = snapshot(e1)
        e1.check()

    def twin(self, controller=True, **kw):
        e = make_env(self.name, one_hot=self.one_hot, **kw)
        if controller:
            e.set_controller(thresholds=self.thr)
        assert np.array_equal(reset_obs(e), self.obs0)
        return e


@functools.lru_cache(maxsize=None)
def get_run(name, one_hot):
    return Run(name, one_hot)


@pytest.fixture(params=[False, True], ids=["scalar", "one_hot"])
def one_hot(request):
    return request.param


@pytest.fixture(params=sorted(CASES))
def run(request, one_hot, gpu_device):
    return get_run(request.param, one_hot)


@pytest.fixture(params=["t5_m3", "t5_m8"])  # a scanned and a searched row
def run_split(request, one_hot, gpu_device):
    return get_run(request.param, one_hot)


# ------------------------------------------------------------------ closed loop == open loop ----
def test_closed_loop_equals_open_loop(run):
    import torch
    shape = (K, B, run.n_obs) if run.one_hot else (K, B)
    assert tuple(run.dev["obs"].shape) == shape
    assert run.dev["obs"].dtype == (torch.uint8 if run.one_hot else torch.int32)
    assert run.out["actions"].dtype == np.int32 and run.out["nodes"].dtype == np.uint8
    assert run.snap["step"] == run.step0 + K  # the counter advanced by K
    assert run.lds == (1 if run.name == "t5_m1" else 0)
    term, trunc = run.out["term"], run.out["trunc"]
    assert (term | trunc).sum(0).min() >= 2          # every env ended two episodes ...
    assert trunc.sum(0)[~term.any(0)].min() >= 2      # ... by truncation unless it terminated
    assert trunc.any()
    e2 = run.twin(controller=False)
    obs, rew, tm, tr = e2.rollout(run.dev["actions"])
    for nm, t in (("obs", obs), ("rew", rew), ("term", tm), ("trunc", tr)):
        assert torch.equal(t, run.dev[nm]), nm
    for a, b in zip(e2.get_state(), run.snap["state"]):
        assert np.array_equal(host(a), b)
    assert e2.metrics() == run.snap["metrics"]
    assert e2.query("philox_step") == run.snap["step"]
    e2.check()
    assert run.snap["metrics"]["env_steps"] == K * B and run.snap["metrics"]["episodes"] == (term | trunc).sum()
    assert run.snap["metrics"]["return_sum"] == float(run.out["rew"].astype(np.float64).sum())


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_hot_rows_are_the_scalar_obs(name, gpu_device):
    run, ref = get_run(name, True), get_run(name, False)
    assert np.array_equal(run.obs0, ref.obs0) and np.array_equal(run.obs, ref.obs)
    for nm in NAMES[1:]:
        assert np.array_equal(run.out[nm], ref.out[nm]), nm
    for a, b in zip(run.snap["state"], ref.snap["state"]):
        assert np.array_equal(a, b)
    assert run.snap["metrics"] == ref.snap["metrics"]


def test_actions_and_nodes_equal_the_oracle(run):
    ref = get_run(run.name, False)  # the scalar obs stream: the scalar twin's
    t = run.thr.astype(np.int64)
    assert (np.diff(t, axis=-1, prepend=0) == 0).any()  # choices of probability exactly 0: empty intervals
    acts, nodes, final = controller_rollout(ref.obs0, ref.obs, run.out["term"], run.out["trunc"], run.thr,
                                            philox_key(SEED), run.step0)
    assert np.array_equal(run.out["actions"], acts)
    assert np.array_equal(run.out["nodes"], nodes)
    assert np.array_equal(run.snap["nodes"], final)
    # the last real action is drawn; nothing beyond it ever is (a counted padding entry would give 5 or more)
    assert run.out["actions"].min() == 0 and run.out["actions"].max() == A - 1
    assert run.out["nodes"].max() < run.M and ref.obs.max() < run.n_obs
    if run.M > 1:
        ended = run.out["term"][:-1] | run.out["trunc"][:-1]
        assert ended.any() and not run.out["nodes"][1:][ended].any()  # node 0 after every episode end
        assert run.out["nodes"].any()


# ------------------------------------------------------------------ the directed case ----
def test_directed_policy_reaches_the_rare_rows(one_hot, gpu_device):
    """The marginal-greedy policy (tests/taxi_controller_oracle.py; test_taxi_controller_cpu.py shows its law gives
    every full tile >= 100 goal moves and task completions): goal moves, task completions whose episode continues (the
    node is not reset there, and a new passenger is drawn), terminations and truncations all inside one launch."""
    import torch
    probs = marginal_greedy_probs(DIRECTED)
    e = taxi_env(DIRECTED, one_hot=one_hot)
    e.set_controller(probs=probs)
    assert e.query("controller_lds") == 1
    obs0 = reset_obs(e)
    step0 = e.query("philox_step")
    out = e.rollout_controller(K)
    rew, term, trunc = host(out["rew"]), host(out["term"]), host(out["trunc"])
    rr = rare_rows(make_oracle(DIRECTED, 1), rew, term, trunc)
    floor = per_tile_floor(rr)
    totals = {k: int(v.sum()) for k, v in rr.items()}
    print(f"directed: totals {totals}, per-tile minimum {floor}, truncations {int(trunc.sum())}")
    assert floor["goal"] >= 1 and floor["task"] >= 1, floor
    assert term.any() and trunc.any()
    obs = scalar_obs(e, out["obs"])
    acts, nodes, final = controller_rollout(obs0, obs, term, trunc, controller_thresholds(probs), philox_key(SEED),
                                            step0)
    assert np.array_equal(host(out["actions"]), acts) and not host(out["nodes"]).any() and not final.any()
    twin = taxi_env(DIRECTED, one_hot=one_hot)
    twin.reset(seed=SEED)
    o2, r2, tm2, tr2 = twin.rollout(out["actions"])
    assert torch.equal(o2, out["obs"]) and torch.equal(r2, out["rew"])
    assert torch.equal(tm2, out["term"]) and torch.equal(tr2, out["trunc"])
    for a, b in zip(twin.get_state(), e.get_state()):
        assert torch.equal(a, b)
    m = e.metrics()
    assert twin.metrics() == m
    assert m["episodes"] == (term | trunc).sum() and m["return_sum"] == float(rew.astype(np.float64).sum())
    e.check()


# ------------------------------------------------------------------ launches in sequence ----
def test_split_launches_equal_one_launch(run_split):
    import torch
    run = run_split
    e = run.twin()
    a = e.rollout_controller(17)
    mid_nodes = host(e.controller_nodes)
    assert e.query("philox_step") == run.step0 + 17
    if run.M > 1:
        assert mid_nodes.any()
    b = e.rollout_controller(31)
    assert np.array_equal(host(b["nodes"][0]), mid_nodes)  # the nodes carried over
    for nm in NAMES:
        assert torch.equal(torch.cat((a[nm], b[nm])), run.dev[nm]), nm
    assert_same_snapshot(e, run.snap)


def test_open_loop_steps_between_closed_loop_launches(run_split):
    """closed(16) -> rollout() of 8 random actions -> closed(24) equals the twin's open loop of the concatenated
    actions; the open-loop call leaves the nodes alone, and the obs comes from the state whoever stepped it."""
    import torch
    run = run_split
    e = run.twin()
    a = e.rollout_controller(16)
    for nm in NAMES:
        assert torch.equal(a[nm], run.dev[nm][:16]), nm
    nodes16 = host(e.controller_nodes)
    g = torch.Generator(device=e.device).manual_seed(2)
    mid_acts = torch.randint(0, A, (8, B), device=e.device, generator=g, dtype=torch.int32)
    mid = e.rollout(mid_acts)
    assert np.array_equal(host(e.controller_nodes), nodes16)
    assert e.query("philox_step") == run.step0 + 24
    obs_mid = scalar_obs(e, mid[0])
    c = e.rollout_controller(24)
    assert np.array_equal(host(c["nodes"][0]), nodes16)
    acts, nodes, final = controller_rollout(obs_mid[-1], scalar_obs(e, c["obs"]), host(c["term"]), host(c["trunc"]),
                                            run.thr, philox_key(SEED), run.step0 + 24, nodes0=nodes16)
    assert np.array_equal(host(c["actions"]), acts) and np.array_equal(host(c["nodes"]), nodes)
    assert np.array_equal(host(e.controller_nodes), final)
    twin = run.twin(controller=False)
    whole = twin.rollout(torch.cat((a["actions"], mid_acts, c["actions"])))
    for i, nm in enumerate(("obs", "rew", "term", "trunc")):
        assert torch.equal(whole[i], torch.cat((a[nm], mid[i], c[nm]))), nm
    for x, y in zip(twin.get_state(), e.get_state()):
        assert torch.equal(x, y)
    assert twin.metrics() == e.metrics() and twin.query("philox_step") == e.query("philox_step") == run.step0 + 48
    e.check()


def test_optional_outputs(run_split):
    import torch
    run = run_split
    e = run.twin()
    assert e.rollout_controller(K, store=()) == {}
    assert_same_snapshot(e, run.snap, "store=()")
    for store in (("actions", "nodes"), ("obs", "term"), ("rew", "trunc", "obs")):
        e = run.twin()
        out = e.rollout_controller(K, store=store)
        assert sorted(out) == sorted(store)
        assert_same_outputs(out, run.dev, store, f"store={store}")
        assert_same_snapshot(e, run.snap, f"store={store}")
    e = run.twin()
    buf = torch.empty((K, B), dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(K, out={"nodes": buf}, store=("nodes", "rew"))
    assert out["nodes"].data_ptr() == buf.data_ptr()
    assert torch.equal(buf, run.dev["nodes"]) and torch.equal(out["rew"], run.dev["rew"])


# ------------------------------------------------------------------ the table in LDS / in global memory ----
@pytest.mark.parametrize("name,knob,want", [("t5_m1", 0, 0), ("t5_m2", 60 * 1024, 1)])
def test_table_in_lds_equals_table_in_global_memory(name, knob, want, one_hot, gpu_device):
    from gym_po_amd._lib import debug_knobs
    run = get_run(name, one_hot)
    assert run.lds == 1 - want  # the default: M = 1 (10,240 B) staged, M = 2 (30,720 B) not
    e = make_env(name, one_hot=one_hot)
    with debug_knobs(ctrl_lds_max=knob):  # read by set_controller
        e.set_controller(thresholds=run.thr)
    assert e.query("controller_lds") == want
    assert np.array_equal(reset_obs(e), run.obs0)
    assert_same_outputs(e.rollout_controller(K), run.dev, msg=f"ctrl_lds_max={knob}")
    assert_same_snapshot(e, run.snap, f"ctrl_lds_max={knob}")
    e.check()


def test_nothing_is_staged_on_the_8x8_map(gpu_device):
    assert get_run("e8_m1", False).lds == 0 and get_run("e8_m1", True).lds == 0


# ------------------------------------------------------------------ several tiles per block ----
def test_blocks_looping_over_several_tiles(one_hot, gpu_device):
    import torch
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    big, k = 2 * 1024 * cus + 5, 4
    kw = dict(DIRECTED, time_limit=2)
    thr = controller_thresholds(random_probs(2, 320, A, seed=6))
    with debug_knobs(persist_bpc=1):
        e = taxi_env(kw, big, one_hot=one_hot)
    e.set_controller(thresholds=thr)  # (the knob is the handle's from its creation on)
    assert e.query("persist_blocks") == cus and e.query("controller_blocks") == cus
    assert (big + 1023) // 1024 == 2 * cus + 1  # 2 tiles a block, block 0 a third
    e.reset(seed=SEED)
    out = e.rollout_controller(k)
    assert bool(out["trunc"].any()) and bool(out["nodes"].any())
    twin = taxi_env(kw, big, one_hot=one_hot)
    twin.reset(seed=SEED)
    whole = twin.rollout(out["actions"])
    for i, nm in enumerate(("obs", "rew", "term", "trunc")):
        assert torch.equal(whole[i], out[nm]), nm
    del whole
    for x, y in zip(twin.get_state(), e.get_state()):
        assert torch.equal(x, y)
    m = e.metrics()
    assert twin.metrics() == m and m["env_steps"] == k * big
    assert m["episodes"] == int((out["term"] | out["trunc"]).sum())
    e.check()


# ------------------------------------------------------------------ misaligned caller buffers ----
GUARD = 0xA5


def _offset_view(torch, dtype, shape, shift, device):
    """A contiguous tensor of `shape` starting `shift` BYTES past a 16-B boundary of a larger allocation whose other
    bytes hold GUARD: (view, raw bytes, first byte of the view)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device=device)
    lo = 16 + shift
    v = raw[lo:lo + nbytes].view(dtype).view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == shift
    return v, raw, lo


def _guards_intact(raw, lo, nbytes):
    return bool((raw[:lo] == GUARD).all()) and bool((raw[lo + nbytes:] == GUARD).all())


@pytest.mark.parametrize("which,shift", [("actions", 4), ("actions", 12), ("nodes", 1), ("nodes", 3), ("obs", 4),
                                         ("obs", 1)])
def test_misaligned_caller_buffers(which, shift, gpu_device):
    """quad_ok's element-wise fallbacks for actions / nodes, and for the one-hot obs the 4-byte (+4) and the byte
    (+1) stream of chunk_size, against the aligned run; GUARD bytes around the view catch a store outside it."""
    import torch
    run = get_run("t5_m3", which == "obs")
    e = run.twin()
    dt = {"actions": torch.int32, "nodes": torch.uint8, "obs": torch.uint8}[which]
    shape = (K, B, run.n_obs) if which == "obs" else (K, B)
    v, raw, lo = _offset_view(torch, dt, shape, shift, e.device)
    out = e.rollout_controller(K, out={which: v})
    assert out[which].data_ptr() == v.data_ptr()
    assert_same_outputs(out, run.dev, msg=f"{which} +{shift}")
    assert _guards_intact(raw, lo, v.numel() * v.element_size()), f"{which} +{shift}: guard bytes"
    assert_same_snapshot(e, run.snap, f"{which} +{shift}")
    e.check()


# ------------------------------------------------------------------ the nodes ----
def test_nodes_round_trip_and_zeroing(gpu_device):
    M = 3
    e = make_env("t5_m3")
    p = np.zeros((M, e.no, A, M))
    for n in range(M):
        p[n, :, A - 1, (n + 1) % M] = 1.0  # always pickup / dropoff; the node cycles 0 -> 1 -> 2 -> 0
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
    # explicit-action calls and set_state leave the nodes alone; reset zeroes them again, and so does set_controller
    before = host(e.controller_nodes)
    assert before.any()
    e.step(np.zeros(B, dtype=np.int64))
    e.set_state(elapsed=np.zeros(B, dtype=np.int32))
    assert np.array_equal(host(e.controller_nodes), before)
    reset_obs(e)
    assert not host(e.controller_nodes).any()
    e.controller_nodes = start
    e.set_controller(probs=p)
    assert not host(e.controller_nodes).any()
    with pytest.raises(ValueError):
        e.controller_nodes = np.full(B, M)
    e.check()


def test_node_beyond_the_controller_is_clamped_and_flagged(gpu_device):
    """A node >= M written from a device tensor (not range-checked on the host) is clamped and flags the handle."""
    import torch
    from gym_po_amd._lib import GymPoError
    e = make_env("t5_m2", num_envs=300)
    e.set_controller(probs=np.full((2, e.no, A, 2), 0.1))
    reset_obs(e)
    e.controller_nodes = torch.full((300,), 2, dtype=torch.uint8, device=e.device)
    out = e.rollout_controller(4)
    assert int(out["nodes"].max()) < 2 and int(out["actions"].max()) < A
    with pytest.raises(GymPoError):
        e.check()


def test_undersized_table_is_clamped_and_flagged(gpu_device):
    """The C ABI takes any n_obs: an obs beyond the table is clamped on the device and flags the handle."""
    import ctypes

    from gym_po_amd import _lib
    from gym_po_amd._lib import GymPoError
    e = make_env("t5_m1", num_envs=300)
    t = controller_thresholds(np.full((2, A), 1.0 / A))  # n_obs = 2: nearly every obs lies beyond it
    _lib.check(_lib.lib().gp_set_controller(e._handle, 1, 2, ctypes.c_void_p(t.ctypes.data)), "gp_set_controller")
    reset_obs(e)
    out = e.rollout_controller(8)
    assert 0 <= int(out["actions"].min()) and int(out["actions"].max()) < A
    with pytest.raises(GymPoError):
        e.check()


# ------------------------------------------------------------------ errors ----
def test_errors(gpu_device):
    from gym_po_amd._lib import GymPoError
    e = make_env("t5_m1", num_envs=64)
    uniform = np.full((e.no, A), 1.0 / A)
    thr = controller_thresholds(uniform)
    reset_obs(e)
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(4)
    with pytest.raises(GymPoError, match="without a controller"):
        e.controller_nodes
    e.set_controller(probs=np.full((8, e.no, A, 8), 1.0 / (8 * A)))  # M = 8, the most: A * M = 40
    assert int(e.rollout_controller(4)["actions"].max()) < A
    e.set_controller()  # removed again
    assert e.query("controller_nodes") == 0
    with pytest.raises(GymPoError, match="without a controller"):
        e.rollout_controller(4)
    for one_hot in (False, True):  # n_obs != env.no: the one-hot Box space has no .n, env.no is checked all the same
        eo = make_env("t5_m1", num_envs=64, one_hot=one_hot)
        with pytest.raises(GymPoError, match="n_obs"):
            eo.set_controller(probs=np.full((eo.no + 1, A), 1.0 / A))
        with pytest.raises(GymPoError, match="n_obs"):
            eo.set_controller(probs=np.full((eo.no - 1, A), 1.0 / A))
    with pytest.raises(GymPoError, match="entries"):
        e.set_controller(probs=np.full((e.no, A + 1), 1.0 / (A + 1)))  # rows of the wrong length
    with pytest.raises(GymPoError, match="entries"):
        e.set_controller(thresholds=np.ascontiguousarray(thr[:, :, :A - 1]))
    bad = thr.copy()
    bad[0, 7, 1], bad[0, 7, 2] = bad[0, 7, 2], bad[0, 7, 1]  # a non-monotone row
    with pytest.raises(GymPoError, match="not nondecreasing"):
        e.set_controller(thresholds=bad)
    bad = thr.copy()
    bad[0, 3, -1] -= 1  # a row that does not end at 2^31
    with pytest.raises(GymPoError, match="not 2\\^31"):
        e.set_controller(thresholds=bad)
    e2 = make_env("t5_m1", num_envs=64)
    e2.set_controller(probs=uniform)
    with pytest.raises(GymPoError, match="before reset"):
        e2.rollout_controller(4)
    # the raw-state obs and the numpy / replay streams take no controller, from any of the three entry points
    raw = make_env("t5_m1", num_envs=64, hansen_obs=False)
    refused = [(raw, controller_thresholds(np.full((raw.no, A), 1.0 / A)), "GP_OBS_TABLE")]
    for mode in ("numpy", "replay"):
        refused.append((make_env("t5_m1", num_envs=64, rng_mode=mode), thr, mode))
    for env, t, why in refused:
        with pytest.raises(GymPoError, match=rf"\(-3\).*{why}"):
            env.set_controller(thresholds=t)
        with pytest.raises(GymPoError, match=rf"\(-3\).*{why}"):
            env.rollout_controller(4)
        with pytest.raises(GymPoError, match=rf"\(-3\).*{why}"):
            env.controller_nodes
    raw.reset(seed=SEED)
    raw.check()
