"""GPU tests of the alpha-vector policy and the closed-loop belief rollout of the tabular POMDP (csrc/pomdp.hip
pd_rollout_belief): one launch does policy choice, env step and filter update for K steps.

The emitted actions, vector indices and values equal the numpy policy (tests/belief_oracle.py) on the restatement's
beliefs, bit for bit; the closed loop equals a twin's open-loop rollout() of the emitted actions (outputs, state,
metrics); the beliefs afterwards equal belief_filter over the planes the launch wrote. B = 1,027, K = 40, time_limit 7,
N in {1, A, 6, 257} with duplicate vectors (the first wins); store subsets; split launches; the four combinations of
model and belief placement; the refusals; Tiger under QMDP vectors; the calibration test on device beliefs and states.
"""
import numpy as np
import pytest

import belief_oracle as bo
from pomdp_oracle import TIGER, Spec
from test_pomdp_gpu import B0, K0, SEED0, fresh, tables

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("obs", "actions", "vec", "value", "rew", "term", "trunc")
_RUNS = {}


def host(x):
    return x.cpu().numpy()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def vectors(S, A, N, seed):
    """Random vectors with exact duplicates (ties: the first must win) and an action per vector. Vector j is the tangent
    plane of |b|^2 at a random point p_j of the simplex, b . alpha_j = |b|^2 - |b - p_j|^2, so the vector of the nearest
    point wins and no vector dominates the others everywhere (plain random vectors do, on Tiger's segment)."""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(S, 0.7), N)
    p = p[np.argsort(((p - 1.0 / S) ** 2).sum(-1))]  # vector 0 wins at the uniform belief
    alpha = (2 * p - (p * p).sum(-1, keepdims=True)).astype(F)
    if N >= 6:
        alpha[4] = alpha[1]
        alpha[N - 1] = alpha[0]
    # (Tiger's belief moves only under action 0, listen: most vectors take it there, the first among them)
    va = None if N == A else np.where(rng.random(N) < (0.7 if S == 2 else 0.0), 0, rng.integers(0, A, N))
    if va is not None and S == 2:
        va[0] = 0
    return alpha, va


def install(env, alpha, va, **knobs):
    from gym_po_amd._lib import debug_knobs
    with debug_knobs(**knobs):
        env.enable_belief()
    env.set_belief_policy(alpha, va)
    assert env.query("belief_vectors") == len(alpha)


class Run:
    """One closed-loop run from SEED0 and its replay by the restatement: made once, left unchanged."""

    def __init__(self, name, N, env_knobs=None, belief_knobs=None):
        env, obs0 = fresh(name, **(env_knobs or {}))
        S, A = env.n_states, env.n_actions
        self.alpha, va = vectors(S, A, N, seed=S + N)
        install(env, self.alpha, va, **(belief_knobs or {}))
        self.va = np.arange(A) if va is None else va
        self.env, self.obs0, self.lw = env, obs0, bo.Laws(Spec.of_env(env))
        self.out = {k: host(v) for k, v in env.rollout_belief(K0).items()}
        self.belief = host(env.belief)
        self.state = [host(x) for x in env.get_state()]
        self.metrics = env.metrics()
        env.check()


def run(name, N):
    if (name, N) not in _RUNS:
        _RUNS[name, N] = Run(name, N)
    return _RUNS[name, N]


CASES = [("tiger", 1), ("tiger", 3), ("tiger", 6), ("tiger", 257), ("m5", 1), ("m5", 2), ("m5", 6), ("m5", 257),
         ("m37", 1), ("m37", 3), ("m37", 6), ("m37", 257)]


@pytest.mark.parametrize("name,N", CASES)
def test_actions_vectors_values_and_beliefs_vs_the_restatement(name, N, gpu_device):
    r = run(name, N)
    out, lw = r.out, r.lw
    assert set(out) == set(NAMES) and out["term"].dtype == np.bool_ and out["vec"].dtype == np.int32
    b, bad = bo.reset_beliefs(lw, r.obs0)
    ties = 0
    for k in range(K0):
        a, j, v = bo.policy(r.alpha, r.va, b)
        np.testing.assert_array_equal(out["vec"][k], j, err_msg=f"vec at step {k}")
        np.testing.assert_array_equal(out["actions"][k], a, err_msg=f"actions at step {k}")
        np.testing.assert_array_equal(bits(out["value"][k]), bits(v), err_msg=f"value at step {k}")
        ties += int(((j == 1) | (j == 0)).sum()) if N >= 6 else 0
        b, bad = bo.filter_step(lw, b, a, out["obs"][k], out["term"][k] | out["trunc"][k])
        assert not bad.any()
    np.testing.assert_array_equal(bits(r.belief), bits(b), err_msg="beliefs after the launch")
    if N >= 6:  # a duplicate never wins; its original does (checked where 6 vectors make that certain)
        assert not np.isin(out["vec"], (4, N - 1)).any() and (ties > 0 or N != 6)
    if N > 1:
        assert len(np.unique(out["vec"])) > 1


@pytest.mark.parametrize("name,N", [("tiger", 3), ("m5", 6), ("m37", 257)])
def test_closed_loop_equals_the_open_loop_of_its_actions(name, N, gpu_device):
    r = run(name, N)
    twin, obs0 = fresh(name)
    np.testing.assert_array_equal(obs0, r.obs0)
    o, rew, tm, tr = twin.rollout(r.out["actions"])
    for n, x in (("obs", o), ("rew", rew), ("term", tm), ("trunc", tr)):
        np.testing.assert_array_equal(bits(host(x)), bits(r.out[n]), err_msg=n)
    for n, x, y in zip(("state", "elapsed", "obs"), twin.get_state(), r.state):
        np.testing.assert_array_equal(host(x), y, err_msg=n)
    assert twin.metrics() == r.metrics and r.metrics["env_steps"] == B0 * K0 and r.metrics["episodes"] >= 5 * B0
    assert twin.query("philox_step") == r.env.query("philox_step") == 1 + K0
    # the beliefs after the closed loop == the filter run over the planes it wrote
    twin.enable_belief()
    twin.reset(seed=SEED0)
    twin.belief_filter(r.out)
    np.testing.assert_array_equal(bits(host(twin.belief)), bits(r.belief))


def test_store_subsets_and_split_launches(gpu_device):
    import torch
    r = run("m5", 6)
    for store in [()] + [(n,) for n in NAMES]:
        env, _ = fresh("m5")
        install(env, r.alpha, r.va)
        out = env.rollout_belief(K0, store=store)
        assert set(out) == set(store)
        for n in store:
            np.testing.assert_array_equal(bits(host(out[n])), bits(r.out[n]), err_msg=f"{n} alone")
        assert env.metrics() == r.metrics
        np.testing.assert_array_equal(bits(host(env.belief)), bits(r.belief))
    env, _ = fresh("m5")
    install(env, r.alpha, r.va)
    bufs = {n: torch.empty((17, B0), dtype=torch.float32, device=gpu_device) for n in ("rew", "value")}
    parts = [env.rollout_belief(17, out=bufs)]
    assert parts[0]["rew"].data_ptr() == bufs["rew"].data_ptr()
    parts = [{k: v.clone() for k, v in parts[0].items()}, env.rollout_belief(1), env.rollout_belief(22)]
    for n in NAMES:
        np.testing.assert_array_equal(bits(host(torch.cat([p[n] for p in parts]))), bits(r.out[n]), err_msg=f"{n} split")
    assert env.rollout_belief(0)["obs"].shape == (0, B0)
    assert env.metrics() == r.metrics
    np.testing.assert_array_equal(bits(host(env.belief)), bits(r.belief))
    with pytest.raises(ValueError, match="unknown output"):
        env.rollout_belief(1, store=("nodes",))
    with pytest.raises(ValueError, match="out value"):
        env.rollout_belief(3, out=bufs)
    env.check()


@pytest.mark.parametrize("model_lds,onchip", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_model_and_belief_placements_give_the_same_bits(model_lds, onchip, gpu_device):
    r = run("m5", 6)
    other = Run("m5", 6, None if model_lds else dict(pomdp_lds_max=0), None if onchip else dict(belief_onchip_max=0))
    assert other.env.query("pomdp_lds") == model_lds and other.env.query("belief_onchip") == onchip
    assert r.env.query("pomdp_lds") == 1 and r.env.query("belief_onchip") == 1
    for n in NAMES:
        np.testing.assert_array_equal(bits(other.out[n]), bits(r.out[n]), err_msg=n)
    np.testing.assert_array_equal(bits(other.belief), bits(r.belief))
    assert other.metrics == r.metrics


def test_two_tiles_per_block(gpu_device):
    """Blocks that loop over two tiles: the on-chip buffers are reloaded per tile and the metrics add up."""
    import torch
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B, K = 2 * 1024 * cus + 5, 4
    from test_pomdp_gpu import make
    res = []
    for knobs in (dict(persist_bpc=1), {}):
        env, _ = make("tiger", B, 3, **knobs)
        env.reset(seed=3)
        alpha, va = vectors(2, 3, 3, seed=1)
        install(env, alpha, va, **knobs)
        out = env.rollout_belief(K)
        res.append(([host(out[n]) for n in NAMES], host(env.belief), env.metrics()))
        env.check()
    for x, y in zip(res[0][0], res[1][0]):
        np.testing.assert_array_equal(bits(x), bits(y))
    np.testing.assert_array_equal(bits(res[0][1]), bits(res[1][1]))
    assert res[0][2] == res[1][2]


# ------------------------------------------------------------------ refusals ----
def test_refusals_by_name(gpu_device):
    import ctypes
    from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv
    from gym_po_amd import _lib
    from gym_po_amd._lib import GymPoError
    UNSUPPORTED = -3  # GP_E_UNSUPPORTED
    env, _ = fresh("tiger")
    alpha = np.zeros((3, 2), dtype=F)
    with pytest.raises(GymPoError, match="without a belief filter"):
        env.rollout_belief(1)
    env.enable_belief()
    with pytest.raises(GymPoError, match="without a policy"):
        env.rollout_belief(1)
    env.set_belief_policy(alpha)
    env.rollout_belief(1)
    env.set_belief_policy(None)
    assert env.query("belief_vectors") == 0
    with pytest.raises(GymPoError, match="without a policy"):
        env.rollout_belief(1)
    for bad in (np.nan, np.inf, -np.inf, 2e30):
        a = alpha.copy()
        a[2, 1] = bad
        with pytest.raises(GymPoError, match=r"alpha\[2\]\[1\]"):
            env.set_belief_policy(a)
    for va in ([0, 1, 3], [0, -1, 2]):
        with pytest.raises(GymPoError, match=r"vec_action\[[12]\]"):
            env.set_belief_policy(alpha, va)
    with pytest.raises(ValueError, match="name each vector"):
        env.set_belief_policy(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="alpha must be"):
        env.set_belief_policy(np.zeros((3, 3)))
    with pytest.raises(GymPoError, match="4097 vectors"):
        env.set_belief_policy(np.zeros((4097, 2)), np.zeros(4097, dtype=np.int64))
    assert env.query("belief_vectors") == 0  # a refused install leaves nothing
    # before reset
    e2 = TabularPOMDPEnv.from_pomdp(TIGER, 8)
    e2.enable_belief()
    e2.set_belief_policy(alpha)
    with pytest.raises(GymPoError, match="before reset"):
        e2.rollout_belief(1)
    # S above the filter's limit
    S = 4097
    thr = np.where(np.arange(S)[None, :] >= np.arange(S)[:, None], 1 << 31, 0).astype(np.uint32)  # identity rows
    one = np.full((1, S, 1), 1 << 31, dtype=np.uint32)
    big = TabularPOMDPEnv.from_thresholds(4, thr[:, None, :], one, thr[0], one[0], np.zeros((S, 1, S), dtype=np.float32),
                                          np.zeros(S, dtype=np.uint8))
    with pytest.raises(GymPoError, match="4097 states.*4096"):
        big.enable_belief()
    with pytest.raises(GymPoError, match="4097 states.*4096"):
        big.set_belief_policy(np.zeros((1, S)), [0])
    assert big.query("belief") == 0
    # other kinds
    hh = HeavenHellGridEnv(8)
    L = _lib.lib()
    assert L.gp_belief_enable(hh._handle, None) == UNSUPPORTED
    assert L.gp_belief_disable(hh._handle) == UNSUPPORTED
    assert L.gp_set_belief_policy(hh._handle, 0, None, None) == UNSUPPORTED
    assert L.gp_rollout_belief(hh._handle, 1, None, None, None, None, None, None, None, None) == UNSUPPORTED
    buf = ctypes.c_void_p(8)
    assert L.gp_belief_get(hh._handle, buf, None) == UNSUPPORTED
    assert L.gp_belief_filter(hh._handle, 0, None, None, None, None, None) == UNSUPPORTED


# ------------------------------------------------------------------ use: Tiger under QMDP ----
def test_tiger_under_qmdp_vectors(gpu_device):
    from gym_po_amd import TabularPOMDPEnv, parse_pomdp, qmdp_vectors
    m = parse_pomdp(TIGER)
    alpha = qmdp_vectors(m["T"], m["R"], None, 0.95, 1000)
    B, K, LISTEN = 4096, 40, 0
    env = TabularPOMDPEnv.from_pomdp(TIGER, B, time_limit=25)
    obs0 = host(env.reset(seed=11)[0])
    env.enable_belief()
    env.set_belief_policy(alpha)  # vector a belongs to action a
    assert env.query("belief_onchip") == 1 and env.query("belief_vectors") == 3
    out = {k: host(v) for k, v in env.rollout_belief(K).items()}
    lw = bo.Laws(Spec.of_env(env))
    b, _ = bo.reset_beliefs(lw, obs0)
    assert (b == 0.5).all()
    a64 = np.asarray(alpha, dtype=np.float32).astype(np.float64)
    opened = 0
    for k in range(K):
        a = out["actions"][k]
        if k == 0:
            assert (a == LISTEN).all()  # the first action of every episode: listen, at (0.5, 0.5)
        else:
            ended = out["term"][k - 1] | out["trunc"][k - 1]
            assert (a[ended] == LISTEN).all()
        v = b.astype(np.float64) @ a64.T
        door = a != LISTEN
        opened += int(door.sum())
        # no door is opened where listening is worth more by 1e-3 (float64 on the restatement's beliefs)
        assert (v[door, LISTEN] - v[door, a[door]] <= 1e-3).all()
        np.testing.assert_array_equal(a, bo.policy(alpha, np.arange(3), b)[0])
        b, bad = bo.filter_step(lw, b, a, out["obs"][k], out["term"][k] | out["trunc"][k])
        assert not bad.any()
    m = env.metrics()
    assert opened > 0 and out["trunc"].any()
    print(f"Tiger under QMDP vectors: mean reward per step {m['return_sum'] / m['env_steps']:.4f}, doors opened "
          f"{opened} in {B * K} env-steps, mean return per finished episode {m['return_sum'] / max(m['episodes'], 1):.3f}")
    env.check()


# ------------------------------------------------------------------ calibration on the device ----
@pytest.mark.parametrize("mode", ["uniform", "greedy"])
@pytest.mark.parametrize("name", ["tiger", "m5", "m37"])
def test_calibration_on_device_beliefs(name, mode, gpu_device):
    """The calibration test of tests/test_belief_cpu.py on the device's beliefs and get_state(): among the envs whose
    belief gives a state probability p, a fraction p is in it. B = 2^16, K = 12, time_limit = 7."""
    import torch
    from gym_po_amd import TabularPOMDPEnv, qmdp_vectors
    T, Z, R, start, terminal, reset_obs = tables(name)
    B, K = 1 << 16, 12
    env = TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs, time_limit=7)
    env.reset(seed=17)
    env.enable_belief()
    l64 = bo.Laws64(Spec.of_env(env))
    env.set_belief_policy(qmdp_vectors(l64.Tf, env.reward.astype(np.float64), env.terminal, 0.95, 200))
    gen = torch.Generator(device="cpu").manual_seed(5)

    def steps():
        yield host(env.belief), host(env.get_state()[0])
        for k in range(K):
            if mode == "uniform":
                a = torch.randint(0, env.n_actions, (1, B), generator=gen, dtype=torch.int32)
                o, r, tm, tr = env.rollout(a)
                env.belief_filter(a, o, tm, tr)
            else:
                env.rollout_belief(1, store=())
            yield host(env.belief), host(env.get_state()[0])
    bo.assert_calibrated(steps(), f"device {name} {mode}")
    env.check()
