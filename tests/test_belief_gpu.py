"""GPU tests of the on-device belief filter of the tabular POMDP (csrc/pomdp.hip pd_belief_filter)
against the numpy restatement tests/belief_oracle.py: every equality is exact, on the float32 bit patterns.

One-step tables through set_state + set_belief + step + belief_filter over every (state, action in -A..A-1, ended or
not) of Tiger (2,3,2), (5,2,3), (37,3,21) and (300,2,70) (S > 255, the global path); rollouts at B = 1,027, K = 40,
time_limit = 7; split launches; B = 3; B = 9,221 under persist_bpc; blocks that loop over two tiles; K = 0; planes
offset by one element; on chip == global through the knob at the exact threshold and one byte below; the degenerate
step; get / set; what leaves the beliefs alone; the filter fed rollout_controller's planes.
"""
import numpy as np
import pytest

import belief_oracle as bo
from pomdp_oracle import Spec
from test_pomdp_gpu import B0, K0, SEED0, TL0, _offset_view, fresh, make, reference_run

pytestmark = pytest.mark.gpu

F = np.float32
# name -> the beliefs stay on chip under the default budget (8,192 S bytes of LDS beside the model blob within 60 KB)
ONCHIP = {"tiger": 1, "m5": 1, "m37": 0, "m300": 0}
KMAX = {"tiger": K0, "m5": K0, "m37": K0, "m300": 6}
_REF = {}


def host(x):
    return x.cpu().numpy()


def assert_bits(got, want, msg=""):
    got = host(got) if not isinstance(got, np.ndarray) else got
    assert got.dtype == np.float32 and got.shape == want.shape, msg
    bad = np.flatnonzero((got.view(np.uint32) != np.asarray(want, dtype=F).view(np.uint32)).any(-1))
    assert bad.size == 0, f"{msg}: {bad.size} envs differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


def laws(env):
    return bo.Laws(Spec.of_env(env))


def belief_ref(name):
    """The reference run of tests/test_pomdp_gpu.py (planes of a 40-step rollout from SEED0) and the beliefs the
    restatement gives over its first KMAX steps: computed once, left unchanged."""
    if name not in _REF:
        ref = reference_run(name)
        lw = bo.Laws(ref["ora"].sp)
        K = KMAX[name]
        obs, _, term, trunc = (x[:K] for x in ref["want"])
        b0, bad = bo.reset_beliefs(lw, ref["obs0"])
        assert not bad.any()
        bK, bad = bo.filter_planes(lw, b0, ref["acts"][:K], obs, term, trunc)
        assert not bad
        assert (bK.max(-1) < 1).any() and len(np.unique(bK.view(np.uint32))) > 4
        _REF[name] = dict(K=K, acts=ref["acts"][:K], obs=obs, term=term, trunc=trunc, b0=b0, bK=bK, obs0=ref["obs0"])
    return _REF[name]


def fresh_belief(name, **knobs):
    from gym_po_amd._lib import debug_knobs
    env, obs0 = fresh(name, **{k: v for k, v in knobs.items() if k != "belief_onchip_max"})
    with debug_knobs(**{k: v for k, v in knobs.items() if k in ("belief_onchip_max", "persist_bpc")}):
        env.enable_belief()
    return env, obs0


# ------------------------------------------------------------------ one-step tables ----
@pytest.mark.parametrize("name", ["tiger", "m5", "m37", "m300"])
def test_one_step_tables(name, gpu_device):
    tl = 9
    env, ora = make(name, 1, tl)
    S, A = env.n_states, env.n_actions
    env.close()
    s, el, act = (x.ravel() for x in np.meshgrid(np.arange(S), np.array([0, tl - 1]), np.arange(-A, A), indexing="ij"))
    B = s.size
    env, ora = make(name, B, tl)
    lw = laws(env)
    env.seed(5)
    env.set_state(state=s, elapsed=el, obs=np.zeros(B, dtype=np.int64))
    env.enable_belief()
    assert env.query("belief") == 1 and env.query("belief_onchip") == ONCHIP[name]
    # enabling sets every belief by the ended rule from the stored obs (0 here)
    want0, _ = bo.reset_beliefs(lw, np.zeros(B, dtype=np.int64))
    assert_bits(env.belief, want0, "after enable")
    rng = np.random.default_rng(S)
    b = rng.random((B, S)) * (rng.random((B, S)) > 0.4)
    b[np.arange(B), s] += 0.05  # the true state keeps mass: no degenerate step
    b = (b / b.sum(-1, keepdims=True)).astype(F)
    env.set_belief(b)
    assert_bits(env.belief, b, "after set_belief")
    o, r, tm, tr, _ = env.step(act)
    env.belief_filter(act[None], o[None], tm[None], tr[None])
    ended = host(tm) | host(tr)
    want, bad = bo.filter_step(lw, b, bo.wrap_actions(act, A), host(o), ended)
    assert not bad.any() and ended.any() and not ended.all()
    assert_bits(env.belief, want, "after the step")
    env.check()


# ------------------------------------------------------------------ rollouts ----
@pytest.mark.parametrize("name", ["tiger", "m5", "m37", "m300"])
def test_filter_over_a_rollouts_planes(name, gpu_device):
    ref = belief_ref(name)
    env, obs0 = fresh(name)
    env.enable_belief()  # after the reset: from the stored obs
    assert env.query("belief_onchip") == ONCHIP[name]
    assert_bits(env.belief, ref["b0"], "enable after reset")
    np.testing.assert_array_equal(host(env.reset(seed=SEED0)[0]), ref["obs0"])
    assert_bits(env.belief, ref["b0"], "reset with the filter enabled")
    o, r, tm, tr = env.rollout(ref["acts"])
    np.testing.assert_array_equal(host(o), ref["obs"])
    assert_bits(env.belief, ref["b0"], "rollout leaves the beliefs alone")
    env.belief_filter(ref["acts"], o, tm, tr)
    assert_bits(env.belief, ref["bK"], "after the filter")
    env.check()


def test_split_launches_and_single_steps(gpu_device):
    ref = belief_ref("m37")
    planes = [ref[n] for n in ("acts", "obs", "term", "trunc")]
    env, _ = fresh_belief("m37")
    for a, b in ((0, 17), (17, 18), (18, 40)):
        env.belief_filter(*(p[a:b] for p in planes))
    assert_bits(env.belief, ref["bK"], "17 + 1 + 22")
    env, _ = fresh_belief("m5")
    ref = belief_ref("m5")
    planes = [ref[n] for n in ("acts", "obs", "term", "trunc")]
    for k in range(K0):
        env.belief_filter(*(p[k:k + 1] for p in planes))
    assert_bits(env.belief, ref["bK"], "40 x K = 1")
    env.check()


def _short_run(name, B, seed, K, tl, **knobs):
    """reset, enable, a K-step rollout, the filter over its planes == the restatement over the same planes."""
    from gym_po_amd._lib import debug_knobs
    env, _ = make(name, B, tl, **knobs)
    obs0 = host(env.reset(seed=seed)[0])
    with debug_knobs(**knobs):
        env.enable_belief()
    lw = laws(env)
    acts = np.random.default_rng(seed).integers(-env.n_actions, env.n_actions, (K, B))
    o, r, tm, tr = env.rollout(acts)
    env.belief_filter(acts, o, tm, tr)
    b0, _ = bo.reset_beliefs(lw, obs0)
    want, bad = bo.filter_planes(lw, b0, acts, host(o), host(tm), host(tr))
    assert not bad
    assert_bits(env.belief, want, f"{name} B={B}")
    env.check()
    return env


@pytest.mark.parametrize("name", ["tiger", "m300"])
def test_three_envs(name, gpu_device):
    _short_run(name, 3, 31, 5, 4)


@pytest.mark.parametrize("name", ["m5", "m37"])
def test_forced_blocks_per_cu(name, gpu_device):
    _short_run(name, 9221, 3, 6, 5, persist_bpc=1)


@pytest.mark.parametrize("name,onchip", [("tiger", 1), ("m5", 0)])
def test_blocks_looping_over_two_tiles(name, onchip, gpu_device):
    """One block per CU and 2 CUs + 1 tiles: every block filters two tiles (on chip: it loads and stores its LDS
    buffers twice), the first block three. Both placements (m5 forced to the global planes)."""
    import torch
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B = 2 * 1024 * cus + 5
    knobs = dict(persist_bpc=1) if onchip else dict(persist_bpc=1, belief_onchip_max=0)
    env = _short_run(name, B, 3, 3, 3, **knobs)
    assert env.query("persist_blocks") == cus and env.query("belief_onchip") == onchip


def test_zero_steps_and_offset_planes(gpu_device):
    import torch
    ref = belief_ref("m5")
    env, _ = fresh_belief("m5")
    empty = torch.zeros((0, B0), dtype=torch.int32, device=gpu_device)
    env.belief_filter(empty, empty, empty.to(torch.uint8), empty.to(torch.uint8))
    assert_bits(env.belief, ref["b0"], "K = 0")
    for offs in ((1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        env, _ = fresh_belief("m5")
        planes = []
        for off, n, dt in zip(offs, ("acts", "obs", "term", "trunc"), (torch.int32, torch.int32, torch.uint8, torch.uint8)):
            v = _offset_view(torch, dt, (K0, B0), off, gpu_device)
            v.copy_(torch.from_numpy(np.ascontiguousarray(ref[n]).astype(np.int32 if dt is torch.int32 else np.uint8)))
            planes.append(v)
        env.belief_filter(*planes)
        assert_bits(env.belief, ref["bK"], f"offsets={offs}")
    env.check()


def test_on_chip_equals_global_at_the_threshold(gpu_device):
    ref = belief_ref("m5")
    env, _ = fresh("m5")
    need = env.query("belief_onchip_bytes")
    assert need == 2 * 5 * 1024 * 4
    planes = [ref[n] for n in ("acts", "obs", "term", "trunc")]
    for knob, path in ((need, 1), (need - 1, 0), (0, 0), (-1, 1)):
        env, _ = fresh_belief("m5", belief_onchip_max=knob)
        assert env.query("belief_onchip") == path, knob
        assert_bits(env.belief, ref["b0"], f"knob {knob}: after enable")
        env.belief_filter(*planes)
        assert_bits(env.belief, ref["bK"], f"knob {knob}")
        env.check()
    # the model in global memory leaves the budget to the beliefs; a model that fills it does not
    env, _ = fresh_belief("m5", pomdp_lds_max=0)
    assert env.query("pomdp_lds") == 0 and env.query("belief_onchip") == 1
    env.belief_filter(*planes)
    assert_bits(env.belief, ref["bK"], "model in global memory")


# ------------------------------------------------------------------ the degenerate step ----
def test_degenerate_step_flags_and_reseed_clears(gpu_device):
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import GymPoError
    T = np.eye(2)[:, None, :]
    Z = np.eye(2)[None]  # state s shows obs s
    env = TabularPOMDPEnv(4, T, Z, np.zeros((2, 1)), start=[0.25, 0.75], time_limit=50)
    env.reset(seed=1)
    env.enable_belief()
    lw = laws(env)
    env.set_state(state=[0, 0, 1, 1], elapsed=[0, 0, 0, 0])
    b = np.array([[0, 1], [1, 0], [0.5, 0.5], [1, 0]], dtype=F)  # envs 0 and 3 put all mass on the other state
    env.set_belief(b)
    o, r, tm, tr, _ = env.step([0, 0, 0, 0])
    assert host(o).tolist() == [0, 0, 1, 1] and not host(tm).any() and not host(tr).any()
    env.check()
    env.belief_filter(np.zeros((1, 4), dtype=np.int32), o[None], tm[None], tr[None])
    want, bad = bo.filter_step(lw, b, [0] * 4, host(o), [False] * 4)
    assert bad.tolist() == [True, False, False, True]
    assert_bits(env.belief, want)
    assert host(env.belief)[0].tolist() == [0.25, 0.75]
    with pytest.raises(GymPoError, match="belief"):
        env.check()
    with pytest.raises(GymPoError, match="0x80"):
        env.metrics()
    env.seed(2)  # a re-seed clears the flag
    env.check()


# ------------------------------------------------------------------ get / set, what leaves the beliefs alone ----
def test_get_set_round_trip(gpu_device):
    env, _ = fresh_belief("m37")
    rng = np.random.default_rng(0)
    b = rng.random((B0, 37)).astype(F)
    b[0, :3] = [1e-45, 3e38, 0.0]  # a denormal, a huge value, a zero: stored as given
    env.set_belief(b)
    assert_bits(env.belief, b)
    import torch
    t = torch.from_numpy(b[::-1].copy()).to(gpu_device)
    env.set_belief(t)
    assert_bits(env.belief, b[::-1])
    for bad in (np.full((B0, 37), -1.0), np.zeros((B0, 37)), np.full((B0, 37), np.nan), np.ones((B0, 36))):
        with pytest.raises(ValueError):
            env.set_belief(bad)
    assert_bits(env.belief, b[::-1], "a refused set changes nothing")
    env.disable_belief()
    assert env.query("belief") == 0
    from gym_po_amd._lib import GymPoError
    for call in (lambda: env.belief, lambda: env.set_belief(b),
                 lambda: env.belief_filter(*(np.zeros((1, B0), dtype=np.int32),) * 4)):
        with pytest.raises(GymPoError, match="without a belief filter"):
            call()


def test_prior_given(gpu_device):
    env, obs0 = fresh("m5")
    with pytest.raises(ValueError, match="prior"):
        env.enable_belief(prior=[1, 1, 1])
    with pytest.raises(ValueError, match="prior"):
        env.enable_belief(prior=[1, -1, 1, 1, 1])
    prior = [4, 1, 2, 1, 0]
    env.enable_belief(prior=prior)
    lw = bo.Laws(Spec.of_env(env), prior=(np.array(prior, dtype=F) / F(8)))
    want, _ = bo.reset_beliefs(lw, obs0)
    assert_bits(env.belief, want)


def test_step_rollout_and_controller_leave_the_beliefs_alone(gpu_device):
    env, _ = fresh_belief("m5")
    ref = belief_ref("m5")
    A = env.n_actions
    env.step(np.zeros(B0, dtype=np.int64))
    env.rollout(ref["acts"][:3])
    env.set_controller(probs=np.full((env.n_obs, A), 1.0 / A))
    out = env.rollout_controller(5)
    env.set_state(state=np.zeros(B0, dtype=np.int64))
    assert_bits(env.belief, ref["b0"], "step, rollout, rollout_controller, set_state")
    env.check()


def test_filter_fed_rollout_controllers_planes(gpu_device):
    env, obs0 = fresh_belief("m37")
    lw = laws(env)
    A = env.n_actions
    env.set_controller(probs=np.full((env.n_obs, A), 1.0 / A))
    out = env.rollout_controller(12)
    env.belief_filter(out)
    b0, _ = bo.reset_beliefs(lw, obs0)
    want, bad = bo.filter_planes(lw, b0, *(host(out[n]) for n in ("actions", "obs", "term", "trunc")))
    assert not bad
    assert_bits(env.belief, want)
    with pytest.raises(ValueError, match="lacks"):
        env.belief_filter({"actions": out["actions"]})
    env.check()
