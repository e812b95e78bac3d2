"""GPU tests of the belief-set expansion of the tabular POMDP (csrc/pomdp_expand.hip, gp_belief_expand,
TabularPOMDPEnv.expand_beliefs). Every equality is on bit patterns.

Parity of all five outputs with the numpy restatement (tests/expand_oracle.py, itself pinned to a scalar statement and
checked against a float64 filter by tests/test_expand_cpu.py) on Tiger, (5,2,3), (37,3,21), (300,2,70) and a hand-made
model with dead candidates, P in {1, 3, 67, 257}, Q in {1, 64, 65, 257, 1027} and ref = NULL, with one-hot, sparse and
unnormalised points, a point without a live candidate, an obs of probability zero, Tiger's tie over the obs, duplicate
reference rows; the model in LDS against the model in global memory; buffers off their boundaries; every output alone
and none; scratch growth and release; the refusals by name and code; no side effects on the handle; live successors
against belief_filter; and the detour maze end to end from the reset beliefs alone against the CPU pipeline.
"""
import ctypes

import numpy as np
import pytest

import expand_cases as xc
import pbvi_cases as pc

pytestmark = pytest.mark.gpu

F = np.float32
bits = xc.bits
INVALID, UNSUPPORTED, STATE = -1, -3, -4
LDS_MODELS = ("tiger", "m5", "hand")


def host(x):
    return x.cpu().numpy()


def make(name, B=8, **knobs):
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import debug_knobs
    T, Z, R, start, terminal, reset_obs = xc.tables(name)
    with debug_knobs(**knobs):
        env = TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs, time_limit=7)
    env.reset(seed=1)
    env.enable_belief()
    return env


_ENVS = {}


def shared_env(name):
    if name not in _ENVS:
        _ENVS[name] = make(name)
    return _ENVS[name]


def assert_expansion(out, want, msg=""):
    assert set(out) == set(xc.OUTPUTS)
    for k in ("actions", "obs", "mass", "dist", "succ"):
        np.testing.assert_array_equal(bits(host(out[k])), bits(want[k]), err_msg=f"{k} {msg}")


def torch_of(x, device):
    import torch
    return torch.as_tensor(x).to(device)


# ------------------------------------------------------------------ parity ----
@pytest.mark.parametrize("name,P,Q", xc.CASES)
def test_expansion_equals_the_restatement(name, P, Q, gpu_device):
    import torch
    env = shared_env(name)
    assert env.query("pomdp_lds") == (name in LDS_MODELS)
    b, q, want = xc.reference(name, P, Q)
    out = env.expand_beliefs(b, q)
    assert all(out[k].dtype == torch.float32 for k in ("succ", "dist", "mass"))
    assert out["actions"].dtype == torch.int32 and out["obs"].dtype == torch.int32
    assert tuple(out["succ"].shape) == (P, env.n_states) and all(tuple(out[k].shape) == (P,) for k in xc.OUTPUTS[1:])
    assert_expansion(out, want)
    # the cases hold what they claim
    if P >= 67 and Q != 1:  # (on Tiger only listen moves a belief off the uniform one)
        assert len(np.unique(want["actions"])) > (name != "tiger") and len(np.unique(want["obs"])) > 1
    if name == "hand" and P > 1:  # the point without a live candidate
        assert want["actions"][1] == -1 and want["obs"][1] == -1 and not want["succ"][1].any()
        assert want["actions"][0] >= 0 and (want["obs"] != 2).all()  # (obs 2 never occurs)
    if name == "tiger" and Q in (65, 1027):  # the tie of the uniform belief under listen: the first obs
        assert (int(want["actions"][0]), int(want["obs"][0])) == (0, 0)
    assert env.query("backup_tables") == 1 and env.query("expand_scratch_bytes") > 0
    env.check()


def test_tensors_on_the_device_are_taken_as_they_are(gpu_device):
    env = shared_env("m37")
    b, q, want = xc.reference("m37", 67, 64)
    assert_expansion(env.expand_beliefs(torch_of(b, gpu_device), torch_of(q, gpu_device)), want)
    # the points as their own reference set, spelled out, are ref = NULL
    b, _, want = xc.reference("m37", 67, None)
    assert_expansion(env.expand_beliefs(b, b), want)


# ------------------------------------------------------------------ placement and buffers ----
def test_model_in_lds_equals_model_in_global_memory(gpu_device):
    """The expansion reads the model through the backup's tables: the blob's placement changes nothing. pomdp_lds_max
    at the blob's size and one byte below."""
    base = shared_env("m5")
    size = base.query("pomdp_model_bytes")
    for knob, lds in ((size, 1), (size - 1, 0)):
        env = make("m5", pomdp_lds_max=knob)
        assert env.query("pomdp_lds") == lds
        for P, Q in ((257, 65), (257, None)):
            b, q, want = xc.reference("m5", P, Q)
            assert_expansion(env.expand_beliefs(b, q), want, f"pomdp_lds {lds}")
        env.check()


def test_buffers_off_their_boundaries(gpu_device):
    import torch
    env = shared_env("m37")
    S = env.n_states
    P, Q = 67, 64
    b, q, want = xc.reference("m37", P, Q)
    pts = torch.zeros(P * S + 1, dtype=torch.float32, device=gpu_device)
    pts[1:] = torch_of(b, gpu_device).reshape(-1)
    ref = torch.zeros(Q * S + 1, dtype=torch.float32, device=gpu_device)
    ref[1:] = torch_of(q, gpu_device).reshape(-1)
    f32, i32 = torch.float32, torch.int32
    raw = {"succ": torch.full((P * S + 2,), -7.0, dtype=f32, device=gpu_device),
           "dist": torch.full((P + 2,), -7.0, dtype=f32, device=gpu_device),
           "actions": torch.full((P + 2,), -7, dtype=i32, device=gpu_device),
           "obs": torch.full((P + 2,), -7, dtype=i32, device=gpu_device),
           "mass": torch.full((P + 2,), -7.0, dtype=f32, device=gpu_device)}
    out = {k: (v[1:-1].view(P, S) if k == "succ" else v[1:-1]) for k, v in raw.items()}
    got = env.expand_beliefs(pts[1:].view(P, S), ref[1:].view(Q, S), out=out)
    assert got["succ"].data_ptr() == raw["succ"].data_ptr() + 4 and got["obs"].data_ptr() % 8 == 4
    assert_expansion(got, want)
    for t in raw.values():  # nothing written outside
        assert float(t[0]) == -7 and float(t[-1]) == -7
    with pytest.raises(ValueError, match="out mass"):
        env.expand_beliefs(b, q, out={"mass": raw["mass"]})
    with pytest.raises(ValueError, match="out succ"):
        env.expand_beliefs(b, q, out={"succ": raw["succ"][:P * S].view(S, P)})
    with pytest.raises(ValueError, match="out obs"):
        env.expand_beliefs(b, q, out={"obs": raw["dist"][:P]})


def test_each_output_alone_and_none(gpu_device):
    import torch
    from gym_po_amd import _lib
    env = shared_env("m5")
    S = env.n_states
    P, Q = 257, 65
    b, q, want = xc.reference("m5", P, Q)
    pts, ref = torch_of(b, gpu_device).contiguous(), torch_of(q, gpu_device).contiguous()
    fn = _lib.lib().gp_belief_expand
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for keep in ((),) + tuple((k,) for k in xc.OUTPUTS) + (xc.OUTPUTS,):
        bufs = {"succ": torch.full((P, S), -7.0, dtype=torch.float32, device=gpu_device),
                "dist": torch.full((P,), -7.0, dtype=torch.float32, device=gpu_device),
                "actions": torch.full((P,), -7, dtype=torch.int32, device=gpu_device),
                "obs": torch.full((P,), -7, dtype=torch.int32, device=gpu_device),
                "mass": torch.full((P,), -7.0, dtype=torch.float32, device=gpu_device)}
        arg = {k: (bufs[k] if k in keep else None) for k in bufs}
        rc = fn(env._handle, P, ptr(pts), Q, ptr(ref), ptr(arg["succ"]), ptr(arg["dist"]), ptr(arg["actions"]),
                ptr(arg["obs"]), ptr(arg["mass"]), env._stream())
        assert rc == 0
        torch.cuda.synchronize()
        for k in bufs:
            if k in keep:
                np.testing.assert_array_equal(bits(host(bufs[k])), bits(want[k]), err_msg=f"{k} of {keep}")
            else:
                assert bool((bufs[k] == -7).all()), k
    env.check()


def test_scratch_grows_and_is_released(gpu_device):
    env = make("m37")
    assert env.query("expand_scratch_bytes") == 0 and env.query("backup_tables") == 0
    S, A, O = env.n_states, env.n_actions, env.n_obs
    per_point = A * (4 * S + 4 * O + 8)
    sizes = []
    for P, Q in ((3, 65), (67, 64), (1, 1027), (67, None), (257, 1)):
        b, q, want = xc.reference("m37", P, Q)
        assert_expansion(env.expand_beliefs(b, q), want, f"P {P} Q {Q}")
        sizes.append(env.query("expand_scratch_bytes"))
    assert sizes[0] == 3 * per_point + 4 * S * 65 and sizes[1] == 67 * per_point + 4 * S * 65
    assert sizes[2] == sizes[3] == 67 * per_point + 4 * S * 1027  # no part of the scratch ever shrinks
    assert sizes[4] == 257 * per_point + 4 * S * 1027
    assert env.query("backup_tables") == 1 and env.query("backup_scratch_bytes") == 257 * A * 4 * S  # acc is shared
    # P = 0: a no-op that returns empty outputs
    out = env.expand_beliefs(np.zeros((0, S), dtype=F))
    assert tuple(out["succ"].shape) == (0, S) and tuple(out["obs"].shape) == (0,)
    assert env.query("expand_scratch_bytes") == sizes[4]
    env.disable_belief()
    assert env.query("expand_scratch_bytes") == 0 and env.query("backup_tables") == 0
    env.enable_belief()  # and built again when needed
    b, q, want = xc.reference("m37", 3, 65)
    assert_expansion(env.expand_beliefs(b, q), want, "after disable / enable")
    assert env.query("expand_scratch_bytes") == sizes[0]
    env.check()


# ------------------------------------------------------------------ refusals ----
def test_refusals_by_name_and_code(gpu_device):
    import torch
    from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv, _lib
    from gym_po_amd._lib import GymPoError
    from pomdp_oracle import TIGER
    env = TabularPOMDPEnv.from_pomdp(TIGER, 8)
    b = np.array([[0.5, 0.5], [1.0, 0.0]], dtype=F)
    with pytest.raises(GymPoError, match=rf"\({STATE}\).*gp_belief_expand without a belief filter"):
        env.expand_beliefs(b)
    env.enable_belief()  # (no reset needed: the expansion reads the model only)
    env.expand_beliefs(b)
    L = _lib.lib()
    pts = torch.as_tensor(b).to(gpu_device)
    p_pts = ctypes.c_void_p(pts.data_ptr())
    err = lambda: L.gp_last_error().decode()  # noqa: E731
    call = lambda h, P, pp, Q, pq: L.gp_belief_expand(h, P, pp, Q, pq, None, None, None, None, None, None)  # noqa: E731
    assert call(env._handle, -1, p_pts, 0, None) == INVALID
    assert "-1 points" in err()
    assert call(env._handle, (1 << 20) + 1, p_pts, 0, None) == INVALID
    assert "1048577 points" in err()
    assert call(env._handle, 2, p_pts, 0, p_pts) == INVALID
    assert "0 reference rows" in err()
    assert call(env._handle, 2, p_pts, -3, p_pts) == INVALID
    assert "-3 reference rows" in err()
    assert call(env._handle, 2, p_pts, (1 << 20) + 1, p_pts) == INVALID
    assert "1048577 reference rows" in err()
    assert call(env._handle, 2, None, 2, p_pts) == INVALID
    assert "points are required" in err()
    assert call(env._handle, 2, p_pts, -3, None) == 0  # without ref, n_ref is not read
    assert call(env._handle, 0, None, 0, None) == 0    # P = 0: a no-op
    assert call(env._handle, 0, None, 2, p_pts) == 0
    # a scratch beyond 2^30 bytes: refused before anything is allocated; by the points and by the reference set
    big = make("m300")
    assert call(big._handle, 1 << 20, p_pts, 1, p_pts) == INVALID
    assert "bytes of scratch" in err() and "1048576 points and 1 reference rows" in err()
    assert call(big._handle, 1, p_pts, 1 << 20, p_pts) == INVALID
    assert "bytes of scratch" in err() and big.query("expand_scratch_bytes") == 0 and big.query("backup_tables") == 0
    # the python checks
    for bad, match in ((np.array([[0.5, -0.5]]), "finite and >= 0"), (np.array([[0.0, 0.0]]), "positive sum"),
                       (np.array([[np.nan, 1.0]]), "finite"), (np.zeros((2, 3)), r"points must be \[P, S\]")):
        with pytest.raises(ValueError, match=match):
            env.expand_beliefs(bad.astype(F))
    for bad, match in ((np.array([[0.5, -0.5]]), "ref must be finite"), (np.array([[np.inf, 0.0]]), "ref must be fin"),
                       (np.zeros((2, 3)), r"ref must be \[Q, S\]"), (np.zeros((0, 2)), "at least one row")):
        with pytest.raises(ValueError, match=match):
            env.expand_beliefs(b, bad.astype(F))
    with pytest.raises(ValueError, match="out must be a dict"):
        env.expand_beliefs(b, out=[])
    # other kinds
    hh = HeavenHellGridEnv(8)
    assert call(hh._handle, 2, p_pts, 0, None) == UNSUPPORTED
    env.check()


# ------------------------------------------------------------------ no side effects ----
def test_an_expansion_leaves_the_handle_alone(gpu_device):
    """Against a twin that does not expand: the closed loop before and after, beliefs, state, metrics, step counter and
    the installed policy are the same, and a point_backup gives the same bits before and after the expansion (which
    shares its acc scratch and its tables)."""
    from test_belief_policy_gpu import vectors
    runs = []
    for with_expansion in (True, False):
        env = make("m37", B=1027)
        alpha, va = vectors(env.n_states, env.n_actions, 6, seed=2)
        env.set_belief_policy(alpha, va)
        first = {k: host(v) for k, v in env.rollout_belief(5).items()}
        pb, pal, _ = pc.reference("m37", 257, 6)
        before = {k: host(v) for k, v in env.point_backup(pb, pal, 0.95).items()}
        if with_expansion:
            b, q, want = xc.reference("m37", 67, 64)
            assert_expansion(env.expand_beliefs(b, q), want)
            b, q, want = xc.reference("m37", 257, 257)
            assert_expansion(env.expand_beliefs(b, q), want)
        after = {k: host(v) for k, v in env.point_backup(pb, pal, 0.95).items()}
        second = {k: host(v) for k, v in env.rollout_belief(9).items()}
        runs.append((first, second, before, after, host(env.belief), [host(x) for x in env.get_state()], env.metrics(),
                     env.query("philox_step"), env.query("belief_vectors")))
        env.check()
    x, y = runs
    for part in (0, 1, 2, 3):
        for k in x[part]:
            np.testing.assert_array_equal(bits(x[part][k]), bits(y[part][k]), err_msg=f"{part} {k}")
    for k in x[2]:
        np.testing.assert_array_equal(bits(x[2][k]), bits(x[3][k]), err_msg=f"backup {k}")
        np.testing.assert_array_equal(bits(x[2][k]), bits(pc.reference("m37", 257, 6)[2][k]), err_msg=f"backup {k}")
    np.testing.assert_array_equal(bits(x[4]), bits(y[4]))
    for u, v in zip(x[5], y[5]):
        np.testing.assert_array_equal(u, v)
    assert x[6] == y[6] and x[7] == y[7] == 1 + 14 and x[8] == y[8] == 6


# ------------------------------------------------------------------ the filter's own beliefs ----
@pytest.mark.parametrize("name,P,Q", [("tiger", 257, 1027), ("m5", 257, 65), ("m37", 257, 257)])
def test_live_successors_are_the_filters_beliefs(name, P, Q, gpu_device):
    """The points as the beliefs of P envs, one belief_filter step over (a*, o*) that did not end: the beliefs are the
    emitted successors bit for bit (unnormalised points included: the filter takes beliefs as given)."""
    import torch
    from gym_po_amd import _lib
    env = make(name, B=P)
    b, q, want = xc.reference(name, P, Q)
    assert (want["actions"] >= 0).all()
    out = env.expand_beliefs(b, q)
    pts = torch_of(b, gpu_device).contiguous()
    _lib.check(_lib.lib().gp_belief_set(env._handle, ctypes.c_void_p(pts.data_ptr()), env._stream()), "gp_belief_set")
    zero = torch.zeros((1, P), dtype=torch.uint8, device=gpu_device)
    env.belief_filter(out["actions"].view(1, P), out["obs"].view(1, P), zero, zero)
    np.testing.assert_array_equal(bits(host(env.belief)), bits(host(out["succ"])))
    np.testing.assert_array_equal(bits(host(env.belief)), bits(want["succ"]))
    env.check()


# ------------------------------------------------------------------ end to end ----
@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_detour_maze_from_the_reset_beliefs(obs_type, gpu_device):
    """reset_points -> pbvi_expanding (expand_beliefs and point_backup on the device) -> set_belief_policy ->
    rollout_belief against the CPU pipeline of tests/pbvi_cases.py, with no collecting walk: the same 14 points, the
    same final vector set bit for bit, every finished episode a termination with +1; the library says that the set is
    closed and that it is not with a point left out."""
    from gym_po_amd import TabularPOMDPEnv, expand_points, is_closed, pbvi_expanding, reset_points
    import expand_oracle as xo
    d = pc.detour_pipeline(obs_type)
    sp = d["sp"]

    def fresh(seed):
        env = TabularPOMDPEnv.from_thresholds(pc.DETOUR_B, sp.trans_thr, sp.obs_thr, sp.start_thr, sp.reset_obs_thr,
                                              sp.reward, sp.terminal, time_limit=pc.DETOUR_TL)
        env.reset(seed=seed)
        env.enable_belief()
        return env
    env = fresh(pc.DETOUR_SEED)
    cpu = xo.CpuEnv(sp)
    start = reset_points(env)
    np.testing.assert_array_equal(bits(start), bits(reset_points(cpu)))
    np.testing.assert_array_equal(bits(expand_points(env, start)), bits(expand_points(cpu, start)))
    resets = {r.tobytes() for r in bits(start)}
    other = next(i for i in range(14) if bits(d["points"][i]).tobytes() not in resets)
    assert is_closed(env, d["points"]) and not is_closed(env, np.delete(d["points"], other, axis=0))
    assert not is_closed(env, start)
    alpha, actions, points, values = pbvi_expanding(env, pc.DETOUR_GAMMA, 32, pc.DETOUR_SWEEPS)
    np.testing.assert_array_equal(bits(points), bits(d["points"]))
    np.testing.assert_array_equal(bits(alpha), bits(d["alpha"]))
    np.testing.assert_array_equal(actions, d["actions"])
    np.testing.assert_array_equal(bits(values[-1]), bits(d["values"]))
    assert env.query("philox_step") == 1  # nothing was stepped
    run = fresh(pc.EVAL_SEED)
    run.set_belief_policy(alpha, actions)
    out = {k: host(v) for k, v in run.rollout_belief(pc.EVAL_K, store=("rew", "term", "trunc")).items()}
    m, want = run.metrics(), d["run_pbvi"]
    assert m["episodes"] == want["episodes"] and m["return_sum"] == float(want["returns"].sum()) == m["episodes"]
    fin = out["term"] | out["trunc"]
    assert fin.sum() >= 4 * pc.DETOUR_B and not out["trunc"].any() and (out["rew"][fin] == 1.0).all()
    run.check()
    env.check()
