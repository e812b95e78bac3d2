"""GPU tests of the point-based value backup of the tabular POMDP (csrc/pomdp_backup.hip, gp_belief_backup,
TabularPOMDPEnv.point_backup). Every equality is on bit patterns.

Parity with the numpy restatement (tests/pbvi_oracle.py, itself pinned to a scalar statement by tests/test_pbvi_cpu.py)
on Tiger, (5,2,3), (37,3,21) and (300,2,70), P in {1, 3, 67, 257, 1027}, N in {1, A, 6, 257}, with one-hot, sparse and
unnormalised points, an obs of probability zero, mixed-sign, duplicate and tied vectors, gamma in {0, 0.95, 1}; the
model in LDS against the model in global memory; buffers off their boundaries; every subset of the outputs; scratch
growth; the refusals by name and code; no side effects on the handle; and the detour maze end to end, collect_beliefs ->
pbvi -> set_belief_policy -> rollout_belief, against the CPU pipeline.
"""
import ctypes

import numpy as np
import pytest

import pbvi_cases as pc
import pbvi_oracle as po

pytestmark = pytest.mark.gpu

F = np.float32
bits = pc.bits
INVALID, UNSUPPORTED, STATE = -1, -3, -4


def host(x):
    return x.cpu().numpy()


def make(name, B=8, **knobs):
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import debug_knobs
    T, Z, R, start, terminal, reset_obs = pc.tables(name)
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


def assert_backup(out, want, msg=""):
    assert set(out) == {"alpha", "actions", "value"}
    np.testing.assert_array_equal(host(out["actions"]), want["actions"], err_msg=f"actions {msg}")
    np.testing.assert_array_equal(bits(host(out["value"])), bits(want["value"]), err_msg=f"value {msg}")
    np.testing.assert_array_equal(bits(host(out["alpha"])), bits(want["alpha"]), err_msg=f"alpha {msg}")


# ------------------------------------------------------------------ parity ----
# the oracle's cost P A O N S stays below 2 10^8 per case
CASES = [("tiger", 1, 1), ("tiger", 3, 3), ("tiger", 257, 6), ("tiger", 1027, 257),
         ("m5", 1, 257), ("m5", 3, 6), ("m5", 257, 2), ("m5", 1027, 1), ("m5", 1027, 257),
         ("m37", 1, 6), ("m37", 3, 257), ("m37", 257, 257), ("m37", 1027, 3), ("m37", 257, 1),
         ("m300", 1, 1), ("m300", 3, 2), ("m300", 3, 257), ("m300", 67, 6), ("m300", 257, 2), ("m300", 1027, 1)]


@pytest.mark.parametrize("name,P,N", CASES)
def test_backup_equals_the_restatement(name, P, N, gpu_device):
    import torch
    env = shared_env(name)
    assert env.query("pomdp_lds") == (name in ("tiger", "m5"))
    b, al, want = pc.reference(name, P, N)
    out = env.point_backup(b, al, 0.95)
    assert out["alpha"].dtype == torch.float32 and out["actions"].dtype == torch.int32
    assert tuple(out["alpha"].shape) == (P, env.n_states) and tuple(out["value"].shape) == (P,)
    assert_backup(out, want)
    if P >= 257 and N > 1:
        assert len(np.unique(want["actions"])) > 1 and len(np.unique(bits(want["alpha"]), axis=0)) > 1
    assert env.query("backup_tables") == 1 and env.query("backup_scratch_bytes") > 0
    env.check()


@pytest.mark.parametrize("gamma", [0.0, 1.0])
@pytest.mark.parametrize("name", ["tiger", "m5", "m37"])
def test_gamma_edges(name, gamma, gpu_device):
    env = shared_env(name)
    b, al, want = pc.reference(name, 257, 6, gamma)
    assert_backup(env.point_backup(torch_of(b, gpu_device), al, gamma), want)


def torch_of(x, device):
    import torch
    return torch.as_tensor(x).to(device)


# ------------------------------------------------------------------ placement and buffers ----
def test_model_in_lds_equals_model_in_global_memory(gpu_device):
    """The backup reads the model through its own tables: the blob's placement changes nothing. pomdp_lds_max at the
    blob's size and one byte below."""
    base = shared_env("m5")
    size = base.query("pomdp_model_bytes")
    b, al, want = pc.reference("m5", 257, 6)
    for knob, lds in ((size, 1), (size - 1, 0)):
        env = make("m5", pomdp_lds_max=knob)
        assert env.query("pomdp_lds") == lds
        assert_backup(env.point_backup(b, al, 0.95), want, f"pomdp_lds {lds}")
        env.check()


def test_buffers_off_their_boundaries(gpu_device):
    import torch
    env = shared_env("m37")
    S = env.n_states
    P, N = 257, 6
    b, al, want = pc.reference("m37", P, N)
    pts = torch.zeros(P * S + 1, dtype=torch.float32, device=gpu_device)
    pts[1:] = torch_of(b, gpu_device).reshape(-1)
    raw = {"alpha": torch.full((P * S + 2,), -7.0, dtype=torch.float32, device=gpu_device),
           "actions": torch.full((P + 2,), -7, dtype=torch.int32, device=gpu_device),
           "value": torch.full((P + 2,), -7.0, dtype=torch.float32, device=gpu_device)}
    out = {"alpha": raw["alpha"][1:-1].view(P, S), "actions": raw["actions"][1:-1], "value": raw["value"][1:-1]}
    got = env.point_backup(pts[1:].view(P, S), al, 0.95, out=out)
    assert got["alpha"].data_ptr() == raw["alpha"].data_ptr() + 4 and got["value"].data_ptr() % 8 == 4
    assert_backup(got, want)
    for t in raw.values():  # nothing written outside
        assert float(t[0]) == -7 and float(t[-1]) == -7
    with pytest.raises(ValueError, match="out value"):
        env.point_backup(b, al, 0.95, out={"value": raw["value"]})
    with pytest.raises(ValueError, match="out alpha"):
        env.point_backup(b, al, 0.95, out={"alpha": raw["alpha"][:P * S].view(S, P)})


def test_each_output_alone_and_none(gpu_device):
    import torch
    from gym_po_amd import _lib
    env = shared_env("m5")
    S = env.n_states
    P, N = 257, 6
    b, al, want = pc.reference("m5", P, N)
    pts = torch_of(b, gpu_device).contiguous()
    fn = _lib.lib().gp_belief_backup
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for keep in ((), ("alpha",), ("actions",), ("value",)):
        bufs = {"alpha": torch.full((P, S), -7.0, dtype=torch.float32, device=gpu_device),
                "actions": torch.full((P,), -7, dtype=torch.int32, device=gpu_device),
                "value": torch.full((P,), -7.0, dtype=torch.float32, device=gpu_device)}
        arg = {k: (bufs[k] if k in keep else None) for k in bufs}
        rc = fn(env._handle, P, ptr(pts), N, ctypes.c_void_p(al.ctypes.data), 0.95, ptr(arg["alpha"]),
                ptr(arg["actions"]), ptr(arg["value"]), env._stream())
        assert rc == 0
        torch.cuda.synchronize()
        for k in bufs:
            if k in keep:
                np.testing.assert_array_equal(bits(host(bufs[k])), bits(want[k]), err_msg=f"{k} alone")
            else:
                assert bool((bufs[k] == -7).all()), k
    env.check()


def test_two_calls_of_different_size_grow_the_scratch(gpu_device):
    env = make("m37")
    assert env.query("backup_scratch_bytes") == 0 and env.query("backup_tables") == 0
    S, A, O = env.n_states, env.n_actions, env.n_obs
    sizes = []
    for P, N in ((3, 257), (257, 257), (1, 6), (257, 1)):
        b, al, want = pc.reference("m37", P, N)
        assert_backup(env.point_backup(b, al, 0.95), want, f"P {P}")
        sizes.append(env.query("backup_scratch_bytes"))
    assert sizes[0] == 3 * A * (4 * S + 2 * O) and sizes[1] == 257 * A * (4 * S + 2 * O)
    assert sizes[2] == sizes[1] == sizes[3]  # the scratch never shrinks between calls
    # P = 0: a no-op that returns empty outputs
    out = env.point_backup(np.zeros((0, S), dtype=F), np.zeros((1, S), dtype=F), 0.95)
    assert tuple(out["alpha"].shape) == (0, S) and tuple(out["actions"].shape) == (0,)
    env.disable_belief()
    assert env.query("backup_scratch_bytes") == 0 and env.query("backup_tables") == 0
    env.enable_belief()  # and built again when needed
    b, al, want = pc.reference("m37", 3, 257)
    assert_backup(env.point_backup(b, al, 0.95), want, "after disable / enable")
    env.check()


# ------------------------------------------------------------------ refusals ----
def test_refusals_by_name_and_code(gpu_device):
    import torch
    from gym_po_amd import HeavenHellGridEnv, TabularPOMDPEnv, _lib
    from gym_po_amd._lib import GymPoError
    from pomdp_oracle import TIGER
    env = TabularPOMDPEnv.from_pomdp(TIGER, 8)
    b = np.array([[0.5, 0.5], [1.0, 0.0]], dtype=F)
    al = np.zeros((3, 2), dtype=F)
    with pytest.raises(GymPoError, match=rf"\({STATE}\).*gp_belief_backup without a belief filter"):
        env.point_backup(b, al)
    env.enable_belief()  # (no reset needed: the backup reads the model only)
    env.point_backup(b, al)
    for bad in (np.nan, np.inf, -np.inf, 2e30):
        a = al.copy()
        a[2, 1] = bad
        with pytest.raises(GymPoError, match=rf"\({INVALID}\).*alpha\[2\]\[1\]"):
            env.point_backup(b, a)
    for g in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(GymPoError, match=rf"\({INVALID}\).*gamma must be in \[0, 1\]"):
            env.point_backup(b, al, g)
    with pytest.raises(GymPoError, match=rf"\({INVALID}\).*4097 vectors"):
        env.point_backup(b, np.zeros((4097, 2), dtype=F))
    L = _lib.lib()
    pts = torch.as_tensor(b).to(gpu_device)
    p_pts, p_al = ctypes.c_void_p(pts.data_ptr()), ctypes.c_void_p(al.ctypes.data)
    err = lambda: L.gp_last_error().decode()  # noqa: E731
    assert L.gp_belief_backup(env._handle, 2, p_pts, 0, p_al, 0.95, None, None, None, None) == INVALID
    assert "0 vectors" in err()
    assert L.gp_belief_backup(env._handle, -1, p_pts, 3, p_al, 0.95, None, None, None, None) == INVALID
    assert "-1 points" in err()
    assert L.gp_belief_backup(env._handle, (1 << 20) + 1, p_pts, 3, p_al, 0.95, None, None, None, None) == INVALID
    assert "1048577 points" in err()
    assert L.gp_belief_backup(env._handle, 2, None, 3, p_al, 0.95, None, None, None, None) == INVALID
    assert L.gp_belief_backup(env._handle, 2, p_pts, 3, None, 0.95, None, None, None, None) == INVALID
    assert "required" in err()
    assert L.gp_belief_backup(env._handle, 0, None, 3, p_al, 0.95, None, None, None, None) == 0  # P = 0: a no-op
    # N S beyond the policy's 2^22 entries, and a scratch beyond 2^30 bytes: refused before anything is allocated
    big = make("m300")
    S = big.n_states
    many = np.zeros((4096, S), dtype=F)  # 4096 * 300 < 2^22: accepted as a size
    assert L.gp_belief_backup(big._handle, 1 << 20, p_pts, 4096, ctypes.c_void_p(many.ctypes.data), 0.95, None, None,
                              None, None) == INVALID
    assert "bytes of scratch" in err() and big.query("backup_scratch_bytes") == 0
    wide = make_wide()
    assert L.gp_belief_backup(wide._handle, 1, p_pts, 4096, p_al, 0.95, None, None, None, None) == INVALID
    assert "entries" in err()
    # the python checks of the points
    for bad, match in ((np.array([[0.5, -0.5]]), "finite and >= 0"), (np.array([[0.0, 0.0]]), "positive sum"),
                       (np.array([[np.nan, 1.0]]), "finite"), (np.zeros((2, 3)), r"points must be \[P, S\]")):
        with pytest.raises(ValueError, match=match):
            env.point_backup(bad.astype(F), al)
    with pytest.raises(ValueError, match="alpha must be"):
        env.point_backup(b, np.zeros((3, 3), dtype=F))
    # other kinds
    hh = HeavenHellGridEnv(8)
    assert L.gp_belief_backup(hh._handle, 2, p_pts, 3, p_al, 0.95, None, None, None, None) == UNSUPPORTED
    env.check()


def make_wide():
    """S = 2,048 (identity transitions, one obs): 4,096 vectors are 2^23 entries."""
    from gym_po_amd import TabularPOMDPEnv
    S = 2048
    thr = np.where(np.arange(S)[None, :] >= np.arange(S)[:, None], 1 << 31, 0).astype(np.uint32)
    one = np.full((1, S, 1), 1 << 31, dtype=np.uint32)
    env = TabularPOMDPEnv.from_thresholds(4, thr[:, None, :], one, thr[0], one[0], np.zeros((S, 1, S), dtype=np.float32),
                                          np.zeros(S, dtype=np.uint8))
    env.enable_belief()
    return env


# ------------------------------------------------------------------ no side effects ----
def test_a_backup_leaves_the_handle_alone(gpu_device):
    from test_belief_policy_gpu import vectors
    runs = []
    for with_backup in (True, False):
        env = make("m37", B=1027)
        alpha, va = vectors(env.n_states, env.n_actions, 6, seed=2)
        env.set_belief_policy(alpha, va)
        first = {k: host(v) for k, v in env.rollout_belief(5).items()}
        if with_backup:
            b, al, want = pc.reference("m37", 257, 6)
            assert_backup(env.point_backup(b, al, 0.95), want)
        second = {k: host(v) for k, v in env.rollout_belief(9).items()}
        runs.append((first, second, host(env.belief), [host(x) for x in env.get_state()], env.metrics(),
                     env.query("philox_step"), env.query("belief_vectors")))
        env.check()
    x, y = runs
    for part in (0, 1):
        for k in x[part]:
            np.testing.assert_array_equal(bits(x[part][k]), bits(y[part][k]), err_msg=k)
    np.testing.assert_array_equal(bits(x[2]), bits(y[2]))
    for u, v in zip(x[3], y[3]):
        np.testing.assert_array_equal(u, v)
    assert x[4] == y[4] and x[5] == y[5] == 1 + 14 and x[6] == y[6] == 6


# ------------------------------------------------------------------ end to end ----
@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
def test_detour_maze_end_to_end(obs_type, gpu_device):
    """collect_beliefs -> pbvi -> set_belief_policy -> rollout_belief on the device at 2,048 envs against the CPU
    pipeline of tests/pbvi_cases.py: the same points, the same final vector set bit for bit, every finished episode a
    termination with +1; the QMDP twin's figures are the CPU-predicted ones (no episode terminates)."""
    from gym_po_amd import TabularPOMDPEnv, collect_beliefs, pbvi
    d = pc.detour_pipeline(obs_type)
    sp = d["sp"]

    def fresh(seed):
        env = TabularPOMDPEnv.from_thresholds(pc.DETOUR_B, sp.trans_thr, sp.obs_thr, sp.start_thr, sp.reset_obs_thr,
                                              sp.reward, sp.terminal, time_limit=pc.DETOUR_TL)
        env.reset(seed=seed)
        env.enable_belief()
        return env
    env = fresh(pc.DETOUR_SEED)
    points = collect_beliefs(env, pc.detour_plane())
    np.testing.assert_array_equal(bits(points), bits(d["points"]))
    assert env.query("philox_step") == 1 + pc.DETOUR_K
    alpha, actions, values = pbvi(env, points, pc.DETOUR_GAMMA, pc.DETOUR_SWEEPS)
    np.testing.assert_array_equal(bits(alpha), bits(d["alpha"]))
    np.testing.assert_array_equal(actions, d["actions"])
    np.testing.assert_array_equal(bits(values), bits(d["values"]))
    for al, va, want in ((alpha, actions, d["run_pbvi"]), (d["qmdp"], np.arange(4), d["run_qmdp"])):
        run = fresh(pc.EVAL_SEED)
        run.set_belief_policy(al, va)
        out = {k: host(v) for k, v in run.rollout_belief(pc.EVAL_K, store=("rew", "term", "trunc")).items()}
        m = run.metrics()
        assert m["episodes"] == want["episodes"] and m["return_sum"] == float(want["returns"].sum())
        assert int(out["term"].sum()) == want["terminated"] and int((out["trunc"] & ~out["term"]).sum()) == want["truncated"]
        if want is d["run_pbvi"]:
            fin = out["term"] | out["trunc"]
            assert fin.sum() >= 4 * pc.DETOUR_B and not out["trunc"].any() and (out["rew"][fin] == 1.0).all()
            assert m["return_sum"] == m["episodes"]
        else:
            assert not out["term"].any() and m["return_sum"] == 0.0 and m["episodes"] >= pc.DETOUR_B
        run.check()
    # the policy collects too: 'policy' gathers the beliefs of the closed loop
    run = fresh(pc.EVAL_SEED)
    run.set_belief_policy(alpha, actions)
    seen = collect_beliefs(run, "policy", 12)
    have = {r.tobytes() for r in bits(points)}
    assert 1 < len(seen) <= len(points) and all(r.tobytes() in have for r in bits(seen))
    env.check()
