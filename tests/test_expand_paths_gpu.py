"""GPU tests of gp_belief_expand's stream order and store paths, in the manner of
tests/test_stream_order_gpu.py and tests/test_store_guard_gpu.py.

Stream order: the call on a non-blocking side stream behind a busy-wait, its points and its reference set arriving by
copies queued behind that wait (tests/stream_order.py). The C call with prepared buffers must return while the wait
still runs (it is asynchronous once its scratch has its size) and compute from the late inputs; the Python wrapper
validates its inputs on the host, so it waits, and computes from the late inputs too; a call that has to grow its
scratch under queued work waits for it.

Store paths: every output in a caller buffer with guard bytes round it (tests/store_guard.py), each at each of its
4-byte shifts and all shifted together, the points and the reference set shifted too; the expected bits are the numpy
restatement's.
"""
import ctypes

import numpy as np
import pytest

import expand_cases as xc
import store_guard as sg
import stream_order as so

pytestmark = pytest.mark.gpu

SEED = 7
DEV = "cuda:0"
NAMES = ("succ", "dist", "actions", "obs", "mass")


def mk(name):
    def make():
        from gym_po_amd import TabularPOMDPEnv
        T, Z, R, start, terminal, reset_obs = xc.tables(name)
        return TabularPOMDPEnv(1027, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs, time_limit=5)
    return make


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_expand(env, pts, ref):
    """gp_belief_expand with prepared buffers: no host-side validation, nothing that waits."""
    import torch
    from gym_po_amd import _lib
    P, S = pts.shape
    out = {"succ": torch.empty((P, S), dtype=torch.float32, device=pts.device)}
    for k in ("dist", "mass"):
        out[k] = torch.empty((P,), dtype=torch.float32, device=pts.device)
    for k in ("actions", "obs"):
        out[k] = torch.empty((P,), dtype=torch.int32, device=pts.device)
    _lib.check(_lib.lib().gp_belief_expand(env._handle, P, ptr(pts), 0 if ref is None else ref.shape[0], ptr(ref),
                                           ptr(out["succ"]), ptr(out["dist"]), ptr(out["actions"]), ptr(out["obs"]),
                                           ptr(out["mass"]), env._stream()), "gp_belief_expand")
    return out


def inputs(name, P, Q):
    """(true, poison): the points and the reference set of expand_cases, and valid rows that differ from them."""
    b, q, want = xc.reference(name, P, Q)
    t = {"pts": b} if q is None else {"pts": b, "ref": q}
    p = {k: (v[:, ::-1].copy() * np.float32(0.5) + np.float32(0.01)) for k, v in t.items()}
    return t, p, want


def warm(P, Q):
    """enable_belief and one expansion of the same size: the tables are built and the scratch has its size, so the
    call under test allocates nothing."""
    def setup(env):
        import torch
        env.enable_belief()
        S = env.n_states
        one = torch.full((max(P, Q or 1), S), 0.5, dtype=torch.float32, device=env.device)
        raw_expand(env, one[:P], None if Q is None else one[:Q])
        torch.cuda.current_stream(env.device).synchronize()
    return setup


def assert_oracle(snap, want, what):
    for k in NAMES:
        dt, shape, data = snap["outs"][k]
        assert data == np.ascontiguousarray(want[k]).tobytes(), f"{what}: {k} differs from the restatement"


# ------------------------------------------------------------------ stream order ----
@pytest.mark.parametrize("name,P,Q", [("tiger", 257, 1027), ("tiger", 257, None), ("m37", 67, 64), ("m37", 67, None)])
def test_expand_on_a_side_stream_from_late_inputs(name, P, Q, gpu_device):
    t, p, want = inputs(name, P, Q)
    ref, poi, got, still = so.run_case(f"pomdp_{name}/gp_belief_expand P={P} Q={Q}", mk(name), SEED,
                                       lambda env, b: raw_expand(env, b["pts"], b.get("ref")), t, p, setup=warm(P, Q))
    assert still
    assert_oracle(ref, want, "null stream")
    assert_oracle(got, want, "side stream")


def test_expand_wrapper_waits_and_sees_the_late_inputs(gpu_device):
    """expand_beliefs validates points and ref on the host: it waits for the stream, then computes from what the late
    copies brought."""
    t, p, want = inputs("m37", 67, 64)
    ref, poi, got, still = so.run_case("pomdp_m37/expand_beliefs", mk("m37"), SEED,
                                       lambda env, b: env.expand_beliefs(b["pts"], b["ref"]), t, p, setup=warm(67, 64),
                                       expect_async=False)
    assert_oracle(got, want, "side stream")


def test_expand_grows_its_scratch_under_queued_work(gpu_device):
    """A first call for 3 points is queued behind the delay; the second needs more scratch: the buffers the first
    call's kernels use are freed only once they are done."""
    t, p, want = inputs("m37", 67, 64)
    _, _, small = xc.reference("m37", 3, 65)
    ts, ps, _ = inputs("m37", 3, 65)
    t2 = {"pts": t["pts"], "ref": t["ref"], "pts3": ts["pts"], "ref65": ts["ref"]}
    p2 = {"pts": p["pts"], "ref": p["ref"], "pts3": ps["pts"], "ref65": ps["ref"]}

    def call(env, b):
        first = raw_expand(env, b["pts3"], b["ref65"])
        n0 = env.query("expand_scratch_bytes")
        second = raw_expand(env, b["pts"], b["ref"])
        assert env.query("expand_scratch_bytes") > n0
        return {"first": first, "second": second}
    ref, poi, got, still = so.run_case("pomdp_m37/gp_belief_expand grows", mk("m37"), SEED, call, t2, p2,
                                       setup=warm(3, 65), expect_async=False)
    for k in NAMES:
        assert got["outs"]["first"][k][2] == np.ascontiguousarray(small[k]).tobytes(), k
        assert got["outs"]["second"][k][2] == np.ascontiguousarray(want[k]).tobytes(), k


# ------------------------------------------------------------------ store paths ----
def G(dtype, shape, shift):
    import torch
    shape = tuple(int(s) for s in shape)
    plane = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return sg.guarded(torch, dtype, shape, shift, DEV, plane)


def filled(x, shift):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x))
    buf = G(t.dtype, t.shape, shift)
    buf[0].copy_(t)
    return buf


@pytest.mark.parametrize("name,P,Q", [("tiger", 1, 1), ("tiger", 257, 1027), ("hand", 67, None), ("m37", 1, 1027),
                                      ("m37", 67, 64), ("m37", 67, None)])
def test_guard_bytes_round_every_output(name, P, Q, gpu_device):
    """succ [P,S], dist, actions, obs, mass [P] guarded, points [P,S] and ref [Q,S] guarded and shifted: the guards
    hold, every element is stored (the poison is gone), the inputs are not written, the handle is untouched."""
    import torch
    b, q, want = xc.reference(name, P, Q)
    S = b.shape[1]
    env = mk(name)()
    try:
        so.reset(env, SEED)
        env.enable_belief()
        before = so.env_snapshot(env)
        dts = {"succ": (torch.float32, (P, S)), "dist": (torch.float32, (P,)), "actions": (torch.int32, (P,)),
               "obs": (torch.int32, (P,)), "mass": (torch.float32, (P,))}
        n0 = sg.STATS["buffers"]
        for shifts in [(0,) * 7] + sg.shift_cases((4,) * 7):
            src = filled(b, shifts[0])
            rsrc = None if q is None else filled(q, shifts[1])
            bufs = {n: G(*dts[n], sh) for n, sh in zip(NAMES, shifts[2:])}
            env.expand_beliefs(src[0], None if rsrc is None else rsrc[0], out={n: v[0] for n, v in bufs.items()})
            torch.cuda.synchronize()
            for n, v in bufs.items():
                sg.check(*v, want[n], f"pomdp_{name}/expand_beliefs P={P} Q={Q} {n} shifts={shifts}")
            sg.check_input(*src, b, f"pomdp_{name}/expand_beliefs points")
            if rsrc is not None:
                sg.check_input(*rsrc, q, f"pomdp_{name}/expand_beliefs ref")
        assert sg.STATS["buffers"] - n0 == 25 * (6 if q is None else 7)
        bad = so.differing(before, so.env_snapshot(env))
        assert not bad, f"the handle differs in {bad}"
        env.check()
    finally:
        torch.cuda.synchronize()
        env.close()


def test_a_subset_of_guarded_outputs(gpu_device):
    """Each output alone in a guarded buffer through the C call (the others NULL), and a refused call writes nothing."""
    import torch
    from gym_po_amd import _lib
    P, Q = 67, 64
    b, q, want = xc.reference("m37", P, Q)
    S = b.shape[1]
    env = mk("m37")()
    try:
        so.reset(env, SEED)
        env.enable_belief()
        fn = _lib.lib().gp_belief_expand
        src, rsrc = filled(b, 4), filled(q, 12)
        dts = {"succ": (torch.float32, (P, S)), "dist": (torch.float32, (P,)), "actions": (torch.int32, (P,)),
               "obs": (torch.int32, (P,)), "mass": (torch.float32, (P,))}
        for keep in NAMES:
            buf = G(*dts[keep], 4)
            a = {n: (buf[0] if n == keep else None) for n in NAMES}
            assert fn(env._handle, P, ptr(src[0]), Q, ptr(rsrc[0]), ptr(a["succ"]), ptr(a["dist"]), ptr(a["actions"]),
                      ptr(a["obs"]), ptr(a["mass"]), env._stream()) == 0
            torch.cuda.synchronize()
            sg.check(*buf, want[keep], f"{keep} alone")
        bufs = {n: G(*dts[n], 8) for n in NAMES}
        assert fn(env._handle, P, ptr(src[0]), 0, ptr(rsrc[0]), *(ptr(bufs[n][0]) for n in NAMES), env._stream()) == -1
        assert "0 reference rows" in _lib.lib().gp_last_error().decode()
        torch.cuda.synchronize()
        for n in NAMES:
            sg.check_untouched(*bufs[n], f"refused {n}")
        sg.check_input(*src, b, "points")
        sg.check_input(*rsrc, q, "ref")
        env.check()
    finally:
        torch.cuda.synchronize()
        env.close()
