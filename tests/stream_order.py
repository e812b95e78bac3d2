"""Helpers of tests/test_stream_order_gpu.py: the late-input pattern that makes a mis-ordered launch visible.

include/gym_po_amd.h promises that every call is asynchronous on the hipStream_t it is given. On the null stream every
kernel and copy is serialised with every other, so an operation queued on the wrong stream cannot show there. Here a
call runs on a non-blocking side stream `s` behind a busy-wait, and its device inputs hold *poison* (valid values that
differ from the true ones) until a copy queued on `s` after the busy-wait replaces them:

    ev = delay(s)            # a busy-wait kernel on s; ev is recorded right after it
    late(buf, true_values)   # buf.copy_(true_values) on s, behind the delay
    out = call(env, buf)     # the call under test, enqueued on s
    still = not ev.query()   # the call returned while the delay was still running

A kernel or copy of the call that is not ordered after the earlier work on `s` reads the poison (or state that the
queued work has not written yet) and the result differs from a twin env that ran the true inputs on the null stream.
`still` shows that the call did not wait, i.e. that it is asynchronous and that none of its work can have run before
the late copy was even queued to execute. Everything is compared bit for bit through the byte view; there is no
tolerance anywhere. A twin run on the poison itself must differ from the reference, else the case proves nothing and
fails.
"""
import time

import numpy as np

DELAY_MS = 100.0      # the busy-wait every case queues (the measured length is held to [DELAY_MS / 2, CAP_MS])
CAP_MS = 200.0
_CYCLES = None
STATS = {"delay_ms": None, "max_enqueue_ms": 0.0, "max_enqueue_case": None}


def _torch():
    import torch
    return torch


def _sleep(cycles):
    torch = _torch()
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(cycles))
    else:  # a chain of dependent matmuls on one tensor
        x = torch.full((256, 256), 1.0 / 256, device="cuda")
        for _ in range(int(cycles)):
            x = x @ x


def _time_ms(cycles):
    torch = _torch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    _sleep(cycles)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calibrate():
    """The `cycles` argument that makes the busy-wait DELAY_MS long, measured once per session with two events (the
    second, longer measurement is the one kept: the first includes the kernel's load)."""
    global _CYCLES
    if _CYCLES is not None:
        return _CYCLES
    has_sleep = hasattr(_torch().cuda, "_sleep")
    n = 1_000_000 if has_sleep else 50
    _time_ms(n)
    for _ in range(4):
        ms = max(_time_ms(n), 1e-3)
        if ms >= DELAY_MS / 4:
            break
        n = int(n * min(DELAY_MS / 2 / ms, 64.0)) + 1
    n = int(n * DELAY_MS / ms) + 1
    got = _time_ms(n)
    assert DELAY_MS / 2 <= got <= CAP_MS, f"the busy-wait measured {got:.1f} ms for a target of {DELAY_MS} ms"
    STATS["delay_ms"] = got
    _CYCLES = n
    return n


def delay(stream):
    """Enqueue the busy-wait on `stream`; returns an event recorded right after it."""
    torch = _torch()
    n = calibrate()
    with torch.cuda.stream(stream):
        _sleep(n)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def late(dst, src):
    """`dst` holds poison; the true values arrive by a copy on the current stream (behind the delay queued there)."""
    assert dst.is_cuda and src.is_cuda and dst.shape == src.shape and dst.dtype == src.dtype
    dst.copy_(src, non_blocking=True)


def raw(x):
    """A value as something `==` compares bit for bit: tensors and arrays through their bytes."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        if x.dtype == torch.bool:
            x = x.view(torch.uint8)
        return (str(x.dtype), tuple(x.shape), x.numpy().tobytes())
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, float):
        return ("f64", np.float64(x).tobytes())
    if isinstance(x, dict):
        return {k: raw(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(raw(v) for v in x)
    return x


def _try(fn):
    from gym_po_amd._lib import GymPoError
    try:
        return fn()
    except (GymPoError, AttributeError):
        return None


def env_snapshot(env):
    """Everything the handle holds after a run: state, metrics, the RNG position, controller nodes, beliefs. Syncs."""
    snap = {"state": raw(tuple(env.get_state())), "metrics": raw(env.metrics())}
    if env.rng_mode == "philox":
        snap["philox_step"] = _try(lambda: env.query("philox_step"))  # (None: a kind that does not answer the key)
    elif env.rng_mode == "numpy":
        snap["rng_state"] = env.rng_state
    if _try(lambda: env.query("controller_nodes")):
        snap["controller_nodes"] = raw(env.controller_nodes)
    if _try(lambda: env.query("belief")):
        snap["belief"] = raw(env.belief)
    return snap


def snapshot(env, outs):
    return {"outs": raw(outs), "env": env_snapshot(env)}


def differing(a, b, prefix=""):
    """The keys under which two snapshots differ."""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        return [k for key in a for k in differing(a[key], b[key], f"{prefix}{key}.")]
    return [] if a == b else [prefix.rstrip(".")]


def dev(x, device):
    torch = _torch()
    return (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))).to(device).contiguous()


def reset(env, seed):
    r = env.reset(seed=seed)
    return r[0] if isinstance(r, tuple) else r


def null_run(make, seed, call, inputs, setup=None):
    """A twin env on the null stream with `inputs` (host arrays by name); returns the snapshot."""
    torch = _torch()
    env = make()
    try:
        reset(env, seed)
        if setup:
            setup(env)
        outs = call(env, {k: dev(v, env.device) for k, v in inputs.items()})
        torch.cuda.synchronize()
        return snapshot(env, outs)
    finally:
        torch.cuda.synchronize()
        env.close()


def side_run(make, seed, call, inputs, poison, setup=None, name=None):
    """The same on a side stream, the call behind a delay and its inputs late. Returns (snapshot, still)."""
    torch = _torch()
    s = torch.cuda.Stream()
    env = None
    try:
        with torch.cuda.stream(s):
            env = make()
            reset(env, seed)
            if setup:
                setup(env)
            src = {k: dev(v, env.device) for k, v in inputs.items()}
            bufs = {k: dev(v, env.device).clone() for k, v in poison.items()}
            torch.cuda.synchronize()
            ev = delay(s)
            for k in bufs:
                late(bufs[k], src[k])
            t0 = time.perf_counter()
            outs = call(env, bufs)
            ms = (time.perf_counter() - t0) * 1e3
            still = not ev.query()
            outs = clone_outputs(outs)
            s.synchronize()
            print(f"[stream-order] {name}: still={still} enqueue={ms:.3f} ms delay={STATS['delay_ms']:.1f} ms")
            if still and ms > STATS["max_enqueue_ms"]:
                STATS["max_enqueue_ms"], STATS["max_enqueue_case"] = ms, name
            return snapshot(env, outs), still
    finally:
        torch.cuda.synchronize()
        if env is not None:
            env.close()


def clone_outputs(x):
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, dict):
        return {k: clone_outputs(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(clone_outputs(v) for v in x)
    return x


_NULL = {}


def run_case(name, make, seed, call, inputs, poison, setup=None, expect_async=True, ref_key=None, ref_call=None):
    """The three runs of one case. `call(env, bufs)` gets device tensors by the names of `inputs` and returns the
    outputs (tensors, dicts, host values). `ref_key`: cases with the same key share their null-stream runs (they
    compute the same thing through different entry points; `ref_call` is the entry point those twins use).
    expect_async=False: the call is documented as waiting; its values are still compared."""
    ref_call = ref_call or call
    key = ref_key or name
    if key not in _NULL:
        ref = null_run(make, seed, ref_call, inputs, setup)
        poi = null_run(make, seed, ref_call, poison, setup)
        _NULL[key] = (ref, poi)
    ref, poi = _NULL[key]
    assert differing(ref["outs"], poi["outs"]) or differing(ref["env"], poi["env"]), \
        f"{name}: the poison twin equals the reference: the case is vacuous"
    got, still = side_run(make, seed, call, inputs, poison, setup, name)
    bad = differing(ref, got)
    assert not bad, (f"{name}: the side-stream run differs from the null-stream reference in {bad}"
                     + (" and equals the poison twin there" if not differing(poi["outs"], got["outs"]) else ""))
    if expect_async:
        assert still, f"{name}: the call returned only after the delay on its stream had ended: it is not asynchronous"
    return ref, poi, got, still
