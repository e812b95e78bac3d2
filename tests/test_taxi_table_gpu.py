"""Taxi (csrc/taxi.hip) against the reference's one-step tables and on directed trajectories.

The env step exists three times on the device -- taxi_env_step (philox / replay rollout kernel), pass 1 of the
one-workgroup taxi_np_kernel, and taxi_npg_pass1 / taxi_npg_pass2 (numpy mode grid-wide) -- over one host-lowered
table trans[s * 6 + a] and obs_of[s]. Random walks hardly reach a goal move, so here

  (a) every (state, action) row of the `taxi_table` fixtures (tests/golden/make_golden.py: the reference stepped once
      on every state, invalid ones included, every action -5..4, elapsed {0, tl-1, tl} x every dropoff count) goes
      through each step copy in ONE launch: outputs, the full post-state, the counts of the rare rows, the metrics;
  (b) a greedy pickup -> dropoff policy (BFS over the oracle's table) drives trajectories in which every 1,024-env
      tile completes tasks and terminates, in numpy mode from the seed alone (both numpy kernels) and in philox mode
      closed-loop on the device's own state, with a K-step rollout of the recorded actions against the single steps;
  (c) all four metrics are compared after every such run;
  (d) act / rew / term / trunc / obs views off their vector alignment take the scalar and the narrower one-hot paths;
  (e) blocks loop over several 1,024-env tiles;
  (f) the 4-bit dropoff count saturates instead of spilling into elapsed.

Everything is compared with ==. The metrics' return_sum is a float64 sum from the thread on: with the dyadic
rewards used here (multiples of 0.25, |r| <= 2) every partial sum is a multiple of 0.25 far below 2^53 / 4, hence exact
in any order (the one-workgroup numpy kernel sums its whole batch in one block, the grid-wide one adds its blocks'
totals atomically). Rewards that are no short binary fractions: tests/test_metrics_precision_gpu.py.
"""
import contextlib
import functools

import numpy as np
import pytest

from fixtures import load_index, load_table, taxi_table_counts, taxi_table_inputs
from oracle.draws import NumpyDraws, ReplayDraws
from taxi_table_oracle import (greedy_policy, make_oracle, metrics_of_step, new_metrics, per_tile_floor,
                               policy_rollout_numpy, rare_rows, replay_draws, set_rows)

pytestmark = pytest.mark.gpu

TABLES = sorted(load_index()["taxi_table"])
TAXI_MAP_TABLES = [n for n in TABLES if load_index()["taxi_table"][n]["kwargs"]["map"] == "TAXI"]
DYADIC = dict(reward_goal=2.0, reward_bad=-1.0, reward_any=-0.25)
DIRECTED = dict(map="TAXI", hansen_obs=True, num_passengers=2, time_limit=24, **DYADIC)
K_DIRECTED = 48
ONE_WG = 1 << 30  # debug_knobs(taxi_npg_min=...): every batch on the one-workgroup numpy kernel


def _env(kw, B, **extra):
    from gym_po_amd import TaxiVecEnv
    from gym_po_amd.maps import EXTENDED_TAXI_MAP, TAXI_MAP
    kw = dict(kw)
    m = kw.pop("map", "TAXI")
    return TaxiVecEnv(B, map=TAXI_MAP if m == "TAXI" else EXTENDED_TAXI_MAP if m == "EXTENDED" else tuple(m), **kw,
                      **extra)


def _numpy_env(kw, B, one_wg=False, **extra):
    from gym_po_amd._lib import debug_knobs
    with debug_knobs(taxi_npg_min=ONE_WG) if one_wg else contextlib.nullcontext():
        return _env(kw, B, rng_mode="numpy", **extra)


def _np(x):
    return x.cpu().numpy()


def _rng6(st):
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = (1 << 64) - 1
    return [s >> 64, s & m, inc >> 64, inc & m, int(st["has_uint32"]), int(st["uinteger"])]


def _rng_dict(r6):
    r6 = [int(v) for v in r6]
    return {"bit_generator": "PCG64", "state": {"state": (r6[0] << 64) | r6[1], "inc": (r6[2] << 64) | r6[3]},
            "has_uint32": r6[4], "uinteger": r6[5]}


@functools.lru_cache(maxsize=None)
def _table(name):
    meta, data = load_table(name)
    return meta, {k: data[k] for k in data.files}, taxi_table_inputs(meta)


@functools.lru_cache(maxsize=None)
def _policy():
    return greedy_policy(DIRECTED)


@functools.lru_cache(maxsize=None)
def _numpy_run(B, seed=3):
    return policy_rollout_numpy(DIRECTED, B, seed, K_DIRECTED, _policy())


def _assert_obs(env, o, ref, msg=""):
    """Scalar obs == ref; one-hot rows == eye(n_obs)[ref] (compared on the device). Any leading shape."""
    import torch
    ref = np.asarray(ref).astype(np.int64)
    if env.one_hot:
        eye = torch.eye(env.no, dtype=torch.uint8, device=o.device)
        assert o.shape == ref.shape + (env.no,) and o.dtype == torch.uint8
        assert torch.equal(o, eye[torch.as_tensor(ref, device=o.device)]), f"one-hot obs {msg}"
    else:
        np.testing.assert_array_equal(_np(o).astype(np.int64), ref, err_msg=f"obs {msg}")


def _assert_outputs(env, out, ref, msg=""):
    _assert_obs(env, out[0], ref[0], msg)
    np.testing.assert_array_equal(_np(out[1]), np.asarray(ref[1], dtype=np.float32), err_msg=f"rew {msg}")
    np.testing.assert_array_equal(_np(out[2]).astype(bool), np.asarray(ref[2], bool), err_msg=f"term {msg}")
    np.testing.assert_array_equal(_np(out[3]).astype(bool), np.asarray(ref[3], bool), err_msg=f"trunc {msg}")


def _assert_state(env, s, elapsed, n_dropoffs, msg=""):
    gs, ge, gn = (_np(x).astype(np.int64) for x in env.get_state())
    np.testing.assert_array_equal(gs, np.asarray(s).astype(np.int64), err_msg=f"s {msg}")
    np.testing.assert_array_equal(ge, np.asarray(elapsed).astype(np.int64), err_msg=f"elapsed {msg}")
    np.testing.assert_array_equal(gn, np.asarray(n_dropoffs).astype(np.int64), err_msg=f"n_dropoffs {msg}")


def _assert_metrics(env, m, msg=""):
    assert env.metrics() == {k: float(v) for k, v in m.items()}, msg


def _set_rows(env, s, e, n):
    """set_state must read back unchanged through get_state."""
    env.set_state(s=s.astype(np.int32), elapsed=e.astype(np.int32), n_dropoffs=n.astype(np.int32))
    _assert_state(env, s, e, n, "after set_state")


def _assert_table_step(env, name, out, post=None):
    """One step over the table's rows against the fixture (`post`: compare obs and the post-state with these oracle
    values instead -- philox mode, whose draws are the device's own)."""
    meta, data, (s, a, e, n) = _table(name)
    ref = (data["obs"], data["rew"], data["term"], data["trunc"]) if post is None else post[0]
    _assert_outputs(env, out, ref, name)
    for k in ("rew", "term", "trunc"):  # never drawn: the reference's in every mode
        np.testing.assert_array_equal(np.asarray(ref[("obs", "rew", "term", "trunc").index(k)]), data[k])
    st = (data["s"], data["elapsed"], data["n_dropoffs"]) if post is None else post[1]
    _assert_state(env, *st, name)
    # no mode passes by skipping the rare rows: counted on the device's outputs
    got = taxi_table_counts(meta, a, _np(out[1]), _np(out[2]), _np(out[3]))
    assert got == meta["counts"], f"{name}: rare rows {got}"
    rare = ("goal", "bad", "pick", "term", "trunc") + (("task",) if meta["kwargs"]["num_passengers"] > 1 else ())
    assert min(sum(got[k]) for k in rare) > 0  # (one passenger: the only dropoff ends the episode, no task row)
    _assert_metrics(env, metrics_of_step(new_metrics(), e, data["rew"], data["term"], data["trunc"]), name)


def test_table_widths_reach_every_one_hot_stream():
    """The one-hot stream writes 16-, 4- or 1-byte chunks by the row width (TaxiBackend::chunk_size)."""
    widths = {n: load_index()["taxi_table"][n]["n_obs"] for n in TABLES}
    cs = {n: 16 if w % 16 == 0 else 4 if w % 4 == 0 else 1 for n, w in widths.items()}
    assert set(cs.values()) == {16, 4, 1}, widths
    assert widths["taxi_table_r_g_plain_2p"] == 18 and widths["taxi_table_rg_plain_2p"] == 12


# ------------------------------------------------------------------ (a) the tables ----
@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("name", TABLES)
def test_table_replay(name, one_hot, gpu_device):
    """taxi_rollout<*, REPLAY>: the recorded post-states handed back as the draws, as run_replay does."""
    meta, data, (s, a, e, n) = _table(name)
    env = _env(meta["kwargs"], meta["num_envs"], rng_mode="replay", one_hot=one_hot, device=gpu_device)
    post = data["s"].astype(np.int32)
    env.set_replay(reset_states=post, pd=post % (env.nlocs * (env.nlocs + 1)))
    env.reset()
    _set_rows(env, s, e, n)
    out = env.step(a)[:4]
    _assert_table_step(env, name, out)
    env.check()


def _numpy_table(name, one_hot, one_wg, device):
    meta, data, (s, a, e, n) = _table(name)
    env = _numpy_env(meta["kwargs"], meta["num_envs"], one_wg=one_wg, one_hot=one_hot, device=device)
    env.reset(seed=meta["seed"])  # the device's own reset burst reaches the recorded pre-step stream
    assert _rng6(env.rng_state) == [int(v) for v in data["pre_rng_state"]]
    env.rng_state = _rng_dict(data["pre_rng_state"])
    _set_rows(env, s, e, n)
    out = env.step(a)[:4]
    _assert_table_step(env, name, out)
    env.check()
    assert _rng6(env.rng_state) == [int(v) for v in data["rng_state"]]


@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("name", TABLES)
def test_table_numpy(name, one_hot, gpu_device):
    """From the recorded stream alone: taxi_npg_* above 1,024 envs (every table but the 720 rows of ("RG",), which
    take the one-workgroup kernel)."""
    _numpy_table(name, one_hot, False, gpu_device)


@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("name", TAXI_MAP_TABLES)
def test_table_numpy_one_workgroup(name, one_hot, gpu_device):
    """taxi_np_kernel forced on the TAXI map's 15,000 / 30,000 rows (its buffers are sized by the batch)."""
    _numpy_table(name, one_hot, True, gpu_device)


@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("name", TABLES)
def test_table_philox(name, one_hot, gpu_device):
    """taxi_rollout<*, false>: the device's own draws, read back and fed to the oracle; and those draws themselves:
    every reset lands in a valid start state, every task completion keeps the taxi's cell (the oracle encodes its
    own cell with the device's pair, so s would differ) and draws p < L, p != d."""
    meta, data, (s, a, e, n) = _table(name)
    B = meta["num_envs"]
    env = _env(meta["kwargs"], B, rng_mode="philox", one_hot=one_hot, device=gpu_device)
    env.reset(seed=meta["seed"])
    _set_rows(env, s, e, n)
    out = env.step(a)[:4]
    post_s = _np(env.get_state()[0]).astype(np.int64)
    ora = make_oracle(meta["kwargs"], B)
    set_rows(ora, s, e, n)
    ref = ora.step(a, replay_draws(ora, post_s))
    _assert_table_step(env, name, out, post=(ref, (ora.s, ora.elapsed, ora.n_dropoffs_completed)))
    fin = ref[2] | ref[3]
    task = (ref[1] == np.float32(ora.GOAL_MOVE)) & ~fin
    assert fin.any() and (task.any() or meta["kwargs"]["num_passengers"] == 1)
    assert np.isin(post_s[fin], ora.valid_states).all(), "reset into an invalid state"
    _, _, p, d = ora.decode(post_s[task])
    assert (p < ora.nlocs).all() and (p != d).all()
    env.check()


# ------------------------------------------------------------------ (b), (c) directed trajectories ----
def _floors(run_ora, outs):
    rr = rare_rows(run_ora, outs[1], outs[2], outs[3])
    totals = {k: int(v.sum()) for k, v in rr.items()}
    floor = per_tile_floor(rr)
    assert min(floor.values()) >= 1, f"a 1,024-env tile without a rare row: per-tile minimum {floor}, totals {totals}"
    return f"totals {totals}, per-tile minimum {floor}"


@pytest.mark.parametrize("one_wg", [False, True], ids=["grid_wide", "one_workgroup"])
def test_directed_numpy_rollout(one_wg, gpu_device):
    """The oracle runs from the seed under the policy; ONE device rollout of its actions reproduces everything. With
    B = 4,099 the k * B plane of every buffer changes alignment at every step."""
    B = 4099
    run = _numpy_run(B)
    report = _floors(run["ora"], run["outs"])
    env = _numpy_env(DIRECTED, B, one_wg=one_wg, device=gpu_device)
    o0, _ = env.reset(seed=3)
    _assert_obs(env, o0, run["obs0"], "reset")
    out = env.rollout(run["acts"])
    _assert_outputs(env, out, run["outs"], report)
    _assert_state(env, *run["states"][-1], report)
    env.check()
    assert _rng6(env.rng_state) == _rng6(run["ora"].gen.bit_generator.state)
    _assert_metrics(env, run["metrics"], report)


@pytest.mark.parametrize("B", [1027, 4099])
def test_directed_philox_closed_loop(B, gpu_device):
    """Step by step: the policy picks each action from the device's own state, the device's draws go to the oracle;
    then one K-step rollout of the recorded actions on a same-seed handle must equal the steps."""
    import torch
    pol, K, seed = _policy(), K_DIRECTED, 7
    env = _env(DIRECTED, B, rng_mode="philox", device=gpu_device)
    ora = make_oracle(DIRECTED, B)
    o0, _ = env.reset(seed=seed)
    s0 = _np(env.get_state()[0]).astype(np.int64)
    assert np.isin(s0, ora.valid_states).all()
    set_rows(ora, s0, np.zeros(B), np.zeros(B))
    _assert_obs(env, o0, ora.obs(), "reset")
    acts, steps, refs, m = [], [], [], new_metrics()
    post_s = s0
    for k in range(K):
        a = pol[post_s]  # chosen from the device's state
        el0 = ora.elapsed.copy()
        out = env.step(a)[:4]
        post_s = _np(env.get_state()[0]).astype(np.int64)
        ref = ora.step(a, replay_draws(ora, post_s))
        _assert_outputs(env, out, ref, f"k={k}")
        _assert_state(env, ora.s, ora.elapsed, ora.n_dropoffs_completed, f"k={k}")
        fin = ref[2] | ref[3]
        assert np.isin(post_s[fin], ora.valid_states).all(), f"k={k}: reset into an invalid state"
        _, _, p, d = ora.decode(post_s[(ref[1] == np.float32(ora.GOAL_MOVE)) & ~fin])
        assert (p < ora.nlocs).all() and (p != d).all(), f"k={k}"
        metrics_of_step(m, el0, ref[1], ref[2], ref[3])
        acts.append(a)
        steps.append(out)
        refs.append(ref)
    report = _floors(ora, [np.stack(x) for x in zip(*refs)])
    _assert_metrics(env, m, report)
    twin = _env(DIRECTED, B, rng_mode="philox", device=gpu_device)
    twin.reset(seed=seed)
    whole = twin.rollout(np.stack(acts))
    for i, nm in enumerate(("obs", "rew", "term", "trunc")):
        assert torch.equal(whole[i], torch.stack([s[i] for s in steps])), nm
    for x, y in zip(twin.get_state(), env.get_state()):
        assert torch.equal(x, y)
    _assert_metrics(twin, m, report)


# ------------------------------------------------------------------ (d) store paths ----
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


def _store_path_cases(one_hot):
    """Byte shifts of (act, obs, rew, term, trunc): each buffer alone at every shift, then all together."""
    obs_shifts = (4, 1) if one_hot else (4, 8, 12)  # 320-wide rows: 4 -> the 4-byte stream, 1 -> the byte stream
    cases = []
    for i, shifts in enumerate(((4, 8, 12), obs_shifts, (4, 8, 12), (1, 2, 3), (1, 2, 3))):
        for sh in shifts:
            c = [0] * 5
            c[i] = sh
            cases.append(tuple(c))
    return cases + [(4, obs_shifts[0], 8, 1, 3), (12, obs_shifts[-1], 4, 3, 2), (8, obs_shifts[1], 12, 2, 1)]


@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("mode", ["philox", "numpy"])
def test_misaligned_caller_buffers(mode, one_hot, gpu_device):
    """quad_ok's scalar fallbacks (per buffer and per step: B = 4,099 moves every k * B plane) and chunk_size's
    pointer test, against an aligned run of the same seed; GUARD bytes around every view catch a store outside it."""
    import torch
    B, K, seed = 4099, 26, 3  # 26 steps under the policy: goal moves, terminations, and truncation at step 25
    env = (_numpy_env(DIRECTED, B, one_hot=one_hot, device=gpu_device) if mode == "numpy" else
           _env(DIRECTED, B, rng_mode="philox", one_hot=one_hot, device=gpu_device))
    if mode == "numpy":
        acts = _numpy_run(B)["acts"][:K]
    else:  # the policy on the device's own states, step by step
        pol, acts = _policy(), []
        env.reset(seed=seed)
        for _ in range(K):
            acts.append(pol[_np(env.get_state()[0]).astype(np.int64)])
            env.step(acts[-1])
    acts = torch.as_tensor(np.stack(acts).astype(np.int32), device=gpu_device)
    env.reset(seed=seed)
    ref = [x.clone() for x in env.rollout(acts)]
    ref_state = [x.clone() for x in env.get_state()]
    ref_metrics = env.metrics()
    assert ref_metrics["env_steps"] == K * B and ref_metrics["episodes"] >= B
    assert bool((ref[1] == 2.0).any()) and bool(ref[2].any()) and bool(ref[3].any())
    if mode == "numpy":  # the aligned run itself is the reference's
        _assert_outputs(env, ref, [x[:K] for x in _numpy_run(B)["outs"]])
    oshape = (K, B, env.no) if one_hot else (K, B)
    odt = torch.uint8 if one_hot else torch.int32
    for shifts in _store_path_cases(one_hot):
        env.reset(seed=seed)
        bufs = [_offset_view(torch, dt, shp, sh, gpu_device) for dt, shp, sh in zip(
            (torch.int32, odt, torch.float32, torch.uint8, torch.uint8), ((K, B), oshape, (K, B), (K, B), (K, B)),
            shifts)]
        bufs[0][0].copy_(acts)
        got = env.rollout(bufs[0][0], out=tuple(b[0] for b in bufs[1:]))
        for nm, x, y in zip(("obs", "rew", "term", "trunc"), got, ref):
            assert torch.equal(x, y), f"{nm} shifts={shifts}"
        for nm, (v, raw, lo) in zip(("act", "obs", "rew", "term", "trunc"), bufs):
            assert _guards_intact(raw, lo, v.numel() * v.element_size()), f"{nm} guard bytes, shifts={shifts}"
        assert torch.equal(bufs[0][0], acts)
        for x, y in zip(ref_state, env.get_state()):
            assert torch.equal(x, y), f"state shifts={shifts}"
        assert env.metrics() == ref_metrics, f"metrics shifts={shifts}"
    env.check()


# ------------------------------------------------------------------ (e) several tiles per block ----
@functools.lru_cache(maxsize=None)
def _multi_tile_run(B, K=4):
    """A replay-fed oracle run under the policy from every state (invalid ones too), elapsed 0..2 and 0 or 1
    dropoffs: goal moves, task completions, terminations and truncations in every tile within K steps."""
    kw = dict(DIRECTED, time_limit=2)
    ora = make_oracle(kw, B)
    rng = np.random.default_rng(12)
    L = ora.nlocs
    pairs = np.array([p * L + d for p in range(L) for d in range(L) if p != d])
    draws = [dict(reset_state=rng.integers(0, ora.ns, B), pd=rng.choice(pairs, B)) for _ in range(K + 1)]
    obs0 = np.asarray(ora.reset(ReplayDraws(draws[0])))
    start = (ora.s.copy(), rng.integers(0, 3, B), rng.integers(0, 2, B))
    set_rows(ora, *start)
    pol, outs, m = _policy(), [], new_metrics()
    acts = []
    for k in range(K):
        a = pol[ora.s]
        el0 = ora.elapsed.copy()
        o, r, d, tr = ora.step(a, ReplayDraws(draws[k + 1]))
        metrics_of_step(m, el0, r, d, tr)
        acts.append(a)
        outs.append((np.asarray(o), r, d, tr))
    return dict(kw=kw, draws=draws, obs0=obs0, start=start, acts=acts, outs=outs, metrics=m,
                state=(ora.s.copy(), ora.elapsed.copy(), ora.n_dropoffs_completed.copy()), ora=ora)


@pytest.mark.parametrize("one_hot", [False, True])
def test_blocks_looping_over_several_tiles(one_hot, gpu_device):
    import torch
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B = 2 * 1024 * cus + 5
    run = _multi_tile_run(B)
    with debug_knobs(persist_bpc=1):
        env = _env(run["kw"], B, rng_mode="replay", one_hot=one_hot, device=gpu_device)
    assert env.query("persist_blocks") == cus and (B + 1023) // 1024 == 2 * cus + 1  # 2 tiles a block, block 0 a third
    d0 = run["draws"][0]
    env.set_replay(reset_states=d0["reset_state"].astype(np.int32), pd=d0["pd"].astype(np.int32))
    o0, _ = env.reset()
    _assert_obs(env, o0, run["obs0"], "reset")
    del o0
    _set_rows(env, *run["start"])
    for k, (a, ref) in enumerate(zip(run["acts"], run["outs"])):
        dk = run["draws"][k + 1]
        env.set_replay(reset_states=dk["reset_state"].astype(np.int32), pd=dk["pd"].astype(np.int32))
        out = env.step(a)[:4]
        _assert_outputs(env, out, ref, f"k={k}")
        del out
    _assert_state(env, *run["state"])
    rr = rare_rows(run["ora"], *(np.stack([o[i] for o in run["outs"]]) for i in (1, 2, 3)))
    assert min(per_tile_floor(rr).values()) >= 1 and np.stack([o[3] for o in run["outs"]]).any()
    _assert_metrics(env, run["metrics"])


# ------------------------------------------------------------------ (f) the dropoff count's 4 bits ----
@pytest.mark.parametrize("mode", ["replay", "numpy_grid_wide", "numpy_one_workgroup"])
def test_dropoff_count_saturates_at_15(mode, gpu_device):
    """set_state stores n_dropoffs up to 15 in a 4-bit field. A goal move from 15 used to carry into bit 16, the low
    bit of elapsed (elapsed 0 read back 1, the count 0): with 3 passengers the reference counts on to 16, never
    terminates, and redraws the passengers. The count now saturates at 15 in all three step copies; s, elapsed, the
    rewards and both flags follow the oracle over two steps of every state under action 4, elapsed 0, 1 and tl."""
    from gym_po_amd._lib import debug_knobs
    kw = dict(map="TAXI", num_passengers=3, time_limit=4, **DYADIC)
    ora0 = make_oracle(kw, 1)
    ns = ora0.ns
    s = np.tile(np.arange(ns), 3)
    e = np.repeat([0, 1, 4], ns)
    B = s.size
    n = np.full(B, 15)
    a = np.full(B, 4)
    ora = make_oracle(kw, B)
    if mode == "replay":
        env = _env(kw, B, rng_mode="replay", device=gpu_device)
        rng = np.random.default_rng(5)
        L = ora.nlocs
        pairs = np.array([p * L + d for p in range(L) for d in range(L) if p != d])
        draws = [dict(reset_state=rng.choice(ora.valid_states, B), pd=rng.choice(pairs, B)) for _ in range(2)]
        env.set_replay(reset_states=draws[0]["reset_state"].astype(np.int32), pd=draws[0]["pd"].astype(np.int32))
        env.reset()
    else:
        with debug_knobs(taxi_npg_min=0 if mode == "numpy_grid_wide" else ONE_WG):
            env = _env(kw, B, rng_mode="numpy", device=gpu_device)
        env.reset(seed=9)
        ora.reset_seed(9)
    _set_rows(env, s, e, n)
    set_rows(ora, s, e, n)
    goals = 0
    for k in range(2):
        if mode == "replay":
            env.set_replay(reset_states=draws[k]["reset_state"].astype(np.int32), pd=draws[k]["pd"].astype(np.int32))
            dr = ReplayDraws(draws[k])
        else:
            dr = NumpyDraws(ora.gen)
        out = env.step(a)[:4]
        ref = ora.step(a, dr)
        goals += int(((ref[1] == np.float32(2.0)) & ~ref[3]).sum())
        assert not ref[2].any()  # 16 dropoffs are not 3
        _assert_outputs(env, out, ref, f"k={k}")
        _assert_state(env, ora.s, ora.elapsed, np.minimum(ora.n_dropoffs_completed, 15), f"k={k}")
    assert goals >= 8  # goal moves at elapsed 0 and 1 went on from a count of 15
    env.check()
    if mode != "replay":
        assert _rng6(env.rng_state) == _rng6(ora.gen.bit_generator.state)
