"""GPU parity of the grid Ant-Tag backend (csrc/anttag.hip) against the numpy oracle of the build's spec.

Ant-Tag has no numpy reference (the reference env is a MuJoCo robot): the oracle restates the
build-defined grid rules (oracle/anttag.py; parity unpinned with respect to the reference). Both
philox mode (the oracle recomputes the device's Philox4x32-10 counters in numpy) and replay mode
must match the oracle bit-for-bit, at ragged and large batch sizes.

The oracle itself is pinned to an independent scalar statement of the spec on the CPU (tests/test_oracle_anttag.py).
Beyond random trajectories from reset states, the tests below put the device through every (ant cell, target cell,
action, choose) of arenas from 2 x 2 to 16 x 16 (the largest stages 64 KB + 256 B of dynamic LDS on top of the
kernel's 16 KB of static LDS), non-default radii and rewards with all four metrics, set_state / get_state, batch
sizes around the 4-env quads and 1,024-env tiles, caller buffers that force the scalar load / store paths, blocks
that loop over several tiles, and split launches.
"""
import math

import numpy as np
import pytest

from oracle.anttag import AntTagOracle
from oracle.philox import philox_key

pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy()


@pytest.mark.parametrize("B,T,tl", [(1000 + 3, 300, 60), (1 << 16, 120, 500), (4096, 700, 500)])
def test_philox_bit_exact_vs_oracle(B, T, tl, gpu_device):
    import torch
    from gym_po_amd import AntTagGridEnv
    env = AntTagGridEnv(B, time_limit=tl)
    ora = AntTagOracle(B, time_limit=tl)
    seed = 12345
    key = philox_key(seed)
    o = env.reset(seed=seed)[0]
    oo = ora.reset(ora.philox_draws(0, key))
    np.testing.assert_array_equal(_np(o), oo)
    rng = np.random.default_rng(2)
    acts = rng.integers(0, 5, (T, B))
    eps = 0
    for t in range(T):
        o, r, d, tr, _ = env.step(acts[t])
        ro, rr, rd, rt = ora.step(acts[t], ora.philox_draws(t + 1, key))
        np.testing.assert_array_equal(_np(o), ro, err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(r), rr, err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(d), rd, err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(tr), rt, err_msg=f"t={t}")
        eps += int((rd | rt).sum())
    a, tg, e = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(a, ora.ant)
    np.testing.assert_array_equal(tg, ora.target)
    np.testing.assert_array_equal(e, ora.elapsed)
    assert env.metrics()["episodes"] == eps


def test_replay_bit_exact_and_rollout(gpu_device):
    import torch
    from gym_po_amd import AntTagGridEnv
    B, T = 2049, 80
    env = AntTagGridEnv(B, time_limit=30, rng_mode="replay")
    ora = AntTagOracle(B, time_limit=30)
    rng = np.random.default_rng(9)

    def draws():
        ant = rng.integers(0, 100, B)
        return dict(choose=rng.integers(0, 4, B), ant=ant, tgt=rng.integers(0, 40, B))

    dr = draws()
    env.set_replay(choose=dr["choose"], ant=dr["ant"], target_idx=dr["tgt"])
    np.testing.assert_array_equal(_np(env.reset()[0]), ora.reset(dr))
    acts = rng.integers(-5, 5, (T, B))
    for t in range(T):
        dr = draws()
        env.set_replay(choose=dr["choose"], ant=dr["ant"], target_idx=dr["tgt"])
        o, r, d, tr, _ = env.step(acts[t])
        ro, rr, rd, rt = ora.step(acts[t], dr)
        np.testing.assert_array_equal(_np(o), ro, err_msg=f"t={t}")
        np.testing.assert_array_equal(_np(r), rr)
        np.testing.assert_array_equal(_np(d), rd)
        np.testing.assert_array_equal(_np(tr), rt)


def test_philox_rollout_equals_single_steps(gpu_device):
    import torch
    from gym_po_amd import AntTagGridEnv
    B, K = 10007, 50
    a, b = AntTagGridEnv(B, time_limit=25), AntTagGridEnv(B, time_limit=25)
    a.reset(seed=1)
    b.reset(seed=1)
    acts = torch.randint(0, 5, (K, B), dtype=torch.int32, device=gpu_device)
    ro, rr, rd, rt = a.rollout(acts)
    for t in range(K):
        o, r, d, tr, _ = b.step(acts[t])
        assert torch.equal(o, ro[t]) and torch.equal(r, rr[t]) and torch.equal(d, rd[t]) and torch.equal(tr, rt[t])


# ------------------------------------------------------------------ helpers of the tests below ----
def _oracle_for(env, B, **kw):
    """The oracle of `env`'s config, built from the squared radii the env reports."""
    return AntTagOracle(B, size=env.size, tag_radius2=env.tag_radius2, visible_radius2=env.visible_radius2,
                        min_start_dist2=env.min_start_dist2, time_limit=env.time_limit, **kw)


def _oracle_rollout(ora, acts, draws):
    """len(acts) oracle steps with draws(k): the stacked outputs and the four metrics the device accumulates
    (length_sum: the episode length of every env that finished, i.e. its elapsed before the same-step reset)."""
    outs, m = [], dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)
    for k in range(len(acts)):
        el0 = ora.elapsed.copy()
        o, r, d, tr = ora.step(acts[k], draws(k))
        fin = d | tr
        m["episodes"] += int(fin.sum())
        m["length_sum"] += int((el0[fin] + 1).sum())
        m["return_sum"] += float(r.astype(np.float64).sum())
        m["env_steps"] += ora.B
        outs.append((o, r, d, tr))
    return [np.stack(x) for x in zip(*outs)], m


def _assert_outputs(dev, want, msg=""):
    for name, x, y in zip(("obs", "rew", "term", "trunc"), dev, want):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def _assert_state(env, ora, msg=""):
    a, tg, e = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(a, ora.ant, err_msg=f"ant {msg}")
    np.testing.assert_array_equal(tg, ora.target, err_msg=f"target {msg}")
    np.testing.assert_array_equal(e, ora.elapsed, err_msg=f"elapsed {msg}")


def _assert_metrics(env, want):
    got = env.metrics()
    for k in ("episodes", "return_sum", "length_sum", "env_steps"):
        assert got[k] == want[k], f"{k}: device {got[k]} oracle {want[k]}"


# Dyadic rewards: every partial sum of the kernel's float64 accumulation (per thread over K steps x 4 envs x tiles, then
# 64 lanes, then 4 waves, then the slots) is a multiple of 0.25 far below 2^53 / 4 and therefore exact in any order, so
# return_sum compares with == against the float64 sum of the oracle's rewards. (Rewards that are no short binary
# fractions, and the bound they are held to: tests/test_metrics_precision_gpu.py.)
DYADIC = dict(tag_reward=2.0, step_reward=-0.25)


# ------------------------------------------------------------------ every transition, sizes 2..16 ----
@pytest.mark.parametrize("size,min_distance", [(2, 0.0), (3, 1.0), (5, 2.0), (7, 3.0), (10, 5.0), (13, 5.0),
                                               (15, 5.0), (16, 5.0), (16, 0.0)])
def test_every_transition_one_step_vs_oracle(size, min_distance, gpu_device):
    from gym_po_amd import AntTagGridEnv
    nc = size * size
    ant, tgt, act, cho = (x.ravel() for x in np.meshgrid(np.arange(nc), np.arange(nc), np.arange(5), np.arange(4),
                                                         indexing="ij"))
    B = ant.size
    assert B == nc * nc * 20 and B <= 1310720
    env = AntTagGridEnv(B, size=size, min_distance=min_distance, rng_mode="replay", **DYADIC)
    ora = _oracle_for(env, B, **DYADIC)
    # sizes 15 and 16 stage more than 64 KB of LDS per block: the occupancy query must still find room for a block
    assert env.query("persist_occupancy") >= 1 and env.query("persist_blocks") >= 1
    if (size, min_distance) == (16, 0.0):  # the u8 count table at its cap
        assert all(len(v) == 255 for v in ora.valid_targets)
    rng = np.random.default_rng(size)
    want_m = dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)
    for el0 in (0, env.time_limit - 1):
        dr = dict(choose=cho, ant=rng.integers(0, nc, B), tgt=rng.integers(0, nc + 8, B))  # tgt: often past the list
        assert (dr["tgt"] >= ora._cnt[dr["ant"]]).any()
        env.set_replay(choose=dr["choose"], ant=dr["ant"], target_idx=dr["tgt"])
        env.set_state(ant, tgt, np.full(B, el0))
        ora.ant[:], ora.target[:], ora.elapsed[:] = ant, tgt, el0
        o, r, d, tr, _ = env.step(act)
        want, m = _oracle_rollout(ora, act[None], lambda k: dr)
        _assert_outputs((o[None], r[None], d[None], tr[None]), want, msg=f"elapsed={el0}")
        _assert_state(env, ora, msg=f"elapsed={el0}")
        assert want[2].any() and want[3].all() == (el0 > 0) and want[3].any() == (el0 > 0)
        for k in want_m:
            want_m[k] += m[k]
    _assert_metrics(env, want_m)  # the second step counts term & trunc together as one episode each
    env.check()


# ------------------------------------------------------------------ radii, rewards, all four metrics ----
def test_squared_radii_of_the_config(gpu_device):
    """tag: d^2 <= floor(r^2); visible: d^2 < ceil(r^2); start: d^2 > floor(r^2) (hand-computed integers)."""
    from gym_po_amd import AntTagGridEnv
    for radius, r2 in ((1.0, 1), (1.5, 2), (2.0, 4), (math.sqrt(5.0), 5)):
        assert AntTagGridEnv(8, tag_radius=radius).tag_radius2 == r2
    for radius, r2 in ((1.0, 1), (3.0, 9), (20.0, 400), (1.5, 3)):
        assert AntTagGridEnv(8, visible_radius=radius).visible_radius2 == r2
    for radius, r2 in ((0, 0), (5, 25), (6.5, 42)):
        assert AntTagGridEnv(8, min_distance=radius).min_start_dist2 == r2


def test_min_distance_12_is_refused(gpu_device):
    """No 10 x 10 cell has a cell farther than 12 from it (the diagonal is sqrt(162) = 12.7, and only from a corner):
    the device refuses the config (GP_E_INVALID, naming min_start_dist2 = 144) and so does the oracle."""
    from gym_po_amd import AntTagGridEnv
    from gym_po_amd._lib import GymPoError
    with pytest.raises(GymPoError, match=r"no target cell farther than sqrt\(144\)"):
        AntTagGridEnv(4099, min_distance=12)
    with pytest.raises(ValueError, match=r"no target cell farther than sqrt\(144\)"):
        AntTagOracle(4099, min_start_dist2=144)


@pytest.mark.parametrize("tag_radius,visible_radius,min_distance,time_limit,elapsed0", [
    (1.0, 3.0, 5, 60, None), (1.5, 1.0, 0, 60, None), (2.0, 20.0, 6.5, 60, None), (math.sqrt(5.0), 3.0, 5, 60, None),
    (1.5, 20.0, 0, 1, None), (2.0, 1.0, 5, 65535, 65533)])
def test_radii_rewards_and_metrics_vs_oracle(tag_radius, visible_radius, min_distance, time_limit, elapsed0,
                                             gpu_device):
    from gym_po_amd import AntTagGridEnv
    B, T, seed = 4099, 100, 77
    env = AntTagGridEnv(B, size=10, tag_radius=tag_radius, visible_radius=visible_radius, min_distance=min_distance,
                        time_limit=time_limit, **DYADIC)
    ora = _oracle_for(env, B, **DYADIC)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    if elapsed0 is not None:
        env.set_state(elapsed=np.full(B, elapsed0))
        ora.elapsed[:] = elapsed0
    acts = np.random.default_rng(seed).integers(0, 5, (T, B))
    dev = env.rollout(acts)
    want, m = _oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    _assert_outputs(dev, want)
    _assert_state(env, ora)
    assert m["env_steps"] == T * B and m["episodes"] > 0 and want[2].any()
    if time_limit == 1:
        assert m["episodes"] == T * B and m["length_sum"] == T * B
    if elapsed0 is not None:  # the first truncation is the 65535th step of the episode
        assert want[3][1].all() and not want[3][0].any() and m["length_sum"] > 65535 * (B // 2)
    if visible_radius == 20.0:
        assert (want[0][..., 2:] >= 0).all()
    _assert_metrics(env, m)


# ------------------------------------------------------------------ set_state / get_state ----
def test_set_state_get_state(gpu_device):
    from gym_po_amd import AntTagGridEnv
    from gym_po_amd._lib import GymPoError
    B, nc, seed = 1003, 100, 8
    env = AntTagGridEnv(B, time_limit=9)
    ora = _oracle_for(env, B)
    rng = np.random.default_rng(1)
    acts = rng.integers(0, 5, (2, B))
    env.seed(seed)
    with pytest.raises(GymPoError, match="before reset"):
        env.step(acts[0])

    def rand():
        return dict(ant=rng.integers(0, nc, B), target=rng.integers(0, nc, B), elapsed=rng.integers(0, 65536, B))

    cur = rand()
    env.set_state(**cur)  # makes step legal without a reset
    for name, x in zip(("ant", "target", "elapsed"), env.get_state()):
        np.testing.assert_array_equal(_np(x), cur[name], err_msg=name)
    # None leaves a field (its bytes of the packed word) alone: each field alone, and each pair
    for given in (("ant",), ("target",), ("elapsed",), ("ant", "target"), ("ant", "elapsed"), ("target", "elapsed")):
        new = rand()
        env.set_state(**{k: new[k] for k in given})
        cur.update({k: new[k] for k in given})
        for name, x in zip(("ant", "target", "elapsed"), env.get_state()):
            np.testing.assert_array_equal(_np(x), cur[name], err_msg=f"{name} after set_state{given}")
    # out-of-range values are clamped: cells to [0, ncells - 1], elapsed to [0, 65535]
    cells = np.resize(np.array([-1, -1000, -2 ** 31, nc, nc + 5, 255, 256, 65536 + 3, 2 ** 31 - 1, 0, nc - 1]), B)
    els = np.resize(np.array([-1, -70000, -2 ** 31, 65536, 65535, 65534, 2 ** 31 - 1, 1 << 16 | 5, 0]), B)
    env.set_state(ant=cells, target=cells[::-1].copy(), elapsed=els)
    a, tg, e = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(a, np.clip(cells, 0, nc - 1))
    np.testing.assert_array_equal(tg, np.clip(cells[::-1], 0, nc - 1))
    np.testing.assert_array_equal(e, np.clip(els, 0, 65535))
    # a step from a set state (never reset) follows the oracle: the first launch after seed() is philox step 0
    st = dict(ant=rng.integers(0, nc, B), target=rng.integers(0, nc, B), elapsed=rng.integers(0, 9, B))
    env.set_state(**st)
    ora.ant[:], ora.target[:], ora.elapsed[:] = st["ant"], st["target"], st["elapsed"]
    key = philox_key(seed)
    dev = env.rollout(acts)
    want, m = _oracle_rollout(ora, acts, lambda k: ora.philox_draws(k, key))
    _assert_outputs(dev, want)
    _assert_state(env, ora)
    _assert_metrics(env, m)


# ------------------------------------------------------------------ batch shapes, store paths, launches ----
@pytest.mark.parametrize("B", [1, 3, 4, 5, 1023, 1024, 1025, 4 * 1024 + 2])
def test_batch_shapes_one_rollout_vs_oracle(B, gpu_device):
    from gym_po_amd import AntTagGridEnv
    K, seed = 9, 31
    env = AntTagGridEnv(B, time_limit=4, **DYADIC)
    ora = _oracle_for(env, B, **DYADIC)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(B).integers(0, 5, (K, B))
    dev = env.rollout(acts)
    want, m = _oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    _assert_outputs(dev, want)
    _assert_state(env, ora)
    assert m["episodes"] >= 2 * B
    _assert_metrics(env, m)


def _offset_view(torch, dtype, shape, offset, device):
    """A contiguous tensor of `shape` that starts `offset` elements into a larger allocation."""
    n = int(np.prod(shape))
    v = torch.zeros(n + 8, dtype=dtype, device=device)[offset:offset + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def test_misaligned_caller_buffers(gpu_device):
    """act / rew / term / trunc views that start off their 16-B (4-B for the flags) boundaries take the scalar load
    and store paths at every step, all of them together and each alone (the kernel chooses per buffer and per
    step); the results must equal the aligned run's. An obs view off its 16-B boundary is refused before anything
    is launched."""
    import torch
    from gym_po_amd import AntTagGridEnv
    from gym_po_amd._lib import GymPoError
    B, K, seed = 4096, 5, 13
    a, b = (AntTagGridEnv(B, time_limit=3, **DYADIC) for _ in range(2))
    a.reset(seed=seed)
    acts = torch.randint(0, 5, (K, B), dtype=torch.int32, device=gpu_device)
    ref = a.rollout(acts)
    assert all(x.data_ptr() % 16 == 0 for x in ref) and acts.data_ptr() % 16 == 0
    ref_state, ref_metrics = a.get_state(), a.metrics()
    assert ref_metrics["episodes"] > 0

    def bufs(o_act, o_rew, o_term, o_trunc):
        act = _offset_view(torch, torch.int32, (K, B), o_act, gpu_device)
        act.copy_(acts)
        return act, (torch.zeros((K, B, 4), dtype=torch.int32, device=gpu_device),
                     _offset_view(torch, torch.float32, (K, B), o_rew, gpu_device),
                     _offset_view(torch, torch.uint8, (K, B), o_term, gpu_device),
                     _offset_view(torch, torch.uint8, (K, B), o_trunc, gpu_device))

    # offsets in elements of (act, rew, term, trunc); term and trunc differ in the first
    for offs in ((1, 1, 1, 3), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 2)):
        b.reset(seed=seed)
        act, out = bufs(*offs)
        if offs == (1, 1, 1, 3):
            # the refusal: nothing runs, the env stays usable, its state and stream position unchanged
            before = [x.clone() for x in b.get_state()]
            bad_obs = _offset_view(torch, torch.int32, (K, B, 4), 1, gpu_device)
            with pytest.raises(GymPoError, match="16-B aligned"):
                b.rollout(act, out=(bad_obs,) + out[1:])
            for x, y in zip(b.get_state(), before):
                assert torch.equal(x, y)
            assert b.metrics()["env_steps"] == 0
        got = b.rollout(act, out=out)
        assert [x.data_ptr() for x in got] == [x.data_ptr() for x in out]  # written in place, not into copies
        assert got[1].data_ptr() % 16 == 4 * offs[1] and got[2].data_ptr() % 4 == offs[2]
        assert got[3].data_ptr() % 4 == offs[3]
        for name, x, y in zip(("obs", "rew", "term", "trunc"), got, ref):
            assert torch.equal(x, y), f"{name} offsets={offs}"
        for x, y in zip(ref_state, b.get_state()):
            assert torch.equal(x, y), f"state offsets={offs}"
        assert b.metrics() == ref_metrics
    b.check()


def test_blocks_looping_over_several_tiles(gpu_device):
    import torch
    from gym_po_amd import AntTagGridEnv
    from gym_po_amd._lib import debug_knobs
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B, K, seed = 2 * 1024 * cus + 5, 6, 3
    with debug_knobs(persist_bpc=1):
        env = AntTagGridEnv(B, time_limit=3, **DYADIC)
    ntiles = (B + 1023) // 1024
    blocks = env.query("persist_blocks")
    assert blocks == cus and ntiles == 2 * cus + 1  # every block handles 2 tiles, block 0 a third, ragged one
    ora = _oracle_for(env, B, **DYADIC)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(seed).integers(0, 5, (K, B))
    dev = env.rollout(acts)
    want, m = _oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    _assert_outputs(dev, want)
    _assert_state(env, ora)
    assert m["episodes"] >= B
    _assert_metrics(env, m)


def test_split_launches_continue_the_philox_counter(gpu_device):
    import torch
    from gym_po_amd import AntTagGridEnv
    B, seed = 4099, 21
    a, b = (AntTagGridEnv(B, time_limit=6, **DYADIC) for _ in range(2))
    a.reset(seed=seed)
    b.reset(seed=seed)
    acts = torch.randint(0, 5, (20, B), dtype=torch.int32, device=gpu_device)
    whole = a.rollout(acts)
    first, second = b.rollout(acts[:7]), b.rollout(acts[7:])
    for name, w, x, y in zip(("obs", "rew", "term", "trunc"), whole, first, second):
        assert torch.equal(w, torch.cat([x, y])), name
    for x, y in zip(a.get_state(), b.get_state()):
        assert torch.equal(x, y)
    assert a.metrics() == b.metrics() and a.metrics()["env_steps"] == 20 * B and a.metrics()["episodes"] >= 3 * B


def test_replay_rollout_equals_steps_and_oracle(gpu_device):
    """Replay mode with K > 1 goes through the generic per-step rollout: K launches reading the installed draws."""
    import torch
    from gym_po_amd import AntTagGridEnv
    B, K = 2049, 3
    a, b = (AntTagGridEnv(B, time_limit=2, min_distance=0, rng_mode="replay", **DYADIC) for _ in range(2))
    ora = _oracle_for(a, B, **DYADIC)
    rng = np.random.default_rng(17)
    dr = dict(choose=rng.integers(0, 4, B), ant=rng.integers(0, 100, B), tgt=rng.integers(0, 120, B))
    want0 = ora.reset(dr)
    for env in (a, b):
        env.set_replay(choose=dr["choose"], ant=dr["ant"], target_idx=dr["tgt"])
        np.testing.assert_array_equal(_np(env.reset()[0]), want0)
    acts = rng.integers(-5, 5, (K, B))
    whole = a.rollout(acts)
    steps = [b.step(acts[k])[:4] for k in range(K)]
    for i, name in enumerate(("obs", "rew", "term", "trunc")):
        assert torch.equal(whole[i], torch.stack([s[i] for s in steps])), name
    want, m = _oracle_rollout(ora, acts, lambda k: dr)
    _assert_outputs(whole, want)
    for env in (a, b):
        _assert_state(env, ora)
        _assert_metrics(env, m)
    assert m["episodes"] >= B and want[2].any()
