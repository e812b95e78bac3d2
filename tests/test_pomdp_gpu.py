"""GPU parity of the tabular POMDP backend (csrc/pomdp.hip) against the numpy oracle of the build-defined rules
(tests/pomdp_oracle.py, itself pinned to a scalar statement by tests/test_pomdp_cpu.py): bit-exact on obs, reward, both
flags, the state afterwards (state, elapsed, last obs), the four metrics and the philox step index.

Models (S, A, O): Tiger (2, 3, 2), rows shorter than one quad; (5, 2, 3); (37, 3, 21), 10 and 6 quads per row: the
binary search over an odd quad count; (300, 2, 70), states above 255 and the tables in global memory. One-step tables
over every (state, elapsed edge, obs, action in -A..A-1) with the draws predicted on the CPU; thresholds planted at the
predicted draws of each env and one above them; rollouts over two 1,024-env tiles with a ragged tail, split launches,
single steps and a prepared plan, a 3-env batch, blocks of a forced grid, blocks that loop over several tiles, caller
buffers off their boundaries; the model in LDS against the model in global memory; the refusals.
"""
import ctypes

import numpy as np
import pytest

from oracle.philox import env_step_words, philox_key
from pomdp_oracle import TAG, TIGER, TOP, PomdpOracle, Spec, oracle_rollout, random_model

pytestmark = pytest.mark.gpu

# Rewards are multiples of 0.25 (Tiger's: integers up to 100): every partial sum of the kernel's float64 accumulation
# (per thread over K steps x 4 envs x tiles, then 64 lanes, then 4 waves, then the slots) is a multiple of 0.25 far
# below 2^53 / 4 and therefore exact in any order, so return_sum compares with == against the float64 sum of the
# oracle's rewards. (Rewards that are no short binary fractions: tests/test_metrics_precision_gpu.py.)
MODELS = {"tiger": None, "m5": (5, 2, 3), "m37": (37, 3, 21), "m300": (300, 2, 70)}
# name -> the model blob is staged in LDS under the default budget (32 KB): m37's is 48,608 B, m300's 1.5 MB
DEFAULT_LDS = {"tiger": 1, "m5": 1, "m37": 0, "m300": 0}
_TABLES = {}


def _np(x):
    return x.cpu().numpy()


def tables(name):
    """(T, Z, R, start, terminal, reset_obs) of a model: made once, left unchanged."""
    if name not in _TABLES:
        if name == "tiger":
            from gym_po_amd import parse_pomdp
            m = parse_pomdp(TIGER)
            _TABLES[name] = (m["T"], m["Z"], m["R"].astype(np.float32), m["start"], np.zeros(2, dtype=bool),
                             np.full((2, 2), 0.5))
        else:
            S, A, O = MODELS[name]
            _TABLES[name] = random_model(S, A, O, seed=S, n_terminal=max(1, S // 8))
    return _TABLES[name]


def make(name, B, time_limit=7, **knobs):
    """An env of a model, under debug knobs if given, and its oracle."""
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import debug_knobs
    T, Z, R, start, terminal, reset_obs = tables(name)
    with debug_knobs(**knobs):
        env = TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs, time_limit=time_limit)
    return env, PomdpOracle(B, Spec.of_env(env))


def assert_outputs(dev, want, msg=""):
    for name, x, y in zip(("obs", "rew", "term", "trunc"), dev, want):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def assert_state(env, ora, msg=""):
    for name, x, y in zip(("state", "elapsed", "obs"), env.get_state(), (ora.state, ora.elapsed, ora.obs)):
        np.testing.assert_array_equal(_np(x), y, err_msg=f"{name} {msg}")


def assert_metrics(env, want):
    got = env.metrics()
    for k in ("episodes", "return_sum", "length_sum", "env_steps"):
        assert got[k] == want[k], f"{k}: device {got[k]} oracle {want[k]}"


# ------------------------------------------------------------------ one-step tables ----
@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_step_tables(name, gpu_device):
    tl, seed = 9, 5
    T = tables(name)[0]
    S, A, _ = T.shape
    O = tables(name)[1].shape[2]
    obs_values = sorted({0, O // 2, O - 1})
    s, el, ob, act = (x.ravel() for x in np.meshgrid(np.arange(S), np.array([0, tl - 1]), np.array(obs_values),
                                                     np.arange(-A, A), indexing="ij"))
    B = s.size
    env, ora = make(name, B, tl)
    assert env.single_action_space.n == A and env.single_observation_space.n == O
    assert env.query("pomdp_lds") == DEFAULT_LDS[name]
    env.seed(seed)
    key = philox_key(seed)
    step = env.query("philox_step")
    assert step == 0
    env.set_state(state=s, elapsed=el, obs=ob)
    ora.state[:], ora.elapsed[:], ora.obs[:] = s, el, ob
    assert_state(env, ora, "after set_state")
    o, r, d, tr, _ = env.step(act)
    draws = ora.philox_draws(step, key)  # predicted on the CPU for each env index
    want, m = oracle_rollout(ora, act[None], lambda k: draws)
    assert_outputs((o[None], r[None], d[None], tr[None]), want)
    assert_state(env, ora)
    assert_metrics(env, m)
    assert env.query("philox_step") == 1
    assert (want[3][0] == (el == tl - 1)).all() and want[3].any() and not want[3].all()
    if name != "tiger":
        assert want[2].any() and not want[2].all()
    assert len(np.unique(want[0])) == O if O <= 3 else len(np.unique(want[0])) > O // 2
    env.check()


# ------------------------------------------------------------------ planted edges ----
def plant(y, target, L):
    """A row of L thresholds under which the draw y counts exactly `target` entries, with the edge on both sides where
    the row has room: the entry before the edge equals y (counted: the comparison is >=), the entry after it y + 1 (not
    counted). target = 0: the first entry is y + 1. target = L - 1: every entry but the last equals y, the first
    included, and only the row's closing 2^31 (and the padding behind it) stays above."""
    y = int(y)
    row = np.full(L, TOP, dtype=np.int64)
    if target == L - 1:
        row[:L - 1] = y
    else:
        row[:target] = 0
        if target > 0:
            row[target - 1] = y
        row[target] = y + 1  # (<= 2^31; the last entry, if this is it, is 2^31 anyway)
        row[L - 1] = TOP
    return row


@pytest.mark.parametrize("lds_max,lds", [(0, 0), (60 * 1024, 1)], ids=["global", "lds"])
def test_planted_edges(lds_max, lds, gpu_device):
    """S = B = 67 (17 quads: the searched path), O = 21 (6 quads), A = 1; env e sits in state e. Row (e, 0) of trans_thr
    sends y0 of env e to a next state of its own, s'(e), with a threshold equal to y0 and one equal to y0 + 1 around the
    edge; row (0, s'(e)) of obs_thr does the same with y1 for an obs target; every third env truncates, and its y2 and
    y2 + 1 stand side by side in the one start row, its y3 in the reset-obs row of the start state that gives."""
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import debug_knobs
    S = B = 67
    O, tl, seed = 21, 9, 77
    key = philox_key(seed)
    y0, y1, y2, y3 = PomdpOracle.draws_of_words(*env_step_words(B, 0, TAG, key))
    e = np.arange(B)
    s_next = (e * 7 + 3) % S  # a permutation: one obs row per env
    assert len(set(s_next)) == S and {0, S - 1} <= set(s_next)
    o_next = e % O
    trans = np.full((S, 1, S), TOP, dtype=np.int64)
    obs = np.full((1, S, O), TOP, dtype=np.int64)
    for i in e:
        trans[i, 0] = plant(y0[i], s_next[i], S)
        obs[0, s_next[i]] = plant(y1[i], o_next[i], O)
    ends = e[e % 3 == 0]
    order = ends[np.argsort(y2[ends])]
    assert (np.diff(y2[order]) >= 2).all() and 2 * len(order) <= S - 1
    start = np.full(S, TOP, dtype=np.int64)
    start[0:2 * len(order):2] = y2[order]       # counted by its own env and by those above it
    start[1:2 * len(order):2] = y2[order] + 1   # not counted by its own env
    s0 = {int(d): 2 * k + 1 for k, d in enumerate(order)}
    robs = np.full((S, O), TOP, dtype=np.int64)
    for d in ends:
        robs[s0[int(d)]] = plant(y3[d], (O - 1 - d) % O, O)
    reward = (np.random.default_rng(0).integers(-8, 9, (S, 1, S)) * 0.25).astype(np.float32)
    with debug_knobs(pomdp_lds_max=lds_max):
        env = TabularPOMDPEnv.from_thresholds(B, trans.astype(np.uint32), obs.astype(np.uint32),
                                              start.astype(np.uint32), robs.astype(np.uint32), reward,
                                              np.zeros(S, dtype=bool), time_limit=tl)
    assert env.query("pomdp_lds") == lds and env.query("pomdp_model_bytes") == 49408
    ora = PomdpOracle(B, Spec.of_env(env))
    env.seed(seed)
    el = np.where(e % 3 == 0, tl - 1, 0)
    env.set_state(state=e, elapsed=el, obs=np.zeros(B, dtype=np.int64))
    ora.state[:], ora.elapsed[:], ora.obs[:] = e, el, 0
    act = np.where(e % 2 == 0, 0, -1)
    o, r, d, tr, _ = env.step(act)
    want, m = oracle_rollout(ora, act[None], lambda k: (y0, y1, y2, y3))
    # the plant did what it says (the oracle's count is pinned by the scalar statement)
    goes_on = e % 3 != 0
    assert np.array_equal(ora.state[goes_on], s_next[goes_on]) and np.array_equal(ora.obs[goes_on], o_next[goes_on])
    assert np.array_equal(ora.state[ends], [s0[int(x)] for x in ends])
    assert np.array_equal(ora.obs[ends], (O - 1 - ends) % O)
    assert np.array_equal(want[1][0], reward[e, 0, s_next]) and np.array_equal(want[3][0], ~goes_on)
    assert_outputs((o[None], r[None], d[None], tr[None]), want)
    assert_state(env, ora)
    assert_metrics(env, m)
    env.check()


# ------------------------------------------------------------------ rollouts ----
B0, K0, TL0, SEED0 = 1027, 40, 7, 12345
_REF = {}


def reference_run(name):
    """The oracle's 40-step run from the seed: computed once, shared, left unchanged."""
    if name not in _REF:
        env, ora = make(name, B0, TL0)
        env.close()
        key = philox_key(SEED0)
        obs0 = ora.reset(ora.philox_draws(0, key))
        state0 = ora.state.copy()
        A = env.single_action_space.n
        acts = np.random.default_rng(2).integers(0, A, (K0, B0)).astype(np.int32)
        want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
        assert (want[2] | want[3]).sum(0).min() >= 5 and want[3].any() and (name == "tiger" or want[2].any())
        _REF[name] = dict(obs0=obs0, state0=state0, acts=acts, want=want, metrics=m, ora=ora)
    return _REF[name]


def fresh(name, seed=SEED0, **knobs):
    env, _ = make(name, B0, TL0, **knobs)
    obs0 = _np(env.reset(seed=seed)[0])
    return env, obs0


def assert_is_reference(env, ref, msg=""):
    assert_state(env, ref["ora"], msg)
    assert_metrics(env, ref["metrics"])
    assert env.query("philox_step") == 1 + K0
    env.check()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_rollout_from_the_seed_vs_oracle(name, gpu_device):
    ref = reference_run(name)
    env, obs0 = fresh(name)
    np.testing.assert_array_equal(obs0, ref["obs0"])
    state, el, ob = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(state, ref["state0"])
    np.testing.assert_array_equal(ob, ref["obs0"])
    assert not el.any() and len(np.unique(state)) > 1
    assert_outputs(env.rollout(ref["acts"]), ref["want"])
    assert_is_reference(env, ref)


def test_split_launches_single_steps_and_plan(gpu_device):
    import torch
    ref = reference_run("m37")
    env, _ = fresh("m37")
    acts = torch.from_numpy(ref["acts"]).to(gpu_device)
    parts = [env.rollout(acts[a:b]) for a, b in ((0, 17), (17, 18), (18, 40))]
    assert_outputs([torch.cat([p[i] for p in parts]) for i in range(4)], ref["want"], "17 + 1 + 22")
    assert_is_reference(env, ref)
    env, _ = fresh("m37")
    steps = [env.step(acts[k])[:4] for k in range(K0)]
    assert_outputs([torch.stack([s[i] for s in steps]) for i in range(4)], ref["want"], "40 steps")
    assert_is_reference(env, ref)
    env, _ = fresh("m37")
    run, out = env.rollout_plan(acts)
    run()
    assert_outputs(out, ref["want"], "plan")
    assert_is_reference(env, ref)


def _short_run(name, B, seed, K, tl, **knobs):
    env, ora = make(name, B, tl, **knobs)
    key = philox_key(seed)
    np.testing.assert_array_equal(_np(env.reset(seed=seed)[0]), ora.reset(ora.philox_draws(0, key)))
    acts = np.random.default_rng(seed).integers(0, env.single_action_space.n, (K, B))
    dev = env.rollout(acts)
    want, m = oracle_rollout(ora, acts, lambda k: ora.philox_draws(k + 1, key))
    assert_outputs(dev, want)
    assert_state(env, ora)
    assert_metrics(env, m)
    assert env.query("philox_step") == 1 + K
    env.check()
    return env, m


@pytest.mark.parametrize("name", ["tiger", "m300"])
def test_three_envs(name, gpu_device):
    _, m = _short_run(name, 3, 31, 9, 4)
    assert m["episodes"] >= 2 * 3 and m["env_steps"] == 27


def test_forced_blocks_per_cu(gpu_device):
    """B = 9,221 is 10 tiles, the last with 5 envs. The knob forces the blocks per CU; on a device with more CUs than
    tiles the grid is then still one block per tile (the next test makes blocks loop)."""
    import torch
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    env, m = _short_run("tiger", 9221, 3, 12, 5, persist_bpc=1)
    assert env.query("persist_blocks") == min(cus, 10)
    assert m["episodes"] >= 2 * 9221


def test_blocks_looping_over_several_tiles(gpu_device):
    import torch
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B = 2 * 1024 * cus + 5
    env, m = _short_run("m5", B, 3, 6, 3, persist_bpc=1)
    assert env.query("persist_blocks") == cus and (B + 1023) // 1024 == 2 * cus + 1
    assert m["episodes"] >= B


def _offset_view(torch, dtype, shape, offset, device):
    """A contiguous tensor of `shape` that starts `offset` elements into a larger allocation."""
    n = int(np.prod(shape))
    v = torch.zeros(n + 8, dtype=dtype, device=device)[offset:offset + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def test_buffers_offset_by_one_element(gpu_device):
    """act / obs / rew / term / trunc views that start one element off their 16-B (4-B for the flags) boundaries take
    the element-wise load and store paths at every step, all together and each alone."""
    import torch
    ref = reference_run("m5")
    acts = torch.from_numpy(ref["acts"]).to(gpu_device)
    for offs in ((1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1)):
        env, _ = fresh("m5")
        act = _offset_view(torch, torch.int32, (K0, B0), offs[0], gpu_device)
        act.copy_(acts)
        out = (_offset_view(torch, torch.int32, (K0, B0), offs[1], gpu_device),
               _offset_view(torch, torch.float32, (K0, B0), offs[2], gpu_device),
               _offset_view(torch, torch.uint8, (K0, B0), offs[3], gpu_device),
               _offset_view(torch, torch.uint8, (K0, B0), offs[4], gpu_device))
        got = env.rollout(act, out=out)
        assert [x.data_ptr() for x in got] == [x.data_ptr() for x in out]  # written in place, not into copies
        assert_outputs(got, ref["want"], f"offsets={offs}")
        assert_is_reference(env, ref, f"offsets={offs}")


# ------------------------------------------------------------------ LDS path == global path ----
def test_model_in_lds_equals_model_in_global_memory(gpu_device):
    """pomdp_lds_max at exactly the blob's size stages it in LDS, one byte below leaves it in global memory; both give
    the reference run's bits. m37's blob (48,608 B) is above the default budget, Tiger's and m5's below it."""
    ref = reference_run("m37")
    env, _ = fresh("m37")
    nbytes = env.query("pomdp_model_bytes")
    assert nbytes == 48608 and env.query("pomdp_lds") == 0
    big, _ = make("m300", 8, pomdp_lds_max=1 << 22)  # the knob is capped at 60 KB: a 1.5 MB blob never goes into LDS
    assert big.query("pomdp_lds") == 0 and big.query("pomdp_model_bytes") == 300 * 2 * 300 * 8 + 4 * (
        2 * 300 * 72 + 300 + 300 * 72) + 304
    for knob, lds in ((nbytes, 1), (nbytes - 1, 0), (60 * 1024, 1), (1 << 20, 1)):
        env, obs0 = fresh("m37", pomdp_lds_max=knob)
        assert env.query("pomdp_lds") == lds, knob
        np.testing.assert_array_equal(obs0, ref["obs0"])
        assert_outputs(env.rollout(ref["acts"]), ref["want"], f"pomdp_lds_max={knob}")
        assert_is_reference(env, ref)
    for name in ("tiger", "m5"):
        ref = reference_run(name)
        env, _ = fresh(name)
        nbytes = env.query("pomdp_model_bytes")
        assert env.query("pomdp_lds") == 1 and nbytes == {"tiger": 304, "m5": 816}[name]
        for knob, lds in ((0, 0), (nbytes - 1, 0), (nbytes, 1)):
            env, _ = fresh(name, pomdp_lds_max=knob)
            assert env.query("pomdp_lds") == lds, (name, knob)
            assert_outputs(env.rollout(ref["acts"]), ref["want"], f"{name} pomdp_lds_max={knob}")
            assert_is_reference(env, ref)


# ------------------------------------------------------------------ reset, state, errors ----
def test_reset_goes_on_in_the_stream_and_state_round_trip(gpu_device):
    B = 1003
    env, ora = make("m37", B)
    S, O = 37, 21
    runs = []
    for seed in (7, 7, 8):
        obs0 = _np(env.reset(seed=seed)[0])
        np.testing.assert_array_equal(obs0, ora.reset(ora.philox_draws(0, philox_key(seed))))
        assert_state(env, ora)
        runs.append(obs0)
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], runs[2])
    env.reset()  # without a seed: the draws of step index 1
    ora.reset(ora.philox_draws(1, philox_key(8)))
    assert_state(env, ora)
    assert env.query("philox_step") == 2 and env.query("num_envs") == B and env.query("rng_mode") == 1
    assert env.query("persist_blocks") >= 1 and env.query("persist_occupancy") >= 1
    assert env.query("controller_nodes") == 0 and env.query("controller_lds") == 0
    # None leaves a field alone
    rng = np.random.default_rng(0)
    draw = lambda: dict(state=rng.integers(0, S, B), elapsed=rng.integers(0, 65536, B), obs=rng.integers(0, O, B))  # noqa: E731
    cur = draw()
    env.set_state(**cur)
    for given in ((), ("state",), ("elapsed",), ("obs",), ("state", "obs")):
        new = draw()
        env.set_state(**{k: new[k] for k in given})
        cur.update({k: new[k] for k in given})
        for name, x in zip(("state", "elapsed", "obs"), env.get_state()):
            np.testing.assert_array_equal(_np(x), cur[name], err_msg=f"{name} after set_state{given}")
    # out-of-range values are clamped
    st = np.resize(np.array([-1, -2 ** 31, S, 255, 65536, 2 ** 31 - 1, 0, S - 1]), B)
    ob = np.resize(np.array([-1, O, O - 1, 2 ** 31 - 1, 0]), B)
    env.set_state(state=st, elapsed=np.resize(np.array([-1, 65536, 65535, 2 ** 31 - 1]), B), obs=ob)
    s, e, o = (_np(x) for x in env.get_state())
    np.testing.assert_array_equal(s, np.clip(st, 0, S - 1))
    np.testing.assert_array_equal(e, np.resize(np.array([0, 65535, 65535, 65535]), B))
    np.testing.assert_array_equal(o, np.clip(ob, 0, O - 1))
    env.check()


def test_actions_wrap_or_flag(gpu_device):
    import torch
    from gym_po_amd._lib import GymPoError
    B, A = 1003, 3
    env, _ = make("m37", B)
    with pytest.raises(NotImplementedError):
        env.render()
    with pytest.raises(GymPoError, match="before reset"):
        env.step(np.zeros(B, dtype=np.int64))
    env.reset(seed=1)
    with pytest.raises(IndexError):
        env.step(np.full(B, A))
    with pytest.raises(IndexError):
        env.step(np.full(B, -A - 1))
    env.check()
    # action -k is action A - k
    twin, _ = make("m37", B)
    twin.reset(seed=1)
    neg = np.random.default_rng(0).integers(-A, 0, B)
    for x, y in zip(env.step(neg)[:4], twin.step(neg + A)[:4]):
        assert torch.equal(x, y)
    for x, y in zip(env.get_state(), twin.get_state()):
        assert torch.equal(x, y)
    env.check()
    # a device tensor with action A is clamped on the device and flags the handle; a re-seed clears the flag
    env.step(torch.full((B,), A, dtype=torch.int32, device=gpu_device))
    with pytest.raises(GymPoError, match=r"\(-5\).*action"):
        env.check()
    env.reset(seed=2)
    env.check()
    env.step(torch.full((B,), -A - 1, dtype=torch.int32, device=gpu_device))
    with pytest.raises(GymPoError, match=r"\(-5\).*action"):
        env.check()


def test_rng_modes_refused(gpu_device):
    from gym_po_amd import TabularPOMDPEnv
    from gym_po_amd._lib import GymPoError
    T, Z, R = tables("tiger")[:3]
    for mode in ("numpy", "replay"):
        with pytest.raises(GymPoError, match=r"\(-3\).*philox"):
            TabularPOMDPEnv(8, T, Z, R, rng_mode=mode)


def test_from_pomdp_tiger(gpu_device):
    from gym_po_amd import TabularPOMDPEnv
    env = TabularPOMDPEnv.from_pomdp(TIGER, 64, time_limit=7)
    ref, _ = make("tiger", 64)
    assert env.model["actions"] == ["listen", "open-left", "open-right"]
    for k in ("trans_thr", "obs_thr", "start_thr", "reset_obs_thr", "reward", "terminal"):
        assert np.array_equal(getattr(env, k), getattr(ref, k)), k
    assert env.obs_thr[0].tolist() == [[1825361100, TOP], [322122547, TOP]]
    assert env.trans_thr[:, 0].tolist() == [[TOP, TOP], [0, TOP]]
    assert np.array_equal(_np(env.reset(seed=3)[0]), _np(ref.reset(seed=3)[0]))


def _create_raw(S=2, A=2, O=2, time_limit=10, skip=None, **tables_):
    """gp_create on hand-made integer tables: every row [.., 2^31] unless given."""
    from gym_po_amd import _lib
    t = dict(trans_thr=np.full((S, A, S), TOP, dtype=np.uint32), obs_thr=np.full((A, S, O), TOP, dtype=np.uint32),
             start_thr=np.full(S, TOP, dtype=np.uint32), reset_obs_thr=np.full((S, O), TOP, dtype=np.uint32),
             reward=np.zeros((S, A, S), dtype=np.float32), terminal=np.zeros(S, dtype=np.uint8))
    t.update({k: np.ascontiguousarray(v, dtype=t[k].dtype) for k, v in tables_.items()})
    cfg = _lib.PomdpConfig()
    cfg.n_states, cfg.n_actions, cfg.n_obs, cfg.time_limit = S, A, O, time_limit
    for k, v in t.items():
        if k != skip:
            setattr(cfg, k, v.ctypes.data_as(type(getattr(cfg, k))))
    h = ctypes.c_void_p()
    rc = _lib.lib().gp_create(_lib.GP_KIND_POMDP, ctypes.byref(cfg), 8, 0, _lib.GP_RNG_PHILOX, ctypes.byref(h))
    msg = _lib.lib().gp_last_error().decode()
    if rc == 0:
        _lib.lib().gp_destroy(h)
    return rc, msg


def test_the_library_refuses_a_bad_config_by_name(gpu_device):
    assert _create_raw()[0] == 0
    assert _create_raw(S=1, A=1, O=1, time_limit=1)[0] == 0 and _create_raw(time_limit=65535)[0] == 0
    full = lambda shape: np.full(shape, TOP, dtype=np.uint32)  # noqa: E731
    bad_trans, bad_obs, bad_start, bad_robs = full((2, 2, 2)), full((2, 2, 2)), full(2), full((2, 2))
    bad_trans[1, 0] = [5, 4]
    bad_obs[1, 0] = [7, TOP - 1]
    bad_start[:] = [TOP, TOP - 1]
    bad_robs[1] = [TOP + 1, TOP + 1]
    for kw, match in [
        (dict(S=0), "sizes"), (dict(A=0), "sizes"), (dict(O=0), "sizes"), (dict(A=65), "sizes"),
        (dict(time_limit=0), "time_limit"), (dict(time_limit=65536), "time_limit"),
        (dict(skip="trans_thr"), "required"), (dict(skip="terminal"), "required"), (dict(skip="reward"), "required"),
        (dict(trans_thr=bad_trans), r"trans_thr row \(s 1, a 0\) is not nondecreasing within \[0, 2\^31\] at entry 1"),
        (dict(obs_thr=bad_obs), r"obs_thr row \(a 1, s' 0\) ends at 2147483647, not 2\^31"),
        (dict(start_thr=bad_start), r"start_thr row is not nondecreasing within \[0, 2\^31\] at entry 1"),
        (dict(reset_obs_thr=bad_robs), r"reset_obs_thr row \(s 1\) is not nondecreasing within \[0, 2\^31\] at entry 0"),
    ]:
        rc, msg = _create_raw(**kw)
        import re
        assert rc == -1 and re.search(match, msg), (kw, rc, msg)
    # the padded tables' entry limit, refused before anything is read: S A Sp = 2^28 + ... for S = 16,388, A = 1
    for kw in (dict(S=16388, A=1, O=1), dict(S=4100, A=1, O=65536)):
        from gym_po_amd import _lib
        cfg = _lib.PomdpConfig()
        cfg.n_states, cfg.n_actions, cfg.n_obs, cfg.time_limit = kw["S"], kw["A"], kw["O"], 10
        one = np.zeros(4, dtype=np.uint32)
        for k in ("trans_thr", "obs_thr", "start_thr", "reset_obs_thr", "reward", "terminal"):
            setattr(cfg, k, one.ctypes.data_as(type(getattr(cfg, k))))
        h = ctypes.c_void_p()
        rc = _lib.lib().gp_create(_lib.GP_KIND_POMDP, ctypes.byref(cfg), 8, 0, _lib.GP_RNG_PHILOX, ctypes.byref(h))
        assert rc == -1 and "too large (max 2^28 each)" in _lib.lib().gp_last_error().decode(), kw
