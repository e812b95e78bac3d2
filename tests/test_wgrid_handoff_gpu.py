"""GPU parity of the windowed rollout's hand-off between the control wave and the env waves (csrc/wgrid.hip).

The control wave places a block's resetter cells by walking the env waves' ballot masks (lane s * 8 + w holds the
mask of slot s, env wave w; the exclusive scan of the popcounts is that segment's first rank) and publishes the same
prefixes for the env waves' own placement paths (blocks of <= 1,024 envs, and the slow path). It publishes the next
window's base before the transitions end, so the fills start as soon as the last env wave is through the window.

Every case compares each step's obs / reward / terminated / truncated, the final env state and the final PCG64 state
(numpy's buffered half-word included) with the numpy oracle through K-step launches of `rollout_plan`. 8,192 envs
are enough: the block geometry comes from the wg_block_envs knob (4,096-env blocks: control-wave cells, 8 slots per
lane; 2,048: 4 slots; default 512: env-wave cells through the published prefixes).
"""
import numpy as np
import pytest

from oracle import gridworld
from stream_plant import np_state, rejected_word, state_before, state_with_output_half

pytestmark = pytest.mark.gpu

B = 8192
GEOMS = {4096: dict(wg_block_envs=4096), 2048: dict(wg_block_envs=2048), 512: {}}
# wg_tmode bit reserved for the old-order switch of a two-stage outcome (the next window offset published ahead of
# the cells; DESIGN.md section 4, round 7: measured slower and taken out again). The kernel ignores the bit; the
# cases stay, so that a later attempt is tested in both orders.
OLD_HANDOFF = 32768


def _rng_tuple(st):
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = (1 << 64) - 1
    return [s >> 64, s & m, inc >> 64, inc & m, st["has_uint32"], st["uinteger"]]


def _check_chunks(env, ora, chunks, action_seed, n_act, before_chunk=None, max_resets=None):
    import torch
    rng = np.random.default_rng(action_seed)
    for ci, K in enumerate(chunks):
        if before_chunk:
            before_chunk(ci)
        a_np = rng.integers(0, n_act, (K, env.num_envs)).astype(np.int32)
        run, (obs, rew, term, trunc) = env.rollout_plan(torch.as_tensor(a_np, device=env.device))
        run()
        o, r, d, t = (x.cpu().numpy() for x in (obs, rew, term, trunc))
        for k in range(K):
            oo, ro, do, tro = ora.step_seeded(a_np[k].astype(np.int64))
            if max_resets is not None:  # the case is meant for the fast path: the slices must cover the resets
                assert int((np.asarray(do) | np.asarray(tro)).sum()) <= max_resets, (ci, k)
            np.testing.assert_array_equal(o[k].astype(np.int64), np.asarray(oo).astype(np.int64),
                                          err_msg=f"obs chunk {ci} K={K} k={k}")
            np.testing.assert_array_equal(r[k], ro, err_msg=f"rew chunk {ci} k={k}")
            np.testing.assert_array_equal(d[k], do, err_msg=f"term chunk {ci} k={k}")
            np.testing.assert_array_equal(t[k], tro, err_msg=f"trunc chunk {ci} k={k}")
    env.check()
    assert _rng_tuple(env.rng_state) == _rng_tuple(ora.gen.bit_generator.state)
    a, g, e = (x.cpu().numpy() for x in env.get_state())
    np.testing.assert_array_equal(a, np.ravel_multi_index(tuple(ora.agent.T), ora.grid.shape))
    np.testing.assert_array_equal(e, ora.elapsed)


def _pair(E, device, seed, **knobs):
    """An env of 8,192 envs in blocks of E and its oracle, both reset from `seed`."""
    from gym_po_amd import MultistoryFourRoomsEnv
    from gym_po_amd._lib import debug_knobs
    with debug_knobs(**GEOMS[E], **knobs):
        env = MultistoryFourRoomsEnv(B, grid_z=1, obs_type="hansen", device=device)
    assert env.query("wgrid") == 1
    assert env.query("wgrid_block_envs") == E and env.query("wgrid_blocks") == B // E
    ora = gridworld.FourRoomsOracle(B, 1, obs_type="hansen")
    r = env.reset(seed=seed)
    o = (r[0] if isinstance(r, tuple) else r).cpu().numpy()
    np.testing.assert_array_equal(o.astype(np.int64), np.asarray(ora.reset_seed(seed)).astype(np.int64))
    return env, ora


def _set_elapsed(env, ora, el):
    env.set_state(elapsed=el.astype(np.int32))
    ora.elapsed = el.astype(int)


@pytest.mark.parametrize("E,tmode", [(4096, 0), (4096, OLD_HANDOFF), (2048, 0), (2048, OLD_HANDOFF), (512, 0),
                                     (512, OLD_HANDOFF), (512, OLD_HANDOFF | 128), (512, OLD_HANDOFF | 16384)])
def test_plain_rollouts(E, tmode, gpu_device):
    """Launches of 1, 7, 12 and 2 steps from reset(seed), with and without the old-order bit (and, on 512-env blocks,
    without candidate cells and with the control wave placing the cells)."""
    env, ora = _pair(E, gpu_device, 19, wg_tmode=tmode)
    _check_chunks(env, ora, (1, 7, 12, 2), action_seed=6, n_act=4)
    assert env.metrics()["env_steps"] == B * 22


@pytest.mark.parametrize("E", [4096, 512])
def test_directed_ranks_fast_path(E, gpu_device):
    """Chosen envs truncate in the first step: all 64 envs of one (slot, wave) segment, three lanes of the next
    segment, the last env of block 0 and the first env of block 1. One control-wave lane walks 64 mask bits beside
    lanes with 0-3, block 1 has a non-zero prefix, and the ranks run past the start of the candidate window. The
    resets stay below the 124 G half-words the rejection slices cover, so the fast path places them."""
    env, ora = _pair(E, gpu_device, 29)
    seg = min(2, E // 512 - 1) * 512 + 3 * 64  # slot 2 (or the block's last slot), env wave 3
    el = np.zeros(B, np.int64)
    el[seg:seg + 64] = ora.time_limit
    el[[seg + 64 + 5, seg + 64 + 17, seg + 64 + 63]] = ora.time_limit
    el[[E - 1, E]] = ora.time_limit
    _set_elapsed(env, ora, el)
    _check_chunks(env, ora, (3, 5), action_seed=14, n_act=4, max_resets=124 * (B // E))


@pytest.mark.parametrize("E", [4096, 2048, 512])
def test_every_env_truncates_at_once(E, gpu_device):
    """b = 8,192 resets in the first step, more than the slices cover: the slow path with coverage rounds (the env
    waves place their resetters from the published prefixes), and a window regenerated in the same step."""
    env, ora = _pair(E, gpu_device, 37)
    assert B > 124 * (B // E)
    _set_elapsed(env, ora, np.full(B, ora.time_limit, np.int64))
    _check_chunks(env, ora, (3, 5), action_seed=15, n_act=4)


@pytest.mark.parametrize("E", [4096, 2048, 512])
@pytest.mark.parametrize("bias", [3000, -600])
def test_forced_window_misses(E, bias, gpu_device):
    """A biased prediction puts every step's window outside its halo: every step regenerates."""
    env, ora = _pair(E, gpu_device, 43, wg_bias=bias)
    _check_chunks(env, ora, (1, 7, 12, 2), action_seed=16, n_act=4)


@pytest.mark.parametrize("word", [3, 300])
@pytest.mark.parametrize("bias", [0, 3000])
def test_planted_rejection_inside_launch(word, bias, gpu_device):
    """Half-word `word` of the choice() stream of the middle launch's first step is a rejected Lemire draw (300 lies
    beyond the 248 half-words that two blocks' slices cover), without and with forced window misses."""
    env, ora = _pair(4096, gpu_device, 7, **({"wg_bias": bias} if bias else {}))
    n = len(ora.valid_agent)

    def plant(ci):
        if ci != 1:
            return
        inc = ora.gen.bit_generator.state["state"]["inc"]
        q, half = word >> 1, word & 1
        s_star = state_with_output_half(rejected_word(n), half, word)
        st = np_state(state_before(s_star, inc, B + q), inc)
        env.rng_state = st
        ora.gen.bit_generator.state = st

    _check_chunks(env, ora, (4, 9, 3), action_seed=21, n_act=4, before_chunk=plant)
