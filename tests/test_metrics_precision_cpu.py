"""CPU test of the reference of tests/test_metrics_precision_gpu.py: at the very shapes and rewards the GPU cases use,
the bound N * 2^-52 * sum|r| of gp_metrics' return_sum (include/gym_po_amd.h) must tell the two summation laws apart.

`float32_law` (tests/metrics_reference.py) restates the accumulation the library had before: a float32 chain per thread,
float32 reductions over lanes and waves, float64 only at the slot. It must fall outside the bound at every case.
`float64_law`, the law the header states, must stay inside it. The planes here are synthetic (the env is not restated):
every env-step earns one of the case's rewards, the step reward most often, as a rollout does. What is being tested is
the arithmetic, which sees only the values and their order.

The counters: thread 0's block totals were 32-bit; at B = G = 1,024 and K = 2^22 + 5 they wrap, 64-bit ones do not.
"""
import numpy as np
import pytest

import metrics_reference as mr

CUS = 256  # the device's CU count sets the looping cases' B = 2 * tile * CUs + 5
F32 = np.float32


def reward_values(kind):
    """The float32 rewards a kind can pay, the step reward first."""
    if kind == "pomdp":
        return (np.random.default_rng(5).random(5 * 2 * 5).astype(F32) - F32(0.3)).astype(F32)  # m5's R table law
    r = mr.REWARDS[kind]
    step = [v for k, v in r.items() if k in ("step_reward", "reward_any")]
    return np.array(step + [v for v in r.values() if v not in step], dtype=F32)


def plane(kind, K, B, seed):
    """rew float32 [K, B]: the first value (the step reward) on about 70 % of the env-steps, the others evenly."""
    vals = reward_values(kind)
    rng = np.random.default_rng(seed)
    if kind == "pomdp":
        idx = rng.integers(0, len(vals), (K, B))
    else:
        u = rng.random((K, B), dtype=np.float32)
        idx = np.where(u < 0.7, 0, 1 + (u * 1009).astype(np.int64) % (len(vals) - 1))
    return vals[idx]


def exact_and_bound(launches):
    """The reference return and the bound of a run given as its launches' rew planes (no episode ends)."""
    rew = np.concatenate(launches)
    none = np.zeros(rew.shape, dtype=bool)
    want = mr.want_metrics(rew, none, none)
    return want["return_sum"], want["bound"]


def check_laws(launches, grid, tile=mr.TILE, what=""):
    exact, bound = exact_and_bound(launches)
    e32 = mr.float32_law(launches, grid, tile) - exact
    e64 = mr.float64_law(launches, grid, tile) - exact
    print(f"{what}: exact {exact!r} bound {bound:.3e} float32 law error {e32:.3e} float64 law error {e64:.3e}")
    assert abs(e64) <= bound, f"{what}: the float64 law misses its own bound: {e64:.3e} > {bound:.3e}"
    assert abs(e32) > bound, f"{what}: the float32 law is inside the bound: the case cannot tell the laws apart"
    return e32, e64, bound


KINDS = sorted(mr.REWARDS) + ["pomdp"]


@pytest.mark.parametrize("kind", KINDS)
def test_small_stored_planes(kind):
    """Part a: B = 1,027, K = 257, one block per tile (C-ROOMS: 512-env tiles, three blocks)."""
    tile = 512 if kind == "crooms" else mr.TILE
    rew = plane(kind, mr.K_SMALL, mr.B_SMALL, seed=1)
    assert len(set(np.unique(rew))) >= 2
    e32, _, bound = check_laws([rew], -(-mr.B_SMALL // tile), tile, kind)
    assert abs(e32) > 100 * bound  # not a near miss: orders of magnitude


@pytest.mark.parametrize("kind", ["rocksample", "pomdp", "crooms"])
def test_blocks_looping_over_tiles(kind):
    """Part a, blocks of a one-per-CU grid looping over two tiles (block 0 over a third, ragged one): the thread's
    chain runs on across tiles."""
    tile = 512 if kind == "crooms" else mr.TILE
    B = 2 * tile * CUS + 5
    rew = plane(kind, mr.K_LOOP, B, seed=2)
    check_laws([rew], CUS, tile, f"{kind} looping")


def test_many_single_steps():
    """Part d: 300 launches of one step: four float32 additions per thread and a float32 block reduction each."""
    rew = plane("heavenhell", mr.N_SINGLE_STEPS, mr.B_SMALL, seed=3)
    check_laws([rew[k:k + 1] for k in range(mr.N_SINGLE_STEPS)], 2, what="300 single steps")


@pytest.mark.parametrize("tile", [4096, 1024, 512])
def test_count_based_epilogues(tile):
    """Part b: the numpy-exact grid kernels count goal, wall and plain steps per thread and multiply once per launch.
    In float32 that is one rounding per product and per addition: about 2^-24 relative, against a bound of
    N * 2^-52."""
    B, vals = mr.B_GRID, reward_values("grid")  # step, wall, goal
    rng = np.random.default_rng(4)
    got32 = got64 = 0.0
    planes = []
    for K in mr.GRID_CHUNKS:
        kind = rng.choice(3, (K, B), p=(0.7, 0.25, 0.05))
        planes.append(vals[kind])
        counts = np.stack([(kind == j).sum(0) for j in range(3)])
        got32 += mr.count_law(counts, vals, B // tile, np.float32, tile)
        got64 += mr.count_law(counts, vals, B // tile, np.float64, tile)
    exact, bound = exact_and_bound(planes)
    print(f"blocks of {tile}: exact {exact!r} bound {bound:.3e} float32 {got32 - exact:.3e} float64 {got64 - exact:.3e}")
    assert abs(got64 - exact) <= bound
    assert abs(got32 - exact) > bound


def test_long_launch_of_a_constant_reward():
    """Part c: K = 65,536 steps of float32(0.1) at B = 1,027, nothing stored: every full thread adds the same value
    262,144 times. The exact return is B * K * float64(float32(0.1)), whatever the trajectory."""
    K, B, v = mr.K_LONG, mr.B_SMALL, mr.CONSTANT_REWARD
    exact = B * K * float(v)
    bound = B * K * 2.0 ** -52 * abs(exact)
    e32 = mr.constant_law(K, B, v, 2, np.float32) - exact
    e64 = mr.constant_law(K, B, v, 2, np.float64) - exact
    print(f"constant 0.1f: exact {exact!r} bound {bound:.3e} float32 {e32:.3e} float64 {e64:.3e}")
    assert abs(e64) <= bound
    assert abs(e32) > bound and abs(e32) / exact > 1e-3  # the systematic bias of a float32 chain of this length
    # and over the twin's 64 launches of 1,024 steps the float32 law misses it too
    part = mr.constant_law(K // mr.LONG_PARTS, B, v, 2, np.float32)
    assert abs(part * mr.LONG_PARTS - exact) > bound


def test_long_launch_of_varying_rewards():
    """Part c: K = 16,384 at B = 1,027 with the tabular model's rewards."""
    rew = plane("pomdp", mr.K_LONG_VARYING, mr.B_SMALL, seed=6)
    check_laws([rew], 2, what="K = 16,384 varying")


def test_want_metrics_counts():
    """episodes, length_sum and env_steps on a plane small enough to count by hand, numpy and torch alike."""
    import torch
    term = np.array([[0, 0, 1], [1, 0, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0]], dtype=np.uint8)
    trunc = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 1, 1]], dtype=np.uint8)
    rew = (np.arange(15, dtype=F32).reshape(5, 3) * F32(0.1)).astype(F32)
    # env 0: one episode of 2 steps; env 1: one of 5; env 2: episodes of 1, 2 and 2 steps
    want = dict(episodes=5, length_sum=2 + 5 + 5, env_steps=15)
    for got in (mr.want_metrics(rew, term, trunc),
                mr.want_metrics(torch.from_numpy(rew), torch.from_numpy(term), torch.from_numpy(trunc).bool())):
        assert {k: got[k] for k in want} == want
        assert got["return_sum"] == pytest.approx(float(rew.astype(np.float64).sum()), abs=1e-12)
        assert got["bound"] == 15 * 2.0 ** -52 * float(np.abs(rew.astype(np.float64)).sum())
    c = mr.EpisodeCounter(3, "cpu")
    c.add(torch.from_numpy(term[:2]), torch.from_numpy(trunc[:2]))
    c.add(torch.from_numpy(term[2:]), torch.from_numpy(trunc[2:]))
    assert c.result() == want


def test_block_totals_of_2_pow_32_env_steps():
    """A 1,024-env block that runs K = 2^22 + 5 steps in one launch: the per-thread counts (4 K) fit 32 bits, their
    block total does not. Summed in 32 bits from the wave shuffle on it wraps to 5,120; in 64 bits it is B * K."""
    K, B = (1 << 22) + 5, 1024
    per_thread = np.full(B // mr.EPT, mr.EPT * K, dtype=np.uint64)
    assert int(per_thread.max()) < 1 << 32
    assert int(per_thread.astype(np.uint32).sum(dtype=np.uint32)) == 5120 != B * K
    assert int(per_thread.sum(dtype=np.uint64)) == B * K
