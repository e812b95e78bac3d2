"""ORACLE / TEST INFRASTRUCTURE — the reference of gp_metrics (include/gym_po_amd.h) from the planes a run emitted, the
bound its return_sum carries, and numpy restatements of two summation laws over the rollout kernels' geometry.

The env is not restated here. `want_metrics` takes the rew / term / trunc planes [K, B] of a run that starts at reset()
and gives the four counters: the three integers exactly, return_sum as the float64 sum of the float32 rewards, and the
bound N * 2^-52 * sum|r| (N = K * B env-steps) that a float64 accumulation in any order keeps: n - 1 additions of
relative error 2^-53 each perturb the sum by at most (n - 1) * 2^-53 * sum|r| (1 + O(n 2^-53)), under half the bound.

`float32_law` restates how the library summed before the float64 law: a sequential float32 chain per thread (its 4
consecutive envs, K steps, every tile its block loops over), a float32 xor-butterfly over the 64 lanes of a wave, the
waves' partials added in order in float32, and only the block's total widened to float64 for the slot. `float64_law`
is the same walk in float64. tests/test_metrics_precision_cpu.py holds both against the bound at the shapes the GPU
tests use: the first must miss it, the second must keep it.
"""
import math

import numpy as np

# ---- the shapes and rewards of tests/test_metrics_precision_gpu.py (the CPU test holds both laws at the same ones) ----
B_SMALL, K_SMALL = 1027, 257          # two 1,024-env tiles, the last quad ragged
K_LOOP = 13                           # blocks looping over tiles: B = 2 * tile * CUs + 5 envs
B_GRID, GRID_CHUNKS = 8192, (1, 7, 12)
K_LONG, LONG_PARTS = 65536, 64        # store=() launches; the twin runs them as 64 launches of 1,024
K_LONG_VARYING = 16384
N_SINGLE_STEPS = 300
CONSTANT_REWARD = np.float32(0.1)
# no reward is a short binary fraction: float32 sums of them round at every addition
STEP, WALL, GOAL = -0.1, -0.3, 0.7
REWARDS = {
    "grid": dict(step_reward=STEP, wall_reward=WALL, goal_reward=GOAL),
    "crooms": dict(step_reward=STEP, wall_reward=WALL, goal_reward=GOAL),
    "rocksample": dict(exit_reward=GOAL, good_reward=1.3, bad_reward=-1.7, empty_reward=-0.9, check_reward=-0.05,
                       step_reward=STEP, wall_reward=WALL),
    "heavenhell": dict(heaven_reward=GOAL, hell_reward=-1.1, step_reward=STEP, wall_reward=WALL),
    "anttag": dict(tag_reward=GOAL, step_reward=STEP),
    "taxi": dict(reward_goal=GOAL, reward_bad=WALL, reward_any=STEP),
}

EPT = 4          # consecutive envs per thread
TILE = 1024      # envs per tile of the streaming rollout kernels (C-ROOMS: 512)
FSUM_MAX = 1 << 21  # planes up to this many entries are summed by math.fsum (correctly rounded)


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def want_metrics(rew, term, trunc):
    """The counters of a run from reset() as a dict: episodes, length_sum, env_steps (int), return_sum (float), and
    `bound`. rew float32 [K, B], term / trunc bool or uint8 [K, B]: numpy arrays, or torch tensors (reduced on their
    device in int64 / float64; a float64 tree sum of n terms errs by at most log2(n) * 2^-53 * sum|r|, far inside the
    bound)."""
    if _is_torch(rew):
        import torch
        K, B = rew.shape
        done = term.to(torch.bool) | trunc.to(torch.bool)
        step = torch.arange(1, K + 1, device=rew.device, dtype=torch.int64).unsqueeze(1)
        last = (done.to(torch.int64) * step).amax(0) if K else torch.zeros(B, dtype=torch.int64)
        r = rew.double()
        ret, mag = float(r.sum()), float(r.abs().sum())
        eps, length = int(done.sum()), int(last.sum())
    else:
        rew = np.asarray(rew)
        assert rew.dtype == np.float32 and rew.ndim == 2
        K, B = rew.shape
        done = np.asarray(term).astype(bool) | np.asarray(trunc).astype(bool)
        # the lengths of an env's ended episodes add up to the step count at its last end
        step = np.arange(1, K + 1, dtype=np.int64)[:, None]
        last = (done * step).max(0, initial=0)
        r = rew.astype(np.float64).ravel()
        ret = math.fsum(r) if r.size <= FSUM_MAX else float(r.sum())
        mag = float(np.abs(r).sum())
        eps, length = int(done.sum()), int(last.sum())
    n = K * B
    return dict(episodes=eps, return_sum=ret, length_sum=length, env_steps=n, bound=n * 2.0 ** -52 * mag)


class EpisodeCounter:
    """The three integers of want_metrics over a run given launch by launch (torch tensors on the device, int64)."""

    def __init__(self, B, device):
        import torch
        self.last = torch.zeros(B, dtype=torch.int64, device=device)
        self.eps = torch.zeros((), dtype=torch.int64, device=device)
        self.k0, self.B = 0, B

    def add(self, term, trunc):
        import torch
        done = term.to(torch.bool) | trunc.to(torch.bool)
        K = done.shape[0]
        step = torch.arange(self.k0 + 1, self.k0 + K + 1, device=done.device, dtype=torch.int64).unsqueeze(1)
        self.last = torch.maximum(self.last, (done.to(torch.int64) * step).amax(0))
        self.eps += done.sum()
        self.k0 += K

    def result(self):
        return dict(episodes=int(self.eps), length_sum=int(self.last.sum()), env_steps=self.k0 * self.B)


def assert_metrics(got, want, what=""):
    """The assertion every case makes: the three integers with ==, return_sum within the bound. The figures are
    printed first (pytest -s, or a failing test's captured output)."""
    err = got["return_sum"] - want["return_sum"]
    print(f"{what}: return_sum {got['return_sum']!r} reference {want['return_sum']!r} error {err:.3e} "
          f"bound {want['bound']:.3e}; episodes {got['episodes']} length_sum {got['length_sum']} "
          f"env_steps {got['env_steps']}")
    for k in ("episodes", "length_sum", "env_steps"):
        assert got[k] == want[k], f"{what} {k}: device {got[k]} reference {want[k]}"
    assert abs(err) <= want["bound"], f"{what} return_sum: |{err:.6e}| > bound {want['bound']:.6e}"


# ---------------------------------------------------------------- summation laws over the kernels' geometry ----
def thread_terms(rew, grid, tile=TILE):
    """The float32 terms every thread adds in one launch, in its order, zero where it has no env: [grid, tile / 4, n].
    Thread t of block b holds envs 4t .. 4t + 3 of tiles b, b + grid, ...; per tile it walks the K steps, 4 envs each."""
    rew = np.asarray(rew, dtype=np.float32)
    K, B = rew.shape
    ntiles = -(-B // tile)
    rounds = -(-ntiles // grid)
    pad = np.zeros((K, rounds * grid * tile), dtype=np.float32)
    pad[:, :B] = rew
    x = pad.reshape(K, rounds, grid, tile // EPT, EPT)  # [k, round, block, thread, i]
    return np.ascontiguousarray(x.transpose(2, 3, 1, 0, 4)).reshape(grid, tile // EPT, rounds * K * EPT)


def _block_reduce(x, dtype):
    """Per-thread values [grid, threads] -> the blocks' totals [grid]: xor-butterfly over each wave's 64 lanes, then
    the waves' lane-0 partials added in order from zero, all in `dtype`."""
    g, t = x.shape
    v = x.astype(dtype).reshape(g, t // 64, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, lane ^ d]).astype(dtype)
    tot = np.zeros(g, dtype=dtype)
    for w in range(t // 64):
        tot = (tot + v[:, w, 0]).astype(dtype)
    return tot


def _chain(terms, dtype):
    """Sequential sums along the last axis in `dtype` (np.cumsum adds in order), a wave of threads at a time."""
    g, t, n = terms.shape
    out = np.zeros((g, t), dtype=dtype)
    if n:
        for b in range(g):
            for w in range(0, t, 64):
                out[b, w:w + 64] = np.cumsum(terms[b, w:w + 64], axis=1, dtype=dtype)[:, -1]
    return out


def float32_law(launches, grid, tile=TILE):
    """return_sum of a sequence of launches (rew planes [K, B]) under the float32 law: float32 up to the block's total,
    float64 from the slot's += on."""
    slot = np.zeros(grid, dtype=np.float64)
    for rew in launches:
        slot += _block_reduce(_chain(thread_terms(rew, grid, tile), np.float32), np.float32).astype(np.float64)
    return float(slot.sum())


def float64_law(launches, grid, tile=TILE):
    """return_sum under the float64 law: the same walk with every sum in float64 from the thread on."""
    slot = np.zeros(grid, dtype=np.float64)
    for rew in launches:
        slot += _block_reduce(_chain(thread_terms(rew, grid, tile), np.float64), np.float64)
    return float(slot.sum())


def count_law(counts, rewards, grid, dtype, tile=TILE):
    """The count-based epilogue of the numpy-exact grid kernels, one launch: counts int [n_kinds, B] (how often each
    env earned each reward), rewards float32 [n_kinds]. Each thread forms sum_j count_j * reward_j over its 4 envs
    once, in `dtype`, and the block reduces in `dtype` (float32: the law before; float64: the law now)."""
    counts = np.asarray(counts, dtype=np.int64)
    n, B = counts.shape
    ntiles = -(-B // tile)
    rounds = -(-ntiles // grid)
    pad = np.zeros((n, rounds * grid * tile), dtype=np.int64)
    pad[:, :B] = counts
    per_thread = pad.reshape(n, rounds, grid, tile // EPT, EPT).sum((1, 4))  # [n, grid, threads]
    x = np.zeros(per_thread.shape[1:], dtype=dtype)
    for j in range(n):
        x = (x + (per_thread[j].astype(dtype) * np.asarray(rewards, dtype=np.float32)[j].astype(dtype)).astype(dtype))
        x = x.astype(dtype)
    return float(_block_reduce(x, dtype).astype(np.float64).sum())


def constant_launch(n_adds, value, dtype):
    """Per-thread sums of a constant float32 `value` added n_adds[t] times in sequence in `dtype`: one chain, read at
    each thread's length (the long store-free launches, where every full thread's chain is the same)."""
    n_adds = np.asarray(n_adds, dtype=np.int64)
    chain = np.cumsum(np.full(int(n_adds.max()), np.float32(value), dtype=np.float32), dtype=dtype)
    chain = np.concatenate((np.zeros(1, dtype=dtype), chain))
    return chain[n_adds]


def constant_law(K, B, value, grid, dtype, tile=TILE):
    """return_sum of one K-step launch in which every reward is `value`, under the law of `dtype` up to the block."""
    ntiles = -(-B // tile)
    rounds = -(-ntiles // grid)
    live = np.zeros(rounds * grid * tile, dtype=np.int64)
    live[:B] = 1
    n_adds = live.reshape(rounds, grid, tile // EPT, EPT).sum((0, 3)) * K  # [grid, threads]
    x = constant_launch(n_adds, value, dtype)
    return float(_block_reduce(x, dtype).astype(np.float64).sum())
