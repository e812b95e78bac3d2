"""Test helpers of test_grid_table_cpu.py / test_grid_table_gpu.py / test_grid_edges_*.py: the grid oracle
(oracle/gridworld.py) set to the rows of a `grid_table` fixture, the uniforms of the recorded step rebuilt with numpy's
own Generator, the replay indices that reproduce the recorded post-state, and the metrics of one step.

Metric bookkeeping as tests/taxi_table_oracle.py: an episode that ends at a step adds 1 to `episodes` and its length
-- its elapsed before the same-step reset, plus this step -- to `length_sum`; every env-step adds its reward to
`return_sum`.
"""
import numpy as np

from fixtures import grid_table_oracle
from oracle.draws import NumpyDraws
from oracle.gridworld import sample_effective_action
from stream_plant import plant_word, state_with_output_word  # noqa: F401  (the edge tests import them from here)

TWO53 = float(2 ** 53)


def rng_dict(r6):
    r6 = [int(v) for v in r6]
    return {"bit_generator": "PCG64", "state": {"state": (r6[0] << 64) | r6[1], "inc": (r6[2] << 64) | r6[3]},
            "has_uint32": r6[4], "uinteger": r6[5]}


def rng6(st):
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = (1 << 64) - 1
    return [s >> 64, s & m, inc >> 64, inc & m, int(st["has_uint32"]), int(st["uinteger"])]


def generator_at(r6):
    bg = np.random.PCG64()
    bg.state = rng_dict(r6)
    return np.random.Generator(bg)


def set_rows(ora, inp):
    """Overwrite the oracle's state with the table's rows (a fixed goal stays the configuration's own)."""
    ora.agent = inp["agent"].astype(int).copy()
    ora.goal = inp["goal"].astype(int).copy()
    ora.elapsed = inp["elapsed"].astype(int).copy()


def table_oracle(meta, inp, pre_rng_state=None):
    """The oracle of the table's configuration on its rows, its Generator at the recorded pre-step state."""
    ora = grid_table_oracle(meta, meta["num_envs"])
    if pre_rng_state is not None:
        ora.gen = generator_at(pre_rng_state)
    set_rows(ora, inp)
    return ora


def step_uniforms(pre_rng_state, B):
    """(u float64 [B], k uint64 [B]) of the step's first draw, Generator.random(B): u == k * 2^-53 exactly."""
    u = generator_at(pre_rng_state).random(B)
    k = (u * TWO53).astype(np.uint64)
    assert np.array_equal(k.astype(np.float64) * 2.0 ** -53, u)
    return u, k


def effective_actions(ora, action, u):
    return sample_effective_action(ora.action_matrix[np.asarray(action)], u)


def table_oracle_step(meta, inp, pre_rng_state):
    """One oracle step on numpy's own stream from the recorded pre-state: (oracle, the four outputs, effective
    actions)."""
    ora = table_oracle(meta, inp, pre_rng_state)
    u, _ = step_uniforms(pre_rng_state, meta["num_envs"])
    eff = effective_actions(ora, inp["action"], u)
    out = ora.step(inp["action"], NumpyDraws(ora.gen))
    return ora, out, eff


def flat(ora, coords):
    return np.ravel_multi_index(tuple(np.asarray(coords).T), ora.grid.shape)


def replay_indices(ora, post_agent, post_goal):
    """(i0 goal index, i1 agent index) int32 [B] into the valid-goal / valid-agent lists such that a reset lands on
    the recorded post-state; 0 where the recorded cell is in no list (an env that did not reset may stand anywhere;
    with a fixed goal or agent the list is not consulted)."""
    def index_in(valid, cells):
        valid = np.asarray(valid)
        pos = np.searchsorted(valid, cells)
        pos = np.minimum(pos, len(valid) - 1)
        return np.where(valid[pos] == cells, pos, 0).astype(np.int32)
    return index_in(ora.valid_goal, flat(ora, post_goal)), index_in(ora.valid_agent, flat(ora, post_agent))


def new_metrics():
    return dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)


def metrics_of_step(m, elapsed_before, rew, term, trunc):
    fin = np.asarray(term, bool) | np.asarray(trunc, bool)
    m["episodes"] += int(fin.sum())
    m["length_sum"] += int((np.asarray(elapsed_before)[fin] + 1).sum())
    m["return_sum"] += float(np.asarray(rew).astype(np.float64).sum())
    m["env_steps"] += int(fin.size)
    return m


# ---- the action-failure thresholds at their edges (test_grid_edges_cpu.py / test_grid_edges_gpu.py) ----
EDGE_PS = (0.0, 0.2, 1.0 / 3, 0.5, 0.9, 1.0)
K_MAX = (1 << 53) - 1


def thresholds(n, p):
    """t[a, j] = floor(cumsum(P[a])_j * 2^53) as Python ints, from numpy's cumsum of the reference's matrix
    (action_utils.py:38-48, :84-90): cumsum_j < k * 2^-53  <=>  k > t_j (scaling by 2^53 is exact)."""
    from oracle.gridworld import action_probability_matrix
    cs = action_probability_matrix(n, p).cumsum(axis=1)
    return [[int(np.floor(v * TWO53)) for v in row] for row in cs]


def threshold_rows(n, p):
    """(action int64 [R], k uint64 [R], dropped k's): every intended action x every threshold j < n - 1 x
    k in {t_j - 1, t_j, t_j + 1} within [0, 2^53 - 1], plus k = 0 and k = 2^53 - 1; without the rows for which the
    reference's formula counts n (all cumulative sums below u: the reference raises IndexError, the device clamps)."""
    from oracle.gridworld import action_probability_matrix
    t = thresholds(n, p)
    rows = []
    for a in range(n):
        ks = {0, K_MAX}
        for j in range(n - 1):
            ks |= {k for k in (t[a][j] - 1, t[a][j], t[a][j] + 1) if 0 <= k <= K_MAX}
        rows += [(a, k) for k in sorted(ks)]
    act = np.array([r[0] for r in rows], np.int64)
    k = np.array([r[1] for r in rows], np.uint64)
    eff = sample_effective_action(action_probability_matrix(n, p)[act], k.astype(np.float64) * 2.0 ** -53)
    keep = eff < n
    return act[keep], k[keep], [(int(a), int(x)) for a, x in zip(act[~keep], k[~keep])]


def planted_words(n, p):
    """[(action, j, word)]: for every intended action and threshold j < n - 1 the largest 64-bit draw that must not
    exceed t_j, (t << 11) | 0x7FF, and the smallest that must, (t + 1) << 11 (thresholds of 2^53 and above, a
    cumulative sum of 1.0 or more, are exceeded by no draw and have no such words)."""
    t = thresholds(n, p)
    out = []
    for a in range(n):
        for j in range(n - 1):
            if t[a][j] <= K_MAX - 1:
                out += [(a, j, (t[a][j] << 11) | 0x7FF), (a, j, (t[a][j] + 1) << 11)]
    return out
