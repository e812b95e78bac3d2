"""Test helpers of test_taxi_table_cpu.py / test_taxi_table_gpu.py: the Taxi oracle (oracle/taxi.py) set to the rows
of a `taxi_table` fixture, a greedy pickup -> dropoff policy found by BFS over the oracle's own transition table, and
oracle rollouts with the four metrics the device accumulates.

Metric bookkeeping as tests/rocksample_oracle.py: an episode that ends at a step adds 1 to `episodes` and its length
-- its elapsed before the same-step reset -- to `length_sum`; every env-step adds its reward to `return_sum`.
"""
import numpy as np

from oracle.draws import NumpyDraws, ReplayDraws
from oracle.taxi import TaxiOracle


def oracle_kwargs(kw):
    kw = dict(kw)
    if isinstance(kw.get("map"), list):
        kw["map"] = tuple(kw["map"])
    return kw


def make_oracle(kw, B):
    return TaxiOracle(B, **oracle_kwargs(kw))


def set_rows(ora, s, elapsed, n_dropoffs):
    ora.s = np.asarray(s).astype(int)
    ora.elapsed = np.asarray(elapsed).astype(int)
    ora.n_dropoffs_completed = np.asarray(n_dropoffs).astype(float)


def replay_draws(ora, s_after):
    """The draws that reproduce a recorded post-step state: a resetting env takes s_after whole, a task completion
    its passenger / destination pair (the oracle keeps its own taxi cell)."""
    s_after = np.asarray(s_after).astype(int)
    return ReplayDraws({"reset_state": s_after, "pd": s_after % (ora.nlocs * (ora.nlocs + 1))})


def metrics_of_step(m, elapsed_before, rew, term, trunc):
    fin = np.asarray(term, bool) | np.asarray(trunc, bool)
    m["episodes"] += int(fin.sum())
    m["length_sum"] += int((np.asarray(elapsed_before)[fin] + 1).sum())
    m["return_sum"] += float(np.asarray(rew).astype(np.float64).sum())
    m["env_steps"] += int(fin.size)
    return m


def new_metrics():
    return dict(episodes=0, return_sum=0.0, length_sum=0, env_steps=0)


def transition_table(kw):
    """(next state [ns, 5], goal [ns]) of the five actions, from one oracle step over every (s, a) row."""
    kw = {k: v for k, v in oracle_kwargs(kw).items() if k not in ("num_passengers", "time_limit")}
    probe = make_oracle(kw, 1)
    ns = probe.ns
    ora = make_oracle(dict(kw, num_passengers=1 << 20, time_limit=1 << 20), ns * 5)
    s, a = (x.ravel() for x in np.meshgrid(np.arange(ns), np.arange(5), indexing="ij"))
    set_rows(ora, s, np.zeros(ns * 5), np.zeros(ns * 5))
    _, rew, _, _ = ora.step(a, replay_draws(ora, s))  # a completed task keeps (p, d) here: goal states are targets
    return ora.s.reshape(ns, 5), (rew == np.float32(ora.GOAL_MOVE)).reshape(ns, 5)[:, 4], ora


def greedy_policy(kw):
    """policy[s]: the first action of a shortest path from s to a goal move (pick the passenger up, carry them to
    the destination, drop them); action 0 where no goal can be reached (taxi walled in)."""
    nxt, goal, ora = transition_table(kw)
    ns = nxt.shape[0]
    dist = np.full(ns, -1)
    pol = np.zeros(ns, dtype=np.int64)
    dist[goal] = 1
    pol[goal] = 4
    d = 1
    while True:
        cand = (dist[nxt] == d) & (dist[:, None] < 0)
        rows = cand.any(1)
        if not rows.any():
            break
        pol[rows] = cand[rows].argmax(1)
        dist[rows] = d + 1
        d += 1
    assert (dist[ora.valid_states] > 0).all(), "a start state cannot reach its goal"
    return pol


def policy_rollout_numpy(kw, B, seed, K, pol):
    """The oracle on numpy's own stream from `seed` under `pol` for K steps: actions [K, B], the stacked outputs, the
    per-step post-states, the metrics, and per-step masks of goal moves / task completions / terminations."""
    ora = make_oracle(kw, B)
    obs0 = np.asarray(ora.reset_seed(seed))
    acts, outs, states, m = [], [], [], new_metrics()
    for _ in range(K):
        a = pol[ora.s]
        el0 = ora.elapsed.copy()
        o, r, d, tr = ora.step(a, NumpyDraws(ora.gen))
        metrics_of_step(m, el0, r, d, tr)
        acts.append(a)
        outs.append((np.asarray(o), r, d, tr))
        states.append((ora.s.copy(), ora.elapsed.copy(), ora.n_dropoffs_completed.copy()))
    return dict(ora=ora, obs0=obs0, acts=np.stack(acts), outs=[np.stack(x) for x in zip(*outs)], states=states,
                metrics=m)


def rare_rows(ora, rew, term, trunc):
    """[K, B] masks of goal moves, task completions and terminations of stacked outputs."""
    goal = rew == np.float32(ora.GOAL_MOVE)
    return dict(goal=goal, task=goal & ~(term | trunc), term=term.astype(bool))


def per_tile_floor(masks, tile=1024):
    """The smallest count of each rare row over the 1024-env tiles of the batch (the last, partial tile excluded
    when it holds fewer than 64 envs)."""
    out = {}
    for k, v in masks.items():
        B = v.shape[1]
        counts = [int(v[:, t:t + tile].sum()) for t in range(0, B, tile) if min(tile, B - t) >= 64]
        out[k] = min(counts)
    return out
