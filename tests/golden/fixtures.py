"""Golden-fixture helpers shared by the generator (make_golden.py) and the tests.

Fixtures are DATA: seeds, actions, and the reference's outputs (obs / reward / terminated /
truncated per step), RNG transcripts (the values each numpy call returned, in call order) and
final internal state. No reference source is stored.
"""
import json
import os

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
INDEX = os.path.join(GOLDEN_DIR, "index.json")


def digest(x):
    """Order-sensitive uint64 checksum of an array's values (ints/bools by value, floats by bits)."""
    x = np.ascontiguousarray(x)
    if x.dtype == np.float32:
        v = x.view(np.uint32).astype(np.uint64).ravel()
    elif x.dtype == np.float64:
        v = x.view(np.uint64).ravel()
    else:
        v = x.astype(np.int64).view(np.uint64).ravel()
    w = (np.arange(v.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    with np.errstate(over="ignore"):
        return np.uint64((v * w + v).sum(dtype=np.uint64))


def load_index():
    with open(INDEX) as f:
        return json.load(f)


def load_case(name):
    idx = load_index()
    meta = idx["cases"][name]
    data = np.load(os.path.join(GOLDEN_DIR, meta["file"]), allow_pickle=False)
    return meta, data


def load_table(name):
    """A `taxi_table` case (make_golden.py TAXI_TABLES): (index entry, recorded arrays)."""
    meta = load_index()["taxi_table"][name]
    return meta, np.load(os.path.join(GOLDEN_DIR, meta["file"]), allow_pickle=False)


def taxi_table_replicas(meta):
    """The (elapsed, n_dropoffs_completed) replicas of a taxi_table case, in row order."""
    tl, npass = meta["kwargs"]["time_limit"], meta["kwargs"]["num_passengers"]
    return [(e, n) for e in (0, tl - 1, tl) for n in range(npass)]


def taxi_table_inputs(meta):
    """Regenerate the rows a taxi_table case was recorded on: (s, action, elapsed, n_dropoffs), int64 [B].
    Row order: replica-major, then every state 0..ns-1, then the actions -5..4."""
    ns = meta["ns"]
    s, a = np.meshgrid(np.arange(ns), np.arange(-5, 5), indexing="ij")
    reps = taxi_table_replicas(meta)
    s, a = np.tile(s.ravel(), len(reps)), np.tile(a.ravel(), len(reps))
    e = np.repeat([r[0] for r in reps], ns * 10)
    n = np.repeat([r[1] for r in reps], ns * 10)
    assert s.size == meta["num_envs"]
    return s, a, e, n


def taxi_table_counts(meta, a, rew, term, trunc):
    """Per-replica counts of the rare rows of one table step, from the step's own outputs: a pickup is the only
    action-4 row paid reward_any; a task completion is a goal row whose episode goes on."""
    kw = meta["kwargs"]
    rew, term, trunc = np.asarray(rew), np.asarray(term).astype(bool), np.asarray(trunc).astype(bool)
    goal, bad = rew == np.float32(kw["reward_goal"]), rew == np.float32(kw["reward_bad"])
    rows = dict(goal=goal, bad=bad, pick=(np.asarray(a) == 4) & (rew == np.float32(kw["reward_any"])), term=term,
                trunc=trunc, task=goal & ~(term | trunc))
    n = len(taxi_table_replicas(meta))
    return {k: [int(x) for x in v.reshape(n, -1).sum(-1)] for k, v in rows.items()}


def step_actions(meta):
    """Regenerate the action sequence a fixture was recorded with."""
    rng = np.random.default_rng(meta["action_seed"])
    T, B = meta["steps"], meta["num_envs"]
    if meta.get("action_kind") == "box2":
        return rng.uniform(-1.0, 1.0, (T, B, 2))
    return rng.integers(0, meta["num_actions"], (T, B))
