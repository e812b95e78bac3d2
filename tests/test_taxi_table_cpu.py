"""The `taxi_table` fixtures (tests/golden/make_golden.py TAXI_TABLES): every (state, action) row of a Taxi map,
invalid states and the negative actions included, stepped once by the reference at the elapsed / dropoff counts where
its branches change. Here the oracle (oracle/taxi.py) must reproduce every recorded row, fed the recorded draws and
on numpy's own stream from the recorded seed, and the fixtures must still hold the rare rows they were made for: the
GPU tests (test_taxi_table_gpu.py) compare the kernels with these rows.
"""
import numpy as np
import pytest

from fixtures import load_index, load_table, taxi_table_counts, taxi_table_inputs, taxi_table_replicas
from oracle.draws import NumpyDraws
from taxi_table_oracle import greedy_policy, make_oracle, policy_rollout_numpy, rare_rows, replay_draws, set_rows

TABLES = sorted(load_index()["taxi_table"])


def _rng6(gen):
    st = gen.bit_generator.state
    m = (1 << 64) - 1
    return [st["state"]["state"] >> 64, st["state"]["state"] & m, st["state"]["inc"] >> 64, st["state"]["inc"] & m,
            int(st["has_uint32"]), int(st["uinteger"])]


def _assert_rows(ora, out, data):
    o, r, d, tr = out
    np.testing.assert_array_equal(np.asarray(o).astype(np.int64), data["obs"].astype(np.int64))
    np.testing.assert_array_equal(r, data["rew"])
    np.testing.assert_array_equal(d, data["term"])
    np.testing.assert_array_equal(tr, data["trunc"])
    np.testing.assert_array_equal(ora.s, data["s"].astype(np.int64))
    np.testing.assert_array_equal(ora.elapsed, data["elapsed"].astype(np.int64))
    np.testing.assert_array_equal(ora.n_dropoffs_completed, data["n_dropoffs"].astype(np.float64))


@pytest.mark.parametrize("name", TABLES)
def test_oracle_reproduces_table_with_recorded_draws(name):
    meta, data = load_table(name)
    s, a, e, n = taxi_table_inputs(meta)
    ora = make_oracle(meta["kwargs"], meta["num_envs"])
    assert (ora.ns, ora.no, ora.nlocs) == (meta["ns"], meta["n_obs"], meta["nlocs"])
    set_rows(ora, s, e, n)
    _assert_rows(ora, ora.step(a, replay_draws(ora, data["s"])), data)


@pytest.mark.parametrize("name", TABLES)
def test_oracle_reproduces_table_from_seed(name):
    meta, data = load_table(name)
    s, a, e, n = taxi_table_inputs(meta)
    ora = make_oracle(meta["kwargs"], meta["num_envs"])
    ora.reset_seed(meta["seed"])
    assert _rng6(ora.gen) == [int(v) for v in data["pre_rng_state"]]
    set_rows(ora, s, e, n)
    _assert_rows(ora, ora.step(a, NumpyDraws(ora.gen)), data)
    assert _rng6(ora.gen) == [int(v) for v in data["rng_state"]]


@pytest.mark.parametrize("name", TABLES)
def test_recorded_counts(name):
    """The index's counts are the file's, every state and action is there, and the rare rows are where the reference's
    rules put them: goal moves and pickups in every replica, terminations in the replicas one dropoff short, task
    completions in those further away that do not run out of time, truncation of every row at elapsed = time_limit."""
    meta, data = load_table(name)
    s, a, e, n = taxi_table_inputs(meta)
    assert sorted(set(a.tolist())) == list(range(-5, 5)) and sorted(set(s.tolist())) == list(range(meta["ns"]))
    c = taxi_table_counts(meta, a, data["rew"], data["term"], data["trunc"])
    assert c == meta["counts"]
    kw, rows = meta["kwargs"], 10 * meta["ns"]
    L = meta["nlocs"]
    for i, (el, nd) in enumerate(taxi_table_replicas(meta)):
        last = nd == kw["num_passengers"] - 1
        late = el == kw["time_limit"]
        assert c["goal"][i] == L and c["pick"][i] == L * L
        assert c["term"][i] == (L if last else 0)
        assert c["trunc"][i] == (rows if late else 0)
        assert c["task"][i] == (0 if last or late else L)


def test_recorded_counts_of_the_taxi_map():
    """The figures the TAXI map was measured at: over the three elapsed replicas of one dropoff count 12 goal rows and
    1,440 bad ones, 5,000 truncated rows, and 8 task completions with two passengers."""
    meta, _ = load_table("taxi_table_taxi_plain_2p")
    c, reps = meta["counts"], taxi_table_replicas(meta)
    assert meta["num_envs"] == 30000 and load_table("taxi_table_ext_plain_2p")[0]["num_envs"] == 76800
    for nd in range(2):
        idx = [i for i, r in enumerate(reps) if r[1] == nd]
        assert sum(c["goal"][i] for i in idx) == 12 and sum(c["bad"][i] for i in idx) == 1440
        assert sum(c["trunc"][i] for i in idx) == 5000
    assert sum(c["task"]) == 8


def test_greedy_policy_completes_tasks_and_terminates():
    """The directed trajectories of the GPU tests: under the BFS policy every 1,024-env tile of a short run holds goal
    moves, task completions, terminations and truncations."""
    kw = dict(map="TAXI", num_passengers=2, time_limit=24, reward_goal=2.0, reward_bad=-1.0, reward_any=-0.25)
    run = policy_rollout_numpy(kw, 2048, 3, 48, greedy_policy(kw))
    _, rew, term, trunc = run["outs"]
    rr = rare_rows(run["ora"], rew, term, trunc)
    for t in (0, 1024):
        assert all(int(v[:, t:t + 1024].sum()) > 0 for v in rr.values())
        assert int(trunc[:, t:t + 1024].sum()) > 0
    assert run["metrics"]["episodes"] == int((term | trunc).sum())
