"""The `grid_table` fixtures (tests/golden/make_golden.py GRID_TABLES: one reference step of FourRooms / ROOMS over
every (agent cell, intended action) x goal and elapsed replicas) against the numpy oracle, and the conditions the
tables were built to meet. No device: the oracle pinned here is what tests/test_grid_table_gpu.py trusts in the modes
whose draws are not the reference's (philox), and the counts are what makes passing it mean something.
"""
import functools
import os

import numpy as np
import pytest

from fixtures import (GOLDEN_DIR, GRID_UNIFORM_P, grid_table_check_counts, grid_table_counts, grid_table_dirs,
                      grid_table_inputs, grid_table_oracle, load_grid_table, load_index)
from grid_table_oracle import metrics_of_step, new_metrics, replay_indices, rng6, step_uniforms, table_oracle_step
from oracle.draws import ReplayDraws

TABLES = sorted(load_index()["grid_table"])


@functools.lru_cache(maxsize=None)
def _table(name):
    meta, data = load_grid_table(name)
    return meta, data, grid_table_inputs(meta)


@functools.lru_cache(maxsize=None)
def _oracle_step(name):
    meta, data, inp = _table(name)
    return table_oracle_step(meta, inp, data["pre_rng_state"])


@pytest.mark.parametrize("name", TABLES)
def test_oracle_reproduces_table_bit_for_bit(name):
    meta, data, inp = _table(name)
    ora, out, _ = _oracle_step(name)
    for k, v in dict(obs=out[0], rew=out[1], term=out[2], trunc=out[3], agent=ora.agent, goal=ora.goal,
                     elapsed=ora.elapsed).items():
        np.testing.assert_array_equal(np.asarray(v).astype(np.float64), data[k].astype(np.float64), err_msg=k)
    assert out[1].dtype == np.float32 and data["rew"].dtype == np.float32
    assert rng6(ora.gen.bit_generator.state) == [int(v) for v in data["rng_state"]]


@pytest.mark.parametrize("name", TABLES)
def test_replay_indices_reproduce_the_post_state(name):
    """The oracle on pre-decided draws (the uniforms of the stream, the recorded post-state as reset indices) gives
    the recorded step: what the device's replay mode is handed."""
    meta, data, inp = _table(name)
    ora = grid_table_oracle(meta, meta["num_envs"])
    ora.agent, ora.goal, ora.elapsed = inp["agent"].copy(), inp["goal"].copy(), inp["elapsed"].copy()
    u, k = step_uniforms(data["pre_rng_state"], meta["num_envs"])
    gi, ai = replay_indices(ora, data["agent"], data["goal"])
    out = ora.step(inp["action"], ReplayDraws({"uniform": u, "goal": gi, "agent": ai}))
    for k_, v in dict(obs=out[0], rew=out[1], term=out[2], trunc=out[3], agent=ora.agent, goal=ora.goal,
                      elapsed=ora.elapsed).items():
        np.testing.assert_array_equal(np.asarray(v).astype(np.float64), data[k_].astype(np.float64), err_msg=k_)


@pytest.mark.parametrize("name", TABLES)
def test_counts_in_the_index_hold(name):
    meta, data, inp = _table(name)
    _, _, eff = _oracle_step(name)
    got = grid_table_counts(meta, inp, eff, data["rew"], data["term"], data["trunc"])
    want = {k: v for k, v in meta["counts"].items() if k not in ("resets", "lemire_rejections")}
    assert got == want
    grid_table_check_counts(meta, got)
    assert meta["counts"]["resets"] == int((data["term"] | data["trunc"]).sum())
    # the metrics of the step are a count over the fixture, not over anything the device does
    m = metrics_of_step(new_metrics(), inp["elapsed"], data["rew"], data["term"], data["trunc"])
    assert m["episodes"] == meta["counts"]["resets"]  # (both count the padding rows)
    assert m["env_steps"] == meta["num_envs"] and m["return_sum"] * 4 == round(m["return_sum"] * 4)


@pytest.mark.parametrize("name", TABLES)
def test_rows_are_what_the_table_promises(name):
    """Every walkable cell x every intended action x elapsed {0, tl - 1, tl}; random goals valid and per row; a
    scalar-obs table is padded to whole 512-env tiles with repeats of its first rows."""
    meta, data, inp = _table(name)
    ora = grid_table_oracle(meta)
    n, B, tl = meta["rows"], meta["num_envs"], meta["kwargs"]["time_limit"]
    walk = np.flatnonzero(ora.grid != ora.wall_value)
    flat = np.ravel_multi_index(tuple(inp["agent"][:n].T), ora.grid.shape)
    nact = ora.actions.shape[0]
    combos = set(zip(flat.tolist(), inp["action"][:n].tolist(), inp["elapsed"][:n].tolist()))
    assert combos == {(c, a, e) for c in walk.tolist() for a in range(nact) for e in (0, tl - 1, tl)}
    gflat = np.ravel_multi_index(tuple(inp["goal"].T), ora.grid.shape)
    assert np.isin(gflat, ora.valid_goal).all()
    per_cell = np.bincount(np.searchsorted(walk, flat))
    assert per_cell.min() >= (48 if nact == 4 else 96)
    scalar = data["obs"].ndim == 1
    assert (B % 512 == 0 and B // 512 <= 256 and B - n < 512) if scalar else B == n
    for k in inp:
        np.testing.assert_array_equal(inp[k][n:], inp[k][:B - n])
    if ora.fixed_goal is None:
        own = inp["variant"][:n] == -2
        top = inp["agent"][:n, 0] == ora.grid.shape[0] - 1 if ora.grid.ndim == 3 else np.ones(n, bool)
        assert (inp["goal"][:n][own & top] == inp["agent"][:n][own & top]).all() and (own & top).any()
        far = inp["variant"][:n] == -1
        assert (np.abs(inp["goal"][:n][far] - inp["agent"][:n][far])[:, -2:].sum(-1) > 2).all()
    assert meta["kwargs"]["action_failure_probability"] in (0.0, 0.2, 1.0 / 3, GRID_UNIFORM_P[nact])
    assert grid_table_dirs(meta) in (4, 8)


def test_group_covers_what_it_must():
    idx = load_index()["grid_table"]
    kws = {n: m["kwargs"] for n, m in idx.items()}
    fr = {n: k for n, k in kws.items() if idx[n]["kind"] == "fourrooms"}
    ro = {n: k for n, k in kws.items() if idx[n]["kind"] == "rooms"}
    assert {k["grid_z"] for k in fr.values()} == {1, 2, 3}
    layouts = {k["layout"] for k in ro.values()}
    assert "4" in layouts and any("b" in x for x in layouts) and layouts & {"16", "32"}
    for grp, default in ((fr, "cardinal"), (ro, "ordinal")):
        assert {k.get("action_type", default) for k in grp.values()} == {"cardinal", "ordinal"}
    rand = {n: k for n, k in kws.items() if k.get("goal_xyz", 0) is None or k.get("goal_xy", 0) is None}
    kinds = {k["obs_type"] for k in rand.values()}
    assert {"hansen", "hansen8", "vector_hansen", "vector_goal_hansen8", "mdp", "goal_mdp", "vector_mdp",
            "vector_goal_mdp", "room", "goal_room", "grid"} <= kinds
    assert {k.get("obs_n", 3) for k in ro.values() if k["obs_type"] == "grid"} == {3, 5}
    fixed = {n: k for n, k in kws.items() if n not in rand}
    assert sorted(idx[n]["kind"] for n in fixed) == ["fourrooms", "rooms"]
    assert all(k["obs_type"] == "hansen" for k in fixed.values())
    assert [k for k in fixed.values() if "grid_z" in k][0]["action_failure_probability"] == 1.0 / 3
    for grp in (fr, ro):
        assert any(k["action_failure_probability"] == 0.0 for k in grp.values())
    assert sum(k["action_failure_probability"] in (0.2, 1.0 / 3) for k in kws.values()) >= 2
    # the ROOMS fixed goal has eight walkable neighbours
    name = [n for n in fixed if idx[n]["kind"] == "rooms"][0]
    ora = grid_table_oracle(idx[name])
    g = ora.fixed_goal
    assert (ora.grid[g[0] - 1:g[0] + 2, g[1] - 1:g[1] + 2] >= 0).all()
    # sizes: no file above the largest fixture committed before this group, the group under 2.5 MB
    sizes = [os.path.getsize(os.path.join(GOLDEN_DIR, m["file"])) for m in idx.values()]
    assert max(sizes) <= 384 * 1024 and sum(sizes) < 2_500_000
    # Lemire rejections among the reset draws (about 1e-8 per draw): a table either holds one, or all 64 seeds were
    # stepped and the index says how many had one. Where none did, the planted rejections of test_grid_gpu.py /
    # test_wgrid_gpu.py cover the slow path.
    for n, m in idx.items():
        scan, rej = m["lemire_scan"], m["counts"]["lemire_rejections"]
        assert rej > 0 or scan["seeds"] == 64, n
        assert (scan["seeds_with_rejection"] > 0) == (rej > 0), n  # a seed with one that met the conditions is taken
