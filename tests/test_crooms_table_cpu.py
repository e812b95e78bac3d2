"""The `crooms_table` fixtures (tests/golden/make_golden.py CROOMS_TABLES): one reference step of C-ROOMS over rows
aimed at the lines where a step decides something -- a proposed coordinate on a cell boundary and one ulp on either
side, an agent on the goal circle, the grid and velocity clips, elapsed at the time limit, a wall hit inside the goal's
radius -- under cell sizes, thresholds and rewards away from their defaults. Here the oracle (oracle/crooms.py) must
reproduce every recorded row on numpy's own stream from the recorded state, a scalar restatement of the reference's
step (crooms.py:276-331) must agree with every row, and the fixtures must still hold the rows they were made for: the
GPU tests (test_crooms_table_gpu.py) compare the kernels with these rows. No tolerance anywhere: equality of bits.
"""
import math
import struct

import numpy as np
import pytest

from crooms_table_oracle import TableOracle, ctor_kwargs, rng6, table_oracle_step
from fixtures import (CROOMS_FAMILIES, crooms_table_check_counts, crooms_table_counts, crooms_table_inputs,
                      load_crooms_table, load_index)
from oracle.gridworld import ACTIONS_CARDINAL, load_maps

TABLES = sorted(load_index()["crooms_table"])


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _assert_step(ora, out, data):
    o, r, d, tr = out
    np.testing.assert_array_equal(_bits(np.asarray(o)), _bits(data["obs"]))
    assert r.dtype == np.float32
    np.testing.assert_array_equal(r.view(np.uint32), data["rew"].view(np.uint32))
    np.testing.assert_array_equal(d, data["term"])
    np.testing.assert_array_equal(tr, data["trunc"])
    np.testing.assert_array_equal(_bits(ora.agent), _bits(data["agent"]))
    np.testing.assert_array_equal(_bits(ora.goal), _bits(data["goal_cell"].astype(np.float64) + 0.5))
    np.testing.assert_array_equal(_bits(ora.velocity), _bits(data["velocity"]))
    np.testing.assert_array_equal(ora.elapsed, data["elapsed"])


@pytest.mark.parametrize("name", TABLES)
def test_oracle_reproduces_table_from_recorded_state(name):
    meta, data = load_crooms_table(name)
    ora, out, _ = table_oracle_step(meta, data, recording=False)
    _assert_step(ora, out, data)
    assert rng6(ora.gen) == [int(v) for v in data["rng_state"]]  # has_uint32 and uinteger included
    np.testing.assert_array_equal(ora.last_oob, data["oob"])
    np.testing.assert_array_equal(_bits(ora.last_move), _bits(data["move"]))


def _proposed(meta, data):
    kw = meta["kwargs"]
    if kw.get("use_velocity", False):
        return data["in_agent"] + (data["in_velocity"] + data["move"]).clip(-5.0, 5.0)
    return data["in_agent"] + data["move"]


@pytest.mark.parametrize("name", TABLES)
def test_recorded_counts_and_conditions(name):
    """The index's counts are the file's and meet the conditions the table was built for; the stored inputs are the
    builder's; every action value is a float32; the row count is odd, no multiple of 512 and at most 4,096."""
    meta, data = load_crooms_table(name)
    kw = meta["kwargs"]
    assert kw["action_std"] == 0.0 and (kw["step_reward"], kw["wall_reward"], kw["goal_reward"]) == (-0.01, -0.5, 2.0)
    # the ring rows hit no wall, so their position before any reset is start + move: the norm recomputed with numpy
    c = crooms_table_counts(meta, data["in_family"], _proposed(meta, data), data["in_goal_cell"], data["oob"],
                            data["term"], data["trunc"], data["in_agent"], data["in_velocity"], data["move"])
    assert c == meta["counts"]
    crooms_table_check_counts(meta, c)
    inp = crooms_table_inputs(meta)
    for k, v in inp.items():
        assert v.dtype == data["in_" + k].dtype
        np.testing.assert_array_equal(v.view(np.uint64) if v.dtype == np.float64 else v,
                                      data["in_" + k].view(np.uint64) if v.dtype == np.float64 else data["in_" + k])
    if data["in_action"].dtype.kind == "f":
        np.testing.assert_array_equal(data["in_action"], data["in_action"].astype(np.float32).astype(np.float64))
    B = meta["num_envs"]
    assert B == len(data["rew"]) and B % 2 == 1 and B % 512 != 0 and B <= 4096 and B > 2 * 512
    # deterministic in every RNG mode: no wall noise, no reset
    det = ~(data["oob"] | data["term"] | data["trunc"])
    assert 2 * int(det.sum()) >= B


def test_threshold_zero_table_has_agents_on_the_goal_centre():
    meta, data = load_crooms_table("crooms_table_thr0")
    ring = data["in_family"] == CROOMS_FAMILIES.index("ring")
    pos, gc = _proposed(meta, data), data["in_goal_cell"].astype(np.float64) + 0.5
    on = ring & (pos == gc).all(-1)
    assert int(on.sum()) >= 30 and data["term"][on].all()
    off = ring & ~(pos == gc).all(-1)
    assert int(off.sum()) >= 30 and not data["term"][off].any()  # one ulp off the centre is outside radius 0


# ---- the scalar restatement: CRoomsEnv.step for one env, from crooms.py:276-331 (and :175-198, :217-244) ----
def scalar_step(cfg, grid, valid, ay, ax, gy, gx, vy, vx, el, action, draws):
    """One env. draws: None where the step may not draw anything that matters (a KeyError otherwise), else this
    env's values of the reference's calls: u (rng.random), noise, wall_noise (rng.normal), goal, agent (indices into
    valid_states of the two rng.choice calls)."""
    cell, power, thr = cfg["cell"], cfg["power"], cfg["thr"]
    H, W = len(grid), len(grid[0])
    draws = draws or {}
    el += 1
    if cfg["cardinal"]:  # vectorized_multinomial_with_rng: the first index whose cumulative probability reaches u
        p, q = 1.0 - cfg["fail"], cfg["fail"] / 3.0
        cum, e = 0.0, 0
        for j in range(4):
            cum = cum + (p if j == action else q)
            if cum < draws["u"]:
                e += 1
        sy, sx = float(ACTIONS_CARDINAL[e][0]), float(ACTIONS_CARDINAL[e][1])  # action_std == 0: no noise is drawn
    else:
        ny, nx = draws["noise"] if "noise" in draws else (0.0, 0.0)  # rng.normal(scale=0.0): +-0.0
        sy, sx = action[0] + ny, action[1] + nx
    my, mx = sy * power, sx * power
    if cfg["velocity"]:
        vy, vx = min(max(vy + my, -5.0), 5.0), min(max(vx + mx, -5.0), 5.0)
        py, px = ay + vy, ax + vx
    else:
        py, px = ay + my, ax + mx
    py, px = min(max(py, 0.0), H - 1 - 1e-6), min(max(px, 0.0), W - 1 - 1e-6)
    oob = grid[math.floor(py / cell)][math.floor(px / cell)] == -1
    if not oob:
        ay, ax = py, px
    else:
        cy, cx = math.floor(ay / cell) * cell + cell / 2, math.floor(ax / cell) * cell + cell / 2
        wy, wx = draws["wall_noise"]
        ay = min(max(cy + wy, cy - cell / 2), cy + cell / 2 - 1e-8)
        ax = min(max(cx + wx, cx - cell / 2), cx + cell / 2 - 1e-8)
        vy = vx = 0.0
    dy, dx = ay - gy, ax - gx
    term = math.sqrt(dy * dy + dx * dx) <= thr
    rew = cfg["r_step"]
    if oob:
        rew = cfg["r_wall"]
    if term:
        rew = cfg["r_goal"]
    trunc = el > cfg["tl"]
    if term or trunc:
        el = 0
        if not cfg["goal_fixed"]:
            g = int(valid[draws["goal"]])
            gy, gx = (g // W) * 1.0 + 1.0 / 2, (g % W) * 1.0 + 1.0 / 2
        a = int(valid[draws["agent"]])
        ay, ax = (a // W) * 1.0 + 1.0 / 2, (a % W) * 1.0 + 1.0 / 2  # the random reset ignores cell_size
        vy = vx = 0.0
    return (ay, ax, gy, gx, vy, vx, el, rew, term, trunc, oob, my, mx)


def _cfg(kw):
    return dict(cell=float(kw.get("cell_size", 1.0)), power=float(kw.get("action_power", 1.0)),
                thr=float(kw.get("goal_threshold", 0.5)), cardinal=kw.get("action_type", "yx") == "cardinal",
                fail=float(kw.get("action_failure_probability", 0.2)), velocity=bool(kw.get("use_velocity", False)),
                tl=int(kw["time_limit"]), r_step=kw["step_reward"], r_wall=kw["wall_reward"],
                r_goal=kw["goal_reward"], goal_fixed=kw.get("goal_xy") is not None)


@pytest.mark.parametrize("name", TABLES)
def test_scalar_restatement_agrees_with_every_row(name):
    meta, data = load_crooms_table(name)
    cfg = _cfg(meta["kwargs"])
    ora, _, rd = table_oracle_step(meta, data)
    rec, grid, valid = rd.rec, ora.grid.tolist(), ora.valid
    det = ~(data["oob"] | data["term"] | data["trunc"])
    if cfg["cardinal"]:
        u = rec["u"].astype(np.float64) * 2.0 ** -53
    B = meta["num_envs"]
    got = np.zeros((B, 13))
    for i in range(B):
        d = None
        if cfg["cardinal"] or not det[i]:  # a pure function of the inputs elsewhere
            d = {k: (tuple(v[i]) if v.ndim == 2 else int(v[i])) for k, v in rec.items() if k != "u"}
            if cfg["cardinal"]:
                d["u"] = float(u[i])
        a = int(data["in_action"][i]) if cfg["cardinal"] else tuple(float(x) for x in data["in_action"][i])
        got[i] = scalar_step(cfg, grid, valid, *(float(x) for x in data["in_agent"][i]),
                             *(float(x) + 0.5 for x in data["in_goal_cell"][i]),
                             *(float(x) for x in data["in_velocity"][i]), int(data["in_elapsed"][i]), a, d)
    np.testing.assert_array_equal(_bits(got[:, 0:2]), _bits(data["agent"]))
    np.testing.assert_array_equal(got[:, 2:4] - 0.5, data["goal_cell"])
    np.testing.assert_array_equal(_bits(got[:, 4:6]), _bits(data["velocity"]))
    np.testing.assert_array_equal(got[:, 6], data["elapsed"])
    np.testing.assert_array_equal(got[:, 7].astype(np.float32), data["rew"])
    np.testing.assert_array_equal(got[:, 8] != 0, data["term"])
    np.testing.assert_array_equal(got[:, 9] != 0, data["trunc"])
    np.testing.assert_array_equal(got[:, 10] != 0, data["oob"])
    np.testing.assert_array_equal(_bits(got[:, 11:13]), _bits(data["move"]))
    # the observation is a function of the state after the step (crooms.py:16-88, pinned by the trajectory fixtures)
    np.testing.assert_array_equal(_bits(np.asarray(ora.obs_fn(got[:, 0:2].copy(), got[:, 2:4].copy()))),
                                  _bits(data["obs"]))


# ---- agent_xy: the reference raises (an ndarray index, crooms.py:234); the evident intent has no fixture ----
@pytest.mark.parametrize("agent_xy,cell_size,want_cell", [((3, 2), 1.0, (2, 3)),   # a walkable cell
                                                          ((8, 3), 1.0, None),     # a wall: rooms_starts_xy
                                                          ((3, 2), 2.0, (2, 3))])  # grid_to_coord honours cell_size
def test_fixed_agent_reset_is_cell_centre_scaled_by_cell_size(agent_xy, cell_size, want_cell):
    B, tl = 7, 3
    maps = load_maps()
    grid = np.array(maps["rooms_layouts"]["4"])
    if want_cell is None:
        assert grid[agent_xy[1], agent_xy[0]] < 0
        want_cell = tuple(reversed(maps["rooms_starts_xy"]["4"]))
    want = [want_cell[0] * cell_size + cell_size / 2, want_cell[1] * cell_size + cell_size / 2]
    ora = TableOracle(B, **ctor_kwargs(dict(obs_type="vector_mdp", agent_xy=agent_xy, cell_size=cell_size,
                                             time_limit=tl, action_std=0.0)))
    o = ora.reset_seed(5)
    assert np.asarray(o).tolist() == [want] * B
    for t in range(2 * (tl + 1)):
        o, r, d, tr = ora.step_seeded(np.full((B, 2), 0.125))
        if (t + 1) % (tl + 1) == 0:  # truncated: back on the fixed cell
            assert tr.all() and np.asarray(o).tolist() == [want] * B
        else:
            assert not tr.any()


# ---- the squared threshold ----
# csrc/crooms.hip sq_threshold is a static host function with no entry point of its own, so its bisection over the
# bit patterns is restated here; the device's use of it is checked on the GPU against the ring rows
# (test_crooms_table_gpu.py), where one wrong bit flips a termination.
def sq_threshold(thr):
    """The largest double s with sqrt(s) <= thr."""
    if not thr >= 0.0:
        return -1.0
    hi = max(thr * thr * 4.0, 1.0)
    while math.sqrt(hi) <= thr:
        hi *= 2.0
    a, b = 0, struct.unpack("<Q", struct.pack("<d", hi))[0]
    while b - a > 1:
        m = a + (b - a) // 2
        if math.sqrt(struct.unpack("<d", struct.pack("<Q", m))[0]) <= thr:
            a = m
        else:
            b = m
    return struct.unpack("<d", struct.pack("<Q", a))[0]


def test_squared_threshold_brackets_the_threshold():
    rng = np.random.default_rng(0)
    thrs = [0.0, 0.3, 0.5, 1.0] + rng.uniform(0.0, 2.0, 40).tolist() + (2.0 ** rng.uniform(-30, 6, 20)).tolist()
    naive_differs = 0
    for thr in thrs:
        s = sq_threshold(thr)
        assert math.sqrt(s) <= thr < math.sqrt(math.nextafter(s, math.inf)), thr
        naive_differs += s != thr * thr
    assert naive_differs >= 10  # thr * thr is not that number: the bisection is needed
    for name in TABLES:  # on the tables' own rows: the squared test decides as the reference's norm does
        meta, data = load_crooms_table(name)
        ring = data["in_family"] == CROOMS_FAMILIES.index("ring")
        d = (_proposed(meta, data) - (data["in_goal_cell"] + 0.5))[ring]
        sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        thr = float(meta["kwargs"].get("goal_threshold", 0.5))
        np.testing.assert_array_equal(sq <= sq_threshold(thr), data["term"][ring])
