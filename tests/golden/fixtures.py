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


def load_crooms_table(name):
    """A `crooms_table` case (make_golden.py CROOMS_TABLES): (index entry, dict of the recorded arrays)."""
    meta = load_index()["crooms_table"][name]
    with np.load(os.path.join(GOLDEN_DIR, meta["file"]), allow_pickle=False) as z:
        return meta, {k: z[k] for k in z.files}


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


# ---- C-ROOMS one-step tables (make_golden.py CROOMS_TABLES) ----
# Every row is one env: a start position, goal cell, velocity, elapsed count and action, aimed so that the proposed
# position (start + action * action_power, exact with action_std = 0) lies on a line where the step decides something.
# The action values are dyadic (exact in float32); the sub-ulp offsets live in the float64 start position.
CROOMS_FAMILIES = ("boundary", "ring", "clip", "time", "goal_wall")
_MAGS = (0.25, 0.5, 1.0)
_MAX_VELOCITY = 5.0


class _Rows:
    def __init__(self, cardinal):
        from oracle.gridworld import ACTIONS_CARDINAL
        self.cardinal, self.moves = cardinal, [tuple(m) for m in ACTIONS_CARDINAL.tolist()]
        self.r = []

    def add(self, fam, y, x, ay, ax, goal, vy=0.0, vx=0.0, el=0):
        a = self.moves.index((int(ay), int(ax))) if self.cardinal else (float(ay), float(ax))
        self.r.append((CROOMS_FAMILIES.index(fam), float(y), float(x), a, (int(goal[0]), int(goal[1])), float(vy),
                       float(vx), int(el)))


def _crooms_grid(meta):
    from oracle.gridworld import load_maps
    return np.array(load_maps()["rooms_layouts"][meta["kwargs"].get("layout", "4")])


def _pick(rng, items, n):
    """n of `items` (all of them if fewer), in their own order."""
    if len(items) <= n:
        return list(items)
    keep = np.sort(rng.permutation(len(items))[:n])
    return [items[i] for i in keep]


def _aim(t, d, c, cell):
    """The start coordinate from which the displacement d lands on t exactly, if it lies in cell c; else None."""
    s = t - d
    if s + d != t or np.floor(s / cell) != c:
        return None
    return s


def crooms_table_inputs(meta):
    """Build the rows of a crooms_table case: dict(family int8 [B], agent f64 [B,2], goal_cell int16 [B,2],
    velocity f64 [B,2], elapsed int32 [B], action f64 [B,2] (yx) or int32 [B] (cardinal: the intended move; the
    effective one comes from the stream)). Deterministic in meta (kwargs, seed, rows, ring_goal)."""
    kw, want = meta["kwargs"], meta["rows"]
    grid = _crooms_grid(meta)
    H, W = grid.shape
    cell, power = float(kw.get("cell_size", 1.0)), float(kw.get("action_power", 1.0))
    thr, tl = float(kw.get("goal_threshold", 0.5)), int(kw["time_limit"])
    cardinal = kw.get("action_type", "yx") == "cardinal"
    vel = bool(kw.get("use_velocity", False))
    mags = (1.0,) if cardinal else (_MAGS if power == 1.0 else (0.125,) + _MAGS)  # displacements within one cell
    hi = np.array([H, W]) - 1 - 1e-6
    rng = np.random.default_rng(1000 + meta["seed"])
    rg = tuple(meta["ring_goal"])  # (y, x) grid cell: the goal of every row but the goal_wall ones
    rows = _Rows(cardinal)

    def wall_at(y, x):
        y, x = min(max(y, 0.0), hi[0]), min(max(x, 0.0), hi[1])
        return grid[int(np.floor(y / cell)), int(np.floor(x / cell))] < 0

    ncy, ncx = int(np.floor(hi[0] / cell)) + 1, int(np.floor(hi[1] / cell)) + 1
    walk = [(i, j) for i in range(ncy) for j in range(ncx) if grid[i, j] >= 0]  # cells of size `cell` one can stand in
    offs = tuple(f * cell for f in (-0.375, -0.25, -0.125, 0.0, 0.125, 0.25, 0.375))  # along the other axis

    # boundary: the proposed coordinate on a shared cell boundary b, one ulp below it and one ulp above it
    if want.get("boundary"):
        into_wall, into_free = [], []
        for (i, j) in walk:
            for axis in (0, 1):
                c = (i, j)[axis]
                for sign in (-1, 1):
                    b = (c + 1) * cell if sign > 0 else c * cell
                    for m in mags:
                        for k in (-1, 0, 1):
                            t = b if k == 0 else float(np.nextafter(b, k * np.inf))
                            d = sign * (1.0 if cardinal else m * power)
                            s = _aim(t, d, c, cell)
                            if s is None and k != 0:
                                # b's own neighbour cannot be reached (b - d lies in a coarser binade): the
                                # neighbour of the start that lands on b instead, one ulp of the start off b
                                s = float(np.nextafter(b - d, k * np.inf))
                                t = s + d
                                s = _aim(t, d, c, cell) if (t - b) * k > 0 and t - d == s else None
                            if s is None:
                                continue
                            a = (sign * (1 if cardinal else m), 0) if axis == 0 else (0, sign * (1 if cardinal else m))
                            for off in offs:
                                o = (j, i)[axis] * cell + cell / 2 + off
                                y, x, ty, tx = (s, o, t, o) if axis == 0 else (o, s, o, t)
                                (into_wall if wall_at(ty, tx) else into_free).append((y, x, a[0], a[1]))
        n = want["boundary"]
        nw = min(len(into_wall), 260)
        for r in _pick(rng, into_wall, nw) + _pick(rng, into_free, n - nw):
            rows.add("boundary", *r, goal=rg)

    # ring: on the circle of radius thr about the goal centre, placed there (zero action) and arriving there
    if want.get("ring"):
        n = want["ring"]
        gc = (rg[0] + 0.5, rg[1] + 0.5)  # the goal centre ignores cell_size
        pool = 4 * n
        if thr > 0.0:
            th = rng.uniform(0.0, 2.0 * np.pi, pool)
            py, px = gc[0] + thr * np.sin(th), gc[1] + thr * np.cos(th)
        else:  # radius 0: the centre itself, and its neighbours one ulp away along one axis or both
            k = rng.integers(-1, 2, (pool, 2))
            k[::3] = 0
            to = np.where(k < 0, -np.inf, np.inf)
            py = np.where(k[:, 0] == 0, gc[0], np.nextafter(gc[0], to[:, 0]))
            px = np.where(k[:, 1] == 0, gc[1], np.nextafter(gc[1], to[:, 1]))
        steps = [(a, b) for a in (0.0,) + tuple(s * m for m in _MAGS for s in (-1, 1))
                 for b in (0.0,) + tuple(s * m for m in _MAGS for s in (-1, 1)) if (a, b) != (0.0, 0.0)]
        if cardinal:
            steps = [(float(a), float(b)) for a, b in rows.moves]
        sc = 1.0 if cardinal else power
        placed = 0 if cardinal else n // 2
        # rounding puts well over half of the points of some circles inside (norm <= thr): take 45 % such rows, so
        # that the rows whose step is deterministic in every RNG mode stay the majority of the table
        for lo, cnt, arrive in ((0, placed, False), (pool // 2, n - placed, True)):
            inside, outside = [], []
            for r in range(lo, lo + pool // 2):
                a = steps[int(rng.integers(len(steps)))] if arrive else (0.0, 0.0)
                y, x = py[r] - a[0] * sc, px[r] - a[1] * sc
                dy, dx = (y + a[0] * sc) - gc[0], (x + a[1] * sc) - gc[1]
                (inside if np.sqrt(dy * dy + dx * dx) <= thr else outside).append((y, x, a[0], a[1]))
            ni = (cnt * 9) // 20
            for r in _pick(rng, inside, ni) + _pick(rng, outside, cnt - ni):
                rows.add("ring", *r, goal=rg)

    # clip: the grid clip to [0, gridshape - 1 - 1e-6] and the velocity clip at +-5
    if want.get("clip"):
        edge, beyond, inside = [], [], []
        for (i, j) in walk:
            for axis in (0, 1):
                c = (i, j)[axis]
                o = (j, i)[axis] * cell + cell / 2
                for sign in (-1, 1):
                    for m in mags:  # aimed at the clip bounds themselves and their neighbours
                        bound = 0.0 if sign < 0 else float(hi[axis])
                        for t in (bound, float(np.nextafter(bound, np.inf)), float(np.nextafter(bound, -np.inf))):
                            s = _aim(t, sign * m * power, c, cell)
                            if s is not None:
                                edge.append(((s, o) if axis == 0 else (o, s),
                                             (sign * m, 0.0) if axis == 0 else (0.0, sign * m), (0.0, 0.0)))
                    if not vel:
                        continue
                    s = c * cell + cell / 2
                    for v0 in (_MAX_VELOCITY, _MAX_VELOCITY - 0.25):
                        for a in (0.125,) + _MAGS:
                            for asign in (-1, 1):
                                v1 = min(max(sign * v0 + asign * a * power, -_MAX_VELOCITY), _MAX_VELOCITY)
                                out = not (0.0 <= s + v1 <= hi[axis])
                                row = ((s, o) if axis == 0 else (o, s),
                                       (asign * a, 0.0) if axis == 0 else (0.0, asign * a),
                                       (sign * v0, 0.0) if axis == 0 else (0.0, sign * v0))
                                (beyond if out else inside).append(row)
        n = want["clip"]
        ne = min(len(edge), n // 4)
        nb = min(len(beyond), (n - ne) // 2)
        for (y, x), a, v in _pick(rng, edge, ne) + _pick(rng, beyond, nb) + _pick(rng, inside, n - ne - nb):
            rows.add("clip", y, x, a[0], a[1], goal=rg, vy=v[0], vx=v[1])

    # goal_wall: inside a goal cell that touches a wall, pushed into that wall (random-goal tables: a goal per row)
    if want.get("goal_wall"):
        cand = []
        for gy in range(1, H - 1):
            for gx in range(1, W - 1):
                if grid[gy, gx] < 0:
                    continue
                for axis, sign in ((0, -1), (0, 1), (1, -1), (1, 1)):
                    for m in mags:
                        d = sign * (1.0 if cardinal else m * power)
                        for fy in (0.125, 0.375, 0.5, 0.75):
                            for fx in (0.25, 0.5, 0.625, 0.875):
                                y, x = gy + fy, gx + fx
                                ty, tx = (y + d, x) if axis == 0 else (y, x + d)
                                if wall_at(y, x) or not wall_at(ty, tx):
                                    continue
                                a = sign * (1 if cardinal else m)
                                cand.append((y, x, a if axis == 0 else 0, a if axis == 1 else 0, (gy, gx)))
        for y, x, ay, ax, g in _pick(rng, cand, want["goal_wall"]):
            rows.add("goal_wall", y, x, ay, ax, goal=g)

    # time: replicas of rows above at elapsed 0, time_limit - 1 and time_limit; a fifth of them reach the goal
    if want.get("time"):
        base = want["time"] // 3
        gc = (rg[0] + 0.5, rg[1] + 0.5)
        hit, miss = [], []
        for r in rows.r:
            if r[4] != rg:
                continue
            a = rows.moves[r[3]] if cardinal else r[3]
            sc = 1.0 if cardinal else power
            vy, vx = ((min(max(r[5] + a[0] * sc, -5.0), 5.0), min(max(r[6] + a[1] * sc, -5.0), 5.0)) if vel
                      else (a[0] * sc, a[1] * sc))
            y, x = r[1] + vy, r[2] + vx
            if wall_at(y, x):
                continue
            dy, dx = y - gc[0], x - gc[1]
            (hit if np.sqrt(dy * dy + dx * dx) <= thr else miss).append(r)
        nh = min(len(hit), base // 5)
        for r in _pick(rng, hit, nh) + _pick(rng, miss, base - nh):
            for el in (0, tl - 1, tl):
                rows.r.append((CROOMS_FAMILIES.index("time"),) + r[1:7] + (el,))

    r = rows.r
    assert len(r) == meta["num_envs"], (len(r), meta["num_envs"])
    out = dict(family=np.array([x[0] for x in r], np.int8), agent=np.array([[x[1], x[2]] for x in r], np.float64),
               goal_cell=np.array([x[4] for x in r], np.int16),
               velocity=np.array([[x[5], x[6]] for x in r], np.float64), elapsed=np.array([x[7] for x in r], np.int32))
    out["action"] = (np.array([x[3] for x in r], np.int32) if cardinal else np.array([x[3] for x in r], np.float64))
    if not cardinal:
        assert np.array_equal(out["action"], out["action"].astype(np.float32).astype(np.float64))
    return out


def crooms_table_counts(meta, family, pos, goal_cell, oob, term, trunc, agent, velocity, move):
    """The per-family counts of one table step. pos: the position after the move and before any reset (for a row
    that hit no wall: start + move), from which the ring rows' norm is recomputed with numpy as the reference does.
    agent, velocity: the input rows; move: the effective action * action_power."""
    thr = float(meta["kwargs"].get("goal_threshold", 0.5))
    family, oob = np.asarray(family), np.asarray(oob, bool)
    term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
    fam = {f: family == i for i, f in enumerate(CROOMS_FAMILIES)}
    c = {"rows_" + f: int(m.sum()) for f, m in fam.items()}
    c["boundary_oob"], c["boundary_free"] = int((fam["boundary"] & oob).sum()), int((fam["boundary"] & ~oob).sum())
    norm = np.linalg.norm(pos - (np.asarray(goal_cell) + 0.5), 2, -1)
    # one ulp above the threshold; at threshold 0 no position has that norm (5e-324): there the nearest norm a
    # position can have, one ulp of the goal centre's coordinate
    up = np.nextafter(thr, np.inf) if thr > 0.0 else np.spacing(float(meta["ring_goal"][0]) + 0.5)
    c["ring_eq"], c["ring_up"] = int((fam["ring"] & (norm == thr)).sum()), int((fam["ring"] & (norm == up)).sum())
    c["ring_oob"] = int((fam["ring"] & oob).sum())
    c["ring_term_is_norm_le_thr"] = bool(np.array_equal(term[fam["ring"]], (norm <= thr)[fam["ring"]]))
    c["goal_wall_oob_term"] = int((fam["goal_wall"] & oob & term).sum())
    c["goal_wall_oob_noterm"] = int((fam["goal_wall"] & oob & ~term).sum())
    t = fam["time"]
    c["time_trunc_only"], c["time_term_only"] = int((t & trunc & ~term).sum()), int((t & term & ~trunc).sum())
    c["time_both"], c["time_neither"] = int((t & term & trunc).sum()), int((t & ~term & ~trunc).sum())
    if bool(meta["kwargs"].get("use_velocity", False)):
        raw = np.asarray(velocity) + np.asarray(move)
        v = raw.clip(-_MAX_VELOCITY, _MAX_VELOCITY)
    else:
        raw = v = np.asarray(move)
    prop, hi = np.asarray(agent) + v, np.array(_crooms_grid(meta).shape) - 1 - 1e-6
    k = fam["clip"]
    c["clip_velocity_over"] = int((k & (np.abs(raw) > _MAX_VELOCITY).any(-1)).sum())
    c["clip_velocity_exact"] = int((k & (np.abs(raw) == _MAX_VELOCITY).any(-1)).sum())
    c["clip_grid_beyond"] = int((k & ((prop < 0.0) | (prop > hi)).any(-1)).sum())
    c["clip_grid_on_bound"] = int((k & ((prop == 0.0) | (prop == hi)).any(-1)).sum())
    # rows on which floor(x / cell_size) is not floor(x * (1 / cell_size)): they tell the divide from a reciprocal
    cell, pc = float(meta["kwargs"].get("cell_size", 1.0)), prop.clip(0.0, hi)
    c["cell_reciprocal_differs"] = int((np.floor(pc / cell) != np.floor(pc * (1.0 / cell))).any(-1).sum())
    c["deterministic"] = int((~oob & ~term & ~trunc).sum())
    return c


def crooms_table_check_counts(meta, c):
    """The conditions every crooms_table case was built to meet (asserted by the generator and by the CPU test)."""
    B, want = meta["num_envs"], meta["rows"]
    assert B <= 4096 and B % 2 == 1 and B % 512 != 0, B
    for f in CROOMS_FAMILIES:
        assert c["rows_" + f] == want.get(f, 0), (f, c["rows_" + f])
    if want.get("boundary"):
        assert c["boundary_oob"] >= 200 and c["boundary_free"] >= 200, c
    if want.get("ring"):
        assert want["ring"] >= 2048 and c["ring_oob"] == 0 and c["ring_term_is_norm_le_thr"], c
        assert c["ring_eq"] >= 30 and c["ring_up"] >= 30, c
    if want.get("clip"):
        assert min(c["clip_velocity_over"], c["clip_velocity_exact"], c["clip_grid_beyond"],
                   c["clip_grid_on_bound"]) >= 10, c
    if want.get("goal_wall"):
        assert c["goal_wall_oob_term"] >= 10 and c["goal_wall_oob_noterm"] >= 10, c
    if want.get("time"):
        assert min(c["time_trunc_only"], c["time_term_only"], c["time_both"], c["time_neither"]) >= 10, c
    if float(meta["kwargs"].get("cell_size", 1.0)) == 1.25:
        assert c["cell_reciprocal_differs"] >= 50, c
    assert 2 * c["deterministic"] >= B, c


# ---- FourRooms / ROOMS one-step tables (make_golden.py GRID_TABLES) ----
# Every row is one env: an agent cell, a goal cell, an elapsed count and an intended action (the effective one comes
# from the stream). Rows: every walkable agent cell (stairs included) x every intended action x the goal replicas x
# elapsed {0, time_limit - 1, time_limit}. Random-goal tables set the goal per row: the cell the intended action leads
# to (stair transit included), the neighbour in each of the 4 / 8 observation directions, the agent's own cell and one
# far cell; a goal that would fall on a cell no goal can take is the far cell instead. Fixed-goal tables keep the
# configuration's goal and repeat every row `reps` times (other draws). Scalar-obs tables are padded with repeats of
# their first rows to a multiple of 512, the staged fused kernel's tile.
def load_grid_table(name):
    """A `grid_table` case (make_golden.py GRID_TABLES): (index entry, dict of the recorded arrays)."""
    meta = load_index()["grid_table"][name]
    with np.load(os.path.join(GOLDEN_DIR, meta["file"]), allow_pickle=False) as z:
        return meta, {k: z[k] for k in z.files}


def grid_table_oracle(meta, B=1):
    """The numpy oracle of a grid_table case's configuration (its maps, actions and valid cells drive the rows)."""
    from oracle import gridworld
    kw = dict(meta["kwargs"])
    for k in ("goal_xyz", "goal_xy"):
        if kw.get(k) is not None:
            kw[k] = tuple(kw[k])
    cls = gridworld.FourRoomsOracle if meta["kind"] == "fourrooms" else gridworld.RoomsOracle
    return cls(B, **kw)


def grid_table_dirs(meta):
    """The observation directions of a table: 8 with a Hansen-8 obs or ordinal actions, else 4."""
    kw = meta["kwargs"]
    default = "cardinal" if meta["kind"] == "fourrooms" else "ordinal"
    return 8 if "8" in kw.get("obs_type", "mdp") or kw.get("action_type", default) == "ordinal" else 4


def grid_dest(ora, cell, a):
    """(cell after effective action a, blocked): the move, then the stair transit (msrooms.py:401-404, :419-428)."""
    prop = tuple(int(v) for v in np.asarray(cell) + ora.actions[a])
    v = ora.grid[prop]
    if v == ora.wall_value:
        return tuple(int(x) for x in cell), True
    if ora.grid.ndim == 3 and v == 3:
        return (prop[0] + 1, int(ora.DOWN_YX[0]), int(ora.DOWN_YX[1])), False
    if ora.grid.ndim == 3 and v == 2:
        return (prop[0] - 1, int(ora.UP_YX[0]), int(ora.UP_YX[1])), False
    return prop, False


def grid_table_cells(ora):
    """Every cell an agent can stand on, all floors: coordinates [n, ndim] in flat order."""
    walk = ora.grid != ora.wall_value
    return np.array(np.nonzero(walk)).T


def grid_table_inputs(meta):
    """Build the rows of a grid_table case: dict(agent [B, ndim], goal [B, ndim], elapsed [B], action [B], all int64;
    variant int8 [B]: 0 destination, 1.. the observation directions, -2 own cell, -1 far, -3 fixed goal).
    Deterministic in meta (kind, kwargs, reps, rows, num_envs)."""
    ora = grid_table_oracle(meta)
    shape, nd = ora.grid.shape, ora.grid.ndim
    tl = int(meta["kwargs"]["time_limit"])
    nact = ora.actions.shape[0]
    from oracle.gridworld import ACTIONS_ORDINAL, ACTIONS_ORDINAL_Z
    dirs = (ACTIONS_ORDINAL_Z if nd == 3 else ACTIONS_ORDINAL)[::8 // grid_table_dirs(meta)]
    cells = grid_table_cells(ora)
    fixed = ora.fixed_goal is not None
    vg = set(int(v) for v in ora.valid_goal)
    vgc = np.array(np.unravel_index(np.asarray(ora.valid_goal), shape)).T
    A, G, E, ACT, V = [], [], [], [], []
    for c in cells:
        c = tuple(int(v) for v in c)
        if fixed:
            goals = [(-3, tuple(int(v) for v in ora.fixed_goal))] * int(meta["reps"])
            far = None
        else:
            dist = np.abs(vgc[:, -2:] - np.array(c[-2:])).sum(-1)
            far = tuple(int(v) for v in vgc[int(dist.argmax())])
        els = (0, tl - 1, tl)
        for a in range(nact):
            if not fixed:
                cand = [(0, grid_dest(ora, c, a)[0])]
                cand += [(1 + j, tuple(int(v) for v in np.array(c) + d)) for j, d in enumerate(dirs)]
                cand += [(-2, c), (-1, far)]
                goals = [(v, g if int(np.ravel_multi_index(g, shape)) in vg else far) for v, g in cand]
            for v, g in goals:
                for e in els:
                    A.append(c)
                    G.append(g)
                    E.append(e)
                    ACT.append(a)
                    V.append(v)
    out = dict(agent=np.array(A, np.int64).reshape(-1, nd), goal=np.array(G, np.int64).reshape(-1, nd),
               elapsed=np.array(E, np.int64), action=np.array(ACT, np.int64), variant=np.array(V, np.int8))
    n = out["elapsed"].size
    assert n == meta["rows"], (n, meta["rows"])
    pad = meta["num_envs"] - n
    assert 0 <= pad < 512
    if pad:
        out = {k: np.concatenate((v, v[:pad])) for k, v in out.items()}
    return out


def grid_table_counts(meta, inp, eff, rew, term, trunc):
    """The counts of one table step from its inputs, the effective actions and the step's outputs (the padding rows
    excluded)."""
    ora = grid_table_oracle(meta)
    kw, n = meta["kwargs"], meta["rows"]
    term, trunc = np.asarray(term, bool)[:n], np.asarray(trunc, bool)[:n]
    rew, eff = np.asarray(rew)[:n], np.asarray(eff)[:n]
    agent, goal = inp["agent"][:n], inp["goal"][:n]
    nact = ora.actions.shape[0]
    cells = grid_table_cells(ora)
    cell_id = {tuple(int(v) for v in c): i for i, c in enumerate(cells)}
    dest = np.zeros((len(cells), nact), np.int64)
    blocked = np.zeros((len(cells), nact), bool)
    onstair = np.zeros((len(cells), nact), bool)
    for i, c in enumerate(cells):
        for a in range(nact):
            d, b = grid_dest(ora, c, a)
            dest[i, a], blocked[i, a] = np.ravel_multi_index(d, ora.grid.shape), b
            onstair[i, a] = (not b) and d != tuple(int(v) for v in c + ora.actions[a])
    ci = np.array([cell_id[tuple(int(v) for v in c)] for c in agent])
    seen = np.zeros((len(cells), nact), bool)
    seen[ci, eff] = True
    need = np.array([[(dest[i] != dest[i, a]).any() for a in range(nact)] for i in range(len(cells))])
    row_blocked, row_stair = blocked[ci, eff], onstair[ci, eff]
    on_goal = (agent == goal).all(-1)
    stepped = agent + ora.actions[eff]  # the cell moved onto, before any stair transit
    c = dict(rows=int(n), cells=int(len(cells)), pairs_needed=int(need.sum()), pairs_seen=int((need & seen).sum()),
             term_only=int((term & ~trunc).sum()), trunc_only=int((trunc & ~term).sum()),
             both=int((term & trunc).sum()), neither=int((~term & ~trunc).sum()),
             blocked=int(row_blocked.sum()),
             blocked_on_goal=int((row_blocked & on_goal & term & (rew == np.float32(kw["goal_reward"]))).sum()),
             wall_reward=int((rew == np.float32(kw["wall_reward"])).sum()),
             stair_transits=int(row_stair.sum()),
             stair_is_goal_not_term=int((row_stair & (stepped == goal).all(-1) & ~term).sum()),
             stair_onto_goal_term=int((row_stair & term).sum()))
    return c


GRID_UNIFORM_P = {4: 0.75, 8: 0.875}  # every effective action has probability 1 / n


def grid_table_check_counts(meta, c):
    """The conditions every grid_table case was built to meet (asserted by the generator and by the CPU test)."""
    ora = grid_table_oracle(meta)
    kw = meta["kwargs"]
    nact = ora.actions.shape[0]
    assert c["rows"] == meta["rows"], c
    assert c["rows"] >= c["cells"] * nact * 12, c  # >= 48 / 96 rows per cell
    if kw["action_failure_probability"] == GRID_UNIFORM_P[nact]:
        assert c["pairs_seen"] == c["pairs_needed"] > 0, c
    assert min(c["term_only"], c["trunc_only"], c["both"], c["neither"]) >= 1, c
    if meta.get("no_blocked_on_goal"):  # a fixed goal with eight walkable neighbours under ordinal actions
        assert c["blocked_on_goal"] == 0, c
    else:
        assert c["blocked_on_goal"] >= 1, c
    assert c["wall_reward"] >= 1 and c["blocked"] >= c["wall_reward"] + c["blocked_on_goal"], c
    if ora.grid.ndim == 3 and ora.grid.shape[0] > 1:
        assert c["stair_transits"] >= 1, c
        if ora.fixed_goal is None:
            assert c["stair_is_goal_not_term"] >= 1 and c["stair_onto_goal_term"] >= 1, c
