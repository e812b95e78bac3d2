"""The planted-draw cases of C-ROOMS and Taxi exact mode, built on the CPU (tests only; a plain module).

tests/test_stream_plant_cpu.py asserts on numpy alone that every case takes its rare branch;
tests/test_crooms_plant_gpu.py and tests/test_taxi_plant_gpu.py run the same cases on the device. A case is a tuple
of plain values (it is also the pytest id); `*_build` turns it into the planted PCG64 state, the env state to set and
the actions, with the oracle (oracle/crooms.py, oracle/taxi.py) in the same state on numpy's Generator.
"""
import numpy as np

import stream_plant as sp
from oracle.crooms import CRoomsOracle
from oracle.draws import NumpyDraws
from oracle.taxi import TaxiOracle

INC = np.random.default_rng(2024).bit_generator.state["state"]["inc"]  # a stream increment (odd), as numpy seeds it


class RecordingDraws(NumpyDraws):
    """NumpyDraws that notes the sites drawn and the generator state before every choice() call."""

    def __init__(self, gen):
        super().__init__(gen)
        self.normal_sites, self.choice_calls = [], []

    def record_normal(self, site, mask, v):
        self.normal_sites.append(site)

    def choice(self, values, mask, site):
        self.choice_calls.append((site, int(mask.sum()), self.gen.bit_generator.state))
        return super().choice(values, mask, site)


# ------------------------------------------------------------------------------------------------ C-ROOMS ----
# path -> (envs, gp_debug_set knobs at create): the one-workgroup kernel (x_choices; 1024-word windows), the grid-wide
# fused calls (xg_cho_fused; 256-word blocks), one partial block, and the two-launch calls (xg_cho_count / _write)
CR_PATHS = {
    "wg600": (600, {}),
    "wg3000": (3000, {"xg_min_envs": 4096}),
    "fused1500": (1500, {}),
    "fused64": (64, {"xg_min_envs": 0}),
    "split1500": (1500, {"disable_fused": 1}),
}
CR_KW = dict(layout="4", action_type="cardinal", action_std=0.0, obs_type="vector_goal_mdp", time_limit=20)
CR_BLOCK_EDGES = (510, 511, 512, 2047, 2048)


def crooms_cases():
    """(path, place, n, h, buffered, call, calls): half-word h of choice call `call` (of `calls`: 2 = goal then agent,
    goal_xy=None) rejected, n draws per call, with or without a buffered half before the first call; place =
    "reset" (n = B, the stream starts at the call) or "step" (B uniforms first, n envs truncate)."""
    out = []
    for path, (B, _) in CR_PATHS.items():
        hs = [h for h in (0, 1) + CR_BLOCK_EDGES + (B - 2, B - 1) if h < B]
        for h in hs:
            out.append((path, "reset", B, h, False, 0, 1))
        for h in (0, B - 1):
            out.append((path, "reset", B, h, True, 0, 1))
        # two calls: the first (goal), then the second (agent), B halves on, the buffered half carried between them
        for buffered in (False, True):
            out += [(path, "reset", B, 0, buffered, 0, 2), (path, "reset", B, B - 1, buffered, 0, 2),
                    (path, "reset", B, 0, buffered, 1, 2), (path, "reset", B, B - 1, buffered, 1, 2)]
        out += [(path, "reset", B, h, False, 1, 2) for h in (1, 511, 512, 2047, 2048) if h < B]
        odd = 301 if B > 301 else 33
        out += [(path, "step", 1, 0, True, 0, 1), (path, "step", 2, 0, True, 0, 1), (path, "step", 1, 0, False, 0, 1),
                (path, "step", 2, 1, False, 0, 1), (path, "step", 2, 1, True, 0, 1)]
        out += [(path, "step", odd, h, b, 0, 1) for h in (0, 1, odd - 2, odd - 1) for b in (False, True)]
        out += [(path, "step", B, h, False, 0, 1) for h in hs]
        out += [(path, "step", odd, odd - 1, False, 0, 2), (path, "step", odd, 0, False, 1, 2),
                (path, "step", odd, odd - 1, True, 1, 2)]
    return out


def crooms_id(case):
    path, place, n, h, buffered, call, calls = case
    return f"{path}-{place}-n{n}-h{h}{'-buf' if buffered else ''}-call{call}of{calls}"


def _open_cell(grid, avoid):
    """A free cell whose four neighbours are free and none of them (nor itself) is within one cell of `avoid`."""
    H, W = grid.shape
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            nb = [(y, x), (y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)]
            if all(grid[c] >= 0 for c in nb) and all(abs(c[0] - avoid[0]) + abs(c[1] - avoid[1]) > 2 for c in nb):
                return y, x
    raise AssertionError("no open cell")


class CRoomsPlant:
    pass


def crooms_build(case, accepted_twin=False):
    """The case on the CPU: .kw (constructor arguments), .B, .st (planted state dict; with `accepted_twin` a
    state built the same way around an accepted half in place of the rejected one), .ora (oracle on a Generator at
    .st, env state set for a "step" case), .agent / .goal_cell / .elapsed (what set_state gets, "step" only),
    .actions ("step" only), .nv (valid cells), .value (the planted half)."""
    path, place, n, h, buffered, call, calls = case
    B = CR_PATHS[path][0]
    c = CRoomsPlant()
    c.case, c.B, c.knobs = case, B, CR_PATHS[path][1]
    c.kw = dict(CR_KW, goal_xy=None) if calls == 2 else dict(CR_KW)
    c.ora = ora = CRoomsOracle(B, **c.kw)
    c.nv = nv = len(ora.valid)
    c.value = sp.rejected_word(nv)
    value = c.value + 1 if accepted_twin else c.value
    assert sp.is_rejected(c.value, nv) and not sp.is_rejected(c.value + 1, nv) and not sp.is_rejected(0x9E3779B9, nv)
    c.words_before = B if place == "step" else 0
    g = h + (n if call == 1 else 0)  # (no rejection before the planted half: the calls' halves are contiguous)
    seed = sum(map(ord, crooms_id(case)))
    c.st = sp.plant_half(INC, g, value, seed, buffered, c.words_before)
    ora.gen = sp.generator_at(c.st)
    if place == "step":
        assert n <= B
        goal = tuple(int(v) for v in ora.fixed_goal) if ora.fixed_goal is not None else (1, 1)
        if ora.grid[goal] < 0:
            goal = tuple(int(v) for v in np.argwhere(ora.grid >= 0)[0])
        cell = _open_cell(ora.grid, goal)
        c.agent = np.tile(np.array(cell, dtype=np.float64) + 0.5, (B, 1))
        c.goal_cell = np.tile(np.array(goal, dtype=np.int32), (B, 1))
        who = np.sort(np.random.default_rng(seed).permutation(B)[:n])
        c.elapsed = np.zeros(B, dtype=np.int32)
        c.elapsed[who] = c.kw["time_limit"]
        c.actions = np.random.default_rng(seed + 1).integers(0, 4, B)
        ora.agent = c.agent.copy()
        ora.goal = c.goal_cell.astype(np.float64) + 0.5
        ora.elapsed = c.elapsed.astype(int)
        ora.velocity = np.zeros((B, 2))
    return c


def crooms_oracle_planted(c):
    """Run the planted reset / step on the oracle; returns (obs, rew, term, trunc) (reset: obs only, the rest None)
    and the RecordingDraws. Asserts what the placement rests on: no normal was drawn, and the choice calls are the
    case's."""
    path, place, n, h, buffered, call, calls = c.case
    draws = RecordingDraws(c.ora.gen)
    if place == "reset":
        out = (c.ora.reset(draws), None, None, None)
    else:
        out = c.ora.step(c.actions, draws)
        assert not out[2].any() and int(out[3].sum()) == n  # no env reached the goal; n truncated
    assert draws.normal_sites == [], draws.normal_sites
    assert [(s, k) for s, k, _ in draws.choice_calls] == ([("goal", n)] if calls == 2 else []) + [("agent", n)]
    return out, draws


# --------------------------------------------------------------------------------------------------- Taxi ----
TAXI_MAP6 = ["R: :G", " : : ", "P: :W", " : : ", "Y: :B"]   # 5 x 3 cells, six locations: integers(6), threshold 4
TAXI_MAP3 = ["R: :G", " : : ", "Y: : "]                     # 3 x 3 cells, three locations: threshold 1 (half 0 only)
TAXI_MAPS = {"six": TAXI_MAP6, "three": TAXI_MAP3}
# path -> (envs, knobs): the one-workgroup kernel (np_draws in taxi_np_kernel), the grid-wide form (taxi_npg_draws)
TX_PD_PATHS = {"wg512": (512, {}), "grid512": (512, {"taxi_npg_min": 0}), "grid4099": (4099, {})}
TX_PD_KW = dict(num_passengers=3, time_limit=200)


def taxi_pd_cases():
    """(path, map, b1, where, mode): b1 task completions in the planted step; the rejected half-word is the buffered
    half ("buf"), in the p range ("p"), in the d range ("d") or in the first redraw round ("redraw"); mode = "step"
    or "rollout" (the second step of a K = 3 launch)."""
    out = []
    for path, (B, _) in TX_PD_PATHS.items():
        for b1 in (1, 2, 37, B):
            for where in ("buf", "p", "d", "redraw"):
                for mode in ("step", "rollout"):
                    out.append((path, "six", b1, where, mode))
        out += [(path, "three", 37, where, "step") for where in ("buf", "p", "d", "redraw")]
    return out


def taxi_pd_id(case):
    return "-".join(str(x) for x in case)


class TaxiPlant:
    pass


def _pd_walk(st, L, b1):
    """_reset_passenger_and_destination's draws from the state dict st on the restated PCG64: (p, d, the rejected
    half-word indices counted over the whole walk, colliders per redraw round, state dict afterwards)."""
    rej, k = [], 0
    p, r, st = sp.lemire_trace(st, L, b1)
    rej += [k + x for x in r]
    k += b1 + len(r)
    d, r, st = sp.lemire_trace(st, L, b1)
    rej += [k + x for x in r]
    k += b1 + len(r)
    rounds = []
    while (p == d).any():
        m = int((p == d).sum())
        rounds.append(m)
        v, r, st = sp.lemire_trace(st, L, m)
        rej += [k + x for x in r]
        k += m + len(r)
        d[p == d] = v
    return p, d, rej, rounds, st


def taxi_pd_build(case, accepted_twin=False):
    """.kw, .B, .st (planted state), .h (the rejected half-word's index in the walk), .s / .actions (noop, planted,
    noop: what the envs hold and do), .who (the completing envs), .ora (oracle at .st with .s set), .walk (the
    restated draws from .st: p, d, rejected indices, redraw rounds, end state)."""
    path, mapname, b1, where, mode = case
    B, knobs = TX_PD_PATHS[path]
    c = TaxiPlant()
    c.case, c.B, c.knobs, c.mode = case, B, knobs, mode
    c.kw = dict(TX_PD_KW, map=TAXI_MAPS[mapname])
    c.ora = ora = TaxiOracle(B, **c.kw)
    L = ora.nlocs
    value = sp.rejected_word(L, 0 if sp.lemire_threshold(L) == 1 else 1)
    assert sp.is_rejected(value, L)
    c.value = value
    base = sum(map(ord, taxi_pd_id(case)))
    buffered = where == "buf" or ((base & 1) == 1 and not (where == "p" and b1 == 1))
    for seed in range(base, base + 400):
        # the half-word to reject (half 0 is the buffered one when there is one); a redraw plant needs a collision
        # in this stream, which the seed decides
        if where == "buf":
            h = 0
        elif where == "p":
            h = (seed * 7) % b1
            h = max(h, 1) if buffered else h
        elif where == "d":
            h = b1 + (seed * 5) % b1
        else:
            h = 2 * b1 + (seed % 3 if b1 > 100 else 0)
        walk = _pd_walk(sp.plant_half(INC, h, value, seed, buffered), L, b1)
        if walk[2] == [h] and (where != "redraw" or h < 2 * b1 + walk[3][0]):
            break
    else:
        raise AssertionError("no stream with the wanted rejection")
    assert not sp.is_rejected(value + 1, L)
    st = sp.plant_half(INC, h, value + 1 if accepted_twin else value, seed, buffered)
    c.st, c.h, c.walk, c.buffered = st, h, walk, buffered
    # every env waits in the taxi on a location; the completing ones on their destination
    rng = np.random.default_rng(base)
    c.who = np.sort(rng.permutation(B)[:b1])
    at = rng.integers(0, L, B)
    dest = (at + rng.integers(1, L, B)) % L
    dest[c.who] = at[c.who]
    locs = ora.np_locs[:L]
    c.s = ora.encode(locs[at, 0], locs[at, 1], L, dest).astype(np.int64)
    noop = np.where(locs[at, 1] == 0, 2, 3)  # west on column 0, east on the last column: the move is clipped
    assert set(np.unique(locs[:, 1])) <= {0, ora.cols - 1}
    planted = noop.copy()
    planted[c.who] = 4
    c.actions = np.stack([noop, planted, noop]) if mode == "rollout" else planted[None]
    c.planted_step = 1 if mode == "rollout" else 0
    ora.gen = sp.generator_at(c.st)
    ora.s = c.s.copy()
    ora.elapsed = np.zeros(B, dtype=int)
    ora.n_dropoffs_completed = np.zeros(B)
    return c


# Taxi multinomial rows: path -> (envs, knobs); np_reset_rows walks 64 rows x 16 deficits per round, taxi_npg_rows
# 1024 rows x 64 candidate starts
TX_ROW_PATHS = {"wg200": (200, {}), "wg1024": (1024, {}), "grid200": (200, {"taxi_npg_min": 0}), "grid2500": (2500, {})}


def taxi_row_cases():
    """(path, place, row, what): the double of one category of multinomial row `row` comes from the word 2^64 - 1.
    what: "c0" / "mid" / "late" / "last" name row 0's category (the first, a middle one, a late one with balls still
    above the inversion's bound, and the last drawn one, whose conditional p is 1: numpy draws the double and does
    not restart); "def0" / "defpos" ask for a row 1 with deficit 0 / positive before it (row 0 drew C0 / fewer
    doubles); "lastof" / "firstof" for rows 63 / 64 as the last of one speculative round of np_reset_rows and the
    first of the next; "any" for no condition. place = "reset" or "step" (every env truncates)."""
    out = []
    for path, (B, _) in TX_ROW_PATHS.items():
        rows = [(0, "c0"), (0, "mid"), (0, "late"), (0, "last"), (1, "def0"), (1, "defpos"), (63, "lastof"),
                (64, "firstof"), (B - 1, "any")]
        if B > 1025:
            rows += [(1023, "any"), (1024, "any")]
        for row, what in rows:
            out.append((path, "reset", row, what))
        out += [(path, "step", row, what) for row, what in ((0, "mid"), (1, "def0"), (64, "firstof"), (B - 1, "any"))]
    return out


def taxi_row_id(case):
    return "-".join(str(x) for x in case)


_ROW_CACHE = {}


def taxi_row_build(case):
    """.kw, .B, .info (stream_plant.plant_multinomial_word's dict: state, row_words, extra, ...), .restarts (whether
    numpy restarts the inversion for this plant: all but "last"), .ora (oracle at the state, elapsed at the limit for
    "step"), .actions."""
    path, place, row, what = case
    B, knobs = TX_ROW_PATHS[path]
    c = TaxiPlant()
    c.case, c.B, c.knobs = case, B, knobs
    c.kw = dict(time_limit=30)
    c.ora = ora = TaxiOracle(B, **c.kw)
    p, ns = ora.state_distribution, ora.ns
    c0 = int((p > 0).sum())
    c.c0 = c0
    cat = {"c0": 0, "mid": c0 // 2, "late": (c0 * 5) // 6, "last": c0 - 1}.get(what)
    accept = None
    if what == "def0":
        accept = lambda i: i["row_words"][0] == c0  # noqa: E731
    elif what == "defpos":
        accept = lambda i: i["row_words"][0] < c0  # noqa: E731
    elif what == "lastof":
        accept = lambda i: (0, 64) == sp.speculative_rounds(i["row_words"], c0)[0][:2]  # noqa: E731
    elif what == "firstof":
        accept = lambda i: (0, 64) == sp.speculative_rounds(i["row_words"], c0)[0][:2]  # noqa: E731
    key = (row, what)
    if key not in _ROW_CACHE:
        _ROW_CACHE[key] = sp.plant_multinomial_word(ns, p, row, INC, cat, seed=1000 * row + len(what), accept=accept)
    c.info = _ROW_CACHE[key]
    c.restarts = what != "last"
    ora.gen = sp.generator_at(c.info["state"])
    if place == "step":
        ora.s = np.random.default_rng(row).choice(ora.valid_states, B)
        ora.elapsed = np.full(B, c.kw["time_limit"], dtype=int)
        ora.n_dropoffs_completed = np.zeros(B)
        c.s = ora.s.copy()
        c.actions = np.random.default_rng(row + 1).integers(0, 4, B)  # (moves only: no pick-up, no drop-off)
    return c
