"""CPU tests of grid Heaven-Hell's host side: the default maze lowered from the reference's geometry by
`heaven_hell_maze`, the refusals of a maze, the numpy oracle of the build-defined rules (tests/heavenhell_oracle.py)
against its own scalar one-env statement over every transition of a 3 x 3 T and of the default maze, the slip
threshold, the ctypes struct and the package export. No GPU is touched."""
import ctypes

import numpy as np
import pytest

from heavenhell_oracle import (FREE, LEFT, PRIEST, RIGHT, START, T3, TOP, HeavenHellOracle, Spec, enumeration,
                               hansen_code, scalar_step)

DYADIC = dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=-0.25, wall_reward=-0.5)
PICTURE = ("LLL....PP....RRR",
           "LLLL..PPPP..RRRR",
           "LLLL..PPPP..RRRR",
           "LLL....PP....RRR",
           "######....######",
           "######....######",
           "######....######",
           "######.SS.######",
           "######....######",
           "######....######")


def test_default_maze_is_the_picture():
    from gym_po_amd import heaven_hell_maze
    from gym_po_amd.envs.heaven_hell_grid import hansen_codes, parse_maze
    maze = heaven_hell_maze(((-6.25, 6.0), (6.25, 6.0)), (0.0, 6.0), 2.0)
    assert maze == PICTURE and heaven_hell_maze() == PICTURE
    H, W, flags = parse_maze(maze)
    assert (H, W) == (10, 16) and flags.dtype == np.uint8
    cells = lambda bit: np.flatnonzero(flags & bit).tolist()  # noqa: E731
    assert len(cells(FREE)) == 88
    assert cells(LEFT) == [0, 1, 2, 16, 17, 18, 19, 32, 33, 34, 35, 48, 49, 50]
    assert cells(RIGHT) == [13, 14, 15, 28, 29, 30, 31, 44, 45, 46, 47, 61, 62, 63]
    assert cells(PRIEST) == [7, 8, 22, 23, 24, 25, 38, 39, 40, 41, 55, 56]
    assert cells(START) == [119, 120]
    # breadth-first distance from each start cell to the priest area: 4 moves
    free = (flags & FREE) != 0
    for s in (119, 120):
        dist, frontier = {s: 0}, [s]
        while frontier:
            nxt = []
            for c in frontier:
                r, q = divmod(c, W)
                for rr, qq in ((r - 1, q), (r, q + 1), (r + 1, q), (r, q - 1)):
                    n = rr * W + qq
                    if 0 <= rr < H and 0 <= qq < W and free[n] and n not in dist:
                        dist[n] = dist[c] + 1
                        nxt.append(n)
            frontier = nxt
        assert len(dist) == 88  # the maze is connected
        assert min(dist[c] for c in cells(PRIEST)) == 4
    # the Hansen codes that occur: the free-neighbour complement of {0, 1, 2, 3, 4, 6, 8, 9, 12}
    codes = hansen_codes(H, W, flags)
    assert codes.dtype == np.int32
    assert [int(codes[c]) for c in range(H * W)] == [hansen_code(H, W, flags.tolist(), c) for c in range(H * W)]
    assert {15 - int(codes[c]) for c in cells(FREE)} == {0, 1, 2, 3, 4, 6, 8, 9, 12}


def test_other_geometry_moves_the_areas():
    from gym_po_amd import heaven_hell_maze
    m = heaven_hell_maze(((-6.25, 6.0), (6.25, 6.0)), (0.0, 6.0), 1.0)
    assert m[0] == "................" and m[1] == ".LL....PP....RR." and m[2] == m[1] and m[7] == PICTURE[7]
    with pytest.raises(ValueError, match="overlap"):
        heaven_hell_maze(((-1.0, 6.0), (6.25, 6.0)), (0.0, 6.0), 2.0)
    with pytest.raises(ValueError, match="start cell"):
        heaven_hell_maze(((-6.25, 6.0), (6.25, 6.0)), (0.0, 1.0), 2.0)


def test_refusals():
    from gym_po_amd import HeavenHellGridEnv
    from gym_po_amd.envs.heaven_hell_grid import check_flags, parse_maze
    with pytest.raises(ValueError, match="no start cell"):
        parse_maze(("LPR", "#.#", "#.#"))
    with pytest.raises(ValueError, match="outside the set"):
        parse_maze(("LPR", "#x#", "#S#"))
    with pytest.raises(ValueError, match="side outside"):
        parse_maze(("S" + "." * 16,))
    with pytest.raises(ValueError, match="side outside"):
        parse_maze(("S",) + (".",) * 16)
    with pytest.raises(ValueError, match="unequal"):
        parse_maze(("LPR", "#S"))
    flags = np.array([FREE | LEFT | START, FREE, FREE | RIGHT], dtype=np.uint8)
    with pytest.raises(ValueError, match="lies in the left or right area"):
        check_flags(1, 3, flags)
    flags[0], flags[2] = FREE | LEFT, FREE | RIGHT | START
    with pytest.raises(ValueError, match="lies in the left or right area"):
        check_flags(1, 3, flags)
    # the constructor raises them before anything touches the GPU
    with pytest.raises(ValueError, match="no start cell"):
        HeavenHellGridEnv(4, maze=("L.R",))
    with pytest.raises(ValueError, match="outside the set"):
        HeavenHellGridEnv(4, maze="LSR\n#?#")
    with pytest.raises(ValueError, match="side outside"):
        HeavenHellGridEnv(4, maze=("S" * 17,))
    with pytest.raises(ValueError, match="obs_type"):
        HeavenHellGridEnv(4, obs_type="vector")
    with pytest.raises(ValueError, match="action_failure_probability"):
        HeavenHellGridEnv(4, action_failure_probability=1.5)
    assert parse_maze("LPR\n#.#\n#S#")[2].tolist() == parse_maze(T3)[2].tolist()


def test_keep_thr():
    from gym_po_amd.envs.heaven_hell_grid import keep_threshold
    assert keep_threshold(0.0) == TOP  # never slips: every 31-bit draw is below it
    assert keep_threshold(1.0) == 0  # always slips
    assert keep_threshold(1 / 3) == 1431655765 == int(np.floor((1.0 - 1 / 3) * 2.0 ** 31))
    assert keep_threshold(0.5) == 1 << 30


# every 32-bit word that matters to a rule: no slip / slip at the threshold's two sides, each slip target at its
# interval's two ends, both start indices of a 2-start maze, both sides
def _draw_variants(keep_thr):
    ys = sorted({0, max(keep_thr - 1, 0), min(keep_thr, TOP - 1), TOP - 1})
    x0s = [2 * y + 1 for y in ys]
    x1s = [0, 0x55555555, 0x55555556, 0xAAAAAAAA, 0xAAAAAAAB, 0xFFFFFFFF]
    x23 = [(0, 0), (0x7FFFFFFF, 1), (0x80000000, 2), (0xFFFFFFFF, 0xFFFFFFFF)]
    return [(x0, x1, x2, x3) for x0 in x0s for x1 in x1s for x2, x3 in x23]


@pytest.mark.parametrize("maze", [T3, PICTURE], ids=["t3", "default"])
@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
@pytest.mark.parametrize("p", [0.0, 1 / 3, 1.0])
def test_vectorised_oracle_equals_the_scalar_statement(maze, obs_type, p):
    from gym_po_amd.envs.heaven_hell_grid import keep_threshold
    tl = 7
    sp = Spec(maze, obs_type, keep_threshold(p), tl, **DYADIC)
    cell, side, act, el = enumeration(sp, tl)
    n = cell.size
    assert n == len(sp.free_cells) * 2 * 8 * 2
    variants = _draw_variants(sp.keep_thr)
    if len(maze) > 3:  # the default maze: not slipped, and slipped to each target; the reset words go round by env
        variants = [(1, 0, 0, 0)] + [(0xFFFFFFFF, x1, 0, 0) for x1 in (0, 0x55555556, 0xAAAAAAAB)]
    V = len(variants)
    cell, side, act, el = (np.repeat(x, V) for x in (cell, side, act, el))
    words = np.array(variants * n, dtype=np.uint64).T
    if len(maze) > 3:
        words[2] = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x80000000], dtype=np.uint64)[np.arange(n * V) % 5]
        words[3] = np.array([0, 1, 2], dtype=np.uint64)[np.arange(n * V) % 3]
    B = cell.size
    ora = HeavenHellOracle(B, sp)
    ora.agent[:], ora.side[:], ora.elapsed[:] = cell, side, el
    draws = ora.draws_of_words(*words)
    o, r, d, tr = ora.step(act, draws)
    assert r.dtype == np.float32 and o.dtype == np.int32
    seen, slipped_to = set(), set()
    for b in range(B):
        x = [int(w) for w in words[:, b]]
        want = scalar_step(sp, int(cell[b]), int(side[b]), int(el[b]), int(act[b]), *x)
        got = (int(ora.agent[b]), int(ora.side[b]), int(ora.elapsed[b]), int(o[b]), r[b], bool(d[b]), bool(tr[b]))
        assert got == want, (b, cell[b], side[b], el[b], act[b], x, got, want)
        seen.add((float(r[b]), bool(d[b]), bool(tr[b])))
        if (x[0] >> 1) >= sp.keep_thr:
            slipped_to.add((x[1] * 3) >> 32)
    assert {x[0] for x in seen} == {1.0, -1.0, -0.25, -0.5}  # every reward of the config occurred
    assert d.any() and tr.any() and not tr.all() and not d.all()
    assert slipped_to == (set() if p == 0.0 else {0, 1, 2})
    assert o.min() >= 0 and o.max() < sp.n_obs and set(np.unique(o % 3)) == {0, 1, 2}
    assert set(np.unique(ora.agent[d | tr])) == set(sp.starts)  # every start cell is drawn


def test_struct_layout_and_exports():
    import gym_po_amd
    from gym_po_amd import _lib
    assert _lib.GP_KIND_HEAVENHELL == 7
    c = _lib.HeavenHellConfig
    assert [f[0] for f in c._fields_] == ["height", "width", "flags", "obs_base", "obs_base_n", "keep_thr",
                                          "time_limit", "heaven_reward", "hell_reward", "step_reward", "wall_reward"]
    offs = {name: getattr(c, name).offset for name, _ in c._fields_}
    assert offs == dict(height=0, width=4, flags=8, obs_base=16, obs_base_n=24, keep_thr=28, time_limit=32,
                        heaven_reward=36, hell_reward=40, step_reward=44, wall_reward=48)
    assert ctypes.sizeof(c) == 56 and ctypes.alignment(c) == 8
    assert c.keep_thr.size == 4 and c.flags.size == 8
    assert "HeavenHellGridEnv" in gym_po_amd.__all__ and "heaven_hell_maze" in gym_po_amd.__all__
    assert gym_po_amd.HeavenHellGridEnv.__name__ == "HeavenHellGridEnv"
