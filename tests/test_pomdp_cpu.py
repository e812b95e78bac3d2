"""CPU tests of the tabular POMDP's host side: the numpy oracle of the build-defined rules (tests/pomdp_oracle.py)
against its own scalar one-env statement over random small models, `row_thresholds`, the parser of the `.pomdp` subset
(Tiger written out in tests/pomdp_oracle.py, every accepted form, every refusal with its line), the ctypes struct and
the exports, and `heaven_hell_pomdp` against the grid Heaven-Hell rules without sampling: for every state and action of
two mazes at three slip probabilities, the row of T is the distribution got by enumerating
`heavenhell_oracle.scalar_step` over the unslipped move and the three slips. No GPU is touched."""
import ctypes
import types

import numpy as np
import pytest

import heavenhell_oracle as hh
from pomdp_oracle import TIGER, TOP, PomdpOracle, Spec, random_model, scalar_step


def lowered(model, time_limit):
    from gym_po_amd import row_thresholds
    T, Z, R, start, terminal, reset_obs = model
    return Spec(row_thresholds(T), row_thresholds(Z), row_thresholds(start), row_thresholds(reset_obs), R, terminal,
                time_limit)


# ------------------------------------------------------------------ the oracle ----
@pytest.mark.parametrize("S,A,O", [(2, 3, 2), (5, 2, 3), (7, 3, 6), (1, 1, 1)])
def test_vectorised_oracle_equals_the_scalar_statement(S, A, O):
    tl = 5
    sp = lowered(random_model(S, A, O, seed=S * 100 + O, n_terminal=1 if S > 1 else 0), tl)
    s, act, el = (x.ravel() for x in np.meshgrid(np.arange(S), np.arange(-A, A), np.array([0, tl - 2, tl - 1]),
                                                 indexing="ij"))
    rng = np.random.default_rng(1)
    # per (state, action, elapsed): random words, and each word at both ends of its range and at a threshold's two sides
    edge = [0, 1, 2, 0xFFFFFFFE, 0xFFFFFFFF]
    V = 24
    s, act, el = (np.repeat(x, V) for x in (s, act, el))
    B = s.size
    words = rng.integers(0, 1 << 32, (4, B), dtype=np.uint64)
    words[:, ::6] = np.array(edge, dtype=np.uint64)[rng.integers(0, len(edge), (4, words[:, ::6].shape[1]))]
    thr = sp.trans_thr[s, np.where(act < 0, act + A, act)]  # y0 at an entry of the row, and one below it
    pick = thr[np.arange(B), rng.integers(0, S, B)]
    at = np.arange(B) % 6 == 1
    words[0, at] = (np.clip(pick[at] - (np.arange(B)[at] // 6 % 2), 0, TOP - 1) * 2 + 1).astype(np.uint64)
    ora = PomdpOracle(B, sp)
    ora.state[:], ora.elapsed[:] = s, el
    o, r, d, tr = ora.step(act, ora.draws_of_words(*words))
    assert r.dtype == np.float32 and o.dtype == np.int32
    for b in range(B):
        x = [int(w) for w in words[:, b]]
        want = scalar_step(sp, int(s[b]), int(el[b]), int(act[b]), *x)
        got = (int(ora.state[b]), int(ora.elapsed[b]), int(o[b]), r[b], bool(d[b]), bool(tr[b]))
        assert got == want, (b, s[b], el[b], act[b], x, got, want)
    assert tr.any() and not tr.all() and (d.any() and not d.all() if S > 1 else not d.any())
    assert set(np.unique(ora.state)) <= set(range(S)) and o.min() >= 0 and o.max() < O
    if S > 1:
        assert len(np.unique(o)) == O
    if S > 2:  # (with two states, one of them terminal, an episode that goes on is in state 0)
        assert len(np.unique(ora.state[~(d | tr)])) > 1


def test_oracle_reset_is_the_scalar_reset():
    sp = lowered(random_model(5, 2, 3, seed=3), 4)
    B = 600
    words = np.random.default_rng(0).integers(0, 1 << 32, (4, B), dtype=np.uint64)
    ora = PomdpOracle(B, sp)
    o = ora.reset(ora.draws_of_words(*words))
    sp1 = lowered(random_model(5, 2, 3, seed=3), 1)  # time_limit 1: every step truncates
    for b in range(B):
        # a step that truncates resets from the same two words
        got = scalar_step(sp1, 0, 0, 0, *[int(w) for w in words[:, b]])
        assert (got[0], got[1], got[2]) == (int(ora.state[b]), 0, int(o[b]))
    assert not sp.terminal[ora.state].any()  # terminal states have start probability 0


# ------------------------------------------------------------------ row_thresholds ----
def test_row_thresholds_is_controller_thresholds_rule():
    from gym_po_amd import controller_thresholds, row_thresholds
    assert row_thresholds([0.85, 0.15, 0]).tolist() == [1825361100, TOP, TOP]
    assert row_thresholds([0.0, 0.0, 1.0, 0.0]).tolist() == [0, 0, TOP, TOP]
    assert row_thresholds([1.0]).tolist() == [TOP] and row_thresholds([0.5, 0.5]).tolist() == [1 << 30, TOP]
    rng = np.random.default_rng(0)
    M, n_obs, A = 3, 7, 5
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.4)
    p[..., 0, 0] += 0.01
    p /= p.sum((-1, -2), keepdims=True)
    t = row_thresholds(p.reshape(M, n_obs, A * M))
    assert t.dtype == np.uint32 and t.shape == (M, n_obs, A * M)
    assert np.array_equal(t, controller_thresholds(p))
    assert (np.diff(t.astype(np.int64), axis=-1) >= 0).all() and (t[..., -1] == TOP).all()
    zero_tail = p.reshape(M, n_obs, -1)[..., -1] == 0
    assert zero_tail.any() and (t[..., -2][zero_tail] == TOP).all()
    assert row_thresholds(np.full((2, 3, 4, 5), 0.2)).shape == (2, 3, 4, 5)


def test_row_thresholds_refusals_name_the_row():
    from gym_po_amd import row_thresholds
    p = np.full((3, 2, 4), 0.25)
    p[2, 1] = [0.5, -0.25, 0.5, 0.25]
    with pytest.raises(ValueError, match=r"row \(2, 1\) has negative"):
        row_thresholds(p)
    p[2, 1] = [0.5, np.nan, 0.25, 0.25]
    with pytest.raises(ValueError, match=r"row \(2, 1\) has negative \(or NaN\)"):
        row_thresholds(p)
    p[2, 1] = 0.25
    p[1, 0, 3] += 2e-6
    with pytest.raises(ValueError, match=r"row \(1, 0\) sums to"):
        row_thresholds(p)
    p[1, 0, 3] = 0.25 + 5e-7  # within the tolerance
    assert row_thresholds(p)[1, 0, -1] == TOP
    with pytest.raises(ValueError, match=r"row \(\) sums to 0"):
        row_thresholds([0.0, 0.0])
    with pytest.raises(ValueError, match="at least one entry"):
        row_thresholds(np.zeros((3, 0)))


# ------------------------------------------------------------------ the parser ----
def tiger_tables():
    T = np.zeros((2, 3, 2))
    T[:, 0] = np.eye(2)
    T[:, 1:] = 0.5
    Z = np.full((3, 2, 2), 0.5)
    Z[0] = [[0.85, 0.15], [0.15, 0.85]]
    R = np.zeros((2, 3, 2))
    R[:, 0] = -1
    R[0, 1], R[1, 1], R[0, 2], R[1, 2] = -100, 10, 10, -100
    return T, Z, R


def test_parser_tiger():
    from gym_po_amd import parse_pomdp
    m = parse_pomdp(TIGER)
    T, Z, R = tiger_tables()
    assert (m["S"], m["A"], m["O"]) == (2, 3, 2) and m["discount"] == 0.95
    assert m["states"] == ["tiger-left", "tiger-right"] and m["actions"] == ["listen", "open-left", "open-right"]
    assert m["observations"] == ["hear-left", "hear-right"]
    assert np.array_equal(m["T"], T) and np.array_equal(m["Z"], Z) and np.array_equal(m["R"], R)
    assert np.array_equal(m["start"], [0.5, 0.5])
    # the same model in the other forms: counts for names, one-line entries, rows, indices, the vector start
    other = """discount: 0.95
values: reward
states: 2
actions: 3
observations: 2
start: 0.5 0.5
T: 0 : 0 : 0 1.0
T: 0 : 1 : 1 1.0
T: 1 : *
0.5 0.5
T: 2 : 0
uniform
T: 2 : 1 uniform
O: 0 : 0
0.85 0.15
O: 0 : 1 : 0 0.15
O: 0 : 1 : 1 0.85
O: 1 : * : * 0.5
O: 2
0.5 0.5
0.5 0.5
R: * : * : * : * -1
R: 1 : 0 : * : * -100   # a comment
R: 1 : 1 : * : * 10
R: 2 : 0 : * : * 10
R: 2 : 1 : * : * -100
R: 1 : * : * : * 0
R: 1 : 0 : * : * -100
R: 1 : 1 : * : * 10
"""
    m2 = parse_pomdp(other)
    assert m2["states"] is None and m2["actions"] is None
    for k in ("T", "Z", "R", "start"):
        assert np.array_equal(m2[k], m[k]), k
    # a start vector on the next line, a full T matrix, later lines overriding earlier ones
    m3 = parse_pomdp("states: a b c\nactions: 1\nobservations: x y\nstart:\n0.2 0.3\n0.5\nT: 0\n0 1 0\n0 0 1\n1 0 0\n"
                     "T: 0 : c : a 0.5\nT: 0 : c : c 0.5\nO: *\nuniform\nR: 0 : a : b : * 2.5\n")
    assert m3["start"].tolist() == [0.2, 0.3, 0.5] and m3["discount"] is None
    assert m3["T"][:, 0].tolist() == [[0, 1, 0], [0, 0, 1], [0.5, 0, 0.5]]
    assert (m3["Z"] == 0.5).all() and m3["R"][0, 0, 1] == 2.5 and m3["R"].sum() == 2.5
    # no start line: uniform
    assert parse_pomdp("states: 4\nactions: 1\nobservations: 1\nT: 0\nidentity\nO: 0\nuniform\n")["start"].tolist() \
        == [0.25] * 4


HEAD = "discount: 0.9\nvalues: reward\nstates: a b\nactions: go stay\nobservations: x y\n"  # 5 lines


@pytest.mark.parametrize("text,line,what", [
    ("discount: 0.9\nvalues: cost\n", 2, "only 'reward'"),
    (HEAD + "E: go\n", 6, "unknown directive"),
    (HEAD + "T: go : c : a 1.0\n", 6, "unknown state 'c'"),
    (HEAD + "T: fly : a : a 1.0\n", 6, "unknown action 'fly'"),
    (HEAD + "O: go : a : z 1.0\n", 6, "unknown observation 'z'"),
    (HEAD + "T: go : 2 : a 1.0\n", 6, r"state index 2 outside \[0, 2\)"),
    (HEAD + "T: go : a : a : a 1.0\n", 6, "at most three fields"),
    (HEAD + "T: go : a : a one\n", 6, "expected a number"),
    (HEAD + "T: go : a : a nan\n", 6, "finite"),
    (HEAD + "T: go : a\n0.5 0.25 0.25\n", 7, "expected 2 numbers, got 3"),
    (HEAD + "T: go : a\n0.5\nT: stay\nidentity\n", 7, "expected 2 numbers"),
    (HEAD + "T: go\n1 0\n0 uniform\n", 8, "must stand alone"),
    (HEAD + "O: go\nidentity\n", 7, "expected 4 numbers"),
    (HEAD + "R: go : a : a : x 1.0\n", 6, "observation field must be"),
    (HEAD + "R: go : a\n1 2\n", 6, "only the one-line form"),
    (HEAD + "start: a\n", 6, "expected 2 numbers"),
    (HEAD + "start include: a\n", 6, "not accepted"),
    (HEAD + "start: 0.5 0.5\nstates: 3\n", 7, "must come before"),
    ("states: 2\nT: 0 : 0 : 0 1.0\n", 2, "'actions:' must come before"),
    ("states: a a\n", 1, "occurs twice"),
    ("states: 0\n", 1, "positive count"),
    (HEAD + "just words\n", 6, "expected a directive"),
    ("states: 2\nactions: 2\n", 2, "no 'observations:' line"),
    (HEAD, 5, "no T: / O: / R: line"),
])
def test_parser_refusals_name_the_line(text, line, what):
    from gym_po_amd import parse_pomdp
    with pytest.raises(ValueError, match=rf"^line {line}: .*{what}"):
        parse_pomdp(text)


# ------------------------------------------------------------------ the struct ----
def test_struct_layout_and_exports():
    import gym_po_amd
    from gym_po_amd import _lib
    assert _lib.GP_KIND_POMDP == 8
    c = _lib.PomdpConfig
    offs = {name: getattr(c, name).offset for name, _ in c._fields_}
    assert offs == dict(n_states=0, n_actions=4, n_obs=8, time_limit=12, trans_thr=16, obs_thr=24, start_thr=32,
                        reset_obs_thr=40, reward=48, terminal=56)
    assert ctypes.sizeof(c) == 64 and ctypes.alignment(c) == 8
    for name in ("TabularPOMDPEnv", "heaven_hell_pomdp", "row_thresholds", "parse_pomdp"):
        assert name in gym_po_amd.__all__ and hasattr(gym_po_amd, name)
    lib = _lib.lib()
    assert lib.gp_abi_version() == 1
    assert lib.gp_debug_set(b"pomdp_lds_max", 1024) == 0
    lib.gp_debug_reset()


def test_constructor_refusals_name_the_argument():
    """Raised before anything touches the GPU."""
    from gym_po_amd import TabularPOMDPEnv
    T, Z, R = tiger_tables()
    for kw, match in [
        (dict(T=T[:, :, :1]), "T must be"), (dict(Z=Z[:2]), "Z must be"), (dict(R=R[:1]), "R must be"),
        (dict(start=[1.0]), "start must be"), (dict(terminal=[0, 0, 1]), "terminal must be"),
        (dict(reset_obs=np.ones((2, 3)) / 3), "reset_obs must be"), (dict(time_limit=0), "time_limit"),
        (dict(time_limit=65536), "time_limit"), (dict(T=T * 0.5), r"T: row \(0, 0\) sums to"),
        (dict(Z=-Z), r"Z: row \(0, 0\) has negative"), (dict(start=[0.5, 0.6]), r"start: row \(\) sums"),
        (dict(reset_obs=[[1, 0], [0.5, 0.4]]), r"reset_obs: row \(1,\) sums"),
    ]:
        args = dict(T=T, Z=Z, R=R)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            TabularPOMDPEnv(4, **args)


# ------------------------------------------------------------------ Heaven-Hell as tables ----
def hh_stand_in(maze, obs_type, p, rewards):
    """What `heaven_hell_pomdp` reads of a HeavenHellGridEnv, without a GPU."""
    from gym_po_amd.envs.heaven_hell_grid import FLAG_START, hansen_codes, keep_threshold, parse_maze
    H, W, flags = parse_maze(maze)
    cell_obs = obs_type == "cell_signal"
    return types.SimpleNamespace(
        maze=tuple(maze), map_size=(H, W), flags=flags, obs_type=obs_type,
        obs_base=np.arange(H * W, dtype=np.int32) if cell_obs else hansen_codes(H, W, flags),
        obs_base_n=H * W if cell_obs else 16, action_failure_probability=float(p), keep_thr=keep_threshold(p),
        start_cells=np.flatnonzero(flags & FLAG_START).astype(np.int32), time_limit=500, rewards=dict(rewards))


REWARDS = dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=-0.25, wall_reward=-0.5)
SLIP_WORDS = (0, 0x55555556, 0xAAAAAAAB)  # x1 of the slips to a + 1, a + 2, a + 3


@pytest.mark.parametrize("p", [0.0, 1 / 3, 1.0], ids=["p0", "p1_3", "p1"])
@pytest.mark.parametrize("obs_type", ["cell_signal", "hansen_signal"])
@pytest.mark.parametrize("maze", ["t3", "default"])
def test_heaven_hell_pomdp_is_the_enumerated_grid_rule(maze, obs_type, p):
    from gym_po_amd import heaven_hell_maze, heaven_hell_pomdp
    maze = hh.T3 if maze == "t3" else heaven_hell_maze()
    env = hh_stand_in(maze, obs_type, p, REWARDS)
    T, Z, R, start, terminal, reset_obs = heaven_hell_pomdp(env)
    sp = hh.Spec.of_env(env)
    # the same maze with the two areas as plain free cells: where a move lands, from the same scalar statement
    plain = hh.Spec([r.replace("L", ".").replace("R", ".") for r in maze], obs_type, sp.keep_thr, 500, **REWARDS)
    n = sp.H * sp.W
    S = 2 * n
    assert T.shape == (S, 4, S) and Z.shape == (4, S, sp.n_obs) and R.shape == (S, 4, S) and R.dtype == np.float32
    assert start.shape == (S,) and terminal.shape == (S,) and reset_obs.shape == (S, sp.n_obs)
    # the draws of the block that exist at this p: (x0, x1, weight x 3)
    cases = []
    if sp.keep_thr > 0:
        cases.append((1, 0, 3.0 * (1.0 - p)))  # y = 0: not slipped
    if sp.keep_thr < TOP:
        cases += [(0xFFFFFFFF, x1, p) for x1 in SLIP_WORDS]  # y = 2^31 - 1: slipped, to each of the three others
    assert len(cases) == {0.0: 1, 1.0: 3}.get(p, 4)
    seen_rewards = set()
    for cell in sp.free_cells:
        for side in range(2):
            s = side * n + cell
            want_obs = hh.scalar_obs(sp, cell, side)
            assert reset_obs[s].sum() == 1.0 and reset_obs[s, want_obs] == 1.0
            assert all(Z[a, s].sum() == 1.0 and Z[a, s, want_obs] == 1.0 for a in range(4))
            assert bool(terminal[s]) == bool(sp.flags[cell] & (hh.LEFT | hh.RIGHT))
            for a in range(4):
                keep, slip = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
                for x0, x1, w in cases:
                    landed = hh.scalar_step(plain, cell, side, 0, a, x0, x1, 0, 0)
                    _, _, _, _, rew, term, trunc = hh.scalar_step(sp, cell, side, 0, a, x0, x1, 0, 0)
                    s1 = landed[1] * n + landed[0]
                    assert landed[1] == side and not landed[5] and not trunc
                    (keep if x0 == 1 else slip)[s1] += 1
                    assert R[s, a, s1] == rew and bool(terminal[s1]) == term, (cell, side, a, s1)
                    seen_rewards.add(float(rew))
                # the weights are (1 - p) and p / 3: compared as the same float64 expression of the integer counts,
                # and x 3 against the integers' weights
                assert np.array_equal(T[s, a], keep * (1.0 - p) + slip * (p / 3.0)), (cell, side, a)
                assert np.allclose(3.0 * T[s, a], 3.0 * (1.0 - p) * keep + p * slip, rtol=0, atol=4e-15)
                assert abs(T[s, a].sum() - 1.0) < 1e-15 and (T[s, a][(keep + slip) == 0] == 0).all()
    assert seen_rewards == {1.0, -1.0, -0.25, -0.5}
    walls = [c for c in range(n) if not sp.flags[c] & hh.FREE]
    for c in walls:  # states no episode reaches: self-loops
        for s in (c, n + c):
            assert (T[s, :, s] == 1.0).all() and not terminal[s] and start[s] == 0
    want_start = np.zeros(S)
    for c in sp.starts:
        want_start[[c, n + c]] = 1.0 / (2 * len(sp.starts))
    assert np.array_equal(start, want_start)
    # the lowered tables are valid rows
    from gym_po_amd import row_thresholds
    for x in (T, Z, start, reset_obs):
        t = row_thresholds(x)
        assert (t[..., -1] == TOP).all()
    if p == 0.0:
        assert set(np.unique(row_thresholds(T))) == {0, TOP}
