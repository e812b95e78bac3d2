"""CPU twins of the planted-draw GPU tests (tests/test_crooms_plant_gpu.py, tests/test_taxi_plant_gpu.py): numpy
alone, no GPU.

A planted GPU case proves something only if numpy really takes the rare branch from that exact state. For every
case of tests/plant_cases.py this file asserts so on numpy's own Generator:
* Lemire: the planted half is below the rejection threshold, `Generator.choice` / `integers` consumes one
  half-word more from the planted state than from a twin state whose half is accepted, the rejection is at the
  case's half-word index, and the resulting state (has_uint32 / uinteger included) is the one the restated
  buffered draws (oracle/pcg64.py) predict;
* restart: `Generator.multinomial` consumes exactly one word more than the rows' ordinary count (one double per
  drawn category), and exactly the ordinary count for the one plant numpy does not restart on (the last drawn
  category: its conditional p is 1);
* search: stream_plant's fixed-point search returns an offset, and the targeted draw lands on the planted word.
Tolerance: none.
"""
import numpy as np
import pytest

import plant_cases as pc
import stream_plant as sp
from oracle.pcg64 import PCG64, lemire_threshold, pcg_output
from oracle.taxi import TaxiOracle


# ------------------------------------------------------------------------------------------ the helper ----
def test_planted_word_and_half_are_drawn_by_numpy():
    for pos, word in ((0, sp.WORD_ALL_ONES), (7, sp.WORD_TOP53), (300, 0x0123456789ABCDEF)):
        gen = sp.generator_at(sp.plant_word(pc.INC, pos, word, seed=pos))
        raw = gen.bit_generator.random_raw(pos + 1)
        assert int(raw[pos]) == word
    for h, buffered in ((0, False), (1, False), (5, True), (6, True), (0, True)):
        gen = sp.generator_at(sp.plant_half(pc.INC, h, 0xDEADBEEF, seed=h, buffered=buffered, words_before=3))
        gen.bit_generator.random_raw(3)
        g = PCG64.from_numpy(gen.bit_generator)
        halves = [g.next32() for _ in range(h + 1)]
        assert halves[h] == 0xDEADBEEF


def test_words_between_and_retreat():
    gen = np.random.default_rng(3)
    s0 = gen.bit_generator.state
    gen.random(1234)
    s1 = gen.bit_generator.state
    assert sp.words_between(s0, s1, 1000, 2000) == 1234
    assert sp.retreat(s1["state"]["state"], s1["state"]["inc"], 1234) == s0["state"]["state"]
    gen.integers(0, 10, 3)  # three 32-bit draws: two words, the high half of the second one kept
    assert sp.halves_between(s1, gen.bit_generator.state) == 3
    with pytest.raises(AssertionError):
        sp.words_between(s0, s1, 0, 1000)


@pytest.mark.parametrize("n", [3, 6, 104, 1000, 12345])
def test_rejected_word_is_below_the_threshold(n):
    r = sp.rejected_word(n, 0 if lemire_threshold(n) == 1 else 1)
    assert (r * n) & 0xFFFFFFFF < lemire_threshold(n)
    assert sp.is_rejected(r, n) and not sp.is_rejected(r + 1, n)


def test_state_with_output_half():
    for half in (0, 1):
        s = sp.state_with_output_half(0xCAFEF00D, half, seed=half)
        assert (pcg_output(s) >> (32 * half)) & 0xFFFFFFFF == 0xCAFEF00D


# --------------------------------------------------------------------------------------------- C-ROOMS ----
@pytest.mark.parametrize("case", pc.crooms_cases(), ids=pc.crooms_id)
def test_crooms_plant_is_a_lemire_rejection_in_numpy(case):
    path, place, n, h, buffered, call, calls = case
    for twin in (False, True):
        c = pc.crooms_build(case, accepted_twin=twin)
        assert c.st["has_uint32"] == int(buffered)
        st0 = c.ora.gen.bit_generator.state
        _, draws = pc.crooms_oracle_planted(c)  # (asserts: no normals, the case's choice calls)
        site, k, before = draws.choice_calls[call]
        assert k == n
        # the call starts where the case says: B words into the step, and n halves after the first call
        assert sp.halves_between(st0, before) == 2 * c.words_before + (n if call == 1 else 0)
        gen = sp.generator_at(before)
        idx = gen.choice(c.nv, n)
        after = gen.bit_generator.state
        vals, rej, st_after = sp.lemire_trace(before, c.nv, n)
        assert rej == ([] if twin else [h])
        assert sp.halves_between(before, after) == n + (0 if twin else 1)
        np.testing.assert_array_equal(idx, vals)
        assert sp.rng6(after) == sp.rng6(st_after)  # has_uint32 / uinteger as the buffered draws leave them
        fresh = n + (0 if twin else 1) - int(before["has_uint32"])
        assert after["has_uint32"] == fresh % 2
    assert sp.is_rejected(c.value, c.nv) and (c.value * c.nv) & 0xFFFFFFFF < lemire_threshold(c.nv)


# ------------------------------------------------------------------------- Taxi: passenger / destination ----
@pytest.mark.parametrize("mapname,L,ns,nvalid,thr", [("six", 6, 630, 450, 4), ("three", 3, 108, 54, 1)])
def test_taxi_maps_are_what_the_cases_assume(mapname, L, ns, nvalid, thr):
    o = TaxiOracle(2, map=pc.TAXI_MAPS[mapname])
    assert (o.nlocs, o.ns, len(o.valid_states), lemire_threshold(o.nlocs)) == (L, ns, nvalid, thr)
    assert o.nlocs & (o.nlocs - 1) != 0


@pytest.mark.parametrize("case", pc.taxi_pd_cases(), ids=pc.taxi_pd_id)
def test_taxi_pd_plant_is_a_lemire_rejection_in_numpy(case):
    path, mapname, b1, where, mode = case
    c = pc.taxi_pd_build(case)
    t = pc.taxi_pd_build(case, accepted_twin=True)
    L = c.ora.nlocs
    assert sp.is_rejected(c.value, L)
    p, d, rej, rounds, st_end = c.walk
    assert rej == [c.h]
    assert {"buf": c.h == 0 and c.st["has_uint32"] == 1, "p": c.h < b1, "d": b1 <= c.h < 2 * b1,
            "redraw": len(rounds) > 0 and 2 * b1 <= c.h < 2 * b1 + rounds[0]}[where]
    assert not (where != "buf" and c.h == 0 and c.st["has_uint32"])
    # numpy itself, through the oracle's _reset_passenger_and_destination, from the planted state and from the twin
    ends = []
    for x in (c, t):
        for k in range(x.actions.shape[0]):
            s_before = x.ora.gen.bit_generator.state
            _, _, done, trunc = x.ora.step_seeded(x.actions[k])
            assert not done.any() and not trunc.any()
            if k != x.planted_step:
                assert x.ora.gen.bit_generator.state == s_before  # (a step without completions draws nothing)
            else:
                s_planted = (s_before, x.ora.gen.bit_generator.state)
        ends.append(s_planted)
    assert sp.rng6(ends[0][1]) == sp.rng6(st_end)
    r_, c_, p_now, d_now = c.ora.decode(c.ora.s[c.who])
    np.testing.assert_array_equal(p_now, p)
    np.testing.assert_array_equal(d_now, d)
    assert (p != d).all()
    tw = pc._pd_walk(t.st, L, b1)
    assert tw[2] == [] and sp.rng6(ends[1][1]) == sp.rng6(tw[4])
    n_c = 2 * b1 + sum(rounds)
    assert sp.halves_between(*ends[0]) == n_c + 1
    # (the twin's state differs in the planted half alone, but that moves every word before it too: its collisions
    # are its own, and so is its count; what it shows is that without the rejection no half-word is drawn twice)
    assert sp.halves_between(*ends[1]) == 2 * b1 + sum(tw[3])


# ------------------------------------------------------------------------------- Taxi: inversion restart ----
@pytest.mark.parametrize("case", pc.taxi_row_cases(), ids=pc.taxi_row_id)
def test_taxi_row_plant_restarts_the_inversion_in_numpy(case):
    path, place, row, what = case
    c = pc.taxi_row_build(case)
    info, ora = c.info, c.ora
    p, ns = ora.state_distribution, ora.ns
    # the search's answer: the rows before the plant consume d - cat_rank words, and the planted draw is the word
    gen = sp.generator_at(info["state"])
    if row:
        gen.multinomial(ns, p, row)
    assert sp.words_between(info["state"], gen.bit_generator.state, info["d"] - info["cat_rank"],
                            info["d"] - info["cat_rank"] + 1) == info["d"] - info["cat_rank"]
    raw = sp.generator_at(gen.bit_generator.state).bit_generator.random_raw(info["cat_rank"] + 1)
    assert int(raw[-1]) == sp.WORD_ALL_ONES
    # the planted row alone: one word more than its ordinary count (none more for the last drawn category)
    s_row = gen.bit_generator.state
    counts = gen.multinomial(ns, p, 1)[0]
    ordinary = sp.ordinary_row_words(counts, p)
    used = sp.words_between(s_row, gen.bit_generator.state, 0, ordinary + 3)
    assert used == ordinary + (1 if c.restarts else 0)
    assert info["extra"] == (1 if c.restarts else 0) and info["row_words"][row] == used
    assert info["cat_rank"] < ordinary  # the planted category was drawn
    # the whole call, as the env makes it
    gen = sp.generator_at(info["state"])
    all_counts = gen.multinomial(ns, p, c.B)
    total = sum(sp.ordinary_row_words(r, p) for r in all_counts)
    assert sp.words_between(info["state"], gen.bit_generator.state, total, total + 3) == total + info["extra"]
    rounds = sp.speculative_rounds(info["row_words"], c.c0)
    if what == "def0":
        assert info["row_words"][0] == c.c0 and rounds[0][2][1] == 0 and rounds[0][1] == 2
    if what == "defpos":
        assert rounds[0][2][1] > 0
    if what == "lastof":
        assert rounds[0][:2] == (0, 64) and row == 63
    if what == "firstof":
        assert rounds[0][:2] == (0, 64) and rounds[1][0] == 64 == row
    if row == 0 and c.restarts:
        assert rounds[0][:2] == (0, 1)  # deficit 0 before it, -1 after: the round ends on the restarted row
