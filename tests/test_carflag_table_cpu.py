"""The Car-Flag one-step tables (tests/golden/carflag_table_*.npz, recorded from the reference by
tests/golden/make_golden_carflag.py): every count the generator accepted them on is derived again from the committed
files, and the NumPy restatement (tests/carflag_oracle.py) is pinned to every row bit for bit, with the recorded draws
and from the recorded PCG64 state."""
import os

import numpy as np
import pytest

import make_golden_carflag as gen
from carflag_oracle import (F32, TABLE_NAMES, NumpyDraws, ReplayDraws, bits_equal, load_index, load_table, rng_state,
                            table_oracle)

FLAG_CLASSES = ("term_plus", "term_minus", "trunc_only", "term_and_trunc", "dir_plus", "dir_minus", "dir_cleared",
                "speed_clipped", "position_clipped")


def test_index_lists_every_table():
    _, idx = load_index()
    assert set(idx["tables"]) == set(TABLE_NAMES) == set(gen.TABLES)


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_size_and_coverage_from_the_file(name):
    here, _ = load_index()
    meta, d = load_table(name)
    assert os.path.getsize(os.path.join(here, meta["file"])) <= gen.MAX_TABLE_BYTES
    assert len(d["term"]) == meta["rows"] <= gen.MAX_TABLE_ROWS and meta["time_limit"] == gen.TABLE_TL
    cov = gen.table_coverage(meta, d)
    assert cov == meta["coverage"]
    for k in FLAG_CLASSES:
        assert cov[k] > 0, k
    # every row group holds every elapsed value: not truncated, one short of the limit, truncated
    for g in np.unique(d["group"]):
        el = set(d["elapsed0"][d["group"] == g])
        assert el == set(gen.ELAPSED) or g in (gen.G_CANCEL, gen.G_TABLE32, gen.G_EDGE), (g, el)
    assert set(d["elapsed0"]) == set(gen.ELAPSED)
    assert np.array_equal(d["trunc"], d["elapsed0"] + 1 >= meta["time_limit"])
    assert (d["s0"][:, 2] != 0).sum() > meta["rows"] // 4  # a non-zero old direction
    if meta["action_dtype"] != "int64":
        a = d["act"]
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any() and cov["nan_rows"] > 0
        tiny = np.finfo(a.dtype).smallest_subnormal
        assert (a == tiny).any() and (a == -tiny).any() and (np.abs(a[np.isfinite(a)]) > 1e30).any()
        assert (np.signbit(a) & (a == 0)).any()
    else:
        n = meta["num_actions"]
        assert set(d["act"]) == set(range(-n, n))
        if n == 4:
            assert cov["table_f32_rows"] >= 16


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_both_sides_of_every_landing_constant(name):
    """x' = x at the float32 below, at and above +-{0.2, 0.3, 0.5, 0.7, 1, 1.03, 1.1}: terminated and direction."""
    meta, d = load_table(name)
    pat = gen.landing_pattern(meta, d)
    assert pat == meta["landing"]
    n = meta.get("num_actions")
    if n is None or n % 2:
        assert pat == gen.LANDING_WANT
    else:
        assert all(v == [[], []] for v in pat.values())  # no zero force: nothing lands
    xs = d["s0"][d["group"] == gen.G_LANDING, 0]
    for x in gen.landing_positions():
        assert (xs.view(np.uint32) == np.array(x).view(np.uint32)).sum() >= 12  # 4 heaven x priest, 3 elapsed


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_wrong_variants_of_the_rules_are_told_apart(name):
    meta, d = load_table(name)
    assert not gen.rows_differing(meta, d).any()  # the rules themselves reproduce every row
    for k, kw in gen.VARIANTS.items():
        c = int(gen.rows_differing(meta, d, **kw).sum())
        want = gen.variant_requirement(meta, k)
        assert c == meta["coverage"]["variants"][k]
        assert want is None or (c == 0 if want == 0 else c >= want), (k, c, want)


def test_f32_and_f64_tables_split_on_the_same_inputs():
    (_, a), (_, b) = load_table("carflag_table_f32"), load_table("carflag_table_f64")
    ma, mb = a["group"] == gen.G_SPLIT, b["group"] == gen.G_SPLIT
    for k in ("s0", "heavens0", "priests0", "elapsed0"):
        assert np.array_equal(a[k][ma], b[k][mb]), k
    assert not a["act"][ma].any() and not b["act"][mb].any()
    stay = ~(a["term"][ma] | a["trunc"][ma] | b["term"][mb] | b["trunc"][mb])
    n_term = int((a["term"][ma] != b["term"][mb]).sum())
    n_dir = int((stay & (a["final_s"][ma, 2] != b["final_s"][mb, 2])).sum())
    assert n_term >= 2 and n_dir >= 2
    assert load_index()[1]["path_split"] == {"term": n_term, "direction": n_dir}
    # the two rows named in the issue
    for x, v, want in ((0.9375, F32(0.0625 - 2.0 ** -28), "term"), (0.6875, F32(0.0125), "dir")):
        m = (a["s0"][ma, 0] == F32(x)) & (a["s0"][ma, 1] == v) & (a["priests0"][ma] == 0.5) & (a["elapsed0"][ma] == 0)
        assert m.sum() == 2
        if want == "term":
            assert a["term"][ma][m].all() and not b["term"][mb][m].any()
        else:
            assert (a["final_s"][ma][m, 2] != 0).all() and not b["final_s"][mb][m, 2].any()


def _check(ora, out, d, what):
    o, r, tm, tr = out
    for got, key in ((o, "obs"), (r, "rew"), (tm, "term"), (tr, "trunc"), (ora.s, "final_s"),
                     (ora.elapsed, "final_elapsed"), (ora.heavens, "final_heavens"), (ora.priests, "final_priests")):
        bad = np.argwhere(~bits_equal(got, d[key]))
        assert len(bad) == 0, f"{what} {key}: {len(bad)} elements differ, first at {bad[0].tolist()}"
    assert np.isnan(d["final_s"]).sum() > 0 or d["act"].dtype == np.int64


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_oracle_replays_every_row(name):
    meta, d = load_table(name)
    dr = ReplayDraws()
    dr.set(d["k53"], d["hidx"], d["pidx"])
    ora = table_oracle(meta, d, dr)
    _check(ora, ora.step(d["act"]), d, "replay")
    done = d["term"] | d["trunc"]
    assert ora.episodes == done.sum() and ora.length_sum == (d["elapsed0"] + 1)[done].sum()


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_oracle_from_the_recorded_stream(name):
    meta, d = load_table(name)
    g = np.random.Generator(np.random.PCG64())
    g.bit_generator.state = rng_state(meta["rng_before"])
    ora = table_oracle(meta, d, NumpyDraws(g))
    _check(ora, ora.step(d["act"]), d, "numpy")
    k, h, p = ora.draws.last
    done = d["term"] | d["trunc"]
    for got, key in ((k, "k53"), (h, "hidx"), (p, "pidx")):
        assert np.array_equal(got, d[key][done]), key
    assert g.bit_generator.state == rng_state(meta["rng_after"])
