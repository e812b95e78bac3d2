"""Planting chosen words in numpy's PCG64 stream (tests only; a plain module, shared by the CPU and GPU tests).

numpy's PCG64 steps its 128-bit LCG state and then outputs XSL-RR of the new state, so "the state whose output is
x" is the state *after* the draw that returns x. A plant is built backwards: pick such a state `s_star`, then step
the LCG back over the `d` words the generator consumes before that draw (`state_before`). What is planted:

* a whole 64-bit word (`state_with_output_word`): Generator.random's double, e.g. 2^64 - 1 for the inversion
  restart of random_binomial_inversion (U above the binomial CDF at its search bound);
* one 32-bit half (`state_with_output_half`): a buffered Lemire draw (`rejected_word(n)`: a half whose product with
  n has a low word below the rejection threshold of range n).

Where the number of words before the target draw depends on the draws themselves (row r > 0 of a multinomial
call), `find_offset` searches for a self-consistent distance.
"""
import numpy as np

from oracle.pcg64 import MASK128, PCG64, PCG_MULT, lemire_threshold, pcg_advance_params, pcg_output

MASK64 = (1 << 64) - 1
WORD_ALL_ONES = MASK64                 # the double (2^53 - 1) * 2^-53
WORD_TOP53 = ((1 << 53) - 1) << 11     # the same double, low 11 bits clear


def rotl64(x, r):
    return ((x << r) | (x >> ((64 - r) & 63))) & MASK64


def state_with_output_word(x, seed):
    """A PCG64 state whose output is the 64-bit word x; the state's high half (which fixes the rotation) comes
    from `seed`."""
    hi = int(np.random.default_rng(seed).integers(0, 2 ** 63)) * 2 + 1
    lo = hi ^ rotl64(x, hi >> 58)
    s = (hi << 64) | lo
    assert pcg_output(s) == x
    return s


def state_with_output_half(half_value, half, seed):
    """A PCG64 state whose output has the given low (half = 0) or high (half = 1) 32 bits; the other half and the
    state's high half come from `seed`."""
    rng = np.random.default_rng(seed)
    hi = int(rng.integers(0, 2 ** 63)) * 2 + 1
    other = int(rng.integers(0, 2 ** 32))
    x = (other << 32) | half_value if half == 0 else (half_value << 32) | other
    lo = hi ^ rotl64(x, hi >> 58)
    s = (hi << 64) | lo
    assert pcg_output(s) == x
    return s


def retreat(state, inc, d):
    """The state d LCG steps before `state`."""
    a, c = pcg_advance_params((1 << 128) - d, inc)
    return (a * state + c) & MASK128


def state_before(s_star, inc, d):
    """The state from which d words are drawn before the word that `s_star` outputs."""
    return retreat(s_star, inc, d + 1)


def np_state(state, inc, has_uint32=0, uinteger=0):
    return {"bit_generator": "PCG64", "state": {"state": state, "inc": inc}, "has_uint32": has_uint32,
            "uinteger": uinteger}


def generator_at(st):
    gen = np.random.Generator(np.random.PCG64())
    gen.bit_generator.state = st
    return gen


def rng6(st):
    s, inc = st["state"]["state"], st["state"]["inc"]
    return [s >> 64, s & MASK64, inc >> 64, inc & MASK64, int(st["has_uint32"]), int(st["uinteger"])]


def plant_word(inc, pos, word, seed=0):
    """The numpy PCG64 state dict from which draw `pos` (0-based) of the next 64-bit draws comes from the word
    `word`: the state with that output, stepped back pos + 1 draws."""
    return np_state(state_before(state_with_output_word(word, seed), inc, pos), inc)


def rejected_word(n, k=1):
    """A 32-bit value that buffered_bounded_lemire_uint32 rejects for range n (the k-th multiple of 2^32 / n on,
    rounded up: the low word of its product with n is the remainder, below the threshold for some of them). k = 0
    gives the value 0, rejected for every n that rejects anything (the only rejected value when the threshold is
    1, e.g. n = 3)."""
    thr = lemire_threshold(n)
    if k == 0:
        assert thr > 0, f"range {n} rejects nothing"
        return 0
    for kk in range(k, k + 10000):
        r = -(-(kk << 32) // n)
        if r < (1 << 32) and (r * n) & 0xFFFFFFFF < thr:
            return r
    raise AssertionError(f"no rejected word for range {n}")


def is_rejected(half, n):
    return (half * n) & 0xFFFFFFFF < lemire_threshold(n)


def plant_half(inc, h, value, seed=0, buffered=False, words_before=0):
    """The state dict from which half-word `h` of the next buffered 32-bit draws is `value`, after `words_before`
    64-bit words drawn first. Without a buffered half, half h is the low (h even) or high (h odd) half of fresh
    word h // 2. With one (`buffered`, has_uint32 = 1), half 0 is the buffer itself (uinteger = value, and the state
    comes from `seed` alone) and half h > 0 is half h - 1 of the fresh words; the buffer then holds a half that
    range-n draws of any n <= 2^16 accept."""
    if buffered and h == 0:
        s = state_with_output_word(0x0123456789ABCDEF, seed)
        return np_state(s, inc, 1, value)
    j = h - 1 if buffered else h
    s_star = state_with_output_half(value, j & 1, seed)
    s0 = state_before(s_star, inc, words_before + (j >> 1))
    return np_state(s0, inc, 1, 0x9E3779B9) if buffered else np_state(s0, inc)


def words_between(state0, state1, lo=0, hi=1 << 16):
    """The number of 64-bit words between two PCG64 state dicts of one stream (the same increment): PCG64.advance
    to the first candidate `lo`, then one LCG step per further candidate below `hi`; AssertionError when it is none
    of them."""
    inc = state0["state"]["inc"]
    assert inc == state1["state"]["inc"]
    bg = np.random.PCG64()
    bg.state = state0
    bg.advance(lo)
    s, target = bg.state["state"]["state"], state1["state"]["state"]
    for d in range(lo, hi):
        if s == target:
            return d
        s = (s * PCG_MULT + inc) & MASK128
    raise AssertionError(f"states are not {lo}..{hi - 1} words apart")


def halves_between(state0, state1, lo=0, hi=1 << 16):
    """32-bit draws between two state dicts: two per word, corrected by the buffered halves at either end."""
    return 2 * words_between(state0, state1, lo, hi) + int(state0["has_uint32"]) - int(state1["has_uint32"])


def find_offset(s_star, inc, words_before_target, candidates):
    """Fixed-point search for a plant behind a data-dependent number of words. For every candidate distance d the
    generator is started d words before the planted draw (`state_before(s_star, inc, d)`) and handed to
    `words_before_target(gen, d)`, which makes the draws that precede the target's own call and returns how many
    words that call consumes before it reaches the target (or None when this start cannot reach the target). d is
    accepted when the generator really is d words on at that point. Returns (d, start state dict, words inside the
    target's call); AssertionError when no candidate fits."""
    for d in candidates:
        st0 = np_state(state_before(s_star, inc, d), inc)
        gen = generator_at(st0)
        extra = words_before_target(gen, d)
        if extra is None or extra < 0 or extra > d:
            continue
        if gen.bit_generator.state["state"]["state"] == retreat(s_star, inc, extra + 1):
            return d, st0, extra
    raise AssertionError("no self-consistent offset among the candidates")


# ---- buffered Lemire draws (Generator.integers / choice with a 32-bit range) ----
def lemire_trace(st, n, count):
    """`count` draws of range n from the state dict `st`, restated on oracle.pcg64.PCG64: (values, indices of the
    rejected half-words among the 32-bit draws of this call, the state dict afterwards)."""
    g = PCG64(st["state"]["state"], st["state"]["inc"], int(st["has_uint32"]), int(st["uinteger"]))
    thr = lemire_threshold(n)
    vals, rej, k = [], [], 0
    for _ in range(count):
        while True:
            m = g.next32() * n
            k += 1
            if (m & 0xFFFFFFFF) >= thr:
                break
            rej.append(k - 1)
        vals.append(m >> 32)
    return np.array(vals, dtype=np.int64), rej, g.to_numpy_state()


# ---- multinomial rows (Taxi's reset: multinomial(ns, p, b).argmax(-1)) ----
def ordinary_row_words(counts, p):
    """Doubles an ordinary row draws: random_multinomial draws one binomial (by inversion here: one double unless it
    restarts) for every category but the last that has p > 0, while balls remain."""
    counts = np.asarray(counts)
    n = int(counts.sum())
    before = np.concatenate(([0], np.cumsum(counts)[:-1]))
    return int(((np.asarray(p)[:-1] > 0) & (before[:-1] < n)).sum())


def plant_multinomial_word(ns, p, row, inc, cat_rank=None, seed=0, word=WORD_ALL_ONES, accept=None, tries=200):
    """A start state from which `Generator.multinomial(ns, p, rows)` draws the double of one category of row `row`
    from `word`. Row 0 takes the `cat_rank`-th category with p > 0 directly. A later row sits behind the words of
    the rows before it, which depend on the draws: `find_offset` starts the generator about row * C0 words back
    and lets the rows run; with `cat_rank` given it accepts a start from which they consume exactly the distance
    less cat_rank, with cat_rank None the category is whichever the rows end on (kept within the first half of the
    categories, where many balls remain and the inversion's search bound is far below them). `accept(info)`, if
    given, may refuse a plant (another seed is then tried). Returns a dict: state (the start state dict), d (words
    before the planted draw), cat_rank, row_words (doubles drawn by each of the rows 0 .. row from this state), extra
    (the words numpy drew beyond the rows' ordinary counts: 1 when the planted draw restarted its inversion; they
    are counted in the planted row's row_words), counts (numpy's rows)."""
    p = np.asarray(p)
    c0 = int((p[:-1] > 0).sum())
    for s in range(seed, seed + tries):
        s_star = state_with_output_word(word, s)
        if row == 0:
            d, st0, cat = cat_rank, np_state(state_before(s_star, inc, cat_rank), inc), cat_rank
        else:
            def before(gen, d):
                s0 = gen.bit_generator.state
                gen.multinomial(ns, p, row)
                if cat_rank is not None:
                    return cat_rank
                w = words_between(s0, gen.bit_generator.state, row * (c0 - 2), row * (c0 + 1) + 1)
                return d - w if d - w <= c0 // 2 else None

            centre = row * c0 - (row * 7) // 32 + (c0 // 4 if cat_rank is None else cat_rank)
            cands = [centre] + [centre + sg * i for i in range(1, 6) for sg in (1, -1)]
            try:
                d, st0, cat = find_offset(s_star, inc, before, cands)
            except AssertionError:
                continue
        gen = generator_at(st0)
        counts = gen.multinomial(ns, p, row + 1)
        words = [ordinary_row_words(c, p) for c in counts]
        total = words_between(st0, gen.bit_generator.state, sum(words), sum(words) + 4)
        extra = total - sum(words)
        words[row] += extra  # (the rows before the plant drew their ordinary counts: their sum is d - cat, below)
        info = dict(state=st0, d=d, cat_rank=cat, row_words=words, extra=extra, counts=counts, seed=s)
        if sum(words[:row]) + cat != d:
            continue  # (a restart of numpy's own before the plant: never seen, the distance would be off)
        if accept is None or accept(info):
            return info
    raise AssertionError("no plant found")


def speculative_rounds(row_words, c0, rows=64, deficits=16):
    """The rounds in which a chain of rows is resolved when `rows` rows are walked at `deficits` guessed offsets
    each (row i of a round at C0 i - deficit): a round chains rows while the deficit of the rows before stays within
    0 .. deficits - 1. Returns [(first row, rows chained, deficit before each chained row)]."""
    out, r0 = [], 0
    while r0 < len(row_words):
        D, n, ds = 0, 0, []
        while r0 + n < len(row_words) and n < rows and 0 <= D < deficits:
            ds.append(D)
            D += c0 - row_words[r0 + n]
            n += 1
        out.append((r0, n, ds))
        r0 += n
    return out
