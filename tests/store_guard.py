"""Helpers of tests/test_store_guard_gpu.py: caller buffers with guard bytes round them, at a chosen alignment.

Every device pointer the library writes through belongs to the caller, and PyTorch's caching allocator places it next to
other live tensors: a store a few bytes outside the documented shape faults nowhere and shows in no value comparison.
Here a buffer is a view into a larger `uint8` allocation:

    [ guard: 0xA5 ... ][ view: 0x5A ... ][ guard: 0xA5 ... ]
                        ^ data_ptr() % 16 == shift

Each guard is at least max(256, plane_bytes + 64) bytes, `plane_bytes` being the size of one [B, ...] plane of the
buffer, so a store at plane index K or -1 lands in a guard too. After the call `check` holds the guards to 0xA5 and the
view to the expected bits, and refuses an expected array that contains the poison pattern: with that, "equal to the
reference" implies "every element was stored". The helper is device-agnostic (tests/test_store_guard_cpu.py is its
positive control on CPU tensors).
"""
import numpy as np

GUARD = 0xA5
POISON = 0x5A
SHIFTS = {4: (4, 8, 12), 8: (8,), 1: (1, 2, 3, 4, 8)}  # by element size: the byte shifts that select other store widths
STATS = {"buffers": 0}


def _itemsize(torch, dtype):
    return torch.empty((), dtype=dtype).element_size()


def guard_bytes(plane_bytes):
    return max(256, int(plane_bytes) + 64)


def guarded(torch, dtype, shape, shift, device, plane_bytes):
    """(view, raw, lo): a contiguous `dtype` tensor of `shape` with data_ptr() % 16 == shift, cut at byte `lo` from the
    uint8 allocation `raw`; the view holds POISON, every other byte of raw GUARD."""
    shape = tuple(int(s) for s in shape)
    size = _itemsize(torch, dtype)
    assert 0 <= shift < 16 and shift % size == 0, f"a {dtype} buffer cannot sit {shift} bytes past a 16-B boundary"
    nbytes = int(np.prod(shape, dtype=np.int64)) * size
    g = guard_bytes(plane_bytes)
    raw = torch.full((g + 32 + nbytes + g,), GUARD, dtype=torch.uint8, device=device)
    lo = g + (shift - (raw.data_ptr() + g)) % 16
    raw[lo:lo + nbytes] = POISON
    view = raw[lo:lo + nbytes].view(dtype).view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == shift and view.data_ptr() == raw.data_ptr() + lo
    assert lo >= g and raw.numel() - (lo + nbytes) >= g
    return view, raw, lo


def _bytes(x):
    """The bytes of a tensor or array, as a flat numpy uint8 array (bool as its byte)."""
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    import torch
    x = x.detach().cpu().contiguous().reshape(-1)
    return (x.view(torch.uint8) if x.numel() else x.new_empty(0, dtype=torch.uint8)).numpy()


def guards_intact(view, raw, lo):
    nbytes = view.numel() * view.element_size()
    r = raw.detach().cpu().numpy()
    return bool((r[:lo] == GUARD).all()), bool((r[lo + nbytes:] == GUARD).all())


def has_poison(want_bytes, itemsize):
    """An element of the expected array carries the poison's bit pattern: a missed store there would not show. 8-byte
    elements are judged by their 4-byte halves (a 4-byte store into one is a store width too)."""
    w = min(itemsize, 4)
    el = want_bytes.reshape(-1, w)
    return bool((el == POISON).all(axis=1).any())


def check(view, raw, lo, want, name="buffer"):
    """The guards hold only GUARD, `view` equals `want` bit for bit, and no element of `want` is the poison pattern."""
    STATS["buffers"] += 1
    before, after = guards_intact(view, raw, lo)
    assert before, f"{name}: a byte before the view was written"
    assert after, f"{name}: a byte after the view was written"
    wb, gb = _bytes(want), _bytes(view)
    assert wb.size == gb.size, f"{name}: {gb.size} bytes against an expected {wb.size}"
    assert not has_poison(wb, view.element_size()), \
        f"{name}: the expected values contain the poison pattern: an unwritten element would not show (vacuous case)"
    if not np.array_equal(wb, gb):
        bad = np.flatnonzero(wb != gb)
        es = view.element_size()
        unwritten = bool((gb.reshape(-1, min(es, 4)) == POISON).all(axis=1).any())
        raise AssertionError(f"{name}: {bad.size} bytes differ from the reference, the first at byte {int(bad[0])} "
                             f"(element {int(bad[0]) // es}) of {gb.size}"
                             + ("; elements were left unwritten" if unwritten else ""))


def check_input(view, raw, lo, put, name="input"):
    """The guards are intact and the buffer still holds what was put in: no kernel writes its inputs."""
    STATS["buffers"] += 1
    before, after = guards_intact(view, raw, lo)
    assert before and after, f"{name}: a byte outside the input view was written"
    assert np.array_equal(_bytes(view), _bytes(put)), f"{name}: the input buffer was written"


def check_untouched(view, raw, lo, name="buffer"):
    """A refused call wrote nothing: the view still holds only POISON and the guards only GUARD."""
    STATS["buffers"] += 1
    before, after = guards_intact(view, raw, lo)
    assert before and after, f"{name}: a refused call wrote outside the view"
    assert bool((_bytes(view) == POISON).all()), f"{name}: a refused call wrote into the view"


def shift_cases(kinds):
    """Byte shifts of a tuple of buffers, by their element sizes `kinds` (4, 8 or 1): each buffer alone at each of its
    shifts (the others aligned), then three combinations with every buffer off its boundary."""
    cases = []
    for i, k in enumerate(kinds):
        for sh in SHIFTS[k]:
            c = [0] * len(kinds)
            c[i] = sh
            cases.append(tuple(c))
    return cases + together_cases(kinds)


def together_cases(kinds):
    """Three combinations in which every buffer is shifted, each buffer walking through its own shifts."""
    out = []
    for r in range(3):
        out.append(tuple(SHIFTS[k][(r + i) % len(SHIFTS[k])] for i, k in enumerate(kinds)))
    return out
