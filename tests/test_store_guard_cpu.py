"""The positive control of tests/store_guard.py, on CPU tensors: `check` fails for a byte written just before the view,
just after it, one plane after it, for an element left unwritten, and for expected values that contain the poison
pattern; `guarded` delivers every requested data_ptr() % 16; `shift_cases` covers every shift of every buffer."""
import numpy as np
import pytest

import store_guard as sg

K, B = 3, 37


def _torch():
    import torch
    return torch


def _filled(dtype, shift, tail=()):
    torch = _torch()
    shape = (K, B) + tail
    plane = B * int(np.prod(tail, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    view, raw, lo = sg.guarded(torch, dtype, shape, shift, "cpu", plane)
    n = int(np.prod(shape))
    want = (torch.arange(n, dtype=torch.int64) % 7 + 1).to(dtype).view(shape)
    view.copy_(want)
    return view, raw, lo, want, plane


DTYPES = [("int32", 4), ("float32", 12), ("uint8", 3), ("float64", 8)]


@pytest.mark.parametrize("dtype,shift", DTYPES)
def test_check_passes_on_an_exact_store(dtype, shift):
    view, raw, lo, want, _ = _filled(getattr(_torch(), dtype), shift)
    sg.check(view, raw, lo, want)
    sg.check(view, raw, lo, want.numpy())
    sg.check_input(view, raw, lo, want)


@pytest.mark.parametrize("dtype,shift", DTYPES)
def test_one_byte_just_before_the_view(dtype, shift):
    view, raw, lo, want, _ = _filled(getattr(_torch(), dtype), shift)
    raw[lo - 1] = 0
    with pytest.raises(AssertionError, match="before the view"):
        sg.check(view, raw, lo, want)
    with pytest.raises(AssertionError, match="outside the input view"):
        sg.check_input(view, raw, lo, want)


@pytest.mark.parametrize("dtype,shift", DTYPES)
def test_one_byte_just_after_the_view(dtype, shift):
    view, raw, lo, want, _ = _filled(getattr(_torch(), dtype), shift)
    raw[lo + view.numel() * view.element_size()] = 0
    with pytest.raises(AssertionError, match="after the view"):
        sg.check(view, raw, lo, want)


@pytest.mark.parametrize("dtype,shift", DTYPES)
def test_one_byte_a_plane_after_the_view(dtype, shift):
    """A store at plane index K (and -1) lands inside the guard, not past it."""
    view, raw, lo, want, plane = _filled(getattr(_torch(), dtype), shift)
    end = lo + view.numel() * view.element_size()
    assert end + plane < raw.numel() and lo - plane - 1 >= 0
    raw[end + plane] = 0
    with pytest.raises(AssertionError, match="after the view"):
        sg.check(view, raw, lo, want)
    raw[end + plane] = sg.GUARD
    raw[lo - plane - 1] = 0
    with pytest.raises(AssertionError, match="before the view"):
        sg.check(view, raw, lo, want)


@pytest.mark.parametrize("dtype,shift", DTYPES)
def test_one_element_left_unwritten(dtype, shift):
    torch = _torch()
    dt = getattr(torch, dtype)
    view, raw, lo = sg.guarded(torch, dt, (K, B), shift, "cpu", B * 8)
    want = (torch.arange(K * B, dtype=torch.int64) % 7 + 1).to(dt).view(K, B)
    flat, wflat = view.view(-1), want.view(-1)
    flat[:50] = wflat[:50]
    flat[51:] = wflat[51:]  # element 50 keeps the poison
    with pytest.raises(AssertionError, match="left unwritten"):
        sg.check(view, raw, lo, want)


@pytest.mark.parametrize("dtype", ["int32", "float32", "uint8", "float64", "int64"])
def test_expected_values_with_the_poison_pattern_are_refused(dtype):
    """An element of the reference that equals the poison would hide a missed store: the case fails as vacuous, even
    though the view (still all poison there) equals the reference."""
    torch = _torch()
    dt = getattr(torch, dtype)
    view, raw, lo = sg.guarded(torch, dt, (K, B), 0, "cpu", B * 8)
    want = torch.ones((K, B), dtype=dt)
    view.copy_(want)
    w = want.clone()
    w.view(-1).view(torch.uint8)[5 * w.element_size():6 * w.element_size()] = sg.POISON
    view.view(-1).view(torch.uint8)[5 * w.element_size():6 * w.element_size()] = sg.POISON
    with pytest.raises(AssertionError, match="vacuous"):
        sg.check(view, raw, lo, w)


def test_check_input_sees_a_written_input():
    view, raw, lo, want, _ = _filled(_torch().int32, 4)
    view[1, 2] += 1
    with pytest.raises(AssertionError, match="input buffer was written"):
        sg.check_input(view, raw, lo, want)


def test_check_untouched():
    torch = _torch()
    view, raw, lo = sg.guarded(torch, torch.float32, (K, B), 8, "cpu", B * 4)
    sg.check_untouched(view, raw, lo)
    view[0, 0] = 1.0
    with pytest.raises(AssertionError, match="into the view"):
        sg.check_untouched(view, raw, lo)


def test_guarded_delivers_every_alignment():
    torch = _torch()
    for dtype, size in ((torch.uint8, 1), (torch.int32, 4), (torch.float32, 4), (torch.float64, 8), (torch.int64, 8)):
        for shift in range(0, 16, size):
            for shape in ((K, B), (K, B, 9), (B,), (1,)):
                plane = int(np.prod(shape[1:] if len(shape) > 1 else shape)) * size
                view, raw, lo = sg.guarded(torch, dtype, shape, shift, "cpu", plane)
                assert view.data_ptr() % 16 == shift and view.is_contiguous() and tuple(view.shape) == shape
                nbytes = view.numel() * size
                g = max(256, plane + 64)
                assert lo >= g and raw.numel() - lo - nbytes >= g
                r = raw.numpy()
                assert (r[:lo] == sg.GUARD).all() and (r[lo + nbytes:] == sg.GUARD).all()
                assert (r[lo:lo + nbytes] == sg.POISON).all()
    with pytest.raises(AssertionError):
        sg.guarded(torch, torch.int32, (4,), 2, "cpu", 16)


def test_shift_cases():
    kinds = (4, 4, 4, 1, 1)
    cases = sg.shift_cases(kinds)
    assert len(cases) == 3 * 3 + 2 * 5 + 3 and len(set(cases)) == len(cases)
    for i, k in enumerate(kinds):
        alone = {c[i] for c in cases if sum(x != 0 for x in c) == 1 and c[i]}
        assert alone == set(sg.SHIFTS[k])
    for c in cases[-3:]:
        assert all(c) and all(sh in sg.SHIFTS[k] for sh, k in zip(c, kinds))
    assert sg.shift_cases((8,))[0] == (8,)
