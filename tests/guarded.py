"""Guarded buffers for the GPU tests (a helper module, not a test file).

Every output of the Python layer comes from torch.empty, so it lies in the caching allocator between other live tensors, often on memory
that held the same result a moment ago: a store one element past an output, or an output row that is never written, changes no value a
test reads back.  Here a tensor is a view INSIDE a larger flat allocation that is filled, interior included, with a canary bit pattern:

    [ band >= 4 KiB | lead elements | the view | band >= 4 KiB ]

arena(shape, dtype, device, lead) makes such a view; check(view) asserts -- on integer views of the bits, a NaN never equals itself --
that everything in front of and behind the view still holds the canary, and returns how many elements of the view still hold it (an
output that was written completely returns 0).  guarded_outputs(lead) replaces torch.empty for the duration of a `with` block, so
that every output generalized_rbda_amd/__init__.py allocates comes from arena(), and hands back the list of them.  place(a, ...) puts an
input into an arena: Tensor.contiguous() of a contiguous view is the view itself, so the library reads through the interior pointer.

lead shifts the view by a number of ELEMENTS: lead = 0 keeps the allocator's alignment (the band is a whole number of 4 KiB), lead = 1
gives a pointer aligned to the element size only.  include/grbda_hip.h states no alignment requirement, so both must work.

What the input bands detect: they are quiet NaNs, so a kernel that reads rows >= B of q, qd, tau / ydd, f_ext or force AND LETS THEM
REACH A LIVE RESULT produces a non-finite output.  An over-read that stays in dead lanes (a ragged tile computing on whatever it
loaded, results masked at the store) is not detected and is not a defect.  What no band can see: the library's own work slabs."""
import contextlib
import math

import torch

BAND_BYTES = 4096
# float types: quiet NaNs (exponent all ones, top mantissa bit set) with a payload to recognise; int32: a fixed odd constant
CANARY = {torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF85A5AC0DE5A5A, torch.int32: 0x5A5A5A5B}
_BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32}
_SIZE = {torch.float32: 4, torch.float64: 8, torch.int32: 4}


def arena(shape, dtype, device, lead=0):
    """A contiguous view of `shape` inside a flat allocation filled with CANARY[dtype], a band in front (plus `lead` elements) and behind."""
    shape = tuple(int(n) for n in shape)
    n = math.prod(shape)
    band = BAND_BYTES // _SIZE[dtype]
    flat = torch.full((band + lead + n + band,), CANARY[dtype], dtype=_BITS[dtype], device=device)
    view = flat.view(dtype)[band + lead: band + lead + n].view(shape)
    assert view.is_contiguous() and view._base is not None and view._base.data_ptr() == flat.data_ptr()
    return view


def place(array, dtype, device, lead=0):
    """`array` (numpy or tensor) copied into an arena of its shape"""
    src = torch.as_tensor(array)
    view = arena(src.shape, dtype, device, lead)
    view.copy_(src.to(dtype))
    return view


def bits(view):
    """(flat integer tensor of the whole allocation, start of the view in it, elements of the view)"""
    base = view._base
    assert base is not None and base.dim() == 1 and base.storage_offset() == 0 and view.is_contiguous(), "not a view made by arena()"
    return base.view(_BITS[view.dtype]), view.storage_offset(), view.numel()


def check(view):
    """Asserts that both bands around `view` hold the canary; returns the number of interior elements that still hold it."""
    flat, start, n = bits(view)
    canary = CANARY[view.dtype]
    for name, part, origin in (("front", flat[:start], -start), ("back", flat[start + n:], n)):
        bad = torch.nonzero(part != canary).flatten()
        if bad.numel():
            first, last = int(bad[0]) + origin, int(bad[-1]) + origin
            raise AssertionError(f"{name} band of a {view.dtype} {tuple(view.shape)} arena overwritten: {bad.numel()} elements, "
                                 f"offsets {first} .. {last} relative to the view's first element ({n} elements)")
    return int((flat[start:start + n] == canary).sum())


def snapshot(view):
    """a copy of the whole allocation's bits (bands included), for same_bits() after a call"""
    return bits(view)[0].clone()


def same_bits(view, before, lo=None, hi=None):
    """the allocation equals `before` bit for bit; with lo / hi, outside the interior elements [lo, hi) of the view only"""
    flat, start, n = bits(view)
    if lo is None:
        return bool(torch.equal(flat, before))
    return bool(torch.equal(flat[:start + lo], before[:start + lo]) and torch.equal(flat[start + hi:], before[start + hi:]))


@contextlib.contextmanager
def guarded_outputs(lead=0):
    """While active, torch.empty(shape, dtype=float32 | float64 | int32, device=...) returns an arena; yields the list of arenas made."""
    made = []
    real = torch.empty

    def empty(*size, dtype=None, device=None, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        if dtype not in CANARY or kw:
            return real(*size, dtype=dtype, device=device, **kw)
        made.append(arena(shape, dtype, device, lead))
        return made[-1]

    torch.empty = empty
    try:
        yield made
    finally:
        torch.empty = real
