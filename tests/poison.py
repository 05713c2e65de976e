"""Poisoned, guarded allocations for the GPU suite (imported by the test modules, as philox_ref / ddim_ref are).

Every wrapper of the package allocates what it hands to the library through ``ops.empty`` / ``ops.empty_like``.  While
``install()`` is active those two return a view into a larger base tensor:

    [ 64 KiB guard | the tensor, padded to a multiple of 256 bytes | 64 KiB guard ]

and the whole base is filled with a recognisable pattern first -- float32 bits 0x7FE5A5A5, float64 bits 0x7FFE5A5A5A5A5A5A
(quiet NaNs with a payload no kernel produces), byte 0xA5 for every other dtype.  An element a kernel does not write stays NaN
and fails ``_close`` / ``torch.equal`` by itself; a store that lands outside the tensor changes a guard, which ``check()``
compares bit for bit.  64 KiB is one 128 x 128 fp32 plane and a multiple of every alignment the kernels select forms by, so
the view is aligned as a fresh torch allocation is.

    unwritten(t)   elements of a float tensor that still carry the pattern
    check()        synchronise, assert every guard of every allocation since the last check is intact (naming shape and call
                   site), release the bases
    install(mp)    patch ops.empty / ops.empty_like through a pytest.MonkeyPatch; undone by mp.undo()

Bases of more than 256 MiB in total trigger a ``check()`` from inside the next allocation, so long loops do not accumulate.  That
check keeps the most recent allocations listed (``KEEP_RECENT``: more than one wrapper call makes), so a tensor allocated just
before the bound was crossed -- and not yet written -- is guard-checked again after its kernel ran.
"""
import traceback

import pytest
import torch

GUARD_BYTES = 64 * 1024
ALIGN = 256
LIMIT_BYTES = 256 << 20
KEEP_RECENT = 8

F32_BITS = 0x7FE5A5A5
F64_BITS = 0x7FFE5A5A5A5A5A5A
BYTE = 0xA5

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(bits: int, width: int) -> int:
    return bits - (1 << width) if bits >> (width - 1) else bits


def _pattern(dtype):
    """(integer dtype of the element's size, the element's pattern as a value of that dtype)"""
    if dtype == torch.float32:
        return torch.int32, _signed(F32_BITS, 32)
    if dtype == torch.float64:
        return torch.int64, _signed(F64_BITS, 64)
    size = torch.empty(0, dtype=dtype).element_size()
    bits = int.from_bytes(bytes([BYTE]) * size, "little")
    return _INT_VIEW[size], (bits if size == 1 else _signed(bits, 8 * size))


class _Alloc:
    __slots__ = ("base", "lo", "hi", "shape", "dtype", "site")


_live = []                  # allocations since the last check()
_live_bytes = 0
_state = {"devices": ("cuda",), "real_empty": None}


def _call_site() -> str:
    """the innermost frames outside this file: the wrapper that allocated and its caller"""
    frames = [f for f in traceback.extract_stack()[:-1] if f.filename != __file__]
    return " <- ".join(f"{f.filename.rsplit('/', 1)[-1]}:{f.lineno} {f.name}" for f in reversed(frames[-2:]))


def _alloc(shape, dtype, device):
    global _live_bytes
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    esize = torch.empty(0, dtype=dtype).element_size()
    body = -(-(numel * esize) // ALIGN) * ALIGN
    total = GUARD_BYTES + body + GUARD_BYTES
    if _live_bytes + total > LIMIT_BYTES and _live:
        check(keep=KEEP_RECENT)
    base = torch.full((total,), BYTE, dtype=torch.uint8, device=device)
    if dtype in (torch.float32, torch.float64):
        idt, val = _pattern(dtype)
        base.view(idt).fill_(val)
    a = _Alloc()
    a.base, a.lo, a.hi = base, GUARD_BYTES, GUARD_BYTES + numel * esize
    a.shape, a.dtype, a.site = shape, dtype, _call_site()
    _live.append(a)
    _live_bytes += total
    return base[a.lo:a.hi].view(dtype).view(shape)


def _wants(device, pin_memory) -> bool:
    return not pin_memory and torch.device(device if device is not None else "cpu").type in _state["devices"]


def _empty(shape, *, dtype, device, pin_memory=False):
    if not _wants(device, pin_memory):
        return _state["real_empty"](shape, dtype=dtype, device=device, pin_memory=pin_memory)
    return _alloc(shape, dtype, device)


def _empty_like(t):
    if not _wants(t.device, False) or not t.is_contiguous():
        return torch.empty_like(t)
    return _alloc(tuple(t.shape), t.dtype, t.device)


def unwritten(t: torch.Tensor) -> int:
    """How many elements of the float tensor ``t`` still carry the allocation pattern."""
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"unwritten() counts float elements; got {t.dtype} (an integer pattern is a legal value)")
    idt, val = _pattern(t.dtype)
    if t.is_cuda:
        torch.cuda.synchronize(t.device)
    return int((t.contiguous().view(idt) == val).sum().item())


def base_of(t: torch.Tensor):
    """(the uint8 base a live view was carved from, the view's first byte in it, the byte behind its last element)"""
    a = next(a for a in _live if a.base.data_ptr() + a.lo == t.data_ptr())
    return a.base, a.lo, a.hi


def check(keep: int = 0) -> None:
    """Every guard band of every allocation since the last check still holds the pattern, bit for bit; then the bases go
    (but for the ``keep`` most recent, which stay listed for the next check)."""
    global _live_bytes
    live, _live[:] = list(_live), (_live[-keep:] if keep else [])
    _live_bytes = sum(a.base.numel() for a in _live)
    if any(a.base.is_cuda for a in live):
        torch.cuda.synchronize()
    bad = []
    for a in live:
        # the base carries one pattern from byte 0 and both bands start on an element boundary; the padding behind the last
        # element belongs to the upper band, so a store one element past the view lands in it
        idt, val = _pattern(a.dtype)
        esize = torch.empty(0, dtype=idt).element_size()
        for name, band in (("below", a.base[:a.lo]), ("above", a.base[a.hi:a.hi + (a.base.numel() - a.hi) // esize * esize])):
            hit = band.view(idt) != val
            if bool(hit.any()):
                where = hit.nonzero().flatten()
                off = int(where[0].item()) if name == "above" else int(where[-1].item()) - hit.numel()
                bad.append(f"{a.dtype} {a.shape} allocated at {a.site}: {int(hit.sum())} guard elements {name} the tensor "
                           f"changed, the nearest {off:+d} elements from its {'end' if name == 'above' else 'start'}")
    assert not bad, "a kernel wrote outside its output:\n  " + "\n  ".join(bad)


def install(mp: "pytest.MonkeyPatch", devices=("cuda",)) -> None:
    """Patch ops.empty / ops.empty_like for tensors on ``devices`` (device types); ``mp.undo()`` restores them."""
    from synt_isic_amd import ops
    _state["devices"] = tuple(devices)
    if ops.empty is not _empty:
        _state["real_empty"] = ops.empty
    mp.setattr(ops, "empty", _empty)
    mp.setattr(ops, "empty_like", _empty_like)


def discard() -> None:
    """Forget the live allocations without checking them (when the patch is removed)."""
    global _live_bytes
    _live[:] = []
    _live_bytes = 0


@pytest.fixture(scope="module", autouse=True)
def poison_allocations():
    """Module scope: module-scoped fixtures (a stage-1 result, a classifier, a sampler) allocate under the patch as well."""
    mp = pytest.MonkeyPatch()
    install(mp)
    try:
        yield
    finally:
        mp.undo()
        discard()


@pytest.fixture(autouse=True)
def guard_bands(poison_allocations):
    yield
    check()
