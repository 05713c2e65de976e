"""tests/poison.py fails when it should: the helper on CPU tensors (the device filter widened to "cpu" for these tests)."""
import pytest
import torch

import poison
from synt_isic_amd import ops


@pytest.fixture
def patched():
    mp = pytest.MonkeyPatch()
    poison.install(mp, devices=("cpu",))
    try:
        yield
    finally:
        mp.undo()
        poison.discard()


@pytest.mark.parametrize("dtype,bits", [(torch.float32, 0x7FE5A5A5), (torch.float64, 0x7FFE5A5A5A5A5A5A)])
def test_fresh_tensor_is_all_pattern_and_one_missing_element_is_counted(patched, dtype, bits):
    t = ops.empty((3, 5, 7), dtype=dtype, device="cpu")
    assert t.shape == (3, 5, 7) and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 64 == 0
    assert torch.isnan(t).all() and poison.unwritten(t) == t.numel()
    idt = torch.int32 if dtype == torch.float32 else torch.int64
    assert int(t.view(idt)[0, 0, 0]) & ((1 << (8 * t.element_size())) - 1) == bits
    t.copy_(torch.arange(t.numel(), dtype=dtype).reshape(t.shape))
    assert poison.unwritten(t) == 0
    u = ops.empty_like(t)
    assert u.shape == t.shape and u.dtype == t.dtype and poison.unwritten(u) == u.numel()
    u.view(-1)[:-1] = 0.5
    assert poison.unwritten(u) == 1
    u.view(-1)[-1] = float("nan")                     # a NaN the kernel computed is not the pattern
    assert poison.unwritten(u) == 0
    poison.check()


@pytest.mark.parametrize("where", ["before", "after"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint8, torch.int32])
def test_a_store_one_element_outside_the_view_fails_check(patched, dtype, where):
    t = ops.empty((2, 3, 11), dtype=dtype, device="cpu")           # 66 elements: the view does not end on a 256-byte boundary
    base, lo, hi = poison.base_of(t)
    flat = base.view(dtype)
    e = t.element_size()
    idx = lo // e - 1 if where == "before" else hi // e
    flat[idx] = 1
    with pytest.raises(AssertionError, match=r"\(2, 3, 11\).*test_poison_cpu.py.*(below|above)"):
        poison.check()
    assert not poison._live                                          # released, reported once
    poison.check()


def test_far_ends_of_the_guard_bands_are_compared_too(patched):
    t = ops.empty(100, dtype=torch.float32, device="cpu")
    base, lo, hi = poison.base_of(t)
    assert lo == poison.GUARD_BYTES and base.numel() - hi >= poison.GUARD_BYTES
    base[0] ^= 1                                                     # one bit, 64 KiB below the tensor
    with pytest.raises(AssertionError, match="below"):
        poison.check()
    t = ops.empty(100, dtype=torch.float32, device="cpu")
    base, lo, hi = poison.base_of(t)
    base[-1] ^= 1
    with pytest.raises(AssertionError, match="above"):
        poison.check()


def test_writes_inside_the_view_leave_the_guards_alone(patched):
    ts = [ops.empty(n, dtype=torch.float32, device="cpu") for n in (1, 63, 64, 65, 16384)]
    for t in ts:
        t.zero_()
    poison.check()


def test_integer_patterns(patched):
    for dtype, want in ((torch.uint8, 0xA5), (torch.int32, 0xA5A5A5A5 - (1 << 32)), (torch.int64, 0xA5A5A5A5A5A5A5A5 - (1 << 64))):
        t = ops.empty((4, 9), dtype=dtype, device="cpu")
        assert t.dtype == dtype and bool((t == want).all())
    with pytest.raises(TypeError):
        poison.unwritten(t)
    poison.check()


def test_pinned_and_other_devices_pass_through(patched):
    poison._state["devices"] = ("cuda",)                             # the suite's filter: CPU tensors are torch's own
    try:
        t = ops.empty((4, 4), dtype=torch.float32, device="cpu")
        assert not poison._live and t.shape == (4, 4)
        like = ops.empty_like(t)
        assert not poison._live and like.shape == t.shape
    finally:
        poison._state["devices"] = ("cpu",)
    # a pinned request goes to the allocation point the patch replaced, with its arguments (pinning itself needs the runtime)
    seen = []
    real = poison._state["real_empty"]
    poison._state["real_empty"] = lambda shape, **kw: seen.append((shape, kw)) or real(shape, **dict(kw, pin_memory=False))
    try:
        p = ops.empty(8, dtype=torch.float32, device="cpu", pin_memory=True)
    finally:
        poison._state["real_empty"] = real
    assert seen == [(8, dict(dtype=torch.float32, device="cpu", pin_memory=True))] and not poison._live and p.shape == (8,)
    assert not torch.isnan(p).any() or poison.unwritten(p) == 0


def test_memory_bound_checks_and_releases(patched, monkeypatch):
    monkeypatch.setattr(poison, "LIMIT_BYTES", 3 * (2 * poison.GUARD_BYTES + 256))
    monkeypatch.setattr(poison, "KEEP_RECENT", 1)
    first = [ops.empty(8, dtype=torch.float32, device="cpu") for _ in range(3)]
    assert len(poison._live) == 3
    ops.empty(8, dtype=torch.float32, device="cpu")                  # the fourth would exceed the bound: check() ran first ...
    assert len(poison._live) == 2                                    # ... and kept the most recent allocation listed
    base, lo, hi = poison.base_of(first[2])                          # (allocated before the bound was crossed, written after it)
    base.view(torch.float32)[hi // 4] = 0.0
    with pytest.raises(AssertionError, match="above"):
        poison.check()
    base, lo, hi = poison.base_of(ops.empty(8, dtype=torch.float32, device="cpu"))
    base[lo - 1] = 0
    monkeypatch.setattr(poison, "LIMIT_BYTES", 0)
    with pytest.raises(AssertionError, match="below"):               # ... and that check is a real one
        ops.empty(8, dtype=torch.float32, device="cpu")


def test_patch_is_undone_on_exit():
    real_empty, real_like = ops.empty, ops.empty_like
    mp = pytest.MonkeyPatch()
    poison.install(mp, devices=("cpu",))
    assert ops.empty is not real_empty and ops.empty_like is not real_like
    mp.undo()
    poison.discard()
    assert ops.empty is real_empty and ops.empty_like is real_like
    t = ops.empty(16, dtype=torch.float32, device="cpu")
    assert not poison._live and t.shape == (16,)


def test_default_helpers_are_torchs():
    t = ops.empty((2, 3), dtype=torch.float64, device="cpu")
    assert t.shape == (2, 3) and t.dtype == torch.float64 and t.device.type == "cpu"
    assert ops.empty_like(t).shape == (2, 3) and ops.empty(5, dtype=torch.uint8, device="cpu").shape == (5,)
