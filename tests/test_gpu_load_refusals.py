"""A refused sisic_unet_load / sisic_resnet_load leaves the handle as it was (include/sisic.h is the product boundary: the Python
wrappers never send a bad state dict, a C caller may).  Each load is called through ``_lib`` directly with a state dict of OTHER
values (twice the loaded ones) whose LAST entry is bad -- every earlier entry is one a load that validated as it went had
already taken by then -- and afterwards the handle must compute, read back and train as before.  The texts are the library's
own (csrc/tensor_dir.h, with the entry point's name in front); so are those of the read / write refusals below.

UNet: architecture D of tests/arch_ref.py (one block, the smallest the suite builds) at 1x3x32x32; classifier at 1x3x32x32."""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

import arch_ref
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _unet():
    from synt_isic_amd.unet import HipUNet2DModel
    from synt_isic_amd.weights import synthetic_unet_state_dict
    cfg = arch_ref.ARCHS["D"]
    sd = synthetic_unet_state_dict(cfg=cfg)
    m = HipUNet2DModel(**arch_ref.unet_kwargs(cfg))
    m.load_state_dict(sd)
    x = torch.randn((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)).to(DEV)
    return m.to(DEV).eval(), sd, lambda: m(x, torch.tensor([500])).sample.cpu()


def _classifier():
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    sd = synthetic_resnet18_state_dict()
    m = HipMelanomaClassifier(num_classes=7)
    m.load_state_dict(sd)
    x = torch.randn((1, 3, 32, 32), generator=torch.Generator().manual_seed(6)).to(DEV)
    return m.to(DEV).eval(), sd, lambda: m(x, preprocessed=True).cpu()


HANDLES = {"unet": (_unet, "unet", "tensors"), "resnet": (_classifier, "resnet", "float tensors")}


def _call(fn, handle, entries):
    """fn(handle, n, names, host_ptrs, numels) over entries of (name, tensor or None, element count): (return code, error text)"""
    from synt_isic_amd import _lib
    n = len(entries)
    names = (C.c_char_p * n)(*[None if k is None else k.encode() for k, _, _ in entries])
    ptrs = (C.c_void_p * n)(*[None if t is None else t.data_ptr() for _, t, _ in entries])
    numels = (C.c_int64 * n)(*[count for _, _, count in entries])
    rc = fn(handle, n, names, ptrs, numels)
    return rc, (_lib.load().sisic_last_error() or b"").decode()


def _bad_state_dicts(who, noun, good):
    """(case, entries, the library's text): `good` with its last entry made bad, or left out"""
    n = len(good)
    first, last = good[0], good[-1]
    return [("count", good[:-1], f"{who}_load: state dict has {n - 1} {noun}, expected {n}"),
            ("null entry", good[:-1] + [(last[0], None, last[2])], f"{who}_load: entry {n - 1} is null"),
            ("unexpected key", good[:-1] + [("not.a.key", last[1], last[2])], f"{who}_load: unexpected key 'not.a.key'"),
            ("duplicate key", good[:-1] + [first], f"{who}_load: duplicate key '{first[0]}'"),
            ("element count", good[:-1] + [(last[0], last[1], last[2] + 1)],
             f"{who}_load: '{last[0]}' has {last[2] + 1} elements, expected {last[2]}")]


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


@pytest.mark.parametrize("kind", list(HANDLES))
def test_a_refused_load_leaves_the_handle_as_it_was(kind):
    from synt_isic_amd import _lib
    build, who, noun = HANDLES[kind]
    model, sd, forward = build()
    lib, h = _lib.load(), model.handle
    load = getattr(lib, f"sisic_{who}_load")
    other = [(k, (sd[k].float() * 2).contiguous(), sd[k].numel()) for k in model._spec]     # held until the last call below
    loaded = OrderedDict((k, sd[k].float()) for k in model._spec)
    before = forward()
    for case, entries, text in _bad_state_dicts(who, noun, other):
        rc, said = _call(load, h, entries)
        assert (rc, said) == (_lib.SISIC_EINVAL, text), case
        assert torch.equal(forward(), before), case
        assert _same(model._read_all(0), loaded), case
    if kind == "resnet":                          # the same under a live optimizer, one step in: training goes on
        from synt_isic_amd.train import HipClassifierAdam
        opt = HipClassifierAdam(model, batchnorm="batch")
        x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(7)).to(DEV)
        model.loss_backward(x, [1, 4], preprocessed=True)
        opt.step()
        held = (model._read_all(0), model.grads(), {k: model.read_tensor(2, k) for k in model.trainable_names("batch")})
        for case, entries, text in _bad_state_dicts(who, noun, other):
            rc, said = _call(load, h, entries)
            assert (rc, said) == (_lib.SISIC_EINVAL, text), case
            assert opt.steps == 1 and model._trainer is opt, case
            now = (model._read_all(0), model.grads(), {k: model.read_tensor(2, k) for k in model.trainable_names("batch")})
            assert all(_same(a, b) for a, b in zip(now, held)), case
        model.loss_backward(x, [1, 4], preprocessed=True)
        assert opt.step() and opt.steps == 2
        opt.close()
        model.load_state_dict(sd)
        assert torch.equal(forward(), before)
    # the same arrays with a good last entry are taken: the refusals above were the last entry's doing
    rc, said = _call(load, h, other)
    assert rc == _lib.SISIC_OK, said
    assert _same(model._read_all(0), OrderedDict((k, t) for k, t, _ in other)) and not torch.equal(forward(), before)


@pytest.mark.parametrize("kind", list(HANDLES))
def test_read_and_write_refusals_keep_their_words(kind):
    from synt_isic_amd import _lib
    build, who, _ = HANDLES[kind]
    model, sd, forward = build()
    if kind == "unet":                            # sisic_unet_read / _write look at `what` once the arenas exist
        from synt_isic_amd.train import HipAdam
        opt = HipAdam(model, lr=1e-4)           # noqa: F841  (kept: it holds the arenas)
    lib, h = _lib.load(), model.handle
    read, write = getattr(lib, f"sisic_{who}_read"), getattr(lib, f"sisic_{who}_write")
    names = list(model._spec)
    name, numel = names[0], sd[names[0]].numel()
    buf = torch.zeros(numel + 1)
    ptr = C.cast(buf.data_ptr(), _lib.c_float_p)
    forms = "folded and packed forms" if kind == "resnet" else "packed forms"
    cases = [(read, (0, len(names), ptr, numel), f"{who}_read: bad arguments"),
             (read, (0, -1, ptr, numel), f"{who}_read: bad arguments"),
             (read, (0, 0, None, numel), f"{who}_read: bad arguments"),
             (read, (0, 0, ptr, numel + 1), f"{who}_read: '{name}' has {numel} elements"),
             (read, (9, 0, ptr, numel), f"{who}_read: what = 9 (0 parameter, 1 gradient, 2 Adam m, 3 Adam v)"),
             (write, (1, len(names), ptr, numel), f"{who}_write: bad arguments"),
             (write, (1, 0, None, numel), f"{who}_write: bad arguments"),
             (write, (1, 0, ptr, numel - 1), f"{who}_write: '{name}' has {numel} elements"),
             (write, (0, 0, ptr, numel), f"{who}_write: parameters are set by sisic_{who}_load (their {forms} must follow); "
                                         "what = 1 gradient, 2 Adam m, 3 Adam v"),
             (write, (9, 0, ptr, numel), f"{who}_write: what = 9 (1 gradient, 2 Adam m, 3 Adam v)")]
    before = forward()
    for fn, args, text in cases:
        assert fn(h, *args) == _lib.SISIC_EINVAL, text
        assert lib.sisic_last_error().decode() == text
    assert not buf.any() and torch.equal(forward(), before)
    assert torch.equal(model.read_tensor(0, name), sd[name].float())
