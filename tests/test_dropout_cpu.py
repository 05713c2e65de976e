"""ResnetBlock2D dropout, the parts that need no GPU: the restatement the GPU suite compares against (tests/dropout_ref.py)
and its mask, the Python mirror's argument checks, the two C entry points in the header and the binding."""
import math
import os
import re

import numpy as np
import pytest
import torch

import dropout_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_without_dropout_is_the_oracle(synthetic_sd):
    from oracle import unet as ounet
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 32, 32, generator=g)
    t = torch.tensor([12, 801])
    with torch.no_grad():
        assert torch.equal(dropout_ref.unet_forward(synthetic_sd, x, t), ounet.unet_forward(synthetic_sd, x, t))


def test_conditional_restatement_without_dropout_is_cond_ref():
    import cond_ref
    from synt_isic_amd.weights import synthetic_unet_state_dict
    sd = synthetic_unet_state_dict(num_class_embeds=3)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 32, 32, generator=g)
    t = torch.tensor([3, 500])
    with torch.no_grad():
        assert torch.equal(dropout_ref.unet_forward(sd, x, t, [1, 0]), cond_ref.unet_forward(sd, x, t, [1, 0]))


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_kept_fraction(p):
    """2^16 elements: the kept count is binomial(n, 1 - p') with p' = ceil(p 2^24) / 2^24, within 2^-24 of p; 5 sigma"""
    n = 1 << 16
    kept = int(dropout_ref.keep_mask(p, seed=1234, call=7, block=3, sample=1, n=n).sum())
    sigma = math.sqrt(n * p * (1.0 - p))
    assert abs(kept - n * (1.0 - p)) <= 5.0 * sigma, (kept, n * (1.0 - p), sigma)


def test_masks_differ_by_block_sample_and_call():
    n, p = 4096, 0.5
    base = dropout_ref.keep_mask(p, seed=9, call=0, block=0, sample=0, n=n)
    assert np.array_equal(base, dropout_ref.keep_mask(p, seed=9, call=0, block=0, sample=0, n=n))      # a pure function
    for kw in ({"block": 1}, {"sample": 1}, {"call": 1}):
        args = {"seed": 9, "call": 0, "block": 0, "sample": 0, **kw}
        other = dropout_ref.keep_mask(p, n=n, **args)
        # independent fair bits agree on n/2 +- sqrt(n)/2: far from all n
        assert (base == other).sum() < 0.6 * n, kw
    # sample b of seed s is sample 0 of seed s + b (the contract's seed + b)
    assert np.array_equal(dropout_ref.keep_mask(p, 9, 0, 0, 2, n), dropout_ref.keep_mask(p, 11, 0, 0, 0, n))


def test_dropped_values_are_zero_and_kept_ones_scaled_once():
    a = torch.randn(2, 8, 4, 4, generator=torch.Generator().manual_seed(1))
    p = 0.25
    out = dropout_ref.dropout(a, p, seed=3, call=2, block=5)
    keep = torch.from_numpy(np.stack([dropout_ref.keep_mask(p, 3, 2, 5, b, 128) for b in range(2)]).reshape(2, 8, 4, 4))
    inv = dropout_ref.inv_keep(p)
    assert inv == np.float32(4.0 / 3.0) and float(inv) != 4.0 / 3.0          # inexact: a second rounding would show
    assert torch.equal(out[keep], a[keep] * float(inv))
    assert (out[~keep] == 0).all() and not torch.signbit(out[~keep]).any()


def test_model_takes_dropout():
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel(dropout=0.1)
    assert m.config.dropout == 0.1
    assert HipUNet2DModel().config.dropout == 0.0
    assert m.dropout_next_call == 0
    m.set_dropout(0.3, seed=5, first_call=17)                                # no handle yet: kept for when there is one
    assert m.config.dropout == 0.3 and m.dropout_next_call == 17
    assert list(m._spec) == list(HipUNet2DModel()._spec)                     # dropout adds no tensors


@pytest.mark.parametrize("p", [-0.1, 1.0, float("nan"), float("inf"), "0.1", True])
def test_bad_dropout_is_a_value_error(p):
    from synt_isic_amd.arch import UNetConfig
    from synt_isic_amd.unet import HipUNet2DModel
    with pytest.raises(ValueError):
        HipUNet2DModel(dropout=p)
    with pytest.raises(ValueError):
        UNetConfig(dropout=p).validate()
    m = HipUNet2DModel(dropout=0.2)
    with pytest.raises(ValueError):
        m.set_dropout(p)
    assert m.config.dropout == 0.2                                            # a refused setting changes nothing


def test_pinned_refusals_stay():
    from synt_isic_amd.unet import HipUNet2DModel
    with pytest.raises(NotImplementedError):
        HipUNet2DModel(dropout=0.1, attention_head_dim=16)
    with pytest.raises(NotImplementedError):
        HipUNet2DModel(dropout=0.1, resnet_time_scale_shift="scale_shift")


def test_training_loops_take_a_dropout_seed():
    import inspect
    from synt_isic_amd import train
    for fn in (train.train_class, train.train_conditional):
        assert inspect.signature(fn).parameters["dropout_seed"].default == 0


def _declarations():
    src = open(os.path.join(ROOT, "include", "sisic.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return src, {name: params for name, params in re.findall(r"\b(sisic_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", plain)}


def test_header_declares_the_two_entry_points_without_a_stream():
    src, decl = _declarations()
    for name in ("sisic_unet_set_dropout", "sisic_unet_dropout_next_call"):
        assert name in decl, name
        assert not re.search(r"\bvoid\s*\*", decl[name]), (name, decl[name])          # no stream, under any name
    assert re.search(r"^#define SISIC_ABI_VERSION 3$", src, flags=re.M)
    assert "tag = 256 + r" in " ".join(src.split())                                    # the mask contract is written down


def test_binding_has_both():
    import ctypes as C
    from synt_isic_amd import _lib
    assert _lib.SIGNATURES["sisic_unet_set_dropout"] == (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint32])
    assert _lib.SIGNATURES["sisic_unet_dropout_next_call"] == (C.c_uint32, [C.c_void_p])
    assert _lib.ABI_VERSION == 3


def test_set_dropout_checks_its_arguments_without_a_gpu():
    """the setter touches no device memory: a null handle is refused with a message"""
    from synt_isic_amd import _lib
    lib = _lib.load()
    assert lib.sisic_unet_set_dropout(None, 0.1, 0, 0) == _lib.SISIC_EINVAL
    assert b"set_dropout" in lib.sisic_last_error()
    assert lib.sisic_unet_dropout_next_call(None) == 0
