"""The bf16x3 Winograd kernel's item table (tile_cfg 74; conv_winograd_bf3.inc): what a workgroup derives from a work item's
index comes from a per-geometry table of 64-byte records, cached in the context.

Every case: each image bit-equal to its own B = 1 run (a B = 1 launch is first-item code only), the output inside the
per-kernel bound of tests/test_gpu_kernels.py against a float64 evaluation (max-abs <= 1e-5 * max(1, |ref|_inf)), and the same
bits with SISIC_BF3_ITEM_TABLE=0 (the kernel derives the items itself) as by default.
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _close(got, ref64, what):
    got = got.detach().cpu().double()
    bound = KTOL * max(1.0, ref64.abs().max().item())
    err = (got - ref64).abs().max().item()
    print(f"{what}: max abs err {err:.3e}, bound {bound:.3e}")
    assert got.shape == ref64.shape, what
    assert err <= bound, f"{what}: max abs err {err:.3e} > {bound:.3e}"


def _ref(x, w, bias, x2, ups, gn, chan_bias, residual):
    x = x.double()
    if x2 is not None:
        x = torch.cat([x, x2.double()], dim=1)
    if gn is not None:
        x = F.silu(x * gn[0].double()[:, :, None, None] + gn[1].double()[:, :, None, None])
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    y = F.conv2d(x, w.double(), bias.double(), padding=1)
    if chan_bias is not None:
        y = y + chan_bias.double()[:, :, None, None]
    if residual is not None:
        y = y + residual.double()
    return y


class _Table:
    """SISIC_BF3_ITEM_TABLE for the launches inside (the library reads it at every launch)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("SISIC_BF3_ITEM_TABLE")
        if self.value is None:
            os.environ.pop("SISIC_BF3_ITEM_TABLE", None)
        else:
            os.environ["SISIC_BF3_ITEM_TABLE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("SISIC_BF3_ITEM_TABLE", None)
        else:
            os.environ["SISIC_BF3_ITEM_TABLE"] = self.old


class _Layer:
    """One convolution's operands on the GPU, and its launch on any slice of the batch."""

    def __init__(self, B, H, W, c0, c1, cout, ups=False, gn=True, res=True, seed=900):
        from synt_isic_amd import ops
        self.B, self.ups, self.cout = B, ups, cout
        C_ = c0 + c1
        self.x = _rand(B, c0, H, W, seed=seed)
        self.x2 = _rand(B, c1, H, W, seed=seed + 1) if c1 else None
        self.w = _rand(cout, C_, 3, 3, seed=seed + 2, scale=(9 * C_) ** -0.5)
        self.b = _rand(cout, seed=seed + 3)
        self.gn = (1.0 + 0.3 * _rand(B, C_, seed=seed + 4), 0.3 * _rand(B, C_, seed=seed + 5)) if gn else None
        self.cb = _rand(B, cout, seed=seed + 6)
        self.Ho, self.Wo = (2 * H, 2 * W) if ups else (H, W)
        self.res = _rand(B, cout, self.Ho, self.Wo, seed=seed + 7) if res else None
        self.wp, self.ww = ops.pack_conv_weight(_d(self.w)), ops.pack_winograd_weight(_d(self.w))
        self.dev = [_d(t) for t in (self.x, self.x2, self.b, self.cb, self.res)] + [None if self.gn is None else (_d(self.gn[0]), _d(self.gn[1]))]

    def run(self, sl=None, **kw):
        from synt_isic_amd import ops
        sl = slice(0, self.B) if sl is None else sl
        x, x2, b, cb, res, gn = self.dev
        c = lambda t: None if t is None else t[sl].contiguous()
        return ops.conv2d(c(x), self.wp, self.cout, 3, bias=b, x2=c(x2), upsample=self.ups,
                          gn_scale=c(gn[0]) if gn else None, gn_shift=c(gn[1]) if gn else None, gn_silu=bool(gn),
                          chan_bias=c(cb), residual=c(res), tile_cfg=74, w_winograd=self.ww, with_stats=True, **kw)

    def reference(self):
        return _ref(self.x, self.w, self.b, self.x2, self.ups, self.gn, self.cb, self.res)


def _check(layer, what):
    """the three checks of this file on one layer; returns the default launch's (output, partials)"""
    with _Table(None):
        y, st = layer.run()
        ones = [layer.run(slice(i, i + 1)) for i in range(layer.B)]
    with _Table("0"):
        y0, st0 = layer.run()
    assert torch.equal(y, y0) and torch.equal(st, st0), f"{what}: the item table changes the bits"
    for i, (yi, sti) in enumerate(ones):
        assert torch.equal(yi[0], y[i]) and torch.equal(sti[0], st[i]), f"{what}: image {i} differs from the same image alone"
    assert torch.all(st[..., 0].sum(dim=2) == layer.Ho * layer.Wo), what
    _close(y, layer.reference(), what)
    return y, st


def test_several_items_per_workgroup_regular():
    """40 x 4 positions x 2 channel tiles = 320 items on 256 workgroups, 8 items per image: a workgroup's next item is the same
    tile and channel tile four images on."""
    _check(_Layer(40, 32, 32, 64, 0, 128), "32x32 64->128 B=40")


def test_several_items_per_workgroup_irregular():
    """5 x 16 positions x 4 channel tiles = 320 items, 64 per image: no whole number of images between a workgroup's items --
    another tile position (a new staging plan) and another channel tile from item to item."""
    _check(_Layer(5, 64, 64, 64, 0, 256, seed=920), "64x64 64->256 B=5")


@pytest.mark.parametrize("H,W", [(20, 28), (19, 21)])
@pytest.mark.parametrize("res", [True, False])
def test_ragged_and_odd_planes(H, W, res):
    """clamped lanes, odd width, partial tiles, two sources: the code behind the whole-tile fast path's branch"""
    _check(_Layer(3, H, W, 64, 32, 70, res=res, seed=940), f"{H}x{W} 64+32->70 B=3 res={res}")


@pytest.mark.parametrize("H", [8, 16])
def test_nearest_2x_instance(H):
    """the upsampling instance: 40 x 1 x 2 = 80 items (8x8 -> 16x16) and 40 x 4 x 2 = 320 items (16x16 -> 32x32)"""
    _check(_Layer(40, H, H, 128, 0, 128, ups=True, gn=False, seed=960), f"nearest-2x {H}x{H} 128->128 B=40")


def test_finalizing_instance():
    """One 16 x 16 tile per image, 256 channels: the workgroup leaves the following GroupNorm's (scale, shift) itself; 66 x 4 =
    264 items, so eight workgroups finalize two images.  Bit-equal to sisic_groupnorm_finalize on the same partials."""
    from synt_isic_amd import ops
    layer = _Layer(66, 16, 16, 256, 0, 256, seed=980)
    gamma, beta = _d(1.0 + 0.1 * _rand(256, seed=990)), _d(0.1 * _rand(256, seed=991))
    y, st = _check(layer, "16x16 256->256 B=66")
    results = []
    for value in (None, "0"):
        with _Table(value):
            yf, stf, fin = layer.run(finalize=(gamma, beta, 32, 1e-5))
        assert fin is not None
        sc, sh = ops.groupnorm_finalize(stf, 256, gamma, beta, 32, 1e-5)
        assert torch.equal(fin[0], sc) and torch.equal(fin[1], sh), f"SISIC_BF3_ITEM_TABLE={value}"
        assert torch.equal(yf, y) and torch.equal(stf, st)
        results.append(fin)
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_table_cache():
    """Two geometries alternate over six launches, then a third batch size of the first: the same bits as every launch on a
    fresh context (whose table is filled in front of that very launch)."""
    from synt_isic_amd import _lib, ops
    lib = _lib.load()
    a, b = _Layer(40, 32, 32, 64, 0, 128, seed=1000), _Layer(5, 64, 64, 64, 0, 256, seed=1010)
    plan = [(a, None), (b, None), (a, None), (b, None), (a, None), (b, None), (a, slice(0, 37))]
    got = [layer.run(sl) for layer, sl in plan]
    idx = torch.cuda.current_device()
    ops.context(torch.device(DEV))
    shared = ops._ctx_by_device[idx]
    try:
        for k, (layer, sl) in enumerate(plan):
            fresh = C.c_void_p()
            _lib.check(lib.sisic_create(idx, C.byref(fresh)))
            ops._ctx_by_device[idx] = fresh
            try:
                y, st = layer.run(sl)
                torch.cuda.synchronize()
            finally:
                ops._ctx_by_device[idx] = shared
                _lib.check(lib.sisic_destroy(fresh))
            assert torch.equal(y, got[k][0]) and torch.equal(st, got[k][1]), f"launch {k}"
    finally:
        ops._ctx_by_device[idx] = shared
    # the third batch size is the first 37 images of the first geometry's batch
    assert torch.equal(got[6][0], got[0][0][:37]) and torch.equal(got[6][1], got[0][1][:37])
