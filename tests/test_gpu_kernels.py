"""Per-kernel parity: each HIP kernel, called through the C ABI, against the CPU oracle's torch op.

Tolerance (unchanged): fp32 kernels max-abs <= 1e-5 * max(1, |ref|_inf) against a float64
evaluation of the same op (round 1 ran these at 2e-5 / 3e-5; the largest error measured over all 974 comparisons of this
file on MI355X is 3.6e-6, tools: SISIC_TEST_ERRLOG); the scheduler step, the de-normalisation and everything integer are
bit-exact.
"""
import itertools

import numpy as np
import os

import pytest
import torch
import torch.nn.functional as F

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5          # per kernel max-abs <= 1e-5 * max(1, |ref|_inf) vs a float64 evaluation


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _close(got: torch.Tensor, ref64: torch.Tensor, tol=KTOL, what=""):
    got = got.detach().cpu().double()
    bound = tol * max(1.0, ref64.abs().max().item())
    err = (got - ref64).abs().max().item()
    if os.environ.get("SISIC_TEST_ERRLOG"):          # measured error / max(1,|ref|) of every comparison, for tolerance audits
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(f"{err / max(1.0, ref64.abs().max().item()):.3e}\t{tol:.1e}\t{what}\n")
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert err <= bound, f"{what}: max abs err {err:.3e} > {bound:.3e}"


def _conv_ref(x, w, bias=None, x2=None, stride=1, upsample=False, gn=None, gn_silu=False, chan_bias=None,
              residual=None, relu=False):
    """float64 restatement with the oracle's torch ops."""
    x = x.double()
    if x2 is not None:
        x = torch.cat([x, x2.double()], dim=1)
    if gn is not None:
        scale, shift = gn
        x = x * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
        if gn_silu:
            x = F.silu(x)
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    k = w.shape[-1]
    y = F.conv2d(x, w.double(), None if bias is None else bias.double(), stride=stride, padding=k // 2)
    if chan_bias is not None:
        y = y + chan_bias.double()[:, :, None, None]
    if residual is not None:
        y = y + residual.double()
    if relu:
        y = F.relu(y)
    return y


def _run_conv(x, w, cfg, **kw):
    from synt_isic_amd import ops
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    wp = ops.pack_conv_weight(d(w))
    gn = kw.get("gn")
    return ops.conv2d(d(x), wp, w.shape[0], w.shape[-1], bias=d(kw.get("bias")), x2=d(kw.get("x2")),
                      stride=kw.get("stride", 1), upsample=kw.get("upsample", False),
                      gn_scale=d(gn[0]) if gn else None, gn_shift=d(gn[1]) if gn else None,
                      gn_silu=kw.get("gn_silu", False), chan_bias=d(kw.get("chan_bias")),
                      residual=d(kw.get("residual")), relu=kw.get("relu", False), tile_cfg=cfg)


# (cfg, H, W) -- natural shapes for each tile configuration plus ragged ones that exercise the masks
CONV3_S1 = [(1, 64, 64), (1, 12, 70), (2, 32, 32), (2, 20, 40), (3, 16, 16), (3, 24, 24), (4, 8, 8), (4, 9, 5),
            (5, 16, 16), (6, 64, 64), (6, 10, 70), (7, 32, 32), (7, 9, 40), (8, 32, 32), (8, 20, 40), (9, 16, 16),
            (9, 24, 20), (14, 16, 16), (14, 20, 12), (15, 8, 8), (15, 16, 24), (16, 8, 8), (16, 9, 5), (17, 8, 8), (17, 12, 7),
            (0, 64, 64), (0, 8, 8)]


@pytest.mark.parametrize("cfg,H,W", CONV3_S1)
def test_conv3x3_plain(cfg, H, W):
    x = _rand(2, 16, H, W, seed=1)
    w = _rand(64, 16, 3, 3, seed=2, scale=0.1)
    b = _rand(64, seed=3)
    _close(_run_conv(x, w, cfg, bias=b), _conv_ref(x, w, b), what=f"conv3x3 cfg{cfg} {H}x{W}")


@pytest.mark.parametrize("cin,cout", [(3, 64), (64, 3), (19, 70), (8, 128), (130, 64)])
def test_conv3x3_channel_edges(cin, cout):
    x = _rand(2, cin, 16, 32, seed=4)
    w = _rand(cout, cin, 3, 3, seed=5, scale=0.1)
    b = _rand(cout, seed=6)
    for cfg in (0, 1, 4, 14, 16):
        _close(_run_conv(x, w, cfg, bias=b), _conv_ref(x, w, b), what=f"conv3x3 {cin}->{cout} cfg{cfg}")


@pytest.mark.parametrize("H,W", [(64, 64), (16, 16), (20, 36), (5, 7)])
def test_conv3x3_small_cout_kernel(H, W):
    """Cout <= 4 takes the vector-ALU kernel (conv_small.hip, tile_cfg 50 / auto): every fused feature."""
    B, c0, c1 = 2, 20, 12
    x, x2 = _rand(B, c0, H, W, seed=80), _rand(B, c1, H, W, seed=81)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=82), 0.3 * _rand(B, c0 + c1, seed=83))
    for cout in (1, 3, 4):
        w = _rand(cout, c0 + c1, 3, 3, seed=84 + cout, scale=0.1)
        b = _rand(cout, seed=90 + cout)
        res = _rand(B, cout, H, W, seed=95 + cout)
        cb = _rand(B, cout, seed=99 + cout)
        outs = {}
        for cfg in (0, 50, 51):
            kw = dict(bias=b, x2=x2, gn=gn, gn_silu=True)
            outs[cfg] = _run_conv(x, w, cfg, **kw)
            _close(outs[cfg], _conv_ref(x, w, **kw), what=f"small-cout {cout} cfg{cfg} {H}x{W}")
            kw = dict(bias=b, x2=x2, gn=gn, gn_silu=False, chan_bias=cb, residual=res, relu=True)
            _close(_run_conv(x, w, cfg, **kw), _conv_ref(x, w, **kw), what=f"small-cout fused {cout} cfg{cfg}")
        # the 32-row and the 8-row tile (picked from the number of workgroups) sum a pixel's channels in the same order
        assert torch.equal(outs[50], outs[51]) and torch.equal(outs[0], outs[50])
        # (from 32 input channels up every tiling splits the channels over four thread groups -- a rule of the shape; tile_cfg 52
        #  is the one-group form, another summation order)
        kw = dict(bias=b, x2=x2, gn=gn, gn_silu=True)
        _close(_run_conv(x, w, 52, **kw), _conv_ref(x, w, **kw), what=f"small-cout {cout} one channel group {H}x{W}")
        assert torch.equal(_run_conv(x[1:2], w, 0, bias=b, x2=x2[1:2], gn=(gn[0][1:2], gn[1][1:2]), gn_silu=True), outs[0][1:2])
    w = _rand(3, 64, 3, 3, seed=101, scale=0.05)
    x = _rand(1, 64, H, W, seed=102)
    _close(_run_conv(x, w, 0), _conv_ref(x, w), what="small-cout plain 64->3")


def test_conv3x3_no_bias_and_identity_weight():
    """A = I with an asymmetric input: catches a swapped MFMA row/column map."""
    C = 64
    x = _rand(1, C, 8, 8, seed=7)
    w = torch.zeros(C, C, 3, 3)
    for c in range(C):
        w[c, c, 1, 1] = 1.0
    for cfg in (1, 2, 3, 4, 5, 6, 7, 8, 9):
        got = _run_conv(x, w, cfg).cpu()
        assert torch.equal(got, x), f"identity conv cfg{cfg} is not exact"
    # shifted identity: out[c] = in[(c+1) % C] moved one pixel right
    w2 = torch.zeros(C, C, 3, 3)
    for c in range(C):
        w2[c, (c + 1) % C, 1, 0] = 1.0
    want = F.conv2d(x, w2, padding=1)
    for cfg in (1, 4):
        assert torch.equal(_run_conv(x, w2, cfg).cpu(), want)


@pytest.mark.parametrize("cfg,H,W", [(1, 64, 64), (2, 32, 32), (3, 16, 16), (4, 8, 8), (2, 20, 24), (5, 16, 16),
                                     (6, 64, 64), (7, 32, 32), (8, 32, 32), (9, 16, 16), (16, 8, 8), (17, 8, 8)])
def test_conv3x3_fused_everything(cfg, H, W):
    """two sources whose seam falls inside a channel chunk + GN/SiLU prologue + time bias + residual."""
    B, c0, c1, cout = 2, 20, 12, 64
    x, x2 = _rand(B, c0, H, W, seed=8), _rand(B, c1, H, W, seed=9)
    w = _rand(cout, c0 + c1, 3, 3, seed=10, scale=0.1)
    b = _rand(cout, seed=11)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=12), 0.3 * _rand(B, c0 + c1, seed=13))
    cb = _rand(B, cout, seed=14)
    res = _rand(B, cout, H, W, seed=15)
    kw = dict(bias=b, x2=x2, gn=gn, gn_silu=True, chan_bias=cb, residual=res)
    _close(_run_conv(x, w, cfg, **kw), _conv_ref(x, w, **kw), what=f"fused conv cfg{cfg}")
    kw = dict(bias=b, x2=x2, gn=gn, gn_silu=False, relu=True)
    _close(_run_conv(x, w, cfg, **kw), _conv_ref(x, w, **kw), what=f"fused conv (no silu, relu) cfg{cfg}")
    # one chan_bias row shared by every sample (the sampler's per-step time embedding)
    kw = dict(bias=b, x2=x2, chan_bias=cb[0])
    ref = _conv_ref(x, w, bias=b, x2=x2, chan_bias=cb[0:1].expand(B, -1))
    _close(_run_conv(x, w, cfg, **kw), ref, what=f"broadcast chan_bias cfg{cfg}")


def _run_wino(x, w, cfg, **kw):
    from synt_isic_amd import ops
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    gn = kw.get("gn")
    return ops.conv2d(d(x), ops.pack_conv_weight(d(w)), w.shape[0], 3, bias=d(kw.get("bias")), x2=d(kw.get("x2")),
                      upsample=kw.get("upsample", False), gn_scale=d(gn[0]) if gn else None,
                      gn_shift=d(gn[1]) if gn else None, gn_silu=kw.get("gn_silu", False),
                      chan_bias=d(kw.get("chan_bias")), residual=d(kw.get("residual")), relu=kw.get("relu", False),
                      tile_cfg=cfg, w_winograd=ops.pack_winograd_weight(d(w)))


@pytest.mark.parametrize("cfg,B,H,W", [(60, 2, 16, 16), (60, 2, 64, 64), (60, 1, 32, 48), (60, 3, 18, 10), (60, 2, 9, 23),
                                       (61, 8, 8, 8), (61, 5, 8, 8), (61, 3, 6, 10), (0, 2, 32, 32), (0, 2, 8, 8),
                                       (62, 2, 16, 16), (62, 2, 64, 64), (62, 3, 18, 10), (62, 2, 9, 23), (63, 8, 8, 8),
                                       (63, 5, 8, 8), (63, 3, 6, 10), (66, 2, 16, 16), (66, 3, 18, 10), (67, 5, 8, 8),
                                       # second geometry: 68 = 128 channels x 32 tiles, 69 = 64 channels x 32 tiles (2 WG / CU)
                                       (68, 2, 16, 16), (68, 2, 64, 64), (68, 1, 32, 48), (68, 3, 18, 10), (68, 2, 9, 23),
                                       (69, 2, 16, 16), (69, 2, 64, 64), (69, 1, 32, 48), (69, 3, 18, 10), (69, 2, 9, 23),
                                       # latency mode: the same geometry with the input channels K-split over workgroups
                                       (78, 2, 16, 16), (78, 1, 32, 48), (78, 2, 9, 23), (79, 2, 16, 16), (79, 1, 64, 64),
                                       # (68 / 69 / 78 / 79 run the third form, conv_winograd_col.inc, since round 3;
                                       #  72 / 73 force the second form, 70 / 71 the third)
                                       (72, 2, 16, 16), (72, 3, 18, 10), (73, 2, 64, 64), (73, 2, 9, 23),
                                       (70, 2, 64, 64), (70, 3, 18, 10), (71, 1, 32, 48), (71, 2, 9, 23),
                                       # 74: fp32-equivalent (bf16x3, six products) on the bf16 matrix pipe, 64 tiles per workgroup
                                       (74, 2, 16, 16), (74, 2, 64, 64), (74, 1, 32, 48), (74, 3, 18, 10), (74, 2, 9, 23),
                                       ])
def test_conv3x3_winograd(cfg, B, H, W):
    """Winograd F(2x2,3x3) on the MFMA pipe == the float64 convolution, plain and with every fused feature
    (cfg 60: 8x8 tiles of one image; 61: 4 images x 4x4 tiles; 0: auto dispatch with Winograd filters present)."""
    c0, c1, cout = 20, 12, 70                        # seam inside a chunk, Cout not a multiple of 64
    x, x2 = _rand(B, c0, H, W, seed=110), _rand(B, c1, H, W, seed=111)
    w = _rand(cout, c0 + c1, 3, 3, seed=112, scale=0.1)
    b = _rand(cout, seed=113)
    _close(_run_wino(x, w[:, :c0].contiguous(), cfg, bias=b), _conv_ref(x, w[:, :c0], b), what=f"winograd plain cfg{cfg}")
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=114), 0.3 * _rand(B, c0 + c1, seed=115))
    cb = _rand(B, cout, seed=116)
    res = _rand(B, cout, H, W, seed=117)
    kw = dict(bias=b, x2=x2, gn=gn, gn_silu=True, chan_bias=cb, residual=res)
    _close(_run_wino(x, w, cfg, **kw), _conv_ref(x, w, **kw), tol=KTOL, what=f"winograd fused cfg{cfg}")
    kw = dict(bias=b, x2=x2, gn=gn, gn_silu=False, relu=True, chan_bias=cb[0])
    ref = _conv_ref(x, w, bias=b, x2=x2, gn=gn, relu=True, chan_bias=cb[0:1].expand(B, -1))
    _close(_run_wino(x, w, cfg, **kw), ref, tol=KTOL, what=f"winograd fused 2 cfg{cfg}")


@pytest.mark.parametrize("cfg,H,W", [(60, 16, 16), (60, 8, 8), (60, 10, 14), (61, 4, 4), (62, 16, 16), (62, 10, 14),
                                     (63, 4, 4),
                                     # 66 / auto: the nine-position form for nearest-2x inputs
                                     (66, 16, 16), (66, 8, 8), (66, 10, 14), (66, 5, 9), (66, 32, 32), (0, 8, 8), (0, 20, 12),
                                     # 74: the bf16x3 form reads a nearest-2x input through its staging addresses (all 16 positions)
                                     (74, 16, 16), (74, 10, 14), (74, 32, 32), (0, 32, 32)])
def test_conv3x3_winograd_upsample(cfg, H, W):
    x = _rand(2, 24, H, W, seed=120)
    w = _rand(64, 24, 3, 3, seed=121, scale=0.1)
    b = _rand(64, seed=122)
    _close(_run_wino(x, w, cfg, bias=b, upsample=True), _conv_ref(x, w, b, upsample=True), what=f"winograd upsample cfg{cfg}")
    # Cout not a multiple of 64, residual on the upsampled grid, ReLU
    w2, b2 = _rand(70, 24, 3, 3, seed=124, scale=0.1), _rand(70, seed=125)
    res = _rand(2, 70, 2 * H, 2 * W, seed=126)
    _close(_run_wino(x, w2, cfg, bias=b2, upsample=True, residual=res, relu=True),
           _conv_ref(x, w2, b2, upsample=True, residual=res, relu=True), what=f"winograd upsample+res cfg{cfg}")


@pytest.mark.parametrize("B,H,W,c0,c1,cout", [(8, 8, 8, 64, 0, 64), (5, 8, 8, 40, 24, 70), (3, 6, 10, 96, 0, 128),
                                              (32, 8, 8, 128, 0, 128)])
def test_conv3x3_winograd_ksplit(B, H, W, c0, c1, cout):
    """tile_cfg 90: the input channels of a tile split over four workgroups + the reduction kernel (bias, embedding,
    residual, ReLU and the GroupNorm partials move into the reduction); the last case is taken by the auto dispatch."""
    from synt_isic_amd import ops
    x = _rand(B, c0, H, W, seed=190)
    x2 = _rand(B, c1, H, W, seed=191) if c1 else None
    w = _rand(cout, c0 + c1, 3, 3, seed=192, scale=0.05)
    b = _rand(cout, seed=193)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=194), 0.3 * _rand(B, c0 + c1, seed=195))
    cb = _rand(B, cout, seed=196)
    res = _rand(B, cout, H, W, seed=197)
    kw = dict(bias=b, x2=x2, gn=gn, gn_silu=True, chan_bias=cb, residual=res)
    _close(_run_wino(x, w, 90, **kw), _conv_ref(x, w, **kw), tol=KTOL, what="winograd K-split fused")
    kw = dict(bias=b, x2=x2, relu=True)
    _close(_run_wino(x, w, 90, **kw), _conv_ref(x, w, **kw), tol=KTOL, what="winograd K-split relu")
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    cfg = 0 if (H, W, c0 + c1, cout) == (8, 8, 128, 128) else 90      # the last case is what the auto dispatch picks
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, 3, bias=d(b), x2=d(x2), residual=d(res), tile_cfg=cfg,
                       w_winograd=ops.pack_winograd_weight(d(w)), with_stats=True)
    _close(y, _conv_ref(x, w, bias=b, x2=x2, residual=res), tol=KTOL, what="winograd K-split + stats")
    assert st is not None and tuple(st.shape) == (B, cout, 1, 4)
    G = 2 if cout % 32 else 32
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=198), 0.1 * _rand(cout, seed=199)
    sc, sh = ops.groupnorm_finalize(st, H * W, d(gamma), d(beta), G, 1e-5)
    yc = y.cpu().double()
    ref = F.group_norm(yc, G, gamma.double(), beta.double(), 1e-5)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="groupnorm from K-split reduction partials")
    from synt_isic_amd._lib import SisicError
    with pytest.raises(SisicError, match="split"):
        _run_wino(x[:, :24].contiguous(), w[:, :24].contiguous(), 90)        # 3 chunks do not split four ways


@pytest.mark.parametrize("B,H,W,c0,c1,cout,ups", [
    (20, 64, 64, 16, 0, 64, False),       # 320 items on 256 persistent workgroups: a quarter of them take a second item
    (70, 28, 28, 24, 8, 64, False),       # 280 items, ragged planes, two sources: padding slots differ from item to item
    (9, 32, 32, 16, 0, 128, True),        # nearest-2x input: 9 x 16 x 2 = 288 items
    (33, 16, 16, 32, 0, 512, False),      # 264 items that differ in their channel tile only
    (40, 64, 64, 16, 0, 64, False),       # 640 items: two or three per workgroup
    (65, 32, 32, 16, 0, 64, False),       # 260 items, not a multiple of 8: the work remap is irregular, every item is decoded
    (32, 48, 48, 16, 0, 64, False),       # 288 items of 9 positions per image: a workgroup's next item is another position (new plan)
    (30, 40, 40, 16, 8, 64, False),       # 270 items, ragged 40 = 2.5 tiles: the next item is another position with OTHER padding slots
])
def test_conv3x3_winograd_bf16x3_persistent_workgroups(B, H, W, c0, c1, cout, ups):
    """More work items than CUs: a workgroup of the bf16x3 Winograd kernel takes several, requesting the next item's first
    halo chunks before its output rounds.  Every feature of the epilogue and the GroupNorm partials, against float64; and
    every image equal, bit for bit, to the same image convolved in a batch that gives each workgroup one item."""
    from synt_isic_amd import ops
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    x = _rand(B, c0, H, W, seed=800)
    x2 = _rand(B, c1, H, W, seed=801) if c1 else None
    C = c0 + c1
    w = _rand(cout, C, 3, 3, seed=802, scale=0.1)
    b = _rand(cout, seed=803)
    gn = None if ups else (1.0 + 0.3 * _rand(B, C, seed=804), 0.3 * _rand(B, C, seed=805))
    cb = _rand(B, cout, seed=806)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    res = _rand(B, cout, Ho, Wo, seed=807)
    wp, ww = ops.pack_conv_weight(d(w)), ops.pack_winograd_weight(d(w))

    def run(sl):
        return ops.conv2d(d(x[sl]), wp, cout, 3, bias=d(b), x2=d(x2[sl]) if c1 else None, upsample=ups,
                          gn_scale=d(gn[0][sl]) if gn else None, gn_shift=d(gn[1][sl]) if gn else None, gn_silu=bool(gn),
                          chan_bias=d(cb[sl]), residual=d(res[sl]), tile_cfg=74, w_winograd=ww, with_stats=True)
    y, st = run(slice(0, B))
    ref = _conv_ref(x, w, bias=b, x2=x2, upsample=ups, gn=gn, gn_silu=bool(gn), chan_bias=cb, residual=res)
    _close(y, ref, tol=KTOL, what="bf16x3 winograd, several items per workgroup")
    # images from both ends and the middle, alone (a handful of items: one per workgroup)
    for i in (0, B // 2, B - 1):
        yi, sti = run(slice(i, i + 1))
        assert torch.equal(yi[0], y[i]) and torch.equal(sti[0], st[i]), f"image {i} differs from the same image alone"
    n = st[..., 0].sum(dim=2)
    assert torch.all(n == Ho * Wo)
    mean = (st[..., 1].double().sum(dim=2) / (Ho * Wo)).cpu()
    _close(mean.float(), ref.mean(dim=(2, 3)), tol=KTOL, what="partials' sums, several items per workgroup")


@pytest.mark.parametrize("B,H,W,c0,c1,cout", [(8, 8, 8, 64, 0, 64), (5, 8, 8, 40, 24, 70), (3, 6, 7, 96, 0, 128),
                                              (32, 8, 8, 128, 0, 128), (1, 7, 7, 64, 0, 200), (2, 4, 4, 32, 0, 256)])
def test_conv3x3_winograd_ksplit_image_pairs(B, H, W, c0, c1, cout):
    """tile_cfg 91: the K-split of tile_cfg 90 on the second geometry -- 128 channels x (two images of <= 4x4 tiles) per
    workgroup, odd batches leave the second image of the last pair empty.  Same filters, same channel order, same
    reduction: every bit equals tile_cfg 90's."""
    x = _rand(B, c0, H, W, seed=290)
    x2 = _rand(B, c1, H, W, seed=291) if c1 else None
    w = _rand(cout, c0 + c1, 3, 3, seed=292, scale=0.05)
    b = _rand(cout, seed=293)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=294), 0.3 * _rand(B, c0 + c1, seed=295))
    cb = _rand(B, cout, seed=296)
    res = _rand(B, cout, H, W, seed=297)
    for kw in (dict(bias=b, x2=x2, gn=gn, gn_silu=True, chan_bias=cb, residual=res), dict(bias=b, x2=x2, relu=True),
               dict(bias=b, x2=x2, gn=gn, gn_silu=False)):
        y = _run_wino(x, w, 91, **kw)
        _close(y, _conv_ref(x, w, **kw), tol=KTOL, what="winograd K-split, image pairs")
        assert torch.equal(y, _run_wino(x, w, 90, **kw))
    # GroupNorm partials from the reduction: one slot per (image, channel) plane
    from synt_isic_amd import ops
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, 3, bias=d(b), x2=d(x2), residual=d(res), tile_cfg=91,
                       w_winograd=ops.pack_winograd_weight(d(w)), with_stats=True)
    assert st is not None and tuple(st.shape) == (B, cout, 1, 4)
    G = 2 if cout % 32 else 32
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=288), 0.1 * _rand(cout, seed=289)
    sc, sh = ops.groupnorm_finalize(st, H * W, d(gamma), d(beta), G, 1e-5)
    yc = y.cpu().double()
    ref = F.group_norm(yc, G, gamma.double(), beta.double(), 1e-5)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="groupnorm from the K-split reduction, image pairs")
    from synt_isic_amd._lib import SisicError
    with pytest.raises(SisicError, match="8x8"):
        _run_wino(_rand(2, 32, 8, 10, seed=298), _rand(64, 32, 3, 3, seed=299), 91)


@pytest.mark.parametrize("B,H,W,c0,c1,cout", [(8, 8, 8, 64, 0, 64), (5, 8, 8, 40, 24, 70), (3, 6, 7, 96, 0, 128),
                                              (32, 8, 8, 128, 0, 128), (1, 7, 7, 64, 0, 200), (6, 8, 8, 256, 256, 256)])
def test_conv3x3_winograd_ksplit_bf16x3(B, H, W, c0, c1, cout):
    """tile_cfg 92: the 8x8 level with fp32-equivalent products on the bf16 matrix pipe -- four images of <= 4x4 tiles per
    workgroup, the input channels split four ways, the same reduction kernel as tile_cfg 90 / 91 (bias, embedding, residual,
    ReLU, GroupNorm partials).  Same bound as the f32 forms; batches that are not a multiple of four leave images empty."""
    x = _rand(B, c0, H, W, seed=390)
    x2 = _rand(B, c1, H, W, seed=391) if c1 else None
    w = _rand(cout, c0 + c1, 3, 3, seed=392, scale=(9 * (c0 + c1)) ** -0.5)
    b = _rand(cout, seed=393)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=394), 0.3 * _rand(B, c0 + c1, seed=395))
    cb = _rand(B, cout, seed=396)
    res = _rand(B, cout, H, W, seed=397)
    for kw in (dict(bias=b, x2=x2, gn=gn, gn_silu=True, chan_bias=cb, residual=res), dict(bias=b, x2=x2, relu=True),
               dict(bias=b, x2=x2, gn=gn, gn_silu=False)):
        _close(_run_wino(x, w, 92, **kw), _conv_ref(x, w, **kw), tol=KTOL, what="winograd bf16x3 K-split, four images")
    from synt_isic_amd import ops
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, 3, bias=d(b), x2=d(x2), residual=d(res), tile_cfg=92,
                       w_winograd=ops.pack_winograd_weight(d(w)), with_stats=True)
    assert st is not None and tuple(st.shape) == (B, cout, 1, 4)
    G = 2 if cout % 32 else 32
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=398), 0.1 * _rand(cout, seed=399)
    sc, sh = ops.groupnorm_finalize(st, H * W, d(gamma), d(beta), G, 1e-5)
    yc = y.cpu().double()
    ref = F.group_norm(yc, G, gamma.double(), beta.double(), 1e-5)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="groupnorm from the K-split reduction, bf16x3")


def test_conv3x3_winograd_reference_layers_and_identity():
    # identity filter: the transform pair must reproduce the input up to fp32 rounding of the 1/2, 1/4 weights
    C = 64
    x = _rand(1, C, 16, 16, seed=123)
    w = torch.zeros(C, C, 3, 3)
    for c in range(C):
        w[c, c, 1, 1] = 1.0
    _close(_run_wino(x, w, 60), x.double(), tol=1e-6, what="winograd identity")
    for i, (cin, cout, r) in enumerate([(64, 64, 64), (192, 64, 64), (384, 128, 32), (512, 256, 16), (3, 64, 64)]):
        xx = _rand(1, cin, r, r, seed=130 + i)
        ww = _rand(cout, cin, 3, 3, seed=140 + i, scale=(cin * 9) ** -0.5)
        bb = _rand(cout, seed=150 + i, scale=0.1)
        outs = {}
        for cfg in (60, 62, 66, 70, 71, 72, 73, 74):   # 74: the bf16x3 form -- same bound, other bits
            outs[cfg] = _run_wino(xx, ww, cfg, bias=bb)
            _close(outs[cfg], _conv_ref(xx, ww, bb), what=f"winograd{cfg} layer {cin}->{cout}@{r}")
        # the second geometry (filters from global memory into registers, 32 tiles per workgroup; 72 / 73) and the third
        # (a wave owns a column of the position grid, half of the output transform on the accumulators; 70 / 71) perform
        # the same fp32 operations in the same order as the first: identical bits
        for cfg in (70, 71, 72, 73):
            assert torch.equal(outs[cfg], outs[66]), cfg
        # ... and with every fused feature (prologue, concat seam, embedding, residual, ReLU), ragged planes included
        B2, H2, W2 = 2, r, max(8, r - 6)
        x1, x2 = _rand(B2, cin, H2, W2, seed=160 + i), _rand(B2, 24, H2, W2, seed=170 + i)
        w2 = _rand(cout, cin + 24, 3, 3, seed=180 + i, scale=(cin * 9) ** -0.5)
        gn = (1.0 + 0.3 * _rand(B2, cin + 24, seed=181 + i), 0.3 * _rand(B2, cin + 24, seed=182 + i))
        kw = dict(bias=bb, x2=x2, gn=gn, gn_silu=True, chan_bias=_rand(B2, cout, seed=183 + i),
                  residual=_rand(B2, cout, H2, W2, seed=184 + i), relu=bool(i & 1))
        fused = {cfg: _run_wino(x1, w2, cfg, **kw) for cfg in (66, 70, 71, 72, 73)}
        for cfg in (70, 71, 72, 73):
            assert torch.equal(fused[cfg], fused[66]), ("fused", cfg)
        _close(_run_wino(x1, w2, 74, **kw), _conv_ref(x1, w2, **kw), tol=KTOL, what=f"winograd74 fused layer {cin}+24->{cout}@{r}")
    from synt_isic_amd import ops
    from synt_isic_amd._lib import SisicError
    with pytest.raises(SisicError, match="w_winograd"):
        ops.conv2d(x.to(DEV), ops.pack_conv_weight(w.to(DEV)), C, 3, tile_cfg=60)


def test_gn_prologue_keeps_padding_zero():
    """Zero padding is applied AFTER GroupNorm+SiLU: a constant shift must not leak into the border."""
    x = torch.zeros(1, 8, 8, 8)
    w = torch.ones(64, 8, 3, 3)
    gn = (torch.ones(1, 8), torch.full((1, 8), 2.0))
    got = _run_conv(x, w, 4, gn=gn, gn_silu=False).cpu()
    assert got[0, 0, 4, 4].item() == pytest.approx(8 * 9 * 2.0)
    assert got[0, 0, 0, 0].item() == pytest.approx(8 * 4 * 2.0)     # corner sees 4 in-bounds taps only


@pytest.mark.parametrize("cfg,H,W", [(0, 32, 32), (0, 16, 16), (0, 8, 8), (1, 32, 32), (2, 16, 16), (3, 8, 8), (4, 4, 4),
                                     (2, 10, 14)])
def test_conv3x3_upsample(cfg, H, W):
    x = _rand(2, 24, H, W, seed=16)
    w = _rand(64, 24, 3, 3, seed=17, scale=0.1)
    b = _rand(64, seed=18)
    _close(_run_conv(x, w, cfg, bias=b, upsample=True), _conv_ref(x, w, b, upsample=True),
           what=f"upsample conv cfg{cfg} {H}x{W}")


@pytest.mark.parametrize("cfg,H,W", [(0, 64, 64), (0, 32, 32), (0, 16, 16), (11, 64, 64), (12, 32, 32), (13, 16, 16),
                                     (11, 20, 36), (13, 6, 10), (18, 16, 16), (18, 20, 36), (19, 32, 32), (19, 6, 10)])
def test_conv3x3_stride2(cfg, H, W):
    x = _rand(2, 16, H, W, seed=19)
    w = _rand(64, 16, 3, 3, seed=20, scale=0.1)
    b = _rand(64, seed=21)
    _close(_run_conv(x, w, cfg, bias=b, stride=2), _conv_ref(x, w, b, stride=2), what=f"stride-2 conv cfg{cfg}")


@pytest.mark.parametrize("cfg,H,W", [(0, 16, 16), (0, 8, 8), (21, 16, 16), (21, 9, 7), (22, 8, 8), (22, 5, 5),
                                     (23, 16, 16), (23, 12, 20), (24, 16, 16), (24, 9, 7), (25, 16, 16), (25, 12, 20),
                                     (26, 32, 32), (27, 8, 8)])
def test_conv1x1(cfg, H, W):
    B, c0, c1, cout = 2, 40, 24, 96
    x, x2 = _rand(B, c0, H, W, seed=22), _rand(B, c1, H, W, seed=23)
    w = _rand(cout, c0 + c1, 1, 1, seed=24, scale=0.2)
    b = _rand(cout, seed=25)
    res = _rand(B, cout, H, W, seed=26)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=27), 0.3 * _rand(B, c0 + c1, seed=28))
    _close(_run_conv(x, w, cfg, bias=b, x2=x2), _conv_ref(x, w, b, x2=x2), what=f"conv1x1 cfg{cfg}")
    kw = dict(bias=b, x2=x2, gn=gn, gn_silu=False, residual=res)
    _close(_run_conv(x, w, cfg, **kw), _conv_ref(x, w, **kw), what=f"conv1x1 fused cfg{cfg}")


@pytest.mark.parametrize("B,c0,c1,cout,H,W", [(2, 64, 0, 128, 32, 32), (3, 128, 64, 64, 16, 16), (2, 256, 128, 128, 8, 16),
                                              (2, 256, 0, 768, 16, 16), (1, 32, 32, 70, 16, 24), (2, 96, 0, 200, 16, 8)])
def test_conv1x1_pointwise(B, c0, c1, cout, H, W):
    """tile_cfg 20 (conv_pointwise.hip): the lean 1x1 kernel -- filters straight into registers from their second packing,
    32-channel chunks of the input through LDS -- against the float64 convolution with every fused feature, bit-equal to
    the generic kernel (same FMA chain in the same channel order), and refusing ragged shapes."""
    from synt_isic_amd import ops
    x = _rand(B, c0, H, W, seed=400)
    x2 = _rand(B, c1, H, W, seed=401) if c1 else None
    w = _rand(cout, c0 + c1, 1, 1, seed=402, scale=(c0 + c1) ** -0.5)
    b = _rand(cout, seed=403)
    res = _rand(B, cout, H, W, seed=404)
    cb = _rand(B, cout, seed=405)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=406), 0.3 * _rand(B, c0 + c1, seed=407))
    for kw in (dict(bias=b, x2=x2), dict(bias=b, x2=x2, gn=gn, gn_silu=False, residual=res),
               dict(x2=x2, gn=gn, gn_silu=True, chan_bias=cb, relu=True)):
        y = _run_conv(x, w, 20, **kw)
        _close(y, _conv_ref(x, w, **kw), what="pointwise conv1x1")
        assert torch.equal(y, _run_conv(x, w, 25, **kw))
        # the auto dispatch: the bf16x3 kernel (tile_cfg 28) where its 64-pixel x 64-channel tiles are whole, this one otherwise
        #   (and its K-split form, tile_cfg 35, for the small levels' layers -- a rule of the layer's shape alone)
        bf3 = cout % 64 == 0 and (H * W) % 64 == 0 and (c0 + c1) % 8 == 0 and c0 % 8 == 0
        ksplit = bf3 and H * W <= 256 and cout <= 256 and (c0 + c1) % 128 == 0
        assert torch.equal(_run_conv(x, w, 0, **kw), _run_conv(x, w, 35 if ksplit else 28, **kw) if bf3 else y)
    # GroupNorm partials of the result: one slot per 32 pixels
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, 1, bias=d(b), x2=d(x2), residual=d(res), tile_cfg=20, with_stats=True)
    assert st is not None and tuple(st.shape) == (B, cout, H * W // 32, 4)
    G = 2 if cout % 32 else 32
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=408), 0.1 * _rand(cout, seed=409)
    sc, sh = ops.groupnorm_finalize(st, H * W, d(gamma), d(beta), G, 1e-5)
    yc = y.cpu().double()
    ref = F.group_norm(yc, G, gamma.double(), beta.double(), 1e-5)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="groupnorm from the pointwise kernel's partials")
    from synt_isic_amd._lib import SisicError
    with pytest.raises(SisicError, match="pointwise"):
        _run_conv(_rand(1, 40, 8, 8, seed=410), _rand(64, 40, 1, 1, seed=411), 20)       # 40 channels, 64 pixels


@pytest.mark.parametrize("B,c0,c1,cout,H,W", [(2, 64, 0, 128, 32, 32), (3, 128, 64, 64, 16, 16), (2, 256, 128, 128, 8, 16),
                                              (2, 256, 0, 768, 16, 16), (1, 8, 0, 64, 8, 8), (2, 40, 24, 192, 8, 24)])
def test_conv1x1_pointwise_bf16x3(B, c0, c1, cout, H, W):
    """tile_cfg 28 (conv_pointwise_bf3.hip): the 1x1 GEMM with fp32-equivalent products on the bf16 matrix pipe (three exact
    bf16 terms per operand, six products, fp32 accumulate) -- against the float64 convolution with every fused feature at the
    SAME bound as the f32 kernels, its GroupNorm partials, and refusing ragged shapes."""
    from synt_isic_amd import ops
    x = _rand(B, c0, H, W, seed=420)
    x2 = _rand(B, c1, H, W, seed=421) if c1 else None
    w = _rand(cout, c0 + c1, 1, 1, seed=422, scale=(c0 + c1) ** -0.5)
    b = _rand(cout, seed=423)
    res = _rand(B, cout, H, W, seed=424)
    cb = _rand(B, cout, seed=425)
    gn = (1.0 + 0.3 * _rand(B, c0 + c1, seed=426), 0.3 * _rand(B, c0 + c1, seed=427))
    for kw in (dict(bias=b, x2=x2), dict(bias=b, x2=x2, gn=gn, gn_silu=False, residual=res),
               dict(x2=x2, gn=gn, gn_silu=True, chan_bias=cb, relu=True)):
        _close(_run_conv(x, w, 28, **kw), _conv_ref(x, w, **kw), what="bf16x3 pointwise conv1x1")
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, 1, bias=d(b), x2=d(x2), residual=d(res), tile_cfg=28, with_stats=True)
    assert st is not None and tuple(st.shape) == (B, cout, H * W // 32, 4)
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=428), 0.1 * _rand(cout, seed=429)
    sc, sh = ops.groupnorm_finalize(st, H * W, d(gamma), d(beta), 32, 1e-5)
    yc = y.cpu().double()
    ref = F.group_norm(yc, 32, gamma.double(), beta.double(), 1e-5)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="groupnorm from the bf16x3 pointwise kernel's partials")
    from synt_isic_amd._lib import SisicError
    with pytest.raises(SisicError, match="pointwise bf16x3"):
        _run_conv(_rand(1, 40, 8, 8, seed=430), _rand(70, 40, 1, 1, seed=431), 28)       # 70 output channels


@pytest.mark.parametrize("cin", [8, 16, 24, 40, 48, 56, 72, 104])
def test_bf16x3_kernels_every_loop_tail(cin):
    """The channel loops of the two bf16x3 kernels are unrolled and software-pipelined (Winograd: first body, pairs of steady
    bodies, up to four tail bodies; pointwise: operands a chunk ahead, two bodies per iteration): 1, 2, 3, 5, 6, 7, 9 and 13
    chunks of eight channels go through every entry and exit of them."""
    x = _rand(2, cin, 16, 16, seed=450 + cin)
    gn = (1.0 + 0.3 * _rand(2, cin, seed=451 + cin), 0.3 * _rand(2, cin, seed=452 + cin))
    w3 = _rand(64, cin, 3, 3, seed=453 + cin, scale=(9 * cin) ** -0.5)
    w1 = _rand(128, cin, 1, 1, seed=454 + cin, scale=cin ** -0.5)
    b3, b1 = _rand(64, seed=455), _rand(128, seed=456)
    for cfg in (74,):
        _close(_run_wino(x, w3, cfg, bias=b3, gn=gn, gn_silu=True), _conv_ref(x, w3, bias=b3, gn=gn, gn_silu=True), tol=KTOL,
               what=f"winograd{cfg} {cin} channels")
    for cfg in (29, 30):
        _close(_run_conv(x, w1, cfg, bias=b1, gn=gn, gn_silu=False), _conv_ref(x, w1, bias=b1, gn=gn, gn_silu=False),
               what=f"bf16x3 pointwise cfg{cfg} {cin} channels")


def _rel_close(got, ref64, what):
    """the bf16x3 bound WITHOUT the max(1, .) floor: error relative to the largest reference output, whatever its magnitude"""
    got = got.detach().cpu().double()
    top = ref64.abs().max().item()
    err = (got - ref64).abs().max().item()
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(f"{err / top:.3e}\t{KTOL:.1e}\t{what}\n")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= KTOL * top, f"{what}: max abs err {err:.3e} > {KTOL} * {top:.3e}"


BF3_CASES = [(74, 3, 2, 32, 32, 72, 64),      # (tile_cfg, ksize, B, H, W, Cin, Cout): Winograd, 16x16-pixel tiles
             (92, 3, 4, 8, 8, 128, 64),       # the 8x8 level: four images per workgroup, channels split four ways
             (28, 1, 2, 16, 16, 136, 128)]    # pointwise


def _bf3_run(cfg, k, x, w, **kw):
    return _run_wino(x, w, cfg, **kw) if k == 3 else _run_conv(x, w, cfg, **kw)


@pytest.mark.parametrize("cfg,k,B,H,W,cin,cout", BF3_CASES)
def test_bf16x3_scale_sweep(cfg, k, B, H, W, cin, cout):
    """the domain of the "fp32-equivalent" bf16x3 kernels.  A bf16 term keeps fp32's exponent, so the exact
    three-term split holds at every magnitude: inputs and weights scaled by 1e-6 ... 1e4 (products from 1e-12 to 1e8 of the
    O(1) case) and magnitudes mixed over eight decades INSIDE one reduction meet the same bound as the O(1) tests -- taken
    relative to the largest output (no max(1, .) floor)."""
    x0 = _rand(B, cin, H, W, seed=900 + cfg)
    w0 = _rand(cout, cin, k, k, seed=901 + cfg, scale=(k * k * cin) ** -0.5)
    b0 = _rand(cout, seed=902 + cfg)
    for sx, sw in itertools.product((1e-6, 1e-3, 1e3, 1e4), repeat=2):
        x, w, b = x0 * sx, w0 * sw, b0 * (sx * sw)
        _rel_close(_bf3_run(cfg, k, x, w, bias=b), _conv_ref(x, w, b), f"bf16x3 cfg{cfg} inputs x{sx:g} weights x{sw:g}")
    # eight decades inside one reduction: channel c of the input carries magnitude 10^e_c, e_c uniform in [-4, 4] ...
    g = torch.Generator().manual_seed(903 + cfg)
    mag = 10.0 ** (8.0 * torch.rand(cin, generator=g) - 4.0)
    xm = x0 * mag[None, :, None, None]
    _rel_close(_bf3_run(cfg, k, xm, w0, bias=b0), _conv_ref(xm, w0, b0), f"bf16x3 cfg{cfg} channel magnitudes 1e-4..1e4")
    # ... and with the weights carrying the inverse magnitudes, so that every channel contributes O(1)
    wm = w0 / mag[None, :, None, None]
    _rel_close(_bf3_run(cfg, k, xm, wm, bias=b0), _conv_ref(xm, wm, b0), f"bf16x3 cfg{cfg} compensated magnitudes")
    # magnitudes mixed pixel by pixel (what the Winograd input transform adds together before the split)
    pm = 10.0 ** (8.0 * torch.rand(B, 1, H, W, generator=g) - 4.0)
    xp = x0 * pm
    _rel_close(_bf3_run(cfg, k, xp, w0, bias=b0), _conv_ref(xp, w0, b0), f"bf16x3 cfg{cfg} pixel magnitudes 1e-4..1e4")


@pytest.mark.parametrize("cfg,k,B,H,W,cin,cout", BF3_CASES)
def test_bf16x3_non_finite_inputs(cfg, k, B, H, W, cin, cout):
    """What +-Inf / NaN inputs produce against F.conv2d: the split computes x - hi, which is NaN for an
    infinite x, so every output that fp32 arithmetic makes +-Inf or NaN is NaN here -- never a finite number -- and every
    output that does not depend on the poisoned input keeps its bits.  That also holds for the Winograd kernels: a patch
    element enters exactly the positions of V whose products reach the outputs with that element in their 3 x 3 window."""
    x = _rand(B, cin, H, W, seed=910 + cfg)
    w = _rand(cout, cin, k, k, seed=911 + cfg, scale=(k * k * cin) ** -0.5)
    clean = _bf3_run(cfg, k, x, w).cpu()
    for (py, px), bad in itertools.product(((5, 2), (0, 0), (H - 1, 3), (2, W - 1)), (float("inf"), float("-inf"), float("nan"))):
        xb = x.clone()
        xb[0, 3, py, px] = bad
        got = _bf3_run(cfg, k, xb, w).cpu()
        dep = ~torch.isfinite(F.conv2d(xb, w, padding=k // 2))          # the outputs fp32 arithmetic makes +-Inf / NaN
        win = torch.zeros(B, cout, H, W, dtype=torch.bool)
        win[0, :, max(0, py - k // 2):py + k // 2 + 1, max(0, px - k // 2):px + k // 2 + 1] = True
        assert torch.equal(dep, win)                                    # (= the k x k window around the pixel, every channel)
        assert torch.isnan(got[dep]).all(), f"cfg{cfg} {bad} at {(py, px)}: a non-finite reference output came out finite"
        assert torch.equal(got[~dep], clean[~dep]), f"cfg{cfg} {bad} at {(py, px)}: an output outside the window changed"
    # a NaN weight poisons its output channel only
    wb = w.clone()
    wb[7, 1, 0, 0] = float("nan")
    got = _bf3_run(cfg, k, x, wb).cpu()
    assert torch.isnan(got[:, 7]).all() and torch.equal(got[:, :7], clean[:, :7]) and torch.equal(got[:, 8:], clean[:, 8:])


def test_conv1x1_pointwise_bf16x3_item_width_does_not_change_bits():
    """The kernel gives a wave 64 pixels when that still leaves every SIMD two waves, 32 otherwise -- a choice that
    depends on the batch.  An image's bits must not: the same image alone (32-pixel items) and inside a batch of 16
    (64-pixel items) comes out bit-equal."""
    B, cin, cout, H, W = 16, 64, 512, 32, 32            # 16 x 16 x 8 = 2048 wide items
    x = _rand(B, cin, H, W, seed=440)
    w = _rand(cout, cin, 1, 1, seed=441, scale=cin ** -0.5)
    b = _rand(cout, seed=442)
    gn = (1.0 + 0.3 * _rand(B, cin, seed=443), 0.3 * _rand(B, cin, seed=444))
    y = _run_conv(x, w, 28, bias=b, gn=gn, gn_silu=False)
    y0 = _run_conv(x[:1].contiguous(), w, 28, bias=b, gn=(gn[0][:1].contiguous(), gn[1][:1].contiguous()), gn_silu=False)
    assert torch.equal(y[:1], y0)
    _close(y, _conv_ref(x, w, bias=b, gn=gn, gn_silu=False), what="bf16x3 pointwise conv1x1, wide items")
    # ... and neither do its GroupNorm partials (they decide the next layer's normalisation): slot = 32 consecutive pixels,
    # one summation tree in both forms
    from synt_isic_amd import ops
    d = lambda t: t.to(DEV).contiguous()
    wp = ops.pack_conv_weight(d(w))
    _, st = ops.conv2d(d(x), wp, cout, 1, bias=d(b), tile_cfg=28, with_stats=True)
    _, st0 = ops.conv2d(d(x[:1]), wp, cout, 1, bias=d(b), tile_cfg=28, with_stats=True)
    assert torch.equal(st[:1], st0)
    # the two forms forced (tile_cfg 29: 32 pixels per wave, 30: 64) on one input, every fused feature
    res, cb = d(_rand(B, cout, H, W, seed=445)), d(_rand(B, cout, seed=446))
    for kw in (dict(), dict(residual=res, relu=True), dict(chan_bias=cb, gn_scale=d(gn[0]), gn_shift=d(gn[1]), gn_silu=True)):
        ya, sa = ops.conv2d(d(x), wp, cout, 1, bias=d(b), tile_cfg=29, with_stats=True, **kw)
        yb, sb = ops.conv2d(d(x), wp, cout, 1, bias=d(b), tile_cfg=30, with_stats=True, **kw)
        assert torch.equal(ya, yb) and torch.equal(sa, sb)
        # ... and the staged form (tile_cfg 34: the pixels' operands split once per workgroup into LDS, a wave per channel item)
        yc, sc = ops.conv2d(d(x), wp, cout, 1, bias=d(b), tile_cfg=34, with_stats=True, **kw)
        assert torch.equal(ya, yc) and torch.equal(sa, sc)


def test_conv1x1_pointwise_bf16x3_staged_qkv_shape():
    """The attention blocks' q, k, v projection (256 -> 768 at 16x16 behind a GroupNorm): the staged form against float64 and,
    bit for bit, against the per-wave form it replaces; a concatenated input as well (the seam on a chunk boundary)."""
    from synt_isic_amd import ops
    d = lambda t: t.to(DEV).contiguous()
    for (c0, c1, cout, H, W, B) in ((256, 0, 768, 16, 16, 3), (128, 64, 384, 8, 16, 2)):
        cin = c0 + c1
        x, x2 = _rand(B, c0, H, W, seed=460), (_rand(B, c1, H, W, seed=461) if c1 else None)
        w = _rand(cout, cin, 1, 1, seed=462, scale=cin ** -0.5)
        b = _rand(cout, seed=463)
        gn = (1.0 + 0.3 * _rand(B, cin, seed=464), 0.3 * _rand(B, cin, seed=465))
        xx = x if x2 is None else torch.cat([x, x2], 1)
        ref = _conv_ref(xx, w, bias=b, gn=gn, gn_silu=False)
        wp = ops.pack_conv_weight(d(w))
        kw = dict(bias=d(b), x2=None if x2 is None else d(x2), gn_scale=d(gn[0]), gn_shift=d(gn[1]), gn_silu=False, with_stats=True)
        ys, ss = ops.conv2d(d(x), wp, cout, 1, tile_cfg=34, **kw)
        yw, sw = ops.conv2d(d(x), wp, cout, 1, tile_cfg=30, **kw)
        _close(ys, ref, what=f"staged bf16x3 pointwise {cin}->{cout}")
        assert torch.equal(ys, yw) and torch.equal(ss, sw)


def test_conv1x1_pointwise_bf16x3_ksplit():
    """tile_cfg 35 (the small levels' 1x1 layers: a workgroup's four waves split the input channels): against float64 with every
    fused feature; the GroupNorm partials against the stored tensor's statistics; and an image's bits do not depend on its batch
    (the form is chosen by layer shape, its summation order is fixed)."""
    from synt_isic_amd import ops
    d = lambda t: t.to(DEV).contiguous()
    for (c0, c1, cout, H, W, B) in ((256, 0, 256, 16, 16, 3), (256, 256, 256, 8, 8, 4), (128, 0, 192, 8, 16, 2)):
        cin = c0 + c1
        x, x2 = _rand(B, c0, H, W, seed=470), (_rand(B, c1, H, W, seed=471) if c1 else None)
        xx = x if x2 is None else torch.cat([x, x2], 1)
        w = _rand(cout, cin, 1, 1, seed=472, scale=cin ** -0.5)
        b, res, cb = _rand(cout, seed=473), _rand(B, cout, H, W, seed=474), _rand(B, cout, seed=475)
        gn = (1.0 + 0.3 * _rand(B, cin, seed=476), 0.3 * _rand(B, cin, seed=477))
        wp = ops.pack_conv_weight(d(w))
        x2d = None if x2 is None else d(x2)
        for kw, rkw in ((dict(), dict()),
                        (dict(residual=d(res), relu=True), dict(residual=res, relu=True)),
                        (dict(chan_bias=d(cb), gn_scale=d(gn[0]), gn_shift=d(gn[1]), gn_silu=True), dict(chan_bias=cb, gn=gn, gn_silu=True))):
            y, st = ops.conv2d(d(x), wp, cout, 1, bias=d(b), x2=x2d, tile_cfg=35, with_stats=True, **kw)
            _close(y, _conv_ref(xx, w, bias=b, **rkw), what=f"K-split bf16x3 pointwise {cin}->{cout}@{H}x{W} {sorted(kw)}")
            y1, st1 = ops.conv2d(d(x[1:2]), wp, cout, 1, bias=d(b), x2=None if x2 is None else d(x2[1:2]), tile_cfg=35, with_stats=True,
                                 **{k: (v[1:2].contiguous() if torch.is_tensor(v) else v) for k, v in kw.items()})
            assert torch.equal(y[1:2], y1) and torch.equal(st[1:2], st1)
            # partials: slot = 32 consecutive pixels: (32, sum, centred sum of squares)
            yv = y.double().cpu().reshape(B, cout, -1, 32)
            assert torch.allclose(st[..., 1].double().cpu(), yv.sum(-1), rtol=1e-5, atol=1e-4)
            assert torch.allclose(st[..., 2].double().cpu(), ((yv - yv.mean(-1, keepdim=True)) ** 2).sum(-1), rtol=1e-4, atol=1e-4)


def test_conv_reference_layer_shapes():
    """The distinct (Cin, Cout, resolution) classes of the reference UNet at 64x64, B=1."""
    shapes = [(3, 64, 64), (64, 64, 64), (192, 64, 64), (128, 128, 32), (384, 128, 32), (256, 256, 16),
              (512, 256, 16), (256, 256, 8), (512, 256, 8), (64, 3, 64)]
    for i, (cin, cout, r) in enumerate(shapes):
        x = _rand(1, cin, r, r, seed=100 + i)
        w = _rand(cout, cin, 3, 3, seed=200 + i, scale=(cin * 9) ** -0.5)
        b = _rand(cout, seed=300 + i, scale=0.1)
        _close(_run_conv(x, w, 0, bias=b), _conv_ref(x, w, b), what=f"layer {cin}->{cout}@{r}")


def test_conv_argument_errors():
    from synt_isic_amd import ops
    from synt_isic_amd._lib import SisicError
    x = _rand(1, 8, 8, 8).to(DEV)
    wp = ops.pack_conv_weight(_rand(64, 8, 3, 3).to(DEV))
    with pytest.raises(SisicError, match="tile_cfg"):
        ops.conv2d(x, wp, 64, 3, tile_cfg=99)
    with pytest.raises(SisicError, match="stride"):
        ops.conv2d(x, wp, 64, 3, stride=3)
    with pytest.raises(ValueError):
        ops.conv2d(x.double(), wp, 64, 3)
    with pytest.raises(ValueError):
        ops.pack_conv_weight(_rand(64, 8, 5, 5).to(DEV))


# ---------------------------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize("c0,c1,H,W", [(64, 0, 64, 64), (256, 128, 16, 16), (128, 64, 32, 32), (512, 0, 8, 8),
                                       (64, 0, 9, 7), (96, 32, 5, 3)])
def test_groupnorm_stats(c0, c1, H, W):
    from synt_isic_amd import ops
    B, G, eps = 3, 32, 1e-5
    x = _rand(B, c0, H, W, seed=30) * 2.0 + 0.7
    x2 = (_rand(B, c1, H, W, seed=31) - 1.5) if c1 else None
    C = c0 + c1
    gamma, beta = 1.0 + 0.1 * _rand(C, seed=32), 0.1 * _rand(C, seed=33)
    sc, sh = ops.groupnorm_stats(x.to(DEV), gamma.to(DEV), beta.to(DEV), G, eps, x2.to(DEV) if c1 else None)
    full = (torch.cat([x, x2], 1) if c1 else x).double()
    ref = F.group_norm(full, G, gamma.double(), beta.double(), eps)
    got = full * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="groupnorm apply")
    # the fused consumer: conv(SiLU(GN(x))) == oracle composition
    w = _rand(64, C, 3, 3, seed=34, scale=0.05)
    wp = ops.pack_conv_weight(w.to(DEV))
    y = ops.conv2d(x.to(DEV), wp, 64, 3, x2=x2.to(DEV) if c1 else None, gn_scale=sc, gn_shift=sh, gn_silu=True)
    _close(y, F.conv2d(F.silu(ref), w.double(), padding=1), tol=KTOL, what="GN+SiLU+conv")


def test_groupnorm_large_mean_is_stable():
    """two-pass variance: |mean| >> std must not lose the variance (E[x^2]-mean^2 would)."""
    from synt_isic_amd import ops
    x = _rand(1, 32, 16, 16, seed=35) * 1e-2 + 100.0
    gamma, beta = torch.ones(32), torch.zeros(32)
    sc, sh = ops.groupnorm_stats(x.to(DEV), gamma.to(DEV), beta.to(DEV), 32, 1e-5)
    ref = F.group_norm(x.double(), 32, eps=1e-5)
    got = x.double() * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    assert (got - ref).abs().max().item() < 5e-3      # fp32 input quantisation at |x|=100 dominates


@pytest.mark.parametrize("cfg,B,H,W,ups", [(66, 3, 32, 32, False), (62, 2, 18, 10, False), (60, 2, 9, 23, False),
                                           (64, 2, 16, 16, True), (61, 5, 8, 8, False), (67, 3, 6, 10, False),
                                           (0, 2, 64, 64, False), (68, 3, 32, 32, False), (68, 2, 18, 10, False),
                                           (69, 2, 9, 23, False), (69, 2, 32, 48, False), (78, 2, 16, 16, False),
                                           (79, 2, 18, 10, False), (72, 3, 32, 32, False), (73, 2, 9, 23, False),
                                           (70, 2, 18, 10, False), (71, 2, 32, 48, False), (74, 3, 32, 32, False),
                                           (74, 2, 18, 10, False)])
def test_conv_epilogue_groupnorm_partials(cfg, B, H, W, ups):
    """sisic_conv_args.stats_out: the Winograd output transform leaves (count, sum, centred M2) per image, channel and
    workgroup tile; sisic_groupnorm_finalize on them == sisic_groupnorm_stats on the stored tensor."""
    from synt_isic_amd import ops
    cin, cout, G, eps = 24, 96, 32, 1e-5
    x = _rand(B, cin, H, W, seed=160)
    w = _rand(cout, cin, 3, 3, seed=161, scale=0.1)
    b = 3.0 * _rand(cout, seed=162)
    res = _rand(B, cout, 2 * H if ups else H, 2 * W if ups else W, seed=163)
    d = lambda t: t.to(DEV).contiguous()
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, 3, bias=d(b), residual=d(res), upsample=ups,
                       tile_cfg=cfg, w_winograd=ops.pack_winograd_weight(d(w)), with_stats=True)
    assert st is not None and st.shape[:2] == (B, cout) and st.shape[3] == 4
    yc, stc = y.cpu().double(), st.cpu().double()
    n, s1, m2 = stc[..., 0].sum(-1), stc[..., 1].sum(-1), stc[..., 2]
    assert torch.equal(n, torch.full_like(n, yc.shape[2] * yc.shape[3]))
    _close(s1.float(), yc.sum((2, 3)), tol=1e-5, what="partial sums")
    mean_i = stc[..., 1] / stc[..., 0].clamp(min=1)
    mean = (s1 / n)[..., None]
    m2_tot = m2.sum(-1) + (stc[..., 0] * (mean_i - mean) ** 2).sum(-1)
    _close(m2_tot.float(), ((yc - yc.mean((2, 3), keepdim=True)) ** 2).sum((2, 3)), tol=1e-5, what="merged M2")
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=164), 0.1 * _rand(cout, seed=165)
    sc, sh = ops.groupnorm_finalize(st, yc.shape[2] * yc.shape[3], d(gamma), d(beta), G, eps)
    sc0, sh0 = ops.groupnorm_stats(y, d(gamma), d(beta), G, eps)
    _close(sc, sc0.cpu().double(), tol=2e-6, what="finalize scale")
    _close(sh, sh0.cpu().double(), tol=2e-6, what="finalize shift")
    ref = F.group_norm(yc, G, gamma.double(), beta.double(), eps)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="groupnorm from partials")
    # launches that cannot produce partials say so instead of writing nothing (vector-ALU kernel for Cout <= 4)
    y2, st2 = ops.conv2d(d(x), ops.pack_conv_weight(d(w[:3].contiguous())), 3, 3, with_stats=True)
    assert st2 is None


@pytest.mark.parametrize("ksize,stride,cfg,B,H,W", [(3, 1, 16, 3, 8, 8), (3, 1, 8, 2, 32, 32), (3, 1, 9, 2, 18, 10), (3, 1, 1, 1, 64, 64),
                                                    (3, 2, 11, 2, 64, 64), (3, 2, 13, 2, 16, 16), (3, 2, 0, 2, 30, 22),
                                                    (1, 1, 24, 2, 32, 32), (1, 1, 25, 2, 16, 16), (1, 1, 22, 3, 8, 8), (1, 1, 0, 2, 9, 23)])
def test_direct_conv_epilogue_groupnorm_partials(ksize, stride, cfg, B, H, W):
    """the direct MFMA kernel's partials (one slot per pixel tile and pixel-wave) -> same GroupNorm as the pass over
    the stored tensor; Cout = 70 leaves a partly filled channel tile."""
    from synt_isic_amd import ops
    cin, cout, G, eps = 24, 70, 35, 1e-5
    x = _rand(B, cin, H, W, seed=180)
    w = _rand(cout, cin, ksize, ksize, seed=181, scale=0.1)
    b = 2.0 * _rand(cout, seed=182)
    d = lambda t: t.to(DEV).contiguous()
    Ho, Wo = (H + 2 * (ksize // 2) - ksize) // stride + 1, (W + 2 * (ksize // 2) - ksize) // stride + 1
    res = _rand(B, cout, Ho, Wo, seed=183)
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, ksize, bias=d(b), residual=d(res), stride=stride,
                       tile_cfg=cfg, with_stats=True)
    assert st is not None and st.shape[:2] == (B, cout)
    yc, stc = y.cpu().double(), st.cpu().double()
    assert torch.equal(stc[..., 0].sum(-1), torch.full((B, cout), float(Ho * Wo), dtype=torch.float64))
    _close(stc[..., 1].sum(-1).float(), yc.sum((2, 3)), tol=1e-5, what="partial sums")
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=184), 0.1 * _rand(cout, seed=185)
    sc, sh = ops.groupnorm_finalize(st, Ho * Wo, d(gamma), d(beta), G, eps)
    ref = F.group_norm(yc, G, gamma.double(), beta.double(), eps)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what=f"groupnorm from direct-conv partials k{ksize} s{stride} cfg{cfg}")


def test_groupnorm_finalize_concat_and_large_mean():
    """two producers with different slot counts and a group that straddles the seam (18 + 14 channels in 8 groups of
    4); and |mean| >> std, where raw second moments would lose the variance."""
    from synt_isic_amd import ops
    d = lambda t: t.to(DEV).contiguous()
    B, G, eps = 2, 8, 1e-5
    xa = _rand(B, 16, 32, 32, seed=170)
    xb = _rand(B, 16, 32, 32, seed=171)
    wa, wb = _rand(18, 16, 3, 3, seed=172, scale=0.1), _rand(14, 16, 3, 3, seed=173, scale=0.1)   # group 4 = channels 16..19 straddles
    ya, sa = ops.conv2d(d(xa), ops.pack_conv_weight(d(wa)), 18, 3, tile_cfg=66, w_winograd=ops.pack_winograd_weight(d(wa)), with_stats=True)
    yb, sb = ops.conv2d(d(xb), ops.pack_conv_weight(d(wb)), 14, 3, tile_cfg=67, w_winograd=ops.pack_winograd_weight(d(wb)), with_stats=True)
    assert sa.shape[2] == 4 and sb.shape[2] == 16
    gamma, beta = 1.0 + 0.1 * _rand(32, seed=174), 0.1 * _rand(32, seed=175)
    sc, sh = ops.groupnorm_finalize(sa, 32 * 32, d(gamma), d(beta), G, eps, stats2=sb)
    full = torch.cat([ya, yb], 1).cpu().double()
    ref = F.group_norm(full, G, gamma.double(), beta.double(), eps)
    got = full * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    _close(got.float(), ref, tol=KTOL, what="concat groupnorm from partials")
    # identity filter + bias 100: output = 1e-2 * noise + 100
    C = 32
    x = _rand(1, C, 16, 16, seed=176) * 1e-2
    w = torch.zeros(C, C, 3, 3)
    for c in range(C):
        w[c, c, 1, 1] = 1.0
    y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), C, 3, bias=d(torch.full((C,), 100.0)), tile_cfg=66,
                       w_winograd=ops.pack_winograd_weight(d(w)), with_stats=True)
    sc, sh = ops.groupnorm_finalize(st, 256, d(torch.ones(C)), d(torch.zeros(C)), 32, eps)
    yc = y.cpu().double()
    ref = F.group_norm(yc, 32, eps=eps)
    got = yc * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]
    assert (got - ref).abs().max().item() < 5e-3


# ---------------------------------------------------------------------------------- attention
def _attn_ref(qkv, heads):
    B, C3, N = qkv.shape
    C = C3 // 3
    d = C // heads
    q, k, v = qkv.double().reshape(B, 3, heads, d, N).unbind(1)            # [B, heads, d, N]
    s = torch.einsum("bhdq,bhdk->bhqk", q, k) * d ** -0.5
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bhqk,bhdk->bhdq", p, v)
    return o.reshape(B, C, N)


@pytest.mark.parametrize("N", [64, 256, 100, 33, 1024, 300, 513])
def test_attention(N):
    from synt_isic_amd import ops
    B, C = 2, 256
    qkv = _rand(B, 3 * C, N, seed=40 + N) * 1.5
    got = ops.attention(qkv.to(DEV), 8)
    _close(got, _attn_ref(qkv, C // 8), tol=KTOL, what=f"attention N={N}")


@pytest.mark.parametrize("B,N", [(64, 64), (40, 256), (48, 100), (36, 300), (32, 1024), (33, 513)])
def test_attention_two_query_blocks_per_wave(B, N):
    """Large batches take attention_kernel<2> (64 queries per wave: a key's K operands and V values are read from LDS once
    for two query blocks).  Against float64, and every image equal bit for bit to the same image in a batch of two, which
    takes attention_kernel<1>: the form follows the batch, the bits must not."""
    from synt_isic_amd import ops
    C = 256
    assert B * (C // 8) * ((N + 255) // 256) >= 4 * 256, "the case must select the two-block form (launch_attention)"
    qkv = _rand(B, 3 * C, N, seed=940 + N) * 1.5
    got = ops.attention(qkv.to(DEV), 8)
    ref_idx = [0, B // 2, B - 1]
    _close(got[ref_idx], _attn_ref(qkv[ref_idx], C // 8), tol=KTOL, what=f"attention, two query blocks per wave, N={N}")
    for i in (0, B - 2):
        small = ops.attention(qkv[i:i + 2].to(DEV).contiguous(), 8)
        assert torch.equal(small, got[i:i + 2]), f"images {i}, {i + 1}: the two forms differ"


def test_attention_online_rescale_branch():
    """N > 256 runs the online softmax across key blocks; spike a key in the LAST block so the running
    maximum jumps there and everything accumulated before must be rescaled (and the reverse)."""
    from synt_isic_amd import ops
    B, C, N = 1, 64, 768
    for spike_at in (700, 5):
        qkv = _rand(B, 3 * C, N, seed=50) * 0.5
        qkv[:, C:2 * C, spike_at] *= 40.0            # one key with a huge norm
        got = ops.attention(qkv.to(DEV), 8)
        ref = _attn_ref(qkv, C // 8)
        assert torch.isfinite(got).all()
        _close(got, ref, tol=KTOL, what=f"attention spike at key {spike_at}")


def test_attention_rejects_other_head_dims():
    from synt_isic_amd import ops
    from synt_isic_amd._lib import SisicError
    with pytest.raises(SisicError, match="head_dim"):
        ops.attention(_rand(1, 3 * 64, 16).to(DEV), 16)


# ---------------------------------------------------------------------------------- scheduler step
@pytest.mark.parametrize("schedule,T", [("squaredcos_cap_v2", 50), ("squaredcos_cap_v2", 1000), ("linear", 1000)])
def test_ddpm_step_bit_exact(schedule, T):
    from oracle import ddpm as oddpm
    from synt_isic_amd.scheduler import HipDDPMScheduler
    o = oddpm.DDPMSchedulerOracle(beta_schedule=schedule)
    o.set_timesteps(T)
    s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule=schedule)
    s.set_timesteps(T)
    x = _rand(2, 3, 16, 16, seed=60) * 1.3
    eps = _rand(2, 3, 16, 16, seed=61)
    z = _rand(2, 3, 16, 16, seed=62)
    ts = [int(t) for t in s.timesteps]
    for t in [ts[0], ts[1], ts[len(ts) // 2], ts[-2], ts[-1]]:
        want = o.step(eps, t, x, noise=z)
        got = s.step(eps.to(DEV), t, x.to(DEV), variance_noise=z.to(DEV)).prev_sample.cpu()
        assert torch.equal(got, want), f"t={t}: max diff {(got - want).abs().max().item():.3e}"


def test_ddpm_step_tail_and_inplace():
    from oracle import ddpm as oddpm
    from synt_isic_amd import ops
    from synt_isic_amd.scheduler import HipDDPMScheduler
    o = oddpm.DDPMSchedulerOracle(); o.set_timesteps(50)
    s = HipDDPMScheduler(beta_schedule="squaredcos_cap_v2"); s.set_timesteps(50)
    n = 4 * 257 + 3                                     # not a multiple of 4: scalar tail
    x, eps, z = _rand(n, seed=63), _rand(n, seed=64), _rand(n, seed=65)
    want = o.step(eps, 500, x, noise=z)
    xd = x.to(DEV)
    ops.ddpm_step(eps.to(DEV), xd, z.to(DEV), s.step_coefficients(500), 1.0, out=xd)      # in place
    assert torch.equal(xd.cpu(), want)
    # misaligned views take the scalar path
    big = _rand(3 * n + 1, seed=66).to(DEV)
    xv = big[1:1 + n]
    got = ops.ddpm_step(eps.to(DEV), xv.contiguous(), z.to(DEV), s.step_coefficients(500), 1.0)
    assert torch.equal(got.cpu(), o.step(eps, 500, xv.cpu(), noise=z))
    # generator-driven noise (the reference's call passes none; diffusers draws on the sample's device)
    g = torch.Generator().manual_seed(5)
    a = s.step(eps.to(DEV), 500, x.to(DEV), generator=g).prev_sample.cpu()
    g2 = torch.Generator().manual_seed(5)
    assert torch.equal(a, o.step(eps, 500, x, generator=g2))


def test_denorm_u8_bit_exact():
    from oracle import sampler as osampler
    from synt_isic_amd import ops
    x = _rand(3, 3, 20, 12, seed=70) * 0.8
    x[0, 0, 0, :8] = torch.tensor([-1.5, -1.0, -0.999, 0.0, 0.5, 0.99999, 1.0, 3.0])
    x[1, 1, 1, 1] = float("inf"); x[1, 1, 1, 2] = -float("inf")
    got = ops.denorm_u8(x.to(DEV)).cpu().numpy()
    assert got.shape == (3, 20, 12, 3) and got.dtype == np.uint8
    assert np.array_equal(got, osampler.denormalize_to_uint8(x))


def test_denorm_u8_three_reference_forms_bit_exact():
    """The reference converts latents to uint8 in three places, each spelled differently: image_generator.py:441-447
    (clamp((x+1)/2) * 255), generate_test.py:94-97 ((clamp(x)+1) * 0.5 * 255) and diffusion_generator.py:231-232
    (clip((x+1) * 127.5, 0, 255)).  Every form of the kernel equals its numpy/torch restatement bit for bit -- and all three
    are bit-identical to each other: halving is exact in binary floating point, so (x+1)/2*255 and (x+1)*127.5 round the
    SAME real number once (VERDICT r01 expected the third form to round differently; measured here on every boundary value
    of both scalings +- a few ulps, it does not)."""
    from oracle import sampler as osampler
    from synt_isic_amd import ops
    g = torch.Generator().manual_seed(71)
    x = torch.randn(4, 3, 64, 64, generator=g) * 0.7
    # values at and around k/127.5 - 1 and k/255*2 - 1 (the integer boundaries of either scaling), k = 0..255, +- ulps
    k = torch.arange(0, 256, dtype=torch.float64)
    edges = torch.cat([(k / 127.5 - 1).float(), (k / 255 * 2 - 1).float()])
    near = [edges]
    for direction in (-9.0, 9.0):
        e = edges.clone()
        for _ in range(3):
            e = torch.nextafter(e, torch.full_like(e, direction))
            near.append(e.clone())
    ulps = torch.cat(near)
    x.view(-1)[: ulps.numel()] = ulps
    x[3, 2, 5, :6] = torch.tensor([-1.5, -1.0, 1.0, 3.0, float("inf"), -float("inf")])
    xd = x.to(DEV)
    a = ops.denorm_u8(xd, "image_generator").cpu().numpy()
    b = ops.denorm_u8(xd, "generate_test").cpu().numpy()
    c = ops.denorm_u8(xd, "diffusion_generator").cpu().numpy()
    assert np.array_equal(a, osampler.denormalize_to_uint8(x))
    assert np.array_equal(b, osampler.denormalize_to_uint8_generate_test(x))
    assert np.array_equal(c, osampler.denormalize_to_uint8_diffusion_generator(x))
    assert np.array_equal(a, b) and np.array_equal(a, c)          # the three spellings agree on every input
    assert np.array_equal(a, ops.denorm_u8(xd).cpu().numpy())    # default = image_generator.py's form


def test_conv2d_auto_dispatch_fuzz():
    """sisic_conv2d with tile_cfg = 0 over 80 seeded random shapes and feature combinations against the float64
    convolution: whatever kernel the dispatch picks (direct, flat 1x1 with float4 staging, Winograd, nine-position
    upsample form, K-split form, vector-ALU small-Cout) must agree, and the GroupNorm partials it reports must
    reproduce the statistics of what it stored."""
    import random
    from synt_isic_amd import ops
    rnd = random.Random(20261004)
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    picked = set()
    for case in range(80):
        k = rnd.choice([1, 3, 3, 3])
        stride = rnd.choice([1, 1, 1, 2])
        ups = k == 3 and stride == 1 and rnd.random() < 0.2
        B = rnd.choice([1, 2, 3, 5, 8])
        H, W = rnd.choice([4, 6, 8, 8, 9, 12, 16, 16, 20, 32, 40]), rnd.choice([4, 5, 8, 8, 10, 16, 16, 24, 32, 36])
        if ups:
            H, W = min(H, 16), min(W, 16)
        c0 = rnd.choice([3, 8, 20, 64, 128, 256])
        c1 = rnd.choice([0, 0, 12, 64, 128])
        cout = rnd.choice([3, 4, 32, 64, 70, 128, 256])
        if c0 + c1 > 256 and H * W > 400:
            H, W = 16, 16
        Cin = c0 + c1
        x = _rand(B, c0, H, W, seed=1000 + case)
        x2 = _rand(B, c1, H, W, seed=2000 + case) if c1 else None
        w = _rand(cout, Cin, k, k, seed=3000 + case, scale=(Cin * k * k) ** -0.5)
        kw = {"stride": stride, "upsample": ups, "x2": x2}
        if rnd.random() < 0.7:
            kw["bias"] = _rand(cout, seed=4000 + case)
        if rnd.random() < 0.5:
            kw["gn"] = (1.0 + 0.3 * _rand(B, Cin, seed=5000 + case), 0.3 * _rand(B, Cin, seed=6000 + case))
            kw["gn_silu"] = rnd.random() < 0.7
        if rnd.random() < 0.4:
            kw["chan_bias"] = _rand(B, cout, seed=7000 + case)
        Hc, Wc = (2 * H, 2 * W) if ups else (H, W)
        Ho, Wo = (Hc + 2 * (k // 2) - k) // stride + 1, (Wc + 2 * (k // 2) - k) // stride + 1
        if rnd.random() < 0.5:
            kw["residual"] = _rand(B, cout, Ho, Wo, seed=8000 + case)
        kw["relu"] = rnd.random() < 0.2
        ref = _conv_ref(x, w, kw.get("bias"), x2=x2, stride=stride, upsample=ups, gn=kw.get("gn"),
                        gn_silu=kw.get("gn_silu", False), chan_bias=kw.get("chan_bias"), residual=kw.get("residual"),
                        relu=kw["relu"])
        gn = kw.get("gn")
        wino = ops.pack_winograd_weight(d(w)) if (k == 3 and rnd.random() < 0.8) else None
        y, st = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, k, bias=d(kw.get("bias")), x2=d(x2), stride=stride,
                           upsample=ups, gn_scale=d(gn[0]) if gn else None, gn_shift=d(gn[1]) if gn else None,
                           gn_silu=kw.get("gn_silu", False), chan_bias=d(kw.get("chan_bias")),
                           residual=d(kw.get("residual")), relu=kw["relu"], w_winograd=wino, with_stats=True)
        what = f"case {case}: k{k} s{stride} ups{int(ups)} B{B} {c0}+{c1}->{cout} @{H}x{W} wino={wino is not None}"
        _close(y, ref, tol=KTOL, what=what)
        picked.add((k, stride, ups, wino is not None, st is not None))
        if st is not None:
            stc, yc = st.cpu().double(), y.cpu().double()
            n = stc[..., 0].sum(-1)
            assert torch.equal(n, torch.full_like(n, float(Ho * Wo))), what
            mean = stc[..., 1].sum(-1) / n
            _close(mean.float(), yc.mean((2, 3)), tol=1e-5, what=what + " (partial sums)")
            mean_i = stc[..., 1] / stc[..., 0].clamp(min=1)
            m2 = stc[..., 2].sum(-1) + (stc[..., 0] * (mean_i - mean[..., None]) ** 2).sum(-1)
            _close((m2 / n).float(), yc.var((2, 3), unbiased=False), tol=1e-4, what=what + " (partial M2)")
    assert len(picked) >= 8          # the draw really covered the dispatch space


@pytest.mark.parametrize("cfg,k,ups,B,H,W,cin,cout", [
    (20, 1, False, 2, 16, 16, 64, 64), (22, 1, False, 2, 12, 20, 40, 70), (28, 1, False, 2, 16, 16, 136, 128),
    (34, 1, False, 2, 16, 16, 64, 384), (35, 1, False, 2, 16, 16, 256, 128),   # the staged and the K-split 1x1 forms
    (0, 3, True, 2, 10, 14, 24, 40),            # the generic MFMA path with a nearest-2x input
    (74, 3, False, 3, 32, 32, 72, 64), (92, 3, False, 5, 8, 8, 128, 64), (0, 3, False, 2, 8, 8, 64, 64), (60, 3, False, 2, 18, 10, 24, 70),
    (4, 3, False, 2, 9, 5, 16, 64), (50, 3, False, 2, 16, 16, 20, 3), (11, 3, False, 2, 16, 16, 16, 64)])
def test_conv_residual_may_alias_out(cfg, k, ups, B, H, W, cin, cout):
    """the backward pass accumulates a data gradient in place (conv2d with out = residual, train.cpp).  The
    contract (include/sisic.h): every kernel reads a residual element in the thread that stores it, before the store --
    also the K-split reductions, whose `residual` and `out` are no longer __restrict__.  In place == out of place, bit for bit."""
    from synt_isic_amd import ops
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    x = _rand(B, cin, H, W, seed=950 + cfg)
    w = _rand(cout, cin, k, k, seed=951 + cfg, scale=(k * k * cin) ** -0.5)
    b = _rand(cout, seed=952 + cfg)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    stride = 2 if cfg == 11 else 1
    if stride == 2:
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
    res = _rand(B, cout, Ho, Wo, seed=953 + cfg)
    ww = ops.pack_winograd_weight(d(w)) if (k == 3 and stride == 1 and cout > 4) else None
    common = dict(bias=d(b), upsample=ups, stride=stride, tile_cfg=cfg, w_winograd=ww)
    want = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, k, residual=d(res), **common)
    buf = d(res).clone()
    got = ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, k, residual=buf, out=buf, **common)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got, want), f"cfg{cfg}: in-place accumulate differs from the out-of-place result"
    _close(got, _conv_ref(x, w, b, upsample=ups, stride=stride, residual=res), what=f"in-place conv cfg{cfg}")


def test_conv_finalizes_its_own_groupnorm_at_the_8x8_level():
    """ABI 3, sisic_conv_args.fin_*: the K-split 8x8-level convolution (tile_cfg 92 / auto) leaves the (scale, shift) of the
    GroupNorm over its own output -- bit for bit what sisic_groupnorm_finalize computes from the partials it also leaves --
    and sisic_conv_finalizes() says where it does not (another level, another group size)."""
    from synt_isic_amd import ops
    d = lambda t: t.to(DEV).contiguous()
    B, cin, cout = 5, 128, 256
    x = _rand(B, cin, 8, 8, seed=700)
    w = _rand(cout, cin, 3, 3, seed=701, scale=(9 * cin) ** -0.5)
    b, res = _rand(cout, seed=702), _rand(B, cout, 8, 8, seed=703)
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=704), 0.1 * _rand(cout, seed=705)
    gn = (1.0 + 0.3 * _rand(B, cin, seed=706), 0.3 * _rand(B, cin, seed=707))
    wp, ww = ops.pack_conv_weight(d(w)), ops.pack_winograd_weight(d(w))
    for cfg in (0, 92, 91):
        y, st, fin = ops.conv2d(d(x), wp, cout, 3, bias=d(b), residual=d(res), gn_scale=d(gn[0]), gn_shift=d(gn[1]), gn_silu=True,
                                tile_cfg=cfg, w_winograd=ww, with_stats=True, finalize=(d(gamma), d(beta), 32, 1e-5))
        assert fin is not None and st is not None
        sc, sh = ops.groupnorm_finalize(st, 64, d(gamma), d(beta), 32, 1e-5)
        assert torch.equal(fin[0], sc) and torch.equal(fin[1], sh), f"cfg {cfg}"
        yc = y.cpu().double()
        ref = F.group_norm(yc, 32, gamma.double(), beta.double(), 1e-5)
        _close((yc * fin[0].cpu().double()[:, :, None, None] + fin[1].cpu().double()[:, :, None, None]).float(), ref, what="fused finalisation")
        # the same output as without the request
        assert torch.equal(y, ops.conv2d(d(x), wp, cout, 3, bias=d(b), residual=d(res), gn_scale=d(gn[0]), gn_shift=d(gn[1]), gn_silu=True,
                                         tile_cfg=cfg, w_winograd=ww))
    # 16 groups of 16 channels: not finalized by the launch
    _, fin = ops.conv2d(d(x), wp, cout, 3, w_winograd=ww, finalize=(d(gamma), d(beta), 16, 1e-5))
    assert fin is None
    # a plane that is ONE 16x16-pixel tile of the bf16x3 Winograd kernel (tile_cfg 74): its workgroup holds 64 channels of an
    # image whole and finalizes their eight groups; ragged planes too (16 x 14); two tiles (16 x 32) not
    for (H, W, does) in ((16, 16, True), (16, 14, True), (16, 32, False)):
        xs = _rand(3, cin, H, W, seed=708)
        rs = _rand(3, cout, H, W, seed=709)
        gs = (1.0 + 0.3 * _rand(3, cin, seed=710), 0.3 * _rand(3, cin, seed=711))
        kw = dict(bias=d(b), residual=d(rs), gn_scale=d(gs[0]), gn_shift=d(gs[1]), gn_silu=True, w_winograd=ww)
        y, st, fin = ops.conv2d(d(xs), wp, cout, 3, with_stats=True, finalize=(d(gamma), d(beta), 32, 1e-5), **kw)
        assert (fin is not None) == does, (H, W)
        if does:
            sc, sh = ops.groupnorm_finalize(st, H * W, d(gamma), d(beta), 32, 1e-5)
            assert torch.equal(fin[0], sc) and torch.equal(fin[1], sh), (H, W)
            assert torch.equal(y, ops.conv2d(d(xs), wp, cout, 3, **kw))
            # without stats_out as well
            _, fin2 = ops.conv2d(d(xs), wp, cout, 3, finalize=(d(gamma), d(beta), 32, 1e-5), **kw)
            assert torch.equal(fin2[0], sc) and torch.equal(fin2[1], sh)


# (tile_cfg, H, W, upsample, Cout, groups, residual misaligned by one float, what sisic_conv_finalizes must answer)
_FIN_CASES = [(cfg, 8, 8, 0, 256, 32, False, 1) for cfg in (90, 91, 92, 0)] + \
             [(cfg, 8, 8, 0, 256, 32, True, 0) for cfg in (90, 91, 92, 0)] + \
             [(0, 7, 7, 0, 256, 32, False, 0), (0, 8, 8, 0, 256, 16, False, 0), (74, 16, 16, 0, 64, 8, False, 1),
              (74, 32, 32, 0, 256, 32, False, 0), (74, 8, 8, 1, 256, 32, False, 0)]


@pytest.mark.parametrize("cfg,H,W,ups,cout,groups,res_off,expect", _FIN_CASES)
def test_conv_writes_fin_outputs_exactly_where_the_predicate_says(cfg, H, W, ups, cout, groups, res_off, expect):
    """The fin_* fields stay set WHATEVER sisic_conv_finalizes() answers (ops.conv2d clears them where it answers 0): the launch
    overwrites fin_scale / fin_shift -- bit-equal to sisic_groupnorm_finalize on the partials it leaves -- exactly where the
    predicate says 1; where it says 0 they are untouched (sisic.h: the fields are ignored) and the output is still right."""
    import ctypes as C
    from synt_isic_amd import _lib, ops
    d = lambda t: t.to(DEV).contiguous()
    B, cin = 5, 128
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    x = _rand(B, cin, H, W, seed=720)
    w = _rand(cout, cin, 3, 3, seed=721, scale=(9 * cin) ** -0.5)
    b, res = _rand(cout, seed=722), _rand(B, cout, Ho, Wo, seed=723)
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=724), 0.1 * _rand(cout, seed=725)
    gn = (1.0 + 0.3 * _rand(B, cin, seed=726), 0.3 * _rand(B, cin, seed=727))
    xd, bd, gd, bed, gn0, gn1 = d(x), d(b), d(gamma), d(beta), d(gn[0]), d(gn[1])
    wp, ww = ops.pack_conv_weight(d(w)), ops.pack_winograd_weight(d(w))
    res_buf = torch.empty(res.numel() + 1, dtype=torch.float32, device=DEV)
    res_d = res_buf[1:] if res_off else res_buf[:-1]            # a view one float off the allocation's alignment
    res_d.copy_(res.reshape(-1))
    out = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=DEV)
    SENTINEL = -7.25
    fin_scale = torch.full((B, cout), SENTINEL, dtype=torch.float32, device=DEV)
    fin_shift = torch.full((B, cout), SENTINEL, dtype=torch.float32, device=DEV)
    lib = _lib.load()
    a = _lib.ConvArgs()
    a.in0 = xd.data_ptr(); a.c0 = cin; a.B = B; a.Hin = H; a.Win = W
    a.upsample = ups; a.ksize = 3; a.stride = 1
    a.w_packed = wp.data_ptr(); a.bias = bd.data_ptr(); a.Cout = cout
    a.gn_scale = gn0.data_ptr(); a.gn_shift = gn1.data_ptr(); a.gn_silu = 1
    a.residual = res_d.data_ptr(); a.out = out.data_ptr(); a.tile_cfg = cfg
    a.w_winograd = ww.data_ptr()
    assert (a.residual % 16 != 0) == res_off
    slots = lib.sisic_conv_stats_slots(C.byref(a))
    assert slots > 0
    stats = torch.empty((B, cout, slots, 4), dtype=torch.float32, device=DEV)
    a.stats_out = stats.data_ptr()
    a.fin_gamma = gd.data_ptr(); a.fin_beta = bed.data_ptr(); a.fin_groups = groups; a.fin_eps = 1e-5
    a.fin_scale = fin_scale.data_ptr(); a.fin_shift = fin_shift.data_ptr()
    says = lib.sisic_conv_finalizes(C.byref(a))
    assert says == expect, f"sisic_conv_finalizes answers {says}"
    _lib.check(lib.sisic_conv2d(ops.context(xd.device), C.byref(a), ops._stream(xd.device)))
    torch.cuda.synchronize()
    _close(out, _conv_ref(x, w, b, upsample=bool(ups), gn=gn, gn_silu=True, residual=res), what=f"fin case cfg {cfg} {H}x{W}")
    if says:
        sc, sh = ops.groupnorm_finalize(stats, Ho * Wo, gd, bed, groups, 1e-5)
        assert torch.equal(fin_scale, sc) and torch.equal(fin_shift, sh)
    else:
        assert bool((fin_scale == SENTINEL).all()) and bool((fin_shift == SENTINEL).all()), "fin_scale / fin_shift written although the predicate says 0"
