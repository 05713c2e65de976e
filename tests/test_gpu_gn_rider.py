"""GroupNorm finalisation riding on a 1x1 convolution's launch (sisic_conv2d_gn_rider; Fwd::resnet's shortcut-first order).

Everything here is a bit-equality condition: the rider workgroups run the function gn_finalize_kernel runs, and the host
workgroups' item mapping is the one of a launch without riders -- no tolerance anywhere.
"""
import itertools

import pytest
import torch

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _partials(B, C, slots, seed, mean=0.0, std=1.0):
    """[B, C, slots, 4] partials (count, sum, M2 about the partial's own mean, 0) of 32 values drawn around `mean`."""
    v = (_rand(B, C, slots, 32, seed=seed) * std + mean).double()
    s1 = v.sum(-1)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([torch.full_like(s1, 32.0), s1, m2, torch.zeros_like(s1)], -1).float()


# name -> (B, groups, [(channels, slots), ...], mean, std): every path of one finalisation job
RIDERS = {
    "one_producer_one_slot": (2, 8, [(64, 1)], 0.0, 1.0),
    "two_producers_4_and_16_slots": (2, 8, [(32, 4), (32, 16)], 0.0, 1.0),
    # the issue's seam case: c0 = 24, c1 = 40 in 8 groups -- 8 channels per group, so the seam falls on a group boundary ...
    "seam_24_40": (2, 8, [(24, 1), (40, 4)], 0.0, 1.0),
    # ... and the case it means: group 2 = channels 16 .. 23 has four channels of each producer
    "group_spans_seam_20_44": (2, 8, [(20, 1), (44, 4)], 0.0, 1.0),
    # 32 channels x 16 slots = 512 partials per group, past the 4 x 64 a wave keeps in registers: the loop behind KEEP runs
    "more_than_256_partials": (2, 4, [(128, 16)], 0.0, 1.0),
    # 18 jobs: the fifth rider workgroup has two idle waves
    "jobs_not_multiple_of_4": (3, 6, [(48, 2)], 0.0, 1.0),
    "large_mean": (2, 8, [(32, 4), (32, 16)], 100.0, 1e-2),
}


@pytest.fixture(scope="module")
def riders():
    """per rider shape: the partials, gamma / beta and the stand-alone launch's (scale, shift) -- computed once, never written"""
    from synt_isic_amd import ops
    out = {}
    for i, (name, (B, G, prods, mean, std)) in enumerate(RIDERS.items()):
        st = [_d(_partials(B, c, s, seed=900 + 10 * i + k, mean=mean, std=std)) for k, (c, s) in enumerate(prods)]
        C = sum(c for c, _ in prods)
        gamma, beta = _d(1.0 + 0.1 * _rand(C, seed=990 + i)), _d(0.1 * _rand(C, seed=995 + i))
        sc, sh = ops.groupnorm_finalize(st[0], 64, gamma, beta, G, EPS, stats2=st[1] if len(st) > 1 else None)
        assert torch.isfinite(sc).all() and torch.isfinite(sh).all()
        out[name] = dict(stats=st[0], stats2=st[1] if len(st) > 1 else None, gamma=gamma, beta=beta, groups=G, scale=sc, shift=sh)
    return out


# tile_cfg -> (Cin, split of Cin with the seam on an 8-channel chunk boundary)
HOSTS = {29: (64, (40, 24)), 30: (64, (40, 24)), 35: (128, (72, 56))}


@pytest.fixture(scope="module")
def hosts():
    """per (tile_cfg, second input, B): the convolution's inputs and sisic_conv2d's output"""
    from synt_isic_amd import ops
    out = {}
    for cfg, (cin, (c0, c1)) in HOSTS.items():
        w = _rand(64, cin, 1, 1, seed=800 + cfg, scale=cin ** -0.5)
        wp, bias = ops.pack_conv_weight(_d(w)), _d(_rand(64, seed=810 + cfg))
        for two, B in itertools.product((False, True), (1, 3)):
            x = _rand(B, cin, 8, 8, seed=820 + cfg + B)
            xa, xb = (_d(x[:, :c0]), _d(x[:, c0:])) if two else (_d(x), None)
            ref = ops.conv2d(xa, wp, 64, 1, bias=bias, x2=xb, tile_cfg=cfg)
            out[(cfg, two, B)] = dict(x=xa, x2=xb, wp=wp, bias=bias, ref=ref)
    return out


@pytest.mark.parametrize("rider", list(RIDERS))
@pytest.mark.parametrize("cfg,two,B", [(c, t, b) for c in HOSTS for t in (False, True) for b in (1, 3)])
def test_rider_on_every_host_form(hosts, riders, cfg, two, B, rider):
    from synt_isic_amd import ops
    h, r = hosts[(cfg, two, B)], riders[rider]
    scale, shift = torch.full_like(r["scale"], float("nan")), torch.full_like(r["shift"], float("nan"))
    y, sc, sh, carried = ops.conv2d_gn_rider(h["x"], h["wp"], 64, 1, r["stats"], 64, r["gamma"], r["beta"], r["groups"], EPS,
                                             stats2=r["stats2"], bias=h["bias"], x2=h["x2"], tile_cfg=cfg, scale=scale, shift=shift)
    assert carried == 1
    assert torch.equal(y, h["ref"]), f"tile_cfg {cfg}: the host's output changed with riders in its grid"
    assert torch.equal(sc, r["scale"]) and torch.equal(sh, r["shift"]), f"{rider}: not sisic_groupnorm_finalize's bits"


def test_rider_is_refused_by_other_kernels(riders):
    """a 3x3 convolution and a 1x1 with a GroupNorm prologue do not carry: carried = 0, the convolution is sisic_conv2d's and
    (scale, shift) are untouched"""
    from synt_isic_amd import ops
    r = riders["two_producers_4_and_16_slots"]
    B = 2
    x = _d(_rand(B, 64, 8, 8, seed=700))
    w3, w1 = _rand(64, 64, 3, 3, seed=701, scale=1 / 24), _rand(64, 64, 1, 1, seed=702, scale=1 / 8)
    gsc, gsh = _d(1.0 + 0.1 * _rand(B, 64, seed=703)), _d(0.1 * _rand(B, 64, seed=704))
    cases = [("3x3", dict(w_packed=ops.pack_conv_weight(_d(w3)), ksize=3), {}),
             ("1x1 with a GroupNorm prologue", dict(w_packed=ops.pack_conv_weight(_d(w1)), ksize=1),
              dict(gn_scale=gsc, gn_shift=gsh, gn_silu=True))]
    for what, conv, kw in cases:
        ref = ops.conv2d(x, conv["w_packed"], 64, conv["ksize"], **kw)
        scale, shift = torch.full_like(r["scale"], -7.0), torch.full_like(r["shift"], -9.0)
        y, sc, sh, carried = ops.conv2d_gn_rider(x, conv["w_packed"], 64, conv["ksize"], r["stats"], 64, r["gamma"], r["beta"],
                                                 r["groups"], EPS, stats2=r["stats2"], scale=scale, shift=shift, **kw)
        assert carried == 0, what
        assert torch.equal(y, ref), what
        assert (sc == -7.0).all() and (sh == -9.0).all(), what


# ---------------------------------------------------------------------------------- the network
def _model(sd, monkeypatch, rider, latency=False):
    from synt_isic_amd.unet import HipUNet2DModel
    if not rider:
        monkeypatch.setenv("SISIC_GN_RIDER", "0")         # read at sisic_unet_create
    m = HipUNet2DModel().set_latency_mode(latency)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m(torch.zeros(1, 3, 32, 32, device=DEV), 1)
    if not rider:
        monkeypatch.delenv("SISIC_GN_RIDER")
    return m


def _profiled(m, x, t):
    from synt_isic_amd import ops
    m(x, t)                                               # workspace and event pool first
    torch.cuda.synchronize()
    ops.profile_enable(DEV, True)
    try:
        ops.profile_reset(DEV)
        y = m(x, t).sample
        torch.cuda.synchronize()
        prof = ops.profile_read(DEV)
    finally:
        ops.profile_enable(DEV, False)
    return y, prof


def test_network_bits_and_launch_counts(synthetic_sd, monkeypatch):
    """SISIC_GN_RIDER=0 against the default: the same bits; at 64x64 every one of the 14 blocks with a shortcut (12 up, the
    first of down levels 1 and 2) loses its stand-alone norm1 launch and no 1x1 launch is added.  At 32x32 the 4x4 level's
    shortcuts are not the bf16x3 kernels' (16 pixels): their launcher answers carried = false and the launch follows."""
    off, on = _model(synthetic_sd, monkeypatch, False), _model(synthetic_sd, monkeypatch, True)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    ya, pa = _profiled(off, x, 321)
    yb, pb = _profiled(on, x, 321)
    assert torch.equal(ya, yb)
    print("groupnorm launches", pa["groupnorm"]["launches"], "->", pb["groupnorm"]["launches"],
          "conv1x1", pa["conv1x1"]["launches"], "->", pb["conv1x1"]["launches"])
    assert pa["groupnorm"]["launches"] - pb["groupnorm"]["launches"] == 14
    assert pa["conv1x1"]["launches"] == pb["conv1x1"]["launches"]
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
    assert torch.equal(off(x, 7).sample, on(x, 7).sample)


def test_network_latency_mode_has_no_hosts(synthetic_sd, monkeypatch):
    """latency mode runs its 1x1 layers on the 64-pixel f32 tiles (tile_cfg 22): nothing carries, every finalisation stays a
    launch of its own, and the bits are those without the switch"""
    off, on = _model(synthetic_sd, monkeypatch, False, latency=True), _model(synthetic_sd, monkeypatch, True, latency=True)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    ya, pa = _profiled(off, x, 321)
    yb, pb = _profiled(on, x, 321)
    assert torch.equal(ya, yb)
    assert pa["groupnorm"]["launches"] == pb["groupnorm"]["launches"]
    assert pa["conv1x1"]["launches"] == pb["conv1x1"]["launches"]
