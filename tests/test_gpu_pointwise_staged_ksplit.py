"""The staged K-split form of the bf16x3 1x1 convolution (tile_cfg 37, conv_pwbsk_kernel): one workgroup per 64-pixel tile, waves =
channel items x K quarters, the tile's operands split once into LDS.

Its contract is BIT equality with the K-split form (tile_cfg 35) on `out` and `stats_out` for every shape both take: that is what
lets the plan choose between them by batch.  Everything else here follows from it: float64 parity at the project's cross-kernel
bound, riders (gn_finalize_kernel's bits, the host's output unchanged), and the suite's poisoned, guarded outputs, under which a
store outside the tile or an element left unwritten shows by itself.
"""
import pytest
import torch

from poison import guard_bands, poison_allocations, unwritten  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
NEW, OLD = 37, 35

# name -> (c0, c1, Cout, H = W): what the row exercises
ROWS = {
    "128_64_8x8": (128, 0, 64, 8),             # one tile, four waves, four chunks per quarter
    "128_128_16x16": (128, 0, 128, 16),        # eight waves
    "256_256_16x16": (256, 0, 256, 16),        # sixteen waves, LDS full
    "128+128_256_16x16": (128, 128, 256, 16),  # seam on a quarter boundary
    "256+128_256_16x16": (256, 128, 256, 16),  # seam inside a quarter, two passes
    "256+256_256_8x8": (256, 256, 256, 8),     # two passes, one tile per image
}
OPTIONS = ("residual", "bias", "chan_bias", "stats")
# every option with and without: all, none, each one alone
COMBOS = [OPTIONS, ()] + [(o,) for o in OPTIONS]
CASES = [(row, 2, combo) for row in ROWS for combo in COMBOS] + [(row, B, OPTIONS) for row in ROWS for B in (1, 3)]


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


@pytest.fixture(scope="module")
def inputs():
    """per (row, B): seeded N(0,1) inputs and weights on the host and the device -- made once, never written"""
    from synt_isic_amd import ops
    out = {}
    for i, (row, (c0, c1, cout, H)) in enumerate(ROWS.items()):
        w = _rand(cout, c0 + c1, 1, 1, seed=3700 + i)
        wp = ops.pack_conv_weight(_d(w))
        for B in (1, 2, 3):
            s = 3710 + 10 * i + B
            host = dict(x=_rand(B, c0 + c1, H, H, seed=s), w=w, bias=_rand(cout, seed=s + 100), chan_bias=_rand(B, cout, seed=s + 200),
                        residual=_rand(B, cout, H, H, seed=s + 300))
            dev = dict(x=_d(host["x"][:, :c0]), x2=_d(host["x"][:, c0:]) if c1 else None, wp=wp, bias=_d(host["bias"]),
                       chan_bias=_d(host["chan_bias"]), residual=_d(host["residual"]))
            out[(row, B)] = (host, dev)
    return out


def _run(dev, cout, cfg, combo):
    from synt_isic_amd import ops
    kw = {o: dev[o] for o in combo if o != "stats"}
    r = ops.conv2d(dev["x"], dev["wp"], cout, 1, x2=dev["x2"], tile_cfg=cfg, with_stats="stats" in combo, **kw)
    return r if "stats" in combo else (r, None)


@pytest.mark.parametrize("row,B,combo", CASES, ids=[f"{r}-B{b}-{'+'.join(c) or 'plain'}" for r, b, c in CASES])
def test_bits_of_the_ksplit_form(inputs, row, B, combo):
    cout = ROWS[row][2]
    _, dev = inputs[(row, B)]
    y_new, st_new = _run(dev, cout, NEW, combo)
    y_old, st_old = _run(dev, cout, OLD, combo)
    assert unwritten(y_new) == 0 and torch.isfinite(y_new).all()
    assert torch.equal(y_new, y_old), f"out differs from tile_cfg {OLD} in {(y_new != y_old).sum().item()} elements"
    if "stats" in combo:
        assert st_new is not None and st_new.shape == st_old.shape == (B, cout, ROWS[row][3] ** 2 // 32, 4)
        assert unwritten(st_new) == 0
        assert torch.equal(st_new, st_old), f"stats_out differs from tile_cfg {OLD} in {(st_new != st_old).sum().item()} elements"


@pytest.mark.parametrize("row", ["256_256_16x16", "256+128_256_16x16"])
def test_parity_with_float64(inputs, row):
    """the project's cross-kernel bound, 1e-5 * max(1, |ref|_inf), on the output; the partials against the output's own float64
    sums at the same relative bound"""
    c0, c1, cout, H = ROWS[row]
    host, dev = inputs[(row, 2)]
    y, st = _run(dev, cout, NEW, OPTIONS)
    ref = torch.einsum("oc,bchw->bohw", host["w"][:, :, 0, 0].double(), host["x"].double())
    ref = ref + host["bias"].double()[None, :, None, None] + host["chan_bias"].double()[:, :, None, None] + host["residual"].double()
    bound = 1e-5 * max(1.0, ref.abs().max().item())
    err = (y.cpu().double() - ref).abs().max().item()
    print(f"{row}: max |y - float64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    blocks = ref.reshape(2, cout, H * H // 32, 32)
    s1 = blocks.sum(-1)
    m2 = ((blocks - blocks.mean(-1, keepdim=True)) ** 2).sum(-1)
    st = st.cpu().double()
    assert (st[..., 0] == 32.0).all() and (st[..., 3] == 0.0).all()
    e1, e2 = (st[..., 1] - s1).abs().max().item(), (st[..., 2] - m2).abs().max().item()
    b1, b2 = 1e-5 * max(1.0, s1.abs().max().item()), 1e-5 * max(1.0, m2.abs().max().item())
    print(f"{row}: partial sums {e1:.3e} (bound {b1:.3e}), M2 {e2:.3e} (bound {b2:.3e})")
    assert e1 <= b1 and e2 <= b2


# ---------------------------------------------------------------------------------- riders
def _partials(B, C, slots, seed):
    """[B, C, slots, 4] partials (count, sum, M2 about the partial's own mean, 0) of 32 N(0,1) values each"""
    v = _rand(B, C, slots, 32, seed=seed).double()
    s1 = v.sum(-1)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([torch.full_like(s1, 32.0), s1, m2, torch.zeros_like(s1)], -1).float()


# jobs = images x groups of the finalisation (its batch is its own): (images, channels, groups)
RIDER_JOBS = {1: (1, 8, 1), 16: (2, 64, 8), 17: (17, 8, 1)}


@pytest.mark.parametrize("row", ["256_256_16x16", "128_64_8x8", "256+256_256_8x8"])        # 16-wave and 4-wave workgroups, two passes
@pytest.mark.parametrize("jobs", list(RIDER_JOBS))
def test_riders(inputs, row, jobs):
    """one job per wave of the host's workgroup: 1 job (surplus waves return), 16 (one full 16-wave workgroup), 17 (a second
    rider workgroup with one job) -- (scale, shift) are gn_finalize_kernel's bits, the host's output is the launch's without riders"""
    from synt_isic_amd import ops
    cout = ROWS[row][2]
    _, dev = inputs[(row, 3)]
    Bs, C, G = RIDER_JOBS[jobs]
    assert Bs * G == jobs
    st = _d(_partials(Bs, C, 4, seed=3790 + jobs))
    gamma, beta = _d(1.0 + 0.1 * _rand(C, seed=3791)), _d(0.1 * _rand(C, seed=3792))
    sc_ref, sh_ref = ops.groupnorm_finalize(st, 128, gamma, beta, G, EPS)
    y_ref = ops.conv2d(dev["x"], dev["wp"], cout, 1, bias=dev["bias"], x2=dev["x2"], tile_cfg=NEW)
    y, sc, sh, carried = ops.conv2d_gn_rider(dev["x"], dev["wp"], cout, 1, st, 128, gamma, beta, G, EPS, bias=dev["bias"], x2=dev["x2"],
                                             tile_cfg=NEW)
    assert carried == 1
    assert unwritten(sc) == 0 and unwritten(sh) == 0
    assert torch.equal(sc, sc_ref) and torch.equal(sh, sh_ref), "not sisic_groupnorm_finalize's bits"
    assert torch.equal(y, y_ref), "the host's output changed with riders in its grid"


def test_refused_shapes_launch_nothing(inputs):
    """a forced tile_cfg 37 on arguments the form does not take is the launch's error (the messages: tests/test_pointwise_plan_cpu.py)"""
    from synt_isic_amd import ops
    _, dev = inputs[("128_64_8x8", 2)]
    gs, gh = _d(1.0 + 0.1 * _rand(2, 128, seed=1)), _d(0.1 * _rand(2, 128, seed=2))
    with pytest.raises(Exception, match="tile_cfg 37"):
        ops.conv2d(dev["x"], dev["wp"], 64, 1, tile_cfg=NEW, gn_scale=gs, gn_shift=gh)
    with pytest.raises(Exception, match="tile_cfg 37"):
        ops.conv2d(dev["x"], dev["wp"], 64, 1, tile_cfg=NEW, relu=True)
