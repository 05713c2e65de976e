"""The stride-2 3x3 convolution with fp32-equivalent products on the bf16 matrix pipe (conv_s2_bf3.hip; tile_cfg 36 forces it,
it is the automatic choice for the arguments it takes) against F.conv2d in float64.  The kernel has ONE form -- the input
channels split over the four waves of a workgroup -- for every shape, so there is no second form to compare bits with.

Bound: the project's per-kernel bound, max-abs <= 1e-5 * max(1, |ref|_inf) (tests/test_gpu_kernels.py).  Every measured
error goes through SISIC_TEST_ERRLOG; measured on MI355X: profiles/r07/test_errors.txt.
"""
import itertools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _log(err, top, what):
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(f"{err / top:.3e}\t{KTOL:.1e}\t{what}\n")


def _close(got, ref64, what):
    got = got.detach().cpu().double()
    top = max(1.0, ref64.abs().max().item())
    err = (got - ref64).abs().max().item()
    _log(err, top, what)
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert err <= KTOL * top, f"{what}: max abs err {err:.3e} > {KTOL * top:.3e}"


def _rel_close(got, ref64, what):
    """the bound WITHOUT the max(1, .) floor: error relative to the largest reference output, whatever its magnitude"""
    got = got.detach().cpu().double()
    top = ref64.abs().max().item()
    err = (got - ref64).abs().max().item()
    _log(err, top, what)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= KTOL * top, f"{what}: max abs err {err:.3e} > {KTOL} * {top:.3e}"


def _ref(x, w, bias=None, gn=None, x2=None, chan_bias=None, residual=None, relu=False):
    x = x.double()
    if x2 is not None:
        x = torch.cat([x, x2.double()], dim=1)
    if gn is not None:
        x = F.silu(x * gn[0].double()[:, :, None, None] + gn[1].double()[:, :, None, None])
    y = F.conv2d(x, w.double(), None if bias is None else bias.double(), stride=2, padding=1)
    if chan_bias is not None:
        y = y + chan_bias.double().reshape(-1, w.shape[0])[:, :, None, None]
    if residual is not None:
        y = y + residual.double()
    return F.relu(y) if relu else y


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _run(x, w, cfg, split=True, with_stats=False, out=None, **kw):
    from synt_isic_amd import ops
    gn = kw.get("gn")
    return ops.conv2d(_d(x), ops.pack_conv_weight(_d(w)), w.shape[0], 3, stride=2, bias=_d(kw.get("bias")), x2=_d(kw.get("x2")),
                      gn_scale=_d(gn[0]) if gn else None, gn_shift=_d(gn[1]) if gn else None, gn_silu=bool(gn),
                      chan_bias=_d(kw.get("chan_bias")), residual=kw.get("residual_dev", _d(kw.get("residual"))),
                      relu=kw.get("relu", False), tile_cfg=cfg, w_winograd=ops.pack_conv_s2_weight(_d(w)) if split else None,
                      with_stats=with_stats, out=out)


# (H, W): whole tiles; one tile; odd sizes with every border tap and Hout = (H + 1) / 2; 17 x 17 outputs: fifteen tiles, the
# last row and column of them ragged
@pytest.mark.parametrize("H,W", [(16, 16), (8, 8), (9, 7), (5, 5), (34, 34)])
def test_base_shapes_forced_and_automatic_agree(H, W):
    x = _rand(2, 16, H, W, seed=1)
    w = _rand(64, 16, 3, 3, seed=2, scale=0.1)
    b = _rand(64, seed=3)
    ref = _ref(x, w, b)
    assert ref.shape[-2:] == ((H + 1) // 2, (W + 1) // 2)
    got = {cfg: _run(x, w, cfg, bias=b) for cfg in (0, 36)}
    for cfg, y in got.items():
        _close(y, ref, f"conv s2 bf16x3 cfg{cfg} 16->64 {H}x{W}")
    assert torch.equal(got[0], got[36])
    assert not torch.equal(got[0], _run(x, w, 0, split=False, bias=b))      # (the f32 kernel: other bits)


# 40 -> 64: five chunks, a quarter-K share that is not a whole number of chunks; 72 -> 128: two channel tiles, nine chunks
@pytest.mark.parametrize("cin,cout,H,W", [(40, 64, 8, 8), (72, 128, 16, 16)])
def test_channel_raggedness(cin, cout, H, W):
    x = _rand(2, cin, H, W, seed=11)
    w = _rand(cout, cin, 3, 3, seed=12, scale=(9 * cin) ** -0.5)
    b = _rand(cout, seed=13)
    ref = _ref(x, w, b)
    got = {cfg: _run(x, w, cfg, bias=b) for cfg in (0, 36)}
    for cfg, y in got.items():
        _close(y, ref, f"conv s2 bf16x3 cfg{cfg} {cin}->{cout} {H}x{W}")
    assert torch.equal(got[0], got[36])


@pytest.mark.parametrize("cfg", [0, 36])
def test_epilogue(cfg):
    B, cin, cout, H, W = 2, 16, 64, 9, 16
    x = _rand(B, cin, H, W, seed=21)
    w = _rand(cout, cin, 3, 3, seed=22, scale=0.1)
    b = _rand(cout, seed=23)
    res = _rand(B, cout, 5, 8, seed=24)
    for cb in (_rand(cout, seed=25), _rand(B, cout, seed=26)):          # chan_bias stride 0 and stride Cout
        for relu in (False, True):
            kw = dict(bias=b, chan_bias=cb, residual=res, relu=relu)
            y = _run(x, w, cfg, **kw)
            _close(y, _ref(x, w, **kw), f"conv s2 bf16x3 cfg{cfg} epilogue chan_bias{tuple(cb.shape)} relu={relu}")
            # residual aliasing out: bit-equal to the out-of-place run
            acc = _d(res).clone()
            y2 = _run(x, w, cfg, bias=b, chan_bias=cb, residual_dev=acc, relu=relu, out=acc)
            assert y2.data_ptr() == acc.data_ptr() and torch.equal(y2, y)


@pytest.mark.parametrize("cfg,H,W", [(0, 16, 16), (36, 9, 7), (0, 34, 34)])
def test_groupnorm_partials(cfg, H, W):
    from synt_isic_amd import ops
    B, cin, cout = 2, 16, 64
    x = _rand(B, cin, H, W, seed=31)
    w = _rand(cout, cin, 3, 3, seed=32, scale=0.1)
    b = _rand(cout, seed=33)
    y, st = _run(x, w, cfg, bias=b, with_stats=True)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert st is not None and tuple(st.shape) == (B, cout, ((Ho + 3) // 4) * ((Wo + 7) // 8), 4)
    assert st[..., 0].sum(dim=2).eq(Ho * Wo).all()                      # the slots' counts cover the plane once
    assert torch.equal(y, _run(x, w, cfg, bias=b))                      # the partials do not change the output
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=34), 0.1 * _rand(cout, seed=35)
    sc, sh = ops.groupnorm_finalize(st, Ho * Wo, _d(gamma), _d(beta), 32, 1e-5)
    sc2, sh2 = ops.groupnorm_stats(y, _d(gamma), _d(beta), 32, 1e-5)
    yc = y.cpu().double()
    ref = F.group_norm(yc, 32, gamma.double(), beta.double(), 1e-5)
    for (s_, h_), name in (((sc, sh), "partials"), ((sc2, sh2), "stats pass")):
        got = yc * s_.cpu().double()[:, :, None, None] + h_.cpu().double()[:, :, None, None]
        _close(got.float(), ref, f"groupnorm from conv s2 bf16x3 cfg{cfg} {H}x{W} {name}")
    _close(sc, sc2.cpu().double(), f"groupnorm scale, partials vs stats pass, cfg{cfg} {H}x{W}")
    _close(sh, sh2.cpu().double(), f"groupnorm shift, partials vs stats pass, cfg{cfg} {H}x{W}")


# a ragged quarter-K share on whole tiles, and one chunk per wave (two waves idle) on fifteen tiles, some ragged
@pytest.mark.parametrize("cin,cout,H,W", [(40, 64, 16, 16), (16, 64, 34, 34)])
def test_batch_independence(cin, cout, H, W):
    x = _rand(3, cin, H, W, seed=41)
    w = _rand(cout, cin, 3, 3, seed=42, scale=0.1)
    b = _rand(cout, seed=43)
    y3, st3 = _run(x, w, 0, bias=b, with_stats=True)
    y1, st1 = _run(x[:1].contiguous(), w, 0, bias=b, with_stats=True)
    assert torch.equal(y3[:1], y1) and torch.equal(st3[:1], st1)
    _close(y3, _ref(x, w, b), f"conv s2 bf16x3 auto {cin}->{cout} {H}x{W} B3")


@pytest.mark.parametrize("cfg", [36])
def test_scale_sweep(cfg):
    """The semantics of test_bf16x3_scale_sweep (tests/test_gpu_kernels.py): inputs and weights scaled by 1e-6 ... 1e4 and
    magnitudes mixed over eight decades inside one reduction, relative to the largest output."""
    B, cin, cout, H, W = 2, 16, 64, 8, 8
    x0 = _rand(B, cin, H, W, seed=900 + cfg)
    w0 = _rand(cout, cin, 3, 3, seed=901 + cfg, scale=(9 * cin) ** -0.5)
    b0 = _rand(cout, seed=902 + cfg)
    for sx, sw in itertools.product((1e-6, 1e-3, 1e3, 1e4), repeat=2):
        x, w, b = x0 * sx, w0 * sw, b0 * (sx * sw)
        _rel_close(_run(x, w, cfg, bias=b), _ref(x, w, b), f"conv s2 bf16x3 cfg{cfg} inputs x{sx:g} weights x{sw:g}")
    g = torch.Generator().manual_seed(903 + cfg)
    mag = 10.0 ** (8.0 * torch.rand(cin, generator=g) - 4.0)
    xm = x0 * mag[None, :, None, None]
    _rel_close(_run(xm, w0, cfg, bias=b0), _ref(xm, w0, b0), f"conv s2 bf16x3 cfg{cfg} channel magnitudes 1e-4..1e4")
    wm = w0 / mag[None, :, None, None]
    _rel_close(_run(xm, wm, cfg, bias=b0), _ref(xm, wm, b0), f"conv s2 bf16x3 cfg{cfg} compensated magnitudes")
    pm = 10.0 ** (8.0 * torch.rand(B, 1, H, W, generator=g) - 4.0)
    xp = x0 * pm
    _rel_close(_run(xp, w0, cfg, bias=b0), _ref(xp, w0, b0), f"conv s2 bf16x3 cfg{cfg} pixel magnitudes 1e-4..1e4")


@pytest.mark.parametrize("cfg", [36])
def test_non_finite_inputs(cfg):
    """The semantics of test_bf16x3_non_finite_inputs: every output that fp32 arithmetic makes +-Inf or NaN is NaN here --
    never a finite number -- and every output that does not depend on the poisoned input keeps its bits (the zero padding is
    a select, never a product with a loaded value)."""
    B, cin, cout, H, W = 2, 16, 64, 8, 8
    x = _rand(B, cin, H, W, seed=910 + cfg)
    w = _rand(cout, cin, 3, 3, seed=911 + cfg, scale=(9 * cin) ** -0.5)
    clean = _run(x, w, cfg).cpu()
    for (py, px), bad in itertools.product(((5, 2), (0, 0), (H - 1, 3), (2, W - 1)), (float("inf"), float("-inf"), float("nan"))):
        xb = x.clone()
        xb[0, 3, py, px] = bad
        got = _run(xb, w, cfg).cpu()
        dep = ~torch.isfinite(F.conv2d(xb, w, stride=2, padding=1))     # the outputs fp32 arithmetic makes +-Inf / NaN
        win = torch.zeros(B, cout, H // 2, W // 2, dtype=torch.bool)    # = the outputs with the pixel in their window
        for oy, ox in itertools.product(range(H // 2), range(W // 2)):
            win[0, :, oy, ox] = abs(2 * oy - py) <= 1 and abs(2 * ox - px) <= 1
        assert torch.equal(dep, win) and dep.any()
        assert torch.isnan(got[dep]).all(), f"cfg{cfg} {bad} at {(py, px)}: a non-finite reference output came out finite"
        assert torch.equal(got[~dep], clean[~dep]), f"cfg{cfg} {bad} at {(py, px)}: an output outside the window changed"
    wb = w.clone()
    wb[7, 1, 0, 0] = float("nan")                                       # a NaN weight poisons its output channel only
    got = _run(x, wb, cfg).cpu()
    assert torch.isnan(got[:, 7]).all() and torch.equal(got[:, :7], clean[:, :7]) and torch.equal(got[:, 8:], clean[:, 8:])


def _switch_cases():
    """(name, kwargs of _run): arguments the bf16x3 form does not take, and one it does."""
    B, H, W = 2, 16, 16
    x = _rand(B, 16, H, W, seed=51)
    x2 = _rand(B, 8, H, W, seed=52)
    gn = (1.0 + 0.3 * _rand(B, 16, seed=53), 0.3 * _rand(B, 16, seed=54))
    w64, w48, w24 = (_rand(co, ci, 3, 3, seed=55 + co, scale=0.1) for co, ci in ((64, 16), (48, 16), (64, 24)))
    b64, b48 = _rand(64, seed=56), _rand(48, seed=57)
    return [("gn prologue", dict(x=x, w=w64, bias=b64, gn=gn)),
            ("c1 > 0", dict(x=x, w=w24, bias=b64, x2=x2)),
            ("Cout 48", dict(x=x, w=w48, bias=b48)),
            ("no split filter", dict(x=x, w=w64, bias=b64, split=False)),
            ("eligible", dict(x=x, w=w64, bias=b64))]


_SWITCH_CHILD = '''
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch
import test_gpu_conv_s2_bf3 as t
torch.save([t._run(kw.pop("x"), kw.pop("w"), 0, **kw).cpu() for _, kw in t._switch_cases()], sys.argv[1])
'''


def test_ineligible_arguments_stay_on_the_f32_kernel(tmp_path):
    """SISIC_S2_BF16X3 is read once per process: a fresh interpreter runs with SISIC_S2_BF16X3=0.  A GroupNorm prologue, a
    second input, Cout = 48 or no split filter give the f32 kernel's result bit for bit with and without the switch; the
    eligible case shows that the switch is what it says."""
    default = [_run(kw.pop("x"), kw.pop("w"), 0, **kw).cpu() for _, kw in _switch_cases()]
    script = tmp_path / "s2_child.py"
    script.write_text(_SWITCH_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ)
    env["SISIC_S2_BF16X3"] = "0"
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "off.pt")], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    off = torch.load(tmp_path / "off.pt")
    for (name, kw), a, b in zip(_switch_cases(), default, off):
        _close(a, _ref(kw["x"], kw["w"], bias=kw["bias"], gn=kw.get("gn"), x2=kw.get("x2")), f"conv s2 switch case: {name}")
        if name == "eligible":
            assert not torch.equal(a, b)                                # bf16x3 by default, the f32 kernel when switched off
            assert torch.equal(b, _run(kw["x"], kw["w"], 0, split=False, bias=kw["bias"]).cpu())
        else:
            assert torch.equal(a, b), name
    from synt_isic_amd._lib import SisicError
    with pytest.raises(SisicError, match="stride-2 bf16x3"):           # forcing the form on arguments it does not take is an error
        _run(_rand(1, 16, 8, 8), _rand(48, 16, 3, 3), 36)


def test_repack_after_an_optimizer_step(synthetic_sd):
    """After an optimizer step the batched re-layout (repack.hip) re-derives the downsamplers' split filters too: the next
    forward equals the forward of a freshly loaded model with the updated weights."""
    from synt_isic_amd.train import HipAdam, mse_loss
    from synt_isic_amd.unet import HipUNet2DModel

    def new_model(sd):
        m = HipUNet2DModel()
        m.load_state_dict(sd)
        return m.to(DEV)

    g = torch.Generator().manual_seed(61)
    x = torch.randn(1, 3, 32, 32, generator=g).to(DEV)
    target = torch.randn(1, 3, 32, 32, generator=g).to(DEV)
    t = torch.tensor([10], device=DEV)
    m = new_model(synthetic_sd)
    opt = HipAdam(m.parameters(), lr=1e-3)
    m.train()
    opt.zero_grad(set_to_none=True)
    mse_loss(m(x, t).sample, target).backward()
    opt.step()
    after = m.state_dict()
    names = [k for k in after if "downsamplers" in k and k.endswith("conv.weight")]
    assert len(names) == 3 and all(not torch.equal(after[k].cpu(), synthetic_sd[k]) for k in names)
    y = m.eval()(x, t).sample
    fresh = new_model(after)
    assert torch.equal(fresh.eval()(x, t).sample, y)
    assert not torch.equal(new_model(synthetic_sd).eval()(x, t).sample, y)
