"""Every kernel output the suite hands out is poisoned and guarded (tests/poison.py); this file asks the two questions that makes
possible, once per kernel form at the smallest ragged shape the form accepts: did the launch write EVERY element it owes
(``unwritten == 0`` on out, stats and both fin tensors) and NOTHING else (guard bands intact) -- next to the usual parity
against float64.  The last test does the same for the memory the executors allocate themselves, through the library switch
SISIC_POISON_ALLOC=1 in a fresh process: what a network computes must not depend on what its buffers held before.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ddim_ref
import philox_ref
import poison
import poison_exec
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)
from test_gpu_kernels import KTOL, _attn_ref, _close, _conv_ref, _rand
from test_gpu_train import _wgrad_geometry, _wgrad_inputs, _wgrad_run

pytestmark = pytest.mark.gpu

DEV = "cuda"
d = lambda t: None if t is None else t.to(DEV).contiguous()


# ---- the instrument, on the device ---------------------------------------------------------------------------------------
def test_instrument_counts_one_missing_element_on_the_device():
    from synt_isic_amd import ops
    for dtype in (torch.float32, torch.float64):
        t = ops.empty((3, 5, 7), dtype=dtype, device=DEV)
        assert t.is_cuda and t.data_ptr() % 512 == 0            # aligned as a fresh torch allocation: the production kernel forms
        assert poison.unwritten(t) == t.numel() and bool(torch.isnan(t).all())
        t.view(-1)[:-1] = 0.5
        assert poison.unwritten(t) == 1
        t.view(-1)[-1] = float("nan")                           # a NaN that was computed is not the pattern
        assert poison.unwritten(t) == 0
    u8 = ops.empty((4, 9), dtype=torch.uint8, device=DEV)
    assert bool((u8 == 0xA5).all())
    i32 = ops.empty_like(torch.zeros(6, dtype=torch.int32, device=DEV))
    assert i32.dtype == torch.int32 and bool((i32 == 0xA5A5A5A5 - (1 << 32)).all())
    assert not ops.empty(4, dtype=torch.float32, device="cpu").is_cuda and len(poison._live) == 4
    poison.check()


@pytest.mark.parametrize("where", ["before", "after"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint8])
def test_instrument_sees_a_store_one_element_outside_the_view_on_the_device(dtype, where):
    from synt_isic_amd import ops
    t = ops.empty((2, 3, 11), dtype=dtype, device=DEV)
    base, lo, hi = poison.base_of(t)
    e = t.element_size()
    base.view(dtype)[lo // e - 1 if where == "before" else hi // e] = 1         # a plain torch store
    with pytest.raises(AssertionError, match=r"\(2, 3, 11\).*test_gpu_poison.py.*" + ("below" if where == "before" else "above")):
        poison.check()
    t.zero_()                                                                   # writes inside the view are not the guards' business
    poison.check()


# ---- every tile configuration once, ragged -------------------------------------------------------------------------------
# id -> (ksize, stride, upsample, B, H, W, c0, c1, Cout, weights): the smallest ragged case the kernel behind the id accepts --
# B = 3, planes that are no multiple of the tile (and more than one tile where a row of the table allows it), Cout = 70 where the
# kernel takes a partly filled channel tile, a concatenated input where it takes one.  weights: "" direct packing only, "wino"
# + Winograd-domain filters, "s2" + the split stride-2 filter.
def _direct_cases():
    from_list = {}
    tilings = """1 3 1 64  2 3 1 32  3 3 1 16  4 3 1 8  5 3 1 16  6 3 1 64  7 3 1 32  8 3 1 32  9 3 1 16  10 3 1 32  14 3 1 16
                 15 3 1 8  16 3 1 8  17 3 1 8  11 3 2 32  12 3 2 16  13 3 2 8  18 3 2 8  19 3 2 8  21 1 1 256  22 1 1 64
                 23 1 1 128  24 1 1 256  25 1 1 128  26 1 1 256  27 1 1 128  31 1 2 32  32 1 2 16  33 1 2 8  41 7 2 32  42 7 2 32"""
    v = [int(s) for s in tilings.split()]                       # (id, ksize, stride, pixels of a tile row): conv_plan.h's list
    for cfg, k, stride, tw in zip(v[0::4], v[1::4], v[2::4], v[3::4]):
        if k == 1 and stride == 1:                              # the image is one flat row of H*W pixels
            H, W = (18, 23) if tw == 256 else (9, 23)           # 414 = 1.6 tiles of 256; 207 = 3.2 / 1.6 tiles of 64 / 128
        elif stride == 1:
            H, W = 9, tw + 7
        else:
            H, W = 18, 2 * (tw + 7) - 1                         # output 9 x (tw + 7)
        c0, c1 = (2, 1) if k == 7 else (20, 12)
        from_list[cfg] = (k, stride, False, 3, H, W, c0, c1, 70, "")
    return from_list


CONV_CASES = _direct_cases()
CONV_CASES.update({
    20: (1, 1, False, 3, 8, 16, 32, 32, 70, ""),                # whole 128-pixel tiles and 32-channel chunks only
    28: (1, 1, False, 3, 8, 24, 40, 24, 128, ""), 29: (1, 1, False, 3, 8, 24, 40, 24, 128, ""),     # whole 64 x 64 tiles only
    30: (1, 1, False, 3, 8, 24, 40, 24, 128, ""),
    34: (1, 1, False, 3, 8, 8, 40, 24, 384, ""),                # staged: 6 .. 12 channel items
    35: (1, 1, False, 3, 8, 24, 72, 56, 128, ""),               # K-split: a multiple of 128 input channels
    36: (3, 2, False, 3, 18, 45, 16, 0, 64, "s2"),              # one input, Cout % 64 == 0; output 9 x 23
    50: (3, 1, False, 3, 9, 35, 20, 12, 3, ""), 51: (3, 1, False, 3, 9, 35, 20, 12, 3, ""), 52: (3, 1, False, 3, 9, 35, 20, 12, 3, ""),
})
CONV_CASES.update({cfg: (3, 1, False, 3, 9, 23, 20, 12, 70, "wino") for cfg in (60, 62, 64, 66, 68, 69, 70, 71, 72, 73, 74, 78, 79)})
CONV_CASES.update({cfg: (3, 1, False, 3, 6, 10, 20, 12, 70, "wino") for cfg in (61, 63, 65, 67)})       # four images of <= 8x8 per workgroup
CONV_CASES.update({cfg: (3, 1, False, 3, 6, 7, 40, 24, 70, "wino") for cfg in (90, 91, 92)})            # 8 chunks split four ways

INTERFACE_IDS = (list(range(1, 20)) + list(range(21, 28)) + [31, 32, 33, 41, 42] + [20, 28, 29, 30, 34, 35, 36] + [50, 51, 52]
                 + list(range(60, 75)) + [78, 79] + [90, 91, 92])

# where the launch finalizes the GroupNorm over its own output (sisic_conv_finalizes): groups of eight channels held whole
FIN_CASES = [(74, 3, 9, 13, 20, 12, 64), (90, 3, 8, 8, 40, 24, 128), (91, 3, 8, 8, 40, 24, 128), (92, 3, 8, 8, 40, 24, 128)]


def test_the_case_table_covers_the_interface_list():
    assert sorted(CONV_CASES) == sorted(INTERFACE_IDS) and len(set(INTERFACE_IDS)) == len(INTERFACE_IDS) == 61


def _conv_inputs(k, stride, ups, B, H, W, c0, c1, cout, seed):
    x = _rand(B, c0, H, W, seed=seed)
    x2 = _rand(B, c1, H, W, seed=seed + 1) if c1 else None
    w = _rand(cout, c0 + c1, k, k, seed=seed + 2, scale=(k * k * (c0 + c1)) ** -0.5)
    b = _rand(cout, seed=seed + 3)
    return x, x2, w, b


def _launch(cfg, k, stride, ups, x, x2, w, b, weights, **kw):
    from synt_isic_amd import ops
    ww = ops.pack_winograd_weight(d(w)) if weights == "wino" else ops.pack_conv_s2_weight(d(w)) if weights == "s2" else None
    return ops.conv2d(d(x), ops.pack_conv_weight(d(w)), w.shape[0], k, bias=d(b), x2=d(x2), stride=stride, upsample=ups,
                      tile_cfg=cfg, w_winograd=ww, **kw)


def _check_stats(st, y, ref, what):
    """every slot written; the counts add up to the plane and the sums to the stored tensor's"""
    assert poison.unwritten(st) == 0, f"{what}: {poison.unwritten(st)} of {st.numel()} statistics elements were not written"
    stc = st.cpu().double()
    hw = ref.shape[2] * ref.shape[3]
    assert torch.equal(stc[..., 0].sum(-1), torch.full(stc.shape[:2], float(hw), dtype=torch.float64)), f"{what}: slot counts"
    _close(stc[..., 1].sum(-1).float() / hw, ref.mean((2, 3)), tol=KTOL, what=f"{what}: partial sums")
    assert bool(torch.isfinite(stc).all())


@pytest.mark.parametrize("cfg", sorted(CONV_CASES))
def test_every_tile_configuration_writes_its_whole_output_and_nothing_else(cfg):
    k, stride, ups, B, H, W, c0, c1, cout, weights = CONV_CASES[cfg]
    x, x2, w, b = _conv_inputs(k, stride, ups, B, H, W, c0, c1, cout, seed=1000 + 10 * cfg)
    y, st = _launch(cfg, k, stride, ups, x, x2, w, b, weights, with_stats=True)
    what = f"cfg {cfg}: {c0}+{c1}->{cout} k{k} s{stride} {B}x{H}x{W}"
    n = poison.unwritten(y)
    assert n == 0, f"{what}: {n} of {y.numel()} output elements were not written"
    ref = _conv_ref(x, w, b, x2=x2, stride=stride, upsample=ups)
    _close(y, ref, tol=KTOL, what=what)
    if 50 <= cfg <= 52:
        assert st is None                                       # the vector-ALU kernel leaves no partials, and says so
    else:
        assert st is not None
        _check_stats(st, y, ref, what)
    poison.check()


@pytest.mark.parametrize("cfg,B,H,W,c0,c1,cout", FIN_CASES)
def test_a_finalizing_launch_writes_both_fin_tensors(cfg, B, H, W, c0, c1, cout):
    x, x2, w, b = _conv_inputs(3, 1, False, B, H, W, c0, c1, cout, seed=2000 + cfg)
    gamma, beta = 1.0 + 0.1 * _rand(cout, seed=2001), 0.1 * _rand(cout, seed=2002)
    y, st, fin = _launch(cfg, 3, 1, False, x, x2, w, b, "wino", with_stats=True, finalize=(d(gamma), d(beta), cout // 8, 1e-5))
    what = f"cfg {cfg} finalizing {c0}+{c1}->{cout} {B}x{H}x{W}"
    assert fin is not None, f"{what}: sisic_conv_finalizes says no"
    assert poison.unwritten(y) == 0 and poison.unwritten(fin[0]) == 0 and poison.unwritten(fin[1]) == 0, what
    ref = _conv_ref(x, w, b, x2=x2)
    _close(y, ref, tol=KTOL, what=what)
    _check_stats(st, y, ref, what)
    yc = y.cpu().double()
    got = yc * fin[0].cpu().double()[:, :, None, None] + fin[1].cpu().double()[:, :, None, None]
    _close(got.float(), F.group_norm(yc, cout // 8, gamma.double(), beta.double(), 1e-5), tol=KTOL, what=what + ": GroupNorm")
    poison.check()


# a forced id on arguments its kernel does not take: the launch's own error, and nothing launched
REFUSALS = [(20, 1, 1, 3, 8, 8, 40, 0, 64, "", "pointwise"), (28, 1, 1, 3, 8, 8, 40, 0, 70, "", "pointwise bf16x3"),
            (34, 1, 1, 3, 8, 8, 64, 0, 128, "", "staged"), (35, 1, 1, 3, 8, 8, 64, 0, 128, "", "K-split"),
            (36, 3, 2, 3, 18, 10, 16, 8, 64, "s2", "stride-2 bf16x3"), (90, 3, 1, 3, 6, 7, 24, 0, 70, "wino", "split"),
            (91, 3, 1, 3, 8, 10, 32, 0, 64, "wino", "8x8"), (92, 3, 1, 3, 8, 10, 32, 0, 64, "wino", "8x8"),
            (68, 3, 1, 3, 9, 23, 20, 12, 70, "wino-ups", "upsample"), (4, 1, 1, 3, 9, 23, 20, 12, 70, "", "tile_cfg")]


@pytest.mark.parametrize("cfg,k,stride,B,H,W,c0,c1,cout,weights,match", REFUSALS)
def test_a_refused_launch_leaves_the_output_untouched(cfg, k, stride, B, H, W, c0, c1, cout, weights, match):
    from synt_isic_amd import ops
    from synt_isic_amd._lib import SisicError
    ups = weights == "wino-ups"
    x, x2, w, b = _conv_inputs(k, stride, ups, B, H, W, c0, c1, cout, seed=3000 + cfg)
    if weights == "s2":
        w_s2 = ops.pack_conv_s2_weight(d(w))
    Ho, Wo = ((H << int(ups)) + 2 * (k // 2) - k) // stride + 1, ((W << int(ups)) + 2 * (k // 2) - k) // stride + 1
    out = ops.empty((B, cout, Ho, Wo), dtype=torch.float32, device=DEV)
    with pytest.raises(SisicError, match=match):
        ops.conv2d(d(x), ops.pack_conv_weight(d(w)), cout, k, bias=d(b), x2=d(x2), stride=stride, upsample=ups, tile_cfg=cfg,
                   w_winograd=w_s2 if weights == "s2" else ops.pack_winograd_weight(d(w)) if weights.startswith("wino") else None,
                   out=out)
    assert poison.unwritten(out) == out.numel(), f"cfg {cfg}: a refused launch wrote {out.numel() - poison.unwritten(out)} elements"
    poison.check()


# ---- the other single operators, one ragged call each ------------------------------------------------------------------------
WGRAD_CASES = [((3, 20, 12, 70, 9, 23, 3, 1, False, True, True), "wino"), ((3, 40, 24, 70, 9, 23, 1, 1, False, True, False), "1x1"),
               ((3, 20, 12, 70, 9, 45, 3, 2, False, False, False), "direct2x16"), ((3, 20, 12, 70, 17, 9, 3, 2, False, False, False), "direct4x8")]


@pytest.mark.parametrize("case,form", WGRAD_CASES, ids=[f for _, f in WGRAD_CASES])
def test_conv_wgrad_writes_every_weight(case, form):
    assert _wgrad_geometry(*case[:9])[0] == form
    x, x2, g, dy, ref = _wgrad_inputs(*case)
    got = _wgrad_run(x, x2, g, dy, case[6], case[7], case[8], case[10])
    assert poison.unwritten(got) == 0
    _close(got, ref, what=f"conv wgrad {form}")
    poison.check()


_WGRAD_DIRECT = [(3, 20, 12, 70, 9, 23, 3, 1, False, True, True), (3, 20, 12, 70, 17, 7, 3, 1, False, False, False)]
_WGRAD_CHILD = '''
import sys
import torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import pytest
import poison
from test_gpu_train import _wgrad_inputs, _wgrad_run
poison.install(pytest.MonkeyPatch())
out = []
for case in {cases!r}:
    x, x2, g, dy, ref = _wgrad_inputs(*case)
    got = _wgrad_run(x, x2, g, dy, case[6], case[7], case[8], case[10])
    out.append((poison.unwritten(got), got.cpu(), ref))
poison.check()
torch.save(out, sys.argv[1])
'''


def test_conv_wgrad_direct_3x3_forms_write_every_weight_in_a_child_process(tmp_path):
    """direct4x16 / direct8x8 are what a 3x3 stride-1 gradient takes with SISIC_WGRAD_WINOGRAD=0, a switch read once per
    process: a fresh interpreter with the same poisoned allocations."""
    assert [_wgrad_geometry(*c[:9], winograd=False)[0] for c in _WGRAD_DIRECT] == ["direct4x16", "direct8x8"]
    tests = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "wgrad_direct_child.py"
    script.write_text(_WGRAD_CHILD.format(root=os.path.dirname(tests), tests=tests, cases=_WGRAD_DIRECT))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "out.pt")], env=dict(os.environ, SISIC_WGRAD_WINOGRAD="0"),
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    for (n, got, ref), form in zip(torch.load(tmp_path / "out.pt"), ("direct4x16", "direct8x8")):
        assert n == 0, f"{form}: {n} weight-gradient elements were not written"
        _close(got, ref, what=f"conv wgrad {form}")


@pytest.mark.parametrize("N", [33, 100, 513])
def test_attention_and_its_gradient_write_every_token(N):
    from synt_isic_amd import ops
    B, C = 3, 24
    qkv = _rand(B, 3 * C, N, seed=4000 + N) * 1.5
    dO = _rand(B, C, N, seed=4001 + N)
    q64 = qkv.double().requires_grad_(True)
    ref = _attn_ref(q64, C // 8)
    ref.backward(dO.double())
    out = ops.attention(d(qkv), 8)
    assert poison.unwritten(out) == 0
    _close(out, ref.detach(), tol=KTOL, what=f"attention N={N}")
    dqkv = ops.attention_bwd(d(qkv), out, d(dO))
    assert poison.unwritten(dqkv) == 0
    _close(dqkv, q64.grad, tol=KTOL, what=f"attention bwd N={N}")
    poison.check()


def test_groupnorm_operators_over_a_concatenation():
    from synt_isic_amd import ops
    B, c0, c1, H, W, G, eps = 3, 40, 24, 9, 7, 8, 1e-5
    x, x2 = _rand(B, c0, H, W, seed=4100) * 2.0 + 0.7, _rand(B, c1, H, W, seed=4101) - 1.5
    C = c0 + c1
    gamma, beta = 1.0 + 0.1 * _rand(C, seed=4102), 0.1 * _rand(C, seed=4103)
    full = torch.cat([x, x2], 1).double()
    ref = F.group_norm(full, G, gamma.double(), beta.double(), eps)
    apply = lambda sc, sh: (full * sc.cpu().double()[:, :, None, None] + sh.cpu().double()[:, :, None, None]).float()
    sc, sh = ops.groupnorm_stats(d(x), d(gamma), d(beta), G, eps, d(x2))
    assert poison.unwritten(sc) == 0 and poison.unwritten(sh) == 0
    _close(apply(sc, sh), ref, tol=KTOL, what="groupnorm_stats over a concatenation")
    # finalize: two producers with different slot counts
    wa, wb = _rand(c0, 16, 3, 3, seed=4104, scale=0.1), _rand(c1, 16, 3, 3, seed=4105, scale=0.1)
    xa, xb = _rand(B, 16, H, W, seed=4106), _rand(B, 16, H, W, seed=4107)
    ya, sa = ops.conv2d(d(xa), ops.pack_conv_weight(d(wa)), c0, 3, tile_cfg=66, w_winograd=ops.pack_winograd_weight(d(wa)), with_stats=True)
    yb, sb = ops.conv2d(d(xb), ops.pack_conv_weight(d(wb)), c1, 3, tile_cfg=4, with_stats=True)
    assert sa.shape[2] != sb.shape[2]
    sc, sh = ops.groupnorm_finalize(sa, H * W, d(gamma), d(beta), G, eps, stats2=sb)
    assert poison.unwritten(sc) == 0 and poison.unwritten(sh) == 0
    full = torch.cat([ya, yb], 1).cpu().double()
    _close(apply(sc, sh), F.group_norm(full, G, gamma.double(), beta.double(), eps), tol=KTOL, what="groupnorm_finalize over a concatenation")
    # backward (one tensor: the entry takes no second input), HW % 4 != 0
    xg = _rand(B, C, H, W, seed=4108) * 1.7 + 0.4
    da = _rand(B, C, H, W, seed=4109)
    x64, g64, b64 = xg.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.silu(F.group_norm(x64, G, g64, b64, eps=eps)).backward(da.double())
    dx, dg, db = ops.groupnorm_bwd(d(da), d(xg), d(gamma), d(beta), G, eps, True)
    assert poison.unwritten(dg) == 0 and poison.unwritten(db) == 0
    _close(dx, x64.grad, what="groupnorm bwd dx")
    _close(dg, g64.grad, what="groupnorm bwd dgamma")
    _close(db, b64.grad, what="groupnorm bwd dbeta")
    poison.check()


@pytest.mark.parametrize("n,B", [(105, 3), (3 * 32 * 32 + 1, 7)])
def test_scheduler_steps_write_every_element(n, B):
    """n = 105 and 3073: float4 bodies with a scalar tail; the generated-noise forms cut them into B images (35 / 439 values:
    no image starts on a 16-byte line)."""
    from oracle import ddpm as oddpm
    from synt_isic_amd import ops
    from synt_isic_amd.scheduler import HipDDPMScheduler
    assert n % B == 0
    eps, x, z = _rand(n, seed=4200 + n), _rand(n, seed=4201 + n) * 1.3, _rand(n, seed=4202 + n)
    o = oddpm.DDPMSchedulerOracle(); o.set_timesteps(50)
    s = HipDDPMScheduler(beta_schedule="squaredcos_cap_v2"); s.set_timesteps(50)
    coef = s.step_coefficients(500)
    got = ops.ddpm_step(d(eps), d(x), d(z), coef, 1.0)
    assert poison.unwritten(got) == 0 and torch.equal(got.cpu(), o.step(eps, 500, x, noise=z))
    row = (0.6, 0.8, 0.3, 0.69, 0.25)
    got = ops.ddim_step(d(eps), d(x), d(z), row, 1.0, False)
    assert poison.unwritten(got) == 0 and torch.equal(got.cpu(), ddim_ref.step_row(eps, x, z, row, 1.0, False))
    seeds, step = [5 + i * ((1 << 33) + 1) for i in range(B)], 17
    zd = ops.noise_fill(seeds, n // B, step)
    assert poison.unwritten(zd) == 0
    for b, sd in enumerate(seeds[:3]):
        zr, rad = philox_ref.noise_normals(sd, step, 0, n // B)
        assert (np.abs(zd[b].cpu().numpy().astype(np.float64) - zr) / np.maximum(1.0, rad)).max() <= 16 * 2.0 ** -23
    got = ops.ddpm_step_rng(d(eps), d(x), seeds, step, coef, 1.0)
    assert poison.unwritten(got) == 0 and torch.equal(got, ops.ddpm_step(d(eps), d(x), zd.reshape(-1), coef, 1.0))
    got = ops.ddim_step_rng(d(eps), d(x), seeds, step, row, 1.0, True)
    assert poison.unwritten(got) == 0 and torch.equal(got, ops.ddim_step(d(eps), d(x), zd.reshape(-1), row, 1.0, True))
    poison.check()


def test_denorm_and_add_noise_write_every_element():
    from oracle import ddpm as oddpm
    from oracle import sampler as osampler
    from synt_isic_amd import ops
    from synt_isic_amd.scheduler import HipDDPMScheduler
    x = _rand(3, 3, 9, 23, seed=4300) * 0.8
    u8 = ops.denorm_u8(d(x))
    assert np.array_equal(u8.cpu().numpy(), osampler.denormalize_to_uint8(x))
    # 0xA5 is a legal pixel: an image that is 0 everywhere (-1 before de-normalisation) shows a skipped store instead
    assert int(ops.denorm_u8(torch.full((3, 3, 9, 23), -1.0, device=DEV)).max()) == 0
    x0, nz = _rand(5, 3, 9, 23, seed=4301).clamp(-1, 1), _rand(5, 3, 9, 23, seed=4302)
    t = torch.tensor([0, 1, 500, 998, 999])
    got = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2").add_noise(d(x0), d(nz), t.to(DEV))
    assert poison.unwritten(got) == 0 and torch.equal(got.cpu(), oddpm.DDPMSchedulerOracle().add_noise(x0, nz, t))
    poison.check()


@pytest.mark.parametrize("entry,k", [("pack_conv_weight", 3), ("pack_conv_weight", 1), ("pack_winograd_weight", 3), ("pack_conv_s2_weight", 3)])
def test_pack_entries_write_the_whole_reported_numel_and_zero_padding(entry, k):
    """cout = 70 / cin = 19 leave partly filled channel tiles and chunks (the stride-2 split filter is packed at 64 / 24: its
    kernel takes whole 64-channel tiles only, so there the input channels' chunks of eight are whole and three of them leave no
    ragged lane -- that case shows 'written', not 'padding').  Every element of the reported numel is written, and the filter
    taps arrive, each as often as the layout stores it.  That the padding lanes are zero is shown indirectly: an all-zero
    filter packs to all-zero words (a lane that got anything but a tap or zero would show there or as a surplus tap)."""
    from synt_isic_amd import ops
    cout, cin = (64, 24) if entry == "pack_conv_s2_weight" else (70, 19)
    w = _rand(cout, cin, k, k, seed=4400 + k) + 3.0 * torch.sign(_rand(cout, cin, k, k, seed=4401 + k))       # no tap near zero
    packed = getattr(ops, entry)(d(w))
    assert poison.unwritten(packed) == 0, f"{poison.unwritten(packed)} of {packed.numel()} packed elements were not written"
    zero = getattr(ops, entry)(torch.zeros(cout, cin, k, k, device=DEV))
    assert zero.shape == packed.shape and int((zero.view(torch.int32) != 0).sum()) == 0, "padding (or an unwritten lane) is not zero"
    if entry == "pack_conv_weight" and k == 3:                  # one layout, [Cin_pad][9][Cout_pad]: every tap exactly once
        nz = packed[packed != 0].cpu()
        assert torch.equal(torch.sort(nz).values, torch.sort(w.reshape(-1)).values)
    elif entry == "pack_conv_weight":                           # 1x1: three layouts behind each other, the first two hold the taps as they are
        vals, counts = torch.unique(packed.cpu(), return_counts=True)
        hit = torch.isin(vals, w.reshape(-1))
        assert int(hit.sum()) == w.numel() and bool((counts[hit] == 2).all())
    elif entry == "pack_winograd_weight":                       # the f32 layout [Cin_pad][16][Cout_pad] comes first: U = G g G^T
        from synt_isic_amd import _lib
        first = packed[:_lib.load().sisic_conv_packed_numel(cout, cin, 3) // 9 * 16].cpu()
        nz = first[first != 0]
        assert nz.numel() == 16 * cout * cin and bool(torch.isfinite(packed).all())
        g = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
        assert abs(float(nz.double().abs().sum()) / float((g @ w.double() @ g.T).abs().sum()) - 1) < 1e-5
    poison.check()


# ---- the executors' own memory -----------------------------------------------------------------------------------------------
def test_executors_do_not_depend_on_what_their_buffers_held(tmp_path, golden_dir):
    """SISIC_POISON_ALLOC=1 in a fresh process fills every pool block, derived weight, grown row, scratch slab and training
    buffer with NaN bytes before use.  The switch changes no launch and no address order, so the results are the same BITS as
    this process computes without it -- anything else read memory nobody wrote."""
    import time
    t0 = time.time()
    child_dir, here_dir = tmp_path / "poisoned", tmp_path / "plain"
    child_dir.mkdir(); here_dir.mkdir()
    r = subprocess.run([sys.executable, os.path.abspath(poison_exec.__file__), str(child_dir)], timeout=600, capture_output=True,
                       text=True, env=dict(os.environ, SISIC_POISON_ALLOC="1"))
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    t1 = time.time()
    poison_exec.run(str(here_dir))
    names = sorted(os.listdir(here_dir))
    assert names == sorted(os.listdir(child_dir)) and len(names) == 4 + 6 + 2 + 8 + 6
    # the switch was read: it forces graph mode off, so the child's latency-mode run built no graph where this process built one
    builds = "latency_graph_builds.npy"
    assert int(np.load(child_dir / builds)) == 0 and int(np.load(here_dir / builds)) >= 1
    names.remove(builds)
    differ = []
    for name in names:
        a, b = np.load(child_dir / name), np.load(here_dir / name)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if not np.isfinite(a.astype(np.float64)).all():
            differ.append(f"{name}: {int((~np.isfinite(a.astype(np.float64))).sum())} non-finite elements under poison")
        elif not np.array_equal(a, b):
            differ.append(f"{name}: {int((a != b).sum())} of {a.size} elements differ, max |d| {np.abs(a.astype(np.float64) - b).max():.3e}")
    print(f"poisoned child {t1 - t0:.1f} s, the same in this process {time.time() - t1:.1f} s")
    assert not differ, "results change when the executors' buffers start as NaN:\n  " + "\n  ".join(differ)
    gold = np.load(os.path.join(golden_dir, "unet_forward_b2_64.npz"))
    err = float(np.abs(np.load(child_dir / "unet_default_b2_64.npy") - gold["y"]).max())
    assert err <= 2e-4 and err <= 4e-5, f"poisoned forward vs golden: {err:.3e}"           # test_gpu_unet.py's FWD_TOL and FWD_GUARD
