"""The training step (diffusion/train_diffusion.py:201-266) on the HIP kernels.

Parity: every backward kernel against torch.autograd over a float64 evaluation of the same op (per-kernel bound
1e-5 * max(1,|ref|)); the whole step at B=2, 3x64x64 against torch.autograd over the CPU oracle (oracle/train.py): every
one of the 330 parameter gradients within 1e-4 of THAT TENSOR's own largest reference gradient (measured on MI355X:
worst 1.5e-5, median 6e-6 -- profiles/r02/test_errors.txt; the fp32 CPU oracle itself sits 5e-6 from its float64
evaluation), median over the tensors <= 5e-5, and the weights after one Adam step within fp32 rounding of
torch.optim.Adam's.  Bit-exact: add_noise, run-to-run determinism (no atomics in the backward pass).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5
GRAD_REL_WORST = 1e-4        # per parameter tensor: max|g - ref| / max|ref|   (measured 1.5e-5)
GRAD_REL_MEDIAN = 5e-5       # median of that over the 324 tensors with a non-zero gradient (measured 6e-6)
PRED_TOL = 5e-5              # the training-mode forward against the oracle's prediction (stated 2e-4; measured ~4e-6)


def _grad_errors(grads, ref_grads, label):
    """(worst, median) of the per-tensor relative gradient error.  to_k.bias has an identically zero gradient (softmax is
    invariant to a shift of the keys' scores): tensors whose reference gradient is below 1e-8 must be below 1e-8 too and are
    left out of the relative measure."""
    rel = []
    for n, r in ref_grads.items():
        scale = r.abs().max().item()
        err = (grads[n] - r).abs().max().item()
        if scale <= 1e-8:
            assert err <= 1e-7, f"{label}: gradient of {n} should vanish, got {err:.3e}"
            continue
        rel.append((err / scale, n))
    rel.sort()
    worst, median = rel[-1], rel[len(rel) // 2]
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(f"{median[0]:.3e}\t{worst[0]:.3e}\trelative gradient error {label}: median / max over {len(rel)} tensors (worst: {worst[1]})\n")
    return worst, median


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(got, ref64, tol=KTOL, what=""):
    got = got.detach().cpu().double()
    bound = tol * max(1.0, ref64.abs().max().item())
    err = (got - ref64).abs().max().item()
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(f"{err / max(1.0, ref64.abs().max().item()):.3e}\t{tol:.1e}\t{what}\n")
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert err <= bound, f"{what}: max abs err {err:.3e} > {bound:.3e}"


def _act64(x, x2, gn, silu, upsample):
    x = x.double()
    if x2 is not None:
        x = torch.cat([x, x2.double()], 1)
    if gn is not None:
        x = x * gn[0].double()[:, :, None, None] + gn[1].double()[:, :, None, None]
        if silu:
            x = F.silu(x)
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return x


@pytest.mark.parametrize("B,c0,c1,cout,H,W,k,stride,ups,gn,silu", [
    (2, 64, 0, 64, 64, 64, 3, 1, False, True, True),       # ResBlock conv at full resolution
    (2, 20, 12, 70, 18, 10, 3, 1, False, True, True),      # concat seam inside a tile, ragged edges, Cout % 64 != 0
    (3, 40, 0, 33, 8, 8, 3, 1, False, False, False),       # 8x8 level
    (2, 96, 32, 128, 16, 16, 3, 1, False, True, False),
    (2, 24, 0, 64, 10, 14, 3, 1, True, False, False),      # nearest-2x upsampler
    (2, 64, 0, 64, 32, 32, 3, 2, False, False, False),     # stride-2 downsampler
    (2, 48, 0, 40, 12, 20, 3, 2, False, False, False),
    (2, 64, 64, 128, 16, 16, 1, 1, False, False, False),   # 1x1 shortcut over a concatenation
    (2, 256, 0, 768, 8, 8, 1, 1, False, True, False),      # fused q/k/v projection (GroupNorm prologue, no SiLU)
    (1, 3, 0, 64, 32, 32, 3, 1, False, False, False),      # conv_in
    (2, 64, 0, 3, 32, 32, 3, 1, False, True, True),        # conv_out
])
def test_conv_wgrad(B, c0, c1, cout, H, W, k, stride, ups, gn, silu):
    from synt_isic_amd import ops
    x = _rand(B, c0, H, W, seed=1)
    x2 = _rand(B, c1, H, W, seed=2) if c1 else None
    g = (1.0 + 0.3 * _rand(B, c0 + c1, seed=3), 0.3 * _rand(B, c0 + c1, seed=4)) if gn else None
    a = _act64(x, x2, g, silu, ups)
    w = torch.zeros(cout, c0 + c1, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a, w, stride=stride, padding=k // 2)
    dy = _rand(*y.shape, seed=5)
    y.backward(dy.double())
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    got = ops.conv2d_wgrad(d(x), d(dy), k, x2=d(x2), stride=stride, upsample=ups, gn_scale=d(g[0]) if gn else None,
                           gn_shift=d(g[1]) if gn else None, gn_silu=silu)
    _close(got, w.grad, what=f"conv wgrad {c0}+{c1}->{cout} k{k} s{stride} ups{int(ups)} {H}x{W}")
    assert torch.equal(got, ops.conv2d_wgrad(d(x), d(dy), k, x2=d(x2), stride=stride, upsample=ups,
                                             gn_scale=d(g[0]) if gn else None, gn_shift=d(g[1]) if gn else None,
                                             gn_silu=silu))          # fixed-order K-split reduction: bit-reproducible


def _cdiv(a, b):
    return -(-a // b)


def _wgrad_geometry(B, c0, c1, cout, H, W, k, stride, ups, winograd=True):
    """(form, nblocks, ksplit, blocks_per_slice) of launch_conv_wgrad: restates wgrad_ksplit (train_kernels.hip:360-367),
    wgrad_wino_ksplit (wgrad_winograd.inc:341-345) and the two slice-count lines after each (blocks_per_slice =
    cdiv(nblocks, ksplit); ksplit = cdiv(nblocks, blocks_per_slice)) in launch_wgrad_cfg and launch_wgrad_wino.
    winograd=False: the SISIC_WGRAD_WINOGRAD=0 route of a 3x3 stride-1 convolution."""
    Hc, Wc = H << int(ups), W << int(ups)
    Hout, Wout = (Hc + 2 * (k // 2) - k) // stride + 1, (Wc + 2 * (k // 2) - k) // stride + 1
    tiles = _cdiv(cout, 64) * _cdiv(c0 + c1, 64)
    if k == 3 and stride == 1 and winograd:
        form, tr, tc = "wino", 4, 8
        ksplit = max(1, min(B * _cdiv(Hout, 4) * _cdiv(Wout, 8), _cdiv(256, tiles)))
    else:
        ksplit = max(1, min(B * _cdiv(Hout, 8) * _cdiv(Wout, 8), _cdiv(1024 if k == 1 else 256, tiles)))
        if k == 1:                                   # flat pixel rows: one row of H*W pixels per image
            form, tr, tc, Hout, Wout = "1x1", 1, 64, 1, Hout * Wout
        elif stride == 2:
            form, tr, tc = ("direct2x16", 2, 16) if Wout > 8 else ("direct4x8", 4, 8)
        else:
            form, tr, tc = ("direct4x16", 4, 16) if Wout > 8 else ("direct8x8", 8, 8)
    nblocks = B * _cdiv(Hout, tr) * _cdiv(Wout, tc)
    blocks_per_slice = _cdiv(nblocks, ksplit)
    return form, nblocks, _cdiv(nblocks, blocks_per_slice), blocks_per_slice


def _wgrad_coverage(B, c0, c1, cout, H, W, k, stride, ups, winograd=True):
    """(form, the K-split situations a case reaches): loop = a slice walks >= 2 blocks (the pipelined staging loop reuses
    its LDS buffers), ragged = the last slice is shorter, cross = slices straddle an image boundary, cap = the slab count
    sits at its cap, scalar = Cout*Cin*k*k % 4 != 0 sends the direct forms' slab sum to the scalar wgrad_reduce_kernel."""
    form, nblocks, ksplit, bps = _wgrad_geometry(B, c0, c1, cout, H, W, k, stride, ups, winograd)
    covers = set()
    if bps >= 2:
        covers.add("loop")
    if nblocks % bps:
        covers.add("ragged")
    if B > 1 and (nblocks // B) % bps:
        covers.add("cross")
    if ksplit == (1024 if k == 1 else 256):
        covers.add("cap")
    if form != "wino" and (cout * (c0 + c1) * k * k) % 4:
        covers.add("scalar")
    return form, covers


def _wgrad_inputs(B, c0, c1, cout, H, W, k, stride, ups, gn, silu):
    """(x, x2, (gn_scale, gn_shift) or None, dy, float64 reference dW) of one weight-gradient case"""
    x = _rand(B, c0, H, W, seed=1)
    x2 = _rand(B, c1, H, W, seed=2) if c1 else None
    g = (1.0 + 0.3 * _rand(B, c0 + c1, seed=3), 0.3 * _rand(B, c0 + c1, seed=4)) if gn else None
    a = _act64(x, x2, g, silu, ups)
    w = torch.zeros(cout, c0 + c1, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a, w, stride=stride, padding=k // 2)
    dy = _rand(*y.shape, seed=5)
    y.backward(dy.double())
    return x, x2, g, dy, w.grad


def _wgrad_run(x, x2, g, dy, k, stride, ups, silu):
    from synt_isic_amd import ops
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    return ops.conv2d_wgrad(d(x), d(dy), k, x2=d(x2), stride=stride, upsample=ups, gn_scale=d(g[0]) if g else None,
                            gn_shift=d(g[1]) if g else None, gn_silu=silu)


# (B, c0, c1, cout, H, W, k, stride, ups, gn, silu), the form it takes, the K-split situations it is there for
WGRAD_LOOP_CASES = [
    # the batch-32 training shapes (3x64x64 input)
    ((32, 64, 0, 64, 64, 64, 3, 1, False, True, True), "wino", {"loop", "cap"}),              # 64^2 ResBlock conv: 256 slabs
    ((32, 128, 0, 128, 32, 32, 3, 1, False, True, True), "wino", {"loop"}),
    ((32, 256, 0, 256, 16, 16, 3, 1, False, True, True), "wino", {"loop", "cross"}),
    ((32, 256, 0, 256, 8, 8, 3, 1, False, True, True), "wino", {"loop", "cross"}),           # the 8x8 level
    ((32, 256, 256, 256, 8, 8, 3, 1, False, True, True), "wino", {"loop", "cross"}),         # its up-path concatenation
    ((32, 256, 0, 256, 8, 8, 3, 1, True, False, False), "wino", {"loop", "cross"}),          # nearest-2x upsampler 8 -> 16
    ((32, 64, 0, 64, 64, 64, 3, 2, False, False, False), "direct2x16", {"loop", "cap"}),     # stride-2 downsampler
    ((32, 256, 0, 768, 16, 16, 1, 1, False, True, False), "1x1", {"loop", "ragged", "cross"}),  # q/k/v: 128 blocks / 22 slices
    ((32, 64, 0, 64, 64, 64, 1, 1, False, False, False), "1x1", {"loop", "cap"}),            # 1024 slabs
    ((32, 128, 64, 128, 32, 32, 1, 1, False, False, False), "1x1", {"loop", "ragged", "cross"}),  # 512 blocks / 171 slices
    # small shapes that reach the remaining situations
    ((27, 20, 12, 70, 17, 4, 3, 1, False, True, True), "wino", {"loop", "ragged", "cross"}),  # concat seam inside a tile
    ((29, 24, 0, 64, 5, 9, 3, 1, True, False, False), "wino", {"loop", "ragged", "cross"}),   # nearest-2x, ragged
    ((29, 40, 0, 33, 33, 4, 3, 1, False, False, False), "wino", {"loop", "ragged", "cross"}),  # plain input
    ((3, 48, 0, 40, 9, 17, 3, 2, False, False, False), "direct2x16", {"loop", "ragged", "cross"}),
    ((3, 48, 0, 40, 17, 4, 3, 2, False, False, False), "direct4x8", {"loop", "ragged", "cross"}),
    ((3, 33, 0, 21, 17, 4, 3, 2, False, True, True), "direct4x8", {"loop", "ragged", "scalar"}),  # 6237 weights: scalar sum
]


@pytest.mark.parametrize("case,form,covers", WGRAD_LOOP_CASES,
                         ids=[f"{c[0]}x{c[1]}+{c[2]}-{c[3]}@{c[4]}x{c[5]}k{c[6]}s{c[7]}u{int(c[8])}" for c, _, _ in WGRAD_LOOP_CASES])
def test_conv_wgrad_k_split_slices(case, form, covers):
    """Weight gradients whose K-split slices walk several blocks (ragged, across images, at the slab cap) against float64:
    the per-slice staging loop, its LDS reuse across iterations and the eight-segment slab sums at batch-32 lengths."""
    B, c0, c1, cout, H, W, k, stride, ups, gn, silu = case
    got_form, got_covers = _wgrad_coverage(B, c0, c1, cout, H, W, k, stride, ups)
    assert got_form == form and covers <= got_covers, (got_form, sorted(got_covers))
    x, x2, g, dy, ref = _wgrad_inputs(*case)
    got = _wgrad_run(x, x2, g, dy, k, stride, ups, silu)
    _close(got, ref, what=f"conv wgrad B{B} {c0}+{c1}->{cout} k{k} s{stride} ups{int(ups)} {H}x{W} ({form})")
    assert torch.equal(got, _wgrad_run(x, x2, g, dy, k, stride, ups, silu))     # fixed-order K-split reduction


def test_conv_wgrad_k_split_coverage():
    """Between them the cases above reach every situation on every form they are meant for."""
    reached = {}
    for case, form, covers in WGRAD_LOOP_CASES:
        reached.setdefault(form, set()).update(covers)
    assert {"loop", "ragged", "cross", "cap"} <= reached["wino"]
    assert {"loop", "ragged", "cross", "cap"} <= reached["1x1"]
    assert {"loop", "ragged"} <= reached["direct2x16"] and {"loop", "ragged", "scalar"} <= reached["direct4x8"]
    wino_inputs = [c for c, f, cov in WGRAD_LOOP_CASES if f == "wino" and "loop" in cov]
    assert any(c[2] > 0 and c[1] % 64 for c in wino_inputs)          # concatenation, seam inside a 64-channel tile
    assert any(c[9] and c[10] for c in wino_inputs)                   # GroupNorm + SiLU prologue
    assert any(c[8] for c in wino_inputs)                             # nearest 2x
    assert any(not c[9] and not c[8] and not c[2] for c in wino_inputs)  # plain


@pytest.mark.parametrize("B,C,N", [(2, 256, 64), (1, 128, 256), (2, 64, 1024), (1, 32, 100),
                                   (2, 256, 1024),     # the 32x32 attention level of the reference's 128x128 training
                                   (1, 256, 1156),     # 136x136: the largest square training resolution
                                   (1, 32, 1170)])     # the most tokens whose key/value rows fit the LDS
def test_attention_bwd(B, C, N):
    from synt_isic_amd import ops
    qkv = _rand(B, 3 * C, N, seed=10)
    dO = _rand(B, C, N, seed=11)
    q64 = qkv.double().requires_grad_(True)
    heads = C // 8
    q, k, v = (t.reshape(B, heads, 8, N).transpose(2, 3) for t in q64.chunk(3, dim=1))
    p = torch.softmax(q @ k.transpose(-1, -2) * 8 ** -0.5, dim=-1)
    o = (p @ v).transpose(2, 3).reshape(B, C, N)
    o.backward(dO.double())
    out = ops.attention(qkv.to(DEV))
    got = ops.attention_bwd(qkv.to(DEV), out, dO.to(DEV))
    _close(got, q64.grad, what=f"attention bwd C={C} N={N}")


def test_attention_bwd_refuses_more_tokens_than_fit_the_lds():
    """1171 tokens: a host-side argument check answers SISIC_EINVAL; nothing is launched."""
    from synt_isic_amd import _lib, ops
    qkv = torch.zeros(1, 3 * 32, 1171, device=DEV)
    out = torch.zeros(1, 32, 1171, device=DEV)
    with pytest.raises(_lib.SisicError) as e:
        ops.attention_bwd(qkv, out, torch.zeros_like(out))
    assert e.value.code == _lib.SISIC_EINVAL and "1170" in str(e.value)


@pytest.mark.parametrize("B,C,H,W,silu", [(2, 64, 16, 16, True), (3, 128, 8, 8, False), (2, 320, 10, 6, True),
                                          (32, 64, 64, 64, True),     # the 64x64 level at the training batch
                                          (3, 64, 5, 7, True),        # HW % 4 != 0: the scalar paths
                                          (2, 128, 9, 9, False),
                                          (2, 512, 8, 8, True)])      # 16 channels per group, the decoder's widest
def test_groupnorm_bwd(B, C, H, W, silu):
    from synt_isic_amd import ops
    x = _rand(B, C, H, W, seed=20) * 1.7 + 0.4
    gamma, beta = 1.0 + 0.2 * _rand(C, seed=21), 0.2 * _rand(C, seed=22)
    da = _rand(B, C, H, W, seed=23)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = F.group_norm(x64, 32, g64, b64, eps=1e-5)
    if silu:
        a = F.silu(a)
    a.backward(da.double())
    dx, dg, db = ops.groupnorm_bwd(da.to(DEV), x.to(DEV), gamma.to(DEV), beta.to(DEV), 32, 1e-5, silu)
    _close(dx, x64.grad, what="groupnorm bwd dx")
    _close(dg, g64.grad, what="groupnorm bwd dgamma")
    _close(db, b64.grad, what="groupnorm bwd dbeta")


def test_add_noise_bit_exact():
    """scheduler.add_noise (train_diffusion.py:217): same fp32 products and sum as the published torch expression."""
    from oracle import ddpm as oddpm
    from synt_isic_amd.scheduler import HipDDPMScheduler
    x0 = _rand(5, 3, 32, 32, seed=30).clamp(-1, 1)
    nz = _rand(5, 3, 32, 32, seed=31)
    t = torch.tensor([0, 1, 500, 998, 999])
    s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    got = s.add_noise(x0.to(DEV), nz.to(DEV), t.to(DEV)).cpu()
    assert torch.equal(got, oddpm.DDPMSchedulerOracle().add_noise(x0, nz, t))


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(77)
    images = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1)
    noise = torch.randn(2, 3, 64, 64, generator=g)
    timesteps = torch.tensor([37, 912])
    return images, noise, timesteps


@pytest.fixture(scope="module")
def reference(synthetic_sd, batch):
    from oracle import train as otrain
    loss, grads, pred = otrain.loss_and_grads(synthetic_sd, *batch)
    return loss, grads, pred


def _new_model(sd):
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel()
    m.load_state_dict(sd)
    return m.to(DEV)


def test_unet_gradients_match_autograd_over_the_oracle(synthetic_sd, batch, reference):
    """B=2, 3x64x64: loss, prediction and every one of the 330 parameter gradients of one training batch against
    torch.autograd over the CPU oracle; the reference's loop spelled with the Hip* stand-ins."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    images, noise, timesteps = (t.to(DEV) for t in batch)
    ref_loss, ref_grads, ref_pred = reference
    model = _new_model(synthetic_sd)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    model.train()
    noisy = scheduler.add_noise(images, noise, timesteps)
    noise_pred = model(noisy, timesteps).sample
    assert (noise_pred.cpu() - ref_pred).abs().max().item() <= PRED_TOL
    model.eval()
    assert torch.equal(model(noisy, timesteps).sample, noise_pred)        # the tape-recording forward IS the forward
    model.train()
    noise_pred = model(noisy, timesteps).sample
    loss = mse_loss(noise_pred, noise)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    grads = model.grads()
    assert list(grads) == list(ref_grads) and len(grads) == 330
    worst, median = _grad_errors(grads, ref_grads, "B2 64x64")
    assert worst[0] <= GRAD_REL_WORST, f"gradient of {worst[1]}: {worst[0]:.3e} of its own largest entry"
    assert median[0] <= GRAD_REL_MEDIAN, median
    # bit-reproducible: a second forward/backward of the same batch gives the same gradients
    noise_pred2 = model(noisy, timesteps).sample
    mse_loss(noise_pred2, noise).backward()
    again = model.grads()
    assert all(torch.equal(again[n], grads[n]) for n in grads)


def test_unet_gradients_in_latency_mode(synthetic_sd, batch, reference):
    """The reference trains with batch 2 (train_diffusion.py:59): set_latency_mode picks the small-batch tilings for the
    forward AND the data-gradient convolutions (K-split Winograd, 64-pixel 1x1 tiles).  Same parity bar as the default mode."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    images, noise, timesteps = (t.to(DEV) for t in batch)
    ref_loss, ref_grads, ref_pred = reference
    model = _new_model(synthetic_sd).set_latency_mode(True)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    model.train()
    noise_pred = model(scheduler.add_noise(images, noise, timesteps), timesteps).sample
    assert (noise_pred.cpu() - ref_pred).abs().max().item() <= PRED_TOL
    loss = mse_loss(noise_pred, noise)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    grads = model.grads()
    worst, median = _grad_errors(grads, ref_grads, "B2 64x64 latency mode")
    assert worst[0] <= GRAD_REL_WORST and median[0] <= GRAD_REL_MEDIAN, (worst, median)


def test_unet_gradients_at_a_ragged_resolution(synthetic_sd):
    """The same comparison at B=3, 3x40x56 (20x28 / 10x14 / 5x7 below): ragged tiles in every backward kernel, the direct
    convolution kernels at the small levels, attention over 280 and 35 tokens."""
    from oracle import train as otrain
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    g = torch.Generator().manual_seed(78)
    images = torch.rand(3, 3, 40, 56, generator=g) * 2 - 1
    noise = torch.randn(3, 3, 40, 56, generator=g)
    timesteps = torch.tensor([0, 500, 999])
    ref_loss, ref_grads, _ = otrain.loss_and_grads(synthetic_sd, images, noise, timesteps)
    model = _new_model(synthetic_sd)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    HipAdam(model.parameters(), lr=1e-4)
    model.train()
    noisy = scheduler.add_noise(images.to(DEV), noise.to(DEV), timesteps.to(DEV))
    loss = mse_loss(model(noisy, timesteps.to(DEV)).sample, noise.to(DEV))
    loss.backward()
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    grads = model.grads()
    worst, median = _grad_errors(grads, ref_grads, "B3 40x56")
    assert worst[0] <= GRAD_REL_WORST and median[0] <= GRAD_REL_MEDIAN, (worst, median)


def test_one_adam_step_matches_torch_adam(synthetic_sd, batch, reference):
    """scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update() (train_diffusion.py:231-233) against
    torch.optim.Adam(lr=1e-4) over the oracle's gradients: after step 1 every weight has moved by ~lr * sign(grad), so the
    comparison is in units of lr; then the Adam kernel alone against torch.optim.Adam on IDENTICAL gradients (fp32 rounding)."""
    from oracle import train as otrain
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, mse_loss
    images, noise, timesteps = (t.to(DEV) for t in batch)
    _, ref_grads, _ = reference
    model = _new_model(synthetic_sd)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    scaler = HipGradScaler()
    model.train()
    loss = mse_loss(model(scheduler.add_noise(images, noise, timesteps), timesteps).sample, noise)
    optimizer.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    scaled = model.grads()
    assert scaler.step(optimizer) is True
    scaler.update()
    assert scaler.get_scale() == 65536.0
    after = model.state_dict()
    assert model.optimizer_state()["step"] == 1
    # (a) loss scaling by 65536 is exact in fp32 (a power of two): the scaled gradients are 65536 x the unscaled ones
    ref_new, _ = otrain.adam_step(synthetic_sd, ref_grads)
    big = 0.0
    for name in ref_new:
        move_ref = ref_new[name] - synthetic_sd[name]
        move = after[name].cpu() - synthetic_sd[name]
        # where |grad| >> eps the first Adam step is lr * sign(grad): compare the moves where the reference gradient is
        # clear of the noise floor of the gradient parity (1e-4 * max(1,|g|))
        clear = ref_grads[name].abs() > 1e-3 * max(1.0, ref_grads[name].abs().max().item())
        if clear.any():
            big = max(big, (move - move_ref)[clear].abs().max().item())
    assert big <= 2e-7, f"largest difference of a weight move: {big:.3e} (lr = 1e-4)"
    # (b) the Adam kernel on identical gradients: feed torch.optim.Adam the GPU's own (unscaled) gradients
    unscaled = {k: v / 65536.0 for k, v in scaled.items()}
    same_new, _ = otrain.adam_step(synthetic_sd, unscaled)
    worst = max((after[k].cpu() - same_new[k]).abs().max().item() for k in same_new)
    assert worst <= 3e-9 + 2 ** -22, f"Adam kernel vs torch.optim.Adam on the same gradients: {worst:.3e}"
    st = model.optimizer_state()
    k = "mid_block.resnets.0.conv1.weight"
    assert torch.allclose(st["exp_avg"][k], (1 - 0.9) * unscaled[k], rtol=1e-6, atol=1e-30)
    assert torch.allclose(st["exp_avg_sq"][k], (1 - 0.999) * unscaled[k] ** 2, rtol=1e-6, atol=1e-30)


def test_grad_scaler_skips_a_step_with_non_finite_gradients(synthetic_sd, batch):
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, mse_loss
    images, noise, timesteps = (t.to(DEV) for t in batch)
    model = _new_model(synthetic_sd)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    scaler = HipGradScaler(init_scale=3.0e38)                      # overflows the scaled gradients
    model.train()
    loss = mse_loss(model(scheduler.add_noise(images, noise, timesteps), timesteps).sample, noise)
    scaler.scale(loss).backward()
    assert scaler.step(optimizer) is False                         # skipped
    scaler.update()
    assert scaler.get_scale() == 1.5e38 and model.optimizer_state()["step"] == 0
    after = model.state_dict()
    assert all(torch.equal(after[k].cpu(), synthetic_sd[k]) for k in synthetic_sd)


def test_training_loop_overfits_one_batch_and_fused_step_agrees(synthetic_sd, tmp_path):
    """train_class (train_diffusion.py:187-266) on a loader of one fixed batch: the loss falls, the best checkpoint is a
    loadable state dict, the fused sisic_unet_train_step takes the same steps as the spelled-out loop, and the trained
    weights sample (eval mode) without touching the training state."""
    from synt_isic_amd.train import train_class
    g = torch.Generator().manual_seed(5)
    images = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    loader = [images] * 4

    def run(fused):
        m = _new_model(synthetic_sd)
        hist = train_class(m, loader, "NV", epochs=3, lr=1e-4, checkpoint_dir=str(tmp_path / ("f" if fused else "s")),
                           fused=fused, generator=torch.Generator().manual_seed(9), log=None)
        return m, hist

    m1, h1 = run(True)
    m2, h2 = run(False)
    assert len(h1) == 3 and h1[-1] < h1[0], h1
    assert np.allclose(h1, h2, rtol=1e-6, atol=0), (h1, h2)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert any(not torch.equal(sd1[k].cpu(), synthetic_sd[k]) for k in sd1)
    ck = torch.load(str(tmp_path / "f" / "unet_NV_best.pth"))
    m3 = _new_model(ck)
    x = torch.randn(1, 3, 32, 32, generator=g).to(DEV)
    assert torch.equal(m3.eval()(x, 10).sample, m1.eval()(x, 10).sample)
    # m1's filters were re-laid out by the batched launches that follow every optimizer step (repack.hip), m3's by the load
    # path's one launch per tensor: the same bits forward (above) and through the backward-data / weight-gradient pass
    from synt_isic_amd.train import HipAdam, mse_loss
    t = torch.tensor([10], device=DEV)
    target = torch.randn(1, 3, 32, 32, generator=g).to(DEV)
    grads = []
    for m in (m1, m3):
        m.train()
        HipAdam(m.parameters(), lr=1e-4).zero_grad()
        mse_loss(m(x, t).sample, target).backward()
        grads.append(m.grads())
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])


def test_a_shape_change_or_a_graph_replayed_run_invalidates_the_tape(synthetic_sd, batch):
    """the recorded forward owns blocks of the activation pool.  An inference call at another shape frees the
    pool, and a graph-replayed sampling run writes into the blocks it was captured with -- in both cases loss.backward()
    must answer SISIC_ESTATE instead of reading freed / overwritten activations; a fresh forward then works again."""
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    images, noise, timesteps = (t.to(DEV) for t in batch)
    model = _new_model(synthetic_sd)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    HipAdam(model.parameters(), lr=1e-4)
    noisy = scheduler.add_noise(images, noise, timesteps)

    def fresh_grads():
        model.train()
        loss = mse_loss(model(noisy, timesteps).sample, noise)
        loss.backward()
        return model.grads()

    ref = fresh_grads()
    # (1) inference at another resolution between forward and backward: the pool is released
    model.train()
    loss = mse_loss(model(noisy, timesteps).sample, noise)
    model.eval()
    model(torch.zeros(1, 3, 32, 32, device=DEV), 5)
    with pytest.raises(_lib.SisicError) as e:
        loss.backward()
    assert e.value.code == _lib.SISIC_ESTATE
    again = fresh_grads()
    assert all(torch.equal(again[k], ref[k]) for k in ref)
    # (2) a graph-replayed sampling run at the SAME shape between forward and backward
    s = Sampler(DEV)
    s.models["NV"] = model.eval()
    model.set_graph_mode(1)
    s.generate_seeds("NV", [1, 2], 6, (64, 64))              # captures the step at B=2, 64x64
    model.train()
    loss = mse_loss(model(noisy, timesteps).sample, noise)
    model.eval()
    s.generate_seeds("NV", [1, 2], 6, (64, 64))              # replays it
    with pytest.raises(_lib.SisicError) as e:
        loss.backward()
    assert e.value.code == _lib.SISIC_ESTATE
    again = fresh_grads()
    assert all(torch.equal(again[k], ref[k]) for k in ref)


# ---- whole steps at the benchmarked configurations, against torch.autograd over the oracle in float64
STEP_CONFIGS = {                 # name: (B, H, W) of a 3-channel batch
    "B32 64x64": (32, 64, 64),         # the training benchmark (tools/train_bench.py --batch 32 --size 64)
    "B2 128x128": (2, 128, 128),       # the reference's configuration: attention backward at C=256, N=1024
    "B20 32x32": (20, 32, 32),         # bias_grad_kernel's batch loop: a partial second trip of its 16 waves
    "B1 136x136": (1, 136, 136),       # 34x34 = 1156 tokens (the largest square size the backward takes), 17x17 levels
}


def _step_batch(name):
    B, H, W = STEP_CONFIGS[name]
    g = torch.Generator().manual_seed(1000 + B * 7 + H)
    images = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    noise = torch.randn(B, 3, H, W, generator=g)
    timesteps = torch.randint(0, 1000, (B,), generator=g)
    timesteps[0], timesteps[-1] = 0, 999
    return images, noise, timesteps


@pytest.fixture(scope="module")
def step_reference64(synthetic_sd):
    """name -> (batch, (loss, grads, pred) of oracle.train.loss_and_grads in float64), each computed once"""
    from oracle import train as otrain
    cache = {}

    def get(name):
        if name not in cache:
            batch = _step_batch(name)
            cache[name] = batch, otrain.loss_and_grads(synthetic_sd, *batch, dtype=torch.float64)
        return cache[name]
    return get


@pytest.mark.parametrize("name,latency", [("B32 64x64", False), ("B2 128x128", False), ("B2 128x128", True),
                                          ("B20 32x32", False), ("B1 136x136", False)])
def test_unet_gradients_at_the_benchmarked_configurations(synthetic_sd, step_reference64, name, latency):
    """The bars of test_unet_gradients_match_autograd_over_the_oracle where the benchmarked step runs: K-split weight
    gradients whose slices walk 3-16 blocks, batch loops past 16, attention backward over 1024 and 1156 tokens."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    batch, (ref_loss, ref_grads, ref_pred) = step_reference64(name)
    images, noise, timesteps = (t.to(DEV) for t in batch)
    model = _new_model(synthetic_sd).set_latency_mode(latency)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    model.train()
    noisy = scheduler.add_noise(images, noise, timesteps)
    noise_pred = model(noisy, timesteps).sample
    pred_err = (noise_pred.cpu().double() - ref_pred).abs().max().item()
    assert pred_err <= PRED_TOL, pred_err
    loss = mse_loss(noise_pred, noise)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss.item(), ref_loss)
    grads = model.grads()
    assert list(grads) == list(ref_grads) and len(grads) == 330
    label = f"{name}{' latency mode' if latency else ''} (float64 oracle)"
    worst, median = _grad_errors(grads, ref_grads, label)
    assert worst[0] <= GRAD_REL_WORST, f"gradient of {worst[1]}: {worst[0]:.3e} of its own largest entry"
    assert median[0] <= GRAD_REL_MEDIAN, median
    mse_loss(model(noisy, timesteps).sample, noise).backward()
    again = model.grads()
    assert all(torch.equal(again[n], grads[n]) for n in grads)


def test_fused_step_matches_the_spelled_out_step_at_batch_32(synthetic_sd):
    """sisic_unet_train_step against scaler.scale(loss).backward(); scaler.step(opt); scaler.update() at the benchmarked
    batch: the same weights, bit for bit, after one step."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, mse_loss, train_step_fused
    images, noise, timesteps = (t.to(DEV) for t in _step_batch("B32 64x64"))
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    spelled = _new_model(synthetic_sd)
    optimizer, scaler = HipAdam(spelled.parameters(), lr=1e-4), HipGradScaler()
    spelled.train()
    loss = mse_loss(spelled(scheduler.add_noise(images, noise, timesteps), timesteps).sample, noise)
    optimizer.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    assert scaler.step(optimizer) is True
    scaler.update()
    fused = _new_model(synthetic_sd)
    value, taken = train_step_fused(fused, scheduler, images, noise, timesteps, HipAdam(fused.parameters(), lr=1e-4),
                                    HipGradScaler())
    assert taken and abs(value - loss.item()) <= 1e-6 * abs(loss.item()), (value, loss.item())
    sd1, sd2 = spelled.state_dict(), fused.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert any(not torch.equal(sd1[k].cpu(), synthetic_sd[k]) for k in sd1)


def test_an_untrainable_resolution_is_refused_before_the_forward(synthetic_sd, batch):
    """144x144 has 36x36 = 1296 tokens at its attention level, more than the attention backward takes: the training
    forward answers SISIC_EINVAL before it records or computes anything, no gradient or weight changes, and the model
    trains at another size afterwards.  Inference at 144x144 stays allowed (test_forward_other_resolutions)."""
    from synt_isic_amd import _lib
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipLoss, mse_loss
    images, noise, timesteps = (t.to(DEV) for t in batch)
    model = _new_model(synthetic_sd)
    HipAdam(model.parameters(), lr=1e-4)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    noisy = scheduler.add_noise(images, noise, timesteps)
    model.train()
    mse_loss(model(noisy, timesteps).sample, noise).backward()          # gradients that must survive the refused call
    grads, params = model.grads(), model._read_all(0)                    # the library's gradient and weight arenas
    big = torch.randn(1, 3, 144, 144, generator=torch.Generator().manual_seed(3)).to(DEV)
    out_of_tape = torch.zeros_like(big)
    with pytest.raises(_lib.SisicError) as e:
        model(big, 10)
    assert e.value.code == _lib.SISIC_EINVAL and "144x144" in str(e.value) and "1170" in str(e.value), str(e.value)
    with pytest.raises(_lib.SisicError) as e:
        HipLoss(model, out_of_tape, torch.zeros_like(big)).backward()     # no tape was recorded
    assert e.value.code == _lib.SISIC_ESTATE
    after = model.grads()
    assert all(torch.equal(after[k], grads[k]) for k in grads)
    assert all(torch.equal(v, params[k]) for k, v in model._read_all(0).items())
    mse_loss(model(noisy, timesteps).sample, noise).backward()
    again = model.grads()
    assert all(torch.equal(again[k], grads[k]) for k in grads)
    model.eval()
    assert model(big, 10).sample.shape == big.shape


# (B, c0, c1, cout, H, W, k, stride, ups, gn, silu) run in a child process with a switch of launch_conv_wgrad set; with
# SISIC_WGRAD_WINOGRAD=0 the 3x3 stride-1 cases take the direct kernels in both tile geometries, slices of >= 2 blocks
WGRAD_SWITCH_CASES = [
    (32, 64, 0, 64, 64, 64, 3, 1, False, True, True),
    (32, 256, 0, 256, 8, 8, 3, 1, False, True, True),
    (29, 40, 0, 33, 65, 4, 3, 1, False, False, False),      # ragged, across images
    (27, 20, 12, 70, 33, 4, 3, 1, False, True, True),       # concat seam inside a tile
    (5, 24, 0, 64, 21, 17, 3, 1, True, False, False),       # nearest 2x
]

_WGRAD_CHILD = '''
import sys
import torch
sys.path.insert(0, {root!r})
from synt_isic_amd import ops
cases = torch.load(sys.argv[1])
out = []
for x, x2, g, dy, k, stride, ups, silu in cases:
    d = lambda t: None if t is None else t.to("cuda").contiguous()
    out.append(ops.conv2d_wgrad(d(x), d(dy), k, x2=d(x2), stride=stride, upsample=ups, gn_scale=d(g[0]) if g else None,
                                gn_shift=d(g[1]) if g else None, gn_silu=silu).cpu())
torch.save(out, sys.argv[2])
'''


def test_conv_wgrad_switch_gated_variants_in_a_child_process(tmp_path):
    """SISIC_WGRAD_WINOGRAD=0 (the direct 3x3 stride-1 kernels conv_wgrad_kernel<3,1,4,16> / <3,1,8,8>) and
    SISIC_WGRAD_FUSED_REDUCE=1 (wgrad_wino_reduce_finish_kernel) are read once per process: each runs in a fresh
    interpreter.  The direct kernels against float64, the fused reduction bit-equal to the default two-kernel one."""
    import subprocess
    import sys
    forms = {_wgrad_geometry(*c[:9], winograd=False)[0] for c in WGRAD_SWITCH_CASES}
    assert forms == {"direct4x16", "direct8x8"}
    for c in WGRAD_SWITCH_CASES:
        assert "loop" in _wgrad_coverage(*c[:9], winograd=False)[1] and _wgrad_geometry(*c[:9])[0] == "wino", c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "wgrad_child.py"
    script.write_text(_WGRAD_CHILD.format(root=root))
    inputs, refs = [], []
    for c in WGRAD_SWITCH_CASES:
        x, x2, g, dy, ref = _wgrad_inputs(*c)
        inputs.append((x, x2, g, dy, c[6], c[7], c[8], c[10]))
        refs.append(ref)
    torch.save(inputs, tmp_path / "inputs.pt")
    default = [_wgrad_run(x, x2, g, dy, k, stride, ups, silu).cpu() for x, x2, g, dy, k, stride, ups, silu in inputs]

    def child(var, value):
        env = dict(os.environ)
        env[var] = value
        out = tmp_path / f"{var}.pt"
        r = subprocess.run([sys.executable, str(script), str(tmp_path / "inputs.pt"), str(out)], env=env, timeout=600,
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{var}={value}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        return torch.load(out)

    direct = child("SISIC_WGRAD_WINOGRAD", "0")
    for c, got, ref in zip(WGRAD_SWITCH_CASES, direct, refs):
        form = _wgrad_geometry(*c[:9], winograd=False)[0]
        _close(got, ref, what=f"conv wgrad SISIC_WGRAD_WINOGRAD=0 B{c[0]} {c[1]}+{c[2]}->{c[3]} {c[4]}x{c[5]} ({form})")
    fused = child("SISIC_WGRAD_FUSED_REDUCE", "1")
    assert all(torch.equal(a, b) for a, b in zip(fused, default))
