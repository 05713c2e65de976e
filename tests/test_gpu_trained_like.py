"""The HIP kernels and the whole UNet under trained-like weights and operands (tests/trained_like.py).

Every other whole-model test loads synthetic_unet_state_dict, under which attention averages uniformly over its tokens
(max_j P_ij ~ 2/N, |score| < 4), every GroupNorm scale is positive and near 1 and no SiLU saturates; the kernel-level tests
stay below |score| ~ 20.  Here the softmax rows are peaked on one key at scores of +-100 - 150 (with exact ties and a
dominant key in the last, partly filled key block), GroupNorm scales are zero, negative and log-normally spread, channels
sit 30 std from their group's mean, one group is exactly constant and SiLU saturates both ways.

Bars.  No fixed bound carries over: at |score| = 150 an fp32 score is good to ~1e-5 absolute, so fp32 itself is further from
float64 than at the synthetic weights.  Every bar is therefore relative to what fp32 can do ON THE SAME INPUTS:
  kernel level   e_ref = error of the same formula evaluated in fp32 torch on the CPU against its float64 evaluation; the
                 kernel must be within max(1e-5 * max(1, |ref|), 8 e_ref) -- three bits over the reference's own fp32 error
                 (the kernels add one rounding of the scaled operand and a 1-ulp hardware exp / rcp, which scale with |s| as
                 e_ref does), or the per-kernel bound of test_gpu_train.py where that is the larger;
  whole model    e32 = error of the fp32 CPU oracle against the float64 oracle on that batch (worst and median tensor of the
                 relative gradient error; max abs error / max |pred| for predictions); the HIP path must be within 10 e32 --
                 the headroom the fixed bars of test_gpu_train.py grant at synthetic weights (1e-4 over a measured 1.0e-5).
Measured on MI355X (profiles/r24/trained_like_kernels.txt, trained_like_model.txt, written through SISIC_TEST_ERRLOG): err / e_ref
0.01 - 2.9 at kernel level, err / e32 0 - 1.24 for the whole model.  attention_bwd_kernel as it stood before this file was at
10.9 e_ref for dQ at 1170 tokens and failed; profiles/r24/attention_bwd_before_after.txt and DESIGN.md section 6 have the cause.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import trained_like as tl
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5                  # test_gpu_train.py's per-kernel bound: 1e-5 * max(1, |ref|)
KERNEL_FACTOR = 8.0
MODEL_FACTOR = 10.0


def _log(line):
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(line + "\n")
    print(line)


def _kernel_bar(got, ref64, ref32, what, failures=None):
    """err = max |got - ref64| against max(KTOL * max(1, |ref64|), 8 * max |ref32 - ref64|); logged relative to the tensor's
    largest reference entry (the measure of test_gpu_train._grad_errors).  With ``failures`` (a list) a miss is appended to it
    instead of raised, so that a case logs all of its tensors before it fails."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    top = ref64.abs().max().item()
    err = (got - ref64).abs().max().item()
    e_ref = (ref32.detach().double() - ref64).abs().max().item()
    floor = KTOL * max(1.0, top)
    bound = max(floor, KERNEL_FACTOR * e_ref)
    _log(f"{err / top:.3e}\t{e_ref / top:.3e}\t{err / e_ref if e_ref else float('inf'):.2f}\t{err / bound:.3f}\t{what}"
         f"  (err, e_ref of max |ref| = {top:.3e}; err / e_ref; err / bound, floor {floor / top:.1e})")
    ok, msg = math.isfinite(err) and err <= bound, f"{what}: max abs err {err:.3e} > {bound:.3e} (fp32 reference: {e_ref:.3e})"
    if failures is not None and not ok:
        failures.append(msg)
        return
    assert ok, msg


# ================================================================ ops.attention, peaky
def _two_block_form(B, C, N):
    """launch_attention's choice: attention_kernel<2> where that still leaves each of the 256 CUs four workgroups"""
    return B * (C // 8) * ((N + 255) // 256) >= 4 * 256


def _check_rows(qkv, N):
    """the operand has what the case is there for: |score| of 100 - 150, peaked rows next to ordinary ones, exact ties, rows
    whose dominant key is the last one"""
    s, p = tl.attention_rows(qkv)
    assert 90.0 <= s.abs().max().item() <= 150.0, s.abs().max().item()
    share = (p.amax(-1) > 0.5).double().mean().item()
    assert 0.2 <= share <= 0.9, share
    top2 = s.topk(2, dim=-1).values
    assert (top2[..., 3, 0] == top2[..., 3, 1]).all() and (top2[..., N // 2, 0] == top2[..., N // 2, 1]).all()
    assert (s.argmax(-1)[..., 1] == N - 1).all() and (s.argmax(-1)[..., N - 2] == N - 1).all()


@pytest.mark.parametrize("B,C,N,two", [(2, 64, 33, False),       # a single key block with a tail
                                       (2, 64, 256, False),      # exactly one block
                                       (2, 64, 300, False),      # two blocks, the second ragged
                                       (1, 64, 513, False),      # a third block of one key: the dominant one
                                       (32, 256, 64, True),      # attention_kernel<2>
                                       (32, 256, 300, True)])
def test_attention_peaky(B, C, N, two):
    from synt_isic_amd import ops
    assert _two_block_form(B, C, N) == two, "the case must select the form it is there for (launch_attention)"
    qkv = tl.peaky_qkv(B, C, N, seed=4000 + N + B)
    idx = [0, B // 2, B - 1] if two else list(range(B))
    _check_rows(qkv[idx], N)
    got = ops.attention(qkv.to(DEV), 8)
    with torch.no_grad():
        ref64, ref32 = tl.attention_ref(qkv[idx].double()), tl.attention_ref(qkv[idx])
    assert torch.isfinite(got).all()
    _kernel_bar(got[idx], ref64, ref32, f"attention peaky B={B} C={C} N={N}{' two query blocks per wave' if two else ''}")
    if two:         # the form follows the batch, the bits must not
        for i in (0, B - 2):
            small = ops.attention(qkv[i:i + 2].to(DEV).contiguous(), 8)
            assert torch.equal(small, got[i:i + 2]), f"images {i}, {i + 1}: the two forms differ"


# ================================================================ ops.attention_bwd, peaky
@pytest.mark.parametrize("N", [64, 100, 1024, 1170])
def test_attention_bwd_peaky(N):
    """dQ, dK, dV each against its own largest reference entry; rows 1 and N - 2 are fully saturated (reference dQ ~ 0)."""
    from synt_isic_amd import ops
    B, C = 2, 16
    qkv = tl.peaky_qkv(B, C, N, seed=5000 + N)
    _check_rows(qkv, N)
    dO = torch.randn(B, C, N, generator=torch.Generator().manual_seed(5100 + N))
    grads = []
    for dtype in (torch.float64, torch.float32):
        x = qkv.to(dtype).requires_grad_(True)
        tl.attention_ref(x).backward(dO.to(dtype))
        grads.append(x.grad)
    g64, g32 = grads
    dq64 = g64[:, :C].reshape(B, C // 8, 8, N)
    assert dq64[..., 1].abs().max().item() <= 1e-6 * dq64.abs().max().item()        # a saturated row
    out = ops.attention(qkv.to(DEV))
    got = ops.attention_bwd(qkv.to(DEV), out, dO.to(DEV))
    assert torch.isfinite(got).all()
    failures = []
    for name, part in zip(("dQ", "dK", "dV"), range(3)):
        sl = slice(part * C, (part + 1) * C)
        _kernel_bar(got[:, sl], g64[:, sl], g32[:, sl], f"attention bwd peaky N={N} {name}", failures)
    assert not failures, failures
    assert torch.equal(got, ops.attention_bwd(qkv.to(DEV), out, dO.to(DEV)))


# ================================================================ ops.groupnorm_bwd
def _gn_operands(B, C, H, W):
    gamma, beta = tl.wild_affine(C, seed=6000 + C)
    x = tl.offset_x(B, C, H, W, seed=6100 + C + H)
    da = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(6200 + C + H))
    return x, gamma, beta, da


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("B,C,H,W", [(2, 64, 5, 7),        # 2 channels per group, HW % 4 != 0: the scalar paths
                                     (2, 512, 8, 8),       # 16 channels per group
                                     (2, 128, 9, 9)])
def test_groupnorm_bwd_wild(B, C, H, W, silu):
    """gamma with zeros, negatives and a log-normal spread, channels ~30 std apart inside a group, one group exactly
    constant (rstd = 1 / sqrt(eps)), pre-activations past +-40 (SiLU saturated both ways)."""
    from synt_isic_amd import ops
    x, gamma, beta, da = _gn_operands(B, C, H, W)
    res = []
    for dtype in (torch.float64, torch.float32):
        xs, gs, bs = (t.to(dtype).requires_grad_(True) for t in (x, gamma, beta))
        u = F.group_norm(xs, 32, gs, bs, eps=1e-5)
        if dtype == torch.float64:
            assert u.max().item() > 40 and u.min().item() < -40
            cpg = C // 32
            const = torch.zeros(B, C, dtype=torch.bool)
            const[0, 3 * cpg:4 * cpg] = True                                      # the constant group: xhat = 0, u = beta
            assert (u[0, 3 * cpg:4 * cpg] - bs[3 * cpg:4 * cpg, None, None]).abs().max().item() < 1e-9
        (F.silu(u) if silu else u).backward(da.to(dtype))
        res.append((xs.grad, gs.grad, bs.grad))
    assert (gamma == 0).any() and (gamma < 0).any()
    dx, dg, db = ops.groupnorm_bwd(da.to(DEV), x.to(DEV), gamma.to(DEV), beta.to(DEV), 32, 1e-5, silu)
    what = f"groupnorm bwd wild {B}x{C}x{H}x{W} silu{int(silu)}"
    # dx of the constant group is 1 / sqrt(eps) = 316 x larger than the rest: each part against its own largest entry
    _kernel_bar(dx[const], res[0][0][const], res[1][0][const], f"{what} dx, the constant group")
    _kernel_bar(dx[~const], res[0][0][~const], res[1][0][~const], f"{what} dx, the other groups")
    _kernel_bar(dg, res[0][1], res[1][1], f"{what} dgamma")
    _kernel_bar(db, res[0][2], res[1][2], f"{what} dbeta")


# ================================================================ ops.conv2d_wgrad behind the GroupNorm (+ SiLU) prologue
@pytest.mark.parametrize("B,c0,c1,cout,H,W,k,silu", [(2, 20, 12, 70, 18, 10, 3, True),      # Winograd, concat seam in a tile
                                                     (2, 256, 0, 768, 8, 8, 1, False)])     # the fused q/k/v projection
def test_conv_wgrad_wild_prologue(B, c0, c1, cout, H, W, k, silu):
    """The weight gradient reads a = act(x * scale + shift) with the scale / shift of the same gamma, beta and offsets: the
    two terms cancel from ~30 * scale down to O(1), and SiLU sees +-40."""
    from synt_isic_amd import ops
    C = c0 + c1
    x, gamma, beta, _ = _gn_operands(B, C, H, W)
    scale, shift = tl.gn_scale_shift(x, gamma, beta)
    dy = torch.randn(B, cout, H, W, generator=torch.Generator().manual_seed(6300 + C))
    refs = []
    for dtype in (torch.float64, torch.float32):
        a = x.to(dtype) * scale.to(dtype)[:, :, None, None] + shift.to(dtype)[:, :, None, None]
        if dtype == torch.float64:
            assert a.max().item() > 40 and a.min().item() < -40
        if silu:
            a = F.silu(a)
        w = torch.zeros(cout, C, k, k, dtype=dtype, requires_grad=True)
        F.conv2d(a, w, padding=k // 2).backward(dy.to(dtype))
        refs.append(w.grad)
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    run = lambda: ops.conv2d_wgrad(d(x[:, :c0]), d(dy), k, x2=d(x[:, c0:]) if c1 else None, gn_scale=d(scale), gn_shift=d(shift),
                                   gn_silu=silu)
    got = run()
    _kernel_bar(got, refs[0], refs[1], f"conv wgrad wild prologue {c0}+{c1}->{cout} k{k} {H}x{W} silu{int(silu)}")
    assert torch.equal(got, run())


# ================================================================ the whole model
@pytest.fixture(scope="module")
def trained_sd(synthetic_sd):
    return tl.trained_like_unet_state_dict(synthetic_sd)


STEP_BATCHES = {"B2 64x64": (2, 64, 64, 77, [37, 912]),        # test_gpu_train.py's batch
                "B3 40x56": (3, 40, 56, 78, [0, 500, 999])}    # ragged levels: 20x28 / 10x14 / 5x7, 280 and 35 tokens


@pytest.fixture(scope="module")
def step_reference(trained_sd):
    """name -> (batch, float64 (loss, grads, pred), e32 = the fp32 oracle's (worst, median, pred) error against it)"""
    from oracle import train as otrain
    cache = {}

    def get(name):
        if name not in cache:
            B, H, W, seed, ts = STEP_BATCHES[name]
            g = torch.Generator().manual_seed(seed)
            batch = torch.rand(B, 3, H, W, generator=g) * 2 - 1, torch.randn(B, 3, H, W, generator=g), torch.tensor(ts)
            ref = otrain.loss_and_grads(trained_sd, *batch, dtype=torch.float64)
            _, g32, p32 = otrain.loss_and_grads(trained_sd, *batch)
            worst, median, _ = tl.grad_errors(g32, ref[1])
            e_pred = (p32.double() - ref[2]).abs().max().item() / ref[2].abs().max().item()
            cache[name] = batch, ref, (worst[0], median[0], e_pred)
        return cache[name]
    return get


def _new_model(sd):
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel()
    m.load_state_dict(sd)
    return m.to(DEV)


def _pred_bar(pred, ref_pred, e_pred, what):
    top = ref_pred.abs().max().item()
    err = (pred.detach().cpu().double() - ref_pred).abs().max().item() / top
    _log(f"{err:.3e}\t{e_pred:.3e}\t{err / e_pred:.2f}\tprediction {what}: max abs err / max |pred| (= {top:.3f}); fp32 oracle; ratio")
    assert math.isfinite(err) and err <= MODEL_FACTOR * e_pred, f"{what}: prediction {err:.3e} > 10 x {e_pred:.3e}"


@pytest.mark.parametrize("name,latency", [("B2 64x64", False), ("B2 64x64", True), ("B3 40x56", False)])
def test_unet_gradients_under_trained_like_weights(trained_sd, step_reference, name, latency):
    """Loss, training-mode prediction and all 330 gradients against the float64 oracle, within 10 x the fp32 oracle's own
    error on the batch; model.eval() equal to the tape-recording forward and a second backward equal to the first, bit for
    bit.  to_k.bias keeps an identically zero gradient: below 1e-7, as in test_gpu_train._grad_errors."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    batch, (ref_loss, ref_grads, ref_pred), (e_worst, e_median, e_pred) = step_reference(name)
    images, noise, timesteps = (t.to(DEV) for t in batch)
    label = f"{name}{' latency mode' if latency else ''}"
    model = _new_model(trained_sd).set_latency_mode(latency)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    model.train()
    noisy = scheduler.add_noise(images, noise, timesteps)
    noise_pred = model(noisy, timesteps).sample
    _pred_bar(noise_pred, ref_pred, e_pred, label)
    model.eval()
    assert torch.equal(model(noisy, timesteps).sample, noise_pred)        # the tape-recording forward IS the forward
    model.train()
    noise_pred = model(noisy, timesteps).sample
    loss = mse_loss(noise_pred, noise)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    # d loss <= 2 * mean |pred - noise| * max |d pred| <= 2 sqrt(loss) * (the prediction's bar), plus the fp32 mean itself
    loss_bound = 2.0 * math.sqrt(ref_loss) * MODEL_FACTOR * e_pred * ref_pred.abs().max().item() + 1e-6 * ref_loss
    _log(f"{abs(loss.item() - ref_loss):.3e}\t{loss_bound:.3e}\t-\tloss {label}: abs err; bound (ref {ref_loss:.6f})")
    assert abs(loss.item() - ref_loss) <= loss_bound, (loss.item(), ref_loss)
    grads = model.grads()
    assert list(grads) == list(ref_grads) and len(grads) == 330
    worst, median, vanishing = tl.grad_errors(grads, ref_grads)
    _log(f"{worst[0]:.3e}\t{e_worst:.3e}\t{worst[0] / e_worst:.2f}\tgradients {label}: worst tensor ({worst[1]}); fp32 oracle's worst; ratio")
    _log(f"{median[0]:.3e}\t{e_median:.3e}\t{median[0] / e_median:.2f}\tgradients {label}: median tensor; fp32 oracle's median; ratio")
    assert vanishing <= 1e-7, f"{label}: a gradient that should vanish: {vanishing:.3e}"
    assert worst[0] <= MODEL_FACTOR * e_worst, f"gradient of {worst[1]}: {worst[0]:.3e} > 10 x {e_worst:.3e}"
    assert median[0] <= MODEL_FACTOR * e_median, (median, e_median)
    mse_loss(model(noisy, timesteps).sample, noise).backward()
    again = model.grads()
    assert all(torch.equal(again[n], grads[n]) for n in grads)


def test_unet_forward_at_the_benchmarked_batch(trained_sd):
    """B=64, 3x64x64: the batch-64 plans and attention_kernel<2>.  GroupNorm and attention are per sample, so the float64
    oracle of images {0, 31, 63} alone is their exact reference."""
    from oracle import unet as ounet
    from oracle import train as otrain
    B, idx = 64, [0, 31, 63]
    g = torch.Generator().manual_seed(640)
    x = torch.randn(B, 3, 64, 64, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0], t[-1] = 0, 999
    assert _two_block_form(B, 256, 64) and _two_block_form(B, 256, 256)
    sd64 = {k: v.double() for k, v in trained_sd.items()}
    with torch.no_grad():
        ref = otrain.unet_forward64(sd64, x[idx].double(), t[idx])
        p32 = ounet.unet_forward(trained_sd, x[idx], t[idx])
    e_pred = (p32.double() - ref).abs().max().item() / ref.abs().max().item()
    model = _new_model(trained_sd).eval()
    out = model(x.to(DEV), t.to(DEV)).sample
    assert torch.isfinite(out).all()
    _pred_bar(out[idx], ref, e_pred, "B64 64x64 eval, images 0 / 31 / 63")
    pair = model(x[62:64].to(DEV).contiguous(), t[62:64].to(DEV)).sample
    assert torch.equal(pair, out[62:64])                                  # an image's bits do not depend on its batch


def test_ddim_chain_under_trained_like_weights(trained_sd, step_reference):
    """DDIM, T=10, B=2, 64x64, eager and graph-replayed: equal to each other bit for bit, finite, and within the forward bar
    (10 x the fp32 oracle's prediction error at B=2, 64x64, of the largest latent) of the Python loop over the model and the
    scheduler mirror."""
    from synt_isic_amd.sampler import Sampler, run_sampling_loop
    from synt_isic_amd.scheduler import HipDDIMScheduler
    e_pred = step_reference("B2 64x64")[2][2]
    x_T = torch.stack([torch.randn(3, 64, 64, generator=torch.Generator().manual_seed(2000 + s)) for s in (1, 2)]).to(DEV)
    finals = []
    for mode in (0, 1):
        s = Sampler(DEV)
        model = s.add_model("NV", trained_sd)
        model.set_graph_mode(mode)
        sched = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        sched.set_timesteps(10)
        res = run_sampling_loop(model, sched, x_T, None, eta=0.0)
        if mode == 1:
            res = run_sampling_loop(model, sched, x_T, None, eta=0.0)     # the second run replays the captured step
        assert res.steps_done == 10 and torch.isfinite(res.latents).all()
        finals.append(res.latents)
        if mode == 0:
            x = x_T.clone()
            for t in sched.timesteps:
                x = sched.step(model(x, t).sample, t, x, eta=0.0).prev_sample
            top = x.abs().max().item()
            err = (res.latents - x).abs().max().item() / top
            _log(f"{err:.3e}\t{e_pred:.3e}\t{err / e_pred:.2f}\tDDIM T=10 B2 64x64 fused loop vs Python loop: max abs err / max |latent| (= {top:.3f}); fp32 oracle's prediction error; ratio")
            assert err <= MODEL_FACTOR * e_pred, err
    assert torch.equal(finals[0], finals[1])
