"""Attention at 32 and 64 channels per head on the GPU: ops.attention, ops.attention_bwd and the two architectures E and F
(tests/wide_head_ref.py) through the forward, the training step and the sampling loops.

Bars are the project's own (test_gpu_trained_like.py, test_gpu_architectures.py); nothing is chosen here:
  ordinary operands   KTOL = 1e-5 * max(1, |ref|) against float64;
  peaky operands      max(that floor, 8 x the error of the same formula in fp32 torch on the CPU) -- _kernel_bar;
  whole model         10 x the fp32 restatement's own error against the float64 restatement (prediction; worst and median
                      tensor of the relative gradient error); vanishing gradients below max(1e-7, 10 x fp32's own largest entry
                      there); the loss within 1e-5 * max(1, |ref|).
test_wide_head_cpu.py shows that these bars see a d = 8 scale or a d = 8 head cut by more than 100 x.

Token counts follow the kernels' tiling (attention_wide.hip: 32-token tiles, 64-token LDS images, 128 queries / keys per
workgroup): 1, 31, 33 (tails on either side of a tile), 64, 65 (an image and one token), 100, 128, 129 (a workgroup and one
token), 256, 300, 513, 1024, and 1300 / 2048 in the backward pass, both past the 1170 tokens the d = 8 backward pass stops at.
The launchers have ONE form per head dimension -- nothing follows the batch -- so the batch-independence case is a single one.
"""
import math
import os

import pytest
import torch

import arch_ref
import stream_probe as sp
import wide_head_ref as wh
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5                  # test_gpu_train.py's per-kernel bound: 1e-5 * max(1, |ref|)
KERNEL_FACTOR = 8.0          # test_gpu_trained_like.py
MODEL_FACTOR = 10.0          # test_gpu_trained_like.py, test_gpu_architectures.py
BWD_MAX_TOKENS = 65536       # train.h: ATTN_BWD_TILED_MAX_TOKENS
WIDTHS = [32, 64]


def _log(line):
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(line + "\n")
    print(line)


def _close(got, ref64, what):
    got = got.detach().cpu().double()
    top = ref64.abs().max().item()
    bound = KTOL * max(1.0, top)
    err = (got - ref64).abs().max().item()
    _log(f"{err / max(1.0, top):.3e}\t{KTOL:.1e}\t{err / bound:.3f}\t{what}  (err / max(1, |ref|); KTOL; err / bound)")
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert math.isfinite(err) and err <= bound, f"{what}: max abs err {err:.3e} > {bound:.3e}"


def _kernel_bar(got, ref64, ref32, what, failures=None):
    """test_gpu_trained_like._kernel_bar: err = max |got - ref64| against max(KTOL * max(1, |ref64|), 8 * max |ref32 - ref64|)"""
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


# ================================================================ ops.attention
@pytest.mark.parametrize("N", [1, 31, 33, 64, 65, 100, 128, 129, 256, 300, 513, 1024])
@pytest.mark.parametrize("d", WIDTHS)
def test_attention_forward(d, N):
    from synt_isic_amd import ops
    B, C = 2, 128
    qkv = wh.ordinary_qkv(B, C, N, d)
    got = ops.attention(qkv.to(DEV), d)
    assert torch.isfinite(got).all()
    with torch.no_grad():
        _close(got, wh.attention_ref(qkv.double(), d), f"attention d={d} N={N}")


@pytest.mark.parametrize("spike_at", [700, 5])
@pytest.mark.parametrize("d", WIDTHS)
def test_attention_online_rescale_branch(d, spike_at):
    """test_gpu_kernels.py's case of this name: one key of huge norm late (everything accumulated before it is rescaled) and
    early (nothing after it may raise the maximum)"""
    from synt_isic_amd import ops
    B, C, N = 1, 64, 768
    qkv = torch.randn(B, 3 * C, N, generator=torch.Generator().manual_seed(50)) * 0.5
    qkv[:, C:2 * C, spike_at] *= 40.0
    got = ops.attention(qkv.to(DEV), d)
    assert torch.isfinite(got).all()
    with torch.no_grad():
        _close(got, wh.attention_ref(qkv.double(), d), f"attention d={d} spike at key {spike_at}")


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("d", WIDTHS)
def test_attention_peaky(d, case):
    from synt_isic_amd import ops
    B, C, N = wh.peaky_shapes(d)[case]
    qkv = wh.peaky_qkv(B, C, N, d, wh.peaky_seed(d, B, N))
    wh.check_rows(qkv, N, d)
    got = ops.attention(qkv.to(DEV), d)
    with torch.no_grad():
        ref64, ref32 = wh.attention_ref(qkv.double(), d), wh.attention_ref(qkv, d)
    assert torch.isfinite(got).all()
    _kernel_bar(got, ref64, ref32, f"attention peaky d={d} B={B} C={C} N={N}")


@pytest.mark.parametrize("d", WIDTHS)
def test_attention_bits_do_not_depend_on_the_batch(d):
    from synt_isic_amd import ops
    B, C, N = 32, 128, 100
    qkv = wh.ordinary_qkv(B, C, N, d).to(DEV)
    got = ops.attention(qkv, d)
    for i in (0, B - 2):
        assert torch.equal(ops.attention(qkv[i:i + 2].contiguous(), d), got[i:i + 2]), f"images {i}, {i + 1}"
    assert torch.equal(ops.attention(qkv, d), got)


# ================================================================ ops.attention_bwd
@pytest.mark.parametrize("B,C,N", [(2, 128, 64), (1, 128, 256), (1, 64, 100), (2, 64, 1024), (1, 64, 1300), (1, 64, 2048)])
@pytest.mark.parametrize("d", WIDTHS)
def test_attention_bwd(d, B, C, N):
    from synt_isic_amd import ops
    qkv = wh.ordinary_qkv(B, C, N, d)
    dO = torch.randn(B, C, N, generator=torch.Generator().manual_seed(5100 + N + d))
    x = qkv.double().requires_grad_(True)
    wh.attention_ref(x, d).backward(dO.double())
    out = ops.attention(qkv.to(DEV), d)
    got = ops.attention_bwd(qkv.to(DEV), out, dO.to(DEV), d)
    assert torch.isfinite(got).all()
    for name, part in zip(("dQ", "dK", "dV"), range(3)):
        sl = slice(part * C, (part + 1) * C)
        _close(got[:, sl], x.grad[:, sl], f"attention bwd d={d} B={B} C={C} N={N} {name}")


@pytest.mark.parametrize("N", [64, 100, 1300, 2048])
@pytest.mark.parametrize("d", WIDTHS)
def test_attention_bwd_peaky(d, N):
    """dQ, dK, dV each against its own largest reference entry; rows 1 and N - 2 are fully saturated (reference dQ ~ 0: the bar
    covers them); two calls give equal bits"""
    from synt_isic_amd import ops
    B, C = (2 if N <= 100 else 1), 2 * d
    qkv = wh.peaky_qkv(B, C, N, d, seed=5000 + N + d)
    wh.check_rows(qkv, N, d)
    dO = torch.randn(B, C, N, generator=torch.Generator().manual_seed(5100 + N + d))
    g64, g32 = wh.backward_refs(qkv, dO, d)
    dq64 = g64[:, :C].reshape(B, C // d, d, N)
    assert dq64[..., 1].abs().max().item() <= 1e-6 * dq64.abs().max().item()        # a saturated row
    out = ops.attention(qkv.to(DEV), d)
    got = ops.attention_bwd(qkv.to(DEV), out, dO.to(DEV), d)
    assert torch.isfinite(got).all()
    failures = []
    for name, part in zip(("dQ", "dK", "dV"), range(3)):
        sl = slice(part * C, (part + 1) * C)
        _kernel_bar(got[:, sl], g64[:, sl], g32[:, sl], f"attention bwd peaky d={d} N={N} {name}", failures)
    assert not failures, failures
    assert torch.equal(got, ops.attention_bwd(qkv.to(DEV), out, dO.to(DEV), d))


# ================================================================ refusals
def _refused(call, *words):
    from synt_isic_amd import _lib
    with pytest.raises(_lib.SisicError) as e:
        call()
    assert e.value.code == _lib.SISIC_EINVAL, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("d", [24, 128])
def test_other_head_dims_are_refused(d):
    from synt_isic_amd import ops
    C = 3 * 128                  # a multiple of 24 and of 128
    qkv, out = torch.zeros(1, 3 * C, 16, device=DEV), torch.zeros(1, C, 16, device=DEV)
    _refused(lambda: ops.attention(qkv, d), "head_dim", str(d))
    _refused(lambda: ops.attention_bwd(qkv, out, out, d), "head_dim", str(d))


@pytest.mark.parametrize("d", WIDTHS)
def test_channels_that_are_no_multiple_of_the_head_dim_are_refused(d):
    from synt_isic_amd import ops
    C = d + 16
    qkv, out = torch.zeros(1, 3 * C, 16, device=DEV), torch.zeros(1, C, 16, device=DEV)
    _refused(lambda: ops.attention(qkv, d), "head_dim", f"C={C}")
    _refused(lambda: ops.attention_bwd(qkv, out, out, d), "head_dim", f"C={C}")


def test_attention_bwd_refuses_more_tokens_than_its_stated_bound():
    """one token more than ATTN_BWD_TILED_MAX_TOKENS at d = 32: refused by the host-side check, before any launch"""
    from synt_isic_amd import ops
    N = BWD_MAX_TOKENS + 1
    qkv, out = torch.zeros(1, 3 * 32, N, device=DEV), torch.zeros(1, 32, N, device=DEV)
    _refused(lambda: ops.attention_bwd(qkv, out, out, 32), str(N), str(BWD_MAX_TOKENS))


# ================================================================ a held side stream
@pytest.mark.parametrize("which", ["attention", "attention_bwd"])
def test_held_side_stream(which):
    """test_gpu_streams.py's probe at d = 32: the result on a held side stream equals the default-stream result bit for bit, and
    the call returns while the stream is still held (the warm call has sized the stream's row-statistics scratch)"""
    from synt_isic_amd import ops
    r = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    if which == "attention":
        fn = lambda qkv: ops.attention(qkv, 32)
        gen = lambda s: [r(2, 3 * 64, 100, seed=80 + s) * 1.5]
    else:
        fn = lambda qkv, o, do: ops.attention_bwd(qkv, o, do, 32)
        gen = lambda s: [r(2, 3 * 64, 100, seed=114 + s), r(2, 64, 100, seed=116 + s), r(2, 64, 100, seed=118 + s)]
    dev = lambda args: [a.to(DEV).contiguous() for a in args]
    baseline, held_out, held = sp.run_held(fn, lambda: dev(gen(0)), lambda: dev(gen(1)), label=f"{which} d=32")
    if which == "attention":
        with torch.no_grad():
            _close(baseline, wh.attention_ref(gen(0)[0].double(), 32), "attention d=32 on the default stream")
    assert sp.same(baseline, held_out), f"{which}: the result on a held side stream differs from the default-stream result"
    assert held, f"{which}: the call waited for its stream"


# ================================================================ the models E and F
NAMES = list(wh.ARCHS_WIDE)
FIRST = {name: wh.SHAPES_WIDE[name][0] for name in NAMES}
ALL_SHAPES = [(name, shape) for name in NAMES for shape in wh.SHAPES_WIDE[name]]
TRAIN_SHAPES = [("E", (2, 16, 16)), ("F", (2, 32, 32)), ("F", (1, 80, 72))]       # F at 1x80x72: 1440 tokens at level 1


def _sid(shape):
    return "x".join(str(v) for v in shape)


@pytest.fixture(scope="module")
def weights():
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return {name: synthetic_unet_state_dict(cfg=cfg) for name, cfg in wh.ARCHS_WIDE.items()}


def _build(name, sd, **over):
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel(**dict(wh.unet_kwargs(wh.ARCHS_WIDE[name]), **over))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def models(weights):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _build(name, weights[name])
        m = cache[name]
        m.set_latency_mode(False)
        return m.eval()
    return get


@pytest.fixture(scope="module")
def reference(weights):
    """(name, shape) -> the batch, the float64 restatement and the fp32 restatement's own errors; the shapes of TRAIN_SHAPES
    carry loss and gradients as well.  Computed once, never changed."""
    cache = {}

    def get(name, shape):
        key = (name, tuple(shape))
        if key in cache:
            return cache[key]
        cfg, sd = wh.ARCHS_WIDE[name], weights[name]
        x, target, t = wh.batch(name, shape)
        r = {"x": x, "target": target, "t": t}
        if key in TRAIN_SHAPES:
            r["loss"], r["grads"], r["pred"] = arch_ref.loss_and_grads(cfg, sd, x, target, t, dtype=torch.float64)
            _, g32, p32 = arch_ref.loss_and_grads(cfg, sd, x, target, t, dtype=torch.float32)
            r["vanishing"] = wh.vanishing_set(name)
            worst, median, own = arch_ref.grad_errors(g32, r["grads"], r["vanishing"])
            r["e32_worst"], r["e32_median"], r["own_vanishing"] = worst[0], median[0], own
        else:
            with torch.no_grad():
                r["pred"] = arch_ref.unet_forward(cfg, {k: v.double() for k, v in sd.items()}, x.double(), t)
                p32 = arch_ref.unet_forward(cfg, sd, x, t)
        r["e32_pred"] = (p32.double() - r["pred"]).abs().max().item()
        assert 0.0 < r["e32_pred"] < 1e-4, r["e32_pred"]
        cache[key] = r
        return r
    return get


def _pred_bar(pred, ref, what):
    top = ref["pred"].abs().max().item()
    err = (pred.detach().cpu().double() - ref["pred"]).abs().max().item()
    e32 = ref["e32_pred"]
    _log(f"{err / top:.3e}\t{e32 / top:.3e}\t{err / (MODEL_FACTOR * e32):.3f}\tprediction {what}: max abs err / max |pred| (= {top:.3f}); "
         f"fp32 restatement's; err / bar")
    assert tuple(pred.shape) == tuple(ref["pred"].shape)
    assert math.isfinite(err) and err <= MODEL_FACTOR * e32, f"{what}: prediction off by {err:.3e} > 10 x {e32:.3e}"


@pytest.mark.parametrize("latency", [False, True], ids=["default", "latency"])
@pytest.mark.parametrize("name,shape", ALL_SHAPES, ids=[f"{n}-{_sid(s)}" for n, s in ALL_SHAPES])
def test_forward_matches_the_restatement(name, shape, latency, models, reference):
    """every shape of the table in both modes against float64; row k of the batch equal to its own batch-1 forward and a second
    call equal to the first, bit for bit"""
    ref = reference(name, shape)
    model = models(name).set_latency_mode(latency)
    try:
        x, t = ref["x"].to(DEV), ref["t"].to(DEV)
        y = model(x, t).sample
        _pred_bar(y, ref, f"{name} {_sid(shape)}{' latency mode' if latency else ''}")
        for k in range(shape[0]):
            one = model(x[k:k + 1].contiguous(), t[k:k + 1]).sample
            assert torch.equal(one, y[k:k + 1]), f"image {k}: its bits depend on the batch it is in"
        assert torch.equal(model(x, t).sample, y)
    finally:
        model.set_latency_mode(False)


# (the first shape of a row in both modes; F at 1x80x72 once, in the default mode)
TRAIN_CASES = [(n, s, lat) for n, s in TRAIN_SHAPES for lat in (False, True) if not lat or s == FIRST[n]]


@pytest.mark.parametrize("name,shape,latency", TRAIN_CASES,
                         ids=[f"{n}-{_sid(s)}-{'latency' if lat else 'default'}" for n, s, lat in TRAIN_CASES])
def test_gradients_match_autograd_over_the_restatement(name, shape, latency, models, reference):
    """test_gpu_architectures.py's test of this name on E and F: loss, training-mode prediction and every gradient against
    float64; the tape-recording forward equal to the eval forward; a second forward / backward equal to the first, bit for bit"""
    from synt_isic_amd.train import HipAdam, mse_loss
    ref = reference(name, shape)
    label = f"{name} {_sid(shape)}{' latency mode' if latency else ''}"
    model = models(name).set_latency_mode(latency)
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    x, target, t = ref["x"].to(DEV), ref["target"].to(DEV), ref["t"].to(DEV)
    try:
        model.train()
        pred = model(x, t).sample
        _pred_bar(pred, ref, f"{label} training mode")
        model.eval()
        assert torch.equal(model(x, t).sample, pred)
        model.train()
        pred = model(x, t).sample
        loss = mse_loss(pred, target)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        _log(f"{abs(loss.item() - ref['loss']):.3e}\t{1e-5 * max(1.0, abs(ref['loss'])):.3e}\t-\tloss {label}: abs err; bound (ref {ref['loss']:.6f})")
        assert abs(loss.item() - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"])), (loss.item(), ref["loss"])
        grads = model.grads()
        assert list(grads) == list(ref["grads"])
        assert all(torch.isfinite(g).all() for g in grads.values())
        worst, median, vanishing = arch_ref.grad_errors(grads, ref["grads"], ref["vanishing"])
        ew, em = ref["e32_worst"], ref["e32_median"]
        _log(f"{worst[0]:.3e}\t{ew:.3e}\t{worst[0] / (MODEL_FACTOR * ew):.3f}\tgradients {label}: worst tensor ({worst[1]}); fp32 restatement's worst; err / bar")
        _log(f"{median[0]:.3e}\t{em:.3e}\t{median[0] / (MODEL_FACTOR * em):.3f}\tgradients {label}: median tensor of {len(grads) - len(vanishing)}; fp32 restatement's median; err / bar")
        assert sorted(vanishing) == sorted(ref["vanishing"])
        over = {n: (v, max(1e-7, MODEL_FACTOR * ref["own_vanishing"][n])) for n, v in vanishing.items()
                if not v <= max(1e-7, MODEL_FACTOR * ref["own_vanishing"][n])}
        _log(f"{max(vanishing.values()):.3e}\t{max(ref['own_vanishing'].values()):.3e}\t-\tgradients {label}: largest entry of the {len(vanishing)} vanishing tensors; fp32 restatement's")
        assert not over, f"{label}: gradients that should vanish (value, bound): {over}"
        assert worst[0] <= MODEL_FACTOR * ew, f"gradient of {worst[1]}: {worst[0]:.3e} > 10 x {ew:.3e}"
        assert median[0] <= MODEL_FACTOR * em, (median, em)
        mse_loss(model(x, t).sample, target).backward()
        again = model.grads()
        assert all(torch.equal(again[n], grads[n]) for n in grads)
    finally:
        model.eval()
        model.set_latency_mode(False)


def test_a_d8_model_of_the_same_widths_is_still_refused_past_1170_tokens(weights):
    """F's widths with 8 channels per head (the same tensors: the head dimension adds none): its training forward at 1x80x72
    stays refused by the LDS bound of the d = 8 backward pass, exactly as before"""
    from synt_isic_amd.train import HipAdam
    model = _build("F", weights["F"], attention_head_dim=8)
    HipAdam(model.parameters(), lr=1e-4)
    x, _, t = wh.batch("F", (1, 80, 72))
    try:
        model.train()
        _refused(lambda: model(x.to(DEV), t.to(DEV)), "80x72", "1440 tokens", "1170")
    finally:
        model.eval()


def _step_batch(name):
    cfg = wh.ARCHS_WIDE[name]
    B, H, W = FIRST[name]
    g = torch.Generator().manual_seed(7000 + ord(name))
    images = torch.rand(B, cfg.in_channels, H, W, generator=g) * 2 - 1
    noise = torch.randn(B, cfg.in_channels, H, W, generator=g)
    return images.to(DEV), noise.to(DEV), torch.tensor(arch_ref.TIMESTEPS[:B]).to(DEV)


@pytest.mark.parametrize("name", NAMES)
def test_fused_step_matches_the_spelled_out_step(name, weights):
    """sisic_unet_train_step against scaler.scale(loss).backward(); scaler.step(opt); scaler.update(): the same weights, bit
    for bit, after one step"""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, mse_loss, train_step_fused
    images, noise, timesteps = _step_batch(name)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    spelled = _build(name, weights[name])
    optimizer, scaler = HipAdam(spelled.parameters(), lr=1e-4), HipGradScaler()
    spelled.train()
    loss = mse_loss(spelled(scheduler.add_noise(images, noise, timesteps), timesteps).sample, noise)
    optimizer.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    assert scaler.step(optimizer) is True
    scaler.update()
    spelled.eval()
    fused = _build(name, weights[name])
    value, taken = train_step_fused(fused, scheduler, images, noise, timesteps, HipAdam(fused.parameters(), lr=1e-4), HipGradScaler())
    assert taken and abs(value - loss.item()) <= 1e-6 * abs(loss.item()), (value, loss.item())
    sd1, sd2 = spelled.state_dict(), fused.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert any(not torch.equal(sd1[k].cpu(), weights[name][k]) for k in sd1)


def _scheduler(rule, n):
    """DDPM: the first n steps (t = 999, 998, ...) of the T = 1000 grid; DPM-Solver++(2M): T = n on the leading grid"""
    from synt_isic_amd.scheduler import HipDDPMScheduler, HipDPMSolverMultistepScheduler
    if rule == "ddpm":
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        s.set_timesteps(1000)
        s.timesteps = s.timesteps[:n]
        assert s.timesteps.tolist() == list(range(999, 999 - n, -1))
    else:
        s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                           timestep_spacing="leading")
        s.set_timesteps(n)
        assert s.timesteps.tolist() == [750, 500, 250, 0]
    return s


def _executor_memory_poisoned():
    e = os.environ.get("SISIC_POISON_ALLOC")
    try:
        return e is not None and int(e) != 0
    except ValueError:
        return False


def _created_graph_mode():
    mode = -1
    if os.environ.get("SISIC_GRAPH") is not None:
        mode = 1 if int(os.environ["SISIC_GRAPH"] or 0) != 0 else 0
    if _executor_memory_poisoned():
        mode = 0
    return mode


@pytest.mark.parametrize("rule", ["ddpm", "dpmsolver++"])
@pytest.mark.parametrize("name", NAMES)
def test_sampling_loop_eager_graph_and_python_loop_agree(name, rule, models):
    """Four steps through run_sampling_loop against the Python loop over model(x, t).sample and the scheduler mirror's step,
    every frame bit for bit, and that run again as a replayed graph: the first call builds exactly one graph, the second none,
    both equal to the eager run.  (With SISIC_POISON_ALLOC set the library keeps graphs off and the graph leg is left out.)"""
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import run_sampling_loop
    lib = _lib.load()
    cfg = wh.ARCHS_WIDE[name]
    B, H, W = FIRST[name]
    model = models(name)
    g = torch.Generator().manual_seed(8000 + ord(name))
    x_T = torch.randn(B, cfg.in_channels, H, W, generator=g).to(DEV)
    n = 4
    sched = _scheduler(rule, n)
    n_noise = int((sched.coefficient_table()[:, 4] != 0).sum())
    assert n_noise == (n if rule == "ddpm" else 0)
    z = torch.randn(n_noise, B, cfg.in_channels, H, W, generator=g).to(DEV) if n_noise else None
    graph = None
    try:
        model.set_graph_mode(0)
        builds = lib.sisic_unet_graph_builds(model.handle)
        eager = run_sampling_loop(model, sched, x_T, z, return_trajectory=True)
        assert eager.steps_done == n and torch.isfinite(eager.latents).all()
        assert lib.sisic_unet_graph_builds(model.handle) == builds               # mode 0 never builds
        if rule != "ddpm":
            sched.set_timesteps(n)                                  # a new run: no history
        x, frames = x_T.clone(), []
        for i, t in enumerate(sched.timesteps):
            eps = model(x, t).sample
            x = sched.step(eps, t, x, variance_noise=None if z is None else z[i]).prev_sample
            frames.append(x)
        frames = torch.stack(frames)
        if not _executor_memory_poisoned():
            model.set_graph_mode(1)
            first = run_sampling_loop(model, sched, x_T, z, return_trajectory=True)     # captures the step
            assert lib.sisic_unet_graph_builds(model.handle) == builds + 1, "the first call in graph mode built no graph"
            graph = run_sampling_loop(model, sched, x_T, z, return_trajectory=True)     # replays it
            assert lib.sisic_unet_graph_builds(model.handle) == builds + 1, "the second call built a graph again"
            assert torch.equal(first.trajectory, graph.trajectory) and torch.equal(first.images, graph.images)
    finally:
        model.set_graph_mode(_created_graph_mode())
    if graph is not None:
        assert graph.steps_done == n
        assert torch.equal(eager.trajectory, graph.trajectory) and torch.equal(eager.latents, graph.latents)
        assert torch.equal(eager.images, graph.images)
    assert torch.equal(eager.trajectory, frames) and torch.equal(eager.latents, frames[-1])
    assert tuple(eager.images.shape) == (B, H, W, cfg.in_channels)


def test_sampler_add_model_passes_the_head_dim_through(weights):
    """Sampler.add_model(..., attention_head_dim=32): the model it builds is E, and generates"""
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV + ":0")
    s.add_model("E", weights["E"], **wh.unet_kwargs(wh.ARCHS_WIDE["E"]))
    res = s.generate_seeds("E", [0, 1], T=4, size=(16, 16))
    assert torch.isfinite(res.latents).all() and tuple(res.latents.shape) == (2, 3, 16, 16)
