"""The UNet, its training step and the sampling loops on architectures other than the reference's.

Every other GPU test, golden and tool runs ONE architecture: (64, 128, 256, 256), two layers per block, attention at level 2,
32 groups, 3 -> 3 channels.  The executor (unet.cpp: which launch gets which operand, which GroupNorm a conv2 finalises, where
each block's columns sit in the fused time projection), the tape and the repack plan follow whatever was described, and the
kernels meet planes, token counts and channel counts the reference's architecture never produces.  Here four others
(tests/arch_ref.py, ARCHS):

  A  (32, 64, 64), one layer, attention in the middle level, 8 groups, 1 -> 1        3x20x28, 2x32x32
  B  (32, 32, 64, 64, 128, 128), two layers, attention at level 4, 16 groups, 3 -> 3  2x64x64 (down to 2x2), 2x32x32 (down to 1x1)
  C  (96, 192), three layers, attention everywhere, 32 groups, 4 -> 4                 2x18x10, 1x16x16
  D  (32,), two layers, no resampler, one channel per group, 3 -> 6                   2x9x7

against tests/arch_ref.py, the config-generic restatement that test_arch_ref_cpu.py pins to the oracle, evaluated in float64.

Bars.  Nothing is fixed in advance but the project's factor: for every architecture and shape the restatement is evaluated in
fp32 and in float64 on the CPU, and the library is held to MODEL_FACTOR = 10 times the fp32 evaluation's own error -- on the
prediction (max abs), on the worst and on the median tensor of the per-tensor relative gradient error (the measure of
test_gpu_train._grad_errors).  It is the margin test_gpu_trained_like.py grants over the same quantity: the
fp32 reference is one legitimate summation order, the library's is another.  The tensors whose gradient vanishes identically
(arch_ref.vanishing_set, pinned on the CPU) stay out of the relative measure and below max(1e-7, 10 x the fp32 restatement's
own largest entry there); the loss is held to 1e-5 * max(1, |ref|).  Measured on MI355X: profiles/r26/arch_test_errors.txt.
"""
import math
import os

import pytest
import torch

import arch_ref
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODEL_FACTOR = 10.0
NAMES = list(arch_ref.ARCHS)
FIRST = {name: arch_ref.SHAPES[name][0] for name in NAMES}
ALL_SHAPES = [(name, shape) for name in NAMES for shape in arch_ref.SHAPES[name]]


def _log(line):
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(line + "\n")
    print(line)


def _sid(shape):
    return "x".join(str(v) for v in shape)


# ---------------------------------------------------------------- shared, computed once
@pytest.fixture(scope="module")
def weights():
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return {name: synthetic_unet_state_dict(cfg=cfg) for name, cfg in arch_ref.ARCHS.items()}


def _build(name, sd):
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel(**arch_ref.unet_kwargs(arch_ref.ARCHS[name]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def models(weights):
    """one model per architecture for the whole module (its weights are never stepped: the step tests build their own)"""
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
    """(name, shape) -> dict: the batch, the float64 restatement and the fp32 restatement's own errors against it.  The first
    shape of a row carries loss and gradients as well (the training tests), the others the prediction alone."""
    cache = {}

    def get(name, shape):
        key = (name, tuple(shape))
        if key in cache:
            return cache[key]
        cfg, sd = arch_ref.ARCHS[name], weights[name]
        x, target, t = arch_ref.batch(name, shape)
        r = {"x": x, "target": target, "t": t}
        if tuple(shape) == tuple(FIRST[name]):
            r["loss"], r["grads"], r["pred"] = arch_ref.loss_and_grads(cfg, sd, x, target, t, dtype=torch.float64)
            _, g32, p32 = arch_ref.loss_and_grads(cfg, sd, x, target, t, dtype=torch.float32)
            r["vanishing"] = arch_ref.vanishing_set(name)
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
    """max |pred - float64 restatement| <= 10 x the fp32 restatement's own; logged relative to the largest |prediction|"""
    top = ref["pred"].abs().max().item()
    err = (pred.detach().cpu().double() - ref["pred"]).abs().max().item()
    e32 = ref["e32_pred"]
    _log(f"{err / top:.3e}\t{e32 / top:.3e}\t{err / (MODEL_FACTOR * e32):.3f}\tprediction {what}: max abs err / max |pred| (= {top:.3f}); "
         f"fp32 restatement's; err / bar")
    assert tuple(pred.shape) == tuple(ref["pred"].shape)
    assert math.isfinite(err) and err <= MODEL_FACTOR * e32, f"{what}: prediction off by {err:.3e} > 10 x {e32:.3e}"


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("latency", [False, True], ids=["default", "latency"])
@pytest.mark.parametrize("name,shape", ALL_SHAPES, ids=[f"{n}-{_sid(s)}" for n, s in ALL_SHAPES])
def test_forward_matches_the_restatement(name, shape, latency, models, reference):
    """Every shape of the table in both modes against float64; row k of the batch equal to its own batch-1 forward and a second
    call equal to the first, bit for bit."""
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


@pytest.mark.parametrize("name", ["A", "C"])
def test_groupnorm_from_conv_epilogues_matches_standalone_pass(name, models, weights, reference, monkeypatch):
    """SISIC_FUSED_GN=0 (read when the handle is created, the route of test_gpu_unet.py's test of this name): the stand-alone
    statistics pass everywhere -- 8 and 4 channels per group in A, 3, 6 and 9 in C, where the epilogues' partials had only
    ever been merged for 8, 4 and 12.  The same network within the forward bar, and itself within the bar of float64."""
    monkeypatch.setenv("SISIC_FUSED_GN", "0")
    plain = _build(name, weights[name])
    monkeypatch.delenv("SISIC_FUSED_GN")
    model = models(name)
    for shape in arch_ref.SHAPES[name]:
        ref = reference(name, shape)
        x, t = ref["x"].to(DEV), ref["t"].to(DEV)
        a, b = model(x, t).sample, plain(x, t).sample
        _pred_bar(b, ref, f"{name} {_sid(shape)} SISIC_FUSED_GN=0")
        diff = (a - b).abs().max().item()
        _log(f"{diff:.3e}\t{MODEL_FACTOR * ref['e32_pred']:.3e}\t{diff / (MODEL_FACTOR * ref['e32_pred']):.3f}\tfused vs stand-alone "
             f"GroupNorm statistics {name} {_sid(shape)}: max abs difference; bar; ratio")
        assert diff <= MODEL_FACTOR * ref["e32_pred"]


# ---------------------------------------------------------------- refusals
def _refused(call, *words):
    from synt_isic_amd import _lib
    with pytest.raises(_lib.SisicError) as e:
        call()
    assert e.value.code == _lib.SISIC_EINVAL, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_a_resolution_that_is_no_multiple_of_the_downsampling_is_refused(models):
    """three levels: multiples of 4; six: multiples of 32.  The answer comes from the shape check, before anything runs."""
    a, b = models("A"), models("B")
    _refused(lambda: a(torch.zeros(1, 1, 18, 18, device=DEV), 5), "multiples of 4", "18x18")
    _refused(lambda: b(torch.zeros(1, 3, 48, 48, device=DEV), 5), "multiples of 32", "48x48")
    # ... and the models are none the worse for it
    assert torch.isfinite(a(torch.zeros(1, 1, 20, 20, device=DEV), 5).sample).all()
    assert torch.isfinite(b(torch.zeros(1, 3, 32, 32, device=DEV), 5).sample).all()


def test_full_resolution_attention_bounds_the_trainable_size(models, weights):
    """C has attention at full resolution: 40x40 = 1600 tokens exceed what the attention backward keeps in LDS
    (ATTN_BWD_MAX_TOKENS = 1170), so check_trainable_resolution refuses the TRAINING forward at its level 0 -- in the reference's
    architecture the bound bites at H*W/16.  The eval forward at that size still matches the restatement."""
    from synt_isic_amd.train import HipAdam
    cfg = arch_ref.ARCHS["C"]
    model = models("C")
    HipAdam(model.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(4040)
    x, t = torch.randn(1, 4, 40, 40, generator=g), torch.tensor([500])
    try:
        model.train()
        _refused(lambda: model(x.to(DEV), t.to(DEV)), "40x40", "1600 tokens", "1170")
    finally:
        model.eval()
    with torch.no_grad():
        p64 = arch_ref.unet_forward(cfg, {k: v.double() for k, v in weights["C"].items()}, x.double(), t)
        p32 = arch_ref.unet_forward(cfg, weights["C"], x, t)
    ref = {"pred": p64, "e32_pred": (p32.double() - p64).abs().max().item()}
    _pred_bar(model(x.to(DEV), t.to(DEV)).sample, ref, "C 1x40x40 eval (untrainable size)")


def test_differing_in_and_out_channels_are_refused_where_the_output_feeds_the_input(models):
    """D maps 3 channels to 6 (the learned-variance layout).  A sampling loop feeds the output back as the input, and the fused
    training step regresses it on the input-shaped noise: both refuse, the fused step naming both counts, before any buffer is
    grown or launch made (the weights and the gradient arena are untouched).  The spelled-out loop refuses the input-shaped
    target in mse_loss and takes an output-shaped one (the training test below)."""
    from synt_isic_amd.sampler import run_sampling_loop
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, mse_loss, train_step_fused
    model = models("D")
    B, H, W = FIRST["D"]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 3, H, W, generator=g).to(DEV)
    noise = torch.randn(B, 3, H, W, generator=g).to(DEV)
    t = torch.tensor(arch_ref.TIMESTEPS[:B])
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    sched.set_timesteps(3)
    _refused(lambda: run_sampling_loop(model, sched, x, None), "in/out channels differ")
    optimizer = HipAdam(model.parameters(), lr=1e-4)
    before, grads = model._read_all(0), model.grads()
    _refused(lambda: train_step_fused(model, sched, x, noise, t, optimizer, HipGradScaler()), "in/out channels differ",
             "3 input channels", "6 output channels")
    assert model.optimizer_state()["step"] == 0
    assert all(torch.equal(v, before[k]) for k, v in model._read_all(0).items())
    assert all(torch.equal(v, grads[k]) for k, v in model.grads().items())
    try:
        model.train()
        pred = model(x, t.to(DEV)).sample
        assert tuple(pred.shape) == (B, 6, H, W)
        with pytest.raises(RuntimeError, match="must match the prediction's"):
            mse_loss(pred, noise)
    finally:
        model.eval()


# ---------------------------------------------------------------- training
@pytest.mark.parametrize("latency", [False, True], ids=["default", "latency"])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_match_autograd_over_the_restatement(name, latency, models, reference):
    """HipAdam + model.train() forward + mse_loss(pred, target).backward(): loss, training-mode prediction and every gradient
    against float64; the tape-recording forward equal to the eval forward and a second forward/backward equal to the first, bit
    for bit."""
    from synt_isic_amd.train import HipAdam, mse_loss
    shape = FIRST[name]
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
        assert torch.equal(model(x, t).sample, pred)              # the tape-recording forward IS the forward
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


def _step_batch(name):
    """(images in [-1, 1], noise, timesteps) of the architecture's first shape, for the steps that add their own noise"""
    cfg = arch_ref.ARCHS[name]
    B, H, W = FIRST[name]
    g = torch.Generator().manual_seed(7000 + ord(name))
    images = torch.rand(B, cfg.in_channels, H, W, generator=g) * 2 - 1
    noise = torch.randn(B, cfg.in_channels, H, W, generator=g)
    return images.to(DEV), noise.to(DEV), torch.tensor(arch_ref.TIMESTEPS[:B]).to(DEV)


def _spelled_out_step(name, sd):
    """one step of the reference's loop on a fresh model: (model, loss value)"""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, mse_loss
    images, noise, timesteps = _step_batch(name)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    model = _build(name, sd)
    optimizer, scaler = HipAdam(model.parameters(), lr=1e-4), HipGradScaler()
    model.train()
    loss = mse_loss(model(scheduler.add_noise(images, noise, timesteps), timesteps).sample, noise)
    optimizer.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    assert scaler.step(optimizer) is True
    scaler.update()
    return model.eval(), loss.item()


@pytest.mark.parametrize("name", ["A", "B"])
def test_repacked_weights_after_a_step_equal_freshly_loaded_ones(name, weights):
    """After optimizer.step() every derived weight form (packed, Winograd, stride-2 split, transposed, the fused q/k/v and time
    projections) is rebuilt by the batched repack plan; a fresh model loaded with model.state_dict() builds them on the load
    path.  The same eval forward, bit for bit: the repack plan of this architecture names every form of every tensor."""
    stepped, _ = _spelled_out_step(name, weights[name])
    sd = stepped.state_dict()
    assert any(not torch.equal(sd[k].cpu(), weights[name][k]) for k in sd)
    fresh = _build(name, sd)
    for shape in arch_ref.SHAPES[name]:
        x, _, t = arch_ref.batch(name, shape)
        a, b = stepped(x.to(DEV), t.to(DEV)).sample, fresh(x.to(DEV), t.to(DEV)).sample
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{name} {_sid(shape)}"


@pytest.mark.parametrize("name", ["A", "B"])
def test_fused_step_matches_the_spelled_out_step(name, weights):
    """sisic_unet_train_step against scaler.scale(loss).backward(); scaler.step(opt); scaler.update(), as
    test_gpu_train.py's test at batch 32: the same weights, bit for bit, after one step."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, train_step_fused
    spelled, loss = _spelled_out_step(name, weights[name])
    images, noise, timesteps = _step_batch(name)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    fused = _build(name, weights[name])
    value, taken = train_step_fused(fused, scheduler, images, noise, timesteps, HipAdam(fused.parameters(), lr=1e-4), HipGradScaler())
    assert taken and abs(value - loss) <= 1e-6 * abs(loss), (value, loss)
    sd1, sd2 = spelled.state_dict(), fused.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert any(not torch.equal(sd1[k].cpu(), weights[name][k]) for k in sd1)


# ---------------------------------------------------------------- sampling
GRAPH_MIN_STEPS = 4          # sisic_sample* replays a captured step only for runs of 4 .. 1000 steps (unet.cpp, use_graph)


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
        assert s.timesteps.tolist() == {3: [666, 333, 0], 4: [750, 500, 250, 0]}[n]
    return s


def _created_graph_mode():
    """the graph mode sisic_unet_create leaves a handle in: SISIC_GRAPH forces 0 / 1, poisoned executor memory turns it off,
    otherwise -1 (follow the latency mode)"""
    mode = -1
    if os.environ.get("SISIC_GRAPH") is not None:
        mode = 1 if int(os.environ["SISIC_GRAPH"] or 0) != 0 else 0
    if _executor_memory_poisoned():
        mode = 0
    return mode


def _executor_memory_poisoned():
    e = os.environ.get("SISIC_POISON_ALLOC")
    try:
        return e is not None and int(e) != 0
    except ValueError:
        return False


@pytest.mark.parametrize("rule", ["ddpm", "dpmsolver++"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sampling_loop_eager_graph_and_python_loop_agree(name, rule, models):
    """Three steps through run_sampling_loop against the Python loop over model(x, t).sample and the scheduler mirror's step --
    every frame, bit for bit -- and image k against its own batch-1 run.  A run of three steps is below the library's graph
    threshold (four), so the same is done at FOUR steps, and that run again as a replayed graph: the mode set explicitly, the
    first call building exactly one graph (sisic_unet_graph_builds), the second building none, both equal to the eager run bit
    for bit.  (With SISIC_POISON_ALLOC set the library keeps graphs off -- no memset nodes go into a captured step -- and
    the graph leg is left out.)"""
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import run_sampling_loop
    lib = _lib.load()
    cfg = arch_ref.ARCHS[name]
    B, H, W = FIRST[name]
    model = models(name)
    g = torch.Generator().manual_seed(8000 + ord(name))
    x_T = torch.randn(B, cfg.in_channels, H, W, generator=g).to(DEV)
    for n in (3, GRAPH_MIN_STEPS):
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
            singles = [run_sampling_loop(model, sched, x_T[k:k + 1].contiguous(), None if z is None else z[:, k:k + 1].contiguous())
                       for k in range(B)]
            assert lib.sisic_unet_graph_builds(model.handle) == builds               # mode 0 never builds
            # the Python loop over the two drop-in objects
            if rule != "ddpm":
                sched.set_timesteps(n)                                  # a new run: no history
            x, frames = x_T.clone(), []
            for i, t in enumerate(sched.timesteps):
                eps = model(x, t).sample
                x = sched.step(eps, t, x, variance_noise=None if z is None else z[i]).prev_sample
                frames.append(x)
            frames = torch.stack(frames)
            if n >= GRAPH_MIN_STEPS and not _executor_memory_poisoned():
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
        for k, one in enumerate(singles):
            assert torch.equal(one.latents, eager.latents[k:k + 1]), f"image {k}: its bits depend on the batch it is in"
