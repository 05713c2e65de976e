"""Classifier guidance on the GPU (include/sisic.h, "classifier guidance"): the per-image-target input gradient, the combine
against the restatement (tests/clf_guide_ref.py), the in-library guided loop against a Python loop over the drop-in objects, the
captured step's key (scale and targets replay, the classifier's workspace generation re-captures, in-place weights do not), the
direction of a guided step, a held side stream, the refusals and the public interface.

UNet: the real configuration with synthetic weights, B = 3 at 3x32x32, T = 6 (tests/test_gpu_cond.py's shape, half its steps).
Classifier: synthetic_resnet18_state_dict, 7 classes, as in tests/test_gpu_classifier.py.  With synthetic weights nothing here
says anything about image quality or class fidelity.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import clf_guide_ref as ref
import stream_probe as sp
from test_gpu_device_noise import eager, graph  # noqa: F401  (the two graph-mode fixtures, shared)

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
NPI = int(np.prod(CHW))
B, T = 3, 6
SEEDS = [11, (1 << 33) + 2, 0]
TARGETS = [0, 2, 0]
SCALE = 2.5
LOOP_RULES = [("ddpm", {}), ("ddim", {"eta": 0.0}), ("ddim", {"eta": 1.0}), ("dpmsolver++", {"solver_order": 1}),
              ("dpmsolver++", {"solver_order": 2})]
LOOP_IDS = ["ddpm", "ddim-eta0", "ddim-eta1", "dpmpp-order1", "dpmpp-order2"]


@pytest.fixture(scope="module")
def clf():
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    m = HipMelanomaClassifier(num_classes=7, pretrained=False)
    m.load_state_dict(synthetic_resnet18_state_dict())
    return m.to(DEV).eval()


def _scheduler(rule, opt, steps=T):
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    if rule == "ddpm":
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    elif rule == "ddim":
        s = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    else:
        s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                           timestep_spacing="leading", solver_order=opt["solver_order"])
    s.set_timesteps(steps)
    return s, float(opt.get("eta", 0.0))


def _table(sched, eta):
    return sched.rule_table(eta)[1]


def _x_T(seeds, chw=CHW):
    # half the usual scale: most pixels of the first steps then lie inside [-1, 1], where the classifier's clamp lets a gradient through
    return torch.stack([0.5 * torch.randn(chw, generator=torch.Generator().manual_seed(5000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _python_loop(model, clf, sched, eta, x_T, seeds, targets, scale, steps=T):
    """image_generator.py:395-403 over the drop-in objects with the guidance spelled out: the UNet, the classifier's input
    gradient at the same latent, ops.clf_guide_eps, the scheduler's step on ops.noise_fill's z.  Returns every frame."""
    from synt_isic_amd import ops
    sched.set_timesteps(steps)                                          # a new run (DPM-Solver++: no history)
    tab = _table(sched, eta)
    kw = dict(eta=eta) if sched.rule == "ddim" else {}
    x, frames = x_T.clone(), []
    for i, t in enumerate(sched.timesteps):
        eps = model(x, t).sample
        g, _ = clf.input_gradient(x, list(targets))
        eps = ops.clf_guide_eps(eps, g, float(tab[i, 0]), scale)
        vn = None
        if float(tab[i, 4]) != 0.0:
            vn = ops.noise_fill(seeds, NPI, i).reshape(x.shape)
        x = sched.step(eps, t, x, variance_noise=vn, **kw).prev_sample
        frames.append(x)
    return torch.stack(frames)


def _guided(model, clf, sched, eta, x_T, seeds, targets, scale, **kw):
    from synt_isic_amd.sampler import ClassifierGuidance, DeviceNoise, run_sampling_loop
    return run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), eta=eta, classifier=ClassifierGuidance(clf, targets, scale), **kw)


# ---- 1. per-image targets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 32, 32), (2, 40, 56)])
def test_per_image_targets_are_the_single_target_rows(clf, shape):
    n, H, W = shape
    x = (torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(7)) * 0.8).to(DEV)
    targets = [0, 2, 0][:n]
    g, logits = clf.input_gradient(x, targets)
    assert torch.equal(logits, clf.forward(x))
    assert torch.isfinite(g).all() and bool((g != 0).any())
    for b, t in enumerate(targets):
        gs, ls = clf.input_gradient(x, t)
        assert torch.equal(g[b], gs[b]) and torch.equal(logits, ls)
    same, _ = clf.input_gradient(x, [1] * n)                            # equal targets: the single-target launch's bits
    assert torch.equal(same, clf.input_gradient(x, 1)[0])
    again, logits2 = clf.input_gradient(x, torch.tensor(targets))
    assert torch.equal(again, g) and torch.equal(logits2, logits)
    assert not torch.equal(g[1], clf.input_gradient(x, 0)[0][1])        # the target reaches the row
    with pytest.raises(ValueError, match="target classes for a batch"):
        clf.input_gradient(x, [0])


# ---- 2. the combine ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 4099, 12288])
def test_clf_guide_eps_is_the_restatement_bit_for_bit(n):
    from synt_isic_amd import ops
    gen = torch.Generator().manual_seed(n)
    e, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3
    for offset in (1, 0):
        view = lambda t: torch.cat([torch.zeros(offset), t, torch.zeros(4)]).to(DEV)[offset:offset + n]     # noqa: E731
        ed, gd = view(e), view(g)
        assert ed.data_ptr() % 16 == 4 * offset
        for sb, scale in ((0.7104, 0.7), (0.9655, 3.0), (0.2691, -0.5), (0.5, 0.0)):
            want = torch.from_numpy(ref.combine_np(e.numpy(), g.numpy(), sb, scale))
            out = view(torch.zeros(n))
            ops.clf_guide_eps(ed, gd, sb, scale, out=out)
            assert torch.equal(out.cpu(), want), (n, offset, sb, scale)
            assert torch.equal(ops.clf_guide_eps(ed, gd, sb, scale).cpu(), want)
            assert torch.equal(want, ref.combine(e, g, sb, scale))
        assert torch.equal(ed.cpu(), e) and torch.equal(gd.cpu(), g)    # the inputs are read only
        a, b = view(e), view(g)                                         # out may be eps
        ops.clf_guide_eps(a, b, 0.9655, 3.0, out=a)
        assert torch.equal(a.cpu(), torch.from_numpy(ref.combine_np(e.numpy(), g.numpy(), 0.9655, 3.0))) and torch.equal(b.cpu(), g)


# ---- 3. the library loop against the Python loop -----------------------------------------------------------------------
@pytest.mark.parametrize("rule,opt", LOOP_RULES, ids=LOOP_IDS)
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_library_loop_equals_python_loop(mode, rule, opt, eager, graph, clf):
    from synt_isic_amd import ops
    s = eager if mode == "eager" else graph
    model = s.models["NV"]
    x_T = _x_T(SEEDS)
    sched, eta = _scheduler(rule, opt)
    frames = _python_loop(model, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    res = _guided(model, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE, return_trajectory=True)
    assert res.steps_done == T and res.classifier_scale == SCALE and res.classifier_passes == T
    assert torch.equal(res.latents, frames[-1]) and torch.equal(res.trajectory, frames)
    assert torch.equal(res.images, ops.denorm_u8(frames[-1])) and not torch.equal(res.images, ops.denorm_u8(x_T))
    keep = [0, 3, T - 1]
    kept = _guided(model, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE, return_trajectory=True, save_indices=keep)
    assert kept.trajectory_steps == keep and torch.equal(kept.trajectory, frames[keep]) and torch.equal(kept.images, res.images)
    # the guidance and the targets reach the result
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    plain = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), eta=eta)
    assert not torch.equal(plain.latents, res.latents)
    other = _guided(model, clf, sched, eta, x_T, SEEDS, [1, 2, 0], SCALE)
    assert not torch.equal(other.latents[0], res.latents[0]) and torch.equal(other.latents[1:], res.latents[1:])


# ---- 4. scale 0 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_scale_zero_gives_the_plain_loop(mode, eager, graph, clf):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    model = (eager if mode == "eager" else graph).models["NV"]
    x_T = _x_T(SEEDS)
    for rule, opt in (LOOP_RULES[0], LOOP_RULES[4]):
        sched, eta = _scheduler(rule, opt)
        plain = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), eta=eta, return_trajectory=True)
        zero = _guided(model, clf, sched, eta, x_T, SEEDS, TARGETS, 0.0, return_trajectory=True)
        assert torch.equal(zero.trajectory, plain.trajectory) and torch.equal(zero.images, plain.images)
        assert zero.classifier_scale == 0.0 and plain.classifier_scale is None and plain.classifier_passes == 0


# ---- 5.-7. the captured step's key -------------------------------------------------------------------------------------
def test_replay_serves_other_scales_and_targets(eager, graph, clf):
    from synt_isic_amd import _lib
    lib = _lib.load()
    gm, em = graph.models["NV"], eager.models["NV"]
    x_T = _x_T(SEEDS)
    sched, eta = _scheduler(*LOOP_RULES[0])
    first = _guided(gm, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    builds = lib.sisic_unet_graph_builds(gm.handle)
    assert builds >= 1
    second = _guided(gm, clf, sched, eta, x_T, SEEDS, [3, 1, 6], -0.75)
    assert lib.sisic_unet_graph_builds(gm.handle) == builds            # another scale, other targets: the same captured step
    want = _guided(em, clf, sched, eta, x_T, SEEDS, [3, 1, 6], -0.75)
    assert torch.equal(second.latents, want.latents) and torch.equal(second.images, want.images)
    assert not torch.equal(second.latents, first.latents)
    assert torch.equal(_guided(gm, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE).latents, first.latents)
    assert lib.sisic_unet_graph_builds(gm.handle) == builds


def test_a_classifier_call_at_another_shape_forces_a_recapture(graph, clf):
    from synt_isic_amd import _lib
    lib = _lib.load()
    gm = graph.models["NV"]
    x_T = _x_T(SEEDS)
    sched, eta = _scheduler(*LOOP_RULES[0])
    first = _guided(gm, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    builds = lib.sisic_unet_graph_builds(gm.handle)
    clf.forward(torch.zeros(5, 3, 32, 32, device=DEV))                  # releases the blocks the captured step holds
    again = _guided(gm, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    assert lib.sisic_unet_graph_builds(gm.handle) == builds + 1
    assert torch.equal(again.latents, first.latents) and torch.equal(again.images, first.images)


def test_a_classifier_created_again_never_matches_the_old_key(eager, graph):
    """a handle destroyed and created again (``to("cpu").to("cuda")``; a classifier that goes out of scope and a new one) usually
    gets the old address back and walks through the same sequence of states: the generations come from one process-wide
    counter, so the captured step of the old handle -- whose blocks and filters are freed -- is not replayed"""
    from synt_isic_amd import _lib
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    lib = _lib.load()
    gm, em = graph.models["NV"], eager.models["NV"]
    x_T = _x_T(SEEDS)
    sched, eta = _scheduler(*LOOP_RULES[0])

    def fresh():
        m = HipMelanomaClassifier(num_classes=7, pretrained=False)
        m.load_state_dict(synthetic_resnet18_state_dict())
        return m.to(DEV).eval()

    own = fresh()
    first = _guided(gm, own, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    builds = lib.sisic_unet_graph_builds(gm.handle)
    own = own.to("cpu").to(DEV)                                         # destroys the handle, creates and loads another
    moved = _guided(gm, own, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    assert lib.sisic_unet_graph_builds(gm.handle) == builds + 1
    assert torch.equal(moved.latents, first.latents) and torch.equal(moved.images, first.images)
    assert torch.equal(moved.latents, _guided(em, own, sched, eta, x_T, SEEDS, TARGETS, SCALE).latents)
    del own                                                             # __del__ destroys; the next handle may reuse the address
    other = fresh()
    other.input_gradient(x_T, TARGETS)                                  # already at the loop's shape before the guided call
    again = _guided(gm, other, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    assert lib.sisic_unet_graph_builds(gm.handle) == builds + 2
    assert torch.equal(again.latents, first.latents) and torch.equal(again.images, first.images)


def test_weights_changed_in_place_need_no_recapture(eager, graph, clf):
    from synt_isic_amd import _lib
    lib = _lib.load()
    gm, em = graph.models["NV"], eager.models["NV"]
    x_T = _x_T(SEEDS)
    sched, eta = _scheduler(*LOOP_RULES[0])
    first = _guided(gm, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    builds = lib.sisic_unet_graph_builds(gm.handle)
    clf.randomize_weights(seed=9, trial=1, strength=0.05)
    try:
        rg = _guided(gm, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
        re = _guided(em, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
        assert torch.equal(rg.latents, re.latents) and not torch.equal(rg.latents, first.latents)
    finally:
        clf.restore_weights()
    back = _guided(gm, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE)
    assert torch.equal(back.latents, first.latents)
    assert torch.equal(back.latents, _guided(em, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE).latents)
    assert lib.sisic_unet_graph_builds(gm.handle) == builds


# ---- 8. batch independence ---------------------------------------------------------------------------------------------
def test_an_image_does_not_depend_on_its_batch(eager, clf):
    model = eager.models["NV"]
    x_T = _x_T(SEEDS)
    for rule, opt in (LOOP_RULES[0], LOOP_RULES[4]):
        sched, eta = _scheduler(rule, opt)
        whole = _guided(model, clf, sched, eta, x_T, SEEDS, TARGETS, SCALE, return_trajectory=True)
        alone = _guided(model, clf, sched, eta, x_T[1:2], SEEDS[1:2], TARGETS[1:2], SCALE, return_trajectory=True)
        assert torch.equal(alone.trajectory[:, 0], whole.trajectory[:, 1]) and torch.equal(alone.images[0], whole.images[1])


# ---- 9. the direction --------------------------------------------------------------------------------------------------
def _one_step(model, clf, name, x, scale, clip=0.0):
    """one eager library step at tests/clf_guide_ref.py's timestep, x0 clipping off: x_prev [B,C,H,W]"""
    from synt_isic_amd import _lib
    from synt_isic_amd._lib import check
    rule, row = ref.direction_row(name)
    sched, _ = _scheduler(rule, dict(next(o for n, _, o in ref.RULES if n == name)), ref.DIRECTION_T)
    t = (C.c_int64 * 1)(int(sched.timesteps[ref.DIRECTION_STEP]))
    coef = (C.c_float * len(row))(*row)
    out = x.clone()
    a = _lib.SampleClfArgs(x=out.data_ptr(), timesteps=C.cast(t, _lib.c_int64_p), coef=C.cast(coef, _lib.c_float_p),
                           seeds=(C.c_uint64 * B)(*SEEDS), classifier=clf.handle, targets=(C.c_int64 * B)(*TARGETS),
                           stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), B=B, H=32, W=32, T=1,
                           rule={"ddpm": _lib.RULE_DDPM, "ddim": _lib.RULE_DDIM, "dpmsolver++": _lib.RULE_DPMPP}[rule],
                           step0=ref.DIRECTION_STEP, clip=clip, scale=scale)
    check(_lib.load().sisic_sample_frames_clf(model.handle, C.byref(a)))
    assert a.steps_done == 1
    return out


# (dpmpp-order2's row at this step has k1 != 0, which a call's first step may not have: its history term is the same in the guided
#  and the plain run, and tests/test_clf_guide_cpu.py covers it; the second-order kernel path runs in the loop tests above)
@pytest.mark.parametrize("name", [n for n, _, _ in ref.RULES if n != "dpmpp-order2"])
def test_a_guided_step_moves_up_the_classifier(name, eager, clf):
    """x_guided - x_plain against the g the library returns: cosine >= 1 - 1e-6 (the bar tests/test_clf_guide_cpu.py shows the
    restatement meets at this timestep and scale), and log p(c | x_prev) does not fall for a scale whose largest shift is 1e-2.

    fp32 torch on the CPU for this pair (oracle/resnet18.py with these weights, latents, targets and Philox z, a random normal
    tensor standing in for the UNet's eps, max |g| = 1.10e-2): log p(c | x_prev) plain -> guided, images 0, 1, 2
        ddpm, ddim-eta1      -2.180615 -> -2.178890,  -3.349737 -> -3.347090,  -2.207894 -> -2.206165   (+1.7e-3 .. +2.6e-3)
        ddim-eta0, dpmpp-1   -2.130119 -> -2.126868,  -3.211618 -> -3.206953,  -2.177580 -> -2.174250   (+3.3e-3 .. +4.7e-3)
    three orders of magnitude above fp32 rounding of the score.  The GPU's own pair is printed below."""
    model = eager.models["NV"]
    x = _x_T(SEEDS)
    g, _ = clf.input_gradient(x, TARGETS)
    assert bool((g != 0).any())
    plain = _one_step(model, clf, name, x, 0.0)
    guided = _one_step(model, clf, name, x, ref.DIRECTION_SCALE)
    cos = ref.cosine((guided - plain).cpu(), g.cpu())
    print(f"{name}: cosine(x_guided - x_plain, g) = 1 - {1 - cos:.3e}")
    assert cos >= ref.DIRECTION_COSINE
    rule, row = ref.direction_row(name)
    small = 1e-2 / (ref.kappa_over_k(rule, row) * row[0] * float(g.abs().max()))
    nudged = _one_step(model, clf, name, x, small)
    shift = float((nudged - plain).abs().max())
    assert 0.5e-2 <= shift <= 1.5e-2
    for b, c in enumerate(TARGETS):
        lp_plain = float(clf.get_per_class_score(plain[b:b + 1], c))
        lp_guided = float(clf.get_per_class_score(nudged[b:b + 1], c))
        print(f"{name}: image {b}, class {c}: log p plain {lp_plain:.6f}, guided {lp_guided:.6f}")
        assert lp_guided >= lp_plain


# ---- 10. a held side stream --------------------------------------------------------------------------------------------
def test_side_stream_gives_the_default_stream_bits(graph, clf):
    """one guided graph run on a side stream that a spin kernel holds, the latents copied in behind the hold"""
    gm = graph.models["NV"]
    sched, eta = _scheduler(*LOOP_RULES[4])

    def fn(x):
        r = _guided(gm, clf, sched, eta, x, SEEDS, TARGETS, SCALE, return_trajectory=True)
        return r.latents, r.trajectory, r.images

    baseline, held, _ = sp.run_held(fn, lambda: [_x_T(SEEDS)], lambda: [_x_T([5, 6, 7])], "classifier-guided graph loop")
    assert sp.same(baseline, held)


# ---- 11. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(eager, clf):
    from synt_isic_amd import _lib, ops
    from synt_isic_amd.sampler import ClassifierGuidance, DeviceNoise, Sampler, run_sampling_loop
    from synt_isic_amd.unet import HipUNet2DModel
    from synt_isic_amd.weights import synthetic_unet_state_dict
    lib = _lib.load()
    model = eager.models["NV"]
    sched, eta = _scheduler(*LOOP_RULES[0])
    x_T = _x_T(SEEDS)
    before = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS)).latents
    x = x_T.clone()
    t = (C.c_int64 * 2)(500, 0)
    coef = (C.c_float * 10)(0.6, 0.8, 0.5, 0.5, 0.1, 0.6, 0.8, 0.5, 0.5, 0.0)
    seeds = (C.c_uint64 * B)(*SEEDS)

    def call(handle=None, **kw):
        f = dict(x=x.data_ptr(), timesteps=C.cast(t, _lib.c_int64_p), coef=C.cast(coef, _lib.c_float_p), seeds=seeds,
                 classifier=clf.handle, targets=(C.c_int64 * B)(*TARGETS), stream=C.c_void_p(torch.cuda.current_stream().cuda_stream),
                 B=B, H=32, W=32, T=2, rule=_lib.RULE_DDPM, clip=1.0, scale=2.0, steps_done=-1)
        f.update(kw)
        a = _lib.SampleClfArgs(**f)
        rc = lib.sisic_sample_frames_clf(handle or model.handle, C.byref(a))
        return rc, a.steps_done, lib.sisic_last_error()

    def refused(needle, **kw):
        rc, done, msg = call(**kw)
        assert rc == _lib.SISIC_EINVAL and done == 0 and needle in msg, (rc, done, msg)

    cond = HipUNet2DModel(num_class_embeds=3)
    cond.load_state_dict(synthetic_unet_state_dict(num_class_embeds=3))
    cond = cond.to(DEV)
    refused(b"class-conditional", handle=cond.handle)
    vmodel = HipUNet2DModel(prediction_type="v_prediction")
    vmodel.load_state_dict(synthetic_unet_state_dict())
    vmodel = vmodel.to(DEV)
    refused(b"prediction_type", handle=vmodel.handle)
    smodel = HipUNet2DModel(prediction_type="sample")
    smodel.load_state_dict(synthetic_unet_state_dict())
    smodel = smodel.to(DEV)
    refused(b"prediction_type", handle=smodel.handle)
    z = torch.zeros((1, B) + CHW, device=DEV)
    refused(b"host noise", noise=z.data_ptr())
    refused(b"host noise", seeds=None)
    h = C.c_void_p()
    _lib.check(lib.sisic_resnet_create(ops.context(torch.device(DEV)), 7, C.byref(h)))
    try:
        refused(b"not loaded", classifier=h)
    finally:
        lib.sisic_resnet_destroy(h)
    ctx2 = C.c_void_p()
    _lib.check(lib.sisic_create(torch.cuda.current_device(), C.byref(ctx2)))
    h2 = C.c_void_p()
    _lib.check(lib.sisic_resnet_create(ctx2, 7, C.byref(h2)))
    try:
        refused(b"another context", classifier=h2)
    finally:
        lib.sisic_resnet_destroy(h2)
        lib.sisic_destroy(ctx2)
    refused(b"224x224", H=256, W=32)
    refused(b"outside [0, 7)", targets=(C.c_int64 * B)(0, 7, 0))
    refused(b"outside [0, 7)", targets=(C.c_int64 * B)(0, 1, -1))
    refused(b"classifier scale", scale=float("nan"))
    refused(b"classifier scale", scale=float("inf"))
    assert torch.equal(x, x_T)                                          # nothing was launched
    # the per-image-target gradient checks every target before its first launch
    gx = torch.zeros_like(x)
    a = _lib.ResnetTargetsArgs(x=x.data_ptr(), targets=(C.c_int64 * B)(0, 1, 7), grad_x=gx.data_ptr(),
                               stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), B=B, H=32, W=32)
    assert lib.sisic_resnet_input_gradient_targets(clf.handle, C.byref(a)) == _lib.SISIC_EINVAL
    assert b"outside [0, 7)" in lib.sisic_last_error() and not bool(gx.any())
    # the Python surface
    cg = ClassifierGuidance(clf, TARGETS, 2.0)
    with pytest.raises(ValueError, match="prediction_type"):
        run_sampling_loop(vmodel, sched, x_T, DeviceNoise(SEEDS), classifier=cg)
    with pytest.raises(ValueError, match="prediction_type"):
        run_sampling_loop(smodel, sched, x_T, DeviceNoise(SEEDS), classifier=cg)
    with pytest.raises(ValueError, match='noise="device"'):
        run_sampling_loop(model, sched, x_T, None, classifier=cg)
    with pytest.raises(ValueError, match="class-conditional"):
        run_sampling_loop(cond, sched, x_T, DeviceNoise(SEEDS), classifier=cg)
    with pytest.raises(ValueError, match="finite"):
        ClassifierGuidance(clf, TARGETS, float("nan"))
    with pytest.raises(ValueError, match="outside"):
        run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), classifier=ClassifierGuidance(clf, [0, 9, 0], 2.0))
    s = Sampler(DEV)
    s.models["NV"] = model
    kw = dict(T=4, size=(32, 32))
    with pytest.raises(ValueError, match="set_classifier"):
        s.generate_seeds("NV", [1], classifier_scale=2.0, noise="device", **kw)
    s.set_classifier(clf, {"NV": 1})
    with pytest.raises(ValueError, match='noise="device"'):
        s.generate_seeds("NV", [1], classifier_scale=2.0, **kw)
    with pytest.raises(ValueError, match="guidance_scale"):
        s.generate_seeds("NV", [1], classifier_scale=2.0, guidance_scale=3.0, noise="device", **kw)
    with pytest.raises(ValueError, match="init_image"):
        s.generate_seeds("NV", [1], classifier_scale=2.0, noise="device", init_image=torch.zeros(1, 3, 32, 32), strength=0.5, **kw)
    with pytest.raises(ValueError, match="outside the classifier"):
        s.set_classifier(clf, {"NV": 7})
    s.add_conditional_model(["MEL", "BCC"], synthetic_unet_state_dict(num_class_embeds=3)).set_graph_mode(0)
    s.set_classifier(clf, {"NV": 1, "MEL": 0, "BCC": 2})
    with pytest.raises(ValueError, match="class-conditional"):
        s.generate_seeds("MEL", [1], classifier_scale=2.0, noise="device", **kw)
    with pytest.raises(ValueError, match="class-conditional"):
        s.generate(1, ["MEL", "BCC"], 4, size=(32, 32), classifier_scale=2.0, noise="device")
    # a plain call afterwards returns the bits it returned before
    assert torch.equal(run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS)).latents, before)


# ---- 12. the public interface ------------------------------------------------------------------------------------------
def test_generate_with_mixed_class_names(eager, clf):
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV)
    s.models["NV"] = s.models["MEL"] = eager.models["NV"]               # one unconditional model under two names
    s.set_classifier(clf, {"NV": 1, "MEL": 4})
    names, seeds = ["MEL", "NV", "MEL"], [3, 0x7FFFFFFF, 12345]
    kw = dict(T=4, size=(32, 32), noise="device", classifier_scale=2.0)
    res = s.generate_seeds(names, seeds, return_trajectory=True, **kw)
    assert res.steps_done == 4 and res.classifier_scale == 2.0 and res.classifier_passes == 4 and torch.isfinite(res.latents).all()
    plain = s.generate_seeds("NV", seeds, T=4, size=(32, 32), noise="device")
    assert res.noise_hashes == plain.noise_hashes and not torch.equal(res.latents, plain.latents)
    for b, (name, seed) in enumerate(zip(names, seeds)):
        one = s.generate_seeds(name, [seed], return_trajectory=True, **kw)
        assert torch.equal(one.latents[0], res.latents[b]) and torch.equal(one.images[0], res.images[b])
        assert torch.equal(one.trajectory[:, 0], res.trajectory[:, b])
    assert not torch.equal(res.latents[0], s.generate_seeds("NV", [seeds[0]], **kw).latents[0])        # the name chooses the target
    imgs, traj = s.generate(7, names, 4, size=(32, 32), noise="device", classifier_scale=2.0)
    by_seed = s.generate_images(names, [7, 8, 9], 4, size=(32, 32), noise="device", classifier_scale=2.0)
    assert traj is None and np.array_equal(imgs, by_seed.images.cpu().numpy())


# ---- 13. a classifier that has seen noisy images -----------------------------------------------------------------------
def _restated_draws(seed, epoch, batch, n, lo, hi):
    """train.classifier_noise_draws, restated: word 2b of numpy's Philox under (key seed, counter (epoch, batch, 0, 0)) gives t_b
    by multiply-shift on its high half, word 2b + 1 is the seed of z_b"""
    words = [int(w) for w in np.random.Philox(key=seed, counter=[epoch, batch, 0, 0]).random_raw(2 * n)]
    return [lo + (((w >> 32) * (hi - lo + 1)) >> 32) for w in words[0::2]], words[1::2]


def _train_batch(n=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, 32, 32, generator=g) * 2 - 1).to(DEV), torch.randint(0, 7, (n,), generator=g)


def _new_clf():
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    m = HipMelanomaClassifier(num_classes=7)
    m.load_state_dict(synthetic_resnet18_state_dict())
    return m.to(DEV)


def test_a_noised_batch_is_add_noise_on_the_restated_draws():
    from synt_isic_amd import ops, train
    from synt_isic_amd.scheduler import HipDDPMScheduler
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    images, _ = _train_batch()
    for epoch, batch, (lo, hi) in ((0, 0, (0, 999)), (2, 5, (100, 400)), (1, 0, (250, 250))):
        x_t, t = train.noise_classifier_batch(images, sched, 77, epoch, batch, (lo, hi))
        ts, zseeds = _restated_draws(77, epoch, batch, 4, lo, hi)
        assert t.tolist() == ts and all(lo <= v <= hi for v in ts)
        z = ops.noise_fill(zseeds, NPI, 0, train.CLASSIFIER_NOISE_TAG).reshape(images.shape)
        assert torch.equal(x_t, sched.add_noise(images, z, torch.tensor(ts)))
        # a pure function of the position: image 1 alone gets image 1's draws only as part of its batch's prefix
        x2, t2 = train.noise_classifier_batch(images[:2], sched, 77, epoch, batch, (lo, hi))
        assert torch.equal(x2, x_t[:2]) and t2.tolist() == ts[:2]
    assert not torch.equal(train.noise_classifier_batch(images, sched, 78, 0, 0, (0, 999))[0],
                           train.noise_classifier_batch(images, sched, 77, 0, 0, (0, 999))[0])
    with pytest.raises(ValueError, match="noise_timesteps"):
        train.classifier_noise_draws(0, 0, 0, 4, (500, 100))


def test_train_classifier_on_noised_batches_equals_the_hand_noised_steps():
    """two steps (one epoch over two batches, then a second epoch's first draw differs) against loss_backward + step on batches
    noised by hand; noise_timesteps=None against today's run"""
    from synt_isic_amd import train
    from synt_isic_amd.scheduler import HipDDPMScheduler
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    batches = [_train_batch(seed=3), _train_batch(seed=4)]

    def trained(**kw):
        clf = _new_clf()
        history = train.train_classifier(clf, batches, epochs=1, lr=1e-3, log=None, **kw)
        return history[0]["loss"], clf.state_dict()

    loss, sd = trained(noise_timesteps=(50, 700), noise_seed=9)
    by_hand = _new_clf()
    opt = train.HipClassifierAdam(by_hand, lr=1e-3)
    total = 0.0
    for i, (images, labels) in enumerate(batches):
        ts, zseeds = _restated_draws(9, 0, i, 4, 50, 700)
        from synt_isic_amd import ops
        z = ops.noise_fill(zseeds, NPI, 0, train.CLASSIFIER_NOISE_TAG).reshape(images.shape)
        value, _ = by_hand.loss_backward(sched.add_noise(images, z, torch.tensor(ts)), labels)
        opt.step()
        total += value
    want = by_hand.state_dict()
    opt.close()
    assert loss == total / 2 and all(torch.equal(sd[k], want[k]) for k in want)
    # off by default: today's launches, today's bits
    loss0, sd0 = trained()
    plain = _new_clf()
    opt = train.HipClassifierAdam(plain, lr=1e-3)
    total = 0.0
    for images, labels in batches:
        total += plain.loss_backward(images, labels)[0]
        opt.step()
    want0 = plain.state_dict()
    opt.close()
    assert loss0 == total / 2 and all(torch.equal(sd0[k], want0[k]) for k in want0)
    assert loss0 != loss and any(not torch.equal(sd0[k], sd[k]) for k in sd)
