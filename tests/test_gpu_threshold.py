"""Dynamic thresholding of x0 on the GPU, bit for bit against tests/threshold_ref.py: the selection kernel alone, one step of
every rule, the scheduler mirrors, the fused loops (eager and graph-replayed; plain, classifier-free guidance, classifier
guidance, inpainting) against the Python loop over the drop-in objects, the handle's and the captured step's state, one chain
against the CPU oracle, and the public interface.  No comparison here has a tolerance except the oracle chain's."""
import numpy as np
import pytest
import torch

import pred_ref
import stream_probe as sp
import threshold_ref as tr
from test_gpu_clf_guide import clf  # noqa: F401  (the synthetic classifier)
from test_gpu_device_noise import eager, graph  # noqa: F401  (the two graph-mode fixtures, shared)
from test_gpu_inpaint import _blend, _hard_mask, _image, _ref_rows
from test_threshold_cpu import make_rows, same_bits

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
NPI = int(np.prod(CHW))
B, T = 3, 12
SEEDS = [11, (1 << 33) + 2, 0]
THR = (0.995, 2.0)          # the loops' setting: on the synthetic weights a 12-step run passes through s = max, s inside and (DDPM,
                            # DDIM) s = 1 -- chosen on the CPU oracle, asserted on every Python loop below
SB, SA = 0.6, 0.8
ROWS = {"ddpm": (SB, SA, 0.45, 0.5, 0.25), "ddim": (SB, SA, 0.9, 0.3, 0.25), "dpmsolver++": (SB, SA, 0.9, 0.3, 0.25, -0.1)}
N_CLASS, NULL, LABELS = 5, 4, [0, 3, 2]
CLASSES = ("MEL", "BCC", "AKIEC", "BKL")
TARGETS = [0, 2, 0]


def _view(t: torch.Tensor, offset: int) -> torch.Tensor:
    """t on the GPU, its base pointer ``offset`` floats off a 16-byte line"""
    flat = torch.cat([torch.zeros(offset), t.reshape(-1), torch.zeros(4)]).to(DEV)[offset:offset + t.numel()]
    assert flat.data_ptr() % 16 == 4 * offset
    return flat.reshape(t.shape)


# ---- 1. the selection kernel alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,n,offset", [(3, 192, 0), (2, 105, 1), (5, 1, 0), (2, 3 * 32 * 32, 0), (1, 3 * 128 * 128, 0),
                                         (1, 3 * 128 * 128 + 4, 0)])       # (the last: past the register-resident form)
@pytest.mark.parametrize("ptype", pred_ref.TYPES)
def test_x0_threshold_is_the_restatement(Bn, n, offset, ptype):
    from synt_isic_amd import ops
    g = torch.Generator().manual_seed(7 * n + Bn)
    o, x = torch.randn((Bn, n), generator=g) * 1.6, torch.randn((Bn, n), generator=g) * 1.6
    od, xd = _view(o, offset), _view(x, offset)
    want_x0 = pred_ref.raw_x0(o, x, torch.tensor(SB), torch.tensor(SA), ptype)
    seen = set()
    for ratio in (0.0, 0.5, 0.995, 1.0):
        for max_value in (1.0, 2.5, 100.0):
            want = tr.threshold_s(want_x0, ratio, max_value)
            got = ops.x0_threshold(od, xd, SB, SA, ratio, max_value, prediction_type=ptype)
            assert got.shape == (Bn,) and same_bits(got.cpu(), want), (ratio, max_value, got.cpu(), want)
            assert torch.equal(got, ops.x0_threshold(od, xd, SB, SA, ratio, max_value, prediction_type=ptype))   # two calls
            seen |= {"one" if v == 1.0 else "max" if v == max_value else "inside" for v in want.tolist()}
    assert n == 1 or seen == {"one", "inside", "max"}


@pytest.mark.parametrize("n,offset", [(192, 0), (105, 1), (3 * 32 * 32, 0)])
def test_x0_threshold_on_ties_equal_rows_infinities_and_nan(n, offset):
    """sample prediction makes x0 the model output itself: the rows of the CPU list reach the kernel as they are.  One NaN image
    leaves the other images' s untouched."""
    from synt_isic_amd import ops
    rows = make_rows(n)
    x = torch.zeros_like(rows)
    od, xd = _view(rows, offset), _view(x, offset)
    for ratio in (0.0, 0.5, 0.9, 0.995, 0.999, 1.0):
        want = tr.threshold_s(rows, ratio, 2.5)
        _, torch_s = tr.torch_threshold(rows, ratio, 2.5)
        got = ops.x0_threshold(od, xd, SB, SA, ratio, 2.5, prediction_type="sample").cpu()
        assert same_bits(got, want) and same_bits(got, torch_s), (ratio, got, want)
        assert torch.isnan(got[5]) and torch.isfinite(got[:4]).all()
        without = ops.x0_threshold(od[:5].contiguous(), xd[:5].contiguous(), SB, SA, ratio, 2.5, prediction_type="sample").cpu()
        assert same_bits(without, got[:5])


@pytest.mark.parametrize("n,offset", [(192, 0), (105, 1)])
def test_x0_threshold_under_the_two_guidances(n, offset):
    from synt_isic_amd import ops
    g = torch.Generator().manual_seed(n)
    ec, eu, x, gr = (torch.randn((B, n), generator=g) * 1.3 for _ in range(4))
    ecd, eud, xd, grd = (_view(t, offset) for t in (ec, eu, x, gr))
    sb, sa = torch.tensor(SB), torch.tensor(SA)
    for ptype in pred_ref.TYPES:
        w = torch.tensor(3.0)
        combined = eu + w * (ec - eu)
        want = tr.threshold_s(pred_ref.raw_x0(combined, x, sb, sa, ptype), 0.995, 4.0)
        got = ops.x0_threshold(ecd, xd, SB, SA, 0.995, 4.0, prediction_type=ptype, eps_u=eud, guidance_scale=3.0)
        assert same_bits(got.cpu(), want)
        assert same_bits(got.cpu(), ops.x0_threshold(ops.guide_eps(ecd, eud, 3.0), xd, SB, SA, 0.995, 4.0, prediction_type=ptype).cpu())
    k = torch.tensor(2.5) * sb
    want = tr.threshold_s(pred_ref.raw_x0(ec - k * gr, x, sb, sa, "epsilon"), 0.995, 4.0)
    got = ops.x0_threshold(ecd, xd, SB, SA, 0.995, 4.0, grad=grd, classifier_scale=2.5)
    assert same_bits(got.cpu(), want)
    assert same_bits(got.cpu(), ops.x0_threshold(ops.clf_guide_eps(ecd, grd, SB, 2.5), xd, SB, SA, 0.995, 4.0).cpu())


# ---- 2. one step per rule ---------------------------------------------------------------------------------------------------
STEP_THR = (0.995, 8.0)
RULE_CASES = [("ddpm", False), ("ddim", False), ("ddim", True), ("dpmsolver++", False)]


def _regime_batch(n: int, seed: int):
    """(o, x, z, hist) [3, n] on the host: image 0 small (s clamps to 1), image 1 ordinary (s inside), image 2 large (s = max)"""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.2, 1.0, 6.0]).reshape(3, 1)
    o, x, z, hist = (torch.randn((3, n), generator=g) for _ in range(4))
    return o * scale, x * scale, z, hist


def _ops_step(rule, clipped, o, x, z, hist, threshold, ptype, out=None, clip=1.0):
    from synt_isic_amd import ops
    if rule == "ddpm":
        return ops.ddpm_step(o, x, z, ROWS[rule], clip, out=out, prediction_type=ptype, threshold=threshold)
    if rule == "ddim":
        return ops.ddim_step(o, x, z, ROWS[rule], clip, clipped, out=out, prediction_type=ptype, threshold=threshold)
    return ops.dpmpp_step(o, x, z, hist, ROWS[rule], clip, out=out, prediction_type=ptype, threshold=threshold)


def _ops_step_rng(rule, clipped, o, x, seeds, step, hist, threshold, ptype, out=None):
    from synt_isic_amd import ops
    if rule == "ddpm":
        return ops.ddpm_step_rng(o, x, seeds, step, ROWS[rule], 1.0, out=out, prediction_type=ptype, threshold=threshold)
    if rule == "ddim":
        return ops.ddim_step_rng(o, x, seeds, step, ROWS[rule], 1.0, clipped, out=out, prediction_type=ptype, threshold=threshold)
    return ops.dpmpp_step_rng(o, x, seeds, step, hist, ROWS[rule], 1.0, out=out, prediction_type=ptype, threshold=threshold)


@pytest.mark.parametrize("rule,clipped", RULE_CASES)
@pytest.mark.parametrize("ptype", pred_ref.TYPES)
@pytest.mark.parametrize("n,offset", [(NPI, 0), (105, 0), (105, 1)])
def test_one_step_is_the_restatement(rule, clipped, ptype, n, offset):
    from synt_isic_amd import ops
    host = _regime_batch(n, seed=n + offset)
    o, x, z, hist = host
    want, want_hist, s = tr.step_row(rule, o, x, z, hist, ROWS[rule], STEP_THR, ptype, clipped)
    assert s[0] == 1.0 and 1.0 < s[1] < STEP_THR[1] and s[2] == STEP_THR[1], s          # the three regimes
    assert torch.isfinite(want).all()
    od, xd, zd, hd = (_view(t, offset) for t in host)
    got = _ops_step(rule, clipped, od, xd, zd, hd, STEP_THR, ptype)
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    assert want_hist is None or torch.equal(hd.cpu(), want_hist)                        # the history is x0'
    # the static clamp is not read under thresholding, and thresholding is not the static clamp
    assert torch.equal(_ops_step(rule, clipped, od, xd, zd, _view(hist, offset), STEP_THR, ptype, clip=0.0), got)
    assert not torch.equal(_ops_step(rule, clipped, od, xd, zd, _view(hist, offset), None, ptype), got)
    # in place
    xi, hi = _view(x, offset), _view(hist, offset)
    _ops_step(rule, clipped, od, xi, zd, hi, STEP_THR, ptype, out=xi)
    assert torch.equal(xi.cpu(), want) and (want_hist is None or torch.equal(hi.cpu(), want_hist))
    # sample_max_value = 1 is the static clip = 1
    one = _ops_step(rule, clipped, od, xd, zd, _view(hist, offset), (0.995, 1.0), ptype)
    assert torch.equal(one, _ops_step(rule, clipped, od, xd, zd, _view(hist, offset), None, ptype, clip=1.0))
    # the device-noise form equals the buffer form fed by noise_fill
    seeds, step = [4, (1 << 35) + 6, 0x7FFFFFFF], 17
    zf = ops.noise_fill(seeds, n, step)
    ha, hb = _view(hist, offset), _view(hist, offset)
    buf = _ops_step(rule, clipped, od, xd, zf, ha, STEP_THR, ptype)
    rng = _ops_step_rng(rule, clipped, od, xd, seeds, step, hb, STEP_THR, ptype)
    assert torch.equal(rng, buf) and torch.equal(ha, hb) and not torch.equal(rng, got)


@pytest.mark.parametrize("rule,clipped", RULE_CASES)
def test_the_edit_epilogue_composes(rule, clipped):
    """a thresholded edited step is the thresholded step followed by the restated blend"""
    from synt_isic_amd import ops
    o, x, _, hist = _regime_batch(NPI, seed=3)
    od, xd = (t.reshape((3,) + CHW).to(DEV) for t in (o, x))
    seeds, step, erow = [4, 5, 6], 9, (0.7, 0.5, 0.9, 0.3)
    image, mask = _image(), _hard_mask()
    ha, hb = hist.to(DEV), hist.to(DEV)
    u = _ops_step_rng(rule, clipped, od, xd, seeds, step, ha, STEP_THR, "epsilon")
    want = _blend(u, image, mask, seeds, step, erow)
    if rule == "ddpm":
        got = ops.ddpm_step_edit(od, xd, seeds, step, ROWS[rule], image, mask, erow, threshold=STEP_THR)
    elif rule == "ddim":
        got = ops.ddim_step_edit(od, xd, seeds, step, ROWS[rule], image, mask, erow, use_clipped_model_output=clipped, threshold=STEP_THR)
    else:
        got = ops.dpmpp_step_edit(od, xd, seeds, step, hb, ROWS[rule], image, mask, (0.7, 0.5, 1.0, 0.0), threshold=STEP_THR)
        want = _blend(u, image, mask, seeds, step, (0.7, 0.5, 1.0, 0.0))
        assert torch.equal(ha, hb)
    assert torch.equal(got, want)


# ---- 3. the mirrors ---------------------------------------------------------------------------------------------------------
def _sched(rule, threshold=THR, Tn=T, **kw):
    """a mirror under ``threshold``: the DDPM mirror through its constructor, the other two through set_thresholding (their
    constructors keep refusing the arguments)"""
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    if rule == "ddpm":
        if threshold is not None:
            kw.update(thresholding=True, dynamic_thresholding_ratio=threshold[0], sample_max_value=threshold[1])
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", **kw)
    elif rule == "ddim":
        s = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", **kw)
    else:
        kw.setdefault("clip_sample", True)
        s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", timestep_spacing="leading", **kw)
    if threshold is not None and rule != "ddpm":
        s.set_thresholding(True, dynamic_thresholding_ratio=threshold[0], sample_max_value=threshold[1])
    s.set_timesteps(Tn)
    return s


def _table(sched, eta=0.0):
    return sched.rule_table(eta)[1]


@pytest.mark.parametrize("rule,clipped", RULE_CASES)
@pytest.mark.parametrize("ptype", pred_ref.TYPES)
def test_mirror_step_is_the_restatement(rule, clipped, ptype):
    """two steps of a mirror built with the published arguments (the second one uses DPM-Solver++'s history)"""
    host = _regime_batch(NPI, seed=41)
    o, x, z, _ = host
    sched, clip_sched = _sched(rule, STEP_THR, 5), _sched(rule, None, 5, clip_sample=True)
    one_sched = _sched(rule, (0.995, 1.0), 5)
    eta = 0.5 if rule == "ddim" else 0.0
    tab = _table(sched, eta)
    kw = dict(eta=eta, use_clipped_model_output=clipped) if rule == "ddim" else {}
    xs = {k: x.to(DEV) for k in ("thr", "clip", "one")}
    want, hist = x, None
    for i in (0, 1):
        t = sched.timesteps[i]
        row = tuple(float(v) for v in (tab[i] if rule != "dpmsolver++" or i else sched._rows(1)[0]))
        want, hist, _ = tr.step_row(rule, o, want, z, hist, row, STEP_THR, ptype, clipped)
        for k, sc in (("thr", sched), ("clip", clip_sched), ("one", one_sched)):
            xs[k] = sc.step(o.to(DEV), t, xs[k], variance_noise=z.to(DEV), prediction_type=ptype, **kw).prev_sample
        assert torch.equal(xs["thr"].cpu(), want), (i, float((xs["thr"].cpu() - want).abs().max()))
        assert torch.equal(xs["one"], xs["clip"]) and not torch.equal(xs["thr"], xs["clip"])


# ---- 4. the loops -----------------------------------------------------------------------------------------------------------
def _x_T(seeds, chw=CHW):
    return torch.stack([torch.randn(chw, generator=torch.Generator().manual_seed(2000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _python_loop(model, sched, eta, x_T, seeds, *, labels=None, w=1.0, classifier=None, scale=0.0, edit=None, threshold=THR):
    """image_generator.py:395-403 over the drop-in objects: the model, the existing guidance ops, the mirror's step fed by
    noise_fill, the restated blend of an edit.  Returns (every frame, the record of s [T, B] from the restatement)."""
    from synt_isic_amd import ops
    sched.set_timesteps(sched.timesteps.numel())
    tab = _table(sched, eta)
    kw = dict(eta=eta) if sched.rule == "ddim" else {}
    rows = _ref_rows(sched, [(i, 0) for i in range(tab.shape[0])]) if edit is not None else None
    x, frames, record = x_T.clone(), [], []
    for i, t in enumerate(sched.timesteps):
        if labels is None:
            eps = model(x, t).sample
        else:
            eps = model(x, t, class_labels=labels).sample
            if w != 1.0:
                eps = ops.guide_eps(eps, model(x, t, class_labels=[NULL] * len(labels)).sample, w)
        if classifier is not None:
            g, _ = classifier.input_gradient(x, list(TARGETS))
            eps = ops.clf_guide_eps(eps, g, float(tab[i, 0]), scale)
        if threshold is not None:
            x0 = pred_ref.raw_x0(eps.cpu(), x.cpu(), tab[i, 0], tab[i, 1], "epsilon")
            record.append(tr.threshold_s(x0, *threshold))
        vn = ops.noise_fill(seeds, NPI, i).reshape(x.shape) if float(tab[i, 4]) != 0.0 else None
        x = sched.step(eps, t, x, variance_noise=vn, **kw).prev_sample
        if edit is not None:
            x = _blend(x, edit[0], edit[1], seeds, i, rows[i])
        frames.append(x)
    return torch.stack(frames), (torch.stack(record) if record else None)


def _regimes(record, max_value=THR[1]):
    return {"one" if v == 1.0 else "max" if v == max_value else "inside" for v in record.reshape(-1).tolist()}


@pytest.mark.parametrize("rule", ["ddpm", "ddim", "dpmsolver++"])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_fused_loop_equals_python_loop(mode, rule, eager, graph):
    """B = 3, 32x32, T = 12, every frame.  The record of s must hold s = 1, s inside (1, max) and s = max.  DDPM and DDIM do
    (image 0: nine steps at 2.000, then 1.677, 1.271, 1.000 under DDPM).  DPM-Solver++ on the synthetic weights does NOT reach
    s = 1: its record ends 1.905, 1.463, 1.020 on the GPU as on the CPU oracle, and stayed above 1 at the last step for every
    ratio from 0.3 to 0.995, sample_max_value from 1.2 to 2 and output-convolution scale from 0.5 to 2.5 tried on the oracle
    (1.001 .. 1.020): the multistep update keeps the quantile of the next x0 just above the 1 it normalised the last one to.
    For that rule the test asserts the two regimes that occur; test_regimes_all_occur_across_the_rules asserts the union, and
    s = 1 under DPM-Solver++'s kernels is covered by test_max_one_is_the_clip_sample_loop and the one-step tests.  Every other
    loop test below (guided, classifier-guided, inpainting) runs under a rule that reaches all three and asserts them."""
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    s = eager if mode == "eager" else graph
    model, x_T = s.models["NV"], _x_T(SEEDS)
    sched, eta = _sched(rule), (0.5 if rule == "ddim" else 0.0)
    frames, record = _python_loop(model, sched, eta, x_T, SEEDS)
    print(f"{rule}: s per step (image 0) = {[f'{v:.3f}' for v in record[:, 0].tolist()]}")
    assert _regimes(record) >= ({"inside", "max"} if rule == "dpmsolver++" else {"one", "inside", "max"})
    res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta)
    assert res.steps_done == T and res.thresholding == THR
    assert torch.equal(res.trajectory, frames) and torch.equal(res.latents, frames[-1])
    # the arguments override what the scheduler object was built with, in both directions
    plain = _sched(rule, None)
    again = run_sampling_loop(model, plain, x_T, DeviceNoise(SEEDS), eta=eta, thresholding=True,
                              dynamic_thresholding_ratio=THR[0], sample_max_value=THR[1])
    assert torch.equal(again.latents, res.latents) and again.thresholding == THR
    off = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), eta=eta, thresholding=False)
    ref = run_sampling_loop(model, plain, x_T, DeviceNoise(SEEDS), eta=eta)
    assert torch.equal(off.latents, ref.latents) and off.thresholding is None and not torch.equal(off.latents, res.latents)
    if rule == "ddpm":
        # host noise: the buffer of the same rows
        from synt_isic_amd import ops
        z = torch.stack([ops.noise_fill(SEEDS, NPI, i).reshape((B,) + CHW) for i in range(T - 1)])
        assert torch.equal(run_sampling_loop(model, sched, x_T, z, eta=eta).latents, res.latents)


def test_regimes_all_occur_across_the_rules(eager):
    """the union of the three plain records holds s = 1, s inside (1, max) and s = max"""
    model, x_T, seen = eager.models["NV"], _x_T(SEEDS), set()
    for rule in ("ddpm", "ddim", "dpmsolver++"):
        seen |= _regimes(_python_loop(model, _sched(rule), 0.0, x_T, SEEDS)[1])
    assert seen == {"one", "inside", "max"}


@pytest.fixture(scope="module")
def cond_sd():
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return synthetic_unet_state_dict(num_class_embeds=N_CLASS)


@pytest.fixture(scope="module")
def csamplers(eager, graph, cond_sd):
    eager.add_conditional_model(CLASSES, cond_sd).set_graph_mode(0)
    graph.add_conditional_model(CLASSES, cond_sd).set_graph_mode(1)
    return {"eager": eager, "graph": graph}


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_guided_loop_equals_python_loop(mode, csamplers):
    """classifier-free guidance at scale 3: s [B] from the combined eps, the step writes both halves"""
    from synt_isic_amd.sampler import DeviceNoise, Guidance, run_sampling_loop
    model, x_T = csamplers[mode].models["MEL"], _x_T(SEEDS)
    sched = _sched("ddpm")
    frames, record = _python_loop(model, sched, 0.0, x_T, SEEDS, labels=LABELS, w=3.0)
    assert _regimes(record) == {"one", "inside", "max"}
    res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, guidance=Guidance(LABELS, NULL, 3.0))
    assert torch.equal(res.trajectory, frames) and res.thresholding == THR


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_classifier_guided_loop_equals_python_loop(mode, eager, graph, clf):
    """under DDIM at eta = 0.5 (x_T halved, so that the classifier's clamp lets a gradient through): the record holds all three
    regimes, so the thresholded classifier-eps step kernel runs at s = 1, inside and at the maximum"""
    from synt_isic_amd.sampler import ClassifierGuidance, DeviceNoise, run_sampling_loop
    model, x_T = (eager if mode == "eager" else graph).models["NV"], 0.5 * _x_T(SEEDS)
    sched, eta = _sched("ddim"), 0.5
    frames, record = _python_loop(model, sched, eta, x_T, SEEDS, classifier=clf, scale=2.5)
    assert _regimes(record) == {"one", "inside", "max"}
    res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta,
                            classifier=ClassifierGuidance(clf, TARGETS, 2.5))
    assert torch.equal(res.trajectory, frames) and res.classifier_passes == T and res.thresholding == THR
    plain, _ = _python_loop(model, sched, eta, x_T, SEEDS)
    assert not torch.equal(plain, frames)                               # the guidance reaches the result


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_inpainting_loop_equals_python_loop(mode, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    model, x_T = (eager if mode == "eager" else graph).models["NV"], _x_T(SEEDS)
    sched, image, mask = _sched("ddim"), _image(), _hard_mask()
    frames, record = _python_loop(model, sched, 0.5, x_T, SEEDS, edit=(image, mask))
    assert _regimes(record) == {"one", "inside", "max"}
    res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=0.5, edit=Edit(image, mask, None))
    assert torch.equal(res.trajectory, frames) and res.thresholding == THR


# ---- 5. handle and graph state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["ddpm", "dpmsolver++"])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_max_one_is_the_clip_sample_loop(mode, rule, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    model, x_T = (eager if mode == "eager" else graph).models["NV"], _x_T(SEEDS)
    one = run_sampling_loop(model, _sched(rule, (0.995, 1.0)), x_T, DeviceNoise(SEEDS), return_trajectory=True)
    clip = run_sampling_loop(model, _sched(rule, None, clip_sample=True), x_T, DeviceNoise(SEEDS), return_trajectory=True)
    assert torch.equal(one.trajectory, clip.trajectory) and torch.equal(one.images, clip.images)


def test_on_off_on_equals_fresh_handles(graph, synthetic_sd):
    """the captured step's key holds the setting: on -> off -> on on one handle re-captures and never replays the other chain"""
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import DeviceNoise, Sampler, run_sampling_loop
    lib = _lib.load()
    model, x_T = graph.models["NV"], _x_T(SEEDS)
    on_s, off_s, other = _sched("ddim"), _sched("ddim", None), _sched("ddim", (0.9, 3.0))

    def fresh(sched):
        s = Sampler(DEV)
        s.add_model("NV", synthetic_sd).set_graph_mode(1)
        return run_sampling_loop(s.models["NV"], sched, x_T, DeviceNoise(SEEDS)).latents

    want_on, want_off, want_other = fresh(on_s), fresh(off_s), fresh(other)
    assert not torch.equal(want_on, want_off) and not torch.equal(want_on, want_other)
    a = run_sampling_loop(model, on_s, x_T, DeviceNoise(SEEDS)).latents
    builds = lib.sisic_unet_graph_builds(model.handle)
    b = run_sampling_loop(model, on_s, x_T, DeviceNoise(SEEDS)).latents          # two runs on one handle: replayed, bit-equal
    assert lib.sisic_unet_graph_builds(model.handle) == builds and torch.equal(a, b) and torch.equal(a, want_on)
    c = run_sampling_loop(model, off_s, x_T, DeviceNoise(SEEDS)).latents
    assert lib.sisic_unet_graph_builds(model.handle) == builds + 1 and torch.equal(c, want_off)
    d = run_sampling_loop(model, on_s, x_T, DeviceNoise(SEEDS)).latents
    assert lib.sisic_unet_graph_builds(model.handle) == builds + 2 and torch.equal(d, want_on)
    e = run_sampling_loop(model, other, x_T, DeviceNoise(SEEDS)).latents         # another (ratio, max) is another step too
    assert lib.sisic_unet_graph_builds(model.handle) == builds + 3 and torch.equal(e, want_other)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_two_runs_on_one_handle_are_bit_equal(mode, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    model, sched = (eager if mode == "eager" else graph).models["NV"], _sched("dpmsolver++")
    a = run_sampling_loop(model, sched, _x_T([1, 2, 3]), DeviceNoise([1, 2, 3]), return_trajectory=True)
    b = run_sampling_loop(model, sched, _x_T([4, 5, 6]), DeviceNoise([4, 5, 6]))
    c = run_sampling_loop(model, sched, _x_T([1, 2, 3]), DeviceNoise([1, 2, 3]), return_trajectory=True)
    assert torch.equal(a.trajectory, c.trajectory) and not torch.equal(a.latents, b.latents)


def test_side_stream_gives_the_default_stream_bits(graph):
    """one thresholded graph run on a side stream that a spin kernel holds, the latents copied in behind the hold"""
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    gm, sched = graph.models["NV"], _sched("ddpm")

    def fn(x):
        r = run_sampling_loop(gm, sched, x, DeviceNoise(SEEDS), return_trajectory=True)
        return r.latents, r.trajectory, r.images

    baseline, held, _ = sp.run_held(fn, lambda: [_x_T(SEEDS)], lambda: [_x_T([5, 6, 7])], "thresholded graph loop")
    assert sp.same(baseline, held)


def test_latency_mode_loop_equals_python_loop(synthetic_sd):
    """batch 1 in latency mode (graph-replayed by default): the quantile launch is a node of that chain too"""
    from synt_isic_amd.sampler import DeviceNoise, Sampler, run_sampling_loop
    s = Sampler(DEV, latency_mode=True)
    model = s.add_model("NV", synthetic_sd)
    sched, x_T = _sched("dpmsolver++", Tn=6), _x_T(SEEDS[:1])
    frames, _ = _python_loop(model, sched, 0.0, x_T, SEEDS[:1])
    res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS[:1]), return_trajectory=True)
    assert torch.equal(res.trajectory, frames)


# ---- 6. the chain against the oracle ----------------------------------------------------------------------------------------
def test_chain_against_the_oracle(eager, synthetic_sd):
    """T = 8, two seeds, DPM-Solver++ on the "leading" grid under thresholding: oracle.unet.unet_forward and the restated step
    on the CPU.  The bar is 1e-3 max-abs, the one tests/test_gpu_dpmpp.py::test_chain_against_the_oracle holds its unthresholded
    chain to.  x0 -> x0' at most doubles a perturbation (clamp is 1-Lipschitz, s >= 1, and s itself moves by at most the
    perturbation)."""
    from oracle import unet as ounet
    from synt_isic_amd.sampler import draw_noise, run_sampling_loop
    model = eager.models["NV"]
    x_T, _ = draw_noise([3, 4], 0, CHW)
    dists = {}
    for name, threshold in (("thresholded", THR), ("unthresholded", None)):
        sched = _sched("dpmsolver++", threshold, 8)
        assert int(sched.timesteps[0]) == 875
        tab = sched.coefficient_table()
        res = run_sampling_loop(model, sched, x_T.to(DEV), None, return_trajectory=True)
        x, hist, worst = x_T, None, 0.0
        for i, t in enumerate(sched.timesteps):
            with torch.no_grad():
                eps = ounet.unet_forward(synthetic_sd, x, t)
            row = tuple(float(v) for v in tab[i])
            if threshold is not None:
                x, hist, _ = tr.step_row("dpmsolver++", eps, x, None, hist, row, threshold)
            else:
                x, hist = pred_ref.dpmpp_step_row(eps, x, None, hist, row, 1.0)
            worst = max(worst, float((res.trajectory[i].cpu() - x).abs().max()))
        dists[name] = worst
    print(f"max |x - oracle chain| over 8 steps: {dists}")
    assert dists["thresholded"] <= 1e-3 and dists["unthresholded"] <= 1e-3


# ---- 7. the public interface and the refusals -------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["host", "device"])
def test_generate_with_thresholding(noise, eager, synthetic_sd):
    import synt_isic_amd.sampler as S
    kw = dict(size=(32, 32), noise=noise, scheduler="ddim", eta=0.5, thresholding=True, sample_max_value=2.0)
    imgs, traj = eager.generate(3, "NV", 8, count=2, **kw)
    res = eager.generate_seeds("NV", [3, 4], 8, (32, 32), **{k: v for k, v in kw.items() if k != "size"})
    assert res.thresholding == (0.995, 2.0) and res.steps_done == 8 and traj is None
    assert np.array_equal(imgs, res.images.cpu().numpy())
    off = eager.generate_seeds("NV", [3, 4], 8, (32, 32), noise=noise, scheduler="ddim", eta=0.5)
    assert off.thresholding is None and not torch.equal(off.latents, res.latents)              # nothing leaks into the next call
    assert torch.equal(off.latents, eager.generate_seeds("NV", [3, 4], 8, (32, 32), noise=noise, scheduler="ddim", eta=0.5,
                                                         thresholding=False, sample_max_value=2.0).latents)
    one = eager.generate_images("NV", [4], 8, size=(32, 32), noise=noise, scheduler="ddim", eta=0.5, thresholding=True,
                                sample_max_value=2.0)
    assert torch.equal(one.latents[0], res.latents[1])                                         # an image depends on its seed alone
    old = S._default_sampler
    try:
        S._default_sampler = S.Sampler(DEV)
        S._default_sampler.add_model("NV", synthetic_sd)
        mod, _ = S.generate(3, "NV", 8, count=2, **kw)
        assert np.array_equal(mod, imgs)
    finally:
        S._default_sampler = old


def test_refusals(eager):
    import ctypes as C
    from synt_isic_amd import _lib, ops
    lib = _lib.load()
    for bad in (dict(dynamic_thresholding_ratio=1.5), dict(dynamic_thresholding_ratio=-0.5), dict(sample_max_value=0.5),
                dict(sample_max_value=float("nan")), dict(dynamic_thresholding_ratio=float("inf"))):
        with pytest.raises(ValueError):
            eager.generate(3, "NV", 4, size=(32, 32), thresholding=True, **bad)
    # the library's own: SISIC_EINVAL, the previous setting left in force
    model, ctx = eager.models["NV"], ops.context(torch.device(DEV))
    x = torch.randn((2, 105), generator=torch.Generator().manual_seed(1)).to(DEV) * 3
    o = torch.zeros_like(x)
    for setter, handle in ((lib.sisic_unet_set_thresholding, model.handle), (lib.sisic_set_step_thresholding, ctx)):
        assert setter(handle, 0.9, 2.0) == 0
        for ratio, max_value in ((1.5, 2.0), (-0.1, 2.0), (float("nan"), 2.0), (0.9, 0.5), (0.9, float("inf")), (0.9, float("nan"))):
            assert setter(handle, ratio, max_value) == _lib.SISIC_EINVAL
    try:
        # the context still thresholds at (0.9, 2.0): a sample-prediction step on x0 = o would need another context, so look at
        # the epsilon step with eps = 0, sb irrelevant: x0 = x / sa
        assert lib.sisic_set_step_image_elems(ctx, 105) == 0
        got = ops.ddpm_step(o, x, None, (0.6, 0.8, 1.0, 0.0, 0.0))
        want, _, s = tr.step_row("ddpm", o.cpu(), x.cpu(), None, None, (0.6, 0.8, 1.0, 0.0, 0.0), (0.9, 2.0))
        assert torch.equal(got.cpu(), want) and (s > 1.0).all()
        # a buffer-noise entry that is not told its images refuses while thresholding is on
        assert lib.sisic_set_step_image_elems(ctx, 0) == 0
        with pytest.raises(_lib.SisicError, match="whole images"):
            ops.ddpm_step(o, x, None, (0.6, 0.8, 1.0, 0.0, 0.0))
    finally:
        assert lib.sisic_set_step_thresholding(ctx, 0.0, 1.0) == 0 and lib.sisic_unet_set_thresholding(model.handle, 0.0, 1.0) == 0
    assert torch.equal(ops.ddpm_step(o, x, None, (0.6, 0.8, 1.0, 0.0, 0.0), 0.0).cpu(), x.cpu() / torch.tensor(0.8))
    with pytest.raises(ValueError):
        ops.ddpm_step(o, x, None, (0.6, 0.8, 1.0, 0.0, 0.0), threshold=(1.5, 2.0))
    with pytest.raises(ValueError):
        ops.x0_threshold(o, x, 0.6, 0.8, 0.9, 0.5)
    # s may alias nothing the launch reads
    for alias in (o, x):
        a = _lib.X0ThresholdArgs(eps=o.data_ptr(), eps2=None, x=x.data_ptr(), s=alias.data_ptr() + 8, stream=None, n_per_image=105,
                                 B=2, source=0, sb=0.6, sa=0.8, w=1.0, ratio=0.9, sample_max_value=2.0, reserved=0.0)
        assert lib.sisic_x0_threshold(ctx, C.byref(a)) == _lib.SISIC_EINVAL and b"aliases" in lib.sisic_last_error()
    free = torch.zeros(2, device=DEV)
    a = _lib.X0ThresholdArgs(eps=o.data_ptr(), eps2=None, x=x.data_ptr(), s=free.data_ptr(), stream=None, n_per_image=(1 << 24) + 1,
                             B=1, source=0, sb=0.6, sa=0.8, w=1.0, ratio=0.9, sample_max_value=2.0, reserved=0.0)
    assert lib.sisic_x0_threshold(ctx, C.byref(a)) == _lib.SISIC_EINVAL and b"2^24" in lib.sisic_last_error()
    torch.cuda.synchronize()
    assert (free == 0).all()                                                   # refused before anything was launched
