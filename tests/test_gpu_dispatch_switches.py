"""The executors on the FALLBACK kernels of the dispatch switches (conv_plan.cpp's nine, and SISIC_WINOGRAD), held to float64.

README and INTEGRATION offer the switches as the way back to the f32-MFMA kernels.  With one off, the producer of nearly every
tensor the executor normalises is another kernel: another count of GroupNorm partial slots, it finalises the consumer's
(scale, shift) or it does not, it carries a rider or it does not.  test_conv_plan_cpu.py pins what the plan PROMISES; this file
checks that the kernels DELIVER it: the UNet forward (default and latency mode), its training step, the sampling loop (eager
and captured) and the classifier's five routes, once per set of switches, each in a fresh interpreter (tests/switch_exec.py: the
switches are read once per process), one child at a time.

Every result is held to the project's own bar against a float64 CPU reference (FWD_GUARD, PRED_TOL, GRAD_REL_WORST / _MEDIAN,
the classifier's rules), lies within twice that bar of the default child's, has no unwritten element and an intact guard band
(tests/poison.py, installed in the child); second backward == first, tape forward == eval forward, batch of one == row 0, the
captured sampler's two calls agree; and the child's own record of plans differs from the default child's by exactly the
transitions test_dispatch_switches_cpu.py pins (for SISIC_WINOGRAD=0, which shows in no plan: zero launches in the Winograd profile
slots).  SISIC_POINTWISE_STAGED_KSPLIT=0, whose comment promises the same bits, is held to equality, at 64x64x64 as well.

What torch fp32 itself reaches against float64 on these inputs (CPU, 2x64x64 / 3x40x56): prediction 2.1e-6 / 2.7e-6, worst
gradient tensor 1.1e-5 / 1.5e-5, median 4.5e-6 / 4.6e-6 -- a factor 7 - 24 inside the bars, which so leave room for an honest f32
path and none for a wrong one (a stale GroupNorm pair moves the prediction by >= 142 x PRED_TOL: test_dispatch_switches_cpu.py).
Measured on MI355X, every error and its bar: profiles/r30/dispatch_switches.txt.

A child that ends by a signal, an abort or at its time limit fails its case and every later one without starting a process.
"""
import json
import os
import subprocess
import sys
from collections import Counter, OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arch_ref
import clf_bn_ref
import clf_train_ref
import switch_exec as sx
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)
from test_gpu_classifier import STRICT_TOL
from test_gpu_train import GRAD_REL_MEDIAN, GRAD_REL_WORST, PRED_TOL
from test_gpu_unet import FWD_GUARD, FWD_TOL

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-5                 # * max(1, |ref|)
LOGITS_TOL = 2e-4               # * max(1, |ref|): test_gpu_classifier.py
IG_COSINE = 0.999               # test_input_gradient_matches_autograd_of_the_oracle
CAM_TOL = 2e-3                  # test_grad_cam_matches_oracle
VANISH_FLOOR, VANISH_FACTOR = 1e-7, 10.0                # test_gpu_architectures.py
# one child at the default set (the 64x64x64 forward included), measured on MI355X: interpreter start-up, import and 1.8 s of
# workload -- 3.7 .. 4.8 s over four runs (profiles/r30/dispatch_switches.txt); the time limit of a child is five times that
CHILD_SECONDS_MEASURED = 4.8
CHILD_TIMEOUT = 5 * CHILD_SECONDS_MEASURED

FAULT_TEXT = ("illegal memory access", "HSA_STATUS_ERROR", "Memory access fault", "hipErrorLaunchFailure")
_STOP = {"why": None}           # set by a child that faulted, aborted or hung: nothing more goes to the GPU


def _log(err, bar, what):
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(f"{err:.3e}\t{bar:.3e}\t{what}\n")


class Checks:
    """Every comparison of a case is logged before any fails it.  Comparisons of one ``group`` (the 62 gradients of a classifier
    call, the frames of a trajectory) are each held to their own bar and logged as one line: the member with the largest error
    over bar, and how many there were."""

    def __init__(self, label):
        self.label, self.failed, self.groups = label, [], OrderedDict()

    def le(self, err, bar, what, group=None):
        if group is None:
            _log(err, bar, f"switches [{self.label}] {what}")
        else:
            self.groups.setdefault(group, []).append((err / bar if bar > 0 else float("inf"), err, bar, what))
        if not err <= bar:
            self.failed.append(f"{what}: {err:.3e} > {bar:.3e}")

    def flush(self):
        for group, rows in self.groups.items():
            _, err, bar, what = max(rows, key=lambda r: (r[0] != r[0], r[0]))          # (a NaN ranks first)
            _log(err, bar, f"switches [{self.label}] {group}: the largest error over bar of {len(rows)} -- {what}")
        self.groups = OrderedDict()

    def true(self, cond, what):
        if not cond:
            self.failed.append(what)

    def done(self):
        self.flush()
        assert not self.failed, f"[{self.label}] " + "; ".join(self.failed)


# ---------------------------------------------------------------- children
def _run_child(name, outdir):
    """the workload in a fresh interpreter with the set's environment; {file stem: array or JSON document}"""
    if _STOP["why"]:
        pytest.fail(f"not started: {_STOP['why']}")
    os.makedirs(outdir, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(sx.__file__), str(outdir)] + (["--b64"] if name in (None, sx.STAGED_SET) else [])
    label = name or "default"
    try:
        r = subprocess.run(cmd, env=sx.set_env(name), timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _STOP["why"] = f"the child of [{label}] was still running after {CHILD_TIMEOUT:.0f} s"
        pytest.fail(_STOP["why"])
    tail = f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or any(t in r.stderr for t in FAULT_TEXT):
        _STOP["why"] = f"the child of [{label}] ended by a signal, an abort or a GPU fault (exit {r.returncode})"
        pytest.fail(f"{_STOP['why']}\n{tail}")
    assert r.returncode == 0, f"[{label}] {tail}"
    out = {}
    for fn in sorted(os.listdir(outdir)):
        stem, ext = os.path.splitext(fn)
        if ext == ".npy":
            out[stem] = np.load(os.path.join(outdir, fn))
        elif ext == ".json":
            with open(os.path.join(outdir, fn)) as f:
                out[stem] = json.load(f)
    return out


@pytest.fixture(scope="module")
def default_child(tmp_path_factory):
    import time
    t0 = time.perf_counter()
    out = _run_child(None, tmp_path_factory.mktemp("switches_default"))
    _log(time.perf_counter() - t0, CHILD_TIMEOUT, "switches [default] seconds of the whole child (start-up, import, workload); its time limit")
    _log(out["seconds"]["workload"], CHILD_TIMEOUT, "switches [default] seconds of the workload alone")
    return out


# ---------------------------------------------------------------- float64 references, once, on the CPU
def _named(flat, names):
    out, at = OrderedDict(), 0
    for n, shape in names:
        k = int(np.prod(shape)) if shape else 1
        out[n] = torch.from_numpy(flat[at:at + k].reshape(shape))
        at += k
    assert at == flat.size
    return out


@pytest.fixture(scope="module")
def refs(synthetic_sd):
    from oracle import ddpm as oddpm, resnet18 as ores
    from synt_isic_amd.arch import UNetConfig
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    cfg, inp, r = UNetConfig(), sx.unet_inputs(), {}
    sd64 = {k: v.double() for k, v in synthetic_sd.items()}
    with torch.no_grad():
        r["b2_64"] = arch_ref.unet_forward(cfg, sd64, inp["x64"].double(), inp["t64"])
        r["b1_72x40"] = arch_ref.unet_forward(cfg, sd64, inp["x72"].double(), inp["t72"])
        r["b3_40x56"] = arch_ref.unet_forward(cfg, sd64, inp["x40"].double(), inp["t40"])
    for tag, key in (("b2_64", "train64"), ("b3_40x56", "train40")):
        images, noise, t = inp[key]
        noisy = oddpm.DDPMSchedulerOracle().add_noise(images, noise, t)
        loss, grads, pred = arch_ref.loss_and_grads(cfg, synthetic_sd, noisy, noise, t, dtype=torch.float64)
        _, g32, p32 = arch_ref.loss_and_grads(cfg, synthetic_sd, noisy, noise, t, dtype=torch.float32)
        # left out of the relative measure: exactly the tensors whose true gradient vanishes -- the six to_k.bias (softmax is
        # invariant to a shift of a row's scores), |g64| <= 2.3e-20 here
        vanishing = [n for n, g in grads.items() if g.abs().max().item() <= 1e-8]
        assert sorted(vanishing) == sorted(n for n in grads if n.endswith(".to_k.bias")) and len(vanishing) == 6, vanishing
        assert max(grads[n].abs().max().item() for n in vanishing) <= 1e-19
        w32, m32, own = arch_ref.grad_errors(g32, grads, vanishing)
        _log(w32[0], GRAD_REL_WORST, f"switches [reference] torch fp32 against float64, train {tag}: worst gradient tensor ({w32[1]})")
        _log(m32[0], GRAD_REL_MEDIAN, f"switches [reference] torch fp32 against float64, train {tag}: median gradient tensor")
        _log((p32.double() - pred).abs().max().item(), PRED_TOL, f"switches [reference] torch fp32 against float64, train {tag}: prediction")
        r["train_" + tag] = dict(noisy=noisy, loss=loss, grads=grads, pred=pred, vanishing=vanishing, own_vanishing=own)
    csd = synthetic_resnet18_state_dict()
    xc = sx.classifier_input()
    r["clf_sd"] = csd
    r["clf_logits"] = ores.classifier_forward(csd, xc)
    r["clf_ig"], r["clf_ig_logits"] = ores.score_input_gradient(csd, xc, sx.CLF_TARGET)
    r["clf_cam"] = ores.grad_cam(csd, xc, sx.CLF_TARGET)
    r["clf_cache"], r["ig_cache"] = {}, {}
    return r


def _clf_train_refs(refs, res):
    """the float64 and fp32 references of the two classifier training calls, routed by the child's own stem activation (as
    test_gpu_clf_train.py and test_gpu_clf_bn.py route theirs); computed once per distinct stem"""
    key = (res["clf_train_stem"].tobytes(), res["clf_bn_stem"].tobytes())
    if key not in refs["clf_cache"]:
        csd, out = refs["clf_sd"], {}
        x, labels, w = clf_train_ref.inputs(sx.CLF_TRAIN_CASE)
        stem = torch.from_numpy(res["clf_train_stem"])
        out["frozen"] = [clf_train_ref.loss_and_grads(csd, x, labels, w, dt, preprocessed=True, stem_override=stem) for dt in (torch.float64, torch.float32)]
        x, labels, w = clf_bn_ref.inputs(sx.CLF_BN_CASE)
        stem = torch.from_numpy(res["clf_bn_stem"])
        out["batch"] = [clf_bn_ref.loss_grads_stats(csd, x, labels, w, dt, preprocessed=True, stem_override=stem) for dt in (torch.float64, torch.float32)]
        refs["clf_cache"] = {key: out}
    return refs["clf_cache"][key]


# ---------------------------------------------------------------- the comparisons
def _maxabs(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def _grad_check(c, what, got, ref, scale_of, worst_bar, median_bar, vanishing, vanishing_bound=None, group=None):
    """test_gpu_train._grad_errors' measure -- per tensor max|g - ref| / max|scale| -- worst and median over the tensors with a gradient"""
    rel = sorted(((got[n].double() - ref[n].double()).abs().max().item() / scale_of[n].abs().max().item(), n) for n in ref if n not in vanishing)
    c.true(len(rel) == 324 and len(ref) == 330, f"{what}: {len(rel)} of {len(ref)} tensors measured")
    c.le(rel[-1][0], worst_bar, f"{what}: worst gradient tensor ({rel[-1][1]}), relative to its largest entry", group=group and f"worst gradient tensor {group}")
    c.le(rel[len(rel) // 2][0], median_bar, f"{what}: median gradient tensor of {len(rel)}", group=group and f"median gradient tensor {group}")
    if vanishing_bound is not None:
        for n in vanishing:
            c.le(got[n].abs().max().item(), vanishing_bound[n], f"largest entry of {n}", group=f"{what}: the tensors whose gradient vanishes")


def _ig_refs(refs, res):
    """autograd over the oracle with the child's own stem activation substituted, so that its max-pool takes the routes the GPU
    took (test_input_gradient_max_abs_when_the_pool_routes_are_replayed); once per distinct stem"""
    from oracle import resnet18 as ores
    key = res["clf_stem"].tobytes()
    if key not in refs["ig_cache"]:
        refs["ig_cache"] = {key: ores.score_input_gradient(refs["clf_sd"], sx.classifier_input(), sx.CLF_TARGET, stem_override=torch.from_numpy(res["clf_stem"]))[0]}
    return refs["ig_cache"][key]


def _ig_check(c, res, refs):
    """The bar of the replayed-route test: on every image one of the two CPU passes -- its own max-pool routes, or the GPU's,
    replayed -- agrees with the GPU EVERYWHERE within STRICT_TOL of the largest gradient; and the statistical test's cosine bar
    against the free pass.  Not REPLAY_TOL against the replayed pass alone: that bound was sized by one ReLU flip on that test's
    inputs (3.7e-4).  At 224 x 224 some pre-activation always lies within rounding of zero, and on the CPU alone a 2e-6 relative
    perturbation of the weights moves this gradient by 4.5e-3 .. 4.7e-2 of its largest entry (seeds 164 .. 175, routes held fixed),
    so which of the two passes a correct kernel lands on is a matter of its rounding: the bf16x3 and the f32 Winograd kernels land
    on different ones for image 1 here, each within 1.3e-6 of its pass."""
    got, replayed, free = torch.from_numpy(res["clf_input_gradient"]), _ig_refs(refs, res), refs["clf_ig"]
    for b in range(got.shape[0]):
        scale = replayed[b].abs().max().item()
        err, err_free = (got[b] - replayed[b]).abs().max().item() / scale, (got[b] - free[b]).abs().max().item() / scale
        c.le(min(err, err_free), STRICT_TOL, f"image {b}: on the GPU's max-pool routes {err:.1e}, on its own {err_free:.1e}", group="input gradient, the nearer of the two CPU passes")
        c.le(1.0 - F.cosine_similarity(got[b].flatten().double(), free[b].flatten().double(), dim=0).item(), 1.0 - IG_COSINE, f"image {b}", group="input gradient, 1 - cosine similarity to the free pass")


def _check_against_float64(c, res, refs):
    for mode in ("default", "latency"):
        for tag in ("b2_64", "b1_72x40", "b3_40x56"):
            c.le(_maxabs(res[f"unet_{mode}_{tag}"], refs[tag]), FWD_GUARD, tag, group=f"eval forwards, {mode} mode, against float64")
    for tag in ("b2_64", "b3_40x56", "b2_64_latency"):
        ref = refs["train_" + tag.replace("_latency", "")]
        c.true(np.array_equal(res[f"train_{tag}_noisy"], ref["noisy"].numpy()), f"train {tag}: add_noise is not the oracle's, bit for bit")
        c.le(_maxabs(res[f"train_{tag}_pred"], ref["pred"]), PRED_TOL, f"train {tag}: training-mode prediction against float64")
        c.le(abs(float(res[f"train_{tag}_loss"]) - ref["loss"]), LOSS_TOL * max(1.0, abs(ref["loss"])), f"train {tag}", group="training loss against float64")
        grads = _named(res[f"train_{tag}_grads"], res[f"train_{tag}_grad_names"])
        c.true(list(grads) == list(ref["grads"]), f"train {tag}: gradient names")
        bound = {n: max(VANISH_FLOOR, VANISH_FACTOR * ref["own_vanishing"][n]) for n in ref["vanishing"]}
        _grad_check(c, f"train {tag}, against float64", grads, ref["grads"], ref["grads"], GRAD_REL_WORST, GRAD_REL_MEDIAN, ref["vanishing"], bound)
    # the classifier
    z = refs["clf_logits"]
    zbar = LOGITS_TOL * max(1.0, z.abs().max().item())
    for name in ("clf_logits", "clf_input_gradient_logits", "clf_grad_cam_logits"):
        c.le(_maxabs(res[name], z), zbar, name, group="classifier logits against the oracle")
        c.true(np.array_equal(res[name], res["clf_logits"]), f"{name}: not the ordinary forward's bits")
    _ig_check(c, res, refs)
    c.le(_maxabs(res["clf_grad_cam"], refs["clf_cam"]), CAM_TOL, "Grad-CAM against the oracle")
    cr = _clf_train_refs(refs, res)
    (l64, g64, z64), (l32, g32, _) = cr["frozen"]
    c.true(len(g64) == 22, "22 gradients with frozen BatchNorm")
    got = _named(res["clf_train_grads"], [(k, list(g.shape)) for k, g in g64.items()])
    e32 = abs(l32 - l64) / abs(l64)
    c.le(abs(float(res["clf_train_loss"]) - l64) / abs(l64), clf_train_ref.bar(e32), f"loss (torch fp32: {e32:.1e})", group="classifier training, frozen BatchNorm, against float64")
    c.le(_maxabs(res["clf_train_logits"], z64), LOGITS_TOL * max(1.0, z64.abs().max().item()), "logits", group="classifier training, frozen BatchNorm, against float64")
    for k in g64:
        e32 = clf_train_ref.rel_err(g32[k], g64[k])
        c.le(clf_train_ref.rel_err(got[k], g64[k]), clf_train_ref.bar(e32), f"{k} (torch fp32: {e32:.1e})", group="classifier training, frozen BatchNorm, against float64")
    (l64, g64, s64, z64), (l32, g32, s32, _) = cr["batch"]
    c.true(len(g64) == 62 and len(s64) == 40, "62 gradients and 40 running statistics with batch statistics")
    got = _named(res["clf_bn_grads"], [(k, list(g.shape)) for k, g in g64.items()])
    stats = _named(res["clf_bn_running"], [(k, list(s.shape)) for k, s in s64.items()])
    e32 = abs(l32 - l64) / abs(l64)
    c.le(abs(float(res["clf_bn_loss"]) - l64) / abs(l64), clf_bn_ref.bar(e32), f"loss (torch fp32: {e32:.1e})", group="classifier training, batch statistics, against float64")
    c.le(_maxabs(res["clf_bn_logits"], z64), LOGITS_TOL * max(1.0, z64.abs().max().item()), "logits", group="classifier training, batch statistics, against float64")
    for k in g64:
        e32 = clf_bn_ref.rel_err(g32[k], g64[k])
        c.le(clf_bn_ref.rel_err(got[k], g64[k]), clf_bn_ref.bar(e32), f"{k} (torch fp32: {e32:.1e})", group="classifier training, batch statistics, against float64")
    for k in s64:
        e32 = clf_bn_ref.rel_err(s32[k], s64[k])
        c.le(clf_bn_ref.rel_err(stats[k], s64[k]), clf_bn_ref.bar(e32), f"{k} (torch fp32: {e32:.1e})", group="classifier training, batch statistics, against float64")


def _check_equalities(c, res, b64):
    for mode in ("default", "latency"):
        c.true(int(res[f"unet_{mode}_row0_equal"]) == 1 and np.array_equal(res[f"unet_{mode}_row0_as_batch_of_one"][0], res[f"unet_{mode}_b2_64"][0]),
               f"{mode} mode: row 0 as a batch of one is not row 0 of the batch")
    for tag in ("b2_64", "b3_40x56", "b2_64_latency"):
        c.true(int(res[f"train_{tag}_second_backward_equal"]) == 1, f"train {tag}: the second forward/backward is not the first, bit for bit")
        c.true(int(res[f"train_{tag}_tape_forward_is_the_forward"]) == 1 and np.array_equal(res[f"train_{tag}_eval_forward"], res[f"train_{tag}_pred"]),
               f"train {tag}: the tape forward is not the eval() forward")
    c.true(int(res["sample_latency_two_calls_equal"]) == 1, "the captured sampler's two calls differ")
    c.true(int(res["sample_latency_graph_builds"]) >= 1, f"the latency-mode sampler built {int(res['sample_latency_graph_builds'])} graphs: the step was not captured")
    _log(float(res["sample_latency_graph_builds"]), 1.0, f"switches [{c.label}] sisic_unet_graph_builds of the latency-mode sampler (at least 1)")
    bad = {k: v for k, v in res["unwritten"].items() if v != 0}
    c.true(not bad, f"unwritten elements: {bad}")
    floats = [k for k, v in res.items() if isinstance(v, np.ndarray) and v.dtype == np.float32 and v.ndim >= 1]
    c.true(("unet_default_b64_64" in res) == b64 and len(floats) == 38 + b64 and set(floats) <= set(res["unwritten"]), f"results missing: {len(floats)} float results")
    # (the guard bands: poison.check() at the end of the child raises, and the child then exits 1)


def _check_against_default(c, res, dflt, refs, equal_bits):
    names = [k for k in dflt if isinstance(dflt[k], np.ndarray) and k in res and (k.startswith(("unet_", "train_", "sample_")))]
    if equal_bits:
        c.true("unet_default_b64_64" in names, "the 64x64x64 forward is missing")
        for k in names:
            c.true(np.array_equal(res[k], dflt[k]), f"{k} is not the default child's, bit for bit")
    for mode in ("default", "latency"):
        for tag in ("b2_64", "b1_72x40", "b3_40x56"):
            k = f"unet_{mode}_{tag}"
            c.le(_maxabs(res[k], dflt[k]), 2 * FWD_GUARD, k, group="eval forwards against the default child")
    for tag in ("b2_64", "b3_40x56", "b2_64_latency"):
        ref = refs["train_" + tag.replace("_latency", "")]
        c.le(_maxabs(res[f"train_{tag}_pred"], dflt[f"train_{tag}_pred"]), 2 * PRED_TOL, f"train {tag}", group="training-mode prediction against the default child")
        c.le(abs(float(res[f"train_{tag}_loss"]) - float(dflt[f"train_{tag}_loss"])), 2 * LOSS_TOL * max(1.0, abs(ref["loss"])), f"train {tag}", group="training loss against the default child")
        a, b = (_named(r[f"train_{tag}_grads"], r[f"train_{tag}_grad_names"]) for r in (res, dflt))
        _grad_check(c, f"train {tag}", a, b, ref["grads"], 2 * GRAD_REL_WORST, 2 * GRAD_REL_MEDIAN, ref["vanishing"], group="against the default child")
    # sampling: frame by frame at the stated forward tolerance; the chain amplifies, the growth is logged
    for rule in ("ddpm", "dpmpp_device"):
        a, b = res[f"sample_{rule}_trajectory"], dflt[f"sample_{rule}_trajectory"]
        c.true(a.shape == b.shape and a.shape[0] >= 8, f"{rule}: trajectory shapes {a.shape}, {b.shape}")
        growth = [_maxabs(a[i], b[i]) for i in range(min(a.shape[0], b.shape[0]))]
        group = f"sampling {rule}, frames and latents against the default child (per frame: {' '.join(f'{g:.1e}' for g in growth)})"
        for i, g in enumerate(growth):
            c.le(g, FWD_TOL, f"frame {i}", group=group)
        c.le(_maxabs(res[f"sample_{rule}_latents"], dflt[f"sample_{rule}_latents"]), FWD_TOL, "latents", group=group)
    c.le(_maxabs(res["sample_latency_latents"], dflt["sample_latency_latents"]), FWD_TOL, "sampling, captured step: latents against the default child")
    # the classifier
    z = refs["clf_logits"]
    c.le(_maxabs(res["clf_logits"], dflt["clf_logits"]), 2 * LOGITS_TOL * max(1.0, z.abs().max().item()), "clf_logits against the default child")
    # (the same stem bits: the same max-pool routes, so the two gradients are comparable element by element)
    c.true(np.array_equal(res["clf_stem"], dflt["clf_stem"]), "the stem activation is not the default child's, bit for bit: no dispatch switch reaches the 7x7 stem")
    scale = refs["clf_ig"].flatten(1).abs().max(1).values.numpy().reshape(-1, 1, 1, 1)
    # (max-abs is logged, not held: two correct kernels may sit on different sides of a ReLU -- see _ig_check -- and each is held to a CPU pass there)
    _log(float((np.abs(res["clf_input_gradient"].astype(np.float64) - dflt["clf_input_gradient"]) / scale).max()), 2 * STRICT_TOL,
         f"switches [{c.label}] input gradient against the default child, worst element (within twice the bar where both follow one CPU pass)")
    for b in range(res["clf_input_gradient"].shape[0]):
        cos = F.cosine_similarity(torch.from_numpy(res["clf_input_gradient"][b]).flatten().double(), torch.from_numpy(dflt["clf_input_gradient"][b]).flatten().double(), dim=0).item()
        c.le(1.0 - cos, 2 * (1.0 - IG_COSINE), f"image {b}", group="input gradient, 1 - cosine similarity to the default child's")
    c.le(_maxabs(res["clf_grad_cam"], dflt["clf_grad_cam"]), 2 * CAM_TOL, "Grad-CAM against the default child")
    cr = _clf_train_refs(refs, res)
    for mode, names64, k_grads in (("frozen", cr["frozen"][0][1], "clf_train_grads"), ("batch", cr["batch"][0][1], "clf_bn_grads")):
        g32 = cr[mode][1][1]
        shapes = [(k, list(g.shape)) for k, g in names64.items()]
        a, b = _named(res[k_grads], shapes), _named(dflt[k_grads], shapes)
        worst = max(((a[k].double() - b[k].double()).abs().max().item() / names64[k].abs().max().item() / (2 * clf_train_ref.bar(clf_train_ref.rel_err(g32[k], names64[k]))), k)
                    for k in names64)
        c.le(worst[0], 1.0, f"classifier training, {mode}: worst gradient against the default child over twice its bar ({worst[1]})")


def _check_plans(c, name, res, dflt):
    table = sx.transitions(dflt["plans"], res["plans"], sx.table_keys())
    c.true(dict(table) == sx.TRANSITIONS[name], f"the child's plans differ from the default child's by {dict(table)}, not by {sx.TRANSITIONS[name]}")
    total = sum(sx.transitions(dflt["plans"], res["plans"]).values())
    c.true(total == sx.RECORD_TOTALS[name], f"{total} convolutions of the whole record changed, not {sx.RECORD_TOTALS[name]}")
    wino = {k: res["profile_launches"][k] for k in ("conv3x3_winograd_main", "conv3x3_winograd_bf16x3")}
    if "SISIC_WINOGRAD" in sx.SETS[name]:
        c.true(sum(wino.values()) == 0, f"launches in the Winograd profile slots with SISIC_WINOGRAD=0: {wino}")
        c.true(sum(dflt["profile_launches"][k] for k in wino) > 0, "the default child has none either: the slots count nothing")
    elif "SISIC_WINO_BF16X3" in sx.SETS[name]:
        c.true(wino["conv3x3_winograd_bf16x3"] == 0 and wino["conv3x3_winograd_main"] > 0, f"launches in the Winograd profile slots: {wino}")
    else:
        c.true(wino["conv3x3_winograd_bf16x3"] > 0, f"launches in the Winograd profile slots: {wino}")


# ---------------------------------------------------------------- the cases
def test_default_child_against_float64(default_child, refs):
    """no switch set, through the same child: the yardstick of every set is itself within the bars"""
    c = Checks("default")
    _check_against_float64(c, default_child, refs)
    _check_equalities(c, default_child, b64=True)
    c.true(sx.transitions(default_child["plans"], default_child["plans"]) == Counter(), "transitions of a record against itself")
    c.done()


@pytest.mark.parametrize("name", list(sx.SETS))
def test_executors_on_the_fallback_kernels(name, default_child, refs, tmp_path):
    res = _run_child(name, tmp_path / "out")
    c = Checks(name)
    _check_plans(c, name, res, default_child)
    _check_equalities(c, res, b64=name == sx.STAGED_SET)
    _check_against_float64(c, res, refs)
    _check_against_default(c, res, default_child, refs, equal_bits=name == sx.STAGED_SET)
    c.done()
