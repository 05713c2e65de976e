"""Training the ResNet18 classifier with batch-statistics BatchNorm (include/sisic.h, "training the classifier with
batch-statistics BatchNorm"): the BatchNorm kernels against float64, the loss, the 62 gradients and the 40 running statistics
against float64 autograd over tests/clf_bn_ref.py, determinism, three optimizer steps beside the restatement, the inference side
after every step, a skipped step, the refusals, a held side stream, and a small learning run from default-initialised weights.

Measure and bar (tests/clf_train_ref.py): max|v - v64| / max|v64| <= max(1e-5, 16 * e32), e32 the same measure for fp32 torch on
the same inputs and routing.  Every gradient case is under the conditioning cap of tests/test_clf_bn_cpu.py (e32 <= 1e-4).
The max-pool of both references is routed by the library's own training-mode stem activation, formed here with the same
launches the model issues (ops.conv2d on the packed conv1 filter, ops.batchnorm_train).

Slice rule of the kernels (batchnorm.hip: a channel's planes are dealt to clamp(B*HW / 8192, 1, 2048 / C) workgroups):
(4,512,1), (3,256,2), (2,64,49) and (2,128,196) are one slice per channel; (8,64,3136) is three slices, (2,8,20000) -- planes
longer than one 4096-float run -- four.  The two apply passes cut a plane into runs of 256 floats: one short run at HW <= 196,
twelve runs and a 64-float rest at 3136, 78 and a 32-float rest at 20000.
"""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

import clf_bn_ref as ref
import clf_train_ref as ctr
import stream_probe as sp
from oracle import resnet18 as ores
from poison import guard_bands, poison_allocations, unwritten  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def clf_sd():
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    return synthetic_resnet18_state_dict()


def _new_clf(sd):
    from synt_isic_amd.classifier import HipMelanomaClassifier
    m = HipMelanomaClassifier(num_classes=7)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _adam(clf, **kw):
    from synt_isic_amd.train import HipClassifierAdam
    kw.setdefault("batchnorm", "batch")
    return HipClassifierAdam(clf, **kw)


def _equal(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def _probe_input():
    return torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(77)) * 1.6 - 0.8


def _train_stem(sd, x, preprocessed):
    """relu(bn1(conv1(.))) with batch statistics by the library's own launches, on the CPU (the max-pool routes of a case)"""
    from synt_isic_amd import ops
    h = x.float() if preprocessed else ores.preprocess_for_classifier(x.float())
    h = h.to(DEV).contiguous()
    w = sd["model.conv1.weight"].detach().float().to(DEV).contiguous()
    y = ops.conv2d(h, ops.pack_conv_weight(w), 64, 7, stride=2)
    out, _, _ = ops.batchnorm_train(y, sd["model.bn1.weight"].float().to(DEV).contiguous(),
                                    sd["model.bn1.bias"].float().to(DEV).contiguous(), eps=ores.BN_EPS, relu=True)
    return out.cpu()


# ---------------------------------------------------------------- kernels
def _check(rows):
    for name, err, e32 in rows:
        print(f"{name}: GPU {err:.3e}, torch fp32 {e32:.3e}, bar {ref.bar(e32):.3e}")
    for name, err, e32 in rows:
        assert err <= ref.bar(e32), f"{name}: {err:.3e} from float64, torch fp32 {e32:.3e}, bar {ref.bar(e32):.3e}"


def _kernel_case(shape, residual, relu, running, offset_mean=False, shift=0):
    """forward and backward of one BatchNorm against float64; shift: floats the operands lie past a 256-byte boundary"""
    from synt_isic_amd import ops
    y, gamma, beta, res, g, rm, rv = ref.kernel_operands(shape, offset_mean=offset_mean)

    def dev(t):
        base = torch.empty(t.numel() + shift, dtype=torch.float32, device=DEV)
        v = base[shift:].view(t.shape)
        v.copy_(t)
        return v
    yd, gd, resd = dev(y), dev(g), dev(res) if residual else None
    gam, bet = gamma.to(DEV), beta.to(DEV)
    rmd, rvd = (rm.to(DEV), rv.to(DEV)) if running else (None, None)
    out, mean, invstd = ops.batchnorm_train(yd, gam, bet, eps=ores.BN_EPS, residual=resd, relu=relu, running_mean=rmd,
                                            running_var=rvd, momentum=0.25)
    assert unwritten(out) == 0 and unwritten(mean) == 0 and unwritten(invstd) == 0
    tag = f"{shape} res={residual} relu={relu} run={running} offset={offset_mean} shift={shift}"
    kw = dict(residual=res if residual else None, relu=False, running=(rm, rv) if running else None, momentum=0.25)
    o64, m64, i64, rm64, rv64 = ref.bn_forward(y, gamma, beta, dtype=torch.float64, **kw)
    o32, m32, i32, rm32, rv32 = ref.bn_forward(y, gamma, beta, dtype=torch.float32, **kw)
    mask = (out.cpu() > 0) if relu else None                 # the ReLU mask from the library's own output
    if relu:
        o64, o32 = o64 * mask, o32 * mask
    rows = [(f"{tag} out", ref.rel_err(out, o64), ref.rel_err(o32, o64)), (f"{tag} mean", ref.rel_err(mean, m64), ref.rel_err(m32, m64)),
            (f"{tag} invstd", ref.rel_err(invstd, i64), ref.rel_err(i32, i64))]
    if running:
        rows += [(f"{tag} running_mean", ref.rel_err(rmd, rm64), ref.rel_err(rm32, rm64)),
                 (f"{tag} running_var", ref.rel_err(rvd, rv64), ref.rel_err(rv32, rv64))]
    # a second call gives equal bits
    rm2, rv2 = (rm.to(DEV), rv.to(DEV)) if running else (None, None)
    again = ops.batchnorm_train(yd, gam, bet, eps=ores.BN_EPS, residual=resd, relu=relu, running_mean=rm2, running_var=rv2, momentum=0.25)
    assert sp.same(again, (out, mean, invstd)) and sp.same((rm2, rv2), (rmd, rvd))
    # backward
    dy, dgamma, dbeta = ops.batchnorm_train_bwd(gd, yd, mean, invstd, gam, act=out if relu else None)
    assert unwritten(dy) == 0 and unwritten(dgamma) == 0 and unwritten(dbeta) == 0
    want = ref.bn_backward(g, y, gamma, mask=mask, dtype=torch.float64)
    yard = ref.bn_backward(g, y, gamma, mask=mask, dtype=torch.float32)
    rows += [(f"{tag} {n}", ref.rel_err(a, b), ref.rel_err(c, b)) for n, a, b, c in zip(("dy", "dgamma", "dbeta"), (dy, dgamma, dbeta), want, yard)]
    assert sp.same(ops.batchnorm_train_bwd(gd, yd, mean, invstd, gam, act=out if relu else None), (dy, dgamma, dbeta))
    _check(rows)


@pytest.mark.parametrize("shape", ref.KERNEL_SHAPES, ids=str)
def test_batchnorm_kernels_match_float64(shape):
    _kernel_case(shape, residual=False, relu=False, running=False)
    _kernel_case(shape, residual=True, relu=True, running=True)
    _kernel_case(shape, residual=False, relu=True, running=True, shift=1)       # every tensor but the outputs off a 16-byte boundary


def test_batchnorm_kernels_on_the_offset_mean_operands():
    """per-channel means of 30 .. 60 at a standard deviation of 0.05: fp32 E[x^2] - E[x]^2 moments are 300 x over this bar
    (tests/test_clf_bn_cpu.py)"""
    _kernel_case(ref.OFFSET_SHAPE, residual=False, relu=False, running=True, offset_mean=True)
    _kernel_case(ref.OFFSET_SHAPE, residual=True, relu=True, running=False, offset_mean=True)


def test_one_value_per_channel_is_refused():
    from synt_isic_amd import ops
    from synt_isic_amd._lib import SisicError
    y = torch.randn(1, 16, 1, device=DEV)
    ones = torch.ones(16, device=DEV)
    with pytest.raises(SisicError, match="more than 1 value per channel"):
        ops.batchnorm_train(y, ones, ones)
    with pytest.raises(SisicError, match="more than 1 value per channel"):
        ops.batchnorm_train_bwd(y, y, ones, ones, ones)
    with pytest.raises(SisicError, match="momentum"):
        ops.batchnorm_train(torch.randn(2, 16, 4, device=DEV), ones, ones, running_mean=ones.clone(), running_var=ones.clone(), momentum=0.0)


# ---------------------------------------------------------------- whole model
@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_loss_gradients_and_running_statistics_match_float64_autograd(clf_sd, case):
    pre = case[0]
    x, labels, w = ref.inputs(case)
    clf = _new_clf(clf_sd)
    opt = _adam(clf, bn_momentum=ref.MOMENTUM)
    assert clf.trainable_names("batch") == ref.trainable_names(clf_sd)
    loss, logits = clf.loss_backward(x, labels, class_weights=w, preprocessed=pre)
    grads = clf.grads()
    stats = OrderedDict((k, clf.read_tensor(0, k)) for k in ref.buffer_names(clf_sd))
    stem = _train_stem(clf_sd, x, pre)
    l64, g64, s64, z64 = ref.loss_grads_stats(clf_sd, x, labels, w, torch.float64, preprocessed=pre, stem_override=stem)
    l32, g32, s32, _ = ref.loss_grads_stats(clf_sd, x, labels, w, torch.float32, preprocessed=pre, stem_override=stem)
    assert list(grads) == list(g64) and len(grads) == 62 and list(stats) == list(s64) and len(stats) == 40
    rows = [(f"{case} loss", abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64))]
    rows += [(f"{case} {k}", ref.rel_err(grads[k], g64[k]), ref.rel_err(g32[k], g64[k])) for k in g64]
    rows += [(f"{case} {k}", ref.rel_err(stats[k], s64[k]), ref.rel_err(s32[k], s64[k])) for k in s64]
    assert (logits.cpu().double() - z64).abs().max().item() <= 2e-4 * max(1.0, z64.abs().max().item())
    _check(rows)
    # the state dict carries the moved statistics; a second call from the same parameters gives the same gradient bits
    sd = clf.state_dict()
    assert all(torch.equal(sd[k].cpu(), stats[k]) for k in stats) and all(torch.equal(sd[k].cpu(), clf_sd[k]) for k in g64)
    if case == ref.CASES[2]:
        opt.zero_grad()
        assert all(not g.any() for g in clf.grads().values())
        loss2, logits2 = clf.loss_backward(x, labels, class_weights=w, preprocessed=pre)
        assert loss2 == loss and torch.equal(logits2, logits) and _equal(clf.grads(), grads)
        assert not torch.equal(clf.read_tensor(0, "model.bn1.running_mean"), stats["model.bn1.running_mean"])     # a second update
    opt.close()


# ---------------------------------------------------------------- optimizer
def _flat(named, names):
    return torch.cat([named[k].detach().cpu().reshape(-1) for k in names])


def _ref_step(state, x, labels, stem, step, adam, max_norm):
    """one step of the restatement in state's dtype: gradients by autograd, clip_grad_norm_, Adam; returns the norm"""
    sd = state["sd"]
    dt = next(iter(sd.values())).dtype
    _, g, stats, _ = ref.loss_grads_stats(sd, x, labels, None, dt, preprocessed=True, stem_override=stem)
    names = list(g)
    norm = torch.sqrt(sum((v.double() ** 2).sum() for v in g.values())).item()
    coef = min(1.0, max_norm / (norm + 1e-6))
    for k in names:
        gk = g[k] * torch.tensor(coef, dtype=dt)
        p, m, v = ctr.adam_step(sd[k], gk, state["m"][k], state["v"][k], step, **adam)
        sd[k], state["m"][k], state["v"][k] = p, m, v
    sd.update(stats)
    return norm


def test_three_steps_beside_the_restatement_and_the_inference_side_after_each(clf_sd):
    case = ref.CASES[0]
    x, labels, _ = ref.inputs(case)
    probe = _probe_input().to(DEV)
    adam = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-3)
    clf = _new_clf(clf_sd)
    opt = _adam(clf, max_grad_norm=1.0, bn_momentum=ref.MOMENTUM, **adam)
    names, buffers = ref.trainable_names(clf_sd), ref.buffer_names(clf_sd)
    states = {}
    for dt in (torch.float64, torch.float32):
        sd = OrderedDict((k, v.to(dt).clone()) for k, v in clf_sd.items())
        states[dt] = {"sd": sd, "m": {k: torch.zeros_like(sd[k]) for k in names}, "v": {k: torch.zeros_like(sd[k]) for k in names}}
    for step in (1, 2, 3):
        stem = _train_stem(clf.state_dict(), x, True)              # the routes of the library's weights as they stand
        clf.loss_backward(x, labels, preprocessed=True)
        assert opt.step() is True and opt.steps == step
        norms = {dt: _ref_step(states[dt], x, labels, stem, step, adam, 1.0) for dt in states}
        s64, s32 = states[torch.float64], states[torch.float32]
        sd = clf.state_dict()
        got = {"param": _flat(sd, names), "exp_avg": _flat({k: clf.read_tensor(2, k) for k in names}, names),
               "exp_avg_sq": _flat({k: clf.read_tensor(3, k) for k in names}, names), "running": _flat(sd, buffers)}
        want = {dt: {"param": _flat(s["sd"], names), "exp_avg": _flat(s["m"], names), "exp_avg_sq": _flat(s["v"], names),
                     "running": _flat(s["sd"], buffers)} for dt, s in states.items()}
        rows = [(f"step {step} {k}", ref.rel_err(got[k], want[torch.float64][k]), ref.rel_err(want[torch.float32][k], want[torch.float64][k]))
                for k in got]
        rows.append((f"step {step} grad_norm", abs(opt.grad_norm - norms[torch.float64]) / norms[torch.float64],
                     abs(norms[torch.float32] - norms[torch.float64]) / norms[torch.float64]))
        _check(rows)
        assert opt.grad_norm > 1.0                                  # the clip was active
        fresh = _new_clf(sd)
        assert torch.equal(clf.forward(probe), fresh.forward(probe)), f"step {step}: the inference side is not a fresh load"
    g1, _ = clf.input_gradient(probe, 1)
    g2, _ = fresh.input_gradient(probe, 1)
    assert torch.equal(g1, g2)
    opt.close()
    assert torch.equal(clf.forward(probe), fresh.forward(probe)) and _equal(clf.state_dict(), sd)
    clf.randomize_weights(3, 0)                                    # restore folds the host copies again: the trained ones
    clf.restore_weights()
    assert torch.equal(clf.forward(probe), fresh.forward(probe))


def test_a_skipped_step_moves_nothing_but_the_inference_side_follows_the_statistics(clf_sd):
    x, labels, _ = ref.inputs(ref.CASES[0])
    probe = _probe_input().to(DEV)
    names = ref.trainable_names(clf_sd)
    clf = _new_clf(clf_sd)
    opt = _adam(clf, lr=1e-3)
    clf.loss_backward(x, labels, preprocessed=True)
    assert opt.step() is True
    before = (clf.state_dict(), {k: clf.read_tensor(2, k) for k in names}, {k: clf.read_tensor(3, k) for k in names})
    clf.loss_backward(x, labels, preprocessed=True)
    bad = clf.read_tensor(1, "model.layer3.1.bn2.weight")
    bad[17] = float("inf")
    clf.write_tensor(1, "model.layer3.1.bn2.weight", bad)
    assert opt.step() is False and opt.steps == 1
    sd = clf.state_dict()
    assert all(torch.equal(sd[k], before[0][k]) for k in names)
    assert _equal({k: clf.read_tensor(2, k) for k in names}, before[1]) and _equal({k: clf.read_tensor(3, k) for k in names}, before[2])
    assert not torch.equal(sd["model.bn1.running_var"], before[0]["model.bn1.running_var"])       # the forward moved them
    assert torch.equal(clf.forward(probe), _new_clf(sd).forward(probe))
    opt.close()


# ---------------------------------------------------------------- plumbing
def test_mode_plumbing_and_refusals(clf_sd):
    from synt_isic_amd import _lib
    from synt_isic_amd._lib import SisicError
    from synt_isic_amd.train import HipClassifierAdam
    x, labels, _ = ref.inputs(ref.CASES[0])
    clf = _new_clf(clf_sd)
    lib = _lib.load()
    assert lib.sisic_resnet_train_bn_mode(clf.handle) == -1
    with pytest.raises(ValueError, match="batchnorm"):
        HipClassifierAdam(clf, batchnorm="eval")
    for m in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(SisicError, match="momentum"):
            HipClassifierAdam(clf, batchnorm="batch", bn_momentum=m)
    cfg = _lib.ResnetBnConfig(2, 0.1)
    assert lib.sisic_resnet_train_begin_bn(clf.handle, C.byref(cfg)) == _lib.SISIC_EINVAL
    assert clf._trainer is None and lib.sisic_resnet_train_bn_mode(clf.handle) == -1
    frozen = HipClassifierAdam(clf)                                  # the default mode, through the old entry
    assert lib.sisic_resnet_train_bn_mode(clf.handle) == 0 and len(clf.grads()) == 22
    with pytest.raises(SisicError, match="frozen"):
        clf.read_tensor(1, "model.bn1.weight")
    frozen.close()
    cfg = _lib.ResnetBnConfig(0, 0.0)                                # mode 0 of the new entry is the old entry
    _lib.check(lib.sisic_resnet_train_begin_bn(clf.handle, C.byref(cfg)))
    assert lib.sisic_resnet_train_bn_mode(clf.handle) == 0
    _lib.check(lib.sisic_resnet_train_end(clf.handle))
    opt = _adam(clf, bn_momentum=1.0)
    assert lib.sisic_resnet_train_bn_mode(clf.handle) == 1 and len(clf.grads()) == 62
    cfg = _lib.ResnetBnConfig(1, 0.1)
    assert lib.sisic_resnet_train_begin_bn(clf.handle, C.byref(cfg)) == _lib.SISIC_ESTATE           # begin twice
    assert b"training already" in lib.sisic_last_error()
    with pytest.raises(RuntimeError, match="already has"):
        _adam(clf)
    with pytest.raises(SisicError, match="running statistic"):
        clf.read_tensor(1, "model.bn1.running_mean")
    with pytest.raises(SisicError, match="running statistic"):
        clf.write_tensor(2, "model.layer4.1.bn2.running_var", torch.zeros(512))
    assert torch.equal(clf.read_tensor(0, "model.bn1.running_mean"), clf_sd["model.bn1.running_mean"])
    with pytest.raises(SisicError, match="more than 1 value per channel"):
        clf.loss_backward(torch.zeros(1, 3, 32, 32), labels[:1], preprocessed=True)
    with pytest.raises(SisicError, match="odd feature map"):
        clf.loss_backward(torch.zeros(4, 3, 36, 32), labels, preprocessed=True)
    # momentum 1: the running statistics are the batch's own, and num_batches_tracked counts the forwards
    full = OrderedDict(clf_sd)
    full["model.bn1.num_batches_tracked"] = torch.tensor(5)
    opt.close()
    clf.load_state_dict(full)
    opt = _adam(clf, bn_momentum=1.0)
    clf.loss_backward(x, labels, preprocessed=True)
    stem_y = torch.nn.functional.conv2d(x.double(), clf_sd["model.conv1.weight"].double(), None, stride=2, padding=3)
    sd = clf.state_dict()
    assert int(sd["model.bn1.num_batches_tracked"]) == 6 and list(sd).index("model.bn1.num_batches_tracked") == 5
    assert ref.rel_err(sd["model.bn1.running_var"], stem_y.var(dim=(0, 2, 3), unbiased=True)) <= 1e-5
    opt.close()


# ---------------------------------------------------------------- a held side stream
def test_side_stream_gives_the_default_stream_bits(clf_sd):
    """loss_backward + step in batch-statistics mode, then ops.batchnorm_train, ops.batchnorm_train_bwd and ops.add_relu, each on
    a side stream that a spin kernel holds.  (Four side streams in this file: torch hands its pool streams out in turn, and the
    hardware queue a later file's stream lands on -- the positive control of tests/test_gpu_streams.py depends on it, with four
    queues per process -- stays the one it was before this file existed.)"""
    from synt_isic_amd import ops
    case = ref.CASES[1]
    _, labels, _ = ref.inputs(case)
    pairs = []
    for _ in range(3):
        clf = _new_clf(clf_sd)
        pairs.append((clf, _adam(clf, lr=1e-3, max_grad_norm=1.0)))
    torch.cuda.synchronize()
    todo = list(pairs)

    def fn(x):
        clf, opt = todo.pop(0)
        loss, logits = clf.loss_backward(x, labels, preprocessed=True)
        ok = opt.step()
        return loss, logits, ok, opt.grad_norm, clf.grads(), clf.state_dict(), clf.forward(x, preprocessed=True)

    baseline, held, _ = sp.run_held(fn, lambda: [ref.inputs(case)[0].to(DEV)],
                                    lambda: [torch.randn(3, 3, 32, 64, generator=torch.Generator().manual_seed(1)).to(DEV)],
                                    "classifier loss_backward + step, batch statistics")
    assert baseline[2] is True and sp.same(baseline, held)
    for _, opt in pairs:
        opt.close()

    # the three operator entries carry their stream in the argument struct as well (no registry entry in stream_probe.py):
    # each on a held side stream of its own, none may wait for it
    y, gamma, beta, res, g, rm, rv = ref.kernel_operands((8, 64, 3136))
    ydev, gam, bet = y.to(DEV), gamma.to(DEV), beta.to(DEV)
    out, mean, invstd = ops.batchnorm_train(ydev, gam, bet, relu=True)

    def fwd(yd, resd, rmd, rvd):
        return ops.batchnorm_train(yd, gam, bet, residual=resd, relu=True, running_mean=rmd, running_var=rvd), rmd, rvd

    def bwd(gd, yd, act):
        return ops.batchnorm_train_bwd(gd, yd, mean, invstd, gam, act=act)

    noise = lambda t: torch.randn(t.shape, generator=torch.Generator().manual_seed(3)).to(DEV)      # noqa: E731
    probes = [("batchnorm_train", fwd, lambda: [y.to(DEV), res.to(DEV), rm.to(DEV), rv.to(DEV)],
               lambda: [noise(y), noise(res), rm.to(DEV), rv.to(DEV)]),
              ("batchnorm_train_bwd", bwd, lambda: [g.to(DEV), y.to(DEV), out.clone()], lambda: [noise(g), noise(y), noise(y)]),
              ("add_relu", ops.add_relu, lambda: [y.to(DEV), res.to(DEV)], lambda: [noise(y), noise(res)])]
    for name, fn, make, warm in probes:
        baseline, held, until_return = sp.run_held(fn, make, warm, name)
        assert sp.same(baseline, held), f"{name}: the result on a held side stream differs from the default-stream result"
        assert until_return, f"sisic_{name} waited for its stream"
    assert torch.equal(ops.add_relu(y.to(DEV), res.to(DEV)).cpu(), torch.relu(y + res))


# ---------------------------------------------------------------- learning from scratch
class _Preprocessed:
    """a classifier whose predict() takes already normalised network inputs (what evaluate_classifier calls)"""

    def __init__(self, clf):
        self.clf, self.num_classes, self.device = clf, clf.num_classes, clf.device

    @property
    def handle(self):
        return self.clf.handle

    def predict(self, x):
        return self.clf.forward(x, preprocessed=True).argmax(dim=1)


def test_learns_two_classes_from_default_initialised_weights():
    """16 normalised 32x32 images, two classes (dark with a bright disc / bright with a dark cross, plus noise), 30 steps at
    batch 16 from an untrained resnet18's weights: the training-mode logits get all 16 right, and so does the inference side
    with the running statistics"""
    from synt_isic_amd.train import evaluate_classifier
    from synt_isic_amd.weights import default_init_resnet18_state_dict
    g = torch.Generator().manual_seed(2)
    yy, xx = torch.meshgrid(torch.arange(32.0), torch.arange(32.0), indexing="ij")
    disc = (((yy - 16) ** 2 + (xx - 16) ** 2) < 9 ** 2).float()
    cross = (((yy - 16).abs() < 3) | ((xx - 16).abs() < 3)).float()
    labels = torch.tensor([0, 1] * 8)
    images = torch.stack([(-1.0 + 2.0 * disc if y == 0 else 1.0 - 2.0 * cross).expand(3, 32, 32) for y in labels.tolist()])
    images = (images + 0.1 * torch.randn(images.shape, generator=g)).to(DEV)
    clf = _new_clf(default_init_resnet18_state_dict(0, 7))
    opt = _adam(clf, lr=1e-3)
    losses = []
    for _ in range(30):
        loss, logits = clf.loss_backward(images, labels, preprocessed=True)
        assert opt.step() is True
        losses.append(loss)
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert int((logits.argmax(dim=1).cpu() == labels).sum()) == 16
    res = evaluate_classifier(_Preprocessed(clf), [(images[:10], labels[:10]), (images[10:], labels[10:])])
    assert res["accuracy"] == 1.0 and res["confusion_matrix"][0, 0] == 8 and res["confusion_matrix"][1, 1] == 8
    opt.close()
