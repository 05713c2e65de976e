"""Training the ResNet18 classifier with BatchNorm frozen (include/sisic.h, "training the classifier"): the 22 gradients and the
loss against float64 autograd over oracle/resnet18.py, determinism, the Adam step, the rebuild of every folded and packed
filter, the paths that must not move, a small learning run, the refusals, and a held side stream.

Gradient bar (tests/clf_train_ref.py): per tensor max|g - g64| / max|g64| <= max(1e-5, 16 * e32), e32 the same measure for
fp32 torch autograd on the same inputs.  Both references are fed the library's own stem activation (stem_override), as
tests/test_gpu_classifier.py does for the input gradient, so a max-pool route that flips in the last bit is not taken for an
error.  Measured values: profiles/r28/classifier_train_parity.txt.

Streams: sisic_resnet_loss_backward and sisic_resnet_optimizer_step carry their stream in the argument struct, so the
registry of tests/stream_probe.py (which lists declarations with a `void* stream` parameter) does not know them; this file
drives both on a held side stream itself, with stream_probe's helpers (test_side_stream_gives_the_default_stream_bits).
Both calls wait for their stream once (the loss, the 12-byte statistics record), as the header says.
"""
import ctypes as C
import math
import os
from collections import OrderedDict

import pytest
import torch

import clf_train_ref as ref
import optim_ext_ref as oref
import stream_probe as sp
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
ADAM_BAR = 2.0          # tests/test_gpu_optimizer.py: the GPU's distance from float64 over torch-fp32's own


@pytest.fixture(scope="module")
def clf_sd():
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    return synthetic_resnet18_state_dict()        # BatchNorm weight 1 + 0.1 N, running_mean 0.1 N, running_var 1 + 0.2 |N|


def _new_clf(sd):
    from synt_isic_amd.classifier import HipMelanomaClassifier
    m = HipMelanomaClassifier(num_classes=7)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _adam(clf, **kw):
    from synt_isic_amd.train import HipClassifierAdam
    return HipClassifierAdam(clf, **kw)


def _stem(clf, x, preprocessed):
    """the library's relu(bn1(conv1(.))) of x (sisic_resnet_stem), on the CPU"""
    from synt_isic_amd import _lib, ops
    x = x.to(DEV).float().contiguous()
    B, _, H, W = x.shape
    h, w = (H // 2, W // 2) if preprocessed else (112, 112)
    out = ops.empty((B, 64, h, w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().sisic_resnet_stem(clf.handle, x.data_ptr(), out.data_ptr(), B, H, W, 0 if preprocessed else 1,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out.cpu()


def _equal(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def _xai_bits(clf, x):
    """logits, input gradient and Grad-CAM of x: what every reader of the filters produces"""
    x = x.to(DEV)
    grad, _ = clf.input_gradient(x, 1)
    cam, _ = clf.grad_cam(x, 2)
    return clf(x).cpu(), grad.cpu(), cam.cpu()


def _probe_input():
    return torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(77)) * 1.6 - 0.8


# ---------------------------------------------------------------- gradients
@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_gradients_and_loss_match_float64_autograd(clf_sd, case):
    pre = case[0]
    x, labels, w = ref.inputs(case)
    clf = _new_clf(clf_sd)
    opt = _adam(clf)
    loss, logits = clf.loss_backward(x, labels, class_weights=w, preprocessed=pre)
    grads = clf.grads()
    assert torch.equal(logits, clf.forward(x, preprocessed=pre))          # the training forward is the forward, bit for bit
    stem = _stem(clf, x, pre)
    l64, g64, z64 = ref.loss_and_grads(clf_sd, x, labels, w, torch.float64, preprocessed=pre, stem_override=stem)
    l32, g32, _ = ref.loss_and_grads(clf_sd, x, labels, w, torch.float32, preprocessed=pre, stem_override=stem)
    assert list(grads) == list(g64) and len(grads) == 22
    rows = [("loss", abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64))]
    rows += [(k, ref.rel_err(grads[k], g64[k]), ref.rel_err(g32[k], g64[k])) for k in g64]
    for name, err, e32 in rows:
        print(f"{case}: {name}: GPU {err:.3e}, torch fp32 {e32:.3e}, bar {ref.bar(e32):.3e}")
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            for name, err, e32 in rows:
                f.write(f"{err:.3e}\t{e32:.3e}\t{ref.bar(e32):.3e}\tclassifier_train {case} {name}\n")
    assert (logits.cpu().double() - z64).abs().max().item() <= 2e-4 * max(1.0, z64.abs().max().item())
    for name, err, e32 in rows:
        assert err <= ref.bar(e32), f"{case}: {name}: {err:.3e} from float64, torch fp32 {e32:.3e}, bar {ref.bar(e32):.3e}"
    opt.close()


def test_two_backward_calls_give_equal_bits(clf_sd):
    x, labels, w = ref.inputs(ref.CASES[1])
    clf = _new_clf(clf_sd)
    opt = _adam(clf)
    l1, z1 = clf.loss_backward(x, labels, class_weights=w, preprocessed=True)
    g1 = clf.grads()
    opt.zero_grad()
    assert all(not g.any() for g in clf.grads().values())
    l2, z2 = clf.loss_backward(x, labels, class_weights=w, preprocessed=True)
    assert l1 == l2 and torch.equal(z1, z2) and _equal(g1, clf.grads())
    opt.close()


# ---------------------------------------------------------------- optimizer
def _flat(named, names):
    return torch.cat([named[k].detach().cpu().reshape(-1) for k in names])


def _grad_seq(sd, names, steps, seed=20261):
    """gradients of the test's choosing: randn * 10^U(-8, 0) per element, a different draw per step"""
    gen = torch.Generator().manual_seed(seed)
    seq = []
    for _ in range(steps):
        seq.append(OrderedDict((k, torch.randn(sd[k].shape, generator=gen)
                                * torch.exp(torch.rand(sd[k].shape, generator=gen) * (-8.0 * math.log(10.0)))) for k in names))
    return seq


def _adam_errors(p, m, v, p64, m64, v64, gmax):
    """the statistics of tests/test_gpu_optimizer.py: parameters max-abs, exp_avg_sq relative, exp_avg over the running max|g|"""
    p, m, v = p.double(), m.double(), v.double()
    return {"param": (p - p64).abs().max().item(),
            "exp_avg_sq": ((v - v64).abs() / v64.clamp(min=1e-30) * (v64 > 1e-30)).max().item(),
            "exp_avg": ((m - m64).abs() / gmax.clamp(min=1e-300) * (gmax > 0)).max().item()}


def test_adam_three_steps_on_injected_gradients(clf_sd):
    names = ref.trainable_names(clf_sd)
    adam = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6)
    clf = _new_clf(clf_sd)
    opt = _adam(clf, **adam)
    state = {dt: [_flat(clf_sd, names).to(dt), None, None] for dt in (torch.float64, torch.float32)}
    for dt in state:
        state[dt][1], state[dt][2] = torch.zeros_like(state[dt][0]), torch.zeros_like(state[dt][0])
    gmax = torch.zeros_like(state[torch.float64][0])
    frozen = {k: v for k, v in clf_sd.items() if k not in names}
    for step, g in enumerate(_grad_seq(clf_sd, names, 3), 1):
        clf.set_grads(g)
        assert _equal(clf.grads(), g)
        assert opt.step() is True and opt.steps == step
        gf = _flat(g, names)
        gmax = torch.maximum(gmax, gf.abs().double())
        for dt in state:
            state[dt] = list(ref.adam_step(*state[dt][:1], gf, *state[dt][1:], step, **adam))
        sd = clf.state_dict()
        got = _adam_errors(_flat(sd, names), _flat({k: clf.read_tensor(2, k) for k in names}, names),
                           _flat({k: clf.read_tensor(3, k) for k in names}, names), *state[torch.float64], gmax)
        yard = _adam_errors(*state[torch.float32], *state[torch.float64], gmax)
        for k in got:
            print(f"step {step}: {k}: GPU {got[k]:.3e}, torch fp32 {yard[k]:.3e}")
            assert got[k] <= ADAM_BAR * yard[k], f"step {step}: {k} is {got[k]:.3e} from float64, torch fp32 {yard[k]:.3e}"
        assert all(torch.equal(sd[k].cpu(), v) for k, v in frozen.items())       # BatchNorm tensors: unchanged
    opt.close()


def test_a_non_finite_gradient_makes_no_update(clf_sd):
    names = ref.trainable_names(clf_sd)
    clf = _new_clf(clf_sd)
    opt = _adam(clf)
    g = _grad_seq(clf_sd, names, 2, seed=5)
    clf.set_grads(g[0])
    assert opt.step() is True
    before = (clf.state_dict(), {k: clf.read_tensor(2, k) for k in names}, {k: clf.read_tensor(3, k) for k in names})
    bits = _xai_bits(clf, _probe_input())
    bad = OrderedDict((k, v.clone()) for k, v in g[1].items())
    bad["model.layer3.1.conv2.weight"].view(-1)[12345] = float("inf")
    clf.set_grads(bad)
    assert opt.step() is False and opt.steps == 1
    assert _equal(clf.state_dict(), before[0])
    assert _equal({k: clf.read_tensor(2, k) for k in names}, before[1]) and _equal({k: clf.read_tensor(3, k) for k in names}, before[2])
    assert sp.same(_xai_bits(clf, _probe_input()), bits)
    bad["model.layer3.1.conv2.weight"].view(-1)[12345] = float("nan")
    clf.set_grads(bad)
    assert opt.step() is False and opt.steps == 1
    clf.set_grads(g[1])
    assert opt.step() is True and opt.steps == 2                             # and training goes on
    opt.close()


def test_clipping_equals_the_unclipped_step_on_the_clipped_gradient(clf_sd):
    names = ref.trainable_names(clf_sd)
    g = OrderedDict((k, v * 3.0) for k, v in _grad_seq(clf_sd, names, 1, seed=9)[0].items())
    norm64, norm32, coef = oref.clip_stats(_flat(g, names), 1.0, 1.0)
    assert coef < 1.0
    clipped = _new_clf(clf_sd)
    opt = _adam(clipped, lr=1e-3, max_grad_norm=1.0)
    clipped.set_grads(g)
    assert opt.step() is True
    assert abs(opt.grad_norm - norm64) <= 2e-7 * norm64
    coef = oref.clip_coef_of(torch.tensor(opt.grad_norm, dtype=torch.float32).numpy(), 1.0)
    plain = _new_clf(clf_sd)
    opt2 = _adam(plain, lr=1e-3)
    plain.set_grads(OrderedDict((k, v * torch.tensor(float(coef), dtype=torch.float32)) for k, v in g.items()))
    assert opt2.step() is True and opt2.grad_norm is not None
    assert _equal(clipped.state_dict(), plain.state_dict())
    assert not _equal(clipped.state_dict(), clf_sd)
    opt.close()
    opt2.close()


# ---------------------------------------------------------------- refold, untouched paths
def test_after_a_step_and_after_close_the_handle_is_a_fresh_load_of_the_state_dict(clf_sd):
    x, labels, w = ref.inputs(ref.CASES[2])
    probe = _probe_input()
    clf = _new_clf(clf_sd)
    opt = _adam(clf, lr=1e-3)
    clf.loss_backward(x, labels)
    assert opt.step() is True
    sd = clf.state_dict()
    names = ref.trainable_names(clf_sd)
    assert all(not torch.equal(sd[k].cpu(), clf_sd[k]) for k in names)
    assert all(torch.equal(sd[k].cpu(), clf_sd[k]) for k in clf_sd if k not in names)
    fresh_bits = _xai_bits(_new_clf(sd), probe)
    assert sp.same(_xai_bits(clf, probe), fresh_bits)
    opt.close()
    assert sp.same(_xai_bits(clf, probe), fresh_bits) and _equal(clf.state_dict(), sd)
    clf.randomize_weights(3, 0)                                # restore folds the host copies again: the trained ones
    clf.restore_weights()
    assert sp.same(_xai_bits(clf, probe), fresh_bits)


def test_train_begin_and_end_without_a_step_move_nothing(clf_sd):
    probe = _probe_input()
    clf = _new_clf(clf_sd)
    before = _xai_bits(clf, probe)
    opt = _adam(clf)
    assert sp.same(_xai_bits(clf, probe), before)
    opt.close()
    assert sp.same(_xai_bits(clf, probe), before) and _equal(clf.state_dict(), clf_sd)


# ---------------------------------------------------------------- learning
def test_learns_two_visibly_different_classes(clf_sd):
    """16 images of 64x64, two classes (dark with a bright disc / bright with a dark cross, plus noise), 30 steps at batch 16:
    the loss falls below half its first value and evaluate_classifier reports every image right"""
    from synt_isic_amd.train import evaluate_classifier
    g = torch.Generator().manual_seed(2)
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    disc = (((yy - 32) ** 2 + (xx - 32) ** 2) < 18 ** 2).float()
    cross = (((yy - 32).abs() < 6) | ((xx - 32).abs() < 6)).float()
    labels = torch.tensor([0, 1] * 8)
    images = torch.stack([(-0.6 + 1.2 * disc if y == 0 else 0.6 - 1.2 * cross).expand(3, 64, 64) for y in labels.tolist()])
    images = (images + 0.05 * torch.randn(images.shape, generator=g)).clamp(-1, 1).to(DEV)
    clf = _new_clf(clf_sd)
    opt = _adam(clf, lr=1e-3)
    losses = []
    for _ in range(30):
        loss, _ = clf.loss_backward(images, labels)
        assert opt.step() is True
        losses.append(loss)
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0], losses
    res = evaluate_classifier(clf, [(images[:10], labels[:10]), (images[10:], labels[10:])])
    assert res["accuracy"] == 1.0 and res["balanced_accuracy"] == 1.0
    assert res["confusion_matrix"][0, 0] == 8 and res["confusion_matrix"][1, 1] == 8 and int(res["confusion_matrix"].sum()) == 16
    opt.close()


def test_train_classifier_over_a_device_loader_saves_a_loadable_checkpoint(clf_sd, tmp_path):
    """train_classifier over data.DeviceLoader with "balanced" weights: the history, the closed optimizer, classifier.pth under the
    reference's keys whose fresh load gives the trained model's bits, and evaluate_classifier with augmentation off"""
    from synt_isic_amd import data, train
    g = torch.Generator().manual_seed(4)
    labels = torch.tensor([1] * 10 + [0] * 4 + [5] * 2)                       # unbalanced: 10 / 4 / 2
    base = torch.tensor([200, 40, 0, 0, 0, 120])[labels].view(16, 1, 1, 1)      # one grey level per class, plus noise
    images = (base + torch.randint(-20, 21, (16, 64, 64, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    ds = data.DeviceDataset(images, DEV, labels=labels)
    w = train.balanced_class_weights(ds.labels, 7)
    assert torch.allclose(w, torch.tensor([16 / 28, 16 / 70, 0, 0, 0, 16 / 14, 0]))
    clf = _new_clf(clf_sd)
    lines = []
    history = train.train_classifier(clf, data.DeviceLoader(ds, 8, seed=1), epochs=2, lr=1e-4, class_weights="balanced",
                                     val_loader=data.DeviceLoader(ds, 16, seed=2), save_dir=str(tmp_path), max_grad_norm=5.0,
                                     log=lines.append)
    assert len(history) == 2 and len(lines) == 2 and all(math.isfinite(h["loss"]) and 0.0 <= h["balanced_accuracy"] <= 1.0 for h in history)
    assert clf._trainer is None                                               # the loop closed its optimizer
    saved = torch.load(os.path.join(str(tmp_path), "classifier.pth"))
    assert list(saved) == list(clf_sd) and all(k.startswith("model.") and v.device.type == "cpu" for k, v in saved.items())
    names = ref.trainable_names(clf_sd)
    assert all(torch.equal(saved[k], clf_sd[k]) for k in clf_sd if k not in names)
    assert all(not torch.equal(saved[k], clf_sd[k]) for k in names)
    best = max(range(2), key=lambda i: history[i]["balanced_accuracy"])       # the first of equal scores is kept
    if best == 1:                                                             # the file is the model as it stands
        assert sp.same(_xai_bits(_new_clf(saved), _probe_input()), _xai_bits(clf, _probe_input()))
    # augmentation off and dataset order, whatever the loader's own settings
    a = train.evaluate_classifier(clf, data.DeviceLoader(ds, 5, seed=3, augment=True, shuffle=True))
    b = train.evaluate_classifier(clf, data.DeviceLoader(ds, 16, augment=False, shuffle=False))
    assert torch.equal(a["confusion_matrix"], b["confusion_matrix"]) and int(a["confusion_matrix"].sum()) == 16
    assert a["confusion_matrix"].sum(1).tolist() == [4, 10, 0, 0, 0, 2, 0]
    pred = clf.predict(next(iter(data.DeviceLoader(ds, 16, augment=False, shuffle=False)))[0]).cpu()
    assert a["accuracy"] == (pred == labels).float().mean().item()


# ---------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(clf_sd):
    from synt_isic_amd import _lib
    from synt_isic_amd._lib import SisicError
    x, labels, _ = ref.inputs(ref.CASES[0])
    clf = _new_clf(clf_sd)
    with pytest.raises(SisicError, match="train_begin"):          # no optimizer yet
        clf.loss_backward(x, labels, preprocessed=True)
    a = _lib.ResnetTrainArgs()
    a.lr, a.beta1, a.beta2, a.eps = 1e-4, 0.9, 0.999, 1e-8
    assert _lib.load().sisic_resnet_optimizer_step(clf.handle, C.byref(a)) == _lib.SISIC_ESTATE
    assert b"train_begin" in _lib.load().sisic_last_error()
    opt = _adam(clf)
    clf.loss_backward(x, labels, preprocessed=True)
    held = clf.grads()
    with pytest.raises(SisicError, match="label 7"):
        clf.loss_backward(x, torch.tensor([0, 7]), preprocessed=True)
    with pytest.raises(SisicError, match="label -1"):
        clf.loss_backward(x, torch.tensor([-1, 2]), preprocessed=True)
    for H, W in [(36, 32), (32, 34), (32, 40)]:                    # 9 rows before layer2; a 17-column stem output; 5 columns before layer3
        with pytest.raises(SisicError, match="odd feature map"):
            clf.loss_backward(torch.zeros(2, 3, H, W), labels, preprocessed=True)
    with pytest.raises(SisicError, match="class weight"):
        clf.loss_backward(x, labels, class_weights=torch.tensor([1.0, -1.0, 1, 1, 1, 1, 1]), preprocessed=True)
    assert _equal(clf.grads(), held)                               # nothing ran: the gradients are those of the last good call
    with pytest.raises(SisicError, match="sisic_resnet_load"):
        clf.write_tensor(0, "model.fc.bias", torch.zeros(7))
    with pytest.raises(SisicError, match="frozen"):
        clf.read_tensor(1, "model.bn1.weight")
    with pytest.raises(SisicError, match="training"):
        clf.randomize_weights(1, 0)
    opt.close()
    with pytest.raises(RuntimeError, match="closed"):
        opt.step()


# ---------------------------------------------------------------- a held side stream
def test_side_stream_gives_the_default_stream_bits(clf_sd):
    """loss_backward and step on a side stream that a spin kernel holds, the images copied in behind the hold: the loss, the
    logits, every gradient and every trained tensor are the bits of the default-stream run.  Each of the three runs has a
    handle of its own, made beforehand, so that nothing between the hold and the library call waits for the device."""
    _, labels, w = ref.inputs(ref.CASES[1])
    pairs = []
    for _ in range(3):
        clf = _new_clf(clf_sd)
        pairs.append((clf, _adam(clf, lr=1e-3, max_grad_norm=1.0)))
    torch.cuda.synchronize()
    todo = list(pairs)

    def fn(x):
        clf, opt = todo.pop(0)
        loss, logits = clf.loss_backward(x, labels, class_weights=w, preprocessed=True)
        ok = opt.step()
        return loss, logits, ok, opt.grad_norm, clf.grads(), clf.state_dict()

    baseline, held, _ = sp.run_held(fn, lambda: [ref.inputs(ref.CASES[1])[0].to(DEV)],
                                    lambda: [torch.randn(3, 3, 64, 96, generator=torch.Generator().manual_seed(1)).to(DEV)],
                                    "classifier loss_backward + step")
    assert baseline[2] is True and sp.same(baseline, held)
    for _, opt in pairs:
        opt.close()
