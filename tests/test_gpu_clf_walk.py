"""The classifier executor's one backward walk (csrc/resnet.cpp: backward_walk behind run_trunk) in its three forms on one
handle: the input gradient, training with BatchNorm frozen and training with batch statistics share the pool, the filter views
and the loop, so what one form leaves behind must not reach the next.

Shapes: (2,3,48,40) raw goes through the 224x224 resize and the pre-processing backward; (2,3,32,32) pre-processed is the smallest
plane the geometry check admits (a last plane of 1x1: B = 2 is the smallest legal BatchNorm batch); (3,3,64,96) pre-processed is
not square, so an h/w or (h,w)/(bh,bw) mix-up changes bits.  Every comparison is bit for bit: the kernels have no atomics and
the pool hands a repeated run the same blocks.
"""
import pytest
import torch

from poison import guard_bands, poison_allocations, unwritten  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CLASS_WEIGHTS = [1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 0.75]
# (shape, labels, pre-processed)
CASES = [((2, 3, 48, 40), [1, 4], False), ((2, 3, 32, 32), [0, 6], True), ((3, 3, 64, 96), [2, 5, 3], True)]
IDS = ["raw_48x40", "pre_32x32", "pre_64x96"]


@pytest.fixture(scope="module")
def clf_sd():
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    return synthetic_resnet18_state_dict()


@pytest.fixture(scope="module")
def clf(clf_sd):
    from synt_isic_amd.classifier import HipMelanomaClassifier
    return HipMelanomaClassifier(num_classes=7).load_state_dict(clf_sd).to(DEV).eval()


def _input(shape):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(shape[2] * shape[3])) * 0.8).to(DEV)


def _adam(clf, mode):
    from synt_isic_amd.train import HipClassifierAdam
    return HipClassifierAdam(clf, batchnorm=mode)


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def _running_stats(clf):
    from synt_isic_amd.arch import resnet18_buffer_names
    return {n: clf.read_tensor(0, n) for n in resnet18_buffer_names(clf.num_classes)}


@pytest.mark.parametrize("shape,labels,preprocessed", CASES, ids=IDS)
def test_input_gradient_is_unchanged_by_training_walks(clf, clf_sd, shape, labels, preprocessed):
    """input_gradient, a frozen loss_backward and a batch-statistics loss_backward (each through its own optimizer, closed without
    a step), then input_gradient again: the gradient's and the logits' bits of the first call"""
    x = _input(shape)
    clf.load_state_dict(clf_sd)
    grad0, logits0 = clf.input_gradient(x, labels)
    assert unwritten(grad0) == 0 and unwritten(logits0) == 0
    for mode in ("frozen", "batch"):
        opt = _adam(clf, mode)
        loss, logits = clf.loss_backward(x, labels, class_weights=CLASS_WEIGHTS, preprocessed=preprocessed)
        assert loss == loss and unwritten(logits) == 0
        opt.close()
    clf.load_state_dict(clf_sd)                  # the batch-statistics forward moved the running statistics
    grad1, logits1 = clf.input_gradient(x, labels)
    assert torch.equal(grad0, grad1) and torch.equal(logits0, logits1)


@pytest.mark.parametrize("shape,labels,preprocessed", CASES, ids=IDS)
def test_frozen_walk_repeats_on_the_same_blocks(clf, clf_sd, shape, labels, preprocessed):
    """a second frozen loss_backward at the same shape: no new pool block, the same loss, logits and 22 gradients"""
    x = _input(shape)
    clf.load_state_dict(clf_sd)
    opt = _adam(clf, "frozen")
    loss0, logits0 = clf.loss_backward(x, labels, class_weights=CLASS_WEIGHTS, preprocessed=preprocessed)
    grads0, bytes0 = clf.grads(), clf.workspace_bytes()
    loss1, logits1 = clf.loss_backward(x, labels, class_weights=CLASS_WEIGHTS, preprocessed=preprocessed)
    grads1, bytes1 = clf.grads(), clf.workspace_bytes()
    opt.close()
    assert len(grads0) == 22 and bytes0 > 0 and bytes1 == bytes0
    assert loss1 == loss0 and torch.equal(logits0, logits1) and _same(grads0, grads1)


@pytest.mark.parametrize("shape,labels,preprocessed", CASES, ids=IDS)
def test_batch_statistics_walk_repeats_on_the_same_blocks(clf, clf_sd, shape, labels, preprocessed):
    """a second batch-statistics loss_backward at the same shape takes no new pool block; with the running statistics restored
    by a reload it gives the same loss, logits, 62 gradients and 40 running statistics"""
    x = _input(shape)
    clf.load_state_dict(clf_sd)
    opt = _adam(clf, "batch")
    loss0, logits0 = clf.loss_backward(x, labels, class_weights=CLASS_WEIGHTS, preprocessed=preprocessed)
    grads0, stats0, bytes0 = clf.grads(), _running_stats(clf), clf.workspace_bytes()
    clf.loss_backward(x, labels, class_weights=CLASS_WEIGHTS, preprocessed=preprocessed)
    bytes1 = clf.workspace_bytes()
    assert len(grads0) == 62 and len(stats0) == 40 and bytes0 > 0 and bytes1 == bytes0
    clf.load_state_dict(clf_sd)                  # ends training: the statistics are the loaded ones again
    opt = _adam(clf, "batch")
    loss1, logits1 = clf.loss_backward(x, labels, class_weights=CLASS_WEIGHTS, preprocessed=preprocessed)
    grads1, stats1 = clf.grads(), _running_stats(clf)
    opt.close()
    assert loss1 == loss0 and torch.equal(logits0, logits1) and _same(grads0, grads1) and _same(stats0, stats1)
