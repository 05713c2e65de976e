"""Weight randomisation on the device (sisic_resnet_randomize / sisic_resnet_restore) and ``xai.sanity_check``.

After ``randomize_weights(s, t, 0.01)`` the handle holds the folded bits that loading ``randomized_state_dict(s, t, 0.01)`` into
a second classifier leaves, and both run the same kernels: logits and input gradients are ``torch.equal``.  Against the CPU
oracle on that state dict the logits keep the existing tolerance, 2e-4 * max(1, |ref|).  ``restore_weights`` gives the original
bits back.  The correlations ``sanity_check`` reports are within 1e-10 of numpy's float64 ``corrcoef`` over maps computed here
with the public pieces and the documented seeds: three float64 sums of n <= 49 152 terms each, about 3 n 2^-53 = 1.6e-11."""
import numpy as np
import pytest
import torch

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NV = 1
H = W = 32


@pytest.fixture(scope="module")
def clf_sd():
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    return synthetic_resnet18_state_dict()


def _classifier(sd):
    from synt_isic_amd.classifier import HipMelanomaClassifier
    return HipMelanomaClassifier(num_classes=7, pretrained=False).load_state_dict(dict(sd)).to(DEV).eval()


@pytest.fixture(scope="module")
def clf(clf_sd):
    return _classifier(clf_sd)


@pytest.fixture(scope="module")
def images():
    return (torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)


@pytest.fixture(scope="module")
def original(clf, images):
    grad, logits = clf.input_gradient(images, NV)
    return clf.forward(images).clone(), grad.clone(), logits.clone()


@pytest.mark.parametrize("seed,trial", [(0, 0), (12345, 1)])
def test_randomize_equals_loading_the_randomized_state_dict(clf, clf_sd, images, original, seed, trial):
    from oracle import resnet18 as ores
    from synt_isic_amd import ops
    rsd = clf.randomized_state_dict(seed, trial, 0.01)
    assert set(rsd) == set(clf_sd)
    for name, value in clf_sd.items():
        if value.dim() > 1:
            assert not torch.equal(rsd[name].cpu(), value), name
            assert tuple(rsd[name].shape) == tuple(value.shape) and 0.008 < rsd[name].std().item() < 0.012, name
        else:
            assert torch.equal(rsd[name].cpu(), value), name
    # tensor 0 of the library is the stem weight (sisic_resnet_tensor_name): its values are the documented noise_fill bits
    w0 = ops.noise_fill([seed], 64 * 3 * 49, trial, tag=16, device=DEV)[0] * 0.01
    assert torch.equal(rsd["model.conv1.weight"].reshape(-1), w0)
    assert clf.state_dict()["model.conv1.weight"].cpu().equal(clf_sd["model.conv1.weight"])

    second = _classifier({k: v.cpu() for k, v in rsd.items()})
    try:
        clf.randomize_weights(seed, trial, 0.01)
        logits = clf.forward(images)
        grad, glogits = clf.input_gradient(images, NV)
        cam = clf.grad_cam(images, NV)[0]
        want_grad, want_glogits = second.input_gradient(images, NV)
        assert torch.equal(logits, second.forward(images))
        assert torch.equal(grad, want_grad) and torch.equal(glogits, want_glogits)
        assert torch.equal(cam, second.grad_cam(images, NV)[0])
        assert not torch.equal(logits, original[0]) and not torch.equal(grad, original[1])
        ref = ores.classifier_forward({k: v.cpu() for k, v in rsd.items()}, images.cpu())
        err = (logits.cpu() - ref).abs().max().item()
        bound = 2e-4 * max(1.0, ref.abs().max().item())
        print(f"seed {seed} trial {trial}: logits vs oracle {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert clf.state_dict()["model.conv1.weight"].cpu().equal(clf_sd["model.conv1.weight"])     # the loaded weights
    finally:
        clf.restore_weights()
    grad, glogits = clf.input_gradient(images, NV)
    assert torch.equal(clf.forward(images), original[0]) and torch.equal(grad, original[1]) and torch.equal(glogits, original[2])


def test_trials_differ_and_a_load_clears_the_randomisation(clf_sd, images, original):
    c = _classifier(clf_sd)
    c.randomize_weights(0, 0, 0.01)
    a = c.forward(images).clone()
    c.randomize_weights(0, 1, 0.01)
    b = c.forward(images).clone()
    c.randomize_weights(0, 0, 0.01)
    assert torch.equal(c.forward(images), a) and not torch.equal(a, b)          # a function of (seed, trial), not of the history
    c.randomize_weights(1, 0, 0.01)
    assert not torch.equal(c.forward(images), a)
    c.load_state_dict(dict(clf_sd))
    assert torch.equal(c.forward(images), original[0])


def _corr(a, b):
    return np.corrcoef(a.detach().cpu().numpy().astype(np.float64).ravel(), b.detach().cpu().numpy().astype(np.float64).ravel())[0, 1]


@pytest.mark.parametrize("seed,target", [(0, NV), (12345, 4)])
def test_sanity_check(clf, images, original, seed, target):
    from synt_isic_amd import xai
    image = images[:1]
    n_trials, steps, aux = 2, 4, 3
    res = xai.sanity_check(clf, image, target, n_trials=n_trials, randomization_strength=0.01, seed=seed, ig_steps=steps,
                           ig_steps_aux=aux)
    assert set(res) == {"weight_randomization_test", "input_independence_test", "model_sensitivity_test",
                        "overall_sanity_score", "overall_interpretation"}
    grad, _ = clf.input_gradient(images, NV)
    assert torch.equal(clf.forward(images), original[0]) and torch.equal(grad, original[1]), "weights not restored"

    def base(c, img):
        return xai.make_baseline(img, "noise", torch.Generator().manual_seed(seed + c))

    def ig(img, cls, n, baseline):
        return xai.compute_integrated_gradients(clf, img, cls, n_steps=n, baseline=baseline)

    c = 0
    orig = ig(image, target, steps, base(c, image))
    want_random = []
    for t in range(n_trials):
        c += 1
        clf.randomize_weights(seed, t, 0.01)
        try:
            m = ig(image, target, steps, base(c, image))
        finally:
            clf.restore_weights()
        r = _corr(orig, m)
        want_random.append(0.0 if np.isnan(r) else abs(r))
    inputs = torch.cat([torch.randn(image.shape, generator=torch.Generator().manual_seed(seed + 1000 + j)) for j in range(3)]).to(DEV)
    baselines = torch.cat([base(c + 1 + j, image) for j in range(3)])
    c += 3
    maps = ig(inputs, target, aux, baselines)
    want_indep = [abs(_corr(maps[i], maps[j])) for i in range(3) for j in range(i + 1, 3)]
    want_indep = [r for r in want_indep if not np.isnan(r)]
    want_classes = []
    for other in range(3):
        if other != target:
            c += 1
            r = _corr(orig, ig(image, other, aux, base(c, image)))
            if not np.isnan(r):
                want_classes.append(abs(r))

    t1, t2, t3 = res["weight_randomization_test"], res["input_independence_test"], res["model_sensitivity_test"]
    got = t1["correlations_per_trial"] + t2["independence_correlations"] + t3["different_class_correlations"]
    want = want_random + want_indep + want_classes
    print(f"seed {seed}: correlations {got}")
    assert len(t1["correlations_per_trial"]) == n_trials and len(t2["independence_correlations"]) == len(want_indep)
    assert len(t3["different_class_correlations"]) == len(want_classes) == (2 if target < 3 else 3)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)
    assert any(r > 1e-6 for r in got), "every correlation is zero: the maps are degenerate"

    assert t1["threshold"] == 0.1 and t2["threshold"] == 0.3 and t3["threshold"] == 0.8
    assert t1["n_trials"] == n_trials and t2["n_independent_inputs"] == 3 and t3["classes_tested"] == len(want_classes)
    assert t1["mean_correlation_with_random"] == np.mean(t1["correlations_per_trial"])
    assert t2["mean_correlation_between_independent"] == (np.mean(t2["independence_correlations"]) if want_indep else 0.0)
    assert t3["mean_correlation_different_classes"] == (np.mean(t3["different_class_correlations"]) if want_classes else 1.0)
    assert t1["test_passed"] == (t1["mean_correlation_with_random"] < 0.1)
    assert t2["test_passed"] == (t2["mean_correlation_between_independent"] < 0.3)
    assert t3["test_passed"] == (t3["mean_correlation_different_classes"] < 0.8)
    score = (int(t1["test_passed"]) + int(t2["test_passed"]) + int(t3["test_passed"])) / 3
    assert res["overall_sanity_score"] == score
    assert res["overall_interpretation"] == ("good" if score >= 0.67 else "moderate" if score >= 0.33 else "poor")


def test_sanity_check_restores_after_an_error(clf, images, original, monkeypatch):
    """an error raised while the weights are randomised propagates, and the weights are back"""
    from synt_isic_amd import xai
    real, calls = xai.compute_integrated_gradients, []

    def failing(*args, **kwargs):
        calls.append(1)
        if len(calls) == 2:                              # the first trial's map: the classifier is randomised
            raise RuntimeError("stopped in trial 0")
        return real(*args, **kwargs)

    monkeypatch.setattr(xai, "compute_integrated_gradients", failing)
    with pytest.raises(RuntimeError, match="stopped in trial 0"):
        xai.sanity_check(clf, images[:1], NV, n_trials=1, ig_steps=2, ig_steps_aux=2)
    assert torch.equal(clf.forward(images), original[0])
