"""tests/clf_bn_ref.py without a GPU: the restatement against the oracle, the conditioning cap of the GPU gradient cases, the
planted errors against the bar, and the host-side surface of the batch-statistics mode."""
import pytest
import torch

import clf_bn_ref as ref
import clf_train_ref as ctr
from oracle import resnet18 as ores


@pytest.fixture(scope="module")
def clf_sd():
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    return synthetic_resnet18_state_dict()


@pytest.fixture(scope="module")
def passes(clf_sd):
    """per case: (float64, float32) results of loss_grads_stats, both routed by the fp32 stem activation; computed once"""
    out = {}
    for case in ref.CASES:
        x, labels, w = ref.inputs(case)
        stem = ref.stem_activation(clf_sd, x, preprocessed=case[0])
        out[case] = tuple(ref.loss_grads_stats(clf_sd, x, labels, w, dt, preprocessed=case[0], stem_override=stem)
                          for dt in (torch.float64, torch.float32))
    return out


def test_eval_mode_is_the_oracle_bit_for_bit(clf_sd):
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    names, buffers = ref.trainable_names(clf_sd), ref.buffer_names(clf_sd)
    assert len(names) == 62 and len(buffers) == 40 and sorted(names + buffers) == sorted(clf_sd)
    for dt in (torch.float32, torch.float64):
        sd = {k: v.to(dt) for k, v in clf_sd.items()}
        got = ref.features({k: sd[k] for k in names}, {k: sd[k] for k in buffers}, x.to(dt), training=False)
        assert torch.equal(got, ores.resnet18_features(sd, x.to(dt)))


def test_names_follow_the_package(clf_sd):
    from synt_isic_amd.arch import resnet18_buffer_names, resnet18_trainable_names
    assert resnet18_trainable_names(7, "batch") == ref.trainable_names(clf_sd)
    assert resnet18_trainable_names(7, "frozen") == ctr.trainable_names(clf_sd)
    assert resnet18_buffer_names(7) == ref.buffer_names(clf_sd)
    with pytest.raises(ValueError):
        resnet18_trainable_names(7, "eval")


@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_every_gradient_case_is_under_the_conditioning_cap(passes, case):
    """a condition on the CASES, not a measurement of anything under test: torch's own fp32 pass stays within E32_CAP of float64
    on all 62 tensors, so that the GPU test's bar max(1e-5, 16 * e32) means something"""
    (l64, g64, s64, _), (l32, g32, s32, _) = passes[case]
    assert len(g64) == 62 and len(s64) == 40
    worst = max((ref.rel_err(g32[k], g64[k]), k) for k in g64)
    print(f"{case}: worst e32 {worst[0]:.2e} on {worst[1]}; loss {abs(l32 - l64) / abs(l64):.2e}; "
          f"running statistics {max(ref.rel_err(s32[k], s64[k]) for k in s64):.2e}")
    assert worst[0] <= ref.E32_CAP, worst


def test_the_dropped_xhat_term_is_far_over_the_bar(clf_sd, passes):
    case = ref.CASES[0]
    x, labels, w = ref.inputs(case)
    (_, g64, _, _), (_, g32, _, _) = passes[case]
    stem = ref.stem_activation(clf_sd, x, preprocessed=case[0])
    _, bad, stats, _ = ref.loss_grads_stats(clf_sd, x, labels, w, torch.float64, preprocessed=case[0], stem_override=stem,
                                            plant="no_xhat_term")
    ratios = {k: ref.rel_err(bad[k], g64[k]) / ref.bar(ref.rel_err(g32[k], g64[k])) for k in g64}
    print("no_xhat_term: over the bar by", min(ratios.values()), "..", max(ratios.values()))
    assert max(ratios.values()) >= 100.0
    assert sum(r >= 100.0 for r in ratios.values()) >= 50          # nearly every tensor sees it
    assert all(torch.allclose(stats[k], passes[case][0][2][k], rtol=1e-9, atol=1e-12) for k in stats)      # the forward is untouched


def test_the_biased_running_variance_is_far_over_the_bar(clf_sd, passes):
    case = ref.CASES[0]
    x, labels, w = ref.inputs(case)
    (_, g64, s64, _), (_, _, s32, _) = passes[case]
    stem = ref.stem_activation(clf_sd, x, preprocessed=case[0])
    _, grads, bad, _ = ref.loss_grads_stats(clf_sd, x, labels, w, torch.float64, preprocessed=case[0], stem_override=stem,
                                            plant="biased_running")
    assert all(torch.equal(grads[k], g64[k]) for k in g64)
    var = [k for k in s64 if k.endswith("running_var")]
    ratios = {k: ref.rel_err(bad[k], s64[k]) / ref.bar(ref.rel_err(s32[k], s64[k])) for k in var}
    print("biased_running: over the bar by", min(ratios.values()), "..", max(ratios.values()))
    # n = 4 at the last plane: var * n / (n - 1) is a third more there; at least the layer4 statistics are far over
    assert max(ratios.values()) >= 100.0 and sum(r >= 100.0 for r in ratios.values()) >= 5


def test_naive_fp32_moments_are_far_over_the_bar_on_the_offset_mean_operands():
    y, gamma, beta, residual, _, _, _ = ref.kernel_operands(ref.OFFSET_SHAPE, offset_mean=True)
    out64 = ref.bn_forward(y, gamma, beta, dtype=torch.float64)[0]
    out32 = ref.bn_forward(y, gamma, beta, dtype=torch.float32)[0]
    bad = ref.bn_forward(y, gamma, beta, dtype=torch.float32, plant="naive_moments")[0]
    e32, err = ref.rel_err(out32, out64), ref.rel_err(bad, out64)
    print(f"offset-mean operands: fp32 {e32:.2e}, bar {ref.bar(e32):.2e}, naive moments {err:.2e} ({err / ref.bar(e32):.0f} x)")
    assert err >= 100.0 * ref.bar(e32)


def test_kernel_shapes_fall_on_both_sides_of_the_slice_rule():
    def slices(B, C, HW):                                   # batchnorm.hip: bn_split
        segs = -(-HW // 4096)
        units = B * segs
        want = min(max(B * HW // 8192, 1), max(1, 2048 // C), units)
        return -(-units // -(-units // want))
    got = [slices(*s) for s in ref.KERNEL_SHAPES]
    assert got == ref.KERNEL_SLICES and min(got) == 1 and max(got) > 1
    assert slices(32, 64, 112 * 112) == 32                   # the stem at batch 32: 2048 workgroups


def test_bn_backward_written_out_is_autograd():
    y, gamma, beta, _, g, _, _ = ref.kernel_operands((2, 64, 49))
    yy, ga, be = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    out = torch.nn.functional.batch_norm(yy, None, None, ga, be, training=True, eps=ores.BN_EPS)
    mask = out > 0
    want = torch.autograd.grad((torch.relu(out) * g.double()).sum(), [yy, ga, be])
    got = ref.bn_backward(g, y, gamma, mask=mask)
    assert all(torch.allclose(a, b, rtol=1e-10, atol=1e-12) for a, b in zip(got, want))
    assert torch.allclose(ref.bn_forward(y, gamma, beta)[0], out.detach(), rtol=1e-10, atol=1e-12)


def test_default_init_is_an_untrained_resnet18():
    from synt_isic_amd.arch import resnet18_param_spec
    from synt_isic_amd.weights import default_init_resnet18_state_dict
    sd = default_init_resnet18_state_dict(5, 7)
    assert list(sd) == list(resnet18_param_spec(7)) and all(tuple(sd[k].shape) == s for k, s in resnet18_param_spec(7).items())
    assert all(torch.equal(v, default_init_resnet18_state_dict(5, 7)[k]) for k, v in sd.items())
    assert not torch.equal(sd["model.conv1.weight"], default_init_resnet18_state_dict(6, 7)["model.conv1.weight"])
    for k, v in sd.items():
        if v.dim() == 4:                                     # kaiming normal, fan-out: std = sqrt(2 / (cout k k))
            std = (2.0 / (v.shape[0] * v.shape[2] * v.shape[3])) ** 0.5
            assert abs(v.std().item() / std - 1.0) < 0.05 and abs(v.mean().item()) < 0.05 * std * 3, k
        elif k.endswith("running_var") or (k.endswith(".weight") and v.dim() == 1):
            assert bool((v == 1).all()), k
        elif k.endswith("running_mean") or ("bn" in k or "downsample.1" in k):
            assert bool((v == 0).all()), k
    bound = 1.0 / 512 ** 0.5
    assert sd["model.fc.weight"].abs().max() <= bound and sd["model.fc.bias"].abs().max() <= bound
    assert sd["model.fc.weight"].std() > 0.5 * bound


def test_host_side_surface_of_the_mode():
    from synt_isic_amd.classifier import HipMelanomaClassifier
    clf = HipMelanomaClassifier(num_classes=7)
    assert len(clf.trainable_names()) == 22 and clf.trainable_names("frozen") == clf.trainable_names()
    assert len(clf.trainable_names("batch")) == 62
    with pytest.raises(ValueError):
        clf.trainable_names("running")
    with pytest.raises(NotImplementedError, match="batch-statistics"):
        clf.train(True)
    # num_batches_tracked entries of a loaded dict come back from state_dict(), each behind its running_var
    from synt_isic_amd.weights import default_init_resnet18_state_dict
    sd = default_init_resnet18_state_dict(0, 7)
    full = {}
    for k, v in sd.items():
        full[k] = v
        if k.endswith("running_var"):
            full[k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(3)
    clf.load_state_dict(full)
    back = clf.state_dict()
    assert list(back) == list(full) and int(back["model.bn1.num_batches_tracked"]) == 3
    clf.load_state_dict(sd)
    assert list(clf.state_dict()) == list(sd)
