"""Counterfactual interventions and causal-shift metrics on the GPU (sisic_intervene, sisic_cfi_metrics and the stage built on
them in synt_isic_amd.xai) against the float64 restatement of tests/xai_ref.py.

Bounds.  'zero', 'noise' and 'shuffle' are bit-equal to the same fp32 torch expressions (the blend multiplies by 0 or 1).
'blur', 'inpaint', 'mean', 'gaussian_noise' and the four statistics: max-abs <= 1e-5 * max(1, |ref|_inf) against float64, the
project's per-kernel bound (these are sums of at most 961 O(1) terms).  The metrics: every float field <= 1e-5 * max(1, |ref|)
against float64 computed from the same fp32 logits; argmax ids exactly (every row has a top-2 gap >= 1e-3).  The stage's
probabilities: 2e-4 against the CPU oracle classifier applied to the restatement's images, the tolerance of the logits."""
import os

import numpy as np
import pytest
import torch

import xai_ref

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NV = 1
TOL = 1e-5


def _close(got, ref, tol, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    bound = tol * max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    print(f"{what}: err {err:.3e} (bound {bound:.3e})")
    assert got.shape == ref.shape and err <= bound, f"{what}: err {err:.3e} > {bound:.3e} (shape {tuple(got.shape)})"


@pytest.fixture(scope="module")
def regions(golden_dir):
    return xai_ref.load_region_fixture(os.path.join(golden_dir, "xai_regions.npz"))


@pytest.fixture(scope="module")
def clf_sd():
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    return synthetic_resnet18_state_dict()


@pytest.fixture(scope="module")
def clf(clf_sd):
    from synt_isic_amd.classifier import HipMelanomaClassifier
    return HipMelanomaClassifier(num_classes=7, pretrained=False).load_state_dict(dict(clf_sd)).to(DEV).eval()


def _masks(regions, H, W):
    """two region masks of the fixture (cut to H x W), an empty one and a full one: bool [4,H,W]"""
    src = 64 if max(H, W) <= 64 else 128
    top = regions[(0, src, 9, "top", 8, True)][0][:H, :W]
    bottom = regions[(1, src, 15, "bottom", 8, True)][0][:H, :W]
    assert 0 < top.sum() < H * W and 0 < bottom.sum() < H * W
    return torch.from_numpy(np.stack([top, bottom, np.zeros((H, W), bool), np.ones((H, W), bool)]))


# (frame, mask, type, blur kernel, noise std): all seven types, three frames, four masks, in one table
JOBS = [
    (0, 0, "noise", 0, 0.5), (1, 1, "gaussian_noise", 0, 0.5), (2, 0, "gaussian_noise", 0, 2.0), (0, 1, "zero", 0, 0.0),
    (1, 0, "mean", 0, 0.0), (2, 1, "blur", 3, 0.0), (0, 0, "blur", 4, 0.0), (1, 1, "blur", 5, 0.0), (2, 0, "blur", 31, 0.0),
    (0, 1, "inpaint", 0, 0.0), (1, 0, "shuffle", 0, 0.0), (2, 1, "shuffle", 0, 0.0), (0, 2, "blur", 5, 0.0),
    (1, 3, "blur", 31, 0.0), (2, 3, "noise", 0, 0.25), (0, 2, "shuffle", 0, 0.0), (1, 3, "mean", 0, 0.0), (2, 3, "zero", 0, 0.0),
    (0, 3, "shuffle", 0, 0.0), (1, 2, "gaussian_noise", 0, 0.5),
]
EXACT = ("zero", "noise", "shuffle")


def _setup(regions, H, W, seed=0):
    from synt_isic_amd import ops
    frames = torch.randn(3, 3, H, W, generator=torch.Generator().manual_seed(100 + seed + H)) * 1.5
    masks = _masks(regions, H, W)
    seeds = [1000 + 7 * j for j in range(len(JOBS))]
    src = torch.stack([xai_ref.shuffle_index(masks[m], 3, seeds[j]) for j, (_, m, *_r) in enumerate(JOBS)]).to(torch.int32)
    z = ops.noise_fill(seeds, 3 * H * W, 0, tag=2, device=DEV).cpu().view(len(JOBS), 3, H, W)
    return frames, masks, seeds, src, z


def _run(frames, masks, jobs, seeds, src, with_intervention=True):
    from synt_isic_amd import ops
    return ops.intervene(frames.to(DEV), masks.to(torch.uint8).to(DEV), jobs, seeds,
                         src_index=None if src is None else src.contiguous().to(DEV), with_intervention=with_intervention)


@pytest.mark.parametrize("H,W", [(64, 64), (128, 128), (96, 40), (30, 70)])
def test_intervene_matches_restatement(regions, H, W):
    frames, masks, seeds, src, z = _setup(regions, H, W)
    assert frames.abs().max() > 1.0                           # the clamp bites outside the masks too
    out, iv, stats = _run(frames, masks, JOBS, seeds, src)
    assert out.shape == iv.shape == (len(JOBS), 3, H, W) and stats.shape == (len(JOBS), 4)
    out, iv, stats = out.cpu(), iv.cpu(), stats.cpu()
    for j, (f, m, kind, k, std) in enumerate(JOBS):
        what = f"{H}x{W} job {j} {kind} k={k} frame {f} mask {m}"
        kw = dict(blur_kernel=k, noise_std=std, z=z[j], src_index=src[j])
        mod64, iv64, st64 = xai_ref.intervene(frames[f], masks[m], kind, **kw)
        if kind in EXACT:
            mod32, iv32, _ = xai_ref.intervene(frames[f], masks[m], kind, dtype=torch.float32, **kw)
            assert torch.equal(iv[j], iv32), f"{what}: intervention is not bit-equal to fp32 torch"
            assert torch.equal(out[j], mod32), f"{what}: modified image is not bit-equal to fp32 torch"
        else:
            _close(iv[j], iv64, TOL, what + " intervention")
            _close(out[j], mod64, TOL, what + " modified")
        _close(stats[j], st64, TOL, what + " stats")
        # the blend is exact: outside the mask the clamped image, inside the clamped intervention, bit for bit
        mm = masks[m][None].expand(3, H, W)
        assert torch.equal(out[j][~mm], frames[f].clamp(-1, 1)[~mm]), what
        assert torch.equal(out[j][mm], iv[j].clamp(-1, 1)[mm]), what
    # without intervention_out the images and statistics are the same
    out2, none, stats2 = _run(frames, masks, JOBS, seeds, src, with_intervention=False)
    assert none is None and torch.equal(out2.cpu(), out) and torch.equal(stats2.cpu(), stats)


def test_noise_is_the_device_noise_contract(regions):
    """the two noise types draw sisic_noise_fill(seed, step 0, tag 2): a pure function of (seed, element)"""
    from synt_isic_amd import ops
    for (H, W) in ((30, 70), (31, 33)):                       # 3*30*70 floats are whole Philox blocks, 3*31*33 are not
        frames = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(5))
        full = torch.ones(1, H, W, dtype=torch.bool)
        seeds = [2**63 + 11, 3]
        jobs = [(0, 0, "noise", 0, 0.5), (1, 0, "noise", 0, 0.125)]
        _, iv, _ = _run(frames, full, jobs, seeds, None)
        z = ops.noise_fill(seeds, 3 * H * W, 0, tag=2, device=DEV).view(2, 3, H, W)
        assert torch.equal(iv[0], z[0] * 0.5) and torch.equal(iv[1], z[1] * 0.125)
        assert not torch.equal(z, ops.noise_fill(seeds, 3 * H * W, 0, tag=0, device=DEV).view(2, 3, H, W))


def test_jobs_are_independent_and_deterministic(regions):
    H, W = 96, 40
    frames, masks, seeds, src, _ = _setup(regions, H, W)
    out, iv, stats = _run(frames, masks, JOBS, seeds, src)
    again = _run(frames, masks, JOBS, seeds, src)
    assert torch.equal(out, again[0]) and torch.equal(iv, again[1]) and torch.equal(stats, again[2])
    # the table reversed: every job's result moves with it
    order = list(range(len(JOBS)))[::-1]
    r = _run(frames, masks, [JOBS[j] for j in order], [seeds[j] for j in order], src[order])
    assert torch.equal(r[0], out[order]) and torch.equal(r[1], iv[order]) and torch.equal(r[2], stats[order])
    # one job on its own, with only its frame and its mask
    for j in (0, 2, 4, 8, 10, 13):
        f, m, kind, k, std = JOBS[j]
        one = _run(frames[f:f + 1], masks[m:m + 1], [(0, 0, kind, k, std)], [seeds[j]], src[j:j + 1])
        assert torch.equal(one[0][0], out[j]) and torch.equal(one[1][0], iv[j]) and torch.equal(one[2][0], stats[j]), JOBS[j]
    # more jobs than one launch carries
    many = [JOBS[j % len(JOBS)] for j in range(70)]
    r = _run(frames, masks, many, [seeds[j % len(JOBS)] for j in range(70)], src[[j % len(JOBS) for j in range(70)]])
    assert torch.equal(r[0][:len(JOBS)], out) and torch.equal(r[0][60:70], out[0:10]) and torch.equal(r[2][60:70], stats[0:10])


def _cfi_inputs():
    g = torch.Generator().manual_seed(77)
    lo = torch.randn(6, 7, generator=g) * 2
    lm = torch.randn(16, 7, generator=g) * 2
    job_frame = [j % 6 for j in range(16)]
    lm[3] = lo[job_frame[3]]                                  # an identical pair: every shift is 0
    lo[4] = torch.tensor([0.3, 40.5, -0.2, 0.1, 0.5, -0.4, 0.0])       # a 40-logit gap: p + 1e-8 = 1e-8 in fp32
    lm[7] = torch.tensor([0.2, -0.1, 40.3, 0.0, 0.4, -0.3, 0.1])
    lo[5] = torch.tensor([0.3, 0.1, -0.2, 120.0, 0.5, -0.4, 0.0])      # a 120-logit gap: p = 0 in fp32
    lm[9] = torch.tensor([120.5, -0.1, 0.3, 0.0, 0.4, -0.3, 0.1])
    for rows in (lo, lm):
        top2 = rows.topk(2, dim=1).values
        assert (top2[:, 0] - top2[:, 1]).min() >= 1e-3
    return lo, lm, job_frame


def test_cfi_metrics_match_float64():
    from synt_isic_amd import ops
    lo, lm, job_frame = _cfi_inputs()
    n = 7
    rows = ops.cfi_metrics(lo.to(DEV), lm.to(DEV), job_frame).cpu()
    ref = xai_ref.cfi_rows(lo, lm, job_frame)
    assert rows.shape == (16, 6 * n + 7)
    names = ["orig_score", "mod_score", "cfi", "delta", "p_orig", "p_mod"]
    for j in range(16):
        for c in range(n):
            for i, name in enumerate(names):
                got, want = rows[j, 6 * c + i].double().item(), ref[j, 6 * c + i].item()
                assert abs(got - want) <= TOL * max(1.0, abs(want)), f"job {j} class {c} {name}: {got} vs {want}"
        tail, rt = rows[j, 6 * n:].double(), ref[j, 6 * n:]
        assert tail[0] == rt[0] and tail[1] == rt[1], f"job {j}: argmax {tail[:2].tolist()} vs {rt[:2].tolist()}"
        for i, name in zip(range(2, 7), ["max p_orig", "max p_mod", "KL", "JS", "TV"]):
            assert abs(tail[i] - rt[i]) <= TOL * max(1.0, abs(rt[i].item())), f"job {j} {name}: {tail[i]} vs {rt[i]}"
    # the identical pair; the gaps
    assert rows[3, 2::6][:n].abs().max() == 0 and rows[3, 6 * n + 4:].abs().max() <= 1e-6
    assert abs(rows[7, 6 * 0 + 1].item() - np.log(1e-8)) < 1e-4
    assert rows[9, 6 * 1 + 5].item() == 0.0 and rows[5, 6 * 0 + 4].item() == 0.0        # p = 0 exactly behind the 120 gap
    err = np.abs(rows.double().numpy() - ref.numpy()) / np.maximum(1.0, np.abs(ref.numpy()))
    print(f"cfi metrics: worst scaled error {err.max():.3e}")


def _flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flatten(v, f"{prefix}{k}."))
        elif isinstance(v, list):
            for i, e in enumerate(v):
                out.update(_flatten(e, f"{prefix}{k}[{i}]."))
        else:
            out[prefix + k] = v
    return out


def test_intervention_stage_end_to_end(clf, clf_sd):
    from oracle import resnet18 as ores
    from synt_isic_amd import ops, xai
    H = W = 64
    n = 6
    g = torch.Generator().manual_seed(9)
    trajectory = [torch.randn(1, 3, H, W, generator=g) * (1.5 - 0.2 * i) for i in range(n)]
    timesteps = [500.0 - 100 * i for i in range(n)]
    region_data = {}
    for i in range(n):
        if i == 2:
            continue                                          # a key frame without regions is skipped
        attr = torch.nn.functional.avg_pool2d(torch.randn(1, 3, H, W, generator=g), 9, 1, 4)
        region_data[f"t_{timesteps[i]:.0f}"] = {"top_k": xai.select_regions(attr, 10, "top"),
                                                 "bottom_k": xai.select_regions(attr, 10, "bottom")}
    types = ("blur", "noise", "shuffle")
    calls = []
    real_forward = clf.forward
    clf.forward = lambda x, *a, **k: (calls.append(tuple(x.shape)), real_forward(x, *a, **k))[1]
    try:
        interventions, cfi = xai.intervention_stage(clf, [f.to(DEV) for f in trajectory], timesteps, region_data, NV,
                                                    intervention_types=types, seed=40)
    finally:
        del clf.forward
    used = [i for i in xai_ref.key_steps(n) if i != 2]                    # [0, 3, 4, 5]
    assert used == [0, 3, 4, 5]
    J = len(used) * 2 * len(types)
    assert calls == [(len(used) + J, 3, H, W)], f"classifier.forward calls: {calls}"
    assert list(interventions) == [f"t_{timesteps[i]:.0f}" for i in used] == list(cfi)

    # against the restatement + the CPU oracle classifier
    z = ops.noise_fill([40 + j for j in range(J)], 3 * H * W, 0, tag=2, device=DEV).cpu().view(J, 3, H, W)
    ref_images, labels = [], []
    j = 0
    for i in used:
        key = f"t_{timesteps[i]:.0f}"
        assert list(interventions[key]) == ["top_k", "bottom_k"]
        for region in ("top_k", "bottom_k"):
            mask = torch.from_numpy(region_data[key][region]["mask"])
            assert list(interventions[key][region]) == list(types)
            for t in types:
                mod64, iv64, st64 = xai_ref.intervene(trajectory[i][0], mask, t, blur_kernel=5, noise_std=0.5, z=z[j],
                                                      src_index=xai_ref.shuffle_index(mask, 3, 40 + j))
                entry = interventions[key][region][t]
                assert set(entry) == {"modified_image", "intervention", "mask_tensor", "difference", "statistics", "parameters"}
                assert entry["modified_image"].shape == (1, 3, H, W) and entry["mask_tensor"].shape == (1, 1, H, W)
                _close(entry["modified_image"][0], mod64, TOL, f"{key} {region} {t} modified")
                _close(entry["intervention"][0], iv64, TOL, f"{key} {region} {t} intervention")
                _close(entry["difference"][0], (trajectory[i][0].double() - mod64).abs(), TOL, f"{key} {region} {t} difference")
                s = entry["statistics"]
                assert s["intervention_type"] == t
                _close(torch.tensor([s["mask_coverage"], s["mean_difference"], s["max_difference"], s["intervention_strength"]]),
                       st64, TOL, f"{key} {region} {t} statistics")
                ref_images.append(mod64.float())
                labels.append((i, key, region, t))
                j += 1
    p_orig = torch.softmax(ores.classifier_forward(clf_sd, torch.cat([trajectory[i] for i in used])).double(), 1)
    p_mod = torch.softmax(ores.classifier_forward(clf_sd, torch.stack(ref_images)).double(), 1)
    for j, (i, key, region, t) in enumerate(labels):
        c = cfi[key][f"{region}_{t}"]
        assert set(c) == {"target_class_analysis", "prediction_analysis", "all_classes_analysis", "distribution_analysis"}
        got_o = torch.tensor([a["original_probability"] for a in c["all_classes_analysis"]])
        got_m = torch.tensor([a["modified_probability"] for a in c["all_classes_analysis"]])
        _close(got_o, p_orig[used.index(i)], 2e-4, f"{key} {region} {t} original probabilities")
        _close(got_m, p_mod[j], 2e-4, f"{key} {region} {t} modified probabilities")
        ta = c["target_class_analysis"]
        assert ta["class_id"] == NV and ta["class_name"] == "NV"
        assert abs(ta["modified_probability"] - p_mod[j, NV].item()) <= 2e-4
        assert abs(ta["cfi"] - (ta["original_score"] - ta["modified_score"])) <= 1e-5 * max(1.0, abs(ta["original_score"]))

    # item by item through the single-image functions: the same numbers
    for j, (i, key, region, t) in enumerate(labels):
        image = trajectory[i].to(DEV)
        one = xai.counterfactual_intervention(image, region_data[key][region]["mask"], t, seed=40 + j)
        entry = interventions[key][region][t]
        for k in ("modified_image", "intervention", "mask_tensor", "difference"):
            _close(one[k], entry[k], TOL, f"item {key} {region} {t} {k}")
        for k, v in one["statistics"].items():
            w = entry["statistics"][k]
            assert v == w if isinstance(v, str) else abs(v - w) <= TOL * max(1.0, abs(w)), (key, region, t, k, v, w)
        shift = _flatten(xai.compute_causal_shift(clf, image, one["modified_image"], NV))
        want = _flatten(cfi[key][f"{region}_{t}"])
        assert set(shift) == set(want)
        for k, w in want.items():
            v = shift[k]
            if isinstance(w, (str, bool, int)):
                assert v == w, (key, region, t, k, v, w)
            else:
                assert abs(v - w) <= TOL * max(1.0, abs(w)), (key, region, t, k, v, w)


def test_argument_errors_raise_and_launch_nothing(regions):
    from synt_isic_amd import ops, xai
    from synt_isic_amd._lib import SisicError
    H = W = 64
    frames = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    masks = _masks(regions, H, W).to(torch.uint8).to(DEV)
    ok = ops.intervene(frames, masks, [(0, 0, "blur", 5, 0.0)], [0])[0].clone()
    with pytest.raises(ValueError, match="masks must be"):
        ops.intervene(frames, masks[:, :32].contiguous(), [(0, 0, "blur", 5, 0.0)], [0])
    with pytest.raises(ValueError, match="masks must be"):
        ops.intervene(frames, masks.float(), [(0, 0, "blur", 5, 0.0)], [0])
    with pytest.raises(ValueError, match="does not cover"):
        xai.counterfactual_intervention(frames[:1], np.ones((32, 64), bool), "zero")
    with pytest.raises(ValueError, match="unknown intervention type"):
        ops.intervene(frames, masks, [(0, 0, "sharpen", 5, 0.0)], [0])
    with pytest.raises(ValueError, match="unknown intervention type"):
        xai.counterfactual_intervention(frames[:1], np.ones((H, W), bool), "sharpen")
    with pytest.raises(SisicError, match="unknown intervention type 7"):
        ops.intervene(frames, masks, [(0, 0, 7, 5, 0.0)], [0])
    with pytest.raises(SisicError, match="frame 2 of 2"):
        ops.intervene(frames, masks, [(0, 0, "zero", 0, 0.0), (2, 0, "zero", 0, 0.0)], [0, 1])
    with pytest.raises(SisicError, match="frame -1 of 2"):
        ops.intervene(frames, masks, [(-1, 0, "zero", 0, 0.0)], [0])
    with pytest.raises(SisicError, match="mask 4 of 4"):
        ops.intervene(frames, masks, [(0, 4, "zero", 0, 0.0)], [0])
    with pytest.raises(SisicError, match="src_index is NULL"):
        ops.intervene(frames, masks, [(0, 0, "shuffle", 0, 0.0)], [0])
    with pytest.raises(SisicError, match="blur kernel 33"):
        ops.intervene(frames, masks, [(0, 0, "blur", 33, 0.0)], [0])
    with pytest.raises(SisicError, match="blur kernel 0"):
        ops.intervene(frames, masks, [(0, 0, "blur", 0, 0.0)], [0])
    with pytest.raises(ValueError, match="seeds"):
        ops.intervene(frames, masks, [(0, 0, "zero", 0, 0.0)], [0, 1])
    logits = torch.zeros(2, 7, device=DEV)
    with pytest.raises(SisicError, match="frame 2 of 2"):
        ops.cfi_metrics(logits, logits, [0, 2])
    with pytest.raises(ValueError):
        ops.cfi_metrics(logits, logits[:, :5], [0, 1])
    # an even kernel of 32 would become 33: refused; 30 becomes 31: taken.  The device is intact after all of the above.
    ops.intervene(frames, masks, [(0, 0, "blur", 30, 0.0)], [0])
    torch.cuda.synchronize()
    assert torch.equal(ops.intervene(frames, masks, [(0, 0, "blur", 5, 0.0)], [0])[0], ok)


def test_combined_attribution(clf):
    """XAI.py:1236-1291: the weighted sum of the existing passes and the per-method details"""
    from synt_isic_amd import xai
    image = (torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 0.8).to(DEV)
    masks = xai.draw_patch_masks(8, 4, 4, generator=torch.Generator().manual_seed(4))
    base = torch.zeros_like(image)
    kw = dict(ig_kwargs={"n_steps": 4, "baseline": base}, shap_kwargs={"n_samples": 8, "patch_masks": masks})
    total, details = xai.compute_combined_attribution(clf, image, NV, methods=("ig", "shap", "gradient"), weights=(0.5, 0.3, 0.2), **kw)
    ig = xai.compute_integrated_gradients(clf, image, NV, n_steps=4, baseline=base)
    shap = xai.compute_shap_approximation(clf, image, NV, n_samples=8, patch_masks=masks)
    grad = xai.compute_gradient_attribution(clf, image, NV)
    _close(total, ig * 0.5 + shap * 0.3 + grad * 0.2, 1e-6, "combined attribution")
    assert list(details) == ["ig", "shap", "gradient"] and details["shap"]["weight"] == 0.3
    assert abs(details["ig"]["mean_attribution"] - ig.abs().mean().item()) < 1e-9
    assert abs(details["gradient"]["max_attribution"] - grad.abs().max().item()) < 1e-9
    both, d2 = xai.compute_combined_attribution(clf, image, NV, **kw)                  # ('ig', 'shap'), equal weights
    _close(both, ig * 0.5 + shap * 0.5, 1e-6, "default combination")
    assert d2["ig"]["weight"] == 0.5 and list(d2) == ["ig", "shap"]
    with pytest.raises(RuntimeError):
        xai.compute_combined_attribution(clf, image, NV, methods=("lime",))
