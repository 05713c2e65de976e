"""Stage 1 as a stage (``xai.attribution_stage``) and the driver (``xai.run_pipeline``) on a 7-frame 32x32 trajectory with the
synthetic classifier.  Nothing here has a tolerance: a stage's output IS what its documented pieces return for the documented
generators, and the driver's entries ARE what the stages return for its seed."""
import numpy as np
import pytest
import torch

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NV = 1
H = W = 32
N_FRAMES = 7
IG_STEPS, SHAP_SAMPLES = 8, 32
TYPES = ("blur", "noise")
SEED = 12345

REFERENCE_KEYS = {"metadata", "xai_maps", "region_analysis", "interventions", "cfi_analysis", "time_shap",
                  "statistical_validation", "sanity_checks", "visualizations", "gradcam", "gradcam_most_important",
                  "gradcam_summary"}


@pytest.fixture(scope="module")
def clf():
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    return HipMelanomaClassifier(num_classes=7, pretrained=False).load_state_dict(synthetic_resnet18_state_dict()).to(DEV).eval()


@pytest.fixture(scope="module")
def trajectory():
    """smooth frames (a noisy start that settles), so that the regions survive the morphological clean-up"""
    g = torch.Generator().manual_seed(3)
    base = torch.nn.functional.avg_pool2d(torch.randn(N_FRAMES, 3, H + 8, W + 8, generator=g), 9, stride=1)
    base = base / base.abs().amax(dim=(1, 2, 3), keepdim=True)
    noise = torch.randn(N_FRAMES, 3, H, W, generator=g) * torch.linspace(0.8, 0.0, N_FRAMES).view(-1, 1, 1, 1)
    return (base + noise).to(DEV)


TIMESTEPS = [999.0, 800.0, 600.0, 400.0, 200.0, 50.0, 0.0]


@pytest.fixture(scope="module")
def stage1(clf, trajectory):
    from synt_isic_amd import xai
    return xai.attribution_stage(clf, trajectory, TIMESTEPS, NV, ig_steps=IG_STEPS, shap_samples=SHAP_SAMPLES, seed=SEED)


@pytest.fixture(scope="module")
def report(clf, trajectory):
    from synt_isic_amd import xai
    return xai.run_pipeline(clf, trajectory, TIMESTEPS, NV, "NV", seed=SEED, intervention_types=TYPES, ig_steps=IG_STEPS,
                            shap_samples=SHAP_SAMPLES)


def _same(a, b, path=""):
    """two result trees hold the same values (tensors and arrays bit for bit); wall-clock stamps aside"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            if k != "analysis_timestamp":
                _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b, equal_nan=True), path
    elif isinstance(a, float) and np.isnan(a):
        assert np.isnan(b), path
    else:
        assert a == b, path


def test_attribution_stage_is_the_combined_attribution(clf, trajectory, stage1):
    from synt_isic_amd import xai
    xai_maps, region_data = stage1
    keys = [f"t_{t:.0f}" for t in TIMESTEPS]
    assert list(xai_maps) == keys and list(region_data) == keys
    nonempty = 0
    for i, key in enumerate(keys):
        g_ig = torch.Generator().manual_seed(SEED + 2 * i)
        masks = xai.draw_patch_masks(SHAP_SAMPLES, H // 16, W // 16, torch.Generator().manual_seed(SEED + 2 * i + 1))
        want, details = xai.compute_combined_attribution(clf, trajectory[i:i + 1], NV, ("ig", "shap"), [0.5, 0.5],
                                                         ig_kwargs={"n_steps": IG_STEPS, "generator": g_ig},
                                                         shap_kwargs={"n_samples": SHAP_SAMPLES, "patch_masks": masks})
        entry = xai_maps[key]
        assert set(entry) == {"timestep", "attribution_map", "method_details", "image_shape"}
        assert torch.equal(entry["attribution_map"], want), key
        assert entry["method_details"] == details and set(details) == {"ig", "shap"} and details["ig"]["weight"] == 0.5
        assert entry["timestep"] == TIMESTEPS[i] and entry["image_shape"] == (1, 3, H, W)
        assert set(region_data[key]) == {"top_k", "bottom_k"}
        for name, rt in (("top_k", "top"), ("bottom_k", "bottom")):
            _same(region_data[key][name], xai.select_regions(want, k_percent=10, region_type=rt), f"{key}/{name}")
            nonempty += int(region_data[key][name]["mask"].sum() > 0)
    print(f"{nonempty} of {2 * N_FRAMES} regions are non-empty after the clean-up")
    assert nonempty >= 1, "every region is empty: the trajectory does not exercise the stage"
    assert not torch.equal(xai_maps[keys[0]]["attribution_map"], xai_maps[keys[1]]["attribution_map"])


def test_pipeline_report(clf, trajectory, stage1, report):
    from synt_isic_amd import xai
    assert set(report) == REFERENCE_KEYS
    assert report["visualizations"] == []
    meta = report["metadata"]
    assert meta["target_class_id"] == NV and meta["target_class_name"] == "NV" and meta["n_timesteps"] == N_FRAMES
    assert meta["timesteps"] == TIMESTEPS and meta["seed"] == SEED
    assert meta["parameters"] == {"top_k_percent": 10, "bottom_k_percent": 10, "ig_n_steps": IG_STEPS,
                                  "shap_n_samples": SHAP_SAMPLES, "intervention_types": list(TYPES), "alpha_level": 0.1}
    _same(report["xai_maps"], stage1[0], "xai_maps")
    _same(report["region_analysis"], stage1[1], "region_analysis")

    interventions, cfi = xai.intervention_stage(clf, trajectory, TIMESTEPS, stage1[1], NV, TYPES, seed=SEED)
    _same(report["cfi_analysis"], cfi, "cfi_analysis")
    _same(report["interventions"], interventions, "interventions")
    n_key = len(xai.key_steps(N_FRAMES))
    assert n_key == 5 and len(cfi) == n_key            # key_steps(7) = 0, 3, 4, 5, 6: the middle frame is also the fourth from the end
    assert all(len(v) == 2 * len(TYPES) for v in cfi.values())

    top = [e["target_class_analysis"]["cfi"] for step in cfi.values() for k, e in step.items() if "top_k" in k]
    bottom = [e["target_class_analysis"]["cfi"] for step in cfi.values() for k, e in step.items() if "bottom_k" in k]
    assert len(top) == len(bottom) == n_key * len(TYPES)
    _same(report["statistical_validation"], xai.statistical_validation(top, bottom, seed=SEED), "statistical_validation")

    importance, raw = xai.compute_time_shap(clf, trajectory, TIMESTEPS, NV)
    ts = report["time_shap"]
    assert set(ts) == {"importance", "raw_data", "most_important_timestep", "most_important_index"}
    assert np.array_equal(ts["importance"], importance) and ts["most_important_index"] == int(np.argmax(importance))
    assert ts["most_important_timestep"] == TIMESTEPS[ts["most_important_index"]]
    cams = xai.compute_grad_cam(clf, trajectory, TIMESTEPS, NV)
    assert np.array_equal(report["gradcam_summary"], cams.pop("summary"))
    _same(report["gradcam"], cams, "gradcam")
    imp = report["gradcam_most_important"]
    assert imp["index"] == ts["most_important_index"] and imp["timestep"] == float(ts["most_important_timestep"])
    assert np.array_equal(imp["gradcam"], cams[f"t_{imp['timestep']:.0f}"])
    _same(report["sanity_checks"], xai.sanity_check(clf, trajectory[-1:], NV, n_trials=3, randomization_strength=0.01, seed=SEED),
          "sanity_checks")


def test_pipeline_is_reproducible(clf, trajectory, report):
    from synt_isic_amd import xai
    again = xai.run_pipeline(clf, trajectory, TIMESTEPS, NV, "NV", seed=SEED, intervention_types=TYPES, ig_steps=IG_STEPS,
                             shap_samples=SHAP_SAMPLES)
    _same(report, again, "report")


def test_one_frame_records_insufficient_data(clf, trajectory):
    from synt_isic_amd import xai
    res = xai.run_pipeline(clf, trajectory[-1:], [0.0], NV, "NV", seed=SEED, ig_steps=2, shap_samples=4)
    assert set(res) == REFERENCE_KEYS
    assert res["statistical_validation"] == {"error": "Insufficient data"}
    assert list(res["cfi_analysis"]) == ["t_0"] and set(res["cfi_analysis"]["t_0"]) == {"top_k_blur", "bottom_k_blur"}
    assert "overall_sanity_score" in res["sanity_checks"]
