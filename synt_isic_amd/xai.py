"""Batched forward passes of the reference's explainability analyses (xai/XAI.py), on the HIP kernels.

* ``compute_time_shap``            -- XAI.py:1179-1234 as coded: per-frame classifier scores, min-max
                                     normalised.  The reference runs 2 batch-1 forwards per frame; here the N
                                     frames are ONE [N,3,H,W] batch.
* ``compute_shap_approximation``   -- XAI.py:1111-1177: 512 random 16x16-patch coalitions x classifier score.
                                     The reference runs 513 batch-1 forwards per image; here the coalition
                                     images are built on the GPU (``sisic_mask_patches``) and scored in batches.
* ``compute_integrated_gradients`` -- XAI.py:1039-1084: captum IntegratedGradients (n_steps = 50, ``riemann_right``) of
                                     the per-class score; all Riemann points go through ONE batched backward-to-input
                                     pass of the HIP classifier (``sisic_resnet_input_gradient``), no autograd.
* ``compute_grad_cam``             -- XAI.py:2945-3134: Grad-CAM on ``layer4[-1].conv2`` for every trajectory frame (ONE
                                     batch instead of a GradCAM call per frame) + the normalised mean map.
* ``compute_gradient_attribution`` -- XAI.py:1086-1109: the plain input gradient (the reference's fallback).
* ``time_shap_permutation``        -- README.md:171-207: Shapley values of the denoising STEPS with
                                     v(S) = F(Dec(x_T; S)) (transitions applied only on the steps in S, the other
                                     steps are skipped) and the unbiased permutation estimator.  The reference
                                     documents this form but does not implement it.

Stage 2 of ``run_comprehensive_xai_pipeline`` (XAI.py:2822-2896), counterfactual interventions and their causal shift:

* ``select_regions``               -- XAI.py:1340-1451: top-k / bottom-k regions of an attribution map with the morphological
                                     clean-up (host, numpy; no scipy).
* ``counterfactual_intervention``  -- XAI.py:1454-1597 for one image, on ``sisic_intervene``.
* ``compute_causal_shift``         -- XAI.py:1600-1700: ONE classifier batch of (original, modified) + ``sisic_cfi_metrics``
                                     instead of 18 batch-1 forwards.
* ``compute_combined_attribution`` -- XAI.py:1236-1291: the weighted sum of the passes above.
* ``intervention_stage``           -- XAI.py:2829-2875: every (key frame, region, intervention type) in ONE ``sisic_intervene``
                                     launch, ONE classifier batch and ONE ``sisic_cfi_metrics`` launch.

The rest of the run (XAI.py:2733-2821, :1708-2210, :3175-3240) -- plots, the PNG / JSON saving stage and the two normality tests
aside:

* ``attribution_stage``            -- stage 1 as a stage: per frame ONE combined IG + patch-SHAP map from generators seeded
                                     ``seed + 2 i`` / ``seed + 2 i + 1`` and its top-k / bottom-k regions, in the layout
                                     ``intervention_stage`` consumes (the reference computes IG and SHAP three times per frame).
* ``statistical_validation``       -- stages 4-5: the classical tests in numpy (``xai_stats``: no scipy) and the 1 000 bootstrap +
                                     10 000 permutation resamples as ONE ``sisic_resample_diffs`` launch drawn from a seed
                                     (device-noise tags 3 and 4), where the reference loops in the interpreter over numpy's
                                     global generator.
* ``sanity_check``                 -- stage 6: weight randomisation, input independence, class sensitivity.  The classifier is
                                     re-randomised ON THE DEVICE (``sisic_resnet_randomize``: Philox normals written in their
                                     BatchNorm-folded and packed forms, device-noise tag 16 + tensor) and restored afterwards.
* ``run_pipeline``                 -- the driver: stages 1-2, Time-SHAP, Grad-CAM, statistics, sanity check -> the reference's
                                     ``results`` dictionary, a function of its seed.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .classifier import CLASS_NAMES, HipMelanomaClassifier
from .sampler import Sampler, draw_noise, run_sampling_loop

SHAP_N_SAMPLES = 512          # xai/XAI.py SHAP_N_SAMPLES


def _as_batch(trajectory) -> torch.Tensor:
    if torch.is_tensor(trajectory):
        t = trajectory
        return t.reshape((-1,) + tuple(t.shape[-3:])) if t.dim() == 5 else t
    return torch.cat([f if f.dim() == 4 else f.unsqueeze(0) for f in trajectory], dim=0)


@torch.no_grad()
def compute_time_shap(classifier: HipMelanomaClassifier, trajectory, timesteps: Sequence[float], target_class: int):
    """(normalized_importance, raw_data) exactly as XAI.py:1179-1234 returns them."""
    frames = _as_batch(trajectory)
    if frames.shape[0] != len(timesteps):
        raise ValueError(f"{frames.shape[0]} frames but {len(timesteps)} timesteps")
    prob, logscore = classifier._scores(frames, target_class)
    confidence_scores = logscore.cpu().numpy().astype(np.float64)
    prob_scores = prob.cpu().numpy().astype(np.float64)
    if len(confidence_scores) > 1 and (confidence_scores.max() - confidence_scores.min()) > 1e-6:
        normalized = (confidence_scores - confidence_scores.min()) / (confidence_scores.max() - confidence_scores.min())
    else:
        normalized = np.ones_like(confidence_scores) / len(confidence_scores)
    raw = {"confidence_scores": confidence_scores, "probability_scores": prob_scores, "timesteps": list(timesteps)}
    return normalized, raw


IG_N_STEPS = 50               # xai/XAI.py:240


def make_baseline(image: torch.Tensor, baseline_type: str = "noise", generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """XAI.py:1010-1037: 'noise' = randn_like(image) * 0.1 (drawn on the CPU here so that it can be seeded), 'zero',
    'blur' = avg_pool2d(kernel 31, stride 1, padding 15); anything else = zero."""
    if baseline_type == "noise":
        return (torch.randn(image.shape, generator=generator, dtype=torch.float32) * 0.1).to(image.device)
    if baseline_type == "blur":
        return torch.nn.functional.avg_pool2d(image, kernel_size=31, stride=1, padding=15)
    return torch.zeros_like(image)


@torch.no_grad()
def compute_gradient_attribution(classifier: HipMelanomaClassifier, image: torch.Tensor, target_class: int) -> torch.Tensor:
    """XAI.py:1086-1109: d get_per_class_score / d image."""
    return classifier.input_gradient(image, target_class)[0]


@torch.no_grad()
def compute_integrated_gradients(classifier: HipMelanomaClassifier, image: torch.Tensor, target_class: int,
                                 n_steps: int = IG_N_STEPS, baseline: Optional[torch.Tensor] = None,
                                 baseline_type: str = "noise", generator: Optional[torch.Generator] = None,
                                 max_batch: int = 128) -> torch.Tensor:
    """XAI.py:1039-1084 (captum ``IntegratedGradients.attribute(image, baselines, n_steps, method='riemann_right')``
    with ``forward_func = get_per_class_score``):
        IG(x) = (x - x') * (1/n) * sum_{k=1..n} grad score(x' + (k/n)(x - x'))
    image: [B,3,H,W]; the n*B Riemann points are differentiated in batches of ``max_batch`` images."""
    image = image.to(classifier.device).to(torch.float32)
    if baseline is None:
        baseline = make_baseline(image, baseline_type, generator)
    baseline = baseline.to(image.device).to(torch.float32)
    B = image.shape[0]
    alphas = torch.arange(1, n_steps + 1, dtype=torch.float32, device=image.device) / n_steps
    diff = image - baseline
    total = torch.zeros_like(image)
    per = max(1, max_batch // B)                       # Riemann points per pass
    for k0 in range(0, n_steps, per):
        a = alphas[k0:k0 + per].view(-1, 1, 1, 1, 1)
        pts = (baseline.unsqueeze(0) + a * diff.unsqueeze(0)).reshape((-1,) + tuple(image.shape[1:]))
        g = classifier.input_gradient(pts, target_class)[0]
        total += g.view((-1, B) + tuple(image.shape[1:])).sum(0)
    return diff * total / n_steps


@torch.no_grad()
def compute_grad_cam(classifier: HipMelanomaClassifier, trajectory, timesteps: Sequence[float], target_class: int) -> Dict:
    """XAI.py:2945-3134: {"t_<timestep>": cam (224,224) numpy in [0,1]} for every frame, and "summary": the mean of the
    frames' maps min-max normalised with eps 1e-8 (``gradcam_summary``, :3102-3104)."""
    frames = _as_batch(trajectory)
    if frames.shape[0] != len(timesteps):
        raise ValueError(f"{frames.shape[0]} frames but {len(timesteps)} timesteps")
    cams = classifier.grad_cam(frames, target_class)[0].cpu().numpy()
    out = {f"t_{float(t):.0f}": cams[i] for i, t in enumerate(timesteps)}
    mean = cams.mean(axis=0)
    out["summary"] = (mean - mean.min()) / (mean.max() - mean.min() + 1e-8)
    return out


def draw_patch_masks(n_samples: int, nh: int, nw: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The reference's per-sample ``torch.rand(nh, nw) > 0.5`` draws (XAI.py:1147), in order, as one bool tensor."""
    return torch.stack([torch.rand(nh, nw, generator=generator) > 0.5 for _ in range(n_samples)])


@torch.no_grad()
def compute_shap_approximation(classifier: HipMelanomaClassifier, image: torch.Tensor, target_class: int,
                               n_samples: int = SHAP_N_SAMPLES, patch_size: int = 16,
                               patch_masks: Optional[torch.Tensor] = None, chunk: int = 256) -> torch.Tensor:
    """Attribution map [1,3,H,W] of XAI.py:1111-1177 for ONE image [1,3,H,W] in [-1,1]."""
    dev = classifier.device
    image = image.to(dev, torch.float32).contiguous()
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError("compute_shap_approximation takes one image [1,3,H,W]")
    _, Cc, H, W = image.shape
    nh, nw = H // patch_size, W // patch_size
    if patch_masks is None:
        patch_masks = draw_patch_masks(n_samples, nh, nw)          # global CPU RNG, like the reference
    if tuple(patch_masks.shape) != (n_samples, nh, nw):
        raise ValueError(f"patch_masks must be [{n_samples},{nh},{nw}]")
    masks_u8 = patch_masks.to(torch.uint8).contiguous().to(dev)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    baseline = classifier.get_per_class_score(torch.zeros_like(image), target_class)       # [1]
    scores = ops.empty(n_samples, dtype=torch.float32, device=dev)
    for s0 in range(0, n_samples, chunk):
        s1 = min(n_samples, s0 + chunk)
        batch = ops.empty((s1 - s0, Cc, H, W), dtype=torch.float32, device=dev)
        check(lib.sisic_mask_patches(ops.context(dev), image.data_ptr(), masks_u8[s0:s1].data_ptr(), batch.data_ptr(),
                                     s1 - s0, Cc, H, W, patch_size, stream))
        scores[s0:s1] = classifier.get_per_class_score(batch, target_class)
    # attribution = (1/n) * sum_s (score_s - baseline) * mask_s  -- a [n] x [n,nh,nw] contraction of ~10^4 values
    contrib = (scores - baseline).double().cpu()
    grid = torch.einsum("s,sij->ij", contrib, patch_masks.double()) / n_samples
    full = torch.zeros(H, W, dtype=torch.float64)
    full[: nh * patch_size, : nw * patch_size] = grid.repeat_interleave(patch_size, 0).repeat_interleave(patch_size, 1)
    return full.float().to(dev).expand(1, Cc, H, W).contiguous()


@torch.no_grad()
def coalition_value(sampler: Sampler, classifier: HipMelanomaClassifier, class_name: str, x_T: torch.Tensor,
                    z: torch.Tensor, T: int, coalitions: Sequence[Sequence[int]], target_class: int) -> torch.Tensor:
    """v(S) for every coalition S (step indices into the T-step grid): the mean over the batch of the target
    logit after a denoising run that applies only the steps in S.  x_T [B,3,H,W], z [n_noise,B,3,H,W] on the
    GPU; the same x_T / z_t serve every coalition, so v is a deterministic set function."""
    model = sampler.models[class_name]
    sched_full = sampler.create_scheduler(T)
    ts_full = sched_full.timesteps.clone()
    noise_index = {}
    k = 0
    for i, t in enumerate(ts_full.tolist()):
        if t > 0:
            noise_index[i] = k
            k += 1
    finals = []
    for S in coalitions:
        steps = sorted(set(int(s) for s in S))
        if steps:
            sched = sampler.create_scheduler(T)
            sched.timesteps = ts_full[steps]                       # descending t, standard coefficients per step
            zi = [noise_index[i] for i in steps if i in noise_index]
            zs = z[zi].contiguous() if zi else None
            finals.append(run_sampling_loop(model, sched, x_T, zs).latents)
        else:
            finals.append(x_T)
    # ONE classifier batch for all coalitions ([n_coalitions * B, 3, H, W]: 16 x 32 = 512 forwards in BASELINE config 5)
    B = x_T.shape[0]
    logits = classifier.forward(torch.cat(finals, dim=0))
    return logits[:, target_class].view(len(finals), B).mean(dim=1)


@torch.no_grad()
def time_shap_permutation(sampler: Sampler, classifier: HipMelanomaClassifier, class_name: str, seeds: Sequence[int],
                          T: int, target_class: int, n_permutations: int = 4, size: Tuple[int, int] = (64, 64),
                          generator: Optional[torch.Generator] = None) -> Dict[str, np.ndarray]:
    """Permutation estimator of README.md:198-207: phi_t = mean_m [ v(Pref_pi_m(t) u {t}) - v(Pref_pi_m(t)) ].
    Per permutation the T+1 nested prefixes give every marginal, so efficiency holds exactly:
    sum_t phi_t = v({all steps}) - v({})."""
    H, W = size
    sched = sampler.create_scheduler(T)
    n_noise = sum(1 for t in sched.timesteps if int(t) > 0)
    x_T, z = draw_noise(seeds, n_noise, (3, H, W))
    x_T, z = x_T.to(sampler.device), z.to(sampler.device)
    phi = np.zeros(T, dtype=np.float64)
    v_full = v_empty = None
    for _ in range(n_permutations):
        perm = torch.randperm(T, generator=generator).tolist()
        coalitions = [perm[:k] for k in range(T + 1)]
        v = coalition_value(sampler, classifier, class_name, x_T, z, T, coalitions, target_class).double().cpu().numpy()
        for k, step in enumerate(perm):
            phi[step] += v[k + 1] - v[k]
        v_empty, v_full = v[0], v[T]
    phi /= n_permutations
    return {"phi": phi, "v_full": np.float64(v_full), "v_empty": np.float64(v_empty),
            "timesteps": np.array([int(t) for t in sched.timesteps])}


# ---- stage 2: regions, counterfactual interventions, causal shift (XAI.py:1340-1700, :2822-2896) ---------------------------
TOP_K_PERCENT = 10            # xai/XAI.py:238
INTERVENTION_TYPES = ("blur",)  # xai/XAI.py:265
NOISE_STD = 0.5               # xai/XAI.py:266
BLUR_KERNEL_SIZE = 5          # xai/XAI.py:267


def _structure_offsets(connectivity: int) -> List[Tuple[int, int]]:
    """3x3 structuring element: the cross for connectivity 4, the full square otherwise (XAI.py:1390-1393)."""
    return [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if connectivity != 4 or dy == 0 or dx == 0]


def _binary_dilate(mask: np.ndarray, offsets) -> np.ndarray:
    H, W = mask.shape
    padded = np.zeros((H + 2, W + 2), dtype=bool)
    padded[1:-1, 1:-1] = mask
    out = np.zeros((H, W), dtype=bool)
    for dy, dx in offsets:
        out |= padded[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return out


def _binary_erode(mask: np.ndarray, offsets) -> np.ndarray:
    """the outside counts as 0, as for the dilation: border pixels go"""
    H, W = mask.shape
    padded = np.zeros((H + 2, W + 2), dtype=bool)
    padded[1:-1, 1:-1] = mask
    out = np.ones((H, W), dtype=bool)
    for dy, dx in offsets:
        out &= padded[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return out


def _drop_small_components(mask: np.ndarray, offsets, min_size: int) -> np.ndarray:
    """keep the connected components (neighbourhood = ``offsets``) of at least ``min_size`` pixels: a flood fill per component"""
    H, W = mask.shape
    Wp = W + 2
    cells = bytearray(np.pad(mask, 1).astype(np.uint8).tobytes())        # 1 = unvisited mask pixel; the zero frame stops the fill
    steps = [dy * Wp + dx for dy, dx in offsets if (dy, dx) != (0, 0)]
    kept: List[int] = []
    for start in np.flatnonzero(np.pad(mask, 1)).tolist():
        if cells[start] != 1:
            continue
        cells[start] = 2
        component = [start]
        k = 0
        while k < len(component):
            here = component[k]
            k += 1
            for st in steps:
                nb = here + st
                if cells[nb] == 1:
                    cells[nb] = 2
                    component.append(nb)
        if len(component) >= min_size:
            kept.extend(component)
    out = np.zeros((H + 2) * Wp, dtype=bool)
    out[kept] = True
    return out.reshape(H + 2, Wp)[1:-1, 1:-1].copy()


def select_regions(attribution_map, k_percent: float = TOP_K_PERCENT, region_type: str = "top",
                   morphology_cleanup: bool = True, connectivity: int = 8) -> Dict:
    """``select_regions_advanced`` (XAI.py:1340-1451): the {mask, threshold, statistics, metadata} dict of the top-k or
    bottom-k percent of an attribution map (L2 norm over channels for [C,H,W] / [1,C,H,W] input, |.| for [H,W]).  The
    clean-up is binary closing x2, opening x1 with the 3x3 structure of ``connectivity``, then components smaller than
    max(10, 1% of the map) are dropped -- in numpy, pixel for pixel what scipy.ndimage gives (tests/test_xai_regions.py)."""
    attr = attribution_map.detach().cpu().numpy() if torch.is_tensor(attribution_map) else np.array(attribution_map)
    original_shape = attr.shape
    if attr.ndim == 4:
        attr = attr[0]
    attr = np.linalg.norm(attr, axis=0) if attr.ndim == 3 else np.abs(attr)
    if region_type == "top":
        threshold = np.percentile(attr.flatten(), 100 - k_percent)
        mask = attr >= threshold
    elif region_type == "bottom":
        threshold = np.percentile(attr.flatten(), k_percent)
        mask = attr <= threshold
    else:
        raise ValueError(f"unknown region_type '{region_type}' ('top' or 'bottom')")
    if morphology_cleanup:
        offs = _structure_offsets(connectivity)
        for op in (_binary_dilate, _binary_dilate, _binary_erode, _binary_erode,      # closing, 2 iterations
                   _binary_erode, _binary_dilate):                                      # opening, 1 iteration
            mask = op(mask, offs)
        mask = _drop_small_components(mask, offs, max(10, int(0.01 * mask.size)))
    selected = np.sum(mask)
    inside = attr[mask]
    has = selected > 0
    return {
        "mask": mask,
        "threshold": threshold,
        "statistics": {
            "total_pixels": attr.size,
            "selected_pixels": selected,
            "target_percentage": k_percent,
            "actual_percentage": (selected / attr.size) * 100,
            "threshold_value": threshold,
            "mean_attribution": np.mean(attr),
            "std_attribution": np.std(attr),
            "mean_attribution_selected": np.mean(inside) if has else 0,
            "std_attribution_selected": np.std(inside) if has else 0,
            "max_attribution_selected": np.max(inside) if has else 0,
            "min_attribution_selected": np.min(inside) if has else 0,
        },
        "metadata": {"region_type": region_type, "morphology_cleanup": morphology_cleanup, "connectivity": connectivity,
                     "original_shape": original_shape},
    }


def _mask_2d(mask, H: int, W: int) -> torch.Tensor:
    """a region mask (numpy or tensor, any leading 1-dimensions) as a CPU bool [H,W]"""
    m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask.detach().cpu()
    if m.numel() != H * W or tuple(m.shape[-2:]) != (H, W):
        raise ValueError(f"mask of shape {tuple(m.shape)} does not cover a {H}x{W} image")
    return m.reshape(H, W) != 0


def _shuffle_index(mask: torch.Tensor, channels: int, generator: torch.Generator) -> torch.Tensor:
    """int32 [C,H*W] source pixels of the 'shuffle' intervention (XAI.py:1540-1566): one ``torch.randperm`` per channel over the
    masked pixels (none when fewer than 2 are masked), the identity elsewhere."""
    flat = mask.reshape(-1)
    inside = torch.nonzero(flat).reshape(-1)
    src = torch.arange(flat.numel(), dtype=torch.int64).repeat(channels, 1)
    if inside.numel() > 1:
        for c in range(channels):
            src[c, inside] = inside[torch.randperm(inside.numel(), generator=generator)]
    return src.to(torch.int32)


def _intervention_entry(image, modified, intervention, mask, stats_row, intervention_type: str, parameters: Dict) -> Dict:
    """the dict ``counterfactual_intervention_advanced`` returns (XAI.py:1582-1595)"""
    return {
        "modified_image": modified,
        "intervention": intervention,
        "mask_tensor": mask.to(image.device, torch.float32).reshape(1, 1, *mask.shape),
        "difference": torch.abs(image - modified),
        "statistics": {"intervention_type": intervention_type, "mask_coverage": float(stats_row[0]),
                       "mean_difference": float(stats_row[1]), "max_difference": float(stats_row[2]),
                       "intervention_strength": float(stats_row[3])},
        "parameters": parameters,
    }


@torch.no_grad()
def counterfactual_intervention(image: torch.Tensor, mask, intervention_type: str = "noise", **kwargs) -> Dict:
    """``counterfactual_intervention_advanced`` (XAI.py:1454-1597) for one image [1,C,H,W] on the GPU:
    modified = clamp(image * (1 - M) + intervention * M, -1, 1).  kwargs: ``noise_std`` (0.5), ``blur_kernel`` (5) and
    ``seed`` (0) -- the noise types draw the device-noise blocks of that seed (tag 2), 'shuffle' one ``torch.randperm`` per
    channel from a CPU generator seeded with it.  An unknown type is an error (the reference falls back to noise)."""
    if image.dim() == 3:
        image = image.unsqueeze(0)
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError(f"counterfactual_intervention takes one image [1,C,H,W], got {tuple(image.shape)}")
    if intervention_type not in ops.INTERVENTION_TYPES:
        raise ValueError(f"unknown intervention type '{intervention_type}' (one of {', '.join(ops.INTERVENTION_TYPES)})")
    image = image.to(torch.float32).contiguous()
    _, Cc, H, W = image.shape
    m = _mask_2d(mask, H, W)
    seed = int(kwargs.get("seed", 0))
    src = None
    if intervention_type == "shuffle":
        src = _shuffle_index(m, Cc, torch.Generator().manual_seed(seed)).unsqueeze(0).contiguous().to(image.device)
    job = (0, 0, intervention_type, int(kwargs.get("blur_kernel", BLUR_KERNEL_SIZE)), float(kwargs.get("noise_std", NOISE_STD)))
    out, iv, stats = ops.intervene(image, m.to(torch.uint8).unsqueeze(0).contiguous().to(image.device), [job], [seed],
                                   src_index=src, with_intervention=True)
    return _intervention_entry(image, out, iv, m, stats[0].cpu(), intervention_type, kwargs)


def _causal_shift_entry(row: np.ndarray, n: int, target_class: int, include_all_classes: bool) -> Dict:
    """one row of ``sisic_cfi_metrics`` as the dict of XAI.py:1641-1698"""
    names = CLASS_NAMES if n == len(CLASS_NAMES) else tuple(str(c) for c in range(n))
    per = row[:ops.CFI_PER_CLASS * n].reshape(n, ops.CFI_PER_CLASS)
    tail = row[ops.CFI_PER_CLASS * n:]
    t = per[target_class]
    po, pm = int(tail[0]), int(tail[1])
    res = {
        "target_class_analysis": {
            "class_id": target_class, "class_name": names[target_class], "cfi": float(t[2]), "delta": float(t[3]),
            "original_score": float(t[0]), "modified_score": float(t[1]), "original_probability": float(t[4]),
            "modified_probability": float(t[5]), "probability_shift": float(t[4] - t[5]),
        },
        "prediction_analysis": {
            "original_prediction": po, "original_prediction_name": names[po], "modified_prediction": pm,
            "modified_prediction_name": names[pm], "prediction_changed": bool(po != pm),
            "original_confidence": float(tail[2]), "modified_confidence": float(tail[3]),
            "confidence_drop": float(tail[2] - tail[3]),
        },
    }
    if include_all_classes:
        res["all_classes_analysis"] = [
            {"class_id": c, "class_name": names[c], "cfi": float(per[c, 2]), "delta": float(per[c, 3]),
             "original_probability": float(per[c, 4]), "modified_probability": float(per[c, 5]),
             "probability_shift": float(per[c, 4] - per[c, 5])} for c in range(n)]
    res["distribution_analysis"] = {"kl_divergence": float(tail[4]), "js_divergence": float(tail[5]),
                                    "total_variation": float(tail[6])}
    return res


@torch.no_grad()
def compute_causal_shift(classifier: HipMelanomaClassifier, original_image: torch.Tensor, modified_image: torch.Tensor,
                         target_class: int, include_all_classes: bool = True) -> Dict:
    """``compute_causal_shift_comprehensive`` (XAI.py:1600-1700) for one (original, modified) pair [1,3,H,W]: CFI, delta, the
    probabilities and predictions, KL / JS / total variation -- one classifier batch of two images and ``sisic_cfi_metrics``."""
    dev = classifier.device
    pair = torch.cat([original_image.to(dev, torch.float32), modified_image.to(dev, torch.float32)], dim=0)
    if pair.shape[0] != 2:
        raise ValueError("compute_causal_shift takes one original and one modified image [1,3,H,W]")
    logits = classifier.forward(pair)
    row = ops.cfi_metrics(logits[:1], logits[1:], [0])[0].cpu().numpy()
    return _causal_shift_entry(row, logits.shape[1], int(target_class), include_all_classes)


@torch.no_grad()
def compute_combined_attribution(classifier: HipMelanomaClassifier, image: torch.Tensor, target_class: int,
                                 methods: Sequence[str] = ("ig", "shap"), weights: Optional[Sequence[float]] = None,
                                 ig_kwargs: Optional[Dict] = None, shap_kwargs: Optional[Dict] = None):
    """XAI.py:1236-1291: (sum_m weight_m * attribution_m, method_details) over 'ig', 'shap' and 'gradient'; equal weights by
    default.  A method name the reference does not know is skipped as there; none left is an error."""
    methods = list(methods)
    if weights is None:
        weights = [1.0 / len(methods)] * len(methods)
    image = image.to(classifier.device, torch.float32)
    total = None
    details = {}
    for method, weight in zip(methods, weights):
        if method == "ig":
            attr = compute_integrated_gradients(classifier, image, target_class, **(ig_kwargs or {}))
        elif method == "shap":
            attr = compute_shap_approximation(classifier, image, target_class, **(shap_kwargs or {}))
        elif method == "gradient":
            attr = compute_gradient_attribution(classifier, image, target_class)
        else:
            continue
        total = attr * weight if total is None else total + attr * weight
        details[method] = {"weight": weight, "mean_attribution": float(attr.abs().mean()),
                           "max_attribution": float(attr.abs().max())}
    if total is None:
        raise RuntimeError(f"no attribution computed: none of {methods} is one of 'ig', 'shap', 'gradient'")
    return total, details


def key_steps(n_frames: int) -> List[int]:
    """The frames stage 2 intervenes on (XAI.py:2829): first, middle and the last four, as indices 0 .. n-1 (a negative index
    of a short trajectory counts from the end, as it does there) without repeats, in that order."""
    if n_frames <= 0:
        return []
    n = n_frames
    out: List[int] = []
    for i in (0, n // 2, n - 4, n - 3, n - 2, n - 1):
        i %= n
        if i not in out:
            out.append(i)
    return out


@torch.no_grad()
def intervention_stage(classifier: HipMelanomaClassifier, trajectory, timesteps: Sequence[float], region_data: Dict,
                       target_class: int, intervention_types: Sequence[str] = INTERVENTION_TYPES, seed: int = 0,
                       noise_std: float = NOISE_STD, blur_kernel: int = BLUR_KERNEL_SIZE):
    """Stage 2 of ``run_comprehensive_xai_pipeline`` (XAI.py:2829-2875).  ``region_data["t_<timestep>"]["top_k" | "bottom_k"]
    ["mask"]`` are the regions of stage 1 (``select_regions``); key frames without an entry are skipped.  Returns
    ``(interventions, cfi)`` as the reference stores them: ``interventions[step_key][region][type]`` = the dict of
    ``counterfactual_intervention``, ``cfi[step_key]["<region>_<type>"]`` = the dict of ``compute_causal_shift``.
    Jobs are ordered key frame -> region -> type; job j draws with seed ``seed + j``.  One ``sisic_intervene`` launch, one
    ``classifier.forward`` over the key frames followed by every modified image, one ``sisic_cfi_metrics`` launch."""
    frames = _as_batch(trajectory)
    if frames.shape[0] != len(timesteps):
        raise ValueError(f"{frames.shape[0]} frames but {len(timesteps)} timesteps")
    types = list(intervention_types)
    for t in types:
        if t not in ops.INTERVENTION_TYPES:
            raise ValueError(f"unknown intervention type '{t}' (one of {', '.join(ops.INTERVENTION_TYPES)})")
    dev = classifier.device
    _, Cc, H, W = frames.shape
    regions = ("top_k", "bottom_k")
    used = [(i, f"t_{float(timesteps[i]):.0f}") for i in key_steps(frames.shape[0])]
    used = [(i, key) for i, key in used if key in region_data]
    if not used or not types:
        return {}, {}
    originals = frames[[i for i, _ in used]].to(dev, torch.float32).contiguous()
    masks = [_mask_2d(region_data[key][r]["mask"], H, W) for _, key in used for r in regions]
    jobs, labels = [], []
    for f, (_, key) in enumerate(used):
        for r in range(len(regions)):
            for t in types:
                jobs.append((f, 2 * f + r, t, blur_kernel, noise_std))
                labels.append((key, regions[r], t))
    J = len(jobs)
    seeds = [int(seed) + j for j in range(J)]
    src = None
    if "shuffle" in types:
        identity = torch.arange(H * W, dtype=torch.int32).repeat(Cc, 1)
        src = torch.stack([_shuffle_index(masks[m], Cc, torch.Generator().manual_seed(seeds[j])) if t == "shuffle" else identity
                           for j, (_, m, t, _, _) in enumerate(jobs)]).contiguous().to(dev)
    masks_dev = torch.stack(masks).to(torch.uint8).contiguous().to(dev)
    modified, iv, stats = ops.intervene(originals, masks_dev, jobs, seeds, src_index=src, with_intervention=True)
    logits = classifier.forward(torch.cat([originals, modified], dim=0))
    F_ = originals.shape[0]
    rows = ops.cfi_metrics(logits[:F_], logits[F_:], [f for f, *_ in jobs]).cpu().numpy()
    stats = stats.cpu()
    interventions: Dict = {}
    cfi: Dict = {}
    for j, (key, region, t) in enumerate(labels):
        f, m = jobs[j][0], jobs[j][1]
        params = {"noise_std": noise_std, "blur_kernel": blur_kernel, "seed": seeds[j]}
        entry = _intervention_entry(originals[f:f + 1], modified[j:j + 1], iv[j:j + 1], masks[m], stats[j], t, params)
        interventions.setdefault(key, {}).setdefault(region, {})[t] = entry
        cfi.setdefault(key, {})[f"{region}_{t}"] = _causal_shift_entry(rows[j], logits.shape[1], int(target_class), True)
    return interventions, cfi


# ---- stages 1, 4-6 and the driver (XAI.py:2733-2821, :1708-2210, :2663-3297) ---------------------------------------------------
BOTTOM_K_PERCENT = 10         # xai/XAI.py:239
ALPHA_LEVEL = 0.1             # xai/XAI.py:270
N_BOOTSTRAP = 1000            # xai/XAI.py:271
N_PERMUTATIONS = 10000        # xai/XAI.py:272
SHAP_PATCH_SIZE = 16          # compute_shap_approximation's default


def _step_key(timestep) -> str:
    return f"t_{float(timestep):.0f}"


@torch.no_grad()
def attribution_stage(classifier: HipMelanomaClassifier, trajectory, timesteps: Sequence[float], target_class: int, *,
                      ig_steps: int = IG_N_STEPS, shap_samples: int = SHAP_N_SAMPLES, k_percent: float = TOP_K_PERCENT,
                      seed: int = 0):
    """Stage 1 of ``run_comprehensive_xai_pipeline`` (XAI.py:2733-2821): ``(xai_maps, region_data)`` keyed ``t_<timestep>``.
    ``xai_maps[key]`` = {timestep, attribution_map, method_details, image_shape}, ``region_data[key]`` = {top_k, bottom_k} of
    ``select_regions`` -- the layout ``intervention_stage`` consumes.

    Frame i's map IS ``compute_combined_attribution(classifier, frame_i, target_class, ("ig", "shap"), [0.5, 0.5],
    ig_kwargs={"n_steps": ig_steps, "generator": g_ig}, shap_kwargs={"n_samples": shap_samples, "patch_masks": masks})`` with
    ``g_ig = torch.Generator().manual_seed(seed + 2 i)`` and ``masks = draw_patch_masks(shap_samples, H // 16, W // 16,
    torch.Generator().manual_seed(seed + 2 i + 1))``.  The reference computes IG and SHAP three times per frame with fresh
    random draws (two for plots); only the combined map reaches the results, and only it is computed here."""
    frames = _as_batch(trajectory)
    if frames.shape[0] != len(timesteps):
        raise ValueError(f"{frames.shape[0]} frames but {len(timesteps)} timesteps")
    H, W = frames.shape[-2:]
    xai_maps: Dict = {}
    region_data: Dict = {}
    for i, timestep in enumerate(timesteps):
        image = frames[i:i + 1]
        g_ig = torch.Generator().manual_seed(int(seed) + 2 * i)
        masks = draw_patch_masks(shap_samples, H // SHAP_PATCH_SIZE, W // SHAP_PATCH_SIZE,
                                 torch.Generator().manual_seed(int(seed) + 2 * i + 1))
        combined, details = compute_combined_attribution(classifier, image, target_class, ("ig", "shap"), [0.5, 0.5],
                                                         ig_kwargs={"n_steps": ig_steps, "generator": g_ig},
                                                         shap_kwargs={"n_samples": shap_samples, "patch_masks": masks})
        key = _step_key(timestep)
        xai_maps[key] = {"timestep": timestep, "attribution_map": combined, "method_details": details,
                         "image_shape": tuple(image.shape)}
        region_data[key] = {"top_k": select_regions(combined, k_percent=k_percent, region_type="top"),
                            "bottom_k": select_regions(combined, k_percent=k_percent, region_type="bottom")}
    return xai_maps, region_data


_NORMALITY_SKIPPED = {"skipped": True, "reason": "not computed: informational in the reference, outside the consensus"}


def statistical_validation(top_k_shifts, bottom_k_shifts, alpha: float = ALPHA_LEVEL, n_bootstrap: int = N_BOOTSTRAP,
                           n_permutations: int = N_PERMUTATIONS, seed: int = 0, device="cuda") -> Dict:
    """``statistical_validation_comprehensive`` (XAI.py:1708-2005): the reference's dictionary, same keys and nesting.  The
    classical tests are ``xai_stats`` (numpy, no scipy); the 1 000 bootstrap and 10 000 permutation resamples are ONE
    ``sisic_resample_diffs`` launch drawn from ``seed`` (device-noise tags 3 and 4) instead of two interpreter loops over
    numpy's global generator: the same distributions, reproducible.  ``normality_tests`` holds the reference's 'skipped' form
    (Shapiro-Wilk and Kolmogorov-Smirnov do not enter the consensus); ``metadata`` gains ``seed``.  Fewer than two values on
    either side raise ``ValueError("Insufficient data")``."""
    from datetime import datetime

    from . import xai_stats
    top_k = np.asarray(top_k_shifts, dtype=np.float64).reshape(-1)
    bottom_k = np.asarray(bottom_k_shifts, dtype=np.float64).reshape(-1)
    if len(top_k) < 2 or len(bottom_k) < 2:
        raise ValueError("Insufficient data")
    if n_bootstrap < 1:
        raise ValueError("n_bootstrap must be at least 1")
    results = xai_stats.classical_tests(top_k, bottom_k, alpha)
    boot, perm = ops.resample_diffs(top_k, bottom_k, seed, n_bootstrap, n_permutations, device)

    bootstrap_diffs = boot.cpu().numpy()
    confidence_level = 1 - alpha
    ci_lower = np.percentile(bootstrap_diffs, (1 - confidence_level) / 2 * 100)
    ci_upper = np.percentile(bootstrap_diffs, (1 + confidence_level) / 2 * 100)
    bootstrap_results = {"bootstrap_diffs": bootstrap_diffs, "mean_diff": np.mean(bootstrap_diffs), "ci_lower": ci_lower,
                         "ci_upper": ci_upper, "ci_contains_zero": bool(ci_lower <= 0 <= ci_upper),
                         "confidence_level": confidence_level}

    observed_diff = np.mean(top_k) - np.mean(bottom_k)
    if len(top_k) >= 2 and len(bottom_k) >= 2 and perm is not None:
        permuted_diffs = perm.cpu().numpy()
    else:
        permuted_diffs = np.array([observed_diff])
    p_value = np.mean(np.abs(permuted_diffs) >= np.abs(observed_diff)) if permuted_diffs.size > 1 else 1.0
    permutation_results = {"observed_difference": observed_diff, "permuted_differences": permuted_diffs, "p_value": p_value,
                           "significant": bool(p_value < alpha), "n_permutations": n_permutations}

    consensus = {
        "parametric_significant": any(t["significant"] for t in results["parametric_tests"].values()),
        "nonparametric_significant": any(t["significant"] for t in results["nonparametric_tests"].values()),
        "bootstrap_significant": not bootstrap_results["ci_contains_zero"],
        "permutation_significant": permutation_results["significant"],
    }
    total_significant = sum(consensus.values())
    overall = total_significant >= len(consensus) // 2 + 1
    return {
        "descriptive_statistics": results["descriptive_statistics"],
        "parametric_tests": results["parametric_tests"],
        "nonparametric_tests": results["nonparametric_tests"],
        "effect_sizes": results["effect_sizes"],
        "bootstrap_analysis": bootstrap_results,
        "permutation_analysis": permutation_results,
        "normality_tests": {"shapiro_wilk": {"top_k": dict(_NORMALITY_SKIPPED), "bottom_k": dict(_NORMALITY_SKIPPED)},
                            "kolmogorov_smirnov": {"top_k": dict(_NORMALITY_SKIPPED), "bottom_k": dict(_NORMALITY_SKIPPED)}},
        "variance_tests": results["variance_tests"],
        "significance_consensus": consensus,
        "overall_conclusion": {"significant": overall, "significant_tests_count": total_significant,
                               "total_tests_count": len(consensus), "alpha_level": alpha,
                               "recommendation": "significant" if overall else "not_significant"},
        "metadata": {"analysis_timestamp": datetime.now().isoformat(), "n_bootstrap_samples": n_bootstrap,
                     "n_permutations": n_permutations, "alpha_level": alpha, "seed": seed},
    }


def pearson_correlation(a: torch.Tensor, b: torch.Tensor) -> float:
    """Pearson's r of two maps in float64 on their device: three plain reductions (no BLAS); NaN where numpy's corrcoef is"""
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    da, db = a - a.mean(), b - b.mean()
    return float(((da * db).sum() / torch.sqrt((da * da).sum() * (db * db).sum())).item())


SANITY_RANDOM_THRESHOLD = 0.1          # XAI.py:2086
SANITY_INDEPENDENCE_THRESHOLD = 0.3    # XAI.py:2129
SANITY_SENSITIVITY_THRESHOLD = 0.8     # XAI.py:2164


@torch.no_grad()
def sanity_check(classifier: HipMelanomaClassifier, test_image: torch.Tensor, target_class: int, n_trials: int = 3,
                 randomization_strength: float = 0.01, seed: int = 0, ig_steps: int = 20, ig_steps_aux: int = 15) -> Dict:
    """``sanity_check_comprehensive`` (XAI.py:2008-2210): weight randomisation (|r| of the Integrated-Gradients map against the
    maps of ``n_trials`` re-randomised classifiers, mean < 0.1), input independence (maps of three random inputs, mean |r| < 0.3)
    and class sensitivity (maps of the other classes among 0..2, mean |r| < 0.8), their score and interpretation.

    IG call c, counted in the reference's order -- the original, the trials, the three independent inputs, the other classes --
    draws its noise baseline from ``torch.Generator().manual_seed(seed + c)``; independent input j is ``torch.randn`` from
    ``manual_seed(seed + 1000 + j)``, and the three go through ONE IG call as a batch of three.  Trial t runs under
    ``classifier.randomize_weights(seed, t, randomization_strength)`` (generated on the device; nothing is uploaded).
    Correlations: ``pearson_correlation``; NaN counts as 0 in the first test and is skipped in the other two, as in the
    reference.  The weights are restored in a ``finally``; a library error propagates."""
    dev = classifier.device
    image = test_image.to(dev, torch.float32)
    if image.dim() == 3:
        image = image.unsqueeze(0)
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError(f"sanity_check takes one image [1,3,H,W], got {tuple(test_image.shape)}")
    call = 0

    def baseline_for(img):
        nonlocal call
        g = torch.Generator().manual_seed(int(seed) + call)
        call += 1
        return make_baseline(img, "noise", g)

    results: Dict = {"weight_randomization_test": {}, "input_independence_test": {}, "model_sensitivity_test": {},
                     "overall_sanity_score": 0.0}
    randomized = False
    try:
        original = compute_integrated_gradients(classifier, image, target_class, n_steps=ig_steps, baseline=baseline_for(image))
        correlations_with_random = []
        for trial in range(n_trials):
            classifier.randomize_weights(seed, trial, randomization_strength)
            randomized = True
            attr = compute_integrated_gradients(classifier, image, target_class, n_steps=ig_steps, baseline=baseline_for(image))
            r = pearson_correlation(original, attr)
            correlations_with_random.append(0.0 if np.isnan(r) else abs(r))
        if randomized:
            classifier.restore_weights()
            randomized = False
        mean_random = np.mean(correlations_with_random)
        results["weight_randomization_test"] = {
            "mean_correlation_with_random": mean_random, "correlations_per_trial": correlations_with_random,
            "test_passed": bool(mean_random < SANITY_RANDOM_THRESHOLD), "threshold": SANITY_RANDOM_THRESHOLD, "n_trials": n_trials}

        n_inputs = 3
        inputs = torch.cat([torch.randn(image.shape, generator=torch.Generator().manual_seed(int(seed) + 1000 + j),
                                        dtype=torch.float32) for j in range(n_inputs)]).to(dev)
        baselines = torch.cat([baseline_for(image) for _ in range(n_inputs)])
        maps = compute_integrated_gradients(classifier, inputs, target_class, n_steps=ig_steps_aux, baseline=baselines)
        independence = []
        for i in range(n_inputs):
            for j in range(i + 1, n_inputs):
                r = pearson_correlation(maps[i], maps[j])
                if not np.isnan(r):
                    independence.append(abs(r))
        mean_independence = np.mean(independence) if independence else 0.0
        results["input_independence_test"] = {
            "mean_correlation_between_independent": mean_independence, "independence_correlations": independence,
            "test_passed": bool(mean_independence < SANITY_INDEPENDENCE_THRESHOLD), "threshold": SANITY_INDEPENDENCE_THRESHOLD,
            "n_independent_inputs": n_inputs}

        different = []
        for other in range(min(3, classifier.num_classes)):
            if other == target_class:
                continue
            attr = compute_integrated_gradients(classifier, image, other, n_steps=ig_steps_aux, baseline=baseline_for(image))
            r = pearson_correlation(original, attr)
            if not np.isnan(r):
                different.append(abs(r))
        mean_different = np.mean(different) if different else 1.0
        results["model_sensitivity_test"] = {
            "mean_correlation_different_classes": mean_different, "different_class_correlations": different,
            "test_passed": bool(mean_different < SANITY_SENSITIVITY_THRESHOLD), "threshold": SANITY_SENSITIVITY_THRESHOLD,
            "classes_tested": len(different)}

        passed = [results[k]["test_passed"] for k in ("weight_randomization_test", "input_independence_test",
                                                      "model_sensitivity_test")]
        score = sum(passed) / len(passed)
        results["overall_sanity_score"] = score
        results["overall_interpretation"] = "good" if score >= 0.67 else "moderate" if score >= 0.33 else "poor"
    finally:
        if randomized:
            classifier.restore_weights()
    return results


@torch.no_grad()
def run_pipeline(classifier: HipMelanomaClassifier, trajectory, timesteps: Sequence[float], target_class_id: int,
                 target_class_name: str, *, seed: int = 0, intervention_types: Sequence[str] = INTERVENTION_TYPES,
                 ig_steps: int = IG_N_STEPS, shap_samples: int = SHAP_N_SAMPLES) -> Dict:
    """``run_comprehensive_xai_pipeline`` (XAI.py:2663-3297) without the plots and the saving stage: the reference's ``results``
    dictionary from stage 1 (``attribution_stage``), stage 2 (``intervention_stage``), Time-SHAP, Grad-CAM, the CFI collection
    of :3178-3186, ``statistical_validation`` and ``sanity_check`` on the last frame.  Every stage draws from ``seed``: two
    runs give the same report.  ``visualizations`` stays an empty list.  Only too few CFI values are recorded as
    ``{'error': 'Insufficient data'}`` (:3221); a library error propagates instead of becoming a string in the report."""
    from datetime import datetime
    frames = _as_batch(trajectory)
    if frames.shape[0] != len(timesteps):
        raise ValueError(f"{frames.shape[0]} frames but {len(timesteps)} timesteps")
    types = list(intervention_types)
    results: Dict = {
        "metadata": {
            "target_class_id": target_class_id, "target_class_name": target_class_name, "n_timesteps": frames.shape[0],
            "timesteps": timesteps, "analysis_timestamp": datetime.now().isoformat(), "seed": seed,
            "parameters": {"top_k_percent": TOP_K_PERCENT, "bottom_k_percent": BOTTOM_K_PERCENT, "ig_n_steps": ig_steps,
                           "shap_n_samples": shap_samples, "intervention_types": types, "alpha_level": ALPHA_LEVEL},
        },
        "visualizations": [],
    }
    xai_maps, region_data = attribution_stage(classifier, frames, timesteps, target_class_id, ig_steps=ig_steps,
                                              shap_samples=shap_samples, k_percent=TOP_K_PERCENT, seed=seed)
    results["xai_maps"], results["region_analysis"] = xai_maps, region_data
    interventions, cfi = intervention_stage(classifier, frames, timesteps, region_data, target_class_id, types, seed=seed)
    results["interventions"], results["cfi_analysis"] = interventions, cfi

    importance, raw = compute_time_shap(classifier, frames, timesteps, target_class_id)
    imp_idx = int(np.argmax(importance))
    results["time_shap"] = {"importance": importance, "raw_data": raw, "most_important_timestep": timesteps[imp_idx],
                            "most_important_index": imp_idx}

    cams = compute_grad_cam(classifier, frames, timesteps, target_class_id)
    results["gradcam_summary"] = cams.pop("summary")
    results["gradcam"] = cams
    results["gradcam_most_important"] = {"timestep": float(timesteps[imp_idx]), "index": imp_idx,
                                         "gradcam": cams[_step_key(timesteps[imp_idx])]}

    top_k_shifts, bottom_k_shifts = [], []
    for step_cfi in cfi.values():
        for intervention_key, entry in step_cfi.items():
            if "top_k" in intervention_key:
                top_k_shifts.append(entry["target_class_analysis"]["cfi"])
            elif "bottom_k" in intervention_key:
                bottom_k_shifts.append(entry["target_class_analysis"]["cfi"])
    try:
        results["statistical_validation"] = statistical_validation(top_k_shifts, bottom_k_shifts, alpha=ALPHA_LEVEL,
                                                                   n_bootstrap=N_BOOTSTRAP, n_permutations=N_PERMUTATIONS,
                                                                   seed=seed, device=classifier.device)
    except ValueError as e:
        if str(e) != "Insufficient data":
            raise
        results["statistical_validation"] = {"error": "Insufficient data"}

    results["sanity_checks"] = sanity_check(classifier, frames[-1:], target_class_id, n_trials=3, randomization_strength=0.01,
                                            seed=seed)
    return results
