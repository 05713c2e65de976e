"""Plain-torch float64 restatement of stage 2 of the explainability pipeline, written from the formulas in include/sisic.h
(sisic_intervene, sisic_cfi_metrics) and the description of the region selection: what the tests of
synt_isic_amd.xai.select_regions / counterfactual_intervention / compute_causal_shift / intervention_stage compare against.

Nothing here touches the GPU or the library.  scipy is imported only by ``regions_scipy`` (the fixture generator and, where
scipy is installed, the live comparison)."""
import numpy as np
import torch
import torch.nn.functional as F

TYPES = ("noise", "gaussian_noise", "zero", "mean", "blur", "inpaint", "shuffle")


# ---- regions ---------------------------------------------------------------------------------------------------------------
def region_cases():
    """(seed, H, pool, region_type, connectivity, cleanup) of tests/golden/xai_regions.npz, in its row order"""
    return [(s, H, ks, rt, conn, cl) for s in range(4) for H in (64, 128) for ks in (1, 9, 15) for rt in ("top", "bottom")
            for conn in (4, 8) for cl in (True, False)]


def region_input(seed: int, H: int, pool: int) -> torch.Tensor:
    x = torch.randn(1, 3, H, H, generator=torch.Generator().manual_seed(seed))
    return F.avg_pool2d(x, pool, 1, pool // 2)


def attribution_magnitude(attribution) -> np.ndarray:
    a = attribution.detach().cpu().numpy() if torch.is_tensor(attribution) else np.asarray(attribution)
    if a.ndim == 4:
        a = a[0]
    return np.linalg.norm(a, axis=0) if a.ndim == 3 else np.abs(a)


def regions_scipy(attribution, k_percent=10, region_type="top", cleanup=True, connectivity=8):
    """(mask, threshold) with scipy.ndimage doing the morphology: closing x2, opening x1, components below
    max(10, 1% of the map) removed"""
    from scipy import ndimage
    mag = attribution_magnitude(attribution)
    if region_type == "top":
        thr = np.percentile(mag.ravel(), 100 - k_percent)
        mask = mag >= thr
    else:
        thr = np.percentile(mag.ravel(), k_percent)
        mask = mag <= thr
    if cleanup:
        st = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
        mask = ndimage.binary_opening(ndimage.binary_closing(mask, structure=st, iterations=2), structure=st, iterations=1)
        labels, count = ndimage.label(mask, structure=st)
        if count:
            sizes = ndimage.sum(mask, labels, range(1, count + 1))
            mask = np.isin(labels, 1 + np.flatnonzero(sizes >= max(10, int(0.01 * mask.size))))
    return mask, thr


FLOAT_STATS = ("actual_percentage", "mean_attribution", "std_attribution", "mean_attribution_selected",
               "std_attribution_selected", "max_attribution_selected", "min_attribution_selected")


def region_statistics(attribution, mask: np.ndarray, threshold, k_percent=10) -> dict:
    mag = attribution_magnitude(attribution)
    n = int(mask.sum())
    inside = mag[mask]
    return {
        "total_pixels": mag.size, "selected_pixels": n, "target_percentage": k_percent,
        "actual_percentage": n / mag.size * 100, "threshold_value": threshold,
        "mean_attribution": np.mean(mag), "std_attribution": np.std(mag),
        "mean_attribution_selected": np.mean(inside) if n else 0, "std_attribution_selected": np.std(inside) if n else 0,
        "max_attribution_selected": np.max(inside) if n else 0, "min_attribution_selected": np.min(inside) if n else 0,
    }


def load_region_fixture(path):
    """{case: (mask bool [H,H], threshold, selected_pixels, float statistics [7])} of tests/golden/xai_regions.npz"""
    z = np.load(path)
    out = {}
    rows = {64: 0, 128: 0}
    for i, case in enumerate(region_cases()):
        H = case[1]
        packed = z[f"masks{H}"][rows[H]]
        rows[H] += 1
        mask = np.unpackbits(packed)[:H * H].reshape(H, H).astype(bool)
        out[case] = (mask, z["threshold"][i], int(z["selected"][i]), z["float_stats"][i])
    assert [tuple(r) for r in z["cases"].tolist()] == [(s, H, ks, int(rt == "top"), conn, int(cl)) for s, H, ks, rt, conn, cl
                                                       in region_cases()], "fixture rows are not region_cases()"
    return out


def key_steps(n: int):
    """first, middle and the last four frames as indices 0 .. n-1, negative ones counted from the end, repeats dropped"""
    out = []
    for i in (0, n // 2, n - 4, n - 3, n - 2, n - 1):
        if n > 0 and i % n not in out:
            out.append(i % n)
    return out


# ---- interventions ---------------------------------------------------------------------------------------------------------
def shuffle_index(mask: torch.Tensor, channels: int, seed: int) -> torch.Tensor:
    """int64 [C, H*W]: per channel one torch.randperm over the masked pixels from a CPU generator seeded with ``seed``"""
    g = torch.Generator().manual_seed(seed)
    flat = mask.reshape(-1).bool()
    inside = torch.nonzero(flat).reshape(-1)
    src = torch.arange(flat.numel()).repeat(channels, 1)
    if inside.numel() > 1:
        for c in range(channels):
            src[c, inside] = inside[torch.randperm(inside.numel(), generator=g)]
    return src


def intervention(image: torch.Tensor, kind: str, blur_kernel=5, noise_std=0.5, z=None, src_index=None, dtype=torch.float64):
    """the intervention [C,H,W] for image [C,H,W]; z [C,H,W]: the normals of the noise types; src_index [C,H*W]"""
    x = image.to(dtype)
    C, H, W = x.shape
    if kind == "noise":
        return z.to(dtype) * noise_std
    if kind == "gaussian_noise":
        return z.to(dtype) * max(noise_std, 0.5 * x.std(unbiased=True).item())
    if kind == "zero":
        return torch.zeros_like(x)
    if kind == "mean":
        return x.mean(dim=(1, 2), keepdim=True).expand_as(x).clone()
    if kind in ("blur", "inpaint"):
        k = 5 if kind == "inpaint" else (blur_kernel + 1 if blur_kernel % 2 == 0 else blur_kernel)
        return F.avg_pool2d(x[None], k, 1, k // 2, count_include_pad=True)[0]
    if kind == "shuffle":
        return torch.gather(x.reshape(C, H * W), 1, src_index.long()).reshape(C, H, W)
    raise ValueError(kind)


def intervene(image, mask, kind, dtype=torch.float64, **kw):
    """(modified, intervention, [coverage, mean |image - modified|, max |image - modified|, mean |intervention|])"""
    x = image.to(dtype)
    m = mask.to(dtype)[None]
    iv = intervention(image, kind, dtype=dtype, **kw)
    mod = torch.clamp(x * (1 - m) + iv * m, -1, 1)
    d = (x - mod).abs()
    stats = torch.stack([m.expand_as(x).mean(), d.mean(), d.max(), iv.abs().mean()])
    return mod, iv, stats


# ---- causal shift ----------------------------------------------------------------------------------------------------------
def cfi_rows(logits_orig: torch.Tensor, logits_mod: torch.Tensor, job_frame) -> torch.Tensor:
    """float64 [J, 6n+7] in the layout of sisic_cfi_metrics, from the fp32 logits"""
    rows = []
    for j, f in enumerate(job_frame):
        po = torch.softmax(logits_orig[f].double(), 0)
        pm = torch.softmax(logits_mod[j].double(), 0)
        so, sm = torch.log(po + 1e-8), torch.log(pm + 1e-8)
        cfi = so - sm
        delta = cfi.abs() / (so.abs() + 1e-8)
        per = torch.stack([so, sm, cfi, delta, po, pm], dim=1).reshape(-1)
        mid = torch.log((po + pm) / 2 + 1e-8)
        kl = torch.xlogy(po, po).sum() - (po * sm).sum()
        js = 0.5 * ((torch.xlogy(po, po) - po * mid).sum() + (torch.xlogy(pm, pm) - pm * mid).sum())
        tv = 0.5 * (po - pm).abs().sum()
        tail = torch.stack([po.argmax().double(), pm.argmax().double(), po.max(), pm.max(), kl, js, tv])
        rows.append(torch.cat([per, tail]))
    return torch.stack(rows)
