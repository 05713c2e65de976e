"""Times stage 2 of the explainability pipeline (counterfactual interventions + causal shift, xai/XAI.py:2822-2896) at the
reference's shape: 6 key frames x 2 regions x ['blur'] on the synthetic ResNet18.

  batched       xai.intervention_stage: one sisic_intervene launch, one classifier batch, one sisic_cfi_metrics launch
  item by item  the reference's loop through this library as it stood before those entries: per (frame, region) the blend
                with torch ops, then 2 get_per_class_score + 2 get_probabilities + 14 get_per_class_score calls (18 batch-1
                classifier forwards) and the divergences with torch ops

Usage: python tools/xai_interventions_bench.py [--sizes 128 64] [--reps 10]
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from synt_isic_amd import xai  # noqa: E402
from synt_isic_amd.classifier import HipMelanomaClassifier  # noqa: E402
from synt_isic_amd.weights import synthetic_resnet18_state_dict  # noqa: E402

DEV = "cuda"


def item_by_item(clf, frames, timesteps, region_data, target):
    out = {}
    for i in xai.key_steps(len(frames)):
        key = f"t_{timesteps[i]:.0f}"
        image = frames[i]
        for region in ("top_k", "bottom_k"):
            m = torch.from_numpy(region_data[key][region]["mask"]).float().to(DEV)[None, None]
            blurred = torch.cat([F.avg_pool2d(image[:, c:c + 1], 5, 1, 2) for c in range(3)], dim=1)
            mod = torch.clamp(image * (1 - m) + blurred * m, -1, 1)
            so, sm = clf.get_per_class_score(image, target), clf.get_per_class_score(mod, target)
            po, pm = clf.get_probabilities(image), clf.get_probabilities(mod)
            per_class = []
            for c in range(7):
                a, b = clf.get_per_class_score(image, c), clf.get_per_class_score(mod, c)
                per_class.append((float(a - b), float(torch.abs(a - b) / (torch.abs(a) + 1e-8))))
            mid = torch.log((po + pm) / 2 + 1e-8)
            kl = float(F.kl_div(torch.log(pm + 1e-8), po, reduction="sum"))
            js = float(0.5 * (F.kl_div(mid, po, reduction="sum") + F.kl_div(mid, pm, reduction="sum")))
            out[(key, region)] = (float(so - sm), per_class, kl, js, float(0.5 * (po - pm).abs().sum()),
                                  float((image - mod).abs().mean()))
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    clf = HipMelanomaClassifier(num_classes=7).load_state_dict(synthetic_resnet18_state_dict()).to(DEV).eval()
    for size in args.sizes:
        g = torch.Generator().manual_seed(size)
        n = 50
        frames = [(torch.randn(1, 3, size, size, generator=g) * (1.5 - 0.02 * i)).to(DEV) for i in range(n)]
        timesteps = [float(1000 - 20 * i) for i in range(n)]
        region_data = {}
        for i in xai.key_steps(n):
            attr = F.avg_pool2d(torch.randn(1, 3, size, size, generator=g), 9, 1, 4)
            region_data[f"t_{timesteps[i]:.0f}"] = {"top_k": xai.select_regions(attr, 10, "top"),
                                                     "bottom_k": xai.select_regions(attr, 10, "bottom")}
        _, cfi = xai.intervention_stage(clf, frames, timesteps, region_data, 1)
        ref = item_by_item(clf, frames, timesteps, region_data, 1)
        worst = max(abs(cfi[k][f"{r}_blur"]["target_class_analysis"]["cfi"] - v[0]) for (k, r), v in ref.items())
        b = timed(lambda: xai.intervention_stage(clf, frames, timesteps, region_data, 1), args.reps)
        s = timed(lambda: item_by_item(clf, frames, timesteps, region_data, 1), args.reps)
        print(f"{size}x{size}: 6 key frames x 2 regions x ['blur'] = {len(ref)} interventions; "
              f"batched {b[0]:.2f} ms (min {b[1]:.2f}, max {b[2]:.2f}); item by item {s[0]:.2f} ms (min {s[1]:.2f}, max {s[2]:.2f}); "
              f"ratio {s[0] / b[0]:.1f}; max |cfi batched - item| = {worst:.2e}; median of {args.reps} runs, wall clock with a "
              f"device synchronisation", flush=True)


if __name__ == "__main__":
    main()
