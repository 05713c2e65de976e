"""Times the tail of the explainability pipeline (stages 1, 4-6 and the driver of synt_isic_amd.xai) on the synthetic ResNet18.

  1. one weight randomisation: classifier.randomize_weights (generated on the device in folded form) against the same weights
     through load_state_dict(randomized_state_dict(...)) -- the host route: float64 BatchNorm fold on the host, uploads of the
     folded raw and transposed filters, packing; with and without a host torch.randn of the 11.2 M values in front
  2. xai.sanity_check with its defaults (3 trials, 20 / 15 IG steps) end to end by both routes
  3. xai.statistical_validation (one sisic_resample_diffs launch + numpy) against the reference's two interpreter loops
     (XAI.py:1845-1904) restated in numpy, 42 against 42 values, 1 000 bootstrap and 10 000 permutation resamples
  4. xai.run_pipeline on a 50-frame 64x64 trajectory, and its stages one by one

Every figure is wall clock around work that ends in a device synchronisation, after a warm-up run of the same call; the two
sides of a comparison alternate (A B A B A B) and all three runs are printed.

Usage: python tools/xai_pipeline_bench.py [--runs 3] [--frames 50] [--size 64]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from synt_isic_amd import xai  # noqa: E402
from synt_isic_amd.classifier import HipMelanomaClassifier  # noqa: E402
from synt_isic_amd.weights import synthetic_resnet18_state_dict  # noqa: E402

DEV = "cuda"
NV = 1


def once(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(sides, runs):
    """{name: [ms per run]}: a warm-up of every side, then the sides in turn, ``runs`` times"""
    for fn in sides.values():
        once(fn)
    out = {name: [] for name in sides}
    for _ in range(runs):
        for name, fn in sides.items():
            out[name].append(once(fn))
    return out


def show(title, times):
    for name, ts in times.items():
        print(f"  {title}: {name}: " + ", ".join(f"{t:.2f}" for t in ts) + f" ms (median {sorted(ts)[len(ts) // 2]:.2f})", flush=True)


class HostRouteClassifier(HipMelanomaClassifier):
    """the same randomisation through the state-dict route: what the sanity check would cost without sisic_resnet_randomize"""

    def randomize_weights(self, seed, trial, strength=0.01):
        if not hasattr(self, "_loaded"):
            self._loaded = {k: v.cpu() for k, v in self.state_dict().items()}
        sd = dict(self._loaded)
        for name, value in self._loaded.items():
            if value.dim() > 1:
                sd[name] = torch.randn(value.shape, generator=torch.Generator().manual_seed(seed * 1000 + trial)) * strength
        self.load_state_dict(sd)

    def restore_weights(self):
        self.load_state_dict(self._loaded)


def reference_loops(top_k, bottom_k, n_bootstrap=1000, n_permutations=10000):
    """the two interpreter loops of XAI.py:1845-1904 as the reference runs them (numpy's global generator)"""
    diffs = []
    for _ in range(n_bootstrap):
        diffs.append(np.mean(np.random.choice(top_k, len(top_k), replace=True)) -
                     np.mean(np.random.choice(bottom_k, len(bottom_k), replace=True)))
    combined = np.concatenate([top_k, bottom_k])
    perm = []
    for _ in range(n_permutations):
        np.random.shuffle(combined)
        perm.append(np.mean(combined[:len(top_k)]) - np.mean(combined[len(top_k):]))
    return np.array(diffs), np.array(perm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xai_pipeline_bench needs an MI355X: there is no CPU path to time")
    sd = synthetic_resnet18_state_dict()
    clf = HipMelanomaClassifier(num_classes=7).load_state_dict(dict(sd)).to(DEV).eval()
    host = HostRouteClassifier(num_classes=7).load_state_dict(dict(sd)).to(DEV).eval()
    g = torch.Generator().manual_seed(0)
    image = (torch.rand(1, 3, args.size, args.size, generator=g) * 2 - 1).to(DEV)

    print("1. one weight randomisation (11.2 M values, 21 tensors)")
    rsd = {k: v.cpu() for k, v in clf.randomized_state_dict(0, 0, 0.01).items()}
    other = HipMelanomaClassifier(num_classes=7).load_state_dict(dict(sd)).to(DEV).eval()
    show("randomise", alternate({
        "device (randomize_weights)": lambda: clf.randomize_weights(0, 0, 0.01),
        "host route, load_state_dict of a ready state dict": lambda: other.load_state_dict(rsd),
        "host route, torch.randn on the host + load_state_dict": lambda: host.randomize_weights(0, 0, 0.01),
    }, args.runs))
    show("restore", alternate({"device handle (restore_weights)": clf.restore_weights,
                               "host route (load_state_dict of the original)": host.restore_weights}, args.runs))

    print("2. sanity_check, defaults (3 trials, 20 / 15 IG steps; 165 classifier backward passes)")
    show("sanity_check", alternate({"device randomisation": lambda: xai.sanity_check(clf, image, NV),
                                    "host route": lambda: xai.sanity_check(host, image, NV)}, args.runs))

    print("3. statistics, 42 against 42 values, 1 000 bootstrap + 10 000 permutation resamples")
    rng = np.random.default_rng(0)
    top, bottom = rng.normal(0.3, 0.2, 42), rng.normal(0.1, 0.2, 42)
    show("resampling", alternate({"statistical_validation (classical tests included)": lambda: xai.statistical_validation(top, bottom),
                                  "the reference's two loops in numpy (resampling only)": lambda: reference_loops(top, bottom)},
                                 args.runs))

    n, size = args.frames, args.size
    print(f"4. run_pipeline, {n} frames of {size}x{size}, intervention_types ['blur'], IG 50 steps, SHAP 512 samples")
    smooth = F.avg_pool2d(torch.randn(n, 3, size + 8, size + 8, generator=g), 9, stride=1)
    frames = (smooth / smooth.abs().amax(dim=(1, 2, 3), keepdim=True) +
              torch.randn(n, 3, size, size, generator=g) * torch.linspace(1.0, 0.0, n).view(-1, 1, 1, 1)).to(DEV)
    timesteps = [float(round(999 * (1 - i / max(1, n - 1)))) for i in range(n)]
    show("whole", alternate({"run_pipeline": lambda: xai.run_pipeline(clf, frames, timesteps, NV, "NV")}, args.runs))
    state = {}

    def stage1():
        state["maps"], state["regions"] = xai.attribution_stage(clf, frames, timesteps, NV)

    def stage2():
        state["cfi"] = xai.intervention_stage(clf, frames, timesteps, state["regions"], NV)[1]

    def stats():
        top_k = [e["target_class_analysis"]["cfi"] for s in state["cfi"].values() for k, e in s.items() if "top_k" in k]
        bottom_k = [e["target_class_analysis"]["cfi"] for s in state["cfi"].values() for k, e in s.items() if "bottom_k" in k]
        xai.statistical_validation(top_k, bottom_k)

    stage1()
    stage2()
    show("stages", alternate({
        "1 attribution_stage": stage1, "2 intervention_stage": stage2,
        "3 time-shap": lambda: xai.compute_time_shap(clf, frames, timesteps, NV),
        "3b grad-cam": lambda: xai.compute_grad_cam(clf, frames, timesteps, NV),
        "4-5 statistical_validation": stats,
        "6 sanity_check": lambda: xai.sanity_check(clf, frames[-1:], NV),
    }, args.runs))


if __name__ == "__main__":
    main()
