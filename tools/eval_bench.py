#!/usr/bin/env python3
"""The evaluation metrics on one MI355X: the Gram kernel beside torch.matmul, and evaluate_generated end to end by stage.

    python tools/eval_bench.py [--reps 5] [--out profiles/r32/eval.txt] [--generated 5000] [--real 500] [--size 64]

Part "gram": ``ops.gram`` (mode dot) at (n, m, d) = (10000, 10000, 512), (5000, 500, 512) and (5000, 500, 12288) -- the feature
set against itself, generated against real features, generated against real pixels -- with ``torch.matmul`` of the same
operands in the same process as the yardstick (whatever library torch dispatches to; this project links none).  Per
configuration: one warm-up, then `reps` rounds that run the two one after the other (alternated, not in blocks); each timing is
a device-event pair around enough launches to fill about 50 ms.  The table gives the median and the min .. max, the rate
2 n m d / t in fp32 TFLOP/s, and that rate as a share of the 157.3 TFLOP/s f32 matrix peak; the largest difference between the
two results is printed beside it (exact fp32 products on both sides, another summation order).
Part "e2e": ``evaluate_generated`` on `generated` against `real` uint8 images of `size` x `size` with the synthetic classifier,
stage by stage (feature extraction, statistics and Frechet distance, kernel distance with 100 subsets of 500, precision /
recall, the audit), host clock around work that ends in a synchronise, medians of `reps` runs.
Synthetic weights and random images: the numbers are times; nothing here says anything about image quality.  Needs the GPU;
there is no CPU path.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX_TFLOPS = 157.3
GRAM_SHAPES = ((10000, 10000, 512), (5000, 500, 512), (5000, 500, 12288))


def spread(xs):
    return f"{statistics.median(xs):9.3f}   ({min(xs):.3f} .. {max(xs):.3f})"


def part_gram(a, say):
    import torch
    from synt_isic_amd import ops
    say("# gram. ops.gram (mode dot) beside torch.matmul of the same operands: ms per call, median (min .. max) of "
        f"{a.reps} alternated rounds")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    say(f"# ops.gram launches one workgroup per 128 x 128 output tile; the device has {cus} CUs")
    say(f"{'n':>6} {'m':>6} {'d':>6}  {'who':<13} {'ms':>28}  {'TFLOP/s':>8}  {'of f32 matrix peak':>18}  max|gram - matmul| / max|matmul|, workgroups")
    for n, m, d in GRAM_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(n + m + d)
        A = torch.randn(n, d, device="cuda", generator=g)
        B = torch.randn(m, d, device="cuda", generator=g)
        runs = {"ops.gram": lambda: ops.gram(A, B), "torch.matmul": lambda: torch.matmul(A, B.T)}
        ref = runs["torch.matmul"]()
        diff = ((runs["ops.gram"]() - ref).abs().max() / ref.abs().max()).item()
        calls = {}
        for name, fn in runs.items():                      # warm-up, and how many calls fill about 50 ms
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            calls[name] = max(1, min(200, int(0.05 / max(time.perf_counter() - t0, 1e-6))))
        times = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, fn in runs.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(calls[name]):
                    fn()
                stop.record()
                stop.synchronize()
                times[name].append(start.elapsed_time(stop) / calls[name])
        for name in runs:
            tf = 2.0 * n * m * d / (statistics.median(times[name]) * 1e-3) / 1e12
            say(f"{n:>6} {m:>6} {d:>6}  {name:<13} {spread(times[name]):>28}  {tf:8.1f}  {100 * tf / PEAK_F32_MATRIX_TFLOPS:17.1f}%"
                + (f"  {diff:.2e}, {-(-n // 128) * -(-m // 128)} workgroups" if name == "ops.gram" else ""))
        del A, B, ref


def part_e2e(a, say):
    import numpy as np
    import torch
    from synt_isic_amd import evaluate as ev
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    clf = HipMelanomaClassifier(num_classes=7)
    clf.load_state_dict(synthetic_resnet18_state_dict())
    clf = clf.to("cuda").eval()
    rng = np.random.default_rng(0)
    gen = torch.from_numpy(rng.integers(0, 256, (a.generated, a.size, a.size, 3), dtype=np.uint8)).to("cuda")
    real = torch.from_numpy(rng.integers(0, 256, (a.real, a.size, a.size, 3), dtype=np.uint8)).to("cuda")
    subset = min(500, a.real, a.generated)
    state = {}

    def features():
        state["Fg"], state["Fr"] = ev.extract_features(clf, gen), ev.extract_features(clf, real)

    def statistics_and_frechet():
        state["fd"] = ev.frechet_distance(ev.FeatureStats.from_features(state["Fg"]), ev.FeatureStats.from_features(state["Fr"]))

    stages = (("feature extraction", features),
              ("statistics + Frechet distance", statistics_and_frechet),
              (f"kernel distance, 100 subsets of {subset}", lambda: ev.kernel_distance(state["Fg"], state["Fr"], subset_size=subset)),
              ("precision / recall, k = 3", lambda: ev.precision_recall(state["Fg"], state["Fr"], k=3)),
              ("memorisation audit (pixels + features)",
               lambda: ev.memorisation_audit(gen, real, features=(state["Fg"], state["Fr"]))),
              ("evaluate_generated, all of it", lambda: ev.evaluate_generated(clf, gen, real, k=3, kid_subset=subset)))
    say("")
    say(f"# e2e. evaluate_generated, {a.generated} generated against {a.real} real uint8 images of {a.size}x{a.size}, synthetic "
        f"classifier: ms per stage, median (min .. max) of {a.reps} runs after one warm-up")
    times = {name: [] for name, _ in stages}
    for rep in range(a.reps + 1):
        for name, fn in stages:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
    for name, _ in stages:
        say(f"{name:<44} {spread(times[name])}")


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--generated", type=int, default=5000)
    p.add_argument("--real", type=int, default=500)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--part", choices=("gram", "e2e", "all"), default="all")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32", "eval.txt"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_bench.py measures on an MI355X: no GPU found, nothing measured")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# tools/eval_bench.py --reps {a.reps} --generated {a.generated} --real {a.real} --size {a.size} on "
        f"{torch.cuda.get_device_name(0)}")
    if a.part in ("gram", "all"):
        part_gram(a, say)
    if a.part in ("e2e", "all"):
        part_e2e(a, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
