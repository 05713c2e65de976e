#!/usr/bin/env python3
"""Where a classifier-guided step's time goes beyond plain step + stand-alone gradient walk (tools/clf_guidance_bench.py finds
the guided step 0.2 ms above that sum): per-kernel times of the three programs under `rocprofv3 --kernel-trace --stats`.

    python tools/clf_guidance_kernels.py [--batch 64] [--size 64] [--out FILE]

Three processes, one after the other, each under `timeout -k 10 200` and none after a failure: the plain DPM-Solver++ loop, the
gradient walk alone (HipMelanomaClassifier.input_gradient with per-image targets) and the classifier-guided loop, each 4 + 40
steps (or calls) at `batch` images of 3 x size x size with device noise, every one of the 44 traced.  The table sums the kernels
that run once per step (everything but the weight packing, uploads and copies of the load) and splits the guided step's excess
over plain + walk into the kernels only the UNet runs, the kernels only the classifier runs and the step kernel.  Kernel
tracing only; no counters.  Synthetic weights.  Needs the GPU and rocprofv3.
"""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODES = ("plain", "walk", "guided")
WARM, STEPS = 4, 40
ONCE = ("pack", "copyBuffer", "fillBuffer", "transpose2d")       # kernels of the load, not of a step


def child(a):
    import torch
    import clf_guidance_bench as cb
    from synt_isic_amd.sampler import ClassifierGuidance, DeviceNoise, run_sampling_loop
    s, model, clf = cb.objects(0)
    n = a.batch
    seeds, targets = tuple(range(n)), [i % 7 for i in range(n)]
    x_T = (0.5 * torch.randn((n, 3, a.size, a.size), generator=torch.Generator().manual_seed(0))).to("cuda")

    def run(T):
        sched = s.create_scheduler(T, cb.DPM)
        if a.mode == "plain":
            run_sampling_loop(model, sched, x_T, DeviceNoise(seeds))
        elif a.mode == "guided":
            run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), classifier=ClassifierGuidance(clf, targets, cb.SCALE))
        else:
            for _ in range(T):
                clf.input_gradient(x_T, targets)

    run(WARM)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(STEPS)
    torch.cuda.synchronize()
    print(f"wall {a.mode} {(time.perf_counter() - t0) / STEPS * 1e3:.3f}", flush=True)


def load(path):
    with open(path) as f:
        return {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)}


def short(name):
    return re.sub(r"\(.*", "", name).replace("void ", "")[:96]


def analyse(stats, wall, a):
    P, W, G = (stats[m] for m in MODES)
    n = WARM + STEPS
    per_step = lambda d: {k: v for k, v in d.items() if not any(w in k for w in ONCE)}      # noqa: E731
    P, W, G = per_step(P), per_step(W), per_step(G)
    ms = lambda d: sum(v[1] for v in d.values()) / n / 1e6                                    # noqa: E731
    lines = [f"# tools/clf_guidance_kernels.py --batch {a.batch} --size {a.size}: rocprofv3 --kernel-trace --stats, DPM-Solver++, device "
             f"noise, {n} steps traced per program; kernels that run once per step only",
             "program   kernel ms/step   launches/step   wall ms/step (the timed 40, under the profiler)"]
    for m, d in zip(MODES, (P, W, G)):
        lines.append(f"{m:8s}  {ms(d):13.3f}   {sum(v[0] for v in d.values()) / n:13.1f}   {wall[m]:12.3f}")
    excess = ms(G) - ms(P) - ms(W)
    lines.append(f"guided - (plain + walk), kernel time: {excess * 1e3:.1f} us per step; guided wall - guided kernel time: "
                 f"{(wall['guided'] - ms(G)) * 1e3:.1f} us per step")
    unet = sum(G[k][1] - P[k][1] for k in G if k in P and k not in W) / n / 1e3
    clf = sum(G[k][1] - W[k][1] for k in G if k in W and k not in P) / n / 1e3
    both = sum(G[k][1] - W[k][1] - P[k][1] for k in G if k in W and k in P) / n / 1e3
    step_g = sum(v[1] for k, v in G.items() if k not in P and k not in W) / n / 1e3
    step_p = sum(v[1] for k, v in P.items() if k not in G) / n / 1e3
    lines.append(f"of it: kernels only the UNet runs {unet:+.1f} us ({unet / (ms(P) * 1e3) * 100:+.1f} % of their plain time), kernels only "
                 f"the classifier runs {clf:+.1f} us ({clf / (ms(W) * 1e3) * 100:+.1f} %), kernels both run {both:+.1f} us, the step kernel "
                 f"{step_g:.1f} us guided against {step_p:.1f} us plain")
    lines.append("the largest per-kernel differences, guided - (plain + walk), us per step (same number of launches in both):")
    rows = sorted(((G[k][1] - P.get(k, (0, 0))[1] - W.get(k, (0, 0))[1]) / n / 1e3, k) for k in G if k in P or k in W)
    for d, k in sorted(rows, key=lambda r: -abs(r[0]))[:8]:
        base = (P.get(k, (0, 0))[1] + W.get(k, (0, 0))[1]) / n / 1e3
        lines.append(f"  {d:+8.1f}  of {base:8.1f}   {short(k)}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--mode", choices=MODES, default=None, help="run this program in this process (what the driver profiles)")
    a = ap.parse_args()
    if a.mode:
        child(a)
        return
    stats, wall = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for m in MODES:
            cmd = ["timeout", "-k", "10", "200", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
                   os.path.join(tmp, m), "-o", m, "--", sys.executable, os.path.abspath(__file__), "--mode", m, "--batch", str(a.batch),
                   "--size", str(a.size)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            found = glob.glob(os.path.join(tmp, m, "**", "*kernel_stats.csv"), recursive=True)
            got = re.search(rf"^wall {m} ([0-9.]+)$", r.stdout, flags=re.M)
            if r.returncode != 0 or not found or not got:
                print(r.stdout[-2000:])
                raise SystemExit(f"program {m} ended with status {r.returncode}: nothing after it was run")
            stats[m], wall[m] = load(found[0]), float(got.group(1))
    lines = analyse(stats, wall, a)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
