#!/usr/bin/env python3
"""Classifier guidance on one MI355X: what the classifier's gradient walk adds to a sampling step.

    python tools/clf_guidance_bench.py [--batch 64] [--size 64] [--reps 5] [--limit 420] [--out FILE]

Part "loop", ms per step of the loop alone (run_sampling_loop on device noise, x_T resident, ends in a synchronise) at `batch`
images of 3 x size x size: plain against classifier-guided under DPM-Solver++ (order 2, ODE) at T = 20 and under DDPM at
T = 250, the guided run eagerly and graph-replayed; the gradient walk alone (HipMelanomaClassifier.input_gradient with
per-image targets) at that batch; and the same guided DPM-Solver++ run through the Python loop of
tests/test_gpu_clf_guide.py (model, input_gradient, ops.clf_guide_eps, scheduler.step per step) -- what the single library
call and the replay save.
Part "e2e", host-inclusive images/sec of Sampler.generate_seeds (seeds in, uint8 images on the host out), plain against
guided, under the same two rules.

The protocol is tools/cfg_bench.py's: every configuration is warmed up once; then `reps` rounds run the configurations one
after the other (alternated, not in blocks), and the table gives the median and the min .. max of the equal runs beside it.
Each part is a process of its own under `timeout -k 10 LIMIT`; the first part that fails or runs out of time ends the run, and
nothing more is started on the GPU.  Synthetic weights: the numbers are times, nothing here says anything about image quality
or class fidelity.  Needs the GPU; there is no CPU path.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("loop", "e2e")
DPM = "dpmsolver++"
RULES = ((DPM, 20, 4), ("ddpm", 250, 1))          # (rule, T, calls per timed window)
SCALE = 2.0


def spread(xs):
    return f"{statistics.median(xs):9.3f}   ({min(xs):.3f} .. {max(xs):.3f})"


def objects(graph=None):
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.weights import synthetic_resnet18_state_dict, synthetic_unet_state_dict
    s = Sampler()
    m = s.add_model("NV", synthetic_unet_state_dict())
    if graph is not None:
        m.set_graph_mode(graph)
    clf = HipMelanomaClassifier(num_classes=7)
    clf.load_state_dict(synthetic_resnet18_state_dict())
    clf = clf.to("cuda").eval()
    s.set_classifier(clf, {"NV": 1})
    return s, m, clf


def part_loop(a, say):
    import torch
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import ClassifierGuidance, DeviceNoise, run_sampling_loop
    s, model, clf = objects(0)
    _, gmodel, gclf = objects(1)
    n, hw = a.batch, (a.size, a.size)
    chw = (3,) + hw
    npi = 3 * a.size * a.size
    seeds, targets = tuple(range(n)), [i % 7 for i in range(n)]
    x_T = (0.5 * torch.randn((n,) + chw, generator=torch.Generator().manual_seed(0))).to("cuda")
    say(f"# loop. run_sampling_loop alone, device noise, {n} images at 3x{a.size}x{a.size}: ms per step")

    def python_loop(sched):
        sched.set_timesteps(len(sched.timesteps))                       # a new run: DPM-Solver++ starts without a history
        tab = sched.coefficient_table()
        x = x_T.clone()
        for i, t in enumerate(sched.timesteps):
            eps = model(x, t).sample
            g, _ = clf.input_gradient(x, targets)
            eps = ops.clf_guide_eps(eps, g, float(tab[i, 0]), SCALE)
            vn = ops.noise_fill(seeds, npi, i).reshape(x.shape) if float(tab[i, 4]) != 0.0 else None
            x = sched.step(eps, t, x, variance_noise=vn).prev_sample
        return x

    runs = []
    for rule, T, calls in RULES:
        sched = s.create_scheduler(T, rule)
        runs.append((f"{rule} T={T} plain", T * calls, calls, lambda sched=sched: run_sampling_loop(model, sched, x_T, DeviceNoise(seeds))))
        runs.append((f"{rule} T={T} guided (eager)", T * calls, calls,
                     lambda sched=sched: run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), classifier=ClassifierGuidance(clf, targets, SCALE))))
        runs.append((f"{rule} T={T} guided (graph)", T * calls, calls,
                     lambda sched=sched: run_sampling_loop(gmodel, sched, x_T, DeviceNoise(seeds), classifier=ClassifierGuidance(gclf, targets, SCALE))))
    psched = s.create_scheduler(20, DPM)
    runs.append((f"{DPM} T=20 guided, Python loop", 20, 1, lambda: python_loop(psched)))
    runs.append(("gradient walk alone (per call)", 20, 20, lambda: clf.input_gradient(x_T, targets)))
    for _, _, calls, fn in runs:
        fn()
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (_, steps, calls, fn) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(calls):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps * 1e3)
    for (name, _, _, _), ts in zip(runs, times):
        say(f"loop  {name:40s} ms/step {spread(ts)}")


def part_e2e(a, say):
    import torch
    s, _, _ = objects()
    seeds, hw = list(range(a.batch)), (a.size, a.size)
    say(f"# e2e. generate_seeds, host-inclusive, noise=device: images/sec for {a.batch} images at 3x{a.size}x{a.size}")
    runs = []
    for rule, T, _ in RULES:
        runs.append((f"{rule} T={T} plain", rule, T, None))
        runs.append((f"{rule} T={T} guided", rule, T, SCALE))
    for _, rule, T, cs in runs:
        s.generate_seeds("NV", seeds, 4, hw, noise="device", scheduler=rule, classifier_scale=cs)
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (_, rule, T, cs) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = s.generate_seeds("NV", seeds, T, hw, noise="device", scheduler=rule, classifier_scale=cs)
            res.images.cpu()
            times[k].append(time.perf_counter() - t0)
            assert res.steps_done == T
    for (name, _, T, _), ts in zip(runs, times):
        say(f"e2e   {name:40s} images/sec {spread([a.batch / t for t in ts])}   ms/step {spread([1e3 * t / T for t in ts])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds each part may take (its `timeout`)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--part", choices=PARTS, default=None, help="run this part in this process (what the driver starts)")
    a = ap.parse_args()

    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("clf_guidance_bench needs an MI355X: nothing is measured without one")
        say = lambda text="": print(text, flush=True)      # noqa: E731
        (part_loop if a.part == "loop" else part_e2e)(a, say)
        return

    # the driver: no GPU work of its own; one child per part, each under its own time limit, none after a failure
    lines = [f"# tools/clf_guidance_bench.py --batch {a.batch} --size {a.size} --reps {a.reps}: one process per part, "
             f"configurations alternated, median (min .. max) of {a.reps} equal runs; classifier scale {SCALE}, synthetic weights"]
    print(lines[0], flush=True)
    status = 0
    for part in PARTS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--batch", str(a.batch), "--size", str(a.size), "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append(f"# part {part} ended with status {r.returncode}: nothing after it was run")
            print(lines[-1], flush=True)
            status = r.returncode
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith(("#", "loop ", "e2e "))] + [""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines).rstrip("\n") + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
