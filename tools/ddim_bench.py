#!/usr/bin/env python3
"""DDIM against DDPM on one MI355X: what the step count buys, and whether a DDIM step costs what a DDPM step costs.

    python tools/ddim_bench.py [--batch 64] [--size 64] [--reps 3] [--out FILE]

Part A, host-inclusive images/sec of Sampler.generate_seeds (seeds in, uint8 images on the host out), in host and device
noise mode: DDPM T = 1000, DDIM eta = 0 at T = 100, 50, 20, DDIM eta = 1 at T = 50, DDPM T = 50.
Part B, ms per step of the loop alone (run_sampling_loop, x_T and any noise buffer resident, ends in a synchronise) at T = 50:
DDPM, DDIM eta = 1 (the same bytes: eps, x, z in, x out) and DDIM eta = 0 (no z), with a resident buffer and with DeviceNoise.

Every configuration is warmed up once; then `reps` rounds run the configurations one after the other (alternated, not in
blocks), and the table gives the median and the min .. max of the equal runs beside it.  Synthetic weights: the numbers are
times, nothing here says anything about image quality.  Needs the GPU; there is no CPU path.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from synt_isic_amd.sampler import DeviceNoise, Sampler, run_sampling_loop  # noqa: E402
from synt_isic_amd.weights import synthetic_unet_state_dict  # noqa: E402

E2E = [("ddpm", 1000, 0.0), ("ddim", 100, 0.0), ("ddim", 50, 0.0), ("ddim", 20, 0.0), ("ddim", 50, 1.0), ("ddpm", 50, 0.0)]
LOOP = [("ddpm", 0.0), ("ddim", 1.0), ("ddim", 0.0)]
LOOP_T, LOOP_CALLS = 50, 4


def spread(xs):
    return f"{statistics.median(xs):9.3f}   ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ddim_bench needs an MI355X: nothing is measured without one")
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    s = Sampler()
    model = s.add_model("NV", synthetic_unet_state_dict())
    seeds, hw = list(range(a.batch)), (a.size, a.size)
    say(f"# tools/ddim_bench.py --batch {a.batch} --size {a.size} --reps {a.reps}: {torch.cuda.get_device_name(0)}, one process, "
        f"configurations alternated, median (min .. max) of {a.reps} equal runs")
    say(f"# A. generate_seeds, host-inclusive: images/sec for {a.batch} images at 3x{a.size}x{a.size}")
    for noise in ("host", "device"):
        times = {c: [] for c in E2E}
        for sched, T, eta in E2E:                                            # warm-up: workspace, staging buffers, every rule
            s.generate_seeds("NV", seeds, min(T, 8), hw, noise=noise, scheduler=sched, eta=eta)
        for _ in range(a.reps):
            for c in E2E:
                sched, T, eta = c
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = s.generate_seeds("NV", seeds, T, hw, noise=noise, scheduler=sched, eta=eta)
                res.images.cpu()
                times[c].append(time.perf_counter() - t0)
                assert res.steps_done == T
        for (sched, T, eta), ts in times.items():
            say(f"noise={noise:6s} {sched} T={T:4d} eta={eta:.0f}   images/sec {spread([a.batch / t for t in ts])}"
                f"   ms/step {spread([1e3 * t / T for t in ts])}")
    say()
    say(f"# B. run_sampling_loop alone at T = {LOOP_T}, noise resident, {LOOP_CALLS} calls per timed window: ms per step")
    chw = (model.config.in_channels,) + hw
    x_T = torch.randn((a.batch,) + chw, generator=torch.Generator().manual_seed(0)).to("cuda")
    rows = torch.randn((LOOP_T, a.batch) + chw, device="cuda")
    for source in ("buffer", "device"):
        runs = {}
        for sched_name, eta in LOOP:
            sched = s.create_scheduler(LOOP_T, sched_name)
            table = sched.coefficient_table(eta) if sched_name == "ddim" else sched.coefficient_table()
            n_noise = int((table[:, 4] != 0).sum())
            noise = DeviceNoise(tuple(seeds)) if source == "device" else (rows[:n_noise] if n_noise else None)
            runs[(sched_name, eta)] = (sched, noise)
            run_sampling_loop(model, sched, x_T, noise, eta=eta)
        times = {c: [] for c in runs}
        for _ in range(a.reps):
            for c, (sched, noise) in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _k in range(LOOP_CALLS):
                    run_sampling_loop(model, sched, x_T, noise, eta=c[1])
                torch.cuda.synchronize()
                times[c].append((time.perf_counter() - t0) / (LOOP_CALLS * LOOP_T) * 1e3)
        for (sched_name, eta), ts in times.items():
            say(f"noise={source:6s} {sched_name} T={LOOP_T} eta={eta:.0f}   ms/step {spread(ts)}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
