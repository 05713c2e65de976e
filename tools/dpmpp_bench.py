#!/usr/bin/env python3
"""DPM-Solver++(2M) against DDIM on one MI355X: what the step count buys, and whether a step with a history costs what a DDIM
step costs.

    python tools/dpmpp_bench.py [--batch 64] [--size 64] [--reps 5] [--limit 300] [--out FILE]

Part A, host-inclusive images/sec of Sampler.generate_seeds (seeds in, uint8 images on the host out), in host and device
noise mode: DDIM eta = 0 at T = 50, DPM-Solver++ (order 2, ODE) at T = 20 and T = 10, and its SDE variant at T = 20.
Part B, ms per step of the loop alone (run_sampling_loop, x_T and any noise buffer resident, ends in a synchronise) at T = 20:
DDIM eta = 0 against DPM-Solver++ ODE (no z either), DDIM eta = 1 against the SDE variant (a z on every step but the last),
with a resident buffer and with DeviceNoise.  The DPM-Solver++ step moves two more streams than the DDIM step (the history,
read and written); the expected result is the same ms per step within the spread of equal runs.

The protocol is tools/ddim_bench.py's: every configuration is warmed up once; then `reps` rounds run the configurations one
after the other (alternated, not in blocks), and the table gives the median and the min .. max of the equal runs beside it.
Each of the four parts (A and B, per noise source) is a process of its own under `timeout -k 10 LIMIT`; the first part that
fails or runs out of time ends the run, and nothing more is started on the GPU.  Synthetic weights: the numbers are times,
nothing here says anything about image quality.  Needs the GPU; there is no CPU path.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("e2e-host", "e2e-device", "loop-buffer", "loop-device")
DPM = "dpmsolver++"
# (scheduler, T, generate_seeds arguments)
E2E = [("ddim", 50, dict(eta=0.0)), (DPM, 20, dict()), (DPM, 10, dict()), (DPM, 20, dict(algorithm_type="sde-dpmsolver++"))]
# (label, scheduler, create_scheduler arguments, eta)
LOOP = [("ddim eta=0", "ddim", (), 0.0), ("dpmsolver++ order 2", DPM, (2, DPM), 0.0),
        ("ddim eta=1", "ddim", (), 1.0), ("sde-dpmsolver++ order 2", DPM, (2, "sde-dpmsolver++"), 0.0)]
LOOP_T, LOOP_CALLS = 20, 8


def spread(xs):
    return f"{statistics.median(xs):9.3f}   ({min(xs):.3f} .. {max(xs):.3f})"


def label(sched, T, kw):
    return f"{kw.get('algorithm_type', sched):16s} T={T:3d}"


def part_e2e(a, noise, say):
    import torch
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.weights import synthetic_unet_state_dict
    s = Sampler()
    s.add_model("NV", synthetic_unet_state_dict())
    seeds, hw = list(range(a.batch)), (a.size, a.size)
    say(f"# A. generate_seeds, host-inclusive, noise={noise}: images/sec for {a.batch} images at 3x{a.size}x{a.size}")
    times = [[] for _ in E2E]
    for sched, T, kw in E2E:                                                 # warm-up: workspace, every rule
        s.generate_seeds("NV", seeds, min(T, 8), hw, noise=noise, scheduler=sched, **kw)
    for _ in range(a.reps):
        for k, (sched, T, kw) in enumerate(E2E):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = s.generate_seeds("NV", seeds, T, hw, noise=noise, scheduler=sched, **kw)
            res.images.cpu()
            times[k].append(time.perf_counter() - t0)
            assert res.steps_done == T
    for (sched, T, kw), ts in zip(E2E, times):
        say(f"noise={noise:6s} {label(sched, T, kw)}   images/sec {spread([a.batch / t for t in ts])}"
            f"   ms/step {spread([1e3 * t / T for t in ts])}")


def part_loop(a, source, say):
    import torch
    from synt_isic_amd.sampler import DeviceNoise, Sampler, run_sampling_loop
    from synt_isic_amd.weights import synthetic_unet_state_dict
    s = Sampler()
    model = s.add_model("NV", synthetic_unet_state_dict())
    seeds, hw = list(range(a.batch)), (a.size, a.size)
    say(f"# B. run_sampling_loop alone at T = {LOOP_T}, noise source {source} (resident), {LOOP_CALLS} calls per timed window: "
        f"ms per step")
    chw = (model.config.in_channels,) + hw
    x_T = torch.randn((a.batch,) + chw, generator=torch.Generator().manual_seed(0)).to("cuda")
    rows = torch.randn((LOOP_T, a.batch) + chw, device="cuda")
    runs = []
    for name, sched_name, args, eta in LOOP:
        sched = s.create_scheduler(LOOP_T, sched_name, *args)
        table = sched.coefficient_table(eta) if sched_name == "ddim" else sched.coefficient_table()
        n_noise = int((table[:, 4] != 0).sum())
        noise = DeviceNoise(tuple(seeds)) if source == "device" else (rows[:n_noise] if n_noise else None)
        runs.append((name, sched, noise, eta, n_noise))
        run_sampling_loop(model, sched, x_T, noise, eta=eta)
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (name, sched, noise, eta, n_noise) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(LOOP_CALLS):
                run_sampling_loop(model, sched, x_T, noise, eta=eta)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / (LOOP_CALLS * LOOP_T) * 1e3)
    for (name, sched, noise, eta, n_noise), ts in zip(runs, times):
        say(f"noise={source:6s} {name:24s} T={LOOP_T} ({n_noise:2d} noisy steps)   ms/step {spread(ts)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds each part may take (its `timeout`)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--part", choices=PARTS, default=None, help="run this part in this process (what the driver starts)")
    a = ap.parse_args()

    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("dpmpp_bench needs an MI355X: nothing is measured without one")
        say = lambda text="": print(text, flush=True)
        kind, source = a.part.split("-")
        (part_e2e if kind == "e2e" else part_loop)(a, source, say)
        return

    # the driver: no GPU work of its own; one child per part, each under its own time limit, none after a failure
    lines = [f"# tools/dpmpp_bench.py --batch {a.batch} --size {a.size} --reps {a.reps}: one process per part, configurations "
             f"alternated, median (min .. max) of {a.reps} equal runs"]
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
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith(("#", "noise="))] + [""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines).rstrip("\n") + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
