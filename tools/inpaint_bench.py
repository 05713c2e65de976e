#!/usr/bin/env python3
"""What the inpainting epilogue costs on one MI355X: the edited step against the unedited one, and what RePaint's resampling
costs end to end.

    python tools/inpaint_bench.py [--batch 64] [--size 64] [--reps 5] [--limit 400] [--out FILE]

Part A, ms per step of the loop alone (run_sampling_loop with DeviceNoise, x_T, the known image and the mask resident, ends in a
synchronise): the unedited loop against the edited one (soft mask, no jumps) under DPM-Solver++ (order 2, ODE) at T = 20 and
under DDPM at T = 250.  The edited step reads two more streams than the unedited one (the known image, and the mask at a third
of its width) and draws one more normal per element (tag 5); the unedited loop issues the launches it issued before the
feature existed, so it is the comparison point.
Part B, host-inclusive images/sec of Sampler.generate_seeds (seeds, image and mask in, uint8 images on the host out) under DDPM
at T = 250 with (jump_length, n_resample) = (10, 1), 250 UNet passes, and (10, 5), 1210 passes.

The protocol is tools/dpmpp_bench.py's: every configuration is warmed up once; then `reps` rounds run the configurations one
after the other (alternated, not in blocks), and the table gives the median and the min .. max of the equal runs beside it.
Each part is a process of its own under `timeout -k 10 LIMIT`; the first part that fails or runs out of time ends the run, and
nothing more is started on the GPU.  Synthetic weights: the numbers are times, nothing here says anything about image quality.
Needs the GPU; there is no CPU path.
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
# (label, scheduler, T, calls per timed window)
LOOP = [("dpmsolver++ order 2", DPM, 20, 8), ("ddpm", "ddpm", 250, 1)]
E2E_T = 250
E2E = [(10, 1), (10, 5)]


def spread(xs):
    return f"{statistics.median(xs):9.3f}   ({min(xs):.3f} .. {max(xs):.3f})"


def inputs(a):
    import torch
    g = torch.Generator().manual_seed(0)
    chw = (3, a.size, a.size)
    x_T = torch.randn((a.batch,) + chw, generator=g).to("cuda")
    image = (torch.rand((a.batch,) + chw, generator=g) * 2 - 1).to("cuda")
    mask = torch.tensor([0.0, 1.0, 0.25, 0.7])[torch.randint(0, 4, (a.batch, 1) + chw[1:], generator=g)].to("cuda")
    return x_T, image, mask


def part_loop(a, say):
    import torch
    from synt_isic_amd.sampler import DeviceNoise, Edit, Sampler, run_sampling_loop
    from synt_isic_amd.weights import synthetic_unet_state_dict
    s = Sampler()
    model = s.add_model("NV", synthetic_unet_state_dict())
    seeds = tuple(range(a.batch))
    x_T, image, mask = inputs(a)
    say(f"# A. run_sampling_loop alone, DeviceNoise, {a.batch} images at 3x{a.size}x{a.size}: ms per step, unedited against "
        f"edited (soft mask, no jumps)")
    runs = []
    for name, sched_name, T, calls in LOOP:
        sched = s.create_scheduler(T, sched_name)
        for edited in (False, True):
            kw = dict(edit=Edit(image, mask)) if edited else {}
            runs.append((name, sched, T, calls, edited, kw))
            run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), **kw)
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (name, sched, T, calls, edited, kw) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(calls):
                res = run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), **kw)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / (calls * T) * 1e3)
            assert res.steps_done == T
    for (name, sched, T, calls, edited, kw), ts in zip(runs, times):
        say(f"loop {name:22s} T={T:3d} {'edited  ' if edited else 'unedited'}   ms/step {spread(ts)}")
    for k in range(0, len(runs), 2):
        plain, edit = statistics.median(times[k]), statistics.median(times[k + 1])
        noise_band = max(max(times[k]) - min(times[k]), max(times[k + 1]) - min(times[k + 1]))
        say(f"loop {runs[k][0]:22s} T={runs[k][2]:3d} edited - unedited = {edit - plain:+.4f} ms/step ({100 * (edit / plain - 1):+.2f} %); "
            f"spread of equal runs {noise_band:.4f} ms/step")


def part_e2e(a, say):
    import torch
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.weights import synthetic_unet_state_dict
    s = Sampler()
    s.add_model("NV", synthetic_unet_state_dict())
    seeds, hw = list(range(a.batch)), (a.size, a.size)
    _, image, mask = inputs(a)
    say(f"# B. generate_seeds, host-inclusive, noise=device, ddpm T = {E2E_T}, inpainting {a.batch} images at 3x{a.size}x{a.size}: "
        f"images/sec")
    s.generate_seeds("NV", seeds, 8, hw, noise="device", init_image=image, mask=mask, jump_length=2, n_resample=2)      # warm-up
    times, passes = [[] for _ in E2E], [0 for _ in E2E]
    for _ in range(a.reps):
        for k, (j, r) in enumerate(E2E):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = s.generate_seeds("NV", seeds, E2E_T, hw, noise="device", init_image=image, mask=mask, jump_length=j, n_resample=r)
            res.images.cpu()
            times[k].append(time.perf_counter() - t0)
            passes[k] = res.unet_passes
            assert res.steps_done == res.unet_passes
    for (j, r), ts, p in zip(E2E, times, passes):
        say(f"e2e  jump_length={j:2d} n_resample={r} ({p:4d} UNet passes)   images/sec {spread([a.batch / t for t in ts])}"
            f"   ms/pass {spread([1e3 * t / p for t in ts])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400, help="seconds each part may take (its `timeout`)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--part", choices=PARTS, default=None, help="run this part in this process (what the driver starts)")
    a = ap.parse_args()

    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("inpaint_bench needs an MI355X: nothing is measured without one")
        say = lambda text="": print(text, flush=True)       # noqa: E731
        (part_loop if a.part == "loop" else part_e2e)(a, say)
        return

    # the driver: no GPU work of its own; one child per part, each under its own time limit, none after a failure
    lines = [f"# tools/inpaint_bench.py --batch {a.batch} --size {a.size} --reps {a.reps}: one process per part, configurations "
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
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith(("#", "loop ", "e2e "))] + [""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines).rstrip("\n") + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
