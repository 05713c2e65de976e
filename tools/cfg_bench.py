#!/usr/bin/env python3
"""Class-conditional sampling and classifier-free guidance on one MI355X: what the labels cost (nothing, is the expectation)
and what guidance costs (a step at twice the batch).

    python tools/cfg_bench.py [--batch 64] [--size 64] [--reps 5] [--limit 300] [--out FILE]

Part A, host-inclusive images/sec of Sampler.generate_seeds (seeds in, uint8 images on the host out) under DPM-Solver++
(order 2, ODE) at T = 20, in host and device noise mode: the unconditional model, the conditional model at guidance_scale 1
(one pass per step, labels mixed over the batch) and at guidance_scale 3 (one pass per step at twice the batch).
Part B, ms per step of the loop alone (run_sampling_loop, x_T and any noise buffer resident, ends in a synchronise) at T = 20
under the ODE and the SDE variant: the unconditional model at `batch` images -- the yardstick, the path an unconditional call
has always taken --, the conditional model at scale 1 at `batch` images, and at scale 3 at batch / 2 images, whose UNet pass
has the yardstick's batch.  Expected: the three within the spread of equal runs of each other.

The protocol is tools/dpmpp_bench.py's: every configuration is warmed up once; then `reps` rounds run the configurations one
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
CLASSES = ("MEL", "NV", "BCC", "AKIEC", "BKL", "DF", "VASC")
T, LOOP_CALLS = 20, 8


def spread(xs):
    return f"{statistics.median(xs):9.3f}   ({min(xs):.3f} .. {max(xs):.3f})"


def samplers(n_cond=1):
    """an unconditional sampler and n_cond conditional ones.  Part A gives each guidance scale a sampler of its own: a handle
    keeps its activation pool for one batch, and a call at scale 1 (batch B) after one at scale 3 (batch 2B) on the same handle
    releases and re-allocates it, as a change of the batch size does -- alternating the two on one handle would time that."""
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.weights import synthetic_unet_state_dict
    plain = Sampler()
    plain.add_model("NV", synthetic_unet_state_dict())
    conds = []
    for _ in range(n_cond):
        conds.append(Sampler())
        conds[-1].add_conditional_model(CLASSES, synthetic_unet_state_dict(num_class_embeds=len(CLASSES) + 1))
    return (plain, *conds)


def part_e2e(a, noise, say):
    import torch
    plain, cond1, cond3 = samplers(2)
    seeds, hw = list(range(a.batch)), (a.size, a.size)
    names = [CLASSES[i % len(CLASSES)] for i in range(a.batch)]
    runs = [("unconditional", plain, "NV", 1.0), ("conditional w=1", cond1, names, 1.0), ("conditional w=3", cond3, names, 3.0)]
    say(f"# A. generate_seeds, host-inclusive, noise={noise}, {DPM} T={T}: images/sec for {a.batch} images at 3x{a.size}x{a.size}")
    times = [[] for _ in runs]
    for _, s, cls, w in runs:                                                # warm-up: workspace, every configuration
        s.generate_seeds(cls, seeds, 8, hw, noise=noise, scheduler=DPM, guidance_scale=w)
    for _ in range(a.reps):
        for k, (_, s, cls, w) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = s.generate_seeds(cls, seeds, T, hw, noise=noise, scheduler=DPM, guidance_scale=w)
            res.images.cpu()
            times[k].append(time.perf_counter() - t0)
            assert res.steps_done == T
    for (name, _, _, _), ts in zip(runs, times):
        say(f"noise={noise:6s} {name:18s} T={T}   images/sec {spread([a.batch / t for t in ts])}"
            f"   ms/step {spread([1e3 * t / T for t in ts])}")


def part_loop(a, source, say):
    import torch
    from synt_isic_amd.sampler import DeviceNoise, Guidance, run_sampling_loop
    plain, cond = samplers()
    pm, cm = plain.models["NV"], cond.models["NV"]
    null, hw, half = len(CLASSES), (a.size, a.size), a.batch // 2
    chw = (pm.config.in_channels,) + hw
    say(f"# B. run_sampling_loop alone at T = {T}, noise source {source} (resident), {LOOP_CALLS} calls per timed window: ms per "
        f"step; the guided run has {half} images, so its UNet pass has the batch of the other two ({a.batch})")
    x_T = torch.randn((a.batch,) + chw, generator=torch.Generator().manual_seed(0)).to("cuda")
    rows = torch.randn((T, a.batch) + chw, device="cuda")
    runs = []
    for alg in (DPM, "sde-dpmsolver++"):
        sched = plain.create_scheduler(T, DPM, 2, alg)
        n_noise = int((sched.coefficient_table()[:, 4] != 0).sum())
        for name, model, n, w in (("unconditional", pm, a.batch, None), ("conditional w=1", cm, a.batch, 1.0),
                                  ("conditional w=3", cm, half, 3.0)):
            if source == "device":
                noise = DeviceNoise(tuple(range(n)))
            else:
                noise = rows[:n_noise, :n].contiguous() if n_noise else None
            g = None if w is None else Guidance([i % null for i in range(n)], null, w)
            runs.append((f"{alg} {name}", model, sched, x_T[:n].contiguous(), noise, g, n))
    for _, model, sched, x, noise, g, _ in runs:
        run_sampling_loop(model, sched, x, noise, guidance=g)
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (_, model, sched, x, noise, g, _) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(LOOP_CALLS):
                run_sampling_loop(model, sched, x, noise, guidance=g)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / (LOOP_CALLS * T) * 1e3)
    for (name, _, _, _, _, _, n), ts in zip(runs, times):
        say(f"noise={source:6s} {name:32s} images={n:3d}   ms/step {spread(ts)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds each part may take (its `timeout`)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--part", choices=PARTS, default=None, help="run this part in this process (what the driver starts)")
    a = ap.parse_args()
    if a.batch < 2 or a.batch % 2:
        raise SystemExit("--batch must be even: the guided loop of part B runs batch / 2 images")

    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("cfg_bench needs an MI355X: nothing is measured without one")
        say = lambda text="": print(text, flush=True)
        kind, source = a.part.split("-")
        (part_e2e if kind == "e2e" else part_loop)(a, source, say)
        return

    # the driver: no GPU work of its own; one child per part, each under its own time limit, none after a failure
    lines = [f"# tools/cfg_bench.py --batch {a.batch} --size {a.size} --reps {a.reps}: one process per part, configurations "
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
