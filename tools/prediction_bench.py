#!/usr/bin/env python3
"""What a v-prediction model costs beside an epsilon one on one MI355X: nothing, is the expectation -- the step kernels move
the same streams under every prediction type (v and sample drop a division), and the fused training step forms the v target
in the registers of the loss kernel it already ran.

    python tools/prediction_bench.py [--batch 64] [--train-batch 32] [--size 64] [--reps 5] [--limit 300] [--out FILE]

Part "loop": ms per step of the loop alone (run_sampling_loop, x_T resident, device noise, ends in a synchronise), an epsilon
model against a v model of the same weights, under DPM-Solver++ (SDE variant, order 2: a z on every step but the last) at
T = 20 and under DDPM at T = 250.
Part "train": ms per fused training step (train_step_fused, loss read back) at --train-batch, epsilon without weights against
v with Min-SNR gamma = 5.

The protocol is tools/dpmpp_bench.py's: every configuration is warmed up once; then `reps` rounds run the configurations one
after the other (alternated, not in blocks), and the table gives the median and the min .. max of the equal runs beside it.
Each part is a process of its own under `timeout -k 10 LIMIT`; the first part that fails or runs out of time ends the run,
and nothing more is started on the GPU.  Synthetic weights: the numbers are times, nothing here says anything about image
quality or convergence.  Needs the GPU; there is no CPU path.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("loop", "train")
TYPES = ("epsilon", "v_prediction")
# (label, scheduler, create_scheduler arguments, T, calls per timed window)
LOOP = [("sde-dpmsolver++ order 2", "dpmsolver++", (2, "sde-dpmsolver++"), 20, 4), ("ddpm", "ddpm", (), 250, 1)]
TRAIN_STEPS = 4


def spread(xs):
    return f"{statistics.median(xs):9.3f}   ({min(xs):.3f} .. {max(xs):.3f})"


def part_loop(a, say):
    import torch
    from synt_isic_amd.sampler import DeviceNoise, Sampler, run_sampling_loop
    from synt_isic_amd.weights import synthetic_unet_state_dict
    s = Sampler()
    sd = synthetic_unet_state_dict()
    models = {kind: s.add_model(kind, sd, prediction_type=kind) for kind in TYPES}
    seeds, hw = list(range(a.batch)), (a.size, a.size)
    say(f"# loop: run_sampling_loop alone, device noise, {a.batch} images at 3x{a.size}x{a.size}: ms per step")
    x_T = torch.randn((a.batch, 3) + hw, generator=torch.Generator().manual_seed(0)).to("cuda")
    runs = []
    for name, sched_name, args, T, calls in LOOP:
        sched = s.create_scheduler(T, sched_name, *args)
        for kind in TYPES:
            runs.append((name, kind, sched, T, calls))
            res = run_sampling_loop(models[kind], sched, x_T, DeviceNoise(tuple(seeds)))
            assert res.steps_done == T and res.prediction_type == kind
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (name, kind, sched, T, calls) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(calls):
                run_sampling_loop(models[kind], sched, x_T, DeviceNoise(tuple(seeds)))
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / (calls * T) * 1e3)
    for (name, kind, sched, T, calls), ts in zip(runs, times):
        say(f"loop  {name:24s} T={T:3d} {kind:12s}   ms/step {spread(ts)}")


def part_train(a, say):
    import torch
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, train_step_fused
    from synt_isic_amd.unet import HipUNet2DModel
    from synt_isic_amd.weights import synthetic_unet_state_dict
    sd = synthetic_unet_state_dict()
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    B, hw = a.train_batch, (a.size, a.size)
    g = torch.Generator().manual_seed(0)
    images = (torch.rand((B, 3) + hw, generator=g) * 2 - 1).to("cuda")
    noise = torch.randn((B, 3) + hw, generator=g).to("cuda")
    timesteps = torch.randint(0, 1000, (B,), generator=g)
    say(f"# train: train_step_fused, {B} images at 3x{a.size}x{a.size}, {TRAIN_STEPS} steps per timed window: ms per step")
    runs = []
    for kind, gamma in (("epsilon", None), ("v_prediction", 5.0)):
        model = HipUNet2DModel(prediction_type=kind)
        model.load_state_dict(sd)
        model = model.to("cuda").train()
        opt = HipAdam(model, lr=1e-4)
        runs.append((kind, gamma, model, opt))
        train_step_fused(model, scheduler, images, noise, timesteps, opt, snr_gamma=gamma)
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (kind, gamma, model, opt) in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _k in range(TRAIN_STEPS):
                train_step_fused(model, scheduler, images, noise, timesteps, opt, snr_gamma=gamma)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / TRAIN_STEPS * 1e3)
    for (kind, gamma, model, opt), ts in zip(runs, times):
        weights = "no weights" if gamma is None else f"Min-SNR gamma={gamma:g}"
        say(f"train {kind:12s} {weights:20s}   ms/step {spread(ts)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds each part may take (its `timeout`)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--part", choices=PARTS, default=None, help="run this part in this process (what the driver starts)")
    a = ap.parse_args()

    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("prediction_bench needs an MI355X: nothing is measured without one")
        say = lambda text="": print(text, flush=True)
        (part_loop if a.part == "loop" else part_train)(a, say)
        return

    # the driver: no GPU work of its own; one child per part, each under its own time limit, none after a failure
    lines = [f"# tools/prediction_bench.py --batch {a.batch} --train-batch {a.train_batch} --size {a.size} --reps {a.reps}: one "
             f"process per part, configurations alternated, median (min .. max) of {a.reps} equal runs"]
    print(lines[0], flush=True)
    status = 0
    for part in PARTS:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--batch", str(a.batch), "--train-batch", str(a.train_batch), "--size", str(a.size), "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append(f"# part {part} ended with status {r.returncode}: nothing after it was run")
            print(lines[-1], flush=True)
            status = r.returncode
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith(("#", "loop ", "train "))] + [""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines).rstrip("\n") + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
