#!/usr/bin/env python3
"""What global-norm clipping and the EMA of the weights cost per training step on one MI355X.

    python tools/train_ema_bench.py [--steps 10] [--rounds 5] [--out FILE]

Per shape (batch 32 at 64x64, and the reference's batch 2 at 128x128) five configurations of the same model are timed in
alternation, `rounds` times each, and the median of the rounds is reported:

    parent     HipAdam(model)                                  sisic_unet_train_step, the launches of every earlier revision
    clip       HipAdam(model, max_grad_norm=1)                 sisic_unet_train_step_ext: statistics pass + fused update pass
    ema        HipAdam(model, ema=ema)                         the EMA rides in the update pass
    both       HipAdam(model, max_grad_norm=1, ema=ema)
    ema-apart  HipAdam(model); ema.step() after every step     the EMA as a launch of its own: what the fusion buys

Two figures per configuration: ms per fused training step (wall clock over `steps` steps, synchronised at both ends), and ms
per optimizer step alone (scaler.step on the gradients the last backward left: the part the configurations differ in).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from synt_isic_amd.scheduler import HipDDPMScheduler  # noqa: E402
from synt_isic_amd.train import HipAdam, HipEMA, HipGradScaler, train_step_fused  # noqa: E402
from synt_isic_amd.unet import HipUNet2DModel  # noqa: E402
from synt_isic_amd.weights import synthetic_unet_state_dict  # noqa: E402

CONFIGS = ["parent", "clip", "ema", "both", "ema-apart"]


def run(B, size, steps, rounds, emit):
    dev = torch.device("cuda")
    m = HipUNet2DModel()
    m.load_state_dict(synthetic_unet_state_dict())
    m = m.to(dev)
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    HipAdam(m)
    ema = HipEMA(m, decay=0.9999)
    opts = {"parent": HipAdam(m, lr=1e-4), "clip": HipAdam(m, lr=1e-4, max_grad_norm=1.0), "ema": HipAdam(m, lr=1e-4, ema=ema),
            "both": HipAdam(m, lr=1e-4, max_grad_norm=1.0, ema=ema), "ema-apart": HipAdam(m, lr=1e-4)}
    scaler = HipGradScaler()
    m.train()
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.rand(B, 3, size, size, generator=g, device=dev) * 2 - 1
    noise = torch.randn(B, 3, size, size, generator=g, device=dev)
    ts = torch.randint(0, 1000, (B,), generator=g, device=dev)

    def train_step(name):
        out = train_step_fused(m, sched, images, noise, ts, opts[name], scaler)
        if name == "ema-apart":
            ema.step()
        return out

    def optimizer_step(name):
        scaler.step(opts[name])
        scaler.update()
        if name == "ema-apart":
            ema.step()

    def timed(fn, name):
        for _ in range(2):
            fn(name)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    step_ms = {c: [] for c in CONFIGS}
    opt_ms = {c: [] for c in CONFIGS}
    for _ in range(rounds):
        for c in CONFIGS:
            step_ms[c].append(timed(train_step, c))
        for c in CONFIGS:
            opt_ms[c].append(timed(optimizer_step, c))
    base_s, base_o = statistics.median(step_ms["parent"]), statistics.median(opt_ms["parent"])
    for c in CONFIGS:
        s, o = statistics.median(step_ms[c]), statistics.median(opt_ms[c])
        emit(json.dumps({"batch": B, "size": size, "config": c, "steps": steps, "rounds": rounds,
                         "train_step_ms": round(s, 4), "train_step_vs_parent_ms": round(s - base_s, 4),
                         "optimizer_step_ms": round(o, 4), "optimizer_step_vs_parent_ms": round(o - base_o, 4),
                         "train_step_ms_rounds": [round(v, 4) for v in step_ms[c]],
                         "optimizer_step_ms_rounds": [round(v, 4) for v in opt_ms[c]],
                         "grad_norm": opts[c].grad_norm}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    a = ap.parse_args()

    def emit(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    emit(f"# tools/train_ema_bench.py --steps {a.steps} --rounds {a.rounds}: medians of {a.rounds} alternated rounds, "
         f"{torch.cuda.get_device_name(0)}")
    run(32, 64, a.steps, a.rounds, emit)
    run(2, 128, a.steps, a.rounds, emit)
