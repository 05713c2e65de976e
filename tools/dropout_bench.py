#!/usr/bin/env python3
"""What ResnetBlock2D dropout costs per training step on one MI355X.

    python tools/dropout_bench.py [--steps 20] [--rounds 5] [--out profiles/r21/dropout.txt]

Per shape (batch 32 at 64x64, and the reference's batch 2 at 128x128) three configurations of ONE model are timed in alternation,
`rounds` times each, and the median of the rounds is reported with the rounds themselves:

    p=0        set_dropout(0.0): the launches of a model without the feature
    p=0 again  the same configuration a second time: the difference between the two is the spread of equal rounds, the
               yardstick for the third
    p=0.1      set_dropout(0.1): per block one elementwise launch forward (h read, the dropped activation written, conv2
               reading it without a GroupNorm prologue) and one in-place mask pass backward

A figure is ms per fused training step (train_step_fused: add_noise, forward, MSE, backward, Adam, repack), wall clock over
`steps` steps synchronised at both ends.  The tape's extra bytes are reported twice: computed from the architecture (the dropped
activation of each of the 22 blocks, 4*B*C*H*W bytes, and as much again of gradient arena) and measured as the growth of the
activation pool (sisic_unet_workspace_bytes) from the first p=0 step to the first p=0.1 step.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from synt_isic_amd import _lib  # noqa: E402
from synt_isic_amd.scheduler import HipDDPMScheduler  # noqa: E402
from synt_isic_amd.train import HipAdam, HipGradScaler, train_step_fused  # noqa: E402
from synt_isic_amd.unet import HipUNet2DModel  # noqa: E402
from synt_isic_amd.weights import synthetic_unet_state_dict  # noqa: E402

CONFIGS = [("p=0", 0.0), ("p=0 again", 0.0), ("p=0.1", 0.1)]


def dropped_activation_bytes(cfg, B, H, W):
    """4 * B * C * h * w summed over the ResNet blocks, in execution order: down (layers_per_block per level), mid (2), up
    (layers_per_block + 1 per level)"""
    boc, n, total = cfg.block_out_channels, len(cfg.block_out_channels), 0
    for i, c in enumerate(boc):
        total += cfg.layers_per_block * c * (H >> i) * (W >> i)
    total += 2 * boc[-1] * (H >> (n - 1)) * (W >> (n - 1))
    for i, c in enumerate(reversed(boc)):
        total += (cfg.layers_per_block + 1) * c * (H >> (n - 1 - i)) * (W >> (n - 1 - i))
    return 4 * B * total


def run(B, size, steps, rounds, emit):
    dev = torch.device("cuda")
    m = HipUNet2DModel()
    m.load_state_dict(synthetic_unet_state_dict())
    m = m.to(dev)
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    opt, scaler = HipAdam(m, lr=1e-4), HipGradScaler()
    m.train()
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.rand(B, 3, size, size, generator=g, device=dev) * 2 - 1
    noise = torch.randn(B, 3, size, size, generator=g, device=dev)
    ts = torch.randint(0, 1000, (B,), generator=g, device=dev)
    lib = _lib.load()

    def pool_bytes():
        torch.cuda.synchronize()
        return int(lib.sisic_unet_workspace_bytes(m.handle))

    def timed(p):
        m.set_dropout(p, seed=1, first_call=m.dropout_next_call)
        for _ in range(2):
            train_step_fused(m, sched, images, noise, ts, opt, scaler)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            train_step_fused(m, sched, images, noise, ts, opt, scaler)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    m.set_dropout(0.0)
    train_step_fused(m, sched, images, noise, ts, opt, scaler)
    pool_off = pool_bytes()
    m.set_dropout(0.1, seed=1)
    train_step_fused(m, sched, images, noise, ts, opt, scaler)
    pool_on = pool_bytes()

    ms = {name: [] for name, _ in CONFIGS}
    for _ in range(rounds):
        for name, p in CONFIGS:
            ms[name].append(timed(p))
    base = statistics.median(ms["p=0"])
    for name, p in CONFIGS:
        med = statistics.median(ms[name])
        emit(json.dumps({"batch": B, "size": size, "config": name, "p": p, "steps": steps, "rounds": rounds,
                         "train_step_ms": round(med, 4), "vs_p0_ms": round(med - base, 4),
                         "vs_p0_percent": round(100.0 * (med - base) / base, 2),
                         "train_step_ms_rounds": [round(v, 4) for v in ms[name]]}))
    computed = dropped_activation_bytes(m.config, B, size, size)
    emit(json.dumps({"batch": B, "size": size, "tape_extra_bytes_computed": computed,
                     "gradient_arena_extra_bytes_computed": computed, "pool_bytes_p0": pool_off, "pool_bytes_p0.1": pool_on,
                     "pool_growth_bytes_measured": pool_on - pool_off}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the result lines to this file (profiles/r21/dropout.txt)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/dropout_bench.py measures on an MI355X: no GPU here, nothing measured")

    def emit(line):
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    emit(f"# tools/dropout_bench.py --steps {a.steps} --rounds {a.rounds}: ms per fused training step, medians of {a.rounds} "
         f"alternated rounds; 'p=0 again' against 'p=0' is the spread of equal rounds; {torch.cuda.get_device_name(0)}")
    run(32, 64, a.steps, a.rounds, emit)
    run(2, 128, a.steps, a.rounds, emit)
