#!/usr/bin/env python3
"""What the GPU-resident loader (synt_isic_amd.data.DeviceLoader) costs a training epoch, and what the reference's host chain gives.

    python tools/augment_bench.py train --batch 32 --size 64  [--images 512 --runs 3]
    python tools/augment_bench.py train --batch 2  --size 128
    python tools/augment_bench.py pil   --size 64 [--images 512]        (host only: never opens the GPU)

train: wall time of ``train_class(model, feed, epochs=1)`` over ``--images`` random images, fed by a DeviceLoader and by a
       pre-made list of fixed device batches (what training could be fed before the loader existed), ``--runs`` alternated
       runs each after one warm-up epoch of each; then the loader alone: HIP events around its two launches per batch, the
       host time of drawing an epoch's parameters and the host time of an epoch of batches without training.
pil:   the same chain (train_diffusion.py:72-81) through PIL in this one process on one thread -- what ``num_workers=1`` gives
       the reference -- in images/s, parameters drawn per sample, ToTensor + Normalize included; states the host's CPU model.
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def images(n, size):
    return np.random.default_rng(0).integers(0, 256, size=(n, size, size, 3), dtype=np.uint8)


def run_train(a):
    import torch
    from synt_isic_amd import data
    from synt_isic_amd.train import train_class
    from synt_isic_amd.unet import HipUNet2DModel
    from synt_isic_amd.weights import synthetic_unet_state_dict
    dev = torch.device("cuda")
    ds = data.DeviceDataset(images(a.images, a.size), dev)
    loader = data.DeviceLoader(ds, a.batch, seed=0)
    fixed = [b.clone() for b in data.DeviceLoader(ds, a.batch, seed=1)]
    model = HipUNet2DModel()
    model.load_state_dict(synthetic_unet_state_dict())
    model = model.to(dev)

    def epoch(feed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train_class(model, feed, "NV", epochs=1, log=None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    epoch(fixed)
    epoch(loader)
    t_fixed, t_loader = [], []
    for _ in range(a.runs):
        t_fixed.append(epoch(fixed))
        t_loader.append(epoch(loader))
    spread = max(t_fixed) - min(t_fixed)
    diff = statistics.median(t_loader) - statistics.median(t_fixed)
    print(json.dumps({"what": "train_class epoch", "batch": a.batch, "size": a.size, "images": a.images, "steps": len(fixed),
                      "fixed_list_ms": t_fixed, "device_loader_ms": t_loader, "fixed_spread_ms": spread,
                      "median_difference_ms": diff, "within_fixed_spread": bool(abs(diff) <= spread),
                      "ms_per_step_fixed": statistics.median(t_fixed) / len(fixed),
                      "ms_per_step_loader": statistics.median(t_loader) / len(fixed)}), flush=True)

    # the loader alone
    t0 = time.perf_counter()
    for _ in range(5):
        loader.epoch_params(7)
    draw_ms = (time.perf_counter() - t0) * 1e3 / 5
    list(loader)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(len(loader))]
    t0 = time.perf_counter()
    it = iter(loader)
    for e0, e1 in ev:
        e0.record()
        next(it)
        e1.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    gpu = [e0.elapsed_time(e1) for e0, e1 in ev]
    print(json.dumps({"what": "loader alone", "batch": a.batch, "size": a.size, "batches": len(ev),
                      "draw_epoch_params_host_ms": draw_ms, "draw_host_us_per_image": draw_ms * 1e3 / a.images,
                      "epoch_of_batches_host_ms": host_ms, "host_ms_per_batch": host_ms / len(ev),
                      "gpu_ms_per_batch_median": statistics.median(gpu), "gpu_ms_per_batch_max": max(gpu),
                      "images_per_sec_host_bound": a.images / (host_ms * 1e-3)}), flush=True)


def run_pil(a):
    import torch
    from PIL import Image, ImageEnhance
    from synt_isic_amd import data
    torch.set_num_threads(1)
    imgs = [Image.fromarray(im) for im in images(a.images, a.size)]
    enhancers = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    S = a.size
    rng = np.random.default_rng(1)

    def sample(k, epoch):
        r = data.draw_augment_params([k], epoch, 0, S, S)[0]
        im = imgs[k].crop((r["crop_x"], r["crop_y"], r["crop_x"] + r["crop_w"], r["crop_y"] + r["crop_h"])).resize((S, S), Image.BILINEAR)
        if r["hflip"]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        if r["vflip"]:
            im = im.transpose(Image.FLIP_TOP_BOTTOM)
        for op in r["order"]:
            im = enhancers[op](im).enhance(float(r["factor"][op]))
        if r["rotate"]:
            im = im.rotate(float(rng.uniform(-15.0, 15.0)), Image.NEAREST)
        t = torch.from_numpy(np.array(im)).permute(2, 0, 1).contiguous().float().div(255)
        return (t - 0.5) / 0.5

    for k in range(min(32, a.images)):
        sample(k, 0)
    t0 = time.perf_counter()
    for k in range(a.images):
        sample(k, 1)
    dt = time.perf_counter() - t0
    print(json.dumps({"what": "PIL chain, one host process, one thread", "size": a.size, "images": a.images,
                      "images_per_sec": a.images / dt, "us_per_image": dt * 1e6 / a.images, "cpu": cpu_model()}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("train", "pil"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    run_train(a) if a.mode == "train" else run_pil(a)
