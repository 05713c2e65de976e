#!/usr/bin/env python3
"""BASELINE config 3 as a program: N seeds, contiguous blocks per GPU, weights replicated, one gather of the uint8
images to rank 0 (the reference loops over images one at a time, image_generator.py:612-648).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29511 \\
        examples/generate_sharded.py --count 512 --T 1000 --size 64 --class-name NV [--weights unet_NV_best.pth] \\
        [--out images.npy] [--noise host|device] [--scheduler ddpm|ddim|dpmsolver++] [--eta 0.0] \\
        [--solver-order 2] [--algorithm-type dpmsolver++|sde-dpmsolver++]

Every image's chain depends only on its own seed, so the gathered result is bit-identical to sampling the same
seeds on one GPU (tests/test_gpu_sampler.py::test_batch_and_shard_independence_small).
"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from synt_isic_amd import dist as sdist  # noqa: E402
from synt_isic_amd.sampler import Sampler, image_seed  # noqa: E402
from synt_isic_amd.weights import synthetic_unet_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=512)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--class-name", default="NV")
    ap.add_argument("--base-seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=64, help="images sampled together on one GPU")
    ap.add_argument("--weights", default=None, help="diffusers-format state dict (.pth); default: seeded synthetic weights")
    ap.add_argument("--out", default=None)
    ap.add_argument("--noise", choices=("host", "device"), default="host",
                    help="host: one CPU torch.Generator per image (the default); device: x_T from torch's device generator "
                         "and z_t generated in the step kernel -- no host RNG, so the ranks do not compete for CPUs")
    ap.add_argument("--scheduler", choices=("ddpm", "ddim", "dpmsolver++"), default="ddpm",
                    help="the step rule: DDPM ancestral sampling (the default), DDIM -- the rule made for --T of 20 to 100 -- or "
                         "DPM-Solver++(2M), the second-order rule for --T of 10 to 25")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM only: 0 is deterministic, 1 has the DDPM rule's sigma")
    ap.add_argument("--solver-order", type=int, choices=(1, 2), default=2, help="dpmsolver++ only: 1 is the DDIM rule")
    ap.add_argument("--algorithm-type", choices=("dpmsolver++", "sde-dpmsolver++"), default="dpmsolver++",
                    help="dpmsolver++ only: the ODE solver (draws nothing beyond x_T) or its stochastic variant")
    ap.add_argument("--thresholding", action="store_true",
                    help="dynamic thresholding of x0 (Imagen): per image, clamp to the --dynamic-thresholding-ratio quantile of "
                         "|x0| (at least 1, at most --sample-max-value) and divide by it, in place of the static clamp")
    ap.add_argument("--dynamic-thresholding-ratio", type=float, default=0.995)
    ap.add_argument("--sample-max-value", type=float, default=1.0)
    a = ap.parse_args()

    rank, world, local = sdist.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    sd = torch.load(a.weights, map_location="cpu") if a.weights else synthetic_unet_state_dict()
    s = Sampler(dev)
    s.add_model(a.class_name, sd)

    seeds = [image_seed(a.base_seed, a.class_name, i) for i in range(a.count)]      # image_generator.py:626-631
    mine = sdist.shard_seeds(seeds, world, rank)
    t0 = time.perf_counter()
    blocks = []
    for i in range(0, len(mine), a.batch):
        blocks.append(s.generate_seeds(a.class_name, mine[i:i + a.batch], a.T, (a.size, a.size), noise=a.noise,
                                       scheduler=a.scheduler, eta=a.eta, solver_order=a.solver_order,
                                       algorithm_type=a.algorithm_type, thresholding=a.thresholding,
                                       dynamic_thresholding_ratio=a.dynamic_thresholding_ratio,
                                       sample_max_value=a.sample_max_value).images)
    local_images = torch.cat(blocks) if blocks else torch.empty((0, a.size, a.size, 3), dtype=torch.uint8, device=dev)
    images = sdist.gather_images(local_images, a.count, dst=0)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    if rank == 0:
        arr = images.cpu().numpy()
        rule = f", ddim eta={a.eta:g}" if a.scheduler == "ddim" else ""
        if a.scheduler == "dpmsolver++":
            rule = f", {a.algorithm_type} order {a.solver_order}"
        if a.thresholding:
            rule += f", thresholding {a.dynamic_thresholding_ratio:g} max {a.sample_max_value:g}"
        print(f"{a.count} images {a.size}x{a.size}, T={a.T}, {world} GPU(s), {a.noise} noise{rule}: {dt:.2f} s -> {a.count / dt:.3f} images/sec; "
              f"sha256 {hashlib.sha256(arr.tobytes()).hexdigest()[:16]}", flush=True)
        if a.out:
            np.save(a.out, arr)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
