#!/usr/bin/env python3
"""What training the ResNet18 classifier with batch-statistics BatchNorm costs on one MI355X, and against what.

    python tools/classifier_bn_bench.py [--steps 10] [--rounds 5] [--out FILE]

Step time, per shape (batch 32 at 64x64 and batch 2 at 128x128, both resized to 224x224 by the pre-processing), timed in
alternation, `rounds` times each; the median of the rounds is reported with the rounds themselves:

    batch       clf.loss_backward + HipClassifierAdam(batchnorm="batch").step     62 trainable tensors, batch statistics
    frozen      the same with batchnorm="frozen" (a second model in the same process)   22 trainable tensors, folded BatchNorm
    torch       torch.autograd over the same network with F.batch_norm(training=True) + torch.optim.Adam over the 62 tensors, on
                the same GPU (MIOpen), the same pre-processing written with device tensors

ms per call: wall clock over `steps` calls, synchronised at both ends.

The BatchNorm launches at the stem's shape (B = 32, C = 64, 112 x 112): kernel time between the events the library's launch
profile records around each launch, per call, median of the rounds.  The forward entry runs (moments, apply) and the backward
entry (reduce, apply); each entry is also run with its first launch alone, and the apply launch is the difference of the two
medians.  GB/s from the bytes the launch must move (every input tensor read once, the output written once; fp32).  Beside them:
launch_add_relu (ops.add_relu: two tensors read, one written) on tensors of the same size in the same run, timed the same way
-- the project's yardstick for an elementwise pass.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import resnet18 as ores  # noqa: E402
from synt_isic_amd import ops  # noqa: E402
from synt_isic_amd.classifier import HipMelanomaClassifier  # noqa: E402
from synt_isic_amd.train import HipClassifierAdam  # noqa: E402
from synt_isic_amd.weights import synthetic_resnet18_state_dict  # noqa: E402

SHAPES = [(32, 64), (2, 128)]
STEM = (32, 64, 112 * 112)
CONFIGS = ["batch", "frozen", "torch"]


def _preprocess(x):
    x = torch.clamp((x + 1.0) / 2.0, 0, 1)
    x = F.interpolate(x, size=(224, 224), mode="bilinear", align_corners=False, antialias=True)
    mean = torch.tensor(ores.IMAGENET_MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(ores.IMAGENET_STD, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def _torch_features(p, stats, x):
    """resnet18 with training-mode BatchNorm (tests/clf_bn_ref.py's structure, device tensors)"""
    bn = lambda n, t: F.batch_norm(t, stats[n + ".running_mean"], stats[n + ".running_var"], p[n + ".weight"], p[n + ".bias"],  # noqa: E731
                                   training=True, momentum=0.1, eps=ores.BN_EPS)
    m = "model."
    x = F.relu(bn(m + "bn1", F.conv2d(x, p[m + "conv1.weight"], None, stride=2, padding=3)))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for l in range(4):
        for j in range(2):
            stride = 2 if (l > 0 and j == 0) else 1
            base = f"{m}layer{l + 1}.{j}"
            identity = x
            out = F.relu(bn(base + ".bn1", F.conv2d(x, p[base + ".conv1.weight"], None, stride=stride, padding=1)))
            out = bn(base + ".bn2", F.conv2d(out, p[base + ".conv2.weight"], None, stride=1, padding=1))
            if base + ".downsample.0.weight" in p:
                identity = bn(base + ".downsample.1", F.conv2d(x, p[base + ".downsample.0.weight"], None, stride=stride))
            x = F.relu(out + identity)
    return F.linear(F.adaptive_avg_pool2d(x, 1).flatten(1), p[m + "fc.weight"], p[m + "fc.bias"])


def _clf(sd, dev, mode):
    clf = HipMelanomaClassifier(num_classes=7)
    clf.load_state_dict(sd)
    clf = clf.to(dev).eval()
    return clf, HipClassifierAdam(clf, lr=1e-4, batchnorm=mode)


def steps_bench(B, size, steps, rounds, emit):
    dev = torch.device("cuda")
    sd = synthetic_resnet18_state_dict()
    pairs = {mode: _clf(sd, dev, mode) for mode in ("batch", "frozen")}
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.rand(B, 3, size, size, generator=g, device=dev) * 1.6 - 0.8
    labels = torch.randint(0, 7, (B,), generator=g, device=dev)
    labels_host = labels.cpu()
    params = {k: v.to(dev).clone().requires_grad_(True) for k, v in sd.items() if "running_" not in k}
    stats = {k: v.to(dev).clone() for k, v in sd.items() if "running_" in k}
    topt = torch.optim.Adam(list(params.values()), lr=1e-4)

    def torch_step():
        topt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(_torch_features(params, stats, _preprocess(images)), labels)
        loss.backward()
        topt.step()
        return loss.item()                      # the library's step returns the loss to the host as well

    def lib_step(mode):
        clf, opt = pairs[mode]
        return lambda: (clf.loss_backward(images, labels_host), opt.step())

    fns = {"batch": lib_step("batch"), "frozen": lib_step("frozen"), "torch": torch_step}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    ms = {c: [] for c in CONFIGS}
    for _ in range(rounds):
        for c in CONFIGS:
            ms[c].append(timed(fns[c]))
    med = {c: statistics.median(ms[c]) for c in CONFIGS}
    for c in CONFIGS:
        emit(json.dumps({"batch": B, "size": size, "config": c, "steps": steps, "rounds": rounds, "ms": round(med[c], 4),
                         "ms_rounds": [round(v, 4) for v in ms[c]]}))
    emit(json.dumps({"batch": B, "size": size, "batch_over_frozen": round(med["batch"] / med["frozen"], 4),
                     "batch_over_torch": round(med["batch"] / med["torch"], 4)}))
    for _, opt in pairs.values():
        opt.close()


def launches_bench(calls, rounds, emit):
    dev = torch.device("cuda")
    B, Cc, HW = STEM
    g = torch.Generator(device=dev).manual_seed(1)
    y, res, grad = (torch.randn(B, Cc, HW, generator=g, device=dev) for _ in range(3))
    gamma, beta = torch.rand(Cc, generator=g, device=dev) + 0.5, torch.randn(Cc, generator=g, device=dev)
    out, mean, invstd = ops.batchnorm_train(y, gamma, beta, residual=res, relu=True)
    numel_bytes = 4.0 * B * Cc * HW
    fns = {
        "moments": lambda: ops.batchnorm_train(y, gamma, beta, apply=False),
        "moments+apply": lambda: ops.batchnorm_train(y, gamma, beta, residual=res, relu=True),
        "bwd_reduce": lambda: ops.batchnorm_train_bwd(grad, y, mean, invstd, gamma, act=out, apply=False),
        "bwd_reduce+apply": lambda: ops.batchnorm_train_bwd(grad, y, mean, invstd, gamma, act=out),
        "add_relu": lambda: ops.add_relu(y, res),
    }

    def kernel_ms(fn):
        fn()
        torch.cuda.synchronize()
        ops.profile_reset(dev)
        ops.profile_enable(dev, True)
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        rec = ops.profile_read(dev)["other"]
        ops.profile_enable(dev, False)
        return rec["ms"] / calls

    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k in fns:
            ms[k].append(kernel_ms(fns[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    # bytes each launch must move: inputs read once, output written once
    rows = [("bn_moments (y)", med["moments"], 1 * numel_bytes, ms["moments"]),
            ("bn_apply (y, residual -> out), by difference", med["moments+apply"] - med["moments"], 3 * numel_bytes, None),
            ("bn_bwd_reduce (g, y, act)", med["bwd_reduce"], 3 * numel_bytes, ms["bwd_reduce"]),
            ("bn_bwd_apply (g, y, act -> dy), by difference", med["bwd_reduce+apply"] - med["bwd_reduce"], 4 * numel_bytes, None),
            ("launch_add_relu (y, identity -> out)", med["add_relu"], 3 * numel_bytes, ms["add_relu"])]
    for name, t, nbytes, rounds_ms in rows:
        rec = {"shape": list(STEM), "launch": name, "calls": calls, "rounds": rounds, "us": round(t * 1e3, 2),
               "GB_per_s": round(nbytes / (t * 1e-3) / 1e9, 1), "bytes": int(nbytes)}
        if rounds_ms is not None:
            rec["us_rounds"] = [round(v * 1e3, 2) for v in rounds_ms]
        emit(json.dumps(rec))
    for k in ("moments+apply", "bwd_reduce+apply"):
        emit(json.dumps({"shape": list(STEM), "entry": k, "us": round(med[k] * 1e3, 2), "us_rounds": [round(v * 1e3, 2) for v in ms[k]]}))


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

    emit(f"# tools/classifier_bn_bench.py --steps {a.steps} --rounds {a.rounds}: medians of {a.rounds} alternated rounds, "
         f"{torch.cuda.get_device_name(0)}")
    for B, size in SHAPES:
        steps_bench(B, size, a.steps, a.rounds, emit)
    emit("# the BatchNorm launches at the stem's shape: kernel time per call between the launch profile's events, GB/s from the bytes "
         "each must move")
    launches_bench(a.steps, a.rounds, emit)
