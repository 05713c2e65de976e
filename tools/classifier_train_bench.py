#!/usr/bin/env python3
"""What a training step of the ResNet18 classifier (BatchNorm frozen) costs on one MI355X, and against what.

    python tools/classifier_train_bench.py [--steps 10] [--rounds 5] [--out FILE]
    python tools/classifier_train_bench.py --profile-run 32x64 [--steps 8]      (the program of a rocprofv3 --kernel-trace run)
    python tools/classifier_train_bench.py --kernel-trace CSV [--out FILE]      (reads that run's kernel_trace.csv, no GPU)

Per shape (batch 32 at 64x64 and batch 2 at 128x128, both resized to 224x224 by the pre-processing) these are timed in
alternation, `rounds` times each, and the median of the rounds is reported with the rounds themselves:

    step            clf.loss_backward + HipClassifierAdam.step        the library's training step
    backward        clf.loss_backward alone                            forward, loss head, data and weight gradients, unfold
    optimizer       HipClassifierAdam.step alone                       statistics, Adam, refold and repack of all 20 filters
    input_gradient  clf.input_gradient at the same shape               yardstick: a step should cost about a forward plus two backwards
    forward         clf.forward
    torch           torch.autograd over oracle/resnet18.py + torch.optim.Adam on the same GPU (MIOpen), eval-mode batch_norm,
                    the same pre-processing written with device tensors -- the other yardstick

ms per call: wall clock over `steps` calls, synchronised at both ends.  --kernel-trace: the per-dispatch trace of a rocprofv3
--kernel-trace run of --profile-run; the tool then reports, per step and as a share of the kernel time of the steps after the
second, what the stem's weight gradient (stem_wgrad_kernel) and the refold (refold_kernel and the pack kernels behind it)
take, beside the other groups of the step.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import resnet18 as ores  # noqa: E402
from synt_isic_amd.classifier import HipMelanomaClassifier  # noqa: E402
from synt_isic_amd.train import HipClassifierAdam  # noqa: E402
from synt_isic_amd.weights import synthetic_resnet18_state_dict  # noqa: E402

CONFIGS = ["step", "backward", "optimizer", "input_gradient", "forward", "torch"]
SHAPES = [(32, 64), (2, 128)]


def _preprocess(x):
    x = torch.clamp((x + 1.0) / 2.0, 0, 1)
    x = F.interpolate(x, size=(224, 224), mode="bilinear", align_corners=False, antialias=True)
    mean = torch.tensor(ores.IMAGENET_MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(ores.IMAGENET_STD, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def _setup(B, size):
    dev = torch.device("cuda")
    sd = synthetic_resnet18_state_dict()
    clf = HipMelanomaClassifier(num_classes=7)
    clf.load_state_dict(sd)
    clf = clf.to(dev).eval()
    opt = HipClassifierAdam(clf, lr=1e-4)
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.rand(B, 3, size, size, generator=g, device=dev) * 1.6 - 0.8
    labels = torch.randint(0, 7, (B,), generator=g, device=dev)
    return dev, sd, clf, opt, images, labels


def run(B, size, steps, rounds, emit):
    dev, sd, clf, opt, images, labels = _setup(B, size)
    labels_host = labels.cpu()
    params = {k: v.to(dev).clone() for k, v in sd.items()}
    leaves = [v.requires_grad_(True) for k, v in params.items() if v.dim() == 4 or k.startswith("model.fc.")]
    topt = torch.optim.Adam(leaves, lr=1e-4)

    def torch_step():
        topt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(ores.resnet18_features(params, _preprocess(images)), labels)
        loss.backward()
        topt.step()
        return loss.item()                      # the library's step returns the loss to the host as well

    fns = {"step": lambda: (clf.loss_backward(images, labels_host), opt.step()),
           "backward": lambda: clf.loss_backward(images, labels_host),
           "optimizer": lambda: opt.step(),
           "input_gradient": lambda: clf.input_gradient(images, 1),
           "forward": lambda: clf(images),
           "torch": torch_step}

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
                         "vs_step": round(med[c] / med["step"], 4), "ms_rounds": [round(v, 4) for v in ms[c]]}))
    emit(json.dumps({"batch": B, "size": size, "step_over_torch": round(med["step"] / med["torch"], 4),
                     "step_over_input_gradient": round(med["step"] / med["input_gradient"], 4),
                     "step_over_forward_plus_two_backwards": round(med["step"] / (med["forward"] + 2 * (med["input_gradient"] - med["forward"])), 4)}))
    opt.close()


def profile_run(B, size, steps):
    _, _, clf, opt, images, labels = _setup(B, size)
    labels_host = labels.cpu()
    for _ in range(steps):
        clf.loss_backward(images, labels_host)
        opt.step()
    torch.cuda.synchronize()
    opt.close()


def kernel_shares(path, emit, warm_steps=2):
    """steady-state shares from the per-dispatch trace: a step begins at its first dispatch after the previous step's last
    repack, i.e. the dispatches between two ce_head_kernel launches minus the forward in front of the second are told apart
    by the stem convolution that opens every step's forward; the first `warm_steps` steps (and the load) are left out"""
    rows = list(csv.DictReader(open(path)))
    key = {k.lower(): k for k in rows[0]}
    name_key, start_key, end_key = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    rows.sort(key=lambda r: int(r[start_key]))
    opens = [i for i, r in enumerate(rows) if "preprocess_kernel" in r[name_key]]        # one per forward, the first launch of a step
    assert len(opens) > warm_steps, f"{len(opens)} steps in the trace, {warm_steps} of them warm-up"
    rows = rows[opens[warm_steps]:]
    steps = len(opens) - warm_steps
    dur = lambda r: int(r[end_key]) - int(r[start_key])
    total = sum(dur(r) for r in rows)
    groups = {"stem_wgrad": ("stem_wgrad_kernel",), "refold": ("refold_kernel",),
              "repack": ("conv_pack_kernel", "winograd_pack_kernel", "winograd_pack_wide_kernel", "winograd_pack_bf3_kernel", "pack_batch_kernel"),
              "unfold": ("unfold_grad_kernel",), "weight_gradients": ("conv_wgrad", "wgrad_reduce", "wgrad_wino"),
              "head": ("ce_head_kernel", "fc_head_bwd_kernel"), "gather_even": ("gather_even_kernel",),
              "maxpool_bwd": ("maxpool_bwd_kernel",), "adam_and_statistics": ("adam", "grad_stats")}
    for label, keys in groups.items():
        sel = [r for r in rows if any(k in r[name_key] for k in keys)]
        ns = sum(dur(r) for r in sel)
        emit(json.dumps({"kernel_group": label, "launches_per_step": round(len(sel) / steps, 1), "us_per_step": round(ns / 1e3 / steps, 1),
                         "share_of_kernel_time": round(ns / total, 4)}))
    emit(json.dumps({"steps": steps, "kernel_us_per_step": round(total / 1e3 / steps, 1), "launches_per_step": round(len(rows) / steps, 1)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    ap.add_argument("--kernel-trace", default=None, help="kernel_trace.csv of a rocprofv3 run of --profile-run: add the kernel shares")
    ap.add_argument("--profile-run", default=None, metavar="BxSIZE", help="only run `steps` training steps at this shape (for rocprofv3)")
    a = ap.parse_args()

    def emit(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.profile_run:
        b, s = a.profile_run.split("x")
        profile_run(int(b), int(s), a.steps)
    elif a.kernel_trace:
        emit("# tools/classifier_train_bench.py --kernel-trace: per step and as shares of the kernel time, the first two steps left out")
        kernel_shares(a.kernel_trace, emit)
    else:
        emit(f"# tools/classifier_train_bench.py --steps {a.steps} --rounds {a.rounds}: medians of {a.rounds} alternated rounds, "
             f"{torch.cuda.get_device_name(0)}")
        for B, size in SHAPES:
            run(B, size, a.steps, a.rounds, emit)
