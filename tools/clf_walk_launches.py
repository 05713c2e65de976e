#!/usr/bin/env python3
"""The ordered list of kernels the classifier executor launches for one frozen loss_backward, one batch-statistics loss_backward
and one input_gradient, at (2, 3, 32, 32) pre-processed: the classifier's kernels outside launch_conv2d do not feed the library's
profile counters, so two builds of csrc/resnet.cpp are compared on what `rocprofv3 --kernel-trace` sees.

    SISIC_LIB_PATH=<library> python tools/clf_walk_launches.py --out FILE

One traced process under `timeout -k 10 200`; kernel tracing only, no counters.  One line per launch in start order, the weight
packing of the load and of train_begin included.  Synthetic weights.  Needs the GPU and rocprofv3.
"""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import torch
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.train import HipClassifierAdam
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    sd = synthetic_resnet18_state_dict()
    clf = HipMelanomaClassifier(num_classes=7).load_state_dict(sd).to("cuda:0").eval()
    x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(33)).to("cuda:0")
    for mode in ("frozen", "batch"):
        opt = HipClassifierAdam(clf, batchnorm=mode)
        clf.loss_backward(x, [0, 6], preprocessed=True)
        opt.close()
    clf.load_state_dict(sd)
    # input_gradient always pre-processes: the walk's tail (stem and pre-processing backward) is in the list
    clf.input_gradient(x, 1)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", action="store_true", help="run the three calls in this process (what the driver traces)")
    a = ap.parse_args()
    if a.child:
        child()
        return
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "200", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "walk", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--out", a.out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not found:
            print(r.stdout[-2000:])
            raise SystemExit(f"the traced program ended with status {r.returncode}")
        with open(found[0]) as f:
            rows = sorted(csv.DictReader(f), key=lambda row: int(row["Start_Timestamp"]))
    names = [re.sub(r"\(.*", "", row["Kernel_Name"]).replace("void ", "") for row in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(names) + "\n")
    print(f"{len(names)} launches -> {a.out}")


if __name__ == "__main__":
    main()
