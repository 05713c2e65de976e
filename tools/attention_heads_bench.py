#!/usr/bin/env python3
"""Per-launch time of ops.attention and ops.attention_bwd at 8, 32 and 64 channels per head, at the same (B, C, N) across the
three widths, through the C ABI.  Five alternated rounds (every case once per round, the widths next to each other), the median
and the spread (min .. max) of the five equal runs of each case.  Not a test.

    python tools/attention_heads_bench.py --emit-resources > resources.txt      # no GPU: registers, LDS, scratch from the compile
    python tools/attention_heads_bench.py [--resources resources.txt] [--out profiles/r27/attention_heads.txt]

FLOP counts are the algorithm's (4 B C N^2 forward; the backward pass is given as time only: the d = 8 kernel and the tiled
kernels recompute different things).
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = (8, 32, 64)
# (what, B, C, N)
SHAPES = [("sampling, 8x8 tokens", 64, 256, 64), ("sampling, 16x16 tokens", 64, 256, 256), ("sampling, 32x32 tokens", 32, 256, 1024),
          ("training, 8x8 tokens", 32, 256, 64), ("training, 32x32 tokens", 2, 256, 1024)]
ROUNDS = 5
WINDOW_MS = 60.0


def emit_resources():
    """hipcc -Rpass-analysis=kernel-resource-usage on attention_wide.hip with the flags of the Makefile"""
    csrc = os.path.join(ROOT, "synt_isic_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "attention_wide.hip"), "-o", os.path.join(tmp, "a.o")]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = {"name": re.sub(r"^void sisic::|\(.*$", "", name)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    print("kernels of attention_wide.hip (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, the Makefile's flags)")
    print(f"{'kernel':42s} {'VGPRs':>6s} {'AGPRs':>6s} {'scratch B/lane':>15s} {'LDS B/block':>12s} {'waves/SIMD':>11s}")
    for r in rows:
        print(f"{r['name']:42s} {r['VGPRs']:>6s} {r['AGPRs']:>6s} {r['ScratchSize']:>15s} {r['LDS']:>12s} {r['Occupancy']:>11s}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emit-resources", action="store_true")
    ap.add_argument("--resources", default=None, help="text of an --emit-resources run, copied to the head of the output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "attention_heads.txt"))
    a = ap.parse_args()
    if a.emit_resources:
        return emit_resources()

    import torch
    from synt_isic_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("attention_heads_bench: needs a GPU")

    cases = []          # (op, what, B, C, N, d, call, iters)
    for what, B, C, N in SHAPES:
        g = torch.Generator().manual_seed(B + C + N)
        qkv = (torch.randn(B, 3 * C, N, generator=g) * 1.5).cuda()
        dO = torch.randn(B, C, N, generator=g).cuda()
        for d in WIDTHS:
            out = ops.attention(qkv, d)
            cases.append(("attention", what, B, C, N, d, (lambda q=qkv, d=d: ops.attention(q, d))))
            cases.append(("attention_bwd", what, B, C, N, d, (lambda q=qkv, o=out, g_=dO, d=d: ops.attention_bwd(q, o, g_, d))))

    def timed(call, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters       # us per launch

    iters = []
    for c in cases:                                      # warm every case, then size its window
        c[6]()
        torch.cuda.synchronize()
        once = timed(c[6], 3)
        iters.append(max(5, min(2000, int(WINDOW_MS * 1e3 / max(once, 1.0)))))
    rounds = [[timed(c[6], n) for c, n in zip(cases, iters)] for _ in range(ROUNDS)]

    lines = []
    if a.resources:
        lines += open(a.resources).read().rstrip("\n").split("\n") + [""]
    lines += [f"per-launch time on {torch.cuda.get_device_name(0)}: device events around back-to-back launches (a window of ~{WINDOW_MS:.0f} ms",
              f"per case and round), {ROUNDS} alternated rounds; median, and min .. max of the {ROUNDS} equal runs of the case",
              "qkv = 1.5 x a normal draw (softmax rows neither uniform nor saturated)", "",
              f"{'op':14s} {'shape (B, C, N)':18s} {'d':>3s} {'heads':>5s} {'median us':>10s} {'min':>9s} {'max':>9s} {'spread':>7s} {'vs d=8':>7s}  {'TFLOP/s (4BCN^2)':>16s}  what"]
    base = {}
    for i, c in enumerate(cases):
        op, what, B, C, N, d, _ = c
        ts = [r[i] for r in rounds]
        med = statistics.median(ts)
        if d == 8:
            base[(op, B, C, N)] = med
        tf = f"{4.0 * B * C * N * N / med / 1e6:16.2f}" if op == "attention" else f"{'-':>16s}"
        lines.append(f"{op:14s} {str((B, C, N)):18s} {d:3d} {C // d:5d} {med:10.1f} {min(ts):9.1f} {max(ts):9.1f} {(max(ts) - min(ts)) / med:7.1%} "
                     f"{med / base[(op, B, C, N)]:7.2f}  {tf}  {what}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
