#!/usr/bin/env python3
"""What dynamic thresholding of x0 costs on one MI355X: the sampling loop with and without it, the unthresholded loop against
another build of the library, and the quantile launch alone.

    python tools/threshold_bench.py [--reps 5] [--limit 400] [--other-lib PATH] [--out profiles/r34/threshold.txt]

Part A, ms per step of the loop alone (run_sampling_loop, x_T resident, DeviceNoise, ends in a synchronise), thresholding off
against thresholding on (ratio 0.995, sample_max_value 2): DPM-Solver++ (order 2) at T = 20 and DDPM at T = 250, for batch 64 at
64x64 (eager launches) and for batch 1 at 128x128 in latency mode (graph-replayed).  On adds one launch per step -- the
selection kernel, one workgroup per image -- and s [B] between it and the step kernel.
Part B (with --other-lib, the library of another commit built beside this one): the UNTHRESHOLDED loops of part A under this
library and under the other, one process per library and alternation (a process loads one library), the order of the two
turned round from one alternation to the next.  The other library may
lack the thresholding entry points: their bindings and the call that switches the handle's setting off are then left out.
Part C, the quantile launch alone (ops.x0_threshold, epsilon prediction) at (B, n) = (64, 12288), (1, 49152), (32, 49152): us per
launch between two events around a window of back-to-back launches.

The protocol is tools/dpmpp_bench.py's: every configuration is warmed up once; then `reps` rounds run the configurations one
after the other (alternated, not in blocks), and the table gives the median and the min .. max of the equal runs beside it.
Every part is a process of its own under `timeout -k 10 LIMIT`; the first that fails or runs out of time ends the run, and
nothing more is started on the GPU.  Synthetic weights: the numbers are times, nothing here says anything about image quality.
Needs the GPU; there is no CPU path.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THR = (0.995, 2.0)
# (label, scheduler, T)
RULES = [("dpmsolver++ order 2", "dpmsolver++", 20), ("ddpm", "ddpm", 250)]
# (label, batch, size, latency mode, calls per timed window for each rule)
SHAPES = [("b64", 64, 64, False, (4, 1)), ("b1", 1, 128, True, (8, 2))]
QUANTILE = [(64, 12288), (1, 49152), (32, 49152)]
NEW_SYMBOLS = ("sisic_set_step_thresholding", "sisic_set_step_image_elems", "sisic_unet_set_thresholding", "sisic_x0_threshold")


def spread(xs):
    return f"{statistics.median(xs):9.4f}   ({min(xs):.4f} .. {max(xs):.4f})"


def tolerate_older_library():
    """a library from before this feature: drop the bindings it lacks and the call that sets the handle's (off) setting
    (sampler._set_thresholding, a private name: this tool is the only place that steps around it, and only for part B)"""
    import ctypes
    from synt_isic_amd import _lib, sampler
    lib = ctypes.CDLL(_lib.lib_path())
    if all(hasattr(lib, name) for name in NEW_SYMBOLS):
        return False
    for name in NEW_SYMBOLS:
        _lib.SIGNATURES.pop(name, None)
    sampler._set_thresholding = lambda lib, model, threshold: None
    return True


def loop_runs(shape, with_on):
    """[(label, callable running `calls` loops, steps per call)] of one shape, warmed up"""
    import torch
    from synt_isic_amd.sampler import DeviceNoise, Sampler, run_sampling_loop
    from synt_isic_amd.weights import synthetic_unet_state_dict
    name, batch, size, latency, calls = shape
    s = Sampler(latency_mode=latency)
    model = s.add_model("NV", synthetic_unet_state_dict())
    seeds = list(range(batch))
    x_T = torch.randn((batch, model.config.in_channels, size, size), generator=torch.Generator().manual_seed(0)).to("cuda")
    runs = []
    for (label, sched_name, T), n_calls in zip(RULES, calls):
        sched = s.create_scheduler(T, sched_name)
        for on in ((False, True) if with_on else (False,)):
            kw = dict(thresholding=True, dynamic_thresholding_ratio=THR[0], sample_max_value=THR[1]) if on else {}

            def run(sched=sched, kw=kw, n_calls=n_calls):
                for _ in range(n_calls):
                    run_sampling_loop(model, sched, x_T, DeviceNoise(tuple(seeds)), **kw)
            run()                                                            # warm-up: workspace, the captured step
            base = f"{name} {label:20s} T={T:3d}"
            runs.append((f"{base} thresholding {'on ' if on else 'off'}", run, n_calls * T, base))
    return runs


def timed(run, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def part_loop(a, shape_name, say):
    shape = next(s for s in SHAPES if s[0] == shape_name)
    runs = loop_runs(shape, True)
    say(f"# A. run_sampling_loop alone, batch {shape[1]} at 3x{shape[2]}x{shape[2]}, {'latency mode (graph-replayed)' if shape[3] else 'eager'}, "
        f"DeviceNoise: ms per step")
    times = [[] for _ in runs]
    for _ in range(a.reps):
        for k, (_, run, steps, _b) in enumerate(runs):
            times[k].append(timed(run, steps))
    for (label, _, _, _b), ts in zip(runs, times):
        say(f"loop  {label}   ms/step {spread(ts)}")
    for k in range(0, len(runs), 2):
        off, on = statistics.median(times[k]), statistics.median(times[k + 1])
        say(f"loop  {runs[k][3]}   on - off = {1e3 * (on - off):8.2f} us per step ({100 * (on - off) / off:+.2f} %)")


def part_lib(a, say):
    """one alternation of part B in this process: the unthresholded loops under the library of SISIC_LIB_PATH"""
    older = tolerate_older_library()
    for shape in SHAPES:
        for label, run, steps, _b in loop_runs(shape, False):
            say(f"lib   {label}   ms/step {timed(run, steps):9.4f}" + ("   (library without the feature)" if older else ""))


def part_quantile(a, say):
    import torch
    from synt_isic_amd import ops
    say("# C. ops.x0_threshold alone (epsilon prediction, ratio 0.995): us per launch, 200 back-to-back launches between two events")
    cases = []
    for B, n in QUANTILE:
        g = torch.Generator().manual_seed(n + B)
        eps, x = (torch.randn((B, n), generator=g).to("cuda") * 1.5 for _ in range(2))
        ops.x0_threshold(eps, x, 0.6, 0.8, *THR)
        cases.append((B, n, eps, x))
    times = [[] for _ in cases]
    for _ in range(a.reps):
        for k, (B, n, eps, x) in enumerate(cases):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _k in range(200):
                ops.x0_threshold(eps, x, 0.6, 0.8, *THR)
            stop.record()
            torch.cuda.synchronize()
            times[k].append(start.elapsed_time(stop) / 200 * 1e3)
    for (B, n, _, _), ts in zip(cases, times):
        say(f"quant (B, n) = ({B:2d}, {n:5d})   us/launch {spread(ts)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400, help="seconds each part may take (its `timeout`)")
    ap.add_argument("--other-lib", default=None, help="libsisic_hip.so of another commit, for part B")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--part", default=None, help="run this part in this process (what the driver starts)")
    a = ap.parse_args()

    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("threshold_bench needs an MI355X: nothing is measured without one")
        say = lambda text="": print(text, flush=True)
        if a.part.startswith("loop-"):
            part_loop(a, a.part[5:], say)
        elif a.part == "lib":
            part_lib(a, say)
        else:
            part_quantile(a, say)
        return

    # the driver: no GPU work of its own; one child per part, each under its own time limit, none after a failure
    lines = [f"# tools/threshold_bench.py --reps {a.reps}: one process per part, configurations alternated, median (min .. max) of "
             f"{a.reps} equal runs; thresholding on = ratio {THR[0]}, sample_max_value {THR[1]}"]
    print(lines[0], flush=True)

    def child(part, env=None):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        if r.returncode != 0:
            print(r.stdout, end="", flush=True)
            lines.append(f"# part {part} ended with status {r.returncode}: nothing after it was run")
            print(lines[-1], flush=True)
            finish(r.returncode)
        return [ln for ln in r.stdout.splitlines() if ln.startswith(("#", "loop ", "lib ", "quant "))]

    def finish(status):
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines).rstrip("\n") + "\n")
        sys.exit(status)

    for part in ("loop-b64", "loop-b1"):
        got = child(part)
        print("\n".join(got), flush=True)
        lines += got + [""]
    if a.other_lib:
        from synt_isic_amd import _lib
        libs = [("this library ", _lib.lib_path()), ("other library", os.path.abspath(a.other_lib))]
        lines.append(f"# B. the unthresholded loops of part A, this library against {os.path.basename(a.other_lib)} (another commit's "
                     f"sources built with the same Makefile): one process per library and alternation, ms per step")
        print(lines[-1], flush=True)
        samples = {}
        for rep in range(a.reps):
            # (the order turns round every alternation: the first process after a pause ran slower whichever library it loaded)
            for which, path in (libs if rep % 2 == 0 else libs[::-1]):
                print(f"# B: alternation {rep + 1} of {a.reps}, {which.strip()}", flush=True)
                for ln in child("lib", dict(os.environ, SISIC_LIB_PATH=path)):
                    label, value = ln[6:].split("   ms/step ")
                    samples.setdefault((label, which), []).append(float(value.split()[0]))
        for label in dict.fromkeys(k[0] for k in samples):
            for which, _ in libs:
                lines.append(f"lib   {label}   {which}   ms/step {spread(samples[(label, which)])}")
                print(lines[-1], flush=True)
            mine, other = samples[(label, libs[0][0])], samples[(label, libs[1][0])]
            diff = 100 * (statistics.median(mine) / statistics.median(other) - 1)
            # what the comparison can resolve: the wider of the two ranges of equal runs, as a share of the median
            width = 100 * max(max(mine) - min(mine), max(other) - min(other)) / statistics.median(other)
            lines.append(f"lib   {label}   median difference {diff:+.2f} %, range of equal runs {width:.2f} %: "
                         f"{'inside' if abs(diff) <= width else 'OUTSIDE'} it (a difference below that range is not resolved)")
            print(lines[-1], flush=True)
        lines.append("")
    got = child("quantile")
    print("\n".join(got), flush=True)
    lines += got
    finish(0)


if __name__ == "__main__":
    main()
