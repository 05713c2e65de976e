"""Generates tests/golden/xai_stats.npz: what the scipy calls of xai/XAI.py:1708-2005 return for the cases of
tests/xai_stats_ref.py::case_inputs(), so that synt_isic_amd.xai_stats (which must not import scipy) is pinned on machines
without scipy.  Recorded with scipy 1.15.3.

Run from the repo root, on a machine with scipy:  python tests/golden/make_xai_stats.py

For every case <name>:  <name>_a, <name>_b  float64: the two samples;  <name>_vals  float64 [16]: xai_stats_ref.KEYS.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import xai_stats_ref  # noqa: E402


def main() -> None:
    import scipy
    out = {}
    for name, (a, b) in xai_stats_ref.case_inputs().items():
        out[name + "_a"], out[name + "_b"] = a, b
        out[name + "_vals"] = xai_stats_ref.scipy_values(a, b)
    path = os.path.join(HERE, "xai_stats.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out) // 3} cases, scipy {scipy.__version__}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
