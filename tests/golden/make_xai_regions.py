"""Generates tests/golden/xai_regions.npz: the region masks of synt_isic_amd.xai.select_regions as scipy.ndimage computes
them, so that the numpy morphology of the product (which must not import scipy) is pinned on machines without scipy.

Run from the repo root, on a machine with scipy:  python tests/golden/make_xai_regions.py

Rows follow tests/xai_ref.py::region_cases(): seeds 0..3 x H in {64, 128} x average-pool edge in {1, 9, 15} x top / bottom x
connectivity 4 / 8 x clean-up on / off.
  masks64, masks128  uint8 [rows of that size, H*H/8]: the masks, bit-packed (np.packbits of the flattened mask)
  cases              int [N,6]: seed, H, pool, 1 = top, connectivity, 1 = clean-up
  threshold          float64 [N]
  selected           int64 [N]: pixels in the mask
  float_stats        float64 [N,7]: xai_ref.FLOAT_STATS of the 'statistics' dict
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import xai_ref  # noqa: E402


def main() -> None:
    masks = {64: [], 128: []}
    cases, thresholds, selected, fstats = [], [], [], []
    for seed, H, pool, rt, conn, cleanup in xai_ref.region_cases():
        attr = xai_ref.region_input(seed, H, pool)
        mask, thr = xai_ref.regions_scipy(attr, 10, rt, cleanup, conn)
        st = xai_ref.region_statistics(attr, mask, thr)
        masks[H].append(np.packbits(mask.ravel()))
        cases.append((seed, H, pool, int(rt == "top"), conn, int(cleanup)))
        thresholds.append(thr)
        selected.append(st["selected_pixels"])
        fstats.append([float(st[k]) for k in xai_ref.FLOAT_STATS])
    path = os.path.join(HERE, "xai_regions.npz")
    np.savez_compressed(path, masks64=np.stack(masks[64]), masks128=np.stack(masks[128]), cases=np.array(cases),
                        threshold=np.array(thresholds, dtype=np.float64), selected=np.array(selected, dtype=np.int64),
                        float_stats=np.array(fstats, dtype=np.float64))
    print(f"{path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
