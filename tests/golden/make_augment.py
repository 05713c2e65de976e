"""Generates tests/golden/augment.npz with PIL: what torchvision's PIL backend returns for given augmentation parameters.

    python tests/golden/make_augment.py

Six random textures (uniform noise and a random walk at 16x16, 32x32 and 24x40 -- height x width; the smallest sizes at which
every stage has interior pixels, three-tap and clamped-edge resize columns, a rotation with filled corners, and H != W) and,
per size, parameter records in three groups with PIL's uint8 results:
  group 0  each stage alone: the full-image box, four shifted / shrunk boxes (one of them x-only, one y-only), the flips,
           each colour operation at the ends of its range and at two interior factors, rotations by +-15, +-0.5 and three
           interior angles                                                                        (all three sizes)
  group 1  the six orders of the three colour operations                                       (16x16 and 24x40)
  group 2  eight full-chain records drawn from a fixed seed                                     (all three sizes)
Keys, per size key K in 16x16, 32x32, 24x40:  img_K uint8 [2,H,W,3]; rec_K the records (struct sisic_augment_params, src
indexes img_K); angle_K the rotation angles in degrees the records' fixed-point maps were made from; group_K; u8_K uint8
[R,H,W,3] PIL's results; f32_K float32 [8,3,H,W] torch's (u8.float()/255 - 0.5)/0.5 of the group-2 results.  norm_lut
float32 [256]: the same normalisation of every uint8 value, which gives the expected floats of every other record.
Not hand-edited; needs PIL and torch.  The GPU tests read the file, never PIL."""
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import augment_ref as R  # noqa: E402

SIZES = {"16x16": (16, 16), "32x32": (32, 32), "24x40": (24, 40)}       # H, W
f32 = lambda v: float(np.float32(v))  # noqa: E731


def textures(rng, H, W):
    noise = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    steps = rng.integers(-9, 10, size=(H, W, 3))
    walk = 128 + np.cumsum(steps, axis=0) + np.cumsum(steps[::-1, ::-1], axis=1)
    return np.stack([noise, np.clip(walk, 0, 255).astype(np.uint8)])


def stage_alone(H, W):
    cases = [dict()]
    w9, h9 = (W * 9 + 9) // 10, (H * 9 + 9) // 10
    cases += [dict(box=(1, 2, W - 3, H - 4)), dict(box=(0, 0, W - 2, H)), dict(box=(0, 3, W, H - 3)),
              dict(box=(W - w9, 0, w9, h9))]
    cases += [dict(hflip=1), dict(vflip=1), dict(hflip=1, vflip=1)]
    for op, factors in ((R.BRIGHTNESS, (0.7, 1.3, 0.8531, 1.1337)), (R.CONTRAST, (0.7, 1.3, 0.9123, 1.2046)),
                        (R.SATURATION, (0.8, 1.2, 0.8817, 1.0719))):
        for f in factors:
            factor = [1.0, 1.0, 1.0]
            factor[op] = f32(f)
            cases.append(dict(order=(op, -1, -1), factor=tuple(factor)))
    cases += [dict(angle=a) for a in (15.0, -15.0, 0.5, -0.5, 7.3, -11.9, 3.14159)]
    return cases


def colour_orders():
    return [dict(order=perm, factor=(f32(1.21), f32(0.77), f32(1.13))) for perm in itertools.permutations(range(3))]


def full_chain(rng, H, W, n=8):
    cases = []
    for k in range(n):
        w = int(rng.integers((W * 17 + 19) // 20, W + 1))
        h = int(rng.integers((H * 17 + 19) // 20, H + 1))
        order = [int(v) for v in rng.permutation(3)]
        if k == n - 1:
            order[int(rng.integers(0, 3))] = -1                    # one record with a skipped slot
        cases.append(dict(box=(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h),
                          hflip=int(rng.integers(0, 2)), vflip=int(rng.integers(0, 2)), order=tuple(order),
                          factor=(f32(rng.uniform(0.7, 1.3)), f32(rng.uniform(0.7, 1.3)), f32(rng.uniform(0.8, 1.2))),
                          angle=float(rng.uniform(-15.0, 15.0)) if k % 8 < 5 else None))
    return cases


def main():
    rng = np.random.default_rng(20181)
    out = {"norm_lut": ((torch.arange(256, dtype=torch.uint8).float() / 255 - 0.5) / 0.5).numpy()}
    for key, (H, W) in SIZES.items():
        imgs = textures(rng, H, W)
        groups = [(0, stage_alone(H, W)), (2, full_chain(rng, H, W))]
        if key != "32x32":
            groups.insert(1, (1, colour_orders()))
        recs, angles, gids, results = [], [], [], []
        for gid, cases in groups:
            for k, case in enumerate(cases):
                rec = R.make_record(k % 2, H, W, **case)
                angle = case.get("angle") or 0.0
                recs.append(rec)
                angles.append(angle)
                gids.append(gid)
                results.append(R.pil_augment(imgs, rec, angle))
        u8 = np.stack(results)
        gids = np.array(gids, dtype=np.int32)
        full = torch.from_numpy(u8[gids == 2]).permute(0, 3, 1, 2)
        out.update({f"img_{key}": imgs, f"rec_{key}": np.array(recs, dtype=R.AUGMENT_DTYPE),
                    f"angle_{key}": np.array(angles, dtype=np.float64), f"group_{key}": gids, f"u8_{key}": u8,
                    f"f32_{key}": ((full.float() / 255 - 0.5) / 0.5).contiguous().numpy()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items() if k.startswith("u8_")})


if __name__ == "__main__":
    main()
