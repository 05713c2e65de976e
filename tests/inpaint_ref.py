"""Plain-torch, CPU restatement of the image-editing feature (include/sisic.h "image editing"), written
from the feature's text and from RePaint (Lugmayr et al. 2022, Algorithm 1 and the published ``get_schedule_jump``), not from
the library:

  * ``visited_levels`` / ``resample_schedule``: the paper's list of visited noise levels, and the same run as one
    ``(grid index, jump)`` per UNet pass;
  * ``edit_rows64`` / ``edit_rows``: {ck, sk, ja, jb} per pass, float64 and rounded to fp32 once;
  * ``edit_one``: the epilogue, one fp32 torch operation per rounding, in the stated order;
  * ``noise``: the epilogue's normals through tests/philox_ref.py (float64, rounded to fp32).

The step kernel's own generator agrees with ``philox_ref`` word for word in its raw bits and within a few ulp in its normals
(tests/test_gpu_device_noise.py), so a bit-for-bit comparison of a step feeds ``edit_one`` the normals ``sisic_noise_fill``
writes under the same (seed, step, tag), and ``noise`` checks those against the contract.
"""
import math

import numpy as np
import torch

import philox_ref

TAG_KNOWN, TAG_JUMP = 5, 6


def visited_levels(T: int, jump_length: int, n_resample: int):
    """RePaint's ``get_schedule_jump`` with one sample per jump height, read in levels: L is the number of reverse steps still to
    go, the run starts at L = T and ends at L = 0 (the clean image), and the first ``n_resample - 1`` times it reaches a
    level in ``range(0, T - jump_length, jump_length)`` it goes ``jump_length`` levels up again, one forward step at a time.
    (The published code keeps the same bookkeeping on its timestep t = L - 1, so its jumps start one level higher; the
    feature's text counts levels, and so does this list.)"""
    jumps = {L: n_resample - 1 for L in range(0, T - jump_length, jump_length)}
    L, levels = T, [T]
    while L >= 1:
        L -= 1
        levels.append(L)
        if jumps.get(L, 0) > 0:
            jumps[L] -= 1
            for _ in range(jump_length):
                L += 1
                levels.append(L)
    return levels


def resample_schedule(T: int, jump_length: int, n_resample: int):
    """the run as UNet passes: consecutive levels (a, b) with b < a are one reverse step, taken by a pass at grid index T - a;
    the rising entries after it are the jump that follows that pass"""
    levels = visited_levels(T, jump_length, n_resample)
    out = []
    for a, b in zip(levels[:-1], levels[1:]):
        if b < a:
            out.append([T - a, 0])
        else:
            out[-1][1] += 1
    return [tuple(e) for e in out]


def abar64(alphas_fp32) -> np.ndarray:
    """cumulative product, in float64, of the scheduler's fp32 ``alphas`` = 1 - betas"""
    return np.cumprod(np.asarray(alphas_fp32, dtype=np.float32).astype(np.float64))


def edit_rows64(alphas_fp32, grid, schedule, rule: str = "ddpm", n_train: int = 1000, n_grid=None) -> np.ndarray:
    """float64 [passes, 4] rows {ck, sk, ja, jb}.  grid: the run's timesteps (descending); n_grid: the length of the full grid
    when ``grid`` is the tail of one (image-to-image).  The level a pass steps to is its own rule row's: under ddpm / ddim the
    timestep ``t - n_train // n_grid`` (abar = 1 below 0), under dpmsolver++ the next grid entry (abar = 1 after the last)."""
    abar = abar64(alphas_fp32)
    grid = [int(t) for t in grid]
    n_grid = len(grid) if n_grid is None else int(n_grid)
    rows = np.zeros((len(schedule), 4), dtype=np.float64)
    for p, (i, jump) in enumerate(schedule):
        if rule == "dpmsolver++":
            prev = abar[grid[i + 1]] if i + 1 < len(grid) else 1.0
        else:
            prev_t = grid[i] - n_train // n_grid
            prev = abar[prev_t] if prev_t >= 0 else 1.0
        ja, jb = 1.0, 0.0
        if jump:
            ratio = abar[grid[i + 1 - jump]] / prev          # the next pass runs at grid entry i + 1 - jump
            ja, jb = math.sqrt(ratio), math.sqrt(1.0 - ratio)
        rows[p] = (math.sqrt(prev), math.sqrt(1.0 - prev), ja, jb)
    return rows


def edit_rows(*args, **kwargs) -> torch.Tensor:
    return torch.from_numpy(edit_rows64(*args, **kwargs).astype(np.float32))


def _f(v) -> torch.Tensor:
    return torch.tensor(float(v), dtype=torch.float32)


def edit_one(u: torch.Tensor, x0k: torch.Tensor, m: torch.Tensor, e1, e2, row) -> torch.Tensor:
    """the epilogue on CPU fp32 tensors: u, x0k [B,C,H,W]; m [B,1,H,W] (broadcast over channels); e1, e2 [B,C,H,W] or None when
    the row does not draw them; row = (ck, sk, ja, jb).  One torch operation per rounding:
        k = ck * x0k + sk * e1;  y = m * k + (1 - m) * u;  out = ja * y + jb * e2"""
    ck, sk, ja, jb = (float(v) for v in row)
    assert u.dtype == x0k.dtype == m.dtype == torch.float32
    k = _f(ck) * x0k
    if sk != 0.0:
        k = k + _f(sk) * e1
    a = m * k
    om = _f(1.0) - m
    b = om * u
    y = a + b
    if jb != 0.0:
        y = _f(ja) * y + _f(jb) * e2
    return y


def noise(seeds, step: int, tag: int, chw) -> torch.Tensor:
    """fp32 [B, C, H, W]: the contract's normals of (seed_b, step, tag), float64 rounded to fp32"""
    n = int(np.prod(chw))
    z = np.stack([philox_ref.noise_normals(int(s), int(step), int(tag), n)[0] for s in seeds])
    return torch.from_numpy(z.astype(np.float32)).reshape((len(seeds),) + tuple(chw))
