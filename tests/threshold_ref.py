"""CPU restatement of dynamic thresholding of x0 (Saharia et al. 2022; include/sisic.h, sisic_x0_threshold), and a numpy model
of the selection the kernel runs.

TEST INFRASTRUCTURE ONLY, in the style of tests/pred_ref.py.  Three things:

* ``torch_threshold``: the published ``_threshold_sample`` as the schedulers write it -- ``torch.quantile(abs, ratio, dim=1)``,
  ``clamp(s, 1, max)``, ``clamp(x0, -s, s) / s``.  The reference of the contract, nothing of ours in it.
* ``quantile_spelled`` / ``threshold_s`` / ``threshold_x0``: the contract's spelling of that quantile -- the rank in fp32, the
  two order statistics, ONE fused multiply-add -- with numpy fp32 scalars and an exactly rounded fma.  What the kernel must equal
  bit for bit; tests/test_threshold_cpu.py holds it to ``torch_threshold``.
* ``radix_select_model``: the kernel's algorithm on the integer keys -- four passes of 8, 8, 8 and 7 bits from the top, the count
  of keys <= a_lo, the successor rule -- held to sorting by the same file.

``step_row``: a step of any rule under any prediction type with the thresholded x0 in place of the clamped one, composed from
tests/pred_ref.py's ``raw_x0`` and the rules' published lines.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

import pred_ref

F32 = np.float32


def torch_threshold(x0: torch.Tensor, ratio: float, sample_max_value: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """the published lines; x0 [B, ...] fp32 on the CPU.  Returns (x0', s [B])"""
    B = x0.shape[0]
    flat = x0.reshape(B, -1)
    s = torch.quantile(flat.abs(), ratio, dim=1)
    s = torch.clamp(s, min=1, max=sample_max_value)
    s = s.unsqueeze(1)
    out = torch.clamp(flat, -s, s) / s
    return out.reshape(x0.shape), s.reshape(B)


def fma32(a, b, c) -> np.float32:
    """fl32(a * b + c) with ONE rounding, for fp32 a, b, c"""
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))      # inf and NaN need no rounding
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        # (the sign of an exact zero: +0 unless both terms are -0, as round-to-nearest has it)
        return F32(float(a) * float(b) + float(c))
    with np.errstate(over="ignore"):
        guess = F32(float(exact))                   # may be double-rounded: look at the neighbours
    best = None
    for cand in (np.nextafter(guess, F32(-np.inf)), guess, np.nextafter(guess, F32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - exact)
        even = (int(F32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, F32(cand), even)
    if best is None:
        return guess
    # overflow past the largest finite value rounds to infinity
    big = Fraction(float(np.finfo(F32).max)) + Fraction(2) ** 103
    if abs(exact) >= big:
        return F32(np.inf) if exact > 0 else F32(-np.inf)
    return best[1]


def rank_of(ratio: float, n: int) -> Tuple[int, int, np.float32]:
    """(lo, hi, w) of the contract: r = fl32(fl32(ratio) * fl32(n - 1))"""
    r = F32(F32(ratio) * F32(n - 1))
    lo, hi = int(np.floor(r)), int(np.ceil(r))
    return lo, hi, F32(r - F32(lo))


def interpolate(a_lo, a_hi, w) -> np.float32:
    """q of the contract from the two order statistics; ``unfused_interpolate`` is the planted error"""
    a_lo, a_hi, w = F32(a_lo), F32(a_hi), F32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = F32(a_hi - a_lo)
        if w < F32(0.5):
            return fma32(w, d, a_lo)
        return fma32(F32(w - F32(1.0)), d, a_hi)


def unfused_interpolate(a_lo, a_hi, w) -> np.float32:
    a_lo, a_hi, w = F32(a_lo), F32(a_hi), F32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = F32(a_hi - a_lo)
        if w < F32(0.5):
            return F32(a_lo + F32(w * d))
        return F32(a_hi + F32(F32(w - F32(1.0)) * d))


def quantile_spelled(row: np.ndarray, ratio: float, *, rank_n: Optional[int] = None, use_abs: bool = True,
                     interp=interpolate) -> np.float32:
    """q of one image (any shape, fp32).  A NaN anywhere gives NaN.  rank_n, use_abs, interp: the planted errors of the tests."""
    a = np.asarray(row, dtype=F32).reshape(-1)
    if use_abs:
        a = np.abs(a)
    if np.isnan(a).any():
        return F32(np.nan)
    a = np.sort(a)
    n = a.size
    lo, hi, w = rank_of(ratio, n if rank_n is None else rank_n)
    return interp(a[lo], a[min(hi, n - 1)], w)


def clamp_s(q, sample_max_value: float) -> np.float32:
    """s = min(max(q, 1), max) with torch.clamp's NaN"""
    q = F32(q)
    if np.isnan(q):
        return q
    return F32(min(max(q, F32(1.0)), F32(sample_max_value)))


def threshold_s(x0: torch.Tensor, ratio: float, sample_max_value: float, **planted) -> torch.Tensor:
    """s [B] of the contract for x0 [B, ...]"""
    flat = x0.detach().to("cpu", torch.float32).reshape(x0.shape[0], -1).numpy()
    return torch.from_numpy(np.array([clamp_s(quantile_spelled(r, ratio, **planted), sample_max_value) for r in flat], dtype=F32))


def apply_s(x0: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """x0' = clamp(x0, -s, s) / s with image b's s"""
    sv = s.to(x0.device).reshape((-1,) + (1,) * (x0.dim() - 1))
    return torch.clamp(x0, -sv, sv) / sv


def threshold_x0(x0: torch.Tensor, ratio: float, sample_max_value: float) -> torch.Tensor:
    return apply_s(x0, threshold_s(x0, ratio, sample_max_value))


# ---- the kernel's selection on integer keys --------------------------------------------------------------------------------
PASSES = ((23, 8), (15, 8), (7, 8), (0, 7))          # (shift, bits) from the top of the 31 key bits


def keys_of(row: np.ndarray) -> np.ndarray:
    """bit patterns of |x0|: non-negative floats order as their bits do"""
    return np.asarray(row, dtype=F32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)


def radix_select_model(keys: np.ndarray, lo: int, hi: int):
    """(a_lo, a_hi, count of keys <= a_lo, has_nan) as the kernel finds them: histogram passes from the top, then a_hi = a_lo
    where the count reaches lo + 2 (or hi == lo), else the smallest key above a_lo"""
    keys = np.asarray(keys, dtype=np.uint32)
    has_nan = bool((keys > np.uint32(0x7F800000)).any())
    prefix, k, cnt = 0, int(lo), 0
    for sh, bits in PASSES:
        top = sh + bits
        match = keys[(keys >> np.uint32(top)) == np.uint32(prefix >> top)] if top < 32 else keys
        hist = np.bincount(((match >> np.uint32(sh)) & np.uint32((1 << bits) - 1)).astype(np.int64), minlength=256)
        excl = 0
        for d in range(256):
            if k < excl + hist[d]:
                prefix |= d << sh
                k -= excl
                cnt = int(hist[d])
                break
            excl += int(hist[d])
        else:
            raise AssertionError("rank outside the keys")
    a_lo = prefix
    cnt_le = (int(lo) - k) + cnt
    if hi == lo or cnt_le >= lo + 2:
        a_hi = a_lo
    else:
        a_hi = int(keys[keys > np.uint32(a_lo)].min())
    return a_lo, a_hi, cnt_le, has_nan


def model_s(row: np.ndarray, ratio: float, sample_max_value: float) -> np.float32:
    """s of one image as the kernel computes it: the selection above, then the five-line float formula"""
    keys = keys_of(row)
    lo, hi, w = rank_of(ratio, keys.size)
    a_lo, a_hi, _, has_nan = radix_select_model(keys, lo, hi)
    if has_nan:
        return F32(np.nan)
    q = interpolate(np.uint32(a_lo).view(F32), np.uint32(a_hi).view(F32), w)
    return clamp_s(q, sample_max_value)


# ---- a step of any rule with the thresholded x0 ------------------------------------------------------------------------------
def step_row(rule: str, o, x, z, hist, row, threshold, prediction_type: str = "epsilon", use_clipped_model_output: bool = False,
             s: Optional[torch.Tensor] = None):
    """one step of ``rule`` ("ddpm", "ddim", "dpmsolver++") under ``threshold = (ratio, max)``; tensors are [B, ...] fp32 on the
    CPU.  Returns (prev_sample, hist or None, s [B]).  ``s``: use this instead of computing it (for planted errors)."""
    dtype = torch.float32
    sc = pred_ref._scalars(row, dtype)
    sb, sa = sc[0], sc[1]
    x0u = pred_ref.raw_x0(o, x, sb, sa, prediction_type)
    if s is None:
        s = threshold_s(x0u, *threshold)
    x0 = apply_s(x0u, s)
    if rule == "ddpm":
        _, _, c0, c1, sigma = sc
        prev = c0 * x0 + c1 * x
        new_hist = None
    elif rule == "ddim":
        _, _, c_prev, c_dir, sigma = sc
        if use_clipped_model_output:
            pe = (x - sa * x0) / sb
        elif prediction_type == "epsilon":
            pe = o
        elif prediction_type == "sample":
            pe = (x - sa * x0u) / sb
        else:
            pe = sa * o + sb * x
        prev = c_prev * x0 + c_dir * pe
        new_hist = None
    else:
        _, _, cx, k0, sigma, k1 = sc
        prev = cx * x + k0 * x0
        if float(k1) != 0.0:
            prev = prev + k1 * hist
        new_hist = x0
    if float(sigma) != 0.0 and z is not None:
        prev = prev + sigma * z
    return prev, new_hist, s
