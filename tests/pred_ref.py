"""CPU restatement of the three step rules under the three prediction types, and of the weighted training loss.

TEST INFRASTRUCTURE ONLY, in the style of tests/ddim_ref.py and tests/dpmpp_ref.py: every scalar is a 0-dim torch tensor of
``dtype`` (fp32 by default; float64 for the algebraic checks of tests/test_prediction_cpu.py), every operation is a separate
torch op with one rounding, in the order of the published ``diffusers`` schedulers (include/sisic.h, SISIC_PRED_*).  Let o be
the model's output, sb and sa columns 0 and 1 of the rule's row:

    x0 before the clamp     epsilon (x - sb*o)/sa          sample o                       v_prediction sa*x - sb*o
    DDIM direction term     epsilon o                      sample (x - sa*x0)/sb          v_prediction sa*o + sb*x
                            (sample: with the UNCLAMPED x0; use_clipped_model_output: (x - sa*x0_clamped)/sb under every type)
    DDPM                    out  = (c0*x0 + c1*x) [+ sigma*z]
    DDIM                    out  = (c_prev*x0 + c_dir*pe) [+ sigma*z]
    DPM-Solver++(2M)        out  = (cx*x + k0*x0) [+ k1*hist] [+ sigma*z];   hist = x0 (clamped)

At ``prediction_type="epsilon"`` these are tests/ddim_ref.py, tests/dpmpp_ref.py and oracle/ddpm.py bit for bit
(tests/test_prediction_cpu.py asserts it).

The weighted loss (numpy fp32, ``weighted_mse``): d = pred - target, c = fp32(grad_scale * 2 / n) formed as the library forms
it, dpred = (c * w_b) * d, loss = sum(w_b * d^2) / n in float64 (the library's fp32 tree is held to 1e-6 of it).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

TYPES = ("epsilon", "sample", "v_prediction")


def _scalars(row, dtype):
    return tuple(torch.tensor(float(v), dtype=dtype) for v in row)


def raw_x0(o: torch.Tensor, x: torch.Tensor, sb: torch.Tensor, sa: torch.Tensor, prediction_type: str) -> torch.Tensor:
    """the model's estimate of x0 before the clamp"""
    if prediction_type == "epsilon":
        return (x - sb * o) / sa
    if prediction_type == "sample":
        return o
    if prediction_type == "v_prediction":
        return sa * x - sb * o
    raise NotImplementedError(prediction_type)


def _clamp(x0: torch.Tensor, clip: float) -> torch.Tensor:
    return x0.clamp(-clip, clip) if clip > 0 else x0


def ddpm_step_row(o, x, z: Optional[torch.Tensor], row, clip: float = 1.0, prediction_type: str = "epsilon",
                  dtype=torch.float32) -> torch.Tensor:
    """row = (sb, sa, c0, c1, sigma)"""
    sb, sa, c0, c1, sigma = _scalars(row, dtype)
    x0 = _clamp(raw_x0(o, x, sb, sa, prediction_type), clip)
    prev = c0 * x0 + c1 * x
    if float(sigma) != 0.0 and z is not None:
        prev = prev + sigma * z
    return prev


def ddim_step_row(o, x, z: Optional[torch.Tensor], row, clip: float = 1.0, use_clipped_model_output: bool = False,
                  prediction_type: str = "epsilon", dtype=torch.float32) -> torch.Tensor:
    """row = (sb, sa, c_prev, c_dir, sigma)"""
    sb, sa, c_prev, c_dir, sigma = _scalars(row, dtype)
    x0u = raw_x0(o, x, sb, sa, prediction_type)
    x0 = _clamp(x0u, clip)
    if use_clipped_model_output:
        pe = (x - sa * x0) / sb
    elif prediction_type == "epsilon":
        pe = o
    elif prediction_type == "sample":
        pe = (x - sa * x0u) / sb
    else:
        pe = sa * o + sb * x
    prev = c_prev * x0 + c_dir * pe
    if float(sigma) != 0.0 and z is not None:
        prev = prev + sigma * z
    return prev


def dpmpp_step_row(o, x, z: Optional[torch.Tensor], hist: Optional[torch.Tensor], row, clip: float = 0.0,
                   prediction_type: str = "epsilon", dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """row = (sb, sa, cx, k0, sigma, k1); returns (prev_sample, this step's clamped x0 = the next step's hist)"""
    sb, sa, cx, k0, sigma, k1 = _scalars(row, dtype)
    x0 = _clamp(raw_x0(o, x, sb, sa, prediction_type), clip)
    prev = cx * x + k0 * x0
    if float(k1) != 0.0:
        prev = prev + k1 * hist
    if float(sigma) != 0.0 and z is not None:
        prev = prev + sigma * z
    return prev, x0


def step_row(rule: str, o, x, z, hist, row, clip, prediction_type: str = "epsilon", use_clipped_model_output: bool = False,
             dtype=torch.float32):
    """one step of ``rule`` ("ddpm", "ddim", "dpmsolver++"); returns (prev_sample, hist or None)"""
    if rule == "ddpm":
        return ddpm_step_row(o, x, z, row, clip, prediction_type, dtype), None
    if rule == "ddim":
        return ddim_step_row(o, x, z, row, clip, use_clipped_model_output, prediction_type, dtype), None
    return dpmpp_step_row(o, x, z, hist, row, clip, prediction_type, dtype)


def velocity(x0: torch.Tensor, noise: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """DDPMScheduler.get_velocity with per-sample rows sa, sb [B]: sa*noise - sb*x0, two products and one difference"""
    shape = (-1,) + (1,) * (x0.dim() - 1)
    return sa.reshape(shape) * noise - sb.reshape(shape) * x0


def model_output_of(prediction_type: str, x0: torch.Tensor, eps: torch.Tensor, sa, sb) -> torch.Tensor:
    """what an exact model of the type returns for (x0, eps) at a level (sa, sb): scalars or per-sample rows"""
    if prediction_type == "epsilon":
        return eps
    if prediction_type == "sample":
        return x0
    return sa * eps - sb * x0


def weighted_mse(pred: np.ndarray, target: np.ndarray, weights: Optional[np.ndarray], grad_scale: float = 1.0):
    """(loss as float64, dpred as fp32 [n]) of the weighted loss; pred, target fp32 [B, per]; weights fp32 [B] or None.
    dpred is what the kernel stores bit for bit: c = fp32(fp32(grad_scale * 2) / fp32(n)), g_b = c * w_b, dpred = g_b * d."""
    pred, target = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    B = pred.shape[0]
    n = pred.size
    d = (pred - target).astype(np.float32)
    c = np.float32(np.float32(np.float32(grad_scale) * np.float32(2.0)) / np.float32(n))
    if weights is None:
        g = np.full((B,), c, dtype=np.float32)
        w64 = np.ones((B,), dtype=np.float64)
    else:
        w = np.asarray(weights, dtype=np.float32).reshape(B)
        g = (c * w).astype(np.float32)
        w64 = w.astype(np.float64)
    shape = (B,) + (1,) * (pred.ndim - 1)
    dpred = (g.reshape(shape) * d).astype(np.float32)
    d64 = pred.astype(np.float64) - target.astype(np.float64)
    loss = float((w64.reshape(shape) * d64 ** 2).sum() / n)
    return loss, dpred
