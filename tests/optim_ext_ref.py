"""Plain torch / numpy restatement of what the clipping / EMA / learning-rate extensions compute (imported by
test_optim_ext_cpu.py and test_gpu_optim_ext.py, as ddim_ref / dpmpp_ref are by theirs).

    get_decay            diffusers.training_utils.EMAModel.get_decay
    ema_update           EMAModel.step on one tensor: s.sub_(one_minus_decay * (s - p)), fp32
    adam_update          the library's Adam update on one vector (torch.optim.Adam's operation order on the unscaled, clipped
                         gradient), fp32, one rounded operation at a time
    clip_stats           torch.nn.utils.clip_grad_norm_: the norm from a float64 sum of squares of the fp32 values g * inv_scale,
                         the coefficient in fp32 from that norm
    clip_coef_of         the coefficient alone, from a given fp32 norm
    cosine_lambda        diffusers.optimization.get_cosine_schedule_with_warmup's lr_lambda
"""
import math

import numpy as np
import torch


def get_decay(optimization_step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0,
              power=2 / 3):
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        value = 1 - (1 + step / inv_gamma) ** -power
    else:
        value = (1 + step) / (10 + step)
    return max(min(value, decay), min_decay)


def ema_update(shadow: torch.Tensor, param: torch.Tensor, decay: float) -> torch.Tensor:
    """In place on ``shadow`` (fp32, any device); one_minus_decay is a Python double that meets the fp32 tensor as fp32."""
    assert shadow.dtype == torch.float32 and param.dtype == torch.float32
    one_minus_decay = 1 - decay
    shadow.sub_(one_minus_decay * (shadow - param))
    return shadow


def adam_update(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, inv_scale: float, clip: float, *,
                lr: float, beta1: float, beta2: float, eps: float):
    """One step of the library's Adam update, in place on ``p``, ``m``, ``v`` (fp32, on the host): one rounded fp32 operation
    per line in the kernel's order (adam_ema_elem), nothing fused.  The scalars are formed in double and rounded to fp32 once,
    as launch_adam_ema forms them; fp32 divide and sqrt are correctly rounded on both sides."""
    assert all(t.dtype == torch.float32 and t.device.type == "cpu" for t in (p, g, m, v))
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)          # noqa: E731
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    omb1, b2, omb2 = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2)
    step_size, bc2_sqrt, eps32 = f32(lr / bc1), f32(math.sqrt(bc2)), f32(eps)
    gi = g * f32(inv_scale)
    gi = gi * f32(clip)
    d = gi - m
    d = omb1 * d
    m.add_(d)                       # m + omb1 * (gi - m)
    t = omb2 * gi
    t = t * gi
    v.mul_(b2)
    v.add_(t)                       # v * b2 + (omb2 * gi) * gi
    denom = torch.from_numpy(np.sqrt(v.numpy()))      # numpy's fp32 sqrt is the correctly rounded one; torch.sqrt on the CPU is not
    denom = denom / bc2_sqrt
    denom = denom + eps32
    u = m / denom
    u = step_size * u
    p.sub_(u)                       # p - step_size * (m / denom)
    return p, m, v


def clip_coef_of(total_norm: np.float32, max_norm: float) -> np.float32:
    """clamp(max_norm / (total_norm + 1e-6), max=1) in fp32; max_norm <= 0 or inf: exactly 1 (no clipping asked for)."""
    if not (max_norm > 0 and math.isfinite(max_norm)):
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        coef = np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))
    assert coef.dtype == np.float32
    return np.float32(1.0) if coef > np.float32(1.0) else coef


def clip_stats(g: torch.Tensor, inv_scale: float, max_norm: float):
    """(total_norm as float64 -- exact to ~1e-13 relative --, its fp32 rounding, the coefficient from that rounding)"""
    gi = (g.detach().cpu().to(torch.float32) * torch.tensor(inv_scale, dtype=torch.float32)).double()
    norm64 = math.sqrt(float((gi * gi).sum().item()))
    with np.errstate(all="ignore"):
        norm32 = np.float32(norm64)
    return norm64, norm32, clip_coef_of(norm32, max_norm)


def cosine_lambda(num_warmup_steps, num_training_steps, num_cycles=0.5):
    def lr_lambda(current_step):
        if current_step < num_warmup_steps:
            return float(current_step) / float(max(1, num_warmup_steps))
        progress = float(current_step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))
    return lr_lambda
