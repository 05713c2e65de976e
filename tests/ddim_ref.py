"""CPU restatement of the published ``diffusers.DDIMScheduler`` for epsilon prediction, in the style of oracle/ddpm.py.

TEST INFRASTRUCTURE ONLY.  The reference project holds no DDIM code and diffusers is not a dependency, so this file is the
yardstick of ``HipDDIMScheduler`` and ``sisic_ddim_step``; tests/test_ddim_cpu.py pins it in turn to the DDPM oracle at
eta = 1, where the two rules describe the same distribution and differ by rounding only.

Every scalar is a 0-dim fp32 torch tensor and the operation order follows the published ``step``:

    variance = ((1 - abar_prev) / (1 - abar_t)) * (1 - abar_t / abar_prev)
    std      = eta * variance ** 0.5
    x0       = (x - (1 - abar_t) ** 0.5 * eps) / abar_t ** 0.5            [clamped to +-clip_sample_range when clip_sample]
    pe       = eps, or (x - abar_t ** 0.5 * x0) / (1 - abar_t) ** 0.5 with use_clipped_model_output
    prev     = abar_prev ** 0.5 * x0 + (1 - abar_prev - std ** 2) ** 0.5 * pe     [+ std * z where std != 0 and z is given]
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from oracle.ddpm import betas_for_alpha_bar


class DDIMSchedulerRef:
    def __init__(self, num_train_timesteps: int = 1000, beta_schedule: str = "squaredcos_cap_v2", beta_start: float = 1e-4,
                 beta_end: float = 0.02, clip_sample: bool = True, clip_sample_range: float = 1.0,
                 set_alpha_to_one: bool = True, steps_offset: int = 0, timestep_spacing: str = "leading"):
        self.num_train_timesteps = num_train_timesteps
        if beta_schedule == "linear":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "squaredcos_cap_v2":
            self.betas = betas_for_alpha_bar(num_train_timesteps)
        else:
            raise NotImplementedError(beta_schedule)
        if timestep_spacing not in ("leading", "trailing"):
            raise NotImplementedError(timestep_spacing)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.clip_sample = clip_sample
        self.clip_sample_range = clip_sample_range
        self.steps_offset = steps_offset
        self.timestep_spacing = timestep_spacing
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())

    def set_timesteps(self, num_inference_steps: int) -> None:
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        if self.timestep_spacing == "leading":
            step_ratio = self.num_train_timesteps // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
            ts += self.steps_offset
        else:
            step_ratio = self.num_train_timesteps / num_inference_steps
            ts = np.round(np.arange(self.num_train_timesteps, 0, -step_ratio)).astype(np.int64)
            ts -= 1
        self.timesteps = torch.from_numpy(ts)

    def previous_timestep(self, t: int) -> int:
        n = self.num_inference_steps if self.num_inference_steps else self.num_train_timesteps
        return t - self.num_train_timesteps // n

    def _scalars(self, timestep, eta: float):
        """(sb, sa, c_prev, radicand of c_dir, std) as 0-dim fp32 tensors"""
        t = int(timestep)
        prev_t = self.previous_timestep(t)
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        variance = (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)
        std_dev_t = eta * variance ** (0.5)
        radicand = 1 - alpha_prod_t_prev - std_dev_t ** 2
        return beta_prod_t ** (0.5), alpha_prod_t ** (0.5), alpha_prod_t_prev ** (0.5), radicand, std_dev_t

    def radicand(self, timestep, eta: float = 0.0) -> float:
        return float(self._scalars(timestep, eta)[3])

    def coefficients(self, timestep, eta: float = 0.0) -> Tuple[float, float, float, float, float]:
        """the table row (sb, sa, c_prev, c_dir, sigma) as fp32 values"""
        sb, sa, c_prev, radicand, std = self._scalars(timestep, eta)
        return float(sb), float(sa), float(c_prev), float(radicand ** (0.5)), float(std)

    def table(self, eta: float = 0.0) -> torch.Tensor:
        return torch.tensor([self.coefficients(t, eta) for t in self.timesteps], dtype=torch.float32)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, eta: float = 0.0,
             use_clipped_model_output: bool = False, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Returns ``prev_sample``.  ``noise`` is added where the step's std is not zero."""
        clip = self.clip_sample_range if self.clip_sample else 0.0
        return step_row(model_output, sample, noise, self.coefficients(timestep, eta), clip, use_clipped_model_output)


def predicted_x0(model_output: torch.Tensor, sample: torch.Tensor, row, clip: float = 1.0) -> torch.Tensor:
    sb, sa = (torch.tensor(float(v), dtype=torch.float32) for v in row[:2])
    x0 = (sample - sb * model_output) / sa
    if clip > 0:
        x0 = x0.clamp(-clip, clip)
    return x0


def step_row(model_output: torch.Tensor, sample: torch.Tensor, noise: Optional[torch.Tensor], row, clip: float = 1.0,
             use_clipped_model_output: bool = False) -> torch.Tensor:
    """The elementwise rule for one table row (sb, sa, c_prev, c_dir, sigma): separate fp32 torch operations, one rounding
    each."""
    sb, sa, c_prev, c_dir, sigma = (torch.tensor(float(v), dtype=torch.float32) for v in row)
    x0 = predicted_x0(model_output, sample, row, clip)
    pred_epsilon = model_output
    if use_clipped_model_output:
        pred_epsilon = (sample - sa * x0) / sb
    prev = c_prev * x0 + c_dir * pred_epsilon
    if float(sigma) != 0.0 and noise is not None:
        prev = prev + sigma * noise
    return prev
