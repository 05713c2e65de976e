"""CPU restatement of DPM-Solver++(2M) (Lu et al. 2022: the second-order multistep data-prediction solver, midpoint rule, as
the published ``DPMSolverMultistepScheduler`` runs it for epsilon prediction with ``final_sigmas_type="zero"``), and of its
stochastic variant ``sde-dpmsolver++``, in the style of tests/ddim_ref.py.

TEST INFRASTRUCTURE ONLY.  The reference project holds no such code and diffusers is not a dependency, so this file is the
yardstick of ``HipDPMSolverMultistepScheduler`` and ``sisic_dpmpp_step``; tests/test_dpmpp_cpu.py pins it in turn to the DDIM
restatement at solver_order = 1, to the unfolded published update, and to the exact solution of a toy problem.

Tables: numpy float64 from the fp32 alphas_cumprod the other restatements build, rounded to fp32 once per row.

    alpha = abar ** 0.5, sig = (1 - abar) ** 0.5, lam = ln alpha - ln sig          (abar = 1, lam = +inf after the last step)
    h = lam_next - lam,  r = (lam - lam_prev) / h
    ODE:  cx = sig_next / sig,              A = -alpha_next * expm1(-h),    sigma = 0
    SDE:  cx = sig_next / sig * exp(-h),    A = -alpha_next * expm1(-2 h),  sigma = sig_next * (-expm1(-2 h)) ** 0.5
    order 1 (first step, last step, solver_order = 1):  k0 = A, k1 = 0
    order 2:                                            k0 = A (1 + 1 / (2 r)), k1 = -A / (2 r)
    row = (sig, alpha, cx, k0, sigma, k1)

Elements: torch CPU fp32, one rounding per operation, in this order:

    x0   = (x - sig * eps) / alpha                       [clamped to +-clip when clip > 0]
    prev = cx * x + k0 * x0   [+ k1 * hist where k1 != 0]   [+ sigma * z where sigma != 0 and z is given]
    hist = x0
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from oracle.ddpm import betas_for_alpha_bar

ALGORITHMS = ("dpmsolver++", "sde-dpmsolver++")


def alphas_cumprod(beta_schedule: str = "squaredcos_cap_v2", n: int = 1000, beta_start: float = 1e-4,
                   beta_end: float = 0.02) -> torch.Tensor:
    if beta_schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    elif beta_schedule == "squaredcos_cap_v2":
        betas = betas_for_alpha_bar(n)
    else:
        raise NotImplementedError(beta_schedule)
    return torch.cumprod(1.0 - betas, dim=0)


def timestep_grid(T: int, spacing: str = "linspace", n_train: int = 1000, steps_offset: int = 0) -> np.ndarray:
    """the three grids as int64: "linspace" is the published default, "leading" and "trailing" are the grids of
    tests/ddim_ref.py (the DDIM restatement), so that the rules can be compared on one grid"""
    if spacing == "linspace":
        return np.linspace(0, n_train - 1, T + 1).round()[::-1][:-1].copy().astype(np.int64)
    if spacing == "leading":
        ratio = n_train // T
        return (np.arange(0, T) * ratio).round()[::-1].copy().astype(np.int64) + steps_offset
    if spacing == "trailing":
        return np.round(np.arange(n_train, 0, -n_train / T)).astype(np.int64) - 1
    raise NotImplementedError(spacing)


def _lambdas(abar: np.ndarray):
    """(alpha, sig, lam) of the run's T points and of its end point abar = 1, float64 [T + 1]"""
    full = np.concatenate([np.asarray(abar, dtype=np.float64), [1.0]])
    alpha, sig = full ** 0.5, (1.0 - full) ** 0.5
    lam = np.empty_like(full)
    lam[:-1] = np.log(alpha[:-1]) - np.log(sig[:-1])
    lam[-1] = np.inf
    return alpha, sig, lam


def step_order(i: int, T: int, solver_order: int) -> int:
    return 1 if (solver_order == 1 or i == 0 or i == T - 1) else 2


def unfolded(abar, i: int, algorithm_type: str):
    """(alpha_i, sig_i, cx, A, sigma, r) of step i in float64: the scalars of the published update
    x = cx * x + A * D0 + 0.5 * A * D1 [+ sigma * z],  D0 = m0,  D1 = (m0 - m1) / r.    r is None where no previous step exists."""
    assert algorithm_type in ALGORITHMS
    alpha, sig, lam = _lambdas(abar)
    h = lam[i + 1] - lam[i]
    if algorithm_type == "dpmsolver++":
        cx, A, sigma = sig[i + 1] / sig[i], -alpha[i + 1] * np.expm1(-h), 0.0
    else:
        cx = sig[i + 1] / sig[i] * np.exp(-h)
        A = -alpha[i + 1] * np.expm1(-2.0 * h)
        sigma = sig[i + 1] * (-np.expm1(-2.0 * h)) ** 0.5
    r = (lam[i] - lam[i - 1]) / h if i > 0 else None
    return alpha[i], sig[i], cx, A, sigma, r


def table64(abar, solver_order: int = 2, algorithm_type: str = "dpmsolver++") -> np.ndarray:
    """float64 [T,6] folded rows (sig, alpha, cx, k0, sigma, k1)"""
    T = len(abar)
    rows = np.zeros((T, 6))
    for i in range(T):
        a, s, cx, A, sigma, r = unfolded(abar, i, algorithm_type)
        if step_order(i, T, solver_order) == 1:
            k0, k1 = A, 0.0
        else:
            k0, k1 = A * (1.0 + 1.0 / (2.0 * r)), -A / (2.0 * r)
        rows[i] = (s, a, cx, k0, sigma, k1)
    return rows


def published_update64(x, m0, m1, z, abar, i: int, solver_order: int, algorithm_type: str):
    """the unfolded published form on float64 arrays: x_next from x, this step's x0 (m0), the previous step's (m1) and z"""
    _, _, cx, A, sigma, r = unfolded(abar, i, algorithm_type)
    out = cx * x + A * m0
    if step_order(i, len(abar), solver_order) == 2:
        D1 = (m0 - m1) / r
        out = out + 0.5 * A * D1
    if sigma != 0.0:
        out = out + sigma * z
    return out


class DPMSolverRef:
    """the restatement as an object: tables from the fp32 alphas_cumprod widened to float64, rows rounded to fp32"""

    def __init__(self, beta_schedule: str = "squaredcos_cap_v2", solver_order: int = 2, algorithm_type: str = "dpmsolver++",
                 timestep_spacing: str = "linspace", clip_sample: bool = False, clip_sample_range: float = 1.0,
                 num_train_timesteps: int = 1000):
        assert solver_order in (1, 2) and algorithm_type in ALGORITHMS
        self.acp = alphas_cumprod(beta_schedule, num_train_timesteps)
        self.n_train = num_train_timesteps
        self.solver_order, self.algorithm_type, self.spacing = solver_order, algorithm_type, timestep_spacing
        self.clip = clip_sample_range if clip_sample else 0.0
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())

    def set_timesteps(self, T: int) -> None:
        self.timesteps = torch.from_numpy(timestep_grid(T, self.spacing, self.n_train))

    def abar(self) -> np.ndarray:
        return self.acp[self.timesteps].numpy().astype(np.float64)

    def table(self, solver_order: Optional[int] = None) -> torch.Tensor:
        order = self.solver_order if solver_order is None else solver_order
        return torch.from_numpy(table64(self.abar(), order, self.algorithm_type).astype(np.float32))

    def chain(self, eps_fn, x_T: torch.Tensor, z: Optional[torch.Tensor] = None):
        """the whole run on the CPU: eps_fn(x, t) -> eps; z rows go to the steps with sigma != 0.  Returns every frame."""
        tab = self.table()
        x, hist, zi, frames = x_T.clone(), None, 0, []
        for i, t in enumerate(self.timesteps):
            vn = None
            if z is not None and float(tab[i, 4]) != 0.0:
                vn = z[zi]
                zi += 1
            x, hist = step_row(eps_fn(x, int(t)), x, vn, hist, tab[i], self.clip)
            frames.append(x)
        assert z is None or zi == z.shape[0]
        return frames


def predicted_x0(model_output: torch.Tensor, sample: torch.Tensor, row, clip: float = 0.0) -> torch.Tensor:
    sb, sa = (torch.tensor(float(v), dtype=torch.float32) for v in tuple(row)[:2])
    x0 = (sample - sb * model_output) / sa
    if clip > 0:
        x0 = x0.clamp(-clip, clip)
    return x0


def step_row(model_output: torch.Tensor, sample: torch.Tensor, noise: Optional[torch.Tensor], hist: Optional[torch.Tensor],
             row, clip: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The elementwise rule for one table row (sb, sa, cx, k0, sigma, k1): separate fp32 torch operations, one rounding each.
    Returns (prev_sample, this step's x0 = the next step's hist).  hist is not touched when k1 == 0 (it may be None)."""
    sb, sa, cx, k0, sigma, k1 = (torch.tensor(float(v), dtype=torch.float32) for v in row)
    x0 = predicted_x0(model_output, sample, row, clip)
    prev = cx * sample + k0 * x0
    if float(k1) != 0.0:
        prev = prev + k1 * hist
    if float(sigma) != 0.0 and noise is not None:
        prev = prev + sigma * noise
    return prev, x0
