"""CPU restatement of classifier guidance (Dhariwal & Nichol 2021, Alg. 2; include/sisic.h, "classifier guidance").

TEST INFRASTRUCTURE ONLY, in the style of tests/pred_ref.py: every scalar is a 0-dim torch tensor of ``dtype`` (fp32 by
default, float64 for the algebraic checks), every operation a separate torch op with one rounding, in the stated order:

    k       = scale * sb          (sb = sqrt(1 - abar_t), entry 0 of the step's row)
    eps_hat = eps - k * g         (k * g, then the subtraction)

and the step rule (tests/pred_ref.py at ``prediction_type="epsilon"``, which is tests/ddim_ref.py, tests/dpmpp_ref.py and
oracle/ddpm.py bit for bit) is applied to ``eps_hat``.  g = d log(softmax(clf(x_t))[c_b] + 1e-8) / d x_t.

With x0 clipping off every rule is affine in eps, so ``x_prev(guided) - x_prev(plain) = kappa * g`` with (``kappa_over_k``)

    DDPM               kappa / k = c0 * sb / sa
    DDIM               kappa / k = c_prev * sb / sa - c_dir
    DPM-Solver++(2M)   kappa / k = k0 * sb / sa                     (either order: the history is the same in both runs)

all positive on the cosine schedule: a guided step moves x_prev along +g, up the classifier's log-probability.

The pins of tests/test_clf_guide_cpu.py and the direction case of tests/test_gpu_clf_guide.py share ``DIRECTION_*`` below.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

import pred_ref

# the direction check: T = 6 on the "leading" grid, step index 2 (t = 498, sb = 0.7104): a mid-grid timestep, and a scale
# that puts scale * sb at 0.5
DIRECTION_T = 6
DIRECTION_STEP = 2
DIRECTION_SCALE = 0.7
DIRECTION_COSINE = 1.0 - 1e-6
# (name, scheduler rule, its options) of the five step rules the loop runs
RULES = (("ddpm", "ddpm", {}), ("ddim-eta0", "ddim", {"eta": 0.0}), ("ddim-eta1", "ddim", {"eta": 1.0}),
         ("dpmpp-order1", "dpmsolver++", {"solver_order": 1}), ("dpmpp-order2", "dpmsolver++", {"solver_order": 2}))


def guide_k(sb: float, scale: float, dtype=torch.float32) -> torch.Tensor:
    return torch.tensor(float(scale), dtype=dtype) * torch.tensor(float(sb), dtype=dtype)


def combine(eps: torch.Tensor, g: torch.Tensor, sb: float, scale: float, dtype=torch.float32) -> torch.Tensor:
    """eps_hat: k = scale * sb, t = k * g, eps - t"""
    t = guide_k(sb, scale, dtype) * g
    return eps - t


def combine_np(eps: np.ndarray, g: np.ndarray, sb: float, scale: float) -> np.ndarray:
    """the same three fp32 operations in numpy"""
    k = np.float32(scale) * np.float32(sb)
    t = (k * g.astype(np.float32)).astype(np.float32)
    return (eps.astype(np.float32) - t).astype(np.float32)


def guided_step(rule: str, eps, g, scale: float, x, z: Optional[torch.Tensor], hist: Optional[torch.Tensor], row, clip: float,
                use_clipped_model_output: bool = False, dtype=torch.float32):
    """one step of ``rule`` ("ddpm", "ddim", "dpmsolver++") on eps_hat; returns (prev_sample, hist or None)"""
    return pred_ref.step_row(rule, combine(eps, g, float(row[0]), scale, dtype), x, z, hist, row, clip, "epsilon",
                             use_clipped_model_output, dtype)


def kappa_over_k(rule: str, row) -> float:
    """(x_prev(guided) - x_prev(plain)) / (k * g) with clipping off, in float64 from the rule's row"""
    r = [float(v) for v in row]
    if rule == "ddpm":
        return r[2] * r[0] / r[1]
    if rule == "ddim":
        return r[2] * r[0] / r[1] - r[3]
    return r[3] * r[0] / r[1]


def mean_shift_factor(row) -> float:
    """Under the ancestral (DDPM) rule the score form above shifts the mean by kappa * g = scale * (c0 * sb^2 / sa) * g, where
    Alg. 1 of the paper shifts it by scale * Sigma * g with Sigma = sigma^2 (the step's variance).  Their per-step factor,
    (c0 * sb^2 / sa) / sigma^2: the two agree to first order in beta_t and differ by this factor on a coarse grid."""
    sb, sa, c0, _, sigma = [float(v) for v in row[:5]]
    return (c0 * sb * sb / sa) / (sigma * sigma)


def cosine(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm()))


def direction_row(name: str):
    """(scheduler rule, the row of DIRECTION_STEP as a list of floats) for an entry of RULES, from the package's scheduler
    mirrors (host tables: no GPU)"""
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    rule, opt = next((r, o) for n, r, o in RULES if n == name)
    if rule == "ddpm":
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        s.set_timesteps(DIRECTION_T)
        tab = s.coefficient_table()
    elif rule == "ddim":
        s = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        s.set_timesteps(DIRECTION_T)
        tab = s.coefficient_table(opt["eta"])
    else:
        s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                           timestep_spacing="leading", solver_order=opt["solver_order"])
        s.set_timesteps(DIRECTION_T)
        tab = s.coefficient_table()
    return rule, [float(v) for v in tab[DIRECTION_STEP]]
