"""HipDDPMScheduler -- drop-in for the ``diffusers.DDPMScheduler`` the reference steps with.

Call surface mirrored:

    DDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")   model_manager.py:199-202
    DDPMScheduler(..., beta_schedule="linear", beta_start=1e-4, beta_end=0.02)    diffusion_generator.py:123-128
    scheduler.set_timesteps(steps)                                                model_manager.py:209
    for t in scheduler.timesteps: ...                                             image_generator.py:395
    latents = scheduler.step(noise_pred, t, latents).prev_sample                  image_generator.py:403

The beta / alphas_cumprod tables, the integer timestep grid and the per-step scalars
are host data built with the same fp32 torch operations the published algorithm uses
(SURVEY.md Appendix B); the elementwise update itself runs in the fused HIP kernel
``sisic_ddpm_step``.

``HipDDIMScheduler`` mirrors ``diffusers.DDIMScheduler`` the same way (the reference itself holds no DDIM code: the swap
is described in INTEGRATION.md); its update runs in ``sisic_ddim_step``.  ``HipDPMSolverMultistepScheduler`` mirrors
``diffusers.DPMSolverMultistepScheduler`` (DPM-Solver++(2M) and its SDE variant); its update, with the one-step history the
rule needs, runs in ``sisic_dpmpp_step``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib, ops


@dataclass
class DDPMSchedulerOutput:
    """Mirror of ``diffusers.schedulers.scheduling_ddpm.DDPMSchedulerOutput``."""
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


def _betas_for_alpha_bar(n: int, max_beta: float = 0.999) -> torch.Tensor:
    def alpha_bar(t):
        return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
    return torch.tensor([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)],
                        dtype=torch.float32)


def check_thresholding(thresholding, dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0):
    """the three published thresholding arguments as the ``threshold`` of the step wrappers: None (off), or a checked
    ``(ratio, sample_max_value)``; ValueError for a ratio outside (0, 1] or a maximum below 1 -- before anything touches the GPU.
    The published classes hand ratio 0 to torch.quantile; here it is refused with the rest, because ratio 0 is how the library
    spells "off"."""
    if not thresholding:
        return None
    ratio, max_value = ops.check_threshold((dynamic_thresholding_ratio, sample_max_value))
    if ratio == 0.0:
        raise ValueError("dynamic_thresholding_ratio 0 with thresholding=True: the library reads ratio 0 as 'off'")
    return ratio, max_value


_THRESHOLD_ARGS = {"thresholding", "dynamic_thresholding_ratio", "sample_max_value"}
_THRESHOLD_HINT = " (dynamic thresholding: call set_thresholding() on the scheduler)"


def _timestep_grid(spacing: str, n_train: int, T: int, steps_offset: int) -> np.ndarray:
    """the T descending int64 timesteps of a run under one of the three published spacings"""
    if spacing == "linspace":                                    # from t = n_train - 1
        return np.linspace(0, n_train - 1, T + 1).round()[::-1][:-1].copy().astype(np.int64)
    if spacing == "leading":                                     # the integer ratio: ends at t = steps_offset
        ts = (np.arange(0, T) * (n_train // T)).round()[::-1].copy().astype(np.int64)
        ts += steps_offset
        return ts
    return np.round(np.arange(n_train, 0, -n_train / T)).astype(np.int64) - 1      # "trailing": the float ratio, no offset


class _HipScheduler:
    """What the three mirrors share: the forward process (beta tables, ``add_noise``, ``get_velocity``), which does not depend
    on the sampling rule, the timestep grids, thresholding, and the host side of ``step`` around the one ``ops.*_step`` call.
    A mirror adds its constructor (signature, refusals, ``config`` fields), its rows and that call."""
    order = 1
    rule: str                   # a name of _lib.RULES: the step rule ``run_sampling_loop`` runs this scheduler's table under
    _published: str             # the diffusers class it mirrors, as messages name it
    _output: type               # the dataclass ``step`` returns
    _takes_eta = False          # ``coefficient_table`` and ``step`` take eta and use_clipped_model_output
    _takes_solver_options = False       # the constructor takes solver_order and algorithm_type

    def _begin(self, unsupported: dict, prediction_type: str, thresholding=(False, 0.995, 1.0)) -> None:
        """the refusals every constructor starts with, and ``threshold``"""
        if unsupported:
            raise NotImplementedError(f"unsupported {self._published} arguments: {sorted(unsupported)}"
                                      + _THRESHOLD_HINT * bool(_THRESHOLD_ARGS & set(unsupported)))
        self.threshold = check_thresholding(*thresholding)
        if prediction_type != "epsilon":
            raise NotImplementedError("only prediction_type='epsilon' (what the reference trains and samples with)")

    def _setup(self, config: SimpleNamespace) -> None:
        """``config`` (the constructor's arguments, so that ``cls(**vars(config))`` builds the scheduler again) and the tables"""
        n = config.num_train_timesteps
        if config.beta_schedule == "linear":
            self.betas = torch.linspace(config.beta_start, config.beta_end, n, dtype=torch.float32)
        elif config.beta_schedule == "squaredcos_cap_v2":
            self.betas = _betas_for_alpha_bar(n)
        else:
            raise NotImplementedError(f"beta_schedule '{config.beta_schedule}' is not used by the reference")
        self.config = config
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps: Optional[int] = None
        self.timesteps = torch.from_numpy(np.arange(0, n)[::-1].copy())

    def set_thresholding(self, thresholding: bool = True, dynamic_thresholding_ratio: float = 0.995,
                         sample_max_value: float = 1.0) -> None:
        """Dynamic thresholding of x0 (Saharia et al. 2022) for this scheduler's ``step`` and for ``run_sampling_loop``: the
        published ``thresholding``, ``dynamic_thresholding_ratio`` and ``sample_max_value``, kept in ``self.threshold`` as (ratio, max)
        or None (and in ``config`` where the constructor takes them).  It takes
        precedence over ``clip_sample``.  ``HipDDPMScheduler`` also takes the three in its constructor; the constructors of the
        DDIM and DPM-Solver++ mirrors keep refusing them, as they always have, and this method is their way in.  ValueError for a
        ratio outside (0, 1] or a maximum below 1."""
        self.threshold = check_thresholding(thresholding, dynamic_thresholding_ratio, sample_max_value)
        # (config holds what the constructor takes, so that cls(**vars(config)) builds the scheduler again: the DDPM mirror's does)
        if hasattr(self.config, "thresholding"):
            self.config.thresholding = bool(thresholding)
            self.config.dynamic_thresholding_ratio = dynamic_thresholding_ratio
            self.config.sample_max_value = sample_max_value

    def __len__(self) -> int:
        return self.config.num_train_timesteps

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        n_train = self.config.num_train_timesteps
        if num_inference_steps > n_train:
            raise ValueError(f"num_inference_steps {num_inference_steps} > num_train_timesteps {n_train}")
        if num_inference_steps < 1:
            raise ValueError("num_inference_steps must be >= 1")
        self.num_inference_steps = num_inference_steps
        # kept on the host: the loop only needs int(t); device= is accepted for API compatibility
        self.timesteps = torch.from_numpy(_timestep_grid(self.config.timestep_spacing, n_train, num_inference_steps,
                                                         self.config.steps_offset))

    def rule_table(self, eta: float = 0.0, use_clipped_model_output: bool = False):
        """``(rule, table, flags)`` for the library's loops: this scheduler's record of ``_lib.RULES``, its host [T, row width]
        fp32 coefficient table over ``timesteps`` (under ``eta`` where the rule has one) and its SISIC_RULE_FLAG_* bits.  Sigma
        is column 4 under every rule."""
        rule = _lib.RULES[self.rule]
        table = self.coefficient_table(eta) if self._takes_eta else self.coefficient_table()
        return rule, table.contiguous(), rule.clipped_output_flag if use_clipped_model_output else 0

    def _draw(self, noisy: bool, model_output: torch.Tensor, device, generator, variance_noise) -> Optional[torch.Tensor]:
        """z of a ``step``, or None on a step that adds no noise: ``variance_noise`` if given, else ``torch.randn`` with
        ``generator`` where the generator lives"""
        if not noisy:
            return None
        if variance_noise is not None:
            return variance_noise.to(device=device, dtype=torch.float32).contiguous()
        if generator is not None and generator.device.type == "cpu":
            return torch.randn(model_output.shape, generator=generator, dtype=torch.float32).to(device)
        return torch.randn(model_output.shape, generator=generator, device=device, dtype=torch.float32)

    def _on_gpu(self, model_output: torch.Tensor) -> None:
        if model_output.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}.step runs on MI355X tensors only (no CPU path)")

    def _clip(self) -> float:
        return self.config.clip_sample_range if self.config.clip_sample else 0.0

    def _result(self, prev: torch.Tensor, return_dict: bool):
        return self._output(prev_sample=prev) if return_dict else (prev,)

    def add_noise_coefficients(self, timesteps: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(alphas_cumprod[t] ** 0.5, (1 - alphas_cumprod[t]) ** 0.5) as fp32 host rows, the scalars of ``add_noise``."""
        t = torch.as_tensor(timesteps).detach().to("cpu").to(torch.int64).reshape(-1)
        acp = self.alphas_cumprod[t]
        return (acp ** 0.5).contiguous(), ((1 - acp) ** 0.5).contiguous()

    @staticmethod
    def _fp32_pair(lead: torch.Tensor, other: torch.Tensor, what: str):
        if lead.device.type != "cuda":
            raise RuntimeError(f"{what} runs on MI355X tensors only (no CPU path)")
        lead = lead.to(torch.float32).contiguous()
        return lead, other.to(device=lead.device, dtype=torch.float32).contiguous()

    @torch.no_grad()
    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """``DDPMScheduler.add_noise`` (diffusion/train_diffusion.py:217):
        noisy = sqrt(abar_t) * x0 + sqrt(1 - abar_t) * noise with one timestep per sample, on the GPU (sisic_add_noise)."""
        x0, nz = self._fp32_pair(original_samples, noise, "HipDDPMScheduler.add_noise")
        a, c = self.add_noise_coefficients(timesteps)
        return ops.add_noise(x0, nz, a, c)

    @torch.no_grad()
    def get_velocity(self, sample: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """``DDPMScheduler.get_velocity``: v = sqrt(abar_t) * noise - sqrt(1 - abar_t) * sample, the regression target of a
        v-prediction model, on the GPU.  It is sisic_add_noise with (x0 := noise, noise := sample, a = sqrt(abar),
        c = -sqrt(1 - abar)): a sum with a negated product rounds exactly as the difference does, so the result equals the
        torch formula bit for bit -- and the target the fused training step forms in its loss kernel."""
        x, nz = self._fp32_pair(sample, noise, "get_velocity")
        a, c = self.add_noise_coefficients(timesteps)
        return ops.add_noise(nz, x, a, -c)


class _StridedScheduler(_HipScheduler):
    """The DDPM and DDIM mirrors: a step goes from t to ``t - num_train_timesteps // num_inference_steps`` (both spacings), and
    past t = 0 to ``_abar_end``."""

    def previous_timestep(self, timestep: int) -> int:
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return int(timestep) - self.config.num_train_timesteps // n

    def abar_prev(self, i: int, abar: Optional[np.ndarray] = None) -> float:
        """abar (float64) at the level grid entry i of ``timesteps`` steps to, as the rule's own row of that entry has it;
        ``abar``: ``_abar64(self)``, for a caller that asks about many entries"""
        abar = _abar64(self) if abar is None else abar
        prev_t = self.previous_timestep(int(self.timesteps[i]))
        return float(abar[prev_t]) if prev_t >= 0 else self._abar_end(abar)

    def _abar_end(self, abar: np.ndarray) -> float:
        return 1.0


class HipDDPMScheduler(_StridedScheduler):
    rule = "ddpm"
    _published = "DDPMScheduler"
    _output = DDPMSchedulerOutput

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", variance_type: str = "fixed_small", clip_sample: bool = True,
                 prediction_type: str = "epsilon", clip_sample_range: float = 1.0,
                 timestep_spacing: str = "leading", steps_offset: int = 0, thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0, **unsupported):
        self._begin(unsupported, prediction_type, (thresholding, dynamic_thresholding_ratio, sample_max_value))
        if variance_type != "fixed_small":
            raise NotImplementedError("only variance_type='fixed_small' (the diffusers default the reference uses)")
        if timestep_spacing != "leading":
            raise NotImplementedError("only timestep_spacing='leading' (the diffusers default the reference uses)")
        self._setup(SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start,
                                    beta_end=beta_end, beta_schedule=beta_schedule, variance_type=variance_type,
                                    clip_sample=clip_sample, prediction_type=prediction_type,
                                    clip_sample_range=clip_sample_range, timestep_spacing=timestep_spacing,
                                    steps_offset=steps_offset, thresholding=thresholding,
                                    dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                                    sample_max_value=sample_max_value))
        self.one = torch.tensor(1.0)

    def step_coefficients(self, timestep) -> Tuple[float, float, float, float, float]:
        """(sqrt(1-abar_t), sqrt(abar_t), c0, c1, sigma) as fp32 values, sigma = 0 at t == 0."""
        t = int(timestep)
        prev_t = self.previous_timestep(t)
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        current_alpha_t = alpha_prod_t / alpha_prod_t_prev
        current_beta_t = 1 - current_alpha_t
        c0 = (alpha_prod_t_prev ** (0.5) * current_beta_t) / beta_prod_t
        c1 = current_alpha_t ** (0.5) * beta_prod_t_prev / beta_prod_t
        sigma = 0.0
        if t > 0:
            variance = (1 - alpha_prod_t_prev) / (1 - alpha_prod_t) * current_beta_t
            variance = torch.clamp(variance, min=1e-20)
            sigma = float(variance ** 0.5)
        return (float(beta_prod_t ** (0.5)), float(alpha_prod_t ** (0.5)), float(c0), float(c1), sigma)

    def coefficient_table(self) -> torch.Tensor:
        """[T,5] fp32 host table for ``sisic_sample``."""
        return torch.tensor([self.step_coefficients(t) for t in self.timesteps], dtype=torch.float32)

    @torch.no_grad()
    def step(self, model_output: torch.Tensor, timestep: Union[int, torch.Tensor], sample: torch.Tensor,
             generator: Optional[torch.Generator] = None, return_dict: bool = True,
             variance_noise: Optional[torch.Tensor] = None, prediction_type: str = "epsilon"):
        """prev_sample = DDPM ancestral update on the GPU.  Noise: ``variance_noise`` if given, else
        ``torch.randn`` on the sample's device with ``generator`` (the reference passes none).  ``prediction_type``: what
        ``model_output`` holds -- "epsilon", "sample" or "v_prediction".  It is the MODEL's property (``HipUNet2DModel
        (prediction_type=)``), so it travels with the call (``model.prediction_type``), not with the scheduler's constructor."""
        self._on_gpu(model_output)
        coef = self.step_coefficients(timestep)
        z = self._draw(int(timestep) > 0, model_output, sample.device, generator, variance_noise)
        prev = ops.ddpm_step(model_output.to(torch.float32).contiguous(), sample.to(torch.float32).contiguous(), z,
                             coef, self._clip(), prediction_type=prediction_type, threshold=self.threshold)
        return self._result(prev, return_dict)


@dataclass
class DDIMSchedulerOutput:
    """Mirror of ``diffusers.schedulers.scheduling_ddim.DDIMSchedulerOutput`` (``pred_original_sample`` is not produced)."""
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


class HipDDIMScheduler(_StridedScheduler):
    """Drop-in for ``diffusers.DDIMScheduler`` with epsilon prediction: the same beta / alphas_cumprod tables, x_T and UNet as
    the DDPM mirror, the step rule that was designed for 20 to 100 steps.  Deterministic at ``eta = 0``; at ``eta = 1`` its
    sigma is the DDPM rule's.

        sched = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        sched.set_timesteps(50)
        for t in sched.timesteps:
            latents = sched.step(model(latents, t).sample, t, latents, eta=0.0).prev_sample
    """
    rule = "ddim"
    _published = "DDIMScheduler"
    _output = DDIMSchedulerOutput
    _takes_eta = True

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", clip_sample: bool = True, set_alpha_to_one: bool = True,
                 steps_offset: int = 0, prediction_type: str = "epsilon", clip_sample_range: float = 1.0,
                 timestep_spacing: str = "leading", **unsupported):
        self._begin(unsupported, prediction_type)
        if timestep_spacing not in ("leading", "trailing"):
            raise NotImplementedError("only timestep_spacing='leading' (the diffusers default) or 'trailing'")
        self._setup(SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                    beta_schedule=beta_schedule, clip_sample=clip_sample,
                                    set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset,
                                    prediction_type=prediction_type, clip_sample_range=clip_sample_range,
                                    timestep_spacing=timestep_spacing))
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]

    def _abar_end(self, abar: np.ndarray) -> float:              # 1, or alphas_cumprod[0] (set_alpha_to_one=False)
        return 1.0 if float(self.final_alpha_cumprod) == 1.0 else float(abar[0])

    def step_coefficients(self, timestep, eta: float = 0.0) -> Tuple[float, float, float, float, float]:
        """(sqrt(1-abar_t), sqrt(abar_t), sqrt(abar_prev), sqrt(1 - abar_prev - sigma^2), sigma) as fp32 values,
        sigma = eta * variance ** 0.5: the table row of ``sisic_ddim_step``."""
        t = int(timestep)
        prev_t = self.previous_timestep(t)
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        variance = (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)
        std_dev_t = float(eta) * variance ** (0.5)
        c_dir = (1 - alpha_prod_t_prev - std_dev_t ** 2) ** (0.5)
        return (float(beta_prod_t ** (0.5)), float(alpha_prod_t ** (0.5)), float(alpha_prod_t_prev ** (0.5)), float(c_dir),
                float(std_dev_t))

    def coefficient_table(self, eta: float = 0.0) -> torch.Tensor:
        """[T,5] fp32 host table for ``sisic_sample_frames_rule`` under SISIC_RULE_DDIM."""
        return torch.tensor([self.step_coefficients(t, eta) for t in self.timesteps], dtype=torch.float32)

    @torch.no_grad()
    def step(self, model_output: torch.Tensor, timestep: Union[int, torch.Tensor], sample: torch.Tensor, eta: float = 0.0,
             use_clipped_model_output: bool = False, generator: Optional[torch.Generator] = None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True, prediction_type: str = "epsilon"):
        """prev_sample = DDIM update on the GPU (``prediction_type``: as in ``HipDDPMScheduler.step``).
        Noise, on the steps with sigma != 0 only: ``variance_noise`` if given, else
        ``torch.randn`` on the sample's device with ``generator``.  (diffusers also draws on a step whose sigma is 0 at
        eta > 0, and multiplies the draw by 0: a generator shared with it is one draw further on after such a step.)"""
        self._on_gpu(model_output)
        coef = self.step_coefficients(timestep, eta)
        z = self._draw(coef[4] != 0.0, model_output, sample.device, generator, variance_noise)
        prev = ops.ddim_step(model_output.to(torch.float32).contiguous(), sample.to(torch.float32).contiguous(), z, coef,
                             self._clip(), use_clipped_model_output, prediction_type=prediction_type, threshold=self.threshold)
        return self._result(prev, return_dict)


DPMPP_ALGORITHMS = ("dpmsolver++", "sde-dpmsolver++")


def check_dpmpp_options(solver_order: int, algorithm_type: str) -> None:
    """the refusals of the DPM-Solver++ mirror that ``generate`` repeats before it touches the GPU"""
    if algorithm_type not in DPMPP_ALGORITHMS:
        raise NotImplementedError(f"algorithm_type must be one of {DPMPP_ALGORITHMS}, got {algorithm_type!r}")
    if solver_order not in (1, 2):
        raise NotImplementedError(f"solver_order must be 1 or 2 (the third-order multistep form is out of scope), got "
                                  f"{solver_order!r}")


def dpmpp_coefficient_rows(abar, solver_order: int = 2, algorithm_type: str = "dpmsolver++") -> np.ndarray:
    """float64 [T,6] rows {sigma_i, alpha_i, cx, k0, sigma, k1} of DPM-Solver++(2M) (Lu et al. 2022, midpoint rule) for a run
    over ``abar`` = alphas_cumprod at its T timesteps, ending at abar = 1 (sigma = 0: the last step returns its x0).

    Everything is float64 with ``expm1``: A = -alpha' * (exp(-h) - 1), and at the small h of a long run exp(-h) - 1 loses in
    fp32 as many digits as h has leading zeros -- at T = 1000 (h of 3e-3 and up) the coefficients would be good to about 2e-5
    relative, where the step kernel itself rounds at 6e-8.  The rows are rounded to fp32 once, by the caller."""
    check_dpmpp_options(solver_order, algorithm_type)
    abar = np.asarray(abar, dtype=np.float64)
    T = abar.shape[0]
    full = np.concatenate([abar, [1.0]])
    alpha, sig = np.sqrt(full), np.sqrt(1.0 - full)
    lam = np.full(T + 1, np.inf)
    lam[:T] = np.log(alpha[:T]) - np.log(sig[:T])
    sde = algorithm_type == "sde-dpmsolver++"
    rows = np.zeros((T, 6), dtype=np.float64)
    for i in range(T):
        h = lam[i + 1] - lam[i]
        if sde:
            cx = (sig[i + 1] / sig[i]) * np.exp(-h)
            A = -alpha[i + 1] * np.expm1(-2.0 * h)
            sigma = sig[i + 1] * np.sqrt(-np.expm1(-2.0 * h))
        else:
            cx = sig[i + 1] / sig[i]
            A = -alpha[i + 1] * np.expm1(-h)
            sigma = 0.0
        k0, k1 = A, 0.0
        if solver_order == 2 and 0 < i < T - 1:                      # first step: no history; last step: h is infinite
            r = (lam[i] - lam[i - 1]) / h
            k0, k1 = A * (1.0 + 1.0 / (2.0 * r)), -A / (2.0 * r)
        rows[i] = (sig[i], alpha[i], cx, k0, sigma, k1)
    return rows


@dataclass
class DPMSolverSchedulerOutput:
    """Mirror of diffusers' ``SchedulerOutput``."""
    prev_sample: torch.Tensor


class HipDPMSolverMultistepScheduler(_HipScheduler):
    """Drop-in for ``diffusers.DPMSolverMultistepScheduler`` with epsilon prediction: DPM-Solver++(2M), the second-order
    multistep solver (``solver_type="midpoint"``, ``final_sigmas_type="zero"``), and its stochastic variant
    ``algorithm_type="sde-dpmsolver++"``.  One UNet call per step like DDIM, which it equals at ``solver_order=1``.

        sched = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        sched.set_timesteps(20)
        for t in sched.timesteps:
            latents = sched.step(model(latents, t).sample, t, latents).prev_sample

    ``step`` is stateful: the object keeps the previous step's predicted x0 and the step index, and ``set_timesteps`` resets
    both.  ``timestep_spacing``: "linspace" (the published default, from t = N - 1), "trailing", or "leading" -- the grid of
    the project's DDPM and DDIM mirrors, so that the three rules can run on one grid.  ``clip_sample`` /
    ``clip_sample_range`` are extensions of this project: the static clamp of x0 the other two mirrors apply, off by
    default.  The published class's ``thresholding`` is offered through ``set_thresholding`` (the constructor keeps
    refusing the argument, as it always has); under it ``clip_sample`` is not read."""
    rule = "dpmsolver++"
    _published = "DPMSolverMultistepScheduler"
    _output = DPMSolverSchedulerOutput
    _takes_solver_options = True

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", solver_order: int = 2, prediction_type: str = "epsilon",
                 algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint", lower_order_final: bool = True,
                 final_sigmas_type: str = "zero", timestep_spacing: str = "linspace", steps_offset: int = 0,
                 clip_sample: bool = False, clip_sample_range: float = 1.0, **unsupported):
        self._begin(unsupported, prediction_type)
        check_dpmpp_options(solver_order, algorithm_type)
        if solver_type != "midpoint":
            raise NotImplementedError("only solver_type='midpoint' (the published default)")
        if final_sigmas_type != "zero":
            raise NotImplementedError("only final_sigmas_type='zero': the run ends at sigma = 0 and returns its x0")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise NotImplementedError("timestep_spacing must be 'linspace' (the published default), 'leading' or 'trailing'")
        # lower_order_final has no effect: with final_sigmas_type='zero' the last step is first order whatever it says
        self._setup(SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                    beta_schedule=beta_schedule, solver_order=solver_order,
                                    prediction_type=prediction_type, algorithm_type=algorithm_type,
                                    solver_type=solver_type, lower_order_final=lower_order_final,
                                    final_sigmas_type=final_sigmas_type, timestep_spacing=timestep_spacing,
                                    steps_offset=steps_offset, clip_sample=clip_sample,
                                    clip_sample_range=clip_sample_range))
        self._reset()

    def _reset(self) -> None:
        self._hist: Optional[torch.Tensor] = None     # the previous step's x0 (device), None before the first step
        self._step_index: Optional[int] = None
        self._tables = None

    @property
    def step_index(self) -> Optional[int]:
        return self._step_index

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        super().set_timesteps(num_inference_steps, device)
        self._reset()

    def abar_prev(self, i: int, abar: Optional[np.ndarray] = None) -> float:
        """abar (float64) at the level grid entry i of ``timesteps`` steps to: the next grid point; the run ends at abar = 1"""
        abar = _abar64(self) if abar is None else abar
        return float(abar[int(self.timesteps[i + 1])]) if i + 1 < self.timesteps.numel() else 1.0

    def _rows(self, solver_order: int) -> torch.Tensor:
        abar = self.alphas_cumprod[self.timesteps.to(torch.int64)].numpy().astype(np.float64)
        return torch.from_numpy(dpmpp_coefficient_rows(abar, solver_order, self.config.algorithm_type).astype(np.float32))

    def coefficient_table(self) -> torch.Tensor:
        """[T,6] fp32 host table {sigma_t, alpha_t, cx, k0, sigma, k1} for ``sisic_sample_frames_rule`` under
        SISIC_RULE_DPMPP: float64 arithmetic (``dpmpp_coefficient_rows``), rounded to fp32 here."""
        return self._rows(self.config.solver_order)

    @torch.no_grad()
    def step(self, model_output: torch.Tensor, timestep: Union[int, torch.Tensor], sample: torch.Tensor,
             generator: Optional[torch.Generator] = None, variance_noise: Optional[torch.Tensor] = None,
             return_dict: bool = True, prediction_type: str = "epsilon"):
        """prev_sample = DPM-Solver++ update on the GPU (``prediction_type``: as in ``HipDDPMScheduler.step``).
        The first call after ``set_timesteps`` finds its place in
        ``timesteps`` by ``timestep`` and is first order (there is no history yet); every call then moves one step on.
        Noise, on the steps with sigma != 0 only (the SDE variant, all but the last): ``variance_noise`` if given, else
        ``torch.randn`` with ``generator``."""
        self._on_gpu(model_output)
        if self._tables is None:
            self._tables = (self._rows(1), self._rows(self.config.solver_order))
        if self._step_index is None:
            at = (self.timesteps == int(timestep)).nonzero()
            if at.numel() == 0:
                raise ValueError(f"timestep {int(timestep)} is not one of this run's timesteps")
            self._step_index = int(at[0])
        i = self._step_index
        if i >= self.timesteps.numel():
            raise RuntimeError("step called past the last timestep; call set_timesteps to start another run")
        x = sample.to(torch.float32).contiguous()
        fresh = self._hist is None or self._hist.shape != x.shape or self._hist.device != x.device
        if fresh:
            self._hist = ops.empty_like(x)
        coef = tuple(float(v) for v in self._tables[0 if fresh else 1][i])
        z = self._draw(coef[4] != 0.0, model_output, x.device, generator, variance_noise)
        prev = ops.dpmpp_step(model_output.to(torch.float32).contiguous(), x, z, self._hist, coef, self._clip(),
                              prediction_type=prediction_type, threshold=self.threshold)
        self._step_index = i + 1
        return self._result(prev, return_dict)


MIRRORS = {cls.rule: cls for cls in (HipDDPMScheduler, HipDDIMScheduler, HipDPMSolverMultistepScheduler)}


# ---- image editing: the RePaint schedule and the rows of the edit epilogue ------------------------------------------------
def resample_schedule(T: int, jump_length: int = 10, n_resample: int = 1) -> List[Tuple[int, int]]:
    """RePaint's resampling schedule (Lugmayr et al. 2022, Algorithm 1 with its ``get_schedule_jump``) over a T-step grid:
    one ``(index into the grid, jump)`` per UNet pass.  In terms of the level L, the number of reverse steps still to go: the
    run goes down from L = T, and the first ``n_resample - 1`` times it reaches a level in ``range(0, T - jump_length,
    jump_length)`` it jumps ``jump_length`` levels back up and comes down again.  ``jump`` is the height of the jump taken
    AFTER the pass (0: none).  ``n_resample == 1`` is the plain grid.  The length is
    ``T + (n_resample - 1) * jump_length * len(range(0, T - jump_length, jump_length))``."""
    T, jump_length, n_resample = int(T), int(jump_length), int(n_resample)
    if T < 1:
        raise ValueError(f"T must be positive, got {T}")
    if jump_length < 1:
        raise ValueError(f"jump_length must be positive, got {jump_length}")
    if n_resample < 1:
        raise ValueError(f"n_resample must be positive, got {n_resample}")
    left = {L: n_resample - 1 for L in range(0, T - jump_length, jump_length)} if n_resample > 1 else {}
    out: List[Tuple[int, int]] = []
    L = T
    while L > 0:
        i = T - L
        L -= 1
        jump = 0
        if left.get(L, 0) > 0:
            left[L] -= 1
            jump = jump_length
            L += jump_length
        out.append((i, jump))
    return out


def _abar64(scheduler) -> np.ndarray:
    """alphas_cumprod in float64: the cumulative product of the scheduler's fp32 ``alphas``, so that a ratio of two entries is
    the product of the alphas between them to float64 precision (the fp32 table loses that at 6e-8 per entry)"""
    return np.cumprod(scheduler.alphas.numpy().astype(np.float64))


def edit_rows(scheduler, schedule) -> torch.Tensor:
    """[len(schedule), 4] fp32 rows ``{ck, sk, ja, jb}`` of the edit epilogue (``sisic_sample_frames_edit``) for a schedule of
    ``(grid index, jump)`` entries over ``scheduler.timesteps``:

    * ``ck = abar_prev ** 0.5``, ``sk = (1 - abar_prev) ** 0.5`` with abar_prev the level the entry's own rule row steps to
      (1 at the last level: ``ck = 1, sk = 0``): the known image at the noise level of the step's result;
    * a jump of j levels: the next pass runs at grid entry ``i + 1 - j``, at ``abar_target``; with ``ratio = abar_target /
      abar_prev``, ``ja = ratio ** 0.5`` and ``jb = (1 - ratio) ** 0.5`` -- the j forward steps of the paper composed into
      one Gaussian draw, which has the same distribution; no jump: ``ja = 1, jb = 0``.

    Everything in float64 over the float64 cumulative product of ``scheduler.alphas``, rounded to fp32 once."""
    rows = edit_rows64(scheduler, schedule)
    return torch.from_numpy(rows.astype(np.float32))


def edit_rows64(scheduler, schedule) -> np.ndarray:
    """``edit_rows`` before the rounding to fp32"""
    abar = _abar64(scheduler)
    n = int(scheduler.timesteps.numel())
    rows = np.zeros((len(schedule), 4), dtype=np.float64)
    for p, (i, jump) in enumerate(schedule):
        i, jump = int(i), int(jump)
        if not 0 <= i < n:
            raise ValueError(f"schedule entry {p}: grid index {i} is outside 0..{n - 1}")
        prev = scheduler.abar_prev(i, abar)
        ja, jb = 1.0, 0.0
        if jump:
            target = i + 1 - jump
            if jump < 0 or not 0 <= target < n:
                raise ValueError(f"schedule entry {p}: a jump of {jump} from grid index {i} leaves the grid")
            ratio = float(abar[int(scheduler.timesteps[target])]) / prev
            if not 0.0 < ratio <= 1.0:
                raise ValueError(f"schedule entry {p}: a jump of {jump} from grid index {i} does not go up the schedule")
            ja, jb = math.sqrt(ratio), math.sqrt(1.0 - ratio)
        rows[p] = (math.sqrt(prev), math.sqrt(max(0.0, 1.0 - prev)), ja, jb)
    return rows
