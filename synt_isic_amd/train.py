"""The training loop of diffusion/train_diffusion.py:201-266 on the HIP kernels.

The reference's loop body, and what stands in for each object here (same names, arguments and call order, so that the loop
reads like the reference's):

    model = create_model().to(DEVICE)                               HipUNet2DModel(...).to("cuda")           :201
    scheduler = DDPMScheduler(1000, "squaredcos_cap_v2")            HipDDPMScheduler(...)                    :202
    optimizer = Adam(model.parameters(), lr=LR)                     HipAdam(model, lr=LR)                    :203
    scaler = amp.GradScaler()                                       HipGradScaler()                          :204
    model.train()                                                   model.train()                            :209
    noise = torch.randn_like(images)                                (torch RNG: plumbing)                    :215
    timesteps = torch.randint(0, TIMESTEPS, (B,), device=DEVICE)                                             :216
    noisy_images = scheduler.add_noise(images, noise, timesteps)    sisic_add_noise                          :217
    noise_pred = model(noisy_images, timesteps).sample              sisic_unet_train_forward                 :218
    loss = torch.nn.functional.mse_loss(noise_pred, noise)          mse_loss(noise_pred, noise)              :219
    optimizer.zero_grad(set_to_none=True)                           HipAdam.zero_grad                        :230
    scaler.scale(loss).backward()                                   sisic_mse_loss + sisic_unet_backward     :231
    scaler.step(optimizer); scaler.update()                         sisic_unet_optimizer_step                :232-233
    epoch_loss += loss.item()                                       HipLoss.item()                           :235

Beyond the reference, the three things diffusers' unconditional training example wraps round the same loop (all off unless
asked for; with none of them the calls above are the only ones made):

    accelerator.clip_grad_norm_(model.parameters(), 1.0)            HipAdam(..., max_grad_norm=1.0)  sisic_unet_optimizer_step_ext
    ema_model.step(model.parameters())                              HipAdam(..., ema=HipEMA(model))  (rides in the same pass)
    lr_scheduler.step()                                             HipLambdaLR(optimizer, cosine_schedule_with_warmup(...)).step()

and the regulariser of the published model itself, ``UNet2DModel(dropout=p)``: ``HipUNet2DModel(dropout=p)`` drops in every ResNet
block of the tape-recording forward (spelled-out and fused steps alike), with masks regenerated from a counter in the backward
pass (include/sisic.h, the mask contract); ``train_class(..., dropout_seed=s)`` seeds them.

The objective is a choice as well: the target follows ``model.prediction_type`` ("epsilon", "sample", "v_prediction") and
``snr_gamma`` weights every sample's loss by Min-SNR-gamma (``min_snr_weights``): ``diffusion_loss`` in the spelled-out loop,
``train_step_fused(..., snr_gamma=)`` in the fused one, ``train_class(..., snr_gamma=)``.  With the defaults nothing changes.

No torch.autograd anywhere: the backward pass is explicit HIP kernels (csrc/train.cpp).  Arithmetic is fp32; the
GradScaler protocol (scale, unscale, inf check, skip, growth/backoff) is implemented, the autocast-to-fp16 is not.
``train_step_fused`` runs the whole loop body in ONE C call (sisic_unet_train_step).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from collections import OrderedDict
from typing import Callable, Dict, Iterable, Optional

import torch

from . import _lib, ops
from ._lib import check
from .scheduler import HipDDPMScheduler
from .unet import HipUNet2DModel

LR = 1e-4            # train_diffusion.py:62
TIMESTEPS = 1000     # train_diffusion.py:60


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class HipLoss:
    """What ``F.mse_loss(noise_pred, noise)`` returns in the reference's loop: ``.item()`` and ``.backward()``."""

    def __init__(self, model: HipUNet2DModel, pred: torch.Tensor, target: torch.Tensor, scale: float = 1.0,
                 weights: Optional[torch.Tensor] = None):
        # the library's loss walks both tensors by the prediction's element count: a target of another shape (the noise of a
        # model whose out_channels differ from its in_channels) is refused here, before any library call
        if tuple(target.shape) != tuple(pred.shape):
            raise RuntimeError(f"mse_loss: the target's shape {tuple(target.shape)} must match the prediction's {tuple(pred.shape)}")
        self.model, self.pred, self.target, self.scale = model, pred, target, float(scale)
        # per-sample loss weights (host fp32 [B]) or None: set on the handle for each of the two sisic_mse_loss calls and
        # cleared after it, so that nothing else is ever weighted by a leftover
        self.weights = None if weights is None else weights.detach().to("cpu", torch.float32).reshape(-1).contiguous()
        self._loss = ops.empty(1, dtype=torch.float32, device=pred.device)
        self._mse(1.0, self._loss.data_ptr(), None)

    def _mse(self, grad_scale: float, loss_ptr, dpred_ptr) -> None:
        with _loss_weights(self.model, self.weights):
            check(_lib.load().sisic_mse_loss(self.model.handle, self.pred.data_ptr(), self.target.data_ptr(), self.pred.numel(),
                                             grad_scale, loss_ptr, dpred_ptr, _stream(self.pred.device)))

    def item(self) -> float:
        return float(self._loss.item())

    def __float__(self) -> float:
        return self.item()

    def detach(self) -> torch.Tensor:
        return self._loss.detach().clone()

    def backward(self) -> None:
        """d(scale * loss)/d(parameters) into the model's gradient arena (the tape of the last forward is consumed)."""
        dpred = ops.empty_like(self.pred)
        lib = _lib.load()
        self._mse(self.scale, None, dpred.data_ptr())
        check(lib.sisic_unet_backward(self.model.handle, dpred.data_ptr(), _stream(self.pred.device)))


def _clear_loss_weights(model: HipUNet2DModel) -> None:
    """clear the handle's loss weights if this module set any (a model that never had weights makes no call)"""
    if getattr(model, "_loss_weights_set", False):
        check(_lib.load().sisic_unet_set_loss_weights(model.handle, None, 0))
        model._loss_weights_set = False


@contextlib.contextmanager
def _loss_weights(model: HipUNet2DModel, weights: Optional[torch.Tensor]):
    """The handle's loss weights for the library calls inside the block: ``weights`` (host fp32 [B]; sisic_unet_set_loss_weights
    keeps them until cleared) or, with None, none -- a leftover is cleared first.  Cleared on the way out, also after an exception."""
    _clear_loss_weights(model)
    if weights is None:
        yield
        return
    check(_lib.load().sisic_unet_set_loss_weights(model.handle, C.cast(weights.data_ptr(), _lib.c_float_p), weights.numel()))
    model._loss_weights_set = True
    try:
        yield
    finally:
        _clear_loss_weights(model)


def mse_loss(noise_pred: torch.Tensor, noise: torch.Tensor) -> HipLoss:
    """``torch.nn.functional.mse_loss(noise_pred, noise)`` for the output of a training-mode ``HipUNet2DModel`` call.  Always
    the plain mean: loss weights left on the handle are cleared first."""
    model = getattr(noise_pred, "_sisic_model", None)
    if model is None:
        raise RuntimeError("mse_loss expects the .sample of a HipUNet2DModel called in training mode")
    return HipLoss(model, noise_pred.contiguous(), noise.to(device=noise_pred.device, dtype=torch.float32).contiguous())


def compute_snr(scheduler, timesteps) -> torch.Tensor:
    """SNR(t) = abar_t / (1 - abar_t) of the scheduler's table, float64 [B] on the host (diffusers' ``compute_snr``)."""
    t = torch.as_tensor(timesteps).detach().to("cpu").to(torch.int64).reshape(-1)
    abar = scheduler.alphas_cumprod.to(torch.float64)[t]
    return abar / (1.0 - abar)


def min_snr_weights(scheduler, timesteps, snr_gamma: float, prediction_type: str = "epsilon") -> torch.Tensor:
    """Min-SNR-gamma loss weights (Hang et al. 2023) per sample, computed in float64 and rounded to fp32 once, host [B]:
    epsilon ``min(snr, g) / snr``; v_prediction ``min(snr, g) / (snr + 1)``; sample ``min(snr, g)``.  ``snr_gamma`` may be
    ``inf`` (epsilon: all ones)."""
    _lib.prediction_code(prediction_type)
    g = float(snr_gamma)
    if not g > 0.0:
        raise ValueError(f"snr_gamma must be positive, got {snr_gamma}")
    snr = compute_snr(scheduler, timesteps)
    capped = torch.clamp(snr, max=g)
    if prediction_type == "epsilon":
        w = capped / snr
    elif prediction_type == "v_prediction":
        w = capped / (snr + 1.0)
    else:
        w = capped
    return w.to(torch.float32)


def diffusion_target(model: HipUNet2DModel, scheduler, images: torch.Tensor, noise: torch.Tensor, timesteps) -> torch.Tensor:
    """what a model of ``model.prediction_type`` regresses on: the noise, the images, or ``scheduler.get_velocity``"""
    kind = model.prediction_type
    if kind == "epsilon":
        return noise
    if kind == "sample":
        return images
    return scheduler.get_velocity(images, noise, timesteps)


def diffusion_loss(model_output: torch.Tensor, images: torch.Tensor, noise: torch.Tensor, timesteps, scheduler,
                   snr_gamma: Optional[float] = None) -> HipLoss:
    """The loss of the spelled-out loop under the model's objective: ``mse_loss(model_output, target)`` with the target that
    follows the model's ``prediction_type`` and, with ``snr_gamma``, the per-sample Min-SNR weights of ``min_snr_weights``
    (set on the handle for the loss's two library calls and cleared after each).  Equal to the fused step bit for bit."""
    model = getattr(model_output, "_sisic_model", None)
    if model is None:
        raise RuntimeError("diffusion_loss expects the .sample of a HipUNet2DModel called in training mode")
    dev = model_output.device
    x0 = images.to(device=dev, dtype=torch.float32).contiguous()
    nz = noise.to(device=dev, dtype=torch.float32).contiguous()
    target = diffusion_target(model, scheduler, x0, nz, timesteps)
    weights = None if snr_gamma is None else min_snr_weights(scheduler, timesteps, snr_gamma, model.prediction_type)
    return HipLoss(model, model_output.contiguous(), target.contiguous(), weights=weights)


class HipEMA:
    """``diffusers.training_utils.EMAModel`` for a HipUNet2DModel: the shadow parameters live in the library, beside the
    trained ones (sisic_unet_ema_begin copies the current weights, as ``EMAModel.__init__`` does).

    Attached to the optimizer -- ``HipAdam(model, ema=ema)`` -- the update rides in the optimizer's own pass over the
    weights and ``ema.step()`` is NOT called by the loop.  Kept separately it is the published spelling, ``ema.step()``
    after ``optimizer.step()``: one more launch over the two arenas (sisic_unet_ema_step).  Either way
    ``optimization_step`` counts every call, a scaler-skipped step included: the shadow then moves towards the unchanged
    weights, exactly as upstream does.

    ``model=None`` gives the decay schedule alone (``get_decay``), which needs no GPU."""

    def __init__(self, model: Optional[HipUNet2DModel] = None, decay: float = 0.9999, min_decay: float = 0.0,
                 update_after_step: int = 0, use_ema_warmup: bool = False, inv_gamma: float = 1.0, power: float = 2 / 3):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay must be in [0, 1], got {decay}")
        if not 0.0 <= float(min_decay) <= 1.0:
            raise ValueError(f"min_decay must be in [0, 1], got {min_decay}")
        self.decay, self.min_decay = float(decay), float(min_decay)
        self.update_after_step, self.use_ema_warmup = int(update_after_step), bool(use_ema_warmup)
        self.inv_gamma, self.power = inv_gamma, power
        self.optimization_step = 0
        self.cur_decay_value = None
        self._stored = None
        self.model = model
        if model is not None:
            model._ensure_training()
            check(_lib.load().sisic_unet_ema_begin(model.handle))

    def get_decay(self, optimization_step: int) -> float:
        """The decay of one step, by the published formula."""
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur_decay_value = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            cur_decay_value = (1 + step) / (10 + step)
        cur_decay_value = min(cur_decay_value, self.decay)
        cur_decay_value = max(cur_decay_value, self.min_decay)
        return cur_decay_value

    def _handle(self):
        if self.model is None:
            raise RuntimeError("this HipEMA was made without a model: it only computes the decay schedule")
        h = self.model.handle
        if not _lib.load().sisic_unet_ema_active(h):
            raise RuntimeError("the model's library handle was rebuilt (moved to another device?): the EMA went with it; "
                               "make a new HipEMA")
        return h

    def _next_decay(self) -> float:
        return self.get_decay(self.optimization_step + 1)

    def _commit(self, decay: float) -> None:
        self.optimization_step += 1
        self.cur_decay_value = decay

    def step(self, parameters=None) -> None:
        """``ema_model.step(model.parameters())`` after an optimizer step that did not carry the EMA."""
        h = self._handle()
        decay = self._next_decay()
        check(_lib.load().sisic_unet_ema_step(h, decay, _stream(self.model.device)))
        self._commit(decay)

    def shadow_params(self) -> "OrderedDict[str, torch.Tensor]":
        self._handle()
        return self.model._read_all(4)

    def state_dict(self) -> dict:
        return {"decay": self.decay, "min_decay": self.min_decay, "optimization_step": self.optimization_step,
                "update_after_step": self.update_after_step, "use_ema_warmup": self.use_ema_warmup,
                "inv_gamma": self.inv_gamma, "power": self.power, "shadow_params": self.shadow_params()}

    def load_state_dict(self, state_dict: dict) -> None:
        sd = dict(state_dict)
        decay, min_decay = float(sd.get("decay", self.decay)), float(sd.get("min_decay", self.min_decay))
        if not 0.0 <= decay <= 1.0 or not 0.0 <= min_decay <= 1.0:
            raise ValueError("decay and min_decay must be in [0, 1]")
        self.decay, self.min_decay = decay, min_decay
        self.optimization_step = int(sd.get("optimization_step", self.optimization_step))
        self.update_after_step = int(sd.get("update_after_step", self.update_after_step))
        self.use_ema_warmup = bool(sd.get("use_ema_warmup", self.use_ema_warmup))
        self.inv_gamma, self.power = sd.get("inv_gamma", self.inv_gamma), sd.get("power", self.power)
        shadow = sd.get("shadow_params")
        if shadow is not None:
            self._handle()
            missing = [k for k in self.model._spec if k not in shadow]
            if missing:
                raise RuntimeError(f"shadow_params lacks {len(missing)} tensors: {missing[:5]}")
            self.model._write_all(4, {k: shadow[k] for k in self.model._spec}, "HipEMA.load_state_dict")

    def copy_to(self, model: Optional[HipUNet2DModel] = None) -> None:
        """Load the averaged weights into ``model`` (default: the EMA's own).  This is a ``load_state_dict``: under an
        existing optimizer the moments start afresh.  To evaluate or save the averaged weights in the middle of a run use
        ``average_parameters()``, which leaves the optimizer alone."""
        (model if model is not None else self.model).load_state_dict(self.shadow_params())

    def store(self, model: Optional[HipUNet2DModel] = None) -> None:
        model = model if model is not None else self.model
        self._stored = OrderedDict((k, v.detach().cpu().clone()) for k, v in model.state_dict().items())

    def restore(self, model: Optional[HipUNet2DModel] = None) -> None:
        if self._stored is None:
            raise RuntimeError("restore() without a store() before it")
        (model if model is not None else self.model).load_state_dict(self._stored)
        self._stored = None

    @contextlib.contextmanager
    def average_parameters(self):
        """Inside the context the model IS the averaged model (sisic_unet_ema_swap: the two arenas exchange contents and
        every packed form follows): calls, ``state_dict()`` and sampling see the EMA; optimizer steps raise.  On exit the
        trained weights are back, bit for bit."""
        h = self._handle()
        lib, model = _lib.load(), self.model
        check(lib.sisic_unet_ema_swap(h, _stream(model.device)))
        model._params_stale = True
        model._ema_swapped = True
        try:
            yield self
        finally:
            check(lib.sisic_unet_ema_swap(h, _stream(model.device)))
            model._params_stale = True
            model._ema_swapped = False


class HipAdam:
    """``torch.optim.Adam(model.parameters(), lr)`` for a HipUNet2DModel: the state (m, v, step) lives in the library.

    ``max_grad_norm``: ``clip_grad_norm_(model.parameters(), max_grad_norm)`` in front of every step; the norm of the last
    step (unscaled, before clipping: what ``clip_grad_norm_`` returns) is ``optimizer.grad_norm``.  ``ema``: a HipEMA whose
    update rides in the step.  With neither, ``step()`` calls the plain entry point: the same update pass, and the statistics
    pass in front of it only when ``check_inf`` asks."""

    def __init__(self, model_or_params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, max_grad_norm: Optional[float] = None, ema: Optional[HipEMA] = None):
        if weight_decay != 0.0 or amsgrad:
            raise NotImplementedError("the reference uses plain Adam (train_diffusion.py:203)")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be None or >= 0, got {max_grad_norm}")
        model = model_or_params if isinstance(model_or_params, HipUNet2DModel) else getattr(model_or_params, "_sisic_model", None)
        if model is None:
            raise RuntimeError("HipAdam needs the HipUNet2DModel (or its .parameters())")
        if ema is not None and ema.model is not model:
            raise ValueError("the HipEMA belongs to another model")
        self.model, self.lr, self.betas, self.eps = model, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema = ema
        self.grad_norm: Optional[float] = None
        model._ensure_training()

    def zero_grad(self, set_to_none: bool = True) -> None:
        check(_lib.load().sisic_unet_zero_grad(self.model.handle, _stream(self.model.device)))

    def _extension(self) -> Optional[_lib.OptimExt]:
        """the options of the *_ext entry points, or None when nothing asks for them (the plain entry points are called)"""
        if self.max_grad_norm is None and self.ema is None:
            return None
        ext = _lib.OptimExt()
        ext.max_grad_norm = self.max_grad_norm if self.max_grad_norm is not None else 0.0
        if self.ema is not None:
            self.ema._handle()
            ext.ema_decay, ext.ema_update = self.ema._next_decay(), 1
        return ext

    def _extension_done(self, ext: _lib.OptimExt, norm: float) -> None:
        self.grad_norm = float(norm)
        if self.ema is not None:
            self.ema._commit(ext.ema_decay)

    def step(self, inv_scale: float = 1.0, check_inf: bool = False) -> bool:
        """One Adam update; returns False when it was skipped because a gradient was inf/nan (GradScaler semantics)."""
        found, norm = C.c_int(0), C.c_float(0.0)
        ext = self._extension()
        args = [self.model.handle, self.lr, self.betas[0], self.betas[1], self.eps, float(inv_scale)]
        args += [C.byref(ext)] if ext is not None else []
        args += [C.byref(found) if check_inf else None]
        args += [C.byref(norm)] if ext is not None else []
        fn = "sisic_unet_optimizer_step" if ext is None else "sisic_unet_optimizer_step_ext"
        check(getattr(_lib.load(), fn)(*args, _stream(self.model.device)))
        if ext is not None:
            self._extension_done(ext, norm.value)
        self.model._params_stale = True
        return found.value == 0


class HipLambdaLR:
    """``torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda)`` for a HipAdam: ``lr`` is a per-call scalar of the step, so
    the scheduler only sets ``optimizer.lr`` (to ``base_lr * lr_lambda(0)`` at construction, as torch does)."""

    def __init__(self, optimizer: HipAdam, lr_lambda: Callable[[int], float]):
        self.optimizer, self.lr_lambda = optimizer, lr_lambda
        self.base_lr = optimizer.lr
        self.last_epoch = 0
        self._last_lr = self.base_lr * lr_lambda(0)
        optimizer.lr = self._last_lr

    def step(self) -> None:
        self.last_epoch += 1
        self._last_lr = self.base_lr * self.lr_lambda(self.last_epoch)
        self.optimizer.lr = self._last_lr

    def get_last_lr(self):
        return [self._last_lr]


def cosine_schedule_with_warmup(num_warmup_steps: int, num_training_steps: int, num_cycles: float = 0.5) -> Callable[[int], float]:
    """The lambda of ``diffusers.optimization.get_cosine_schedule_with_warmup``: a linear ramp over the warm-up steps, then
    the cosine from 1 towards 0 over the remaining ones."""

    def lr_lambda(current_step: int) -> float:
        if current_step < num_warmup_steps:
            return float(current_step) / float(max(1, num_warmup_steps))
        progress = float(current_step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))

    return lr_lambda


class _ScaledLoss:
    def __init__(self, loss: HipLoss, scale: float):
        self.loss, self.scale = loss, scale

    def backward(self) -> None:
        self.loss.scale = self.scale
        self.loss.backward()


class HipGradScaler:
    """``torch.cuda.amp.GradScaler()`` (train_diffusion.py:204): defaults init_scale 65536, growth 2 every 2000 clean steps,
    backoff 0.5 after a step with inf/nan gradients (that step is skipped)."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000, enabled: bool = True):
        self._scale = float(init_scale) if enabled else 1.0
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        self.enabled = enabled
        self._growth_tracker = 0
        self._found_inf = False

    def get_scale(self) -> float:
        return self._scale

    def scale(self, loss: HipLoss) -> _ScaledLoss:
        return _ScaledLoss(loss, self._scale)

    def step(self, optimizer: HipAdam) -> bool:
        ok = optimizer.step(inv_scale=1.0 / self._scale, check_inf=self.enabled)
        self._found_inf = not ok
        return ok

    def update(self) -> None:
        if not self.enabled:
            return
        if self._found_inf:
            self._scale *= self.backoff_factor
            self._growth_tracker = 0
        else:
            self._growth_tracker += 1
            if self._growth_tracker == self.growth_interval:
                self._scale *= self.growth_factor
                self._growth_tracker = 0
        self._found_inf = False


def train_step_fused(model: HipUNet2DModel, scheduler: HipDDPMScheduler, images: torch.Tensor, noise: torch.Tensor,
                     timesteps: torch.Tensor, optimizer: HipAdam, scaler: Optional[HipGradScaler] = None, class_labels=None,
                     snr_gamma: Optional[float] = None):
    """The loop body of train_diffusion.py:215-233 in one library call (sisic_unet_train_step; sisic_unet_train_step_ext
    when the optimizer clips or carries an EMA -- the norm is then ``optimizer.grad_norm``); returns (loss, step_taken).
    ``class_labels``: one integer per image for a class-conditional model (sisic_unet_train_step_cond), None otherwise; the
    library takes them as a host array, so labels on the device cost one small blocking copy per step.
    The target follows ``model.prediction_type`` (the handle carries it; v is formed inside the loss kernel).  ``snr_gamma``:
    Min-SNR-gamma weights of this batch's timesteps (``min_snr_weights``), set on the handle for this call and cleared after."""
    labels = model._labels_host(class_labels, images.shape[0])
    model._ensure_training()
    weights = None if snr_gamma is None else min_snr_weights(scheduler, timesteps, snr_gamma, model.prediction_type).contiguous()
    with _loss_weights(model, weights):
        return _train_step_fused(model, scheduler, images, noise, timesteps, optimizer, scaler, labels)


def _train_step_fused(model, scheduler, images, noise, timesteps, optimizer, scaler, labels):
    x0 = images.to(device=model.device, dtype=torch.float32).contiguous()
    nz = noise.to(device=model.device, dtype=torch.float32).contiguous()
    B, _, H, W = x0.shape
    t = torch.as_tensor(timesteps).detach().to("cpu").to(torch.int64).reshape(-1).contiguous()
    a, c = scheduler.add_noise_coefficients(t)
    loss, found, norm = C.c_float(0.0), C.c_int(0), C.c_float(0.0)
    scale = scaler.get_scale() if scaler is not None else 1.0
    found_ref = C.byref(found) if scaler is not None and scaler.enabled else None
    ext = optimizer._extension()
    # one argument list for the three entry points: labels go in behind the timesteps (sisic_unet_train_step_cond), the options
    # and the norm where the chosen symbol takes them (_cond takes both always, ext may be NULL; _ext when there are options)
    cond, extended = labels is not None, labels is not None or ext is not None
    args = [model.handle, x0.data_ptr(), nz.data_ptr(), C.cast(t.data_ptr(), _lib.c_int64_p)]
    args += [C.cast(labels.data_ptr(), _lib.c_int64_p)] if cond else []
    args += [C.cast(a.data_ptr(), _lib.c_float_p), C.cast(c.data_ptr(), _lib.c_float_p), B, H, W, optimizer.lr, optimizer.betas[0],
             optimizer.betas[1], optimizer.eps, float(scale)]
    args += [C.byref(ext) if ext is not None else None] if extended else []
    args += [C.byref(loss), found_ref]
    args += [C.byref(norm)] if extended else []
    fn = "sisic_unet_train_step_cond" if cond else "sisic_unet_train_step_ext" if ext is not None else "sisic_unet_train_step"
    check(getattr(_lib.load(), fn)(*args, _stream(model.device)))
    if ext is not None:
        optimizer._extension_done(ext, norm.value)
    model._params_stale = True
    if scaler is not None:
        scaler._found_inf = bool(found.value)
        scaler.update()
    return loss.value, found.value == 0


def drop_labels(labels: torch.Tensor, cond_drop_prob: float, null_label: int,
                generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The label dropout of classifier-free guidance training (Ho & Salimans 2022): ONE draw ``torch.rand(B) < cond_drop_prob``
    from ``generator`` (on the generator's device; the labels' device without one), and the labels it marks become
    ``null_label``.  ``cond_drop_prob`` 0 still consumes the draw, so that the random stream does not depend on it."""
    if not 0.0 <= float(cond_drop_prob) <= 1.0:
        raise ValueError(f"cond_drop_prob must be in [0, 1], got {cond_drop_prob}")
    dev = generator.device if generator is not None else labels.device
    drop = torch.rand(labels.shape[0], generator=generator, device=dev) < float(cond_drop_prob)
    return torch.where(drop.to(labels.device), torch.full_like(labels, int(null_label)), labels)


def _train_loop(model: HipUNet2DModel, loader, name: str, epochs: int, lr: float, checkpoint_dir: Optional[str], fused: bool,
                generator: Optional[torch.Generator], log, max_grad_norm, ema_decay, ema_warmup: bool, lr_schedule,
                cond_drop_prob: Optional[float], dropout_seed: int = 0, snr_gamma: Optional[float] = None):
    """the loop of train_class; cond_drop_prob not None: the loader yields (images, labels) and the model is conditional"""
    dev = model.device
    if model.config.dropout > 0:
        # the masks of this run: seeded here, the counter going on from where the model stands (0 for a new model; a resumed run
        # that restored it with set_dropout(..., first_call=saved dropout_next_call) continues its stream)
        model.set_dropout(model.config.dropout, seed=dropout_seed, first_call=model.dropout_next_call)
    scheduler = HipDDPMScheduler(num_train_timesteps=TIMESTEPS, beta_schedule="squaredcos_cap_v2")
    ema = HipEMA(model, decay=ema_decay, use_ema_warmup=ema_warmup) if ema_decay is not None else None
    optimizer = HipAdam(model, lr=lr, max_grad_norm=max_grad_norm, ema=ema)
    lr_scheduler = HipLambdaLR(optimizer, lr_schedule) if lr_schedule is not None else None
    scaler = HipGradScaler()
    best_loss = float("inf")
    history = []
    conditional = cond_drop_prob is not None

    def save(tag: str) -> None:
        torch.save(model.state_dict(), os.path.join(checkpoint_dir, f"unet_{name}_{tag}.pth"))
        if ema is not None:
            with ema.average_parameters():
                torch.save(model.state_dict(), os.path.join(checkpoint_dir, f"unet_{name}_{tag}_ema.pth"))

    for epoch in range(epochs):
        model.train()
        epoch_loss, n_batches = 0.0, 0
        for item in loader:
            images, labels = item if conditional else (item, None)
            images = images.to(dev, non_blocking=True)
            noise = torch.randn(images.shape, generator=generator, device=generator.device if generator is not None else dev)
            timesteps = torch.randint(0, TIMESTEPS, (images.size(0),), generator=generator,
                                      device=generator.device if generator is not None else dev).long()
            if conditional:
                # the library takes the labels as a host array (they select rows on the host side of the launch): one copy of
                # 8 B bytes per batch from a DeviceLoader's device labels, beside the loss read-back that synchronises every
                # step anyway; the dropout then runs on the host
                labels = drop_labels(torch.as_tensor(labels).to("cpu", torch.int64), cond_drop_prob,
                                     model.config.num_class_embeds - 1, generator)
            if fused:
                value, _ = train_step_fused(model, scheduler, images, noise, timesteps, optimizer, scaler, class_labels=labels,
                                            snr_gamma=snr_gamma)
            else:
                noisy_images = scheduler.add_noise(images, noise, timesteps)
                noise_pred = model(noisy_images, timesteps, class_labels=labels).sample
                if snr_gamma is None and model.prediction_type == "epsilon":
                    loss = mse_loss(noise_pred, noise)
                else:
                    loss = diffusion_loss(noise_pred, images, noise, timesteps, scheduler, snr_gamma=snr_gamma)
                optimizer.zero_grad(set_to_none=True)
                scaler.scale(loss).backward()
                scaler.step(optimizer)
                scaler.update()
                value = loss.item()
            if lr_scheduler is not None:
                lr_scheduler.step()
            epoch_loss += value
            n_batches += 1
        avg_loss = epoch_loss / max(1, n_batches)
        history.append(avg_loss)
        if log:
            log(f"Loss: {avg_loss:.5f}")
        if checkpoint_dir:
            os.makedirs(checkpoint_dir, exist_ok=True)
            if avg_loss < best_loss:
                best_loss = avg_loss
                save("best")
            if (epoch + 1) % 5 == 0:
                save(f"epoch_{epoch + 1:02d}")
        elif avg_loss < best_loss:
            best_loss = avg_loss
    return history


def train_class(model: HipUNet2DModel, loader: Iterable[torch.Tensor], class_name: str, epochs: int = 50, lr: float = LR,
                checkpoint_dir: Optional[str] = None, fused: bool = True, generator: Optional[torch.Generator] = None,
                log: Optional[Callable[[str], None]] = print, max_grad_norm: Optional[float] = None,
                ema_decay: Optional[float] = None, ema_warmup: bool = False,
                lr_schedule: Optional[Callable[[int], float]] = None, dropout_seed: int = 0,
                snr_gamma: Optional[float] = None):
    """``train_class`` of train_diffusion.py:187-266 for one class: epochs over ``loader`` (batches of images in [-1,1],
    [B,3,H,W]), best-loss checkpoint ``unet_{class}_best.pth`` and a checkpoint every 5 epochs.  Returns the per-epoch
    average losses.  ``generator`` seeds noise / timestep draws (the reference uses the global RNG).

    Beyond the reference, each off by default: ``max_grad_norm`` clips the global gradient norm; ``ema_decay`` keeps an EMA of
    the weights (``ema_warmup``: EMAModel's warm-up decay) and saves it beside every checkpoint as ``..._ema.pth``;
    ``lr_schedule`` is a lambda step -> factor of ``lr`` (``cosine_schedule_with_warmup``), advanced once per batch.
    A model built with ``dropout > 0`` trains with it; ``dropout_seed`` seeds its masks (they do not consume ``generator``), and
    the checkpoints are those of a model without: dropout adds no tensors.  The objective is the model's: a model built with
    ``prediction_type="v_prediction"`` or ``"sample"`` regresses on v or on the images; ``snr_gamma`` weights every sample's
    loss by Min-SNR-gamma (``min_snr_weights``; 5.0 is the published choice).  The type is not recorded in the checkpoint."""
    if model.config.num_class_embeds is not None:
        raise ValueError("train_class trains an unconditional model; a class-conditional one takes train_conditional")
    return _train_loop(model, loader, class_name, epochs, lr, checkpoint_dir, fused, generator, log, max_grad_norm, ema_decay,
                       ema_warmup, lr_schedule, None, dropout_seed, snr_gamma)


def train_conditional(model: HipUNet2DModel, loader, name: str, cond_drop_prob: float = 0.1, epochs: int = 50, lr: float = LR,
                      checkpoint_dir: Optional[str] = None, fused: bool = True, generator: Optional[torch.Generator] = None,
                      log: Optional[Callable[[str], None]] = print, max_grad_norm: Optional[float] = None,
                      ema_decay: Optional[float] = None, ema_warmup: bool = False,
                      lr_schedule: Optional[Callable[[int], float]] = None, dropout_seed: int = 0,
                      snr_gamma: Optional[float] = None):
    """``train_class`` for ONE class-conditional model over all classes: ``loader`` yields ``(images, labels)`` (a
    ``data.DeviceLoader`` over a labelled ``DeviceDataset``), the labels go to the model as ``class_labels``.  Checkpoints
    (``unet_{name}_best.pth``, every 5 epochs, the ``_ema`` files), clipping, EMA, schedule and the returned history are
    train_class's, and so is ``dropout_seed`` for a model built with ``dropout > 0``.

    Classifier-free guidance: with probability ``cond_drop_prob`` an image trains under the null label, by convention the
    LAST row of the table, ``num_class_embeds - 1`` -- build the model with ``n_classes + 1`` rows.  Per batch ``generator``
    is consumed in a fixed order: the noise (``randn``), the timesteps (``randint``), then the dropout (``drop_labels``:
    ``torch.rand(B) < cond_drop_prob``)."""
    if model.config.num_class_embeds is None:
        raise ValueError("train_conditional needs a class-conditional model (HipUNet2DModel(num_class_embeds=n_classes + 1))")
    if not 0.0 <= float(cond_drop_prob) <= 1.0:
        raise ValueError(f"cond_drop_prob must be in [0, 1], got {cond_drop_prob}")
    return _train_loop(model, loader, name, epochs, lr, checkpoint_dir, fused, generator, log, max_grad_norm, ema_decay,
                       ema_warmup, lr_schedule, float(cond_drop_prob), dropout_seed, snr_gamma)


# ---- the ResNet18 classifier (xai/XAI.py:357-471), BatchNorm frozen or with batch statistics ------------------------------
# What the reference leaves to torch: training the lesion classifier whose explanations the XAI passes compute.
# batchnorm="frozen" (the default, for fine-tuning a loaded checkpoint): BatchNorm keeps the constants it was loaded with
# (torchvision.ops.FrozenBatchNorm2d), which is the function the library's folded forward computes, so the training forward is
# the inference forward.  batchnorm="batch" (for training from random weights, weights.default_init_resnet18_state_dict):
# nn.BatchNorm2d in training mode -- batch moments in the forward, gamma and beta trained, running statistics updated with
# ``bn_momentum`` -- and after every step the inference side is the folded form of the current state dict.  Training is entered
# through the optimizer object, not through ``clf.train()``.
class HipClassifierAdam:
    """``torch.optim.Adam`` over the trainable tensors of a HipMelanomaClassifier: with ``batchnorm="frozen"`` the 22 (20
    convolution weights, fc.weight, fc.bias), with ``batchnorm="batch"`` the 62 (the BatchNorm gamma and beta as well; the
    running statistics follow the batches with ``bn_momentum``, torch's ``momentum``, in (0, 1]).  Parameters, gradients and
    moments live in the library (sisic_resnet_train_begin / _begin_bn on construction).
    ``max_grad_norm``: ``clip_grad_norm_`` in front of every step; ``grad_norm`` is the norm of the last step before clipping.
    ``close()`` ends training (sisic_resnet_train_end): the model is then what loading its ``state_dict()`` would give."""

    def __init__(self, clf, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: Optional[float] = None,
                 batchnorm: str = "frozen", bn_momentum: float = 0.1):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be None or >= 0, got {max_grad_norm}")
        if batchnorm not in ("frozen", "batch"):
            raise ValueError(f"batchnorm {batchnorm!r}: 'frozen' or 'batch'")
        handle = clf.handle                      # a model on the CPU raises here: MI355X only
        if clf._trainer is not None:
            raise RuntimeError("this classifier already has a HipClassifierAdam; close() it first")
        self.clf, self.lr, self.betas, self.eps = clf, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm: Optional[float] = None
        self.batchnorm, self.bn_momentum = batchnorm, float(bn_momentum)
        if batchnorm == "batch":
            cfg = _lib.ResnetBnConfig(1, self.bn_momentum)
            check(_lib.load().sisic_resnet_train_begin_bn(handle, C.byref(cfg)))
        else:
            check(_lib.load().sisic_resnet_train_begin(handle))
        self._active = True
        clf._trainer = self

    def _handle(self):
        if not self._active:
            raise RuntimeError("this HipClassifierAdam is closed (close(), or the model was reloaded or moved)")
        return self.clf.handle

    @property
    def steps(self) -> int:
        return int(_lib.load().sisic_resnet_train_steps(self._handle()))

    def zero_grad(self, set_to_none: bool = True) -> None:
        check(_lib.load().sisic_resnet_zero_grad(self._handle()))

    def step(self) -> bool:
        """One Adam update and the rebuild of every folded and packed filter; False: a gradient was inf/nan, nothing moved."""
        a = _lib.ResnetTrainArgs()
        a.lr, a.beta1, a.beta2, a.eps = self.lr, self.betas[0], self.betas[1], self.eps
        a.max_grad_norm = self.max_grad_norm if self.max_grad_norm is not None else 0.0
        a.stream = torch.cuda.current_stream(self.clf.device).cuda_stream
        check(_lib.load().sisic_resnet_optimizer_step(self._handle(), C.byref(a)))
        self.grad_norm = float(a.grad_norm)
        if self.batchnorm == "batch":
            self.clf._params_stale = True         # the running statistics moved in loss_backward, whatever the step did
        if a.found_inf:
            return False
        self.clf._params_stale = True
        return True

    def close(self) -> None:
        if self._active:
            self.clf._sync_params()
            check(_lib.load().sisic_resnet_train_end(self.clf.handle))
            self._active = False
            self.clf._trainer = None


def balanced_class_weights(labels, num_classes: int) -> torch.Tensor:
    """inverse class frequency, sklearn's "balanced": N / (num_classes * count[c]); a class without samples gets 0"""
    lab = torch.as_tensor(labels).detach().to("cpu", torch.int64)
    count = torch.bincount(lab, minlength=num_classes)[:num_classes].double()
    w = torch.where(count > 0, lab.numel() / (num_classes * count.clamp(min=1)), torch.zeros_like(count))
    return w.float()


@torch.no_grad()
def evaluate_classifier(clf, loader) -> Dict[str, object]:
    """Confusion matrix (rows: true class, columns: predicted), accuracy and balanced accuracy (mean recall over the classes
    that occur) of ``clf`` over ``loader`` (items ``(images, labels)``), batched forwards.  A ``data.DeviceLoader`` is walked
    once in dataset order with its augmentation off, whatever its own settings."""
    clf.handle                                   # a model on the CPU raises here: MI355X only
    from .data import DeviceLoader
    if isinstance(loader, DeviceLoader):
        loader = DeviceLoader(loader.dataset, loader.batch_size, shuffle=False, augment=False)
    n = clf.num_classes
    cm = torch.zeros((n, n), dtype=torch.int64)
    for images, labels in loader:
        pred = clf.predict(images.to(clf.device)).to("cpu", torch.int64)
        lab = torch.as_tensor(labels).to("cpu", torch.int64)
        cm += torch.bincount(lab * n + pred, minlength=n * n).view(n, n)
    total = int(cm.sum())
    support = cm.sum(1)
    recall = cm.diag().double() / support.clamp(min=1).double()
    return {"confusion_matrix": cm, "accuracy": float(cm.diag().sum()) / max(1, total),
            "balanced_accuracy": float(recall[support > 0].mean()) if total else 0.0}


CLASSIFIER_NOISE_TAG = 7          # include/sisic.h, device-noise contract: the z of a noised classifier batch


def classifier_noise_draws(noise_seed: int, epoch: int, batch_index: int, B: int, noise_timesteps):
    """(timesteps int64 [B], z seeds list [B]) of one noised classifier batch: a pure function of (seed, epoch, batch index,
    position).  The 2B raw 64-bit words of numpy's Philox generator under key ``noise_seed`` and counter
    (epoch, batch_index, 0, 0): word 2b gives image b's timestep, ``t_lo + ((word >> 32) * (t_hi - t_lo + 1) >> 32)`` --
    uniform on the inclusive range -- and word 2b + 1 is the 64-bit seed its z is drawn under (``ops.noise_fill``, step 0,
    ``CLASSIFIER_NOISE_TAG``)."""
    import numpy as np
    t_lo, t_hi = (int(v) for v in noise_timesteps)
    if not 0 <= t_lo <= t_hi <= 999:
        raise ValueError(f"noise_timesteps must be (t_lo, t_hi) with 0 <= t_lo <= t_hi <= 999, got {noise_timesteps!r}")
    if noise_seed < 0 or noise_seed >> 64 or epoch < 0 or batch_index < 0:
        raise ValueError("noise_seed must lie in 0 .. 2**64-1, epoch and batch_index must not be negative")
    words = np.random.Philox(key=int(noise_seed), counter=[int(epoch), int(batch_index), 0, 0]).random_raw(2 * int(B))
    t = t_lo + (((words[0::2] >> np.uint64(32)) * np.uint64(t_hi - t_lo + 1)) >> np.uint64(32)).astype(np.int64)
    return torch.from_numpy(t), [int(w) for w in words[1::2]]


def noise_classifier_batch(images: torch.Tensor, scheduler, noise_seed: int, epoch: int, batch_index: int, noise_timesteps):
    """x_t = sqrt(abar_t) * x0 + sqrt(1 - abar_t) * z for one batch (``scheduler.add_noise``, sisic_add_noise) under the draws
    of ``classifier_noise_draws``; returns (x_t, timesteps)."""
    t, seeds = classifier_noise_draws(noise_seed, epoch, batch_index, images.shape[0], noise_timesteps)
    z = ops.noise_fill(seeds, images[0].numel(), 0, CLASSIFIER_NOISE_TAG, device=images.device).reshape(images.shape)
    return scheduler.add_noise(images, z, t), t


def train_classifier(clf, loader, epochs: int, lr: float = LR, class_weights=None, val_loader=None,
                     save_dir: Optional[str] = None, max_grad_norm: Optional[float] = None,
                     log: Optional[Callable[[str], None]] = print, batchnorm: str = "frozen", bn_momentum: float = 0.1,
                     noise_timesteps=None, noise_seed: int = 0, noise_scheduler=None):
    """``train_class``'s loop for the classifier: epochs over ``loader`` (items ``(images, labels)``, images in [-1,1] as the
    sampler makes them -- a ``data.DeviceLoader`` over ``DeviceDataset.from_isic_classes``), cross-entropy, Adam, BatchNorm
    frozen or, with ``batchnorm="batch"``, with batch statistics (``bn_momentum``: see ``HipClassifierAdam``; validation uses
    the running statistics, as ``model.eval()`` does).  ``class_weights``: None, a [num_classes] tensor, or ``"balanced"`` (inverse class frequency from
    ``loader.dataset.labels``; ISIC is 67 % NV).  ``val_loader``: ``evaluate_classifier`` after every epoch, its balanced
    accuracy selects the best checkpoint (otherwise the epoch loss does).  ``save_dir``: ``classifier.pth`` under the
    reference's key names (``model.`` prefix), which ``load_state_dict`` here and the reference's
    ``load_classifier_with_fallback`` both take.  Returns the per-epoch history (loss, and the validation record).
    ``noise_timesteps=(t_lo, t_hi)``: a classifier for classifier guidance sees x_t, not x_0, so every batch is noised before
    ``loss_backward`` (``noise_classifier_batch``: t per image uniform on the inclusive range, z from the device-noise contract,
    both pure functions of (``noise_seed``, epoch, batch index, position)) under ``noise_scheduler`` (default: the samplers'
    1000-step squaredcos_cap_v2 schedule).  None (the default) issues the launches it always has."""
    clf.handle                                   # a model on the CPU raises here: MI355X only
    if noise_timesteps is not None:
        classifier_noise_draws(noise_seed, 0, 0, 1, noise_timesteps)      # refuse a bad range before anything is allocated
        if noise_scheduler is None:
            noise_scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    if isinstance(class_weights, str):
        if class_weights != "balanced":
            raise ValueError(f"class_weights {class_weights!r}: None, a tensor or 'balanced'")
        labels = getattr(getattr(loader, "dataset", None), "labels", None)
        if labels is None:
            raise ValueError("class_weights='balanced' needs loader.dataset.labels")
        class_weights = balanced_class_weights(labels, clf.num_classes)
    optimizer = HipClassifierAdam(clf, lr=lr, max_grad_norm=max_grad_norm, batchnorm=batchnorm, bn_momentum=bn_momentum)
    history = []
    best = None
    try:
        for epoch in range(epochs):
            epoch_loss, n_batches = 0.0, 0
            for batch_index, (images, labels) in enumerate(loader):
                if noise_timesteps is not None:
                    images, _ = noise_classifier_batch(images.to(clf.device), noise_scheduler, noise_seed, epoch, batch_index,
                                                       noise_timesteps)
                value, _ = clf.loss_backward(images, labels, class_weights=class_weights)
                optimizer.step()
                epoch_loss += value
                n_batches += 1
            record = {"loss": epoch_loss / max(1, n_batches)}
            if val_loader is not None:
                record.update(evaluate_classifier(clf, val_loader))
            history.append(record)
            if log:
                log(f"Loss: {record['loss']:.5f}" + (f"  balanced accuracy: {record['balanced_accuracy']:.4f}"
                                                     if val_loader is not None else ""))
            score = record["balanced_accuracy"] if val_loader is not None else -record["loss"]
            if best is None or score > best:
                best = score
                if save_dir:
                    os.makedirs(save_dir, exist_ok=True)
                    torch.save(OrderedDict((k, v.cpu()) for k, v in clf.state_dict().items()), os.path.join(save_dir, "classifier.pth"))
    finally:
        optimizer.close()
    return history
