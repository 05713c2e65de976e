"""HipUNet2DModel -- drop-in for the ``diffusers.UNet2DModel`` object the reference samples with.

It mirrors exactly what the reference's callers touch:

    model = UNet2DModel(sample_size=128, in_channels=3, ...)      model_manager.py:173-194
    model.load_state_dict(torch.load(path, map_location=dev))     model_manager.py:138-139 (strict)
    model = model.to(dev); model.eval()                           model_manager.py:142-143
    str(model.device); next(model.parameters()).device; model.training      image_generator.py:347-358,
                                                                            model_manager.py:286-313
    noise_pred = model(latents, t).sample                         image_generator.py:400

All arithmetic runs in libsisic_hip.so (``sisic_unet_forward``); this class only owns
the handle, keeps the state dict for ``state_dict()/parameters()`` and translates
arguments.  It raises if the model is asked to run anywhere but on an MI355X.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Iterator, Optional, Sequence, Union

import torch

from . import _lib
from ._lib import UNetConfigC, check
from ._module import HipModule
from .arch import UNetConfig, normalize_state_dict_keys, unet_param_spec
from . import ops


@dataclass
class UNet2DOutput:
    """Mirror of ``diffusers.models.unets.unet_2d.UNet2DOutput``."""
    sample: torch.Tensor


def timestep_frequencies(dim: int) -> torch.Tensor:
    """fp32 frequency table of ``get_timestep_embedding`` (max_period 10000, shift 0), computed with
    the same torch CPU ops the reference's diffusers code uses, then handed to the library."""
    half = dim // 2
    exponent = -math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32)
    exponent = exponent / (half - 0)
    return torch.exp(exponent)


class _ParameterView:
    """``model.parameters()``: an iterator over the tensors (``next(model.parameters()).device``,
    image_generator.py:347-358) that also knows its model (``Adam(model.parameters(), lr)`` in the reference's training
    loop becomes ``HipAdam(model.parameters(), lr)``)."""

    def __init__(self, model, tensors):
        self._it = iter(tensors)
        self._sisic_model = model

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._it)


class HipUNet2DModel(HipModule):
    _PREFIX, _NAME, _NO_CPU_PATH, _KEYS = "sisic_unet", "HipUNet2DModel", "there is no CPU path", "state-dict keys"

    def __init__(self, sample_size: int = 128, in_channels: int = 3, out_channels: int = 3,
                 layers_per_block: int = 2, block_out_channels: Sequence[int] = (64, 128, 256, 256),
                 down_block_types: Sequence[str] = ("DownBlock2D", "DownBlock2D", "AttnDownBlock2D", "DownBlock2D"),
                 up_block_types: Sequence[str] = ("UpBlock2D", "AttnUpBlock2D", "UpBlock2D", "UpBlock2D"),
                 class_embed_type=None, norm_num_groups: int = 32, norm_eps: float = 1e-5,
                 attention_head_dim: int = 8, num_class_embeds: Optional[int] = None, dropout: float = 0.0,
                 prediction_type: str = "epsilon", **unsupported):
        if class_embed_type is not None:
            raise NotImplementedError("class_embed_type must be None (the reference's models are unconditional; a "
                                      "class-conditional model is num_class_embeds=N, diffusers' nn.Embedding form)")
        if unsupported:
            raise NotImplementedError(f"unsupported UNet2DModel arguments: {sorted(unsupported)}")
        self.config = UNetConfig(sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
                                 layers_per_block=layers_per_block, block_out_channels=tuple(block_out_channels),
                                 down_block_types=tuple(down_block_types), up_block_types=tuple(up_block_types),
                                 norm_num_groups=norm_num_groups, norm_eps=norm_eps,
                                 attention_head_dim=attention_head_dim, num_class_embeds=num_class_embeds, dropout=dropout,
                                 prediction_type=prediction_type)
        self.config.validate()
        if isinstance(attention_head_dim, bool) or attention_head_dim not in (8, 32, 64):
            raise NotImplementedError(f"attention_head_dim must be 8, 32 or 64 (the widths the HIP attention kernels are built "
                                      f"for), got {attention_head_dim!r}")
        cfg = self.config
        n = len(cfg.block_out_channels)
        for i, ch in enumerate(cfg.block_out_channels):      # down block i, up block n-1-i and the mid block share a width
            if attention_head_dim != 8 and (cfg.down_has_attn[i] or cfg.up_has_attn[n - 1 - i] or i == n - 1) \
                    and ch % attention_head_dim:      # (8: the library's own check, as before)
                raise ValueError(f"block_out_channels[{i}] = {ch} carries attention and is no multiple of "
                                 f"attention_head_dim = {attention_head_dim}")
        super().__init__(unet_param_spec(self.config))
        self.training = True                  # nn.Module default until .eval()
        self._train_begun = False             # gradient / Adam arenas exist in the library (HipAdam creates them)
        self._tape_input = None               # input of the last training-mode forward (the tape points into it)
        self._latency_mode = False
        self._ema_swapped = False             # inside HipEMA.average_parameters(): the library holds the averaged weights
        self._dropout_seed = 0                # the mask stream of config.dropout (set_dropout): its seed and the counter value
        self._dropout_call = 0                #   a handle that does not exist yet starts from

    # ------------------------------------------------------------------ nn.Module surface
    @property
    def dtype(self) -> torch.dtype:
        return torch.float32

    def eval(self) -> "HipUNet2DModel":
        self.training = False
        return self

    def train(self, mode: bool = True) -> "HipUNet2DModel":
        """``model.train()`` (diffusion/train_diffusion.py:209).  The network has no batch statistics; the mode decides whether
        a call records the tape for ``loss.backward()`` (once an optimizer exists, synt_isic_amd.train) and, with
        ``dropout > 0``, whether the ResNet blocks drop: exactly the tape-recording calls do, ``eval()`` calls and every sampling
        loop never.  A training-mode call of a model with ``dropout > 0`` and no optimizer raises instead of running undropped."""
        self.training = bool(mode)
        return self

    def requires_grad_(self, flag: bool = True) -> "HipUNet2DModel":
        return self

    def set_dropout(self, p: float, seed: int = 0, first_call: int = 0) -> "HipUNet2DModel":
        """``dropout=p`` of the published UNet2DModel from now on (0 turns it off): every ResnetBlock2D computes
        ``conv2(dropout(silu(norm2(h))))`` in tape-recording forwards.  The masks are a pure function of ``(seed, call, block,
        sample, element)`` (include/sisic.h, the mask contract); ``call`` starts at ``first_call`` and advances by one per such
        forward, so ``first_call=k`` reproduces forward k of the stream and ``dropout_next_call`` continues a resumed run."""
        seed, first_call = int(seed), int(first_call)
        if not 0 <= seed < 1 << 64 or not 0 <= first_call < 1 << 32:
            raise ValueError(f"seed must fit 64 bits and first_call 32, got {seed} and {first_call}")
        config = dataclasses.replace(self.config, dropout=p)
        config.validate()
        self.config, self._dropout_seed, self._dropout_call = config, seed, first_call
        if self._handle is not None:
            check(_lib.load().sisic_unet_set_dropout(self._handle, float(p), seed, first_call))
        return self

    @property
    def prediction_type(self) -> str:
        """what ``model(x, t).sample`` means: "epsilon", "sample" or "v_prediction" (``config.prediction_type``)"""
        return self.config.prediction_type

    def set_prediction_type(self, prediction_type: str) -> "HipUNet2DModel":
        """Say what the output means from now on (sisic_unet_set_prediction_type).  The network does not know: ``model(x, t)``
        returns the same bits.  The sampling loops read it (how the step rule gets its x0: include/sisic.h SISIC_PRED_*) and so
        does the fused training step (its regression target); a scheduler mirror's ``step`` takes it per call
        (``prediction_type=model.prediction_type``).  Anything but the three names raises NotImplementedError."""
        config = dataclasses.replace(self.config, prediction_type=prediction_type)
        config.validate()
        self.config = config
        if self._handle is not None:
            check(_lib.load().sisic_unet_set_prediction_type(self._handle, _lib.prediction_code(prediction_type)))
        return self

    @property
    def dropout_next_call(self) -> int:
        """the counter value the next tape-recording forward draws its masks with"""
        if self._handle is not None:
            return int(_lib.load().sisic_unet_dropout_next_call(self._handle))
        return self._dropout_call

    def set_latency_mode(self, on: bool = True) -> "HipUNet2DModel":
        """Kernel choices for single-image latency (sisic_unet_set_latency_mode): the reference samples one image at a
        time (image_generator.py:379).  Results are batch-independent within a mode and differ in the last bits between
        modes, so a sampler should stay in one mode."""
        self._latency_mode = bool(on)
        if self._handle is not None:
            check(_lib.load().sisic_unet_set_latency_mode(self._handle, int(self._latency_mode)))
        return self

    def set_graph_mode(self, mode: int = 1) -> "HipUNet2DModel":
        """sisic_sample as a replayed hipGraph: 1 on, 0 off, -1 follow the latency mode (the default)."""
        check(_lib.load().sisic_unet_set_graph_mode(self.handle, int(mode)))
        return self

    def _ensure_training(self) -> None:
        """allocate the gradient and Adam arenas in the library (sisic_unet_train_begin), once"""
        if not self._train_begun:
            check(_lib.load().sisic_unet_train_begin(self.handle))
            self._train_begun = True

    def grads(self) -> "OrderedDict[str, torch.Tensor]":
        """{name: d loss / d parameter} of the last backward pass, on the host (what ``p.grad`` holds in the reference)."""
        if not self._train_begun:
            raise RuntimeError("no backward pass has run: create a HipAdam for this model first")
        return self._read_all(1)

    def set_grads(self, mapping: Dict[str, torch.Tensor]) -> None:
        """Write {name: tensor} into the gradient arena (sisic_unet_write); tensors not named keep what they hold.  For
        optimizer tests that choose their own gradients instead of running a backward pass."""
        if not self._train_begun:
            raise RuntimeError("no gradient arena: create a HipAdam for this model first")
        self._write_all(1, mapping, "set_grads")

    def optimizer_state(self) -> Dict[str, "OrderedDict[str, torch.Tensor]"]:
        return {"exp_avg": self._read_all(2), "exp_avg_sq": self._read_all(3),
                "step": int(_lib.load().sisic_unet_train_steps(self.handle))}

    def parameters(self):
        self._refresh_params()
        return _ParameterView(self, list(self._params.values()))

    def named_parameters(self):
        self._refresh_params()
        return iter(self._params.items())

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        self._refresh_params()
        return OrderedDict((k, v) for k, v in self._params.items())

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """Strict load of a flat ``{name: tensor}`` dict with diffusers key names."""
        if self._ema_swapped:
            raise RuntimeError("load_state_dict inside HipEMA.average_parameters(): the trained weights are swapped out and "
                               "would overwrite the loaded ones on exit")
        sd = normalize_state_dict_keys(dict(state_dict))
        missing = [k for k in self._spec if k not in sd]
        unexpected = [k for k in sd if k not in self._spec]
        if missing or (unexpected and strict):
            raise RuntimeError(f"Error(s) in loading state_dict for HipUNet2DModel: missing keys {missing[:5]}"
                               f"{'...' if len(missing) > 5 else ''} ({len(missing)}), unexpected keys "
                               f"{unexpected[:5]}{'...' if len(unexpected) > 5 else ''} ({len(unexpected)})")
        new = OrderedDict()
        for name, shape in self._spec.items():
            t = sd[name]
            if tuple(t.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {name}: checkpoint {tuple(t.shape)} vs model {tuple(shape)}")
            new[name] = t.detach().to(device=self._device, dtype=torch.float32).contiguous().clone()
        self._set_params(new)
        return self

    # ------------------------------------------------------------------ library handle (the shell's hooks)
    def _create_handle(self) -> None:
        lib = _lib.load()
        cfg = self.config
        c = UNetConfigC()
        c.in_channels, c.out_channels = cfg.in_channels, cfg.out_channels
        c.layers_per_block = cfg.layers_per_block
        c.n_blocks = len(cfg.block_out_channels)
        for i, ch in enumerate(cfg.block_out_channels):
            c.block_out_channels[i] = ch
            c.down_attn[i] = int(cfg.down_has_attn[i])
            c.up_attn[i] = int(cfg.up_has_attn[i])
        c.norm_groups, c.norm_eps, c.head_dim = cfg.norm_num_groups, cfg.norm_eps, cfg.attention_head_dim
        freqs = timestep_frequencies(cfg.block_out_channels[0]).contiguous()
        c.n_freqs = freqs.numel()
        c.freqs = C.cast(freqs.data_ptr(), _lib.c_float_p)
        h = C.c_void_p()
        if cfg.num_class_embeds is None:
            check(lib.sisic_unet_create(ops.context(self._device), C.byref(c), C.byref(h)))
        else:
            check(lib.sisic_unet_create_cond(ops.context(self._device), C.byref(c), int(cfg.num_class_embeds), C.byref(h)))
        self._handle = h
        if self._latency_mode:
            check(lib.sisic_unet_set_latency_mode(h, 1))
        if cfg.dropout > 0:
            check(lib.sisic_unet_set_dropout(h, float(cfg.dropout), self._dropout_seed, self._dropout_call))
        if cfg.prediction_type != "epsilon":
            check(lib.sisic_unet_set_prediction_type(h, _lib.prediction_code(cfg.prediction_type)))

    def _after_upload(self) -> None:
        if self._train_begun:                 # new weights under an existing optimizer: fresh moments, like a new Adam
            check(_lib.load().sisic_unet_train_begin(self._handle))

    def _before_release(self) -> None:
        if self._handle is not None:
            self._dropout_call = int(_lib.load().sisic_unet_dropout_next_call(self._handle))     # a new handle continues the stream
            self._train_begun = False

    # ------------------------------------------------------------------ forward
    def _timesteps_host(self, timestep, batch: int) -> torch.Tensor:
        if not torch.is_tensor(timestep):
            t = torch.tensor([timestep], dtype=torch.int64)
        else:
            t = timestep.detach().to("cpu").to(torch.int64).reshape(-1)
        if t.numel() == 1:
            t = t.expand(batch)
        elif t.numel() != batch:
            raise ValueError(f"timestep has {t.numel()} entries for a batch of {batch}")
        return t.contiguous()

    def _labels_host(self, class_labels, batch: int) -> Optional[torch.Tensor]:
        """diffusers' two checks (UNet2DModel.forward), then the labels as host int64 [batch], each inside the table"""
        n = self.config.num_class_embeds
        if n is None:
            if class_labels is not None:
                raise ValueError("class_embedding needs to be initialized in order to use class conditioning")
            return None
        if class_labels is None:
            raise ValueError("class_labels should be provided when doing class conditioning")
        if torch.is_tensor(class_labels):
            if class_labels.dtype.is_floating_point or class_labels.dtype == torch.bool:
                raise ValueError(f"class_labels must be integers, got {class_labels.dtype}")
            lab = class_labels.detach().to("cpu").to(torch.int64).reshape(-1)
        else:
            lab = torch.as_tensor(class_labels)
            if lab.dtype.is_floating_point or lab.dtype == torch.bool:
                raise ValueError(f"class_labels must be integers, got {lab.dtype}")
            lab = lab.to(torch.int64).reshape(-1)
        if lab.numel() == 1:
            lab = lab.expand(batch)
        elif lab.numel() != batch:
            raise ValueError(f"class_labels has {lab.numel()} entries for a batch of {batch}")
        if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= n):
            raise ValueError(f"class_labels must lie in [0, {n}), got {int(lab.min())} .. {int(lab.max())}")
        return lab.contiguous()

    @torch.no_grad()
    def __call__(self, sample: torch.Tensor, timestep: Union[torch.Tensor, float, int],
                 class_labels=None, return_dict: bool = True):
        # (before the handle: the two ValueErrors are diffusers' and need no GPU; a malformed sample is refused below)
        labels = self._labels_host(class_labels, sample.shape[0]) if sample.dim() == 4 else None
        h = self.handle
        if sample.device != self._device:
            raise RuntimeError(f"sample is on {sample.device} but the model is on {self._device}")
        if sample.dim() != 4 or sample.shape[1] != self.config.in_channels:
            raise ValueError(f"sample must be [B,{self.config.in_channels},H,W], got {tuple(sample.shape)}")
        x = sample.to(torch.float32).contiguous()
        B, _, H, W = x.shape
        t = self._timesteps_host(timestep, B)
        out = ops.empty((B, self.config.out_channels, H, W), dtype=torch.float32, device=x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        lab = C.cast(labels.data_ptr(), _lib.c_int64_p) if labels is not None else None
        if self.training and self.config.dropout > 0 and not self._train_begun:
            raise RuntimeError(f"training-mode call of a model with dropout={self.config.dropout} but no optimizer: dropout is "
                               "applied by the tape-recording forward, which needs the gradient arenas a HipAdam creates; "
                               "create the optimizer first, or call model.eval() for an undropped prediction")
        if self.training and self._train_begun:
            # training mode with an optimizer: the same kernels, every activation kept for loss.backward()
            fn = "sisic_unet_train_forward" if labels is None else "sisic_unet_train_forward_cond"
            labs = () if labels is None else (lab,)           # the one argument the conditional entry point takes more
            check(getattr(_lib.load(), fn)(h, x.data_ptr(), C.cast(t.data_ptr(), _lib.c_int64_p), *labs, out.data_ptr(), B, H, W,
                                           stream))
            out._sisic_model = self
            # the tape refers to the input by address (conv_in's weight gradient reads it in the backward pass): keep the
            # tensor alive until the next forward, as autograd's graph would
            self._tape_input = x
        elif labels is not None:
            check(_lib.load().sisic_unet_forward_cond(h, x.data_ptr(), C.cast(t.data_ptr(), _lib.c_int64_p), lab,
                                                      out.data_ptr(), B, H, W, stream))
        else:
            check(_lib.load().sisic_unet_forward(h, x.data_ptr(), C.cast(t.data_ptr(), _lib.c_int64_p), out.data_ptr(),
                                                 B, H, W, stream))
        if not return_dict:
            return (out,)
        return UNet2DOutput(sample=out)

    forward = __call__
