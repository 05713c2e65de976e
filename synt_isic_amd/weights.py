"""Seeded synthetic weights (host-side data generation only).

The reference's trained checkpoints ``unet_{CLASS}_best.pth`` are fetched from
Google Drive by download_models.py:15-59 and are not available offline, so
tests, the smoke run and the benchmark use random-initialised weights of the
reference architecture.  The recipe is fixed here once ("fixture descriptor"):

  * one CPU ``torch.Generator`` seeded with ``seed`` walks the tensors in
    ``unet_param_spec`` order;
  * conv / linear weights and biases ~ U(-1/sqrt(fan_in), +1/sqrt(fan_in))
    (the bound torch's default ``kaiming_uniform_(a=sqrt(5))`` produces);
  * GroupNorm weight = 1 + 0.1*N(0,1), bias = 0.1*N(0,1) so the affine part of
    every normalisation is exercised (a default-initialised 1/0 would hide it).

``state_dict_sha256`` fingerprints the result so fixtures can detect drift.
"""
from __future__ import annotations

import dataclasses
import hashlib
import math
from collections import OrderedDict
from typing import Dict, Optional

import torch

from .arch import UNetConfig, unet_param_spec

DEFAULT_WEIGHT_SEED = 1234


def _fill(spec, seed: int) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    fan_in_of_layer: Dict[str, int] = {}
    for name, shape in spec.items():
        layer, kind = name.rsplit(".", 1)
        if len(shape) >= 2:                                   # conv / linear weight
            fan_in = math.prod(shape[1:])
            fan_in_of_layer[layer] = fan_in
            bound = 1.0 / math.sqrt(fan_in)
            sd[name] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound
        elif layer in fan_in_of_layer:                        # bias of the conv / linear just seen
            bound = 1.0 / math.sqrt(fan_in_of_layer[layer])
            sd[name] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound
        elif kind == "weight":                                # norm scale
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
        else:                                                 # norm shift
            sd[name] = 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
    return sd


CLASS_TABLE_SEED_OFFSET = 0x636C73          # the class embedding's own generator is seeded with seed + this


def synthetic_unet_state_dict(seed: int = DEFAULT_WEIGHT_SEED, cfg: UNetConfig = UNetConfig(),
                              num_class_embeds: Optional[int] = None) -> "OrderedDict[str, torch.Tensor]":
    """``num_class_embeds=N`` (or a ``cfg`` that has it) adds ``class_embedding.weight`` ~ N(0,1), nn.Embedding's default
    initialisation, at its place in the state dict.  The table comes from a generator of its own, so the other 330 tensors
    are those of the unconditional call bit for bit (the goldens are computed from them)."""
    if num_class_embeds is not None:
        cfg = dataclasses.replace(cfg, num_class_embeds=num_class_embeds)
    plain = _fill(unet_param_spec(dataclasses.replace(cfg, num_class_embeds=None)), seed)
    if cfg.num_class_embeds is None:
        return plain
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed) + CLASS_TABLE_SEED_OFFSET)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in unet_param_spec(cfg).items():
        sd[name] = plain[name] if name in plain else torch.randn(shape, generator=g, dtype=torch.float32)
    return sd


def state_dict_sha256(sd: Dict[str, torch.Tensor]) -> str:
    h = hashlib.sha256()
    for name, t in sd.items():
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def synthetic_resnet18_state_dict(seed: int = 4321, num_classes: int = 7) -> "OrderedDict[str, torch.Tensor]":
    """Seeded random classifier (``IMAGENET1K_V1`` weights are a network download, XAI.py:389, unavailable
    offline).  Conv/fc ~ U(+-sqrt(3/fan_in)) (unit-gain so activations stay O(1) through 18 layers),
    BatchNorm weight 1+0.1N, bias 0.1N, running_mean 0.1N, running_var 1+0.2|N|."""
    from .arch import resnet18_param_spec
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in resnet18_param_spec(num_classes).items():
        if len(shape) >= 2:
            bound = math.sqrt(3.0 / math.prod(shape[1:]))
            sd[name] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound
        elif name.endswith("running_var"):
            sd[name] = 1.0 + 0.2 * torch.randn(shape, generator=g, dtype=torch.float32).abs()
        elif name.endswith("running_mean") or name.endswith(".bias"):
            sd[name] = 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
        else:
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
    return sd


def default_init_resnet18_state_dict(seed: int = 0, num_classes: int = 7) -> "OrderedDict[str, torch.Tensor]":
    """What an untrained ``torchvision.models.resnet18()`` (fc -> num_classes) holds, from one seeded CPU generator walking the
    tensors in state-dict order: convolution weights kaiming-normal with fan-out and ReLU gain (std = sqrt(2 / (cout k k))),
    BatchNorm gamma 1, beta 0, running statistics (0, 1), and ``nn.Linear``'s default for fc (weight and bias
    U(+-1/sqrt(fan_in))).  The starting point of training from scratch with batch-statistics BatchNorm."""
    from .arch import resnet18_param_spec
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in resnet18_param_spec(num_classes).items():
        if len(shape) == 4:
            std = math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
            sd[name] = torch.randn(shape, generator=g, dtype=torch.float32) * std
        elif name.startswith("model.fc."):
            bound = 1.0 / math.sqrt(512.0)
            sd[name] = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound
        elif name.endswith("running_var") or name.endswith(".weight"):
            sd[name] = torch.ones(shape, dtype=torch.float32)
        else:
            sd[name] = torch.zeros(shape, dtype=torch.float32)
    return sd
