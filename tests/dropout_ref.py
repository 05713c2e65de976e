"""CPU restatement of the UNet with ResnetBlock2D dropout (test infrastructure only).

oracle/unet.py restates the published ``UNet2DModel`` at ``dropout=0`` and has no hook for a mask, so the forward is restated
here over ITS OWN pieces (``timestep_embedding``, ``group_norm``, ``attention_block``) with a residual block of this file that
adds the one line of ``ResnetBlock2D.forward`` the oracle leaves out:

    hidden_states = self.norm2(hidden_states); hidden_states = self.nonlinearity(hidden_states)
    hidden_states = self.dropout(hidden_states)                       # <- here
    hidden_states = self.conv2(hidden_states)

torch's ``nn.Dropout`` draws from torch's generator; the library draws from the device-noise contract instead (include/sisic.h,
"ResnetBlock2D dropout"), so the mask is restated from the contract text over tests/philox_ref.py: for sample b, block r (0-based,
execution order), element e of the sample's [C,H,W] activation, word e & 3 of the Philox block (seed + b, e >> 2, step = call,
tag = 256 + r) gives u = (word >> 8) * 2^-24; kept iff u >= p in fp32; kept values are multiplied by
inv_keep = fp32(1 / (1 - double(fp32(p)))), dropped ones are +0.  ``test_dropout_cpu.py`` anchors the restatement: at p = 0 it
must ``torch.equal`` ``oracle.unet.unet_forward``.  The conditional variant adds tests/cond_ref.py's one line.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import philox_ref
from oracle import ddpm as oddpm
from oracle import unet as ounet

TAG_BASE = 256
TABLE = "class_embedding.weight"
N_RESNETS = 22          # 8 down, 2 mid, 12 up in the default architecture


def inv_keep(p: float) -> np.float32:
    """fp32(1 / (1 - p)) with p the fp32 the library receives, the quotient formed in double: one rounding"""
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep_mask(p: float, seed: int, call: int, block: int, sample: int, n: int) -> np.ndarray:
    """bool [n]: which of the n elements of one sample's activation are kept"""
    bits = philox_ref.noise_bits((int(seed) + int(sample)) & 0xFFFFFFFFFFFFFFFF, int(call), TAG_BASE + int(block), n)[:n]
    u = (bits >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def dropout(a: torch.Tensor, p: float, seed: int, call: int, block: int) -> torch.Tensor:
    """a [B,C,H,W] -> kept values times inv_keep, dropped values +0 (differentiable in a)"""
    B = a.shape[0]
    n = a[0].numel()
    keep = np.stack([keep_mask(p, seed, call, block, b, n) for b in range(B)]).reshape(tuple(a.shape))
    scaled = a * torch.tensor(float(inv_keep(p)), dtype=a.dtype)
    return torch.where(torch.from_numpy(keep), scaled, torch.zeros_like(a))


def resnet_block(sd: Dict[str, torch.Tensor], pfx: str, x: torch.Tensor, temb_act: torch.Tensor, p: float, seed: int, call: int,
                 block: int) -> torch.Tensor:
    """ResnetBlock2D with its dropout: out = shortcut(x) + conv2(dropout(silu(norm2(conv1(silu(norm1(x))) + temb))))"""
    h = ounet.group_norm(x, sd[f"{pfx}.norm1.weight"], sd[f"{pfx}.norm1.bias"], True)
    h = F.conv2d(h, sd[f"{pfx}.conv1.weight"], sd[f"{pfx}.conv1.bias"], padding=1)
    t = F.linear(temb_act, sd[f"{pfx}.time_emb_proj.weight"], sd[f"{pfx}.time_emb_proj.bias"])
    h = h + t[:, :, None, None]
    h = ounet.group_norm(h, sd[f"{pfx}.norm2.weight"], sd[f"{pfx}.norm2.bias"], True)
    if p > 0:
        h = dropout(h, p, seed, call, block)
    h = F.conv2d(h, sd[f"{pfx}.conv2.weight"], sd[f"{pfx}.conv2.bias"], padding=1)
    if f"{pfx}.conv_shortcut.weight" in sd:
        x = F.conv2d(x, sd[f"{pfx}.conv_shortcut.weight"], sd[f"{pfx}.conv_shortcut.bias"])
    return x + h


def unet_forward(sd: Dict[str, torch.Tensor], sample: torch.Tensor, timestep, class_labels=None, p: float = 0.0, seed: int = 0,
                 call: int = 0) -> torch.Tensor:
    """The training-mode ``UNet2DModel(dropout=p).__call__(sample, timestep[, class_labels]).sample`` on the CPU, its masks those
    of tape-recording forward ``call`` of a handle seeded with ``seed``."""
    B = sample.shape[0]
    t = ounet._broadcast_t(timestep, B)
    temb = ounet.timestep_embedding(t)
    temb = F.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    temb = F.silu(temb)
    temb = F.linear(temb, sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    if class_labels is not None:
        labels = torch.as_tensor(class_labels).to(torch.int64).reshape(-1)
        labels = labels.expand(B) if labels.numel() == 1 else labels.reshape(B)
        temb = temb + sd[TABLE][labels]
    temb_act = F.silu(temb)

    blocks = iter(range(N_RESNETS))

    def res(pfx, x):
        return resnet_block(sd, pfx, x, temb_act, p, seed, call, next(blocks))

    x = F.conv2d(sample, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    skips: List[torch.Tensor] = [x]
    n = len(ounet.BLOCK_OUT_CHANNELS)
    for i in range(n):
        for j in range(ounet.LAYERS_PER_BLOCK):
            x = res(f"down_blocks.{i}.resnets.{j}", x)
            if ounet.DOWN_HAS_ATTN[i]:
                x = ounet.attention_block(sd, f"down_blocks.{i}.attentions.{j}", x)
            skips.append(x)
        if i != n - 1:
            q = f"down_blocks.{i}.downsamplers.0.conv"
            x = F.conv2d(x, sd[f"{q}.weight"], sd[f"{q}.bias"], stride=2, padding=1)
            skips.append(x)
    x = res("mid_block.resnets.0", x)
    x = ounet.attention_block(sd, "mid_block.attentions.0", x)
    x = res("mid_block.resnets.1", x)
    for i in range(n):
        for j in range(ounet.LAYERS_PER_BLOCK + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            x = res(f"up_blocks.{i}.resnets.{j}", x)
            if ounet.UP_HAS_ATTN[i]:
                x = ounet.attention_block(sd, f"up_blocks.{i}.attentions.{j}", x)
        if i != n - 1:
            q = f"up_blocks.{i}.upsamplers.0.conv"
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = F.conv2d(x, sd[f"{q}.weight"], sd[f"{q}.bias"], padding=1)
    assert not skips and next(blocks, None) is None
    x = ounet.group_norm(x, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], True)
    return F.conv2d(x, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def loss_and_grads(sd: Dict[str, torch.Tensor], images: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor,
                   class_labels=None, p: float = 0.0, seed: int = 0, call: int = 0
                   ) -> Tuple[float, "OrderedDict[str, torch.Tensor]", torch.Tensor]:
    """(loss, {name: d loss / d parameter}, noise_pred) of one training batch under dropout, as oracle.train.loss_and_grads."""
    params = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in sd.items())
    noisy = oddpm.DDPMSchedulerOracle().add_noise(images, noise, timesteps)
    with torch.enable_grad():
        pred = unet_forward(params, noisy, timesteps, class_labels, p, seed, call)
        loss = F.mse_loss(pred, noise)
        grads = torch.autograd.grad(loss, list(params.values()))
    return float(loss.detach()), OrderedDict((k, g.detach()) for k, g in zip(params, grads)), pred.detach()
