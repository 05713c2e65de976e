"""CPU restatement of the class-conditional UNet and of classifier-free guidance (test infrastructure only).

oracle/unet.py is the functional restatement of the unconditional ``UNet2DModel`` and has no hook for a class embedding, so
the forward is restated here over ITS OWN pieces (``timestep_embedding``, ``resnet_block``, ``attention_block``,
``group_norm``) with the one line a conditional ``UNet2DModel.forward`` adds:

    emb = self.time_embedding(t_emb)
    emb = emb + self.class_embedding(class_labels)            # nn.Embedding(num_class_embeds, time_embed_dim)

and every ResnetBlock2D then consumes ``time_emb_proj(silu(emb))`` as before.  ``test_cond_cpu.py`` anchors the restatement:
with an all-zero table it must ``torch.equal`` ``oracle.unet.unet_forward``.

Beside it: loss and gradients by autograd (as ``oracle.train.loss_and_grads``), the guidance combine in numpy float32 as three
separate operations, the label-dropout draw of ``train.train_conditional``, and a guided chain over the DPM-Solver++
restatement (tests/dpmpp_ref.py).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ddpm as oddpm
from oracle import unet as ounet

TABLE = "class_embedding.weight"


def unet_forward(sd: Dict[str, torch.Tensor], sample: torch.Tensor, timestep, class_labels) -> torch.Tensor:
    """``UNet2DModel(num_class_embeds=N).__call__(sample, timestep, class_labels).sample`` on the CPU."""
    B = sample.shape[0]
    t = ounet._broadcast_t(timestep, B)
    labels = torch.as_tensor(class_labels).to(torch.int64).reshape(-1)
    labels = labels.expand(B) if labels.numel() == 1 else labels.reshape(B)

    temb = ounet.timestep_embedding(t)
    temb = F.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    temb = F.silu(temb)
    temb = F.linear(temb, sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    temb = temb + sd[TABLE][labels]                       # the class embedding's row of each sample
    temb_act = F.silu(temb)

    x = F.conv2d(sample, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    skips: List[torch.Tensor] = [x]
    n = len(ounet.BLOCK_OUT_CHANNELS)
    for i in range(n):
        for j in range(ounet.LAYERS_PER_BLOCK):
            x = ounet.resnet_block(sd, f"down_blocks.{i}.resnets.{j}", x, temb_act)
            if ounet.DOWN_HAS_ATTN[i]:
                x = ounet.attention_block(sd, f"down_blocks.{i}.attentions.{j}", x)
            skips.append(x)
        if i != n - 1:
            p = f"down_blocks.{i}.downsamplers.0.conv"
            x = F.conv2d(x, sd[f"{p}.weight"], sd[f"{p}.bias"], stride=2, padding=1)
            skips.append(x)
    x = ounet.resnet_block(sd, "mid_block.resnets.0", x, temb_act)
    x = ounet.attention_block(sd, "mid_block.attentions.0", x)
    x = ounet.resnet_block(sd, "mid_block.resnets.1", x, temb_act)
    for i in range(n):
        for j in range(ounet.LAYERS_PER_BLOCK + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            x = ounet.resnet_block(sd, f"up_blocks.{i}.resnets.{j}", x, temb_act)
            if ounet.UP_HAS_ATTN[i]:
                x = ounet.attention_block(sd, f"up_blocks.{i}.attentions.{j}", x)
        if i != n - 1:
            p = f"up_blocks.{i}.upsamplers.0.conv"
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = F.conv2d(x, sd[f"{p}.weight"], sd[f"{p}.bias"], padding=1)
    assert not skips
    x = ounet.group_norm(x, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], True)
    return F.conv2d(x, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def loss_and_grads(sd: Dict[str, torch.Tensor], images: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor,
                   class_labels) -> Tuple[float, "OrderedDict[str, torch.Tensor]", torch.Tensor]:
    """(loss, {name: d loss / d parameter}, noise_pred) of one conditional training batch, as oracle.train.loss_and_grads."""
    params = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in sd.items())
    noisy = oddpm.DDPMSchedulerOracle().add_noise(images, noise, timesteps)
    with torch.enable_grad():
        pred = unet_forward(params, noisy, timesteps, class_labels)
        loss = F.mse_loss(pred, noise)
        grads = torch.autograd.grad(loss, list(params.values()))
    return float(loss.detach()), OrderedDict((k, g.detach()) for k, g in zip(params, grads)), pred.detach()


def guide(eps_c: np.ndarray, eps_u: np.ndarray, w: float) -> np.ndarray:
    """eps_u + w * (eps_c - eps_u) in float32: subtract, multiply, add, one rounding each"""
    c, u = np.asarray(eps_c, dtype=np.float32), np.asarray(eps_u, dtype=np.float32)
    d = np.subtract(c, u, dtype=np.float32)
    t = np.multiply(np.float32(w), d, dtype=np.float32)
    return np.add(u, t, dtype=np.float32)


def guide_t(eps_c: torch.Tensor, eps_u: torch.Tensor, w: float) -> torch.Tensor:
    return torch.from_numpy(guide(eps_c.numpy(), eps_u.numpy(), w))


def dropout_draw(batch_shape, cond_drop_prob: float, generator: torch.Generator):
    """The per-batch draws of train.train_conditional in their documented order: noise, timesteps, then the dropout mask."""
    noise = torch.randn(batch_shape, generator=generator)
    timesteps = torch.randint(0, 1000, (batch_shape[0],), generator=generator).long()
    drop = torch.rand(batch_shape[0], generator=generator) < cond_drop_prob
    return noise, timesteps, drop


def drop_labels(labels: torch.Tensor, drop: torch.Tensor, null_label: int) -> torch.Tensor:
    return torch.where(drop, torch.full_like(labels, null_label), labels)


def guided_chain(sd: Dict[str, torch.Tensor], solver, x_T: torch.Tensor, labels, null_label: int, w: float,
                 z: Optional[torch.Tensor] = None):
    """``solver.chain`` (a dpmpp_ref.DPMSolverRef) whose eps is the guided combination of two conditional forwards."""
    labels = torch.as_tensor(labels).to(torch.int64)
    null = torch.full_like(labels, int(null_label))

    def eps_fn(x, t):
        with torch.no_grad():
            c = unet_forward(sd, x, t, labels)
            if w == 1.0:
                return c
            return guide_t(c, unet_forward(sd, x, t, null), w)

    return solver.chain(eps_fn, x_T, z)
