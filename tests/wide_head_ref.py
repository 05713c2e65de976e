"""Attention references and operands at any head dimension, and the two architectures with 32 and 64 channels per head
(imported by test_wide_head_cpu.py and test_gpu_wide_heads.py, as trained_like / arch_ref are).

``attention_ref``, ``attention_rows`` and ``peaky_qkv`` are ``trained_like``'s three functions with the head dimension as a
parameter -- the same torch calls in the same order, so that at d = 8 they return ``trained_like``'s bits
(test_wide_head_cpu.py pins that).  Everything here is host-side torch.

  E  (64, 128), one layer, attention everywhere, 32 groups, 32 channels per head      2x16x16, 2x20x12
       2 and 4 heads over 256, 64, 240 and 60 tokens
  F  (64, 128, 128), two layers, attention at level 1, 32 groups, 64 per head         2x32x32, 1x80x72
       2 heads; at 1x80x72 level 1 is 40x36 = 1440 tokens, past the 1170 of the d = 8 backward pass
"""
from collections import OrderedDict

import torch

import arch_ref
from synt_isic_amd.arch import UNetConfig, unet_param_spec


def attention_ref(qkv, d):
    """softmax(q k^T / sqrt(d)) v of qkv [B, 3C, N] in qkv's own dtype -> [B, C, N]; differentiable"""
    B, C3, N = qkv.shape
    C = C3 // 3
    q, k, v = (t.reshape(B, C // d, d, N).transpose(2, 3) for t in qkv.chunk(3, dim=1))
    p = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1)
    return (p @ v).transpose(2, 3).reshape(B, C, N)


def attention_rows(qkv, d):
    """(scores [B, heads, N, N], probabilities) in float64"""
    B, C3, N = qkv.shape
    C = C3 // 3
    q, k, _ = (t.reshape(B, C // d, d, N).transpose(2, 3) for t in qkv.double().chunk(3, dim=1))
    s = q @ k.transpose(-1, -2) * d ** -0.5
    return s, torch.softmax(s, dim=-1)


def peaky_qkv(B, C, N, d, seed, peak=125.0):
    """trained_like.peaky_qkv for C / d heads of d channels: fp32 qkv [B, 3C, N] whose largest |score| is ``peak``; odd queries
    6 x, every fourth key 5 x a normal draw; a dominant last key that queries 1 and N - 2 point along (saturated rows); key N // 3
    and its exact copy at (N // 3 + N // 2) % N, which queries 3 and N // 2 point along (two exactly tied top scores)"""
    g = torch.Generator().manual_seed(int(seed))
    heads = C // d
    t = torch.randn(B, 3, heads, d, N, generator=g, dtype=torch.float64)
    q, k = t[:, 0], t[:, 1]
    q[..., 1::2] *= 6.0
    k[..., 3::4] *= 5.0
    last, src, dup = N - 1, N // 3, (N // 3 + N // 2) % N
    assert len({last, src, dup}) == 3 and N >= 8
    others = torch.ones(N, dtype=torch.bool)
    others[[last, src, dup]] = False
    top = k[..., others].norm(dim=-2).amax(-1)                        # [B, heads]
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)
    u_last = unit(k[..., last])
    u_src = unit(k[..., src] - (k[..., src] * u_last).sum(-1, keepdim=True) * u_last)      # orthogonal to the last key
    k[..., last] = u_last * (1.5 * top)[..., None]
    k[..., src] = u_src * (1.25 * top)[..., None]
    k[..., dup] = k[..., src]
    for i, u in ((1, u_last), (N - 2, u_last), (3, u_src), (N // 2, u_src)):
        q[..., i] = u * q[..., i].norm(dim=-1, keepdim=True)
    biggest = max((q[b].transpose(-1, -2) @ k[b]).abs().max().item() for b in range(B)) * d ** -0.5
    q *= peak / biggest
    out = t.reshape(B, 3 * C, N).float()
    kk = out[:, C:2 * C]
    kk[..., dup] = kk[..., src]                                       # the copy stays exact after rounding
    return out


def ordinary_qkv(B, C, N, d, scale=1.5):
    """fp32 qkv [B, 3C, N], 1.5 x a standard normal draw seeded by the shape (|score| up to ~ 12)"""
    g = torch.Generator().manual_seed(3000 + 11 * d + 5 * N + B + C)
    return torch.randn(B, 3 * C, N, generator=g) * scale


def check_rows(qkv, N, d):
    """test_gpu_trained_like._check_rows at head dimension d; returns the share of peaked rows"""
    s, p = attention_rows(qkv, d)
    assert 90.0 <= s.abs().max().item() <= 150.0, s.abs().max().item()
    share = (p.amax(-1) > 0.5).double().mean().item()
    assert 0.2 <= share <= 0.9, share
    top2 = s.topk(2, dim=-1).values
    assert (top2[..., 3, 0] == top2[..., 3, 1]).all() and (top2[..., N // 2, 0] == top2[..., N // 2, 1]).all()
    assert (s.argmax(-1)[..., 1] == N - 1).all() and (s.argmax(-1)[..., N - 2] == N - 1).all()
    return share


# (B, C, N) of the peaky forward cases, per head dimension: a single key tile with a tail, ragged blocks, a last block of one
# key (513 = 8 x 64 + 1: the dominant one), one head over 1300 and 2048 tokens
def peaky_shapes(d):
    return [(2, 2 * d, 33), (2, 2 * d, 100), (2, 2 * d, 300), (1, 2 * d, 513), (1, d, 1300), (1, d, 2048)]


def peaky_seed(d, B, N):
    return 4000 + 7 * d + N + B


def backward_refs(qkv, dO, d):
    """(float64, float32) gradients of sum(attention_ref(qkv, d) * dO) with respect to qkv, by torch.autograd"""
    grads = []
    for dtype in (torch.float64, torch.float32):
        x = qkv.to(dtype).requires_grad_(True)
        attention_ref(x, d).backward(dO.to(dtype))
        grads.append(x.grad)
    return grads


# ---------------------------------------------------------------------------------------------- architectures
ARCHS_WIDE: "OrderedDict[str, UNetConfig]" = OrderedDict([
    ("E", UNetConfig(sample_size=16, in_channels=3, out_channels=3, layers_per_block=1, block_out_channels=(64, 128),
                     down_block_types=arch_ref._types("Down", (1, 1)), up_block_types=arch_ref._types("Up", (1, 1)),
                     norm_num_groups=32, attention_head_dim=32)),
    ("F", UNetConfig(sample_size=32, in_channels=3, out_channels=3, layers_per_block=2, block_out_channels=(64, 128, 128),
                     down_block_types=arch_ref._types("Down", (0, 1, 0)), up_block_types=arch_ref._types("Up", (0, 1, 0)),
                     norm_num_groups=32, attention_head_dim=64)),
])
SHAPES_WIDE = {"E": [(2, 16, 16), (2, 20, 12)], "F": [(2, 32, 32), (1, 80, 72)]}


def unet_kwargs(cfg):
    return dict(arch_ref.unet_kwargs(cfg), attention_head_dim=cfg.attention_head_dim)


def batch(name, shape):
    """arch_ref.batch for E and F: x ~ N(0,1), target ~ N(0,1) in the output shape, timesteps [0, 500, 999][:B]"""
    cfg = ARCHS_WIDE[name]
    B, H, W = shape
    g = torch.Generator().manual_seed(9000 + 131 * (ord(name) - ord("A")) + 17 * H + W + B)
    x = torch.randn(B, cfg.in_channels, H, W, generator=g)
    target = torch.randn(B, cfg.out_channels, H, W, generator=g)
    return x, target, torch.tensor(arch_ref.TIMESTEPS[:B])


def vanishing_set(name):
    """every ``to_k.bias`` (softmax is invariant to a shift of a row's scores), in state-dict order: 7 in E, 6 in F"""
    return [k for k in unet_param_spec(ARCHS_WIDE[name]) if k.endswith("to_k.bias")]
