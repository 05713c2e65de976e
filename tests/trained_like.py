"""Trained-like weights and operands (imported by the test modules, as philox_ref / ddim_ref are).

``synthetic_unet_state_dict`` is an initialisation-like draw: conv / linear weights U(+-1/sqrt(fan_in)), GroupNorm gamma
1 + 0.1 N, beta 0.1 N.  Under it every attention row of the network is a uniform average (max_j P_ij ~ 2/N, |score| < 4),
every gamma is positive and near 1, no channel's mean sits far from its group's and no SiLU saturates.  A checkpoint
out of a training run looks different; ``trained_like_unet_state_dict`` is a deterministic transform of a synthetic state
dict that does:

  * every tensor with dim >= 2 times ``gain`` (sqrt(3): unit-gain layers, the residual stream grows with depth), but
    ``*.to_q.weight`` / ``*.to_k.weight`` times ``qk_gain`` (peaky softmax rows, |score| > 100);
  * every norm weight exp(0.6 N), a random 5 % of the entries with the sign flipped, every 29th entry exactly 0;
  * every norm bias 0.5 N;
  * every conv / linear bias times 4, and in biases of >= 64 entries every 37th entry +-6 (outlier channels whose |mean|
    is far above the std inside their group);
  * all draws from one ``torch.Generator().manual_seed(seed)`` walking the state dict in order.

The operand generators below build the kernel-level cases of test_gpu_trained_like.py: peaky q/k/v (with exactly tied
top scores and a dominant last key), gamma / beta with zeros, negatives and a log-normal spread, x with per-channel
offsets of ~30 std, an exactly constant group.  Everything here is host-side torch; nothing touches a GPU.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

HEAD_DIM = 8
ATT_SCALE = HEAD_DIM ** -0.5


def _is_norm(name: str) -> bool:
    return "norm" in name.rsplit(".", 1)[0].rsplit(".", 1)[-1]


def trained_like_unet_state_dict(sd, seed: int = 7, qk_gain: float = 6.0, gain: float = math.sqrt(3.0)):
    g = torch.Generator().manual_seed(int(seed))
    out = OrderedDict()
    for name, t in sd.items():
        kind = name.rsplit(".", 1)[1]
        if t.dim() >= 2:
            qk = name.endswith(".to_q.weight") or name.endswith(".to_k.weight")
            out[name] = t * (qk_gain if qk else gain)
        elif _is_norm(name) and kind == "weight":
            w = torch.exp(0.6 * torch.randn(t.shape, generator=g))
            flip = torch.rand(t.shape, generator=g) < 0.05
            w = torch.where(flip, -w, w)
            w[::29] = 0.0
            out[name] = w.to(t.dtype)
        elif _is_norm(name):
            out[name] = (0.5 * torch.randn(t.shape, generator=g)).to(t.dtype)
        else:                                                # conv / linear bias
            b = t * 4.0
            if b.numel() >= 64:
                n = b[::37].numel()
                b[::37] = torch.where(torch.rand(n, generator=g) < 0.5, -6.0, 6.0)
            out[name] = b
    return out


# ---------------------------------------------------------------------------------------------- attention
def attention_blocks(sd):
    """prefixes of the six attention blocks, in forward order"""
    return [n[:-len(".to_q.weight")] for n in sd if n.endswith(".to_q.weight")]


def attention_probe(sd, sample, timestep):
    """{attention block: (share of rows with max_j P_ij > 0.5, mean over rows of max_j P_ij, max |score|)} of one oracle
    forward in the dtype of ``sd`` -- the block's own arithmetic (oracle/unet.py attention_block) restated on its input"""
    from oracle import unet as ounet
    stats = OrderedDict()
    orig = ounet.attention_block

    def probed(sd_, p, x):
        B, C, H, W = x.shape
        heads = C // HEAD_DIM
        h = ounet.group_norm(x.reshape(B, C, H * W), sd_[f"{p}.group_norm.weight"], sd_[f"{p}.group_norm.bias"], False)
        h = h.transpose(1, 2)
        split = lambda z: z.reshape(B, H * W, heads, HEAD_DIM).transpose(1, 2)
        q = split(F.linear(h, sd_[f"{p}.to_q.weight"], sd_[f"{p}.to_q.bias"]))
        k = split(F.linear(h, sd_[f"{p}.to_k.weight"], sd_[f"{p}.to_k.bias"]))
        s = torch.matmul(q, k.transpose(-1, -2)) * ATT_SCALE
        pmax = torch.softmax(s, dim=-1).amax(-1)
        stats[p] = ((pmax > 0.5).double().mean().item(), pmax.mean().item(), s.abs().max().item())
        return orig(sd_, p, x)

    ounet.attention_block = probed
    try:
        with torch.no_grad():
            ounet.unet_forward(sd, sample, timestep)
    finally:
        ounet.attention_block = orig
    return stats


def attention_ref(qkv):
    """softmax(q k^T / sqrt(8)) v of qkv [B, 3C, N] in qkv's own dtype (float64: the reference; float32: the same formula
    at the kernels' precision) -> [B, C, N]; differentiable"""
    B, C3, N = qkv.shape
    C = C3 // 3
    q, k, v = (t.reshape(B, C // HEAD_DIM, HEAD_DIM, N).transpose(2, 3) for t in qkv.chunk(3, dim=1))
    p = torch.softmax(q @ k.transpose(-1, -2) * ATT_SCALE, dim=-1)
    return (p @ v).transpose(2, 3).reshape(B, C, N)


def attention_rows(qkv):
    """(scores [B, heads, N, N], probabilities) in float64"""
    B, C3, N = qkv.shape
    C = C3 // 3
    q, k, _ = (t.reshape(B, C // HEAD_DIM, HEAD_DIM, N).transpose(2, 3) for t in qkv.double().chunk(3, dim=1))
    s = q @ k.transpose(-1, -2) * ATT_SCALE
    return s, torch.softmax(s, dim=-1)


def peaky_qkv(B, C, N, seed, peak=125.0):
    """fp32 qkv [B, 3C, N] whose largest |score| is ``peak``, ordinary rows mixed in:

      * odd queries are 6 x, every fourth key 5 x a standard normal draw: sharp rows next to ordinary ones;
      * the last key (in the last, partly filled key block when N is no multiple of the block) has 1.5 x the largest other
        key norm of its head, and queries 1 and N - 2 point along it: it dominates their rows, which saturate;
      * key N // 3 has 1.25 x that norm, is orthogonal to the last key, and key (N // 3 + N // 2) % N is a copy of it;
        queries 3 and N // 2 point along it: two exactly tied top scores;
      * q as a whole is then scaled so that max |score| = peak."""
    g = torch.Generator().manual_seed(int(seed))
    heads = C // HEAD_DIM
    t = torch.randn(B, 3, heads, HEAD_DIM, N, generator=g, dtype=torch.float64)
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
    biggest = max((q[b].transpose(-1, -2) @ k[b]).abs().max().item() for b in range(B)) * ATT_SCALE
    q *= peak / biggest
    out = t.reshape(B, 3 * C, N).float()
    kk = out[:, C:2 * C]
    kk[..., dup] = kk[..., src]                                       # the copy stays exact after rounding
    return out


# ---------------------------------------------------------------------------------------------- GroupNorm
def wild_affine(C, seed, reach=40.0):
    """(gamma, beta) fp32 [C]: gamma exp(0.6 N) with ~5 % (at least one) negative and every 29th entry 0, beta 0.5 N; two
    channels carry beta = +-reach under a small gamma (SiLU saturated both ways whatever x does) and two gamma = +-reach/3"""
    g = torch.Generator().manual_seed(int(seed))
    gamma = torch.exp(0.6 * torch.randn(C, generator=g))
    flip = torch.rand(C, generator=g) < 0.05
    flip[7] = True
    gamma = torch.where(flip, -gamma, gamma)
    gamma[::29] = 0.0
    beta = 0.5 * torch.randn(C, generator=g)
    gamma[5], beta[5] = 0.25, reach + 2.0
    gamma[6], beta[6] = 0.25, -(reach + 2.0)
    gamma[10], gamma[11] = reach / 3.0, -reach / 3.0
    return gamma, beta


def offset_x(B, C, H, W, seed, groups=32, offset=30.0, constant=(0, 3, 3.25)):
    """fp32 x [B, C, H, W]: unit noise plus a per-channel offset of ``offset`` N (channels of one group sit ~30 std of their
    own noise apart); group ``constant[1]`` of image ``constant[0]`` holds exactly ``constant[2]`` everywhere (variance 0:
    rstd = 1 / sqrt(eps))"""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(B, C, H, W, generator=g) + offset * torch.randn(1, C, 1, 1, generator=g)
    if constant is not None:
        b, grp, val = constant
        cpg = C // groups
        x[b, grp * cpg:(grp + 1) * cpg] = val
    return x


def gn_scale_shift(x, gamma, beta, groups=32, eps=1e-5):
    """the per-(image, channel) pair the convolution prologues read: a = x * scale + shift = GroupNorm(x); fp32, computed in
    float64 from the fp32 operands"""
    B, C = x.shape[:2]
    xg = x.double().reshape(B, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    cpg = C // groups
    scale = gamma.double()[None] * rstd.repeat_interleave(cpg, 1)
    shift = beta.double()[None] - mean.repeat_interleave(cpg, 1) * scale
    return scale.float(), shift.float()


# ---------------------------------------------------------------------------------------------- float64 restatement
# The backward formulas the HIP kernels implement (train_kernels.hip: attention_bwd_kernel, gn_bwd_*), spelled in float64
# with the two places a kernel could be subtly wrong made switchable.  Unmutated it reproduces torch.autograd over the oracle.
MUTANTS = (None, "attention_without_D", "groupnorm_abs_gamma")


def _attention_core(mutant):
    class Core(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q, k, v):                      # [B, heads, N, d]
            p = torch.softmax(q @ k.transpose(-1, -2) * ATT_SCALE, dim=-1)
            o = p @ v
            ctx.save_for_backward(q, k, v, p, o)
            return o

        @staticmethod
        def backward(ctx, do):
            q, k, v, p, o = ctx.saved_tensors
            dp = do @ v.transpose(-1, -2)
            D = (do * o).sum(-1, keepdim=True)
            ds = p * (dp if mutant == "attention_without_D" else dp - D)
            return ds @ k * ATT_SCALE, ds.transpose(-1, -2) @ q * ATT_SCALE, p.transpose(-1, -2) @ do
    return Core.apply


def _group_norm(mutant, groups, eps):
    class GN(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            B, C = x.shape[:2]
            xg = x.reshape(B, groups, -1)
            mean, var = xg.mean(-1, keepdim=True), xg.var(-1, unbiased=False, keepdim=True)
            rstd = (var + eps).rsqrt()
            xh = ((xg - mean) * rstd).reshape(x.shape)
            ctx.save_for_backward(xh, rstd, w)
            bc = (1, C) + (1,) * (x.dim() - 2)
            return xh * w.reshape(bc) + b.reshape(bc)

        @staticmethod
        def backward(ctx, du):
            xh, rstd, w = ctx.saved_tensors
            B, C = xh.shape[:2]
            bc = (1, C) + (1,) * (xh.dim() - 2)
            red = (0,) + tuple(range(2, xh.dim()))
            gm = (w.abs() if mutant == "groupnorm_abs_gamma" else w).reshape(bc)
            gdu = (gm * du).reshape(B, groups, -1)
            xg = xh.reshape(B, groups, -1)
            dx = rstd * (gdu - gdu.mean(-1, keepdim=True) - xg * (gdu * xg).mean(-1, keepdim=True))
            return dx.reshape(xh.shape), (du * xh).sum(red), du.sum(red)
    return GN.apply


def restated_loss_and_grads(sd, images, noise, timesteps, mutant=None):
    """oracle.train.loss_and_grads(..., dtype=float64) with attention and GroupNorm differentiated by the formulas above
    instead of by torch.autograd; ``mutant`` (one of MUTANTS) plants one error in one backward formula"""
    from oracle import train as otrain
    from oracle import unet as ounet
    assert mutant in MUTANTS
    core = _attention_core(mutant)
    gn = _group_norm(mutant, ounet.NORM_GROUPS, ounet.NORM_EPS)

    def group_norm(x, w, b, silu):
        y = gn(x, w, b)
        return F.silu(y) if silu else y

    def attention_block(sd_, p, x):
        B, C, H, W = x.shape
        heads = C // HEAD_DIM
        h = group_norm(x.reshape(B, C, H * W), sd_[f"{p}.group_norm.weight"], sd_[f"{p}.group_norm.bias"], False)
        h = h.transpose(1, 2)
        split = lambda z: z.reshape(B, H * W, heads, HEAD_DIM).transpose(1, 2)
        o = core(*(split(F.linear(h, sd_[f"{p}.to_{n}.weight"], sd_[f"{p}.to_{n}.bias"])) for n in "qkv"))
        o = o.transpose(1, 2).reshape(B, H * W, C)
        o = F.linear(o, sd_[f"{p}.to_out.0.weight"], sd_[f"{p}.to_out.0.bias"])
        return o.transpose(1, 2).reshape(B, C, H, W) + x

    saved = ounet.group_norm, ounet.attention_block
    ounet.group_norm, ounet.attention_block = group_norm, attention_block
    try:
        return otrain.loss_and_grads(sd, images, noise, timesteps, dtype=torch.float64)
    finally:
        ounet.group_norm, ounet.attention_block = saved


def grad_errors(grads, ref_grads):
    """((worst, name), (median, name)) of max |g - ref| / max |ref| over the tensors whose reference gradient is not
    identically zero -- the measure of test_gpu_train._grad_errors -- and the largest |g| among those that are (to_k.bias)"""
    rel, vanishing = [], 0.0
    for n, r in ref_grads.items():
        scale = r.abs().max().item()
        err = (grads[n].detach().cpu().double() - r.double()).abs().max().item()
        if scale <= 1e-8:
            vanishing = max(vanishing, err)
            continue
        rel.append((err / scale, n))
    rel.sort()
    return rel[-1], rel[len(rel) // 2], vanishing
