"""CPU checks of the references, operands and bars that test_gpu_wide_heads.py holds the d = 32 / 64 attention kernels to.

  * tests/wide_head_ref.py at d = 8 IS tests/trained_like.py, bit for bit, on the operands of test_attention_peaky;
  * at d = 32 and 64 the peaky operands have what they are there for (|score| 90 - 150, peaked rows beside ordinary ones, two
    exact ties, a dominant last key), and the saturated rows' float64 dQ vanishes;
  * the two most likely real mistakes -- the d = 8 scale, the heads cut as C / 8 heads of 8 -- evaluated in float64 miss the GPU
    test's bars by more than 100 x on its own operands, in out and in at least one of dQ, dK, dV: the bars can see them;
  * HipUNet2DModel(attention_head_dim = 32 | 64) constructs with the state dict of arch.unet_param_spec, anything outside
    {8, 32, 64} stays NotImplementedError;
  * E and F's identically vanishing gradients are exactly their to_k.bias.
"""
import pytest
import torch

import arch_ref
import trained_like as tl
import wide_head_ref as wh

KTOL = 1e-5
KERNEL_FACTOR = 8.0


# ---------------------------------------------------------------- d = 8: trained_like's bits
@pytest.mark.parametrize("B,C,N", [(2, 64, 33), (2, 64, 256), (2, 64, 300), (1, 64, 513), (32, 256, 64), (32, 256, 300)])
def test_at_head_dim_8_the_helpers_are_trained_likes(B, C, N):
    seed = 4000 + N + B
    qkv = wh.peaky_qkv(B, C, N, 8, seed)
    assert torch.equal(qkv, tl.peaky_qkv(B, C, N, seed))
    idx = [0, B // 2, B - 1] if B > 2 else list(range(B))          # the images test_attention_peaky evaluates
    sub = qkv[idx]
    with torch.no_grad():
        assert torch.equal(wh.attention_ref(sub, 8), tl.attention_ref(sub))
        assert torch.equal(wh.attention_ref(sub.double(), 8), tl.attention_ref(sub.double()))
    for a, b in zip(wh.attention_rows(sub, 8), tl.attention_rows(sub)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- d = 32, 64: the peaky operands
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("case", range(6))
def test_peaky_operands_have_what_they_are_there_for(d, case):
    B, C, N = wh.peaky_shapes(d)[case]
    qkv = wh.peaky_qkv(B, C, N, d, wh.peaky_seed(d, B, N))
    share = wh.check_rows(qkv, N, d)
    dO = torch.randn(B, C, N, generator=torch.Generator().manual_seed(5100 + N + d))
    x = qkv.double().requires_grad_(True)
    wh.attention_ref(x, d).backward(dO.double())
    dq = x.grad[:, :C].reshape(B, C // d, d, N)
    sat = dq[..., 1].abs().max().item() / dq.abs().max().item()
    print(f"d={d} B={B} C={C} N={N}: share of peaked rows {share:.2f}, saturated row dQ / max dQ {sat:.1e}")
    assert sat <= 1e-6


# ---------------------------------------------------------------- planted errors against the GPU test's bars
def _bar(ref64, ref32, peaky):
    floor = KTOL * max(1.0, ref64.abs().max().item())
    return max(floor, KERNEL_FACTOR * (ref32.double() - ref64).abs().max().item()) if peaky else floor


def _out_and_grads(fn, qkv, dO):
    x = qkv.requires_grad_(True)
    o = fn(x)
    o.backward(dO.to(o.dtype))
    return [o.detach(), x.grad]


@pytest.mark.parametrize("peaky", [False, True], ids=["ordinary", "peaky"])
@pytest.mark.parametrize("mutant", ["scale_of_8", "heads_of_8"])
@pytest.mark.parametrize("d", [32, 64])
def test_the_bars_see_the_two_likely_mistakes(d, mutant, peaky):
    B, C, N = 2, 2 * d, 100
    qkv = wh.peaky_qkv(B, C, N, d, wh.peaky_seed(d, B, N)) if peaky else wh.ordinary_qkv(B, C, N, d)
    dO = torch.randn(B, C, N, generator=torch.Generator().manual_seed(5100 + N + d))
    o64, g64 = _out_and_grads(lambda x: wh.attention_ref(x, d), qkv.double(), dO)
    o32, g32 = _out_and_grads(lambda x: wh.attention_ref(x, d), qkv.clone(), dO)
    if mutant == "scale_of_8":      # d heads, 8^-1/2 in place of d^-1/2: the scores times sqrt(d / 8)
        def wrong(x):
            scaled = torch.cat([x[:, :C] * (d / 8.0) ** 0.5, x[:, C:]], dim=1)
            return wh.attention_ref(scaled, d)
    else:                           # C / 8 heads of 8 channels
        wrong = lambda x: wh.attention_ref(x, 8)
    ow, gw = _out_and_grads(wrong, qkv.double(), dO)
    ratio_out = (ow - o64).abs().max().item() / _bar(o64, o32, peaky)
    ratios = []
    for part in range(3):
        sl = slice(part * C, (part + 1) * C)
        ratios.append((gw[:, sl] - g64[:, sl]).abs().max().item() / _bar(g64[:, sl], g32[:, sl], peaky))
    print(f"d={d} {mutant} {'peaky' if peaky else 'ordinary'}: error / bar out {ratio_out:.0f}, dQ dK dV {[round(r) for r in ratios]}")
    assert ratio_out > 100.0 and max(ratios) > 100.0


# ---------------------------------------------------------------- the Python surface
@pytest.mark.parametrize("name", ["E", "F"])
def test_model_constructs_at_32_and_64_channels_per_head(name):
    from synt_isic_amd.arch import unet_param_spec
    from synt_isic_amd.unet import HipUNet2DModel
    from synt_isic_amd.weights import synthetic_unet_state_dict
    cfg = wh.ARCHS_WIDE[name]
    assert cfg.attention_head_dim == {"E": 32, "F": 64}[name]
    model = HipUNet2DModel(**wh.unet_kwargs(cfg))
    assert model.config == cfg
    model.load_state_dict(synthetic_unet_state_dict(cfg=cfg))
    spec = unet_param_spec(cfg)
    sd = model.state_dict()
    assert list(sd) == list(spec)
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    assert sum(k.endswith("to_k.bias") for k in spec) == {"E": 7, "F": 6}[name]


@pytest.mark.parametrize("d", [16, 24, 128, 0])
def test_other_head_dims_stay_not_implemented(d):
    from synt_isic_amd.unet import HipUNet2DModel
    with pytest.raises(NotImplementedError, match="8, 32 or 64"):
        HipUNet2DModel(**dict(wh.unet_kwargs(wh.ARCHS_WIDE["E"]), attention_head_dim=d))


def test_attention_width_must_divide_by_the_head_dim():
    """(64, 128) with attention at the 64-wide level cannot have 128 channels per head... nor 64 at a 96-wide one"""
    from synt_isic_amd.unet import HipUNet2DModel
    kw = dict(wh.unet_kwargs(wh.ARCHS_WIDE["E"]), block_out_channels=(96, 192), attention_head_dim=64)
    with pytest.raises(ValueError, match="attention_head_dim"):
        HipUNet2DModel(**kw)
    # a level without attention may have any width: F's 64-wide level 0 under 64 per head, and 96 under 64
    HipUNet2DModel(**dict(wh.unet_kwargs(wh.ARCHS_WIDE["F"]), block_out_channels=(96, 128, 128)))


# ---------------------------------------------------------------- E and F: the vanishing gradients
@pytest.mark.parametrize("name", ["E", "F"])
def test_vanishing_gradients_are_the_key_biases(name):
    from synt_isic_amd.weights import synthetic_unet_state_dict
    cfg = wh.ARCHS_WIDE[name]
    sd = synthetic_unet_state_dict(cfg=cfg)
    x, target, t = wh.batch(name, wh.SHAPES_WIDE[name][0])
    _, grads, _ = arch_ref.loss_and_grads(cfg, sd, x, target, t, dtype=torch.float64)
    top = max(g.abs().max().item() for g in grads.values())
    vanishing = [k for k, g in grads.items() if g.abs().max().item() <= 1e-10 * top]
    assert vanishing == wh.vanishing_set(name)
    assert len(vanishing) == {"E": 7, "F": 6}[name]
