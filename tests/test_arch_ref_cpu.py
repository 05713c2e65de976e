"""tests/arch_ref.py, the config-generic restatement of the UNet, pinned on the CPU (no GPU anywhere in this file).

  * at the default config it IS the oracle: torch.equal to oracle.unet.unet_forward and to oracle.train.loss_and_grads (fp32);
  * for each architecture of the GPU tests (arch_ref.ARCHS) it consumes exactly the tensors of arch.unet_param_spec, in the
    order the library's own description gives (sisic_unet_tensor_name: host code, no device is touched);
  * it sees structure: two planted errors -- two equal-width blocks' time_emb_proj exchanged, the first two skip tensors popped
    in exchanged order -- move the float64 prediction by more than 100 times the bar the GPU forward is held to;
  * the tensors whose gradient vanishes identically are exactly arch_ref.vanishing_set: the cap on what the GPU gradient test
    may leave out of its relative measure.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import arch_ref

MODEL_FACTOR = 10.0          # tests/test_gpu_architectures.py holds the library to 10 x the fp32 restatement's own error
NAMES = list(arch_ref.ARCHS)


@pytest.fixture(scope="module")
def evaluated():
    """name -> (sd, batch, float64 (loss, grads, pred), fp32 (loss, grads, pred)) at the first shape of the row, computed once"""
    from synt_isic_amd.weights import synthetic_unet_state_dict
    cache = {}

    def get(name):
        if name not in cache:
            cfg = arch_ref.ARCHS[name]
            sd = synthetic_unet_state_dict(cfg=cfg)
            batch = arch_ref.batch(name, arch_ref.SHAPES[name][0])
            cache[name] = (sd, batch, arch_ref.loss_and_grads(cfg, sd, *batch, dtype=torch.float64),
                           arch_ref.loss_and_grads(cfg, sd, *batch, dtype=torch.float32))
        return cache[name]
    return get


def test_default_config_is_the_oracle_bit_for_bit(synthetic_sd, golden_dir):
    from oracle import ddpm as oddpm
    from oracle import train as otrain
    from oracle import unet as ounet
    from synt_isic_amd.arch import UNetConfig
    cfg = UNetConfig()
    g = np.load(os.path.join(golden_dir, "unet_forward_b2_64.npz"))
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    with torch.no_grad():
        assert torch.equal(arch_ref.unet_forward(cfg, synthetic_sd, x, t), ounet.unet_forward(synthetic_sd, x, t))
    gen = torch.Generator().manual_seed(31)
    images = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
    noise = torch.randn(2, 3, 32, 32, generator=gen)
    ts = torch.tensor([3, 871])
    with torch.no_grad():
        assert torch.equal(arch_ref.unet_forward(cfg, synthetic_sd, images, ts), ounet.unet_forward(synthetic_sd, images, ts))
        assert torch.equal(arch_ref.unet_forward(cfg, synthetic_sd, images, 40), ounet.unet_forward(synthetic_sd, images, 40))
    ref_loss, ref_grads, ref_pred = otrain.loss_and_grads(synthetic_sd, images, noise, ts)
    noisy = oddpm.DDPMSchedulerOracle().add_noise(images, noise, ts)
    loss, grads, pred = arch_ref.loss_and_grads(cfg, synthetic_sd, noisy, noise, ts)
    assert loss == ref_loss and torch.equal(pred, ref_pred)
    assert list(grads) == list(ref_grads) and all(torch.equal(grads[k], ref_grads[k]) for k in grads)
    # the float64 form is the oracle's too: the sinusoid in double from the fp32 table
    sd64 = {k: v.double() for k, v in synthetic_sd.items()}
    with torch.no_grad():
        assert torch.equal(arch_ref.unet_forward(cfg, sd64, images.double(), ts), otrain.unet_forward64(sd64, images.double(), ts))


class _CountingDict(dict):
    """a state dict that records which keys the forward read"""

    def __init__(self, *a):
        super().__init__(*a)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_consumes_exactly_the_spec(name):
    from synt_isic_amd.arch import unet_param_spec
    from synt_isic_amd.weights import synthetic_unet_state_dict
    cfg = arch_ref.ARCHS[name]
    spec = unet_param_spec(cfg)
    sd = _CountingDict(synthetic_unet_state_dict(cfg=cfg))
    assert list(sd) == list(spec) and all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    sd.read.clear()
    B, H, W = arch_ref.SHAPES[name][-1]
    x, _, t = arch_ref.batch(name, (B, H, W))
    with torch.no_grad():
        y = arch_ref.unet_forward(cfg, sd, x, t)
    assert tuple(y.shape) == (B, cfg.out_channels, H, W)
    assert sd.read == set(spec)           # every tensor read, none beyond the spec asked for (a missing key raises)
    # a tensor of another shape is not silently accepted: conv / linear / norm all check their operands
    bad = dict(sd)
    k = next(k for k in spec if k.endswith("resnets.0.conv1.weight"))
    bad[k] = torch.zeros(spec[k][0] + 1, *spec[k][1:])
    with pytest.raises(RuntimeError), torch.no_grad():
        arch_ref.unet_forward(cfg, bad, x, t)


@pytest.mark.parametrize("name", NAMES)
def test_library_describes_the_same_tensors_in_the_same_order(name):
    """sisic_unet_create keeps the context pointer and builds its tensor list on the host (describe() in unet.cpp); it makes
    no device call and does not read the context -- include/sisic.h states this as part of the entry point's contract, and this
    test relies on it: the context here is a zeroed stand-in, so the test fails (or crashes) the day create reads a context
    field.  The handle is NOT destroyed: sisic_unet_destroy synchronises the device, which a test without the gpu mark must not
    touch; what is left behind is a few kilobytes of host memory per architecture."""
    from synt_isic_amd import _lib
    from synt_isic_amd.arch import unet_param_spec
    from synt_isic_amd.unet import timestep_frequencies
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    cfg = arch_ref.ARCHS[name]
    c = _lib.UNetConfigC()
    c.in_channels, c.out_channels, c.layers_per_block = cfg.in_channels, cfg.out_channels, cfg.layers_per_block
    c.n_blocks = len(cfg.block_out_channels)
    for i, ch in enumerate(cfg.block_out_channels):
        c.block_out_channels[i], c.down_attn[i], c.up_attn[i] = ch, int(cfg.down_has_attn[i]), int(cfg.up_has_attn[i])
    c.norm_groups, c.norm_eps, c.head_dim = cfg.norm_num_groups, cfg.norm_eps, cfg.attention_head_dim
    freqs = timestep_frequencies(cfg.block_out_channels[0]).contiguous()
    c.n_freqs, c.freqs = freqs.numel(), C.cast(freqs.data_ptr(), _lib.c_float_p)
    fake_ctx = C.create_string_buffer(4096)
    h = C.c_void_p()
    _lib.check(lib.sisic_unet_create(C.cast(fake_ctx, C.c_void_p), C.byref(c), C.byref(h)))
    names = [lib.sisic_unet_tensor_name(h, i).decode() for i in range(lib.sisic_unet_num_tensors(h))]
    assert names == list(unet_param_spec(cfg))
    assert lib.sisic_unet_tensor_name(h, len(names)) is None


@pytest.mark.parametrize("name", NAMES)
def test_plan_table_tool_walks_every_convolution_of_the_description(name):
    """tools/arch_plan_table.py restates the executor's sequence of convolutions by hand (the table of DESIGN.md section 6 is its
    output).  Tied to the description: per architecture it must list one convolution per conv tensor of unet_param_spec -- which
    the test above ties to the library's own description -- plus two per attention block (the fused q/k/v projection, three
    linear tensors in one launch, and to_out), and convolutions of the spec's channel counts."""
    import sys
    from synt_isic_amd.arch import unet_param_spec
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import arch_plan_table
    finally:
        sys.path.pop(0)
    cfg = arch_ref.ARCHS[name]
    spec = unet_param_spec(cfg)
    conv_tensors = [k for k, s in spec.items() if len(s) == 4]
    attn_blocks = [k for k in spec if k.endswith(".to_q.weight")]
    B, H, W = arch_ref.SHAPES[name][0]
    convs = [c for level in arch_plan_table.walk(cfg, B, H, W).values() for c in level]
    assert len(convs) == len(conv_tensors) + 2 * len(attn_blocks)
    assert not any(p.startswith("REFUSED") for _, p in convs), convs
    # (Cin, Cout, k) of every convolution, as a multiset, against the spec's
    want = sorted([(s[1], s[0], s[2]) for s in (spec[k] for k in conv_tensors)]
                  + [v for k in attn_blocks for v in ((spec[k][1], 3 * spec[k][0], 1), (spec[k][1], spec[k][0], 1))])
    got = []
    for what, _ in convs:
        k, chans = what.split()[0], what.split()[1]
        cin, cout = chans.split("->")
        got.append((sum(int(v) for v in cin.split("+")), int(cout), int(k[0])))
    assert sorted(got) == want


def _swapped_time_projections(cfg, sd):
    """two blocks of equal width whose time_emb_proj tensors (same shapes) change places: the first pair in state-dict order
    (A: down_blocks.0.resnets.0 and up_blocks.2.resnets.0; B and C: the two ResNet blocks of down block 0)"""
    from synt_isic_amd.arch import unet_param_spec
    spec = unet_param_spec(cfg)
    blocks = [k[:-len(".time_emb_proj.weight")] for k in spec if k.endswith(".time_emb_proj.weight")]
    for i, a in enumerate(blocks):
        for b in blocks[i + 1:]:
            if spec[a + ".time_emb_proj.weight"] == spec[b + ".time_emb_proj.weight"]:
                out = dict(sd)
                for s in (".time_emb_proj.weight", ".time_emb_proj.bias"):
                    out[a + s], out[b + s] = sd[b + s], sd[a + s]
                return out, (a, b)
    raise AssertionError("no two blocks of equal width")


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_planted_structural_errors_are_far_over_the_forward_bar(name, evaluated):
    cfg = arch_ref.ARCHS[name]
    sd, (x, _, t), (_, _, p64), (_, _, p32) = evaluated(name)
    bar = MODEL_FACTOR * (p32.double() - p64).abs().max().item()          # what the GPU forward is held to, absolute
    assert 0.0 < bar < 1e-4
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        assert torch.equal(arch_ref.unet_forward(cfg, sd64, x.double(), t), p64)
        swapped, pair = _swapped_time_projections(cfg, sd64)
        e_temb = (arch_ref.unet_forward(cfg, swapped, x.double(), t) - p64).abs().max().item()
        e_skip = (arch_ref.unet_forward(cfg, sd64, x.double(), t, swap_first_skips=True) - p64).abs().max().item()
    assert e_temb >= 100.0 * bar, f"{name}: time_emb_proj of {pair} exchanged moves the prediction by {e_temb:.3e}, bar {bar:.3e}"
    assert e_skip >= 100.0 * bar, f"{name}: first two skips exchanged moves the prediction by {e_skip:.3e}, bar {bar:.3e}"


@pytest.mark.parametrize("name,count", [("A", 4), ("B", 6), ("C", 15), ("D", 30)])
def test_the_vanishing_gradients_are_exactly_the_stated_set(name, count, evaluated):
    _, _, (_, g64, _), _ = evaluated(name)
    vanishing = [k for k, g in g64.items() if g.abs().max().item() <= 1e-8]
    assert vanishing == arch_ref.vanishing_set(name) and len(vanishing) == count
    if name == "D":
        kinds = {"conv1.bias", "conv2.bias", "conv_shortcut.bias", "to_k.bias"}
        assert all(k.rsplit(".", 2)[-2] + "." + k.rsplit(".", 2)[-1] in kinds or ".time_emb_proj." in k
                   or k.startswith("time_embedding.linear_") for k in vanishing)
    else:
        assert all(k.endswith("to_k.bias") for k in vanishing)
    # every other tensor has a gradient the relative measure can stand on
    assert min(g.abs().max().item() for k, g in g64.items() if k not in vanishing) >= 1e-6


def test_a_producer_finalises_groups_of_eight_channels_only():
    """sisic_conv_stats_slots / sisic_conv_finalizes at the group sizes of the architectures (test_conv_plan_cpu.py pins 8 and 4):
    a 16x16 convolution whose 64-channel tile holds whole groups of eight finalises the following GroupNorm itself -- A's level 1
    at 32x32, 64 channels in 8 groups, as the reference's 256 in 32 -- while 96 in 32 (three per group), 192 in 32 (six) and 32
    in 32 (one) leave partials for the stand-alone finalisation.  Host code: no device is touched."""
    import test_conv_plan_cpu as cp
    from synt_isic_amd import _lib
    lib = _lib.load()
    got = {}
    for cin, cout, per_group in ((64, 64, 8), (256, 256, 8), (96, 96, 3), (192, 192, 6), (32, 32, 1), (64, 64, 4)):
        for B in (1, 2, 64):
            a = cp.make_args(cp.row(3, 1, 0, 1, 0, cin, cout, (16, 16), 1, per_group=per_group), B)
            got.setdefault((cout, per_group), set()).add((lib.sisic_conv_stats_slots(C.byref(a)), lib.sisic_conv_finalizes(C.byref(a))))
    assert all(len(v) == 1 for v in got.values()), got                       # never by the batch
    got = {k: v.pop() for k, v in got.items()}
    assert all(slots > 0 for slots, _ in got.values()), got
    assert {k: fin for k, (_, fin) in got.items()} == {(64, 8): 1, (256, 8): 1, (96, 3): 0, (192, 6): 0, (32, 1): 0, (64, 4): 0}, got


def test_mse_loss_refuses_a_target_of_another_shape():
    """the spelled-out loop on a model whose output channels differ from its input channels: mse_loss(pred, noise) with the
    input-shaped noise raises before any library call (no GPU here: a library call would fail differently)"""
    from synt_isic_amd.train import mse_loss
    pred = torch.zeros(2, 6, 9, 7)
    pred._sisic_model = object()
    with pytest.raises(RuntimeError, match=r"target's shape \(2, 3, 9, 7\) must match the prediction's \(2, 6, 9, 7\)"):
        mse_loss(pred, torch.zeros(2, 3, 9, 7))
    with pytest.raises(RuntimeError, match="must match"):
        mse_loss(pred, torch.zeros(2, 6, 7, 9))           # the same element count is not the same shape
