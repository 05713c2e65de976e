"""Every entry point with a `void* stream` on a NON-default stream: held, across streams and concurrently.

The rest of the suite passes ``torch.cuda.current_stream()``, the null stream, everywhere.  Here each case of
``stream_probe.CASES`` runs through ``stream_probe.run_held``: baseline on the default stream, a warm call and then the real
call on a side stream that a spin kernel holds, the inputs NaN until copies queued behind the hold fill them.  A launch,
memset or copy that the library puts on stream 0 (or on a stream not ordered behind the caller's) reads the NaN, or stale
library memory, and the result is not ``torch.equal`` to the baseline.  A call that include/sisic.h does not document as
synchronising must also return while the stream is still held.

Bounds of the baselines (so that this file stands alone): KTOL = 1e-5 * max(1, |ref|_inf) against float64 for the convolutions
and attention (tests/test_gpu_kernels.py); 5e-5 max-abs for a UNet forward against the CPU oracle (PRED_TOL of
tests/test_gpu_train.py, inside the stated 2e-4 FWD_TOL of tests/test_gpu_unet.py).  Everything else is compared bit for bit
with the default-stream run of the same call, which the other files hold to their references.
"""
import ctypes as C
import functools
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_probe as sp
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5
PRED_TOL = 5e-5
N_CLASS = 5                  # embedding rows of the conditional model: four classes and the null label
T_LOOP = 6


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _dev(args):
    return [a.to(DEV).contiguous() if torch.is_tensor(a) else a for a in args]


def _close(got, ref64, what):
    got = got.detach().cpu().double()
    bound = KTOL * max(1.0, ref64.abs().max().item())
    err = (got - ref64).abs().max().item()
    print(f"{what}: baseline max abs err {err:.3e}, bound {bound:.3e}")
    assert got.shape == ref64.shape and err <= bound, f"{what}: max abs err {err:.3e} > {bound:.3e}"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from synt_isic_amd import _lib
    return _lib


def _ctx():
    from synt_isic_amd import ops
    return ops.context(torch.device(DEV))


class Case:
    """fn(*args) -> result; gen(k) -> host arguments (k = 0: the real values, k = 1: the warm call's); check(baseline): the
    baseline against its own reference, or None; extra() -> (default-stream state, side-stream state) read after the run"""

    def __init__(self, fn, gen, check=None, extra=None):
        self.fn, self.gen, self.check, self.extra = fn, gen, check, extra


BUILDERS = {}


def case(*names):
    def deco(f):
        for n in names:
            assert n not in BUILDERS, n
            BUILDERS[n] = functools.partial(f, n)
        return f
    return deco


# ================================================================ kernels through ops ==================================
#        name -> (B, cin, cout, H, W, ksize, tile_cfg, second filter form, stride, nearest-2x)
CONVS = {
    "conv3x3_f32_direct": (2, 16, 64, 20, 40, 3, 2, None, 1, False),                   # ragged 32x32 tiles
    "conv3x3_winograd_bf16x3_cfg74": (2, 24, 64, 18, 10, 3, 74, "wino", 1, False),     # reads the item table
    "conv3x3_winograd_ksplit_f32": (8, 64, 64, 8, 8, 3, 90, "wino", 1, False),         # per-stream K-split scratch
    "conv3x3_winograd_ksplit_bf16x3": (8, 64, 64, 8, 8, 3, 92, "wino", 1, False),
    "conv1x1_pointwise_bf16x3": (2, 64, 128, 16, 16, 1, 28, None, 1, False),
    "conv1x1_pointwise_bf16x3_ksplit": (2, 128, 192, 8, 16, 1, 35, None, 1, False),
    "conv3x3_stride2_bf16x3": (2, 64, 64, 16, 16, 3, 36, "s2", 2, False),
    "conv3x3_small_cout": (2, 32, 3, 20, 36, 3, 50, None, 1, False),
    "conv3x3_nearest2x_upsample": (2, 24, 64, 10, 14, 3, 74, "wino", 1, True),
}


@case(*CONVS)
def _conv(name):
    from synt_isic_amd import ops
    B, cin, cout, H, W, k, cfg, form, stride, ups = CONVS[name]

    def gen(s):
        return [_rand(B, cin, H, W, seed=10 + s), _rand(cout, cin, k, k, seed=20 + s, scale=(k * k * cin) ** -0.5),
                _rand(cout, seed=30 + s)]

    def fn(x, w, b):
        second = ops.pack_winograd_weight(w) if form == "wino" else ops.pack_conv_s2_weight(w) if form == "s2" else None
        return ops.conv2d(x, ops.pack_conv_weight(w), cout, k, bias=b, stride=stride, upsample=ups, tile_cfg=cfg,
                          w_winograd=second)

    def check(base):
        x, w, b = (t.double() for t in gen(0))
        if ups:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        _close(base, F.conv2d(x, w, b, stride=stride, padding=k // 2), name)
    return Case(fn, gen, check)


def _partials(B, Cc, slots, seed):
    """[B, C, slots, 4] epilogue partials (count, sum, M2 about the partial's own mean, 0) of 32 values each"""
    v = _rand(B, Cc, slots, 32, seed=seed).double()
    s1 = v.sum(-1)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([torch.full_like(s1, 32.0), s1, m2, torch.zeros_like(s1)], -1).float()


@case("groupnorm_stats")
def _gn_stats(name):
    from synt_isic_amd import ops
    gen = lambda s: [_rand(2, 40, 9, 7, seed=40 + s), _rand(2, 24, 9, 7, seed=42 + s), 1.0 + 0.1 * _rand(64, seed=44 + s),
                     0.1 * _rand(64, seed=46 + s)]
    return Case(lambda x, x2, g, b: ops.groupnorm_stats(x, g, b, 8, 1e-5, x2=x2), gen)


@case("groupnorm_finalize")
def _gn_finalize(name):
    from synt_isic_amd import ops
    gen = lambda s: [_partials(2, 24, 1, 50 + s), _partials(2, 40, 4, 52 + s), 1.0 + 0.1 * _rand(64, seed=54 + s),
                     0.1 * _rand(64, seed=56 + s)]
    return Case(lambda s0, s1, g, b: ops.groupnorm_finalize(s0, 64, g, b, 8, 1e-5, stats2=s1), gen)


@case("conv2d_gn_rider")
def _gn_rider(name):
    from synt_isic_amd import ops
    gen = lambda s: [_rand(3, 64, 8, 8, seed=60 + s), _rand(64, 64, 1, 1, seed=62 + s, scale=0.125), _rand(64, seed=64 + s),
                     _partials(3, 48, 2, 66 + s), 1.0 + 0.1 * _rand(48, seed=68 + s), 0.1 * _rand(48, seed=70 + s)]

    def fn(x, w, b, st, g, be):
        out, sc, sh, carried = ops.conv2d_gn_rider(x, ops.pack_conv_weight(w), 64, 1, st, 64, g, be, 6, 1e-5, bias=b, tile_cfg=29)
        assert carried == 1, "the bf16x3 1x1 kernel did not carry the finalisation"
        return out, sc, sh
    return Case(fn, gen)


def _attn_ref(qkv, heads):
    B, C3, N = qkv.shape
    Cc = C3 // 3
    d = Cc // heads
    q, k, v = qkv.double().reshape(B, 3, heads, d, N).unbind(1)
    p = torch.softmax(torch.einsum("bhdq,bhdk->bhqk", q, k) * d ** -0.5, dim=-1)
    return torch.einsum("bhqk,bhdk->bhdq", p, v).reshape(B, Cc, N)


@case("attention_n100", "attention_n300")
def _attention(name):
    from synt_isic_amd import ops
    N = int(name.rsplit("n", 1)[1])
    gen = lambda s: [_rand(2, 3 * 64, N, seed=80 + s + N) * 1.5]
    return Case(lambda qkv: ops.attention(qkv, 8), gen, lambda base: _close(base, _attn_ref(gen(0)[0], 8), name))


SEEDS = [11, (1 << 40) + 5]
ROWS = {"ddpm": (0.6, 0.8, 0.3, 0.7, 0.1), "ddim": (0.6, 0.8, 0.9, 0.4, 0.1), "dpmpp": (0.6, 0.8, 0.5, 0.4, 0.1, -0.05)}
EDIT_ROW = (0.9, 0.43, 0.95, 0.31)


@case(*(f"{r}_step{f}" for r in ROWS for f in ("", "_rng", "_edit")))
def _step(name):
    """the elementwise step kernels: 2 x 3 x 18 x 18 floats (not a multiple of the block, whole float4s)"""
    from synt_isic_amd import ops
    rule, _, form = name.partition("_step")
    row, shape = ROWS[rule], (2, 3, 18, 18)

    def gen(s):
        a = [_rand(*shape, seed=90 + s), _rand(*shape, seed=92 + s)]                       # eps, x
        if form == "":
            a.append(_rand(*shape, seed=94 + s))                                            # z
        if rule == "dpmpp":
            a.append(_rand(*shape, seed=96 + s))                                            # the previous step's x0
        if form == "_edit":
            a += [_rand(*shape, seed=98 + s).clamp(-1, 1), (torch.rand(2, 1, 18, 18, generator=torch.Generator().manual_seed(99 + s)) > 0.5).float()]
        return a

    def fn(eps, x, *rest):
        rest = list(rest)
        z = rest.pop(0) if form == "" else None
        hist = rest.pop(0).clone() if rule == "dpmpp" else None
        if form == "":
            out = ops.dpmpp_step(eps, x, z, hist, row, clip=1.0) if rule == "dpmpp" else getattr(ops, f"{rule}_step")(eps, x, z, row)
        elif form == "_rng":
            out = ops.dpmpp_step_rng(eps, x, SEEDS, 3, hist, row, clip=1.0) if rule == "dpmpp" else \
                getattr(ops, f"{rule}_step_rng")(eps, x, SEEDS, 3, row)
        else:
            x0k, mask = rest
            out = ops.dpmpp_step_edit(eps, x, SEEDS, 3, hist, row, x0k, mask, EDIT_ROW, clip=1.0) if rule == "dpmpp" else \
                getattr(ops, f"{rule}_step_edit")(eps, x, SEEDS, 3, row, x0k, mask, EDIT_ROW)
        return out, hist
    return Case(fn, gen)


@case("guide_eps")
def _guide(name):
    from synt_isic_amd import ops
    return Case(lambda a, b: ops.guide_eps(a, b, 3.0), lambda s: [_rand(2, 3, 18, 18, seed=100 + s), _rand(2, 3, 18, 18, seed=102 + s)])


@case("noise_fill", "noise_bits")
def _noise(name):
    from synt_isic_amd import ops
    return Case(lambda seeds: getattr(ops, name)(seeds, 3001, 4, tag=0), lambda s: [[7 + s, (1 << 33) + s]])


@case("denorm_u8")
def _denorm(name):
    from synt_isic_amd import ops

    def fn(x):
        B, Cc, H, W = x.shape
        plain = ops.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
        _lib().check(_lib().load().sisic_denorm_u8(_ctx(), x.data_ptr(), plain.data_ptr(), B, Cc, H, W, _stream()))
        return ops.denorm_u8(x, "diffusion_generator"), plain
    return Case(fn, lambda s: [_rand(2, 3, 18, 18, seed=104 + s)])


#          name -> (B, c0, cout, H, W, k, stride): rows of tests/test_gpu_train.py::test_conv_wgrad
WGRADS = {"conv2d_wgrad_winograd": (3, 40, 33, 8, 8, 3, 1), "conv2d_wgrad_direct_stride2": (2, 48, 40, 12, 20, 3, 2)}


@case(*WGRADS)
def _wgrad(name):
    from synt_isic_amd import ops
    B, c0, cout, H, W, k, stride = WGRADS[name]
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    return Case(lambda x, dy: ops.conv2d_wgrad(x, dy, k, stride=stride),
                lambda s: [_rand(B, c0, H, W, seed=110 + s), _rand(B, cout, Ho, Wo, seed=112 + s)])


@case("attention_bwd")
def _attention_bwd(name):
    from synt_isic_amd import ops
    return Case(lambda qkv, o, do: ops.attention_bwd(qkv, o, do, 8),
                lambda s: [_rand(2, 96, 100, seed=114 + s), _rand(2, 32, 100, seed=116 + s), _rand(2, 32, 100, seed=118 + s)])


@case("groupnorm_bwd")
def _groupnorm_bwd(name):
    from synt_isic_amd import ops
    return Case(lambda da, x, g, b: ops.groupnorm_bwd(da, x, g, b, 8, 1e-5, True),
                lambda s: [_rand(2, 64, 9, 7, seed=120 + s), _rand(2, 64, 9, 7, seed=122 + s), 1.0 + 0.1 * _rand(64, seed=124 + s),
                           0.1 * _rand(64, seed=126 + s)])


@case("add_noise")
def _add_noise(name):
    from synt_isic_amd import ops

    def fn(x0, nz, a, c):
        out = ops.empty_like(x0)
        _lib().check(_lib().load().sisic_add_noise(_ctx(), x0.data_ptr(), nz.data_ptr(), a.data_ptr(), c.data_ptr(), out.data_ptr(),
                                                   x0.shape[0], x0[0].numel(), _stream()))
        return out
    return Case(fn, lambda s: [_rand(2, 3, 18, 18, seed=130 + s), _rand(2, 3, 18, 18, seed=132 + s),
                               torch.tensor([0.9, 0.3]) + 0.01 * s, torch.tensor([0.43, 0.95]) - 0.01 * s])


N_OPT = 5003


@case("grad_stats")
def _grad_stats(name):
    from synt_isic_amd import ops

    def fn(g):
        rec = ops.empty(3, dtype=torch.int32, device=g.device)
        _lib().check(_lib().load().sisic_grad_stats(_ctx(), g.data_ptr(), g.numel(), 0.5, 0.01, rec.data_ptr(), _stream()))
        return rec
    return Case(fn, lambda s: [_rand(N_OPT, seed=134 + s)])


@case("adam_ema")
def _adam_ema(name):
    def gen(s):
        rec = torch.from_numpy(np.array([3.0 + s, 0.25 + 0.1 * s, 0.0], dtype=np.float32).view(np.int32).copy())
        rec[2] = 0
        return [_rand(N_OPT, seed=136 + s), _rand(N_OPT, seed=138 + s), _rand(N_OPT, seed=140 + s) * 0.1,
                _rand(N_OPT, seed=142 + s).abs() * 0.01, _rand(N_OPT, seed=144 + s), rec]

    def fn(p, g, m, v, ema, rec):
        p, m, v, ema = p.clone(), m.clone(), v.clone(), ema.clone()
        _lib().check(_lib().load().sisic_adam_ema(_ctx(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(),
                                                  p.numel(), 1e-3, 0.9, 0.999, 1e-8, 3, 0.5, rec.data_ptr(), 0.99, _stream()))
        return p, m, v, ema
    return Case(fn, gen)


@case("augment")
def _augment(name):
    from synt_isic_amd import ops
    from synt_isic_amd.data import draw_augment_params
    params = draw_augment_params([0, 3, 1], 2, 17, 16, 24)

    def gen(s):
        return [torch.randint(0, 256, (4, 16, 24, 3), generator=torch.Generator().manual_seed(146 + s), dtype=torch.uint8)]
    return Case(lambda ds: (ops.augment(ds, params), ops.augment(ds, params, u8=True)), gen)


@case("intervene")
def _intervene(name):
    from synt_isic_amd import ops
    jobs = [(0, 0, "noise", 0, 0.5), (1, 1, "mean", 0, 0.0), (0, 1, "blur", 3, 0.0), (1, 0, "gaussian_noise", 0, 0.1)]

    def gen(s):
        g = torch.Generator().manual_seed(148 + s)
        return [_rand(2, 3, 16, 20, seed=150 + s), (torch.rand(2, 16, 20, generator=g) > 0.5).to(torch.uint8)]
    return Case(lambda fr, m: ops.intervene(fr, m, jobs, [3, 4, 5, 6], with_intervention=True), gen)


@case("cfi_metrics")
def _cfi(name):
    from synt_isic_amd import ops
    return Case(lambda lo, lm: ops.cfi_metrics(lo, lm, [0, 1, 1]), lambda s: [_rand(2, 7, seed=152 + s), _rand(3, 7, seed=154 + s)])


@case("mask_patches")
def _mask_patches(name):
    from synt_isic_amd import ops

    def fn(img, masks):
        out = ops.empty((5, 3, 16, 16), dtype=torch.float32, device=img.device)
        _lib().check(_lib().load().sisic_mask_patches(_ctx(), img.data_ptr(), masks.data_ptr(), out.data_ptr(), 5, 3, 16, 16, 4,
                                                      _stream()))
        return out

    def gen(s):
        g = torch.Generator().manual_seed(156 + s)
        return [_rand(3, 16, 16, seed=158 + s), (torch.rand(5, 4, 4, generator=g) > 0.4).to(torch.uint8)]
    return Case(fn, gen)


@case("resample_diffs")
def _resample(name):
    from synt_isic_amd import ops
    return Case(lambda top, bottom: ops.resample_diffs(top, bottom, 77, 96, 80),
                lambda s: [(np.arange(13) * 0.37 + s).tolist(), (np.arange(9) * 0.21 - s).tolist()])


# ================================================================ UNet forward ==========================================
@functools.lru_cache(maxsize=None)
def _sd(cond=False):
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return synthetic_unet_state_dict(num_class_embeds=N_CLASS) if cond else synthetic_unet_state_dict()


@functools.lru_cache(maxsize=None)
def _unet(kind, tag=0):
    """one model per (kind, tag): 'default', 'latency', 'cond'; tags give the tests models of their own"""
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel(num_class_embeds=N_CLASS) if kind == "cond" else HipUNet2DModel()
    m.set_latency_mode(kind == "latency")
    m.load_state_dict(_sd(kind == "cond"))
    return m.to(DEV).eval()


FWD_T = [37, 912]
FWD_LABELS = [0, 3]


def _fwd_x(s):
    return _rand(2, 3, 32, 32, seed=160 + s)


@functools.lru_cache(maxsize=None)
def _oracle_forward(cond):
    """the CPU oracle's prediction for the real inputs: computed once, shared by the forward cases, never written"""
    with torch.no_grad():
        if cond:
            import cond_ref
            return cond_ref.unet_forward(_sd(True), _fwd_x(0), torch.tensor(FWD_T), FWD_LABELS)
        from oracle import unet as ounet
        return ounet.unet_forward(_sd(), _fwd_x(0), torch.tensor(FWD_T))


@case("unet_forward_default", "unet_forward_latency", "unet_forward_cond")
def _unet_forward(name):
    kind = name.rsplit("_", 1)[1]
    m = _unet(kind)
    t = torch.tensor(FWD_T)

    def fn(x):
        return m(x, t, class_labels=FWD_LABELS).sample if kind == "cond" else m(x, t).sample

    def check(base):
        err = (base.cpu() - _oracle_forward(kind == "cond")).abs().max().item()
        print(f"{name}: baseline max |out - oracle| = {err:.3e}, bound {PRED_TOL:.1e}")
        assert err <= PRED_TOL
    return Case(fn, lambda s: [_fwd_x(s)], check)


# ================================================================ sampling loops ========================================
def _scheduler(rule):
    from synt_isic_amd.sampler import Sampler
    if rule == "dpmpp":
        return Sampler(DEV).create_scheduler(T_LOOP, "dpmsolver++", 2, "sde-dpmsolver++")
    return Sampler(DEV).create_scheduler(T_LOOP, rule)


LOOPS = {  # variant -> (rule, eta, noise source, what else)
    "ddpm_host": ("ddpm", 0.0, "host", None), "ddim_host": ("ddim", 0.5, "host", None), "dpmpp_host": ("dpmpp", 0.0, "host", None),
    "ddpm_device": ("ddpm", 0.0, "device", None), "dpmpp_device": ("dpmpp", 0.0, "device", None),
    "guided": ("ddpm", 0.0, "device", "guided"), "edit": ("ddpm", 0.0, "device", "edit"),
    "guided_edit": ("ddim", 0.5, "device", "guided+edit"), "traj_rows": ("ddpm", 0.0, "host", "traj"),
}


@case(*(f"loop_{mode}_{v}" for mode in ("eager", "graph") for v in LOOPS))
def _loop(name):
    """B = 2 at 32x32, T = 6 through run_sampling_loop.  The guided runs draw on the device: graph-replayed they make five
    small uploads through the handle's pinned ring (seeds, timesteps, labels, the guidance table, the loop tables), and six
    when the run is edited as well (the edit rows) -- the most one call makes."""
    from synt_isic_amd.sampler import DeviceNoise, Edit, Guidance, _rule_tables, run_sampling_loop
    _, mode, variant = name.split("_", 2)
    rule, eta, source, what = LOOPS[variant]
    what = set(what.split("+")) if what else set()
    m = _unet("cond" if "guided" in what else "default")
    sched = _scheduler(rule)
    n_noise = int((_rule_tables(sched, eta, False)[0][:, 4] != 0).sum())
    assert n_noise > 0

    def gen(s):
        a = [_rand(2, 3, 32, 32, seed=170 + s)]
        if source == "host":
            a.append(_rand(n_noise, 2, 3, 32, 32, seed=172 + s))
        if "edit" in what:
            a += [_rand(2, 3, 32, 32, seed=174 + s).clamp(-1, 1), (torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(176 + s)) > 0.5).float()]
        return a

    def fn(x_T, *rest):
        rest = list(rest)
        noise = rest.pop(0) if source == "host" else DeviceNoise((21, 22))
        m.set_graph_mode(1 if mode == "graph" else 0)
        res = run_sampling_loop(m, sched, x_T, noise, eta=eta,
                                return_trajectory="traj" in what, save_indices=[1, 4, 5] if "traj" in what else None,
                                guidance=Guidance((0, 3), N_CLASS - 1, 3.0) if "guided" in what else None,
                                edit=Edit(rest[0], rest[1]) if "edit" in what else None)
        assert res.steps_done == T_LOOP and not res.cancelled
        return res.latents, res.images, res.trajectory
    return Case(fn, gen)


def _ddpm_tables():
    sched = _scheduler("ddpm")
    ts = sched.timesteps.to(torch.int64).contiguous()
    coef = sched.coefficient_table().contiguous()
    clip = sched.config.clip_sample_range if sched.config.clip_sample else 0.0
    return ts, coef, float(clip), int((coef[:, 4] != 0).sum())


@case("loop_eager_ddpm_entries")
def _loop_entries(name):
    """sisic_sample, sisic_sample_frames and sisic_sample_frames_rng themselves (the Python loop calls the _rule forms)"""
    from synt_isic_amd import ops
    m = _unet("default")
    ts, coef, clip, n_noise = _ddpm_tables()
    rows = np.array([-1, 0, -1, -1, 1, -1], dtype=np.int32)
    seeds = (C.c_uint64 * 2)(31, 32)

    def fn(x_T, noise):
        lib, h = _lib().load(), m.handle
        m.set_graph_mode(0)
        head = (2, 32, 32, T_LOOP, C.cast(ts.data_ptr(), _lib().c_int64_p), C.cast(coef.data_ptr(), _lib().c_float_p), clip)
        x1, x2, x3 = x_T.clone(), x_T.clone(), x_T.clone()
        u8 = ops.empty((2, 32, 32, 3), dtype=torch.uint8, device=x_T.device)
        traj = ops.empty((2, 2, 3, 32, 32), dtype=torch.float32, device=x_T.device)
        _lib().check(lib.sisic_sample(h, x1.data_ptr(), *head, noise.data_ptr(), None, u8.data_ptr(), None, None, _stream()))
        _lib().check(lib.sisic_sample_frames(h, x2.data_ptr(), *head, noise.data_ptr(), traj.data_ptr(),
                                             rows.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, _stream()))
        _lib().check(lib.sisic_sample_frames_rng(h, x3.data_ptr(), *head, seeds, 0, None, None, None, None, None, _stream()))
        return x1, u8, x2, traj, x3
    return Case(fn, lambda s: [_rand(2, 3, 32, 32, seed=178 + s), _rand(n_noise, 2, 3, 32, 32, seed=180 + s)])


@case("loop_eager_cancel_flag")
def _loop_cancel(name):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    m, sched, flag = _unet("default"), _scheduler("ddpm"), C.c_int(0)

    def fn(x_T):
        m.set_graph_mode(0)
        res = run_sampling_loop(m, sched, x_T, DeviceNoise((41, 42)), cancel_flag=flag)
        assert res.steps_done == T_LOOP and not res.cancelled
        return res.latents, res.images
    return Case(fn, lambda s: [_rand(2, 3, 32, 32, seed=182 + s)])


# ================================================================ training ==============================================
class _Pair:
    """Two models with the same weights and the same history: the first serves the default-stream call, the second the side
    stream's two.  run_held calls fn three times -- baseline, warm, held -- so the first model takes its warm step (same
    values, default stream) when the case is built: both models then run [warm step, real step], on different streams."""

    def __init__(self, cond):
        from synt_isic_amd.scheduler import HipDDPMScheduler
        from synt_isic_amd.train import HipAdam, HipEMA
        from synt_isic_amd.unet import HipUNet2DModel
        self.cond = cond
        self.sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        self.models, self.plain, self.ext, self.ema = [], [], [], []
        for _ in range(2):
            m = HipUNet2DModel(num_class_embeds=N_CLASS) if cond else HipUNet2DModel()
            m.load_state_dict(_sd(cond))
            m = m.to(DEV)
            self.models.append(m)
            self.plain.append(HipAdam(m, lr=1e-3))
            self.ema.append(HipEMA(m))
            self.ext.append(HipAdam(m, lr=1e-3, max_grad_norm=0.5, ema=self.ema[-1]))
        self.calls = 0

    def case(self, step, gen, read=("grads", "weights")):
        """step(i, *args) runs on model i"""
        self.calls = 0
        step(0, *_dev(gen(1)))
        torch.cuda.synchronize()

        def fn(*args):
            i = 0 if self.calls == 0 else 1
            self.calls += 1
            return step(i, *args)

        def extra():
            out = ([], [])
            for i in (0, 1):
                if "grads" in read:
                    out[i].append(self.models[i].grads())
                if "weights" in read:
                    out[i].append(self.models[i]._read_all(0))
                if "ema" in read:
                    out[i].append(self.models[i]._read_all(4))
                    out[i].append(self.models[i].optimizer_state())
            return out
        return Case(fn, gen, None, extra)


@functools.lru_cache(maxsize=None)
def _pair(cond=False):
    return _Pair(cond)


TRAIN_T = [3, 871]


def _train_gen(s):
    g = torch.Generator().manual_seed(190 + s)
    return [torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, torch.randn(2, 3, 32, 32, generator=g)]


@case("train_spelled_out", "train_cond_spelled_out")
def _train_spelled(name):
    from synt_isic_amd.train import mse_loss
    p = _pair("cond" in name)
    t = torch.tensor(TRAIN_T)

    def step(i, images, noise):
        m, opt = p.models[i].train(), p.plain[i]
        opt.zero_grad()
        noisy = p.sched.add_noise(images, noise, t)
        loss = mse_loss(m(noisy, t, class_labels=FWD_LABELS).sample if p.cond else m(noisy, t).sample, noise)
        loss.backward()
        opt.step()
        return loss.detach()
    return p.case(step, _train_gen)


@case("train_step_fused", "train_step_ext_clip_ema", "train_step_cond")
def _train_fused(name):
    from synt_isic_amd.train import train_step_fused
    p = _pair(name == "train_step_cond")
    ext = name == "train_step_ext_clip_ema"
    t = torch.tensor(TRAIN_T)

    def step(i, images, noise):
        opt = (p.ext if ext else p.plain)[i]
        loss, taken = train_step_fused(p.models[i].train(), p.sched, images, noise, t, opt, class_labels=FWD_LABELS if p.cond else None)
        return loss, taken, opt.grad_norm
    return p.case(step, _train_gen, ("grads", "weights", "ema") if ext else ("grads", "weights"))


@case("optimizer_step_ext")
def _optimizer_ext(name):
    from synt_isic_amd.train import mse_loss
    p = _pair(False)
    t = torch.tensor(TRAIN_T)

    def step(i, noisy, noise):
        m, opt = p.models[i].train(), p.ext[i]
        loss = mse_loss(m(noisy, t).sample, noise)
        loss.backward()
        opt.step()
        return loss.detach(), opt.grad_norm
    return p.case(step, _train_gen, ("grads", "weights", "ema"))


@case("ema_step_and_swap")
def _ema(name):
    """EMAModel.step on its own, then the averaged weights swapped in for a forward and out again for another"""
    p = _pair(False)
    t = torch.tensor(FWD_T)

    def step(i, x):
        m, ema = p.models[i].eval(), p.ema[i]
        ema.step()
        with ema.average_parameters():
            averaged = m(x, t).sample
        return averaged, m(x, t).sample
    return p.case(step, lambda s: [_fwd_x(s)], ("weights", "ema"))


# ================================================================ classifier ============================================
@functools.lru_cache(maxsize=None)
def _clf():
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    m = HipMelanomaClassifier(num_classes=7, pretrained=False)
    m.load_state_dict(synthetic_resnet18_state_dict())
    return m.to(DEV).eval()


CLF = {
    "classifier_forward": lambda c, x: c.forward(x),
    "classifier_stem": lambda c, x: c.stem_activation(x),
    "classifier_input_gradient": lambda c, x: c.input_gradient(x, 1),
    "classifier_gradcam": lambda c, x: c.grad_cam(x, 1),
    "classifier_class_scores": lambda c, x: c._scores(x, 1),
    "classifier_randomize_forward": lambda c, x: (c.randomize_weights(5, 2, 0.05), c.forward(x))[1],
    "classifier_restore_forward": lambda c, x: (c.restore_weights(), c.forward(x))[1],
}


@case(*CLF)
def _classifier(name):
    c = _clf()
    return Case(lambda x: CLF[name](c, x), lambda s: [_rand(2, 3, 64, 64, seed=200 + s) * 0.8])


# ================================================================ Python surface ========================================
@functools.lru_cache(maxsize=None)
def _sampler():
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV)
    s.add_model("NV", _sd())
    return s


@case("sampler_generate_host_noise", "sampler_generate_host_noise_copy_stream", "sampler_generate_device_noise")
def _generate(name):
    s = _sampler()
    noise = "device" if name.endswith("device_noise") else "host"

    def fn(seed):
        old = os.environ.get("SISIC_NOISE_SAME_STREAM")
        if name.endswith("copy_stream"):
            os.environ["SISIC_NOISE_SAME_STREAM"] = "0"         # the NoiseStream uploads on its copy stream, ordered by events
        try:
            images, _ = s.generate(seed, "NV", T_LOOP, count=2, size=(32, 32), noise=noise)
            res = s.generate_images("NV", [seed, seed + 1], T_LOOP, size=(32, 32), noise=noise)
        finally:
            if old is None:
                os.environ.pop("SISIC_NOISE_SAME_STREAM", None)
            else:
                os.environ["SISIC_NOISE_SAME_STREAM"] = old
        assert np.array_equal(images, res.images.cpu().numpy())
        return torch.from_numpy(images), list(res.noise_hashes)
    return Case(fn, lambda k: [500 + 10 * k])


# ================================================================ the tests =============================================
def test_probe_sees_a_launch_on_the_null_stream():
    """Positive control: an entry point called with stream = NULL while its inputs are produced behind a hold on a side stream
    reads the NaN pre-fill.  Where the null stream and the side stream share a hardware queue -- or side streams block against
    the null stream -- it would read the real values, and every test below would pass whatever the library did."""
    from synt_isic_amd import ops
    lib = _lib().load()
    a, b = _rand(2, 3, 18, 18, seed=1).to(DEV), _rand(2, 3, 18, 18, seed=2).to(DEV)
    baseline = ops.guide_eps(a, b, 3.0)
    torch.cuda.synchronize()
    ha, hb = torch.full_like(a, float("nan")), torch.full_like(b, float("nan"))
    out = torch.zeros_like(a)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ev = sp.hold(side, sp.HOLD_FLOOR_MS)
        ha.copy_(a, non_blocking=True)
        hb.copy_(b, non_blocking=True)
    _lib().check(lib.sisic_guide_eps(_ctx(), ha.data_ptr(), hb.data_ptr(), 3.0, out.data_ptr(), a.numel(), None))
    held = not ev.query()
    torch.cuda.synchronize()
    differs = not torch.equal(out, baseline)
    print(f"positive control: hold {sp.HOLD_FLOOR_MS:.0f} ms, held until return: {held}, the null-stream launch read the pre-fill: {differs}")
    assert differs, ("the probe is blind on this machine: a launch on the null stream waited for a held side stream, so a "
                     "wrong-stream launch in the library would go unnoticed by every test of this file")
    assert torch.isnan(out).all()


@pytest.mark.parametrize("name", list(sp.CASES))
def test_held_stream(name):
    """(b) the held side-stream result equals the default-stream result bit for bit; (c) a call the header does not document
    as synchronising returns while the stream is still held."""
    c = BUILDERS[name]()
    baseline, held_out, held = sp.run_held(c.fn, lambda: _dev(c.gen(0)), lambda: _dev(c.gen(1)), label=name)
    if c.check is not None:
        c.check(baseline)
    assert sp.same(baseline, held_out), f"{name}: the result on a held side stream differs from the default-stream result"
    if c.extra is not None:
        on_default, on_side = c.extra()
        assert sp.same(on_default, on_side), f"{name}: the state left on a held side stream differs from the default-stream run"
    why = sp.CASES[name][1]
    if why is None:
        assert held, (f"{name}: the call waited for its stream (the hold had elapsed when it returned) and include/sisic.h does "
                      "not say that it synchronises")
    else:
        print(f"{name}: synchronises by design -- \"{' '.join(why.split())}\"")


def test_graph_key_follows_the_stream():
    """One model in graph mode, B = 1 at 32x32, T = 6: a second run on the same stream replays, every other stream -- the
    default one included, which gets the handle's own blocking stream -- captures again, and so does coming back."""
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    lib = _lib().load()
    m, sched = _unet("default", tag=1), _scheduler("ddpm")
    x_T = _rand(1, 3, 32, 32, seed=300).to(DEV)
    noise = DeviceNoise((51,))
    m.set_graph_mode(0)
    eager = run_sampling_loop(m, sched, x_T, noise).latents
    torch.cuda.synchronize()
    m.set_graph_mode(1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    builds = lambda: int(lib.sisic_unet_graph_builds(m.handle))
    n0 = builds()
    steps = []
    for stream, grows in ((s1, 1), (s1, 0), (s2, 1), (None, 1), (s1, 1)):
        before = builds()
        if stream is None:
            out = run_sampling_loop(m, sched, x_T, noise).latents
        else:
            with torch.cuda.stream(stream):
                out = run_sampling_loop(m, sched, x_T, noise).latents
        torch.cuda.synchronize()
        steps.append(builds() - before)
        assert torch.equal(out, eager), f"run {len(steps)} differs from the eager default-stream run"
        assert steps[-1] == grows, f"graph builds moved by {steps} over the runs (s1, s1, s2, default, s1)"
    print(f"graph builds: {n0} before, {steps} over the runs (s1, s1, s2, default, s1)")


def test_item_table_filled_on_a_held_stream_is_not_read_by_another():
    """A cfg-74 geometry no other case of this file uses.  Stream A is held and launches the convolution: its table fill is
    enqueued and cannot have run.  The same geometry on stream B must not read that table -- its fill event has not passed --
    and derives its items itself; B is synchronised while A is still held.  Then A drains, and a third launch on B uses the
    table.  Deterministic and single-threaded.  (The same inside a graph capture on B is not covered: the loop captures whole
    UNet steps, not a chosen convolution.)"""
    from synt_isic_amd import ops
    B, cin, cout, H, W = 3, 24, 64, 22, 26
    x, w, b = _dev([_rand(B, cin, H, W, seed=310), _rand(cout, cin, 3, 3, seed=311, scale=(9 * cin) ** -0.5), _rand(cout, seed=312)])
    wp, ww = ops.pack_conv_weight(w), ops.pack_winograd_weight(w)
    run = lambda cfg: ops.conv2d(x, wp, cout, 3, bias=b, tile_cfg=cfg, w_winograd=ww)
    old = os.environ.get("SISIC_BF3_ITEM_TABLE")
    os.environ["SISIC_BF3_ITEM_TABLE"] = "0"             # the baseline leaves no table of this geometry behind
    try:
        baseline = run(74)
    finally:
        if old is None:
            os.environ.pop("SISIC_BF3_ITEM_TABLE", None)
        else:
            os.environ["SISIC_BF3_ITEM_TABLE"] = old
    torch.cuda.synchronize()
    _close(baseline, F.conv2d(x.cpu().double(), w.cpu().double(), b.cpu().double(), padding=1), "item-table geometry")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        ev = sp.hold(sa, 150.0)
        out_a = run(74)
    with torch.cuda.stream(sb):
        out_b = run(74)
    sb.synchronize()
    a_still_held = not ev.query()
    b_first = out_b.clone()
    sa.synchronize()
    with torch.cuda.stream(sb):
        out_b2 = run(74)
    sb.synchronize()
    print(f"item table: stream A still held when B had drained: {a_still_held}")
    assert torch.equal(b_first, baseline), "stream B read an item table whose fill was still queued on stream A"
    assert torch.equal(out_a, baseline) and torch.equal(out_b2, baseline)


def test_two_lanes_on_two_streams():
    """Smoke check of the supported concurrent use: two threads, each with its own latency-mode model and its own stream, 4
    eager steps at B = 1, 32x32 (tools/two_stream_probe.py); each lane's result equals the same lane run alone.  The lanes share
    the context -- its K-split scratch is per stream -- but nothing forces their kernels to overlap, so a shared buffer can
    slip through: the test runs once and does not repeat itself to hunt for a race."""
    from synt_isic_amd.sampler import Sampler, run_sampling_loop
    models = [_unet("latency", tag=10 + i) for i in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    xs = [_rand(1, 3, 32, 32, seed=320 + i).to(DEV) for i in range(2)]
    for m in models:
        m.set_graph_mode(0)
    torch.cuda.synchronize()

    def lane(i, out, errors):
        try:
            sched = Sampler(DEV).create_scheduler(4, "ddpm")
            with torch.cuda.stream(streams[i]):
                out[i] = run_sampling_loop(models[i], sched, xs[i], None).latents
            streams[i].synchronize()
        except BaseException as e:          # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    alone, errors = [None, None], []
    for i in range(2):
        lane(i, alone, errors)
    assert not errors, errors
    together = [None, None]
    threads = [threading.Thread(target=lane, args=(i, together, errors)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(2):
        assert torch.isfinite(alone[i]).all()
        assert torch.equal(together[i], alone[i]), f"lane {i} beside the other lane differs from lane {i} alone"
