"""Thin torch-tensor wrappers over the single-operator entry points of libsisic_hip.so.

torch is plumbing here (device memory + the current HIP stream); every function
passes raw device pointers to the C ABI.  Tensors must be contiguous fp32 on an
MI355X (``cuda``) device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import ConvArgs, check

_ctx_by_device = {}


def _context(device, code: int, tag: Optional[str] = None) -> C.c_void_p:
    """The ``sisic_ctx`` of ``_ctx_by_device`` for a device, a step prediction type (SISIC_PRED_*) and a tag, created on first
    use.  The key is the device index alone for the default context (epsilon, no tag), which is the only one whose step
    prediction type is never set; ``(index, code)`` for the other untagged ones."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"synt_isic_amd runs on MI355X (torch device 'cuda'); got '{device}'. There is no CPU path.")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, code, tag) if tag is not None else idx if code == _lib.PRED_EPSILON else (idx, code)
    if key not in _ctx_by_device:
        lib = _lib.load()
        h = C.c_void_p()
        check(lib.sisic_create(idx, C.byref(h)))
        if key != idx:
            check(lib.sisic_set_step_prediction_type(h, code))
        _ctx_by_device[key] = h
    return _ctx_by_device[key]


def context(device: torch.device, step_prediction: str = "epsilon") -> C.c_void_p:
    """One ``sisic_ctx`` per (device, step prediction type), created on first use.  ``step_prediction`` says what the ``eps``
    argument of the single-step wrappers below means to the context (sisic_set_step_prediction_type); it is set once, when the
    context is created, and never changed: the default context stays an epsilon context and no call toggles shared state.
    Everything but the step wrappers uses the default context."""
    return _context(device, _lib.prediction_code(step_prediction))


def check_threshold(threshold):
    """``(ratio, sample_max_value)`` of a thresholded step as two floats, or ValueError: ratio inside [0, 1], the maximum finite
    and at least 1 (what the library refuses with SISIC_EINVAL, refused here before anything is set)."""
    try:
        ratio, max_value = (float(v) for v in threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold {threshold!r}: a pair (dynamic_thresholding_ratio, sample_max_value)") from None
    if not (np.isfinite(ratio) and 0.0 <= ratio <= 1.0):
        raise ValueError(f"dynamic_thresholding_ratio {ratio} is outside [0, 1]")
    if not (np.isfinite(max_value) and max_value >= 1.0):
        raise ValueError(f"sample_max_value {max_value} is below 1 or not finite")
    return ratio, max_value


THRESHOLD_MAX_PER_IMAGE = 1 << 24


def _step_context(x: torch.Tensor, prediction_type: str, threshold, B: Optional[int] = None) -> C.c_void_p:
    """The context of a single-step wrapper.  ``threshold`` None: the shared context of the prediction type, which no call
    changes.  ``threshold=(ratio, max)``: dynamic thresholding (sisic_set_step_thresholding) on a second context per
    prediction type that only thresholded steps use; its setting and its image size are host state the entry reads when it
    is called, so they are set before every call.  Images: ``B`` of them, or x's leading dimension."""
    if threshold is None:
        return _context(x.device, _lib.prediction_code(prediction_type))
    ratio, max_value = check_threshold(threshold)
    if ratio == 0.0:
        raise ValueError("threshold=(0, ...) switches thresholding off: pass threshold=None")
    if B is None:
        if x.dim() < 2:
            raise ValueError("a thresholded step takes x as [B, ...]: the images are its leading dimension")
        B = x.shape[0]
    npi = x.numel() // B
    if npi > THRESHOLD_MAX_PER_IMAGE:
        raise ValueError(f"thresholding takes images of at most 2**24 elements, these have {npi}")
    lib = _lib.load()
    h = _context(x.device, _lib.prediction_code(prediction_type), "threshold")
    check(lib.sisic_set_step_thresholding(h, ratio, max_value))
    check(lib.sisic_set_step_image_elems(h, npi))
    return h


def x0_threshold(eps: torch.Tensor, x: torch.Tensor, sb: float, sa: float, ratio: float, sample_max_value: float = 1.0, *,
                 prediction_type: str = "epsilon", eps_u: Optional[torch.Tensor] = None, guidance_scale: float = 1.0,
                 grad: Optional[torch.Tensor] = None, classifier_scale: float = 0.0) -> torch.Tensor:
    """sisic_x0_threshold: every image's ``s = clamp(quantile(|x0|, ratio), 1, sample_max_value)`` of dynamic thresholding
    (include/sisic.h), fp32 [B] for x = [B, ...].  x0 is the rule's estimate before any clamp, from ``eps`` as the step sees
    it: as it stands, combined with ``eps_u`` under ``guidance_scale`` (classifier-free guidance), or with the classifier's
    gradient ``grad`` under ``classifier_scale``."""
    lib = _lib.load()
    if x.dim() < 2:
        raise ValueError("x0_threshold takes x as [B, ...]: the images are its leading dimension")
    ratio, max_value = check_threshold((ratio, sample_max_value))
    if eps_u is not None and grad is not None:
        raise ValueError("eps_u and grad: one guidance at a time")
    second = eps_u if eps_u is not None else grad
    for name, t in (("eps", eps), ("eps_u / grad", second)):
        if t is not None and t.numel() != x.numel():
            raise ValueError(f"{name} holds {t.numel()} elements for an x of {x.numel()}")
    B = x.shape[0]
    if x.numel() // B > THRESHOLD_MAX_PER_IMAGE:
        raise ValueError(f"thresholding takes images of at most 2**24 elements, these have {x.numel() // B}")
    s = empty((B,), dtype=torch.float32, device=x.device)
    a = _lib.X0ThresholdArgs(eps=_ptr(eps, "eps"), eps2=_ptr(second, "eps_u / grad"), x=_ptr(x, "x"), s=s.data_ptr(),
                             stream=_stream(x.device), n_per_image=x.numel() // B, B=B,
                             source=1 if eps_u is not None else 2 if grad is not None else 0, sb=float(sb), sa=float(sa),
                             w=float(guidance_scale if eps_u is not None else classifier_scale), ratio=ratio,
                             sample_max_value=max_value, reserved=0.0)
    check(lib.sisic_x0_threshold(context(x.device, prediction_type), C.byref(a)))
    return s


def empty(shape, *, dtype, device, pin_memory=False) -> torch.Tensor:
    """The package's one allocation point for tensors it hands to the library uninitialised: ``torch.empty``.  (The GPU suite
    replaces it, and ``empty_like``, with a poisoned, guarded allocation: tests/poison.py.)"""
    return torch.empty(shape, dtype=dtype, device=device, pin_memory=pin_memory)


def empty_like(t: torch.Tensor) -> torch.Tensor:
    return torch.empty_like(t)


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def upload(host: torch.Tensor, device) -> torch.Tensor:
    """A small host tensor on ``device``, copied through pinned memory on the current stream without blocking the host.  (A
    copy out of pageable memory waits for the stream: a wrapper that made one would synchronise, which include/sisic.h says
    the entry points behind these wrappers do not.)"""
    staged = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
    staged.copy_(host)
    return staged.to(device, non_blocking=True)


def _ptr(t: Optional[torch.Tensor], name: str = "tensor") -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous fp32 tensor on the GPU (got {t.dtype}, {t.device}, "
                         f"contiguous={t.is_contiguous()})")
    return t.data_ptr()


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW -> the kernel's [Cin_pad][k*k][Cout_pad] layout (sisic_conv_pack_weights)."""
    lib = _lib.load()
    cout, cin, k, k2 = w.shape
    assert k == k2
    n = lib.sisic_conv_packed_numel(cout, cin, k)
    if n < 0:
        raise ValueError(f"unsupported conv weight shape {tuple(w.shape)}")
    out = empty(n, dtype=torch.float32, device=w.device)
    check(lib.sisic_conv_pack_weights(context(w.device), _ptr(w, "weight"), cout, cin, k, out.data_ptr(),
                                      _stream(w.device)))
    return out


def pack_winograd_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 -> Winograd-domain filters G g G^T, [Cin_pad][16][Cout_pad] (sisic_conv_winograd_pack)."""
    lib = _lib.load()
    cout, cin, k, k2 = w.shape
    if k != 3 or k2 != 3:
        raise ValueError("Winograd F(2x2,3x3) needs a 3x3 weight")
    out = empty(lib.sisic_conv_winograd_numel(cout, cin), dtype=torch.float32, device=w.device)
    check(lib.sisic_conv_winograd_pack(context(w.device), _ptr(w, "weight"), cout, cin, out.data_ptr(),
                                       _stream(w.device)))
    return out


def pack_conv_s2_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 -> the split (bf16x3) filter of the stride-2 kernel (sisic_conv_s2_pack); passed to conv2d as ``w_winograd``."""
    lib = _lib.load()
    cout, cin, k, k2 = w.shape
    if k != 3 or k2 != 3:
        raise ValueError("the stride-2 bf16x3 kernel needs a 3x3 weight")
    out = empty(lib.sisic_conv_s2_numel(cout, cin), dtype=torch.float32, device=w.device)
    check(lib.sisic_conv_s2_pack(context(w.device), _ptr(w, "weight"), cout, cin, out.data_ptr(), _stream(w.device)))
    return out


def conv2d(x: torch.Tensor, w_packed: torch.Tensor, cout: int, ksize: int, *, bias=None, x2=None, stride=1,
           upsample=False, gn_scale=None, gn_shift=None, gn_silu=False, chan_bias=None, residual=None,
           relu=False, tile_cfg=0, w_winograd=None, with_stats=False, out=None, finalize=None):
    """sisic_conv2d.  with_stats=True also returns the GroupNorm partials the epilogue wrote, as a
    [B, Cout, slots, 4] tensor of (count, sum, centred M2, 0), or None when this launch cannot produce them
    (sisic_conv_stats_slots() == 0).  ``out``: the output tensor to write (it may be ``residual`` itself: include/sisic.h).
    ``finalize=(gamma, beta, groups, eps)``: ask the launch to finalize the GroupNorm over its own output as well; the result
    then ends with ``(scale, shift)`` [B, Cout] tensors, or ``None`` where sisic_conv_finalizes() says this launch does not."""
    lib = _lib.load()
    B, c0, H, W = x.shape
    c1 = 0 if x2 is None else x2.shape[1]
    Hc, Wc = (2 * H, 2 * W) if upsample else (H, W)
    pad = ksize // 2
    Ho = (Hc + 2 * pad - ksize) // stride + 1
    Wo = (Wc + 2 * pad - ksize) // stride + 1
    if out is None:
        out = empty((B, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, cout, Ho, Wo) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous fp32 {(B, cout, Ho, Wo)} tensor on {x.device}")
    a = ConvArgs()
    a.in0 = _ptr(x, "x"); a.in1 = _ptr(x2, "x2"); a.c0 = c0; a.c1 = c1
    a.B = B; a.Hin = H; a.Win = W
    a.upsample = int(upsample); a.ksize = ksize; a.stride = stride
    a.w_packed = _ptr(w_packed, "w_packed"); a.bias = _ptr(bias, "bias"); a.Cout = cout
    a.gn_scale = _ptr(gn_scale, "gn_scale"); a.gn_shift = _ptr(gn_shift, "gn_shift"); a.gn_silu = int(gn_silu)
    a.chan_bias = _ptr(chan_bias, "chan_bias"); a.chan_bias_stride = cout if chan_bias is not None and chan_bias.dim() == 2 and chan_bias.shape[0] == B else 0
    a.residual = _ptr(residual, "residual"); a.relu = int(relu)
    a.out = out.data_ptr(); a.tile_cfg = tile_cfg
    a.w_winograd = _ptr(w_winograd, "w_winograd")
    stats = None
    if with_stats:
        slots = lib.sisic_conv_stats_slots(C.byref(a))
        if slots > 0:
            stats = empty((B, cout, slots, 4), dtype=torch.float32, device=x.device)
            a.stats_out = stats.data_ptr()
    fin = None
    if finalize is not None:
        gamma, beta, groups, eps = finalize
        a.fin_gamma = _ptr(gamma, "gamma"); a.fin_beta = _ptr(beta, "beta"); a.fin_groups = int(groups); a.fin_eps = float(eps)
        if lib.sisic_conv_finalizes(C.byref(a)):
            fin = (empty((B, cout), dtype=torch.float32, device=x.device), empty((B, cout), dtype=torch.float32, device=x.device))
            a.fin_scale, a.fin_shift = fin[0].data_ptr(), fin[1].data_ptr()
        else:
            a.fin_gamma = None
    check(lib.sisic_conv2d(context(x.device), C.byref(a), _stream(x.device)))
    res = (out, stats) if with_stats else out
    if finalize is not None:
        res = (res + (fin,)) if with_stats else (res, fin)
    return res


def groupnorm_finalize(stats: torch.Tensor, hw: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                       stats2: Optional[torch.Tensor] = None):
    """scale/shift of GroupNorm over the (concatenated) producers' outputs from their epilogue partials."""
    lib = _lib.load()
    B, c0, slots0, _ = stats.shape
    c1, slots1 = (0, 0) if stats2 is None else (stats2.shape[1], stats2.shape[2])
    scale = empty((B, c0 + c1), dtype=torch.float32, device=stats.device)
    shift = empty_like(scale)
    check(lib.sisic_groupnorm_finalize(context(stats.device), _ptr(stats, "stats"), c0, slots0, _ptr(stats2, "stats2"),
                                       c1, slots1, B, hw, groups, float(eps), _ptr(gamma, "gamma"), _ptr(beta, "beta"),
                                       scale.data_ptr(), shift.data_ptr(), _stream(stats.device)))
    return scale, shift


def conv2d_gn_rider(x: torch.Tensor, w_packed: torch.Tensor, cout: int, ksize: int, stats: torch.Tensor, hw: int,
                    gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, *, stats2: Optional[torch.Tensor] = None,
                    bias=None, x2=None, gn_scale=None, gn_shift=None, gn_silu=False, tile_cfg=0, w_winograd=None,
                    scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None):
    """sisic_conv2d_gn_rider: the stride-1 convolution of ``conv2d`` whose launch also carries the GroupNorm finalisation of
    ``groupnorm_finalize(stats, hw, gamma, beta, groups, eps, stats2)`` where the chosen kernel can.  Returns
    ``(out, scale, shift, carried)``; with ``carried == 0`` the launch did not run the jobs and ``scale`` / ``shift`` (the
    tensors passed in, or fresh uninitialised ones) are as they were."""
    lib = _lib.load()
    B, c0, H, W = x.shape
    c1 = 0 if x2 is None else x2.shape[1]
    out = empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    a = ConvArgs()
    a.in0 = _ptr(x, "x"); a.in1 = _ptr(x2, "x2"); a.c0 = c0; a.c1 = c1
    a.B = B; a.Hin = H; a.Win = W
    a.upsample = 0; a.ksize = ksize; a.stride = 1
    a.w_packed = _ptr(w_packed, "w_packed"); a.bias = _ptr(bias, "bias"); a.Cout = cout
    a.gn_scale = _ptr(gn_scale, "gn_scale"); a.gn_shift = _ptr(gn_shift, "gn_shift"); a.gn_silu = int(gn_silu)
    a.out = out.data_ptr(); a.tile_cfg = tile_cfg
    a.w_winograd = _ptr(w_winograd, "w_winograd")
    Bs, s0, slots0, _ = stats.shape
    s1, slots1 = (0, 0) if stats2 is None else (stats2.shape[1], stats2.shape[2])
    if scale is None:
        scale = empty((Bs, s0 + s1), dtype=torch.float32, device=stats.device)
    if shift is None:
        shift = empty((Bs, s0 + s1), dtype=torch.float32, device=stats.device)
    if tuple(scale.shape) != (Bs, s0 + s1) or tuple(shift.shape) != (Bs, s0 + s1):
        raise ValueError(f"scale / shift must be {(Bs, s0 + s1)} tensors")
    carried = C.c_int(0)
    check(lib.sisic_conv2d_gn_rider(context(x.device), C.byref(a), _ptr(stats, "stats"), s0, slots0, _ptr(stats2, "stats2"),
                                    s1, slots1, Bs, hw, groups, float(eps), _ptr(gamma, "gamma"), _ptr(beta, "beta"),
                                    _ptr(scale, "scale"), _ptr(shift, "shift"), C.byref(carried), _stream(x.device)))
    return out, scale, shift, carried.value


def groupnorm_stats(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                    x2: Optional[torch.Tensor] = None):
    lib = _lib.load()
    B, c0 = x.shape[0], x.shape[1]
    c1 = 0 if x2 is None else x2.shape[1]
    HW = x[0, 0].numel()
    scale = empty((B, c0 + c1), dtype=torch.float32, device=x.device)
    shift = empty_like(scale)
    check(lib.sisic_groupnorm_stats(context(x.device), _ptr(x, "x"), c0, _ptr(x2, "x2"), c1, B, HW, groups,
                                    float(eps), _ptr(gamma, "gamma"), _ptr(beta, "beta"), scale.data_ptr(),
                                    shift.data_ptr(), _stream(x.device)))
    return scale, shift


def attention(qkv: torch.Tensor, head_dim: int = 8) -> torch.Tensor:
    """qkv [B,3C,N] -> [B,C,N]."""
    lib = _lib.load()
    B, C3, N = qkv.shape
    Cc = C3 // 3
    out = empty((B, Cc, N), dtype=torch.float32, device=qkv.device)
    check(lib.sisic_attention(context(qkv.device), _ptr(qkv, "qkv"), out.data_ptr(), B, Cc, N, head_dim,
                              _stream(qkv.device)))
    return out


_DDPM, _DDIM, _DPMPP = _lib.RULES.values()
_step_entries = {}              # (stem, form) -> the function of the library (``_lib.load()``: one per process), once looked up


def _step(rule: _lib.StepRule, eps, x, coef, clip, out, prediction_type, threshold, z=None, hist=None, flag=False, seeds=None,
          step=0, x0k=None, mask=None, erow=None) -> torch.Tensor:
    """The nine single-step wrappers below: ``sisic_<stem>_step<form>`` of ``rule`` (_lib.RULES), its arguments in the order
    include/sisic.h declares.  The form is what the call carries: no ``seeds``, the buffer form with its ``z``; ``seeds`` and
    ``step``, the ``_rng`` form; with ``x0k``, ``mask`` and ``erow`` as well, the ``_edit`` form.  Every check runs before
    anything is allocated or set; nothing here waits for the stream."""
    form = "" if seeds is None else "_rng" if x0k is None else "_edit"
    row = tuple(map(float, coef))
    if len(row) != rule.row_width:
        raise ValueError(f"a {rule.title} row holds {rule.row_width} values")
    n, B = x.numel(), None
    if form:
        arr = _seed_array(seeds)
        B = len(arr)
        if n % B:
            raise ValueError(f"{n} elements are not {B} equal images")
        if form == "_edit":
            if x0k.numel() != n:
                raise ValueError(f"the known image holds {x0k.numel()} elements for an x of {n}")
            if mask.numel() % B or mask.numel() == 0 or (n // B) % (mask.numel() // B):
                raise ValueError(f"a mask of {mask.numel()} elements is not [B, 1, H, W] for {B} images of {n // B} elements")
            hw = mask.numel() // B
            ck, sk, ja, jb = (float(v) for v in erow)
    if rule.takes_hist and hist.numel() != n:
        raise ValueError(f"hist holds {hist.numel()} elements for an x of {n}")
    ctx = _step_context(x, prediction_type, threshold, B)
    if out is None:
        out = empty_like(x)
    args = [ctx, _ptr(eps, "eps"), _ptr(x, "x")]
    if not form:
        args.append(_ptr(z, "z"))
    if rule.takes_hist:
        args.append(_ptr(hist, "hist"))
    args.append(_ptr(out, "out"))
    if form:
        seeds_dev = upload(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int64), x.device)      # the uint64 bit patterns
        args += (B, n // B, seeds_dev.data_ptr(), int(step))
    else:
        args.append(n)
    args += row
    args.append(float(clip))
    if rule.clipped_output_flag:
        args.append(int(bool(flag)))
    if form == "_edit":
        args += (_ptr(x0k, "x0k"), _ptr(mask, "mask"), n // B // hw, hw, ck, sk, ja, jb)
    args.append(_stream(x.device))
    entry = _step_entries.get((rule.stem, form))
    if entry is None:
        entry = _step_entries[rule.stem, form] = getattr(_lib.load(), f"sisic_{rule.stem}_step{form}")
    check(entry(*args))
    return out


def ddpm_step(eps: torch.Tensor, x: torch.Tensor, z: Optional[torch.Tensor], coef, clip: float = 1.0,
              out: Optional[torch.Tensor] = None, prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """coef = (sqrt_beta_prod, sqrt_alpha_prod, c0, c1, sigma).  ``prediction_type`` (here and in every step wrapper below):
    what ``eps`` holds -- "epsilon", "sample" (x0) or "v_prediction" (include/sisic.h SISIC_PRED_*).  ``threshold`` (likewise):
    None, or ``(dynamic_thresholding_ratio, sample_max_value)`` for dynamic thresholding of x0 in place of ``clip``, which is
    then not read; x is [B, ...] (or, in the ``_rng`` and ``_edit`` wrappers, len(seeds) equal images)."""
    return _step(_DDPM, eps, x, coef, clip, out, prediction_type, threshold, z)


def guide_eps(eps_c: torch.Tensor, eps_u: torch.Tensor, guidance_scale: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sisic_guide_eps: the classifier-free guidance combine ``eps_u + w * (eps_c - eps_u)``, subtract, multiply, add in fp32
    with no fused multiply-add -- the device function the guided step kernels of ``sisic_sample_frames_cond`` call, so a loop
    of two ``model(..., class_labels=)`` calls, this and a scheduler step reproduces the library loop bit for bit."""
    lib = _lib.load()
    if eps_c.shape != eps_u.shape:
        raise ValueError(f"eps_c {tuple(eps_c.shape)} and eps_u {tuple(eps_u.shape)} differ in shape")
    if out is None:
        out = empty_like(eps_c)
    elif out.shape != eps_c.shape:
        raise ValueError(f"out {tuple(out.shape)} does not have the inputs' shape {tuple(eps_c.shape)}")
    check(lib.sisic_guide_eps(context(eps_c.device), _ptr(eps_c, "eps_c"), _ptr(eps_u, "eps_u"), float(guidance_scale),
                              _ptr(out, "out"), eps_c.numel(), _stream(eps_c.device)))
    return out


def clf_guide_eps(eps: torch.Tensor, g: torch.Tensor, sb: float, scale: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sisic_clf_guide_eps: the classifier-guidance combine ``eps - (scale * sb) * g`` -- ``scale * sb``, times ``g``, then the
    subtraction, each rounded to fp32 with no fused multiply-add: the device function the guided step kernels of
    ``sisic_sample_frames_clf`` call.  ``g`` is the classifier's input gradient at the step's latent
    (``HipMelanomaClassifier.input_gradient``), ``sb`` the step's sqrt(1 - abar_t).  ``out`` may be ``eps``."""
    lib = _lib.load()
    if eps.shape != g.shape:
        raise ValueError(f"eps {tuple(eps.shape)} and g {tuple(g.shape)} differ in shape")
    if out is None:
        out = empty_like(eps)
    elif out.shape != eps.shape:
        raise ValueError(f"out {tuple(out.shape)} does not have the inputs' shape {tuple(eps.shape)}")
    a = _lib.ClfGuideArgs(eps=_ptr(eps, "eps"), g=_ptr(g, "g"), out=_ptr(out, "out"), stream=_stream(eps.device), n=eps.numel(),
                          sb=float(sb), scale=float(scale))
    check(lib.sisic_clf_guide_eps(context(eps.device), C.byref(a)))
    return out


def _seed_array(seeds):
    """HOST uint64 [B] as the C ABI takes it; seeds are 64-bit unsigned (negative values are refused, not wrapped)."""
    seeds = [int(s) for s in seeds]
    if not seeds or any(s < 0 or s >> 64 for s in seeds):
        raise ValueError("seeds must be a non-empty sequence of integers in 0 .. 2**64-1")
    return (C.c_uint64 * len(seeds))(*seeds)


def noise_fill(seeds, n_per_image: int, step: int, tag: int = 0, device="cuda") -> torch.Tensor:
    """sisic_noise_fill: fp32 [B, n_per_image] normals of the device-noise contract for
    ``(seeds[b], step, tag)`` -- what the scheduler step of ``sisic_sample_frames_rng`` adds at step index ``step`` (tag 0)."""
    lib = _lib.load()
    device = torch.device(device)
    arr = _seed_array(seeds)
    out = empty((len(arr), int(n_per_image)), dtype=torch.float32, device=device)
    check(lib.sisic_noise_fill(context(device), out.data_ptr(), len(arr), int(n_per_image), arr, int(step), int(tag),
                               _stream(device)))
    return out


def noise_bits(seeds, n_per_image: int, step: int, tag: int = 0, device="cuda") -> torch.Tensor:
    """sisic_noise_bits: the Philox4x32-10 words behind ``noise_fill``, [B, 4*ceil(n_per_image/4)] (int32 tensor holding the
    uint32 bit patterns: view it as uint32 on the host)."""
    lib = _lib.load()
    device = torch.device(device)
    arr = _seed_array(seeds)
    words = 4 * ((int(n_per_image) + 3) // 4)
    out = empty((len(arr), words), dtype=torch.int32, device=device)
    check(lib.sisic_noise_bits(context(device), out.data_ptr(), len(arr), int(n_per_image), arr, int(step), int(tag),
                               _stream(device)))
    return out


def ddpm_step_rng(eps: torch.Tensor, x: torch.Tensor, seeds, step: int, coef, clip: float = 1.0,
                  out: Optional[torch.Tensor] = None, prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """``ddpm_step`` with z generated in the kernel: eps, x are [B, ...] (or flat with B = len(seeds) equal images);
    image b draws ``noise_fill([seeds[b]], n_per_image, step)``."""
    return _step(_DDPM, eps, x, coef, clip, out, prediction_type, threshold, seeds=seeds, step=step)


def ddim_step(eps: torch.Tensor, x: torch.Tensor, z: Optional[torch.Tensor], coef, clip: float = 1.0,
              use_clipped_model_output: bool = False, out: Optional[torch.Tensor] = None,
              prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """sisic_ddim_step: coef = (sqrt_beta_prod, sqrt_alpha_prod, c_prev, c_dir, sigma), a row of
    ``HipDDIMScheduler.coefficient_table``.  z None or sigma == 0: no noise is added."""
    return _step(_DDIM, eps, x, coef, clip, out, prediction_type, threshold, z, None, use_clipped_model_output)


def ddim_step_rng(eps: torch.Tensor, x: torch.Tensor, seeds, step: int, coef, clip: float = 1.0,
                  use_clipped_model_output: bool = False, out: Optional[torch.Tensor] = None,
                  prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """``ddim_step`` with z generated in the kernel, as ``ddpm_step_rng``: image b draws
    ``noise_fill([seeds[b]], n_per_image, step)``, and nothing when sigma == 0."""
    return _step(_DDIM, eps, x, coef, clip, out, prediction_type, threshold, flag=use_clipped_model_output,
                 seeds=seeds, step=step)


def dpmpp_step(eps: torch.Tensor, x: torch.Tensor, z: Optional[torch.Tensor], hist: torch.Tensor, coef, clip: float = 0.0,
               out: Optional[torch.Tensor] = None, prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """sisic_dpmpp_step: coef = (sigma_t, alpha_t, cx, k0, sigma, k1), a row of
    ``HipDPMSolverMultistepScheduler.coefficient_table``.  hist: the previous step's x0, a tensor of x's size that the
    call overwrites with this step's x0 and reads only when k1 != 0.  z None or sigma == 0: no noise is added."""
    return _step(_DPMPP, eps, x, coef, clip, out, prediction_type, threshold, z, hist)


def dpmpp_step_rng(eps: torch.Tensor, x: torch.Tensor, seeds, step: int, hist: torch.Tensor, coef, clip: float = 0.0,
                   out: Optional[torch.Tensor] = None, prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """``dpmpp_step`` with z generated in the kernel, as ``ddpm_step_rng``: image b draws
    ``noise_fill([seeds[b]], n_per_image, step)``, and nothing when sigma == 0."""
    return _step(_DPMPP, eps, x, coef, clip, out, prediction_type, threshold, hist=hist, seeds=seeds, step=step)


def ddpm_step_edit(eps: torch.Tensor, x: torch.Tensor, seeds, step: int, coef, x0k: torch.Tensor, mask: torch.Tensor, erow,
                   clip: float = 1.0, out: Optional[torch.Tensor] = None, prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """sisic_ddpm_step_edit: ``ddpm_step_rng`` with the inpainting epilogue (include/sisic.h) fused into the kernel.
    x0k: the known image, fp32 of x's size, finite; mask: fp32 [B,1,H,W] (1 = keep); erow = (ck, sk, ja, jb).  The epilogue
    draws under tags 5 (``sk != 0``) and 6 (``jb != 0``) of ``noise_fill`` at the same ``step``."""
    return _step(_DDPM, eps, x, coef, clip, out, prediction_type, threshold, seeds=seeds, step=step, x0k=x0k,
                 mask=mask, erow=erow)


def ddim_step_edit(eps: torch.Tensor, x: torch.Tensor, seeds, step: int, coef, x0k: torch.Tensor, mask: torch.Tensor, erow,
                   clip: float = 1.0, use_clipped_model_output: bool = False,
                   out: Optional[torch.Tensor] = None, prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """sisic_ddim_step_edit: ``ddim_step_rng`` with the inpainting epilogue, as ``ddpm_step_edit``."""
    return _step(_DDIM, eps, x, coef, clip, out, prediction_type, threshold, flag=use_clipped_model_output,
                 seeds=seeds, step=step, x0k=x0k, mask=mask, erow=erow)


def dpmpp_step_edit(eps: torch.Tensor, x: torch.Tensor, seeds, step: int, hist: torch.Tensor, coef, x0k: torch.Tensor,
                    mask: torch.Tensor, erow, clip: float = 0.0, out: Optional[torch.Tensor] = None,
                    prediction_type: str = "epsilon", threshold=None) -> torch.Tensor:
    """sisic_dpmpp_step_edit: ``dpmpp_step_rng`` with the inpainting epilogue, as ``ddpm_step_edit``; ``hist`` receives the
    model's predicted x0, which the epilogue does not touch."""
    return _step(_DPMPP, eps, x, coef, clip, out, prediction_type, threshold, hist=hist, seeds=seeds,
                 step=step, x0k=x0k, mask=mask, erow=erow)


def add_noise(x0: torch.Tensor, noise: torch.Tensor, a: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """sisic_add_noise: ``out[b] = a[b] * x0[b] + c[b] * noise[b]`` (two products and one sum, each rounded to fp32) for
    x0 = [B, ...] and ``noise`` of its size, with HOST fp32 rows a, c of B values."""
    B = x0.shape[0]
    if a.numel() != B:
        raise ValueError(f"{a.numel()} timesteps for a batch of {B}")
    a, c = upload(torch.stack([a, c]), x0.device)          # pinned, non-blocking: the call does not wait for the stream
    out = empty_like(x0)
    check(_lib.load().sisic_add_noise(context(x0.device), _ptr(x0, "x0"), _ptr(noise, "noise"), a.data_ptr(), c.data_ptr(),
                                      out.data_ptr(), B, x0[0].numel(), _stream(x0.device)))
    return out


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, ksize: int, *, x2=None, stride=1, upsample=False, gn_scale=None,
                 gn_shift=None, gn_silu=False) -> torch.Tensor:
    """d/dW of ``conv2d`` with the same prologue / index maps: dW [Cout, Cin, k, k] from the forward input(s) and the
    gradient dy of the convolution's output (sisic_conv2d_wgrad)."""
    lib = _lib.load()
    B, c0, H, W = x.shape
    c1 = 0 if x2 is None else x2.shape[1]
    cout = dy.shape[1]
    dw = empty((cout, c0 + c1, ksize, ksize), dtype=torch.float32, device=x.device)
    a = ConvArgs()
    a.in0 = _ptr(x, "x"); a.in1 = _ptr(x2, "x2"); a.c0 = c0; a.c1 = c1
    a.B = B; a.Hin = H; a.Win = W
    a.upsample = int(upsample); a.ksize = ksize; a.stride = stride; a.Cout = cout
    a.gn_scale = _ptr(gn_scale, "gn_scale"); a.gn_shift = _ptr(gn_shift, "gn_shift"); a.gn_silu = int(gn_silu)
    check(lib.sisic_conv2d_wgrad(context(x.device), C.byref(a), _ptr(dy, "dy"), dw.data_ptr(), _stream(x.device)))
    return dw


def attention_bwd(qkv: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, head_dim: int = 8) -> torch.Tensor:
    """gradient of ``attention`` w.r.t. qkv [B,3C,N]."""
    lib = _lib.load()
    B, C3, N = qkv.shape
    dqkv = empty_like(qkv)
    check(lib.sisic_attention_bwd(context(qkv.device), _ptr(qkv, "qkv"), _ptr(out, "out"), _ptr(d_out, "d_out"),
                                  dqkv.data_ptr(), B, C3 // 3, N, head_dim, _stream(qkv.device)))
    return dqkv


def groupnorm_bwd(da: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                  silu: bool):
    """(dx, dgamma, dbeta) of a = act(GroupNorm(x)), act = SiLU or identity."""
    lib = _lib.load()
    B, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    dx = torch.zeros_like(x)
    dg = empty(Cc, dtype=torch.float32, device=x.device)
    db = empty_like(dg)
    check(lib.sisic_groupnorm_bwd(context(x.device), _ptr(da, "da"), _ptr(x, "x"), B, Cc, HW, groups, float(eps),
                                  _ptr(gamma, "gamma"), _ptr(beta, "beta"), int(silu), dx.data_ptr(), dg.data_ptr(),
                                  db.data_ptr(), _stream(x.device)))
    return dx, dg, db


def batchnorm_train(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, residual=None, relu: bool = False,
                    running_mean=None, running_var=None, momentum: float = 0.1, apply: bool = True):
    """``nn.BatchNorm2d`` in training mode on y [B,C,...] (sisic_batchnorm_train): returns ``(out, mean, invstd)`` with
    ``out = [relu](gamma (y - mean) invstd + beta [+ residual])``, mean and invstd = 1/sqrt(var + eps) of the batch [C].
    ``running_mean`` / ``running_var`` (both or neither) are updated in place with the unbiased variance.  ``apply=False``: the
    moments alone, ``out`` is None (what tools time the first launch with)."""
    lib = _lib.load()
    B, Cc = y.shape[0], y.shape[1]
    out = empty_like(y) if apply else None
    mean = empty(Cc, dtype=torch.float32, device=y.device)
    invstd = empty_like(mean)
    a = _lib.BnArgs()
    a.y = _ptr(y, "y"); a.gamma = _ptr(gamma, "gamma"); a.beta = _ptr(beta, "beta"); a.residual = _ptr(residual, "residual")
    a.running_mean = _ptr(running_mean, "running_mean"); a.running_var = _ptr(running_var, "running_var")
    a.out = out.data_ptr() if apply else None; a.mean = mean.data_ptr(); a.invstd = invstd.data_ptr()
    a.stream = _stream(y.device).value
    a.momentum = float(momentum); a.eps = float(eps); a.relu = int(bool(relu))
    a.B, a.C, a.HW = B, Cc, y[0, 0].numel()
    check(lib.sisic_batchnorm_train(context(y.device), C.byref(a)))
    return out, mean, invstd


def batchnorm_train_bwd(g: torch.Tensor, y: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: torch.Tensor, act=None,
                        apply: bool = True):
    """``(dy, dgamma, dbeta)`` of ``batchnorm_train`` for g = dL/d(out) (sisic_batchnorm_train_bwd).  ``act``: the activation
    behind the BatchNorm's ReLU; g counts where it is positive (None: no ReLU, or g is masked already).  ``apply=False``: the
    two sums alone, ``dy`` is None."""
    lib = _lib.load()
    B, Cc = y.shape[0], y.shape[1]
    dy = empty_like(y) if apply else None
    dgamma = empty(Cc, dtype=torch.float32, device=y.device)
    dbeta = empty_like(dgamma)
    a = _lib.BnArgs()
    a.g = _ptr(g, "g"); a.y = _ptr(y, "y"); a.mean = _ptr(mean, "mean"); a.invstd = _ptr(invstd, "invstd")
    a.gamma = _ptr(gamma, "gamma"); a.act = _ptr(act, "act")
    a.dy = dy.data_ptr() if apply else None; a.dgamma = dgamma.data_ptr(); a.dbeta = dbeta.data_ptr()
    a.stream = _stream(y.device).value
    a.B, a.C, a.HW = B, Cc, y[0, 0].numel()
    check(lib.sisic_batchnorm_train_bwd(context(y.device), C.byref(a)))
    return dy, dgamma, dbeta


def add_relu(y: torch.Tensor, identity: torch.Tensor) -> torch.Tensor:
    """relu(y + identity) (sisic_add_relu): the library's plain elementwise pass, the yardstick of the BatchNorm passes"""
    out = empty_like(y)
    a = _lib.BnArgs()
    a.y = _ptr(y, "y"); a.residual = _ptr(identity, "identity"); a.out = out.data_ptr()
    a.stream = _stream(y.device).value
    a.B, a.C, a.HW = 1, 1, y.numel()
    check(_lib.load().sisic_add_relu(context(y.device), C.byref(a)))
    return out


DENORM_FORMS = {"image_generator": 0, "generate_test": 1, "diffusion_generator": 2}


def denorm_u8(x: torch.Tensor, form="image_generator") -> torch.Tensor:
    """[B,C,H,W] fp32 -> uint8 [B,H,W,C] in the fp32 operation order of one of the reference's three call sites:
    "image_generator" (image_generator.py:441-447), "generate_test" (generate_test.py:94-97, bit-equal to the first) or
    "diffusion_generator" (diffusion_generator.py:231-232, `(x+1)*127.5` -- rounds differently)."""
    lib = _lib.load()
    B, Cc, H, W = x.shape
    out = empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
    f = DENORM_FORMS[form] if isinstance(form, str) else int(form)
    check(lib.sisic_denorm_u8_form(context(x.device), _ptr(x, "x"), out.data_ptr(), B, Cc, H, W, f, _stream(x.device)))
    return out


INTERVENTION_TYPES = {"noise": 0, "gaussian_noise": 1, "zero": 2, "mean": 3, "blur": 4, "inpaint": 5, "shuffle": 6}
CFI_PER_CLASS = 6          # orig_score, mod_score, cfi, delta, p_orig, p_mod
CFI_TAIL = 7               # argmax p_orig, argmax p_mod, max p_orig, max p_mod, KL, JS, TV


def intervene(frames: torch.Tensor, masks: torch.Tensor, jobs, seeds, src_index: Optional[torch.Tensor] = None,
              with_intervention: bool = False):
    """sisic_intervene: frames [F,C,H,W] fp32, masks uint8 [M,H,W], ``jobs`` a sequence of
    ``(frame, mask, type, blur_kernel, noise_std)`` with ``type`` a name of INTERVENTION_TYPES or its number, ``seeds`` one
    64-bit seed per job, ``src_index`` int32 [J,C,H*W] for shuffle jobs.  Returns ``(modified [J,C,H,W], intervention
    [J,C,H,W] or None, stats [J,4])``: stats = mask coverage, mean |image - modified|, max |image - modified|, mean |intervention|."""
    lib = _lib.load()
    if frames.dim() != 4:
        raise ValueError(f"frames must be [F,C,H,W], got {tuple(frames.shape)}")
    F_, Cc, H, W = frames.shape
    if not masks.is_cuda or masks.dtype != torch.uint8 or not masks.is_contiguous() or masks.dim() != 3 \
            or tuple(masks.shape[1:]) != (H, W) or masks.device != frames.device:
        raise ValueError(f"masks must be a contiguous uint8 [M,{H},{W}] tensor on {frames.device} (got {masks.dtype}, "
                         f"{tuple(masks.shape)}, {masks.device})")
    jobs = list(jobs)
    J = len(jobs)
    if J == 0:
        raise ValueError("no intervention jobs")
    table = (_lib.InterventionJob * J)()
    for j, (f, m, typ, k, std) in enumerate(jobs):
        if isinstance(typ, str):
            if typ not in INTERVENTION_TYPES:
                raise ValueError(f"unknown intervention type '{typ}' (one of {', '.join(INTERVENTION_TYPES)})")
            typ = INTERVENTION_TYPES[typ]
        table[j] = _lib.InterventionJob(int(f), int(m), int(typ), int(k), float(std))
    arr = _seed_array(seeds)
    if len(arr) != J:
        raise ValueError(f"{len(arr)} seeds for {J} jobs")
    if src_index is not None and (not src_index.is_cuda or src_index.dtype != torch.int32 or not src_index.is_contiguous()
                                  or tuple(src_index.shape) != (J, Cc, H * W) or src_index.device != frames.device):
        raise ValueError(f"src_index must be a contiguous int32 {(J, Cc, H * W)} tensor on {frames.device}")
    out = empty((J, Cc, H, W), dtype=torch.float32, device=frames.device)
    iv = empty_like(out) if with_intervention else None
    stats = empty((J, 4), dtype=torch.float32, device=frames.device)
    check(lib.sisic_intervene(context(frames.device), _ptr(frames, "frames"), F_, masks.data_ptr(), masks.shape[0], Cc, H, W, J,
                              table, arr, None if src_index is None else src_index.data_ptr(), out.data_ptr(),
                              None if iv is None else iv.data_ptr(), stats.data_ptr(), _stream(frames.device)))
    return out, iv, stats


def cfi_metrics(logits_orig: torch.Tensor, logits_mod: torch.Tensor, job_frame) -> torch.Tensor:
    """sisic_cfi_metrics: logits_orig [F,n], logits_mod [J,n], job_frame[j] = the row of logits_orig that job j modified.
    Returns the [J, 6n+7] rows documented in include/sisic.h."""
    lib = _lib.load()
    if logits_orig.dim() != 2 or logits_mod.dim() != 2 or logits_orig.shape[1] != logits_mod.shape[1]:
        raise ValueError(f"logits must be [F,n] and [J,n], got {tuple(logits_orig.shape)} and {tuple(logits_mod.shape)}")
    J, n = logits_mod.shape
    frames = [int(f) for f in job_frame]
    if len(frames) != J:
        raise ValueError(f"{len(frames)} frame indices for {J} rows of logits")
    rows = empty((J, CFI_PER_CLASS * n + CFI_TAIL), dtype=torch.float32, device=logits_mod.device)
    check(lib.sisic_cfi_metrics(context(logits_mod.device), _ptr(logits_orig, "logits_orig"), logits_orig.shape[0],
                                _ptr(logits_mod, "logits_mod"), J, n, (C.c_int * J)(*frames), rows.data_ptr(),
                                _stream(logits_mod.device)))
    return rows


RESAMPLE_MAX_VALUES = 4096   # n_top + n_bottom of sisic_resample_diffs (the values live in LDS)


def resample_diffs(top, bottom, seed: int, n_bootstrap: int, n_permutations: int, device="cuda"):
    """sisic_resample_diffs: ``(boot [n_bootstrap], perm [n_permutations])`` float64 device tensors (None for a count of 0) -- the
    mean differences of the bootstrap resamples (tag 3) and of the random relabellings (tag 4) of two samples, a function of
    ``(top, bottom, seed)`` alone (include/sisic.h states the draws)."""
    lib = _lib.load()
    device = torch.device(device)
    top = np.ascontiguousarray(np.asarray(top, dtype=np.float64).reshape(-1))
    bottom = np.ascontiguousarray(np.asarray(bottom, dtype=np.float64).reshape(-1))
    seed = int(seed)
    if seed < 0 or seed >> 64:
        raise ValueError("seed must be an integer in 0 .. 2**64-1")
    n_bootstrap, n_permutations = int(n_bootstrap), int(n_permutations)
    boot = empty(n_bootstrap, dtype=torch.float64, device=device) if n_bootstrap > 0 else None
    perm = empty(n_permutations, dtype=torch.float64, device=device) if n_permutations > 0 else None
    dp = C.POINTER(C.c_double)
    check(lib.sisic_resample_diffs(context(device), top.ctypes.data_as(dp), top.size, bottom.ctypes.data_as(dp), bottom.size,
                                   seed, n_bootstrap, n_permutations, None if boot is None else boot.data_ptr(),
                                   None if perm is None else perm.data_ptr(), _stream(device)))
    return boot, perm


# struct sisic_augment_params as a numpy record (96 bytes, the C layout)
AUGMENT_DTYPE = np.dtype([("src", "<i4"), ("crop_x", "<i4"), ("crop_y", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"),
                          ("hflip", "<i4"), ("vflip", "<i4"), ("order", "<i4", (3,)), ("factor", "<f4", (3,)),
                          ("rotate", "<i4"), ("rot", "<i4", (6,)), ("reserved", "<i4", (4,))])


def validate_augment_params(params: np.ndarray, N: int, H: int, W: int) -> None:
    """What sisic_augment cannot check itself (its records are in device memory): raises ``SisicError(SISIC_EINVAL)`` naming
    the first bad record -- src out of range, a box outside the image or larger than the output, an unknown operation."""
    def refuse(msg):
        raise _lib.SisicError(_lib.SISIC_EINVAL, "augment: " + msg)
    if H <= 0 or W <= 0 or H % 8 or W % 8:
        refuse(f"{H} x {W}: height and width must be positive multiples of 8")
    if params.dtype != AUGMENT_DTYPE or params.ndim != 1 or len(params) == 0:
        refuse("params must be a non-empty 1-D array of ops.AUGMENT_DTYPE records")
    checks = (
        ((params["src"] < 0) | (params["src"] >= N), lambda r: f"src {r['src']} of {N} images"),
        ((params["crop_w"] <= 0) | (params["crop_w"] > W) | (params["crop_h"] <= 0) | (params["crop_h"] > H),
         lambda r: f"a {r['crop_w']} x {r['crop_h']} box for a {W} x {H} output (only 0 < size <= output: down-scaling is refused)"),
        ((params["crop_x"] < 0) | (params["crop_y"] < 0) | (params["crop_x"].astype(np.int64) + params["crop_w"] > W)
         | (params["crop_y"].astype(np.int64) + params["crop_h"] > H),
         lambda r: f"box x {r['crop_x']} y {r['crop_y']} w {r['crop_w']} h {r['crop_h']} leaves the {W} x {H} image"),
        (((params["order"] < -1) | (params["order"] > 2)).any(axis=1),
         lambda r: f"order {r['order'].tolist()} (0 brightness, 1 contrast, 2 saturation, -1 skip)"),
        (~np.isfinite(params["factor"]).all(axis=1), lambda r: f"factor {r['factor'].tolist()} is not finite"),
    )
    for bad, describe in checks:
        if bad.any():
            i = int(np.argmax(bad))
            refuse(f"record {i}: " + describe(params[i]))


def augment(dataset: torch.Tensor, params: np.ndarray, *, u8: bool = False) -> torch.Tensor:
    """sisic_augment / sisic_augment_u8: ``dataset`` uint8 [N,H,W,3] on the GPU, ``params`` a host array of AUGMENT_DTYPE
    records (``data.draw_augment_params``).  Returns fp32 [B,3,H,W] in [-1,1], or with ``u8`` the uint8 [B,H,W,3] image PIL
    returns for the same parameters.  The records are validated here, then uploaded from pinned memory without blocking; the
    two launches run on the current stream and nothing synchronises with the host."""
    lib = _lib.load()
    if not dataset.is_cuda or dataset.dtype != torch.uint8 or not dataset.is_contiguous() or dataset.dim() != 4 \
            or dataset.shape[3] != 3:
        raise ValueError(f"dataset must be a contiguous uint8 [N,H,W,3] tensor on the GPU (got {dataset.dtype}, "
                         f"{tuple(dataset.shape)}, {dataset.device})")
    N, H, W, _ = dataset.shape
    params = np.ascontiguousarray(params)
    validate_augment_params(params, N, H, W)
    B = len(params)
    dev = dataset.device
    staged = torch.empty(B * AUGMENT_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
    staged.numpy()[:] = params.view(np.uint8)
    params_dev = staged.to(dev, non_blocking=True)
    scratch = empty(B, dtype=torch.int32, device=dev)
    if u8:
        out = empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        fn = lib.sisic_augment_u8
    else:
        out = empty((B, 3, H, W), dtype=torch.float32, device=dev)
        fn = lib.sisic_augment
    check(fn(context(dev), dataset.data_ptr(), N, H, W, params_dev.data_ptr(), B, scratch.data_ptr(), out.data_ptr(),
             _stream(dev)))
    return out


# ---- evaluation of generated sets (include/sisic.h; synt_isic_amd/evaluate.py builds the metrics on these) ------------------------
def _mat(t: torch.Tensor, name: str):
    """(pointer, rows, cols, leading dimension) of a row-major fp32 matrix on the GPU; rows may be strided (a column slice)"""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} must be a non-empty fp32 [rows, cols] tensor on the GPU (got {t.dtype}, {t.device}, "
                         f"{tuple(t.shape)})")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name} must be row-major with unit column stride (strides {t.stride()})")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    return t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(ld)


def _vec(t: Optional[torch.Tensor], n: int, name: str) -> Optional[int]:
    if t is None:
        return None
    if t.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {tuple(t.shape)}")
    return _ptr(t, name)


def col_means(x: torch.Tensor) -> torch.Tensor:
    """sisic_col_means: the column means of ``x`` [n,d] as float64 [d], summed in double in a fixed order."""
    p, n, d, ld = _mat(x, "x")
    out = empty(d, dtype=torch.float64, device=x.device)
    a = _lib.ColMeansArgs(x=p, mean_out=out.data_ptr(), stream=_stream(x.device), ld=ld, n=n, d=d)
    check(_lib.load().sisic_col_means(context(x.device), C.byref(a)))
    return out


def gram(a: torch.Tensor, b: Optional[torch.Tensor] = None, *, mode: str = "dot", shift_a: Optional[torch.Tensor] = None,
         shift_b: Optional[torch.Tensor] = None, contract_rows: bool = False) -> torch.Tensor:
    """sisic_gram: ``f((a - shift_a) (b - shift_b)^T)`` [n,m] on the f32 matrix pipe, ``mode`` one of ``dot``, ``sqdist``
    (``max(0, |a'|^2 + |b'|^2 - 2 s)``) and ``poly3`` (``(s / d + 1)^3``); ``b`` None: ``a``.  The shifts (fp32 [d]) are
    subtracted while the operands are staged.  ``contract_rows``: ``(a - shift_a)^T (a - shift_a)`` [d,d] instead."""
    if mode not in _lib.GRAM_MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(_lib.GRAM_MODES)}")
    pa, n, d, lda = _mat(a, "a")
    pb, m, ldb = None, n, 0
    if b is not None:
        pb, m, db, ldb = _mat(b, "b")
        if db != d or b.device != a.device:
            raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} differ in row length or device")
    if contract_rows and (b is not None or shift_b is not None or mode != "dot"):
        raise ValueError("contract_rows computes (a - shift_a)^T (a - shift_a): no b, no shift_b, mode 'dot'")
    out = empty((d, d) if contract_rows else (n, m), dtype=torch.float32, device=a.device)
    g = _lib.GramArgs(a=pa, b=pb, shift_a=_vec(shift_a, d, "shift_a"), shift_b=_vec(shift_b, d, "shift_b"), out=out.data_ptr(),
                      stream=_stream(a.device), lda=lda, ldb=ldb, ldo=out.shape[1], n=n, m=m, d=d, mode=_lib.GRAM_MODES[mode],
                      contract_rows=1 if contract_rows else 0)
    check(_lib.load().sisic_gram(context(a.device), C.byref(g)))
    return out


def rows_topk(dist: torch.Tensor, k: int, *, col_offset: Optional[torch.Tensor] = None, skip_diagonal: bool = False):
    """sisic_rows_topk: per row of ``dist`` [n,m] the ``k`` (1..8) smallest of ``dist[i,j] - col_offset[j]``, ascending, ties to
    the lower column, ``j == i`` left out with ``skip_diagonal``: (values fp32 [n,k], columns int32 [n,k])."""
    p, n, m, ld = _mat(dist, "dist")
    k = int(k)
    val = empty((n, max(k, 1)), dtype=torch.float32, device=dist.device)
    idx = empty((n, max(k, 1)), dtype=torch.int32, device=dist.device)
    a = _lib.RowsTopkArgs(dist=p, col_offset=_vec(col_offset, m, "col_offset"), val_out=val.data_ptr(), idx_out=idx.data_ptr(),
                          stream=_stream(dist.device), ld=ld, n=n, m=m, k=k, skip_diagonal=1 if skip_diagonal else 0)
    check(_lib.load().sisic_rows_topk(context(dist.device), C.byref(a)))
    return val, idx


def pair_sqdist(a: torch.Tensor, b: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """sisic_pair_sqdist: ``sum_c (a[i,c] - b[idx[i,j],c])^2`` [n,k], the differences and the sum in double, stored as fp32."""
    pa, n, d, lda = _mat(a, "a")
    pb, nb, db, ldb = _mat(b, "b")
    if db != d or b.device != a.device:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} differ in row length or device")
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != n or idx.shape[1] < 1 or not idx.is_contiguous() \
            or idx.device != a.device:
        raise ValueError(f"idx must be a contiguous int32 [{n}, k] tensor on {a.device}, got {idx.dtype} {tuple(idx.shape)}")
    out = empty(tuple(idx.shape), dtype=torch.float32, device=a.device)
    g = _lib.PairSqdistArgs(a=pa, b=pb, idx=idx.data_ptr(), out=out.data_ptr(), stream=_stream(a.device), lda=lda, ldb=ldb, n=n,
                            nb=nb, d=d, k=int(idx.shape[1]))
    check(_lib.load().sisic_pair_sqdist(context(a.device), C.byref(g)))
    return out


def matrix_sum(x: torch.Tensor, exclude_diagonal: bool = False) -> torch.Tensor:
    """sisic_matrix_sum: the sum of ``x`` [n,m] (without the entries ``i == j`` if asked) as a float64 [1] on the device, summed
    in double in a fixed order."""
    p, n, m, ld = _mat(x, "x")
    out = empty(1, dtype=torch.float64, device=x.device)
    a = _lib.MatrixSumArgs(x=p, out=out.data_ptr(), stream=_stream(x.device), ld=ld, n=n, m=m,
                           exclude_diagonal=1 if exclude_diagonal else 0)
    check(_lib.load().sisic_matrix_sum(context(x.device), C.byref(a)))
    return out


_KINDS = {"conv3x3": 0, "conv1x1": 1, "groupnorm": 2, "attention": 3, "ddpm_step": 4, "other": 5,
          "conv3x3_winograd_main": 6, "conv3x3_winograd_bf16x3": 7}


def profile_enable(device, on: bool) -> None:
    check(_lib.load().sisic_profile_enable(context(device), int(on)))


def profile_reset(device) -> None:
    check(_lib.load().sisic_profile_reset(context(device)))


def profile_read(device) -> dict:
    """{kind: {"ms", "launches", "bytes", "flops", "flops_executed"}} accumulated since the last reset."""
    lib = _lib.load()
    out = {}
    for name, kind in _KINDS.items():
        ms, by, fl, fx = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        n = C.c_int64()
        check(lib.sisic_profile_read(context(device), kind, C.byref(ms), C.byref(n), C.byref(by), C.byref(fl),
                                     C.byref(fx)))
        out[name] = {"ms": ms.value, "launches": n.value, "bytes": by.value, "flops": fl.value,
                     "flops_executed": fx.value}
    return out
