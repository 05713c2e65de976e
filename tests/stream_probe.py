"""Held-stream probe for the GPU suite (imported by test_gpu_streams.py, as philox_ref / poison are) and the registry of
its cases (plain data: test_stream_inventory.py reads it without a GPU).

include/sisic.h: "`stream` is a hipStream_t passed as void* (NULL = the default stream); all work is enqueued asynchronously
on it unless stated otherwise".  A launch, memset or copy that an entry point issues on stream 0 -- or on a stream of the
library's own that is not ordered behind the caller's -- goes unnoticed as long as every caller is on the null stream.  The
probe makes it visible: torch's side streams do not block against the null stream, so when the side stream is held by a
spin kernel, the inputs are copied in BEHIND the hold and the entry point is called right after, anything that does not wait
for the side stream reads the NaN the inputs were pre-filled with (or library memory that a warm call left other values in).

    hold(stream, ms)                       occupy ``stream`` for at least ``ms``; returns an event recorded behind the hold
    run_held(fn, make_inputs, warm_inputs) baseline on the default stream, warm call and held call on a fresh side stream;
                                           returns (baseline, held result, held-until-return flag)
    same(a, b)                             torch.equal over nested results (NaN never compares equal)

Nothing here loops or retries.
"""
import gc
import time

import torch

HOLD_FLOOR_MS = 30.0         # shortest hold: above the launch latency of the longest single enqueue by a wide margin
HOLD_MULT = 4.0              # the warm call's host time is a first call at its shape (allocations, table builds): the held
                             # call enqueues faster, so four times the warm call covers its whole enqueue
HOLD_CAP_MS = 600.0          # well under a second: a test stays quick whatever the warm call measured
_SPIN_MARGIN = 1.25          # "at least ms": the calibration ran at whatever clock the device had then

_calibration = {}


def _cycles_per_ms() -> float:
    """spin cycles of torch.cuda._sleep per millisecond, measured once per process between two events"""
    if "cycles_per_ms" not in _calibration:
        torch.cuda._sleep(1000)                  # loads the spin kernel
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 20_000_000
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        _calibration["cycles_per_ms"] = cycles / max(a.elapsed_time(b), 1e-3)
        print(f"stream_probe: {_calibration['cycles_per_ms']:.0f} spin cycles per ms")
    return _calibration["cycles_per_ms"]


def hold(stream: "torch.cuda.Stream", ms: float) -> "torch.cuda.Event":
    """Occupy ``stream`` with a spin kernel of at least ``ms`` milliseconds; the event returned is recorded behind it, so
    ``event.query()`` is False for as long as the hold lasts."""
    cycles = int(_cycles_per_ms() * float(ms) * _SPIN_MARGIN) + 1
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def hold_for(host_ms: float) -> float:
    """the hold that covers a call whose warm run took ``host_ms`` on the host"""
    return min(HOLD_CAP_MS, max(HOLD_FLOOR_MS, HOLD_MULT * host_ms))


def _poisoned(t):
    """a tensor of t's shape that no kernel may read: NaN for floats, another bit pattern for integers"""
    if not torch.is_tensor(t) or not t.is_cuda:
        return t
    if t.dtype.is_floating_point:
        return torch.full_like(t, float("nan"))
    return torch.full_like(t, 0x5A)


def same(a, b) -> bool:
    """torch.equal over tensors, tuples / lists / dicts of them and host scalars; a NaN anywhere is a difference"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype \
            and bool(torch.equal(a.detach().cpu(), b.detach().cpu()))
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b) \
            and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return bool(a == b)              # host numbers, strings; nan == nan is False, as wanted


def run_held(fn, make_inputs, warm_inputs, label: str = ""):
    """``fn(*inputs)`` three times: on the default stream (the baseline), on a fresh side stream with ``warm_inputs()`` (sizes
    every pool block, scratch buffer and table of the library at this shape and leaves OTHER values in them), and on that side
    stream again behind a hold, its inputs pre-filled with NaN and receiving their values behind the hold too.

    ``make_inputs()`` / ``warm_inputs()`` return a sequence of arguments; the tensors among them are device tensors.
    Returns ``(baseline, held result, held_until_return)``; the last is True when the hold's event had not passed when ``fn``
    returned, i.e. the call did not wait for the stream."""
    baseline = fn(*make_inputs())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    warm = list(warm_inputs())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        warm_out = fn(*warm)
        host_ms = (time.perf_counter() - t0) * 1e3
    side.synchronize()
    del warm_out
    real = list(make_inputs())
    held_in = [_poisoned(t) for t in real]
    torch.cuda.synchronize()
    ms = hold_for(host_ms)
    # No cyclic garbage collection between the hold and the query: a full collection of a process that holds the whole suite takes
    # ~100 ms on the host (measured: 95 ms right after collecting 1823 items), three times the shortest hold, and where one lands is
    # a matter of how many objects the tests before allocated -- it would be reported as a call that waited for its stream.
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            ev = hold(side, ms)
            for dst, src in zip(held_in, real):
                if torch.is_tensor(dst):
                    dst.copy_(src, non_blocking=True)
            out = fn(*held_in)
            held = not ev.query()
    finally:
        if gc_was_on:
            gc.enable()
    side.synchronize()
    print(f"stream_probe {label}: warm call {host_ms:.2f} ms on the host, hold {ms:.0f} ms, held until return: {held}")
    return baseline, out, held


# ---------------------------------------------------------------------------------------------------------------------------
# The registry.  name -> (entry points of include/sisic.h the case calls on the side stream, why the call may wait for the
# stream).  The second field is None for a call that must return while the stream is still held; otherwise it QUOTES the
# sentence of include/sisic.h that says the call synchronises (test_stream_inventory.py looks the quote up in the header).
# test_gpu_streams.py holds one builder per name; a name without a builder, or a builder without a name, fails the CPU suite.
SYNC_SCRATCH = "Synchronises the stream: the scratch is freed before the call returns."
SYNC_CANCEL = "A non-NULL cancel makes the call synchronise the stream before step 0 and before every eighth step after it"
SYNC_LOSS = "loss_out (host, may be NULL) receives the unscaled loss (one synchronisation)."
SYNC_EXT = "one 12-byte read-back (one synchronisation, also when found_inf is NULL)"
SYNC_RESTORE = "sisic_resnet_restore derives the filters of the loaded state dict again (the load path, blocking uploads)"
SYNC_RESAMPLE = "anything else is SISIC_EINVAL.  Synchronises the stream."

_PACK = ("sisic_conv_pack_weights",)
_WINO = ("sisic_conv_pack_weights", "sisic_conv_winograd_pack", "sisic_conv2d")

CASES = {
    # ---- kernels through ops (each conv case packs its filters inside the call: the packers run on the held stream too)
    "conv3x3_f32_direct": (_PACK + ("sisic_conv2d",), None),
    "conv3x3_winograd_bf16x3_cfg74": (_WINO, None),
    "conv3x3_winograd_ksplit_f32": (_WINO, None),
    "conv3x3_winograd_ksplit_bf16x3": (_WINO, None),
    "conv1x1_pointwise_bf16x3": (_PACK + ("sisic_conv2d",), None),
    "conv1x1_pointwise_bf16x3_ksplit": (_PACK + ("sisic_conv2d",), None),
    "conv3x3_stride2_bf16x3": (_PACK + ("sisic_conv_s2_pack", "sisic_conv2d"), None),
    "conv3x3_small_cout": (_PACK + ("sisic_conv2d",), None),
    "conv3x3_nearest2x_upsample": (_WINO, None),
    "groupnorm_stats": (("sisic_groupnorm_stats",), None),
    "groupnorm_finalize": (("sisic_groupnorm_finalize",), None),
    "conv2d_gn_rider": (_PACK + ("sisic_conv2d_gn_rider",), None),
    "attention_n100": (("sisic_attention",), None),
    "attention_n300": (("sisic_attention",), None),
    "ddpm_step": (("sisic_ddpm_step",), None),
    "ddpm_step_rng": (("sisic_ddpm_step_rng",), None),
    "ddpm_step_edit": (("sisic_ddpm_step_edit",), None),
    "ddim_step": (("sisic_ddim_step",), None),
    "ddim_step_rng": (("sisic_ddim_step_rng",), None),
    "ddim_step_edit": (("sisic_ddim_step_edit",), None),
    "dpmpp_step": (("sisic_dpmpp_step",), None),
    "dpmpp_step_rng": (("sisic_dpmpp_step_rng",), None),
    "dpmpp_step_edit": (("sisic_dpmpp_step_edit",), None),
    "guide_eps": (("sisic_guide_eps",), None),
    "noise_fill": (("sisic_noise_fill",), None),
    "noise_bits": (("sisic_noise_bits",), None),
    "denorm_u8": (("sisic_denorm_u8", "sisic_denorm_u8_form"), None),
    "conv2d_wgrad_winograd": (("sisic_conv2d_wgrad",), SYNC_SCRATCH),
    "conv2d_wgrad_direct_stride2": (("sisic_conv2d_wgrad",), SYNC_SCRATCH),
    "attention_bwd": (("sisic_attention_bwd",), None),
    "groupnorm_bwd": (("sisic_groupnorm_bwd",), SYNC_SCRATCH),
    "add_noise": (("sisic_add_noise",), None),
    "grad_stats": (("sisic_grad_stats",), SYNC_SCRATCH),
    "adam_ema": (("sisic_adam_ema",), None),
    "augment": (("sisic_augment", "sisic_augment_u8"), None),
    "intervene": (("sisic_intervene",), None),
    "cfi_metrics": (("sisic_cfi_metrics",), None),
    "mask_patches": (("sisic_mask_patches",), None),
    "resample_diffs": (("sisic_resample_diffs",), SYNC_RESAMPLE),
    # ---- UNet forward, B = 2 at 3x32x32 (the 8x8 level is inside)
    "unet_forward_default": (("sisic_unet_forward",), None),
    "unet_forward_latency": (("sisic_unet_forward",), None),
    "unet_forward_cond": (("sisic_unet_forward_cond",), None),
    # ---- sampling loops, B = 2 at 32x32, T = 6, eager and graph-replayed
    "loop_eager_ddpm_host": (("sisic_sample_frames_rule",), None),
    "loop_eager_ddim_host": (("sisic_sample_frames_rule",), None),
    "loop_eager_dpmpp_host": (("sisic_sample_frames_rule",), None),
    "loop_eager_ddpm_device": (("sisic_sample_frames_rule_rng",), None),
    "loop_eager_dpmpp_device": (("sisic_sample_frames_rule_rng",), None),
    "loop_eager_guided": (("sisic_sample_frames_cond",), None),
    "loop_eager_edit": (("sisic_sample_frames_edit",), None),
    "loop_eager_guided_edit": (("sisic_sample_frames_edit",), None),
    "loop_eager_traj_rows": (("sisic_sample_frames_rule",), None),
    "loop_eager_ddpm_entries": (("sisic_sample", "sisic_sample_frames", "sisic_sample_frames_rng"), None),
    "loop_eager_cancel_flag": (("sisic_sample_frames_rule_rng",), SYNC_CANCEL),
    "loop_graph_ddpm_host": (("sisic_sample_frames_rule",), None),
    "loop_graph_ddim_host": (("sisic_sample_frames_rule",), None),
    "loop_graph_dpmpp_host": (("sisic_sample_frames_rule",), None),
    "loop_graph_ddpm_device": (("sisic_sample_frames_rule_rng",), None),
    "loop_graph_dpmpp_device": (("sisic_sample_frames_rule_rng",), None),
    "loop_graph_guided": (("sisic_sample_frames_cond",), None),
    "loop_graph_edit": (("sisic_sample_frames_edit",), None),
    "loop_graph_guided_edit": (("sisic_sample_frames_edit",), None),
    "loop_graph_traj_rows": (("sisic_sample_frames_rule",), None),
    # ---- training, B = 2 at 32x32
    "train_spelled_out": (("sisic_unet_zero_grad", "sisic_add_noise", "sisic_unet_train_forward", "sisic_mse_loss",
                           "sisic_unet_backward", "sisic_unet_optimizer_step"), None),
    "train_step_fused": (("sisic_unet_train_step",), SYNC_LOSS),
    "train_step_ext_clip_ema": (("sisic_unet_train_step_ext",), SYNC_EXT),
    "optimizer_step_ext": (("sisic_unet_train_forward", "sisic_unet_optimizer_step_ext"), SYNC_EXT),
    "ema_step_and_swap": (("sisic_unet_ema_step", "sisic_unet_ema_swap", "sisic_unet_forward"), None),
    "train_cond_spelled_out": (("sisic_unet_train_forward_cond", "sisic_unet_backward", "sisic_unet_optimizer_step"), None),
    "train_step_cond": (("sisic_unet_train_step_cond",), SYNC_LOSS),
    # ---- classifier, B = 2 at 64x64
    "classifier_forward": (("sisic_resnet_forward",), None),
    "classifier_stem": (("sisic_resnet_stem",), None),
    "classifier_input_gradient": (("sisic_resnet_input_gradient",), None),
    "classifier_gradcam": (("sisic_resnet_gradcam",), None),
    "classifier_class_scores": (("sisic_resnet_forward", "sisic_class_scores"), None),
    "classifier_randomize_forward": (("sisic_resnet_randomize", "sisic_resnet_forward"), None),
    "classifier_restore_forward": (("sisic_resnet_restore", "sisic_resnet_forward"), SYNC_RESTORE),
    # ---- Python surface: generate() hands host arrays back and polls the sampler's stop flag
    "sampler_generate_host_noise": (("sisic_sample_frames_rule",), SYNC_CANCEL),
    "sampler_generate_host_noise_copy_stream": (("sisic_sample_frames_rule",), SYNC_CANCEL),
    "sampler_generate_device_noise": (("sisic_sample_frames_rule_rng",), SYNC_CANCEL),
}

# the other tests of test_gpu_streams.py that drive entry points on side streams
OTHER_TESTS = {
    "test_probe_sees_a_launch_on_the_null_stream": ("sisic_guide_eps",),
    "test_graph_key_follows_the_stream": ("sisic_sample_frames_rule_rng", "sisic_unet_graph_builds"),
    "test_item_table_filled_on_a_held_stream_is_not_read_by_another": ("sisic_conv2d",),
    "test_two_lanes_on_two_streams": ("sisic_sample_frames_rule",),
}

# entry points with a `void* stream` that no test above names, each with its reason
EXEMPT = {}
