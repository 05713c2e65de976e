"""ctypes binding of libsisic_hip.so (include/sisic.h).

This is the reference-side binding a SYNT_ISIC maintainer would add:
plain pointers and sizes, no torch types cross the boundary.  There is no CPU
fallback: if the library has not been built, ``load()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional

_LIB_PATH = os.environ.get("SISIC_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                             "libsisic_hip.so")
_lib: Optional[C.CDLL] = None

ABI_VERSION = 3          # include/sisic.h SISIC_ABI_VERSION

SISIC_OK = 0
SISIC_EINVAL = -1
SISIC_EHIP = -2
SISIC_ESTATE = -3
SISIC_ECANCEL = -4


class StepRule(NamedTuple):
    """One step rule of the sampling loop, as every layer above the C ABI needs it described."""
    name: str                   # the public name: ``scheduler=`` of generate(), the ``rule`` of a scheduler mirror
    id: int                     # SISIC_RULE_*
    row_width: int              # SISIC_RULE_ROW_WIDTH: floats per row of its coefficient table
    stem: str                   # sisic_<stem>_step, sisic_<stem>_step_rng, sisic_<stem>_step_edit
    title: str                  # as messages spell it
    takes_hist: bool            # its step reads and writes the previous step's x0
    clipped_output_flag: int    # SISIC_RULE_FLAG_CLIPPED_OUTPUT where its step takes use_clipped_model_output, else 0


# the one place a rule is described; everything below, ops._step, the scheduler mirrors and the sampler read it
RULES = {r.name: r for r in (StepRule("ddpm", 0, 5, "ddpm", "DDPM", False, 0),
                             StepRule("ddim", 1, 5, "ddim", "DDIM", False, 1),
                             StepRule("dpmsolver++", 2, 6, "dpmpp", "DPM-Solver++", True, 0))}
RULE_DDPM, RULE_DDIM, RULE_DPMPP = (r.id for r in RULES.values())
RULE_FLAG_CLIPPED_OUTPUT = RULES["ddim"].clipped_output_flag
RULE_ROW_WIDTH = {r.id: r.row_width for r in RULES.values()}
STEP_FORMS = ("", "_rng", "_edit")      # suffix of the entry: z from a buffer; drawn in the kernel; that plus the edit epilogue


def _step_argtypes(rule: StepRule, form: str) -> list:
    """the argument types of ``sisic_<stem>_step<form>`` in the order include/sisic.h declares (``ops._step`` fills them)"""
    p, f = C.c_void_p, C.c_float
    tensors = [p, p] + [p] * (form == "") + [p] * rule.takes_hist + [p]             # eps, x, [z], [hist], out
    size = [C.c_int64] if form == "" else [C.c_int, C.c_int64, p, C.c_uint32]       # n, or B, n_per_image, seeds, step
    scalars = [f] * (rule.row_width + 1) + [C.c_int] * bool(rule.clipped_output_flag)   # the row, clip, [flag]
    edit = [p, p, C.c_int, C.c_int64, f, f, f, f] if form == "_edit" else []        # x0k, mask, C, HW, ck, sk, ja, jb
    return [p] + tensors + size + scalars + edit + [p]                              # ctx ... stream


# what a model's output means (SISIC_PRED_*), under the names diffusers gives the three types
PRED_EPSILON = 0
PRED_SAMPLE = 1
PRED_V = 2
PREDICTION_TYPES = {"epsilon": PRED_EPSILON, "sample": PRED_SAMPLE, "v_prediction": PRED_V}


def prediction_code(prediction_type: str) -> int:
    """SISIC_PRED_* of a diffusers ``prediction_type`` string; anything else is NotImplementedError."""
    try:
        return PREDICTION_TYPES[prediction_type]
    except (KeyError, TypeError):
        raise NotImplementedError(f"prediction_type {prediction_type!r}: one of {sorted(PREDICTION_TYPES)}") from None

c_float_p = C.POINTER(C.c_float)
c_int64_p = C.POINTER(C.c_int64)


class ConvArgs(C.Structure):
    """struct sisic_conv_args"""
    _fields_ = [
        ("in0", C.c_void_p), ("in1", C.c_void_p),
        ("c0", C.c_int), ("c1", C.c_int),
        ("B", C.c_int), ("Hin", C.c_int), ("Win", C.c_int),
        ("upsample", C.c_int), ("ksize", C.c_int), ("stride", C.c_int),
        ("w_packed", C.c_void_p), ("bias", C.c_void_p), ("Cout", C.c_int),
        ("gn_scale", C.c_void_p), ("gn_shift", C.c_void_p), ("gn_silu", C.c_int),
        ("chan_bias", C.c_void_p), ("chan_bias_stride", C.c_int),
        ("residual", C.c_void_p), ("relu", C.c_int),
        ("out", C.c_void_p), ("tile_cfg", C.c_int),
        ("w_winograd", C.c_void_p),
        ("stats_out", C.c_void_p),
        ("fin_gamma", C.c_void_p), ("fin_beta", C.c_void_p), ("fin_groups", C.c_int), ("fin_eps", C.c_float),
        ("fin_scale", C.c_void_p), ("fin_shift", C.c_void_p), ("fin_mean_rstd", C.c_void_p),
    ]


class UNetConfigC(C.Structure):
    """struct sisic_unet_config"""
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int),
        ("layers_per_block", C.c_int), ("n_blocks", C.c_int),
        ("block_out_channels", C.c_int * 8),
        ("down_attn", C.c_int * 8), ("up_attn", C.c_int * 8),
        ("norm_groups", C.c_int), ("norm_eps", C.c_float), ("head_dim", C.c_int),
        ("n_freqs", C.c_int), ("freqs", c_float_p),
    ]


class InterventionJob(C.Structure):
    """struct sisic_intervention_job"""
    _fields_ = [("frame", C.c_int), ("mask", C.c_int), ("type", C.c_int), ("blur_kernel", C.c_int),
                ("noise_std", C.c_float)]


class AugmentParams(C.Structure):
    """struct sisic_augment_params (96 bytes; synt_isic_amd.ops.AUGMENT_DTYPE is the numpy form)"""
    _fields_ = [("src", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32),
                ("crop_h", C.c_int32), ("hflip", C.c_int32), ("vflip", C.c_int32), ("order", C.c_int32 * 3),
                ("factor", C.c_float * 3), ("rotate", C.c_int32), ("rot", C.c_int32 * 6), ("reserved", C.c_int32 * 4)]


class OptimExt(C.Structure):
    """struct sisic_optim_ext (16 bytes, no padding)"""
    _fields_ = [("ema_decay", C.c_double), ("max_grad_norm", C.c_float), ("ema_update", C.c_int)]


class GradStats(C.Structure):
    """the record sisic_grad_stats writes (3 x 4 bytes)"""
    _fields_ = [("total_norm", C.c_float), ("clip_coef", C.c_float), ("found_inf", C.c_int)]


class ResnetTrainArgs(C.Structure):
    """struct sisic_resnet_train_args (104 bytes, no padding)"""
    _fields_ = [("x", C.c_void_p), ("labels", c_int64_p), ("class_weights", c_float_p), ("logits_out", C.c_void_p),
                ("stream", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("preprocess", C.c_int), ("max_grad_norm", C.c_float),
                ("loss", C.c_float), ("grad_norm", C.c_float), ("found_inf", C.c_int)]


class ResnetTargetsArgs(C.Structure):
    """struct sisic_resnet_targets_args (56 bytes, no padding)"""
    _fields_ = [("x", C.c_void_p), ("targets", c_int64_p), ("grad_x", C.c_void_p), ("logits_out", C.c_void_p),
                ("stream", C.c_void_p), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("reserved", C.c_int)]


class X0ThresholdArgs(C.Structure):
    """struct sisic_x0_threshold_args (80 bytes, no padding)"""
    _fields_ = [("eps", C.c_void_p), ("eps2", C.c_void_p), ("x", C.c_void_p), ("s", C.c_void_p), ("stream", C.c_void_p),
                ("n_per_image", C.c_int64), ("B", C.c_int), ("source", C.c_int), ("sb", C.c_float), ("sa", C.c_float),
                ("w", C.c_float), ("ratio", C.c_float), ("sample_max_value", C.c_float), ("reserved", C.c_float)]


class ClfGuideArgs(C.Structure):
    """struct sisic_clf_guide_args (48 bytes, no padding)"""
    _fields_ = [("eps", C.c_void_p), ("g", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p), ("n", C.c_int64),
                ("sb", C.c_float), ("scale", C.c_float)]


class SampleClfArgs(C.Structure):
    """struct sisic_sample_clf_args (136 bytes, no padding)"""
    _fields_ = [("x", C.c_void_p), ("timesteps", c_int64_p), ("coef", c_float_p), ("noise", C.c_void_p),
                ("seeds", C.POINTER(C.c_uint64)), ("classifier", C.c_void_p), ("targets", c_int64_p), ("traj", C.c_void_p),
                ("traj_row", C.POINTER(C.c_int)), ("out_u8", C.c_void_p), ("cancel", C.POINTER(C.c_int)), ("stream", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("T", C.c_int), ("rule", C.c_int), ("rule_flags", C.c_int),
                ("step0", C.c_int), ("steps_done", C.c_int), ("clip", C.c_float), ("scale", C.c_float)]


class BnArgs(C.Structure):
    """struct sisic_bn_args (152 bytes, no padding)"""
    _fields_ = [("y", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("residual", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("out", C.c_void_p), ("mean", C.c_void_p),
                ("invstd", C.c_void_p), ("g", C.c_void_p), ("act", C.c_void_p), ("dy", C.c_void_p), ("dgamma", C.c_void_p),
                ("dbeta", C.c_void_p), ("stream", C.c_void_p), ("momentum", C.c_double), ("eps", C.c_float), ("relu", C.c_int),
                ("B", C.c_int), ("C", C.c_int), ("HW", C.c_int), ("reserved", C.c_int)]


class ResnetBnConfig(C.Structure):
    """struct sisic_resnet_bn_config: mode 0 frozen BatchNorm, 1 batch statistics with ``momentum`` in (0, 1]"""
    _fields_ = [("mode", C.c_int), ("momentum", C.c_double)]


# epilogues of sisic_gram (SISIC_GRAM_*)
GRAM_DOT = 0
GRAM_SQDIST = 1
GRAM_POLY3 = 2
GRAM_MODES = {"dot": GRAM_DOT, "sqdist": GRAM_SQDIST, "poly3": GRAM_POLY3}


class ResnetFeaturesArgs(C.Structure):
    """struct sisic_resnet_features_args (40 bytes, no padding)"""
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("preprocess", C.c_int)]


class ColMeansArgs(C.Structure):
    """struct sisic_col_means_args (40 bytes, no padding)"""
    _fields_ = [("x", C.c_void_p), ("mean_out", C.c_void_p), ("stream", C.c_void_p), ("ld", C.c_int64), ("n", C.c_int),
                ("d", C.c_int)]


class GramArgs(C.Structure):
    """struct sisic_gram_args (96 bytes, no padding)"""
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("shift_a", C.c_void_p), ("shift_b", C.c_void_p), ("out", C.c_void_p),
                ("stream", C.c_void_p), ("lda", C.c_int64), ("ldb", C.c_int64), ("ldo", C.c_int64), ("n", C.c_int), ("m", C.c_int),
                ("d", C.c_int), ("mode", C.c_int), ("contract_rows", C.c_int), ("reserved", C.c_int)]


class RowsTopkArgs(C.Structure):
    """struct sisic_rows_topk_args (64 bytes, no padding)"""
    _fields_ = [("dist", C.c_void_p), ("col_offset", C.c_void_p), ("val_out", C.c_void_p), ("idx_out", C.c_void_p),
                ("stream", C.c_void_p), ("ld", C.c_int64), ("n", C.c_int), ("m", C.c_int), ("k", C.c_int),
                ("skip_diagonal", C.c_int)]


class PairSqdistArgs(C.Structure):
    """struct sisic_pair_sqdist_args (72 bytes, no padding)"""
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("idx", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("n", C.c_int), ("nb", C.c_int), ("d", C.c_int), ("k", C.c_int)]


class MatrixSumArgs(C.Structure):
    """struct sisic_matrix_sum_args (48 bytes, no padding)"""
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p), ("ld", C.c_int64), ("n", C.c_int), ("m", C.c_int),
                ("exclude_diagonal", C.c_int), ("reserved", C.c_int)]


# name -> (restype, argtypes); every symbol include/sisic.h declares
SIGNATURES = {
    "sisic_abi_version": (C.c_int, []),
    "sisic_last_error": (C.c_char_p, []),
    "sisic_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "sisic_destroy": (C.c_int, [C.c_void_p]),
    "sisic_conv_packed_numel": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "sisic_conv_pack_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sisic_conv_winograd_numel": (C.c_int64, [C.c_int, C.c_int]),
    "sisic_conv_winograd_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sisic_conv_s2_numel": (C.c_int64, [C.c_int, C.c_int]),
    "sisic_conv_s2_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sisic_conv2d": (C.c_int, [C.c_void_p, C.POINTER(ConvArgs), C.c_void_p]),
    "sisic_conv_stats_slots": (C.c_int, [C.POINTER(ConvArgs)]),
    "sisic_conv_finalizes": (C.c_int, [C.POINTER(ConvArgs)]),
    "sisic_conv_plan_info": (C.c_int, [C.POINTER(ConvArgs), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "sisic_groupnorm_finalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "sisic_conv2d_gn_rider": (C.c_int, [C.c_void_p, C.POINTER(ConvArgs), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "sisic_groupnorm_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "sisic_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sisic_denorm_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sisic_denorm_u8_form": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p]),
    "sisic_unet_create": (C.c_int, [C.c_void_p, C.POINTER(UNetConfigC), C.POINTER(C.c_void_p)]),
    "sisic_unet_create_cond": (C.c_int, [C.c_void_p, C.POINTER(UNetConfigC), C.c_int, C.POINTER(C.c_void_p)]),
    "sisic_unet_destroy": (C.c_int, [C.c_void_p]),
    "sisic_unet_num_tensors": (C.c_int, [C.c_void_p]),
    "sisic_unet_tensor_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "sisic_unet_load": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_int64_p]),
    "sisic_unet_set_latency_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "sisic_unet_set_graph_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "sisic_unet_graph_builds": (C.c_int64, [C.c_void_p]),
    "sisic_unet_forward": (C.c_int, [C.c_void_p, C.c_void_p, c_int64_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    "sisic_unet_forward_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int64_p, c_int64_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]),
    "sisic_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p, c_float_p,
                               C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                               C.c_void_p]),
    "sisic_sample_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p, c_float_p,
                                      C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.c_void_p]),
    "sisic_noise_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_uint64), C.c_uint32,
                                   C.c_uint32, C.c_void_p]),
    "sisic_noise_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_uint64), C.c_uint32,
                                   C.c_uint32, C.c_void_p]),
    "sisic_sample_frames_rng": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p, c_float_p,
                                          C.c_float, C.POINTER(C.c_uint64), C.c_int, C.c_void_p, C.POINTER(C.c_int),
                                          C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "sisic_sample_frames_rule": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p, c_float_p,
                                           C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                           C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "sisic_sample_frames_rule_rng": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p,
                                               c_float_p, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int,
                                               C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int),
                                               C.POINTER(C.c_int), C.c_void_p]),
    "sisic_sample_frames_cond": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p, c_float_p,
                                           C.c_float, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, c_int64_p,
                                           C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "sisic_guide_eps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p]),
    "sisic_clf_guide_eps": (C.c_int, [C.c_void_p, C.POINTER(ClfGuideArgs)]),
    "sisic_sample_frames_clf": (C.c_int, [C.c_void_p, C.POINTER(SampleClfArgs)]),
    "sisic_sample_frames_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int64_p, c_float_p,
                                           C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, c_int64_p, C.c_int,
                                           C.c_float, C.c_void_p, C.c_void_p, c_float_p, C.c_void_p, C.POINTER(C.c_int),
                                           C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "sisic_unet_train_begin": (C.c_int, [C.c_void_p]),
    "sisic_unet_train_end": (C.c_int, [C.c_void_p]),
    "sisic_add_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_int64, C.c_void_p]),
    "sisic_unet_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, c_int64_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p]),
    "sisic_unet_train_forward_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int64_p, c_int64_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_int, C.c_void_p]),
    "sisic_unet_set_dropout": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_uint32]),
    "sisic_unet_dropout_next_call": (C.c_uint32, [C.c_void_p]),
    "sisic_unet_set_prediction_type": (C.c_int, [C.c_void_p, C.c_int]),
    "sisic_unet_prediction_type": (C.c_int, [C.c_void_p]),
    "sisic_unet_set_loss_weights": (C.c_int, [C.c_void_p, c_float_p, C.c_int]),
    "sisic_set_step_prediction_type": (C.c_int, [C.c_void_p, C.c_int]),
    "sisic_set_step_thresholding": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "sisic_set_step_image_elems": (C.c_int, [C.c_void_p, C.c_int64]),
    "sisic_unet_set_thresholding": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "sisic_x0_threshold": (C.c_int, [C.c_void_p, C.POINTER(X0ThresholdArgs)]),
    "sisic_step_prediction_type": (C.c_int, [C.c_void_p]),
    "sisic_mse_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "sisic_unet_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "sisic_unet_zero_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sisic_unet_optimizer_step": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float,
                                            C.POINTER(C.c_int), C.c_void_p]),
    "sisic_unet_train_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int64_p, c_float_p, c_float_p, C.c_int,
                                        C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float,
                                        C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_void_p]),
    "sisic_unet_optimizer_step_ext": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float,
                                                C.POINTER(OptimExt), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p]),
    "sisic_unet_train_step_ext": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int64_p, c_float_p, c_float_p, C.c_int,
                                            C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float,
                                            C.POINTER(OptimExt), C.POINTER(C.c_float), C.POINTER(C.c_int),
                                            C.POINTER(C.c_float), C.c_void_p]),
    "sisic_unet_train_step_cond": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int64_p, c_int64_p, c_float_p, c_float_p,
                                             C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                             C.c_float, C.POINTER(OptimExt), C.POINTER(C.c_float), C.POINTER(C.c_int),
                                             C.POINTER(C.c_float), C.c_void_p]),
    "sisic_unet_ema_begin": (C.c_int, [C.c_void_p]),
    "sisic_unet_ema_step": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "sisic_unet_ema_swap": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sisic_unet_ema_active": (C.c_int, [C.c_void_p]),
    "sisic_grad_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "sisic_adam_ema": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_float, C.c_void_p,
                                 C.c_double, C.c_void_p]),
    "sisic_unet_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, C.c_int64]),
    "sisic_unet_write": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, C.c_int64]),
    "sisic_unet_train_steps": (C.c_int64, [C.c_void_p]),
    "sisic_conv2d_wgrad": (C.c_int, [C.c_void_p, C.POINTER(ConvArgs), C.c_void_p, C.c_void_p, C.c_void_p]),
    "sisic_attention_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p]),
    "sisic_groupnorm_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sisic_batchnorm_train": (C.c_int, [C.c_void_p, C.POINTER(BnArgs)]),
    "sisic_batchnorm_train_bwd": (C.c_int, [C.c_void_p, C.POINTER(BnArgs)]),
    "sisic_add_relu": (C.c_int, [C.c_void_p, C.POINTER(BnArgs)]),
    "sisic_resnet_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "sisic_resnet_destroy": (C.c_int, [C.c_void_p]),
    "sisic_resnet_num_tensors": (C.c_int, [C.c_void_p]),
    "sisic_resnet_tensor_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "sisic_resnet_load": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), c_int64_p]),
    "sisic_resnet_randomize": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p]),
    "sisic_resnet_restore": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sisic_resnet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p]),
    "sisic_resnet_stem": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sisic_resnet_input_gradient": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "sisic_resnet_input_gradient_targets": (C.c_int, [C.c_void_p, C.POINTER(ResnetTargetsArgs)]),
    "sisic_resnet_gradcam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "sisic_resnet_train_begin": (C.c_int, [C.c_void_p]),
    "sisic_resnet_train_end": (C.c_int, [C.c_void_p]),
    "sisic_resnet_loss_backward": (C.c_int, [C.c_void_p, C.POINTER(ResnetTrainArgs)]),
    "sisic_resnet_optimizer_step": (C.c_int, [C.c_void_p, C.POINTER(ResnetTrainArgs)]),
    "sisic_resnet_zero_grad": (C.c_int, [C.c_void_p]),
    "sisic_resnet_train_steps": (C.c_int64, [C.c_void_p]),
    "sisic_resnet_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, C.c_int64]),
    "sisic_resnet_write": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, C.c_int64]),
    "sisic_resnet_train_begin_bn": (C.c_int, [C.c_void_p, C.POINTER(ResnetBnConfig)]),
    "sisic_resnet_train_bn_mode": (C.c_int, [C.c_void_p]),
    "sisic_resnet_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "sisic_unet_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "sisic_class_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "sisic_mask_patches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "sisic_intervene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(InterventionJob), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "sisic_cfi_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int),
                                    C.c_void_p, C.c_void_p]),
    "sisic_resample_diffs": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, C.c_uint64,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sisic_augment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "sisic_augment_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "sisic_resnet_features": (C.c_int, [C.c_void_p, C.POINTER(ResnetFeaturesArgs)]),
    "sisic_col_means": (C.c_int, [C.c_void_p, C.POINTER(ColMeansArgs)]),
    "sisic_gram": (C.c_int, [C.c_void_p, C.POINTER(GramArgs)]),
    "sisic_rows_topk": (C.c_int, [C.c_void_p, C.POINTER(RowsTopkArgs)]),
    "sisic_pair_sqdist": (C.c_int, [C.c_void_p, C.POINTER(PairSqdistArgs)]),
    "sisic_matrix_sum": (C.c_int, [C.c_void_p, C.POINTER(MatrixSumArgs)]),
    "sisic_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "sisic_profile_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), c_int64_p, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sisic_profile_reset": (C.c_int, [C.c_void_p]),
}
SIGNATURES.update({f"sisic_{r.stem}_step{form}": (C.c_int, _step_argtypes(r, form))
                   for r in RULES.values() for form in STEP_FORMS})


def lib_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load the HIP library; raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} is missing: the HIP library has not been built and synt_isic_amd has no CPU "
            "fallback.  Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C synt_isic_amd/csrc`).")
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.sisic_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libsisic_hip.so ABI {lib.sisic_abi_version()} != {ABI_VERSION}; rebuild the library")
    _lib = lib
    return lib


class SisicError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libsisic_hip error {code}: {message}")
        self.code = code


def check(rc: int) -> None:
    if rc != SISIC_OK:
        msg = load().sisic_last_error()
        raise SisicError(rc, msg.decode("utf-8", "replace") if msg else "")
