"""Prediction types and Min-SNR weights without a GPU: the restatement tests/pred_ref.py against the three existing
restatements at epsilon, the algebra of the v and sample rules in float64, a toy problem whose exact predictors are known,
``train.min_snr_weights`` against its formulas, and the host-side refusals.

The float64 bound: a v step fed ``sa*eps - sb*x0`` and a sample step fed ``x0`` compute what the epsilon step fed ``eps``
computes, exactly in real arithmetic when sa^2 + sb^2 = 1.  In float64 each of about ten operations rounds at 1.1e-16 and the
epsilon rule amplifies by at most 1/sa^2 = 400 at the levels used (sa >= 0.05): about 1e-12 of the result, against the bound of
1e-9 of max|out|; a wrong sign or coefficient is an error of order one."""
import math
import os
import re

import numpy as np
import pytest
import torch

import ddim_ref
import dpmpp_ref
import pred_ref
from oracle.ddpm import DDPMSchedulerOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
TYPES = pred_ref.TYPES
BOUND = 1e-9

# every declaration of include/sisic.h with a `void* stream` at the parent of the commit that added the prediction types:
# the feature adds none (its state is set through stream-less setters)
STREAM_ENTRY_POINTS = """
sisic_adam_ema sisic_add_noise sisic_attention sisic_attention_bwd sisic_augment sisic_augment_u8 sisic_cfi_metrics
sisic_class_scores sisic_conv2d sisic_conv2d_gn_rider sisic_conv2d_wgrad sisic_conv_pack_weights sisic_conv_s2_pack
sisic_conv_winograd_pack sisic_ddim_step sisic_ddim_step_edit sisic_ddim_step_rng sisic_ddpm_step sisic_ddpm_step_edit
sisic_ddpm_step_rng sisic_denorm_u8 sisic_denorm_u8_form sisic_dpmpp_step sisic_dpmpp_step_edit sisic_dpmpp_step_rng
sisic_grad_stats sisic_groupnorm_bwd sisic_groupnorm_finalize sisic_groupnorm_stats sisic_guide_eps sisic_intervene
sisic_mask_patches sisic_mse_loss sisic_noise_bits sisic_noise_fill sisic_resample_diffs sisic_resnet_forward
sisic_resnet_gradcam sisic_resnet_input_gradient sisic_resnet_randomize sisic_resnet_restore sisic_resnet_stem
sisic_sample sisic_sample_frames sisic_sample_frames_cond sisic_sample_frames_edit sisic_sample_frames_rng
sisic_sample_frames_rule sisic_sample_frames_rule_rng sisic_unet_backward sisic_unet_ema_step sisic_unet_ema_swap
sisic_unet_forward sisic_unet_forward_cond sisic_unet_optimizer_step sisic_unet_optimizer_step_ext
sisic_unet_train_forward sisic_unet_train_forward_cond sisic_unet_train_step sisic_unet_train_step_cond
sisic_unet_train_step_ext sisic_unet_zero_grad
""".split()


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ---- 1. at epsilon the restatement is the three existing ones, bit for bit ------------------------------------------------
@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_epsilon_is_the_existing_restatements_bit_for_bit(clip):
    e, x, z, h = (_randn((2, 3, 8, 8), s) for s in (1, 2, 3, 4))
    # DDIM: rows of the cosine table at T = 20, eta 0 and 0.7, with and without use_clipped_model_output
    r = ddim_ref.DDIMSchedulerRef()
    r.set_timesteps(20)
    for eta in (0.0, 0.7):
        for t in (950, 500, 0):
            row = r.coefficients(t, eta)
            for flag in (False, True):
                for noise in (z, None):
                    want = ddim_ref.step_row(e, x, noise, row, clip, flag)
                    assert torch.equal(pred_ref.ddim_step_row(e, x, noise, row, clip, flag, "epsilon"), want), (t, eta, flag)
    # DPM-Solver++: first, interior (second-order) and last rows of both variants
    for alg in dpmpp_ref.ALGORITHMS:
        d = dpmpp_ref.DPMSolverRef("squaredcos_cap_v2", 2, alg, "linspace")
        d.set_timesteps(20)
        tab = d.table()
        for i in (0, 10, 19):
            row = tuple(float(v) for v in tab[i])
            want, want_hist = dpmpp_ref.step_row(e, x, z, h, row, clip)
            got, got_hist = pred_ref.dpmpp_step_row(e, x, z, h, row, clip, "epsilon")
            assert torch.equal(got, want) and torch.equal(got_hist, want_hist), (alg, i)
    # DDPM: the oracle's own step (clip_sample on or off), with the noise it adds at t > 0
    orc = DDPMSchedulerOracle(clip_sample=clip > 0, clip_sample_range=clip if clip > 0 else 1.0)
    orc.set_timesteps(50)
    for t in (980, 500, 20, 0):
        c = orc.coefficients(t)
        row = (c.sqrt_beta_prod_t, c.sqrt_alpha_prod_t, c.pred_original_coeff, c.current_sample_coeff, c.sigma)
        assert torch.equal(pred_ref.ddpm_step_row(e, x, z, row, clip, "epsilon"), orc.step(e, t, x, noise=z)), t


# ---- 2. the algebra in float64 ----------------------------------------------------------------------------------------------
def _abar64(beta_schedule="squaredcos_cap_v2"):
    return dpmpp_ref.alphas_cumprod(beta_schedule).numpy().astype(np.float64)


def _ddpm_row64(abar, t, prev_t):
    a_t, a_p = abar[t], (abar[prev_t] if prev_t >= 0 else 1.0)
    cur = a_t / a_p
    var = (1 - a_p) / (1 - a_t) * (1 - cur)
    return (math.sqrt(1 - a_t), math.sqrt(a_t), math.sqrt(a_p) * (1 - cur) / (1 - a_t), math.sqrt(cur) * (1 - a_p) / (1 - a_t),
            math.sqrt(var) if t > 0 else 0.0)


def _ddim_row64(abar, t, prev_t, eta):
    a_t, a_p = abar[t], (abar[prev_t] if prev_t >= 0 else 1.0)
    std = eta * math.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))
    return (math.sqrt(1 - a_t), math.sqrt(a_t), math.sqrt(a_p), math.sqrt(1 - a_p - std * std), std)


def _rows64(rule, abar, grid, eta=0.0):
    """float64 rows of a run over ``grid`` (descending timesteps, evenly spaced, ending at 0)"""
    stride = int(grid[0] - grid[1])
    if rule == "ddpm":
        return [_ddpm_row64(abar, int(t), int(t) - stride) for t in grid]
    if rule == "ddim":
        return [_ddim_row64(abar, int(t), int(t) - stride, eta) for t in grid]
    alg = "sde-dpmsolver++" if rule == "sde-dpmsolver++" else "dpmsolver++"
    return [tuple(r) for r in dpmpp_ref.table64(abar[np.asarray(grid)], 2, alg)]


RULES = ["ddpm", "ddim", "dpmsolver++", "sde-dpmsolver++"]


def _kind(rule):
    return "dpmsolver++" if rule.endswith("dpmsolver++") else rule


@pytest.mark.parametrize("beta_schedule", ["squaredcos_cap_v2", "linear"])
@pytest.mark.parametrize("rule", RULES)
def test_v_and_sample_steps_equal_the_epsilon_step_in_float64(rule, beta_schedule):
    abar = _abar64(beta_schedule)
    grid = np.arange(0, 1000, 50)[::-1].copy()
    grid = grid[np.sqrt(abar[grid]) >= 0.05]
    assert len(grid) >= 15 and grid[-1] == 0
    rows = _rows64(rule, abar, grid, eta=0.6)
    x0, eps, z, hist = (_randn((2, 3, 8, 8), s, F64) for s in (11, 12, 13, 14))
    assert any(r[4] != 0.0 for r in rows) == (rule != "dpmsolver++")
    for row in rows:
        sb, sa = torch.tensor(row[0], dtype=F64), torch.tensor(row[1], dtype=F64)
        assert float(sa) >= 0.05 and abs(float(sa * sa + sb * sb) - 1.0) < 1e-15
        x = sa * x0 + sb * eps
        outs = {}
        for kind in TYPES:
            o = pred_ref.model_output_of(kind, x0, eps, sa, sb)
            outs[kind], h = pred_ref.step_row(_kind(rule), o, x, z, hist, row, 0.0, kind, dtype=F64)
            if h is not None:
                assert float((h - x0).abs().max()) <= BOUND * float(x0.abs().max())       # hist is x0 under every type
        want = outs["epsilon"]
        scale = float(want.abs().max())
        for kind in ("sample", "v_prediction"):
            err = float((outs[kind] - want).abs().max())
            assert err <= BOUND * scale, (rule, kind, row, err / scale)
    # the check has teeth: the v rule with the sign of sb flipped is an error of order one
    row = rows[len(rows) // 2]
    sb, sa = torch.tensor(row[0], dtype=F64), torch.tensor(row[1], dtype=F64)
    x = sa * x0 + sb * eps
    wrong, _ = pred_ref.step_row(_kind(rule), -(sa * eps - sb * x0), x, z, hist, row, 0.0, "v_prediction", dtype=F64)
    right, _ = pred_ref.step_row(_kind(rule), eps, x, z, hist, row, 0.0, "epsilon", dtype=F64)
    assert float((wrong - right).abs().max()) > 1e-2 * float(right.abs().max())


def test_clipped_model_output_uses_the_clamped_x0_under_every_type():
    """with use_clipped_model_output the direction term is (x - sa*x0_clamped)/sb whatever the type: fed exact outputs, the
    three types still agree when the clamp is ON (it acts on the same x0)"""
    abar = _abar64()
    row = _ddim_row64(abar, 500, 450, 0.3)
    sb, sa = torch.tensor(row[0], dtype=F64), torch.tensor(row[1], dtype=F64)
    x0, eps, z = (_randn((2, 3, 8, 8), s, F64) for s in (21, 22, 23))
    x = sa * x0 + sb * eps
    outs = [pred_ref.ddim_step_row(pred_ref.model_output_of(k, x0, eps, sa, sb), x, z, row, 1.0, True, k, F64) for k in TYPES]
    assert float((x0.abs() > 1).double().mean()) > 0.1
    for o in outs[1:]:
        assert float((o - outs[0]).abs().max()) <= BOUND * float(outs[0].abs().max())
    # without the flag, a sample model's direction term uses the UNCLAMPED x0: it differs from the flagged form where x0 clamps
    plain = pred_ref.ddim_step_row(x0, x, z, row, 1.0, False, "sample", F64)
    assert float((plain - outs[1]).abs().max()) > 1e-3


# ---- 3. a toy problem with known exact predictors ---------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_a_whole_run_ends_at_the_same_sample_under_every_type(rule):
    """x0 ~ N(0, s^2): the exact predictors are linear in x,
        x0* = sa s^2 x / (sa^2 s^2 + sb^2),  eps* = (x - sa x0*) / sb,  v* = sa eps* - sb x0*,
    and a run of a rule fed the predictor of its type ends at the same sample under all three."""
    s2 = 0.5 ** 2
    abar = _abar64()
    grid = np.arange(0, 1000, 100)[::-1].copy()                  # t = 900 .. 0: sa(900) = 0.16
    rows = _rows64(rule, abar, grid, eta=0.5)
    x_T = _randn((2, 3, 8, 8), 31, F64)
    zs = _randn((len(grid), 2, 3, 8, 8), 32, F64)
    ends = {}
    for kind in TYPES:
        x, hist = x_T.clone(), None
        for i, row in enumerate(rows):
            sb, sa = torch.tensor(row[0], dtype=F64), torch.tensor(row[1], dtype=F64)
            x0s = sa * s2 * x / (sa * sa * s2 + sb * sb)
            epss = (x - sa * x0s) / sb
            o = {"epsilon": epss, "sample": x0s, "v_prediction": sa * epss - sb * x0s}[kind]
            x, hist = pred_ref.step_row(_kind(rule), o, x, zs[i], hist, row, 0.0, kind, dtype=F64)
        ends[kind] = x
    scale = float(ends["epsilon"].abs().max())
    assert scale > 1e-3 and torch.isfinite(ends["epsilon"]).all()
    for kind in ("sample", "v_prediction"):
        err = float((ends[kind] - ends["epsilon"]).abs().max())
        assert err <= BOUND * scale, (rule, kind, err / scale)


# ---- 4. Min-SNR weights -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta_schedule", ["squaredcos_cap_v2", "linear"])
def test_min_snr_weights_against_the_formulas(beta_schedule):
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import compute_snr, min_snr_weights
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule=beta_schedule)
    t = torch.tensor([0, 500, 999])
    abar = sched.alphas_cumprod.numpy().astype(np.float64)[[0, 500, 999]]
    snr = abar / (1.0 - abar)
    got_snr = compute_snr(sched, t)
    assert got_snr.dtype == torch.float64 and np.array_equal(got_snr.numpy(), snr) and np.isfinite(snr).all() and (snr > 0).all()
    for gamma in (5.0, 1.0, float("inf")):
        want = {"epsilon": np.minimum(snr, gamma) / snr, "v_prediction": np.minimum(snr, gamma) / (snr + 1.0),
                "sample": np.minimum(snr, gamma)}
        for kind in TYPES:
            w = min_snr_weights(sched, t, gamma, kind)
            assert w.dtype == torch.float32 and tuple(w.shape) == (3,) and torch.isfinite(w).all() and bool((w > 0).all())
            assert np.array_equal(w.numpy(), want[kind].astype(np.float32)), (kind, gamma)
    assert torch.equal(min_snr_weights(sched, t, float("inf"), "epsilon"), torch.ones(3))
    every = torch.arange(1000)
    assert bool((min_snr_weights(sched, every, 5.0, "v_prediction") <= 1.0).all())
    assert bool((min_snr_weights(sched, every, float("inf"), "v_prediction") <= 1.0).all())
    assert torch.equal(min_snr_weights(sched, every, float("inf"), "epsilon"), torch.ones(1000))
    if beta_schedule == "squaredcos_cap_v2":
        assert int((compute_snr(sched, every) < 5.0).sum()) == 739             # the figure of the feature's rationale
    with pytest.raises(ValueError):
        min_snr_weights(sched, t, 0.0, "epsilon")
    with pytest.raises(NotImplementedError):
        min_snr_weights(sched, t, 5.0, "flow")


# ---- 5. host-side refusals ---------------------------------------------------------------------------------------------------
def test_bad_type_strings_are_refused_on_the_host():
    from synt_isic_amd import _lib
    from synt_isic_amd.arch import UNetConfig
    from synt_isic_amd.unet import HipUNet2DModel
    assert [_lib.prediction_code(k) for k in TYPES] == [0, 1, 2]
    for bad in ("v", "eps", "V_PREDICTION", "", None, 2):
        with pytest.raises(NotImplementedError):
            _lib.prediction_code(bad)
        with pytest.raises(NotImplementedError):
            HipUNet2DModel(prediction_type=bad)
    m = HipUNet2DModel(prediction_type="v_prediction")
    assert m.prediction_type == "v_prediction" and m.config.prediction_type == "v_prediction"
    assert HipUNet2DModel().prediction_type == "epsilon" and UNetConfig().prediction_type == "epsilon"
    with pytest.raises(NotImplementedError):
        m.set_prediction_type("velocity")
    assert m.prediction_type == "v_prediction"                                  # a refused type leaves the setting
    assert m.set_prediction_type("sample") is m and m.prediction_type == "sample"
    # the type adds no tensors: the expected state dict is that of an epsilon model
    assert list(m._spec) == list(HipUNet2DModel()._spec)


def test_the_mirror_constructors_still_refuse_v_prediction():
    """the model owns what its output means; the mirrors take it per call (``step(..., prediction_type=)``)"""
    import inspect
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    for cls in (HipDDPMScheduler, HipDDIMScheduler, HipDPMSolverMultistepScheduler):
        for kind in ("v_prediction", "sample"):
            with pytest.raises(NotImplementedError):
                cls(prediction_type=kind)
        p = inspect.signature(cls.step).parameters["prediction_type"]
        assert p.default == "epsilon"
        assert callable(cls.get_velocity)
    from synt_isic_amd import ops
    with pytest.raises(NotImplementedError):                                   # refused before the device is looked at
        ops.context("cuda:0", "flow")


def test_the_header_declares_no_new_stream_entry_point():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sisic.h")).read(), flags=re.S)
    decls = re.findall(r"\b(sisic_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src)
    with_stream = sorted({name for name, params in decls if re.search(r"\bvoid\s*\*\s*stream\b", params)})
    assert with_stream == sorted(STREAM_ENTRY_POINTS) and len(with_stream) == 62
    declared = {name for name, _ in decls}
    new = {"sisic_unet_set_prediction_type", "sisic_unet_prediction_type", "sisic_unet_set_loss_weights",
           "sisic_set_step_prediction_type", "sisic_step_prediction_type"}
    assert new <= declared and not (new & set(with_stream))
    for name, value in (("SISIC_PRED_EPSILON", 0), ("SISIC_PRED_SAMPLE", 1), ("SISIC_PRED_V", 2), ("SISIC_ABI_VERSION", 3)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src), name
