"""The training objective on the GPU (include/sisic.h "training objective"): per-sample loss weights in
sisic_mse_loss, ``get_velocity``, the fused step under v- and x0-prediction with Min-SNR weights against the spelled-out
``diffusion_loss`` step, every gradient against torch.autograd over the CPU oracle, and no state left behind on a handle."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pred_ref
from test_gpu_train import GRAD_REL_MEDIAN, GRAD_REL_WORST, PRED_TOL, _grad_errors, batch  # noqa: F401  (batch: the fixture)

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
B = 2
N_CLASS, NULL = 5, 4


def _scheduler():
    from synt_isic_amd.scheduler import HipDDPMScheduler
    return HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")


def _new_model(sd, kind="epsilon", cond=False):
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel(prediction_type=kind, **(dict(num_class_embeds=N_CLASS) if cond else {}))
    m.load_state_dict(sd)
    return m.to(DEV)


def _equal(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def cond_sd():
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return synthetic_unet_state_dict(num_class_embeds=N_CLASS)


@pytest.fixture(scope="module")
def trainee(synthetic_sd):
    """a model with its training arenas: the handle sisic_mse_loss and the weight setter act on"""
    from synt_isic_amd.train import HipAdam
    m = _new_model(synthetic_sd)
    HipAdam(m, lr=1e-4)
    return m


# ---- 1. the weighted loss kernel -------------------------------------------------------------------------------------------
def _mse(lib, h, pred, target, grad_scale):
    """(loss [1], dpred [n]) of one sisic_mse_loss call, and the loss of a second call without dpred"""
    from synt_isic_amd._lib import check
    n = pred.numel()
    loss, loss_only = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    dpred = torch.full((n,), math.nan, device=DEV)
    check(lib.sisic_mse_loss(h, pred.data_ptr(), target.data_ptr(), n, grad_scale, loss.data_ptr(), dpred.data_ptr(), _stream()))
    check(lib.sisic_mse_loss(h, pred.data_ptr(), target.data_ptr(), n, grad_scale, loss_only.data_ptr(), None, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_only)                                    # dpred = NULL: the same loss
    return loss.cpu(), dpred.cpu()


@pytest.mark.parametrize("grad_scale", [1.0, 65536.0])
@pytest.mark.parametrize("nb,per", [(3, 105), (2, 3 * 32 * 32), (3, 174763)])
def test_weighted_mse_loss_kernel(trainee, nb, per, grad_scale):
    """(3, 105): a few blocks, samples that end inside a block; (2, 3072): the training shape of this file; (3, 174763): 524289
    elements, one into the second grid-stride trip of 2048 blocks.  dpred is the restatement bit for bit; the loss is held to
    1e-6 of float64, the bar tests/test_gpu_optimizer.py::test_mse_loss_kernel derives from the depth of the reduction, which
    is unchanged (the weighted kernel keeps the grid, the block tree and the final tree, and adds one rounding per term)."""
    from synt_isic_amd import _lib
    lib, h = _lib.load(), trainee.handle
    gen = torch.Generator().manual_seed(1000 + per % 977)
    n = nb * per
    pred, target = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    w = (1.0 - torch.rand(nb, generator=gen)) * 5.0                        # (0, 5]
    assert float(w.min()) > 0.0 and float(w.max()) <= 5.0
    dp, dt = pred.to(DEV), target.to(DEV)
    plain_loss, plain_dpred = _mse(lib, h, dp, dt, grad_scale)
    try:
        wc = w.contiguous()
        assert lib.sisic_unet_set_loss_weights(h, C.cast(wc.data_ptr(), _lib.c_float_p), nb) == 0
        loss, dpred = _mse(lib, h, dp, dt, grad_scale)
        ref_loss, ref_dpred = pred_ref.weighted_mse(pred.numpy().reshape(nb, per), target.numpy().reshape(nb, per), w.numpy(), grad_scale)
        rel = abs(loss.item() - ref_loss) / ref_loss
        print(f"weighted mse B={nb} per={per} grad_scale={grad_scale}: loss relative error {rel:.3e}")
        assert np.isfinite(dpred.numpy()).all() and np.array_equal(dpred.numpy(), ref_dpred.reshape(-1))
        assert rel <= 1e-6, (loss.item(), ref_loss)
        assert not torch.equal(loss, plain_loss)
        # n that is not B equal samples is refused while weights are set
        assert lib.sisic_mse_loss(h, dp.data_ptr(), dt.data_ptr(), n - 1, grad_scale, None, None, _stream()) == _lib.SISIC_EINVAL
        # weights of all ones: the bits of no weights
        ones = torch.ones(nb)
        assert lib.sisic_unet_set_loss_weights(h, C.cast(ones.data_ptr(), _lib.c_float_p), nb) == 0
        one_loss, one_dpred = _mse(lib, h, dp, dt, grad_scale)
        assert torch.equal(one_loss, plain_loss) and torch.equal(one_dpred, plain_dpred)
        # a weight that is not finite is refused and the table stays
        bad = torch.tensor([1.0] * (nb - 1) + [float("nan")])
        assert lib.sisic_unet_set_loss_weights(h, C.cast(bad.data_ptr(), _lib.c_float_p), nb) == _lib.SISIC_EINVAL
    finally:
        assert lib.sisic_unet_set_loss_weights(h, None, 0) == 0
    # cleared: the unweighted bits, at any n
    after_loss, after_dpred = _mse(lib, h, dp, dt, grad_scale)
    assert torch.equal(after_loss, plain_loss) and torch.equal(after_dpred, plain_dpred)
    unweighted_ref, unweighted_dpred = pred_ref.weighted_mse(pred.numpy().reshape(nb, per), target.numpy().reshape(nb, per), None, grad_scale)
    assert np.array_equal(plain_dpred.numpy(), unweighted_dpred.reshape(-1)) and abs(plain_loss.item() - unweighted_ref) <= 1e-6 * unweighted_ref
    assert lib.sisic_mse_loss(h, dp.data_ptr(), dt.data_ptr(), n - 1, grad_scale, None, None, _stream()) == 0


def test_a_stale_weight_table_is_an_error_in_the_fused_step(trainee):
    """weights for another batch size: SISIC_EINVAL before anything runs, never a silent loss"""
    from synt_isic_amd import _lib
    from synt_isic_amd.train import HipAdam, train_step_fused
    lib, h = _lib.load(), trainee.handle
    g = torch.Generator().manual_seed(5)
    images, noise = torch.rand((B,) + CHW, generator=g) * 2 - 1, torch.randn((B,) + CHW, generator=g)
    before = trainee.state_dict()
    three = torch.tensor([1.0, 2.0, 3.0])
    assert lib.sisic_unet_set_loss_weights(h, C.cast(three.data_ptr(), _lib.c_float_p), 3) == 0
    try:
        with pytest.raises(_lib.SisicError, match="3 loss weights are set, the batch is 2"):
            train_step_fused(trainee, _scheduler(), images, noise, torch.tensor([5, 640]), HipAdam(trainee, lr=1e-4))
    finally:
        assert lib.sisic_unet_set_loss_weights(h, None, 0) == 0
    assert int(lib.sisic_unet_train_steps(h)) == 0 and _equal(before, trainee.state_dict())


# ---- 2. get_velocity -------------------------------------------------------------------------------------------------------
def test_get_velocity_is_the_torch_formula_bit_for_bit():
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    g = torch.Generator().manual_seed(8)
    x0, nz = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1, torch.randn(4, 3, 16, 16, generator=g)
    t = torch.tensor([0, 37, 500, 999])
    for beta_schedule in ("squaredcos_cap_v2", "linear"):
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule=beta_schedule)
        acp = s.alphas_cumprod[t]
        sa, sb = (acp ** 0.5).reshape(-1, 1, 1, 1), ((1 - acp) ** 0.5).reshape(-1, 1, 1, 1)
        want = sa * nz - sb * x0                                           # DDPMScheduler.get_velocity
        got = s.get_velocity(x0.to(DEV), nz.to(DEV), t)
        assert torch.equal(got.cpu(), want)
        assert torch.equal(want, pred_ref.velocity(x0, nz, sa.reshape(-1), sb.reshape(-1)))
    assert HipDDIMScheduler.get_velocity is HipDDPMScheduler.get_velocity is HipDPMSolverMultistepScheduler.get_velocity


# ---- 3. the fused step against the spelled-out step ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def steps():
    """two training batches at B = 2, 32x32: (images, noise, timesteps, labels)"""
    g = torch.Generator().manual_seed(79)
    out = []
    for ts, labels in (([5, 640], [2, NULL]), ([999, 311], [0, 3])):
        images = torch.rand((B,) + CHW, generator=g) * 2 - 1
        noise = torch.randn((B,) + CHW, generator=g)
        out.append((images.to(DEV), noise.to(DEV), torch.tensor(ts), torch.tensor(labels)))
    return out


@pytest.mark.parametrize("kind,gamma,cond,ext", [("v_prediction", 5.0, False, False), ("sample", None, False, True),
                                                 ("v_prediction", 5.0, True, True), ("sample", None, True, False),
                                                 ("epsilon", 5.0, False, False)])
def test_fused_steps_equal_spelled_out_diffusion_loss_steps(synthetic_sd, cond_sd, steps, kind, gamma, cond, ext):
    """two optimizer steps: parameters, Adam moments and losses bit for bit; ext: with max_grad_norm and an EMA (the _ext entry)"""
    from synt_isic_amd.train import HipAdam, HipEMA, HipGradScaler, diffusion_loss, train_step_fused
    sd = cond_sd if cond else synthetic_sd
    scheduler = _scheduler()
    spelled, fused = _new_model(sd, kind, cond), _new_model(sd, kind, cond)
    spelled.train(), fused.train()
    opt_kw = dict(lr=1e-4, max_grad_norm=1.0) if ext else dict(lr=1e-4)
    opt_s = HipAdam(spelled, ema=HipEMA(spelled, decay=0.9999) if ext else None, **opt_kw)
    opt_f = HipAdam(fused, ema=HipEMA(fused, decay=0.9999) if ext else None, **opt_kw)
    scaler_s, scaler_f = (None, None) if ext else (HipGradScaler(), HipGradScaler())
    for images, noise, timesteps, labels in steps:
        lab = labels if cond else None
        out = spelled(scheduler.add_noise(images, noise, timesteps), timesteps, class_labels=lab).sample
        loss = diffusion_loss(out, images, noise, timesteps, scheduler, snr_gamma=gamma)
        opt_s.zero_grad(set_to_none=True)
        if ext:
            loss.backward()
            assert opt_s.step() is True
        else:
            scaler_s.scale(loss).backward()
            assert scaler_s.step(opt_s) is True
            scaler_s.update()
        value, taken = train_step_fused(fused, scheduler, images, noise, timesteps, opt_f, scaler_f, class_labels=lab, snr_gamma=gamma)
        assert taken and value == loss.item() and math.isfinite(value) and value > 0
        if ext:
            assert opt_s.grad_norm == opt_f.grad_norm and opt_s.grad_norm > 0
    sd1, sd2 = spelled.state_dict(), fused.state_dict()
    assert _equal(sd1, sd2) and not torch.equal(sd1["conv_in.weight"].cpu(), sd["conv_in.weight"])
    o1, o2 = spelled.optimizer_state(), fused.optimizer_state()
    assert o1["step"] == o2["step"] == 2 and _equal(o1["exp_avg"], o2["exp_avg"]) and _equal(o1["exp_avg_sq"], o2["exp_avg_sq"])
    if ext:
        assert _equal(opt_s.ema.shadow_params(), opt_f.ema.shadow_params())
    # nothing is left on either handle
    assert not getattr(spelled, "_loss_weights_set", False) and not getattr(fused, "_loss_weights_set", False)


# ---- 4. every gradient against autograd ------------------------------------------------------------------------------------
def test_gradients_under_v_and_min_snr_match_autograd_over_the_oracle(synthetic_sd, batch):
    """B = 2, 3x64x64, t = (37, 912), v-prediction with Min-SNR gamma = 5: the prediction and all 330 gradients against
    torch.autograd over oracle/unet.py with the same target and weights.  The backward pass is the epsilon objective's and
    linear in dpred, so the bars are tests/test_gpu_train.py's."""
    from oracle import ddpm as oddpm, unet as ounet
    from synt_isic_amd.train import HipAdam, diffusion_loss, min_snr_weights
    images, noise, timesteps = batch
    scheduler = _scheduler()
    w = min_snr_weights(scheduler, timesteps, 5.0, "v_prediction")
    assert bool((w > 0).all()) and bool((w < 1).all())
    # the reference: fp32 autograd on the CPU
    params = {k: v.detach().clone().requires_grad_(True) for k, v in synthetic_sd.items()}
    orc = oddpm.DDPMSchedulerOracle()
    acp = orc.alphas_cumprod[timesteps]
    target = pred_ref.velocity(images, noise, acp ** 0.5, (1 - acp) ** 0.5)
    with torch.enable_grad():
        ref_pred = ounet.unet_forward(params, orc.add_noise(images, noise, timesteps), timesteps)
        ref_loss = (w.reshape(-1, 1, 1, 1) * (ref_pred - target) ** 2).mean()
        ref_grads = dict(zip(params, torch.autograd.grad(ref_loss, list(params.values()))))
    ref_loss = float(ref_loss.detach())
    model = _new_model(synthetic_sd, "v_prediction")
    HipAdam(model.parameters(), lr=1e-4)
    model.train()
    di, dn = images.to(DEV), noise.to(DEV)
    out = model(scheduler.add_noise(di, dn, timesteps), timesteps).sample
    pred_err = (out.cpu() - ref_pred.detach()).abs().max().item()
    loss = diffusion_loss(out, di, dn, timesteps, scheduler, snr_gamma=5.0)
    loss.backward()
    grads = model.grads()
    assert list(grads) == list(ref_grads) and len(grads) == 330
    worst, median = _grad_errors(grads, ref_grads, "B2 64x64 v-prediction, Min-SNR 5")
    print(f"v / Min-SNR 5: prediction error {pred_err:.3e}, loss {loss.item():.6e} vs {ref_loss:.6e}, "
          f"gradient error worst {worst[0]:.3e} ({worst[1]}), median {median[0]:.3e}")
    assert pred_err <= PRED_TOL
    assert abs(loss.item() - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert worst[0] <= GRAD_REL_WORST, f"gradient of {worst[1]}: {worst[0]:.3e} of its own largest entry"
    assert median[0] <= GRAD_REL_MEDIAN, median


# ---- 5. nothing stays on the handle ----------------------------------------------------------------------------------------
def test_epsilon_after_v_with_weights_is_a_fresh_handles_step(synthetic_sd, steps):
    from synt_isic_amd import _lib
    from synt_isic_amd.train import HipAdam, train_step_fused
    lib = _lib.load()
    scheduler = _scheduler()
    images, noise, timesteps, _ = steps[0]
    used = _new_model(synthetic_sd)
    opt = HipAdam(used, lr=1e-4)
    w = torch.tensor([0.25, 3.0])
    used.set_prediction_type("v_prediction")
    assert lib.sisic_unet_set_loss_weights(used.handle, C.cast(w.data_ptr(), _lib.c_float_p), B) == 0
    v_loss, _ = train_step_fused(used, scheduler, images, noise, timesteps, opt)      # v, weighted: the table is the handle's
    used.set_prediction_type("epsilon")
    assert lib.sisic_unet_set_loss_weights(used.handle, None, 0) == 0
    used.load_state_dict(synthetic_sd)                                                # the weights and the moments of a new run
    fresh = _new_model(synthetic_sd)
    got = train_step_fused(used, scheduler, images, noise, timesteps, opt)
    want = train_step_fused(fresh, scheduler, images, noise, timesteps, HipAdam(fresh, lr=1e-4))
    assert got == want and got[0] != v_loss
    assert _equal(used.state_dict(), fresh.state_dict())
    o1, o2 = used.optimizer_state(), fresh.optimizer_state()
    assert o1["step"] == o2["step"] == 1 and _equal(o1["exp_avg"], o2["exp_avg"]) and _equal(o1["exp_avg_sq"], o2["exp_avg_sq"])
