"""ResnetBlock2D dropout on the GPU: h = conv2(dropout(silu(norm2(h)))) in every residual block of a tape-recording forward,
the masks regenerated from (seed, call, block, sample, element) in the backward pass (include/sisic.h, the mask contract).

Parity is against tests/dropout_ref.py -- the oracle's UNet with the published block's dropout line and the contract's mask,
differentiated by torch.autograd -- under the bars of tests/test_gpu_train.py (PRED_TOL, GRAD_REL_WORST, GRAD_REL_MEDIAN): the
mask is decided by integer words, so the GPU and the restatement drop the SAME elements and what remains is the rounding of the
same convolutions; a wrong mask, scale or block index gives errors of order one.  p = 0.25 makes inv_keep = 4/3 inexact, so a
second rounding of it would show.  Synthetic weights, batch 2; every case runs in seconds.

Measured on MI355X (profiles/r21): prediction 2.6e-6 / 2.7e-6 / 2.8e-6 / 1.8e-6 at 32x32 / 64x64 / 40x56 / conditional
(bar 5e-5), worst per-tensor relative gradient error 1.2e-5 / 1.5e-5 / 1.4e-5 / 1.1e-5 (bar 1e-4), median 5.1e-6 / 5.3e-6 /
6.5e-6 / 3.5e-6 (bar 5e-5): the figures of the undropped model, no bar moved.
"""
import numpy as np
import pytest
import torch

import dropout_ref
import stream_probe as sp
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)
from test_gpu_train import GRAD_REL_MEDIAN, GRAD_REL_WORST, PRED_TOL, _grad_errors

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 0.25
SEED = 0xC0FFEE0012345678          # both key words in use
N_CLASS = 3


def _sd(cond=False):
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return synthetic_unet_state_dict(num_class_embeds=N_CLASS) if cond else synthetic_unet_state_dict()


def _model(sd, **kw):
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel(**kw)
    m.load_state_dict(sd)
    return m.to(DEV)


def _batch(H, W, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, H, W, generator=g) * 2 - 1, torch.randn(B, 3, H, W, generator=g), torch.tensor([37, 912][:B])


def _scheduler():
    from synt_isic_amd.scheduler import HipDDPMScheduler
    return HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")


def _forward_backward(model, images, noise, t, labels=None):
    """one spelled-out forward and backward of the batch (host tensors in): prediction, loss, gradients on the host"""
    from synt_isic_amd.train import mse_loss
    model.train()
    noisy = _scheduler().add_noise(images.to(DEV), noise.to(DEV), t.to(DEV))
    pred = model(noisy, t, class_labels=labels).sample if labels is not None else model(noisy, t).sample
    loss = mse_loss(pred, noise.to(DEV))
    loss.backward()
    return pred.cpu(), loss.item(), model.grads()


def _launches():
    from synt_isic_amd import ops
    return {k: v["launches"] for k, v in ops.profile_read(DEV).items()}


# ---- 1. off is off ------------------------------------------------------------------------------------------------------
def test_zero_dropout_is_the_model_without(synthetic_sd):
    """set_dropout(0.0) against a model that never heard of dropout: the same prediction, the same 330 gradients and the same
    launch counts; and with p = 0.3 set, the eval() forward and a 4-step generate are those of a model without."""
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.train import HipAdam
    images, noise, t = _batch(32, 32, 301)
    plain, zero = _model(synthetic_sd), _model(synthetic_sd)
    HipAdam(plain, lr=1e-4), HipAdam(zero, lr=1e-4)
    zero.set_dropout(0.0, seed=SEED, first_call=9)
    _forward_backward(plain, images, noise, t), _forward_backward(zero, images, noise, t)       # shapes met: pools sized
    ops.profile_enable(DEV, True)
    try:
        counts = []
        for m in (plain, zero):
            ops.profile_reset(DEV)
            out = _forward_backward(m, images, noise, t)
            counts.append((_launches(), out))
    finally:
        ops.profile_enable(DEV, False)
    (n_plain, (pred_a, loss_a, grads_a)), (n_zero, (pred_b, loss_b, grads_b)) = counts
    assert n_plain == n_zero and sum(n_plain.values()) > 100, (n_plain, n_zero)
    assert torch.equal(pred_a, pred_b) and loss_a == loss_b
    assert len(grads_a) == 330 and all(torch.equal(grads_a[k], grads_b[k]) for k in grads_a)
    assert zero.dropout_next_call == 9                      # p == 0: the counter stands still

    s = Sampler("cuda:0")
    ref, drop = s.add_model("plain", synthetic_sd), s.add_model("drop", synthetic_sd, dropout=0.3)
    HipAdam(drop, lr=1e-4)
    drop.set_dropout(0.3, seed=SEED)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert torch.equal(drop.eval()(x, t).sample, ref.eval()(x, t).sample)
    drop.train()                                            # the sampling loops never record a tape, whatever the mode says
    a = s.generate_seeds("plain", [3, 4], T=4, size=(32, 32))
    b = s.generate_seeds("drop", [3, 4], T=4, size=(32, 32))
    assert torch.equal(a.latents, b.latents) and np.array_equal(a.images.cpu().numpy(), b.images.cpu().numpy())
    assert drop.dropout_next_call == 0


# ---- 2. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,cond", [(32, 32, False), (64, 64, False), (40, 56, False), (32, 32, True)],
                         ids=["32x32", "64x64", "40x56", "32x32-cond"])
def test_parity_with_the_restatement(H, W, cond):
    """32x32: the direct kernels at the deep levels (4x4); 64x64: every Winograd form with no GroupNorm prologue -- conv2
    forward, its transposed filters in backward-data, its weight gradient reading the dropped activation; 40x56: 5x7 planes,
    where a block of four elements straddles channels; the conditional model with labels [1, 0].  call = 3 through first_call."""
    from synt_isic_amd.train import HipAdam
    sd = _sd(cond)
    images, noise, t = _batch(H, W, 310 + H)
    labels = torch.tensor([1, 0]) if cond else None
    ref_loss, ref_grads, ref_pred = dropout_ref.loss_and_grads(sd, images, noise, t, labels, p=P, seed=SEED, call=3)
    m = _model(sd, dropout=P, **({"num_class_embeds": N_CLASS} if cond else {}))
    HipAdam(m, lr=1e-4)
    m.set_dropout(P, seed=SEED, first_call=3)
    pred, loss, grads = _forward_backward(m, images, noise, t, labels)
    perr = (pred - ref_pred).abs().max().item()
    worst, median = _grad_errors(grads, ref_grads, f"dropout B2 {H}x{W}{' cond' if cond else ''}")
    print(f"dropout parity {H}x{W} cond={cond}: pred {perr:.3e} loss {abs(loss - ref_loss):.3e} grad worst {worst[0]:.3e} "
          f"({worst[1]}) median {median[0]:.3e}")
    assert perr <= PRED_TOL, perr
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert list(grads) == list(ref_grads) and len(grads) == (331 if cond else 330)
    assert worst[0] <= GRAD_REL_WORST, f"gradient of {worst[1]}: {worst[0]:.3e} of its own largest entry"
    assert median[0] <= GRAD_REL_MEDIAN, median
    assert m.dropout_next_call == 4


# ---- 3. the counter ---------------------------------------------------------------------------------------------------------
def test_counter_and_seed(synthetic_sd):
    from synt_isic_amd.train import HipAdam
    images, noise, t = _batch(32, 32, 320)
    m = _model(synthetic_sd, dropout=P)
    HipAdam(m, lr=1e-4)
    m.set_dropout(P, seed=SEED)
    x = _scheduler().add_noise(images.to(DEV), noise.to(DEV), t.to(DEV))
    m.train()
    assert m.dropout_next_call == 0
    first = m(x, t).sample.clone()
    assert m.dropout_next_call == 1
    second = m(x, t).sample.clone()
    assert m.dropout_next_call == 2
    assert not torch.equal(first, second)                   # two consecutive training forwards of one batch: other masks
    quiet = m.eval()(x, t).sample.clone()
    assert m.dropout_next_call == 2                         # an eval forward draws nothing
    assert torch.equal(quiet, _model(synthetic_sd).eval()(x, t).sample)
    m.train()
    m.set_dropout(P, seed=SEED, first_call=1)
    assert torch.equal(m(x, t).sample, second) and m.dropout_next_call == 2      # call 1 again, bit for bit
    m.set_dropout(P, seed=SEED, first_call=0)
    assert torch.equal(m(x, t).sample, first)
    m.set_dropout(P, seed=SEED + 1, first_call=0)
    assert not torch.equal(m(x, t).sample, first)           # another seed, other masks


# ---- 4. fused equals spelled-out -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "clip+ema"])
def test_fused_step_equals_the_spelled_out_step(synthetic_sd, ext):
    """sisic_unet_train_step[_ext] against add_noise, forward, mse_loss, backward, optimizer.step from the same weights and
    (seed, call): the same loss and the same weights (and EMA), bit for bit."""
    from synt_isic_amd.train import HipAdam, HipEMA, HipGradScaler, mse_loss, train_step_fused
    images, noise, t = (v.to(DEV) for v in _batch(32, 32, 330))
    scheduler = _scheduler()

    def fresh():
        m = _model(synthetic_sd, dropout=P)
        ema = HipEMA(m, decay=0.9999) if ext else None
        opt = HipAdam(m, lr=1e-4, max_grad_norm=1.0 if ext else None, ema=ema)
        m.set_dropout(P, seed=SEED, first_call=5)
        return m.train(), opt, ema, HipGradScaler()

    spelled, opt, ema_a, scaler = fresh()
    loss = mse_loss(spelled(scheduler.add_noise(images, noise, t), t).sample, noise)
    opt.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    assert scaler.step(opt) is True
    scaler.update()
    fused, opt_f, ema_b, scaler_f = fresh()
    value, taken = train_step_fused(fused, scheduler, images, noise, t, opt_f, scaler_f)
    assert taken and value == loss.item(), (value, loss.item())
    assert spelled.dropout_next_call == 6 and fused.dropout_next_call == 6
    sd1, sd2 = spelled.state_dict(), fused.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert any(not torch.equal(sd1[k].cpu(), synthetic_sd[k]) for k in sd1)
    if ext:
        assert opt.grad_norm == opt_f.grad_norm
        e1, e2 = ema_a.shadow_params(), ema_b.shadow_params()
        assert all(torch.equal(e1[k], e2[k]) for k in e1)


# ---- 5. side stream ------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_on_a_held_side_stream(synthetic_sd):
    """The dropout launches go to the stream the training entry points receive: a forward plus backward on a held side stream,
    its inputs arriving behind the hold, returns the default-stream bits -- prediction, loss and all 330 gradients."""
    from synt_isic_amd.train import HipAdam, mse_loss
    t = torch.tensor([3, 871])
    models = [_model(synthetic_sd, dropout=P), _model(synthetic_sd, dropout=P)]      # [0] the baseline, [1] warm and held
    for m in models:
        HipAdam(m, lr=1e-4)
    calls = []

    def fn(noisy, noise):
        m = models[0 if not calls else 1].train()
        calls.append(1)
        m.set_dropout(P, seed=SEED, first_call=4)           # (host state only: every run is forward 4 of the stream)
        pred = m(noisy, t).sample
        loss = mse_loss(pred, noise)
        loss.backward()
        return pred, loss.detach()

    def gen(s):
        g = torch.Generator().manual_seed(340 + s)
        return [(torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(DEV), torch.randn(2, 3, 32, 32, generator=g).to(DEV)]

    baseline, held_out, held = sp.run_held(fn, lambda: gen(0), lambda: gen(1), label="dropout forward+backward")
    assert sp.same(baseline, held_out)
    g0, g1 = models[0].grads(), models[1].grads()
    assert len(g0) == 330 and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert any(g0[k].abs().max() > 0 for k in g0)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(synthetic_sd):
    from synt_isic_amd import _lib
    from synt_isic_amd.train import HipAdam
    images, noise, t = _batch(32, 32, 350)
    m = _model(synthetic_sd, dropout=P)
    x = _scheduler().add_noise(images.to(DEV), noise.to(DEV), t.to(DEV))
    # training mode, dropout > 0, no optimizer and so no arenas: an error, not an undropped prediction
    with pytest.raises(RuntimeError, match="no optimizer"):
        m.train()(x, t)
    HipAdam(m, lr=1e-4)
    m.set_dropout(P, seed=SEED, first_call=2)
    want = m.train()(x, t).sample.clone()
    m.set_dropout(P, seed=SEED, first_call=2)
    lib = _lib.load()
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert lib.sisic_unet_set_dropout(m.handle, bad, 99, 99) == _lib.SISIC_EINVAL, bad
        assert b"set_dropout" in lib.sisic_last_error()
    assert m.dropout_next_call == 2                         # the previous setting is still in force: p, seed and counter
    assert torch.equal(m(x, t).sample, want)
