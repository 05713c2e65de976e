"""The host side of clipping / EMA / learning-rate schedules (synt_isic_amd.train): the EMA decay schedule, the LambdaLR
mirror with the cosine lambda, argument validation.  No GPU: a HipEMA without a model is the schedule alone."""
import pytest
import torch

import optim_ext_ref as ref
from synt_isic_amd.train import HipAdam, HipEMA, HipLambdaLR, cosine_schedule_with_warmup

STEPS = [0, 1, 2, 10, 1000, 10 ** 6]


@pytest.mark.parametrize("update_after_step", [0, 5])
@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
def test_get_decay_is_the_published_formula(warmup, update_after_step):
    ema = HipEMA(None, decay=0.9999, use_ema_warmup=warmup, update_after_step=update_after_step)
    for step in STEPS + [update_after_step + 1, update_after_step + 2]:
        want = ref.get_decay(step, decay=0.9999, use_ema_warmup=warmup, update_after_step=update_after_step)
        assert ema.get_decay(step) == want, (step, ema.get_decay(step), want)
        assert 0.0 <= ema.get_decay(step) <= 0.9999
    # nothing is averaged until the step after update_after_step + 1
    assert ema.get_decay(update_after_step) == 0.0 and ema.get_decay(update_after_step + 1) == 0.0
    assert ema.get_decay(update_after_step + 2) > 0.0
    if not warmup:
        assert ema.get_decay(10 ** 6) == 0.9999                   # (1 + s) / (10 + s) has passed the clamp; the warm-up form has not


def test_get_decay_literal_values():
    ema = HipEMA(None)
    assert ema.get_decay(0) == 0.0 and ema.get_decay(1) == 0.0
    assert ema.get_decay(2) == 2 / 11
    assert ema.get_decay(10) == 10 / 19
    assert ema.get_decay(10 ** 6) == 0.9999                       # clamped to decay
    warm = HipEMA(None, use_ema_warmup=True)
    assert warm.get_decay(1) == 0.0
    assert warm.get_decay(2) == 1 - 2 ** -(2 / 3)
    assert HipEMA(None, decay=0.5, min_decay=0.3).get_decay(2) == 0.3      # clamped from below: 2/11 < 0.3
    assert HipEMA(None, decay=0.5, min_decay=0.3).get_decay(1000) == 0.5


def test_lambda_lr_with_the_cosine_lambda_equals_torch():
    """50 steps, warm-up 5, against torch.optim.lr_scheduler.LambdaLR on a throw-away SGD: equal doubles."""

    class _Opt:                                                   # what HipLambdaLR touches of a HipAdam
        lr = 1e-4

    lam = cosine_schedule_with_warmup(5, 50)
    want_lam = ref.cosine_lambda(5, 50)
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    theirs = torch.optim.lr_scheduler.LambdaLR(sgd, want_lam)
    opt = _Opt()
    ours = HipLambdaLR(opt, lam)
    assert ours.get_last_lr() == theirs.get_last_lr() == [0.0] and opt.lr == 0.0       # step 0 of the ramp
    seen = []
    for step in range(1, 51):
        sgd.step()
        theirs.step()
        ours.step()
        assert lam(step) == want_lam(step)
        assert ours.get_last_lr() == theirs.get_last_lr(), step
        assert opt.lr == sgd.param_groups[0]["lr"], step
        seen.append(opt.lr)
    assert seen[4] == 1e-4 and max(seen) == 1e-4                  # the ramp ends at the base rate
    assert seen[-1] == 0.0 or seen[-1] < 1e-19                    # cos(pi) = -1: the schedule ends at (numerically) zero
    assert all(a >= b for a, b in zip(seen[4:], seen[5:]))        # and falls monotonically after the warm-up


@pytest.mark.parametrize("kwargs", [dict(decay=-0.1), dict(decay=1.5), dict(decay=float("nan")), dict(min_decay=2.0)])
def test_ema_refuses_a_decay_outside_the_unit_interval(kwargs):
    with pytest.raises(ValueError):
        HipEMA(None, **kwargs)


@pytest.mark.parametrize("value", [-1.0, -1e-9, float("nan")])
def test_adam_refuses_a_negative_max_grad_norm(value):
    # validated before the model is looked at: no GPU needed
    with pytest.raises(ValueError):
        HipAdam(None, max_grad_norm=value)


def test_ema_without_a_model_has_no_shadow():
    ema = HipEMA(None)
    with pytest.raises(RuntimeError):
        ema.step()
    with pytest.raises(RuntimeError):
        ema.state_dict()
