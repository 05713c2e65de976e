"""Classifier guidance without a GPU: the restatement (tests/clf_guide_ref.py) against its own pins.

  * scale 0 is the unguided restatement, bit for bit, under every rule;
  * in float64, on a 1-D Gaussian prior with a logistic p(c|x), -eps_hat/sb is the analytic score of p(x_t) * p(c|x_t)^s;
  * the direction: x_prev(guided) - x_prev(plain) = kappa * g with kappa > 0 under every rule, measured in fp32 as a cosine of
    at least 1 - 1e-6 (the bar tests/test_gpu_clf_guide.py then holds the GPU to, at the same timestep and scale);
  * a planted sign error gives a cosine of -1, a planted omission of sb is off by its factor 1/sb.
"""
import math

import numpy as np
import pytest
import torch

import clf_guide_ref as ref
import ddim_ref
import dpmpp_ref
import pred_ref

NAMES = [n for n, _, _ in ref.RULES]


def _inputs(n=3 * 32 * 32, seed=5):
    g = torch.Generator().manual_seed(seed)
    eps, x, grad, z, hist = (torch.randn(n, generator=g) for _ in range(5))
    return eps, x, grad, z, hist * 0.5


def _steps(name, scale, clip=0.0, combine=None):
    rule, row = ref.direction_row(name)
    eps, x, grad, z, hist = _inputs()
    if combine is None:
        guided, _ = ref.guided_step(rule, eps, grad, scale, x, z, hist, row, clip)
    else:
        guided, _ = pred_ref.step_row(rule, combine(eps, grad, row[0], scale), x, z, hist, row, clip)
    plain, _ = pred_ref.step_row(rule, eps, x, z, hist, row, clip)
    return rule, row, guided, plain, grad


def test_the_combine_in_numpy_and_in_torch_agree():
    eps, _, grad, _, _ = _inputs()
    for sb, scale in ((0.7104, 0.7), (0.9655, -3.0), (0.0064, 10.0), (0.5, 0.0)):
        a = ref.combine(eps, grad, sb, scale)
        b = torch.from_numpy(ref.combine_np(eps.numpy(), grad.numpy(), sb, scale))
        assert torch.equal(a, b)
        assert a.dtype == torch.float32


@pytest.mark.parametrize("name", NAMES)
def test_scale_zero_is_the_unguided_restatement(name):
    for clip in (0.0, 1.0):
        rule, row, guided, plain, _ = _steps(name, 0.0, clip)
        assert torch.equal(guided, plain)
    # and the unguided restatement is the published rule's (tests/ddim_ref.py, tests/dpmpp_ref.py)
    eps, x, _, z, hist = _inputs()
    if rule == "ddim":
        assert torch.equal(plain, ddim_ref.step_row(eps, x, z, row, 1.0))
    elif rule == "dpmsolver++":
        assert torch.equal(plain, dpmpp_ref.step_row(eps, x, z, hist, row, 1.0)[0])


def test_order_two_rows_read_the_history():
    """the chosen step is second order under solver_order = 2 and first order under 1: both forms of the kernel are covered"""
    assert ref.direction_row("dpmpp-order2")[1][5] != 0.0 and ref.direction_row("dpmpp-order1")[1][5] == 0.0
    assert ref.direction_row("ddim-eta0")[1][4] == 0.0 and ref.direction_row("ddim-eta1")[1][4] != 0.0


def test_eps_hat_is_the_score_of_the_tilted_density():
    """x0 ~ N(0, s0^2), x_t = sa x0 + sb e: p(x_t) = N(0, v), v = sa^2 s0^2 + sb^2, so the exact eps is sb * x_t / v.
    p(c|x) = sigmoid(a x + b).  The score of p(x_t) p(c|x_t)^s is -x/v + s * d log p(c|x) / dx, and -eps_hat / sb must be it."""
    f64 = torch.float64
    x = torch.linspace(-3, 3, 41, dtype=f64)
    s0, a, b = 0.8, 1.7, -0.3
    for sb in (0.9655, 0.7104, 0.2691):
        sa = math.sqrt(1 - sb * sb)
        v = sa * sa * s0 * s0 + sb * sb
        eps = sb * x / v
        p = torch.sigmoid(a * x + b)
        g = a * p * (1 - p) / (p + 1e-8)                    # d log(p + 1e-8) / dx
        for s in (0.0, 1.0, 4.0, -2.0):
            eps_hat = ref.combine(eps, g, sb, s, dtype=f64)
            want = -x / v + s * g
            assert torch.allclose(-eps_hat / sb, want, rtol=1e-12, atol=1e-12)
            xr = x.clone().requires_grad_(True)             # the same score by autograd over the log-density
            pr = torch.sigmoid(a * xr + b)
            (-(xr * xr) / (2 * v) + s * torch.log(pr + 1e-8)).sum().backward()
            assert torch.allclose(xr.grad, want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_a_guided_step_moves_along_the_gradient(name):
    """the bar of the GPU direction test, met here by the restatement alone at the same timestep and scale"""
    rule, row, guided, plain, grad = _steps(name, ref.DIRECTION_SCALE)
    k = ref.DIRECTION_SCALE * row[0]
    assert 0.4 < k < 0.6                                    # scale * sb of order 0.5
    kappa = ref.kappa_over_k(rule, row) * k
    assert kappa > 0
    d = guided - plain
    cos = ref.cosine(d, grad)
    print(f"{name}: t index {ref.DIRECTION_STEP}, k = {k:.4f}, kappa = {kappa:.4f}, 1 - cos = {1 - cos:.3e}")
    assert cos >= ref.DIRECTION_COSINE
    # and its length is kappa's: the least-squares slope of d on g
    slope = float((d.double() @ grad.double()) / (grad.double() @ grad.double()))
    assert abs(slope / kappa - 1) < 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_kappa_is_positive_on_the_whole_grid(name):
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    rule, opt = next((r, o) for n, r, o in ref.RULES if n == name)
    for T in (6, 50, 1000):
        if rule == "ddpm":
            s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
            s.set_timesteps(T)
            tab = s.coefficient_table()
        elif rule == "ddim":
            s = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
            s.set_timesteps(T)
            tab = s.coefficient_table(opt["eta"])
        else:
            s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                               timestep_spacing="leading", solver_order=opt["solver_order"])
            s.set_timesteps(T)
            tab = s.coefficient_table()
        assert all(ref.kappa_over_k(rule, row) > 0 for row in tab.tolist()), (name, T)


@pytest.mark.parametrize("name", NAMES)
def test_a_planted_sign_error_points_the_other_way(name):
    wrong = lambda eps, g, sb, scale: eps + ref.guide_k(sb, scale) * g         # noqa: E731
    _, _, guided, plain, grad = _steps(name, ref.DIRECTION_SCALE, combine=wrong)
    assert ref.cosine(guided - plain, grad) <= -ref.DIRECTION_COSINE


@pytest.mark.parametrize("name", NAMES)
def test_a_planted_omission_of_sb_shows_by_its_factor(name):
    no_sb = lambda eps, g, sb, scale: eps - torch.tensor(scale, dtype=torch.float32) * g     # noqa: E731
    rule, row, guided, plain, grad = _steps(name, ref.DIRECTION_SCALE, combine=no_sb)
    _, _, right, _, _ = _steps(name, ref.DIRECTION_SCALE)
    gd = grad.double()
    slope = lambda d: float((d.double() @ gd) / (gd @ gd))                      # noqa: E731
    ratio = slope(guided - plain) / slope(right - plain)
    assert abs(ratio * row[0] - 1) < 1e-5 and abs(ratio - 1) > 0.3              # off by 1 / sb = 1.41


def test_the_score_form_against_the_mean_shift_of_algorithm_1():
    """under DDPM the shift is scale * (c0 sb^2 / sa) * g; Alg. 1's is scale * sigma^2 * g.  The factor between them is
    (1 - abar_t) / ((1 - abar_prev) sqrt(alpha_t)) for the posterior variance: above 1, and 1 in the limit of small steps --
    within a few per cent on the 1000-step grid, several times on a 6-step one"""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    for T, hi in ((1000, 1.05), (6, math.inf)):
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        s.set_timesteps(T)
        tab = s.coefficient_table().tolist()
        mid = tab[len(tab) // 3: -max(2, len(tab) // 10)]                        # (sigma is 0 on the last row, tiny before it)
        f = [ref.mean_shift_factor(r) for r in mid]
        print(f"T = {T}: mean-shift factor between the score form and Alg. 1 over the middle of the grid: {min(f):.4f} .. {max(f):.4f}")
        assert 1.0 <= min(f) and max(f) <= hi


def test_the_training_noise_draws_are_a_pure_function_of_their_position():
    """train.classifier_noise_draws (host logic): image b's timestep and z seed depend on (seed, epoch, batch index, b) alone,
    the timesteps cover the inclusive range, and the tag is one the device-noise contract lists for it"""
    import os
    from synt_isic_amd import train
    t8, s8 = train.classifier_noise_draws(5, 1, 2, 8, (100, 103))
    t3, s3 = train.classifier_noise_draws(5, 1, 2, 3, (100, 103))
    assert t8[:3].tolist() == t3.tolist() and s8[:3] == s3
    assert train.classifier_noise_draws(5, 1, 2, 8, (100, 103))[0].tolist() == t8.tolist()
    for other in ((6, 1, 2), (5, 2, 2), (5, 1, 3)):
        assert train.classifier_noise_draws(*other, 8, (100, 103))[1] != s8
    t, s = train.classifier_noise_draws(0, 0, 0, 4000, (100, 103))
    counts = np.bincount(t.numpy() - 100, minlength=4)
    assert counts.sum() == 4000 and counts.min() > 900 and len(set(s)) == 4000      # uniform on {100..103}: 1000 +- 3 sigma (82)
    assert train.classifier_noise_draws(0, 0, 0, 5, (7, 7))[0].tolist() == [7] * 5
    for bad in ((5, 1), (-1, 5), (0, 1000)):
        with pytest.raises(ValueError):
            train.classifier_noise_draws(0, 0, 0, 1, bad)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sisic.h")).read()
    assert f"tag {train.CLASSIFIER_NOISE_TAG}: the z of a noised classifier-training batch" in header
