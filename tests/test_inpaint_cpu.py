"""Host side of image-to-image and inpainting (no GPU): RePaint's resampling schedule, the edit rows, the refusals of the
public interface and the strength arithmetic, against the restatement of tests/inpaint_ref.py."""
import math

import numpy as np
import pytest
import torch

import inpaint_ref

from synt_isic_amd import sampler as smp
from synt_isic_amd import scheduler as sch

LENGTHS = {(12, 4, 2): 20, (12, 4, 1): 12, (12, 5, 3): 32, (12, 12, 2): 12, (12, 1, 2): 23, (20, 10, 2): 30,
           (250, 10, 10): 2410}


def _mirror(rule: str, T: int, **kw):
    if rule == "dpmsolver++":
        s = sch.HipDPMSolverMultistepScheduler(beta_schedule="squaredcos_cap_v2", timestep_spacing="leading", clip_sample=True, **kw)
    else:
        s = (sch.HipDDIMScheduler if rule == "ddim" else sch.HipDDPMScheduler)(beta_schedule="squaredcos_cap_v2", **kw)
    s.set_timesteps(T)
    return s


@pytest.mark.parametrize("case", sorted(LENGTHS))
def test_schedule_lengths(case):
    T, j, r = case
    got = sch.resample_schedule(T, j, r)
    assert len(got) == LENGTHS[case]
    assert len(got) == T + (r - 1) * j * len(range(0, T - j, j))
    assert got == inpaint_ref.resample_schedule(T, j, r)
    # the run is connected: a pass follows the previous one a level further down, or `jump` levels up from there
    for (i, jump), (nxt, _) in zip(got[:-1], got[1:]):
        assert nxt == i + 1 - jump
    assert got[0][0] == 0 and got[-1] == (T - 1, 0)


def test_the_listed_sequence():
    got = sch.resample_schedule(12, 4, 2)
    idx = [i for i, _ in got]
    assert idx == list(range(0, 8)) + list(range(4, 12)) + list(range(8, 12))
    assert [p for p, (_, j) in enumerate(got) if j] == [7, 15] and got[7] == (7, 4) and got[15] == (11, 4)
    assert sch.resample_schedule(12, 4, 1) == [(i, 0) for i in range(12)]


@pytest.mark.parametrize("bad", [(0, 4, 2), (12, 0, 2), (12, 4, 0), (12, -1, 2)])
def test_schedule_refusals(bad):
    with pytest.raises(ValueError):
        sch.resample_schedule(*bad)


@pytest.mark.parametrize("rule", ["ddpm", "ddim", "dpmsolver++"])
def test_rows_equal_the_restatement(rule):
    s = _mirror(rule, 12)
    schedule = sch.resample_schedule(12, 4, 2) if rule != "dpmsolver++" else [(i, 0) for i in range(12)]
    got = sch.edit_rows(s, schedule)
    want = inpaint_ref.edit_rows(s.alphas.numpy(), s.timesteps.tolist(), schedule, rule)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(schedule), 4)
    assert torch.equal(got, want)
    # the last level is the clean image; a pass without a jump leaves its result alone
    assert got[-1].tolist() == [1.0, 0.0, 1.0, 0.0]
    for (i, jump), row in zip(schedule, got.tolist()):
        if not jump:
            assert row[2:] == [1.0, 0.0]
        else:
            assert 0.0 < row[2] < 1.0 and 0.0 < row[3] < 1.0
    # ck, sk are the scalars of add_noise at the level the pass arrives at (abar of the next grid entry), which come from the
    # fp32 table: abar there is rounded at 6e-8, so sqrt(1 - abar) moves by up to 6e-8 / (2 sk) = 5e-6 at the smallest sk
    # of this grid (0.0064)
    for (i, _), row in zip(schedule, got.tolist()):
        if i + 1 < 12:
            a, c = s.add_noise_coefficients(s.timesteps[i + 1:i + 2])
            assert abs(row[0] - float(a)) <= 2e-7 and abs(row[1] - float(c)) <= 1e-5


def test_rows_of_a_grid_tail():
    """image-to-image keeps the last entries of the grid: the rows of the tail are the tail of the rows (ddpm, ddim), and
    DPM-Solver++ steps to its next grid entry"""
    for rule in ("ddpm", "ddim", "dpmsolver++"):
        full = _mirror(rule, 12)
        rows = sch.edit_rows(full, [(i, 0) for i in range(12)])
        tail = _mirror(rule, 12)
        tail.timesteps = tail.timesteps[6:]
        got = sch.edit_rows(tail, [(i, 0) for i in range(6)])
        assert torch.equal(got, rows[6:])
        assert torch.equal(got, inpaint_ref.edit_rows(tail.alphas.numpy(), tail.timesteps.tolist(), [(i, 0) for i in range(6)],
                                                      rule, n_grid=12))


def test_jump_is_the_product_of_the_alphas_it_composes():
    """full 1000-step DDPM grid, jump_length 3: ja^2 = the product of the three (1 - beta) the jump composes, 1e-12 relative in
    float64 before the rounding to fp32"""
    s = _mirror("ddpm", 1000)
    schedule = sch.resample_schedule(1000, 3, 2)
    rows = sch.edit_rows64(s, schedule)
    alphas = (1.0 - s.betas).numpy().astype(np.float64)
    n = 0
    for (i, jump), row in zip(schedule, rows):
        if not jump:
            continue
        t_prev = int(s.timesteps[i]) - 1                 # the level the pass arrives at: x_{t-1}; -1 is the clean image
        want = np.prod(alphas[t_prev + 1:t_prev + 4])    # forward steps t_prev+1, +2, +3
        assert abs(row[2] ** 2 - want) <= 1e-12 * want, (i, row[2] ** 2, want)
        assert abs(row[2] ** 2 + row[3] ** 2 - 1.0) <= 1e-12
        n += 1
    assert n == len(range(0, 997, 3))


@pytest.mark.parametrize("strength,steps", [(0.5, 6), (0.99, 11), (1.0, 12)])
def test_strength_arithmetic(strength, steps):
    assert smp.strength_steps(12, strength) == steps == min(int(12 * strength), 12)
    s = _mirror("ddpm", 12)
    assert s.timesteps[12 - steps:].tolist() == s.timesteps.tolist()[-steps:]


def test_strength_refusals():
    with pytest.raises(ValueError, match="no step"):
        smp.strength_steps(12, 0.01)
    for bad in (0.0, -0.5, 1.5, True, "0.5", float("nan")):
        with pytest.raises(ValueError):
            smp.strength_steps(12, bad)


def test_option_refusals():
    ok = dict(scheduler="ddpm", noise="device", has_image=True, has_mask=True, strength=1.0, jump_length=10, n_resample=1)
    smp.check_edit_options(**ok)
    smp.check_edit_options(**{**ok, "n_resample": 5})
    smp.check_edit_options(**{**ok, "scheduler": "ddim", "n_resample": 2})
    smp.check_edit_options(**{**ok, "scheduler": "dpmsolver++"})
    smp.check_edit_options(**{**ok, "has_mask": False, "strength": 0.5, "noise": "host"})
    smp.check_edit_options(**{**ok, "has_image": False, "has_mask": False})
    with pytest.raises(ValueError, match="device"):                    # a mask under host noise
        smp.check_edit_options(**{**ok, "noise": "host"})
    with pytest.raises(ValueError, match="ignore"):                    # image-to-image at full strength
        smp.check_edit_options(**{**ok, "has_mask": False})
    with pytest.raises(ValueError, match="DPM-Solver"):                # resampling under DPM-Solver++
        smp.check_edit_options(**{**ok, "scheduler": "dpmsolver++", "n_resample": 2})
    with pytest.raises(ValueError, match="init_image"):                # a mask without an image
        smp.check_edit_options(**{**ok, "has_image": False})
    with pytest.raises(ValueError, match="init_image"):
        smp.check_edit_options(**{**ok, "has_image": False, "has_mask": False, "strength": 0.5})
    with pytest.raises(ValueError):
        smp.check_edit_options(**{**ok, "has_mask": False, "strength": 0.5, "n_resample": 2})
    for key, bad in (("strength", 0.0), ("strength", 1.01), ("n_resample", 0), ("n_resample", 1.5), ("jump_length", 0)):
        with pytest.raises(ValueError):
            smp.check_edit_options(**{**ok, key: bad})
    # the loop's own refusal of a jump under DPM-Solver++, and the plain schedule it fills in
    with pytest.raises(ValueError, match="DPM-Solver"):
        smp.check_edit_schedule("dpmsolver++", sch.resample_schedule(12, 4, 2), 12)
    assert smp.check_edit_schedule("dpmsolver++", None, 4) == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert smp.check_edit_schedule("ddpm", sch.resample_schedule(12, 4, 2), 12) == sch.resample_schedule(12, 4, 2)
    with pytest.raises(ValueError):
        sch.edit_rows(_mirror("ddpm", 12), [(12, 0)])
    with pytest.raises(ValueError):
        sch.edit_rows(_mirror("ddpm", 12), [(2, 4)])               # would land above the grid


def test_image_and_mask_preparation():
    u8 = torch.randint(0, 256, (8, 8, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    img = smp.prepare_init_image(u8, 2, (3, 8, 8), "cpu")
    assert tuple(img.shape) == (2, 3, 8, 8) and img.dtype == torch.float32 and torch.equal(img[0], img[1])
    assert torch.equal(img[0], (u8.float() / 255.0 * 2.0 - 1.0).permute(2, 0, 1))
    f = torch.rand((2, 3, 8, 8)) * 2 - 1
    assert torch.equal(smp.prepare_init_image(f, 2, (3, 8, 8), "cpu"), f)
    assert tuple(smp.prepare_init_image(f[0], 3, (3, 8, 8), "cpu").shape) == (3, 3, 8, 8)
    m = smp.prepare_mask(torch.ones(8, 8), 2, (8, 8), "cpu")
    assert tuple(m.shape) == (2, 1, 8, 8) and m.dtype == torch.float32
    bad = f.clone()
    bad[1, 2, 3, 4] = float("nan")
    for call in (lambda: smp.prepare_init_image(bad, 2, (3, 8, 8), "cpu"),
                 lambda: smp.prepare_init_image(f, 3, (3, 8, 8), "cpu"),
                 lambda: smp.prepare_init_image(f, 2, (3, 8, 4), "cpu"),
                 lambda: smp.prepare_init_image(torch.zeros(8, 8, 3, dtype=torch.int64), 2, (3, 8, 8), "cpu"),
                 lambda: smp.prepare_mask(torch.ones(4, 8), 2, (8, 8), "cpu"),
                 lambda: smp.prepare_mask(torch.full((8, 8), 1.5), 2, (8, 8), "cpu"),
                 lambda: smp.prepare_mask(torch.ones(3, 1, 8, 8), 2, (8, 8), "cpu")):
        with pytest.raises(ValueError):
            call()


def test_epilogue_restatement_limits():
    """the stated order has the limits the GPU tests lean on: m = 0 returns u, m = 1 returns k, whatever the other operand"""
    g = torch.Generator().manual_seed(5)
    u, x0k, e1 = (torch.randn(2, 3, 4, 4, generator=g) for _ in range(3))
    row = (0.75, 0.5, 1.0, 0.0)
    assert torch.equal(inpaint_ref.edit_one(u, x0k, torch.zeros(2, 1, 4, 4), e1, None, row), u)
    k = torch.tensor(0.75) * x0k + torch.tensor(0.5) * e1
    assert torch.equal(inpaint_ref.edit_one(u, x0k, torch.ones(2, 1, 4, 4), e1, None, row), k)
    assert math.isclose(float(inpaint_ref.noise([7], 3, 5, (3, 4, 4)).std()), 1.0, rel_tol=0.5)
