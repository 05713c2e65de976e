"""The DDIM sampler, the part that needs no GPU: timestep grids, the coefficient table against the restatement
(tests/ddim_ref.py), the structure of the sigma column, the restatement itself against the DDPM oracle at eta = 1, the C ABI's
new entries, and what the public interface refuses before it touches the GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import ddim_ref
from oracle.ddpm import DDPMSchedulerOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sisic_ddim_step", "sisic_ddim_step_rng", "sisic_sample_frames_rule", "sisic_sample_frames_rule_rng")
SCHEDULES = ("linear", "squaredcos_cap_v2")


def _mirror(**kw):
    from synt_isic_amd.scheduler import HipDDIMScheduler
    return HipDDIMScheduler(**kw)


def test_timestep_lists():
    def ts(T, **kw):
        s = _mirror(beta_schedule="squaredcos_cap_v2", **kw)
        s.set_timesteps(T)
        r = ddim_ref.DDIMSchedulerRef(**kw)
        r.set_timesteps(T)
        assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == r.timesteps.tolist()
        return s.timesteps.tolist()
    assert ts(50) == list(range(980, -1, -20))
    assert ts(50, steps_offset=1) == list(range(981, 0, -20))
    assert ts(50, timestep_spacing="trailing") == list(range(999, 18, -20))
    assert ts(7, timestep_spacing="trailing") == [999, 856, 713, 570, 428, 285, 142]
    # prev_t is t - N // n under both spacings: the last trailing step of 7 lands on 0, not below it
    s = _mirror(timestep_spacing="trailing")
    s.set_timesteps(7)
    assert s.previous_timestep(142) == 0 and s.previous_timestep(999) == 857
    from synt_isic_amd.scheduler import HipDDPMScheduler
    d = HipDDPMScheduler()
    d.set_timesteps(50)
    assert ts(50) == d.timesteps.tolist()


@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("alpha_to_one", [True, False])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_coefficient_table_is_the_restatements(schedule, alpha_to_one, spacing):
    kw = dict(beta_schedule=schedule, set_alpha_to_one=alpha_to_one, timestep_spacing=spacing)
    s, r = _mirror(**kw), ddim_ref.DDIMSchedulerRef(**kw)
    for T in (1000, 50, 7):
        s.set_timesteps(T)
        r.set_timesteps(T)
        for eta in (0.0, 0.5, 1.0):
            got, want = s.coefficient_table(eta), r.table(eta)
            assert got.shape == (T, 5) and got.dtype == torch.float32
            assert torch.equal(got, want), (T, eta)
            assert s.step_coefficients(s.timesteps[T // 2], eta) == r.coefficients(r.timesteps[T // 2], eta)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_structure_of_the_table(schedule):
    from synt_isic_amd.scheduler import HipDDPMScheduler
    for T in (1000, 50, 20, 7):
        s, r = _mirror(beta_schedule=schedule), ddim_ref.DDIMSchedulerRef(beta_schedule=schedule)
        d = HipDDPMScheduler(beta_schedule=schedule)
        for o in (s, r, d):
            o.set_timesteps(T)
        for eta in (0.0, 0.5, 1.0):
            assert all(r.radicand(t, eta) >= 0.0 for t in r.timesteps), (T, eta)          # c_dir is never a NaN
            tab = s.coefficient_table(eta)
            assert torch.isfinite(tab).all()
            if eta == 0.0:
                assert (tab[:, 4] == 0).all()
            else:                                       # set_alpha_to_one: exactly the last step adds no noise, as under DDPM
                assert (tab[:-1, 4] != 0).all() and tab[-1, 4] == 0
        # eta = 1: the DDPM rule's sigma, bit for bit
        assert torch.equal(s.coefficient_table(1.0)[:, 4], d.coefficient_table()[:, 4])
        oracle = DDPMSchedulerOracle(beta_schedule=schedule)
        oracle.set_timesteps(T)
        assert [float(v) for v in s.coefficient_table(1.0)[:, 4]] == \
            [float(torch.tensor(oracle.coefficients(t).sigma, dtype=torch.float32)) for t in oracle.timesteps]
    # trailing spacing, 7 steps: the last step's prev_t is 0, so it still adds noise at eta > 0 (the published behaviour)
    s = _mirror(beta_schedule=schedule, timestep_spacing="trailing")
    s.set_timesteps(7)
    tab = s.coefficient_table(0.5)
    assert (tab[:, 4] != 0).all() and int((tab[:, 4] != 0).sum()) == 7
    assert (s.coefficient_table(0.0)[:, 4] == 0).all()


# 4x the largest differences measured when the rule was written down (8.2e-5 at T = 1000, 9.2e-6 at T = 50): the margin
# covers other draws, it is not an accuracy of the library.  A wrong radicand or an inverted variance moves this by >= 1e-2.
PIN_BOUND = {1000: 3.3e-4, 50: 3.7e-5}


@pytest.mark.parametrize("T", [1000, 50])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_restatement_is_the_ddpm_oracle_at_eta_1(schedule, T):
    """clip_sample=False, eta = 1: one DDIM step and one DDPM ancestral step from the same (x_t, eps, z) differ by rounding
    only, at every timestep of the run."""
    r = ddim_ref.DDIMSchedulerRef(beta_schedule=schedule, clip_sample=False)
    o = DDPMSchedulerOracle(beta_schedule=schedule, clip_sample=False)
    r.set_timesteps(T)
    o.set_timesteps(T)
    g = torch.Generator().manual_seed(1234)
    shape = (2, 3, 16, 16)
    worst, worst_t = 0.0, -1
    for t in r.timesteps:
        x0 = torch.rand(shape, generator=g) * 2 - 1
        e, z = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        x = o.add_noise(x0, e, torch.full((shape[0],), int(t)))
        d = (r.step(e, t, x, eta=1.0, noise=z) - o.step(e, t, x, noise=z)).abs().max().item()
        if d > worst:
            worst, worst_t = d, int(t)
    print(f"{schedule} T={T}: max |ddim_ref.step - DDPMSchedulerOracle.step| = {worst:.3e} at t = {worst_t}")
    assert worst < PIN_BOUND[T]


def test_header_declares_and_binding_table_binds_the_new_entries():
    from synt_isic_amd import _lib
    text = open(os.path.join(ROOT, "include", "sisic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sisic_[a-z0-9_]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/sisic.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert "#define SISIC_ABI_VERSION 3" in text and _lib.ABI_VERSION == 3                      # additive only
    for macro, value in (("SISIC_RULE_DDPM", _lib.RULE_DDPM), ("SISIC_RULE_DDIM", _lib.RULE_DDIM),
                         ("SISIC_RULE_FLAG_CLIPPED_OUTPUT", _lib.RULE_FLAG_CLIPPED_OUTPUT)):
        assert re.search(rf"#define {macro} {value}\b", text)
    sig = _lib.SIGNATURES
    # the twins of the DDPM entries: the flag right before the stream; rule and flags right behind clip
    assert sig["sisic_ddim_step"][1] == sig["sisic_ddpm_step"][1][:-1] + [C.c_int, C.c_void_p]
    assert sig["sisic_ddim_step_rng"][1] == sig["sisic_ddpm_step_rng"][1][:-1] + [C.c_int, C.c_void_p]
    for new, old in (("sisic_sample_frames_rule", "sisic_sample_frames"), ("sisic_sample_frames_rule_rng", "sisic_sample_frames_rng")):
        assert sig[new][1] == sig[old][1][:9] + [C.c_int, C.c_int] + sig[old][1][9:]


def test_library_exports_the_new_entries():
    from synt_isic_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name)
    # argument validation needs no GPU
    assert lib.sisic_ddim_step(None, None, None, None, None, 4, 0.6, 0.8, 0.3, 0.69, 0.25, 1.0, 0, None) == _lib.SISIC_EINVAL
    assert b"ddim_step" in lib.sisic_last_error()
    assert lib.sisic_ddim_step_rng(None, None, None, None, 1, 4, None, 0, 0.6, 0.8, 0.3, 0.69, 0.25, 1.0, 1, None) == _lib.SISIC_EINVAL
    assert lib.sisic_sample_frames_rule(None, None, 1, 32, 32, 4, None, None, 1.0, _lib.RULE_DDIM, 0, None, None, None, None,
                                        None, None, None) == _lib.SISIC_EINVAL
    assert lib.sisic_sample_frames_rule_rng(None, None, 1, 32, 32, 4, None, None, 1.0, _lib.RULE_DDIM, 0, None, 0, None, None,
                                            None, None, None, None) == _lib.SISIC_EINVAL
    assert b"seeds" in lib.sisic_last_error()


def test_refusals_come_before_the_gpu_is_touched():
    """no model is loaded and this machine may have no GPU: the error has to come first"""
    from synt_isic_amd import sampler as S
    from synt_isic_amd.scheduler import HipDDIMScheduler
    s = S.Sampler("cuda")
    for call in (lambda **kw: s.generate_seeds("NV", [0], T=4, size=(32, 32), **kw),
                 lambda **kw: s.generate_images("NV", [0], 4, size=(32, 32), **kw),
                 lambda **kw: s.generate(0, "NV", 4, size=(32, 32), **kw)):
        with pytest.raises(ValueError, match="scheduler must be one of"):
            call(scheduler="heun")
        with pytest.raises(ValueError, match="scheduler='ddim'"):
            call(scheduler="ddpm", eta=0.5)
        with pytest.raises(ValueError, match="scheduler='ddim'"):
            call(eta=1.0)                                       # "ddpm" is the default
        with pytest.raises(KeyError):                           # a known rule goes on to the model lookup
            call(scheduler="ddim", eta=0.5)
    with pytest.raises(ValueError, match="scheduler must be one of"):
        s.create_scheduler(10, "heun")
    assert s.create_scheduler(10, "ddim").rule == "ddim" and s.create_scheduler(10).rule == "ddpm"
    assert isinstance(s.create_scheduler(10, "ddim"), HipDDIMScheduler)
    for kw in (dict(thresholding=True), dict(rescale_betas_zero_snr=True), dict(prediction_type="v_prediction"),
               dict(timestep_spacing="linspace"), dict(beta_schedule="scaled_linear"), dict(dynamic_thresholding_ratio=0.9)):
        with pytest.raises(NotImplementedError):
            HipDDIMScheduler(**kw)
    sched = HipDDIMScheduler()
    sched.set_timesteps(10)
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sched.step(x, 900, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sched.add_noise(x, x, torch.tensor([5]))
