"""DPM-Solver++(2M) without a GPU: the timestep grids, the coefficient table against the DDIM restatement at solver_order = 1
and against the unfolded published update, the order of convergence on a toy problem with a known solution, the SDE variant's
moments on the same toy, the ABI, and the refusals that have to come before the GPU is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ddim_ref
import dpmpp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sisic_dpmpp_step", "sisic_dpmpp_step_rng")
SCHEDULES = ("squaredcos_cap_v2", "linear")


def _mirror(T, **kw):
    from synt_isic_amd.scheduler import HipDPMSolverMultistepScheduler
    kw.setdefault("beta_schedule", "squaredcos_cap_v2")
    s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, **kw)
    s.set_timesteps(T)
    return s


# ---- 1. grids ----------------------------------------------------------------------------------------------------------
GRIDS = {
    ("linspace", 7): [999, 856, 714, 571, 428, 285, 143],
    ("leading", 7): [852, 710, 568, 426, 284, 142, 0],
    ("trailing", 7): [999, 856, 713, 570, 428, 285, 142],               # the grid tests/test_gpu_ddim.py pins
    ("linspace", 20): [999, 949, 899, 849, 799, 749, 699, 649, 599, 549, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50],
    ("leading", 20): list(range(950, -1, -50)),
    ("trailing", 20): list(range(999, 0, -50)),
}


@pytest.mark.parametrize("spacing,T", sorted(GRIDS))
def test_timestep_grids_are_exact_integers(spacing, T):
    s = _mirror(T, timestep_spacing=spacing)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == GRIDS[(spacing, T)]
    assert dpmpp_ref.timestep_grid(T, spacing).tolist() == GRIDS[(spacing, T)]
    if spacing != "linspace":                                    # the two grids the DDIM mirror has are the same grids here
        d = ddim_ref.DDIMSchedulerRef(timestep_spacing=spacing)
        d.set_timesteps(T)
        assert d.timesteps.tolist() == GRIDS[(spacing, T)]


def test_mirror_table_is_the_restatements():
    for schedule in SCHEDULES:
        for spacing in ("linspace", "leading", "trailing"):
            for order in (1, 2):
                for alg in dpmpp_ref.ALGORITHMS:
                    s = _mirror(20, beta_schedule=schedule, timestep_spacing=spacing, solver_order=order, algorithm_type=alg)
                    r = dpmpp_ref.DPMSolverRef(schedule, order, alg, spacing)
                    r.set_timesteps(20)
                    tab = s.coefficient_table()
                    assert tab.dtype == torch.float32 and tuple(tab.shape) == (20, 6) and torch.equal(tab, r.table())
                    assert torch.isfinite(tab).all()
                    # first and last steps are first order; the run ends at sigma = 0 and returns its x0
                    assert float(tab[0, 5]) == 0.0 and float(tab[-1, 5]) == 0.0
                    assert tuple(float(v) for v in tab[-1, 2:]) == (0.0, 1.0, 0.0, 0.0)
                    assert bool((tab[1:-1, 5] != 0).all()) == (order == 2)
                    assert int((tab[:, 4] != 0).sum()) == (19 if alg == "sde-dpmsolver++" else 0)
    assert s.rule == "dpmsolver++"


# ---- 2. order 1 is DDIM ------------------------------------------------------------------------------------------------
# Both sides in float64 from the same fp32 alphas_cumprod.  Measured worst differences over T = 10, 20, 50 and both beta
# schedules: ODE against eta = 0: 3.9e-16 (cx exact, k0 3.9e-16); SDE against eta = 1: cx 6.6e-15, k0 6.7e-15, sigma 1.3e-15.
# The bounds are 100 x the measured worst: the two sides are different float64 expressions of one quantity, with cancellation
# at small t (1 - abar_prev - sigma^2 on the DDIM side).
IDENTITY_BOUND = {"dpmsolver++": 4e-14, "sde-dpmsolver++": 7e-13}


def _ddim_rows64(schedule, T, eta):
    """float64 (cx, k0, sigma) the DDIM rule implies: prev = c_prev*x0 + c_dir*eps with eps = (x - sa*x0)/sb"""
    d = ddim_ref.DDIMSchedulerRef(beta_schedule=schedule)
    d.set_timesteps(T)
    acp = d.alphas_cumprod.numpy().astype(np.float64)
    rows = []
    for t in d.timesteps.tolist():
        prev_t = d.previous_timestep(t)
        at, ap = acp[t], (acp[prev_t] if prev_t >= 0 else 1.0)
        variance = ((1 - ap) / (1 - at)) * (1 - at / ap)
        sigma = eta * variance ** 0.5
        c_prev, c_dir, sb, sa = ap ** 0.5, (1 - ap - sigma ** 2) ** 0.5, (1 - at) ** 0.5, at ** 0.5
        rows.append((c_dir / sb, c_prev - c_dir * sa / sb, sigma))
    return d.timesteps, acp, np.array(rows)


@pytest.mark.parametrize("alg,eta", [("dpmsolver++", 0.0), ("sde-dpmsolver++", 1.0)])
def test_order_1_table_is_the_ddim_table(alg, eta):
    worst = np.zeros(3)
    for schedule in SCHEDULES:
        for T in (10, 20, 50):
            ts, acp, want = _ddim_rows64(schedule, T, eta)
            assert ts.tolist() == dpmpp_ref.timestep_grid(T, "leading").tolist()
            got = dpmpp_ref.table64(acp[ts.numpy()], 1, alg)
            assert np.all(got[:, 5] == 0)
            worst = np.maximum(worst, np.abs(got[:, [2, 3, 4]] - want).max(axis=0))
    print(f"{alg} order 1 against DDIM eta = {eta}: worst |cx|, |k0|, |sigma| differences = {worst}")
    assert worst.max() <= IDENTITY_BOUND[alg]


# ---- 3. folded = unfolded ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", dpmpp_ref.ALGORITHMS)
def test_folded_coefficients_are_the_published_update(alg):
    rng = np.random.default_rng(5)
    worst = 0.0
    for schedule in SCHEDULES:
        for T, spacing in ((10, "linspace"), (20, "leading"), (50, "trailing")):
            abar = dpmpp_ref.alphas_cumprod(schedule).numpy().astype(np.float64)[dpmpp_ref.timestep_grid(T, spacing)]
            tab = dpmpp_ref.table64(abar, 2, alg)
            for i in range(T):
                x, m0, m1, z = rng.standard_normal((4, 64))
                want = dpmpp_ref.published_update64(x, m0, m1, z, abar, i, 2, alg)
                _, _, cx, k0, sigma, k1 = tab[i]
                got = cx * x + k0 * m0 + k1 * m1 + sigma * z
                worst = max(worst, float((np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max()))
    print(f"{alg}: worst relative |folded - unfolded| = {worst:.3e}")
    assert worst <= 1e-12


# ---- 4. convergence ----------------------------------------------------------------------------------------------------
# data N(mu, s^2): x_t ~ N(alpha_t mu, v_t), v_t = abar_t s^2 + 1 - abar_t, so eps(x, t) = sigma_t (x - alpha_t mu) / v_t and the
# probability-flow ODE keeps the standardised coordinate: x(abar = 1) = mu + s (x_T - alpha_T mu) / v_T^0.5
MU, S, X_T = 0.3, 0.5, 1.7


def _toy_eps(x, abar):
    return (1 - abar) ** 0.5 * (x - abar ** 0.5 * MU) / (abar * S * S + 1 - abar)


def _toy_run(T, order, alg="dpmsolver++", x=X_T, z=None):
    abar = dpmpp_ref.alphas_cumprod("squaredcos_cap_v2").numpy().astype(np.float64)[dpmpp_ref.timestep_grid(T, "leading")]
    tab = dpmpp_ref.table64(abar, order, alg)
    m1 = 0.0
    for i in range(T):
        sb, sa, cx, k0, sigma, k1 = tab[i]
        m0 = (x - sb * _toy_eps(x, abar[i])) / sa
        x = cx * x + k0 * m0 + k1 * m1
        if sigma != 0.0:
            x = x + sigma * z[i]
        m1 = m0
    return x, abar


def test_convergence_order_on_the_toy_problem():
    err = {}
    for order in (1, 2):
        for T in (50, 100, 200):
            x, abar = _toy_run(T, order)
            exact = MU + S * (X_T - abar[0] ** 0.5 * MU) / (abar[0] * S * S + 1 - abar[0]) ** 0.5
            err[(order, T)] = abs(x - exact)
    rates = {o: [float(np.log2(err[(o, a)] / err[(o, b)])) for a, b in ((50, 100), (100, 200))] for o in (1, 2)}
    print("errors:", {k: f"{v:.3e}" for k, v in err.items()}, "observed orders:", rates)
    assert all(0.9 <= r <= 1.1 for r in rates[1])
    assert all(r >= 1.8 for r in rates[2])
    assert err[(2, 200)] < 0.25 * err[(1, 200)]


# ---- 5. the SDE variant ------------------------------------------------------------------------------------------------
def test_sde_moments_on_the_toy_problem():
    N, T = 200_000, 50
    rng = np.random.default_rng(1234)
    abar0 = dpmpp_ref.alphas_cumprod("squaredcos_cap_v2").numpy().astype(np.float64)[dpmpp_ref.timestep_grid(T, "leading")][0]
    x_T = abar0 ** 0.5 * MU + (abar0 * S * S + 1 - abar0) ** 0.5 * rng.standard_normal(N)      # the marginal at t_0
    z = rng.standard_normal((T, N))
    off = {}
    for order in (1, 2):
        x, _ = _toy_run(T, order, "sde-dpmsolver++", x_T.copy(), z)
        off[order] = (abs(x.mean() - MU), abs(x.std() - S))
    print("SDE |mean - mu|, |std - s| by order:", off)
    slack = 3 * S / N ** 0.5
    assert off[2][0] <= off[1][0] + slack and off[2][1] <= off[1][1] + slack


# ---- 6. ABI and refusals -----------------------------------------------------------------------------------------------
def test_header_declares_and_binding_table_binds_the_new_entries():
    from synt_isic_amd import _lib
    text = open(os.path.join(ROOT, "include", "sisic.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sisic_[a-z0-9_]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/sisic.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert "#define SISIC_ABI_VERSION 3" in text and _lib.ABI_VERSION == 3                      # additive only
    assert re.search(r"#define SISIC_RULE_DPMPP 2\b", text) and _lib.RULE_DPMPP == 2
    assert re.search(r"#define SISIC_RULE_DDPM 0\b", text) and re.search(r"#define SISIC_RULE_DDIM 1\b", text)
    assert "SISIC_RULE_ROW_WIDTH(rule)" in text
    assert _lib.RULE_ROW_WIDTH == {_lib.RULE_DDPM: 5, _lib.RULE_DDIM: 5, _lib.RULE_DPMPP: 6}
    sig = _lib.SIGNATURES
    # the twins of the DDPM entries: the history in front of out, k1 behind sigma
    f = C.c_float
    assert sig["sisic_dpmpp_step"][1] == [C.c_void_p] * 6 + [C.c_int64] + [f] * 7 + [C.c_void_p]
    assert sig["sisic_dpmpp_step_rng"][1] == [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_void_p, C.c_uint32] + [f] * 7 + [C.c_void_p]
    assert len(sig["sisic_dpmpp_step"][1]) == len(sig["sisic_ddpm_step"][1]) + 2
    assert len(sig["sisic_dpmpp_step_rng"][1]) == len(sig["sisic_ddpm_step_rng"][1]) + 2


def test_library_exports_the_new_entries():
    from synt_isic_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name)
    # argument validation needs no GPU
    assert lib.sisic_dpmpp_step(None, None, None, None, None, None, 4, 0.6, 0.8, 0.9, 0.3, 0.25, -0.1, 1.0, None) == _lib.SISIC_EINVAL
    assert b"dpmpp_step" in lib.sisic_last_error()
    assert lib.sisic_dpmpp_step_rng(None, None, None, None, None, 1, 4, None, 0, 0.6, 0.8, 0.9, 0.3, 0.25, -0.1, 1.0,
                                    None) == _lib.SISIC_EINVAL
    assert b"dpmpp_step_rng" in lib.sisic_last_error()
    assert lib.sisic_sample_frames_rule(None, None, 1, 32, 32, 4, None, None, 1.0, _lib.RULE_DPMPP, 0, None, None, None, None,
                                        None, None, None) == _lib.SISIC_EINVAL
    assert lib.sisic_sample_frames_rule_rng(None, None, 1, 32, 32, 4, None, None, 1.0, _lib.RULE_DPMPP, 0, None, 0, None, None,
                                            None, None, None, None) == _lib.SISIC_EINVAL
    assert b"seeds" in lib.sisic_last_error()


def test_refusals_come_before_the_gpu_is_touched():
    """no model is loaded and this machine may have no GPU: the error has to come first"""
    from synt_isic_amd import sampler as S
    from synt_isic_amd.scheduler import HipDPMSolverMultistepScheduler
    assert "dpmsolver++" in S.SCHEDULERS and S.SCHEDULERS[0] == "ddpm"
    s = S.Sampler("cuda")
    for call in (lambda **kw: s.generate_seeds("NV", [0], T=4, size=(32, 32), **kw),
                 lambda **kw: s.generate_images("NV", [0], 4, size=(32, 32), **kw),
                 lambda **kw: s.generate(0, "NV", 4, size=(32, 32), **kw)):
        with pytest.raises(ValueError, match="algorithm_type"):
            call(scheduler="dpmsolver++", algorithm_type="dpmsolver")
        with pytest.raises(ValueError, match="solver_order"):
            call(scheduler="dpmsolver++", solver_order=3)
        with pytest.raises(ValueError, match="scheduler='ddim'"):
            call(scheduler="dpmsolver++", eta=0.5)
        with pytest.raises(ValueError, match="scheduler='ddim'"):
            call(scheduler="dpmsolver++", use_clipped_model_output=True)
        with pytest.raises(ValueError, match="scheduler='dpmsolver\\+\\+'"):
            call(scheduler="ddim", solver_order=1)
        with pytest.raises(ValueError, match="scheduler='dpmsolver\\+\\+'"):
            call(algorithm_type="sde-dpmsolver++")                # "ddpm" is the default
        for kw in (dict(), dict(solver_order=1), dict(algorithm_type="sde-dpmsolver++")):
            with pytest.raises(KeyError):                         # a known rule goes on to the model lookup
                call(scheduler="dpmsolver++", **kw)
    sched = s.create_scheduler(10, "dpmsolver++", 1, "sde-dpmsolver++")
    assert isinstance(sched, HipDPMSolverMultistepScheduler) and sched.rule == "dpmsolver++"
    assert sched.config.solver_order == 1 and sched.config.algorithm_type == "sde-dpmsolver++" and sched.config.clip_sample
    assert sched.timesteps.tolist() == s.create_scheduler(10).timesteps.tolist()         # one grid for the three rules
    assert s.create_scheduler(10).rule == "ddpm" and s.create_scheduler(10, "ddim").rule == "ddim"
    for kw in (dict(solver_order=3), dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver"),
               dict(solver_type="heun"), dict(final_sigmas_type="sigma_min"), dict(prediction_type="v_prediction"),
               dict(thresholding=True), dict(use_karras_sigmas=True), dict(timestep_spacing="karras"),
               dict(beta_schedule="scaled_linear")):
        with pytest.raises(NotImplementedError):
            HipDPMSolverMultistepScheduler(**kw)
    plain = HipDPMSolverMultistepScheduler(lower_order_final=False)          # accepted, no effect
    other = HipDPMSolverMultistepScheduler()
    plain.set_timesteps(10)
    other.set_timesteps(10)
    assert torch.equal(plain.coefficient_table(), other.coefficient_table())
    assert not other.config.clip_sample and other.config.solver_order == 2 and other.config.timestep_spacing == "linspace"
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        plain.step(x, 999, x)
    from synt_isic_amd.sampler import NoiseStream, run_sampling_loop
    ns = NoiseStream.__new__(NoiseStream)                         # a run under this rule is never cut into segments
    with pytest.raises(ValueError, match="not cut into segments"):
        run_sampling_loop(None, plain, x, ns)
