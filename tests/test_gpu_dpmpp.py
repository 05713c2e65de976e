"""The DPM-Solver++(2M) sampler on the GPU: the fused step and its history bit for bit against the restatement
(tests/dpmpp_ref.py), generated noise against buffer noise, the stateful mirror, the in-library loop against the Python loop
over the two drop-in objects, the captured step's key, run-to-run independence of the history, the chain against the CPU
oracle, and the public interface."""
import numpy as np
import pytest
import torch

import dpmpp_ref
from test_gpu_device_noise import eager, graph  # noqa: F401  (the two graph-mode fixtures, shared)

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
B, T = 3, 12
FIXED_ROW = (0.6, 0.8, 0.9, 0.3, 0.25, -0.1)               # {sb, sa, cx, k0, sigma, k1}: second order, noisy
ALGS = dpmpp_ref.ALGORITHMS


def _dpm(T, **kw):
    from synt_isic_amd.scheduler import HipDPMSolverMultistepScheduler
    kw.setdefault("beta_schedule", "squaredcos_cap_v2")
    kw.setdefault("clip_sample", True)
    s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, **kw)
    s.set_timesteps(T)
    return s


def _x_T(seeds, chw=CHW):
    return torch.stack([torch.randn(chw, generator=torch.Generator().manual_seed(2000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _z_rows(n_rows, batch=B, chw=CHW, seed=77):
    return torch.randn((n_rows, batch) + tuple(chw), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _n_noise(sched):
    return int((sched.coefficient_table()[:, 4] != 0).sum())


def _python_loop(model, sched, x_T, z):
    """image_generator.py:395-403 over the drop-in objects; z rows go to the steps with sigma != 0.  Returns every frame."""
    sched.set_timesteps(sched.num_inference_steps)              # a new run: no history
    tab = sched.coefficient_table()
    x, zi, frames = x_T.clone(), 0, []
    for i, t in enumerate(sched.timesteps):
        eps = model(x, t).sample
        vn = None
        if z is not None and float(tab[i, 4]) != 0.0:
            vn = z[zi]
            zi += 1
        x = sched.step(eps, t, x, variance_noise=vn).prev_sample
        frames.append(x)
    assert z is None or zi == z.shape[0]
    return torch.stack(frames)


def _same(a, b):
    assert torch.equal(a.latents, b.latents) and torch.equal(a.images, b.images)
    if a.trajectory is not None or b.trajectory is not None:
        assert a.trajectory_steps == b.trajectory_steps and torch.equal(a.trajectory, b.trajectory)


def _filled_buffer(sched, seeds, chw, step0=0):
    """[n_noise,B,C,H,W]: the row of step i (sigma != 0) = sisic_noise_fill(step = step0 + i)"""
    from synt_isic_amd import ops
    coef = sched.coefficient_table()
    rows = [ops.noise_fill(seeds, int(np.prod(chw)), step0 + i).reshape((len(seeds),) + tuple(chw))
            for i in range(coef.shape[0]) if float(coef[i, 4]) != 0.0]
    return torch.stack(rows) if rows else torch.empty((0, len(seeds)) + tuple(chw), device=DEV)


# ---- 1. one step -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_inputs():
    g = torch.Generator().manual_seed(20)
    n = B * int(np.prod(CHW))
    return tuple(torch.randn(n, generator=g) for _ in range(4))          # e, x, z, hist on the host


@pytest.fixture(scope="module")
def table_rows():
    """first, interior (second-order) and last rows of the cosine table at T = 20; the rows of t = 999, 500 and 0 of the
    linear-beta table over all 1000 steps; both variants; and the fixed row"""
    rows = []
    for alg in ALGS:
        cos = dpmpp_ref.DPMSolverRef("squaredcos_cap_v2", 2, alg, "linspace")
        cos.set_timesteps(20)
        tab = cos.table()
        rows += [tuple(float(v) for v in tab[i]) for i in (0, 10, 19)]
        lin = dpmpp_ref.DPMSolverRef("linear", 2, alg, "leading")
        lin.set_timesteps(1000)
        assert lin.timesteps[0] == 999 and lin.timesteps[499] == 500 and lin.timesteps[-1] == 0
        tab = lin.table()
        rows += [tuple(float(v) for v in tab[i]) for i in (0, 499, 999)]
    assert len(rows) == 12
    assert [r[5] != 0.0 for r in rows] == [False, True, False] * 4
    assert [r[4] != 0.0 for r in rows] == [False] * 6 + [True, True, False] * 2
    return rows + [FIXED_ROW]


@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_one_step_is_the_restatement_bit_for_bit(step_inputs, table_rows, clip):
    from synt_isic_amd import ops
    e, x, z, h = step_inputs
    ed, xd, zd, hd = (t.to(DEV) for t in step_inputs)
    for row in table_rows:
        for noise in (z, None):
            want, want_hist = dpmpp_ref.step_row(e, x, noise, h, row, clip)
            hist = hd.clone()
            got = ops.dpmpp_step(ed, xd, zd if noise is not None else None, hist, row, clip)
            assert torch.isfinite(want).all()
            assert torch.equal(got.cpu(), want), (row, float((got.cpu() - want).abs().max()))
            assert torch.equal(hist.cpu(), want_hist), row                       # the history is this step's x0
        if row[5] == 0.0:
            # a first-order step does not read the history: whatever lies there stays out of the result
            hist = torch.full_like(hd, float("nan"))
            got = ops.dpmpp_step(ed, xd, zd, hist, row, clip)
            assert torch.isfinite(got).all() and torch.equal(got.cpu(), want_first(e, x, z, row, clip))
            assert torch.equal(hist.cpu(), dpmpp_ref.predicted_x0(e, x, row, clip))
    # the fixed row clamps about half of its x0: both sides of the clamp are exercised
    share = float((dpmpp_ref.predicted_x0(e, x, FIXED_ROW, 0.0).abs() > 1.0).float().mean())
    print(f"clipped share of x0 under the fixed row: {share:.3f}")
    assert 0.05 <= share <= 0.95
    # the history reaches the result, and the clamp reaches the history
    assert not torch.equal(ops.dpmpp_step(ed, xd, zd, hd.clone(), FIXED_ROW, clip), ops.dpmpp_step(ed, xd, zd, (hd + 1).clone(), FIXED_ROW, clip))
    # in place
    inplace, hist = xd.clone(), hd.clone()
    ops.dpmpp_step(ed, inplace, zd, hist, FIXED_ROW, clip, out=inplace)
    want, want_hist = dpmpp_ref.step_row(e, x, z, h, FIXED_ROW, clip)
    assert torch.equal(inplace.cpu(), want) and torch.equal(hist.cpu(), want_hist)


def want_first(e, x, z, row, clip):
    return dpmpp_ref.step_row(e, x, z, None, row, clip)[0]


@pytest.mark.parametrize("n,offset", [(105, 0), (105, 1), (3 * 3 * 32 * 32, 1)])
def test_scalar_tail_and_unaligned_tensors(n, offset):
    """105 elements on a line: 26 float4 and a tail of one; a base pointer one float off a line: the element-by-element path"""
    from synt_isic_amd import ops
    g = torch.Generator().manual_seed(n + offset)
    host = [torch.randn(n, generator=g) for _ in range(4)]
    view = lambda t: torch.cat([torch.zeros(offset), t, torch.zeros(4)]).to(DEV)[offset:offset + n]
    for row in (FIXED_ROW, FIXED_ROW[:5] + (0.0,)):
        e, x, z, h = (view(t) for t in host)
        assert e.data_ptr() % 16 == 4 * offset and h.data_ptr() % 16 == 4 * offset
        out = view(torch.zeros(n))
        ops.dpmpp_step(e, x, z, h, row, 1.0, out=out)
        want, want_hist = dpmpp_ref.step_row(host[0], host[1], host[2], host[3], row, 1.0)
        assert torch.equal(out.cpu(), want) and torch.equal(h.cpu(), want_hist)
        h2 = view(host[3])
        ops.dpmpp_step(e, x, z, h2, row, 1.0, out=x)                             # in place
        assert torch.equal(x.cpu(), want) and torch.equal(h2.cpu(), want_hist)


@pytest.mark.parametrize("n_per_image,offset", [(3 * 32 * 32, 0), (3 * 32 * 32, 1), (105, 0), (105, 1)])
def test_step_rng_equals_step_fed_by_noise_fill(n_per_image, offset):
    """float4 lines, tensors four bytes off a line, and images of 105 floats whose blocks straddle two images"""
    from synt_isic_amd import ops
    seeds, step = [4, (1 << 35) + 6, 0x7FFFFFFF], 17
    n = len(seeds) * n_per_image
    g = torch.Generator().manual_seed(n + offset)
    view = lambda t: torch.cat([torch.zeros(offset), t, torch.zeros(4)]).to(DEV)[offset:offset + n]
    eps, x, h0 = (torch.randn(n, generator=g) for _ in range(3))
    eps, x = view(eps), view(x)
    assert eps.data_ptr() % 16 == 4 * offset
    z = ops.noise_fill(seeds, n_per_image, step).reshape(-1)
    quiet = FIXED_ROW[:4] + (0.0, FIXED_ROW[5])
    first = FIXED_ROW[:5] + (0.0,)
    for row in (FIXED_ROW, first):
        ha, hb = view(h0), view(h0)
        want = ops.dpmpp_step(eps, x, z, ha, row, 1.0)
        got = ops.dpmpp_step_rng(eps, x, seeds, step, hb, row, 1.0)
        assert torch.isfinite(got).all() and torch.equal(got, want) and torch.equal(ha, hb)
        assert not torch.equal(got, ops.dpmpp_step(eps, x, None, view(h0), row, 1.0))            # sigma != 0 adds noise
        inplace, hc = view(x.cpu()), view(h0)
        ops.dpmpp_step_rng(eps, inplace, seeds, step, hc, row, 1.0, out=inplace)
        assert torch.equal(inplace, want) and torch.equal(hc, ha)
    # sigma == 0 draws nothing
    assert torch.equal(ops.dpmpp_step_rng(eps, x, seeds, step, view(h0), quiet, 1.0), ops.dpmpp_step(eps, x, None, view(h0), quiet, 1.0))
    # k1 == 0 does not read a NaN history
    nan = view(torch.full((n,), float("nan")))
    assert torch.equal(ops.dpmpp_step_rng(eps, x, seeds, step, nan, first, 1.0), ops.dpmpp_step(eps, x, z, view(h0), first, 1.0))
    assert torch.isfinite(nan).all()


# ---- 2. the stateful mirror --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_stateful_step_of_the_scheduler_mirror(alg):
    g = torch.Generator().manual_seed(31)
    shape = (B,) + CHW
    x_T = torch.randn(shape, generator=g)
    eps = [torch.randn(shape, generator=g) for _ in range(5)]
    z = torch.randn((4,) + shape, generator=g)
    s = _dpm(5, algorithm_type=alg)
    r = dpmpp_ref.DPMSolverRef("squaredcos_cap_v2", 2, alg, "linspace", clip_sample=True)
    r.set_timesteps(5)
    assert s.timesteps.tolist() == r.timesteps.tolist() and torch.equal(s.coefficient_table(), r.table())
    sde = alg == "sde-dpmsolver++"
    want = r.chain(lambda x, t, it=iter(eps): next(it), x_T, z if sde else None)

    def run():
        x, zi, out = x_T.to(DEV), 0, []
        for i, t in enumerate(s.timesteps):
            assert s.step_index in (None, i)
            vn = None
            if sde and i < 4:
                vn, zi = z[zi].to(DEV), zi + 1
            x = s.step(eps[i].to(DEV), t, x, variance_noise=vn).prev_sample
            out.append(x.cpu())
        return out

    first = run()
    for a, b in zip(first, want):
        assert torch.equal(a, b)
    assert bool((s.coefficient_table()[1:4, 5] != 0).all())     # the three interior steps used the history
    with pytest.raises(RuntimeError, match="past the last timestep"):
        s.step(eps[0].to(DEV), 0, x_T.to(DEV))
    s.set_timesteps(5)                                          # resets the history and the step index
    assert s.step_index is None
    for a, b in zip(run(), want):
        assert torch.equal(a, b)
    s.set_timesteps(5)
    assert s.step(eps[0].to(DEV), int(s.timesteps[0]), x_T.to(DEV), return_dict=False)[0].shape == shape


# ---- 3. the loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_fused_loop_equals_python_loop(mode, alg, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    s = eager if mode == "eager" else graph
    model = s.models["NV"]
    seeds = [11, (1 << 33) + 2, 0]
    x_T = _x_T(seeds)
    keep = [0, 5, T - 1]
    for order in (2, 1):
        sched = _dpm(T, algorithm_type=alg, solver_order=order, timestep_spacing="leading")
        n_noise = _n_noise(sched)
        assert n_noise == (T - 1 if alg == "sde-dpmsolver++" else 0)
        for z in ((_z_rows(n_noise), _filled_buffer(sched, seeds, CHW)) if n_noise else (None,)):
            frames = _python_loop(model, sched, x_T, z)
            res = run_sampling_loop(model, sched, x_T, z, return_trajectory=True)
            assert res.steps_done == T and res.scheduler == "dpmsolver++"
            assert torch.equal(res.latents, frames[-1]) and torch.equal(res.trajectory, frames)
            kept = run_sampling_loop(model, sched, x_T, z, return_trajectory=True, save_indices=keep)
            assert kept.trajectory_steps == keep and torch.equal(kept.trajectory, frames[keep]) and torch.equal(kept.latents, frames[-1])
        # generated noise = the buffer of noise_fill rows (z is that buffer here), every frame
        dn = run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), return_trajectory=True)
        assert torch.equal(dn.trajectory, frames) and torch.equal(dn.images, res.images)
        if order == 2:
            second = res
    assert not torch.equal(second.latents, res.latents)         # the history term is there: order 2 is not order 1
    if alg == "dpmsolver++":
        # ... and not DDIM's result on the same grid
        from synt_isic_amd.scheduler import HipDDIMScheduler
        ddim = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
        ddim.set_timesteps(T)
        assert ddim.timesteps.tolist() == sched.timesteps.tolist()
        assert not torch.equal(run_sampling_loop(model, ddim, x_T, None).latents, second.latents)


def test_a_call_starts_without_history(eager):
    """row 0 of a call must be first order: the library refuses a table cut in the middle, and a NoiseStream is not taken"""
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import run_sampling_loop
    whole = _dpm(T)

    class Cut(type(whole)):                      # the mirror of the whole run, from its second grid entry on
        def __init__(self):
            vars(self).update(vars(whole))
            self.timesteps = whole.timesteps[1:]

        def coefficient_table(self):
            return whole.coefficient_table()[1:]

    with pytest.raises(_lib.SisicError, match="k1 = .* no history"):
        run_sampling_loop(eager.models["NV"], Cut(), _x_T([1, 2, 3]), None)


# ---- 4. the ODE variant ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_ode_ignores_the_noise_source(mode, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    s = eager if mode == "eager" else graph
    model, seeds = s.models["NV"], [5, 6, 7]
    sched = _dpm(T)
    assert sched.config.clip_sample and sched.config.solver_order == 2 and sched.config.timestep_spacing == "linspace"
    x_T = _x_T(seeds)
    none = run_sampling_loop(model, sched, x_T, None, return_trajectory=True)
    _same(run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), return_trajectory=True), none)
    _same(run_sampling_loop(model, sched, x_T, torch.empty((0, B) + CHW, device=DEV), return_trajectory=True), none)
    with pytest.raises(ValueError, match="noise must be fp32"):
        run_sampling_loop(model, sched, x_T, _z_rows(T - 1))
    # the last step returns its clamped x0
    assert torch.isfinite(none.latents).all() and float(none.latents.abs().max()) <= 1.0
    eps = model(none.trajectory[-2], sched.timesteps[-1]).sample
    x0 = dpmpp_ref.predicted_x0(eps.cpu(), none.trajectory[-2].cpu(), sched.coefficient_table()[-1], 1.0)
    assert torch.equal(none.latents.cpu(), x0 * 1.0 + 0.0 * none.trajectory[-2].cpu())


# ---- 5. the captured step ----------------------------------------------------------------------------------------------
def test_graph_is_keyed_by_the_rule(graph):
    from synt_isic_amd import _lib
    lib = _lib.load()
    mg = graph.models["NV"]
    seeds, Tn = [31, 32], 8
    kw = dict(noise="device", scheduler="dpmsolver++", algorithm_type="sde-dpmsolver++")
    ddim = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device", scheduler="ddim", eta=0.7)
    first = graph.generate_seeds("NV", seeds, Tn, (32, 32), **kw)
    builds = lib.sisic_unet_graph_builds(mg.handle)
    assert builds >= 2
    second = graph.generate_seeds("NV", seeds, Tn, (32, 32), **kw)
    other = graph.generate_seeds("NV", [77, 78], Tn, (32, 32), **dict(kw, solver_order=1))
    assert lib.sisic_unet_graph_builds(mg.handle) == builds             # same rule, shape and noise source: replayed
    assert torch.equal(first.latents, second.latents) and not torch.equal(first.latents, other.latents)
    # a DDIM call never replays a DPM-Solver++ step, nor the other way round
    after = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device", scheduler="ddim", eta=0.7)
    assert lib.sisic_unet_graph_builds(mg.handle) == builds + 1
    assert torch.equal(after.latents, ddim.latents) and torch.equal(after.images, ddim.images)
    again = graph.generate_seeds("NV", seeds, Tn, (32, 32), **kw)
    assert lib.sisic_unet_graph_builds(mg.handle) == builds + 2
    assert torch.equal(again.latents, first.latents) and torch.equal(again.images, first.images)


# ---- 6. no history leaks from run to run -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_two_runs_on_one_handle_are_bit_equal(mode, eager, graph):
    from synt_isic_amd.sampler import run_sampling_loop
    s = eager if mode == "eager" else graph
    model, sched = s.models["NV"], _dpm(T)
    a = run_sampling_loop(model, sched, _x_T([1, 2, 3]), None, return_trajectory=True)
    b = run_sampling_loop(model, sched, _x_T([4, 5, 6]), None)                   # leaves another history behind
    c = run_sampling_loop(model, sched, _x_T([1, 2, 3]), None, return_trajectory=True)
    _same(a, c)
    assert not torch.equal(a.latents, b.latents)


# ---- 7. the chain against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_chain_against_the_oracle(alg, eager, synthetic_sd):
    """T = 8, two seeds: oracle.unet.unet_forward + dpmpp_ref on the CPU.  1e-3 max-abs is the project's tolerance for this
    comparison (tests/test_gpu_ddim.py::test_chain_against_the_oracle, tests/test_gpu_sampler.py), which those tests make on the
    "leading" grid (t_0 = 875 at T = 8); so does this one.  The tolerance does not carry over to a grid that starts at t = 999
    of the cosine schedule ("linspace", "trailing"): there alpha_t = 4.9e-5, and the first step multiplies any difference in eps
    by k0 * sigma_t / alpha_t = 3.9e3, so a difference of 3e-7 between two fp32 UNets is 1.3e-3 after one step
    (measured on that grid: 1.29e-3 after step 0, 5.9e-3 at the end).  The step and the loop on those grids are covered bit for
    bit by the tests above."""
    from oracle import unet as ounet
    from synt_isic_amd.sampler import draw_noise, run_sampling_loop
    model = eager.models["NV"]
    sched = _dpm(8, algorithm_type=alg, timestep_spacing="leading")
    r = dpmpp_ref.DPMSolverRef("squaredcos_cap_v2", 2, alg, "leading", clip_sample=True)
    r.set_timesteps(8)
    assert sched.timesteps.tolist() == r.timesteps.tolist() and int(r.timesteps[0]) == 875
    x_T, z = draw_noise([3, 4], 7, CHW)
    zz = z if alg == "sde-dpmsolver++" else None
    assert _n_noise(sched) == (7 if zz is not None else 0)
    res = run_sampling_loop(model, sched, x_T.to(DEV), zz.to(DEV) if zz is not None else None, return_trajectory=True)
    with torch.no_grad():
        frames = r.chain(lambda x, t: ounet.unet_forward(synthetic_sd, x, t), x_T, zz)
    diffs = [(res.trajectory[i].cpu() - f).abs().max().item() for i, f in enumerate(frames)]
    print(f"{alg}: max |x - oracle chain| per step = {[f'{d:.2e}' for d in diffs]}")
    assert max(diffs) <= 1e-3


# ---- 8. public interface -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["host", "device"])
def test_generate_seeds_under_dpmsolver(noise, eager):
    a, b, c = 3, 0x7FFFFFFF, 12345
    Tn = 10
    ddpm = eager.generate_seeds("NV", [a, b, c], Tn, (32, 32), noise=noise)
    results = {}
    for alg in ALGS:
        kw = dict(noise=noise, scheduler="dpmsolver++", algorithm_type=alg)
        res = eager.generate_seeds("NV", [a, b, c], Tn, (32, 32), return_trajectory=True, **kw)
        assert res.steps_done == Tn and not res.cancelled and res.scheduler == "dpmsolver++" and res.eta == 0.0
        assert res.seeds == ddpm.seeds and res.noise_hashes == ddpm.noise_hashes              # x_T does not depend on the rule
        assert res.timesteps == ddpm.timesteps == dpmpp_ref.timestep_grid(Tn, "leading").tolist()
        assert torch.isfinite(res.latents).all() and not torch.equal(res.latents, ddpm.latents)
        one = eager.generate_seeds("NV", [c], Tn, (32, 32), **kw)                             # an image depends on its seed alone
        assert torch.equal(one.latents[0], res.latents[2]) and torch.equal(one.images[0], res.images[2])
        assert one.noise_hashes == res.noise_hashes[2:]
        first = eager.generate_seeds("NV", [a, b, c], Tn, (32, 32), solver_order=1, **kw)
        assert not torch.equal(first.latents, res.latents)                                    # solver_order reaches the table
        imgs, traj = eager.generate(a, "NV", Tn, size=(32, 32), **kw)
        assert traj is None and np.array_equal(imgs[0], res.images[0].cpu().numpy())
        results[alg] = res
    assert not torch.equal(results[ALGS[0]].latents, results[ALGS[1]].latents)                # algorithm_type reaches it too
    # a stop request ends a run under this rule like any other
    eager.request_stop()
    stopped = eager.generate_seeds("NV", [a, b, c], Tn, (32, 32), noise=noise, scheduler="dpmsolver++")
    assert stopped.cancelled and stopped.steps_done < Tn
    assert eager.generate_images("NV", [a, b, c], Tn, size=(32, 32), noise=noise, scheduler="dpmsolver++").steps_done == Tn


def test_host_mode_rows_are_draw_noises(eager):
    """host mode: x_T, then one z per step with sigma != 0 from the image's CPU generator, in ONE library call; the ODE variant
    draws nothing but x_T; neither makes a staging buffer"""
    from synt_isic_amd.sampler import Sampler, draw_noise, run_sampling_loop
    seeds, Tn = [21, 22], 10
    fresh = Sampler(DEV)
    fresh.models["NV"] = eager.models["NV"]
    for alg in ALGS:
        sched = fresh.create_scheduler(Tn, "dpmsolver++", 2, alg)
        n = _n_noise(sched)
        assert n == (Tn - 1 if alg == "sde-dpmsolver++" else 0)
        x_T, z = draw_noise(seeds, n, CHW)
        want = run_sampling_loop(eager.models["NV"], sched, x_T.to(DEV), z.to(DEV) if n else None)
        got = fresh.generate_seeds("NV", seeds, Tn, (32, 32), scheduler="dpmsolver++", algorithm_type=alg)
        assert torch.equal(got.latents, want.latents) and torch.equal(got.images, want.images)
    assert fresh._noise_buffers == {}


def test_module_level_generate_passes_the_rule_through(synthetic_sd):
    from synt_isic_amd import sampler as S
    old = S._default_sampler
    try:
        S._default_sampler = S.Sampler(DEV)
        S._default_sampler.add_model("NV", synthetic_sd)
        kw = dict(scheduler="dpmsolver++", solver_order=1, algorithm_type="sde-dpmsolver++")
        a, _ = S.generate(6, "NV", 4, size=(32, 32), **kw)
        b = S._default_sampler.generate_seeds("NV", [6], 4, (32, 32), **kw)
        c = S._default_sampler.generate_seeds("NV", [6], 4, (32, 32), scheduler="dpmsolver++")
        assert np.array_equal(a, b.images.cpu().numpy()) and not torch.equal(b.latents, c.latents)
        with pytest.raises(ValueError):
            S.generate(6, "NV", 4, size=(32, 32), scheduler="dpmsolver++", solver_order=3)
    finally:
        S._default_sampler = old
