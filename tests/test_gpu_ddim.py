"""The DDIM sampler on the GPU: the fused step bit for bit against the restatement (tests/ddim_ref.py), generated noise
against buffer noise, the in-library loop against the Python loop over the two drop-in objects, the noise-row rule (rows go to
the steps with sigma != 0, whatever their t), the chain against the CPU oracle, and the public interface."""
import numpy as np
import pytest
import torch

import ddim_ref
from test_gpu_device_noise import eager, graph  # noqa: F401  (the two graph-mode fixtures, shared)

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
B, T = 3, 12
FIXED_ROW = (0.6, 0.8, 0.3, 0.69, 0.25)


def _ddim(T, **kw):
    from synt_isic_amd.scheduler import HipDDIMScheduler
    kw.setdefault("beta_schedule", "squaredcos_cap_v2")
    s = HipDDIMScheduler(num_train_timesteps=1000, **kw)
    s.set_timesteps(T)
    return s


def _x_T(seeds, chw=CHW):
    return torch.stack([torch.randn(chw, generator=torch.Generator().manual_seed(2000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _z_rows(n_rows, batch=B, chw=CHW, seed=77):
    return torch.randn((n_rows, batch) + tuple(chw), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _n_noise(sched, eta):
    return int((sched.coefficient_table(eta)[:, 4] != 0).sum())


def _python_loop(model, sched, x_T, z, eta, clipped=False):
    """image_generator.py:395-403 over the drop-in objects; z rows go to the steps with sigma != 0.  Returns every frame."""
    x, zi, frames = x_T.clone(), 0, []
    for t in sched.timesteps:
        eps = model(x, t).sample
        vn = None
        if z is not None and sched.step_coefficients(t, eta)[4] != 0.0:
            vn = z[zi]
            zi += 1
        x = sched.step(eps, t, x, eta=eta, use_clipped_model_output=clipped, variance_noise=vn).prev_sample
        frames.append(x)
    assert z is None or zi == z.shape[0]
    return torch.stack(frames)


def _same(a, b):
    assert torch.equal(a.latents, b.latents) and torch.equal(a.images, b.images)
    if a.trajectory is not None or b.trajectory is not None:
        assert a.trajectory_steps == b.trajectory_steps and torch.equal(a.trajectory, b.trajectory)


def _filled_buffer(sched, eta, seeds, chw, step0=0):
    """[n_noise,B,C,H,W]: the row of step i (sigma != 0) = sisic_noise_fill(step = step0 + i)"""
    from synt_isic_amd import ops
    coef = sched.coefficient_table(eta)
    rows = [ops.noise_fill(seeds, int(np.prod(chw)), step0 + i).reshape((len(seeds),) + tuple(chw))
            for i in range(coef.shape[0]) if float(coef[i, 4]) != 0.0]
    return torch.stack(rows) if rows else torch.empty((0, len(seeds)) + tuple(chw), device=DEV)


# ---- 1. one step -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_inputs():
    g = torch.Generator().manual_seed(20)
    n = B * int(np.prod(CHW))
    return tuple(torch.randn(n, generator=g) for _ in range(3))          # e, x, z on the host


def _table_rows():
    rows = []
    cos = ddim_ref.DDIMSchedulerRef(beta_schedule="squaredcos_cap_v2")
    cos.set_timesteps(50)
    lin = ddim_ref.DDIMSchedulerRef(beta_schedule="linear")
    lin.set_timesteps(1000)
    for eta in (0.0, 0.5, 1.0):
        rows += [cos.coefficients(cos.timesteps[i], eta) for i in (0, 25, 49)]
        rows += [lin.coefficients(t, eta) for t in (999, 500, 1, 0)]
    return rows + [FIXED_ROW]


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_one_step_is_the_restatement_bit_for_bit(step_inputs, clip, clipped):
    from synt_isic_amd import ops
    e, x, z = step_inputs
    ed, xd, zd = (t.to(DEV) for t in step_inputs)
    rows = _table_rows()
    assert len(rows) == 22
    for row in rows:
        want = ddim_ref.step_row(e, x, z, row, clip, clipped)
        got = ops.ddim_step(ed, xd, zd, row, clip, clipped)
        assert torch.isfinite(want).all()
        assert torch.equal(got.cpu(), want), (row, float((got.cpu() - want).abs().max()))
        # without a noise buffer the step adds none
        assert torch.equal(ops.ddim_step(ed, xd, None, row, clip, clipped).cpu(), ddim_ref.step_row(e, x, None, row, clip, clipped))
    # the fixed row clamps about half of its x0: both sides of the clamp are exercised
    share = float((ddim_ref.predicted_x0(e, x, FIXED_ROW, 0.0).abs() > 1.0).float().mean())
    print(f"clipped share of x0 under the fixed row: {share:.3f}")
    assert 0.05 <= share <= 0.95
    # in place
    inplace = xd.clone()
    ops.ddim_step(ed, inplace, zd, FIXED_ROW, clip, clipped, out=inplace)
    assert torch.equal(inplace.cpu(), ddim_ref.step_row(e, x, z, FIXED_ROW, clip, clipped))


def test_step_of_the_scheduler_mirror(step_inputs):
    """HipDDIMScheduler.step = the restatement's step, from the timestep"""
    e, x, z = (t.reshape((B,) + CHW) for t in step_inputs)
    s = _ddim(50)
    r = ddim_ref.DDIMSchedulerRef(beta_schedule="squaredcos_cap_v2")
    r.set_timesteps(50)
    for t, eta, clipped in ((980, 0.0, False), (500, 0.5, True), (0, 1.0, False)):
        got = s.step(e.to(DEV), t, x.to(DEV), eta=eta, use_clipped_model_output=clipped, variance_noise=z.to(DEV))
        assert torch.equal(got.prev_sample.cpu(), r.step(e, t, x, eta=eta, use_clipped_model_output=clipped, noise=z))
    assert s.step(e.to(DEV), 500, x.to(DEV), return_dict=False)[0].shape == x.shape


# ---- 2. generated noise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_per_image,offset", [(3 * 32 * 32, 0), (3 * 32 * 32, 1), (105, 0), (105, 1)])
def test_step_rng_equals_step_fed_by_noise_fill(n_per_image, offset):
    """float4 lines, tensors four bytes off a line, and images of 105 floats whose blocks straddle two images"""
    from synt_isic_amd import ops
    seeds, step = [4, (1 << 35) + 6, 0x7FFFFFFF], 17
    n = len(seeds) * n_per_image
    g = torch.Generator().manual_seed(n + offset)
    view = lambda t: torch.cat([torch.zeros(offset), t, torch.zeros(4)]).to(DEV)[offset:offset + n]
    eps, x = view(torch.randn(n, generator=g)), view(torch.randn(n, generator=g))
    assert eps.data_ptr() % 16 == 4 * offset
    z = ops.noise_fill(seeds, n_per_image, step).reshape(-1)
    quiet = FIXED_ROW[:4] + (0.0,)
    for clipped in (False, True):
        want = ops.ddim_step(eps, x, z, FIXED_ROW, 1.0, clipped)
        got = ops.ddim_step_rng(eps, x, seeds, step, FIXED_ROW, 1.0, clipped)
        assert torch.isfinite(got).all() and torch.equal(got, want)
        assert not torch.equal(got, ops.ddim_step(eps, x, None, FIXED_ROW, 1.0, clipped))          # sigma != 0 adds noise
        # sigma == 0 draws nothing
        assert torch.equal(ops.ddim_step_rng(eps, x, seeds, step, quiet, 1.0, clipped), ops.ddim_step(eps, x, None, quiet, 1.0, clipped))
        inplace = x.clone() if offset == 0 else view(x.cpu())
        ops.ddim_step_rng(eps, inplace, seeds, step, FIXED_ROW, 1.0, clipped, out=inplace)
        assert torch.equal(inplace, want)
    assert not torch.equal(ops.ddim_step(eps, x, z, FIXED_ROW, 1.0, False), ops.ddim_step(eps, x, z, FIXED_ROW, 1.0, True))


# ---- 3. the loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_fused_loop_equals_python_loop(mode, eager, graph):
    from synt_isic_amd.sampler import run_sampling_loop
    s = eager if mode == "eager" else graph
    model = s.models["NV"]
    sched = _ddim(T)
    x_T = _x_T([1, 2, 3])
    keep = [0, 5, T - 1]
    for eta, clipped in ((0.0, False), (0.7, False), (0.7, True)):
        n_noise = _n_noise(sched, eta)
        assert n_noise == (0 if eta == 0.0 else T - 1)
        z = _z_rows(n_noise) if n_noise else None
        frames = _python_loop(model, sched, x_T, z, eta, clipped)
        res = run_sampling_loop(model, sched, x_T, z, return_trajectory=True, eta=eta, use_clipped_model_output=clipped)
        assert res.steps_done == T and res.scheduler == "ddim" and res.eta == eta
        assert torch.equal(res.latents, frames[-1]) and torch.equal(res.trajectory, frames)
        kept = run_sampling_loop(model, sched, x_T, z, return_trajectory=True, save_indices=keep, eta=eta,
                                 use_clipped_model_output=clipped)
        assert kept.trajectory_steps == keep and torch.equal(kept.trajectory, frames[keep]) and torch.equal(kept.latents, frames[-1])
    # the rule is not DDPM's
    ddpm = s.create_scheduler(T)
    assert not torch.equal(run_sampling_loop(model, ddpm, x_T, None).latents, run_sampling_loop(model, sched, x_T, None).latents)


# ---- 4. device noise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_device_noise_adds_exactly_the_filled_rows(mode, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    s = eager if mode == "eager" else graph
    model, seeds, eta = s.models["NV"], [11, (1 << 33) + 2, 0], 0.7
    sched = _ddim(T)
    x_T = _x_T(seeds)
    buf = _filled_buffer(sched, eta, seeds, CHW)
    assert buf.shape[0] == T - 1
    whole = run_sampling_loop(model, sched, x_T, buf, return_trajectory=True, eta=eta)
    _same(run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), return_trajectory=True, eta=eta), whole)
    assert not torch.equal(whole.latents, run_sampling_loop(model, sched, x_T, None, eta=eta).latents)      # noise was added
    buf7 = _filled_buffer(sched, eta, seeds, CHW, step0=7)
    _same(run_sampling_loop(model, sched, x_T, DeviceNoise(seeds, step0=7), eta=eta), run_sampling_loop(model, sched, x_T, buf7, eta=eta))
    assert not torch.equal(buf7[0], buf[0])
    # the run cut into two calls
    first, second = _ddim(T), _ddim(T)
    first.timesteps, second.timesteps = sched.timesteps[:6], sched.timesteps[6:]
    half = run_sampling_loop(model, first, x_T, DeviceNoise(seeds), eta=eta)
    rest = run_sampling_loop(model, second, half.latents, DeviceNoise(seeds, step0=6), eta=eta)
    assert torch.equal(rest.latents, whole.latents) and torch.equal(rest.images, whole.images)


# ---- 5. rows go to the steps with sigma != 0, whatever their t ---------------------------------------------------------
def test_trailing_spacing_consumes_a_row_on_every_step(eager):
    from synt_isic_amd.sampler import run_sampling_loop
    model, eta = eager.models["NV"], 0.5
    sched = _ddim(7, timestep_spacing="trailing")
    assert sched.timesteps.tolist() == [999, 856, 713, 570, 428, 285, 142]
    assert _n_noise(sched, eta) == 7                           # 6 steps have t > 0 ... and so has the last one
    x_T = _x_T([1, 2, 3])
    z = _z_rows(7)
    with pytest.raises(ValueError, match="noise must be fp32"):
        run_sampling_loop(model, sched, x_T, z[:6], eta=eta)
    res = run_sampling_loop(model, sched, x_T, z, return_trajectory=True, eta=eta)
    frames = _python_loop(model, sched, x_T, z, eta)
    assert res.steps_done == 7 and torch.equal(res.trajectory, frames)
    other = z.clone()
    other[6] += 1.0
    assert not torch.equal(run_sampling_loop(model, sched, x_T, other, eta=eta).latents, res.latents)      # row 7 is read


# ---- 6. eta = 0 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_eta_0_ignores_the_noise_source(mode, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    s = eager if mode == "eager" else graph
    model, seeds = s.models["NV"], [5, 6, 7]
    sched = _ddim(T)
    assert sched.config.set_alpha_to_one and sched.config.clip_sample
    x_T = _x_T(seeds)
    none = run_sampling_loop(model, sched, x_T, None, return_trajectory=True)
    _same(run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), return_trajectory=True), none)
    _same(run_sampling_loop(model, sched, x_T, torch.empty((0, B) + CHW, device=DEV), return_trajectory=True), none)
    with pytest.raises(ValueError, match="noise must be fp32"):
        run_sampling_loop(model, sched, x_T, _z_rows(T - 1))
    # the last step returns its clamped x0
    assert torch.isfinite(none.latents).all() and float(none.latents.abs().max()) <= 1.0


# ---- 7. the chain against the oracle -----------------------------------------------------------------------------------
def test_chain_against_the_oracle(eager, synthetic_sd):
    """T = 8, two seeds: oracle.unet.unet_forward + ddim_ref.step on the CPU.  1e-3 max-abs is the project's tolerance for this
    comparison under DDPM (tests/test_gpu_sampler.py::test_loop_equals_reference_style_python_loop)."""
    from oracle import unet as ounet
    from synt_isic_amd.sampler import draw_noise, run_sampling_loop
    model = eager.models["NV"]
    sched = _ddim(8)
    r = ddim_ref.DDIMSchedulerRef(beta_schedule="squaredcos_cap_v2")
    r.set_timesteps(8)
    x_T, z = draw_noise([3, 4], 7, CHW)
    for eta in (0.0, 1.0):
        zz = z if eta else None
        assert _n_noise(sched, eta) == (7 if eta else 0)
        res = run_sampling_loop(model, sched, x_T.to(DEV), zz.to(DEV) if zz is not None else None, return_trajectory=True, eta=eta)
        x, zi, diffs = x_T.clone(), 0, []
        with torch.no_grad():
            for i, t in enumerate(r.timesteps):
                vn = None
                if zz is not None and r.coefficients(t, eta)[4] != 0.0:
                    vn = zz[zi]
                    zi += 1
                x = r.step(ounet.unet_forward(synthetic_sd, x, int(t)), int(t), x, eta=eta, noise=vn)
                diffs.append((res.trajectory[i].cpu() - x).abs().max().item())
        print(f"eta = {eta}: max |x - oracle chain| per step = {[f'{d:.2e}' for d in diffs]}")
        assert max(diffs) <= 1e-3


# ---- 8. public interface -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["host", "device"])
def test_generate_seeds_under_ddim(noise, eager):
    from synt_isic_amd.dist import shard_seeds
    seeds, Tn = [3, 0x7FFFFFFF, 12345, 8], 10
    ddpm = eager.generate_seeds("NV", seeds, Tn, (32, 32), noise=noise)
    for eta in (0.0, 0.7):
        res = eager.generate_seeds("NV", seeds, Tn, (32, 32), noise=noise, scheduler="ddim", eta=eta, return_trajectory=True)
        assert res.steps_done == Tn and not res.cancelled and res.scheduler == "ddim" and res.eta == eta
        assert res.seeds == ddpm.seeds and res.timesteps == ddpm.timesteps and res.noise_hashes == ddpm.noise_hashes
        assert torch.isfinite(res.latents).all() and not torch.equal(res.latents, ddpm.latents)
        for b, sd in enumerate(seeds[:2]):                       # each image alone
            one = eager.generate_seeds("NV", [sd], Tn, (32, 32), noise=noise, scheduler="ddim", eta=eta)
            assert torch.equal(one.latents[0], res.latents[b]) and torch.equal(one.images[0], res.images[b])
        parts = [eager.generate_seeds("NV", shard_seeds(seeds, 2, r), Tn, (32, 32), noise=noise, scheduler="ddim", eta=eta)
                 for r in range(2)]
        assert torch.equal(torch.cat([p.images for p in parts]), res.images)
        assert torch.equal(torch.cat([p.latents for p in parts]), res.latents)
        assert [h for p in parts for h in p.noise_hashes] == res.noise_hashes
    assert ddpm.scheduler == "ddpm" and ddpm.eta == 0.0
    det = eager.generate_seeds("NV", seeds, Tn, (32, 32), noise=noise, scheduler="ddim")
    assert not torch.equal(det.latents, res.latents)             # eta reaches the table
    # generate(): scheduler and eta go through
    imgs, traj = eager.generate(seeds[0], "NV", Tn, size=(32, 32), noise=noise, scheduler="ddim", eta=0.7)
    assert traj is None and np.array_equal(imgs[0], res.images[0].cpu().numpy())
    imgs0, _ = eager.generate(seeds[0], "NV", Tn, size=(32, 32), noise=noise, scheduler="ddim")
    assert np.array_equal(imgs0[0], det.images[0].cpu().numpy())
    # a stop request ends a DDIM run like a DDPM one
    eager.request_stop()
    stopped = eager.generate_seeds("NV", seeds, Tn, (32, 32), noise=noise, scheduler="ddim", eta=0.7)
    assert stopped.cancelled and stopped.steps_done < Tn
    assert eager.generate_images("NV", seeds, Tn, size=(32, 32), noise=noise, scheduler="ddim", eta=0.7).steps_done == Tn


def test_host_mode_rows_are_draw_noises(eager):
    """host mode: x_T, then one z per step with sigma != 0 from the image's CPU generator -- the streamed run equals the
    buffer run over draw_noise's rows; at eta = 0 nothing but x_T is drawn and no staging buffer is made"""
    from synt_isic_amd.sampler import Sampler, draw_noise, run_sampling_loop
    seeds, Tn = [21, 22], 10
    sched = eager.create_scheduler(Tn, "ddim")
    x_T, z = draw_noise(seeds, _n_noise(sched, 0.7), CHW)
    want = run_sampling_loop(eager.models["NV"], sched, x_T.to(DEV), z.to(DEV), eta=0.7)
    got = eager.generate_seeds("NV", seeds, Tn, (32, 32), scheduler="ddim", eta=0.7)
    assert torch.equal(got.latents, want.latents)
    fresh = Sampler(DEV)
    fresh.models["NV"] = eager.models["NV"]
    det = fresh.generate_seeds("NV", seeds, Tn, (32, 32), scheduler="ddim")
    assert torch.equal(det.latents, run_sampling_loop(eager.models["NV"], sched, x_T.to(DEV), None).latents)
    assert fresh._noise_buffers == {}


def test_module_level_generate_passes_the_rule_through(synthetic_sd):
    from synt_isic_amd import sampler as S
    old = S._default_sampler
    try:
        S._default_sampler = S.Sampler(DEV)
        S._default_sampler.add_model("NV", synthetic_sd)
        a, _ = S.generate(6, "NV", 4, size=(32, 32), scheduler="ddim", eta=0.5)
        b = S._default_sampler.generate_seeds("NV", [6], 4, (32, 32), scheduler="ddim", eta=0.5)
        c = S._default_sampler.generate_seeds("NV", [6], 4, (32, 32))
        assert np.array_equal(a, b.images.cpu().numpy()) and not torch.equal(b.latents, c.latents)
        with pytest.raises(ValueError):
            S.generate(6, "NV", 4, size=(32, 32), scheduler="heun")
    finally:
        S._default_sampler = old


# ---- 9. the captured step ----------------------------------------------------------------------------------------------
def test_graph_is_keyed_by_the_rule(graph):
    from synt_isic_amd import _lib
    lib = _lib.load()
    mg = graph.models["NV"]
    seeds, Tn = [31, 32], 8
    before = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device")
    first = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device", scheduler="ddim", eta=0.7)
    builds = lib.sisic_unet_graph_builds(mg.handle)
    assert builds >= 2
    second = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device", scheduler="ddim", eta=0.7)
    other = graph.generate_seeds("NV", [77, 78], Tn, (32, 32), noise="device", scheduler="ddim", eta=0.3)
    assert lib.sisic_unet_graph_builds(mg.handle) == builds             # same rule, shape and noise source: replayed
    assert torch.equal(first.latents, second.latents) and not torch.equal(first.latents, other.latents)
    # the flag chooses another kernel: its own capture
    flagged = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device", scheduler="ddim", eta=0.7, use_clipped_model_output=True)
    assert lib.sisic_unet_graph_builds(mg.handle) == builds + 1 and not torch.equal(flagged.latents, first.latents)
    # a DDPM call never replays a DDIM step, nor the other way round
    after = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device")
    assert lib.sisic_unet_graph_builds(mg.handle) == builds + 2
    assert torch.equal(after.latents, before.latents) and torch.equal(after.images, before.images)
    again = graph.generate_seeds("NV", seeds, Tn, (32, 32), noise="device", scheduler="ddim", eta=0.7)
    assert torch.equal(again.latents, first.latents)
