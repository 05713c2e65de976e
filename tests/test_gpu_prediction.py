"""v- and x0-prediction models in the sampler (include/sisic.h SISIC_PRED_*): the three step kernels under
the two new types bit for bit against tests/pred_ref.py; tails, unaligned tensors, generated noise and the edit epilogue; the
scheduler mirrors' per-call keyword; the fused loop (eager and graph-replayed, plain, guided and edited) against a Python loop
over the model and the mirror; the key of a captured step; the refusals.  Full UNet at 3x32x32, B = 2, T = 3 or 4."""
import ctypes as C

import numpy as np
import pytest
import torch

import inpaint_ref
import pred_ref

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
B, T = 2, 4
SEEDS = [11, (1 << 33) + 2]
NEW_TYPES = ("sample", "v_prediction")
# {sb, sa, ...} with sa^2 + sb^2 = 1; each clamps a good share of its x0 at clip = 1
FIXED = {"ddpm": (0.6, 0.8, 0.3, 0.65, 0.25), "ddim": (0.6, 0.8, 0.9, 0.4, 0.15), "dpmsolver++": (0.6, 0.8, 0.9, 0.3, 0.25, -0.1)}


def _scheduler(rule, steps=T):
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    if rule == "ddpm":
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    elif rule == "ddim":
        s = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    else:
        s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                           timestep_spacing="leading", algorithm_type=rule)
    s.set_timesteps(steps)
    return s


def _table(sched, eta):
    return sched.rule_table(eta)[1]


def _x_T(seeds, chw=CHW):
    return torch.stack([torch.randn(chw, generator=torch.Generator().manual_seed(7000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _step(rule, o, x, z, hist, row, clip, kind, flag=False, out=None):
    """the buffer-noise entry of a rule under a type; returns (prev_sample, hist or None)"""
    from synt_isic_amd import ops
    if rule == "ddpm":
        return ops.ddpm_step(o, x, z, row, clip, out=out, prediction_type=kind), None
    if rule == "ddim":
        return ops.ddim_step(o, x, z, row, clip, flag, out=out, prediction_type=kind), None
    return ops.dpmpp_step(o, x, z, hist, row, clip, out=out, prediction_type=kind), hist


@pytest.fixture(scope="module")
def eager(synthetic_sd):
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV)
    s.add_model("NV", synthetic_sd).set_graph_mode(0)
    return s


@pytest.fixture(scope="module")
def graph(synthetic_sd):
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV)
    s.add_model("NV", synthetic_sd).set_graph_mode(1)
    return s


class _as_type:
    """the model under a prediction type for the length of a block; epsilon again after it"""

    def __init__(self, model, kind):
        self.model, self.kind = model, kind

    def __enter__(self):
        return self.model.set_prediction_type(self.kind)

    def __exit__(self, *exc):
        self.model.set_prediction_type("epsilon")


# ---- 1. one step ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_inputs():
    g = torch.Generator().manual_seed(25)
    n = 2 * 3 * 32 * 32
    return tuple(torch.randn(n, generator=g) for _ in range(4))          # o, x, z, hist on the host


@pytest.fixture(scope="module")
def table_rows():
    """per rule: the fixed row and rows of the cosine table at T = 20 -- the first (t = 950 on the leading grid; DPM-Solver++'s
    linspace grid starts at t = 999, where sa = 4.9e-5 and the epsilon rule divides by it), an interior one (DPM-Solver++: second
    order, it reads the history) and the last"""
    rows = {}
    for rule in ("ddpm", "ddim"):
        s = _scheduler(rule, 20)
        tab = _table(s, 0.5)
        rows[rule] = [FIXED[rule]] + [tuple(float(v) for v in tab[i]) for i in (0, 10, 19)]
    from synt_isic_amd.scheduler import HipDPMSolverMultistepScheduler
    s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", algorithm_type="sde-dpmsolver++")
    s.set_timesteps(20)
    assert int(s.timesteps[0]) == 999
    tab = s.coefficient_table()
    rows["dpmsolver++"] = [FIXED["dpmsolver++"]] + [tuple(float(v) for v in tab[i]) for i in (0, 10, 19)]
    assert [r[5] != 0.0 for r in rows["dpmsolver++"]] == [True, False, True, False] and rows["dpmsolver++"][1][1] < 1e-4
    return rows


@pytest.mark.parametrize("clip", [1.0, 0.0])
@pytest.mark.parametrize("kind", NEW_TYPES)
def test_one_step_is_the_restatement_bit_for_bit(step_inputs, table_rows, kind, clip):
    o, x, z, h = step_inputs
    od, xd, zd, hd = (t.to(DEV) for t in step_inputs)
    for rule, rows in table_rows.items():
        for row in rows:
            for flag in ((False, True) if rule == "ddim" else (False,)):
                for noise in (z, None):
                    want, want_hist = pred_ref.step_row(rule, o, x, noise, h, row, clip, kind, flag)
                    hist = hd.clone()
                    got, got_hist = _step(rule, od, xd, zd if noise is not None else None, hist, row, clip, kind, flag)
                    assert torch.isfinite(want).all()
                    assert torch.equal(got.cpu(), want), (rule, row, flag, noise is None, float((got.cpu() - want).abs().max()))
                    if want_hist is not None:
                        assert torch.equal(got_hist.cpu(), want_hist), (rule, row)          # the history is the clamped x0
        # the type reaches the kernel: the same inputs under epsilon give another result
        eps_out, _ = _step(rule, od, xd, zd, hd.clone(), FIXED[rule], clip, "epsilon")
        new_out, _ = _step(rule, od, xd, zd, hd.clone(), FIXED[rule], clip, kind)
        assert not torch.equal(eps_out, new_out)
        # in place
        inplace, hist = xd.clone(), hd.clone()
        _step(rule, od, inplace, zd, hist, FIXED[rule], clip, kind, out=inplace)
        assert torch.equal(inplace.cpu(), pred_ref.step_row(rule, o, x, z, h, FIXED[rule], clip, kind)[0])
    if clip > 0:
        share = float((pred_ref.raw_x0(o, x, torch.tensor(0.6), torch.tensor(0.8), kind).abs() > 1.0).float().mean())
        assert 0.05 <= share <= 0.95, share                                  # both sides of the clamp are exercised


def test_epsilon_context_is_untouched_by_the_typed_ones(step_inputs):
    """one context per (device, type): a typed call never changes what the default context computes"""
    from synt_isic_amd import _lib, ops
    import ddim_ref
    o, x, z, _ = step_inputs
    od, xd, zd = o.to(DEV), x.to(DEV), z.to(DEV)
    lib = _lib.load()
    before = ops.ddim_step(od, xd, zd, FIXED["ddim"], 1.0)
    ops.ddim_step(od, xd, zd, FIXED["ddim"], 1.0, prediction_type="v_prediction")
    assert torch.equal(ops.ddim_step(od, xd, zd, FIXED["ddim"], 1.0), before)
    assert torch.equal(before.cpu(), ddim_ref.step_row(o, x, z, FIXED["ddim"], 1.0))
    assert lib.sisic_step_prediction_type(ops.context(DEV)) == 0
    assert lib.sisic_step_prediction_type(ops.context(DEV, "v_prediction")) == 2
    assert lib.sisic_step_prediction_type(ops.context(DEV, "sample")) == 1
    assert ops.context(DEV, "sample") is ops.context(DEV, "sample") and ops.context(DEV, "epsilon") is ops.context(DEV)


# ---- 2. tails, unaligned tensors, generated noise, the edit epilogue ------------------------------------------------------
def _view(t, offset):
    n = t.numel()
    return torch.cat([torch.zeros(offset), t.reshape(-1), torch.zeros(4)]).to(DEV)[offset:offset + n]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("kind", NEW_TYPES)
def test_scalar_tail_and_unaligned_tensors(kind, offset):
    """105 elements: 26 float4 and a tail of one; a base pointer one float off a 16-byte line: the element-by-element path"""
    n = 105
    g = torch.Generator().manual_seed(n + offset)
    host = [torch.randn(n, generator=g) for _ in range(4)]
    for rule in FIXED:
        for flag in ((False, True) if rule == "ddim" else (False,)):
            o, x, z, h = (_view(t, offset) for t in host)
            assert o.data_ptr() % 16 == 4 * offset and h.data_ptr() % 16 == 4 * offset
            want, want_hist = pred_ref.step_row(rule, host[0], host[1], host[2], host[3], FIXED[rule], 1.0, kind, flag)
            out = _view(torch.zeros(n), offset)
            _step(rule, o, x, z, h, FIXED[rule], 1.0, kind, flag, out=out)
            assert torch.equal(out.cpu(), want), (rule, flag)
            if want_hist is not None:
                assert torch.equal(h.cpu(), want_hist)


@pytest.mark.parametrize("offset", [0, 1])
def test_rng_and_edit_entries_equal_the_buffer_entry_under_v(offset):
    """images of 105 floats (3 x 5 x 7: blocks straddle two images) and, per offset, tensors on or off a line: the generated-noise
    entry is the buffer entry fed ops.noise_fill's rows, and the edited entry is that result through the restated epilogue"""
    from synt_isic_amd import ops
    kind, seeds, step = "v_prediction", [4, (1 << 35) + 6, 0x7FFFFFFF], 17
    npi, hw = 105, 35
    n = len(seeds) * npi
    g = torch.Generator().manual_seed(500 + offset)
    o_h, x_h, h_h = (torch.randn(n, generator=g) for _ in range(3))
    image_h = torch.rand(n, generator=g) * 2 - 1
    mask_h = torch.tensor([0.0, 1.0, 0.25, 0.7])[torch.randint(0, 4, (len(seeds) * hw,), generator=g)]
    z = ops.noise_fill(seeds, npi, step).reshape(-1)
    e1 = ops.noise_fill(seeds, npi, step, tag=inpaint_ref.TAG_KNOWN).reshape(len(seeds), 3, 5, 7).cpu()
    e2 = ops.noise_fill(seeds, npi, step, tag=inpaint_ref.TAG_JUMP).reshape(len(seeds), 3, 5, 7).cpu()
    erow = (0.8, 0.6, 0.65, 0.75)
    shape = (len(seeds), 3, 5, 7)
    for rule in FIXED:
        row = FIXED[rule]
        o, x = _view(o_h, offset), _view(x_h, offset)
        ha, hb, hc = (_view(h_h, offset) for _ in range(3))
        want, _ = _step(rule, o, x, z, ha, row, 1.0, kind)
        assert torch.equal(want.cpu(), pred_ref.step_row(rule, o_h, x_h, z.cpu(), h_h, row, 1.0, kind)[0])
        image, mask = _view(image_h, offset), _view(mask_h, offset)
        if rule == "ddpm":
            got = ops.ddpm_step_rng(o, x, seeds, step, row, 1.0, prediction_type=kind)
            edited = ops.ddpm_step_edit(o, x, seeds, step, row, image, mask, erow, 1.0, prediction_type=kind)
        elif rule == "ddim":
            got = ops.ddim_step_rng(o, x, seeds, step, row, 1.0, prediction_type=kind)
            edited = ops.ddim_step_edit(o, x, seeds, step, row, image, mask, erow, 1.0, prediction_type=kind)
        else:
            got = ops.dpmpp_step_rng(o, x, seeds, step, hb, row, 1.0, prediction_type=kind)
            edited = ops.dpmpp_step_edit(o, x, seeds, step, hc, row, image, mask, erow, 1.0, prediction_type=kind)
            assert torch.equal(hb, ha) and torch.equal(hc, ha)                 # the epilogue leaves the history alone
        assert torch.equal(got, want), rule
        blended = inpaint_ref.edit_one(want.cpu().reshape(shape), image_h.reshape(shape), mask_h.reshape(len(seeds), 1, 5, 7), e1, e2, erow)
        assert torch.equal(edited.cpu().reshape(shape), blended), rule


# ---- 3. the mirrors' keyword ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", NEW_TYPES)
@pytest.mark.parametrize("rule", ["ddpm", "ddim", "dpmsolver++", "sde-dpmsolver++"])
def test_scheduler_mirrors_take_the_type_per_call(rule, kind):
    """five steps over given model outputs, the stateful DPM-Solver++ mirror included, against the restatement's chain"""
    g = torch.Generator().manual_seed(33)
    shape = (B,) + CHW
    x_T = torch.randn(shape, generator=g)
    outs = [torch.randn(shape, generator=g) for _ in range(5)]
    zs = [torch.randn(shape, generator=g) for _ in range(5)]
    sched = _scheduler(rule, 5)
    eta = 0.5 if rule == "ddim" else 0.0
    tab = _table(sched, eta)
    clip = sched.config.clip_sample_range if sched.config.clip_sample else 0.0
    kw = dict(eta=eta) if rule == "ddim" else {}
    x, xr, hist = x_T.to(DEV), x_T.clone(), None
    for i, t in enumerate(sched.timesteps):
        x = sched.step(outs[i].to(DEV), t, x, variance_noise=zs[i].to(DEV), prediction_type=kind, **kw).prev_sample
        xr, hist = pred_ref.step_row(sched.rule, outs[i], xr, zs[i], hist, tuple(float(v) for v in tab[i]), clip, kind)
        assert torch.equal(x.cpu(), xr), (rule, i)
    if sched.rule == "dpmsolver++":
        assert bool((tab[1:4, 5] != 0).all())                              # the interior steps read the history
    sched.set_timesteps(5)                                                 # a new run (the DPM-Solver++ mirror counts its steps)
    with pytest.raises(NotImplementedError):
        sched.step(outs[0].to(DEV), sched.timesteps[0], x_T.to(DEV), prediction_type="velocity")


# ---- 4. the fused loop against the Python loop ---------------------------------------------------------------------------
def _python_loop(model, sched, eta, x_T, z, labels=None, null=None, w=1.0):
    """image_generator.py:395-403 over the drop-in objects: model(x, t).sample, then the mirror's step under the MODEL's type.
    z rows go to the steps with sigma != 0.  Returns every frame."""
    from synt_isic_amd import ops
    sched.set_timesteps(sched.timesteps.numel())                          # a new run (DPM-Solver++: no history)
    tab = _table(sched, eta)
    kw = dict(eta=eta) if sched.rule == "ddim" else {}
    x, zi, frames = x_T.clone(), 0, []
    for i, t in enumerate(sched.timesteps):
        if labels is None:
            o = model(x, t).sample
        else:
            o = model(x, t, class_labels=labels).sample
            if w != 1.0:
                o = ops.guide_eps(o, model(x, t, class_labels=[null] * len(labels)).sample, w)
        vn = None
        if z is not None and float(tab[i, 4]) != 0.0:
            vn, zi = z[zi], zi + 1
        x = sched.step(o, t, x, variance_noise=vn, prediction_type=model.prediction_type, **kw).prev_sample
        frames.append(x)
    assert z is None or zi == z.shape[0]
    return torch.stack(frames)


@pytest.mark.parametrize("rule", ["ddpm", "ddim", "sde-dpmsolver++"])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_fused_loop_equals_python_loop(mode, rule, eager, graph):
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    model = (eager if mode == "eager" else graph).models["NV"]
    sched, eta = _scheduler(rule), (0.5 if rule == "ddim" else 0.0)
    tab = _table(sched, eta)
    noisy = [i for i in range(T) if float(tab[i, 4]) != 0.0]
    assert len(noisy) == T - 1
    if rule == "sde-dpmsolver++":
        assert bool((tab[1:3, 5] != 0).all())                              # T = 4: two second-order steps
    x_T = _x_T(SEEDS)
    host = torch.randn((len(noisy), B) + CHW, generator=torch.Generator().manual_seed(78)).to(DEV)
    filled = torch.stack([ops.noise_fill(SEEDS, int(np.prod(CHW)), i).reshape((B,) + CHW) for i in noisy])
    plain = run_sampling_loop(model, sched, x_T, host, eta=eta)
    assert plain.prediction_type == "epsilon"
    for kind in (("v_prediction", "sample") if rule == "ddim" else ("v_prediction",)):
        with _as_type(model, kind):
            for z, source in ((host, host), (filled, DeviceNoise(SEEDS))):
                frames = _python_loop(model, sched, eta, x_T, z)
                res = run_sampling_loop(model, sched, x_T, source, return_trajectory=True, eta=eta)
                assert res.steps_done == T and res.prediction_type == kind
                assert torch.equal(res.trajectory, frames) and torch.equal(res.latents, frames[-1])
                assert torch.equal(res.images, ops.denorm_u8(frames[-1]))
                kept = run_sampling_loop(model, sched, x_T, source, return_trajectory=True, save_indices=[1, T - 1], eta=eta)
                assert kept.trajectory_steps == [1, T - 1] and torch.equal(kept.trajectory, frames[[1, T - 1]])
            assert torch.isfinite(res.latents).all()
    # epsilon again: the bits of before the alternation
    again = run_sampling_loop(model, sched, x_T, host, eta=eta)
    assert torch.equal(again.latents, plain.latents) and torch.equal(again.images, plain.images)
    assert not torch.equal(res.latents, plain.latents)                     # the type reaches the loop


# ---- 5. guidance ---------------------------------------------------------------------------------------------------------
def test_guided_run_under_v_equals_two_labelled_passes(synthetic_sd):
    """a conditional model at guidance_scale = 3 under v, DDIM, T = 3: two labelled passes, ops.guide_eps and the mirror"""
    from synt_isic_amd.sampler import DeviceNoise, Guidance, Sampler, run_sampling_loop
    from synt_isic_amd.weights import synthetic_unet_state_dict
    n_class, null, labels = 5, 4, [0, 3]
    s = Sampler(DEV)
    model = s.add_conditional_model(("MEL", "BCC", "AKIEC", "BKL"), synthetic_unet_state_dict(num_class_embeds=n_class),
                                    prediction_type="v_prediction")
    assert model.prediction_type == "v_prediction" and s.models["BKL"] is model
    sched, eta = _scheduler("ddim", 3), 0.5
    x_T = _x_T(SEEDS)
    from synt_isic_amd import ops
    tab = _table(sched, eta)
    filled = torch.stack([ops.noise_fill(SEEDS, int(np.prod(CHW)), i).reshape((B,) + CHW) for i in range(3) if float(tab[i, 4]) != 0.0])
    frames = _python_loop(model, sched, eta, x_T, filled, labels, null, 3.0)
    res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta, guidance=Guidance(labels, null, 3.0))
    assert res.prediction_type == "v_prediction" and torch.equal(res.trajectory, frames)
    unguided = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), eta=eta, guidance=Guidance(labels, null, 1.0))
    assert torch.equal(unguided.latents, _python_loop(model, sched, eta, x_T, filled, labels, null, 1.0)[-1])
    assert not torch.equal(unguided.latents, res.latents)


# ---- 6. an edited run ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_edited_ddpm_run_under_v(mode, eager, graph):
    """a mask and one jump at T = 4 (six passes): every frame against the model's own outputs stepped by pred_ref and blended by
    inpaint_ref on the CPU, with the normals ops.noise_fill writes under tags 0, 5 and 6"""
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    model = (eager if mode == "eager" else graph).models["NV"]
    sched = _scheduler("ddpm")
    schedule = inpaint_ref.resample_schedule(T, 2, 2)
    assert len(schedule) == 6 and sum(1 for _, j in schedule if j) == 1
    g = torch.Generator().manual_seed(91)
    image = (torch.rand((B,) + CHW, generator=g) * 2 - 1).to(DEV)
    mask = torch.tensor([0.0, 1.0, 0.25, 0.7])[torch.randint(0, 4, (B, 1) + CHW[1:], generator=g)].to(DEV)
    rows = inpaint_ref.edit_rows(sched.alphas.numpy(), sched.timesteps.tolist(), schedule, "ddpm")
    tab = sched.coefficient_table()
    x_T = _x_T(SEEDS)
    npi = int(np.prod(CHW))
    with _as_type(model, "v_prediction"):
        res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, edit=Edit(image, mask, schedule))
        assert res.steps_done == 6 and res.prediction_type == "v_prediction"
        x = x_T
        for p, (i, _) in enumerate(schedule):
            o = model(x, sched.timesteps[i]).sample
            z = ops.noise_fill(SEEDS, npi, p).reshape(x.shape).cpu()
            u = pred_ref.ddpm_step_row(o.cpu(), x.cpu(), z, tuple(float(v) for v in tab[i]), 1.0, "v_prediction")
            e1 = ops.noise_fill(SEEDS, npi, p, tag=inpaint_ref.TAG_KNOWN).reshape(x.shape).cpu() if float(rows[p][1]) != 0.0 else None
            e2 = ops.noise_fill(SEEDS, npi, p, tag=inpaint_ref.TAG_JUMP).reshape(x.shape).cpu() if float(rows[p][3]) != 0.0 else None
            want = inpaint_ref.edit_one(u, image.cpu(), mask.cpu(), e1, e2, rows[p])
            assert torch.equal(res.trajectory[p].cpu(), want), (p, schedule[p])
            x = res.trajectory[p]


# ---- 7. the key of a captured step ---------------------------------------------------------------------------------------
def test_graph_is_keyed_by_the_prediction_type(graph, synthetic_sd):
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import DeviceNoise, Sampler, run_sampling_loop
    lib = _lib.load()
    model = graph.models["NV"]
    never = Sampler(DEV).add_model("NV", synthetic_sd).set_graph_mode(1)        # a handle that never has a type set
    sched = _scheduler("ddim", 6)
    x_T = _x_T(SEEDS)
    run = lambda m: run_sampling_loop(m, sched, x_T, DeviceNoise(SEEDS), eta=0.5)
    first = run(model)
    builds = lib.sisic_unet_graph_builds(model.handle)
    assert builds >= 1 and torch.equal(run(model).latents, first.latents)
    assert lib.sisic_unet_graph_builds(model.handle) == builds             # same type: replayed
    with _as_type(model, "v_prediction"):
        assert lib.sisic_unet_prediction_type(model.handle) == 2
        v = run(model)
        assert lib.sisic_unet_graph_builds(model.handle) == builds + 1     # an epsilon step is never replayed for a v model
        assert torch.equal(run(model).latents, v.latents) and lib.sisic_unet_graph_builds(model.handle) == builds + 1
    assert lib.sisic_unet_prediction_type(model.handle) == 0
    second = run(model)
    assert lib.sisic_unet_graph_builds(model.handle) == builds + 2
    assert torch.equal(second.latents, first.latents) and torch.equal(second.images, first.images)
    assert not torch.equal(v.latents, first.latents)
    # ... and they are the bits of a handle that never had a type set
    assert lib.sisic_unet_prediction_type(never.handle) == 0
    ref = run(never)
    assert torch.equal(ref.latents, first.latents) and torch.equal(ref.images, first.images)
    # the forward pass does not know the type
    t = sched.timesteps[0]
    plain = model(x_T, t).sample
    with _as_type(model, "sample"):
        assert torch.equal(model(x_T, t).sample, plain)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_private_flag_bits_and_unknown_types_are_refused(eager):
    from synt_isic_amd import _lib, ops
    lib = _lib.load()
    model = eager.models["NV"]
    h = model.handle
    for bad in (-1, 3, 256):
        assert lib.sisic_unet_set_prediction_type(h, bad) == _lib.SISIC_EINVAL
        assert lib.sisic_unet_prediction_type(h) == 0                      # the setting is unchanged
    assert lib.sisic_unet_set_prediction_type(h, 2) == 0 and lib.sisic_unet_set_prediction_type(h, 7) == _lib.SISIC_EINVAL
    assert lib.sisic_unet_prediction_type(h) == 2
    assert lib.sisic_unet_set_prediction_type(h, 0) == 0
    ctx = C.c_void_p()
    _lib.check(lib.sisic_create(torch.cuda.current_device(), C.byref(ctx)))
    try:
        assert lib.sisic_step_prediction_type(ctx) == 0
        for bad in (-1, 3):
            assert lib.sisic_set_step_prediction_type(ctx, bad) == _lib.SISIC_EINVAL and lib.sisic_step_prediction_type(ctx) == 0
        assert lib.sisic_set_step_prediction_type(ctx, 1) == 0 and lib.sisic_step_prediction_type(ctx) == 1
    finally:
        lib.sisic_destroy(ctx)
    # a caller's rule_flags takes SISIC_RULE_FLAG_CLIPPED_OUTPUT only: the private bits that carry the type are refused
    sched = _scheduler("ddim")
    ts = sched.timesteps.to(torch.int64).contiguous()
    coef = sched.coefficient_table(0.0).contiguous()
    x = _x_T(SEEDS)
    before = x.clone()
    done = C.c_int(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for flags in (1 << 8, 2 << 8, (1 << 8) | 1, 2):
        rc = lib.sisic_sample_frames_rule(h, x.data_ptr(), B, 32, 32, T, C.cast(ts.data_ptr(), _lib.c_int64_p),
                                          C.cast(coef.data_ptr(), _lib.c_float_p), 1.0, _lib.RULE_DDIM, flags, None, None, None,
                                          None, None, C.byref(done), stream)
        assert rc == _lib.SISIC_EINVAL and b"rule flags" in lib.sisic_last_error(), flags
    torch.cuda.synchronize()
    assert torch.equal(x, before) and done.value == 0
    # DDIM under sample prediction divides by sb: a row with sb == 0 is refused
    o = torch.zeros(8, device=DEV)
    with pytest.raises(_lib.SisicError, match="sqrt_beta_prod is zero under sample prediction"):
        ops.ddim_step(o, o, None, (0.0, 1.0, 1.0, 0.0, 0.0), 1.0, prediction_type="sample")
    for kind in pred_ref.TYPES:
        with pytest.raises(_lib.SisicError, match="sqrt_alpha_prod is zero"):   # zero-terminal-SNR tables stay refused
            ops.ddim_step(o, o, None, (1.0, 0.0, 1.0, 0.0, 0.0), 1.0, prediction_type=kind)
