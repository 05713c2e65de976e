"""Image-to-image and RePaint inpainting on the GPU (include/sisic.h "image editing"): the edit epilogue of
the step kernels bit for bit against tests/inpaint_ref.py; the fused loop (eager and graph-replayed) against a Python loop over
the model, the scheduler mirror's step, ``ops.noise_fill`` and the restated blend; the graph key; batch independence; a run cut
into calls; image-to-image; and the public interface.  Full UNet at 3x32x32, B = 3, T = 12."""
import numpy as np
import pytest
import torch

import inpaint_ref
import philox_ref
from test_gpu_device_noise import eager, graph  # noqa: F401  (the two graph-mode fixtures, shared)

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
B, T = 3, 12
SEEDS = [11, (1 << 33) + 2, 0]
N_CLASS, NULL, LABELS = 5, 4, [0, 3, 2]
CLASSES = ("MEL", "BCC", "AKIEC", "BKL")
FP32_ULP = 2.0 ** -23
JUMPS = (12, 4, 2)                                 # (T, jump_length, n_resample): 20 passes


# ---- shared inputs -----------------------------------------------------------------------------------------------------
def _x_T(seeds, chw=CHW):
    return torch.stack([torch.randn(chw, generator=torch.Generator().manual_seed(5000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _image(n=B, chw=CHW, seed=17):
    """a known image in [-1, 1], different for every image of the batch"""
    return (torch.rand((n,) + tuple(chw), generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def _soft_mask(n=B, hw=CHW[1:], seed=23):
    """[n,1,H,W] with the values 0, 1, 0.25 and 0.7, different for every image of the batch"""
    pick = torch.randint(0, 4, (n, 1) + tuple(hw), generator=torch.Generator().manual_seed(seed))
    return torch.tensor([0.0, 1.0, 0.25, 0.7])[pick].to(DEV)


def _hard_mask(n=B, hw=CHW[1:]):
    """1 (keep) outside a centred rectangle, 0 (synthesise) inside"""
    m = torch.ones((n, 1) + tuple(hw))
    m[:, :, hw[0] // 4:3 * hw[0] // 4, hw[1] // 4:3 * hw[1] // 4] = 0.0
    return m.to(DEV)


def _scheduler(rule, T=T):
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    if rule == "ddpm":
        s = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    elif rule == "ddim":
        s = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    else:
        s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                           timestep_spacing="leading", algorithm_type=rule)
    s.set_timesteps(T)
    return s


def _ref_rows(sched, schedule):
    return inpaint_ref.edit_rows(sched.alphas.numpy(), sched.timesteps.tolist(), schedule, sched.rule)


def _blend(u, image, mask, seeds, step, row):
    """the restated epilogue on the GPU's own normals of (seed, step, tag 5 / 6)"""
    from synt_isic_amd import ops
    npi = u[0].numel()
    e1 = ops.noise_fill(seeds, npi, step, tag=inpaint_ref.TAG_KNOWN).reshape(u.shape).cpu() if float(row[1]) != 0.0 else None
    e2 = ops.noise_fill(seeds, npi, step, tag=inpaint_ref.TAG_JUMP).reshape(u.shape).cpu() if float(row[3]) != 0.0 else None
    return inpaint_ref.edit_one(u.cpu(), image.cpu(), mask.cpu(), e1, e2, row).to(u.device)


def _python_loop(model, sched, eta, x_T, seeds, image, mask, schedule, labels=None, w=1.0):
    """one UNet call per schedule entry, the scheduler mirror's step under the entry's own timestep fed by noise_fill(tag 0),
    then the restated blend.  Returns every frame."""
    from synt_isic_amd import ops
    sched.set_timesteps(sched.timesteps.numel())                         # a new run (DPM-Solver++: no history)
    tab = sched.rule_table(eta)[1]
    rows = _ref_rows(sched, schedule)
    kw = dict(eta=eta) if sched.rule == "ddim" else {}
    x, frames = x_T.clone(), []
    for p, (i, _) in enumerate(schedule):
        t = sched.timesteps[i]
        if labels is None:
            eps = model(x, t).sample
        else:
            eps = model(x, t, class_labels=labels).sample
            if w != 1.0:
                eps = ops.guide_eps(eps, model(x, t, class_labels=[NULL] * len(labels)).sample, w)
        vn = None
        if float(tab[i, 4]) != 0.0:
            vn = ops.noise_fill(seeds, x[0].numel(), p).reshape(x.shape)
        u = sched.step(eps, t, x, variance_noise=vn, **kw).prev_sample
        x = _blend(u, image, mask, seeds, p, rows[p])
        frames.append(x)
    return torch.stack(frames)


def _plain(n):
    return [(i, 0) for i in range(n)]


# ---- 0. the two new streams of the contract ------------------------------------------------------------------------------
def test_tags_5_and_6_are_the_contracts():
    from synt_isic_amd import ops
    n = 3 * 32 * 32
    for tag in (inpaint_ref.TAG_KNOWN, inpaint_ref.TAG_JUMP):
        bits = ops.noise_bits(SEEDS, n, 7, tag).cpu().numpy().view(np.uint32)
        z = ops.noise_fill(SEEDS, n, 7, tag).cpu()
        for b, s in enumerate(SEEDS):
            assert np.array_equal(bits[b], philox_ref.noise_bits(s, 7, tag, n))
            rad = philox_ref.noise_normals(s, 7, tag, n)[1]
            err = np.abs(z[b].numpy().astype(np.float64) - inpaint_ref.noise([s], 7, tag, (n,))[0].numpy()) / np.maximum(1.0, rad)
            assert err.max() <= 16 * FP32_ULP
        assert not torch.equal(z, ops.noise_fill(SEEDS, n, 7, 0).cpu())


# ---- 1. one step --------------------------------------------------------------------------------------------------------
ROWS = [(0.8, 0.6, 1.0, 0.0), (1.0, 0.0, 1.0, 0.0), (0.8, 0.6, 0.65, 0.75), (1.0, 0.0, 0.92, 0.39)]
STEP_ROWS = {"ddpm": (0.6, 0.8, 0.3, 0.65, 0.25), "ddim": (0.6, 0.8, 0.9, 0.4, 0.15), "dpmpp": (0.6, 0.8, 0.7, 0.5, 0.2, -0.1)}


def _carve(t, offset):
    """the same values in a buffer that starts ``offset`` floats past a 16-byte line"""
    if not offset:
        return t
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("geometry", ["32x32", "5x7", "offset"])
@pytest.mark.parametrize("rule", ["ddpm", "ddim", "ddim-clipped", "dpmpp"])
def test_one_step_equals_the_restatement(rule, geometry):
    """the edited kernel = the restated epilogue applied to the unedited kernel's result (itself bit-exact against torch:
    tests/test_gpu_kernels.py, test_gpu_ddim.py, test_gpu_dpmpp.py), bit for bit; 32x32: the vector path, 9 blocks; 5x7: 105 per
    image, the scalar path with a block straddling images; offset: every tensor one float past a 16-byte line"""
    from synt_isic_amd import ops
    chw = (3, 5, 7) if geometry == "5x7" else CHW
    off = 1 if geometry == "offset" else 0
    g = torch.Generator().manual_seed(41)
    eps, x = (_carve(torch.randn((B,) + chw, generator=g).to(DEV), off) for _ in range(2))
    image, mask = _carve(_image(chw=chw), off), _carve(_soft_mask(hw=chw[1:]), off)
    assert set(mask.unique().tolist()) == {0.0, 0.25, float(torch.tensor(0.7)), 1.0}
    base = rule.split("-")[0]
    clipped = rule.endswith("clipped")
    for sigma_on in (True, False):
        coef = list(STEP_ROWS[base])
        if not sigma_on:
            coef[4] = 0.0
        for row in ROWS:
            for step in (0, 5):
                if base == "dpmpp":
                    k1s = (coef[5], 0.0)
                else:
                    k1s = (None,)
                for k1 in k1s:
                    if base == "ddpm":
                        u = ops.ddpm_step_rng(eps, x, SEEDS, step, coef, 1.0)
                        got = ops.ddpm_step_edit(eps, x, SEEDS, step, coef, image, mask, row, 1.0, out=_carve(torch.empty_like(u), off))
                    elif base == "ddim":
                        u = ops.ddim_step_rng(eps, x, SEEDS, step, coef, 1.0, clipped)
                        got = ops.ddim_step_edit(eps, x, SEEDS, step, coef, image, mask, row, 1.0, clipped,
                                                 out=_carve(torch.empty_like(u), off))
                    else:
                        c6 = coef[:5] + [k1]
                        prev = torch.randn((B,) + chw, generator=g).to(DEV)
                        if k1 == 0.0:
                            prev[1, 2, 3, 4] = float("nan")             # a first-order step does not read the history
                        h_ref, h_got = prev.clone(), _carve(prev.clone(), off)
                        u = ops.dpmpp_step_rng(eps, x, SEEDS, step, h_ref, c6, 1.0)
                        got = ops.dpmpp_step_edit(eps, x, SEEDS, step, h_got, c6, image, mask, row, 1.0,
                                                  out=_carve(torch.empty_like(u), off))
                        assert torch.equal(h_got, h_ref) and torch.isfinite(h_got).all()      # the model's x0, untouched
                    want = _blend(u, image, mask, SEEDS, step, row)
                    assert torch.isfinite(got).all()
                    assert torch.equal(got, want), (rule, geometry, sigma_on, row, step, k1)
    # in place (the loop's form), and the epilogue reaches the result
    coef, row = list(STEP_ROWS[base]), ROWS[2]
    if base == "ddpm":
        u = ops.ddpm_step_rng(eps, x, SEEDS, 3, coef, 1.0)
        xi = _carve(x.clone(), off)
        ops.ddpm_step_edit(eps, xi, SEEDS, 3, coef, image, mask, row, 1.0, out=xi)
        assert torch.equal(xi, _blend(u, image, mask, SEEDS, 3, row)) and not torch.equal(xi, u)


def test_one_step_refusals():
    from synt_isic_amd import ops
    from synt_isic_amd._lib import SisicError
    eps, x, image, mask = _x_T(SEEDS), _x_T([4, 5, 6]), _image(), _soft_mask()
    coef = STEP_ROWS["ddpm"]
    with pytest.raises(ValueError):
        ops.ddpm_step_edit(eps, x, SEEDS, 0, coef, image[:2], mask, ROWS[0])
    with pytest.raises(ValueError):
        ops.ddpm_step_edit(eps, x, SEEDS, 0, coef, image, mask[:, :, :5], ROWS[0])
    with pytest.raises(SisicError):
        ops.ddpm_step_edit(eps, x, SEEDS, 0, coef, image, mask, (float("nan"), 0.0, 1.0, 0.0))
    with pytest.raises(SisicError):                                           # the mask aliases the output
        ops.ddpm_step_edit(eps, x, SEEDS, 0, coef, image, mask, ROWS[0], out=image)


# ---- the loop -------------------------------------------------------------------------------------------------------------
RULES = [("ddpm", 0.0), ("ddim", 0.5), ("dpmsolver++", 0.0), ("sde-dpmsolver++", 0.0)]


@pytest.mark.parametrize("rule,eta", RULES)
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_mask_of_zeros_is_the_unedited_run_and_mask_of_ones_the_known_image(mode, rule, eta, eager, graph):
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    model = (eager if mode == "eager" else graph).models["NV"]
    sched, x_T, image = _scheduler(rule), _x_T(SEEDS), _image()
    plain = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta)
    zeros = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta,
                              edit=Edit(image, torch.zeros((B, 1) + CHW[1:], device=DEV)))
    assert zeros.steps_done == T and zeros.unet_passes == T
    assert torch.equal(zeros.trajectory, plain.trajectory) and torch.equal(zeros.latents, plain.latents)
    assert torch.equal(zeros.images, plain.images)
    ones = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), eta=eta,
                             edit=Edit(image, torch.ones((B, 1) + CHW[1:], device=DEV)))
    assert torch.equal(ones.latents, image) and torch.equal(ones.images, ops.denorm_u8(image))


LOOP_CASES = [("ddpm", 0.0, None), ("ddim", 0.0, None), ("ddim", 1.0, None), ("dpmsolver++", 0.0, None),
              ("sde-dpmsolver++", 0.0, None), ("ddpm", 0.0, JUMPS), ("ddim", 0.5, JUMPS)]


@pytest.mark.parametrize("rule,eta,jumps", LOOP_CASES)
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_fused_loop_equals_python_loop(mode, rule, eta, jumps, eager, graph):
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = (eager if mode == "eager" else graph).models["NV"]
    sched, x_T, image, mask = _scheduler(rule), _x_T(SEEDS), _image(), _soft_mask()
    schedule = resample_schedule(*jumps) if jumps else _plain(T)
    P = len(schedule)
    assert P == (20 if jumps else T)
    frames = _python_loop(model, sched, eta, x_T, SEEDS, image, mask, schedule)
    edit = Edit(image, mask, schedule if jumps else None)
    res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta, edit=edit)
    assert res.steps_done == P and res.unet_passes == P and res.timesteps == [int(sched.timesteps[i]) for i, _ in schedule]
    for p in range(P):
        assert torch.equal(res.trajectory[p], frames[p]), (p, schedule[p])
    assert torch.equal(res.latents, frames[-1]) and torch.equal(res.images, ops.denorm_u8(frames[-1]))
    keep = [0, 7, 8, P - 1]
    kept = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, save_indices=keep, eta=eta, edit=edit)
    assert kept.trajectory_steps == keep and torch.equal(kept.trajectory, frames[keep]) and torch.equal(kept.latents, frames[-1])
    if jumps:
        # the jump is in the frame after which it is taken: frame 7 is noisier than the same level reached without a jump
        again = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta,
                                  edit=Edit(image, mask, None))
        assert not torch.equal(again.trajectory[7], res.trajectory[7]) and torch.equal(again.trajectory[6], res.trajectory[6])


@pytest.fixture(scope="module")
def cond_sd():
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return synthetic_unet_state_dict(num_class_embeds=N_CLASS)


@pytest.fixture(scope="module")
def ceager(eager, cond_sd):
    eager.add_conditional_model(CLASSES, cond_sd).set_graph_mode(0)
    return eager


@pytest.fixture(scope="module")
def cgraph(graph, cond_sd):
    graph.add_conditional_model(CLASSES, cond_sd).set_graph_mode(1)
    return graph


@pytest.mark.parametrize("rule,eta,jumps", [("ddpm", 0.0, JUMPS), ("ddim", 0.5, None), ("sde-dpmsolver++", 0.0, None)])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_guided_fused_loop_equals_python_loop(mode, rule, eta, jumps, ceager, cgraph):
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import DeviceNoise, Edit, Guidance, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = (ceager if mode == "eager" else cgraph).models["MEL"]
    sched, x_T, image, mask = _scheduler(rule), _x_T(SEEDS), _image(), _soft_mask()
    schedule = resample_schedule(*jumps) if jumps else _plain(T)
    edit = Edit(image, mask, schedule if jumps else None)
    for w in (3.0, 1.0):
        frames = _python_loop(model, sched, eta, x_T, SEEDS, image, mask, schedule, LABELS, w)
        res = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, eta=eta, edit=edit,
                                guidance=Guidance(LABELS, NULL, w))
        assert res.steps_done == len(schedule)
        for p in range(len(schedule)):
            assert torch.equal(res.trajectory[p], frames[p]), (w, p, schedule[p])
        assert torch.equal(res.images, ops.denorm_u8(frames[-1]))


def test_graph_key(graph):
    """a captured edited step serves every image, mask and jump schedule at a shape; edited or not is part of the key; an
    unedited run is not touched by an edited one before it"""
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    lib = _lib.load()
    model = graph.models["NV"]
    sched, x_T = _scheduler("ddpm"), _x_T(SEEDS)
    builds = lambda: lib.sisic_unet_graph_builds(model.handle)      # noqa: E731
    before = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS))
    n0 = builds()
    first = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), edit=Edit(_image(), _soft_mask()))
    assert builds() == n0 + 1                                                          # unedited -> edited re-captures
    image2, mask2, schedule2 = _image(seed=99), _hard_mask(), resample_schedule(12, 3, 2)
    second = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, edit=Edit(image2, mask2, schedule2))
    assert builds() == n0 + 1 and second.steps_done == len(schedule2) == 21
    want = _python_loop(model, sched, 0.0, x_T, SEEDS, image2, mask2, schedule2)
    assert torch.equal(second.trajectory, want) and not torch.equal(second.latents, first.latents)
    third = run_sampling_loop(model, sched, x_T, DeviceNoise([5, 6, 7], step0=3), edit=Edit(_image(), _soft_mask()))
    assert builds() == n0 + 1 and not torch.equal(third.latents, first.latents)
    after = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS))
    assert builds() == n0 + 2                                                          # edited -> unedited re-captures
    assert torch.equal(after.latents, before.latents) and torch.equal(after.images, before.images)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_an_image_does_not_depend_on_its_batch(mode, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = (eager if mode == "eager" else graph).models["NV"]
    sched, x_T, image, mask, schedule = _scheduler("ddpm"), _x_T(SEEDS), _image(), _soft_mask(), resample_schedule(*JUMPS)
    whole = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), edit=Edit(image, mask, schedule))
    for b in (1, 2):
        alone = run_sampling_loop(model, sched, x_T[b:b + 1], DeviceNoise(SEEDS[b:b + 1]),
                                  edit=Edit(image[b:b + 1], mask[b:b + 1], schedule))
        assert torch.equal(alone.latents[0], whole.latents[b]) and torch.equal(alone.images[0], whole.images[b])


@pytest.mark.parametrize("rule,eta", [("ddpm", 0.0), ("ddim", 0.5)])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_a_run_cut_into_calls_equals_the_uncut_run(mode, rule, eta, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = (eager if mode == "eager" else graph).models["NV"]
    sched, x_T = _scheduler(rule), _x_T(SEEDS)
    edit = Edit(_image(), _soft_mask(), resample_schedule(*JUMPS))
    keep = [0, 6, 7, 13, 19]
    uncut = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, save_indices=keep, eta=eta, edit=edit)
    cut = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True, save_indices=keep, eta=eta, edit=edit,
                            max_call_steps=7)
    assert cut.steps_done == uncut.steps_done == 20 and cut.trajectory_steps == keep
    assert torch.equal(cut.trajectory, uncut.trajectory) and torch.equal(cut.latents, uncut.latents)
    assert torch.equal(cut.images, uncut.images)
    if rule == "ddpm":
        with pytest.raises(ValueError, match="DPM-Solver"):
            run_sampling_loop(model, _scheduler("dpmsolver++"), x_T, DeviceNoise(SEEDS), edit=Edit(_image(), _soft_mask()),
                              max_call_steps=7)
        with pytest.raises(ValueError):
            run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), edit=edit, max_call_steps=1001)


def test_loop_refusals(eager):
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = eager.models["NV"]
    sched, x_T, image, mask = _scheduler("ddpm"), _x_T(SEEDS), _image(), _soft_mask()
    z = torch.zeros((T - 1, B) + CHW, device=DEV)
    for noise in (z, None):
        with pytest.raises(ValueError, match="device"):
            run_sampling_loop(model, sched, x_T, noise, edit=Edit(image, mask))
    with pytest.raises(ValueError, match="DPM-Solver"):
        run_sampling_loop(model, _scheduler("dpmsolver++"), x_T, DeviceNoise(SEEDS), edit=Edit(image, mask, resample_schedule(*JUMPS)))
    with pytest.raises(ValueError):
        run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), edit=Edit(image[:2], mask))
    with pytest.raises(ValueError):
        run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), edit=Edit(image, mask[:, 0]))
    # the library's own refusal of a jump under DPM-Solver++ (SISIC_EINVAL), below the Python checks
    import ctypes as C
    lib = _lib.load()
    ds = _scheduler("dpmsolver++")
    ts, coef = ds.timesteps.to(torch.int64).contiguous(), ds.coefficient_table().contiguous()
    rows = torch.tensor([[0.5, 0.5, 1.0, 0.0]] * T)
    rows[3] = torch.tensor([0.5, 0.5, 0.8, 0.6])
    x, done = x_T.clone(), C.c_int(0)
    rc = lib.sisic_sample_frames_edit(model.handle, x.data_ptr(), B, 32, 32, T, C.cast(ts.data_ptr(), _lib.c_int64_p),
                                      C.cast(coef.data_ptr(), _lib.c_float_p), 1.0, _lib.RULE_DPMPP, 0, (C.c_uint64 * B)(*SEEDS), 0,
                                      None, 0, 1.0, image.data_ptr(), mask.data_ptr(), C.cast(rows.data_ptr(), _lib.c_float_p),
                                      None, None, None, None, C.byref(done), None)
    assert rc == _lib.SISIC_EINVAL and b"jump" in lib.sisic_last_error() and done.value == 0
    assert torch.equal(x, x_T)


# ---- image-to-image ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,eta,algo", [("ddpm", 0.0, "dpmsolver++"), ("ddim", 0.5, "dpmsolver++"),
                                           ("dpmsolver++", 0.0, "sde-dpmsolver++")])
@pytest.mark.parametrize("noise", ["host", "device"])
def test_image_to_image(noise, rule, eta, algo, eager):
    """strength 0.5 at T = 12: the last 6 grid entries from add_noise(init_image, x_T, their first timestep), no edit kernels: the
    result is run_sampling_loop handed that start and the sliced scheduler"""
    from synt_isic_amd.sampler import (DeviceNoise, _rule_tables, draw_noise, draw_x_T_device, noise_hash, run_sampling_loop)
    model = eager.models["NV"]
    image = _image()
    res = eager.generate_seeds("NV", SEEDS, T, size=CHW[1:], noise=noise, scheduler=rule, eta=eta, algorithm_type=algo,
                               init_image=image, strength=0.5, return_trajectory=True)
    sched = eager.create_scheduler(T, rule, 2, algo)
    sched.timesteps = sched.timesteps[6:]
    n_noise = int((_rule_tables(sched, eta, False)[0][:, 4] != 0).sum())
    if noise == "device":
        x_T, source = draw_x_T_device(SEEDS, CHW, torch.device(DEV)), DeviceNoise(SEEDS)
    else:
        x_T, z = draw_noise(SEEDS, n_noise, CHW)
        x_T, source = x_T.to(DEV), (z.to(DEV) if n_noise else None)
    t0 = int(sched.timesteps[0])
    start = sched.add_noise(image, x_T, torch.tensor([t0] * B))
    abar = sched.alphas_cumprod[t0]
    assert torch.equal(start, (abar ** 0.5).to(DEV) * image + ((1 - abar) ** 0.5).to(DEV) * x_T)
    want = run_sampling_loop(model, sched, start, source, return_trajectory=True, eta=eta)
    assert res.steps_done == 6 and res.unet_passes == 6 and res.strength == 0.5 and res.n_resample == 1
    assert res.timesteps == sched.timesteps.tolist() and len(res.timesteps) == 6
    assert torch.equal(res.trajectory, want.trajectory) and torch.equal(res.images, want.images)
    assert res.noise_hashes == [noise_hash(x_T[b:b + 1]) for b in range(B)]          # those of a plain run of the seeds
    assert res.noise_hashes == eager.generate_seeds("NV", SEEDS, 4, size=CHW[1:], noise=noise, scheduler=rule, eta=eta,
                                                    algorithm_type=algo).noise_hashes


# ---- the public interface -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_generate_seeds_inpaints(mode, eager, graph):
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import DeviceNoise, Edit, draw_x_T_device, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    s = eager if mode == "eager" else graph
    model = s.models["NV"]
    image, mask = _image(), _hard_mask()
    res = s.generate_seeds("NV", SEEDS, T, size=CHW[1:], noise="device", init_image=image, mask=mask, jump_length=4, n_resample=2,
                           return_trajectory=True)
    assert res.strength == 1.0 and res.n_resample == 2 and res.unet_passes == 20 and res.steps_done == 20
    assert len(res.timesteps) == 20 and res.seeds == SEEDS and len(res.noise_hashes) == B
    sched, x_T = s.create_scheduler(T), draw_x_T_device(SEEDS, CHW, torch.device(DEV))
    want = run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), return_trajectory=True,
                             edit=Edit(image, mask, resample_schedule(12, 4, 2)))
    assert torch.equal(res.trajectory, want.trajectory) and torch.equal(res.images, want.images)
    # the known region of the images holds under a hard mask, and the hole does not
    keep = mask[:, 0].bool().unsqueeze(-1).expand(B, 32, 32, 3)
    known = ops.denorm_u8(image)
    assert torch.equal(res.images[keep], known[keep]) and not torch.equal(res.images[~keep], known[~keep])
    # strength below 1 with a mask: the tail of the grid from the noised image; uint8 image and [H,W] mask, both broadcast
    u8 = ops.denorm_u8(image[:1])[0]
    part = s.generate_seeds("NV", SEEDS, T, size=CHW[1:], noise="device", scheduler="dpmsolver++", init_image=u8,
                            mask=mask[0, 0].cpu(), strength=0.5)
    assert part.steps_done == 6 and part.unet_passes == 6 and part.strength == 0.5
    back = ops.denorm_u8((u8.float() / 255.0 * 2.0 - 1.0).permute(2, 0, 1)[None].contiguous())[0]
    assert torch.equal(part.images[keep[:1].expand(B, 32, 32, 3)].view(B, -1), back[keep[0]].view(1, -1).expand(B, -1))


def test_generate_passes_the_keywords_and_refuses(eager):
    image, mask = _image(n=2), _hard_mask(n=2)
    imgs, traj = eager.generate(5, "NV", T, count=2, size=CHW[1:], noise="device", init_image=image, mask=mask, jump_length=4,
                                n_resample=2, return_trajectory=True)
    assert imgs.shape == (2, 32, 32, 3) and len(traj) == 20
    res = eager.generate_seeds("NV", [5, 6], T, size=CHW[1:], noise="device", init_image=image, mask=mask, jump_length=4,
                               n_resample=2)
    assert np.array_equal(imgs, res.images.cpu().numpy())
    plain = eager.generate_seeds("NV", [5, 6], T, size=CHW[1:], noise="device")
    assert plain.strength == 1.0 and plain.n_resample == 1 and plain.unet_passes == T
    common = dict(size=CHW[1:], init_image=image)
    for kw in (dict(noise="host", mask=mask),                                       # inpainting draws on the device
               dict(noise="device"),                                                # image-to-image at strength 1
               dict(noise="device", strength=0.01),                                 # no step left
               dict(noise="device", strength=0.0),
               dict(noise="device", mask=mask, scheduler="dpmsolver++", n_resample=2),
               dict(noise="device", strength=0.5, n_resample=2),                    # resampling without a mask
               dict(noise="device", mask=mask[:, :, :16]),
               dict(noise="device", mask=mask, init_image=image[:, :, :16])):
        with pytest.raises(ValueError):
            eager.generate_seeds("NV", [5, 6], T, **{**common, **kw})
    with pytest.raises(ValueError, match="init_image"):
        eager.generate_seeds("NV", [5, 6], T, size=CHW[1:], noise="device", mask=mask)
