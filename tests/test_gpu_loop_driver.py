"""The Python driver of the sampling loop (synt_isic_amd/sampler.py ``run_sampling_loop``) across its kinds of run: a run cut by a
``NoiseStream``'s segments or by ``max_call_steps`` against the same run in one call, the stop flag, every non-tensor field of
``SampleResult``, and the refusals.  Every comparison is ``torch.equal``.

Full UNet with synthetic weights (the conditional one of tests/test_gpu_inpaint.py), B = 2 at 3x32x32, T = 9: the grid is
[888, 777, ..., 111, 0], every step but the last adds noise, and a ``NoiseStream`` of 4-step segments cuts the run into calls of
4, 4 and 1 steps, the last of which runs the eager form in graph mode too (a replayed call has at least 4 steps)."""
import ctypes as C

import pytest
import torch

from test_gpu_clf_guide import clf  # noqa: F401  (the synthetic classifier, shared)
from test_gpu_device_noise import eager, graph  # noqa: F401  (the two graph-mode fixtures, shared)
from test_gpu_inpaint import _image, _scheduler, _soft_mask, ceager, cgraph, cond_sd  # noqa: F401  (conditional fixtures, shared)

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
B, T = 2, 9
SEEDS = [11, (1 << 33) + 2]
NULL, LABELS = 4, [0, 3]
GRID = [888, 777, 666, 555, 444, 333, 222, 111, 0]
KEEP = [1, 4, 8]
THRESHOLD = dict(thresholding=True, dynamic_thresholding_ratio=0.995, sample_max_value=2.0)
JUMPS = (9, 3, 2)                                  # (T, jump_length, n_resample): 15 passes
PASS_GRID = [888, 777, 666, 555, 444, 333, 555, 444, 333, 222, 111, 0, 222, 111, 0]


def _host_noise(n_noise=T - 1):
    from synt_isic_amd.sampler import draw_noise
    x_T, z = draw_noise(SEEDS, n_noise, CHW)
    return x_T.to(DEV), z.to(DEV)


def _stream(monkeypatch=None):
    """a NoiseStream of 4-step segments; with ``monkeypatch`` its uploads go over its copy stream and the two events per slot
    (uploads of this size ride the sampling stream otherwise).  Two NoiseStreams of this file do, in the first test: with the
    library's own stream of each of the file's two graph-mode handles that is four newly used streams, so the hardware queue a
    later file's stream lands on -- the positive control of tests/test_gpu_streams.py depends on it, with four queues per
    process -- stays the one it was before this file existed (tests/test_gpu_clf_bn.py keeps the same count)."""
    from synt_isic_amd.sampler import NoiseStream
    if monkeypatch is not None:
        monkeypatch.setenv("SISIC_NOISE_SAME_STREAM", "0")
    ns = NoiseStream(SEEDS, CHW, torch.device(DEV, torch.cuda.current_device()), 4)
    assert ns.same_stream == (monkeypatch is None)
    return ns


def _same_run(a, b):
    assert a.trajectory_steps == b.trajectory_steps and a.steps_done == b.steps_done
    assert (a.trajectory is None) == (b.trajectory is None)
    if a.trajectory is not None:
        assert torch.equal(a.trajectory, b.trajectory)
    assert torch.equal(a.latents, b.latents) and torch.equal(a.images, b.images)


# ---- 1. streamed = resident buffer -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_streamed_run_equals_the_resident_buffer(mode, ceager, cgraph, monkeypatch):
    from synt_isic_amd.sampler import Guidance, run_sampling_loop, segment_bounds
    model = (ceager if mode == "eager" else cgraph).models["MEL"]
    kw = dict(return_trajectory=True, save_indices=KEEP, guidance=Guidance(LABELS, NULL, 3.0), **THRESHOLD)
    x_T, z = _host_noise()
    whole = run_sampling_loop(model, _scheduler("ddpm", T), x_T, z, **kw)
    ns = _stream(monkeypatch)
    try:
        assert segment_bounds(T, ns.seg, B * 3 * 32 * 32) == [0, 4, 8, 9] and torch.equal(ns.x_T.to(DEV), x_T)
        cut = run_sampling_loop(model, _scheduler("ddpm", T), ns.x_T.to(DEV), ns, **kw)
        torch.cuda.synchronize()
    finally:
        ns.close()
    assert cut.steps_done == T and cut.trajectory_steps == KEEP and tuple(cut.trajectory.shape) == (3, B) + CHW
    assert not cut.cancelled and cut.thresholding == (0.995, 2.0)
    _same_run(cut, whole)


# ---- 2. a cut edited run = the uncut run -------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,eta", [("ddpm", 0.0), ("ddim", 0.5)])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_cut_edited_run_equals_the_uncut_run(mode, rule, eta, ceager, cgraph):
    from synt_isic_amd.sampler import DeviceNoise, Edit, Guidance, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = (ceager if mode == "eager" else cgraph).models["MEL"]
    schedule = resample_schedule(*JUMPS)
    keep = [0, 3, 4, 11, 14]
    kw = dict(return_trajectory=True, save_indices=keep, eta=eta, guidance=Guidance(LABELS, NULL, 3.0),
              edit=Edit(_image(B), _soft_mask(B), schedule), **THRESHOLD)
    x_T = _host_noise()[0]
    uncut = run_sampling_loop(model, _scheduler(rule, T), x_T, DeviceNoise(SEEDS), **kw)
    cut = run_sampling_loop(model, _scheduler(rule, T), x_T, DeviceNoise(SEEDS), max_call_steps=4, **kw)
    assert len(schedule) == 15
    for res in (uncut, cut):
        assert res.steps_done == res.unet_passes == len(schedule) and res.trajectory_steps == keep and not res.cancelled
        assert res.timesteps == PASS_GRID
    _same_run(cut, uncut)


# ---- 3. the stop flag, set before the first step ---------------------------------------------------------------------------
def _streamed(model, flag, **kw):
    from synt_isic_amd.sampler import run_sampling_loop
    ns = _stream()
    try:
        res = run_sampling_loop(model, _scheduler("ddpm", T), ns.x_T.to(DEV), ns, cancel_flag=flag, **kw)
        torch.cuda.synchronize()
    finally:
        ns.close()
    return res


def _edited_cut(model, flag, **kw):
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    return run_sampling_loop(model, _scheduler("ddpm", T), _host_noise()[0], DeviceNoise(SEEDS), cancel_flag=flag,
                             edit=Edit(_image(B), _soft_mask(B), resample_schedule(*JUMPS)), max_call_steps=4, **kw)


@pytest.mark.parametrize("kind", ["streamed", "edited"])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_stop_flag_set_before_the_first_step(mode, kind, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = (eager if mode == "eager" else graph).models["NV"]
    run = _streamed if kind == "streamed" else _edited_cut
    x_T, z = _host_noise()
    flag = C.c_int(1)
    stopped = run(model, flag, return_trajectory=True)
    assert stopped.cancelled and stopped.steps_done == 0
    assert int(stopped.images.count_nonzero()) == 0 and torch.equal(stopped.latents, x_T)
    flag.value = 0
    done = run(model, flag, return_trajectory=True)
    if kind == "streamed":
        want = run_sampling_loop(model, _scheduler("ddpm", T), x_T, z, return_trajectory=True)
    else:
        want = run_sampling_loop(model, _scheduler("ddpm", T), x_T, DeviceNoise(SEEDS), return_trajectory=True,
                                 edit=Edit(_image(B), _soft_mask(B), resample_schedule(*JUMPS)))
    assert not done.cancelled and done.steps_done == (T if kind == "streamed" else 15)
    _same_run(done, want)


# ---- 4. the record of a run --------------------------------------------------------------------------------------------------
def _record(res):
    return dict(scheduler=res.scheduler, eta=res.eta, timesteps=res.timesteps, trajectory_steps=res.trajectory_steps,
                steps_done=res.steps_done, unet_passes=res.unet_passes, prediction_type=res.prediction_type,
                classifier_scale=res.classifier_scale, classifier_passes=res.classifier_passes, thresholding=res.thresholding)


PLAIN = dict(scheduler="ddpm", eta=0.0, timesteps=GRID, trajectory_steps=[], steps_done=T, unet_passes=T,
             prediction_type="epsilon", classifier_scale=None, classifier_passes=0, thresholding=None)


def test_sample_result_fields_of_every_kind_of_run(eager, clf):  # noqa: F811
    from synt_isic_amd.sampler import ClassifierGuidance, DeviceNoise, Edit, run_sampling_loop
    from synt_isic_amd.scheduler import resample_schedule
    model = eager.models["NV"]
    x_T, z = _host_noise()
    # a resident buffer, every frame kept
    res = run_sampling_loop(model, _scheduler("ddpm", T), x_T, z, return_trajectory=True)
    assert _record(res) == dict(PLAIN, trajectory_steps=list(range(T))) and tuple(res.trajectory.shape) == (T, B) + CHW
    assert res.cancelled is False and res.seeds == [] and res.noise_hashes == [] and res.strength == 1.0 and res.n_resample == 1
    # a NoiseStream, DDIM at eta 0.5, thresholded, strided frames
    ns = _stream()
    try:
        res = run_sampling_loop(model, _scheduler("ddim", T), ns.x_T.to(DEV), ns, eta=0.5, return_trajectory=True,
                                save_indices=[8, 1, 4, 4], **THRESHOLD)
        torch.cuda.synchronize()
    finally:
        ns.close()
    assert _record(res) == dict(PLAIN, scheduler="ddim", eta=0.5, trajectory_steps=KEEP, thresholding=(0.995, 2.0))
    assert tuple(res.trajectory.shape) == (3, B) + CHW
    # device noise, no trajectory
    res = run_sampling_loop(model, _scheduler("ddpm", T), x_T, DeviceNoise(SEEDS))
    assert _record(res) == PLAIN and res.trajectory is None
    # an edited run with jumps, cut into calls
    res = run_sampling_loop(model, _scheduler("ddpm", T), x_T, DeviceNoise(SEEDS), return_trajectory=True, save_indices=[14, 2],
                            edit=Edit(_image(B), _soft_mask(B), resample_schedule(*JUMPS)), max_call_steps=4)
    assert _record(res) == dict(PLAIN, timesteps=PASS_GRID, trajectory_steps=[2, 14], steps_done=15, unet_passes=15)
    # classifier guidance
    res = run_sampling_loop(model, _scheduler("ddpm", T), x_T, DeviceNoise(SEEDS), classifier=ClassifierGuidance(clf, [0, 2], 2.5),
                            thresholding=False)
    assert _record(res) == dict(PLAIN, classifier_scale=2.5, classifier_passes=T)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(eager, clf):  # noqa: F811
    from synt_isic_amd.sampler import ClassifierGuidance, DeviceNoise, Edit, run_sampling_loop
    model = eager.models["NV"]
    x_T, z = _host_noise()
    sched = _scheduler("ddpm", T)
    edit = Edit(_image(B), _soft_mask(B))
    ns = _stream()
    try:
        with pytest.raises(ValueError, match="DPM-Solver\\+\\+ run is not cut into segments"):
            run_sampling_loop(model, _scheduler("sde-dpmsolver++", T), x_T, ns)
    finally:
        ns.close()
    for noise in (z, None):
        with pytest.raises(ValueError, match="inpainting draws on the device only"):
            run_sampling_loop(model, sched, x_T, noise, edit=edit)
        with pytest.raises(ValueError, match='classifier guidance requires noise="device"'):
            run_sampling_loop(model, sched, x_T, noise, classifier=ClassifierGuidance(clf, [0, 2], 2.0))
    for kw in (dict(), dict(edit=edit)):
        with pytest.raises(ValueError, match="DeviceNoise holds 3 seeds for a batch of 2"):
            run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS + [5]), **kw)
    with pytest.raises(ValueError, match="noise must be fp32"):
        run_sampling_loop(model, sched, x_T, z[:-1])
    with pytest.raises(ValueError, match="noise must be fp32"):
        run_sampling_loop(model, sched, x_T, z[:, :1])
    for bad in (0, 1001):
        with pytest.raises(ValueError, match="max_call_steps must lie in 1 .. 1000"):
            run_sampling_loop(model, sched, x_T, DeviceNoise(SEEDS), edit=edit, max_call_steps=bad)
    with pytest.raises(ValueError, match="a DPM-Solver\\+\\+ run of 9 steps is not cut into calls of 4"):
        run_sampling_loop(model, _scheduler("dpmsolver++", T), x_T, DeviceNoise(SEEDS), edit=edit, max_call_steps=4)
