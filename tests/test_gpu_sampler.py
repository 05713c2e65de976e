"""The T-step loop (sisic_sample) against the oracle, the committed trajectory fixture, and -- at
BASELINE.json's full batch size -- size-independent properties (determinism, batch/shard independence).

Stated tolerances: T=50 trajectory end <= 2e-3 max-abs in [-1,1]; uint8 images within
+-1 LSB on >= 99 % of pixels; integer pieces bit-exact.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def sampler(synthetic_sd):
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV)
    s.add_model("NV", synthetic_sd)
    return s


def test_config1_T50_seed0_matches_golden(sampler, golden_dir):
    """BASELINE config 1: 1 image, 3x64x64, T=50, seed=0, class NV."""
    g = np.load(os.path.join(golden_dir, "sample_T50_seed0_64.npz"))
    res = sampler.generate_seeds("NV", [0], T=50, size=(64, 64), return_trajectory=True)
    assert res.timesteps == list(range(980, -1, -20))               # integer grid, bit-exact
    assert res.noise_hashes == ["ce480957dd270985"]                 # image_generator.py:383-389 anchor
    assert res.steps_done == 50
    traj = res.trajectory.cpu().numpy()                             # [50,1,3,64,64]
    for i, step in enumerate(g["steps"]):
        err = np.abs(traj[int(step)] - g["traj"][i]).max()
        assert err <= 2e-3, f"step {step}: {err:.3e}"
    assert np.abs(res.latents.cpu().numpy() - g["final"]).max() <= 2e-3
    img = res.images.cpu().numpy()
    assert img.shape == (1, 64, 64, 3) and img.dtype == np.uint8
    assert np.mean(np.abs(img.astype(int) - g["image"].astype(int)) <= 1) >= 0.99
    # the final image is the de-normalisation of the final latents, bit-exact
    from oracle import sampler as osampler
    assert np.array_equal(img, osampler.denormalize_to_uint8(res.latents.cpu()))


def test_generate_call_surface(sampler):
    images, traj = sampler.generate(0, "NV", 6, count=2, size=(32, 32), return_trajectory=True)
    assert images.shape == (2, 32, 32, 3) and images.dtype == np.uint8
    assert isinstance(traj, list) and len(traj) == 6 and traj[0].shape == (2, 3, 32, 32)
    assert float(traj[0].abs().max()) < 10
    images2, none = sampler.generate(0, "NV", 6, count=2, size=(32, 32))
    assert none is None and np.array_equal(images, images2)
    # base-seed semantics of the GUI path: seed_i = (base + md5 offset + i) & 0x7fffffff
    from synt_isic_amd.sampler import image_seed
    a, _ = sampler.generate(42, "NV", 4, count=1, size=(32, 32), seed_is_base=True)
    b = sampler.generate_seeds("NV", [image_seed(42, "NV", 0)], 4, (32, 32)).images.cpu().numpy()
    assert np.array_equal(a, b)
    with pytest.raises(KeyError):
        sampler.generate(0, "MEL", 4)


def test_loop_equals_reference_style_python_loop(sampler, synthetic_sd):
    """The literal loop of image_generator.py:395-403 over the two drop-in objects gives the same
    latents as the fused in-library loop, and both match the oracle."""
    from oracle import sampler as osampler
    from synt_isic_amd.sampler import draw_noise
    model = sampler.models["NV"]
    scheduler = sampler.create_scheduler(8)
    x_T, z = draw_noise([3, 4], 7, (3, 32, 32))
    latents = x_T.to(DEV)
    zi = 0
    with torch.no_grad():
        for step_idx, t in enumerate(scheduler.timesteps):
            noise_pred = model(latents, t).sample
            vn = None
            if int(t) > 0:
                vn = z[zi].to(DEV); zi += 1
            latents = scheduler.step(noise_pred, t, latents, variance_noise=vn).prev_sample
    res = sampler.generate_seeds("NV", [3, 4], T=8, size=(32, 32))
    assert torch.equal(res.latents, latents)
    _, ref, _ = osampler.sample(synthetic_sd, [3, 4], 8, (32, 32))
    assert (latents.cpu() - ref).abs().max().item() <= 1e-3


def test_linear_schedule_variant(sampler, synthetic_sd):
    """diffusion_generator.py:123-144: beta_schedule='linear', all 1000 train steps (truncated here)."""
    from oracle import ddpm as oddpm, unet as ounet
    from synt_isic_amd.scheduler import HipDDPMScheduler
    model = sampler.models["NV"]
    s = HipDDPMScheduler(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear")
    o = oddpm.DDPMSchedulerOracle(beta_schedule="linear")
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 3, 32, 32, generator=g)
    xr = x.clone()
    xd = x.to(DEV)
    for t in list(s.timesteps)[:4]:
        z = torch.randn(1, 3, 32, 32, generator=g)
        xd = s.step(model(xd, t).sample, t, xd, variance_noise=z.to(DEV)).prev_sample
        with torch.no_grad():
            xr = o.step(ounet.unet_forward(synthetic_sd, xr, int(t)), int(t), xr, noise=z)
    assert (xd.cpu() - xr).abs().max().item() <= 1e-3


def test_batch_and_shard_independence_small(sampler):
    """An image's chain depends only on its own seed: any batch composition gives bit-identical results
    (this is what makes the 8-GPU sharding of BASELINE config 3 equal to the single-GPU run)."""
    seeds = [0, 5, 9, 11]
    full = sampler.generate_seeds("NV", seeds, T=10, size=(32, 32))
    for i, s in enumerate(seeds):
        one = sampler.generate_seeds("NV", [s], T=10, size=(32, 32))
        assert torch.equal(one.latents[0], full.latents[i])
        assert torch.equal(one.images[0], full.images[i])
    a = sampler.generate_seeds("NV", seeds[:2], T=10, size=(32, 32))
    b = sampler.generate_seeds("NV", seeds[2:], T=10, size=(32, 32))
    assert torch.equal(torch.cat([a.images, b.images]), full.images)


def test_full_batch_properties(sampler):
    """BASELINE config 2 shape (batch=64, 3x64x64), shortened to 3 steps: determinism, batch independence
    and the clip invariant |x0_hat| <= 1 => latents stay bounded."""
    from synt_isic_amd.sampler import draw_noise, run_sampling_loop
    seeds = list(range(64))
    sched = sampler.create_scheduler(1000)
    sched.timesteps = sched.timesteps[:3]                # 999, 998, 997 with the T=1000 spacing
    x_T, z = draw_noise(seeds, 3, (3, 64, 64))
    model = sampler.models["NV"]
    r1 = run_sampling_loop(model, sched, x_T.to(DEV), z.to(DEV), return_trajectory=True)
    r2 = run_sampling_loop(model, sched, x_T.to(DEV), z.to(DEV))
    assert r1.steps_done == 3 and torch.equal(r1.latents, r2.latents) and torch.equal(r1.images, r2.images)
    assert torch.equal(r1.trajectory[-1], r1.latents)
    assert torch.isfinite(r1.latents).all() and float(r1.latents.abs().max()) < 8.0
    k = 17
    rk = run_sampling_loop(model, sched, x_T[k:k + 1].to(DEV), z[:, k:k + 1].contiguous().to(DEV))
    assert torch.equal(rk.latents[0], r1.latents[k])
    # x_T itself is untouched by the call (the loop works on a copy)
    assert torch.equal(x_T, draw_noise(seeds, 0, (3, 64, 64))[0])


def test_cancel_flag_stops_the_loop(sampler):
    from synt_isic_amd.sampler import draw_noise, run_sampling_loop
    sched = sampler.create_scheduler(50)
    x_T, z = draw_noise([1], 49, (3, 32, 32))
    flag = ctypes.c_int(1)                                 # stop requested before the first step
    res = run_sampling_loop(sampler.models["NV"], sched, x_T.to(DEV), z.to(DEV), cancel_flag=flag)
    assert res.steps_done == 0 and res.cancelled
    assert torch.equal(res.latents.cpu(), x_T)            # nothing was applied
    assert int(res.images.max()) == 0                      # a cancelled run hands back zeros, never uninitialised pixels
    flag.value = 0
    res = run_sampling_loop(sampler.models["NV"], sched, x_T.to(DEV), z.to(DEV), cancel_flag=flag)
    assert res.steps_done == 50 and not res.cancelled


def test_stop_then_generate_then_generate(sampler):
    """request_stop() -> generate -> generate (image_generator.py:567 clears stop_requested at the start of every
    generate_images): a stale stop flag must not cancel later runs, and a cancelled run must not return pixels."""
    base, _ = sampler.generate(5, "NV", 4, count=2, size=(32, 32))
    sampler.request_stop()                                   # nothing is running: the flag is stale when generate starts
    images, traj = sampler.generate(5, "NV", 4, count=2, size=(32, 32), return_trajectory=True)
    assert images is not None and np.array_equal(images, base) and len(traj) == 4
    again, _ = sampler.generate(5, "NV", 4, count=2, size=(32, 32))
    assert np.array_equal(again, base)
    # a stop that is pending inside the run (generate_seeds keeps the flag it is given): cancelled, zero-filled, flagged
    sampler.cancel.value = 1
    res = sampler.generate_seeds("NV", [5, 6], 4, (32, 32))
    assert res.cancelled and res.steps_done == 0 and int(res.images.max()) == 0
    sampler.cancel.value = 0


def test_noise_shape_is_validated(sampler):
    from synt_isic_amd.sampler import draw_noise, run_sampling_loop
    sched = sampler.create_scheduler(4)
    x_T, z = draw_noise([1], 2, (3, 32, 32))               # needs 3 noise tensors for T=4
    with pytest.raises(ValueError, match="noise"):
        run_sampling_loop(sampler.models["NV"], sched, x_T.to(DEV), z.to(DEV))


def test_smoke_entry():
    import __graft_entry__
    __graft_entry__.smoke()


def test_streamed_noise_equals_materialised_noise(sampler):
    """generate_seeds draws z on worker threads segment by segment while the GPU samples (NoiseStream); the values and
    therefore every latent of the trajectory equal the all-up-front path, whatever the segment length."""
    from synt_isic_amd.sampler import draw_noise, run_sampling_loop
    seeds, T = [7, 8, 9], 11
    sched = sampler.create_scheduler(T)
    x_T, z = draw_noise(seeds, T - 1, (3, 32, 32))
    ref = run_sampling_loop(sampler.models["NV"], sched, x_T.to(DEV), z.to(DEV), return_trajectory=True)
    old = sampler.noise_segment_steps
    try:
        for seg in (1, 3, 4, 11, 64):
            sampler.noise_segment_steps = seg
            res = sampler.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True)
            assert res.steps_done == T
            assert torch.equal(res.trajectory, ref.trajectory), f"segment length {seg}"
            assert torch.equal(res.images, ref.images)
    finally:
        sampler.noise_segment_steps = old
    # the host-side stream alone: bit-identical to draw_noise (CPU values, before any upload)
    from synt_isic_amd.sampler import NoiseStream
    ns = NoiseStream(seeds, (3, 32, 32), torch.device(DEV), segment_steps=4, workers=2)
    try:
        assert torch.equal(ns.x_T, x_T)
        got = []
        for k, n in enumerate((4, 4, 2)):
            ns.prefetch(k & 1, n)
            got.append(ns.acquire(k & 1, n).cpu().clone())
            ns.release(k & 1)
        assert torch.equal(torch.cat(got), z)
    finally:
        ns.close()


def test_T1000_chain_matches_golden(sampler, golden_dir):
    """The whole 1000-step chain of one 3x32x32 image against the oracle fixture: error accumulation over T=1000.
    Stated tolerance: <= 1e-2 in [-1,1] at the end, uint8 within 1 LSB on >= 99 % of pixels."""
    g = np.load(os.path.join(golden_dir, "sample_T1000_seed3_32.npz"))
    res = sampler.generate_seeds("NV", [3], T=1000, size=(32, 32), return_trajectory=True)
    assert res.steps_done == 1000 and res.timesteps[0] == 999 and res.timesteps[-1] == 0
    traj = res.trajectory.cpu().numpy()
    for i, step in enumerate(g["steps"]):
        err = np.abs(traj[int(step)] - g["traj"][i]).max()
        assert err <= 1e-2, f"step {step}: {err:.3e}"
    assert np.abs(res.latents.cpu().numpy() - g["final"]).max() <= 1e-2
    img = res.images.cpu().numpy()
    assert np.mean(np.abs(img.astype(int) - g["image"].astype(int)) <= 1) >= 0.99


def test_generate_postprocess_and_pth_round_trip(sampler, synthetic_sd, tmp_path):
    """a checkpoint written as the reference's `unet_{CLASS}_best.pth` (torch.save of the
    diffusers-keyed state dict) loads through torch.load + load_state_dict, and generate(postprocess=True) applies the
    class colour statistics to the same images (image_generator.py:449-452, 502-545)."""
    from synt_isic_amd.sampler import Sampler, apply_color_statistics
    path = tmp_path / "unet_NV_best.pth"
    torch.save(synthetic_sd, path)
    s2 = Sampler(DEV)
    s2.add_model("NV", torch.load(path, map_location="cpu"))               # model_manager.py:138-139
    a, _ = sampler.generate(5, "NV", 4, count=2, size=(32, 32))
    b, _ = s2.generate(5, "NV", 4, count=2, size=(32, 32))
    assert np.array_equal(a, b)
    stats = {"NV": {"rgb": {"mean": [190.0, 140.0, 120.0], "std": [35.0, 40.0, 45.0]}}}
    s2.color_statistics = stats
    c, _ = s2.generate(5, "NV", 4, count=2, size=(32, 32), postprocess=True)
    assert np.array_equal(c, apply_color_statistics(a, stats["NV"])) and not np.array_equal(c, a)
    d, _ = s2.generate(5, "NV", 4, count=2, size=(32, 32), postprocess=False)
    assert np.array_equal(d, a)


def test_graph_replayed_loop_is_bit_identical(synthetic_sd):
    """sisic_sample with one captured step replayed T-1 times (hipGraph) against the launch-by-launch loop: same kernels,
    same bits -- final latents, uint8 images and every trajectory frame -- for a run, a second run that reuses the cached
    graph with other seeds, the segmented noise stream (several sisic_sample calls per run) and a cancelled run."""
    from synt_isic_amd.sampler import Sampler
    plain, graph = Sampler(DEV), Sampler(DEV)
    plain.add_model("NV", synthetic_sd)
    graph.add_model("NV", synthetic_sd).set_graph_mode(1)
    plain.models["NV"].set_graph_mode(0)
    for seeds, T in (([0, 1], 12), ([7, 8], 12), ([3], 9)):
        a = plain.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True)
        b = graph.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True)
        assert b.steps_done == T
        assert torch.equal(a.latents, b.latents) and torch.equal(a.images, b.images) and torch.equal(a.trajectory, b.trajectory)
    graph.noise_segment_steps = plain.noise_segment_steps = 5            # three sisic_sample calls per run
    a = plain.generate_seeds("NV", [11, 12, 13], 14, (32, 32))
    b = graph.generate_seeds("NV", [11, 12, 13], 14, (32, 32))
    assert torch.equal(a.latents, b.latents) and torch.equal(a.images, b.images)
    # latency mode switches the graph on by itself; another resolution rebuilds it
    lat = Sampler(DEV, latency_mode=True)
    lat.add_model("NV", synthetic_sd)
    r1 = lat.generate_seeds("NV", [5], 8, (64, 64))
    r2 = lat.generate_seeds("NV", [5], 8, (64, 64))
    r3 = lat.generate_seeds("NV", [5], 8, (32, 32))
    assert torch.equal(r1.latents, r2.latents) and r3.latents.shape[-1] == 32 and torch.isfinite(r3.latents).all()
    # a longer run after a shorter one re-allocates the time-embedding table the captured step reads: the graph is rebuilt
    r4 = lat.generate_seeds("NV", [5], 40, (32, 32))
    p4 = Sampler(DEV, latency_mode=True)
    p4.add_model("NV", synthetic_sd).set_graph_mode(0)
    assert torch.equal(r4.latents, p4.generate_seeds("NV", [5], 40, (32, 32)).latents)
    lat.cancel.value = 1
    rc = lat.generate_seeds("NV", [5], 8, (32, 32))
    assert rc.cancelled and rc.steps_done == 0
    lat.cancel.value = 0


def test_graph_is_rebuilt_after_load_state_dict(synthetic_sd):
    """load_state_dict on a handle that has sampled in graph mode frees and re-allocates every packed filter the
    captured step points at.  The next run at the same shape must rebuild the graph: bit-equal to the launch-by-launch
    loop over the NEW weights (and different from the old weights' result)."""
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.weights import synthetic_unet_state_dict
    other = synthetic_unet_state_dict(4321)
    graph, plain = Sampler(DEV), Sampler(DEV)
    graph.add_model("NV", synthetic_sd).set_graph_mode(1)
    plain.add_model("NV", other).set_graph_mode(0)
    a = graph.generate_seeds("NV", [0, 1], 10, (32, 32))
    graph.models["NV"].load_state_dict(other)
    b = graph.generate_seeds("NV", [0, 1], 10, (32, 32))
    c = plain.generate_seeds("NV", [0, 1], 10, (32, 32))
    assert torch.equal(b.latents, c.latents) and torch.equal(b.images, c.images)
    assert not torch.equal(a.latents, b.latents)


def test_second_call_at_the_same_shape_reuses_the_graph(synthetic_sd):
    """the reference calls the sampler once per image (image_generator.py:369-403); the captured step
    is instantiated on the first call at a shape and only replayed afterwards (sisic_unet_graph_builds counts builds)."""
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV, latency_mode=True)
    m = s.add_model("NV", synthetic_sd)
    lib = _lib.load()
    s.generate_seeds("NV", [0], 8, (32, 32))
    n1 = lib.sisic_unet_graph_builds(m.handle)
    for seed in (1, 2, 3):
        s.generate_seeds("NV", [seed], 8, (32, 32))
    assert n1 == 1 and lib.sisic_unet_graph_builds(m.handle) == 1
    s.generate_seeds("NV", [0], 8, (64, 64))
    assert lib.sisic_unet_graph_builds(m.handle) == 2


@pytest.mark.parametrize("name,size", [("sample_T1000_seed0_64.npz", 64), ("sample_T1000_seed5_128.npz", 128)])
def test_T1000_chain_at_the_headline_resolutions(sampler, golden_dir, name, size):
    """the full 1000-step chain of one image at BASELINE config 2's own resolution (3x64x64) and at config 4's
    (3x128x128, attention over 1024 and 256 tokens) against the oracle fixtures (tests/golden/make_golden.py --long).
    Stated tolerance: <= 1e-2 in [-1,1] at every kept frame and at the end; uint8 within 1 LSB on
    >= 99 % of the pixels."""
    g = np.load(os.path.join(golden_dir, name))
    seed = int(g["seed"])
    res = sampler.generate_seeds("NV", [seed], T=1000, size=(size, size), return_trajectory=True)
    assert res.steps_done == 1000 and res.timesteps[0] == 999 and res.timesteps[-1] == 0
    traj = res.trajectory.cpu().numpy()
    worst = 0.0
    for i, step in enumerate(g["steps"]):
        err = np.abs(traj[int(step)] - g["traj"][i]).max()
        worst = max(worst, float(err))
        assert err <= 1e-2, f"step {step}: {err:.3e}"
    end = float(np.abs(res.latents.cpu().numpy() - g["final"]).max())
    assert end <= 1e-2, end
    # regression guard far inside the stated tolerance: the chain is contractive (x0 is clipped every step) and the library
    # measures 1e-5 at both resolutions (profiles/r03/test_errors.txt)
    assert max(worst, end) <= 5e-4, (worst, end)
    img = res.images.cpu().numpy()
    frac = float(np.mean(np.abs(img.astype(int) - g["image"].astype(int)) <= 1))
    if os.environ.get("SISIC_TEST_ERRLOG"):
        with open(os.environ["SISIC_TEST_ERRLOG"], "a") as f:
            f.write(f"{max(worst, end):.3e}\t1.0e-02\tT=1000 chain {size}x{size} seed {seed}: worst kept frame / end; uint8 within 1 LSB {frac:.5f}\n")
    assert frac >= 0.99


def test_trajectory_stride_keeps_the_same_frames(synthetic_sd):
    """VERDICT r03 item 7 (xai/XAI.py:751-757 `save_indices`): with save_every_n the trajectory holds every n-th step and the
    last one only, and those frames are bit-equal to the same frames of the all-frames run -- launch-by-launch loop,
    graph-replayed loop, segmented noise stream and the generate() call surface."""
    from synt_isic_amd.sampler import Sampler, draw_noise, run_sampling_loop, trajectory_save_indices
    plain, graph = Sampler(DEV), Sampler(DEV)
    plain.add_model("NV", synthetic_sd).set_graph_mode(0)
    graph.add_model("NV", synthetic_sd).set_graph_mode(1)
    seeds, T = [3, 4], 13
    full = plain.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True)
    assert full.trajectory.shape[0] == T and full.trajectory_steps == list(range(T))
    for every in (1, 4, 5, 12, 13):
        keep = trajectory_save_indices(full.timesteps, every)
        for s in (plain, graph):
            for seg in (64, 5):                                      # one sisic_sample_frames call, or three
                s.noise_segment_steps = seg
                r = s.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True, save_every_n=every)
                assert r.trajectory_steps == keep and r.trajectory.shape == (len(keep), 2, 3, 32, 32)
                assert torch.equal(r.trajectory, full.trajectory[keep]), (every, seg)
                assert torch.equal(r.latents, full.latents) and torch.equal(r.images, full.images)
    plain.noise_segment_steps = graph.noise_segment_steps = 64
    keep = trajectory_save_indices(full.timesteps, 4)
    assert keep == [0, 4, 8, 12]
    # resident noise + explicit indices (run_sampling_loop), and a list that is not sorted
    sched = plain.create_scheduler(T)
    x_T, z = draw_noise(seeds, T - 1, (3, 32, 32))
    r = run_sampling_loop(plain.models["NV"], sched, x_T.to(DEV), z.to(DEV), return_trajectory=True, save_indices=[12, 2, 7, 2])
    assert r.trajectory_steps == [2, 7, 12] and torch.equal(r.trajectory, full.trajectory[[2, 7, 12]])
    with pytest.raises(ValueError):
        run_sampling_loop(plain.models["NV"], sched, x_T.to(DEV), z.to(DEV), return_trajectory=True, save_indices=[13])
    # the call surface: a list of the kept frames, their step indices beside it
    images, traj = plain.generate(3, "NV", T, count=2, size=(32, 32), return_trajectory=True, save_every_n=4)
    assert len(traj) == 4 and plain.last_trajectory_steps == [0, 4, 8, 12]
    assert torch.equal(traj[-1], full.latents) and np.array_equal(images, full.images.cpu().numpy())
    plain.close()
    graph.close()
