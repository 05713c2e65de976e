"""Device-noise mode on the GPU: the step kernel's generator is the contract's Philox4x32-10 + Box-Muller
bit for bit (raw words) and within a measured bound (normals); the sampling loop adds exactly the noise sisic_noise_fill
writes; an image depends on its seed alone; the captured graph does not hold the seeds; and the public interface."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import philox_ref

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHW = (3, 32, 32)
FP32_ULP = 2.0 ** -23
# Largest |z_dev - z_ref| / max(1, sqrt(-2 ln u1)) over the 1 572 864 values of `stat_sample`, measured on an MI355X:
# 2.264e-7 = 1.90 fp32 ulp of 1.0.  The test asserts twice that, and the a-priori cap of 16 ulp.
MEASURED_NORMAL_ERR = 2.264e-7


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def stat_sample():
    """seeds 1000..1007, steps 0..15, 3072 blocks each: (device fp32 values, float64 restatement, radius), 1 572 864 long"""
    from synt_isic_amd import ops
    seeds, n = list(range(1000, 1008)), 3 * 64 * 64
    dev, ref, rad = [], [], []
    for step in range(16):
        dev.append(ops.noise_fill(seeds, n, step).cpu().numpy())
        zr = [philox_ref.noise_normals(s, step, 0, n) for s in seeds]
        ref.append(np.stack([z for z, _ in zr]))
        rad.append(np.stack([r for _, r in zr]))
    dev, ref, rad = (np.stack(a, axis=1).reshape(-1) for a in (dev, ref, rad))      # seed-major, as the issue counts them
    assert dev.size == 1572864
    return dev, ref, rad


@pytest.mark.parametrize("n_per_image", [3 * 32 * 32, 3 * 128 * 128])
def test_bits_equal_the_restatement_word_for_word(n_per_image):
    from synt_isic_amd import ops
    seeds = [0, 1, 0x7FFFFFFF, (1 << 32) + 5, 0xDEADBEEF12345678]
    for step in (0, 1, 999):
        for tag in (0, 1):
            got = _u32(ops.noise_bits(seeds, n_per_image, step, tag))
            assert got.shape == (len(seeds), n_per_image)
            for b, s in enumerate(seeds):
                want = philox_ref.noise_bits(s, step, tag, n_per_image)
                assert np.array_equal(got[b], want), (hex(s), step, tag, int(np.argmax(got[b] != want)))
    # the high key word, the step and the tag each reach the block
    a = _u32(ops.noise_bits([5, (1 << 32) + 5], 64, 0, 0))
    assert (a[0] != a[1]).mean() > 0.9
    assert (_u32(ops.noise_bits([5], 64, 1, 0)) != a[0]).mean() > 0.9 and (_u32(ops.noise_bits([5], 64, 0, 1)) != a[0]).mean() > 0.9


def test_image_sizes_that_are_not_whole_blocks():
    """n_per_image = 105: image b starts in the middle of a 16-byte line, the last block is cut.  Bits are whole blocks
    ([B, 108]); the normals are the first 105 of each image's 108, bit-equal to the vector path's."""
    from synt_isic_amd import ops
    seeds = [7, 8, (3 << 32) + 1]
    bits = _u32(ops.noise_bits(seeds, 105, 3, 0))
    assert bits.shape == (3, 108)
    for b, s in enumerate(seeds):
        assert np.array_equal(bits[b], philox_ref.noise_bits(s, 3, 0, 105))
    z105, z108 = ops.noise_fill(seeds, 105, 3), ops.noise_fill(seeds, 108, 3)
    assert z105.shape == (3, 105) and torch.equal(z105, z108[:, :105])
    for b, s in enumerate(seeds):
        ref, rad = philox_ref.noise_normals(s, 3, 0, 105)
        err = np.abs(z105[b].cpu().numpy().astype(np.float64) - ref) / np.maximum(1.0, rad)
        assert err.max() <= 16 * FP32_ULP
    # more images than one launch carries seeds for (64): image 70's row is its own seed's
    many = ops.noise_fill(list(range(100, 172)), 48, 2)
    assert torch.equal(many[70], ops.noise_fill([170], 48, 2)[0]) and torch.equal(many[3], ops.noise_fill([103], 48, 2)[0])


def test_normals_are_the_contracts(stat_sample):
    dev, ref, rad = stat_sample
    assert np.isfinite(dev).all()
    err = np.abs(dev.astype(np.float64) - ref.astype(np.float32).astype(np.float64)) / np.maximum(1.0, rad)
    worst = float(err.max())
    print(f"device normals vs float64 restatement rounded to fp32: max |dz| / max(1, radius) = {worst:.3e} "
          f"({worst / FP32_ULP:.2f} ulp), largest |z| {np.abs(dev).max():.3f}")
    assert MEASURED_NORMAL_ERR <= 16 * FP32_ULP            # a measurement above 16 ulp would mean something else is wrong
    assert worst <= 16 * FP32_ULP
    assert worst <= 2 * MEASURED_NORMAL_ERR


def test_distribution(stat_sample):
    from synt_isic_amd import ops
    dev = stat_sample[0].astype(np.float64)
    n = dev.size
    d, p = philox_ref.ks_pvalue_normal(dev)
    print(f"N = {n}: mean {dev.mean():.3e}, var {dev.var():.5f}, KS D {d:.3e} p {p:.3f}")
    assert p >= 1e-3
    assert abs(dev.mean()) < 4 / math.sqrt(n)
    assert abs(dev.var() - 1.0) < 4 * math.sqrt(2.0 / n)
    m = 3 * 64 * 64
    a = ops.noise_fill([42], m, 3)[0].cpu().numpy().astype(np.float64)
    b = ops.noise_fill([42], m, 4)[0].cpu().numpy().astype(np.float64)
    c = ops.noise_fill([43], m, 3)[0].cpu().numpy().astype(np.float64)
    r_step, r_seed = float(np.corrcoef(a, b)[0, 1]), float(np.corrcoef(a, c)[0, 1])
    print(f"correlation (42,3)x(42,4) {r_step:.4f}, (42,3)x(43,3) {r_seed:.4f}")
    assert abs(r_step) < 4 / math.sqrt(m) and abs(r_seed) < 4 / math.sqrt(m)


# ---- the loop ----------------------------------------------------------------------------------------------------------
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


def _sched(sampler, T, lo=0, hi=None):
    s = sampler.create_scheduler(T)
    s.timesteps = s.timesteps[lo:hi]
    return s


def _x_T(seeds, chw=CHW):
    return torch.stack([torch.randn(chw, generator=torch.Generator().manual_seed(1000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _filled_buffer(sched, seeds, chw, step0=0):
    """[n_noise,B,C,H,W]: the row of step i (sigma != 0) = sisic_noise_fill(step = step0 + i)"""
    from synt_isic_amd import ops
    coef = sched.coefficient_table()
    rows = [ops.noise_fill(seeds, int(np.prod(chw)), step0 + i).reshape((len(seeds),) + tuple(chw))
            for i in range(coef.shape[0]) if float(coef[i, 4]) != 0.0]
    return torch.stack(rows)


def _same(a, b):
    assert torch.equal(a.latents, b.latents) and torch.equal(a.images, b.images)
    if a.trajectory is not None or b.trajectory is not None:
        assert a.trajectory_steps == b.trajectory_steps and torch.equal(a.trajectory, b.trajectory)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_loop_adds_exactly_the_filled_noise(mode, eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    s = eager if mode == "eager" else graph
    model, seeds, T = s.models["NV"], [11, (1 << 33) + 2, 0], 12
    sched = _sched(s, T)
    x_T = _x_T(seeds)
    buf = _filled_buffer(sched, seeds, CHW)
    assert buf.shape[0] == T - 1
    want = run_sampling_loop(model, sched, x_T, buf, return_trajectory=True)
    got = run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), return_trajectory=True)
    assert got.steps_done == T and torch.isfinite(got.latents).all()
    _same(got, want)
    assert not torch.equal(got.latents, run_sampling_loop(model, sched, x_T, None).latents)      # noise was added
    # kept frames only, and a run that does not start at step index 0
    keep = [0, 5, T - 1]
    _same(run_sampling_loop(model, sched, x_T, DeviceNoise(seeds), return_trajectory=True, save_indices=keep),
          run_sampling_loop(model, sched, x_T, buf, return_trajectory=True, save_indices=keep))
    buf7 = _filled_buffer(sched, seeds, CHW, step0=7)
    _same(run_sampling_loop(model, sched, x_T, DeviceNoise(seeds, step0=7)), run_sampling_loop(model, sched, x_T, buf7))
    assert not torch.equal(buf7[0], buf[0])


@pytest.mark.parametrize("n_per_image,offset", [(3 * 32 * 32, 0), (3 * 32 * 32, 1), (105, 0), (105, 1)])
def test_single_step_aligned_unaligned_and_cut_blocks(n_per_image, offset):
    """sisic_ddpm_step_rng against sisic_ddpm_step fed with sisic_noise_fill's values: whole blocks on 16-byte lines (the
    float4 path), tensors four bytes off a line, and images of 105 floats whose blocks straddle two images (the
    element-by-element path, which picks one lane of a block per element).  Bit-equal; in place too."""
    from synt_isic_amd import ops
    seeds, step = [4, (1 << 35) + 6, 0x7FFFFFFF], 17
    n = len(seeds) * n_per_image
    g = torch.Generator().manual_seed(n + offset)
    view = lambda t: torch.cat([torch.zeros(offset), t, torch.zeros(4)]).to(DEV)[offset:offset + n]
    eps, x = view(torch.randn(n, generator=g)), view(torch.randn(n, generator=g))
    assert eps.data_ptr() % 16 == 4 * offset
    z = ops.noise_fill(seeds, n_per_image, step).reshape(-1)
    coef = (0.6, 0.8, 0.3, 0.69, 0.25)
    want = ops.ddpm_step(eps, x, z, coef, 1.0)
    got = ops.ddpm_step_rng(eps, x, seeds, step, coef, 1.0)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, ops.ddpm_step(eps, x, None, coef, 1.0))
    # sigma == 0 draws nothing
    quiet = coef[:4] + (0.0,)
    assert torch.equal(ops.ddpm_step_rng(eps, x, seeds, step, quiet, 1.0), ops.ddpm_step(eps, x, None, quiet, 1.0))
    inplace = x.clone() if offset == 0 else view(x.cpu())
    ops.ddpm_step_rng(eps, inplace, seeds, step, coef, 1.0, out=inplace)
    assert torch.equal(inplace, want)


def test_an_image_depends_on_its_seed_alone(eager, graph):
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    seeds, T = [5, (7 << 32) + 9, 0x7FFFFFFF], 10
    x_T = _x_T(seeds)
    me, mg = eager.models["NV"], graph.models["NV"]
    whole = run_sampling_loop(me, _sched(eager, T), x_T, DeviceNoise(seeds), return_trajectory=True)
    # each image alone
    for b, s in enumerate(seeds):
        one = run_sampling_loop(me, _sched(eager, T), x_T[b:b + 1], DeviceNoise([s]), return_trajectory=True)
        assert torch.equal(one.latents[0], whole.latents[b]) and torch.equal(one.images[0], whole.images[b])
        assert torch.equal(one.trajectory[:, 0], whole.trajectory[:, b])
    # the run cut into two calls
    for m, smp in ((me, eager), (mg, graph)):
        first = run_sampling_loop(m, _sched(smp, T, 0, 6), x_T, DeviceNoise(seeds))
        second = run_sampling_loop(m, _sched(smp, T, 6, None), first.latents, DeviceNoise(seeds, step0=6))
        assert torch.equal(second.latents, whole.latents) and torch.equal(second.images, whole.images)
        wrong = run_sampling_loop(m, _sched(smp, T, 6, None), first.latents, DeviceNoise(seeds))
        assert not torch.equal(wrong.latents, whole.latents)
    # graph and eager
    _same(run_sampling_loop(mg, _sched(graph, T), x_T, DeviceNoise(seeds), return_trajectory=True), whole)


def test_graph_is_reused_across_seeds(eager, graph):
    from synt_isic_amd import _lib
    from synt_isic_amd.sampler import DeviceNoise, run_sampling_loop
    lib, T = _lib.load(), 8
    mg, me = graph.models["NV"], eager.models["NV"]
    x_T = _x_T([1, 2])
    first = run_sampling_loop(mg, _sched(graph, T), x_T, DeviceNoise([31, 32]))
    builds = lib.sisic_unet_graph_builds(mg.handle)
    assert builds >= 1
    second = run_sampling_loop(mg, _sched(graph, T), x_T, DeviceNoise([(9 << 32) + 1, 77]))
    third = run_sampling_loop(mg, _sched(graph, T, 2, None), second.latents, DeviceNoise([31, 32], step0=2))
    assert lib.sisic_unet_graph_builds(mg.handle) == builds
    assert not torch.equal(first.latents, second.latents)
    assert torch.equal(second.latents, run_sampling_loop(me, _sched(eager, T), x_T, DeviceNoise([(9 << 32) + 1, 77])).latents)
    assert torch.equal(third.latents, run_sampling_loop(me, _sched(eager, T, 2, None), second.latents, DeviceNoise([31, 32], step0=2)).latents)
    # a buffer-noise call at the shape captures its own step (another kernel), and is still right afterwards
    sched = _sched(graph, T)
    buf = _filled_buffer(sched, [31, 32], CHW)
    assert torch.equal(run_sampling_loop(mg, sched, x_T, buf).latents, first.latents)
    assert torch.equal(run_sampling_loop(mg, _sched(graph, T), x_T, DeviceNoise([31, 32])).latents, first.latents)


# ---- public interface --------------------------------------------------------------------------------------------------
def _torch_device_x_T(seed, chw):
    g = torch.Generator(device=DEV)
    g.manual_seed(int(seed))
    return torch.randn((1,) + tuple(chw), device=DEV, generator=g)


def test_generate_seeds_in_device_mode(eager):
    from synt_isic_amd.sampler import image_seed, noise_hash
    seeds, T = [3, 0x7FFFFFFF, 12345], 9
    r1 = eager.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True, noise="device")
    r2 = eager.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True, noise="device")
    host = eager.generate_seeds("NV", seeds, T, (32, 32), noise="host")
    assert r1.steps_done == T and not r1.cancelled and r1.seeds == seeds
    assert r1.noise_hashes == [noise_hash(_torch_device_x_T(s, CHW)) for s in seeds]
    assert all(a != b for a, b in zip(r1.noise_hashes, host.noise_hashes))
    assert torch.isfinite(r1.latents).all() and torch.isfinite(r1.trajectory).all()
    assert r1.images.cpu().numpy().tobytes() == r2.images.cpu().numpy().tobytes()
    assert torch.equal(r1.latents, r2.latents) and torch.equal(r1.trajectory, r2.trajectory)
    assert torch.equal(host.images, eager.generate_seeds("NV", seeds, T, (32, 32)).images)       # the default is host mode
    assert not torch.equal(host.images, r1.images)
    # save_every_n keeps the same frames as in host mode, bit-equal to those of the all-frames run
    kept = eager.generate_seeds("NV", seeds, T, (32, 32), return_trajectory=True, save_every_n=4, noise="device")
    assert kept.trajectory_steps == [0, 4, 8] and torch.equal(kept.trajectory, r1.trajectory[[0, 4, 8]])
    # generate(): count images from consecutive seeds, or from the GUI's image_seed
    imgs, traj = eager.generate(40, "NV", T, count=3, size=(32, 32), noise="device")
    assert traj is None and imgs.shape == (3, 32, 32, 3)
    for i in range(3):
        one, _ = eager.generate(40 + i, "NV", T, size=(32, 32), noise="device")
        assert np.array_equal(one[0], imgs[i])
    imgs_b, _ = eager.generate(40, "NV", T, count=3, size=(32, 32), seed_is_base=True, noise="device")
    for i in range(3):
        one = eager.generate_seeds("NV", [image_seed(40, "NV", i)], T, (32, 32), noise="device")
        assert np.array_equal(one.images[0].cpu().numpy(), imgs_b[i])
    # a stop request ends a device-mode run like a host-mode one
    eager.request_stop()
    stopped = eager.generate_seeds("NV", seeds, T, (32, 32), noise="device")
    assert stopped.cancelled and stopped.steps_done < T
    assert eager.generate_images("NV", seeds, T, size=(32, 32), noise="device").steps_done == T     # clears the flag


def test_module_level_generate_passes_the_mode_through(synthetic_sd):
    from synt_isic_amd import sampler as S
    old = S._default_sampler
    try:
        S._default_sampler = S.Sampler(DEV)
        S._default_sampler.add_model("NV", synthetic_sd)
        a, _ = S.generate(6, "NV", 4, size=(32, 32), noise="device")
        b = S._default_sampler.generate_seeds("NV", [6], 4, (32, 32), noise="device")
        assert np.array_equal(a, b.images.cpu().numpy())
        with pytest.raises(ValueError):
            S.generate(6, "NV", 4, size=(32, 32), noise="philox")
    finally:
        S._default_sampler = old


def test_T1000_chain_in_device_mode_stays_finite_and_clipped(synthetic_sd):
    """64x64, T=1000, B=2 (set up like test_T1000_chain_at_the_headline_resolutions; device mode has no golden file):
    every kept frame is finite and, clip_sample being on, the last step returns its clipped x0."""
    from synt_isic_amd.sampler import Sampler
    s = Sampler(DEV)
    s.add_model("NV", synthetic_sd)
    assert s.create_scheduler(1000).config.clip_sample
    res = s.generate_seeds("NV", [0, 5], T=1000, size=(64, 64), return_trajectory=True, save_every_n=100, noise="device")
    assert res.steps_done == 1000 and res.timesteps[0] == 999 and res.timesteps[-1] == 0
    assert torch.isfinite(res.trajectory).all() and torch.isfinite(res.latents).all()
    assert float(res.latents.abs().max()) <= 1.0
    assert not torch.equal(res.latents[0], res.latents[1])
    again = s.generate_seeds("NV", [5], T=1000, size=(64, 64), noise="device")
    assert torch.equal(again.latents[0], res.latents[1])


def test_shards_concatenate_to_the_unsharded_run(eager):
    """test_config3_eight_shards_of_64_equal_one_run_of_512 in device mode at a small size: 16 seeds in 4 shards"""
    from synt_isic_amd.dist import shard_seeds
    seeds = list(range(200, 216))
    whole = eager.generate_seeds("NV", seeds, T=3, size=(32, 32), noise="device")
    assert whole.images.shape == (16, 32, 32, 3) and whole.steps_done == 3
    parts = [eager.generate_seeds("NV", shard_seeds(seeds, 4, r), T=3, size=(32, 32), noise="device") for r in range(4)]
    assert all(p.images.shape[0] == 4 for p in parts)
    assert torch.equal(torch.cat([p.images for p in parts]), whole.images)
    assert torch.equal(torch.cat([p.latents for p in parts]), whole.latents)
    assert [h for p in parts for h in p.noise_hashes] == whole.noise_hashes
