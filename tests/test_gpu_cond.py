"""The class-conditional UNet and classifier-free guidance on the GPU: forward and gradients against the restatement
(tests/cond_ref.py), the fused training step against the spelled-out one, the guidance combine bit for bit, the in-library
guided loop against a Python loop over the drop-in objects, the captured step's key, the guided chain against the CPU
restatement, the refusals and the public interface.

Real UNet configuration, N = 5 embedding rows (four classes and the null label), B = 3 at 3x32x32 unless a test says otherwise.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cond_ref
import dpmpp_ref
from test_gpu_device_noise import eager, graph  # noqa: F401  (the two graph-mode fixtures, shared)
from test_gpu_train import GRAD_REL_MEDIAN, GRAD_REL_WORST, _grad_errors
from test_gpu_unet import FWD_TOL

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 5
NULL = N - 1
CLASSES = ("MEL", "BCC", "AKIEC", "BKL")        # labels 0 .. 3 ("NV" is the shared fixtures' unconditional model)
CHW = (3, 32, 32)
B, T = 3, 12
LABELS = [0, 3, 2]
# 1e-3 max-abs is the project's tolerance for a chain against the CPU oracle on the "leading" grid (test_chain_against_the_oracle
# of tests/test_gpu_dpmpp.py and tests/test_gpu_ddim.py, which run T = 8 with two seeds; this chain runs T = 12 with three, on the
# same grid and image size), times |w| + |1 - w| = 5 at w = 3: how far the combine can amplify the error of its two forwards
CHAIN_TOL = 1e-3 * 5


@pytest.fixture(scope="module")
def cond_sd():
    from synt_isic_amd.weights import synthetic_unet_state_dict
    return synthetic_unet_state_dict(num_class_embeds=N)


def _new_model(sd, n=N):
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel(num_class_embeds=n)
    m.load_state_dict(sd)
    return m.to(DEV)


@pytest.fixture(scope="module")
def ceager(eager, cond_sd):
    eager.add_conditional_model(CLASSES, cond_sd).set_graph_mode(0)
    return eager


@pytest.fixture(scope="module")
def cgraph(graph, cond_sd):
    graph.add_conditional_model(CLASSES, cond_sd).set_graph_mode(1)
    return graph


@pytest.fixture(scope="module")
def cmodel(ceager):
    return ceager.models["MEL"]


# ---- 1. forward --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd_case(cond_sd):
    x = torch.randn((B,) + CHW, generator=torch.Generator().manual_seed(91))
    cases = []
    for t in ([37, 912, 500], [500] * 3):
        with torch.no_grad():
            cases.append((torch.tensor(t), cond_ref.unet_forward(cond_sd, x, torch.tensor(t), [0, 4, 2])))
    return x, cases


def test_forward_matches_the_restatement(cmodel, fwd_case):
    """labels [0, 4, 2] under mixed timesteps, and under uniform ones: there one embedding row must NOT serve every sample"""
    x, cases = fwd_case
    for t, ref in cases:
        out = cmodel(x.to(DEV), t, class_labels=torch.tensor([0, 4, 2])).sample.cpu()
        err = (out - ref).abs().max().item()
        print(f"t = {t.tolist()}: max |out - restatement| = {err:.3e}")
        assert err <= FWD_TOL
    # the labels reach the output: the uniform case under one label differs in the two other images
    t, _ = cases[1]
    one = cmodel(x.to(DEV), t, class_labels=0).sample
    mixed = cmodel(x.to(DEV), t, class_labels=[0, 4, 2]).sample
    assert torch.equal(one[0], mixed[0]) and not torch.equal(one[1], mixed[1]) and not torch.equal(one[2], mixed[2])


# ---- 2. forward bit properties -----------------------------------------------------------------------------------------
def test_zero_table_is_the_unconditional_model(eager, cond_sd, fwd_case):
    x, cases = fwd_case
    sd = dict(cond_sd)
    sd[cond_ref.TABLE] = torch.zeros_like(sd[cond_ref.TABLE])
    zero = _new_model(sd).eval()
    plain = eager.models["NV"]                                          # the same 330 weights
    for t, _ in cases:
        assert torch.equal(zero(x.to(DEV), t, class_labels=[0, 4, 2]).sample, plain(x.to(DEV), t).sample)


def test_forward_is_batch_independent(cmodel, fwd_case):
    x, cases = fwd_case
    for t, _ in cases:
        whole = cmodel(x.to(DEV), t, class_labels=[0, 4, 2]).sample
        alone = cmodel(x[1:2].to(DEV), t[1:2], class_labels=[4]).sample
        assert torch.equal(alone[0], whole[1])
        assert torch.equal(cmodel(x.to(DEV), t, class_labels=[0, 4, 2]).sample, whole)     # and deterministic


# ---- 3. gradients ------------------------------------------------------------------------------------------------------
def test_gradients_match_autograd_over_the_restatement(cond_sd):
    """B = 3 at 3x40x56, labels [1, 1, 3], timesteps [0, 500, 999]: loss and all 331 gradients; rows 0, 2 and 4 of the
    embedding's gradient are written as exact zeros; a second backward gives the same bits."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    g = torch.Generator().manual_seed(78)
    images = torch.rand(3, 3, 40, 56, generator=g) * 2 - 1
    noise = torch.randn(3, 3, 40, 56, generator=g)
    timesteps, labels = torch.tensor([0, 500, 999]), torch.tensor([1, 1, 3])
    ref_loss, ref_grads, _ = cond_ref.loss_and_grads(cond_sd, images, noise, timesteps, labels)
    model = _new_model(cond_sd)
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    HipAdam(model.parameters(), lr=1e-4)
    model.train()
    noisy = scheduler.add_noise(images.to(DEV), noise.to(DEV), timesteps.to(DEV))

    def backward():
        loss = mse_loss(model(noisy, timesteps.to(DEV), class_labels=labels).sample, noise.to(DEV))
        loss.backward()
        return loss.item(), model.grads()

    loss, grads = backward()
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert list(grads) == list(ref_grads) and len(grads) == 331
    worst, median = _grad_errors(grads, ref_grads, "conditional B3 40x56")
    print(f"relative gradient error: worst {worst[0]:.3e} ({worst[1]}), median {median[0]:.3e}")
    assert worst[0] <= GRAD_REL_WORST, f"gradient of {worst[1]}: {worst[0]:.3e} of its own largest entry"
    assert median[0] <= GRAD_REL_MEDIAN, median
    dE, ref_dE = grads[cond_ref.TABLE], ref_grads[cond_ref.TABLE]
    assert dE.shape == (N, 256)
    for k in (0, 2, 4):
        assert torch.equal(dE[k], torch.zeros(256)) and not ref_dE[k].any()
    for k in (1, 3):
        scale = ref_dE.abs().max().item()
        assert dE[k].abs().max().item() > 0 and (dE[k] - ref_dE[k]).abs().max().item() <= GRAD_REL_WORST * scale
    _, again = backward()
    assert all(torch.equal(again[n], grads[n]) for n in grads)


# ---- 4. training steps -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_batch():
    g = torch.Generator().manual_seed(79)
    images = torch.rand((B,) + CHW, generator=g) * 2 - 1
    noise = torch.randn((B,) + CHW, generator=g)
    return images.to(DEV), noise.to(DEV), torch.tensor([5, 640, 999]), torch.tensor([2, NULL, 0])


def _equal(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def test_fused_step_equals_the_spelled_out_step(cond_sd, train_batch):
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipGradScaler, mse_loss, train_step_fused
    images, noise, timesteps, labels = train_batch
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    spelled = _new_model(cond_sd)
    optimizer, scaler = HipAdam(spelled.parameters(), lr=1e-4), HipGradScaler()
    spelled.train()
    loss = mse_loss(spelled(scheduler.add_noise(images, noise, timesteps), timesteps, class_labels=labels).sample, noise)
    optimizer.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    assert scaler.step(optimizer) is True
    scaler.update()
    fused = _new_model(cond_sd)
    value, taken = train_step_fused(fused, scheduler, images, noise, timesteps, HipAdam(fused.parameters(), lr=1e-4),
                                    HipGradScaler(), class_labels=labels)
    assert taken and value == loss.item()
    sd1, sd2 = spelled.state_dict(), fused.state_dict()
    assert len(sd1) == 331 and _equal(sd1, sd2)
    o1, o2 = spelled.optimizer_state(), fused.optimizer_state()
    assert o1["step"] == o2["step"] == 1 and _equal(o1["exp_avg"], o2["exp_avg"]) and _equal(o1["exp_avg_sq"], o2["exp_avg_sq"])
    table = sd1[cond_ref.TABLE].cpu()
    moved = [k for k in range(N) if not torch.equal(table[k], cond_sd[cond_ref.TABLE][k])]
    assert moved == [0, 2, NULL]                                         # the rows of the batch's labels, and only those
    # the fused step with clipping and an EMA equals the spelled-out one too (the _ext form of the same entry point)
    from synt_isic_amd.train import HipEMA
    a, b = _new_model(cond_sd), _new_model(cond_sd)
    a.train(), b.train()
    opt_a = HipAdam(a, lr=1e-4, max_grad_norm=1.0, ema=HipEMA(a, decay=0.9999))
    opt_b = HipAdam(b, lr=1e-4, max_grad_norm=1.0, ema=HipEMA(b, decay=0.9999))
    la = mse_loss(a(scheduler.add_noise(images, noise, timesteps), timesteps, class_labels=labels).sample, noise)
    la.backward()
    assert opt_a.step() is True
    vb, _ = train_step_fused(b, scheduler, images, noise, timesteps, opt_b, None, class_labels=labels)
    assert vb == la.item() and opt_a.grad_norm == opt_b.grad_norm and opt_a.grad_norm > 0
    assert _equal(a.state_dict(), b.state_dict()) and _equal(opt_a.ema.shadow_params(), opt_b.ema.shadow_params())


def test_grad_norm_covers_the_table_and_the_ema_round_trips(cond_sd, train_batch):
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipEMA, mse_loss
    images, noise, timesteps, labels = train_batch
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    m = _new_model(cond_sd)
    ema = HipEMA(m, decay=0.9999)
    opt = HipAdam(m, lr=1e-3, max_grad_norm=1e-3, ema=ema)
    m.train()
    mse_loss(m(scheduler.add_noise(images, noise, timesteps), timesteps, class_labels=labels).sample, noise).backward()
    grads = m.grads()
    assert opt.step() is True
    norm64 = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
    without = math.sqrt(sum(float((g.double() ** 2).sum()) for k, g in grads.items() if k != cond_ref.TABLE))
    got, want = np.float32(opt.grad_norm), np.float32(norm64)
    print(f"grad_norm {got!r}, float64 over 331 tensors {norm64!r}, without the table {without!r}")
    assert abs(float(got) - float(want)) <= float(np.spacing(np.abs(want)))
    assert 0 < without < norm64                                         # the table has a share in it
    # average_parameters: the table is swapped in and back with the rest
    for _ in range(2):                                                  # two more steps: the EMA lags the weights
        mse_loss(m(scheduler.add_noise(images, noise, timesteps), timesteps, class_labels=labels).sample, noise).backward()
        assert opt.step() is True
    trained, shadow = m.state_dict(), ema.shadow_params()
    assert len(shadow) == 331 and not torch.equal(trained[cond_ref.TABLE].cpu(), shadow[cond_ref.TABLE])
    x = torch.randn((1,) + CHW, generator=torch.Generator().manual_seed(41)).to(DEV)
    m.eval()
    trained_out = m(x, 10, class_labels=[2]).sample.clone()
    fresh_out = _new_model(shadow).eval()(x, 10, class_labels=[2]).sample
    with ema.average_parameters():
        assert _equal(m.state_dict(), shadow)
        assert torch.equal(m(x, 10, class_labels=[2]).sample, fresh_out)
    assert _equal(m.state_dict(), trained) and torch.equal(m(x, 10, class_labels=[2]).sample, trained_out)
    assert not torch.equal(fresh_out, trained_out)


def test_train_conditional_over_a_labelled_loader(cond_sd, tmp_path):
    """one epoch over two labelled batches from a DeviceLoader: checkpoints of 331 tensors, the fused and the spelled-out loop
    agree bit for bit under the same generator (the same noise, timesteps and dropped labels)"""
    import os
    from synt_isic_amd.data import DeviceDataset, DeviceLoader
    from synt_isic_amd.train import train_conditional
    gen = torch.Generator().manual_seed(61)
    imgs = torch.randint(0, 256, (4, 32, 32, 3), generator=gen, dtype=torch.uint8)
    ds = DeviceDataset(imgs, DEV, labels=[0, 1, 2, 3])
    plain_batches = list(DeviceLoader(DeviceDataset(imgs, DEV), 2, shuffle=True, seed=5, augment=False))
    batches = list(DeviceLoader(ds, 2, shuffle=True, seed=5, augment=False))
    assert len(batches) == 2 and all(isinstance(b, tuple) and len(b) == 2 for b in batches)
    seen = torch.cat([lab for _, lab in batches])
    assert seen.dtype == torch.int64 and seen.device.type == "cuda" and sorted(seen.tolist()) == [0, 1, 2, 3]
    for (x, lab), px in zip(batches, plain_batches):
        assert torch.is_tensor(px) and torch.equal(x, px)               # an unlabelled dataset yields what it always did
        for img, k in zip(x, lab.tolist()):                             # the label travels with its image
            want = (imgs[k].permute(2, 0, 1).float() / 255 - 0.5) / 0.5
            assert torch.equal(img.cpu(), want)
    runs = []
    for fused in (True, False):
        m = _new_model(cond_sd)
        hist = train_conditional(m, DeviceLoader(ds, 2, shuffle=True, seed=5, augment=False), "all", cond_drop_prob=0.5,
                                 epochs=1, checkpoint_dir=str(tmp_path / str(fused)), fused=fused,
                                 generator=torch.Generator().manual_seed(62), log=None, max_grad_norm=1.0, ema_decay=0.9999)
        assert len(hist) == 1 and math.isfinite(hist[0])
        assert sorted(os.listdir(tmp_path / str(fused))) == ["unet_all_best.pth", "unet_all_best_ema.pth"]
        runs.append((hist, m.state_dict()))
    assert runs[0][0] == runs[1][0] and _equal(runs[0][1], runs[1][1])
    saved = torch.load(os.path.join(tmp_path, "True", "unet_all_best.pth"), map_location="cpu")
    assert list(saved) == list(cond_sd) and _equal(saved, runs[0][1])
    assert not torch.equal(saved[cond_ref.TABLE], cond_sd[cond_ref.TABLE])


def test_from_isic_classes_labels_by_position(monkeypatch):
    """load_isic per class id (stubbed: no ISIC files here), concatenated in the order of class_ids, label = position"""
    from synt_isic_amd.data import DeviceDataset, DeviceLoader
    calls = []

    def fake_load(image_dir, csv_path, class_id, image_size=128, max_samples=500):
        calls.append((image_dir, csv_path, class_id, image_size, max_samples))
        n = {5: 3, 2: 1, 6: 2}[class_id]
        return np.full((n, image_size, image_size, 3), 10 * class_id, dtype=np.uint8)

    monkeypatch.setattr(DeviceDataset, "load_isic", staticmethod(fake_load))
    ds = DeviceDataset.from_isic_classes("dir", "gt.csv", [5, 2, 6], image_size=16, max_samples=3, device=DEV)
    assert calls == [("dir", "gt.csv", cid, 16, 3) for cid in (5, 2, 6)]
    assert len(ds) == 6 and ds.labels.dtype == torch.int64 and ds.labels.tolist() == [0, 0, 0, 1, 2, 2]
    assert ds.images[:, 0, 0, 0].tolist() == [50, 50, 50, 20, 60, 60]
    for x, lab in DeviceLoader(ds, 4, shuffle=True, seed=1, augment=False):
        value = {0: 50, 1: 20, 2: 60}
        assert [round((float(v) * 0.5 + 0.5) * 255) for v in x[:, 0, 0, 0]] == [value[k] for k in lab.tolist()]


# ---- 5. the guidance combine -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_guide_eps_is_the_restatement_bit_for_bit(n):
    """pointers one float past a 16-byte line: the element-by-element path; aligned ones: the vector path and its tail"""
    from synt_isic_amd import ops
    g = torch.Generator().manual_seed(n)
    c, u = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    for offset in (1, 0):
        view = lambda t: torch.cat([torch.zeros(offset), t, torch.zeros(4)]).to(DEV)[offset:offset + n]
        cd, ud = view(c), view(u)
        assert cd.data_ptr() % 16 == 4 * offset
        for w in (0.0, 1.0, 3.0, -0.5):
            want = torch.from_numpy(cond_ref.guide(c.numpy(), u.numpy(), w))
            out = view(torch.zeros(n))
            ops.guide_eps(cd, ud, w, out=out)
            assert torch.equal(out.cpu(), want), (n, offset, w)
            assert torch.equal(ops.guide_eps(cd, ud, w).cpu(), want)
        assert torch.equal(cd.cpu(), c) and torch.equal(ud.cpu(), u)    # the inputs are read only
        for w in (3.0, -0.5):                                           # out may be either input
            want = torch.from_numpy(cond_ref.guide(c.numpy(), u.numpy(), w))
            for which in (0, 1):
                a, b = view(c), view(u)
                ops.guide_eps(a, b, w, out=(a, b)[which])
                assert torch.equal((a, b)[which].cpu(), want) and torch.equal((a, b)[1 - which].cpu(), (c, u)[1 - which])
    assert torch.equal(ops.guide_eps(c.to(DEV), u.to(DEV), 0.0).cpu(), u + 0.0 * (c - u))


# ---- 6. the library loop against the Python loop -----------------------------------------------------------------------
def _scheduler(rule):
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    if rule == "ddpm":
        s, eta = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2"), 0.0
    elif rule == "ddim":
        s, eta = HipDDIMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2"), 0.5
    else:
        s = HipDPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", clip_sample=True,
                                           timestep_spacing="leading", algorithm_type=rule)
        eta = 0.0
    s.set_timesteps(T)
    return s, eta


def _table(sched, eta):
    return sched.rule_table(eta)[1]


def _x_T(seeds, chw=CHW):
    return torch.stack([torch.randn(chw, generator=torch.Generator().manual_seed(3000 + int(s) % 1000)) for s in seeds]).to(DEV)


def _python_loop(model, sched, eta, x_T, z, labels, w):
    """image_generator.py:395-403 over the drop-in objects with guidance spelled out: two batch-B calls, ops.guide_eps, the
    scheduler's step.  Returns every frame."""
    from synt_isic_amd import ops
    sched.set_timesteps(T)                                              # a new run (DPM-Solver++: no history)
    tab = _table(sched, eta)
    kw = dict(eta=eta) if sched.rule == "ddim" else {}
    x, zi, frames = x_T.clone(), 0, []
    for i, t in enumerate(sched.timesteps):
        eps = model(x, t, class_labels=labels).sample
        if w != 1.0:
            eps = ops.guide_eps(eps, model(x, t, class_labels=[NULL] * len(labels)).sample, w)
        vn = None
        if z is not None and float(tab[i, 4]) != 0.0:
            vn, zi = z[zi], zi + 1
        x = sched.step(eps, t, x, variance_noise=vn, **kw).prev_sample
        frames.append(x)
    assert z is None or zi == z.shape[0]
    return torch.stack(frames)


@pytest.mark.parametrize("rule", ["ddpm", "ddim", "dpmsolver++", "sde-dpmsolver++"])
@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_library_loop_equals_python_loop(mode, noise, rule, ceager, cgraph):
    from synt_isic_amd import _lib, ops
    from synt_isic_amd.sampler import DeviceNoise, Guidance, run_sampling_loop
    s = ceager if mode == "eager" else cgraph
    model = s.models["MEL"]
    seeds = [11, (1 << 33) + 2, 0]
    x_T = _x_T(seeds)
    sched, eta = _scheduler(rule)
    tab = _table(sched, eta)
    noisy = [i for i in range(T) if float(tab[i, 4]) != 0.0]
    assert len(noisy) == {"ddpm": T - 1, "ddim": T - 1, "dpmsolver++": 0, "sde-dpmsolver++": T - 1}[rule]
    if noise == "device":
        rows = [ops.noise_fill(seeds, int(np.prod(CHW)), i).reshape((B,) + CHW) for i in noisy]
        z, source = (torch.stack(rows) if rows else None), DeviceNoise(seeds)
    else:
        z = torch.randn((len(noisy), B) + CHW, generator=torch.Generator().manual_seed(77)).to(DEV) if noisy else None
        source = z
    keep = [0, 5, T - 1]
    results = {}
    for w in (3.0, 1.0):
        frames = _python_loop(model, sched, eta, x_T, z, LABELS, w)
        res = run_sampling_loop(model, sched, x_T, source, return_trajectory=True, eta=eta, guidance=Guidance(LABELS, NULL, w))
        assert res.steps_done == T
        assert torch.equal(res.latents, frames[-1]) and torch.equal(res.trajectory, frames)
        # the uint8 images are those of the final latent (the loop de-normalises x after its last copy back from the work buffer)
        assert torch.equal(res.images, ops.denorm_u8(frames[-1])) and not torch.equal(res.images, ops.denorm_u8(x_T))
        kept = run_sampling_loop(model, sched, x_T, source, return_trajectory=True, save_indices=keep, eta=eta,
                                 guidance=Guidance(LABELS, NULL, w))
        assert kept.trajectory_steps == keep and torch.equal(kept.trajectory, frames[keep]) and torch.equal(kept.images, res.images)
        plain = run_sampling_loop(model, sched, x_T, source, eta=eta, guidance=Guidance(LABELS, NULL, w))
        assert torch.equal(plain.latents, res.latents) and torch.equal(plain.images, res.images)
        results[w] = res
    assert not torch.equal(results[3.0].latents, results[1.0].latents)  # the guidance reaches the result
    other = run_sampling_loop(model, sched, x_T, source, eta=eta, guidance=Guidance([1, 1, 1], NULL, 1.0))
    assert not torch.equal(other.latents, results[1.0].latents)         # and so do the labels
    if mode == "graph":
        # a second call with other labels (another number of distinct ones) and another w replays the captured step; a call
        # at w = 1 after one at w = 3 is another step (one pass at batch B): it re-captures
        lib = _lib.load()
        first = run_sampling_loop(model, sched, x_T, source, eta=eta, guidance=Guidance(LABELS, NULL, 3.0))
        builds = lib.sisic_unet_graph_builds(model.handle)
        assert builds >= 1 and torch.equal(first.latents, results[3.0].latents)
        second = run_sampling_loop(model, sched, x_T, source, eta=eta, guidance=Guidance([1, 1, 2], NULL, -0.5))
        assert lib.sisic_unet_graph_builds(model.handle) == builds
        want = _python_loop(model, sched, eta, x_T, z, [1, 1, 2], -0.5)[-1]
        assert torch.equal(second.latents, want) and torch.equal(second.images, ops.denorm_u8(want))
        run_sampling_loop(model, sched, x_T, source, eta=eta, guidance=Guidance(LABELS, NULL, 1.0))
        assert lib.sisic_unet_graph_builds(model.handle) == builds + 1


# ---- 7. the guided chain against the CPU restatement -------------------------------------------------------------------
def test_guided_chain_against_the_restatement(ceager, cond_sd):
    """DPM-Solver++ (ODE), T = 12 on the "leading" grid (the grid of the chain tests this bound comes from), w = 3."""
    from synt_isic_amd.sampler import Guidance, draw_noise, run_sampling_loop
    model = ceager.models["MEL"]
    sched, _ = _scheduler("dpmsolver++")
    r = dpmpp_ref.DPMSolverRef("squaredcos_cap_v2", 2, "dpmsolver++", "leading", clip_sample=True)
    r.set_timesteps(T)
    assert sched.timesteps.tolist() == r.timesteps.tolist()
    x_T, _ = draw_noise([3, 4, 5], 0, CHW)
    res = run_sampling_loop(model, sched, x_T.to(DEV), None, return_trajectory=True, guidance=Guidance(LABELS, NULL, 3.0))
    frames = cond_ref.guided_chain(cond_sd, r, x_T, LABELS, NULL, 3.0)
    diffs = [(res.trajectory[i].cpu() - f).abs().max().item() for i, f in enumerate(frames)]
    print(f"guided chain, w = 3: max |x - restatement| per step = {[f'{d:.2e}' for d in diffs]}")
    assert max(diffs) <= CHAIN_TOL


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(ceager, cond_sd):
    from synt_isic_amd import _lib
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, train_step_fused
    lib = _lib.load()
    cond, plain = _new_model(cond_sd), ceager.models["NV"]
    HipAdam(cond)
    x = torch.zeros((B,) + CHW, device=DEV)
    out = torch.zeros_like(x)
    t = (C.c_int64 * B)(1, 2, 3)
    lab = (C.c_int64 * B)(0, 1, 2)
    bad = (C.c_int64 * B)(0, 1, N)
    coef = (C.c_float * 10)(0.6, 0.8, 0.5, 0.5, 0.0, 0.6, 0.8, 0.5, 0.5, 0.0)
    ab = (C.c_float * B)(0.5, 0.5, 0.5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    einval = _lib.SISIC_EINVAL
    ch, ph = cond.handle, plain.handle
    fwd = (x.data_ptr(), C.cast(t, _lib.c_int64_p))
    shape = (out.data_ptr(), B, 32, 32, stream)
    loop = (x.data_ptr(), B, 32, 32, 2, C.cast(t, _lib.c_int64_p), C.cast(coef, _lib.c_float_p), 1.0)
    tail = (None, None, None, None, None, stream)
    step = (B, 32, 32, 1e-4, 0.9, 0.999, 1e-8, 1.0)
    abp = (C.cast(ab, _lib.c_float_p), C.cast(ab, _lib.c_float_p))
    # the unlabelled entry points on a conditional handle
    assert lib.sisic_unet_forward(ch, *fwd, *shape) == einval
    assert b"class-conditional" in lib.sisic_last_error()
    assert lib.sisic_unet_train_forward(ch, *fwd, *shape) == einval
    assert lib.sisic_unet_train_step(ch, x.data_ptr(), x.data_ptr(), fwd[1], *abp, *step, None, None, stream) == einval
    assert lib.sisic_unet_train_step_ext(ch, x.data_ptr(), x.data_ptr(), fwd[1], *abp, *step, None, None, None, None, stream) == einval
    assert lib.sisic_sample(ch, *loop, None, None, None, None, None, stream) == einval
    assert lib.sisic_sample_frames(ch, *loop, None, *tail) == einval
    assert lib.sisic_sample_frames_rule(ch, *loop, 0, 0, None, *tail) == einval
    seeds = (C.c_uint64 * B)(1, 2, 3)
    assert lib.sisic_sample_frames_rng(ch, *loop, seeds, 0, *tail) == einval
    assert lib.sisic_sample_frames_rule_rng(ch, *loop, 0, 0, seeds, 0, *tail) == einval
    # the labelled entry points on an unconditional handle
    HipAdam(plain)
    assert lib.sisic_unet_forward_cond(ph, *fwd, C.cast(lab, _lib.c_int64_p), *shape) == einval
    assert b"no class embedding" in lib.sisic_last_error()
    assert lib.sisic_unet_train_forward_cond(ph, *fwd, C.cast(lab, _lib.c_int64_p), *shape) == einval
    assert lib.sisic_unet_train_step_cond(ph, x.data_ptr(), x.data_ptr(), fwd[1], C.cast(lab, _lib.c_int64_p), *abp, *step,
                                          None, None, None, None, stream) == einval
    assert lib.sisic_sample_frames_cond(ph, *loop, 0, 0, None, None, 0, C.cast(lab, _lib.c_int64_p), NULL, 3.0, *tail) == einval
    # label N, a null label outside the table, a scale that is no number
    assert lib.sisic_unet_forward_cond(ch, *fwd, C.cast(bad, _lib.c_int64_p), *shape) == einval
    assert b"outside [0, 5)" in lib.sisic_last_error()
    assert lib.sisic_unet_train_forward_cond(ch, *fwd, C.cast(bad, _lib.c_int64_p), *shape) == einval
    assert lib.sisic_sample_frames_cond(ch, *loop, 0, 0, None, None, 0, C.cast(bad, _lib.c_int64_p), NULL, 3.0, *tail) == einval
    assert lib.sisic_sample_frames_cond(ch, *loop, 0, 0, None, None, 0, C.cast(lab, _lib.c_int64_p), N, 3.0, *tail) == einval
    assert lib.sisic_sample_frames_cond(ch, *loop, 0, 0, None, None, 0, C.cast(lab, _lib.c_int64_p), NULL, float("nan"), *tail) == einval
    assert lib.sisic_sample_frames_cond(ch, *loop, 0, 0, None, None, 0, None, NULL, 3.0, *tail) == einval
    assert not bool(out.any()) and not bool(x.any())                    # nothing was launched
    # the Python surface
    with pytest.raises(ValueError, match="class_labels should be provided"):
        cond(x, 5)
    with pytest.raises(ValueError, match="class_embedding needs to be initialized"):
        plain(x, 5, class_labels=[0, 1, 2])
    with pytest.raises(ValueError):
        cond(x, 5, class_labels=[0, 1, N])
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    with pytest.raises(ValueError, match="class_labels should be provided"):
        train_step_fused(cond, sched, x, x, torch.tensor([1, 2, 3]), HipAdam(cond))
    # a guided generate on an unconditional model
    with pytest.raises(ValueError, match="needs a class-conditional model"):
        ceager.generate(3, "NV", 4, size=(32, 32), guidance_scale=3.0)
    with pytest.raises(ValueError, match="needs a class-conditional model"):
        ceager.generate_seeds("NV", [3], 4, (32, 32), guidance_scale=0.0)


# ---- 9. the public interface -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["host", "device"])
def test_generate_seeds_with_mixed_classes_and_guidance(noise, cond_sd):
    from synt_isic_amd.sampler import Sampler, image_seed
    s = Sampler(DEV)
    s.add_conditional_model(["MEL", "NV", "BCC", "AKIEC"], cond_sd).set_graph_mode(0)
    names, seeds = ["MEL", "NV", "MEL"], [3, 0x7FFFFFFF, 12345]
    kw = dict(T=T, size=(32, 32), scheduler="dpmsolver++", noise=noise)
    res = s.generate_seeds(names, seeds, guidance_scale=3.0, return_trajectory=True, **kw)
    assert res.steps_done == T and not res.cancelled and res.seeds == seeds and torch.isfinite(res.latents).all()
    from synt_isic_amd import ops
    assert torch.equal(res.images, ops.denorm_u8(res.latents)) and torch.equal(res.latents, res.trajectory[-1])
    unguided = s.generate_seeds(names, seeds, **kw)
    assert res.noise_hashes == unguided.noise_hashes and not torch.equal(res.latents, unguided.latents)
    for b, (name, seed) in enumerate(zip(names, seeds)):                # per-image calls at batch 1, the same mode
        one = s.generate_seeds(name, [seed], guidance_scale=3.0, return_trajectory=True, **kw)
        assert torch.equal(one.latents[0], res.latents[b]) and torch.equal(one.images[0], res.images[b])
        assert torch.equal(one.trajectory[:, 0], res.trajectory[:, b]) and one.noise_hashes == res.noise_hashes[b:b + 1]
    assert not torch.equal(res.latents[0], s.generate_seeds("NV", [seeds[0]], guidance_scale=3.0, **kw).latents[0])
    # scale 0 is the null-label model at scale 1: one pass per step
    zero = s.generate_seeds(names, seeds, guidance_scale=0, **kw)
    model = s.models["MEL"]
    from synt_isic_amd.sampler import DeviceNoise, Guidance, draw_noise, draw_x_T_device, run_sampling_loop
    x_T = draw_x_T_device(seeds, CHW, torch.device(DEV)) if noise == "device" else draw_noise(seeds, 0, CHW)[0].to(DEV)
    want = run_sampling_loop(model, s.create_scheduler(T, "dpmsolver++"), x_T, DeviceNoise(seeds) if noise == "device" else None,
                             guidance=Guidance([NULL] * 3, NULL, 1.0))
    assert torch.equal(zero.latents, want.latents)
    # generate(): one image per name, each seed from its own class name
    imgs, traj = s.generate(7, names, T, size=(32, 32), seed_is_base=True, scheduler="dpmsolver++", noise=noise, guidance_scale=3.0)
    by_seed = s.generate_seeds(names, [image_seed(7, n, i) for i, n in enumerate(names)], guidance_scale=3.0, **kw)
    assert traj is None and imgs.shape == (3, 32, 32, 3) and np.array_equal(imgs, by_seed.images.cpu().numpy())
    # the streamed host-noise path (DDPM draws a z per step) carries the labels through its segments
    if noise == "host":
        s.noise_segment_steps = 5
        a = s.generate_seeds(names, seeds, T, (32, 32), guidance_scale=3.0)
        x_T, z = draw_noise(seeds, T - 1, CHW)
        b = run_sampling_loop(model, s.create_scheduler(T), x_T.to(DEV), z.to(DEV), guidance=Guidance([0, 1, 0], NULL, 3.0))
        assert torch.equal(a.latents, b.latents) and torch.equal(a.images, b.images)
    s.close()
