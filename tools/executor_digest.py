#!/usr/bin/env python3
"""One line per item with a sha256 of its raw bytes: what the two network executors (csrc/unet.cpp with csrc/train.cpp, and
csrc/resnet.cpp) compute, launch and keep as workspace, at the smallest shapes that reach every branch of their host code.
Two builds of the library that print the same file run the same launches on the same pool blocks.  The ``step.`` lines are the
Python step layer on top of one library (the scheduler mirrors' host tables and refusals first, without the GPU; every single-step
wrapper's marshalling last): two trees of the package that print the same lines compute the same bits.

    SISIC_LIB_PATH=<library> python tools/executor_digest.py > digest.txt
    python tools/executor_digest.py --host-only          the step layer's host lines alone: needs no GPU (compare two trees on one
                                                         machine: the DDPM / DDIM tables are fp32 torch host arithmetic, CPU-dependent)
    python tools/executor_digest.py --step-layer         the step layer's lines alone
    python tools/executor_digest.py --train              the training lines alone (train.* and clf.*), after the host lines
    python tools/executor_digest.py --shell              the model wrappers' lines alone (shell.*), after the host lines
    python tools/executor_digest.py --step-layer-items   with any of the above: every item of the step layer on its own line (by
                                                         default one line per mirror case / wrapper: the sha256 of its items)
    python tools/executor_digest.py --step-layer-times   wall time per call of the wrappers and the mirrors' step

The kernels have no atomics: two runs of one library print the same file."""
import hashlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from synt_isic_amd import _lib, ops  # noqa: E402
from synt_isic_amd import scheduler as sch  # noqa: E402
from synt_isic_amd.classifier import HipMelanomaClassifier  # noqa: E402
from synt_isic_amd.sampler import Sampler  # noqa: E402
from synt_isic_amd.scheduler import resample_schedule  # noqa: E402
from synt_isic_amd.arch import resnet18_buffer_names  # noqa: E402
from synt_isic_amd.train import HipAdam, HipClassifierAdam, mse_loss  # noqa: E402
from synt_isic_amd.weights import synthetic_resnet18_state_dict, synthetic_unet_state_dict  # noqa: E402

DEV = torch.device("cuda", 0)


def sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def emit(name, value) -> None:
    print(f"{name}\t{value}", flush=True)


def rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def unet_forward(sampler: Sampler, tag: str, B: int, size: int) -> None:
    """output, launch counts / bytes / flops per kind of ONE forward at a shape the pool already holds, workspace bytes"""
    m = sampler.models["NV"]
    x = rand((B, 3, size, size), 10 * B + size).to(DEV)
    t = torch.tensor([500] * B)
    m(x, t)                                     # sizes the pool
    ops.profile_enable(DEV, True)
    ops.profile_reset(DEV)
    y = m(x, t).sample
    torch.cuda.synchronize()
    prof = ops.profile_read(DEV)
    ops.profile_enable(DEV, False)
    emit(f"unet.{tag}.out", sha(y))
    for kind, v in prof.items():
        emit(f"unet.{tag}.launches.{kind}", f"{v['launches']} bytes={v['bytes']:.0f} flops={v['flops']:.0f}")
    emit(f"unet.{tag}.workspace_bytes", _lib.load().sisic_unet_workspace_bytes(m.handle))


def unet_items(sd) -> None:
    s = Sampler(DEV)
    m = s.add_model("NV", sd)
    unet_forward(s, "b2_64", 2, 64)             # every shortcut's GroupNorm rider is carried
    unet_forward(s, "b1_32", 1, 32)             # the 4x4 shortcuts are not: the stand-alone finalisation follows
    # sampling: eager and graph-replayed, host and device noise, DDPM and DDIM, then every other form of the loop
    cm = s.add_conditional_model(["MEL", "BCC"], synthetic_unet_state_dict(num_class_embeds=3))
    s.set_classifier(HipMelanomaClassifier(num_classes=7).load_state_dict(synthetic_resnet18_state_dict()).to(DEV).eval(),
                     {"NV": 1})
    image = rand((2, 3, 32, 32), 41).clamp(-1, 1)
    mask = (torch.rand((2, 1, 32, 32), generator=torch.Generator().manual_seed(42)) < 0.5).float()
    passes = len(resample_schedule(8, 3, 2))
    forms = {          # name -> (class names, model, keywords of generate_seeds); "streamed_<n>": NoiseStream segments of n steps
        "dpmpp_ode": ("NV", m, dict(scheduler="dpmsolver++")),
        "dpmpp_sde": ("NV", m, dict(scheduler="dpmsolver++", algorithm_type="sde-dpmsolver++")),
        "dpmpp_sde_device": ("NV", m, dict(scheduler="dpmsolver++", algorithm_type="sde-dpmsolver++", noise="device")),
        "guided": (["MEL", "BCC"], cm, dict(guidance_scale=3.0)),
        "edited_jumps_two_calls": ("NV", m, dict(noise="device", init_image=image, mask=mask, n_resample=2, jump_length=3,
                                                 max_call_steps=(passes + 1) // 2)),
        "classifier_guided": ("NV", m, dict(noise="device", classifier_scale=2.0)),
        "thresholded": ("NV", m, dict(thresholding=True, dynamic_thresholding_ratio=0.995, sample_max_value=2.0)),
        # T = 8 as library calls of 3, 3 and 2 steps (eager in both modes: a replayed call has at least 4 steps), and of 4 and 4
        "streamed_3_strided": ("NV", m, dict(return_trajectory=True, save_every_n=3)),
        "streamed_4_strided": ("NV", m, dict(return_trajectory=True, save_every_n=3)),
    }
    for graph in (0, 1):
        m.set_graph_mode(graph)
        cm.set_graph_mode(graph)
        mode = "graph" if graph else "eager"
        for noise in ("host", "device"):
            for rule, eta in (("ddpm", 0.0), ("ddim", 0.5)):
                r = s.generate_seeds("NV", [3, 4], 8, (32, 32), noise=noise, scheduler=rule, eta=eta)
                tag = f"sample.{mode}.{noise}.{rule}"
                emit(f"{tag}.latents", sha(r.latents))
                emit(f"{tag}.images", sha(r.images))
                emit(f"{tag}.graph_builds", _lib.load().sisic_unet_graph_builds(m.handle))
        for name, (classes, model, kw) in forms.items():
            s.noise_segment_steps = int(name.split("_")[1]) if name.startswith("streamed") else 64
            r = s.generate_seeds(classes, [3, 4], 8, (32, 32), **kw)
            tag = f"sample.{mode}.{name}"
            emit(f"{tag}.latents", sha(r.latents))
            emit(f"{tag}.images", sha(r.images))
            if r.trajectory is not None:
                emit(f"{tag}.trajectory", f"{sha(r.trajectory)} steps={r.trajectory_steps}")
            emit(f"{tag}.calls", f"steps_done={r.steps_done} unet_passes={r.unet_passes}")
            emit(f"{tag}.graph_builds", _lib.load().sisic_unet_graph_builds(model.handle))
    s.close()
    lat = Sampler(DEV, latency_mode=True)
    lat.add_model("NV", sd)
    unet_forward(lat, "b1_64_latency", 1, 64)
    lat.close()


def train_items(sd) -> None:
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel()
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    opt = HipAdam(m, lr=1e-4)
    x, noise, t = rand((2, 3, 32, 32), 21).to(DEV), rand((2, 3, 32, 32), 22).to(DEV), torch.tensor([37, 640])
    opt.zero_grad()
    loss = mse_loss(m(x, t).sample, noise)
    loss.backward()
    emit("train.loss", sha(loss.detach()))
    emit("train.grads", sha(*m.grads().values()))           # state-dict order
    opt.step()
    emit("train.forward_after_step", sha(m(x, t).sample))
    emit("train.workspace_bytes", _lib.load().sisic_unet_workspace_bytes(m.handle))


def _train_state(m, ema=None) -> str:
    """weights | m | v after a step, the step count and (with an EMA) the shadow weights"""
    st = m.optimizer_state()
    line = f"{sha(*m.state_dict().values(), *st['exp_avg'].values(), *st['exp_avg_sq'].values())} step={st['step']}"
    return line if ema is None else f"{line} ema={sha(*ema.shadow_params().values())}"


def train_step_items(sd) -> None:
    """One training step at batch 2, 32x32 (every level, both attention widths in use, the K-split weight gradient) from fresh
    weights and moments, fused and spelled out, under every optimizer option, scaler, label and objective: loss, gradients and
    weights | m | v each; a scaler-skipped step with the EMA on; sisic_mse_loss alone."""
    import ctypes as C
    from synt_isic_amd.train import HipEMA, HipGradScaler, diffusion_loss, train_step_fused
    from synt_isic_amd.unet import HipUNet2DModel
    sched = sch.HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    x, noise, t = rand((2, 3, 32, 32), 21).clamp(-1, 1).to(DEV), rand((2, 3, 32, 32), 22).to(DEV), torch.tensor([37, 640])
    options = {"plain": (None, False), "clip": (1e-3, False), "ema": (None, True), "both": (1e-3, True)}

    def step(tag, m, weights, fused, option, scaled, labels=None, snr_gamma=None):
        m.load_state_dict(weights)               # fresh moments, step 0
        m.train()
        max_norm, with_ema = options[option]
        ema = HipEMA(m, decay=0.9999) if with_ema else None
        opt = HipAdam(m, lr=1e-4, max_grad_norm=max_norm, ema=ema)
        scaler = HipGradScaler() if scaled else None
        if fused:
            value, taken = train_step_fused(m, sched, x, noise, t, opt, scaler, class_labels=labels, snr_gamma=snr_gamma)
        else:
            pred = m(sched.add_noise(x, noise, t), t, class_labels=labels).sample
            if snr_gamma is None and m.prediction_type == "epsilon":
                loss = mse_loss(pred, noise)
            else:
                loss = diffusion_loss(pred, x, noise, t, sched, snr_gamma=snr_gamma)
            opt.zero_grad()
            if scaler is None:
                loss.backward()
                taken = opt.step()
            else:
                scaler.scale(loss).backward()
                taken = scaler.step(opt)
                scaler.update()
            value = loss.item()
        emit(f"train.{tag}.loss", f"{float(value).hex()} taken={taken} norm={opt.grad_norm}")
        emit(f"train.{tag}.grads", sha(*m.grads().values()))
        emit(f"train.{tag}.state", _train_state(m, ema))
        return opt, ema

    m = HipUNet2DModel()
    m.load_state_dict(sd)
    m = m.to(DEV)
    for fused in (True, False):
        form = "fused" if fused else "spelled"
        for option in options:
            for scaled in (False, True):
                step(f"{form}.{option}.scaler{int(scaled)}", m, sd, fused, option, scaled)
        for kind, gamma in (("v_prediction", 5.0), ("sample", None)):
            m.set_prediction_type(kind)
            step(f"{form}.{kind}.snr{gamma}", m, sd, fused, "plain", True, snr_gamma=gamma)
        m.set_prediction_type("epsilon")
    # a step the scaler skips, the EMA on: two clean steps first (the EMA then lags the weights), then one planted inf
    opt, ema = step("skip.clean1", m, sd, True, "both", True)
    scaler = HipGradScaler()
    train_step_fused(m, sched, x, noise, t, opt, scaler)
    emit("train.skip.before", _train_state(m, ema))
    name, g = next(iter(m.grads().items()))
    g.view(-1)[g.numel() // 2] = float("inf")
    m.set_grads({name: g})
    emit("train.skip.taken", scaler.step(opt))
    emit("train.skip.after", _train_state(m, ema))
    # sisic_mse_loss alone, 210 elements (a partial block): no weights, and weights of ones
    lib = _lib.load()
    pred, target = rand((2, 3, 5, 7), 23).to(DEV), rand((2, 3, 5, 7), 24).to(DEV)
    ones = torch.ones(2)
    for tag, w in (("plain", None), ("ones", ones)):
        loss, dpred = ops.empty(1, dtype=torch.float32, device=DEV), ops.empty_like(pred)
        _lib.check(lib.sisic_unet_set_loss_weights(m.handle, C.cast(w.data_ptr(), _lib.c_float_p) if w is not None else None,
                                                   2 if w is not None else 0))
        _lib.check(lib.sisic_mse_loss(m.handle, pred.data_ptr(), target.data_ptr(), pred.numel(), 3.0, loss.data_ptr(),
                                      dpred.data_ptr(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
        _lib.check(lib.sisic_unet_set_loss_weights(m.handle, None, 0))
        emit(f"train.mse_loss.{tag}", f"loss={sha(loss)} dpred={sha(dpred)}")
    # the class-conditional model, with the extension and without
    csd = synthetic_unet_state_dict(num_class_embeds=3)
    cm = HipUNet2DModel(num_class_embeds=3)
    cm.load_state_dict(csd)
    cm = cm.to(DEV)
    for fused in (True, False):
        for option in ("plain", "both"):
            step(f"cond.{'fused' if fused else 'spelled'}.{option}", cm, csd, fused, option, True, labels=torch.tensor([2, 0]))


def classifier_items() -> None:
    sd = synthetic_resnet18_state_dict()
    clf = HipMelanomaClassifier(num_classes=7).load_state_dict(sd).to(DEV).eval()
    x = (rand((2, 3, 48, 40), 31) * 0.8).to(DEV)
    emit("clf.logits", sha(clf(x)))
    emit("clf.logits.workspace_bytes", clf.workspace_bytes())
    emit("clf.stem", sha(clf.stem_activation(x)))
    emit("clf.stem.workspace_bytes", clf.workspace_bytes())
    grad, logits = clf.input_gradient(x, 1)
    emit("clf.input_gradient", sha(grad) + " logits=" + sha(logits))
    emit("clf.input_gradient.workspace_bytes", clf.workspace_bytes())
    cam, logits = clf.grad_cam(x, 1)
    emit("clf.grad_cam", sha(cam) + " logits=" + sha(logits))
    emit("clf.grad_cam.workspace_bytes", clf.workspace_bytes())
    emit("clf.logits_b3", sha(clf((rand((3, 3, 48, 40), 32) * 0.8).to(DEV))))          # the shape change empties the pool
    emit("clf.logits_b3.workspace_bytes", clf.workspace_bytes())
    grad, logits = clf.input_gradient(x, [1, 4])
    emit("clf.input_gradient_targets", sha(grad) + " logits=" + sha(logits))
    emit("clf.input_gradient_targets.workspace_bytes", clf.workspace_bytes())
    emit("clf.features", sha(clf.features(x)))
    emit("clf.features.workspace_bytes", clf.workspace_bytes())
    # training, BatchNorm frozen and with batch statistics: the raw input through the 224x224 resize, then pre-processed inputs at
    # the smallest plane the geometry check admits (32x32: a last plane of 1x1) and at a non-square one
    cw = torch.tensor([1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 0.75])
    batches = (("raw_48x40", x, [1, 4], False),
               ("pre_32x32", rand((2, 3, 32, 32), 33).to(DEV), [0, 6], True),
               ("pre_64x96", rand((3, 3, 64, 96), 34).to(DEV), [2, 5, 3], True))
    for mode in ("frozen", "batch"):
        clf.load_state_dict(sd)                  # the weights the previous section's step moved
        opt = HipClassifierAdam(clf, batchnorm=mode)
        for tag, images, labels, preprocessed in batches:
            loss, logits = clf.loss_backward(images, labels, class_weights=cw, preprocessed=preprocessed)
            name = f"clf.train.{mode}.{tag}"
            emit(f"{name}.loss", float(loss).hex() + " logits=" + sha(logits))
            grads = clf.grads()
            emit(f"{name}.grads", f"{sha(*grads.values())} n={len(grads)}")
            if mode == "batch":
                stats = [clf.read_tensor(0, n) for n in resnet18_buffer_names(clf.num_classes)]
                emit(f"{name}.running_stats", f"{sha(*stats)} n={len(stats)}")
            emit(f"{name}.workspace_bytes", clf.workspace_bytes())
        opt.step()
        emit(f"clf.train.{mode}.logits_after_step", sha(clf(x)))
        emit(f"clf.train.{mode}.logits_after_step.workspace_bytes", clf.workspace_bytes())
        opt.close()
    clf.load_state_dict(sd)
    grad, logits = clf.input_gradient(x, 1)      # the first item's bits again
    emit("clf.input_gradient_after_training", sha(grad) + " logits=" + sha(logits))
    emit("clf.input_gradient_after_training.workspace_bytes", clf.workspace_bytes())


def shell_items(sd) -> None:
    """The handle-owning shell of both model classes through one sequence: load, state dict, to(cpu), to(cuda), forward, an
    optimizer, one backward and one step at batch 2, 32x32, what the step left, a device round trip with stale host copies, a
    reload under the live optimizer, forward; then what every refusal of the shell says."""
    from synt_isic_amd.unet import HipUNet2DModel
    x, noise, t = rand((2, 3, 32, 32), 71).to(DEV), rand((2, 3, 32, 32), 72).to(DEV), torch.tensor([37, 640])
    csd = synthetic_resnet18_state_dict()

    def unet_step(m, opt):
        m.train()
        opt.zero_grad()
        mse_loss(m(x, t).sample, noise).backward()
        opt.step()
        st = m.optimizer_state()
        return sha(*st["exp_avg"].values(), *st["exp_avg_sq"].values()) + f" step={st['step']}"

    def clf_step(m, opt):
        opt.zero_grad()
        m.loss_backward(x, [1, 4], preprocessed=True)
        opt.step()
        names = m.trainable_names(opt.batchnorm)
        return sha(*[m.read_tensor(w, n) for w in (2, 3) for n in names]) + f" step={opt.steps}"

    cases = (("unet", HipUNet2DModel, sd, lambda m: m.eval()(x, t).sample, lambda m: HipAdam(m.train(), lr=1e-4), unet_step),
             ("clf", lambda: HipMelanomaClassifier(num_classes=7), csd, lambda m: m(x, preprocessed=True),
              lambda m: HipClassifierAdam(m, batchnorm="batch"), clf_step))
    for tag, make, weights, forward, optimizer, step in cases:
        m = make()
        m.load_state_dict(weights)
        emit(f"shell.{tag}.state_dict", f"{sha(*m.state_dict().values())} keys={sha_text(m.state_dict())} device={m.device}")
        m = m.to("cpu").to("cuda")
        emit(f"shell.{tag}.device", f"{m.device} params={sorted({str(p.device) for p in m.parameters()})}")
        emit(f"shell.{tag}.forward", sha(forward(m)))
        opt = optimizer(m)
        emit(f"shell.{tag}.moments", step(m, opt))
        emit(f"shell.{tag}.grads", f"{sha(*m.grads().values())} n={len(m.grads())}")
        emit(f"shell.{tag}.state_dict_after_step", f"{sha(*m.state_dict().values())} keys={sha_text(m.state_dict())}")
        step(m, opt)                                         # host copies stale again: the move reads them back first
        m = m.to("cpu")
        emit(f"shell.{tag}.state_dict_on_cpu", f"{sha(*m.state_dict().values())} device={m.device}")
        m = m.to(DEV)
        emit(f"shell.{tag}.forward_after_round_trip", sha(forward(m)))
        opt = optimizer(m)
        emit(f"shell.{tag}.moments_after_round_trip", step(m, opt))
        m.load_state_dict(weights)                           # under the live optimizer
        emit(f"shell.{tag}.forward_after_reload", sha(forward(m)))
        emit(f"shell.{tag}.state_dict_after_reload", sha(*m.state_dict().values()))
        if tag == "unet":
            emit("shell.unet.moments_after_reload", step(m, opt))
        else:
            emit("shell.clf.optimizer_after_reload", f"active={opt._active} trainer={m._trainer} " + said(lambda: opt.steps))
    # refusals: the handle, the arenas, the two load_state_dicts
    um, cm = HipUNet2DModel(), HipMelanomaClassifier(num_classes=7)
    for tag, fresh, weights in (("unet", um, sd), ("clf", cm, csd)):
        emit(f"shell.{tag}.refusal.handle_on_cpu", said(lambda: fresh.handle))
        fresh.to(DEV)
        emit(f"shell.{tag}.refusal.handle_without_weights", said(lambda: fresh.handle))
        first, last = next(iter(weights)), next(reversed(weights))
        emit(f"shell.{tag}.refusal.load_missing", said(lambda: fresh.load_state_dict({k: v for k, v in weights.items() if k != last})))
        emit(f"shell.{tag}.refusal.load_extra", said(lambda: fresh.load_state_dict(dict(weights, extra=torch.zeros(1)))))
        emit(f"shell.{tag}.refusal.load_shape", said(lambda: fresh.load_state_dict(dict(weights, **{first: torch.zeros(3)}))))
        emit(f"shell.{tag}.refusal.load_nonstrict_without_weights",
             said(lambda: fresh.load_state_dict({k: v for k, v in weights.items() if k != last}, strict=False)))
        emit(f"shell.{tag}.refusal.handle_after_refused_loads", said(lambda: fresh.handle))
        fresh.load_state_dict(weights)
        emit(f"shell.{tag}.nonstrict_extra", said(lambda: fresh.load_state_dict(dict(weights, extra=torch.zeros(1)), strict=False)))
        emit(f"shell.{tag}.nonstrict_fallback", said(lambda: fresh.load_state_dict(
            dict({k: v * 2 for k, v in weights.items() if k != last}, **{first: torch.zeros(3)}), strict=False)))
        emit(f"shell.{tag}.nonstrict_fallback.state_dict", sha(*fresh.state_dict().values()))
        fresh.load_state_dict(weights)
    name, shape = next(iter(um._spec.items()))
    emit("shell.unet.refusal.grads_without_optimizer", said(um.grads))
    emit("shell.unet.refusal.set_grads_without_optimizer", said(lambda: um.set_grads({name: torch.zeros(shape)})))
    emit("shell.unet.refusal.write_all_without_optimizer", said(lambda: um._write_all(1, {name: torch.zeros(shape)}, "digest")))
    HipAdam(um, lr=1e-4)
    emit("shell.unet.refusal.set_grads_unknown", said(lambda: um.set_grads({"no.such.weight": torch.zeros(1)})))
    emit("shell.unet.refusal.set_grads_shape", said(lambda: um.set_grads({name: torch.zeros(3)})))
    emit("shell.unet.refusal.write_all_parameters", said(lambda: um._write_all(0, {name: torch.zeros(shape)}, "digest")))
    emit("shell.unet.refusal.write_all_what_9", said(lambda: um._write_all(9, {name: torch.zeros(shape)}, "digest")))
    emit("shell.unet.refusal.read_all_what_9", said(lambda: um._read_all(9)))
    um.set_grads({name: torch.ones(shape)})
    emit("shell.unet.set_grads", sha(um.grads()[name]))
    bn, fc = "model.bn1.weight", "model.fc.bias"
    emit("shell.clf.refusal.read_without_optimizer", said(lambda: cm.read_tensor(1, fc)))
    emit("shell.clf.refusal.write_without_optimizer", said(lambda: cm.write_tensor(1, fc, torch.zeros(7))))
    emit("shell.clf.read_parameter_without_optimizer", sha(cm.read_tensor(0, bn)))
    opt = HipClassifierAdam(cm)
    emit("shell.clf.refusal.read_frozen", said(lambda: cm.read_tensor(1, bn)))
    emit("shell.clf.refusal.write_frozen", said(lambda: cm.write_tensor(2, bn, torch.zeros(64))))
    emit("shell.clf.read_frozen_parameter", sha(cm.read_tensor(0, bn)))
    emit("shell.clf.refusal.read_unknown", said(lambda: cm.read_tensor(0, "no.such.weight")))
    emit("shell.clf.refusal.read_what_9", said(lambda: cm.read_tensor(9, fc)))
    emit("shell.clf.refusal.write_shape", said(lambda: cm.write_tensor(1, fc, torch.zeros(3))))
    emit("shell.clf.refusal.write_unknown", said(lambda: cm.write_tensor(1, "no.such.weight", torch.zeros(3))))
    emit("shell.clf.refusal.write_parameters", said(lambda: cm.write_tensor(0, fc, torch.zeros(7))))
    emit("shell.clf.refusal.write_what_9", said(lambda: cm.write_tensor(9, fc, torch.zeros(7))))
    emit("shell.clf.refusal.set_grads_missing", said(lambda: cm.set_grads({fc: torch.zeros(7)})))
    cm.write_tensor(1, fc, torch.ones(7))
    emit("shell.clf.write_tensor", sha(cm.read_tensor(1, fc)))
    opt.close()
    emit("shell.clf.refusal.closed_optimizer", said(lambda: opt.steps))


def sha_text(names) -> str:
    return hashlib.sha256("\n".join(names).encode()).hexdigest()[:16]


# ---- the Python step layer (ops.*_step*, the scheduler mirrors, sampler._check_scheduler): names of both sides of its fold only
NEW_MIRROR_METHODS = {"rule_table", "abar_prev"}        # what the fold added to every mirror: left out of the attribute lists


ITEMS = "--step-layer-items" in sys.argv           # every item of the step layer on a line of its own, not one line per group
_groups = {}


def item(group: str, name: str, value) -> None:
    """an item of the step layer: its own line under --step-layer-items, else part of its group's line (``close_groups``)"""
    if ITEMS:
        emit(f"{group}.{name}", value)
    else:
        _groups.setdefault(group, []).append(f"{name}\t{value}\n")


def close_groups() -> None:
    """one line per group: the sha256 of its items' lines, which --step-layer-items prints one by one to find a difference"""
    for group, lines in _groups.items():
        emit(group, f"{hashlib.sha256(''.join(lines).encode()).hexdigest()} items={len(lines)}")
    _groups.clear()


def said(fn) -> str:
    """what a call that should be refused says"""
    try:
        fn()
    except Exception as e:          # noqa: BLE001
        return f"{type(e).__name__}: {e}"
    return "accepted"


def mirror_cases():
    """(tag, class, constructor keywords, etas of its coefficient_table) over every mirror's constructor options"""
    for beta in ("linear", "squaredcos_cap_v2"):
        yield f"ddpm.{beta}", sch.HipDDPMScheduler, dict(beta_schedule=beta), (None,)
        for spacing in ("leading", "trailing"):
            for one in (True, False):
                yield (f"ddim.{beta}.{spacing}.one{int(one)}", sch.HipDDIMScheduler,
                       dict(beta_schedule=beta, timestep_spacing=spacing, set_alpha_to_one=one), (0.0, 0.5, 1.0))
        for spacing in ("linspace", "leading", "trailing"):
            for order in (1, 2):
                for alg in sch.DPMPP_ALGORITHMS:
                    yield (f"dpmpp.{beta}.{spacing}.o{order}.{alg}", sch.HipDPMSolverMultistepScheduler,
                           dict(beta_schedule=beta, timestep_spacing=spacing, solver_order=order, algorithm_type=alg), (None,))


def step_layer_host() -> None:
    """tables, grids, configs and refusals of the mirrors: no GPU"""
    from synt_isic_amd.sampler import _check_scheduler
    np.seterr(all="ignore")         # DPM-Solver++ on a grid with two equal neighbours divides by zero: its bits are printed as they are
    classes = (sch.HipDDPMScheduler, sch.HipDDIMScheduler, sch.HipDPMSolverMultistepScheduler)
    for tag, cls, kw, etas in mirror_cases():
        for T in (1, 2, 7, 50, 1000):
            s = cls(**kw)
            s.set_timesteps(T)
            item(f"step.host.{tag}", f"T{T}.timesteps", sha(s.timesteps))
            for eta in etas:
                table = s.coefficient_table() if eta is None else s.coefficient_table(eta)
                item(f"step.host.{tag}", f"T{T}.table.eta{eta}", f"{sha(table)} {tuple(table.shape)}")
            item(f"step.host.{tag}", f"T{T}.edit_rows", sha(sch.edit_rows(s, resample_schedule(T, 3, 2))))
        s = cls(**kw)
        item(f"step.host.{tag}", "config", list(vars(s.config).items()))
        before = s.threshold
        s.set_thresholding(True, 0.9, 2.0)
        item(f"step.host.{tag}", "threshold", f"{before} -> {s.threshold}; config {list(vars(s.config).items())}")
    for cls in classes:
        name = cls.__name__
        item(f"step.host.{name}", "public", sorted(n for n in dir(cls) if not n.startswith("_") and n not in NEW_MIRROR_METHODS))
        for what, kw in (("thresholding", dict(thresholding=True)), ("v_prediction", dict(prediction_type="v_prediction")),
                         ("scaled_linear", dict(beta_schedule="scaled_linear")), ("unknown", dict(rescale_betas_zero_snr=True)),
                         ("thresholding_ratio_0", dict(thresholding=True, dynamic_thresholding_ratio=0.0))):
            item(f"step.host.{name}", f"refusal.{what}", said(lambda: cls(**kw)))
        for T in (0, 1001):
            item(f"step.host.{name}", f"refusal.set_timesteps_{T}", said(lambda: cls().set_timesteps(T)))
    for args in (("heun", 0.0), ("ddpm", 0.5), ("ddpm", 0.0, True), ("dpmsolver++", 0.5), ("dpmsolver++", 0.0, True), ("ddim", 1.5),
                 ("ddim", -0.1), ("dpmsolver++", 0.0, False, 3), ("dpmsolver++", 0.0, False, 2, "dpmsolver"),
                 ("ddpm", 0.0, False, 1), ("ddim", 0.0, False, 2, "sde-dpmsolver++"), (None, 0.0)):
        item("step.host.check_scheduler", str(args), said(lambda: _check_scheduler(*args)))
    close_groups()


def shifted(t: torch.Tensor) -> torch.Tensor:
    """the same values one float past an allocation's start: contiguous, off every 16-byte line"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


# rows with sigma != 0; the second DPM-Solver++ row reads hist (k1 != 0)
STEP_ROWS = {"ddpm": ((0.6, 0.8, 0.3, 0.7, 0.25),), "ddim": ((0.6, 0.8, 0.9, 0.35, 0.25),),
             "dpmpp": ((0.6, 0.8, 0.7, 0.4, 0.25, 0.0), (0.55, 0.835, 0.75, 0.45, 0.2, -0.15))}


def step_layer_gpu() -> None:
    """every wrapper's marshalling at [2,3,5,7] (210 elements: a scalar tail; 105 per image: image 1 off the 16-byte lines),
    aligned and shifted by one float; the mirrors' ``step`` under the three noise sources; add_noise and get_velocity"""
    shape, seeds, step = (2, 3, 5, 7), (3, 2 ** 63 + 5), 4
    base = dict(x=rand(shape, 51).to(DEV), eps=rand(shape, 52).to(DEV), z=rand(shape, 53).to(DEV),
                x0k=rand(shape, 54).clamp(-1, 1).to(DEV),
                mask=(torch.rand((2, 1, 5, 7), generator=torch.Generator().manual_seed(55)) < 0.5).float().to(DEV))
    erow = (0.9, 0.43, 0.95, 0.31)
    for place in ("aligned", "shifted"):
        t = base if place == "aligned" else {k: shifted(v) for k, v in base.items()}
        for stem, rows in STEP_ROWS.items():
            for flag in ((False, True) if stem == "ddim" else (None,)):
                for form in ("", "_rng", "_edit"):
                    fn = getattr(ops, f"{stem}_step{form}")
                    for pred in ("epsilon", "sample", "v_prediction"):
                        for thr in (None, (0.9, 2.0)):
                            kw = dict(clip=1.0, prediction_type=pred, threshold=thr)
                            if flag is not None:
                                kw["use_clipped_model_output"] = flag
                            hist = torch.zeros_like(t["x"]) if stem == "dpmpp" else None
                            x, shas = t["x"], []
                            for row in rows:
                                lead = (t["eps"], x) + ((t["z"],) if form == "" else (seeds, step))
                                lead += (hist,) if hist is not None else ()
                                tail = (t["x0k"], t["mask"], erow) if form == "_edit" else ()
                                x = fn(*lead, row, *tail, **kw)
                                shas.append(sha(x) if hist is None else f"{sha(x)} hist={sha(hist)}")
                            item(f"step.gpu.{place}.{stem}{form}", f"flag{flag}.{pred}.thr{thr}", " ".join(shas))
    eps, x0 = base["eps"], base["x"]
    for tag, cls, kw, step_kw in (("ddpm", sch.HipDDPMScheduler, {}, {}), ("ddim", sch.HipDDIMScheduler, {}, dict(eta=0.5)),
                                  ("dpmpp", sch.HipDPMSolverMultistepScheduler, dict(algorithm_type="sde-dpmsolver++"), {})):
        sources = {"variance_noise": lambda: dict(variance_noise=base["z"]),
                   "cpu_generator": lambda: dict(generator=torch.Generator().manual_seed(7)),
                   "device_generator": lambda: dict(generator=torch.Generator(device=DEV).manual_seed(7))}
        for name, source in sources.items():
            s = cls(beta_schedule="squaredcos_cap_v2", **kw)
            s.set_timesteps(10)
            x, noise_kw = x0, source()
            for t_ in s.timesteps[:2]:
                x = s.step(eps, t_, x, **step_kw, **noise_kw).prev_sample
            item(f"step.gpu.mirror.{tag}", name, sha(x))
        ts = torch.tensor([37, 640])
        item(f"step.gpu.mirror.{tag}", "add_noise", sha(s.add_noise(x0, eps, ts)))
        item(f"step.gpu.mirror.{tag}", "get_velocity", sha(s.get_velocity(x0, eps, ts)))
    torch.cuda.synchronize()
    close_groups()


def step_layer_times(calls: int = 2000) -> None:
    """host cost of the layer: wall microseconds per call of each buffer-form wrapper and each mirror's ``step`` on [2,3,8,8],
    nothing synchronised before the last call has been issued"""
    shape = (2, 3, 8, 8)
    x, eps, z = (rand(shape, 60 + i).to(DEV) for i in range(3))
    hist = torch.zeros_like(x)
    wrappers = {"ops.ddpm_step": lambda: ops.ddpm_step(eps, x, z, STEP_ROWS["ddpm"][0]),
                "ops.ddim_step": lambda: ops.ddim_step(eps, x, z, STEP_ROWS["ddim"][0]),
                "ops.dpmpp_step": lambda: ops.dpmpp_step(eps, x, z, hist, STEP_ROWS["dpmpp"][1])}
    for name, call in wrappers.items():
        call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        emit(f"time.{name}.us_per_call", f"{(time.perf_counter() - t0) / calls * 1e6:.2f}")
    for tag, cls, kw in (("ddpm", sch.HipDDPMScheduler, {}), ("ddim", sch.HipDDIMScheduler, {}),
                         ("dpmpp", sch.HipDPMSolverMultistepScheduler, dict(timestep_spacing="leading"))):
        s = cls(beta_schedule="squaredcos_cap_v2", **kw)
        spent, timed = 0.0, 0
        while timed < calls:            # runs of the whole 1000-step grid; the first step of a run (DPM-Solver++ builds its tables) untimed
            s.set_timesteps(1000)
            s.step(eps, s.timesteps[0], x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t_ in s.timesteps[1:min(1000, 1 + calls - timed)]:
                s.step(eps, t_, x)
                timed += 1
            torch.cuda.synchronize()
            spent += time.perf_counter() - t0
        emit(f"time.{cls.__name__}.step.us_per_call", f"{spent / timed * 1e6:.2f}")


def main() -> None:
    sd = synthetic_unet_state_dict()
    if "--rider0-child" in sys.argv:             # SISIC_GN_RIDER is read when a model is created: a process of its own
        s = Sampler(DEV)
        s.add_model("NV", sd)
        unet_forward(s, "b2_64_rider0", 2, 64)
        return
    if "--step-layer-times" in sys.argv:
        return step_layer_times()
    step_layer_host()                            # first, and without the GPU: a machine that has none compares these lines
    if "--host-only" in sys.argv:
        return
    if "--step-layer" in sys.argv:
        return step_layer_gpu()
    print("library:", _lib.lib_path(), file=sys.stderr)
    if "--shell" in sys.argv:
        return shell_items(sd)
    if "--train" in sys.argv:
        train_items(sd)
        train_step_items(sd)
        return classifier_items()
    unet_items(sd)
    sys.stdout.flush()
    subprocess.run([sys.executable, os.path.abspath(__file__), "--rider0-child"], check=True, timeout=300,
                   env=dict(os.environ, SISIC_GN_RIDER="0"))
    train_items(sd)
    train_step_items(sd)
    classifier_items()
    shell_items(sd)
    step_layer_gpu()


if __name__ == "__main__":
    main()
