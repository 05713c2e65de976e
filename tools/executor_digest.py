#!/usr/bin/env python3
"""One line per item with a sha256 of its raw bytes: what the two network executors (csrc/unet.cpp with csrc/train.cpp, and
csrc/resnet.cpp) compute, launch and keep as workspace, at the smallest shapes that reach every branch of their host code.
Two builds of the library that print the same file run the same launches on the same pool blocks.

    SISIC_LIB_PATH=<library> python tools/executor_digest.py > digest.txt

The kernels have no atomics: two runs of one library print the same file."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from synt_isic_amd import _lib, ops  # noqa: E402
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


def main() -> None:
    sd = synthetic_unet_state_dict()
    if "--rider0-child" in sys.argv:             # SISIC_GN_RIDER is read when a model is created: a process of its own
        s = Sampler(DEV)
        s.add_model("NV", sd)
        unet_forward(s, "b2_64_rider0", 2, 64)
        return
    print("library:", _lib.lib_path(), file=sys.stderr)
    unet_items(sd)
    sys.stdout.flush()
    subprocess.run([sys.executable, os.path.abspath(__file__), "--rider0-child"], check=True, timeout=300,
                   env=dict(os.environ, SISIC_GN_RIDER="0"))
    train_items(sd)
    classifier_items()


if __name__ == "__main__":
    main()
