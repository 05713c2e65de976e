"""The executors' workload of tests/test_gpu_poison.py: UNet forwards, two short sampling runs, two training steps and the
classifier's four routes, every result written as .npy into a directory.  The test runs it once in a fresh process with
SISIC_POISON_ALLOC=1 (``python tests/poison_exec.py OUTDIR``) and once in its own process without, and compares the files."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda"
UNET_KW = dict(sample_size=128, in_channels=3, out_channels=3, layers_per_block=2, block_out_channels=(64, 128, 256, 256),
               down_block_types=("DownBlock2D", "DownBlock2D", "AttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "AttnUpBlock2D", "UpBlock2D", "UpBlock2D"), class_embed_type=None)


def _flat(named) -> np.ndarray:
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in named.values()])


def run(outdir: str) -> None:
    from synt_isic_amd import _lib
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, mse_loss
    from synt_isic_amd.unet import HipUNet2DModel
    from synt_isic_amd.weights import synthetic_resnet18_state_dict, synthetic_unet_state_dict

    def save(name, t):
        np.save(os.path.join(outdir, name + ".npy"), t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))

    sd = synthetic_unet_state_dict()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "unet_forward_b2_64.npz"))
    x64, t64 = torch.from_numpy(gold["x"]).to(DEV), torch.from_numpy(gold["t"])
    x72 = torch.randn(1, 3, 72, 40, generator=torch.Generator().manual_seed(7240)).to(DEV)

    # UNet forward, default and latency mode, whole and ragged tiles
    model = HipUNet2DModel(**UNET_KW)
    model.load_state_dict(sd)
    model = model.to(torch.device(DEV))
    model.eval()
    for mode in ("default", "latency"):
        model.set_latency_mode(mode == "latency")
        save(f"unet_{mode}_b2_64", model(x64, t64).sample)
        save(f"unet_{mode}_b1_72x40", model(x72, 321).sample)
    model.set_latency_mode(False)

    # eight steps of the fused sampling loop (eager: the sampler is not in latency mode), both rules
    s = Sampler(DEV)
    s.add_model("NV", sd)
    for rule, kw in (("ddpm", {}), ("ddim", dict(scheduler="ddim", eta=0.5))):
        res = s.generate_seeds("NV", [0, 1], T=8, size=(32, 32), return_trajectory=True, **kw)
        save(f"{rule}_latents", res.latents)
        save(f"{rule}_images", res.images)
        save(f"{rule}_trajectory", res.trajectory)
    del s
    # one image in latency mode: a replayed hipGraph by default, eager under the switch (no memset nodes in captured steps) --
    # the same bits either way, and the build count says which it was
    s = Sampler(DEV, latency_mode=True)
    m = s.add_model("NV", sd)
    save("latency_ddpm_latents", s.generate_seeds("NV", [3], T=8, size=(32, 32)).latents)
    save("latency_graph_builds", np.int64(_lib.load().sisic_unet_graph_builds(m.handle)))
    del s, m

    # two training steps of the reference's loop body
    model.train()
    opt = HipAdam(model, lr=1e-3)
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    g = torch.Generator().manual_seed(99)
    for step in (1, 2):
        images = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
        noise = torch.randn(2, 3, 64, 64, generator=g).to(DEV)
        timesteps = torch.tensor([17 * step, 990 - step])
        pred = model(sched.add_noise(images, noise, timesteps), timesteps).sample
        loss = mse_loss(pred, noise)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        save(f"train_pred{step}", pred)
        save(f"train_loss{step}", np.float32(loss.item()))
        save(f"train_grads{step}", _flat(model.grads()))
        assert opt.step()
        save(f"train_weights{step}", _flat(model._read_all(0)))
    del opt, model

    # the classifier's four routes
    clf = HipMelanomaClassifier(num_classes=7, pretrained=False)
    clf.load_state_dict(synthetic_resnet18_state_dict())
    clf = clf.to(DEV).eval()
    xc = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(64)) * 1.8 - 0.9).to(DEV)
    save("clf_logits", clf(xc))
    save("clf_stem", clf.stem_activation(xc))
    grad, logits = clf.input_gradient(xc, 5)
    save("clf_input_gradient", grad)
    save("clf_input_gradient_logits", logits)
    cam, logits = clf.grad_cam(xc, 5)
    save("clf_grad_cam", cam)
    save("clf_grad_cam_logits", logits)
    torch.cuda.synchronize()


if __name__ == "__main__":
    run(sys.argv[1])
