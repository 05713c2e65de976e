"""The workload of one child process of tests/test_gpu_dispatch_switches.py, and the table of what each set of dispatch switches
changes (pinned on the host by tests/test_dispatch_switches_cpu.py).

conv_plan.cpp reads nine switches once per process and sisic_unet_create reads SISIC_WINOGRAD, so a set is the environment of a
fresh interpreter:

    python tests/switch_exec.py OUTDIR [--b64]     the executors' workload on the GPU, every result as .npy into OUTDIR
    python tests/switch_exec.py --plans            the host-only record of plans as JSON on stdout (no device is touched)

The workload installs tests/poison.py before anything allocates, counts the unwritten elements of every result
(``unwritten.json``) and checks the guard bands at the end.  ``plans.json`` is the child's own walk of every forward convolution
(tools/arch_plan_table.py) -- the proof that the environment reached the library in this process.  ``--b64`` adds one eval()
forward at 64x64x64, the only batch at which the staged K-split form of the 1x1 convolutions is chosen (256 workgroups).
"""
import json
import os
import sys
import time
from collections import Counter, OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda"

PLAN_SWITCHES = ("SISIC_WINO_WIDE", "SISIC_WINO_BF16X3", "SISIC_WINO_COL", "SISIC_KSPLIT", "SISIC_POINTWISE", "SISIC_POINTWISE_BF16X3",
                 "SISIC_POINTWISE_KSPLIT", "SISIC_S2_BF16X3", "SISIC_POINTWISE_STAGED_KSPLIT")
SWITCHES = PLAN_SWITCHES + ("SISIC_WINOGRAD",)

# the sets that are run: every variable of a set is "0".  One switch at a time would leave most fallback kernels unvisited
# (SISIC_WINO_WIDE / SISIC_WINO_COL alone change only the layers bf16x3 leaves, SISIC_POINTWISE alone changes nothing).
SETS = OrderedDict([
    ("wino_bf16x3", ("SISIC_WINO_BF16X3",)),
    ("wino_bf16x3+col", ("SISIC_WINO_BF16X3", "SISIC_WINO_COL")),
    ("wino_bf16x3+wide", ("SISIC_WINO_BF16X3", "SISIC_WINO_WIDE")),
    ("ksplit", ("SISIC_KSPLIT",)),
    ("pointwise_bf16x3", ("SISIC_POINTWISE_BF16X3",)),
    ("pointwise_bf16x3+pointwise", ("SISIC_POINTWISE_BF16X3", "SISIC_POINTWISE")),
    ("pointwise_ksplit", ("SISIC_POINTWISE_KSPLIT",)),
    ("s2_bf16x3", ("SISIC_S2_BF16X3",)),
    ("pointwise_staged_ksplit", ("SISIC_POINTWISE_STAGED_KSPLIT",)),
    ("winograd", ("SISIC_WINOGRAD",)),
    ("all_off", SWITCHES),
])
STAGED_SET = "pointwise_staged_ksplit"          # "both forms give the same bits" (conv_plan.cpp): held to equality, and run with --b64

# (B, H, W) of the plan record: what the workload runs (2x64x64, 3x40x56, the sampler's 2x32x32, 1x72x40, 64x64x64)
RECORD_SHAPES = ((2, 64, 64), (3, 40, 56), (2, 32, 32), (1, 72, 40), (64, 64, 64))
# the walk the transition table below was counted over: 4 x 40 distinct (plane, convolution) pairs and the classifier's 11
TABLE_SHAPES = ((2, 64, 64), (2, 32, 32), (1, 72, 40), (64, 64, 64))
TABLE_TOTALS = {"wino_bf16x3": 68, "wino_bf16x3+col": 78, "wino_bf16x3+wide": 78, "ksplit": 13, "pointwise_bf16x3": 41,
                "pointwise_bf16x3+pointwise": 41, "pointwise_ksplit": 18, "s2_bf16x3": 15, "pointwise_staged_ksplit": 4}

# The (default plan -> fallback plan) transitions of every set, counted over TABLE_SHAPES and the classifier: 171 distinct
# convolutions.  tests/test_dispatch_switches_cpu.py pins it against the library on the host; the GPU test requires every child's own
# record to show exactly these.  (SISIC_WINOGRAD=0 shows in no plan: sisic_unet_create withholds the Winograd filters instead.)
TRANSITIONS = {
    "wino_bf16x3": {
        "Winograd bf16x3, cfg 74 -> Winograd first, cfg 66": 9,             # nearest-2x inputs
        "Winograd bf16x3, cfg 74 -> Winograd third, cfg 68": 30,
        "Winograd bf16x3, cfg 74 -> Winograd third, cfg 69": 17,
        "Winograd bf16x3, cfg 92 -> Winograd third, cfg 91": 12,            # the 8x8 level: image pairs
    },
    "wino_bf16x3+col": {
        "Winograd bf16x3, cfg 74 -> Winograd first, cfg 66": 9,
        "Winograd bf16x3, cfg 74 -> Winograd second, cfg 68": 30,
        "Winograd bf16x3, cfg 74 -> Winograd second, cfg 69": 17,
        "Winograd bf16x3, cfg 92 -> Winograd second, cfg 91": 12,
        "Winograd third, cfg 68 -> Winograd second, cfg 68": 6,             # conv_in and the ragged layers bf16x3 leaves
        "Winograd third, cfg 69 -> Winograd second, cfg 69": 4,
    },
    "wino_bf16x3+wide": {
        "Winograd bf16x3, cfg 74 -> Winograd first, cfg 66": 56,
        "Winograd bf16x3, cfg 92 -> Winograd first, cfg 90": 12,
        "Winograd third, cfg 68 -> Winograd first, cfg 66": 6,
        "Winograd third, cfg 69 -> Winograd first, cfg 66": 4,
    },
    "ksplit": {                                                             # the tensors that finalise their consumer's GroupNorm
        "Winograd bf16x3, cfg 92 -> direct, cfg 16": 12,
        "Winograd first, cfg 90 -> direct, cfg 16": 1,
    },
    "pointwise_bf16x3": {                                                   # the riders go
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 22": 3,
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 24": 2,
        "pointwise bf16x3 (32 px), cfg 28 -> pointwise f32, cfg 20": 11,
        "pointwise bf16x3 (64 px), cfg 28 -> pointwise f32, cfg 20": 6,
        "pointwise bf16x3 (K-split), cfg 28 -> direct, cfg 22": 8,
        "pointwise bf16x3 (K-split), cfg 28 -> pointwise f32, cfg 20": 6,
        "pointwise bf16x3 (staged K-split), cfg 28 -> pointwise f32, cfg 20": 4,
        "pointwise bf16x3 (staged), cfg 28 -> pointwise f32, cfg 20": 1,
    },
    "pointwise_bf16x3+pointwise": {
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 22": 3,
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 24": 10,
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 25": 3,
        "pointwise bf16x3 (64 px), cfg 28 -> direct, cfg 24": 6,
        "pointwise bf16x3 (K-split), cfg 28 -> direct, cfg 22": 8,
        "pointwise bf16x3 (K-split), cfg 28 -> direct, cfg 25": 6,
        "pointwise bf16x3 (staged K-split), cfg 28 -> direct, cfg 25": 4,
        "pointwise bf16x3 (staged), cfg 28 -> direct, cfg 25": 1,
    },
    "pointwise_ksplit": {
        "pointwise bf16x3 (K-split), cfg 28 -> pointwise bf16x3 (32 px), cfg 28": 14,
        "pointwise bf16x3 (staged K-split), cfg 28 -> pointwise bf16x3 (32 px), cfg 28": 4,
    },
    "s2_bf16x3": {                                                          # (three of these are the classifier's rows: see plan_record)
        "stride-2 bf16x3, cfg 36 -> direct, cfg 11": 3,
        "stride-2 bf16x3, cfg 36 -> direct, cfg 12": 5,
        "stride-2 bf16x3, cfg 36 -> direct, cfg 18": 7,
    },
    "pointwise_staged_ksplit": {                                            # only at batch 64
        "pointwise bf16x3 (staged K-split), cfg 28 -> pointwise bf16x3 (K-split), cfg 28": 4,
    },
    "winograd": {},
    "all_off": {
        "Winograd bf16x3, cfg 74 -> Winograd first, cfg 66": 56,
        "Winograd bf16x3, cfg 92 -> direct, cfg 16": 12,
        "Winograd first, cfg 90 -> direct, cfg 16": 1,
        "Winograd third, cfg 68 -> Winograd first, cfg 66": 6,
        "Winograd third, cfg 69 -> Winograd first, cfg 66": 4,
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 22": 3,
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 24": 10,
        "pointwise bf16x3 (32 px), cfg 28 -> direct, cfg 25": 3,
        "pointwise bf16x3 (64 px), cfg 28 -> direct, cfg 24": 6,
        "pointwise bf16x3 (K-split), cfg 28 -> direct, cfg 22": 8,
        "pointwise bf16x3 (K-split), cfg 28 -> direct, cfg 25": 6,
        "pointwise bf16x3 (staged K-split), cfg 28 -> direct, cfg 25": 4,
        "pointwise bf16x3 (staged), cfg 28 -> direct, cfg 25": 1,
        "stride-2 bf16x3, cfg 36 -> direct, cfg 11": 3,
        "stride-2 bf16x3, cfg 36 -> direct, cfg 12": 5,
        "stride-2 bf16x3, cfg 36 -> direct, cfg 18": 7,
    },
}
# the same count over the whole record (RECORD_SHAPES: the ragged 3x40x56 as well)
RECORD_TOTALS = {"wino_bf16x3": 71, "wino_bf16x3+col": 92, "wino_bf16x3+wide": 92, "ksplit": 16, "pointwise_bf16x3": 43,
                 "pointwise_bf16x3+pointwise": 43, "pointwise_ksplit": 18, "s2_bf16x3": 18, "pointwise_staged_ksplit": 4, "winograd": 0,
                 "all_off": 154}

UNET_KW = dict(sample_size=128, in_channels=3, out_channels=3, layers_per_block=2, block_out_channels=(64, 128, 256, 256),
               down_block_types=("DownBlock2D", "DownBlock2D", "AttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "AttnUpBlock2D", "UpBlock2D", "UpBlock2D"), class_embed_type=None)

CLF_TARGET = 5
CLF_TRAIN_CASE = (True, 2, 32, 32)              # the smallest of clf_train_ref.CASES
CLF_BN_CASE = (True, 4, 32, 32, 1)              # the smallest gradient case of clf_bn_ref.CASES


def set_env(name, base=None):
    """the environment of a set's child: the parent's own copies of all ten variables removed, the set's added as "0"
    (name None: no switch set)"""
    env = dict(os.environ if base is None else base)
    for v in SWITCHES:
        env.pop(v, None)
    for v in (SETS[name] if name is not None else ()):
        env[v] = "0"
    return env


# ---------------------------------------------------------------- the record of plans (host only)
def classifier_convs():
    """(what, cin, cout, H, ksize, stride) of the classifier's distinct convolutions at 224 x 224"""
    out = [("7x7 3->64 stride 2 @224", 3, 64, 224, 7, 2)]
    h, cin = 56, 64
    for layer, cout in enumerate((64, 128, 256, 512)):
        if layer:
            out.append((f"3x3 {cin}->{cout} stride 2 @{h}", cin, cout, h, 3, 2))
            out.append((f"1x1 {cin}->{cout} stride 2 @{h}", cin, cout, h, 1, 2))
            h //= 2
        out.append((f"3x3 {cout}->{cout} @{h}", cout, cout, h, 3, 1))
        cin = cout
    return out


def plan_record():
    """{"BxHxW": [[plane + convolution, plan], ...] in execution order, ..., "classifier": [...]}: every forward convolution of the
    reference architecture at RECORD_SHAPES as Fwd::run issues them, and the classifier's at 2x224x224, each put to
    sisic_conv_plan_info.  (The classifier's rows are planned as tools/arch_plan_table.plan plans a convolution: a stride-2 3x3
    row carries a split filter.  resnet.cpp builds none for its three downsampling 3x3 convolutions, so those three rows say what
    sisic_conv2d does for a caller who passes one; the classifier itself runs them on the direct kernel either way.)"""
    import arch_plan_table as apt
    from synt_isic_amd.arch import UNetConfig
    rec = OrderedDict()
    for B, H, W in RECORD_SHAPES:
        rows = []
        for lvl, convs in apt.walk(UNetConfig(), B, H, W).items():
            rows += [[f"{H >> lvl}x{W >> lvl} {what}", p] for what, p in convs]
        rec[f"{B}x{H}x{W}"] = rows
    rec["classifier"] = [[what, apt.plan(2, cin, 0, cout, h, h, k, stride=stride)] for what, cin, cout, h, k, stride in classifier_convs()]
    return rec


def transitions(default, other, keys=None):
    """Counter{"default plan -> fallback plan": n} over the distinct (shape, plane, convolution) entries whose plan differs"""
    out = Counter()
    for key in (keys if keys is not None else default):
        assert [w for w, _ in default[key]] == [w for w, _ in other[key]], key
        for what, a, b in {(w, a, b) for (w, a), (_, b) in zip(default[key], other[key]) if a != b}:
            out[f"{a} -> {b}"] += 1
    return out


def table_keys():
    return [f"{B}x{H}x{W}" for B, H, W in TABLE_SHAPES] + ["classifier"]


# ---------------------------------------------------------------- the inputs (shared with the parent's float64 references)
def unet_inputs():
    """every UNet input of the workload, CPU tensors"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "unet_forward_b2_64.npz"))
    inp = {"x64": torch.from_numpy(gold["x"]), "t64": torch.from_numpy(gold["t"]),
           "x72": torch.randn(1, 3, 72, 40, generator=torch.Generator().manual_seed(7240)), "t72": torch.tensor([321]),
           "x40": torch.randn(3, 3, 40, 56, generator=torch.Generator().manual_seed(4056)), "t40": torch.tensor([0, 500, 999])}
    # the batch of test_gpu_train.py's ``batch`` fixture, and its ragged case
    g = torch.Generator().manual_seed(77)
    inp["train64"] = ((torch.rand(2, 3, 64, 64, generator=g) * 2 - 1), torch.randn(2, 3, 64, 64, generator=g), torch.tensor([37, 912]))
    g = torch.Generator().manual_seed(78)
    inp["train40"] = (torch.rand(3, 3, 40, 56, generator=g) * 2 - 1, torch.randn(3, 3, 40, 56, generator=g), torch.tensor([0, 500, 999]))
    return inp


def classifier_input():
    """the 2x64x64 batch of test_gpu_classifier.py's input-gradient test"""
    return torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(100 + 64)) * 1.6 - 0.8


def _flat(named) -> np.ndarray:
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in named.values()])


# ---------------------------------------------------------------- the workload
def run(outdir: str, b64: bool = False) -> None:
    import pytest
    import poison
    poison.install(pytest.MonkeyPatch())          # before anything allocates
    import clf_bn_ref
    import clf_train_ref
    from oracle import resnet18 as ores
    from synt_isic_amd import _lib, ops
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.sampler import Sampler
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipClassifierAdam, mse_loss
    from synt_isic_amd.unet import HipUNet2DModel
    from synt_isic_amd.weights import synthetic_resnet18_state_dict, synthetic_unet_state_dict

    t_start = time.perf_counter()
    unwritten = OrderedDict()

    def save(name, t):
        if torch.is_tensor(t):
            if t.dtype in (torch.float32, torch.float64):
                unwritten[name] = poison.unwritten(t)
            t = t.detach().cpu().numpy()
        np.save(os.path.join(outdir, name + ".npy"), np.asarray(t))

    with open(os.path.join(outdir, "plans.json"), "w") as f:
        json.dump(plan_record(), f)

    sd = synthetic_unet_state_dict()
    inp = unet_inputs()

    def new_model():
        m = HipUNet2DModel(**UNET_KW)
        m.load_state_dict(sd)
        return m.to(torch.device(DEV))

    # ---- UNet forward, default and latency mode, whole and ragged tiles; a batch of one
    model = new_model().eval()
    x64, x72, x40 = inp["x64"].to(DEV), inp["x72"].to(DEV), inp["x40"].to(DEV)
    for mode in ("default", "latency"):
        model.set_latency_mode(mode == "latency")
        y64 = model(x64, inp["t64"]).sample
        save(f"unet_{mode}_b2_64", y64)
        save(f"unet_{mode}_b1_72x40", model(x72, 321).sample)
        save(f"unet_{mode}_b3_40x56", model(x40, inp["t40"]).sample)
        one = model(x64[:1].contiguous(), inp["t64"][:1]).sample
        save(f"unet_{mode}_row0_as_batch_of_one", one)
        save(f"unet_{mode}_row0_equal", np.int64(torch.equal(one[0], y64[0])))
    model.set_latency_mode(False)
    # launches in the Winograd profile slots over one forward (SISIC_WINOGRAD=0 shows in no plan: the executor withholds the filters)
    torch.cuda.synchronize()
    ops.profile_enable(DEV, True)
    try:
        ops.profile_reset(DEV)
        model(x64, inp["t64"])
        torch.cuda.synchronize()
        prof = ops.profile_read(DEV)
    finally:
        ops.profile_enable(DEV, False)
    with open(os.path.join(outdir, "profile_launches.json"), "w") as f:
        json.dump({k: v["launches"] for k, v in prof.items()}, f)
    if b64:
        xb = torch.randn(64, 3, 64, 64, generator=torch.Generator().manual_seed(6464)).to(DEV)
        save("unet_default_b64_64", model(xb, 500).sample)
        del xb
    del model

    # ---- UNet training: loss, prediction, the 330 gradients; a second forward/backward; the eval() forward of the same input
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    for tag, key, latency in (("b2_64", "train64", False), ("b3_40x56", "train40", False), ("b2_64_latency", "train64", True)):
        images, noise, timesteps = (t.to(DEV) for t in inp[key])
        model = new_model().set_latency_mode(latency)
        opt = HipAdam(model, lr=1e-4)
        model.train()
        noisy = sched.add_noise(images, noise, timesteps)
        pred = model(noisy, timesteps).sample
        loss = mse_loss(pred, noise)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        grads = model.grads()
        save(f"train_{tag}_noisy", noisy)
        save(f"train_{tag}_pred", pred)
        save(f"train_{tag}_loss", np.float64(loss.item()))
        save(f"train_{tag}_grads", torch.from_numpy(_flat(grads)))
        with open(os.path.join(outdir, f"train_{tag}_grad_names.json"), "w") as f:
            json.dump([[n, list(g.shape)] for n, g in grads.items()], f)
        pred2 = model(noisy, timesteps).sample
        mse_loss(pred2, noise).backward()
        again = model.grads()
        save(f"train_{tag}_second_backward_equal", np.int64(torch.equal(pred2, pred) and list(again) == list(grads)
                                                            and all(torch.equal(again[n], grads[n]) for n in grads)))
        model.eval()
        ev = model(noisy, timesteps).sample
        save(f"train_{tag}_eval_forward", ev)
        save(f"train_{tag}_tape_forward_is_the_forward", np.int64(torch.equal(ev, pred)))
        del opt, model

    # ---- UNet sampling: eight steps of the fused loop under two rules; one image through the captured step
    s = Sampler(DEV)
    s.add_model("NV", sd)
    for rule, kw in (("ddpm", {}), ("dpmpp_device", dict(scheduler="dpmsolver++", noise="device"))):
        res = s.generate_seeds("NV", [0, 1], T=8, size=(32, 32), return_trajectory=True, **kw)
        save(f"sample_{rule}_latents", res.latents)
        save(f"sample_{rule}_trajectory", res.trajectory)
    del s
    s = Sampler(DEV, latency_mode=True)
    m = s.add_model("NV", sd)
    first = s.generate_seeds("NV", [3], T=8, size=(32, 32)).latents
    second = s.generate_seeds("NV", [3], T=8, size=(32, 32)).latents
    save("sample_latency_latents", first)
    save("sample_latency_two_calls_equal", np.int64(torch.equal(first, second)))
    save("sample_latency_graph_builds", np.int64(_lib.load().sisic_unet_graph_builds(m.handle)))
    del s, m

    # ---- the classifier: logits, input gradient, Grad-CAM; one loss_backward with frozen BatchNorm, one with batch statistics
    csd = synthetic_resnet18_state_dict()

    def new_clf():
        c = HipMelanomaClassifier(num_classes=7, pretrained=False)
        c.load_state_dict(csd)
        return c.to(DEV).eval()

    clf = new_clf()
    xc = classifier_input().to(DEV)
    save("clf_logits", clf(xc))
    grad, logits = clf.input_gradient(xc, CLF_TARGET)
    save("clf_input_gradient", grad)
    save("clf_input_gradient_logits", logits)
    save("clf_stem", clf.stem_activation(xc))     # the max-pool routes of the replayed reference (test_gpu_classifier.py)
    cam, logits = clf.grad_cam(xc, CLF_TARGET)
    save("clf_grad_cam", cam)
    save("clf_grad_cam_logits", logits)

    x, labels, w = clf_train_ref.inputs(CLF_TRAIN_CASE)
    opt = HipClassifierAdam(clf)
    loss, logits = clf.loss_backward(x, labels, class_weights=w, preprocessed=True)
    save("clf_train_loss", np.float64(loss))
    save("clf_train_logits", logits)
    save("clf_train_grads", torch.from_numpy(_flat(clf.grads())))
    # the stem activation the max-pool routes of the float64 reference are taken from (sisic_resnet_stem)
    import ctypes as C
    xd = x.to(DEV).float().contiguous()
    stem = ops.empty((xd.shape[0], 64, xd.shape[2] // 2, xd.shape[3] // 2), dtype=torch.float32, device=xd.device)
    _lib.check(_lib.load().sisic_resnet_stem(clf.handle, xd.data_ptr(), stem.data_ptr(), xd.shape[0], xd.shape[2], xd.shape[3], 0,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    save("clf_train_stem", stem)
    opt.close()
    del clf, opt

    clf = new_clf()
    x, labels, w = clf_bn_ref.inputs(CLF_BN_CASE)
    opt = HipClassifierAdam(clf, batchnorm="batch", bn_momentum=clf_bn_ref.MOMENTUM)
    loss, logits = clf.loss_backward(x, labels, class_weights=w, preprocessed=True)
    save("clf_bn_loss", np.float64(loss))
    save("clf_bn_logits", logits)
    save("clf_bn_grads", torch.from_numpy(_flat(clf.grads())))
    save("clf_bn_running", torch.from_numpy(_flat(OrderedDict((k, clf.read_tensor(0, k)) for k in clf_bn_ref.buffer_names(csd)))))
    # the training-mode stem by the library's own launches (test_gpu_clf_bn.py::_train_stem)
    y = ops.conv2d(x.to(DEV).float().contiguous(), ops.pack_conv_weight(csd["model.conv1.weight"].float().to(DEV).contiguous()), 64, 7, stride=2)
    stem, _, _ = ops.batchnorm_train(y, csd["model.bn1.weight"].float().to(DEV).contiguous(), csd["model.bn1.bias"].float().to(DEV).contiguous(),
                                     eps=ores.BN_EPS, relu=True)
    save("clf_bn_stem", stem)
    opt.close()
    del clf, opt

    torch.cuda.synchronize()
    poison.check()                                # every guard band of every allocation still holds the pattern
    with open(os.path.join(outdir, "unwritten.json"), "w") as f:
        json.dump(unwritten, f)
    with open(os.path.join(outdir, "seconds.json"), "w") as f:
        json.dump({"workload": time.perf_counter() - t_start}, f)


if __name__ == "__main__":
    if sys.argv[1] == "--plans":
        print(json.dumps(plan_record()))
    else:
        run(sys.argv[1], b64="--b64" in sys.argv[2:])
