"""Plain torch restatement of what training the ResNet18 classifier with frozen BatchNorm computes (imported by
test_clf_train_cpu.py and test_gpu_clf_train.py, as optim_ext_ref / xai_ref are by theirs).

    loss_and_grads       cross-entropy and its 22 gradients by torch.autograd over oracle/resnet18.py::resnet18_features
                         (eval-mode F.batch_norm: BatchNorm frozen), the state-dict tensors as leaves, float64 or float32
    cross_entropy        the loss written out: sum_b w[y_b] (lse_b - z[b, y_b]) / sum_b w[y_b]
    bn_scale             gamma / sqrt(var + eps) of the BatchNorm behind a convolution, in float64 (the fold of the library)
    adam_step            torch.optim.Adam's single-tensor update written out, in the tensors' dtype
    stem_activation      the stem's fp32 activation (what the CPU suite routes the max-pool by)
    rel_err, bar         the measure and the bound of the gradient tests
    CASES, inputs        the shapes and the seeded inputs of the GPU gradient tests
    plant= ...           two planted errors (the CPU suite shows each far over the bar on those inputs):
                           "unscaled"       the BatchNorm scale left off the weight gradient (the gradient of the FOLDED filter)
                           "no_downsample"  the downsample branch's contribution to the block-input gradient dropped
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import resnet18 as ores

NUM_CLASSES = 7
# (preprocessed, B, H, W): planes down to 1x1, a non-square stem, every border of the 7x7 kernel; then the sampler's latents
# resized to 224x224: planes 112 .. 7, the Winograd weight gradient on an odd plane
CASES = [(True, 2, 32, 32), (True, 3, 64, 96), (False, 2, 64, 64)]
GRAD_FLOOR = 1e-5          # the project's cross-kernel parity bound
GRAD_MARGIN = 16.0         # a different summation order through 17 layers, over torch-fp32's own distance from float64


def trainable_names(sd):
    """the 22 tensors a step moves, in state-dict order: 20 convolution weights, fc.weight, fc.bias"""
    return [k for k in sd if (k.endswith(".weight") and sd[k].dim() == 4) or k.startswith("model.fc.")]


def bn_name(conv_weight_name: str) -> str:
    """'model.layer2.0.downsample.0.weight' -> 'model.layer2.0.downsample.1', '...conv1.weight' -> '...bn1'"""
    base = conv_weight_name[:-len(".weight")]
    if base.endswith("downsample.0"):
        return base[:-1] + "1"
    return base[:-len("convN")] + "bn" + base[-1]


def bn_scale(sd, conv_weight_name: str) -> torch.Tensor:
    bn = bn_name(conv_weight_name)
    return sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + ores.BN_EPS)


def inputs(case):
    """(x, labels, class_weights or None) of a case, seeded by its shape; the second case carries class weights"""
    pre, B, H, W = case
    g = torch.Generator().manual_seed(7000 + 13 * H + W + B)
    if pre:
        x = torch.randn(B, 3, H, W, generator=g)                       # an already normalised network input
    else:
        x = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8            # latents in [-1, 1]
    labels = torch.randint(0, NUM_CLASSES, (B,), generator=g)
    weights = None
    if case == CASES[1]:
        weights = torch.rand(NUM_CLASSES, generator=g) * 2.0 + 0.25
    return x, labels, weights


def cross_entropy(logits, labels, weight=None):
    """F.cross_entropy(logits, labels, weight=weight, reduction="mean") written out"""
    lse = torch.logsumexp(logits, dim=1)
    picked = logits.gather(1, labels.view(-1, 1)).squeeze(1)
    w = torch.ones_like(lse) if weight is None else weight.to(logits.dtype)[labels]
    return (w * (lse - picked)).sum() / w.sum()


def _features_no_downsample_grad(sd, x, stem_override=None):
    """resnet18_features with the planted error: the downsample branch reads a detached copy of the block's input, so its
    share of the block-input gradient is missing (its own weight gradient is not)"""
    p = "model."
    x = F.conv2d(x, sd[p + "conv1.weight"], None, stride=2, padding=3)
    x = F.relu(ores._bn(sd, p + "bn1", x))
    if stem_override is not None:
        x = x + (stem_override.to(x.dtype) - x).detach()
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for l in range(4):
        for j in range(2):
            stride = 2 if (l > 0 and j == 0) else 1
            base = f"{p}layer{l + 1}.{j}"
            identity = x
            out = F.relu(ores._bn(sd, base + ".bn1", F.conv2d(x, sd[base + ".conv1.weight"], None, stride=stride, padding=1)))
            out = ores._bn(sd, base + ".bn2", F.conv2d(out, sd[base + ".conv2.weight"], None, stride=1, padding=1))
            if base + ".downsample.0.weight" in sd:
                identity = ores._bn(sd, base + ".downsample.1", F.conv2d(x.detach(), sd[base + ".downsample.0.weight"], None, stride=stride))
            x = F.relu(out + identity)
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    return F.linear(x, sd[p + "fc.weight"], sd[p + "fc.bias"])


def loss_and_grads(sd, x, labels, weight=None, dtype=torch.float64, preprocessed=True, stem_override=None, plant=None):
    """(loss, {name: d loss / d tensor} for the 22 trainable tensors, logits).  stem_override: the VALUES of the stem's
    activation to route the max-pool by (oracle/resnet18.py); plant: None or one of the planted errors above."""
    assert plant in (None, "unscaled", "no_downsample")
    params = OrderedDict((k, v.detach().to(dtype).clone()) for k, v in sd.items())
    names = trainable_names(sd)
    for k in names:
        params[k].requires_grad_(True)
    with torch.enable_grad():
        h = x.to(dtype)
        if not preprocessed:
            h = ores.preprocess_for_classifier(h)
        forward = _features_no_downsample_grad if plant == "no_downsample" else ores.resnet18_features
        logits = forward(params, h, stem_override=stem_override)
        loss = cross_entropy(logits, labels, None if weight is None else weight.to(dtype))
        grads = torch.autograd.grad(loss, [params[k] for k in names])
    out = OrderedDict((k, g.detach()) for k, g in zip(names, grads))
    if plant == "unscaled":
        for k in names:
            if out[k].dim() == 4:
                out[k] = out[k] / bn_scale(sd, k).to(dtype).view(-1, 1, 1, 1)
    return float(loss.detach()), out, logits.detach()


@torch.no_grad()
def stem_activation(sd, x, preprocessed=True) -> torch.Tensor:
    """relu(bn1(conv1(.))) in fp32: a stand-in for the library's stem activation where there is no GPU (the CPU suite routes
    the float64 and the float32 pass by the same values, as the GPU suite routes both by the library's)"""
    h = x.float() if preprocessed else ores.preprocess_for_classifier(x.float())
    return F.relu(ores._bn(sd, "model.bn1", F.conv2d(h, sd["model.conv1.weight"], None, stride=2, padding=3)))


def rel_err(g, g64) -> float:
    g64 = g64.double()
    return ((g.detach().cpu().double() - g64).abs().max() / g64.abs().max().clamp(min=1e-300)).item()


def bar(e32: float) -> float:
    return max(GRAD_FLOOR, GRAD_MARGIN * e32)


def adam_step(p, g, m, v, step: int, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update number ``step`` (>= 1) written out, in p's dtype; returns the new (p, m, v).  lr, betas and
    eps are Python doubles that meet the tensors as scalars, as in torch's single-tensor path."""
    b1, b2 = betas
    g = g.to(p.dtype)
    m = m.lerp(g, 1 - b1)
    v = v * b2 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v
