"""Plain torch restatement of what training the ResNet18 classifier with batch-statistics BatchNorm computes (imported by
test_clf_bn_cpu.py and test_gpu_clf_bn.py, as clf_train_ref is by its two files).

    features             oracle/resnet18.py::resnet18_features' structure with F.batch_norm(training=..., momentum=m); in eval mode
                         it IS that function, bit for bit (the CPU suite checks it)
    loss_grads_stats     cross-entropy, its 62 gradients (20 conv weights, 20 gamma, 20 beta, fc.weight, fc.bias) by torch.autograd
                         and the 40 running statistics after the forward's update, float64 or float32
    stem_activation      the stem's training-mode fp32 activation (what the CPU suite routes the max-pool by)
    bn_forward / bn_backward   one BatchNorm written out, for the kernel tests (float64 reference, fp32 yardstick)
    KERNEL_SHAPES, kernel_operands, OFFSET_*    the kernel tests' shapes and seeded operands
    CASES, inputs        the whole-model cases of the GPU gradient tests (every one under the conditioning cap E32_CAP)
    rel_err, bar         clf_train_ref's measure and bound: max|g - g64| / max|g64| <= max(1e-5, 16 * e32)
    plant= ...           planted errors (the CPU suite shows each at least 100 x over the bar on these inputs):
                           "no_xhat_term"    the -xhat * dgamma / n term dropped from the BatchNorm's dy
                           "biased_running"  the biased instead of the unbiased variance in the running update
                           "naive_moments"   (bn_forward) fp32 E[x^2] - E[x]^2 moments
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import clf_train_ref as ctr
from oracle import resnet18 as ores

NUM_CLASSES = ctr.NUM_CLASSES
MOMENTUM = 0.1
E32_CAP = 1e-4             # conditioning cap of a gradient case: fp32 torch's own distance from float64, every tensor

# (preprocessed, B, H, W, seed): seed None takes clf_train_ref.inputs (the second of those carries class weights), a number
# takes torch.randn from that seed.  Last planes of 4, 6 and 6 values per channel, then the sampler's latents at 224 x 224.
# Not used, measured over the cap: (True, 2, 32, 32, None) -- two values per channel at the last plane, ill-conditioned (3.5e-2
# on layer1.0.bn1.bias) -- and latents (3, 32, 32) from seed 9 (1.8e-2 on layer2.0.conv2.weight).
CASES = [(True, 4, 32, 32, 1), (True, 3, 32, 64, 1), (True, 3, 64, 96, None), (False, 2, 64, 64, None)]


def trainable_names(sd):
    """the 62 tensors a step moves in batch-statistics mode, in state-dict order"""
    return [k for k in sd if "running_" not in k and not k.endswith("num_batches_tracked")]


def buffer_names(sd):
    return [k for k in sd if "running_" in k]


def inputs(case):
    """(x, labels, class_weights or None) of a case"""
    pre, B, H, W, seed = case
    if seed is None:
        return ctr.inputs((pre, B, H, W))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g)
    labels = torch.randint(0, NUM_CLASSES, (B,), generator=g)
    return x, labels, None


class _BnNoXhatTerm(torch.autograd.Function):
    """training-mode BatchNorm whose backward drops the -xhat * dgamma / n term of dy (the planted error)"""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        mean = x.mean(dim=(0, 2, 3), keepdim=True)
        var = x.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        invstd = torch.rsqrt(var + eps)
        xhat = (x - mean) * invstd
        ctx.save_for_backward(xhat, invstd, gamma)
        return xhat * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        xhat, invstd, gamma = ctx.saved_tensors
        n = g.numel() // g.shape[1]
        dbeta = g.sum(dim=(0, 2, 3))
        dgamma = (g * xhat).sum(dim=(0, 2, 3))
        dx = gamma.view(1, -1, 1, 1) * invstd * (g - dbeta.view(1, -1, 1, 1) / n)
        return dx, dgamma, dbeta, None


def _bn(params, stats, name, x, training, momentum, plant):
    rm, rv = stats[f"{name}.running_mean"], stats[f"{name}.running_var"]
    w, b = params[f"{name}.weight"], params[f"{name}.bias"]
    if not training:
        return F.batch_norm(x, rm, rv, w, b, training=False, eps=ores.BN_EPS)
    if plant == "biased_running":
        with torch.no_grad():
            xd = x.detach()
            rm.copy_((1 - momentum) * rm + momentum * xd.mean(dim=(0, 2, 3)))
            rv.copy_((1 - momentum) * rv + momentum * xd.var(dim=(0, 2, 3), unbiased=False))
        return F.batch_norm(x, None, None, w, b, training=True, eps=ores.BN_EPS)
    if plant == "no_xhat_term":
        with torch.no_grad():
            F.batch_norm(x.detach(), rm, rv, None, None, training=True, momentum=momentum, eps=ores.BN_EPS)     # the update
        out = _BnNoXhatTerm.apply(x, w, b, ores.BN_EPS)
    else:
        out = F.batch_norm(x, rm, rv, w, b, training=True, momentum=momentum, eps=ores.BN_EPS)
    return out


def features(params, stats, x, training=True, momentum=MOMENTUM, stem_override=None, plant=None):
    """resnet18_features with every BatchNorm in training mode (``stats``, the 40 running statistics, are updated in place) or,
    with training=False, in eval mode.  stem_override: as in oracle/resnet18.py."""
    p = "model."
    bn = lambda name, t: _bn(params, stats, name, t, training, momentum, plant)     # noqa: E731
    x = F.conv2d(x, params[p + "conv1.weight"], None, stride=2, padding=3)
    x = F.relu(bn(p + "bn1", x))
    if stem_override is not None:
        x = x + (stem_override.to(x.dtype) - x).detach()
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for l in range(4):
        for j in range(2):
            stride = 2 if (l > 0 and j == 0) else 1
            base = f"{p}layer{l + 1}.{j}"
            identity = x
            out = F.conv2d(x, params[base + ".conv1.weight"], None, stride=stride, padding=1)
            out = F.relu(bn(base + ".bn1", out))
            out = F.conv2d(out, params[base + ".conv2.weight"], None, stride=1, padding=1)
            out = bn(base + ".bn2", out)
            if base + ".downsample.0.weight" in params:
                identity = F.conv2d(x, params[base + ".downsample.0.weight"], None, stride=stride)
                identity = bn(base + ".downsample.1", identity)
            x = F.relu(out + identity)
    x = F.adaptive_avg_pool2d(x, 1).flatten(1)
    return F.linear(x, params[p + "fc.weight"], params[p + "fc.bias"])


def loss_grads_stats(sd, x, labels, weight=None, dtype=torch.float64, preprocessed=True, stem_override=None,
                     momentum=MOMENTUM, plant=None):
    """(loss, {name: gradient} for the 62 trainable tensors, {name: value} for the 40 updated running statistics, logits)"""
    assert plant in (None, "no_xhat_term", "biased_running")
    names, buffers = trainable_names(sd), buffer_names(sd)
    params = OrderedDict((k, sd[k].detach().to(dtype).clone().requires_grad_(True)) for k in names)
    stats = OrderedDict((k, sd[k].detach().to(dtype).clone()) for k in buffers)
    with torch.enable_grad():
        h = x.to(dtype)
        if not preprocessed:
            h = ores.preprocess_for_classifier(h)
        logits = features(params, stats, h, True, momentum, stem_override, plant)
        loss = ctr.cross_entropy(logits, labels, None if weight is None else weight.to(dtype))
        grads = torch.autograd.grad(loss, [params[k] for k in names])
    return float(loss.detach()), OrderedDict((k, g.detach()) for k, g in zip(names, grads)), stats, logits.detach()


@torch.no_grad()
def stem_activation(sd, x, preprocessed=True) -> torch.Tensor:
    """relu(bn1(conv1(.))) with batch statistics in fp32: the stand-in for the library's stem activation where there is no GPU"""
    h = x.float() if preprocessed else ores.preprocess_for_classifier(x.float())
    y = F.conv2d(h, sd["model.conv1.weight"], None, stride=2, padding=3)
    return F.relu(F.batch_norm(y, None, None, sd["model.bn1.weight"], sd["model.bn1.bias"], training=True, eps=ores.BN_EPS))


rel_err = ctr.rel_err
bar = ctr.bar


# ---------------------------------------------------------------- one BatchNorm, for the kernel tests
# (B, C, HW).  The kernels deal a channel's planes to S = clamp(B*HW / 8192, 1, 2048 / C) workgroups (include/sisic.h, batchnorm.hip):
# the first four shapes are one slice per channel, (8, 64, 3136) is three (8 planes, 3 + 3 + 2), and (2, 8, 20000) -- planes longer
# than a 4096-float run, starting off a 16-byte boundary when the tensor is offset -- is four.
KERNEL_SHAPES = [(4, 512, 1), (3, 256, 2), (2, 64, 49), (2, 128, 196), (8, 64, 3136), (2, 8, 20000)]
KERNEL_SLICES = [1, 1, 1, 1, 3, 4]
# the offset-mean operands: per-channel mean OFFSET_MEAN * (1 + c / C) (30 .. 60), standard deviation OFFSET_STD.  At these values
# fp32 E[x^2] - E[x]^2 moments are 1.2e-1 from float64, 300 x over the case's bar of 3.9e-4 (test_clf_bn_cpu.py asserts 100 x).
OFFSET_SHAPE = (8, 64, 3136)
OFFSET_MEAN = 30.0
OFFSET_STD = 0.05


def kernel_operands(shape, seed=0, offset_mean=False):
    """(y, gamma, beta, residual, g, running_mean, running_var) of a kernel case, fp32"""
    B, C, HW = shape
    gen = torch.Generator().manual_seed(1000 * seed + 7 * C + HW + B)
    y = torch.randn(B, C, HW, generator=gen)
    if offset_mean:
        y = y * OFFSET_STD + OFFSET_MEAN * (1.0 + torch.arange(C).view(1, C, 1) / C)
    else:
        y = y * (0.5 + torch.rand(1, C, 1, generator=gen)) + torch.randn(1, C, 1, generator=gen)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=gen)
    beta = 0.3 * torch.randn(C, generator=gen)
    residual = torch.randn(B, C, HW, generator=gen)
    g = torch.randn(B, C, HW, generator=gen)
    rm = 0.1 * torch.randn(C, generator=gen)
    rv = 1.0 + 0.2 * torch.randn(C, generator=gen).abs()
    return y, gamma, beta, residual, g, rm, rv


def bn_forward(y, gamma, beta, eps=ores.BN_EPS, residual=None, relu=False, running=None, momentum=MOMENTUM, dtype=torch.float64,
               plant=None):
    """(out, mean, invstd, new running_mean, new running_var) of one training-mode BatchNorm over [B, C, HW] in ``dtype``"""
    assert plant in (None, "naive_moments")
    y = y.to(dtype)
    n = y.shape[0] * y.shape[2]
    if plant == "naive_moments":
        mean = y.sum(dim=(0, 2)) / n
        var = ((y * y).sum(dim=(0, 2)) / n - mean * mean).clamp(min=0)
    else:
        mean = y.mean(dim=(0, 2))
        var = y.var(dim=(0, 2), unbiased=False)
    invstd = torch.rsqrt(var + eps)
    out = (y - mean.view(1, -1, 1)) * invstd.view(1, -1, 1) * gamma.to(dtype).view(1, -1, 1) + beta.to(dtype).view(1, -1, 1)
    if residual is not None:
        out = out + residual.to(dtype)
    if relu:
        out = F.relu(out)
    rm = rv = None
    if running is not None:
        rm = (1 - momentum) * running[0].to(dtype) + momentum * mean
        rv = (1 - momentum) * running[1].to(dtype) + momentum * var * n / (n - 1)
    return out, mean, invstd, rm, rv


def bn_backward(g, y, gamma, eps=ores.BN_EPS, mask=None, dtype=torch.float64):
    """(dy, dgamma, dbeta) written out; mask (bool, or None): where the ReLU behind the BatchNorm let the gradient through"""
    g, y, gamma = g.to(dtype), y.to(dtype), gamma.to(dtype)
    if mask is not None:
        g = g * mask.to(dtype)
    n = y.shape[0] * y.shape[2]
    mean = y.mean(dim=(0, 2), keepdim=True)
    invstd = torch.rsqrt(y.var(dim=(0, 2), unbiased=False, keepdim=True) + eps)
    xhat = (y - mean) * invstd
    dbeta = g.sum(dim=(0, 2))
    dgamma = (g * xhat).sum(dim=(0, 2))
    dy = gamma.view(1, -1, 1) * invstd * (g - dbeta.view(1, -1, 1) / n - xhat * dgamma.view(1, -1, 1) / n)
    return dy, dgamma, dbeta
