"""HipMelanomaClassifier -- drop-in for ``MelanomaClassifierAdaptive`` (xai/XAI.py:357-471): forward, explanations, and
training with BatchNorm frozen or with batch statistics (``loss_backward`` here, ``HipClassifierAdam`` / ``train_classifier``
in train.py).

The reference wraps ``torchvision.models.resnet18`` (fc -> num_classes) and feeds it diffusion latents in
[-1,1] through ``preprocess_for_classifier`` (clamp, bilinear resize to 224x224, ImageNet normalisation).
Here the whole forward -- pre-processing, the BN-folded convolutions on the f32 MFMA kernel, pooling, fc and
the softmax/log scores -- runs in libsisic_hip.so (``sisic_resnet_forward`` / ``sisic_class_scores``).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Iterator

import torch

from . import _lib, ops
from ._lib import check
from ._module import HipModule
from .arch import resnet18_buffer_names, resnet18_param_spec, resnet18_trainable_names

NUM_CLASSES = 7                                     # xai/XAI.py:196 ISIC classes
CLASS_NAMES = ("MEL", "NV", "BCC", "AKIEC", "BKL", "DF", "VASC")
CLASSIFIER_IMAGE_SIZE = 224


class HipMelanomaClassifier(HipModule):
    _PREFIX, _NAME, _NO_CPU_PATH, _KEYS = "sisic_resnet", "HipMelanomaClassifier", "no CPU path", "classifier keys"

    def __init__(self, num_classes: int = NUM_CLASSES, architecture: str = "resnet18", pretrained: bool = False):
        if architecture not in ("resnet18", "auto"):
            raise NotImplementedError("only the built-in resnet18 architecture of the reference is implemented")
        if pretrained:
            raise NotImplementedError("IMAGENET1K_V1 weights are a network download (XAI.py:389); pass a "
                                      "state dict to load_state_dict instead")
        self.num_classes = num_classes
        self.architecture = "resnet18"
        super().__init__(resnet18_param_spec(num_classes))
        self._batches_tracked: "OrderedDict[str, torch.Tensor]" = OrderedDict()    # num_batches_tracked of the loaded dict, if any
        self._trainer = None            # the train.HipClassifierAdam that holds the library's training arenas, if any
        self.training = True

    # ---- module surface -------------------------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("train() does not switch BatchNorm to batch-statistics mode: training is entered through "
                                      "the optimizer object, train.HipClassifierAdam(clf, batchnorm='batch') for batch statistics "
                                      "(the default keeps BatchNorm frozen), and loss_backward")
        return self.eval()

    def parameters(self) -> Iterator[torch.Tensor]:
        self._sync_params()
        return (v for k, v in self._params.items() if "running_" not in k)

    def state_dict(self):
        """the weights as they stand: after ``HipClassifierAdam.step`` the trained tensors (read back from the library once).
        With BatchNorm frozen the BatchNorm tensors are unchanged; with batch statistics gamma, beta and the running statistics
        are the trained / updated ones, and the ``num_batches_tracked`` entries the loaded dict had (each behind its
        ``running_var``) have advanced by one per training forward."""
        self._sync_params()
        out = OrderedDict()
        for k, v in self._params.items():
            out[k] = v
            nbt = k[:-len("running_var")] + "num_batches_tracked"
            if k.endswith("running_var") and nbt in self._batches_tracked:
                out[nbt] = self._batches_tracked[nbt].clone()
        return out

    # ---- training (train.HipClassifierAdam owns train_begin / train_end) -------------------------------------------
    def trainable_names(self, batchnorm: str = "frozen"):
        """the tensors an optimizer step moves, in state-dict order: ``"frozen"`` the 20 convolution weights, fc.weight and
        fc.bias (22); ``"batch"`` the 20 BatchNorm gamma and 20 beta as well (62)"""
        return resnet18_trainable_names(self.num_classes, batchnorm)

    def _mode(self) -> str:
        """the BatchNorm mode of the optimizer that holds the training arenas ("frozen" without one)"""
        return self._trainer.batchnorm if self._trainer is not None else "frozen"

    def _stale_names(self):
        """what an optimizer step moves: the trainable tensors of the trainer's mode, and with batch statistics the buffers"""
        names = self.trainable_names(self._mode())
        return names + resnet18_buffer_names(self.num_classes) if self._mode() == "batch" else names

    def grads(self) -> "OrderedDict[str, torch.Tensor]":
        """the gradients of the last ``loss_backward`` (or ``set_grads``), CPU tensors under the state-dict names"""
        return OrderedDict((n, self.read_tensor(1, n)) for n in self.trainable_names(self._mode()))

    def set_grads(self, grads: Dict[str, torch.Tensor]) -> None:
        """gradients of the caller's choosing (optimizer parity tests): every trainable tensor must be given"""
        names = self.trainable_names(self._mode())
        missing = [n for n in names if n not in grads]
        if missing or len(grads) != len(names):
            raise ValueError(f"set_grads needs exactly the {len(names)} trainable tensors; missing {missing[:3]}")
        for n in names:
            self.write_tensor(1, n, grads[n])

    def loss_backward(self, images: torch.Tensor, labels, class_weights=None, preprocessed: bool = False):
        """``loss = F.cross_entropy(model(images), labels, weight=class_weights); loss.backward()`` in one library call
        (sisic_resnet_loss_backward): returns ``(loss, logits)``, the loss a float, the logits the forward's own bits.  The
        gradients replace those of the previous call (``grads()``).  Needs a ``train.HipClassifierAdam``; its ``batchnorm`` mode
        decides whether BatchNorm is frozen or uses (and updates) batch statistics, in which case the logits are the
        training-mode ones and the running statistics move by one update."""
        h = self.handle
        if images.device != self._device:
            images = images.to(self._device)
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"classifier input must be [B,3,H,W], got {tuple(images.shape)}")
        x = images.detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        lab = torch.as_tensor(labels).detach().to("cpu", torch.int64).contiguous()
        if lab.shape != (B,):
            raise ValueError(f"labels must be [{B}], got {tuple(lab.shape)}")
        cw = None
        if class_weights is not None:
            cw = torch.as_tensor(class_weights).detach().to("cpu", torch.float32).contiguous()
            if cw.shape != (self.num_classes,):
                raise ValueError(f"class_weights must be [{self.num_classes}], got {tuple(cw.shape)}")
        logits = ops.empty((B, self.num_classes), dtype=torch.float32, device=x.device)
        a = _lib.ResnetTrainArgs()
        a.x, a.logits_out = x.data_ptr(), logits.data_ptr()
        a.labels = C.cast(lab.data_ptr(), _lib.c_int64_p)
        a.class_weights = C.cast(cw.data_ptr(), _lib.c_float_p) if cw is not None else None
        a.B, a.H, a.W, a.preprocess = B, H, W, 0 if preprocessed else 1
        a.stream = torch.cuda.current_stream(x.device).cuda_stream
        check(_lib.load().sisic_resnet_loss_backward(h, C.byref(a)))
        if self._mode() == "batch":                      # the forward moved the running statistics
            self._params_stale = True
            for v in self._batches_tracked.values():
                v += 1
        return float(a.loss), logits

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """strict=False keeps only keys whose name AND shape match, like load_classifier_with_fallback
        (XAI.py:518-527).  Integer buffers (num_batches_tracked) do not reach the library; they are kept on the host, counted up by
        training forwards with batch statistics, and returned by ``state_dict()``."""
        sd = {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        tracked = OrderedDict((k, torch.as_tensor(v).detach().to("cpu", torch.int64).clone()) for k, v in state_dict.items()
                              if k.endswith("num_batches_tracked") and k[:-len("num_batches_tracked")] + "running_var" in self._spec)
        self._sync_params()
        cur = dict(self._params)
        new = OrderedDict()
        for name, shape in self._spec.items():
            t = sd.get(name)
            if t is not None and tuple(t.shape) == tuple(shape):
                new[name] = t.detach().to(device=self._device, dtype=torch.float32).contiguous().clone()
            elif strict:
                raise RuntimeError(f"Error(s) in loading state_dict for HipMelanomaClassifier: "
                                   f"{'missing key' if t is None else 'size mismatch for'} {name}")
            elif name in cur:
                new[name] = cur[name]
            else:
                raise RuntimeError(f"no value for {name} (non-strict load needs a previously loaded model)")
        if strict:
            extra = [k for k in sd if k not in self._spec]
            if extra:
                raise RuntimeError(f"unexpected keys in state_dict: {extra[:5]}")
        self._batches_tracked = tracked
        self._set_params(new)
        return self

    # ---- library handle (the shell's hooks) -----------------------------------------------------
    def _create_handle(self) -> None:
        h = C.c_void_p()
        check(_lib.load().sisic_resnet_create(ops.context(self._device), self.num_classes, C.byref(h)))
        self._handle = h

    def _drop_trainer(self) -> None:
        if self._trainer is not None:
            self._trainer._active = False
            self._trainer = None

    _after_upload = _before_release = _drop_trainer          # a reload ends training in the library, and so does a move

    # ---- weight randomisation (the sanity check of xai/XAI.py:2043-2098) ---------------------------
    RANDOMIZE_TAG0 = 16          # device-noise tag of tensor k: 16 + k (include/sisic.h)

    def randomize_weights(self, seed: int, trial: int, strength: float = 0.01) -> None:
        """``param.data = randn_like(param) * strength`` for every parameter with more than one dimension (XAI.py:2056-2059), on
        the device (sisic_resnet_randomize): tensor k holds ``noise_fill([seed], numel, trial, tag=16 + k) * strength``, a
        function of (seed, trial, strength) alone.  ``state_dict()`` keeps returning the loaded weights; ``restore_weights()``
        brings them back."""
        seed = int(seed)
        if seed < 0 or seed >> 64:
            raise ValueError("seed must be an integer in 0 .. 2**64-1")
        h = self.handle
        check(_lib.load().sisic_resnet_randomize(h, seed, int(trial), float(strength),
                                                 C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)))

    def restore_weights(self) -> None:
        """the filters of the loaded state dict again, bit for bit (sisic_resnet_restore)"""
        h = self.handle
        check(_lib.load().sisic_resnet_restore(h, C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)))

    def randomized_state_dict(self, seed: int, trial: int, strength: float = 0.01) -> "OrderedDict[str, torch.Tensor]":
        """The state dict the device holds after ``randomize_weights(seed, trial, strength)``, built with ``ops.noise_fill``:
        loading it into another classifier gives the same filters (tests, the oracle)."""
        order = self._tensor_index()
        out = OrderedDict()
        for name, value in self._params.items():
            if value.dim() > 1:
                z = ops.noise_fill([seed], value.numel(), int(trial), tag=self.RANDOMIZE_TAG0 + order[name], device=self._device)
                out[name] = (z[0] * torch.tensor(float(strength), dtype=torch.float32, device=z.device)).view(value.shape)
            else:
                out[name] = value.clone()
        return out

    # ---- forward --------------------------------------------------------------------------------
    # Frames per library call.  The callers in xai.py hand over whole trajectories (N frames = N inference steps, up to
    # 1000) and coalition sets; the library's activation workspace scales with the batch of a call (stem output:
    # 3.2 MB per image, the backward passes keep every block's activations), so the batch of one call is capped and
    # longer inputs are walked in chunks.  Rows do not depend on the chunking (no kernel choice depends on the batch).
    max_forward_batch = 512
    max_backward_batch = 128

    @staticmethod
    def _chunks(total: int, cap: int):
        lo = 0
        while lo < total:
            n = min(cap, total - lo)
            yield lo, n
            lo += n

    def workspace_bytes(self) -> int:
        """activation workspace the library keeps for this model (released when the input shape changes)"""
        return int(_lib.load().sisic_resnet_workspace_bytes(self._handle)) if self._handle is not None else 0

    @torch.no_grad()
    def forward(self, x: torch.Tensor, preprocessed: bool = False) -> torch.Tensor:
        """logits [B,num_classes].  x: [B,3,H,W] in [-1,1] (H,W <= 224); it is moved to the model's device like
        preprocess_for_classifier does (XAI.py:407-409)."""
        h = self.handle
        if x.device != self._device:
            x = x.to(self._device)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"classifier input must be [B,3,H,W], got {tuple(x.shape)}")
        x = x.to(torch.float32).contiguous()
        B, _, H, W = x.shape
        out = ops.empty((B, self.num_classes), dtype=torch.float32, device=x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        for lo, n in self._chunks(B, self.max_forward_batch):
            check(_lib.load().sisic_resnet_forward(h, x[lo:].data_ptr(), out[lo:].data_ptr(), n, H, W,
                                                   0 if preprocessed else 1, stream))
        return out

    __call__ = forward

    FEATURE_DIM = 512

    @torch.no_grad()
    def features(self, x: torch.Tensor, preprocessed: bool = False) -> torch.Tensor:
        """The pooled features [B,512]: ``forward`` up to and including ``AdaptiveAvgPool2d(1)`` (sisic_resnet_features), what
        the final Linear reads.  ``x`` as for ``forward``; walked in chunks of ``max_forward_batch``, and a row does not depend
        on the chunking."""
        h = self.handle
        if x.device != self._device:
            x = x.to(self._device)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"classifier input must be [B,3,H,W], got {tuple(x.shape)}")
        x = x.to(torch.float32).contiguous()
        B, _, H, W = x.shape
        out = ops.empty((B, self.FEATURE_DIM), dtype=torch.float32, device=x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        for lo, n in self._chunks(B, self.max_forward_batch):
            a = _lib.ResnetFeaturesArgs(x=x[lo:].data_ptr(), out=out[lo:].data_ptr(), stream=stream, B=n, H=H, W=W,
                                        preprocess=0 if preprocessed else 1)
            check(_lib.load().sisic_resnet_features(h, C.byref(a)))
        return out

    def _scores(self, x: torch.Tensor, target_class: int):
        logits = self.forward(x)
        B = logits.shape[0]
        prob = ops.empty(B, dtype=torch.float32, device=logits.device)
        logscore = ops.empty_like(prob)
        check(_lib.load().sisic_class_scores(ops.context(logits.device), logits.data_ptr(), B, self.num_classes,
                                             int(target_class), prob.data_ptr(), logscore.data_ptr(),
                                             C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)))
        return prob, logscore

    def get_probabilities(self, x: torch.Tensor) -> torch.Tensor:
        """softmax over the 7 logits (XAI.py:438-441): [B,7]; assembled from the per-class score kernel."""
        logits = self.forward(x)
        cols = []
        for c in range(self.num_classes):
            p = ops.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
            check(_lib.load().sisic_class_scores(ops.context(logits.device), logits.data_ptr(), logits.shape[0],
                                                 self.num_classes, c, p.data_ptr(), None,
                                                 C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)))
            cols.append(p)
        return torch.stack(cols, dim=1)

    def get_per_class_score(self, x: torch.Tensor, target_class: int) -> torch.Tensor:
        """log(p(c|x) + 1e-8)   (XAI.py:443-459)."""
        return self._scores(x, target_class)[1]

    def get_confidence(self, x: torch.Tensor, target_class: int) -> torch.Tensor:
        """p(c|x)   (XAI.py:467-471)."""
        return self._scores(x, target_class)[0]

    @torch.no_grad()
    def stem_activation(self, x: torch.Tensor) -> torch.Tensor:
        """relu(bn1(conv1(preprocess(x)))) [B,64,112,112]: the tensor the stem's max-pool picks its arg-maxima from
        (sisic_resnet_stem; used by the parity tests of the backward pass)."""
        h = self.handle
        x = x.to(self._device).detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        out = ops.empty((B, 64, 112, 112), dtype=torch.float32, device=x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        for lo, n in self._chunks(B, self.max_forward_batch):
            check(_lib.load().sisic_resnet_stem(h, x[lo:].data_ptr(), out[lo:].data_ptr(), n, H, W, 1, stream))
        return out

    def input_gradient(self, x: torch.Tensor, target_class):
        """(d get_per_class_score / d x, logits): the gradient captum's IntegratedGradients and the plain-gradient
        fallback of XAI.py:1039-1109 take, through the pre-processing, with no autograd graph -- the transposed
        network runs on the same HIP convolution kernels (sisic_resnet_input_gradient).
        target_class: one class for every image, or a sequence / tensor of B classes, image b's own
        (sisic_resnet_input_gradient_targets: row b has the bits of the single-target call with its class)."""
        h = self.handle
        if x.device != self._device:
            x = x.to(self._device)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"classifier input must be [B,3,H,W], got {tuple(x.shape)}")
        x = x.detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        grad = ops.empty_like(x)
        logits = ops.empty((B, self.num_classes), dtype=torch.float32, device=x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        targets = None
        if isinstance(target_class, torch.Tensor) and target_class.dim() > 0:
            targets = [int(v) for v in target_class.tolist()]
        elif isinstance(target_class, (list, tuple)):
            targets = [int(v) for v in target_class]
        if targets is not None and len(targets) != B:
            raise ValueError(f"{len(targets)} target classes for a batch of {B}")
        for lo, n in self._chunks(B, self.max_backward_batch):
            if targets is None:
                check(_lib.load().sisic_resnet_input_gradient(h, x[lo:].data_ptr(), n, H, W, int(target_class),
                                                              grad[lo:].data_ptr(), logits[lo:].data_ptr(), stream))
            else:
                a = _lib.ResnetTargetsArgs(x=x[lo:].data_ptr(), targets=(C.c_int64 * n)(*targets[lo:lo + n]),
                                           grad_x=grad[lo:].data_ptr(), logits_out=logits[lo:].data_ptr(), stream=stream,
                                           B=n, H=H, W=W)
                check(_lib.load().sisic_resnet_input_gradient_targets(h, C.byref(a)))
        return grad, logits

    def grad_cam(self, x: torch.Tensor, target_class: int):
        """(cam [B,224,224] in [0,1], logits): pytorch_grad_cam's GradCAM on ``model.layer4[-1].conv2`` for the raw class
        logit, as xai/XAI.py:2945-3035 calls it on each trajectory frame (sisic_resnet_gradcam)."""
        h = self.handle
        if x.device != self._device:
            x = x.to(self._device)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"classifier input must be [B,3,H,W], got {tuple(x.shape)}")
        x = x.detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        cam = ops.empty((B, 224, 224), dtype=torch.float32, device=x.device)
        logits = ops.empty((B, self.num_classes), dtype=torch.float32, device=x.device)
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        for lo, n in self._chunks(B, self.max_backward_batch):
            check(_lib.load().sisic_resnet_gradcam(h, x[lo:].data_ptr(), n, H, W, int(target_class),
                                                   cam[lo:].data_ptr(), logits[lo:].data_ptr(), stream))
        return cam, logits

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        return torch.argmax(self.forward(x), dim=1)
