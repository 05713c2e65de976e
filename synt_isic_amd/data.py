"""The training script's data pipeline (diffusion/train_diffusion.py:19-50, :72-114) with the dataset in device memory.

The reference decodes, resizes and colour-corrects every image with PIL / numpy and then pushes every sample of every epoch
through a torchvision transform chain in one host worker.  Here the colour-corrected uint8 images of a class (at most 500 of
128x128x3: 24.6 MB) are uploaded once (``DeviceDataset``), the random parameters of an epoch are drawn on the host from
counter-based generators (``draw_augment_params``), and each batch is one small parameter upload and two kernel launches
(``DeviceLoader`` on ``ops.augment``).  For given parameters the kernels compute exactly what torchvision's PIL backend
does (include/sisic.h); the random stream is this module's own -- torchvision draws from torch's global generator, which
cannot be matched without it -- with torchvision's distributions.
"""
from __future__ import annotations

import itertools
import math
import os
from typing import Iterator, Sequence

import numpy as np
import torch

from . import ops
from .ops import AUGMENT_DTYPE

# gain / brightness / target mean per class id of enhance_color (train_diffusion.py:24-39; ids in the order of the
# ground-truth CSV's columns)
CLASS_COLOR_PARAMS = {
    0: {"gain": [1.04462, 0.8474, 0.7931], "brightness": 0.23741, "target": [0.7525, 0.5645, 0.5303]},
    1: {"gain": [1.0561, 0.86, 0.883], "brightness": 0.218, "target": [0.7453, 0.54, 0.5721]},
    2: {"gain": [1.125, 0.99, 0.922], "brightness": 0.262, "target": [0.784, 0.635, 0.573]},
    3: {"gain": [1.158, 0.952, 0.82], "brightness": 0.275, "target": [0.781, 0.618, 0.593]},
    4: {"gain": [1.1242, 0.846, 0.796], "brightness": 0.25, "target": [0.766, 0.574, 0.561]},
    5: {"gain": [1.0, 1.1, 1.1], "brightness": 0.23, "target": [0.79, 0.66, 0.66]},
    6: {"gain": [1.08, 1.05, 0.945], "brightness": 0.09, "target": [0.79, 0.64, 0.597]},
}


def enhance_color(img_u8_hwc, class_id: int) -> np.ndarray:
    """The per-class colour correction of train_diffusion.py:19-50 on a uint8 [H,W,3] image, in numpy float32 operation for
    operation: ``x = img / 255.0``, per channel ``clip(x + (target - mean(x)) * gain + brightness, 0, 1)``, then
    ``(x * 255).astype(uint8)``.  Runs on the host: once per image, at most 500 images."""
    if class_id not in CLASS_COLOR_PARAMS:
        raise ValueError(f"class_id {class_id}: one of {sorted(CLASS_COLOR_PARAMS)}")
    cp = CLASS_COLOR_PARAMS[class_id]
    x = np.array(img_u8_hwc, dtype=np.float32) / 255.0
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"enhance_color takes an [H,W,3] image, got {x.shape}")
    mean = np.mean(x, axis=(0, 1))
    for c in range(3):
        shift = cp["target"][c] - mean[c]
        x[..., c] = np.clip(x[..., c] + shift * cp["gain"][c] + cp["brightness"], 0, 1)
    return (x * 255).astype(np.uint8)


# ---- random parameters ------------------------------------------------------------------------------------------------------
_PERMUTATIONS = np.array(list(itertools.permutations(range(3))), dtype=np.int32)
_PERMUTATION_STREAM = 0xFFFFFFFF            # the "dataset index" whose generator shuffles an epoch
_DRAWS = 32                                 # uniforms taken from a sample's generator, in a fixed layout (below)
_CROP_ATTEMPTS = 10


def _generator(seed: int, epoch: int, index: int) -> np.random.Generator:
    """Philox keyed by (seed, epoch, dataset index): a stream of its own for every such triple."""
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in 0 .. 2**64-1")
    if not 0 <= epoch < 1 << 32 or not 0 <= index <= _PERMUTATION_STREAM:
        raise ValueError("epoch and dataset index must be in 0 .. 2**32-1")
    return np.random.Generator(np.random.Philox(key=np.array([seed, (epoch << 32) | index], dtype=np.uint64)))


class _KeyedUniforms:
    """``_generator(seed, epoch, index).random(n)`` for many indices: one Philox re-keyed in place (counter 0, empty buffer)
    instead of a new generator per sample -- the same numbers at a quarter of the cost."""

    def __init__(self, seed: int, epoch: int):
        _generator(seed, epoch, 0)                                   # range checks
        self._bits = np.random.Philox(key=np.zeros(2, dtype=np.uint64))
        self._gen = np.random.Generator(self._bits)
        self._state = self._bits.state
        self._state["state"]["key"][0] = seed
        self._high = epoch << 32

    def __call__(self, index: int, n: int) -> np.ndarray:
        if not 0 <= index < _PERMUTATION_STREAM:
            raise ValueError("dataset index must be in 0 .. 2**32-2")
        st = self._state
        st["state"]["key"][1] = self._high | index
        st["state"]["counter"][:] = 0
        st["buffer_pos"], st["has_uint32"], st["uinteger"] = 4, 0, 0
        self._bits.state = st
        return self._gen.random(n)


def epoch_permutation(n: int, epoch: int, seed: int) -> np.ndarray:
    """The order in which ``DeviceLoader(shuffle=True)`` visits ``n`` samples in ``epoch``."""
    return _generator(int(seed), int(epoch), _PERMUTATION_STREAM).permutation(n)


def rotation_fixed(angle: float, H: int, W: int):
    """PIL's 16.16 fixed-point inverse affine map (a0 .. a5) of ``Image.rotate(angle)`` about the centre of a W x H image:
    the matrix as ``PIL.Image.Image.rotate`` builds it in Python floats, converted as ``affine_fixed`` (Geometry.c) does.
    Returns None where PIL does not resample at all (angle % 360 == 0)."""
    angle = angle % 360.0
    if angle == 0.0:
        return None
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy

    def fix(v):
        return math.floor(v * 65536.0 + 0.5)
    out = (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))
    if any(abs(v) >= 1 << 31 for v in out):
        raise ValueError(f"a {W} x {H} image is too large for the 16.16 fixed-point rotation")
    return out


def identity_params(indices: Sequence[int], H: int, W: int) -> np.ndarray:
    """Records that leave the images as they are: full-image box, no flip, no colour operation, no rotation."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    p = np.zeros(len(idx), dtype=AUGMENT_DTYPE)
    p["src"] = idx
    p["crop_w"], p["crop_h"] = W, H
    p["order"] = -1
    p["factor"] = 1.0
    return p


def draw_augment_params(indices: Sequence[int], epoch: int, seed: int, H: int, W: int, *, scale=(0.9, 1.0),
                        ratio=(3.0 / 4.0, 4.0 / 3.0), brightness: float = 0.3, contrast: float = 0.3, saturation: float = 0.2,
                        degrees: float = 15.0, p_rotate: float = 0.5, hflip: bool = True, vflip: bool = True,
                        return_fallback: bool = False):
    """One ``ops.AUGMENT_DTYPE`` record (struct sisic_augment_params) per entry of ``indices`` for the transform chain of
    train_diffusion.py:72-81 at output size W x H; the defaults are the reference's values.

    Every sample draws from ``numpy.random.Generator(numpy.random.Philox(key=(seed, epoch << 32 | index)))``: its augmentation
    depends on (seed, epoch, dataset index) alone -- not on the batch size, its position in the batch or the shuffling -- the
    same contract as the sampler's device noise.  A sample takes 32 uniforms in a fixed layout whatever is switched off:
    twenty for the crop attempts, two for the crop position, two flips, the order, three factors, whether to rotate, the angle.

    Distributions are torchvision's.  RandomResizedCrop: up to 10 attempts of ``area * U(scale)``, ``exp(U(log ratio))``,
    ``w = round(sqrt(a * r))``, ``h = round(sqrt(a / r))``, accepted when ``0 < w <= W and 0 < h <= H``, then a uniform
    position; after 10 failures the central crop with the aspect clamped into ``ratio``.  Flips with probability 1/2 each.
    ColorJitter: factors ``U(1 - v, 1 + v)`` (lower end clamped at 0) applied in a uniformly drawn order; an operation whose
    ``v`` is 0 is skipped (order -1).  Rotation by ``U(-degrees, degrees)`` with probability ``p_rotate``, as PIL's
    fixed-point map (``rotation_fixed``).  The reference's ``RandomApply([CenterCrop(IMAGE_SIZE)], p=0.3)`` is the identity
    at the output size: it consumes no draw and has no field.

    ``return_fallback=True`` also returns a bool array marking the records whose crop is the fallback."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    n = len(idx)
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"output size {W} x {H}")
    if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
        raise ValueError(f"scale {scale} / ratio {ratio}: positive, ascending")
    seed, epoch = int(seed), int(epoch)
    u = np.empty((n, _DRAWS), dtype=np.float64)
    uniforms = _KeyedUniforms(seed, epoch)
    for k in range(n):
        u[k] = uniforms(int(idx[k]), _DRAWS)
    p = np.zeros(n, dtype=AUGMENT_DTYPE)
    p["src"] = idx

    # RandomResizedCrop.get_params
    area = float(H * W)
    target = area * (scale[0] + (scale[1] - scale[0]) * u[:, 0:2 * _CROP_ATTEMPTS:2])
    aspect = np.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * u[:, 1:2 * _CROP_ATTEMPTS:2])
    w_try = np.rint(np.sqrt(target * aspect)).astype(np.int64)
    h_try = np.rint(np.sqrt(target / aspect)).astype(np.int64)
    ok = (w_try > 0) & (w_try <= W) & (h_try > 0) & (h_try <= H)
    first = np.argmax(ok, axis=1)
    fallback = ~ok.any(axis=1)
    rows = np.arange(n)
    cw, ch = w_try[rows, first], h_try[rows, first]
    cy = np.minimum((u[:, 20] * (H - ch + 1)).astype(np.int64), H - ch)
    cx = np.minimum((u[:, 21] * (W - cw + 1)).astype(np.int64), W - cw)
    in_ratio = W / H
    if in_ratio < ratio[0]:
        fw, fh = W, int(round(W / ratio[0]))
    elif in_ratio > ratio[1]:
        fh = H
        fw = int(round(H * ratio[1]))
    else:
        fw, fh = W, H
    fw, fh = min(fw, W), min(fh, H)
    cw, ch = np.where(fallback, fw, cw), np.where(fallback, fh, ch)
    cx, cy = np.where(fallback, (W - fw) // 2, cx), np.where(fallback, (H - fh) // 2, cy)
    p["crop_x"], p["crop_y"], p["crop_w"], p["crop_h"] = cx, cy, cw, ch

    p["hflip"] = (u[:, 22] < 0.5) & bool(hflip)
    p["vflip"] = (u[:, 23] < 0.5) & bool(vflip)

    # ColorJitter
    order = _PERMUTATIONS[np.minimum((u[:, 24] * len(_PERMUTATIONS)).astype(np.int64), len(_PERMUTATIONS) - 1)].copy()
    for op, v in enumerate((brightness, contrast, saturation)):
        if v < 0:
            raise ValueError("brightness, contrast and saturation are non-negative")
        lo, hi = max(0.0, 1.0 - v), 1.0 + v
        p["factor"][:, op] = lo + (hi - lo) * u[:, 25 + op]
        if v == 0:
            order[order == op] = -1
    p["order"] = order

    # RandomApply([RandomRotation(degrees)], p_rotate)
    rotate = u[:, 28] < p_rotate
    angle = -degrees + 2.0 * degrees * u[:, 29]
    for k in np.nonzero(rotate)[0]:
        fixed = rotation_fixed(float(angle[k]), H, W)
        if fixed is not None:
            p["rotate"][k] = 1
            p["rot"][k] = fixed
    return (p, fallback) if return_fallback else p


# ---- the dataset in device memory -----------------------------------------------------------------------------------------
class DeviceDataset:
    """uint8 [N,H,W,3] images (numpy or torch), uploaded once; H and W multiples of 8.  ``labels``: one integer class label
    per image (a class-conditional model's ``class_labels``), kept on the device as int64; None: an unlabelled dataset."""

    def __init__(self, images_u8, device="cuda", labels=None):
        t = images_u8 if isinstance(images_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images_u8))
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] == 0:
            raise ValueError(f"images must be uint8 [N,H,W,3] with N > 0, got {t.dtype} {tuple(t.shape)}")
        if t.shape[1] % 8 or t.shape[2] % 8:
            raise ValueError(f"image height and width must be multiples of 8, got {t.shape[1]} x {t.shape[2]}")
        if labels is not None:
            lab = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels)
            if lab.dtype.is_floating_point or lab.dtype == torch.bool or lab.dim() != 1:
                raise ValueError(f"labels must be a 1-D integer array, got {lab.dtype} {tuple(lab.shape)}")
            if lab.shape[0] != t.shape[0]:
                raise ValueError(f"{lab.shape[0]} labels for {t.shape[0]} images")
            if lab.numel() and int(lab.min()) < 0:
                raise ValueError("labels must be non-negative")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DeviceDataset lives on an MI355X (torch device 'cuda'); got '{device}'. There is no CPU path.")
        self.images = t.contiguous().to(device)
        self.labels = None if labels is None else lab.to(torch.int64).contiguous().to(device)

    def __len__(self) -> int:
        return self.images.shape[0]

    @property
    def height(self) -> int:
        return self.images.shape[1]

    @property
    def width(self) -> int:
        return self.images.shape[2]

    @property
    def device(self) -> torch.device:
        return self.images.device

    @staticmethod
    def load_isic(image_dir: str, csv_path: str, class_id: int, image_size: int = 128, max_samples: int = 500) -> np.ndarray:
        """``SingleClassDataset.__init__`` / ``__getitem__`` of train_diffusion.py:85-112 up to and including enhance_color,
        on the host: uint8 [n, image_size, image_size, 3]."""
        try:
            import pandas as pd
            from PIL import Image
        except ImportError as e:
            raise ImportError(f"DeviceDataset.from_isic reads the ISIC CSV with pandas and decodes JPEGs with PIL ({e}); "
                              "install both, or decode elsewhere and pass uint8 [N,H,W,3] images to DeviceDataset") from e
        df = pd.read_csv(csv_path)
        classes = [c for c in df.columns if c != "image"]
        df["label"] = df[classes].values.argmax(axis=1)
        present = {f.split(".")[0] for f in os.listdir(image_dir) if f.endswith(".jpg")}
        df = df[df["image"].isin(present)].reset_index(drop=True)
        rows = df[df["label"] == class_id]
        if len(rows) == 0:
            raise ValueError(f"no image of class {class_id} in {image_dir}")
        rows = rows.sample(n=min(max_samples, len(rows)), random_state=42).reset_index(drop=True)
        out = np.empty((len(rows), image_size, image_size, 3), dtype=np.uint8)
        for k, name in enumerate(rows["image"]):
            img = Image.open(os.path.join(image_dir, name + ".jpg")).convert("RGB").resize((image_size, image_size))
            out[k] = enhance_color(np.asarray(img), class_id)
        return out

    @classmethod
    def from_isic(cls, image_dir: str, csv_path: str, class_id: int, image_size: int = 128, max_samples: int = 500,
                  device="cuda") -> "DeviceDataset":
        """The reference's per-class dataset (label = argmax over the non-``image`` columns, only files present,
        ``sample(n, random_state=42)``, ``convert("RGB").resize((s, s))``, ``enhance_color``), decoded once and uploaded."""
        return cls(cls.load_isic(image_dir, csv_path, class_id, image_size, max_samples), device)

    @classmethod
    def from_isic_classes(cls, image_dir: str, csv_path: str, class_ids: Sequence[int], image_size: int = 128,
                          max_samples: int = 500, device="cuda") -> "DeviceDataset":
        """One labelled dataset over several classes, for ``train.train_conditional``: ``load_isic`` per class (each with its
        own colour correction and at most ``max_samples`` images), concatenated in the order of ``class_ids``; an image's label
        is the POSITION of its class in ``class_ids``, so the labels run 0 .. len(class_ids) - 1 whatever the ids are."""
        class_ids = list(class_ids)
        if not class_ids or len(set(class_ids)) != len(class_ids):
            raise ValueError(f"class_ids must be a non-empty list of distinct class ids, got {class_ids}")
        parts = [cls.load_isic(image_dir, csv_path, cid, image_size, max_samples) for cid in class_ids]
        labels = np.concatenate([np.full(len(p), k, dtype=np.int64) for k, p in enumerate(parts)])
        return cls(np.concatenate(parts), device, labels=labels)


def epoch_batches(n: int, batch_size: int, epoch: int, seed: int, shuffle: bool = True, drop_last: bool = False):
    """The index batches of one epoch: every index once (``drop_last`` drops a ragged last batch)."""
    order = epoch_permutation(n, epoch, seed) if shuffle else np.arange(n)
    stop = n - n % batch_size if drop_last else n
    return [order[i:i + batch_size] for i in range(0, stop, batch_size)]


class DeviceLoader:
    """Batches of augmented images straight from a ``DeviceDataset``: each ``__iter__`` is one epoch (the epoch counter
    advances), each item a [B,3,H,W] fp32 device tensor in [-1,1] made by one non-blocking parameter upload and two launches
    on the current stream.  Shuffling and augmentation are functions of (seed, epoch, dataset index): the same seed gives the
    same epochs.  ``augment=False`` yields the images themselves, normalised, through the same kernels.  ``augment_kwargs``
    go to ``draw_augment_params``.  Drop-in for the DataLoader of ``train.train_class``.  Over a labelled dataset each item
    is ``(images, labels)``, the labels an int64 device tensor [B] in the batch's order (``train.train_conditional``)."""

    def __init__(self, dataset: DeviceDataset, batch_size: int, *, shuffle: bool = True, seed: int = 0, augment: bool = True,
                 drop_last: bool = False, **augment_kwargs):
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.dataset, self.batch_size, self.shuffle, self.seed = dataset, int(batch_size), bool(shuffle), int(seed)
        self.augment, self.drop_last, self.augment_kwargs = bool(augment), bool(drop_last), dict(augment_kwargs)
        self.epoch = 0
        draw_augment_params([], 0, self.seed, dataset.height, dataset.width, **self.augment_kwargs)      # refuse bad keywords now

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def epoch_params(self, epoch: int):
        """The parameter records of ``epoch``, one array per batch (what ``__iter__`` uploads)."""
        H, W = self.dataset.height, self.dataset.width
        batches = epoch_batches(len(self.dataset), self.batch_size, epoch, self.seed, self.shuffle, self.drop_last)
        if not batches:
            return []
        flat = np.concatenate(batches)
        params = draw_augment_params(flat, epoch, self.seed, H, W, **self.augment_kwargs) if self.augment \
            else identity_params(flat, H, W)
        return np.split(params, np.cumsum([len(b) for b in batches])[:-1])

    def __iter__(self) -> Iterator[torch.Tensor]:
        epoch = self.epoch
        self.epoch += 1
        labels = getattr(self.dataset, "labels", None)
        for params in self.epoch_params(epoch):
            images = ops.augment(self.dataset.images, params)
            if labels is None:
                yield images
            else:
                src = torch.from_numpy(np.ascontiguousarray(params["src"]).astype(np.int64)).to(labels.device)
                yield images, labels.index_select(0, src)
