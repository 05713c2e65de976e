"""numpy restatement of the augmentation chain of sisic_augment (include/sisic.h) -- PIL's arithmetic written out -- and of the
rotation matrix code of ``data.draw_augment_params``: what tests/test_augment_cpu.py holds against PIL itself and against
tests/golden/augment.npz, and the GPU tests' description of the kernels.  Nothing here imports the package under test.
``pil_augment`` is the same chain through PIL (imported lazily: the fixture generator and the CPU test use it)."""
import math

import numpy as np

AUGMENT_DTYPE = np.dtype([("src", "<i4"), ("crop_x", "<i4"), ("crop_y", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"),
                          ("hflip", "<i4"), ("vflip", "<i4"), ("order", "<i4", (3,)), ("factor", "<f4", (3,)),
                          ("rotate", "<i4"), ("rot", "<i4", (6,)), ("reserved", "<i4", (4,))])
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
PRECISION_BITS = 22


def rotation_fixed(angle, H, W):
    """a0 .. a5 of Image.rotate(angle) for a W x H image: Image.rotate's matrix in Python floats, Geometry.c's FIX()."""
    angle = angle % 360.0
    rad = -math.radians(angle)
    m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))          # noqa: E731
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def make_record(src, H, W, box=None, hflip=0, vflip=0, order=(-1, -1, -1), factor=(1.0, 1.0, 1.0), angle=None):
    r = np.zeros((), dtype=AUGMENT_DTYPE)
    x, y, w, h = box if box is not None else (0, 0, W, H)
    r["src"], r["crop_x"], r["crop_y"], r["crop_w"], r["crop_h"] = src, x, y, w, h
    r["hflip"], r["vflip"] = hflip, vflip
    r["order"] = order
    r["factor"] = factor
    if angle is not None and angle % 360.0 != 0.0:
        r["rotate"] = 1
        r["rot"] = rotation_fixed(angle, H, W)
    return r


# ---- stage 1: img.crop(box).resize((W, H), BILINEAR) -----------------------------------------------------------------------
def resize_coeffs(n_in, n_out):
    """per output index: first tap, integer coefficients (at most three, 0 beyond the support); scale <= 1, support 1"""
    scale = n_in / n_out
    lo = np.zeros(n_out, dtype=np.int64)
    kk = np.zeros((n_out, 3), dtype=np.int64)
    for o in range(n_out):
        c = (o + 0.5) * scale
        xmin = max(int(c - 1.0 + 0.5), 0)
        xmax = min(int(c + 1.0 + 0.5), n_in)
        w = [max(0.0, 1.0 - abs(x - c + 0.5)) for x in range(xmin, xmax)]
        ww = sum(w)
        lo[o] = xmin
        for i, v in enumerate(w):
            kk[o, i] = int(v / ww * (1 << PRECISION_BITS) + 0.5)
    return lo, kk


def _resize_rows(a, n_out):
    """resample axis 0 of uint8 [n_in, ...] to n_out; a copy when the lengths agree"""
    n_in = a.shape[0]
    if n_in == n_out:
        return a.copy()
    lo, kk = resize_coeffs(n_in, n_out)
    out = np.empty((n_out,) + a.shape[1:], dtype=np.uint8)
    src = a.astype(np.int64)
    for o in range(n_out):
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for i in range(3):
            if kk[o, i]:
                acc += kk[o, i] * src[lo[o] + i]
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def crop_resize(img, box, H, W):
    x, y, w, h = box
    crop = img[y:y + h, x:x + w]
    horizontal = _resize_rows(crop.transpose(1, 0, 2), W).transpose(1, 0, 2)      # uint8 before the vertical pass
    return _resize_rows(horizontal, H)


# ---- stage 3 ------------------------------------------------------------------------------------------------------------------
def gray(img):
    a = img.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.int64)


def blend(d, img, f):
    """Image.blend(degenerate, image, f) per band in float32: one multiply, one add, truncation"""
    d = np.broadcast_to(np.asarray(d, dtype=np.int64), img.shape)
    t = d.astype(np.float32) + np.float32(f) * (img.astype(np.int64) - d).astype(np.float32)
    assert t.dtype == np.float32
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int64))).astype(np.uint8)


def mean_gray(img):
    g = gray(img)
    return int(math.floor(int(g.sum()) / g.size + 0.5))


def colour(img, op, f):
    if op == BRIGHTNESS:
        return blend(0, img, f)
    if op == CONTRAST:
        return blend(mean_gray(img), img, f)
    if op == SATURATION:
        return blend(gray(img)[..., None], img, f)
    return img


# ---- stage 4 ------------------------------------------------------------------------------------------------------------------
def rotate_nearest(img, rot):
    H, W = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in rot)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    wrap = lambda v: ((v + (1 << 31)) % (1 << 32)) - (1 << 31)      # noqa: E731  (int32 accumulation)
    sx = wrap(a2 + y * a1 + x * a0) >> 16
    sy = wrap(a5 + y * a4 + x * a3) >> 16
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    out = np.zeros_like(img)
    out[inside] = img[sy[inside], sx[inside]]
    return out


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def augment_u8(images, rec):
    """uint8 [H,W,3]: what PIL returns for record ``rec`` on ``images[rec['src']]``"""
    img = np.asarray(images[int(rec["src"])])
    H, W = img.shape[:2]
    out = crop_resize(img, (int(rec["crop_x"]), int(rec["crop_y"]), int(rec["crop_w"]), int(rec["crop_h"])), H, W)
    if rec["hflip"]:
        out = out[:, ::-1]
    if rec["vflip"]:
        out = out[::-1]
    for op in rec["order"]:
        if op >= 0:
            out = colour(out, int(op), rec["factor"][int(op)])
    if rec["rotate"]:
        out = rotate_nearest(out, rec["rot"])
    return np.ascontiguousarray(out)


def normalize(u8_hwc):
    """ToTensor + Normalize(0.5, 0.5): float32 [3,H,W]"""
    x = u8_hwc.astype(np.float32) / np.float32(255.0)
    x = (x - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def pil_augment(images, rec, angle):
    """the same record through PIL, as torchvision's PIL backend calls it; ``angle`` is the rotation in degrees the record's
    fixed-point map was made from"""
    from PIL import Image, ImageEnhance
    img = np.asarray(images[int(rec["src"])])
    H, W = img.shape[:2]
    im = Image.fromarray(img, "RGB")
    x, y, w, h = int(rec["crop_x"]), int(rec["crop_y"]), int(rec["crop_w"]), int(rec["crop_h"])
    im = im.crop((x, y, x + w, y + h)).resize((W, H), Image.BILINEAR)
    if rec["hflip"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if rec["vflip"]:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    enhancers = {BRIGHTNESS: ImageEnhance.Brightness, CONTRAST: ImageEnhance.Contrast, SATURATION: ImageEnhance.Color}
    for op in rec["order"]:
        if op >= 0:
            im = enhancers[int(op)](im).enhance(float(rec["factor"][int(op)]))
    if rec["rotate"]:
        im = im.rotate(float(angle), Image.NEAREST, False, None, fillcolor=None)
    return np.asarray(im).copy()
