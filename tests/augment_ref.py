"""numpy restatement of the training transform of seg18/dataset/Endovis2018_new.py:61-107, 145-182 (and the identical `_random_scale`
of segcata/dataset/CATA_new_512.py:115-152) on uint8 clips and labels: the reference of stswincl_amd.augment.ClipAugmenter.

It works on whole images, the way the reference does (resize everything, pad, crop, flip, value table, rotate, convert), where the
device works on the crop window with per-sample tables - the two share formulas, not code.  A parameter object `p` has the attributes
long_size, x1, y1, hflip, vflip, alpha, beta (both None: no value table) and angle (None: no rotation).

Pinned to a library:     BILINEAR resize (pil_resize_ref, equal to Pillow), NEAREST resize (nearest_index, equal to Pillow),
                         ImageOps.expand(fill=0), crop, the flips, `astype(float) / 255.`, the CaDIS normalisation.
Defined here, not pinned: the brightness/contrast table (value_table) and the rotation (rotate_tables / rotate) - albumentations and
                         cv2 are not available; the arithmetic follows cv2.warpAffine's fixed-point path."""
from __future__ import annotations

import math
import types

import numpy as np

import pil_resize_ref as pr

AB_BITS = 10            # fraction bits of the rotation's per-column / per-row position tables
INTER_BITS = 5          # fraction bits of a source position (1/32 pixel)


def P(long_size, x1, y1, hflip=False, vflip=False, alpha=None, beta=None, angle=None):
    return types.SimpleNamespace(long_size=long_size, x1=x1, y1=y1, hflip=hflip, vflip=vflip, alpha=alpha, beta=beta, angle=angle)


# --------------------------------------------------------------------------------------------- geometry (_random_scale)
def geometry(long_size: int, src_hw, crop_hw):
    """-> (ow, oh, padw, padh) as _random_scale derives them, its comparison of the short side with the crop WIDTH included."""
    (h, w), (crop_h, crop_w) = src_hw, crop_hw
    if h > w:
        oh = long_size
        ow = int(1.0 * w * long_size / h + 0.5)
        short = ow
    else:
        ow = long_size
        oh = int(1.0 * h * long_size / w + 0.5)
        short = oh
    padw = padh = 0
    if short < crop_w:
        padh = crop_h - oh if oh < crop_h else 0
        padw = crop_w - ow if ow < crop_w else 0
    return ow, oh, padw, padh


def draw_geometry(rng, base_w: int, src_hw, crop_hw):
    """The reference's three draws from a random.Random, in its order -> (long_size, x1, y1)."""
    long_size = rng.randint(int(base_w * 0.5), int(base_w * 2.0))
    ow, oh, padw, padh = geometry(long_size, src_hw, crop_hw)
    x1 = rng.randint(0, ow + padw - crop_hw[1])
    y1 = rng.randint(0, oh + padh - crop_hw[0])
    return long_size, x1, y1


def nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """Source index per output index of Pillow's NEAREST resize (libImaging ImagingScaleAffine): a float64 position that starts at
    scale / 2 and is advanced by `+= scale` per output pixel, truncated.  NOT floor((x + 0.5) * scale): the sums round differently."""
    scale = float(in_size) / out_size
    steps = np.full(out_size, scale, np.float64)
    steps[0] = scale * 0.5
    return np.add.accumulate(steps).astype(np.int64)


def resize_nearest(label: np.ndarray, H: int, W: int) -> np.ndarray:
    if label.shape == (H, W):
        return label.copy()
    return label[nearest_index(label.shape[0], H)[:, None], nearest_index(label.shape[1], W)[None, :]]


def _pad_crop_flip(a: np.ndarray, p, padw, padh, crop_hw) -> np.ndarray:
    canvas = np.zeros((a.shape[0] + padh, a.shape[1] + padw) + a.shape[2:], a.dtype)          # ImageOps.expand(border=(0, 0, padw, padh), fill=0)
    canvas[:a.shape[0], :a.shape[1]] = a
    if not (0 <= p.x1 <= canvas.shape[1] - crop_hw[1] and 0 <= p.y1 <= canvas.shape[0] - crop_hw[0]):
        raise ValueError(f"crop ({p.x1}, {p.y1}) outside the scaled image {canvas.shape[:2]}")
    a = canvas[p.y1:p.y1 + crop_hw[0], p.x1:p.x1 + crop_hw[1]]
    if p.hflip:
        a = a[:, ::-1]
    if p.vflip:
        a = a[::-1]
    return np.ascontiguousarray(a)


def scale_crop(frames: np.ndarray, label: np.ndarray, p, crop_hw):
    """Stage 1 of one sample: uint8 frames [T][Hs][Ws][3], label [Hs][Ws] -> uint8 crops [T][Hc][Wc][3], label crop [Hc][Wc]."""
    ow, oh, padw, padh = geometry(p.long_size, label.shape, crop_hw)
    crops = np.stack([_pad_crop_flip(pr.resize(f, oh, ow), p, padw, padh, crop_hw) for f in frames])
    return crops, _pad_crop_flip(resize_nearest(label, oh, ow), p, padw, padh, crop_hw)


def scale_crop_pillow(frames: np.ndarray, label: np.ndarray, p, crop_hw):
    """The same through Pillow itself, call for call as _random_scale (plus the flips)."""
    from PIL import Image, ImageOps
    ow, oh, padw, padh = geometry(p.long_size, label.shape, crop_hw)
    box = (p.x1, p.y1, p.x1 + crop_hw[1], p.y1 + crop_hw[0])

    def one(a, resample):
        im = Image.fromarray(a).resize((ow, oh), resample)
        if padw or padh:
            im = ImageOps.expand(im, border=(0, 0, padw, padh), fill=0)
        a = np.array(im.crop(box))
        if p.hflip:
            a = a[:, ::-1]
        if p.vflip:
            a = a[::-1]
        return np.ascontiguousarray(a)

    return np.stack([one(f, Image.BILINEAR) for f in frames]), one(label, Image.NEAREST)


# --------------------------------------------------------------------------------------------- value table, rotation
def value_table(alpha, beta) -> np.ndarray:
    """uint8 [256]: brightness / contrast as one table, clip(round(alpha * u + beta * 255), 0, 255) with alpha = 1 + the contrast
    draw and beta = the brightness draw (brightness_by_max: times 255).  THE rounding: float64, floor(x + 0.5)."""
    if alpha is None and beta is None:
        return np.arange(256, dtype=np.uint8)
    u = np.arange(256, dtype=np.float64)
    v = np.floor(float(1.0 if alpha is None else alpha) * u + float(0.0 if beta is None else beta) * 255.0 + 0.5)
    return np.clip(v, 0, 255).astype(np.uint8)


def rotate_tables(angle: float, H: int, W: int):
    """int32 position tables of the inverse rotation by `angle` degrees (positive = counter-clockwise on the screen) about
    ((W - 1) / 2, (H - 1) / 2): (colx [W], coly [W], rowx [H], rowy [H]) with AB_BITS fraction bits, the rounding term of half a
    1/32 pixel folded into the row tables.  Source position of output (y, x) in 1/32 pixel: ((rowx[y] + colx[x]) >> 5,
    (rowy[y] + coly[x]) >> 5)."""
    r = math.radians(float(angle))
    a, b = math.cos(r), math.sin(r)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    m00, m01, m02 = a, -b, cx - a * cx + b * cy            # source = M (x, y, 1)
    m10, m11, m12 = b, a, cy - b * cx - a * cy
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    scale = float(1 << AB_BITS)
    rnd = (1 << AB_BITS) // (1 << INTER_BITS) // 2
    colx = np.rint(m00 * xs * scale).astype(np.int64)
    coly = np.rint(m10 * xs * scale).astype(np.int64)
    rowx = np.rint((m01 * ys + m02) * scale).astype(np.int64) + rnd
    rowy = np.rint((m11 * ys + m12) * scale).astype(np.int64) + rnd
    return tuple(t.astype(np.int32) for t in (colx, coly, rowx, rowy))


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    """Border index gfedcb|abcdefgh|gfedcba for any integer i."""
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def rotate(crops: np.ndarray, label: np.ndarray, angle, table: np.ndarray):
    """Stage 2 without the conversion: the value table on every source pixel, then the fixed-point bilinear rotation (labels: the
    nearest source pixel).  uint8 crops [T][H][W][3], label [H][W] -> the same shapes.  angle None: the table only."""
    v = table[crops]
    if angle is None:
        return v, label.copy()
    H, W = label.shape
    colx, coly, rowx, rowy = (t.astype(np.int64) for t in rotate_tables(angle, H, W))
    shift = AB_BITS - INTER_BITS
    one = 1 << INTER_BITS
    X = (rowx[:, None] + colx[None, :]) >> shift
    Y = (rowy[:, None] + coly[None, :]) >> shift
    sx, sy, fx, fy = X >> INTER_BITS, Y >> INTER_BITS, X & (one - 1), Y & (one - 1)
    x0, x1, y0, y1 = reflect101(sx, W), reflect101(sx + 1, W), reflect101(sy, H), reflect101(sy + 1, H)
    v = v.astype(np.int64)
    fx, fy = fx[None, :, :, None], fy[None, :, :, None]
    acc = ((one - fx) * (one - fy) * v[:, y0, x0] + fx * (one - fy) * v[:, y0, x1]
           + (one - fx) * fy * v[:, y1, x0] + fx * fy * v[:, y1, x1])
    out = ((acc + (1 << (2 * INTER_BITS - 1))) >> (2 * INTER_BITS)).astype(np.uint8)
    nx = reflect101((X + one // 2) >> INTER_BITS, W)
    ny = reflect101((Y + one // 2) >> INTER_BITS, H)
    return out, label[ny, nx]


# --------------------------------------------------------------------------------------------- conversion
CADIS_MEAN = np.array([0.40789654, 0.44719302, 0.47026115], dtype=np.float32)       # CATA_new_512.py:21-22
CADIS_STD = np.array([0.28863828, 0.27408164, 0.27809835], dtype=np.float32)


def to_float(crops: np.ndarray, protocol: str = "endovis18") -> np.ndarray:
    """uint8 [T][H][W][3] -> fp32 [T][3][H][W]: `astype(float) / 255.` (CaDIS: then `(x - MEAN) / STD` in float64), `.float()`."""
    x = crops.astype(np.float64) / 255.
    if protocol == "cadis":
        x = (x - CADIS_MEAN) / CADIS_STD
    return np.ascontiguousarray(x.astype(np.float32).transpose(0, 3, 1, 2))


def label_table(protocol: str = "endovis18", class_num: int = 12) -> np.ndarray:
    t = np.arange(256, dtype=np.int64)
    if protocol == "cadis":
        t[255] = class_num - 1                                                         # CATA_new_512.py:237
    return t


def augment_one(frames, label, p, crop_hw, protocol="endovis18", class_num=12):
    crops, lab = scale_crop(frames, label, p, crop_hw)
    crops, lab = rotate(crops, lab, p.angle, value_table(p.alpha, p.beta))
    return to_float(crops, protocol), label_table(protocol, class_num)[lab]


def augment(frames, labels, params, crop_hw, protocol="endovis18", class_num=12):
    """uint8 frames [B][T][Hs][Ws][3], labels [B][Hs][Ws], B parameter objects -> (fp32 [B][T][3][Hc][Wc], int64 [B][Hc][Wc])."""
    res = [augment_one(f, l, p, crop_hw, protocol, class_num) for f, l, p in zip(frames, labels, params)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# --------------------------------------------------------------------------------------------- seeded inputs
def seeded_clip(seed: int, T: int, H: int, W: int, classes: int = 12):
    """A clip a test can regenerate from its seed: uint8 frames [T][H][W][3] (a moving gradient plus noise, so that neighbouring
    pixels and frames differ) and a uint8 label [H][W] of blocks."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    frames = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        for c in range(3):
            base = (x * (3 + c) + y * (5 - c) + 37 * t + 60 * c) % 256
            frames[t, :, :, c] = (base + rng.integers(0, 48, (H, W))) % 256
    label = rng.integers(0, classes, ((H + 7) // 8, (W + 7) // 8), dtype=np.uint8).repeat(8, 0).repeat(8, 1)[:H, :W]
    return frames, np.ascontiguousarray(label)
