"""numpy restatement of Pillow's `Image.resize(size, Image.BILINEAR)` on uint8 RGB frames (the per-frame transform of
seg18/dataset/Endovis2018_new.py:125-127), used as the reference of the frame-ingest kernel.

Pillow (libImaging/Resample.c) resamples separably: a horizontal pass when the width changes, first, then a vertical pass when the
height changes, with the intermediate clipped and stored as uint8.  Per output index the triangle filter is sampled over
[center - support, center + support), normalised by its float64 sum and converted to int32 with 22 fraction bits; every output is
clip((2^21 + sum u * k) >> 22, 0, 255)."""
from __future__ import annotations

import numpy as np

PRECISION_BITS = 22


def coeffs(in_size: int, out_size: int):
    """-> (xmin [out], n [out], k int64 [out][ksize]) exactly as precompute_coeffs + normalize_coeffs_8bpc compute them."""
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmin = np.zeros(out_size, np.int64)
    n = np.zeros(out_size, np.int64)
    k = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = []
        ww = 0.0
        for x in range(hi - lo):
            t = abs((x + lo - center + 0.5) * ss)
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(hi - lo):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS))
        xmin[xx], n[xx] = lo, hi - lo
    return xmin, n, k


def _pass(a: np.ndarray, out_size: int, axis: int) -> np.ndarray:
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    xmin, n, k = coeffs(a.shape[0], out_size)
    acc = np.full((out_size,) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for j in range(k.shape[1]):
        src = np.minimum(xmin + j, a.shape[0] - 1)
        kj = np.where(j < n, k[:, j], 0).reshape((out_size,) + (1,) * (a.ndim - 1))
        acc += a[src] * kj
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, H: int, W: int) -> np.ndarray:
    """uint8 [Hs][Ws][3] -> uint8 [H][W][3], bit-exact with PIL.Image.fromarray(img).resize((W, H), Image.BILINEAR)."""
    out = img
    if img.shape[1] != W:
        out = _pass(out, W, 1)
    if img.shape[0] != H:
        out = _pass(out, H, 0)
    return np.ascontiguousarray(out)


def to_float(img: np.ndarray) -> np.ndarray:
    """The reference's `astype(float) / 255.` followed by `.float()`: uint8 [H][W][3] -> fp32 [3][H][W]."""
    return (img.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1).copy()


def transform(img: np.ndarray, H: int, W: int) -> np.ndarray:
    return to_float(resize(img, H, W))
