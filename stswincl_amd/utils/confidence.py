"""Confidence of the labels: the definitions of hip.upsample_confidence (stswin_upsample_confidence) and hip.confidence_sums
(stswin_confidence_sums) in numpy, and what is made of the sums on the host.  No torch.

The reference computes the softmax between its resize and its argmax and throws it away (seg18/test.py:153-158); the label launches
skip it because it is monotone.  The confidence of a pixel is that probability for the label the pixel got, as a byte:
conf = min(255, floor(255 p + 0.5)), p = exp(v_l - m) / sum_c exp(v_c - m) with v_c the bilinear value of class c and m their maximum.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np


def _source(n_in: int, n_out: int, align_corners: bool):
    """Source indices and weight of the bilinear resize of one axis, in float32 by the expressions of include/stswin_hip.h (index
    choice cannot be toleranced) -> (i0 int64 [n_out], i1 int64 [n_out], weight of i1 float32 [n_out])."""
    f32 = np.float32
    d = np.arange(n_out, dtype=np.int64).astype(f32)
    if align_corners:
        scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        src = d * scale
    else:
        scale = f32(n_in) / f32(n_out)
        src = np.maximum(scale * (d + f32(0.5)) - f32(0.5), f32(0))
    src = src.astype(f32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (src - i0.astype(f32)).astype(f32)


def upsample_softmax(logits, size: Sequence[int], align_corners: bool = True) -> np.ndarray:
    """float64 [F][nc][H][W]: the softmax over the classes of the bilinear resize of `logits` [F][nc][h][w] to size = (H, W).  Indices
    and weights in float32 (_source), the rest in float64."""
    lg = np.asarray(logits)
    H, W = (int(v) for v in size)
    if lg.ndim != 4 or lg.size == 0 or H < 1 or W < 1:
        raise ValueError(f"confidence: logits are [F][nc][h][w], not empty, resized to (H, W) >= 1, got {lg.shape} and {(H, W)}")
    h, w = lg.shape[2:]
    y0, y1, wy = _source(h, H, align_corners)
    x0, x1, wx = _source(w, W, align_corners)
    wy = wy.astype(np.float64)[None, None, :, None]
    wx = wx.astype(np.float64)[None, None, None, :]
    v = lg.astype(np.float64)
    top = (1.0 - wx) * v[:, :, y0][:, :, :, x0] + wx * v[:, :, y0][:, :, :, x1]
    bot = (1.0 - wx) * v[:, :, y1][:, :, :, x0] + wx * v[:, :, y1][:, :, :, x1]
    v = (1.0 - wy) * top + wy * bot                            # [F][nc][H][W]
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def pick_labels(p: np.ndarray, labels) -> np.ndarray:
    """float64 [F][H][W]: p [F][nc][H][W] at each pixel's label (uint8 [F][H][W]); 0 where the label is >= nc."""
    lab = np.asarray(labels)
    if p.ndim != 4 or lab.dtype != np.uint8 or lab.shape != (p.shape[0],) + p.shape[2:]:
        raise ValueError(f"confidence: labels are uint8 [F][H][W] = {(p.shape[0],) + p.shape[2:]}, got {lab.dtype} {lab.shape}")
    known = lab < p.shape[1]
    picked = np.take_along_axis(p, np.where(known, lab, 0).astype(np.int64)[:, None], axis=1)[:, 0]
    return np.where(known, picked, 0.0)


def upsample_probability(logits, labels, align_corners: bool = True) -> np.ndarray:
    """float64 [F][H][W]: the softmax probability, over the classes of the bilinear resize of `logits` [F][nc][h][w] to the labels'
    (H, W), of each pixel's label; 0 where the label is >= nc (upsample_softmax, then pick_labels)."""
    lab = np.asarray(labels)
    if lab.ndim != 3 or lab.size == 0:
        raise ValueError(f"confidence: labels are uint8 [F][H][W], not empty, got {lab.dtype} {lab.shape}")
    return pick_labels(upsample_softmax(logits, lab.shape[1:], align_corners), lab)


def upsample_confidence(logits, labels, align_corners: bool = True) -> np.ndarray:
    """uint8 [F][H][W] = min(255, floor(255 p + 0.5)) of upsample_probability: the definition of hip.upsample_confidence (which works
    in float32: a byte may differ by one where 255 p is within its error of a half)."""
    p = upsample_probability(logits, labels, align_corners)
    return np.minimum(255, np.floor(255.0 * p + 0.5)).astype(np.uint8)


def confidence_sums(maps, conf, K: int, low: int = 128) -> np.ndarray:
    """maps uint8 or int32 [n][H][W], conf uint8 [n][H][W] -> int64 [n][K][3]: per frame and map value i in [0, K) the number of its
    pixels, the sum of their conf and the number of them with conf < low; other values are counted nowhere.  What
    hip.confidence_sums matches bit for bit."""
    m = np.asarray(maps)
    q = np.asarray(conf)
    if m.dtype not in (np.uint8, np.int32) or m.ndim != 3 or m.size == 0 or q.dtype != np.uint8 or q.shape != m.shape:
        raise ValueError(f"confidence_sums: maps are uint8 or int32 [n][H][W] and conf uint8 of that shape, got {m.dtype} {m.shape} "
                         f"and {q.dtype} {q.shape}")
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= 1024:
        raise ValueError(f"confidence_sums: K is an integer 1 .. 1024, got {K!r}")
    if isinstance(low, bool) or not isinstance(low, (int, np.integer)) or not 0 <= low <= 256:
        raise ValueError(f"confidence_sums: low is an integer 0 .. 256, got {low!r}")
    out = np.zeros((m.shape[0], K, 3), dtype=np.int64)
    for f in range(m.shape[0]):
        v = m[f].reshape(-1).astype(np.int64)
        c = q[f].reshape(-1).astype(np.int64)
        keep = (v >= 0) & (v < K)
        v, c = v[keep], c[keep]
        out[f, :, 0] = np.bincount(v, minlength=K)
        out[f, :, 1] = np.bincount(v, weights=c, minlength=K).astype(np.int64)       # (< 2^53: exact in float64)
        out[f, :, 2] = np.bincount(v[c < low], minlength=K)
    return out


def _ratios(sums, what: str):
    s = np.asarray(sums)
    if s.ndim == 2:
        s = s[None]
    if s.ndim != 3 or s.shape[2] != 3 or s.dtype.kind not in "iu":
        raise ValueError(f"ConfidenceReport: {what} are integers [rows][K][3], got {s.dtype} {s.shape}")
    s = s.astype(np.int64)
    count = s[:, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(count > 0, s[:, :, 1] / (255.0 * count), np.nan)
        low = np.where(count > 0, s[:, :, 2] / count.astype(np.float64), np.nan)
    return s, mean, low


class ConfidenceReport:
    """How sure the model was, per frame (row r), from the sums of confidence_sums:

      class_sums      int64   [rows][nc][3]   count, sum of conf, pixels with conf < low, per class
      mean            float64 [rows][nc]      sum / (255 count): the mean probability of the class's pixels, NaN where it has none
      low_fraction    float64 [rows][nc]      the share of its pixels with conf < low, NaN where it has none
      instance_sums, instance_mean, instance_low_fraction   the same per instance ordinal [rows][K] when instances are on, else None

    frames / sequences: per row the frame index and the sequence ordinal, as the instrument report's; names: per class, the caller's;
    low: the threshold the sums were taken with."""

    def __init__(self):
        self.low = 128
        self.names = None
        self.frames: List[int] = []
        self.sequences: List[int] = []
        self.class_sums = self.mean = self.low_fraction = None
        self.instance_sums = self.instance_mean = self.instance_low_fraction = None

    @classmethod
    def from_sums(cls, class_sums, instance_sums=None, low: int = 128, names: Optional[Sequence[str]] = None,
                  frames: Optional[Sequence[int]] = None, sequences: Optional[Sequence[int]] = None) -> "ConfidenceReport":
        """class_sums: integers [rows][nc][3] (or one frame's [nc][3]), numpy or a CPU torch tensor; instance_sums [rows][K][3] or None."""
        rep = cls()
        rep.class_sums, rep.mean, rep.low_fraction = _ratios(class_sums, "class sums")
        rows, nc = rep.mean.shape
        if instance_sums is not None:
            rep.instance_sums, rep.instance_mean, rep.instance_low_fraction = _ratios(instance_sums, "instance sums")
            if rep.instance_mean.shape[0] != rows:
                raise ValueError(f"ConfidenceReport: instance sums of {rep.instance_mean.shape[0]} rows for {rows} rows")
        if isinstance(low, bool) or not isinstance(low, (int, np.integer)) or not 0 <= low <= 256:
            raise ValueError(f"ConfidenceReport: low is an integer 0 .. 256, got {low!r}")
        if names is not None and len(names) != nc:
            raise ValueError(f"ConfidenceReport: {len(names)} names for {nc} classes")
        for what, v in (("frames", frames), ("sequences", sequences)):
            if v is not None and len(v) != rows:
                raise ValueError(f"ConfidenceReport: {len(v)} {what} for {rows} rows")
        rep.low = int(low)
        rep.names = list(names) if names is not None else None
        rep.frames = [int(f) for f in frames] if frames is not None else list(range(rows))
        rep.sequences = [int(s) for s in sequences] if sequences is not None else [0] * rows
        return rep

    def __len__(self) -> int:
        return len(self.frames)

    def as_rows(self) -> List[dict]:
        """One dict per row and class with pixels, in row order then class order: sequence, frame, class (and name, when names were
        given), pixels, mean, low_fraction as plain Python values."""
        out = []
        for r in range(len(self)):
            for c in np.nonzero(self.class_sums[r, :, 0])[0].tolist():
                row = {"sequence": self.sequences[r], "frame": self.frames[r], "class": c}
                if self.names is not None:
                    row["name"] = self.names[c]
                row.update(pixels=int(self.class_sums[r, c, 0]), mean=float(self.mean[r, c]), low_fraction=float(self.low_fraction[r, c]))
                out.append(row)
        return out
