"""Per-frame instrument report: which classes a label map holds, how large each is, where it lies and which way it points.  The numpy
statement of what hip.label_moments computes, and the report VideoSegmenter(report=...) returns.  numpy only, no GPU needed.

One row of ten integers per frame and class c, over the pixels (y, x) whose label equals c (include/stswin_hip.h,
stswin_label_moments):

    0: count      1, 2: sum x, sum y      3, 4, 5: sum x^2, sum xy, sum y^2
    6, 7: max(W - x), max(H - y)          8, 9: max(x + 1), max(y + 1)

The extent is four maxima, so an all-zero row is an absent class and rows pool by adding 0 .. 5 and taking the maximum of 6 .. 9; the
half-open box of a present class is [W - row[6], row[8]) x [H - row[7], row[9]).  Labels >= nc are counted nowhere.

This module ships no dataset's class names: pass `names` if the rows of a log should carry them."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

ROW = 10                # integers per frame and class


def label_moments(labels, nc: int) -> np.ndarray:
    """uint8 (or any integer) labels [n][H][W] (or one [H][W]) -> int64 [n][nc][10], the row above, in np.int64 arithmetic: what
    hip.label_moments gives bit for bit."""
    lab = np.asarray(labels)
    if lab.ndim == 2:
        lab = lab[None]
    if lab.ndim != 3 or lab.dtype.kind not in "iu" or min(lab.shape) < 1:
        raise ValueError(f"label_moments: labels are integers [n][H][W], got {lab.dtype} {lab.shape}")
    if not 1 <= nc <= 64:
        raise ValueError(f"label_moments: 1 .. 64 classes, got {nc}")
    n, H, W = lab.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    out = np.zeros((n, nc, ROW), dtype=np.int64)
    for f in range(n):
        for c in range(nc):
            m = lab[f] == c
            if not m.any():
                continue
            x, y = xs[m], ys[m]
            out[f, c] = [x.size, x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(),
                         (W - x).max(), (H - y).max(), (x + 1).max(), (y + 1).max()]
    return out


class InstrumentReport:
    """What a consumer of a segmented frame acts on, per frame (row r) and class c, from the moments rows:

      present  bool    [rows][nc]      count >= min_area
      area     int64   [rows][nc]      the pixel count (0 where not present)
      box      float64 [rows][nc][4]   (x0, y0, x1, y1), half-open, whole numbers
      centroid float64 [rows][nc][2]   (cx, cy) = (sum x, sum y) / count
      angle    float64 [rows][nc]      direction of the principal axis in radians in (-pi/2, pi/2], from +x towards +y:
                                       atan2(2 mu11, mu20 - mu02) / 2
      axes     float64 [rows][nc][2]   (sigma_major, sigma_minor): square roots of the eigenvalues of the central second-moment
                                       matrix [[mu20, mu11], [mu11, mu02]]

    Where a class is not present (absent, or smaller than min_area) area is 0 and box, centroid, angle and axes are NaN (None in
    as_rows()).  The central moments come from exact integer numerators n sum x^2 - (sum x)^2, n sum xy - sum x sum y and n sum y^2 -
    (sum y)^2 in Python integers, divided once by n^2 in float64: sum x^2 / n - cx^2 in floating point cancels at 1280-wide frames.
    The smaller eigenvalue is the (exact) determinant over the larger one, so a one-pixel-wide line has sigma_minor = 0 exactly.

    frames / sequences: per row the frame index and the sequence ordinal (None: rows 0 .. and one sequence); names: per class, for
    as_rows() only."""

    def __init__(self):
        self.size = None
        self.min_area = 1
        self.names = None
        self.frames: List[int] = []
        self.sequences: List[int] = []
        self.moments = self.present = self.area = self.box = self.centroid = self.angle = self.axes = None

    @classmethod
    def from_moments(cls, moments, size: Sequence[int], min_area: int = 1, names: Optional[Sequence[str]] = None,
                     frames: Optional[Sequence[int]] = None, sequences: Optional[Sequence[int]] = None) -> "InstrumentReport":
        """moments: integers [rows][nc][10] (or one frame's [nc][10]), numpy or a CPU torch tensor; size = (H, W) of the label maps."""
        mom = np.asarray(moments)
        if mom.ndim == 2:
            mom = mom[None]
        if mom.ndim != 3 or mom.shape[2] != ROW or mom.dtype.kind not in "iu":
            raise ValueError(f"InstrumentReport: moments are integers [rows][nc][{ROW}], got {mom.dtype} {mom.shape}")
        if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 1:
            raise ValueError(f"InstrumentReport: min_area is an integer >= 1, got {min_area!r}")
        H, W = (int(v) for v in size)
        rows, nc = mom.shape[:2]
        if names is not None and len(names) != nc:
            raise ValueError(f"InstrumentReport: {len(names)} names for {nc} classes")
        for what, v in (("frames", frames), ("sequences", sequences)):
            if v is not None and len(v) != rows:
                raise ValueError(f"InstrumentReport: {len(v)} {what} for {rows} rows")
        rep = cls()
        rep.size, rep.min_area = (H, W), int(min_area)
        rep.names = list(names) if names is not None else None
        rep.frames = [int(f) for f in frames] if frames is not None else list(range(rows))
        rep.sequences = [int(s) for s in sequences] if sequences is not None else [0] * rows
        rep.moments = mom.astype(np.int64)
        rep.present = rep.moments[:, :, 0] >= rep.min_area
        rep.area = np.where(rep.present, rep.moments[:, :, 0], 0)
        rep.box = np.full((rows, nc, 4), np.nan)
        rep.centroid = np.full((rows, nc, 2), np.nan)
        rep.angle = np.full((rows, nc), np.nan)
        rep.axes = np.full((rows, nc, 2), np.nan)
        for r, c in zip(*np.nonzero(rep.present)):
            n, sx, sy, sxx, sxy, syy, ex0, ey0, ex1, ey1 = (int(v) for v in rep.moments[r, c])      # Python integers: exact
            rep.box[r, c] = (W - ex0, H - ey0, ex1, ey1)
            rep.centroid[r, c] = (sx / n, sy / n)
            n20, n11, n02 = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy                 # n^2 (mu20, mu11, mu02)
            rep.angle[r, c] = 0.5 * math.atan2(2 * n11, n20 - n02)
            big = (n20 + n02) + math.sqrt((n20 - n02) ** 2 + 4 * n11 * n11)                         # 2 n^2 lambda_major
            major = big / (2 * n * n)
            minor = 2 * (n20 * n02 - n11 * n11) / (n * n * big) if big > 0 else 0.0
            rep.axes[r, c] = (math.sqrt(major), math.sqrt(max(minor, 0.0)))
        return rep

    def __len__(self) -> int:
        return len(self.frames)

    def presence(self) -> np.ndarray:
        """bool [rows][nc]: which classes each frame holds (count >= min_area)."""
        return self.present.copy()

    def as_rows(self, absent: bool = False) -> List[dict]:
        """One dict per row and present class, in row order then class order, for a log: sequence, frame, class (and name, when names
        were given), area, box, centroid, angle, axes as plain Python values.  absent=True lists the classes that are not present too:
        present False, area 0, the rest None."""
        out = []
        for r in range(len(self)):
            for c in range(self.present.shape[1]):
                here = bool(self.present[r, c])
                if not here and not absent:
                    continue
                row = {"sequence": self.sequences[r], "frame": self.frames[r], "class": c}
                if self.names is not None:
                    row["name"] = self.names[c]
                row["present"] = here
                row["area"] = int(self.area[r, c])
                row["box"] = tuple(int(v) for v in self.box[r, c]) if here else None
                row["centroid"] = tuple(float(v) for v in self.centroid[r, c]) if here else None
                row["angle"] = float(self.angle[r, c]) if here else None
                row["axes"] = tuple(float(v) for v in self.axes[r, c]) if here else None
                out.append(row)
        return out
