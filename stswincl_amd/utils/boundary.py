"""Boundary scores of a segmentation - the normalised surface distance (NSD) and the Hausdorff distance - from exact distances
between the contours of two label maps: the numpy definition that hip.boundary_counts (include/stswin_hip.h, stswin_boundary_counts)
matches bit for bit, and BoundaryScores, what an evaluation reads from the counts.

For a map M and a class c the contour B_c(M) is the set of pixels with M == c that have at least one 4-neighbour with M != c, a
neighbour outside the image counting as different: `mask & ~scipy.ndimage.binary_erosion(mask)` with scipy's defaults, MONAI's
get_mask_edges.  A value outside 0 .. nc-1 belongs to no class.  Distances are Euclidean distances between pixel centres in pixels,
kept as exact squared integers."""
from __future__ import annotations

import numpy as np

MAX_BINS, MAX_CLASSES, MAX_SIDE = 256, 64, 16384


def contour(mask: np.ndarray) -> np.ndarray:
    """bool [H][W] -> the pixels of the mask with a 4-neighbour outside it (outside the image counts as outside the mask)."""
    p = np.pad(np.asarray(mask, dtype=bool), 1)
    return p[1:-1, 1:-1] & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def nearest_d2(own: np.ndarray, other: np.ndarray, chunk: int = 1 << 22) -> np.ndarray:
    """Pixel lists int [k][2] and [m][2] (m >= 1) -> int64 [k]: per own pixel the smallest squared distance to a pixel of `other`."""
    own, other = np.asarray(own, dtype=np.int64), np.asarray(other, dtype=np.int64)
    out = np.empty(len(own), dtype=np.int64)
    step = max(1, chunk // len(other))
    for i in range(0, len(own), step):
        d = own[i:i + step, None, :] - other[None, :, :]
        out[i:i + step] = (d * d).sum(axis=2).min(axis=1)
    return out


def ceil_sqrt(d2: np.ndarray) -> np.ndarray:
    """The smallest integer k with k k >= d2, exactly (the float root only seeds it)."""
    d2 = np.asarray(d2, dtype=np.int64)
    k = np.sqrt(d2.astype(np.float64)).astype(np.int64)
    k -= (k > 0) & ((k - 1) * (k - 1) >= d2)
    k += k * k < d2
    k += k * k < d2
    return k


def boundary_counts(gt, pred, nc: int, bins: int = 32, skip=()) -> np.ndarray:
    """Integer maps gt, pred [n][H][W] -> int32 [n][nc][2][2 + bins].  Row out[f][c][d], d = 0: the contour of gt's class c measured
    against the one of pred's, d = 1: pred against gt; d2(p) = the minimum over the other contour's pixels q of |p - q|^2:
        [0]        the number of pixels of the own contour
        [1]        the maximum of d2 over them, -1 when either contour is empty
        [2 + k]    k < bins - 1: the own contour pixels with ceil(sqrt(d2)) == k;  [2 + bins - 1]: those with ceil(sqrt(d2)) >= bins - 1
                   (all zero when either contour is empty)
    The rows of the classes in `skip` are all zero.  2 <= bins <= 256, 1 <= nc <= 64, 1 <= H, W <= 16384: d2 < 2^30."""
    return counts_from_d2(*contour_d2(gt, pred, nc, skip), bins, skip)


def contour_d2(gt, pred, nc: int, skip=()):
    """The first half of boundary_counts, what does not depend on bins: -> (sizes int64 [n][nc][2], the contours' pixel counts, d2: a
    dict (f, c, d) -> int64 [sizes[f][c][d]], the squared distance of every pixel of that contour to the other one, for the classes
    not in `skip` whose two contours are both non-empty)."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    if gt.ndim != 3 or gt.shape != pred.shape or gt.dtype.kind not in "iu" or pred.dtype.kind not in "iu":
        raise ValueError(f"boundary_counts: gt and pred must be integer [n][H][W] of one shape, got {gt.shape} and {pred.shape}")
    n, H, W = gt.shape
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"boundary_counts: a {H} x {W} map, the definition takes 1 .. {MAX_SIDE} per side")
    if not 1 <= nc <= MAX_CLASSES:
        raise ValueError(f"boundary_counts: nc must be 1 .. {MAX_CLASSES}, got {nc}")
    skip = {int(c) for c in skip}
    sizes, d2 = np.zeros((n, nc, 2), dtype=np.int64), {}
    for f in range(n):
        for c in range(nc):
            if c in skip:
                continue
            pts = [np.argwhere(contour(m[f] == c)) for m in (gt, pred)]
            sizes[f, c] = len(pts[0]), len(pts[1])
            if len(pts[0]) and len(pts[1]):
                d2[f, c, 0], d2[f, c, 1] = nearest_d2(pts[0], pts[1]), nearest_d2(pts[1], pts[0])
    return sizes, d2


def counts_from_d2(sizes, d2, bins: int = 32, skip=()) -> np.ndarray:
    """The second half of boundary_counts: contour_d2's pair -> the rows int32 [n][nc][2][2 + bins], zero for the classes in `skip`."""
    if not 2 <= bins <= MAX_BINS:
        raise ValueError(f"boundary_counts: bins must be 2 .. {MAX_BINS}, got {bins}")
    skip = {int(c) for c in skip}
    n, nc = sizes.shape[:2]
    out = np.zeros((n, nc, 2, 2 + bins), dtype=np.int32)
    for f in range(n):
        for c in range(nc):
            if c in skip:
                continue
            for d in range(2):
                out[f, c, d, 0] = sizes[f, c, d]
                out[f, c, d, 1] = -1
                if (f, c, d) in d2:
                    out[f, c, d, 1] = d2[f, c, d].max()
                    out[f, c, d, 2:] = np.bincount(np.minimum(ceil_sqrt(d2[f, c, d]), bins - 1), minlength=bins)
    return out


class BoundaryScores:
    """What an evaluation reads from boundary counts [F][nc][2][2 + bins] (boundary_counts, hip.boundary_counts,
    VideoSegmenter.boundary_scores()).  A class is scored in a frame when it is not skipped (an all-zero row) and present in the
    ground truth (its gt contour is not empty): EndoScores' rule for Dice, with the caller's skip set in the place of class 0.

    counts, sequences, frames   the counts, and per row the ordinal of its sequence and its frame index
    count, classes, bins        rows, nc, bins
    nsd(tau), hausdorff(), hausdorff_percentile(q)      per frame [[class, value], ...] over the scored classes
    aggregate(lists)            the aggregates of such lists with EndoScores' rules (below)
    as_rows(names=None)         one dict per frame and scored class

    aggregate -> a namespace with mean (the mean over the frames of the frame's mean over its scored classes), per_sequence (float64
    [sequences], the same over the frames of one sequence), each (float64 [nc], per class the mean of its values over the frames that
    score it), tool_each (float64 [nc], the number of those frames) and empty_frames (the rows without a scored class).  Sums run in
    float64 in row order.  As in EndoScores a frame without a scored class has the mean of an empty list, NaN, and makes mean and its
    sequence's entry NaN; a class no frame scores is 0 / 0 = NaN in each.  An infinite Hausdorff distance (the prediction lacks the
    class) makes the sums it enters infinite."""

    def __init__(self, counts: np.ndarray, sequences, frames):
        self.counts = counts
        self.sequences, self.frames = [int(s) for s in sequences], [int(f) for f in frames]
        self.count, self.classes, self.bins = counts.shape[0], counts.shape[1], counts.shape[3] - 2
        self.names = None                      # class names, the default of as_rows()

    @classmethod
    def from_counts(cls, counts, sequences=None, frames=None) -> "BoundaryScores":
        """counts: integer [F][nc][2][2 + bins] (numpy, or a torch tensor on any device); sequences: per row the ordinal of its sequence
        (default: all 0); frames: per row its frame index (default: the row index)."""
        if hasattr(counts, "cpu"):
            counts = counts.cpu().numpy()
        cnt = np.asarray(counts)
        if cnt.ndim != 4 or cnt.shape[2] != 2 or cnt.shape[3] < 4 or cnt.dtype.kind not in "iu":
            raise ValueError(f"BoundaryScores.from_counts: counts must be integer [F][nc][2][2 + bins], got {cnt.dtype} {cnt.shape}")
        sequences = [0] * cnt.shape[0] if sequences is None else list(sequences)
        frames = list(range(cnt.shape[0])) if frames is None else list(frames)
        if len(sequences) != cnt.shape[0] or any(int(s) != s or s < 0 for s in sequences) or len(frames) != cnt.shape[0]:
            raise ValueError(f"BoundaryScores.from_counts: one sequence ordinal >= 0 and one frame per row of counts, got {len(sequences)} "
                             f"and {len(frames)} for {cnt.shape[0]}")
        return cls(cnt.astype(np.int64), sequences, frames)

    def __len__(self) -> int:
        return self.count

    def scored(self, f: int):
        """The classes scored in row f: gt contour not empty (a skipped class's row is all zero)."""
        return [c for c in range(self.classes) if self.counts[f, c, 0, 0] > 0]

    def nsd(self, tau: int):
        """The normalised surface distance at the whole-pixel tolerance tau, 0 <= tau <= bins - 2: the share of the pixels of both
        contours that lie within tau of the other contour, (sum_{k <= tau} hist[0][k] + sum_{k <= tau} hist[1][k]) / (count[0] +
        count[1]).  MONAI's compute_surface_dice for whole-pixel tolerances (d <= tau is ceil(sqrt(d2)) <= tau), ROBUST-MIS's NSD.  0
        when the prediction has no pixel of the class."""
        if isinstance(tau, bool) or int(tau) != tau or not 0 <= tau <= self.bins - 2:
            raise ValueError(f"nsd: tau must be an integer 0 .. bins - 2 = {self.bins - 2}, got {tau!r}")
        tau = int(tau)
        out = []
        for f in range(self.count):
            row = []
            for c in self.scored(f):
                r = self.counts[f, c]
                row.append([c, float(r[0, 2:3 + tau].sum() + r[1, 2:3 + tau].sum()) / float(r[0, 0] + r[1, 0])])
            out.append(row)
        return out

    def hausdorff(self):
        """The Hausdorff distance sqrt(max(d2 of both directions)) in pixels, exact; inf when the prediction has no pixel of the class."""
        out = []
        for f in range(self.count):
            row = []
            for c in self.scored(f):
                m = max(int(self.counts[f, c, 0, 1]), int(self.counts[f, c, 1, 1]))
                row.append([c, float(np.sqrt(np.float64(m))) if m >= 0 else float("inf")])
            out.append(row)
        return out

    def hausdorff_percentile(self, q: float = 95.0):
        """The q-th percentile Hausdorff distance at whole-pixel resolution: per direction the smallest k for which at least q % of
        the contour pixels have a distance <= k (nearest rank), then the larger of the two directions; inf when that k is the tail
        bin (distances >= bins - 1 are not resolved) or the prediction has no pixel of the class.  An upper bound of the percentile
        of the true distances, at most one pixel above it - not np.percentile's interpolation between ranks."""
        if not 0 < q <= 100:
            raise ValueError(f"hausdorff_percentile: q must be in (0, 100], got {q!r}")
        out = []
        for f in range(self.count):
            row = []
            for c in self.scored(f):
                worst = 0.0
                for d in range(2):
                    r = self.counts[f, c, d]
                    if r[1] < 0:
                        worst = float("inf")
                        continue
                    k = int(np.argmax(np.cumsum(r[2:]) * 100.0 >= int(r[0]) * float(q)))     # (the last bin always holds: the first True)
                    worst = max(worst, float("inf") if k >= self.bins - 1 else float(k))
                row.append([c, worst])
            out.append(row)
        return out

    def aggregate(self, lists):
        """Per-frame lists [[class, value], ...] (nsd, hausdorff, hausdorff_percentile) -> their aggregates (the class docstring)."""
        from types import SimpleNamespace
        nseq = max(self.sequences) + 1 if self.sequences else 0
        total, per_seq, count_seq = np.zeros(()), np.zeros((nseq,)), np.zeros((nseq,))
        each, tool_each, empty = np.zeros((self.classes,)), np.zeros((self.classes,)), []
        for f, (row, s) in enumerate(zip(lists, self.sequences)):
            for c, v in row:
                each[c] += v
                tool_each[c] += 1
            if row:
                frame = np.mean([v for _, v in row])
            else:                                                 # np.mean([]) without its warning
                frame = np.float64("nan")
                empty.append(f)
            total = total + frame
            per_seq[s] += frame
            count_seq[s] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = total / self.count if self.count else np.float64("nan")
            per_seq = per_seq / count_seq
            each = each / tool_each
        return SimpleNamespace(mean=float(mean), per_sequence=per_seq, each=each, tool_each=tool_each, empty_frames=empty)

    @property
    def empty_frames(self):
        """The rows whose ground truth has no scored class."""
        return [f for f in range(self.count) if not self.scored(f)]

    @property
    def tool_each(self) -> np.ndarray:
        """float64 [nc]: the number of rows that score the class."""
        t = np.zeros((self.classes,))
        for f in range(self.count):
            for c in self.scored(f):
                t[c] += 1
        return t

    def as_rows(self, names=None, tau: int = 1, q: float = 95.0):
        """One dict per row and scored class: sequence, frame, class, name, gt_pixels and pred_pixels (the contours' sizes), nsd (at
        tau, clipped to bins - 2), hausdorff, hausdorff_percentile (at q)."""
        tau = min(int(tau), self.bins - 2)
        names = names if names is not None else self.names
        nsd, hd, hp = self.nsd(tau), self.hausdorff(), self.hausdorff_percentile(q)
        rows = []
        for f in range(self.count):
            for (c, a), (_, b), (_, p) in zip(nsd[f], hd[f], hp[f]):
                rows.append({"sequence": self.sequences[f], "frame": self.frames[f], "class": c,
                             "name": names[c] if names is not None else str(c), "gt_pixels": int(self.counts[f, c, 0, 0]),
                             "pred_pixels": int(self.counts[f, c, 1, 0]), "nsd": a, "hausdorff": b, "hausdorff_percentile": p})
        return rows
