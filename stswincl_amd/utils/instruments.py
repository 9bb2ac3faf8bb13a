"""Per-frame instrument report: which classes a label map holds, how large each is, where it lies and which way it points.  The numpy
statement of what hip.label_moments computes, and the report VideoSegmenter(report=...) returns.  numpy only, no GPU needed.

One row of ten integers per frame and class c, over the pixels (y, x) whose label equals c (include/stswin_hip.h,
stswin_label_moments):

    0: count      1, 2: sum x, sum y      3, 4, 5: sum x^2, sum xy, sum y^2
    6, 7: max(W - x), max(H - y)          8, 9: max(x + 1), max(y + 1)

The extent is four maxima, so an all-zero row is an absent class and rows pool by adding 0 .. 5 and taking the maximum of 6 .. 9; the
half-open box of a present class is [W - row[6], row[8]) x [H - row[7], row[9]).  Labels >= nc are counted nowhere.

label_components splits the classes into connected instances (hip.label_components, VideoSegmenter(instances=K)): one row of twelve
integers per frame and instance - its class, its first pixel y * W + x in raster order, then the ten above over its pixels - and
InstanceReport reads those rows as InstrumentReport reads the class rows, by the same arithmetic.

InstanceTracker gives the instances of consecutive frames a common id (hip.track_instances, VideoSegmenter(tracks=True)) by greedy
matching on intersection over union in integers, and TrackReport reads the ids beside an InstanceReport: one entry per track.

group_table maps the classes that are parts of one instrument (shaft, wrist, clasper) to one representative, so that the components of
the grouped labels are whole instruments (VideoSegmenter(instance_groups=...)); instance_parts says per instance and class what it
is made of (the ten integers again) and how many pixel edges it shares with each class outside itself (hip.instance_parts,
VideoSegmenter(parts=...)), and PartsReport reads both beside the instance and track reports.  instance_clearance says how near an
instance comes to each class it does not hold - the exact squared distance and the two pixels that realise it (hip.instance_clearance,
VideoSegmenter(clearance=...)) - and ClearanceReport reads it the same way.

clean_labels states what hip.labels_clean writes (VideoSegmenter(clean_area=A)): the label map with its small components relabelled by
the vote of their stable neighbours - specks out, small holes filled - before anything above reads it.

This module ships no dataset's class names or ids: pass `names` if the rows of a log should carry them."""
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


INSTANCE_ROW = 12       # integers per frame and instance: class, first pixel, then the ten above


def label_components(labels, nc: int, connectivity: int = 8, skip: Sequence[int] = (), max_instances: int = 256):
    """Integer labels [n][H][W] (or one [H][W]) -> (components int32 [n][H][W], rows int64 [n][K][12], total int32 [n]) with K =
    max_instances: what hip.label_components gives bit for bit.

    A component is a maximal set of pixels of one frame with the same label c < nc, c not in `skip`, joined under 4- or
    8-connectivity.  A frame's components of all classes are numbered 0, 1, 2, ... by their first pixel in raster order (the smallest
    y * W + x they hold).  components holds every pixel's ordinal (not bounded by K), -1 for skipped labels and labels >= nc; total[f]
    is the frame's number of components (not bounded by K either); rows[f][i] for i < min(total[f], K) is [class, first = y * W + x]
    followed by the ten integers of the moments row over the component's pixels, and all zero from total[f] on.  With total > K the rows
    kept are the first K in that order.

    Two passes with a union-find whose roots are the smallest index of their set, so a root is its component's first pixel."""
    lab = np.asarray(labels)
    if lab.ndim == 2:
        lab = lab[None]
    if lab.ndim != 3 or lab.dtype.kind not in "iu" or min(lab.shape) < 1:
        raise ValueError(f"label_components: labels are integers [n][H][W], got {lab.dtype} {lab.shape}")
    if isinstance(nc, bool) or int(nc) != nc or not 1 <= nc <= 64:
        raise ValueError(f"label_components: 1 .. 64 classes, got {nc!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"label_components: connectivity is 4 or 8, got {connectivity!r}")
    skip = tuple(skip)
    if any(isinstance(c, bool) or int(c) != c or not 0 <= c <= 63 for c in skip):
        raise ValueError(f"label_components: skip holds classes 0 .. 63, got {skip!r}")
    K = max_instances
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= 1024:
        raise ValueError(f"label_components: max_instances is 1 .. 1024, got {K!r}")
    n, H, W = lab.shape
    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])     # the neighbours that come earlier in raster order
    comp = np.full((n, H, W), -1, dtype=np.int32)
    rows = np.zeros((n, K, INSTANCE_ROW), dtype=np.int64)
    total = np.zeros(n, dtype=np.int32)
    for f in range(n):
        # plain Python lists and integers from here on (exact, and quicker to index than arrays); -1: a pixel of no component
        cls = [c if 0 <= c < nc and c not in skip else -1 for c in lab[f].reshape(-1).tolist()]
        parent = list(range(H * W))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        for p in range(H * W):                # pass 1: join every pixel with its earlier neighbours of the same label
            if cls[p] < 0:
                continue
            y, x = divmod(p, W)
            for dy, dx in back:
                v, u = y + dy, x + dx
                if v >= 0 and 0 <= u < W and cls[v * W + u] == cls[p]:
                    a, b = find(p), find(v * W + u)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
        ordinal, kept, flat = {}, [], [-1] * (H * W)
        for p in range(H * W):                # pass 2: roots come up in raster order of the first pixel
            if cls[p] < 0:
                continue
            y, x = divmod(p, W)
            r = find(p)
            if r == p:
                ordinal[r] = len(ordinal)
                if len(kept) < K:
                    kept.append([cls[p], p, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
            i = flat[p] = ordinal[r]
            if i < K:
                row = kept[i]
                for k, v in enumerate((1, x, y, x * x, x * y, y * y)):
                    row[2 + k] += v
                for k, v in enumerate((W - x, H - y, x + 1, y + 1)):
                    row[8 + k] = max(row[8 + k], v)
        comp[f] = np.asarray(flat, dtype=np.int32).reshape(H, W)
        if kept:
            rows[f, :len(kept)] = kept
        total[f] = len(ordinal)
    return comp, rows, total


def _shape_of(row, H: int, W: int):
    """One present ten-integer row -> (box, centroid, angle, axes), the arithmetic both reports share."""
    n, sx, sy, sxx, sxy, syy, ex0, ey0, ex1, ey1 = (int(v) for v in row)                    # Python integers: exact
    n20, n11, n02 = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy                 # n^2 (mu20, mu11, mu02)
    big = (n20 + n02) + math.sqrt((n20 - n02) ** 2 + 4 * n11 * n11)                         # 2 n^2 lambda_major
    major = big / (2 * n * n)
    minor = 2 * (n20 * n02 - n11 * n11) / (n * n * big) if big > 0 else 0.0
    return ((W - ex0, H - ey0, ex1, ey1), (sx / n, sy / n), 0.5 * math.atan2(2 * n11, n20 - n02),
            (math.sqrt(major), math.sqrt(max(minor, 0.0))))


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
            rep.box[r, c], rep.centroid[r, c], rep.angle[r, c], rep.axes[r, c] = _shape_of(rep.moments[r, c], H, W)
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


class InstanceReport:
    """InstrumentReport per connected instance: from the rows and totals of label_components (hip.label_components,
    VideoSegmenter(instances=K)), per row-frame r and kept instance i < K:

      present   bool    [rows][K]      i < total and count >= min_area
      cls       int64   [rows][K]      the instance's class (-1 where not present)
      first     int64   [rows][K]      y * W + x of its first pixel in raster order (-1 where not present)
      area, box, centroid, angle, axes   as InstrumentReport's, by the same arithmetic, [rows][K] in front
      total     int64   [rows]         the frame's number of components, not bounded by K
      truncated bool    [rows]         total > K: the frame holds more instances than rows were kept for

    frames / sequences / names as InstrumentReport's; names are per class."""

    def __init__(self):
        self.size = None
        self.min_area = 1
        self.names = None
        self.frames: List[int] = []
        self.sequences: List[int] = []
        self.rows = self.total = self.truncated = self.present = self.cls = self.first = None
        self.area = self.box = self.centroid = self.angle = self.axes = None

    @classmethod
    def from_rows(cls, rows, total, size: Sequence[int], min_area: int = 1, names: Optional[Sequence[str]] = None,
                  frames: Optional[Sequence[int]] = None, sequences: Optional[Sequence[int]] = None) -> "InstanceReport":
        """rows: integers [frames][K][12] (or one frame's [K][12]), total: integers [frames] (or a scalar), numpy or CPU torch tensors;
        size = (H, W) of the label maps."""
        rw = np.asarray(rows)
        tot = np.asarray(total)
        if rw.ndim == 2:
            rw = rw[None]
        tot = tot.reshape(-1)
        if rw.ndim != 3 or rw.shape[2] != INSTANCE_ROW or rw.dtype.kind not in "iu":
            raise ValueError(f"InstanceReport: rows are integers [frames][K][{INSTANCE_ROW}], got {rw.dtype} {rw.shape}")
        n, K = rw.shape[:2]
        if tot.dtype.kind not in "iu" or tot.shape != (n,):
            raise ValueError(f"InstanceReport: total holds one integer per frame ({n}), got {tot.dtype} {tot.shape}")
        if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 1:
            raise ValueError(f"InstanceReport: min_area is an integer >= 1, got {min_area!r}")
        H, W = (int(v) for v in size)
        for what, v in (("frames", frames), ("sequences", sequences)):
            if v is not None and len(v) != n:
                raise ValueError(f"InstanceReport: {len(v)} {what} for {n} rows")
        rep = cls()
        rep.size, rep.min_area = (H, W), int(min_area)
        rep.names = list(names) if names is not None else None
        rep.frames = [int(f) for f in frames] if frames is not None else list(range(n))
        rep.sequences = [int(s) for s in sequences] if sequences is not None else [0] * n
        rep.rows = rw.astype(np.int64)
        rep.total = tot.astype(np.int64)
        rep.truncated = rep.total > K
        rep.present = (np.arange(K)[None, :] < rep.total[:, None]) & (rep.rows[:, :, 2] >= rep.min_area)
        rep.cls = np.where(rep.present, rep.rows[:, :, 0], -1)
        rep.first = np.where(rep.present, rep.rows[:, :, 1], -1)
        rep.area = np.where(rep.present, rep.rows[:, :, 2], 0)
        rep.box = np.full((n, K, 4), np.nan)
        rep.centroid = np.full((n, K, 2), np.nan)
        rep.angle = np.full((n, K), np.nan)
        rep.axes = np.full((n, K, 2), np.nan)
        for r, i in zip(*np.nonzero(rep.present)):
            rep.box[r, i], rep.centroid[r, i], rep.angle[r, i], rep.axes[r, i] = _shape_of(rep.rows[r, i, 2:], H, W)
        if rep.names is not None and rep.present.any() and int(rep.cls.max()) >= len(rep.names):
            raise ValueError(f"InstanceReport: {len(rep.names)} names, the rows hold class {int(rep.cls.max())}")
        return rep

    def __len__(self) -> int:
        return len(self.frames)

    def counts(self, nc: Optional[int] = None) -> np.ndarray:
        """int64 [frames][nc]: the number of present instances per class (nc: the names' length, else the largest class + 1)."""
        if nc is None:
            nc = len(self.names) if self.names is not None else (int(self.cls.max()) + 1 if self.present.any() else 0)
        out = np.zeros((len(self), nc), dtype=np.int64)
        for r, i in zip(*np.nonzero(self.present)):
            out[r, self.cls[r, i]] += 1
        return out

    def as_rows(self) -> List[dict]:
        """One dict per present instance, in frame order then instance order, for a log: sequence, frame, instance, class (and name,
        when names were given), area, box, centroid, angle, axes as plain Python values."""
        out = []
        for r in range(len(self)):
            for i in np.nonzero(self.present[r])[0]:
                row = {"sequence": self.sequences[r], "frame": self.frames[r], "instance": int(i), "class": int(self.cls[r, i])}
                if self.names is not None:
                    row["name"] = self.names[row["class"]]
                row["area"] = int(self.area[r, i])
                row["box"] = tuple(int(v) for v in self.box[r, i])
                row["centroid"] = tuple(float(v) for v in self.centroid[r, i])
                row["angle"] = float(self.angle[r, i])
                row["axes"] = tuple(float(v) for v in self.axes[r, i])
                out.append(row)
        return out


class InstanceTracker:
    """Identity of the instances of label_components from frame to frame: the numpy statement of what hip.track_instances computes,
    in integers throughout, matched bit for bit (VideoSegmenter(tracks=True)).

    update(components int32 [H][W], rows int64 [K][12], total) -> (ids int32 [K], started): an instance takes part if its ordinal is
    < min(total, K) and its area rows[i][2] >= min_area.  With P the previous frame's participants (class cp, area ap, id tp) and C
    this frame's (cc, ac): ov[i][j] = the pixels that carry ordinal i in the previous map and j in this one (-1 and ordinals >= K count
    nowhere), u = ap[i] + ac[j] - ov.  (i, j) is a candidate iff ov > 0, cp[i] == cc[j] (dropped with same_class=False) and
    1000 ov >= min_iou u (min_iou: thousandths, 0 .. 1000).  (i, j) is preferred to (i', j') iff ov u' > ov' u, then smaller i, then
    smaller j: a strict total order.  Repeatedly the most preferred candidate whose i and j are both unmatched is matched and ids[j] =
    tp[i]; the participants left over take next, next + 1, ... in ascending j; every other entry of ids is -1.  started is `next` after
    the frame: the number of tracks begun since reset().  An instance that was absent for a frame comes back under a new id."""

    def __init__(self, K: int, min_iou: int = 100, same_class: bool = True, min_area: int = 1):
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= 1024:
            raise ValueError(f"InstanceTracker: K is 1 .. 1024, got {K!r}")
        if isinstance(min_iou, bool) or int(min_iou) != min_iou or not 0 <= min_iou <= 1000:
            raise ValueError(f"InstanceTracker: min_iou is an integer 0 .. 1000 (thousandths), got {min_iou!r}")
        if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 1:
            raise ValueError(f"InstanceTracker: min_area is an integer >= 1, got {min_area!r}")
        self.K, self.min_iou, self.same_class, self.min_area = int(K), int(min_iou), bool(same_class), int(min_area)
        self.reset()

    def reset(self) -> None:
        self.next = 0
        self._map = None                  # the previous frame's component map ...
        self._part = {}                   # ... and its participants: ordinal -> (class, area, id)

    def update(self, components, rows, total):
        comp = np.asarray(components)
        rw = np.asarray(rows)
        K = self.K
        if comp.ndim != 2 or comp.dtype.kind not in "iu" or min(comp.shape) < 1:
            raise ValueError(f"InstanceTracker: components are integers [H][W], got {comp.dtype} {comp.shape}")
        if rw.shape != (K, INSTANCE_ROW) or rw.dtype.kind not in "iu":
            raise ValueError(f"InstanceTracker: rows are integers [{K}][{INSTANCE_ROW}], got {rw.dtype} {rw.shape}")
        if self._map is not None and self._map.shape != comp.shape:
            raise ValueError(f"InstanceTracker: a {comp.shape} map after {self._map.shape} ones (reset() starts a new sequence)")
        total = int(np.asarray(total).reshape(-1)[0])
        comp = comp.astype(np.int64)
        n = min(max(total, 0), K)
        cur = {j: (int(rw[j, 0]), int(rw[j, 2])) for j in range(n) if int(rw[j, 2]) >= self.min_area}
        cand = []
        if self._map is not None and self._part and cur:
            both = (self._map >= 0) & (self._map < K) & (comp >= 0) & (comp < K)
            pairs, counts = np.unique(self._map[both] * K + comp[both], return_counts=True)
            for key, ov in zip(pairs.tolist(), counts.tolist()):
                i, j = divmod(key, K)
                if i not in self._part or j not in cur:
                    continue
                cp, ap, _ = self._part[i]
                cc, ac = cur[j]
                u = ap + ac - ov
                if (cp == cc or not self.same_class) and 1000 * ov >= self.min_iou * u:
                    cand.append((ov, u, i, j))
        ids = np.full(K, -1, dtype=np.int32)
        used_i, used_j = set(), set()
        while True:                           # the most preferred candidate whose i and j are both still free (Python integers: exact)
            best = None
            for c in cand:
                if c[2] in used_i or c[3] in used_j:
                    continue
                if best is None or c[0] * best[1] > best[0] * c[1] or (c[0] * best[1] == best[0] * c[1] and c[2:] < best[2:]):
                    best = c
            if best is None:
                break
            used_i.add(best[2])
            used_j.add(best[3])
            ids[best[3]] = self._part[best[2]][2]
        for j in sorted(cur):
            if j not in used_j:
                ids[j] = self.next
                self.next += 1
        self._map = comp
        self._part = {j: (cur[j][0], cur[j][1], int(ids[j])) for j in cur}
        return ids, self.next


class MemoryTracker:
    """InstanceTracker with a memory: a track whose instrument is out of view stays alive for up to max_gap frames and is matched
    against the mask it had when it was last seen.  The numpy statement of what hip.track_instances computes on a
    hip.TrackState(..., max_gap=g), in integers throughout, matched bit for bit (VideoSegmenter(tracks=True, track_max_gap=g)).

    State: next, the next id; the live tracks id -> (class, area, age), age = the frames since the track was last matched; mem
    [H][W], the id of the track a pixel is remembered for, -1 for none.  update(components int32 [H][W], rows int64 [K][12], total) ->
    (ids int32 [K], started), one frame:
      1 an instance takes part if its ordinal j < min(total, K) and rows[j][2] >= min_area, as with InstanceTracker
      2 ov[t][j] = the pixels with mem == t and components == j, u = area[t] + area[j] - ov with area[t] the track's area at its
        last sighting, even where other instruments have overwritten part of its remembered mask since
      3 (t, j) is a candidate iff ov > 0, the classes are equal (dropped with same_class=False) and 1000 ov >= min_iou u
      4 (t, j) is preferred to (t', j') iff ov u' > ov' u in exact integers, then smaller track id, then smaller j
      5 repeatedly the most preferred candidate whose t and j are both free is matched: ids[j] = t
      6 the participants left over take next, next + 1, ... in ascending j; every other entry of ids is -1; started = next
      7 a matched track takes the instance's class and area and age 0; a new track has age 0; every other live track ages by one and
        ends when its age exceeds max_gap
      8 if more than K tracks are live now, lost tracks (age >= 1) end until K are: the largest age first, then the smallest id
      9 a pixel of a participant j takes ids[j]; any other pixel becomes -1 if its track ended or was matched in this frame (a
        matched track's mask is replaced, not extended) and stays as it is otherwise: only lost tracks keep a remembered mask
    With max_gap=0 every unmatched track ends at once and the result is InstanceTracker's wherever track ids ascend with the previous
    frame's ordinals among equally preferred pairs (the tie-break is the id here, the ordinal there).

    Two properties are deliberate.  An instrument of the same class that moves onto a lost track's remembered place inherits its id:
    the memory cannot tell a returning tool from one that takes its place.  And there is still no motion model: a track is looked
    for where it was last seen."""

    def __init__(self, K: int, max_gap: int, min_iou: int = 100, same_class: bool = True, min_area: int = 1):
        if isinstance(K, bool) or int(K) != K or not 1 <= K <= 1024:
            raise ValueError(f"MemoryTracker: K is 1 .. 1024, got {K!r}")
        if isinstance(max_gap, bool) or int(max_gap) != max_gap or not 0 <= max_gap <= 1000000:
            raise ValueError(f"MemoryTracker: max_gap is an integer 0 .. 1000000 (frames), got {max_gap!r}")
        if isinstance(min_iou, bool) or int(min_iou) != min_iou or not 0 <= min_iou <= 1000:
            raise ValueError(f"MemoryTracker: min_iou is an integer 0 .. 1000 (thousandths), got {min_iou!r}")
        if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 1:
            raise ValueError(f"MemoryTracker: min_area is an integer >= 1, got {min_area!r}")
        self.K, self.max_gap, self.min_iou = int(K), int(max_gap), int(min_iou)
        self.same_class, self.min_area = bool(same_class), int(min_area)
        self.reset()

    def reset(self) -> None:
        self.next = 0
        self.mem = None                   # int64 [H][W]: the track a pixel is remembered for
        self.live = {}                    # id -> (class, area, age)

    def update(self, components, rows, total):
        comp = np.asarray(components)
        rw = np.asarray(rows)
        K = self.K
        if comp.ndim != 2 or comp.dtype.kind not in "iu" or min(comp.shape) < 1:
            raise ValueError(f"MemoryTracker: components are integers [H][W], got {comp.dtype} {comp.shape}")
        if rw.shape != (K, INSTANCE_ROW) or rw.dtype.kind not in "iu":
            raise ValueError(f"MemoryTracker: rows are integers [{K}][{INSTANCE_ROW}], got {rw.dtype} {rw.shape}")
        if self.mem is not None and self.mem.shape != comp.shape:
            raise ValueError(f"MemoryTracker: a {comp.shape} map after {self.mem.shape} ones (reset() starts a new sequence)")
        total = int(np.asarray(total).reshape(-1)[0])
        comp = comp.astype(np.int64)
        if self.mem is None:
            self.mem = np.full(comp.shape, -1, dtype=np.int64)
        n = min(max(total, 0), K)
        cur = {j: (int(rw[j, 0]), int(rw[j, 2])) for j in range(n) if int(rw[j, 2]) >= self.min_area}
        cand = []
        if self.live and cur:
            both = (self.mem >= 0) & (comp >= 0) & (comp < K)
            pairs, counts = np.unique(self.mem[both] * K + comp[both], return_counts=True)
            for key, ov in zip(pairs.tolist(), counts.tolist()):
                t, j = divmod(key, K)
                if t not in self.live or j not in cur:
                    continue
                ct, at, _ = self.live[t]
                cc, ac = cur[j]
                u = at + ac - ov
                if (ct == cc or not self.same_class) and 1000 * ov >= self.min_iou * u:
                    cand.append((ov, u, t, j))
        ids = np.full(K, -1, dtype=np.int32)
        used_t, used_j = set(), set()
        while True:                           # the most preferred candidate whose t and j are both still free (Python integers: exact)
            best = None
            for c in cand:
                if c[2] in used_t or c[3] in used_j:
                    continue
                if best is None or c[0] * best[1] > best[0] * c[1] or (c[0] * best[1] == best[0] * c[1] and c[2:] < best[2:]):
                    best = c
            if best is None:
                break
            used_t.add(best[2])
            used_j.add(best[3])
            ids[best[3]] = best[2]
        for j in sorted(cur):
            if j not in used_j:
                ids[j] = self.next
                self.next += 1
        gone = set(used_t)                    # the tracks whose remembered pixels go: matched (replaced by the instance) or ended
        live = {int(ids[j]): (cur[j][0], cur[j][1], 0) for j in cur}
        for t, (ct, at, age) in self.live.items():
            if t in used_t:
                continue
            if age + 1 > self.max_gap:
                gone.add(t)
            else:
                live[t] = (ct, at, age + 1)
        lost = sorted((t for t in live if live[t][2] >= 1), key=lambda t: (-live[t][2], t))
        for t in lost[:max(len(live) - K, 0)]:
            del live[t]
            gone.add(t)
        self.live = live
        if gone:
            self.mem[np.isin(self.mem, sorted(gone))] = -1
        of = np.full(K, -1, dtype=np.int64)   # ordinal -> its track, participants only
        for j in cur:
            of[j] = int(ids[j])
        new = np.where((comp >= 0) & (comp < K), of[np.clip(comp, 0, K - 1)], -1)
        self.mem = np.where(new >= 0, new, self.mem)
        return ids, self.next


class TrackReport:
    """The instance report with identities: from an InstanceReport and the ids of InstanceTracker (hip.track_instances,
    VideoSegmenter(tracks=True).track_report()), row for row:

      ids      int32 [frames][K]    as given: the track of instance i of row-frame r, -1 where it takes no part
      started  int64 [frames]       the tracks begun in the row's sequence up to and including its frame
      tracks   list of dict         one per (sequence, id), in that order: sequence, track, class (at first sight), first and last
                                    (frame indices), seen (frames), frames int64 [seen], centroids float64 [seen][2] and areas
                                    int64 [seen], by the InstanceReport's own arithmetic

    Ids start at 0 with every sequence."""

    def __init__(self):
        self.report = self.ids = self.started = None
        self.tracks: List[dict] = []

    @classmethod
    def from_ids(cls, instance_report: InstanceReport, ids, started) -> "TrackReport":
        rep = instance_report
        if not isinstance(rep, InstanceReport) or rep.present is None:
            raise ValueError("TrackReport: the first argument is an InstanceReport (InstanceReport.from_rows)")
        n, K = rep.present.shape
        idv = np.asarray(ids)
        st = np.asarray(started).reshape(-1)
        if idv.ndim == 1 and n == 1:
            idv = idv[None]
        if idv.shape != (n, K) or idv.dtype.kind not in "iu":
            raise ValueError(f"TrackReport: ids are integers [{n}][{K}], got {idv.dtype} {idv.shape}")
        if st.shape != (n,) or st.dtype.kind not in "iu":
            raise ValueError(f"TrackReport: started holds one integer per frame ({n}), got {st.dtype} {st.shape}")
        if ((idv >= 0) != rep.present).any():
            raise ValueError("TrackReport: ids and the report disagree on which instances are present (another min_area?)")
        out = cls()
        out.report, out.ids, out.started = rep, idv.astype(np.int32), st.astype(np.int64)
        seen = {}
        for r in range(n):
            for i in np.nonzero(rep.present[r])[0]:
                key = (rep.sequences[r], int(idv[r, i]))
                t = seen.get(key)
                if t is None:
                    t = seen[key] = {"sequence": key[0], "track": key[1], "class": int(rep.cls[r, i]), "first": rep.frames[r],
                                     "frames": [], "centroids": [], "areas": []}
                t["frames"].append(rep.frames[r])
                t["centroids"].append(rep.centroid[r, i])
                t["areas"].append(int(rep.area[r, i]))
        for key in sorted(seen):
            t = seen[key]
            t["last"], t["seen"] = t["frames"][-1], len(t["frames"])
            t["frames"] = np.asarray(t["frames"], dtype=np.int64)
            t["centroids"] = np.asarray(t["centroids"], dtype=np.float64).reshape(-1, 2)
            t["areas"] = np.asarray(t["areas"], dtype=np.int64)
            out.tracks.append(t)
        return out

    def __len__(self) -> int:
        return len(self.report)

    def as_rows(self) -> List[dict]:
        """The InstanceReport's rows, each with its "track"."""
        out = self.report.as_rows()
        k = 0
        for r in range(len(self.report)):
            for i in np.nonzero(self.report.present[r])[0]:
                out[k]["track"] = int(self.ids[r, i])
                k += 1
        return out


def check_groups(groups, nc: int, skip: Sequence[int] = ()) -> tuple:
    """Instance groups (VideoSegmenter(instance_groups=...)) as a tuple of tuples of ints, or ValueError: a sequence of groups, each a
    sequence of at least two distinct classes 0 .. nc - 1, the groups disjoint, no class of a group in `skip`."""
    try:
        out = tuple(tuple(g) for g in groups)
    except TypeError:
        raise ValueError(f"instance_groups is a sequence of groups of classes, got {groups!r}") from None
    seen = set()
    for g in out:
        if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < nc for c in g):
            raise ValueError(f"instance_groups: a group holds classes 0 .. {nc - 1}, got {g!r}")
        if len(g) < 2 or len(set(g)) != len(g):
            raise ValueError(f"instance_groups: a group holds at least two distinct classes, got {g!r}")
        if seen & set(g):
            raise ValueError(f"instance_groups: the groups are disjoint, {sorted(seen & set(g))} are in two")
        if set(g) & set(skip):
            raise ValueError(f"instance_groups: {sorted(set(g) & set(skip))} are skipped classes (instance_skip) and cannot be parts")
        seen |= set(g)
    return tuple(tuple(int(c) for c in g) for g in out)


def group_table(groups, nc: int) -> np.ndarray:
    """Instance groups -> uint8 [256]: every grouped class maps to its group's representative, the smallest class of the group, and
    every other byte value to itself (values >= nc stay >= nc and so outside every component).  The id-coded table of hip.gt_decode;
    with it the components of a frame are label_components(group_table[labels], ...): one instrument instead of its parts."""
    table = np.arange(256, dtype=np.uint8)
    for g in check_groups(groups, nc):
        table[list(g)] = min(g)
    return table


def instance_parts(labels, components, K: int, nc: int):
    """Integer labels [n][H][W] and components [n][H][W] (label_components' map, -1 = none; or one [H][W] each) -> (parts int64
    [n][K][nc][10], contacts int64 [n][K][nc]): what hip.instance_parts gives bit for bit.

    parts[f][i][c], 0 <= i < K, 0 <= c < nc: the ten integers of the moments row over the pixels of frame f with components == i and
    labels == c (all zero where there are none).  contacts[f][i][c]: the number of ordered pairs (p, q), p a pixel of frame f with
    components[p] == i, q one of p's four neighbours inside the frame with components[q] != i and labels[q] == c - the length in
    pixel edges of the border between instance i and class c outside it.  Borders between the parts of one instance are not counted;
    a neighbour of another instance, of a skipped class or of an ordinal >= K is counted under its label.  Pixels with ordinal -1 or
    >= K are nobody's p; labels >= nc count nowhere."""
    lab, comp = np.asarray(labels), np.asarray(components)
    if lab.ndim == 2 and comp.ndim == 2:
        lab, comp = lab[None], comp[None]
    if lab.ndim != 3 or lab.dtype.kind not in "iu" or min(lab.shape) < 1:
        raise ValueError(f"instance_parts: labels are integers [n][H][W], got {lab.dtype} {lab.shape}")
    if comp.shape != lab.shape or comp.dtype.kind not in "iu":
        raise ValueError(f"instance_parts: components are integers {lab.shape} as the labels are, got {comp.dtype} {comp.shape}")
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= 1024:
        raise ValueError(f"instance_parts: K is 1 .. 1024, got {K!r}")
    if isinstance(nc, bool) or int(nc) != nc or not 1 <= nc <= 64:
        raise ValueError(f"instance_parts: 1 .. 64 classes, got {nc!r}")
    n, H, W = lab.shape
    lab, comp = lab.astype(np.int64), comp.astype(np.int64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    parts = np.zeros((n, K * nc, ROW), dtype=np.int64)
    contacts = np.zeros((n, K * nc), dtype=np.int64)
    owned = (comp >= 0) & (comp < K)
    classed = (lab >= 0) & (lab < nc)
    for f in range(n):
        m = owned[f] & classed[f]
        if m.any():
            key, x, y = comp[f][m] * nc + lab[f][m], xs[m], ys[m]
            order = np.argsort(key, kind="stable")
            key, x, y = key[order], x[order], y[order]
            first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
            at = key[first]
            for k, v in enumerate((np.ones_like(x), x, y, x * x, x * y, y * y)):
                parts[f, at, k] = np.add.reduceat(v, first)
            for k, v in enumerate((W - x, H - y, x + 1, y + 1)):
                parts[f, at, 6 + k] = np.maximum.reduceat(v, first)
        # p and q = p + (dy, dx) for the four neighbours, as slices of the frame
        for p, q in (((slice(1, None), slice(None)), (slice(None, -1), slice(None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None))),
                     ((slice(None), slice(1, None)), (slice(None), slice(None, -1))), ((slice(None), slice(None, -1)), (slice(None), slice(1, None)))):
            e = owned[f][p] & (comp[f][q] != comp[f][p]) & classed[f][q]
            contacts[f] += np.bincount(comp[f][p][e] * nc + lab[f][q][e], minlength=K * nc)
    return parts.reshape(n, K, nc, ROW), contacts.reshape(n, K, nc)


def clean_labels(labels, nc: int, min_area: int, connectivity: int = 8, keep: Sequence[int] = (), max_small: int = 4096):
    """Integer labels [n][H][W] -> (out uint8 [n][H][W], stats int32 [n][2]): the label map with its specks removed and its small holes
    filled, what hip.labels_clean gives bit for bit (VideoSegmenter(clean_area=...)).

    The components are those of label_components(labels, nc, connectivity, skip=()): of every class c < nc, nothing skipped; pixels
    with a label >= nc belong to no component, are never changed and never vote.  A component is small if its area is < min_area and
    its class is not in `keep` (the classes that are thin by nature: thread, needle); every other pixel of a class < nc is stable.
    The small components of a frame are numbered s = 0, 1, ... by their first pixel in raster order and only those with s < max_small
    can be relabelled; the rest stay as they are but still count as small: they do not vote.  votes[s][c] is the number of ordered
    pairs (p, q), p a pixel of small component s, q one of p's four neighbours inside the frame, stable and with labels[q] == c -
    always of the input labels: one pass.  Only stable pixels vote, so two adjacent specks cannot swap labels and a speck among specks
    stays.  The component's new label is the smallest c with the largest votes[s][c] if that is > 0, else its own.
    stats[f] = (the frame's number of small components, not bounded by max_small: a truncated frame shows as stats[f][0] > max_small;
    the number of pixels whose label changed)."""
    lab = np.asarray(labels)
    if lab.ndim != 3 or lab.dtype.kind not in "iu" or min(lab.shape) < 1:
        raise ValueError(f"clean_labels: labels are integers [n][H][W], got {lab.dtype} {lab.shape}")
    if isinstance(nc, bool) or int(nc) != nc or not 1 <= nc <= 64:
        raise ValueError(f"clean_labels: 1 .. 64 classes, got {nc!r}")
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or not 2 <= min_area <= 1 << 30:
        raise ValueError(f"clean_labels: min_area is an int 2 .. 2^30, got {min_area!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"clean_labels: connectivity is 4 or 8, got {connectivity!r}")
    try:
        keep = tuple(keep)
    except TypeError:
        raise ValueError(f"clean_labels: keep holds classes 0 .. 63, got {keep!r}") from None
    if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c <= 63 for c in keep):
        raise ValueError(f"clean_labels: keep holds classes 0 .. 63, got {keep!r}")
    if isinstance(max_small, bool) or not isinstance(max_small, (int, np.integer)) or not 1 <= max_small <= 65536:
        raise ValueError(f"clean_labels: max_small is an int 1 .. 65536, got {max_small!r}")
    n, H, W = lab.shape
    comp = label_components(lab, nc, connectivity, (), 1)[0].astype(np.int64)          # ordinals in raster order of the first pixel
    lab64 = lab.astype(np.int64)
    out = lab.astype(np.uint8)
    stats = np.zeros((n, 2), dtype=np.int32)
    for f in range(n):
        c, l = comp[f], lab64[f]
        inside = c >= 0
        if not inside.any():
            continue
        area = np.bincount(c[inside])
        cls = np.zeros(area.size, dtype=np.int64)
        cls[c[inside][::-1]] = l[inside][::-1]                                        # (every pixel of a component has its class)
        small = (area < min_area) & ~np.isin(cls, keep)
        number = np.cumsum(small) - 1                                                 # s of a small component
        stats[f, 0] = int(small.sum())
        live = small & (number < max_small)                                           # the ones that can be relabelled
        S = min(int(small.sum()), max_small)
        if S == 0:
            continue
        stable = inside & ~small[np.where(inside, c, 0)]
        voter = inside & live[np.where(inside, c, 0)]
        votes = np.zeros(S * nc, dtype=np.int64)
        for p, q in (((slice(1, None), slice(None)), (slice(None, -1), slice(None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None))),
                     ((slice(None), slice(1, None)), (slice(None), slice(None, -1))), ((slice(None), slice(None, -1)), (slice(None), slice(1, None)))):
            e = voter[p] & stable[q]
            votes += np.bincount(number[c[p][e]] * nc + l[q][e], minlength=S * nc)
        votes = votes.reshape(S, nc)
        best = votes.argmax(axis=1)                                                   # the first, so the smallest, class of the maximum
        old = cls[live]
        new = np.where(votes.max(axis=1) > 0, best, old)
        table = cls.copy()
        table[live] = new
        stats[f, 1] = int(area[live][new != old].sum())
        out[f][inside] = table[c[inside]].astype(np.uint8)
    return out, stats


class PartsReport:
    """What the instances are made of and what they touch (hip.instance_parts, VideoSegmenter(parts="deferred").parts_report()), per
    row-frame r, instance ordinal i < K and class c, from parts [rows][K][nc][10] and contacts [rows][K][nc]:

      has      bool    [rows][K][nc]     instance i holds pixels of class c
      area     int64   [rows][K][nc]     their number
      box, centroid, angle, axes         of that part, as InstrumentReport's, by the same arithmetic (NaN where the part is absent)
      contacts int64   [rows][K][nc]     the pixel edges between instance i and pixels of class c outside it

    With instance_groups the classes of an instance are its parts (shaft, wrist, clasper); without, an instance has the one class of
    its component.  parts(r, i) and touches(r, i) give the two as dicts, direction(r, i, a, b) the unit vector from part a to part b.
    instances / tracks: the InstanceReport and TrackReport of the same rows (None: none); as_rows() then lists the present instances
    with their class (the group's representative) and track.  frames / sequences / names as InstrumentReport's."""

    def __init__(self, parts, contacts, size: Sequence[int], names: Optional[Sequence[str]] = None, frames: Optional[Sequence[int]] = None,
                 sequences: Optional[Sequence[int]] = None, instances=None, tracks=None):
        pt, ct = np.asarray(parts), np.asarray(contacts)
        if pt.ndim == 3:
            pt = pt[None]
        if ct.ndim == 2:
            ct = ct[None]
        if pt.ndim != 4 or pt.shape[3] != ROW or pt.dtype.kind not in "iu":
            raise ValueError(f"PartsReport: parts are integers [rows][K][nc][{ROW}], got {pt.dtype} {pt.shape}")
        if ct.shape != pt.shape[:3] or ct.dtype.kind not in "iu":
            raise ValueError(f"PartsReport: contacts are integers {pt.shape[:3]} as the parts are, got {ct.dtype} {ct.shape}")
        n, K, nc = ct.shape
        if names is not None and len(names) != nc:
            raise ValueError(f"PartsReport: {len(names)} names for {nc} classes")
        for what, v in (("frames", frames), ("sequences", sequences)):
            if v is not None and len(v) != n:
                raise ValueError(f"PartsReport: {len(v)} {what} for {n} rows")
        if tracks is not None and instances is None:
            instances = tracks.report
        if instances is not None and (len(instances) != n or instances.present.shape[1] != K):
            raise ValueError(f"PartsReport: an instance report of {len(instances)} rows and {instances.present.shape[1]} instances for "
                             f"{n} rows and {K} instances")
        H, W = (int(v) for v in size)
        self.size = (H, W)
        self.names = list(names) if names is not None else None
        self.frames = [int(f) for f in frames] if frames is not None else list(range(n))
        self.sequences = [int(s) for s in sequences] if sequences is not None else [0] * n
        self.instances, self.tracks = instances, tracks
        self.moments, self.contacts = pt.astype(np.int64), ct.astype(np.int64)
        self.has = self.moments[..., 0] > 0
        self.area = self.moments[..., 0].copy()
        self.box = np.full((n, K, nc, 4), np.nan)
        self.centroid = np.full((n, K, nc, 2), np.nan)
        self.angle = np.full((n, K, nc), np.nan)
        self.axes = np.full((n, K, nc, 2), np.nan)
        for r, i, c in zip(*np.nonzero(self.has)):
            self.box[r, i, c], self.centroid[r, i, c], self.angle[r, i, c], self.axes[r, i, c] = _shape_of(self.moments[r, i, c], H, W)

    def __len__(self) -> int:
        return len(self.frames)

    def parts(self, r: int, i: int) -> dict:
        """class -> {area, box, centroid, angle, axes} for the classes instance i of row r holds, as plain Python values."""
        return {int(c): {"area": int(self.area[r, i, c]), "box": tuple(int(v) for v in self.box[r, i, c]),
                         "centroid": tuple(float(v) for v in self.centroid[r, i, c]), "angle": float(self.angle[r, i, c]),
                         "axes": tuple(float(v) for v in self.axes[r, i, c])} for c in np.nonzero(self.has[r, i])[0]}

    def touches(self, r: int, i: int) -> dict:
        """class -> the pixel edges instance i of row r shares with pixels of that class outside itself (the classes it touches)."""
        return {int(c): int(self.contacts[r, i, c]) for c in np.nonzero(self.contacts[r, i])[0]}

    def direction(self, r: int, i: int, a: int, b: int) -> np.ndarray:
        """float64 [2]: the unit vector (dx, dy) from the centroid of part a of instance i of row r to that of its part b - shaft ->
        clasper is where the instrument points; NaN where either part is absent or the centroids coincide."""
        d = self.centroid[r, i, b] - self.centroid[r, i, a]
        length = float(np.hypot(d[0], d[1]))
        return d / length if length > 0 else np.full(2, np.nan)

    def as_rows(self) -> List[dict]:
        """One dict per instance, in row order then instance order, for a log: sequence, frame, instance, class (and name) and track
        where the instance and track reports were given, parts and touches as above.  With an instance report its present instances
        are listed, else the instances that hold a pixel."""
        out = []
        some = self.instances.present if self.instances is not None else self.has.any(axis=2)
        for r in range(len(self)):
            for i in np.nonzero(some[r])[0]:
                row = {"sequence": self.sequences[r], "frame": self.frames[r], "instance": int(i)}
                if self.instances is not None:
                    row["class"] = int(self.instances.cls[r, i])
                    if self.names is not None:
                        row["name"] = self.names[row["class"]]
                if self.tracks is not None:
                    row["track"] = int(self.tracks.ids[r, i])
                row["parts"], row["touches"] = self.parts(r, int(i)), self.touches(r, int(i))
                out.append(row)
        return out


def instance_clearance(labels, components, K: int, nc: int, targets=None, max_distance=None) -> np.ndarray:
    """Integer labels [n][H][W] and components [n][H][W] (label_components' map, -1 = none; or one [H][W] each) -> int64
    [n][K][nc][3]: how near each instance comes to each class, what hip.instance_clearance gives bit for bit.

    For frame f, ordinal i < K and class c < nc, with I the pixels of components == i and Q the pixels of labels == c, the entry is
    (d2, p, q): d2 the smallest squared Euclidean pixel distance between a pixel of I and a pixel of Q, p = y W + x the smallest raster
    index among the pixels of I that reach d2, q the smallest raster index among the pixels of Q at squared distance d2 from p.  It is
    (-1, -1, -1) where I is empty, c is not in `targets` (default: every class 0 .. nc - 1), Q is empty, instance i itself holds a
    pixel of class c, or max_distance = r is given and d2 > r^2.  Ordinals -1 and >= K are nobody's, labels >= nc are nowhere, as in
    instance_parts.

    Own classes are left out on purpose: the kernels measure against one plane of distances per class, and a plane cannot leave out
    the instance's own pixels, so the distance between two instruments of one class is not measured here.  With instance_groups an
    arm's own shaft, wrist and clasper are its own classes; everything else is measured.

    Only contour pixels are compared (boundary.contour, of the instance's mask and of the class's): were a pixel of a nearest pair
    surrounded by its own set, its neighbour a step towards the other pixel would be nearer."""
    from .boundary import contour, nearest_d2
    lab, comp = np.asarray(labels), np.asarray(components)
    if lab.ndim == 2 and comp.ndim == 2:
        lab, comp = lab[None], comp[None]
    if lab.ndim != 3 or lab.dtype.kind not in "iu" or min(lab.shape) < 1:
        raise ValueError(f"instance_clearance: labels are integers [n][H][W], got {lab.dtype} {lab.shape}")
    if comp.shape != lab.shape or comp.dtype.kind not in "iu":
        raise ValueError(f"instance_clearance: components are integers {lab.shape} as the labels are, got {comp.dtype} {comp.shape}")
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= 1024:
        raise ValueError(f"instance_clearance: K is 1 .. 1024, got {K!r}")
    if isinstance(nc, bool) or int(nc) != nc or not 1 <= nc <= 64:
        raise ValueError(f"instance_clearance: 1 .. 64 classes, got {nc!r}")
    if targets is None:
        targets = range(nc)
    try:
        targets = sorted({int(c) for c in targets})
    except TypeError:
        raise ValueError(f"instance_clearance: targets holds classes 0 .. {nc - 1}, got {targets!r}") from None
    if any(not 0 <= c < nc for c in targets):
        raise ValueError(f"instance_clearance: targets holds classes 0 .. {nc - 1}, got {targets!r}")
    if max_distance is not None and (isinstance(max_distance, bool) or int(max_distance) != max_distance or max_distance < 0):
        raise ValueError(f"instance_clearance: max_distance is None or an int >= 0, got {max_distance!r}")
    n, H, W = lab.shape
    lab, comp = lab.astype(np.int64), comp.astype(np.int64)
    out = np.full((n, K, nc, 3), -1, dtype=np.int64)
    for f in range(n):
        there = {c: np.argwhere(contour(lab[f] == c)) for c in targets}                  # (argwhere lists in raster order)
        there = {c: pts for c, pts in there.items() if len(pts)}
        owned = (comp[f] >= 0) & (comp[f] < K)
        for i in np.unique(comp[f][owned]) if there else ():
            inside = comp[f] == i
            own = set(np.unique(lab[f][inside]).tolist())
            mine = np.argwhere(contour(inside))
            for c, pts in there.items():
                if c in own:
                    continue
                d = nearest_d2(mine, pts)
                k = int(np.argmin(d))                                                     # the first of the smallest: the smallest index
                if max_distance is not None and d[k] > int(max_distance) ** 2:
                    continue
                e = ((pts - mine[k]) ** 2).sum(axis=1)
                j = int(np.argmin(e))
                out[f, i, c] = d[k], mine[k, 0] * W + mine[k, 1], pts[j, 0] * W + pts[j, 1]
    return out


class ClearanceReport:
    """How near the instances come to what they do not touch (hip.instance_clearance, VideoSegmenter(clearance="deferred")
    .clearance_report()), per row-frame r, instance ordinal i < K and class c, from clearance int64 [rows][K][nc][3], the triples
    (d2, p, q) of instance_clearance, (-1, -1, -1) where nothing is measured:

      measured bool    [rows][K][nc]     a distance exists
      d2       int64   [rows][K][nc]     the squared distance in pixels, -1 where none
      p, q     int64   [rows][K][nc]     the raster indices y W + x of the instance's pixel and of the class's, -1 where none

    distance(r, i) gives class -> sqrt(d2) for the measured classes, nearest(r, i, c) the two pixels ((y, x), (y, x)).
    instances / tracks: the InstanceReport and TrackReport of the same rows (None: none); as_rows() then lists the present instances
    with their class and track.  frames / sequences / names as InstrumentReport's."""

    def __init__(self, clearance, size: Sequence[int], names: Optional[Sequence[str]] = None, frames: Optional[Sequence[int]] = None,
                 sequences: Optional[Sequence[int]] = None, instances=None, tracks=None):
        cl = np.asarray(clearance)
        if cl.ndim == 3:
            cl = cl[None]
        if cl.ndim != 4 or cl.shape[3] != 3 or cl.dtype.kind not in "iu":
            raise ValueError(f"ClearanceReport: clearance is integers [rows][K][nc][3], got {cl.dtype} {cl.shape}")
        n, K, nc = cl.shape[:3]
        if names is not None and len(names) != nc:
            raise ValueError(f"ClearanceReport: {len(names)} names for {nc} classes")
        for what, v in (("frames", frames), ("sequences", sequences)):
            if v is not None and len(v) != n:
                raise ValueError(f"ClearanceReport: {len(v)} {what} for {n} rows")
        if tracks is not None and instances is None:
            instances = tracks.report
        if instances is not None and (len(instances) != n or instances.present.shape[1] != K):
            raise ValueError(f"ClearanceReport: an instance report of {len(instances)} rows and {instances.present.shape[1]} instances "
                             f"for {n} rows and {K} instances")
        H, W = (int(v) for v in size)
        self.size = (H, W)
        self.names = list(names) if names is not None else None
        self.frames = [int(f) for f in frames] if frames is not None else list(range(n))
        self.sequences = [int(s) for s in sequences] if sequences is not None else [0] * n
        self.instances, self.tracks = instances, tracks
        self.clearance = cl.astype(np.int64)
        self.d2, self.p, self.q = (self.clearance[..., k] for k in range(3))
        self.measured = self.d2 >= 0
        if self.measured.any() and (W < 1 or max(self.p.max(), self.q.max()) >= H * W):
            raise ValueError(f"ClearanceReport: pixel indices up to {max(self.p.max(), self.q.max())} in a frame of {H} x {W}")

    def __len__(self) -> int:
        return len(self.frames)

    def distance(self, r: int, i: int) -> dict:
        """class -> the distance in pixels (sqrt of d2) from instance i of row r to the nearest pixel of that class, for the classes
        measured."""
        return {int(c): float(np.sqrt(float(self.d2[r, i, c]))) for c in np.nonzero(self.measured[r, i])[0]}

    def nearest(self, r: int, i: int, c: int):
        """((y, x), (y, x)): the pixel of instance i of row r nearest to class c and the pixel of the class nearest to it; None where
        nothing is measured."""
        if not self.measured[r, i, c]:
            return None
        W = self.size[1]
        p, q = int(self.p[r, i, c]), int(self.q[r, i, c])
        return (p // W, p % W), (q // W, q % W)

    def as_rows(self) -> List[dict]:
        """One dict per instance, in row order then instance order, for a log: sequence, frame, instance, class (and name) and track
        where the instance and track reports were given, distance as above and nearest as class -> ((y, x), (y, x)).  With an
        instance report its present instances are listed, else the instances with a measured class."""
        out = []
        some = self.instances.present if self.instances is not None else self.measured.any(axis=2)
        for r in range(len(self)):
            for i in np.nonzero(some[r])[0]:
                row = {"sequence": self.sequences[r], "frame": self.frames[r], "instance": int(i)}
                if self.instances is not None:
                    row["class"] = int(self.instances.cls[r, i])
                    if self.names is not None:
                        row["name"] = self.names[row["class"]]
                if self.tracks is not None:
                    row["track"] = int(self.tracks.ids[r, i])
                row["distance"] = self.distance(r, int(i))
                row["nearest"] = {c: self.nearest(r, int(i), c) for c in row["distance"]}
                out.append(row)
        return out
