"""Run-length masks: the definition of hip.rle_encode (stswin_rle_encode) in numpy, and what is made of its runs on the host - dense
maps, COCO's per-object `counts` (list and compressed string) and MOTS text lines - without touching a dense mask.  No torch.

A map m [H][W] is read in column-major order, v[p] = m[y][x] with p = x H + y: COCO's order, in which a run continues from the bottom
of column x - 1 into the top of column x.  A run starts at p = 0 and wherever v[p] != v[p - 1]; R is the number of run starts.  The
run list of a map is runs[i] = (p_i, v[p_i]) in ascending p: run i covers p_i .. p_{i+1} - 1, the last one up to H W - 1.  A label map
of surgical instruments is a few thousand runs where the map itself is 1.3 MB (uint8) or 5.2 MB (int32 components) at 1024 x 1280.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

MAX_RUNS = 1 << 20            # the largest `cap` of stswin_rle_encode


def _maps(maps) -> np.ndarray:
    m = np.asarray(maps)
    if m.dtype not in (np.uint8, np.int32) or m.ndim not in (2, 3) or m.size == 0:
        raise ValueError(f"rle: maps are uint8 or int32 [n][H][W] or [H][W], not empty, got {m.dtype} {m.shape}")
    return m[None] if m.ndim == 2 else m


def encode(maps, cap: int):
    """uint8 or int32 maps [n][H][W] (or one [H][W]) -> (runs int32 [n][cap][2], count int32 [n]): count[f] = R, not bounded by cap;
    runs[f][i] = (p_i, v[p_i]) for i < min(R, cap) - the first cap runs are the ones kept - and zero from there on.  uint8 values are
    zero-extended, int32 values kept as they are (-1 included)."""
    m = _maps(maps)
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= MAX_RUNS:
        raise ValueError(f"rle.encode: cap is an integer 1 .. {MAX_RUNS}, got {cap!r}")
    n = m.shape[0]
    runs = np.zeros((n, cap, 2), dtype=np.int32)
    count = np.zeros(n, dtype=np.int32)
    for f in range(n):
        v = m[f].T.reshape(-1)
        p = np.concatenate(([0], np.nonzero(v[1:] != v[:-1])[0] + 1))
        count[f] = len(p)
        k = min(len(p), cap)
        runs[f, :k, 0] = p[:k]
        runs[f, :k, 1] = v[p[:k]]
    return runs, count


def _one(runs, count, size, what: str):
    """One map's runs [cap][2] and count, checked -> (p int64 [R], v int64 [R], lengths int64 [R], H, W)."""
    rn = np.asarray(runs)
    c = np.asarray(count).reshape(-1)
    if rn.ndim != 2 or rn.shape[1] != 2 or rn.dtype.kind not in "iu" or c.shape != (1,) or c.dtype.kind not in "iu":
        raise ValueError(f"{what}: one map's runs are integers [cap][2] with one count, got {rn.dtype} {rn.shape} and {c.shape}")
    H, W = (int(s) for s in size)
    R = int(c[0])
    if R > rn.shape[0]:
        raise ValueError(f"{what}: the map has {R} runs and only the first {rn.shape[0]} were kept (a larger cap / mask_runs keeps all)")
    if R < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: a map of {H} x {W} with {R} runs")
    p = rn[:R, 0].astype(np.int64)
    if p[0] != 0 or (np.diff(p) <= 0).any() or p[-1] >= H * W:
        raise ValueError(f"{what}: the run starts do not ascend from 0 within {H} x {W}")
    return p, rn[:R, 1].astype(np.int64), np.diff(np.append(p, H * W)), H, W


def decode(runs, count, size: Sequence[int], dtype=np.int32) -> np.ndarray:
    """One map's runs [cap][2] and count -> the dense map [H][W] (size = (H, W)).  Raises ValueError when count > cap."""
    p, v, lengths, H, W = _one(runs, count, size, "rle.decode")
    return np.repeat(v, lengths).astype(dtype).reshape(W, H).T.copy()


def mask_counts(runs, count, size: Sequence[int], values: Sequence[int]) -> List[int]:
    """COCO's uncompressed `counts` of the binary mask (m in values) of one map, from its runs in O(runs): alternating off / on
    lengths in column-major order, starting with an off run that may be 0."""
    p, v, lengths, H, W = _one(runs, count, size, "rle.mask_counts")
    on = np.isin(v, np.asarray(list(values), dtype=np.int64))
    first = np.concatenate(([0], np.nonzero(on[1:] != on[:-1])[0] + 1))        # the runs at which the mask changes
    out = np.add.reduceat(lengths, first).tolist()
    return [0] + out if on[0] else out


def counts_to_string(counts: Sequence[int]) -> str:
    """COCO's compressed `counts` string (pycocotools' rleToString): count i > 2 as its difference to count i - 2, then 5 bits per
    character, low bits first, bit 5 = more follow, bit 4 of the last one = the sign; character = chr(bits + 48)."""
    cs = [int(c) for c in counts]
    out = []
    for i, x in enumerate(cs):
        if i > 2:
            x -= cs[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if c & 0x10 else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def string_to_counts(s: str) -> List[int]:
    """The inverse of counts_to_string (pycocotools' rleFrString)."""
    out: List[int] = []
    i = 0
    while i < len(s):
        x = k = 0
        more = True
        while more:
            if i >= len(s):
                raise ValueError("rle.string_to_counts: the string ends inside a count")
            c = ord(s[i]) - 48
            if not 0 <= c < 64:
                raise ValueError(f"rle.string_to_counts: character {s[i]!r} at {i}")
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            i += 1
            k += 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(out) > 2:
            x += out[-2]
        out.append(x)
    return out


class MaskReport:
    """The run-length masks of the frames of an evaluation (VideoSegmenter(masks="deferred").mask_report()), row for row:

      size       (H, W) of the maps
      source     "labels": the runs' values are classes;  "instances": they are the per-frame ordinals of label_components, -1 = none
      frames, sequences   the row's frame index and its sequence's ordinal, as the instrument report's
      runs       int32 [rows][cap][2]   encode()'s runs
      count      int32 [rows]           the number of runs, not bounded by cap
      truncated  bool  [rows]           count > cap: the row's map cannot be rebuilt (dense, objects and mots_lines raise ValueError)

    instances / tracks: the utils.instruments.InstanceReport (source "instances": classes, areas, which instances are present) and
    TrackReport of the same rows; min_area, skip (source "labels": classes left out) and names (per class) shape objects().
    confidence: the utils.confidence.ConfidenceReport of the same rows (None: none); objects() then adds "score", the mean probability
    of the instance's pixels, or of the class's for source "labels" - what COCO-style result files ask for per object."""

    def __init__(self, runs, count, size: Sequence[int], source: str = "labels", frames: Optional[Sequence[int]] = None,
                 sequences: Optional[Sequence[int]] = None, instances=None, tracks=None, min_area: int = 1, skip: Sequence[int] = (),
                 names: Optional[Sequence[str]] = None, confidence=None):
        rn = np.asarray(runs)
        c = np.asarray(count).reshape(-1)
        if rn.ndim == 2:
            rn = rn[None]
        if rn.ndim != 3 or rn.shape[2] != 2 or rn.dtype.kind not in "iu" or c.shape != (rn.shape[0],) or c.dtype.kind not in "iu":
            raise ValueError(f"MaskReport: runs are integers [rows][cap][2] with one count per row, got {rn.dtype} {rn.shape} and {c.shape}")
        if source not in ("labels", "instances"):
            raise ValueError(f"MaskReport: source is 'labels' or 'instances', got {source!r}")
        n = rn.shape[0]
        for what, v in (("frames", frames), ("sequences", sequences)):
            if v is not None and len(v) != n:
                raise ValueError(f"MaskReport: {len(v)} {what} for {n} rows")
        if tracks is not None and instances is None:
            instances = tracks.report
        if instances is not None and (source != "instances" or len(instances) != n):
            raise ValueError(f"MaskReport: an instance report of {len(instances)} rows for {n} rows of source {source!r}")
        if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or min_area < 1:
            raise ValueError(f"MaskReport: min_area is an integer >= 1, got {min_area!r}")
        self.size = (int(size[0]), int(size[1]))
        self.source = source
        self.frames = [int(f) for f in frames] if frames is not None else list(range(n))
        self.sequences = [int(s) for s in sequences] if sequences is not None else [0] * n
        self.runs, self.count = rn.astype(np.int32), c.astype(np.int32)
        self.truncated = self.count > rn.shape[1]
        self.instances, self.tracks = instances, tracks
        self.min_area, self.skip = int(min_area), tuple(int(s) for s in skip)
        self.names = list(names) if names is not None else None
        if confidence is not None:
            if len(confidence) != n:
                raise ValueError(f"MaskReport: a confidence report of {len(confidence)} rows for {n} rows")
            if source == "instances" and confidence.instance_mean is None:
                raise ValueError("MaskReport: source 'instances' needs a confidence report with instance sums")
        self.confidence = confidence

    def __len__(self) -> int:
        return len(self.frames)

    def _score(self, r: int, d: dict):
        """The mean probability of the object's pixels: the instance's, or the class's for source "labels" (None: it has no pixels, or
        its ordinal lies beyond the K of the sums)."""
        mean = self.confidence.instance_mean if self.source == "instances" else self.confidence.mean
        i = d["instance"] if self.source == "instances" else d["cls"]
        return float(mean[r, i]) if i < mean.shape[1] and not np.isnan(mean[r, i]) else None

    def dense(self, r: int) -> np.ndarray:
        """Row r's map int32 [H][W]."""
        return decode(self.runs[r], self.count[r], self.size)

    def _name(self, c):
        return self.names[c] if self.names is not None and c is not None else None

    def objects(self, r: int) -> List[dict]:
        """Row r's objects, each with its mask as COCO RLE {"size": [H, W], "counts": compressed string}.  Source "instances": one dict
        per present instance (i < min(total, K) with area >= min_area; without an instance report: every ordinal >= 0 with that
        area, cls None) with instance, cls, name, track (with a track report), size, counts.  Source "labels": one per class with at
        least min_area pixels and not in skip, with cls, name, size, counts."""
        p, v, lengths, H, W = _one(self.runs[r], self.count[r], self.size, "MaskReport.objects")
        out = []
        if self.source == "instances" and self.instances is not None:
            rep = self.instances
            for i in np.nonzero(rep.present[r])[0]:
                d = {"instance": int(i), "cls": int(rep.cls[r, i]), "name": self._name(int(rep.cls[r, i]))}
                if self.tracks is not None:
                    d["track"] = int(self.tracks.ids[r, i])
                out.append(d)
        else:
            values, inverse = np.unique(v, return_inverse=True)
            areas = np.bincount(inverse, weights=lengths).astype(np.int64)
            for val, a in zip(values.tolist(), areas.tolist()):
                if a < self.min_area or val < 0:
                    continue
                if self.source == "instances":
                    out.append({"instance": val, "cls": None, "name": None})
                elif val not in self.skip:
                    out.append({"cls": val, "name": self._name(val)})
        for d in out:
            d["size"] = [H, W]
            d["counts"] = counts_to_string(mask_counts(self.runs[r], self.count[r], self.size, (d.get("instance", d["cls"]),)))
            if self.confidence is not None:
                d["score"] = self._score(r, d)
        return out

    def mots_lines(self, sequence: int = 0) -> List[str]:
        """The MOTS text lines of one sequence, "{frame} {id} {cls} {H} {W} {rle}" with id = cls * 1000 + track, in frame then instance
        order; frames without objects give no line.  Needs tracks; ValueError for a track id >= 1000 or a truncated row."""
        if self.tracks is None:
            raise ValueError("MaskReport.mots_lines: needs the track ids (VideoSegmenter(tracks=True) with report='deferred')")
        lines = []
        for r in range(len(self)):
            if self.sequences[r] != sequence:
                continue
            for d in self.objects(r):
                if d["track"] >= 1000:
                    raise ValueError(f"MaskReport.mots_lines: track {d['track']} of frame {self.frames[r]} does not fit id = cls * 1000 + track")
                lines.append(f"{self.frames[r]} {d['cls'] * 1000 + d['track']} {d['cls']} {self.size[0]} {self.size[1]} {d['counts']}")
        return lines
