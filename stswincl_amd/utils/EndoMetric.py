"""Drop-in for ``utils.EndoMetric`` (seg18/utils/EndoMetric.py) plus the fused device-side evaluation step of
seg18/test.py:153-175: ``predict_and_score`` resizes the logits (bilinear, align_corners=True), takes the arg-max and
accumulates the per-class counts in one HIP kernel; Dice / IoU then follow the reference's formulas per frame over the
classes present in the ground truth (class 0 = background is skipped)."""
from __future__ import annotations

import numpy as np
import torch

from .. import hip


def jaccard(y_true, y_pred):
    inter = (y_true * y_pred).sum()
    union = y_true.sum() + y_pred.sum() - inter
    return (inter + 1e-15) / (union + 1e-15)


def dice(y_true, y_pred):
    return (2 * (y_true * y_pred).sum() + 1e-15) / (y_true.sum() + y_pred.sum() + 1e-15)


def general_dice(y_true, y_pred):
    return [[c, dice(y_true == c, y_pred == c)] for c in set(np.asarray(y_true).flatten()) if c != 0]


def general_jaccard(y_true, y_pred):
    return [[c, jaccard(y_true == c, y_pred == c)] for c in set(np.asarray(y_true).flatten()) if c != 0]


def predict_and_score(logits: torch.Tensor, size, gt: torch.Tensor = None):
    """logits (F,nc,h,w) on the GPU -> labels (F,H,W) uint8 and, with gt (F,H,W) int64, per-frame lists
    [[class, dice], ...], [[class, iou], ...] exactly as general_dice / general_jaccard would give them."""
    H, W = size
    labels, counts = hip.upsample_argmax(logits, H, W, gt)
    if gt is None:
        return labels
    cnt = counts.cpu().numpy().astype(np.float64)          # [F][3][nc]: |gt|, |pred|, |gt & pred|
    dices, ious = [], []
    for f in range(cnt.shape[0]):
        g, p, i = cnt[f]
        present = [c for c in range(1, cnt.shape[2]) if g[c] > 0]
        dices.append([[c, (2 * i[c] + 1e-15) / (g[c] + p[c] + 1e-15)] for c in present])
        ious.append([[c, (i[c] + 1e-15) / (g[c] + p[c] - i[c] + 1e-15)] for c in present])
    return labels, dices, ious


def _frame_lists(cnt: np.ndarray):
    """float64 counts [F][3][nc] (|gt|, |pred|, |gt & pred| per class) -> per-frame [[class, dice], ...], [[class, iou], ...] over the
    classes > 0 present in the ground truth."""
    dices, ious = [], []
    for f in range(cnt.shape[0]):
        g, p, i = cnt[f]
        present = [c for c in range(1, cnt.shape[2]) if g[c] > 0]
        dices.append([[c, (2 * i[c] + 1e-15) / (g[c] + p[c] + 1e-15)] for c in present])
        ious.append([[c, (i[c] + 1e-15) / (g[c] + p[c] - i[c] + 1e-15)] for c in present])
    return dices, ious


class EndoScores:
    """What the reference's val_map prints (seg18/test.py:140-207, seg18/train_swin.py:185-252), from per-frame class counts.

    dices, ious   per frame [[class, value], ...] over the classes > 0 present in the frame's ground truth: predict_and_score's lists
    sequences     per frame, the ordinal of its sequence
    count         frames
    dice, iou     mean over the frames of the frame's mean over its present classes
    dice_seq, iou_seq   float64 [sequences]: the same mean over the frames of one sequence (the reference prints them with four
                  decimals; these are not rounded)
    dice_each, iou_each float64 [nc]: per class, the mean of its values over the frames that have it
    tool_each     float64 [nc]: the number of frames that have the class
    empty_frames  indices (rows of the counts) of the frames whose ground truth has no class > 0

    All sums run in float64 in frame order, the frame's mean is np.mean of its list, as the reference computes them.  Its oddities are
    kept: a frame without any class > 0 has the mean of an empty list, NaN, and makes dice, iou and its sequence's entries NaN
    (empty_frames says which frames did it); a class that no frame has is 0 / 0 = NaN in dice_each and iou_each, class 0 always."""

    def __init__(self, dices, ious, sequences, classes: int):
        self.dices, self.ious = dices, ious
        self.sequences = [int(s) for s in sequences]
        self.count = len(dices)
        nseq = max(self.sequences) + 1 if self.sequences else 0
        total = np.zeros((2,))
        per_seq = np.zeros((2, nseq))
        count_seq = np.zeros((nseq,))
        self.dice_each, self.iou_each, self.tool_each = np.zeros((classes,)), np.zeros((classes,)), np.zeros((classes,))
        self.empty_frames = []
        for f, (d, j, s) in enumerate(zip(dices, ious, self.sequences)):
            for (c, dv), (_, jv) in zip(d, j):
                self.dice_each[c] += dv
                self.iou_each[c] += jv
                self.tool_each[c] += 1
            if d:
                frame = (np.mean([v for _, v in d]), np.mean([v for _, v in j]))
            else:                                                 # np.mean([]) without its warning
                frame = (np.float64("nan"), np.float64("nan"))
                self.empty_frames.append(f)
            for k in range(2):
                total[k] += frame[k]
                per_seq[k][s] += frame[k]
            count_seq[s] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            total /= self.count
            per_seq /= count_seq
            self.dice_each /= self.tool_each
            self.iou_each /= self.tool_each
        self.dice, self.iou = total[0], total[1]
        self.dice_seq, self.iou_seq = per_seq[0], per_seq[1]

    @classmethod
    def from_counts(cls, counts, sequences=None) -> "EndoScores":
        """counts: integer [F][3][nc], the rows hip.upsample_argmax returns with gt (a torch tensor on any device, or numpy);
        sequences: per row the ordinal of its sequence (default: all 0)."""
        if isinstance(counts, torch.Tensor):
            counts = counts.cpu().numpy()
        cnt = np.asarray(counts).astype(np.float64)
        if cnt.ndim != 3 or cnt.shape[1] != 3:
            raise ValueError(f"EndoScores.from_counts: counts must be [F][3][nc], got {cnt.shape}")
        sequences = [0] * cnt.shape[0] if sequences is None else list(sequences)
        if len(sequences) != cnt.shape[0] or any(int(s) != s or s < 0 for s in sequences):
            raise ValueError(f"EndoScores.from_counts: one sequence ordinal >= 0 per row of counts, got {len(sequences)} for {cnt.shape[0]}")
        dices, ious = _frame_lists(cnt)
        return cls(dices, ious, sequences, cnt.shape[2])
