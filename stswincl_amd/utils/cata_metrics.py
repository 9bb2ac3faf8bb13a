"""Drop-in for ``utils.cata_metrics`` of the CaDIS package (segcata/utils/cata_metrics.py): one confusion matrix over a whole test
set, then pixel accuracy (PA), per-class pixel accuracy (PAC) and intersection over union (mIoU).

Same names, arguments and return values.  The matrix is float64 [num_classes][num_classes], rows ground truth, columns prediction;
a pixel counts only when both its ground truth and its prediction lie in [0, num_classes), so the ignore label (>= num_classes)
drops out.  Per-class values of a class absent from both sides are NaN (0 / 0) and the means skip them (``np.nanmean``).

``ConfusionMatrix.update_from_logits`` adds a batch of logits straight from the GPU: bilinear resize, argmax and counting in one
HIP launch (stswin_upsample_argmax_cm), without a label map on the host.

Left out: the reference's ``segmentation_metrics_task1`` .. ``task3`` unpack three values from ``segmentation_metrics``, which
returns five, so they raise ValueError whenever they are called; call ``segmentation_metrics(gt, pred, num_classes=8 | 17 | 25)``.
"""
from __future__ import annotations

import numpy as np


class ConfusionMatrix:
    """Accumulates a confusion matrix until reset(); the ignore label must be >= num_classes."""

    def __init__(self, num_classes):
        super().__init__()
        self.num_classes = num_classes
        self.confusion_matrix = np.zeros((num_classes, num_classes))

    def reset(self):
        self.confusion_matrix = np.zeros((self.num_classes, self.num_classes))

    def get_confusion_matrix(self):
        return self.confusion_matrix

    def update_confusion_matrix(self, gt_mask, pre_mask):
        """Count one ground-truth / prediction pair of equal shape; -> the updated matrix."""
        assert gt_mask.shape == pre_mask.shape, f" {gt_mask.shape} == {pre_mask.shape}"
        n = self.num_classes
        g = np.asarray(gt_mask)
        p = np.asarray(pre_mask)
        keep = (g >= 0) & (g < n) & (p >= 0) & (p < n)
        flat = g[keep].astype(np.int64) * n + p[keep].astype(np.int64)
        self.confusion_matrix += np.bincount(flat, minlength=n * n).reshape(n, n)
        return self.confusion_matrix

    def update_from_logits(self, logits, gt, size, align_corners=False):
        """Count the predictions of NCHW logits [F][nc][h][w] (torch, bf16 / fp32, on the GPU): F.interpolate(logits, size,
        'bilinear', align_corners) -> argmax (cata_test.py:129-131), against gt int64 [F][*size] on the same device.  The counts are
        exact 64-bit integers on the device, added to this float64 matrix once per call; -> the updated matrix."""
        import torch
        from .. import hip
        gt = torch.as_tensor(gt).to(logits.device, torch.int64)
        if gt.dim() == 2:
            gt = gt[None]
        cm = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=logits.device)
        hip.upsample_argmax_cm(logits, int(size[0]), int(size[1]), gt=gt, cm=cm, align_corners=align_corners, labels=False)
        self.confusion_matrix += cm.cpu().numpy()
        return self.confusion_matrix


def _per_class(num, den):
    """num / den per class, NaN where den == 0 (the reference's 0 / 0) without ever dividing by zero: no floating-point exception
    is raised, whatever the process's exception mask."""
    num = np.asarray(num, dtype=np.float64)
    den = np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den != 0)


def _nanmean(v):
    """np.nanmean (the sum of the non-NaN values over their count, summed as np.nanmean does), NaN when every value is NaN."""
    keep = ~np.isnan(v)
    cnt = int(keep.sum())
    return np.sum(np.where(keep, v, 0.)) / cnt if cnt else np.float64(np.nan)


def pixel_accuracy(confusion_matrix):
    """Correct pixels over all counted pixels."""
    cm = np.asarray(confusion_matrix)
    total = cm.sum()
    return np.trace(cm) / total if total else np.float64(np.nan)


def pixel_accuracy_class(confusion_matrix):
    """-> (mean over classes, per-class accuracy): correct pixels of a class over its ground-truth pixels."""
    cm = np.asarray(confusion_matrix)
    acc_c = _per_class(np.diagonal(cm), cm.sum(axis=1))
    return _nanmean(acc_c), acc_c


def per_class_intersection_over_union(confusion_matrix):
    """Per-class IoU: true positives over (ground-truth pixels + predicted pixels - true positives)."""
    cm = np.asarray(confusion_matrix)
    tp = np.diagonal(cm)
    return _per_class(tp, cm.sum(axis=1) + cm.sum(axis=0) - tp)


def mean_intersection_over_union(confusion_matrix):
    """-> (mean IoU over classes, per-class IoU)."""
    iou = per_class_intersection_over_union(confusion_matrix)
    return _nanmean(iou), iou


def _pooled(gt_masks, pred_masks, num_classes):
    assert len(gt_masks) == len(pred_masks)
    acc = ConfusionMatrix(num_classes=num_classes)
    for g, p in zip(gt_masks, pred_masks):
        acc.update_confusion_matrix(g, p)
    return acc.get_confusion_matrix()


def segmentation_metrics(gt_masks, pred_masks, num_classes):
    """One matrix over all mask pairs -> (pa, pac, pac_c, miou, miou_c)."""
    cm = _pooled(gt_masks, pred_masks, num_classes)
    pac, pac_c = pixel_accuracy_class(cm)
    miou, miou_c = mean_intersection_over_union(cm)
    return pixel_accuracy(cm), pac, pac_c, miou, miou_c


def iou_per_class_metrics(gt_masks, pred_masks, num_classes):
    """One matrix over all mask pairs -> the per-class IoU vector."""
    return per_class_intersection_over_union(_pooled(gt_masks, pred_masks, num_classes))
