"""Float64 reference of the OHEM cross entropy (OhemCELoss2D, seg18/utils/losses.py:32-40) in the call forms of the library's
kernels (stswincl_amd/csrc/headops.hip: ce_fwd, ohem_select, ce_bwd; include/stswin_hip.h, a15 section).

Shared by tests/test_ohem_ref.py (CPU: the reference against float64 autograd of F.cross_entropy and against a sort-based
implementation) and tests/test_hip_ohem_contract.py (GPU: the kernels against it).  Plain torch, on whatever device its inputs live on.

  pixel_loss  per-pixel CE of logits [F][nc][H][W] (or [F][nc][HW]) with ignore_index -> 0; a label outside [0, nc) that is not
              ignore_index raises, as F.cross_entropy does.
  value       the OHEM loss: n_hard = #(loss > thresh); n_hard > n_min (the reference's "sorted[n_min] > thresh") -> mean of the
              losses above thresh; else the mean of the n_min largest.
  selection   the per-pixel weights of that value's gradient, taken from GIVEN losses (a GPU test hands it the kernel's float32
              losses, so that a selection disagreement is not confused with an arithmetic one).  Top-n_min branch with t losses
              tied at the cut kth and k_rem of them inside the top n_min: each tied pixel gets k_rem / (t * n_min) - the gradient of
              sort-then-slice averaged over the orders of the tied pixels (the value does not depend on that order).
  gradient    dlogits = g * w * (softmax - onehot) in float64, 0 at ignore_index.
"""
from __future__ import annotations

import torch

F64 = torch.float64


def _flat(logits):
    return logits.to(F64).reshape(logits.shape[0], logits.shape[1], -1)           # [F][nc][HW]


def check_labels(labels, nc, ignore_index):
    bad = (labels != ignore_index) & ((labels < 0) | (labels >= nc))
    if bool(bad.any()):
        raise ValueError(f"{int(bad.sum())} label(s) outside [0, {nc}) that are not ignore_index")


def pixel_loss(logits, labels, ignore_index):
    """float64 [F * HW] per-pixel cross entropy (log-sum-exp - logit of the label), 0 at ignore_index."""
    x = _flat(logits)
    nc = x.shape[1]
    lab = labels.reshape(x.shape[0], -1).to(torch.long)
    check_labels(lab, nc, ignore_index)
    keep = lab != ignore_index
    safe = torch.where(keep, lab, torch.zeros_like(lab))
    lse = torch.logsumexp(x, dim=1)
    xl = x.gather(1, safe.unsqueeze(1)).squeeze(1)
    return torch.where(keep, lse - xl, torch.zeros((), dtype=F64, device=x.device)).reshape(-1)


def value(loss, n_min, thresh):
    """The OHEM loss of per-pixel losses (float64 sums of the given values)."""
    l = loss.to(F64).reshape(-1)
    n_hard = int((l > thresh).sum())
    if n_hard > n_min:
        return l[l > thresh].sum() / n_hard
    return torch.topk(l, n_min).values.sum() / n_min


def selection(loss, n_min, thresh):
    """Branch, cut and per-pixel weights (float64 [n]) of the OHEM value's gradient from the given losses (compared as they are)."""
    l = loss.reshape(-1)
    n_hard = int((l > thresh).sum())
    w = torch.zeros(l.numel(), dtype=F64, device=l.device)
    if n_hard > n_min:
        w[l > thresh] = 1.0 / n_hard
        return {"topk": False, "cut": float(thresh), "n_hard": n_hard, "ties": 0, "k_rem": 0, "w": w}
    kth = torch.topk(l, n_min).values[-1]
    above = l > kth
    tie = l == kth
    n_above, t = int(above.sum()), int(tie.sum())
    k_rem = n_min - n_above
    assert 1 <= k_rem <= t
    w[above] = 1.0 / n_min
    w[tie] = k_rem / (t * n_min)
    return {"topk": True, "cut": float(kth), "n_hard": n_hard, "ties": t, "k_rem": k_rem, "w": w}


def gradient(logits, labels, w, ignore_index, g=1.0):
    """dlogits [F][nc][...] float64 = g * w(px) * (softmax - onehot), 0 at ignore_index; w = selection(...)["w"]."""
    x = _flat(logits)
    F_, nc, HW = x.shape
    lab = labels.reshape(F_, HW).to(torch.long)
    check_labels(lab, nc, ignore_index)
    keep = lab != ignore_index
    p = torch.softmax(x, dim=1)
    oh = torch.zeros_like(p)
    oh.scatter_(1, torch.where(keep, lab, torch.zeros_like(lab)).unsqueeze(1), 1.0)
    ww = (w.to(F64).reshape(F_, 1, HW) * keep.unsqueeze(1)) * g
    return (ww * (p - oh)).reshape(logits.shape)


def errors(got, ref):
    """(max |got - ref| / max |ref|, ||got - ref|| / ||ref||), float64 on ref's device."""
    gg = got.to(device=ref.device, dtype=F64)
    r = ref.to(F64)
    diff = gg - r
    return float(diff.abs().max()) / max(float(r.abs().max()), 1e-300), float(diff.norm() / r.norm().clamp_min(1e-300))
