"""tests/ohem_ref.py (the float64 reference of the OHEM cross-entropy kernels) checked on the CPU before any kernel is held against
it: per-pixel losses against F.cross_entropy, the value and gradient against float64 autograd of the reference's sort-then-slice form
(losses.py:35-39) on tie-free data, and the tie rule as the exact average over the orders of the tied pixels."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import ohem_ref as R

F64 = torch.float64
IGN = 255


def _case(F_, nc, H, W, seed, scale=2.0, ignore_frac=0.1):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(F_, nc, H, W, generator=g, dtype=F64) * scale
    labels = torch.randint(0, nc, (F_, H, W), generator=g)
    labels[torch.rand(F_, H, W, generator=g) < ignore_frac] = IGN
    return logits, labels


def _sorted_ohem(logits, labels, n_min, thresh):
    """losses.py:32-39 as written: per-pixel CE, sort descending, threshold or top-n_min slice, mean."""
    loss = F.cross_entropy(logits, labels, ignore_index=IGN, reduction="none").reshape(-1)
    srt = torch.sort(loss, descending=True)[0]
    return srt[srt > thresh].mean() if srt[n_min] > thresh else srt[:n_min].mean()


@pytest.mark.parametrize("F_,nc,H,W", [(2, 2, 5, 7), (1, 13, 9, 9), (3, 8, 4, 6)])
def test_pixel_loss_equals_cross_entropy(F_, nc, H, W):
    logits, labels = _case(F_, nc, H, W, nc)
    want = F.cross_entropy(logits, labels, ignore_index=IGN, reduction="none").reshape(-1)
    assert torch.allclose(R.pixel_loss(logits, labels, IGN), want, rtol=1e-14, atol=1e-15)


def test_pixel_loss_rejects_labels_outside_the_classes():
    logits, labels = _case(1, 4, 3, 3, 0)
    for bad in (4, -1, 100):
        lab = labels.clone()
        lab[0, 1, 2] = bad
        with pytest.raises(ValueError):
            R.pixel_loss(logits, lab, IGN)
        with pytest.raises(ValueError):
            R.gradient(logits, lab, torch.ones(9, dtype=F64), IGN)


@pytest.mark.parametrize("n_min,thresh", [(20, 0.3), (20, 5.0), (60, 1.0), (1, 0.7), (150, 100.0)])
def test_value_and_gradient_equal_sorted_autograd(n_min, thresh):
    """Both branches (which one is asserted below), tie-free data: value and dlogits against autograd of the sort-based form."""
    logits, labels = _case(2, 5, 8, 10, n_min)
    lg = logits.clone().requires_grad_(True)
    want = _sorted_ohem(lg, labels, n_min, thresh)
    want.backward()
    loss = R.pixel_loss(logits, labels, IGN)
    assert int(torch.unique(loss[loss > 0]).numel()) == int((loss > 0).sum())          # tie-free (besides the ignored zeros)
    assert float(R.value(loss, n_min, thresh)) == pytest.approx(float(want.detach()), rel=1e-13)
    sel = R.selection(loss, n_min, thresh)
    assert sel["topk"] == (int((loss > thresh).sum()) <= n_min)
    got = R.gradient(logits, labels, sel["w"], IGN)
    assert torch.allclose(got, lg.grad, rtol=1e-12, atol=1e-15)
    assert float(sel["w"].sum()) == pytest.approx(1.0, rel=1e-13)


def test_both_branches_are_covered_by_the_cases_above():
    logits, labels = _case(2, 5, 8, 10, 20)
    loss = R.pixel_loss(logits, labels, IGN)
    assert not R.selection(loss, 20, 0.3)["topk"] and R.selection(loss, 20, 5.0)["topk"]


@pytest.mark.parametrize("t,k_rem,n_above", [(3, 1, 2), (4, 2, 0), (5, 5, 1), (4, 3, 3)])
def test_tie_rule_is_the_average_over_tie_orders(t, k_rem, n_above):
    """Losses with t copies of the cut value, k_rem of them inside the top n_min: every order of the tied pixels gives the sort's
    gradient to a different subset; the exact average over all t! orders is k_rem / (t * n_min) per tied pixel."""
    n_min = n_above + k_rem
    above = 5.0 + torch.arange(n_above, dtype=F64)
    below = 0.5 * torch.arange(1, 6, dtype=F64) / 6
    loss = torch.cat([below[:2], torch.full((t,), 2.0, dtype=F64), above, below[2:]])
    tie_pos = torch.nonzero(loss == 2.0).reshape(-1)
    sel = R.selection(loss, n_min, thresh=1e9)
    assert sel["topk"] and sel["ties"] == t and sel["k_rem"] == k_rem and sel["cut"] == 2.0
    avg = torch.zeros_like(loss)
    orders = list(itertools.permutations(range(t)))
    for order in orders:
        # break the tie by the order: rank keys = loss, then the tied pixel's place in `order`
        key = loss.clone()
        key[tie_pos] = key[tie_pos] + 1e-9 * (t - torch.tensor(order, dtype=F64))
        top = torch.topk(key, n_min).indices
        w = torch.zeros_like(loss)
        w[top] = 1.0 / n_min
        avg += w
    avg /= len(orders)
    assert torch.allclose(sel["w"], avg, rtol=1e-14, atol=0)
    assert float(sel["w"].sum()) == pytest.approx(1.0, rel=1e-14)
    assert float(R.value(loss, n_min, 1e9)) == pytest.approx(float(torch.sort(loss, descending=True)[0][:n_min].mean()), rel=1e-14)


def test_gradient_scales_with_the_incoming_gradient():
    logits, labels = _case(1, 3, 4, 4, 3, ignore_frac=0.3)
    loss = R.pixel_loss(logits, labels, IGN)
    w = R.selection(loss, 5, 0.1)["w"]
    g1 = R.gradient(logits, labels, w, IGN)
    assert torch.allclose(R.gradient(logits, labels, w, IGN, g=2.5), 2.5 * g1, rtol=1e-15, atol=0)
    ign = (labels == IGN).reshape(1, 1, 4, 4).expand_as(g1)
    assert bool((g1[ign] == 0).all())
