"""The OHEM cross-entropy kernels (stswincl_amd/csrc/headops.hip: ce_fwd, ohem_select, ce_bwd; include/stswin_hip.h, a15 section)
against the float64 reference of tests/ohem_ref.py, called through the hip.* entry points, fp32 and bf16 logits.

Every case prints its measured error.  Metrics:
  loss  per-pixel loss, max over pixels of |got - ref| / (ref + 2^-20): relative for the losses that matter, absolute below ~1e-6;
  sum   the 64-bit fixed-point sum of ce_fwd against the float64 sum of the kernel's OWN losses above thresh (relative);
  value ohem_select's value against the float64 OHEM value of the kernel's own losses (relative);
  grad  ce_bwd against the float64 gradient with the selection taken from the kernel's losses (max / l2 as in tests/attn_ref.py).
The count stats[0], the cut sel[0], the branch and the weights sel[1] / sel[3] are checked exactly (up to the one rounding of a
float32 quotient).

Regimes (logits): "near0" 0.1 randn (losses ~ log nc); "peaked" 6 randn; "offset20" / "offset80" +-20 / +-80 plus randn, the label's
class raised by 6 in 90 % of the pixels (a small loss on a large arg-max logit: the cancellation case of the old `mx + log(s) - x[lab]`
form, which measured ~ulp(|mx|) / 2 absolute there).

Bounds: at most 2x the error measured on MI355X (table BOUND; bf16 logits are exact in fp32, so both dtypes share the loss bounds).
"""
import time

import pytest
import torch

import ohem_ref as R
from stswincl_amd import hip
from stswincl_amd import headops as H

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FLOOR = 2.0 ** -20

# 1.8 x the largest error measured on MI355X over the cases of each key, rounded up to two digits (<= 2x).  Measured: per-pixel loss
# 1.6e-7 (near0), 2.9e-7 (offset20), 3.5e-7 (offset80), 5.6e-7 (peaked) - the old `mx + log(s) - x[lab]` measured 1.4e-2 / 3.4e-2 /
# 0.40 there; fixed-point sum 7.1e-8; value 1.0e-7; dlogits f32 3.4e-7 max, 7.9e-8 l2; bf16 2.7e-3 / 1.6e-3 (bf16 output rounding);
# total selected weight f32 6.3e-8, bf16 1.7e-3.
BOUND = {
    ("loss", "near0"): 2.8e-7, ("loss", "offset20"): 5.3e-7, ("loss", "offset80"): 6.4e-7, ("loss", "peaked"): 1.1e-6,
    "sum": 1.3e-7,
    "value": 1.9e-7,
    ("grad", "f32"): (6.2e-7, 1.5e-7),
    ("grad", "bf16"): (5.0e-3, 3.0e-3),
    ("weight", "f32"): 1.2e-7,
    ("weight", "bf16"): 3.2e-3,
}
MEASURED = {}


def _note(key, *vals):
    MEASURED.setdefault(key, [0.0] * len(vals))
    MEASURED[key] = [max(a, b) for a, b in zip(MEASURED[key], vals)]
    print(f"[ohem] {key}: " + " ".join(f"{v:.2e}" for v in vals))


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[ohem contract] wall time {time.perf_counter() - t0:.1f} s; measured maxima:")
    for k, v in sorted(MEASURED.items(), key=str):
        print(f"[ohem]   {k}: " + " ".join(f"{x:.2e}" for x in v))


def _logits(F_, nc, HW, regime, dt, seed, ignore_index=-1, ignore_frac=0.1):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, nc, (F_, HW), generator=g)
    x = torch.randn(F_, nc, HW, generator=g)
    if regime == "near0":
        x = x * 0.1
    elif regime == "peaked":
        x = x * 6
    else:
        off = float(regime[len("offset"):])
        sign = torch.where(torch.rand(F_, 1, HW, generator=g) < 0.5, -1.0, 1.0)
        x = x + sign * off
        boost = (torch.rand(F_, HW, generator=g) < 0.9).float() * 6
        x.scatter_add_(1, lab.unsqueeze(1), boost.unsqueeze(1))
    lab[torch.rand(F_, HW, generator=g) < ignore_frac] = ignore_index
    return x.to(dt).cuda(), lab.cuda()


def _loss_err(got, ref):
    return float(((got.double() - ref).abs() / (ref.abs() + FLOOR)).max())


def _fix_sum(stats):
    return float(stats[2:4].view(torch.int64)[0]) / 4294967296.0


# ---------------------------------------------------------------------------------------------------------------- ce_fwd
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("nc,F_,HW", [(2, 1, 1000), (13, 3, 4097), (12, 4, 64 * 80 + 3), (25, 2, 777), (17, 1, 300)])
@pytest.mark.parametrize("regime", ["near0", "peaked", "offset20", "offset80"])
def test_ce_fwd_per_pixel_loss_and_stats(dt, nc, F_, HW, regime):
    x, lab = _logits(F_, nc, HW, regime, dt, nc * 31 + F_ + len(regime))
    thresh = 0.357
    loss, stats = hip.ce_fwd(x, lab, -1, thresh)
    ref = R.pixel_loss(x, lab, -1)
    e = _loss_err(loss, ref)
    _note(("loss", regime), e)
    assert e <= BOUND[("loss", regime)], (regime, e)
    assert bool((loss[lab.reshape(-1) == -1] == 0).all())
    # stats[0] exactly the count of the kernel's own losses above thresh; stats[1] no bad label
    hard = loss > thresh
    assert float(stats[0]) == float(hard.sum()) and float(stats[1]) == 0.0
    want = float(loss[hard].double().sum())
    es = abs(_fix_sum(stats) - want) / max(want, 1e-30)
    _note("sum", es)
    assert es <= BOUND["sum"]


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_ce_fwd_all_pixels_ignored(dt):
    x, lab = _logits(2, 12, 515, "peaked", dt, 1)
    lab.fill_(255)
    loss, stats = hip.ce_fwd(x, lab, 255, 0.357)
    assert bool((loss == 0).all()) and float(stats[0]) == 0.0 and _fix_sum(stats) == 0.0 and float(stats[1]) == 0.0


def test_out_of_range_labels_are_never_read_and_make_the_value_nan():
    """A label >= nc or < 0 that is not ignore_index: loss NaN at that pixel (no read at that label), stats[1] counts it, the OHEM
    value is NaN in both branches, and ce_bwd gives that pixel no gradient (the others are untouched)."""
    nc, F_, HW = 12, 2, 1000
    x, lab = _logits(F_, nc, HW, "near0", F32, 7)
    bad = lab.clone()
    bad[0, 5], bad[1, 17], bad[1, 400] = nc, -3, 1 << 40
    loss, stats = hip.ce_fwd(x, bad, -1, 0.357)
    badpx = torch.zeros(F_ * HW, dtype=torch.bool, device="cuda")
    badpx[[5, HW + 17, HW + 400]] = True
    assert bool(torch.isnan(loss[badpx]).all()) and bool(torch.isfinite(loss[~badpx]).all())
    assert float(stats[1]) == 3.0
    good_loss, _ = hip.ce_fwd(x, lab, -1, 0.357)
    assert torch.equal(loss[~badpx], good_loss[~badpx])
    for n_min in (10, F_ * HW - 50):                      # threshold branch, top-n_min branch
        value, sel = hip.ohem_select(loss, stats, n_min, 0.357)
        assert bool(torch.isnan(value)), n_min
        d = hip.ce_bwd(x, bad, loss, sel, torch.ones(1, device="cuda"), -1)
        dpx = d.reshape(F_, nc, HW).permute(0, 2, 1).reshape(-1, nc)
        assert bool((dpx[badpx] == 0).all()) and bool(torch.isfinite(d).all())
    with pytest.raises(ValueError):
        R.pixel_loss(x, bad, -1)


# ---------------------------------------------------------------------------------------------------------------- ohem_select
def _select_check(loss, stats, n_min, thresh):
    value, sel = hip.ohem_select(loss, stats, n_min, thresh)
    ref = R.selection(loss, n_min, thresh)
    want = float(R.value(loss, n_min, thresh))
    ev = abs(float(value) - want) / max(abs(want), 1e-30)
    _note("value", ev)
    assert ev <= BOUND["value"], (float(value), want)
    s = sel.tolist()
    assert (s[2] == 1.0) == ref["topk"]
    assert s[0] == ref["cut"] if ref["topk"] else s[0] == pytest.approx(thresh)
    if ref["topk"]:
        assert s[1] == torch.tensor(1.0 / n_min, dtype=F32).item()
        assert s[3] == pytest.approx(ref["k_rem"] / (ref["ties"] * n_min), rel=1e-7)
    else:
        assert s[1] == pytest.approx(1.0 / ref["n_hard"], rel=1e-7) and s[3] == 0.0
    return value, sel, ref


def _tied_logits(F_, nc, HW, dt, seed, n_tie):
    """peaked logits where n_tie pixels share one logit vector and label (bit-identical losses), a loss above the median"""
    x, lab = _logits(F_, nc, HW, "peaked", dt, seed, ignore_frac=0.05)
    xf, lf = x.permute(0, 2, 1).reshape(-1, nc), lab.reshape(-1)
    loss = R.pixel_loss(x, lab, -1)
    src = int(torch.argsort(loss)[int(0.8 * loss.numel())])            # a pixel at the 80th percentile
    g = torch.Generator().manual_seed(seed)
    dst = torch.randperm(F_ * HW, generator=g)[:n_tie].cuda()
    xf[dst] = xf[src].clone()
    lf[dst] = lf[src].clone()
    return xf.view(F_, HW, nc).permute(0, 2, 1).contiguous(), lf.view(F_, HW).contiguous(), src


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_ohem_select_on_real_losses_both_branches_and_the_boundary(dt):
    S, F_ = 256, 2                                       # n_min = S*S//16 as in bench.py (per frame pair)
    x, lab = _logits(F_, 12, S * S, "near0", dt, 3)
    x = x * 30                                           # spread the losses (near0 x 30 ~ 3 randn)
    n_min = S * S // 16
    for thresh in (0.357, 1e3):                          # threshold branch, top-n_min branch
        loss, stats = hip.ce_fwd(x, lab, -1, thresh)
        _, sel, ref = _select_check(loss, stats, n_min, thresh)
        assert ref["topk"] == (thresh == 1e3)
    loss, _ = hip.ce_fwd(x, lab, -1, 0.357)
    srt = torch.sort(loss.double(), descending=True)[0]
    for n_hard in (n_min, n_min + 1):                    # branch boundary: n_hard == n_min -> top-n_min, n_min + 1 -> threshold
        thresh = float(torch.tensor((float(srt[n_hard - 1]) + float(srt[n_hard])) / 2, dtype=F32))
        loss, stats = hip.ce_fwd(x, lab, -1, thresh)
        assert int(stats[0]) == n_hard
        _, sel, ref = _select_check(loss, stats, n_min, thresh)
        assert ref["topk"] == (n_hard == n_min)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("k_rem", [1, 37, 99])
def test_ohem_select_and_ce_bwd_with_ties_exactly_at_the_cut(dt, k_rem):
    """n_tie = 100 bit-identical losses; n_min chosen so the cut lands on them with k_rem of them inside the top n_min: the value
    counts k_rem copies, the gradient gives each tied pixel k_rem / (t n_min) (total selected weight 1)."""
    F_, nc, HW, n_tie = 2, 12, 4000, 100
    x, lab, src = _tied_logits(F_, nc, HW, dt, 11 + k_rem, n_tie)
    loss, _ = hip.ce_fwd(x, lab, -1, 1e6)
    tie_val = loss[src]
    t = int((loss == tie_val).sum())
    assert t >= n_tie
    n_min = int((loss > tie_val).sum()) + k_rem
    loss, stats = hip.ce_fwd(x, lab, -1, 1e6)            # threshold above everything: top-n_min branch
    value, sel, ref = _select_check(loss, stats, n_min, 1e6)
    assert ref["ties"] == t and ref["k_rem"] == k_rem and float(sel[0]) == float(tie_val)
    _bwd_check(x, lab, loss, sel, ref, "f32" if dt == F32 else "bf16", gscale=0.75)


# ---------------------------------------------------------------------------------------------------------------- ce_bwd
def _bwd_check(x, lab, loss, sel, ref, fam, gscale):
    d = hip.ce_bwd(x, lab, loss, sel, torch.full((1,), gscale, device="cuda"), -1)
    want = R.gradient(x, lab, ref["w"], -1, g=gscale)
    emax, el2 = R.errors(d, want)
    _note(("grad", fam), emax, el2)
    bm, bl = BOUND[("grad", fam)]
    assert emax <= bm and el2 <= bl, (emax, el2)
    # total selected weight from the label channel: d[lab] = g w (p_lab - 1); pixels with p_lab < 0.9 (a stable division)
    F_, nc = x.shape[:2]
    xf = x.double().reshape(F_, nc, -1)
    lf = lab.reshape(F_, -1)
    keep = lf != -1
    p = torch.softmax(xf, 1).gather(1, torch.where(keep, lf, 0).unsqueeze(1)).squeeze(1)
    dl = d.double().reshape(F_, nc, -1).gather(1, torch.where(keep, lf, 0).unsqueeze(1)).squeeze(1)
    use = keep & (p < 0.9)
    w_got = float((dl[use] / (gscale * (p[use] - 1))).sum())
    w_ref = float(ref["w"].reshape(F_, -1)[use].sum())
    ew = abs(w_got - w_ref) / w_ref
    _note(("weight", fam), ew)
    assert ew <= BOUND[("weight", fam)], (w_got, w_ref)
    return d


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("regime,nc,thresh", [("near0", 13, 0.357), ("peaked", 12, 0.357), ("peaked", 12, 50.0),
                                              ("offset80", 8, 0.357), ("offset20", 25, 1e6)])
def test_ce_bwd_against_float64_gradient(dt, regime, nc, thresh):
    F_, HW = 3, 2500
    x, lab = _logits(F_, nc, HW, regime, dt, nc + len(regime))
    n_min = F_ * HW // 16
    loss, stats = hip.ce_fwd(x, lab, -1, thresh)
    _, sel, ref = _select_check(loss, stats, n_min, thresh)
    _bwd_check(x, lab, loss, sel, ref, "f32" if dt == F32 else "bf16", gscale=1.3)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("thresh", [0.357, 1e6])
def test_ohem_ce_fn_end_to_end(dt, thresh):
    """OhemCEFn through autograd (value and dlogits for an upstream gradient of 2) against the reference on the kernel's losses."""
    F_, nc, S = 2, 12, 96
    x, lab = _logits(F_, nc, S * S, "peaked", dt, 5)
    x = x.view(F_, nc, S, S).clone().requires_grad_(True)
    lab = lab.view(F_, S, S)
    n_min = S * S // 16
    v = H.OhemCEFn.apply(x, lab, n_min, thresh, -1)
    (2.0 * v).backward()
    loss, _ = hip.ce_fwd(x.detach(), lab, -1, thresh)
    want = float(R.value(loss, n_min, thresh))
    v = float(v.detach())
    _note("value", abs(v - want) / want)
    assert abs(v - want) <= BOUND["value"] * want
    assert v == pytest.approx(float(R.value(R.pixel_loss(x.detach(), lab, -1), n_min, thresh)), rel=1e-5)
    ref = R.gradient(x.detach(), lab, R.selection(loss, n_min, thresh)["w"], -1, g=2.0)
    emax, el2 = R.errors(x.grad, ref)
    _note(("grad", "f32" if dt == F32 else "bf16"), emax, el2)
    bm, bl = BOUND[("grad", "f32" if dt == F32 else "bf16")]
    assert emax <= bm and el2 <= bl, (emax, el2)
