"""tests/labels_ref.py on the CPU: the float64 reference against float64 F.interpolate, an fp32 emulation of the kernels' association
against the derived bound, the properties that make each case worth running (the 2 % cap on undecided pixels, every class winning,
exact ties in the exact regime), and nine planted defects, each of which must put a DECIDED pixel outside its allowed set (the
narrowed ground truth: change a count) in every case it can affect.  tests/test_hip_labels_contract.py asks the same of the kernels."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import labels_ref as L

F64, F32 = torch.float64, torch.float32
CASES = L.cases()


def _id(c):
    return c.name.replace(" ", "_")


@functools.lru_cache(maxsize=None)
def _ref(c):
    lg = L.make_logits(c)
    v = L.upsample(lg, c.H, c.W, c.align)
    b = L.bound(lg, c.H, c.W, c.align, c.exact)
    return (lg, v, b) + L.verdict(v, b)


def emulate(logits, H, W, align, defect=None):
    """The kernels' fp32 expressions in their association (upsample_argmax_cm_kernel; align = 1 is upsample_argmax_kernel's), one IEEE
    operation per torch operation, -> (uint8 labels [F][H][W], fp32 values [F][nc][H][W]).  `defect` plants one mistake."""
    F_, nc, h, w = logits.shape
    flat = torch.cat([logits.to(F32).reshape(-1), torch.zeros(w + 2)])        # (a defect may read past the last plane)
    f32 = lambda n: torch.tensor(float(n), dtype=F32)                         # noqa: E731
    al = align ^ 1 if defect == "align formulas swapped" else align

    def coord(n_in, n_out):
        d = torch.arange(n_out, dtype=F32)
        if al:
            f = d * (f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0))
        else:
            f = ((f32(n_in) / f32(n_out)) * (d + 0.5) - 0.5).clamp_min(0.0)
        i0 = ((f + 0.5) if defect == "rounded to nearest" else f).floor().long().clamp_max(n_in - 1)
        return i0, f - i0.to(F32)

    y0, wy = coord(h, H)
    x0, wx = coord(w, W)
    y1 = (y0 + 1).clamp_max(h - 1)
    x1 = x0 + 1 if defect == "x1 not clamped" else (x0 + 1).clamp_max(w - 1)
    WY, WX = wy.view(H, 1).expand(H, W), wx.view(1, W).expand(H, W)
    if defect == "wx and wy swapped":
        WY, WX = WX, WY
    stride = h * w - 1 if defect == "class stride h w - 1" else h * w
    frame = torch.zeros(F_, dtype=torch.long) if defect == "frame 0 for every frame" else torch.arange(F_)
    base = (frame * nc * h * w).view(F_, 1, 1, 1) + (torch.arange(nc) * stride).view(1, nc, 1, 1)
    at = lambda yy, xx: flat[base + (yy.view(H, 1) * w + xx.view(1, W))]      # noqa: E731
    v = (1.0 - WY) * ((1.0 - WX) * at(y0, x0) + WX * at(y0, x1)) + WY * ((1.0 - WX) * at(y1, x0) + WX * at(y1, x1))
    idx = torch.arange(nc).view(1, nc, 1, 1)
    hit = v == v.amax(1, keepdim=True)
    if defect == "last maximum":
        lab = torch.where(hit, idx, torch.full_like(idx, -1)).amax(1)
    else:
        lab = torch.where(hit, idx, torch.full_like(idx, nc)).amin(1)
    lab = lab.to(torch.uint8)
    if defect == "last pixel not written":
        lab[:, -1, -1] = L.SENTINEL
    return lab, v


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_upsample_is_float64_interpolate(c):
    lg, v = _ref(c)[:2]
    want = TF.interpolate(lg.to(F64), (c.H, c.W), mode="bilinear", align_corners=bool(c.align))
    scale = float(lg.to(F64).abs().max())
    assert v.shape == (c.F, c.nc, c.H, c.W) and v.dtype == F64
    assert float((v - want).abs().max()) <= 1e-13 * max(scale, 1e-30) * max(c.h, c.w)
    if (c.h, c.w) == (c.H, c.W):
        assert torch.equal(v, lg.to(F64))


def test_the_cases_cover_what_the_issue_names():
    shapes = {(c.F, c.h, c.w, c.H, c.W) for c in CASES if not c.exact}
    assert shapes == {(3, 1, 1, 4, 6), (2, 23, 37, 101, 77), (2, 8, 10, 67, 131), (1, 16, 20, 13, 9), (1, 3, 5, 40, 24), (1, 5, 7, 25, 41),
                      (1, 64, 80, 135, 240)}
    for s in shapes:
        assert {(c.align, c.dtype) for c in CASES if (c.F, c.h, c.w, c.H, c.W) == s} == {(a, t) for a in (0, 1) for t in (F32, L.BF)}
    assert {c.nc for c in CASES} == {1, 2, 9, 12, 64}
    for regime in ("normal", "large", "smooth", "exact"):
        got = {(c.align, c.dtype) for c in CASES if c.regime == regime}
        assert got == {(a, t) for a in (0, 1) for t in (F32, L.BF)}, regime
    assert {(c.h, c.w, c.H, c.W, c.align) for c in CASES if c.exact} == {(5, 7, 5, 7, 0), (5, 7, 5, 7, 1), (5, 7, 10, 14, 0), (6, 6, 24, 24, 0),
                                                                         (5, 9, 9, 17, 1)}
    assert 25 * 41 == 1025 and 101 * 77 == 7777 and sum(c.H * c.W > 30000 for c in CASES) == 4
    for c in CASES:
        assert bool(torch.isfinite(L.make_logits(c).float()).all())


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_fp32_emulation_stays_inside_the_bound(c):
    lg, v, b = _ref(c)[:3]
    _, v32 = emulate(lg, c.H, c.W, c.align)
    err = (v32.to(F64) - v).abs()
    if c.exact:
        assert float(b.max()) == 0.0 and float(err.max()) == 0.0            # every coordinate, weight, product and sum is exact
        return
    assert bool((b > 0).all())
    ratio = float((err / b).max())
    print(f"[labels] {c.name}: fp32 emulation err / bound = {ratio:.3f}")
    assert ratio <= 1.0
    if c.regime == "large":                                                  # the bound scales with the values
        assert float(b.max()) > 1e-3


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_case_properties(c):
    lg, v, b, allowed, decided, first, delta = _ref(c)
    n = decided.numel()
    undecided = n - int(decided.sum())
    print(f"[labels] {c.name}: {undecided} of {n} pixels undecided ({undecided / n:.2e})")
    assert bool(allowed.gather(1, first.unsqueeze(1)).all())
    if c.exact:
        assert 0.04 <= undecided / n <= 0.90                                 # exact ties: first maximum wins is exercised
        assert bool((delta == 0).all())
        winners = first
    else:
        assert undecided <= L.CAP * n                                       # a condition on the reference alone
        winners = first[decided]
    if c.nc <= 12:                                                           # a wrong class stride shows
        assert sorted(winners.unique().tolist()) == list(range(c.nc))
    if c.nc == 1:
        assert bool(decided.all()) and not bool(first.any())
    # the emulation itself is a kernel the contract accepts
    lab, _ = emulate(lg, c.H, c.W, c.align)
    assert not bool(L.offenders(lab, allowed, first, c.exact).any())


# ------------------------------------------------------------------------------------------------------------------ planted defects
def _one_source_pixel(c):
    return c.h * c.w == 1


def _identity(c):
    return (c.h, c.w) == (c.H, c.W)


# which cases a defect can affect at all (nc = 1 has one label; the reasons for the rest stand beside each entry)
DEFECTS = {
    # one source pixel: every coordinate reads it; identity: both formulas give src = dst
    "align formulas swapped": lambda c: c.nc > 1 and not _one_source_pixel(c) and not _identity(c),
    # one source pixel: the four taps are one value; identity: both weights are 0
    "wx and wy swapped": lambda c: c.nc > 1 and not _one_source_pixel(c) and not _identity(c),
    # x0 = w - 1 with wx > 0 happens only at the right edge of an align = 0 up-sampling (align = 1 ends at src = w - 1 with wx = 0,
    # align = 0 down-sampling ends below w - 1).  With one source pixel the next element is the next class, and with two classes and three
    # frames that may change no winner: left out
    "x1 not clamped": lambda c: c.nc > 1 and c.align == 0 and c.W > c.w and not _one_source_pixel(c),
    "rounded to nearest": lambda c: c.nc > 1 and not _one_source_pixel(c) and not _identity(c),
    "last maximum": lambda c: c.nc > 1 and c.exact,
    "class stride h w - 1": lambda c: c.nc > 1,
    "frame 0 for every frame": lambda c: c.nc > 1 and c.F > 1,
    "last pixel not written": lambda c: True,
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_caught(defect):
    hit = 0
    for c in CASES:
        if not DEFECTS[defect](c):
            continue
        lg, v, b, allowed, decided, first, delta = _ref(c)
        lab, _ = emulate(lg, c.H, c.W, c.align, defect)
        bad = L.offenders(lab, allowed, first, c.exact)
        if not c.exact:                                                      # (the exact regime judges every pixel, ties included)
            bad = bad & decided
        assert bool(bad.any()), f"{defect} goes unnoticed at {c.name}"
        hit += 1
    assert hit >= 10 or defect == "last maximum" and hit == sum(c.exact and c.nc > 1 for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_narrowed_ground_truth_changes_a_count(c):
    """Planted defect 9: reading the int64 ground truth as 32 bits counts 2^32 as class 0, 2^32 + 3 as class 3, -2^32 + 2 as class 2."""
    first = _ref(c)[5]
    labels = first.to(torch.uint8)
    gt = L.ground_truth(c, labels)
    for v in L.edge_values(c.nc):
        per_frame = (gt == v).flatten(1).sum(1)
        assert int(per_frame.min()) >= max(1, min(c.H * c.W // 256, 1))
    last = gt.flatten(1)[:, (c.H * c.W - 1) // 256 * 256:]
    assert bool(torch.isin(last, torch.tensor(L.edge_values(c.nc))).any(1).all())      # the last partial block holds one too
    narrowed = gt.to(torch.int32).to(torch.int64)
    assert not torch.equal(L.counts(labels, narrowed, c.nc), L.counts(labels, gt, c.nc))
    for ncm in {max(c.nc - 1, 1), c.nc, 64}:
        assert not torch.equal(L.confusion(labels, narrowed, ncm), L.confusion(labels, gt, ncm))
        want = L.confusion(labels, gt, ncm)
        keep = (gt >= 0) & (gt < ncm) & (labels.long() < ncm)
        assert int(want.sum()) == int(keep.sum())
    cnt = L.counts(labels, gt, c.nc)
    assert cnt.shape == (c.F, 3, c.nc) and int(cnt[:, 1].sum()) == labels.numel() and bool((cnt[:, 2] <= cnt[:, 0]).all())
    assert int(cnt[:, 2].sum()) > 0
