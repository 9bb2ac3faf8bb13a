"""The kernels that turn logits into what the project reports (stswincl_amd/csrc/headops.hip: upsample_argmax_kernel,
upsample_argmax_cm_kernel, labels_score_kernel) against the float64 contract of tests/labels_ref.py, per PIXEL, through the raw entry
points.  No number here comes from a GPU run: the only thresholds are labels_ref's derived delta and its 2 % cap on undecided pixels, and
tests/test_labels_ref.py asserts both on the CPU - there an fp32 emulation of the kernels' association stays inside the bound at every
case and nine planted defects (swapped formulas or weights, a missing clamp, a wrong stride, frame or maximum, an unwritten pixel, a
narrowed ground truth) land outside.

For every case (stswin_upsample_argmax_cm with the case's align_corners; align_corners = 1 also through stswin_upsample_argmax):
  * every label lies in its allowed set, so every decided pixel is exact; in the exact regime every label is the first maximum of the
    float64 values, ties included.  A failure names the pixel, the workgroup and lane of both kernels, the label, the allowed set, the gap
    over delta and the number of offenders; one line per case is printed;
  * the two kernels agree bitwise for align_corners = 1;
  * nothing else is written: the labels live at byte offsets 0, 1 and 3 inside a buffer of a sentinel byte whose guards must stay, the
    logits and the ground truth are bit-identical afterwards, labels = NULL writes only the matrix, a second call gives the same bytes;
  * counts and matrix equal labels_ref.counts / confusion of the kernel's OWN labels exactly, with a ground truth that holds -1, nc - 1,
    nc, 63, 64, 255, 2^31, 2^32, 2^32 + 3, -2^32 + 2 and the int64 extremes in every workgroup, for ncm < nc, ncm = nc and ncm = 64, on
    pre-filled outputs; stswin_labels_score gives the same integers in its three forms;
  * refused calls launch nothing."""
import functools
import time

import pytest
import torch

import labels_ref as L
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = L.cases()
GUARD = 64                       # sentinel bytes on either side of a label map
INT_GUARD = -77777               # sentinel around the int32 counts and the int64 matrix


def _id(c):
    return c.name.replace(" ", "_")


def _st():
    return hip._stream()


def _dt(c):
    return 0 if c.dtype == L.BF else 1


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n[labels] wall time of this file: {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def _ref(c):
    """The case's logits on the device and its float64 verdict, computed once."""
    lg = L.make_logits(c).to(DEV)
    v = L.upsample(lg, c.H, c.W, c.align)
    allowed, decided, first, delta = L.verdict(v, L.bound(lg, c.H, c.W, c.align, c.exact))
    return lg, lg.clone(), v, allowed, decided, first, delta


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _label_buffer(c, off):
    n = c.F * c.H * c.W
    buf = torch.full((GUARD + off + n + GUARD,), L.SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 8 == 0
    return buf, buf[GUARD + off:GUARD + off + n]


def _guards_stand(buf, view, tag):
    lo = view.data_ptr() - buf.data_ptr()
    assert bool((buf[:lo] == L.SENTINEL).all()) and bool((buf[lo + view.numel():] == L.SENTINEL).all()), f"{tag}: bytes around the labels were written"


def _int_buffer(shape, dtype, prefill):
    """An output inside a guarded buffer, 16 bytes in -> (buffer, view, lead)."""
    n = prefill.numel()
    lead = 16 // prefill.element_size()
    buf = torch.full((lead + n + lead,), INT_GUARD, dtype=dtype, device=DEV)
    buf[lead:lead + n] = prefill.flatten()
    return buf, buf[lead:lead + n].view(shape), lead


def _int_guards_stand(buf, lead, tag):
    assert bool((buf[:lead] == INT_GUARD).all()) and bool((buf[-lead:] == INT_GUARD).all()), f"{tag}: written outside the output"


def _cm_call(c, lg, labels, gt=None, cm=None, ncm=0, **over):
    a = dict(frames=c.F, nc=c.nc, h=c.h, w=c.w, H=c.H, W=c.W, align=c.align)
    a.update(over)
    return hip.load().stswin_upsample_argmax_cm(_dt(c), hip._p(lg), hip._p(labels), hip._p(gt), hip._p(cm), ncm, a["align"], a["frames"], a["nc"],
                                                a["h"], a["w"], a["H"], a["W"], _st())


def _endo_call(c, lg, labels, gt=None, counts=None, **over):
    a = dict(frames=c.F, nc=c.nc, h=c.h, w=c.w, H=c.H, W=c.W)
    a.update(over)
    return hip.load().stswin_upsample_argmax(_dt(c), hip._p(lg), hip._p(labels), hip._p(gt), hip._p(counts), a["frames"], a["nc"], a["h"], a["w"],
                                             a["H"], a["W"], _st())


def _score_call(c, labels, gt, counts=None, cm=None, ncm=0, **over):
    a = dict(n=c.F, H=c.H, W=c.W, nc=c.nc)
    a.update(over)
    return hip.load().stswin_labels_score(hip._p(labels), hip._p(gt), hip._p(counts), hip._p(cm), ncm, a["n"], a["H"], a["W"], a["nc"], _st())


def _labels_of(c, call, tag):
    """The kernel's labels, written at byte offsets 0, 1 and 3 inside sentinel buffers (twice at offset 0): the same bytes every time."""
    maps = []
    for off in (0, 0, 1, 3):
        buf, view = _label_buffer(c, off)
        rc = call(view)
        assert rc == 0, f"{tag}: returned {rc}"
        _guards_stand(buf, view, f"{tag} at byte offset {off}")
        maps.append(view.clone().view(c.F, c.H, c.W))
    assert torch.equal(maps[0], maps[1]), f"{tag}: a second call gave other bytes"
    assert torch.equal(maps[0], maps[2]) and torch.equal(maps[0], maps[3]), f"{tag}: the labels depend on the buffer's alignment"
    return maps[0]


def _explain(c, tag, labels, v, allowed, first, delta, bad):
    f, y, x = bad.nonzero()[0].tolist()
    got = int(labels[f, y, x])
    col = v[f, :, y, x]
    d = float(delta[f, y, x])
    gap = float(col.max() - col[got]) if got < c.nc else float("inf")
    over = gap / d if d > 0 else float("inf")
    return (f"{tag}: {int(bad.sum())} of {bad.numel()} labels outside the contract, the first at {L.where(c, f, y, x)}: got {got}, allowed "
            f"{allowed[f, :, y, x].nonzero().flatten().tolist()}, first maximum {int(first[f, y, x])}, gap {gap:.3g} = {over:.3g} delta")


def _judge(c, tag, labels, ref):
    _, _, v, allowed, decided, first, delta = ref
    bad = L.offenders(labels, allowed, first, c.exact)
    n = decided.numel()
    undecided = ~decided
    print(f"[labels] {tag}: {int(undecided.sum())} of {n} pixels undecided ({int(undecided.sum()) / n:.2e}), "
          f"{int((undecided & (labels.long() != first)).sum())} of them differ from the float64 arg-max; {int(bad.sum())} outside the contract")
    assert not bool(bad.any()), _explain(c, tag, labels, v, allowed, first, delta, bad)
    assert torch.equal(labels.long()[decided], first[decided])


# ========================================================================================================================= labels
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_labels(c):
    ref = _ref(c)
    lg, lg0 = ref[:2]
    assert c.exact or int((~ref[4]).sum()) <= L.CAP * ref[4].numel()          # (the cap, as the CPU test holds it)
    cm_labels = _labels_of(c, lambda view: _cm_call(c, lg, view), f"upsample_argmax_cm {c.name}")
    _judge(c, f"upsample_argmax_cm {c.name}", cm_labels, ref)
    if c.align == 1:
        endo = _labels_of(c, lambda view: _endo_call(c, lg, view), f"upsample_argmax {c.name}")
        _judge(c, f"upsample_argmax {c.name}", endo, ref)
        assert torch.equal(endo, cm_labels), f"{c.name}: the two kernels disagree on {int((endo != cm_labels).sum())} pixels"
    assert torch.equal(_bits(lg), _bits(lg0)), f"{c.name}: the logits were written"


# ============================================================================================================== counts and matrix
def _prefill_counts(c):
    return (torch.arange(c.F * 3 * c.nc, dtype=torch.int32, device=DEV) % 1000 + 7).view(c.F, 3, c.nc)


def _prefill_cm(ncm):
    return ((1 << 33) + torch.arange(ncm * ncm, dtype=torch.int64, device=DEV)).view(ncm, ncm)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_counts_and_matrix_of_the_kernels_own_labels(c):
    lg, lg0 = _ref(c)[:2]
    labels = torch.full((c.F, c.H, c.W), L.SENTINEL, dtype=torch.uint8, device=DEV)
    assert _cm_call(c, lg, labels) == 0
    gt = L.ground_truth(c, labels)
    gt0 = gt.clone()
    assert gt.dtype == torch.int64 and all(bool((gt == e).any()) for e in L.edge_values(c.nc))
    pre = _prefill_counts(c)
    want_counts = pre.long() + L.counts(labels, gt, c.nc)
    fails = []

    def counts_check(tag, run):
        buf, view, lead = _int_buffer((c.F, 3, c.nc), torch.int32, pre)
        rc = run(view)
        assert rc == 0, f"{tag}: returned {rc}"
        _int_guards_stand(buf, lead, tag)
        diff = view.long() - want_counts
        if bool(diff.any()):
            f, k, cl = diff.nonzero()[0].tolist()
            fails.append(f"{tag}: {int((diff != 0).sum())} of {diff.numel()} counts differ from labels_ref.counts of the kernel's own labels, the "
                         f"first at frame {f}, {('|gt == c|', '|labels == c|', '|gt == c and labels == c|')[k]}, c = {cl}: got "
                         f"{int(view[f, k, cl]) - int(pre[f, k, cl])}, want {int(want_counts[f, k, cl]) - int(pre[f, k, cl])} (on top of the pre-filled "
                         f"{int(pre[f, k, cl])})")

    def cm_check(tag, ncm, run):
        pc = _prefill_cm(ncm)
        buf, view, lead = _int_buffer((ncm, ncm), torch.int64, pc)
        rc = run(view)
        assert rc == 0, f"{tag}: returned {rc}"
        _int_guards_stand(buf, lead, tag)
        diff = view - (pc + L.confusion(labels, gt, ncm))
        if bool(diff.any()):
            g, p = diff.nonzero()[0].tolist()
            fails.append(f"{tag}: {int((diff != 0).sum())} of {ncm * ncm} bins differ from labels_ref.confusion of the kernel's own labels, the first "
                         f"at gt {g} label {p}: {int(diff[g, p]):+d}")

    if c.align == 1:                                                         # the EndoVis kernel: labels and counts in one launch
        own = torch.full_like(labels, L.SENTINEL)
        counts_check(f"upsample_argmax {c.name}", lambda view: _endo_call(c, lg, own, gt, view))
        assert torch.equal(own, labels)
    counts_check(f"labels_score (counts) {c.name}", lambda view: _score_call(c, labels, gt, counts=view))
    for ncm in sorted({max(c.nc - 1, 1), c.nc, 64}):
        again = torch.full_like(labels, L.SENTINEL)
        cm_check(f"upsample_argmax_cm ncm={ncm} {c.name}", ncm, lambda view: _cm_call(c, lg, again, gt, view, ncm))
        assert torch.equal(again, labels), f"{c.name}: the labels change when a matrix is counted"
        cm_check(f"upsample_argmax_cm ncm={ncm} labels=NULL {c.name}", ncm, lambda view: _cm_call(c, lg, None, gt, view, ncm))
        cm_check(f"labels_score (cm) ncm={ncm} {c.name}", ncm, lambda view: _score_call(c, labels, gt, cm=view, ncm=ncm))
        both = _int_buffer((c.F, 3, c.nc), torch.int32, pre)
        cm_check(f"labels_score (both) ncm={ncm} {c.name}", ncm, lambda view: _score_call(c, labels, gt, counts=both[1], cm=view, ncm=ncm))
        _int_guards_stand(both[0], both[2], f"labels_score (both) {c.name}")
        if not torch.equal(both[1].long(), want_counts):
            fails.append(f"labels_score (both) ncm={ncm} {c.name}: the counts differ")
    assert not fails, "; ".join(fails[:4]) + (f" ({len(fails)} in all)" if len(fails) > 4 else "")
    assert torch.equal(gt, gt0), f"{c.name}: the ground truth was written"
    assert torch.equal(_bits(lg), _bits(lg0)), f"{c.name}: the logits were written"


# ======================================================================================================================= refusals
def _refusal_operands():
    c = L.Case(2, 9, 5, 7, 25, 41, 1, L.F32, "normal", 0)
    lg = L.make_logits(c).to(DEV)
    lbuf, labels = _label_buffer(c, 1)
    gt = torch.zeros(c.F, c.H, c.W, dtype=torch.int64, device=DEV)
    cbuf, counts, _ = _int_buffer((c.F, 3, c.nc), torch.int32, _prefill_counts(c))
    mbuf, cm, _ = _int_buffer((c.nc, c.nc), torch.int64, _prefill_cm(c.nc))
    return c, lg, labels, gt, counts, cm, (lbuf, cbuf, mbuf)


def _untouched(bufs, before):
    torch.cuda.synchronize()
    return all(torch.equal(a, b) for a, b in zip(bufs, before))


GEOMETRY = [{k: v} for k in ("frames", "h", "w", "H", "W") for v in (0, -1)]


def test_upsample_argmax_refuses_before_a_launch():
    c, lg, labels, gt, counts, cm, bufs = _refusal_operands()
    before = [b.clone() for b in bufs]
    for over in GEOMETRY + [{"nc": 0}, {"nc": 65}]:
        assert _endo_call(c, lg, labels, gt, counts, **over) == -1406, over
        assert _endo_call(c, lg, labels, **over) == -1406, over
    assert _endo_call(c, None, labels, gt, counts) == -1406
    assert _endo_call(c, lg, None, gt, counts) == -1406
    assert _endo_call(c, lg, labels, gt, None) == -1406                      # gt without counts
    assert _untouched(bufs, before), "a refused call wrote an output"
    assert _endo_call(c, lg, labels, gt, counts) == 0


def test_upsample_argmax_cm_refuses_before_a_launch():
    c, lg, labels, gt, counts, cm, bufs = _refusal_operands()
    before = [b.clone() for b in bufs]
    for over in GEOMETRY + [{"nc": 0}, {"nc": 65}]:
        assert _cm_call(c, lg, labels, gt, cm, c.nc, **over) == -1406, over
    assert _cm_call(c, None, labels, gt, cm, c.nc) == -1407
    assert _cm_call(c, lg, labels, gt, None, c.nc) == -1408                  # gt without a matrix
    assert _cm_call(c, lg, labels, None, cm, c.nc) == -1408                  # a matrix without gt
    assert _cm_call(c, lg, labels, gt, cm, 0) == -1408
    assert _cm_call(c, lg, labels, gt, cm, 65) == -1408
    assert _cm_call(c, lg, None) == -1409                                    # nothing to write
    assert _untouched(bufs, before), "a refused call wrote an output"
    assert _cm_call(c, lg, labels, gt, cm, c.nc) == 0


def test_labels_score_refuses_before_a_launch():
    c, lg, labels, gt, counts, cm, bufs = _refusal_operands()
    assert _cm_call(c, lg, labels) == 0
    torch.cuda.synchronize()
    before = [b.clone() for b in bufs]
    for over in ({"n": 0}, {"H": 0}, {"W": -1}, {"H": 16385}, {"W": 16385}):
        assert _score_call(c, labels, gt, counts, cm, c.nc, **over) == -1910, over
    assert _score_call(c, None, gt, counts, cm, c.nc) == -1911
    assert _score_call(c, labels, None, counts, cm, c.nc) == -1911
    assert _score_call(c, labels, gt, None, None, c.nc) == -1911
    assert _score_call(c, labels, gt, counts, cm, c.nc, nc=0) == -1912
    assert _score_call(c, labels, gt, counts, cm, c.nc, nc=65) == -1912
    assert _score_call(c, labels, gt, counts, cm, 0) == -1912
    assert _score_call(c, labels, gt, counts, cm, 65) == -1912
    lib = hip.load()
    tail = (c.F, c.H, c.W, c.nc, _st())
    assert lib.stswin_labels_score(hip._p(labels), gt.data_ptr() + 4, hip._p(counts), hip._p(cm), c.nc, *tail) == -1913
    assert lib.stswin_labels_score(hip._p(labels), hip._p(gt), counts.data_ptr() + 2, hip._p(cm), c.nc, *tail) == -1913
    assert lib.stswin_labels_score(hip._p(labels), hip._p(gt), hip._p(counts), cm.data_ptr() + 4, c.nc, *tail) == -1913
    assert _untouched(bufs, before), "a refused call wrote an output"
    assert _score_call(c, labels, gt, counts, None, 65) == 0                 # ncm is looked at only with a matrix
