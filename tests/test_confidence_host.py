"""Confidence of the labels on the host: the numpy definitions (utils/confidence.py) against torch in float64 and a plain loop, the
reports made of the sums, MaskReport's score, and the plumbing of the report chain.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stswincl_amd import hip
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import confidence as C
from stswincl_amd.utils import rle as R
from stswincl_amd.video_report import ReportChain, Yield

# (h, w, H, W, align_corners)
GEOMETRIES = [(1, 1, 8, 8, True), (4, 5, 30, 37, True), (5, 6, 40, 48, True), (13, 9, 5, 7, True), (6, 10, 6, 10, True),
              (16, 20, 34, 60, False)]


def _logits(rng, F_, nc, h, w):
    return np.clip(rng.standard_normal((F_, nc, h, w)) * 3.0, -16.0, 16.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the definition against torch
@pytest.mark.parametrize("h,w,H,W,align", GEOMETRIES)
def test_the_definition_agrees_with_float64_torch(h, w, H, W, align):
    """|255 p_ref - 255 p_torch| <= 0.26.  The reference takes the source coordinates in float32 as the kernels do; a coordinate off
    by n_out 2^-23 moves a weight by that much, a value by at most 4 * 16 times it (|logit| <= 16), and p by at most half of that
    (|dp/dv| <= 1/4, two values move): about 1e-3 at n_out <= 64, 0.26 in units of a byte.  A cap from the arithmetic."""
    rng = np.random.default_rng(h * 1000 + W)
    nc = 7
    lg = _logits(rng, 2, nc, h, w)
    lab = rng.integers(0, nc, (2, H, W)).astype(np.uint8)
    p = C.upsample_probability(lg, lab, align)
    up = F.interpolate(torch.from_numpy(lg).double(), size=(H, W), mode="bilinear", align_corners=align)
    want = up.softmax(1).gather(1, torch.from_numpy(lab.astype(np.int64))[:, None])[:, 0].numpy()
    err = np.abs(255.0 * p - 255.0 * want).max()
    print(f"{(h, w)} -> {(H, W)} align={align}: max |255 p_ref - 255 p_torch| = {err:.3g}")
    assert err <= 0.26
    q = C.upsample_confidence(lg, lab, align)
    assert q.dtype == np.uint8 and np.array_equal(q, np.minimum(255, np.floor(255.0 * p + 0.5)).astype(np.uint8))


def test_labels_of_the_argmax_get_the_largest_probability():
    rng = np.random.default_rng(5)
    lg = _logits(rng, 1, 12, 5, 6)
    up = F.interpolate(torch.from_numpy(lg).double(), size=(40, 48), mode="bilinear", align_corners=True)
    lab = up.argmax(1).numpy().astype(np.uint8)
    p = C.upsample_probability(lg, lab, True)
    assert np.abs(p - up.softmax(1).max(1).values.numpy()).max() <= 1e-3 and p.min() >= 1.0 / 12 - 1e-3


# ------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("nc,want", [(1, 255), (3, 85), (5, 51), (15, 17)])
def test_constant_logits_give_one_over_nc(nc, want):
    for value in (0.0, -3.25, 7.5):
        lg = np.full((2, nc, 4, 5), value, dtype=np.float32)
        lab = np.random.default_rng(nc).integers(0, nc, (2, 30, 37)).astype(np.uint8)
        for align in (True, False):
            assert (C.upsample_confidence(lg, lab, align) == want).all()


def test_a_class_far_above_the_rest_saturates_and_large_logits_give_no_nan():
    lg = np.zeros((1, 6, 4, 5), dtype=np.float32)
    lg[:, 2] = 80.0
    lab = np.full((1, 30, 37), 2, dtype=np.uint8)
    assert (C.upsample_confidence(lg, lab) == 255).all()
    assert (C.upsample_confidence(lg, np.zeros_like(lab)) == 0).all()       # exp(-80) of a byte
    for value in (1e4, -1e4):
        p = C.upsample_probability(np.full((1, 4, 4, 5), value, dtype=np.float32), np.zeros((1, 9, 11), dtype=np.uint8))
        assert not np.isnan(p).any() and np.allclose(p, 0.25)


def test_a_label_that_is_no_class_gives_zero():
    lg = _logits(np.random.default_rng(1), 1, 3, 4, 5)
    lab = np.random.default_rng(2).integers(0, 6, (1, 30, 37)).astype(np.uint8)
    lab[0, 0, :4] = (3, 255, 2, 64)
    q = C.upsample_confidence(lg, lab)
    known = C.upsample_confidence(lg, np.where(lab < 3, lab, 0).astype(np.uint8))
    assert (lab >= 3).sum() > 100 and (q[lab >= 3] == 0).all() and np.array_equal(q[lab < 3], known[lab < 3]) and q.max() > 128


def test_the_definition_refuses_other_forms():
    lg, lab = np.zeros((1, 3, 4, 5), dtype=np.float32), np.zeros((1, 8, 8), dtype=np.uint8)
    for a, b in ((lg[0], lab), (lg, lab[0]), (lg, lab.astype(np.int32)), (lg, np.zeros((2, 8, 8), dtype=np.uint8))):
        with pytest.raises(ValueError):
            C.upsample_confidence(a, b)


# ---------------------------------------------------------------------------------------------------------- confidence_sums
def _loop_sums(maps, conf, K, low):
    out = np.zeros((maps.shape[0], K, 3), dtype=np.int64)
    for f in range(maps.shape[0]):
        for v, q in zip(maps[f].reshape(-1).tolist(), conf[f].reshape(-1).tolist()):
            if 0 <= v < K:
                out[f, v, 0] += 1
                out[f, v, 1] += q
                out[f, v, 2] += q < low
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
@pytest.mark.parametrize("low", [0, 128, 256])
def test_confidence_sums_against_a_plain_loop(dtype, low):
    rng = np.random.default_rng(low + 1)
    K = 5
    maps = rng.integers(0, K + 3, (3, 9, 13)).astype(dtype)                  # values >= K present
    if dtype == np.int32:
        maps[rng.random(maps.shape) < 0.3] = -1
    conf = rng.integers(0, 256, maps.shape).astype(np.uint8)
    conf[0, 0, :3] = (127, 128, 255)
    got = C.confidence_sums(maps, conf, K, low)
    assert got.dtype == np.int64 and np.array_equal(got, _loop_sums(maps, conf, K, low))
    assert (got[:, :, 2] == (0 if low == 0 else got[:, :, 0])).all() or low == 128
    for bad in (dict(K=0), dict(K=1025), dict(K=True), dict(low=-1), dict(low=257), dict(low=1.0)):
        with pytest.raises(ValueError):
            C.confidence_sums(maps, conf, **{"K": K, **bad})
    with pytest.raises(ValueError):
        C.confidence_sums(maps.astype(np.int64), conf, K)
    with pytest.raises(ValueError):
        C.confidence_sums(maps, conf[:, :4], K)


# ------------------------------------------------------------------------------------------------------------------ reports
def test_confidence_report_arithmetic_and_ordering():
    cs = np.zeros((3, 4, 3), dtype=np.int64)
    cs[0, 1] = (10, 2550, 0)
    cs[0, 3] = (4, 510, 3)
    cs[2, 0] = (8, 8 * 51, 8)
    inst = np.zeros((3, 2, 3), dtype=np.int64)
    inst[0, 0] = (4, 4 * 255, 0)
    inst[0, 1] = (6, 6 * 85, 6)
    rep = C.ConfidenceReport.from_sums(cs, inst, low=100, names=["bg", "shaft", "wrist", "clasper"], frames=[4, 2, 0], sequences=[0, 0, 1])
    assert len(rep) == 3 and rep.low == 100 and rep.frames == [4, 2, 0] and rep.sequences == [0, 0, 1]
    assert rep.mean[0, 1] == 1.0 and rep.mean[0, 3] == 0.5 and rep.mean[2, 0] == 0.2 and rep.low_fraction[0, 3] == 0.75
    assert np.isnan(rep.mean[1]).all() and np.isnan(rep.low_fraction[0, 0]) and rep.low_fraction[2, 0] == 1.0
    assert rep.instance_mean[0].tolist() == [1.0, 85 / 255] and rep.instance_low_fraction[0].tolist() == [0.0, 1.0]
    assert np.isnan(rep.instance_mean[1:]).all()
    rows = rep.as_rows()
    assert [(r["sequence"], r["frame"], r["class"], r["name"]) for r in rows] == [(0, 4, 1, "shaft"), (0, 4, 3, "clasper"), (1, 0, 0, "bg")]
    assert rows[1] == {"sequence": 0, "frame": 4, "class": 3, "name": "clasper", "pixels": 4, "mean": 0.5, "low_fraction": 0.75}
    one = C.ConfidenceReport.from_sums(cs[0])                                # one frame's sums, the "frame" mode
    assert len(one) == 1 and one.frames == [0] and one.instance_mean is None and one.names is None and one.mean[0, 1] == 1.0
    for bad in (dict(class_sums=cs[:, :, :2]), dict(class_sums=cs.astype(np.float64)), dict(instance_sums=inst[:2]), dict(names=["a"]),
                dict(frames=[0]), dict(sequences=[0]), dict(low=300)):
        with pytest.raises(ValueError):
            C.ConfidenceReport.from_sums(**{"class_sums": cs, **bad})


def test_mask_report_objects_gain_a_score_only_with_a_report():
    labels = np.zeros((1, 4, 6), dtype=np.uint8)
    labels[0, 1:3, 1:3] = 2
    labels[0, 3, 4:] = 1
    conf = np.full((1, 4, 6), 255, dtype=np.uint8)
    conf[0, 1, 1:3] = 0
    runs, count = R.encode(labels, 32)
    assert all("score" not in d for d in R.MaskReport(runs, count, (4, 6), skip=(0,)).objects(0))
    rep = C.ConfidenceReport.from_sums(C.confidence_sums(labels, conf, 3))
    objs = R.MaskReport(runs, count, (4, 6), skip=(0,), confidence=rep).objects(0)
    assert [(d["cls"], d["score"]) for d in objs] == [(1, 1.0), (2, 0.5)]
    comp = np.where(labels == 2, 0, np.where(labels == 1, 1, -1)).astype(np.int32)
    cruns, ccount = R.encode(comp, 32)
    with pytest.raises(ValueError, match="instance sums"):
        R.MaskReport(cruns, ccount, (4, 6), "instances", confidence=rep)
    both = C.ConfidenceReport.from_sums(C.confidence_sums(labels, conf, 3), C.confidence_sums(comp, conf, 1))
    objs = R.MaskReport(cruns, ccount, (4, 6), "instances", confidence=both).objects(0)
    assert [(d["instance"], d["score"]) for d in objs] == [(0, 0.5), (1, None)]     # ordinal 1 lies beyond the K of the sums
    with pytest.raises(ValueError, match="rows"):
        R.MaskReport(runs, count, (4, 6), confidence=C.ConfidenceReport.from_sums(np.zeros((2, 3, 3), dtype=np.int64)))


# ---------------------------------------------------------------------------------------------------------------- the chain
def _chain(*extra, out="labels", **kw):
    args = dict(report=None, min_area=1, instances=None, connectivity=8, instance_skip=None, tracks=False, track_iou=100, track_same_class=True)
    for k in list(kw):
        if k in args:
            args[k] = kw.pop(k)
    return ReportChain("cpu", kw.pop("classes", 12), "endovis18", out, *args.values(), *extra, **kw)


def test_report_chain_confidence_refusals_and_log_columns():
    for kw in (dict(confidence="always"), dict(confidence=True), dict(confidence="frame", out="logits"),
               dict(confidence="deferred", out="logits"), dict(confidence_low=64), dict(confidence="frame", confidence_low=257),
               dict(confidence="frame", confidence_low=-1), dict(confidence="deferred", confidence_low=64.0),
               dict(confidence="frame", confidence_low=True), dict(confidence="frame", classes=65)):
        with pytest.raises(StswinHipError, match="confidence"):
            _chain(**kw)
    c = _chain(confidence="frame", confidence_low=0)                       # needs neither report nor masks; "frame" logs nothing
    assert c.confidence == "frame" and c.confidence_low == 0 and c.report is None and c.masks is None and not c.log.columns
    c = _chain(confidence="deferred", confidence_low=256, out="overlay")
    assert c.log.columns == {"class_sums": ((12, 3), torch.int64)}
    c = _chain(confidence="deferred", report="frame", instances=4)
    assert list(c.log.columns) == ["class_sums", "instance_sums"] and c.log.columns["instance_sums"] == ((4, 3), torch.int64)
    c = _chain(None, 16384, 0, "deferred", 7, False)                         # the keywords' positions behind track_max_gap
    assert c.confidence == "deferred" and c.confidence_low == 7 and c.align_corners is False
    plain = _chain(report="deferred", masks="deferred")
    assert plain.confidence is None and list(plain.log.columns) == ["moments", "runs", "count"]
    assert _chain().labelled(torch.zeros(1, 4, 4, dtype=torch.uint8)) is None


def test_yield_appends_and_logs_the_confidence_fields():
    assert Yield._fields[:7] == ("moments", "rows", "total", "ids", "started", "runs", "count")
    conf = torch.arange(2 * 4 * 6, dtype=torch.uint8).view(2, 4, 6)
    cs = torch.arange(2 * 12 * 3, dtype=torch.int64).view(2, 12, 3)
    ins = torch.arange(2 * 4 * 3, dtype=torch.int64).view(2, 4, 3) + 100
    y = Yield(moments=torch.ones(2, 12, 10, dtype=torch.int64), conf=conf, class_sums=cs, instance_sums=ins).clip(1)
    assert tuple(y.conf.shape) == (1, 4, 6) and torch.equal(y.class_sums[0], cs[1])
    assert len(y.appended("r")) == 2 and len(y.appended("r", False)) == 1            # today's tuples without the new argument
    r = y.appended(("r", 0.5), True, False, True)
    assert len(r) == 6 and torch.equal(r[3], conf[1]) and torch.equal(r[4], cs[1]) and torch.equal(r[5], ins[1])
    assert len(y._replace(instance_sums=None).appended("r", False, False, True)) == 3
    # "frame": appended behind the result, nothing logged; "deferred": results unchanged, the sums (not the map) logged
    c = _chain(confidence="frame")
    res = c.released([3], ["a"], [y._replace(moments=None, instance_sums=None)])
    assert len(res[0]) == 3 and res[0][0] == "a" and torch.equal(res[0][1], conf[1]) and not c.log.keys
    c = _chain(confidence="deferred", report="frame", instances=4)
    res = c.released([3], ["a"], [y._replace(rows=torch.zeros(1, 4, 12, dtype=torch.int64), total=torch.zeros(1, dtype=torch.int32))])
    assert len(res[0]) == 4 and c.log.keys == [(0, 3)] and "conf" not in c.log.columns
    cols, sequences, frames = c.log.download()
    assert np.array_equal(cols["class_sums"][0], cs[1].numpy()) and np.array_equal(cols["instance_sums"][0], ins[1].numpy())
    # report="deferred" beside confidence="frame": the log has the report's columns only
    c = _chain(confidence="frame", report="deferred")
    res = c.released([0], ["a"], [y._replace(instance_sums=None)])
    assert len(res[0]) == 3 and list(c.log.columns) == ["moments"] and c.log.keys == [(0, 0)]


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_abi_declares_the_confidence_launches():
    for s in ("stswin_upsample_confidence", "stswin_confidence_sums"):
        assert s in hip.declared_symbols()
    lib = hip.load()
    assert lib.stswin_abi_version() == 1 and hasattr(lib, "stswin_upsample_confidence") and hasattr(lib, "stswin_confidence_sums")
    # refusals that need no GPU: the checks run before anything is launched
    assert lib.stswin_upsample_confidence(1, None, None, None, 1, 1, 3, 4, 4, 8, 8, None) == -1882
    assert lib.stswin_upsample_confidence(1, None, None, None, 1, 1, 0, 4, 4, 8, 8, None) == -1881
    assert lib.stswin_upsample_confidence(1, None, None, None, 1, 1, 65, 4, 4, 8, 8, None) == -1881
    assert lib.stswin_upsample_confidence(1, None, None, None, 1, 0, 3, 4, 4, 8, 8, None) == -1880
    assert lib.stswin_upsample_confidence(1, None, None, None, 1, 1, 3, 4, 4, 8, 0, None) == -1880
    assert lib.stswin_confidence_sums(None, 1, None, None, 4, 128, 1, 8, 8, None) == -1885
    assert lib.stswin_confidence_sums(None, 1, None, None, 4, 128, 0, 8, 8, None) == -1884
    assert lib.stswin_confidence_sums(None, 1, None, None, 4, 128, 1, 8, 16385, None) == -1884
    with pytest.raises(StswinHipError, match="GPU"):
        hip.upsample_confidence(torch.zeros(1, 3, 4, 4), torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(StswinHipError, match="GPU"):
        hip.confidence_sums(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8), 4)
    with pytest.raises(StswinHipError, match="GPU"):
        hip.confidence_sums(torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8, dtype=torch.uint8), 4, 0)
