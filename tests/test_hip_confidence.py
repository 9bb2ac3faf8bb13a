"""hip.upsample_confidence and hip.confidence_sums against the numpy definitions (stswincl_amd/utils/confidence.py), and
VideoSegmenter(confidence=...).

The map: every pixel within 0.5 + EPS of 255 p_ref.  Largest excess over 0.5 seen on an MI355X over all the cases below: 1.79e-05
(4x5 -> 30x37, bf16); the bound stays the derived cap, EPS = 0.01."""
import numpy as np
import pytest
import torch

import test_hip_components as C
import test_hip_tracks as T
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import confidence as CF, instruments as I

pytestmark = pytest.mark.gpu

# The reference shares the kernel's float32 source coordinates, so what remains between q and 255 p_ref beside the rounding to a byte
# (0.5) is float32 arithmetic: a few ulps on each interpolated value (|v| <= 16: about 4e-6 absolute, as much relative on p), a couple
# of ulps per expf and nc <= 64 ulps on the sum - below 2e-5 relative on p, 5e-3 in units of a byte.  EPS doubles that.  A cap, not
# a measurement.
EPS = 0.01

# (h, w, H, W, align_corners)
GEOMETRIES = [(1, 1, 8, 8, True), (4, 5, 30, 37, True), (5, 6, 40, 48, True), (13, 9, 5, 7, True), (6, 10, 6, 10, True),
              (16, 20, 34, 60, False), (16, 20, 128, 160, False), (64, 80, 135, 240, False)]
FRAMES = 3


def _padded(shape, dtype, offset=0, fill=77):
    """A tensor of `shape` whose bytes start `offset` bytes behind a 512-byte boundary, inside a buffer of `fill`: (view, buffer)."""
    n = int(np.prod(shape))
    size = torch.empty(0, dtype=dtype).element_size()
    assert offset % size == 0
    buf = torch.full((n + 256 + offset // size,), fill, dtype=dtype, device="cuda")
    lo = 128 + offset // size
    return buf[lo:lo + n].view(shape), buf


def _sentinels_hold(view, buf, fill=77):
    n, lo = view.numel(), view.storage_offset()
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + n:] == fill).all())


def _logits(nc, h, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(FRAMES, nc, h, w, generator=g) * 3).clamp_(-16, 16).to(dtype).cuda()


def _excess(q, softmax, labels):
    """max over the pixels of |q - 255 p_ref| - 0.5, p_ref the reference's softmax [F][nc][H][W] at the labels."""
    p = CF.pick_labels(softmax, labels.cpu().numpy())
    return float((np.abs(q.cpu().numpy().astype(np.float64) - 255.0 * p) - 0.5).max())


# --------------------------------------------------------------------------------------------------- the map against the reference
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("h,w,H,W,align", GEOMETRIES)
def test_every_pixel_is_within_half_a_step_of_the_reference(h, w, H, W, align, dtype):
    worst = -1.0
    for nc in (1, 3, 12, 64):
        lg = _logits(nc, h, w, dtype, seed=nc + 100 * h)
        made = [hip.upsample_argmax_cm(lg, H, W, align_corners=align)]
        if align:
            made.append(hip.upsample_argmax(lg, H, W)[0])
            assert torch.equal(made[0], made[1])
        g = torch.Generator().manual_seed(nc + H)
        rnd = torch.randint(0, nc + 3, (FRAMES, H, W), generator=g).to(torch.uint8)
        rnd[:, 0, 0] = 255
        # the reference, once per logits, on what the kernel reads (bf16 values are exact in float64)
        softmax = CF.upsample_softmax(lg.float().cpu().numpy(), (H, W), align)
        for labels in made[:1] + [rnd.cuda()]:
            q = hip.upsample_confidence(lg, labels, align)
            assert q.dtype == torch.uint8 and tuple(q.shape) == (FRAMES, H, W)
            e = _excess(q, softmax, labels)
            worst = max(worst, e)
            assert e <= EPS, (nc, e)
            assert bool((q[labels >= nc] == 0).all())
            one = hip.upsample_confidence(lg[:1], labels[:1], align)       # one frame: the first of the three, bit for bit
            assert torch.equal(one, q[:1])
        arg = hip.upsample_confidence(lg, made[0], align)                    # the largest probability: never below 1 / nc
        assert int(arg.min()) >= int(np.floor(255.0 / nc + 0.5)) - 1
    print(f"[confidence] {(h, w)} -> {(H, W)} align={align} {dtype}: largest excess over 0.5 = {worst:.3g}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_exact_cases(dtype):
    for align, (H, W) in ((True, (30, 37)), (False, (34, 60))):
        for nc, want in ((1, 255), (3, 85), (5, 51), (15, 17)):
            labels = torch.randint(0, nc, (2, H, W), generator=torch.Generator().manual_seed(nc)).to(torch.uint8).cuda()
            for value in (0.0, -3.25, 7.5):
                lg = torch.full((2, nc, 4, 5), value, dtype=dtype, device="cuda")
                assert bool((hip.upsample_confidence(lg, labels, align) == want).all()), (nc, value, align)
        lg = torch.zeros(1, 6, 4, 5, dtype=dtype, device="cuda")
        lg[:, 2] = 80.0
        labels = torch.full((1, H, W), 2, dtype=torch.uint8, device="cuda")
        assert bool((hip.upsample_confidence(lg, labels, align) == 255).all())
        assert bool((hip.upsample_confidence(lg, torch.zeros_like(labels), align) == 0).all())
        for value in (1e4, -1e4):                                           # equal logits far out: 1 / 4 -> 64, no NaN on the way
            lg = torch.full((1, 4, 4, 5), value, dtype=dtype, device="cuda")
            assert bool((hip.upsample_confidence(lg, torch.zeros_like(labels), align) == 64).all()), value
        lg = _logits(3, 4, 5, dtype, seed=9)[:1]
        for bad in (3, 4, 64, 255):
            assert bool((hip.upsample_confidence(lg, torch.full_like(labels, bad), align) == 0).all())


# ------------------------------------------------------------------------------------------------------------- map plumbing
@pytest.mark.parametrize("W", [48, 37])
def test_the_wide_and_the_byte_body_agree_and_write_nothing_else(W):
    H, nc = 40, 12
    lg = _logits(nc, 5, 6, torch.float32, seed=3)
    labels = hip.upsample_argmax(lg, H, W)[0]
    want = hip.upsample_confidence(lg, labels)                              # fresh tensors: aligned; W = 48 takes the wide body
    assert labels.data_ptr() % 4 == 0 and want.data_ptr() % 4 == 0
    for lab_off, out_off in ((0, 0), (1, 0), (0, 1), (3, 2), (2, 2)):
        lab, lab_buf = _padded(labels.shape, torch.uint8, lab_off)
        lab.copy_(labels)
        out, out_buf = _padded(labels.shape, torch.uint8, out_off, fill=201)
        assert lab.data_ptr() % 4 == lab_off and out.data_ptr() % 4 == out_off
        assert hip.upsample_confidence(lg, lab, out=out) is out
        assert torch.equal(out, want), (lab_off, out_off)
        assert _sentinels_hold(out, out_buf, 201) and _sentinels_hold(lab, lab_buf) and torch.equal(lab, labels)


def test_map_wrapper_refusals():
    lg = torch.zeros(2, 3, 4, 5, device="cuda")
    lab = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    for a, b, kw in ((lg[0], lab, {}), (lg, lab[0], {}), (lg.double(), lab, {}), (lg, lab.int(), {}), (lg, lab[:1], {}),
                     (lg[:, :, :, ::2], lab, {}), (lg, lab[:, :, ::2], {}), (torch.zeros(2, 65, 4, 5, device="cuda"), lab, {}),
                     (lg, lab, dict(out=torch.zeros(2, 8, 10, device="cuda"))), (lg, lab, dict(out=lab)),
                     (lg, lab, dict(out=torch.zeros(2, 8, 9, dtype=torch.uint8, device="cuda"))), (lg.cpu(), lab, {}), (lg, lab.cpu(), {})):
        with pytest.raises(StswinHipError, match="upsample_confidence"):
            hip.upsample_confidence(a, b, **kw)


# --------------------------------------------------------------------------------------------------------- confidence_sums
def _ids(shape, dtype, K, seed, coherent):
    g = np.random.default_rng(seed)
    hi = min(K + 3, 256) if dtype == np.uint8 else K + 3
    if coherent:                                                            # blocks of 8 x 24 pixels of one id: long runs
        n, H, W = shape
        cells = g.integers(0, hi, (n, (H + 7) // 8, (W + 23) // 24))
        m = np.repeat(np.repeat(cells, 8, axis=1), 24, axis=2)[:, :H, :W]
    else:
        m = g.integers(0, hi, shape)
    m = m.astype(dtype)
    if dtype == np.int32:
        m[g.random(shape) < 0.2] = -1
    return np.ascontiguousarray(m)


def _check_sums(maps, conf, K, low, map_off=0, conf_off=0):
    want = torch.from_numpy(CF.confidence_sums(maps, conf, K, low))
    dm, dm_buf = _padded(maps.shape, torch.from_numpy(maps).dtype, map_off)
    dm.copy_(torch.from_numpy(maps))
    dc, dc_buf = _padded(conf.shape, torch.uint8, conf_off)
    dc.copy_(torch.from_numpy(conf))
    out, out_buf = _padded((maps.shape[0], K, 3), torch.int64, fill=-5)
    assert hip.confidence_sums(dm, dc, K, low, out=out) is out
    bad = (out.cpu() != want).nonzero()
    assert bad.numel() == 0, (bad[:6].tolist(), out.cpu()[tuple(bad[0])].item(), want[tuple(bad[0])].item())
    assert _sentinels_hold(out, out_buf, -5) and _sentinels_hold(dm, dm_buf) and _sentinels_hold(dc, dc_buf)
    hip.confidence_sums(dm, dc, K, low, out=out)                            # a second call overwrites, it does not accumulate
    assert torch.equal(out.cpu(), want)
    fresh = hip.confidence_sums(dm, dc, K, low)                             # the wrapper's own out
    assert fresh.dtype == torch.int64 and torch.equal(fresh.cpu(), want)
    assert torch.equal(dm.cpu(), torch.from_numpy(maps)) and torch.equal(dc.cpu(), torch.from_numpy(conf))


@pytest.mark.parametrize("K", [1, 12, 64, 1024])
@pytest.mark.parametrize("dtype", [np.uint8, np.int32], ids=["uint8", "int32"])
def test_sums_equal_the_definition(dtype, K):
    size = 4 if dtype == np.int32 else 1
    for shape in ((3, 67, 131), (2, 64, 80)):                               # H W % 16 != 0: the element body; == 0 and aligned: 16-byte loads
        for coherent in (False, True):
            maps = _ids(shape, dtype, K, seed=K + shape[1], coherent=coherent)
            assert coherent or (maps.min() < (0 if dtype == np.int32 else 1) and maps.max() >= min(K, 255))
            conf = np.random.default_rng(K).integers(0, 256, shape).astype(np.uint8)
            for low in (0, 128, 256):
                _check_sums(maps, conf, K, low)
            _check_sums(maps, conf, K, 128, map_off=size, conf_off=0)       # either pointer off a 16-byte boundary: the element body
            _check_sums(maps, conf, K, 128, map_off=0, conf_off=3)
            _check_sums(maps, conf, K, 77, map_off=3 * size, conf_off=1)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32], ids=["uint8", "int32"])
@pytest.mark.parametrize("shape", [(3, 67, 131), (1, 540, 960)])
def test_every_pixel_in_one_bin_at_full_confidence(shape, dtype):
    maps = np.full(shape, 2, dtype=dtype)
    conf = np.full(shape, 255, dtype=np.uint8)
    _check_sums(maps, conf, 12, 128)
    got = hip.confidence_sums(torch.from_numpy(maps).cuda(), torch.from_numpy(conf).cuda(), 3, 256).cpu()
    hw = shape[1] * shape[2]
    assert got[:, 2].tolist() == [[hw, 255 * hw, hw]] * shape[0] and int(got[:, :2].abs().sum()) == 0


def test_sums_wrapper_refusals():
    m = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    q = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    for a, b, kw in ((m[0], q[0], {}), (m.long(), q, {}), (m, q.int(), {}), (m, q[:1], {}), (m[:, :, ::2], q[:, :, ::2], {}),
                     (m, q, dict(K=0)), (m, q, dict(K=1025)), (m, q, dict(K=4.0)), (m, q, dict(low=-1)), (m, q, dict(low=257)),
                     (m, q, dict(low=True)), (m, q, dict(out=torch.zeros(2, 4, 3, device="cuda"))),
                     (m, q, dict(out=torch.zeros(2, 5, 3, dtype=torch.int64, device="cuda"))), (m.cpu(), q, {}), (m, q.cpu(), {})):
        with pytest.raises(StswinHipError, match="confidence_sums"):
            hip.confidence_sums(a, b, **{"K": 4, **kw})
    lib = hip.load()
    out = torch.zeros(2, 4, 3, dtype=torch.int64, device="cuda")
    args = (q.data_ptr(), out.data_ptr(), 4, 128, 2, 8, 10, None)
    assert lib.stswin_confidence_sums(m.data_ptr(), 2, *args) == -1886
    assert lib.stswin_confidence_sums(m.data_ptr() + 1, 4, *args) == -1889
    assert lib.stswin_confidence_sums(m.data_ptr(), 1, q.data_ptr(), out.data_ptr() + 4, 4, 128, 2, 8, 10, None) == -1889
    assert lib.stswin_confidence_sums(m.data_ptr(), 1, q.data_ptr(), out.data_ptr(), 4, 300, 2, 8, 10, None) == -1888
    assert lib.stswin_upsample_confidence(2, m.data_ptr(), m.data_ptr(), q.data_ptr(), 1, 1, 3, 4, 4, 8, 10, None) == -1883
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                        # refused before anything was launched


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE, N = C.SIZE, C.N
K = 4
LOW = 128
_WANT = {}
_SEG_MODES = {"eager": {}, "batch2": dict(batch=2), "graph": dict(graph=True)}


def _want(protocol):
    """Per protocol, on the shared case's first sequence: the confidence maps hip.upsample_confidence makes of the logits of an
    out="logits" segmenter and the case's labels, and hip.confidence_sums of them over the labels and over the host's component maps.
    Computed once, shared, never changed."""
    if protocol not in _WANT:
        c = C._case(protocol)
        s = c["seqs"][0]
        with torch.no_grad():
            logits = torch.stack(video.VideoSegmenter(c["m"], protocol=protocol).segment_sequence(s["fr"]))
        labels = s["labels"].cuda()
        conf = hip.upsample_confidence(logits, labels, protocol != "cadis")
        comp = torch.from_numpy(I.label_components(s["labels"].numpy(), c["nc"], 8, c["skip"], K)[0].astype(np.int32)).cuda()
        low = max(int(np.median(conf.cpu().numpy())), int(conf.min()) + 1)   # confidence_low: some pixels lie below it and some do not
        assert int(conf.min()) < low <= int(conf.max()), "the random model is as sure everywhere: the sums test little"
        _WANT[protocol] = dict(conf=conf.cpu(), low=low, sums=hip.confidence_sums(labels, conf, c["nc"], low).cpu(),
                               inst=hip.confidence_sums(comp, conf, K, low).cpu())
    return _WANT[protocol]


def _is_want(r, w, f, inst=False):
    """The last 2 (3) elements of result r are frame f's (conf, class_sums[, instance_sums]) on the device."""
    tail = r[-3:] if inst else r[-2:]
    ok = all(t.is_cuda for t in tail) and tail[0].dtype == torch.uint8 and tuple(tail[0].shape) == SIZE and tail[1].dtype == torch.int64
    ok = ok and torch.equal(tail[0].cpu(), w["conf"][f]) and torch.equal(tail[1].cpu(), w["sums"][f])
    return ok and (not inst or torch.equal(tail[2].cpu(), w["inst"][f]))


@pytest.mark.parametrize("mode", list(_SEG_MODES))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_frame_confidence(protocol, mode):
    c, w = C._case(protocol), _want(protocol)
    s = c["seqs"][0]
    plain_kw = dict(out="labels", out_size=SIZE, protocol=protocol, **_SEG_MODES[mode])
    kw = dict(confidence_low=w["low"], **plain_kw)
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], confidence="frame", **kw)
        got = seg.segment_sequence(s["fr"])
        assert len(got) == N
        for f, r in enumerate(got):                                          # the labels are those of a segmenter without the keyword
            assert len(r) == 3 and torch.equal(r[0].cpu(), s["labels"][f]) and _is_want(r, w, f), f
            assert torch.equal(r[2], hip.confidence_sums(r[0][None], r[1][None], c["nc"], w["low"])[0]), f
        # with ground truth the labels, and so the maps and sums, come from the scoring launches: the same bits
        plain = video.VideoSegmenter(c["m"], **plain_kw).segment_sequence(s["fr"], gt=s["gt"])
        for f, (r, p) in enumerate(zip(seg.segment_sequence(s["fr"], gt=s["gt"]), plain)):
            p = p if isinstance(p, tuple) else (p,)
            assert len(r) == len(p) + 2 and torch.equal(r[0], p[0]) and list(r[1:len(p)]) == list(p[1:]) and _is_want(r, w, f), f
        if protocol == "endovis18":
            scored = video.VideoSegmenter(c["m"], confidence="frame", scores="deferred", **kw)
            for f, r in enumerate(scored.segment_sequence(s["fr"], gt=s["gt"])):
                assert len(r) == 3 and torch.equal(r[0].cpu(), s["labels"][f]) and _is_want(r, w, f), f
            assert len(scored.endo_scores().frames) == N


@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_eager_and_graph_agree_with_instances_and_tracks(protocol):
    c = T._case(protocol)
    s = c["seqs"][0]
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, tracks=True, confidence="frame",
              confidence_low=LOW)
    with torch.no_grad():
        eager = video.VideoSegmenter(c["m"], **kw).segment_sequence(s["fr"])
        graphed = video.VideoSegmenter(c["m"], graph=True, **kw)
        graph = graphed.segment_sequence(s["fr"])
        plain = video.VideoSegmenter(c["m"], **{**kw, "confidence": None}).segment_sequence(s["fr"])
    assert graphed.captured and len(eager) == len(graph) == N
    for f, (e, g, p) in enumerate(zip(eager, graph, plain)):                 # frames 4 and 5 (5 and 6) were parked on the way
        assert len(e) == len(g) == 8 and len(p) == 5, f
        assert all(torch.equal(a, b) for a, b in zip(e, g)), f
        assert all(torch.equal(a, b) for a, b in zip(e[:5], p)), f           # what was there is what it was
        comp = torch.from_numpy(I.label_components(e[0].cpu().numpy()[None], c["nc"], 8, c["skip"], K)[0].astype(np.int32)).cuda()
        assert torch.equal(e[7], hip.confidence_sums(comp, e[5][None], K, LOW)[0]), f
        assert torch.equal(e[6], hip.confidence_sums(e[0][None], e[5][None], c["nc"], LOW)[0]), f
    assert any(int(e[7][:, 0].sum()) > 0 for e in eager), "no frame has an instance: the instance sums test little"


@pytest.mark.parametrize("protocol,mode", [("endovis18", "eager"), ("endovis18", "batch2"), ("endovis18", "graph"), ("cadis", "graph")])
def test_segmenter_deferred_confidence(protocol, mode):
    c, w = C._case(protocol), _want(protocol)
    a, b = c["seqs"]
    names = [f"class {k}" for k in range(c["nc"])]
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="deferred", instances=K, masks="deferred", mask_runs=2048,
              confidence="deferred", confidence_low=w["low"], **_SEG_MODES[mode])
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], **kw)
        assert len(seg.confidence_report()) == 0
        got = seg.segment_sequence(a["fr"]) + seg.segment_sequence(b["fr"])  # (segment_sequence ends with a reset(): the log is kept)
    assert all(isinstance(r, torch.Tensor) for r in got)                      # the results are unchanged
    assert all(torch.equal(r.cpu(), q["labels"][f]) for q, part in ((a, got[:N]), (b, got[N:])) for f, r in enumerate(part))
    rep = seg.confidence_report(names=names)
    assert rep.sequences == [0] * N + [1] * N and rep.frames == list(range(N)) * 2 and rep.low == w["low"] and rep.names == names
    assert np.array_equal(rep.class_sums[:N], w["sums"].numpy()) and np.array_equal(rep.instance_sums[:N], w["inst"].numpy())
    want = CF.ConfidenceReport.from_sums(w["sums"].numpy(), w["inst"].numpy())
    assert np.array_equal(rep.mean[:N], want.mean, equal_nan=True) and np.array_equal(rep.low_fraction[:N], want.low_fraction, equal_nan=True)
    masks = seg.mask_report(names=names)                                      # the objects carry the instance's mean probability
    scores = 0
    for r in range(N):
        for o in masks.objects(r):
            i = o["instance"]
            assert o["score"] == (float(want.instance_mean[r, i]) if i < K else None), (r, i)
            scores += o["score"] is not None
    assert scores >= 2
    seg.reset_metrics()
    assert len(seg.confidence_report()) == 0 and len(seg.mask_report()) == 0


def test_segmenter_overlay_and_label_scores():
    c, w = C._case("endovis18"), _want("endovis18")
    s = c["seqs"][0]
    with torch.no_grad():
        plain = video.VideoSegmenter(c["m"], out="overlay").segment_sequence(s["fr"])
        seg = video.VideoSegmenter(c["m"], out="overlay", confidence="frame", confidence_low=w["low"], masks="deferred", mask_runs=2048)
        got = seg.segment_sequence(s["fr"])
        both = video.VideoSegmenter(c["m"], out="overlay", confidence="deferred", masks="deferred", mask_runs=2048, batch=2)
        both.segment_sequence(s["fr"])
    for f, (r, p) in enumerate(zip(got, plain)):
        assert len(r) == 3 and torch.equal(r[0], p) and _is_want(r, w, f), f
    assert all("score" not in o for o in seg.mask_report().objects(0))        # confidence="frame": nothing in the log to score with
    with pytest.raises(StswinHipError, match="deferred"):
        seg.confidence_report()
    want = CF.ConfidenceReport.from_sums(w["sums"].numpy())
    rep = both.mask_report()
    scored = 0
    for f in range(N):                                                       # source "labels": the class's mean probability
        objs = rep.objects(f)
        assert all(o["score"] == float(want.mean[f, o["cls"]]) for o in objs), f
        scored += len(objs)
    assert scored >= 1


def test_segmenter_confidence_refusals():
    m = C._case("endovis18")["m"]
    for kwargs in (dict(out="labels", confidence="always"), dict(out="labels", confidence=True), dict(out="logits", confidence="frame"),
                   dict(confidence="deferred"), dict(out="labels", confidence_low=64), dict(out="labels", confidence="frame", confidence_low=257),
                   dict(out="labels", confidence="frame", confidence_low=-1), dict(out="labels", confidence="deferred", confidence_low=128.0)):
        with pytest.raises(StswinHipError, match="confidence"):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(out="labels", confidence="frame"), dict(out="labels", report="deferred"), dict(out="labels")):
        with pytest.raises(StswinHipError, match="confidence"):
            video.VideoSegmenter(m, **kwargs).confidence_report()
    seg = video.VideoSegmenter(m, out="overlay", confidence="deferred", confidence_low=0)
    assert seg.confidence == "deferred" and seg.confidence_low == 0 and seg.report is None and seg.masks is None
