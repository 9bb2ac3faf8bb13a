"""GPU: stswin_gt_decode / hip.gt_decode against utils.groundtruth.decode_colours / decode_ids, and VideoSegmenter(gt_table=...,
scores="deferred") against the int64 / scores="frame" path."""
import os

import numpy as np
import pytest
import torch

from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import EndoMetric as EM
from stswincl_amd.utils import groundtruth as G
from stswincl_amd.utils import visualize as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay_colormap.npz")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _colour_case(n, H, W, ch, ncolours, seed):
    """A table of `ncolours` rows whose last row repeats the first row's colour under another label (ncolours > 1), and an image
    of table colours, of table colours with one channel off by 1, and of random colours; random alpha."""
    g = np.random.default_rng(seed)
    colours = g.integers(0, 256, (ncolours, 3))
    if ncolours > 1:
        colours[-1] = colours[0]
    table = G.colour_table(colours.tolist(), labels=g.permutation(256)[:ncolours].tolist())
    img = colours[g.integers(0, ncolours, (n, H, W))]
    off = g.random((n, H, W)) < 0.15
    chan = g.integers(0, 3, (n, H, W))
    img[off, chan[off]] = (img[off, chan[off]] + 1) % 256
    rnd = g.random((n, H, W)) < 0.1
    img[rnd] = g.integers(0, 256, (int(rnd.sum()), 3))
    img.reshape(-1, 3)[0] = colours[0]                          # the duplicate colour occurs even in a 1 x 1 image
    img = img.astype(np.uint8)
    if ch == 4:
        img = np.concatenate([img, g.integers(0, 256, (n, H, W, 1), dtype=np.uint8)], axis=3)
    return img, table


def _id_case(n, H, W, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, H, W), dtype=np.uint8), g.integers(0, 256, 256, dtype=np.uint8)


def _same(got: torch.Tensor, want: np.ndarray, dtype) -> bool:
    return got.dtype == dtype and got.shape == want.shape and torch.equal(got.cpu(), torch.from_numpy(want).to(dtype))


SHAPES = [(1, 1, 1), (2, 5, 7), (3, 33, 130)]      # 33 * 130 = 4290 is no multiple of 4: frames 1 and 2 start off the vector grid; 13 workgroups


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("ncolours", [1, 12, 256])
@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_colour_form_against_decode_colours(n, H, W, ch, ncolours, dtype):
    img, table = _colour_case(n, H, W, ch, ncolours, seed=H * W + ncolours + ch)
    want, missing = G.decode_colours(img, table)
    if ncolours > 1:
        assert want.reshape(-1)[0] == table[-1, 3] != table[0, 3]           # the later row of the duplicate colour decided
    if H * W > 1:
        assert 0 < missing.sum() < n * H * W
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    got = hip.gt_decode(_dev(img), _dev(table), dtype, unmatched=counts)
    assert _same(got, want, dtype)
    assert counts.cpu().tolist() == missing.tolist()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_id_form_against_decode_ids(n, H, W, dtype):
    img, table = _id_case(n, H, W, seed=H + W)
    assert _same(hip.gt_decode(_dev(img), _dev(table), dtype), G.decode_ids(img, table), dtype)


def _offset_view(a: np.ndarray, off: int, fill: int = 0):
    """(buffer, view): a contiguous GPU tensor holding `a`, `off` bytes into a uint8 allocation with 32 more bytes behind it."""
    nbytes = a.size * a.itemsize
    buf = torch.full((off + nbytes + 32,), fill, dtype=torch.uint8, device="cuda")
    v = buf[off:off + nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off
    return buf, v


@pytest.mark.parametrize("which", ["in", "out", "both"])
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_misaligned_in_and_uint8_out(ch, off, which):
    n, H, W = 2, 9, 31
    if ch == 1:
        img, table = _id_case(n, H, W, seed=off)
        want = G.decode_ids(img, table)
    else:
        img, table = _colour_case(n, H, W, ch, 12, seed=off + ch)
        want = G.decode_colours(img, table)[0]
    _, src = _offset_view(img, off if which in ("in", "both") else 0)
    o = off if which in ("out", "both") else 0
    buf, out = _offset_view(np.full((n, H, W), 171, np.uint8), o, fill=171)
    got = hip.gt_decode(src, _offset_view(table, 1)[1], torch.uint8, out=out)     # (the table's own alignment does not matter either)
    assert got is out and _same(got, want, torch.uint8)
    assert (buf[:o] == 171).all() and (buf[o + n * H * W:] == 171).all(), "bytes around out were written"


@pytest.mark.parametrize("ch", [1, 4])
def test_int64_out_that_is_only_8_byte_aligned(ch):
    n, H, W = 2, 9, 31
    img, table = _id_case(n, H, W, seed=3) if ch == 1 else _colour_case(n, H, W, 4, 12, seed=4)
    want = G.decode_ids(img, table) if ch == 1 else G.decode_colours(img, table)[0]
    buf, out = _offset_view(np.full((n, H, W), -1, np.int64), 8, fill=255)
    assert out.data_ptr() % 16 == 8
    got = hip.gt_decode(_dev(img), _dev(table), torch.int64, out=out)
    assert got is out and _same(got, want, torch.int64)
    assert (buf[:8] == 255).all() and (buf[8 + 8 * n * H * W:] == 255).all()


def test_unmatched_accumulates_and_may_be_absent():
    img, table = _colour_case(3, 33, 130, 4, 12, seed=8)
    img2 = np.ascontiguousarray(img[:, ::-1])
    img2[1] |= 1                                                # frame 1: fewer pixels still match
    m1, m2 = G.decode_colours(img, table)[1], G.decode_colours(img2, table)[1]
    assert m2[1] > m2[0] and (m1 > 0).all()
    counts = torch.full((3,), 5, dtype=torch.int32, device="cuda")        # never cleared by the kernel
    hip.gt_decode(_dev(img), _dev(table), unmatched=counts)
    assert counts.cpu().tolist() == (m1 + 5).tolist()
    hip.gt_decode(_dev(img2), _dev(table), torch.int64, unmatched=counts)
    assert counts.cpu().tolist() == (m1 + m2 + 5).tolist()
    assert _same(hip.gt_decode(_dev(img), _dev(table), unmatched=None), G.decode_colours(img, table)[0], torch.uint8)
    ids, idtab = _id_case(3, 33, 130, seed=1)                   # the id form counts nothing
    hip.gt_decode(_dev(ids), _dev(idtab), unmatched=counts)
    assert counts.cpu().tolist() == (m1 + m2 + 5).tolist()


def test_round_trip_through_the_overlay():
    g = np.random.default_rng(2)
    labels = _dev(g.integers(0, 256, (2, 96, 80), dtype=np.uint8))
    picture = hip.labels_overlay(labels, _dev(V.overlay_table(V.default_palette(), alpha=255)), None, None)
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    back = hip.gt_decode(picture, _dev(G.colour_table(V.default_palette())), unmatched=counts)
    assert torch.equal(back, labels) and counts.cpu().tolist() == [0, 0]


def test_one_full_size_frame():
    img, table = _colour_case(1, 1024, 1280, 4, 12, seed=11)
    want, missing = G.decode_colours(img, table)
    src, tab = _dev(img), _dev(table)
    for dtype in (torch.uint8, torch.int64):
        counts = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert _same(hip.gt_decode(src, tab, dtype, unmatched=counts), want, dtype)
        assert counts.cpu().tolist() == missing.tolist()


def test_refusals():
    img, table = _colour_case(2, 8, 16, 4, 12, seed=1)
    src, tab = _dev(img), _dev(table)
    ids, idtab = (_dev(a) for a in _id_case(2, 8, 16, seed=2))
    ok = hip.gt_decode(src, tab)
    sentinel = torch.full((2, 8, 16), 99, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    for args, kwargs in (((src.int(), tab), {}), ((src[0], tab), {}), ((src[..., :2], tab), {}), ((src[:, :, ::2], tab), {}),
                         ((src[..., :1].contiguous(), tab), {}), ((src[:0], tab), {}),
                         ((src, tab.int()), {}), ((src, tab[:, :3].contiguous()), {}), ((src, tab[:0]), {}), ((src, tab.cpu()), {}),
                         ((src, torch.zeros(257, 4, dtype=torch.uint8, device="cuda")), {}), ((src, idtab), {}), ((ids, tab), {}),
                         ((ids, idtab[:255]), {}), ((src, tab, torch.int32), {}), ((src, tab, torch.float32), {}),
                         ((src, tab), dict(unmatched=counts.long())), ((src, tab), dict(unmatched=counts[:1])),
                         ((src, tab), dict(unmatched=counts.cpu())), ((src, tab, torch.int64), dict(out=sentinel)),
                         ((src, tab), dict(out=sentinel[:1])), ((src, tab), dict(out=sentinel.cpu())),
                         ((src, tab), dict(out=sentinel.transpose(1, 2)))):
        with pytest.raises(StswinHipError):
            hip.gt_decode(*args, out=kwargs.pop("out", sentinel if len(args) < 3 else None), **kwargs)
    # out must not share memory with src
    with pytest.raises(StswinHipError, match="shares memory"):
        hip.gt_decode(src, tab, out=src.view(-1)[64:64 + 2 * 8 * 16].view(2, 8, 16))
    with pytest.raises(StswinHipError, match="shares memory"):
        hip.gt_decode(ids, idtab, out=ids)
    # the C entry point's own codes
    fn, st = hip.load().stswin_gt_decode, torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    assert fn(p(src), p(tab), p(sentinel), None, 0, 8, 16, 4, 12, 1, st) == -1418
    assert fn(p(src), p(tab), p(sentinel), None, 2, -8, 16, 4, 12, 1, st) == -1418
    assert fn(p(src), p(tab), p(sentinel), None, 2, 8, 0, 4, 12, 1, st) == -1418
    assert fn(None, p(tab), p(sentinel), None, 2, 8, 16, 4, 12, 1, st) == -1419
    assert fn(p(src), None, p(sentinel), None, 2, 8, 16, 4, 12, 1, st) == -1419
    assert fn(p(src), p(tab), None, None, 2, 8, 16, 4, 12, 1, st) == -1419
    assert fn(p(src), p(tab), p(sentinel), None, 2, 8, 16, 2, 12, 1, st) == -1420
    assert fn(p(src), p(tab), p(sentinel), None, 2, 8, 16, 5, 12, 1, st) == -1420
    assert fn(p(src), p(tab), p(sentinel), None, 2, 8, 16, 4, 0, 1, st) == -1421
    assert fn(p(src), p(tab), p(sentinel), None, 2, 8, 16, 4, 257, 1, st) == -1421
    assert fn(p(src), p(tab), p(sentinel), None, 2, 8, 16, 4, 12, 4, st) == -1422
    assert fn(p(src), p(tab), p(src) + 1000, None, 2, 8, 16, 4, 12, 1, st) == -1423
    assert fn(p(src), p(tab), p(src), None, 2, 8, 16, 4, 12, 8, st) == -1423
    torch.cuda.synchronize()
    assert (sentinel == 99).all() and (counts == 0).all() and torch.equal(src.cpu(), torch.from_numpy(img)), "a refused call launched"
    assert torch.equal(hip.gt_decode(src, tab), ok)


def test_capturable_into_a_graph():
    img, table = _colour_case(2, 33, 67, 4, 12, seed=9)
    src, tab = _dev(img), _dev(table)
    out = torch.zeros(2, 33, 67, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    hip.gt_decode(src, tab, torch.int64, counts, out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.gt_decode(src, tab, torch.int64, counts, out)
    img2, _ = _colour_case(2, 33, 67, 4, 12, seed=10)
    src.copy_(torch.from_numpy(img2))
    counts.zero_()
    graph.replay()
    want, missing = G.decode_colours(img2, table)
    assert not np.array_equal(want, G.decode_colours(img, table)[0])
    assert _same(out, want, torch.int64) and counts.cpu().tolist() == missing.tolist()


# ------------------------------------------------------------------------------------------------------- the segmenter
def _model(protocol, seed):
    torch.manual_seed(seed)
    if protocol == "cadis":
        from stswincl_amd.net.Ours.base_cata_np import TswinPlusv5
        m = TswinPlusv5(9, (8, 8))
    else:
        from stswincl_amd.net.Ours.base18 import TswinPlus
        m = TswinPlus(12, (8, 8))
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    return m.cuda().eval()


def _frames(n, hs, ws, seed):
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (1, hs, ws, 3), dtype=np.int64)
    return np.clip(base + g.integers(-24, 25, (n, hs, ws, 3)), 0, 255).astype(np.uint8)


def _host_counts(labels, gt, classes):
    """int32 [F][3][nc] from label maps: |gt|, |pred|, |gt & pred| per class."""
    out = np.zeros((len(labels), 3, classes), dtype=np.int32)
    for f, (p, y) in enumerate(zip(labels, gt)):
        for c in range(classes):
            out[f, :, c] = ((y == c).sum(), (p == c).sum(), ((y == c) & (p == c)).sum())
    return out


def _same_scores(got, want):
    for name in ("dice", "iou", "dice_seq", "iou_seq", "dice_each", "iou_each", "tool_each"):
        a, b = np.asarray(getattr(got, name), dtype=np.float64), np.asarray(getattr(want, name), dtype=np.float64)
        assert np.array_equal(a, b, equal_nan=True), name
    assert got.dices == want.dices and got.ious == want.ious and got.count == want.count and got.sequences == want.sequences
    assert got.empty_frames == want.empty_frames


@pytest.fixture(scope="module")
def endovis():
    """Two 10-frame sequences of 64 x 64 frames scored at 96 x 80 by the int64 gt / scores="frame" path, and the same ground truth
    as RGBA pictures under the first 12 colours of the default palette (a few pixels in a colour the table lacks: class 0)."""
    m = _model("endovis18", seed=4)
    size, n = (96, 80), 10
    g = np.random.default_rng(21)
    palette = V.default_palette()[:12]
    seqs = []
    for s in range(2):
        fr = _frames(n, 64, 64, seed=30 + s)
        gt = g.integers(0, 12, (n, *size))
        gt[:, 40:60, 10:50] = 3                              # some structure: not every class in every frame is a sliver
        stray = (g.random((n, *size)) < 0.01) & (gt == 0)
        rgba = np.concatenate([palette[gt], g.integers(0, 256, (n, *size, 1), dtype=np.uint8)], axis=3)
        rgba[stray, :3] = (1, 2, 3)
        assert stray.sum() > 0
        with torch.no_grad():
            res = video.VideoSegmenter(m, out="labels", out_size=size).segment_sequence(fr, gt=torch.from_numpy(gt))
        seqs.append(dict(fr=fr, gt=gt, rgba=rgba, stray=int(stray.sum()), res=res))
    return dict(m=m, size=size, seqs=seqs, table=G.colour_table(palette))


@pytest.mark.parametrize("mode", ["eager", "batch4", "graph"])
def test_segmenter_endovis18_stored_gt_and_deferred_scores(endovis, mode):
    e = endovis
    kw = dict(batch=4) if mode == "batch4" else dict(graph=True) if mode == "graph" else {}
    a, b = e["seqs"]
    with torch.no_grad():
        seg = video.VideoSegmenter(e["m"], out="labels", out_size=e["size"], gt_table=e["table"], scores="deferred", **kw)
        assert seg.endo_scores().count == 0 and seg.unmatched() == 0
        got_a = seg.segment_sequence(a["fr"], gt=a["rgba"])                   # stored form from the host
        one = seg.endo_scores()
        got_b = seg.segment_sequence(b["fr"], gt=torch.from_numpy(b["rgba"]).cuda())     # ... and from the device
        two = seg.endo_scores()
    for got, s in ((got_a, a), (got_b, b)):
        assert len(got) == 10
        for f in range(10):
            assert isinstance(got[f], torch.Tensor) and torch.equal(got[f], s["res"][f][0]), f
    assert seg.unmatched() == a["stray"] + b["stray"]
    # per-frame lists: those of the frame path; aggregates: from_counts of the frame path's counts
    assert one.dices == [r[1] for r in a["res"]] and one.ious == [r[2] for r in a["res"]]
    assert one.frames == list(range(10)) and one.sequences == [0] * 10
    counts = [_host_counts([r[0].cpu().numpy() for r in s["res"]], s["gt"], 12) for s in (a, b)]
    _same_scores(one, EM.EndoScores.from_counts(counts[0], [0] * 10))
    assert np.isfinite(one.dice) and 0 <= one.iou <= one.dice <= 1
    assert two.dices == [r[1] for r in a["res"] + b["res"]] and two.ious == [r[2] for r in a["res"] + b["res"]]
    assert two.sequences == [0] * 10 + [1] * 10 and two.frames == list(range(10)) * 2          # segment_sequence resets twice
    _same_scores(two, EM.EndoScores.from_counts(np.concatenate(counts), [0] * 10 + [1] * 10))
    assert two.dice_seq[0] == one.dice and two.dice_seq[1] == EM.EndoScores.from_counts(counts[1]).dice
    seg.reset_metrics()
    empty = seg.endo_scores()
    assert empty.count == 0 and empty.dices == [] and seg.unmatched() == 0
    with torch.no_grad():
        seg.segment_sequence(b["fr"], gt=b["rgba"])
    again = seg.endo_scores()
    assert again.sequences == [0] * 10 and again.dice == two.dice_seq[1]


def test_segmenter_deferred_log_grows_and_frame_scores_with_stored_gt(endovis):
    e = endovis
    a = e["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(e["m"], out="labels", out_size=e["size"], scores="deferred")     # int64 gt, deferred
        for _ in range(7):                                   # 70 rows: past the log's first 64
            seg.segment_sequence(a["fr"], gt=torch.from_numpy(a["gt"]))
        sc = seg.endo_scores()
        stored = video.VideoSegmenter(e["m"], out="labels", out_size=e["size"], gt_table=e["table"])      # stored gt, scores="frame"
        res = stored.segment_sequence(a["fr"], gt=a["rgba"][..., :3])                                 # RGB
    assert sc.count == 70 and sc.sequences == [s for s in range(7) for _ in range(10)]
    assert sc.dices == [r[1] for r in a["res"]] * 7 and sc.dice_seq.tolist() == [sc.dice_seq[0]] * 7
    for f in range(10):
        assert torch.equal(res[f][0], a["res"][f][0]) and res[f][1] == a["res"][f][1] and res[f][2] == a["res"][f][2]
    assert stored.unmatched() == a["stray"]


def test_segmenter_ground_truth_refusals(endovis):
    e = endovis
    m, a = e["m"], e["seqs"][0]
    with pytest.raises(StswinHipError, match="endovis18"):
        video.VideoSegmenter(m, protocol="cadis", scores="deferred")          # (refused before the model is looked at)
    for kwargs in (dict(scores="later"), dict(gt_table=np.zeros((12, 3), np.uint8)), dict(gt_table=np.zeros(255, np.uint8)),
                   dict(gt_table=np.zeros((12, 4), np.int64)), dict(gt_table=np.zeros((257, 4), np.uint8))):
        with pytest.raises(StswinHipError):
            video.VideoSegmenter(m, **kwargs)
    plain = video.VideoSegmenter(m, out="labels", out_size=e["size"])
    with pytest.raises(StswinHipError):
        plain.endo_scores()
    with pytest.raises(StswinHipError):
        plain.unmatched()
    seg = video.VideoSegmenter(m, out="labels", out_size=e["size"], gt_table=e["table"])
    for bad in (a["gt"][:1], a["rgba"][:1, :, :, :2], a["rgba"][:1, :50], a["rgba"][:2], a["rgba"][:1].astype(np.int64)):
        with pytest.raises(StswinHipError):
            seg.push(a["fr"][0], gt=bad)
    ids = video.VideoSegmenter(m, out="labels", out_size=e["size"], gt_table=np.arange(256, dtype=np.uint8))
    with pytest.raises(StswinHipError):
        ids.push(a["fr"][0], gt=a["rgba"][:1])


@pytest.mark.parametrize("graph", [False, True])
def test_segmenter_cadis_raw_ids_give_the_host_remapped_matrix(graph):
    with np.load(GOLDEN) as z:
        mask, remapped = z["mask"], z["exp1/remapped"]
    pairs = dict(zip(mask.ravel().tolist(), remapped.ravel().tolist()))
    table = G.remap_table(pairs, ignore_to=8)
    m = _model("cadis", seed=4)
    n, size = 10, (45, 58)
    fr = _frames(n, 64, 64, seed=12)
    g = np.random.default_rng(5)
    raw = g.choice(np.array(sorted(pairs), dtype=np.uint8), size=(n, *size))
    host = torch.from_numpy(G.decode_ids(raw, table).astype(np.int64))
    assert int(host.max()) == 8 and (raw == 255).any()
    kw = dict(protocol="cadis", out="labels", out_size=size, graph=graph)
    with torch.no_grad():
        want_seg = video.VideoSegmenter(m, **kw)
        want = want_seg.segment_sequence(fr, gt=host)
        seg = video.VideoSegmenter(m, gt_table=table, **kw)
        got = []
        for f in range(n):                                   # online, one frame and its raw-id map per push
            got += [(i, r.clone()) for i, r in seg.push(fr[f], gt=raw[f])]
        got += [(i, r.clone()) for i, r in seg.finish()]
    got = [r for _, r in sorted(got, key=lambda ir: ir[0])]
    cm = want_seg.confusion_matrix()
    assert cm.shape == (8, 8) and cm.sum() > 0 and np.array_equal(seg.confusion_matrix(), cm)
    for f in range(n):
        assert torch.equal(got[f], want[f]), f
    assert seg.unmatched() == 0
