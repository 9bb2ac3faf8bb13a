"""VideoSegmenter(clean_area=A): the labels are the cleaned labels everywhere.  The reference is utils.instruments.clean_labels of the
labels a segmenter without the keyword returns (the shared cases of the other video tests); integers are compared exactly."""
import numpy as np
import pytest
import torch

import test_hip_components as C
import test_hip_tracks as T
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import EndoMetric as E, boundary as B, instruments as I

pytestmark = pytest.mark.gpu

SIZE, N, K = C.SIZE, C.N, 16
KEEP = (7,)
_REF = {}


def _ref(protocol):
    """Per protocol: clean_area, chosen on the reference as the smallest of a fixed ladder at which the definition changes pixels of the
    case's plain labels (a random model's map may have no specks: then whole small regions qualify), and per sequence the cleaned
    labels and stats of the definition.  Computed once, shared, never changed."""
    if protocol not in _REF:
        c = T._case(protocol)
        for area in (16, 64, 256, 1024, 3000):
            seqs = [I.clean_labels(s["labels"].numpy(), c["nc"], area, 8, KEEP) for s in c["seqs"]]
            if all(st[:, 1].sum() > 0 for _, st in seqs):
                break
        else:
            raise AssertionError("no clean_area of the ladder changes a pixel of both sequences: another seed")
        _REF[protocol] = dict(area=area, labels=[l for l, _ in seqs], stats=[st for _, st in seqs])
    return _REF[protocol]


def _kw(protocol, **more):
    return dict(out="labels", out_size=SIZE, protocol=protocol, clean_area=_ref(protocol)["area"], clean_keep=KEEP, **more)


@pytest.mark.parametrize("mode", ["eager", "batch2"])
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_labels_are_the_cleaned_labels_and_the_report_holds_the_stats(protocol, mode):
    c, ref = T._case(protocol), _ref(protocol)
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], **_kw(protocol), **({"batch": 2} if mode == "batch2" else {}))
        assert len(seg.clean_report()) == 0
        for s, q in enumerate(c["seqs"]):
            got = seg.segment_sequence(q["fr"])
            assert len(got) == N
            for f, r in enumerate(got):
                assert r.dtype == torch.uint8 and np.array_equal(r.cpu().numpy(), ref["labels"][s][f]), (s, f)
    assert any(int(st[:, 1].max()) > 0 for st in ref["stats"])
    rep = seg.clean_report()
    assert len(rep) == 2 * N and rep.sequences == [0] * N + [1] * N and rep.frames == list(range(N)) * 2
    want = np.concatenate(ref["stats"])
    assert np.array_equal(rep.small, want[:, 0]) and np.array_equal(rep.changed, want[:, 1])
    assert [r["changed"] for r in rep.as_rows()] == want[:, 1].tolist()
    seg.reset()                                                              # reset() keeps the log, reset_metrics() clears it
    assert len(seg.clean_report()) == 2 * N
    seg.reset_metrics()
    assert len(seg.clean_report()) == 0


def test_the_chain_reads_the_cleaned_labels():
    protocol = "endovis18"
    c, ref = T._case(protocol), _ref(protocol)
    q, nc = c["seqs"][0], c["nc"]
    kw = dict(protocol=protocol, clean_area=ref["area"], clean_keep=KEEP, report="frame", instances=K)
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="overlay", masks="frame", confidence="frame", parts="frame", **kw)
        got = seg.segment_sequence(q["fr"])
        logits = video.VideoSegmenter(c["m"], out="logits", protocol=protocol).segment_sequence(q["fr"])
        tracked = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, tracks=True, **kw).segment_sequence(q["fr"])
    assert seg.out_size == SIZE
    for f, r in enumerate(got):
        assert len(r) == 11
        lab = torch.from_numpy(ref["labels"][0][f:f + 1]).cuda()
        frame = torch.from_numpy(q["fr"][f:f + 1]).cuda()
        comp, rows, total = hip.label_components(lab, nc, 8, c["skip"], K)
        conf = hip.upsample_confidence(logits[f][None].contiguous(), lab, True)
        want = (hip.labels_overlay(lab, seg._table, frame, seg.edge_alpha)[0], hip.label_moments(lab, nc)[0], rows[0], total[0],
                *(t[0] for t in hip.rle_encode(comp, 16384)), conf[0], hip.confidence_sums(lab, conf, nc, 128)[0],
                hip.confidence_sums(comp, conf, K, 128)[0], *(t[0] for t in hip.instance_parts(lab, comp, K, nc)))
        for k, (a, b) in enumerate(zip(r, want)):
            assert a.shape == b.shape and torch.equal(a, b), (f, k)
    comp, rows, total = I.label_components(ref["labels"][0], nc, 8, c["skip"], K)
    tracker = I.InstanceTracker(K, 100, True, 1)
    for f, r in enumerate(tracked):                                          # (labels, moments, rows, total, ids): the tracker in frame order
        assert len(r) == 5 and np.array_equal(r[0].cpu().numpy(), ref["labels"][0][f])
        want_ids = tracker.update(comp[f], rows[f], total[f])[0]
        assert np.array_equal(r[4].cpu().numpy(), want_ids), f


def test_graph_replay_equals_eager():
    protocol = "endovis18"
    c, ref = T._case(protocol), _ref(protocol)
    assert N >= video.min_frames(protocol) + 3
    kw = _kw(protocol, report="frame", instances=K, confidence="frame")
    with torch.no_grad():
        eager = video.VideoSegmenter(c["m"], **kw)
        graph = video.VideoSegmenter(c["m"], graph=True, **kw)
        for s, q in enumerate(c["seqs"]):                                    # segment_sequence resets: the second sequence replays too
            a, b = eager.segment_sequence(q["fr"]), graph.segment_sequence(q["fr"])
            assert graph.captured and len(a) == len(b) == N
            for f, (x, y) in enumerate(zip(a, b)):
                assert len(x) == len(y) == 7 and all(torch.equal(u, v) for u, v in zip(x, y)), (s, f)
                assert np.array_equal(y[0].cpu().numpy(), ref["labels"][s][f]), (s, f)
        live = []                                                            # pushed frame by frame: the last replayed step's labels are
        for f in range(N):                                                   # a view of the graph's buffer, cloned here
            live += [(g, r[0].clone()) for g, r in graph.push(q["fr"][f])]
        live += [(g, r[0].clone()) for g, r in graph.finish()]
    assert all(np.array_equal(r.cpu().numpy(), ref["labels"][1][g]) for g, r in live) and len(live) == N
    a, b = eager.clean_report(), graph.clean_report()
    assert a.sequences == b.sequences[:2 * N] and np.array_equal(a.small, b.small[:2 * N]) and np.array_equal(a.changed, b.changed[:2 * N])
    assert np.array_equal(b.changed[2 * N:], ref["stats"][1][:, 1]) and b.sequences[2 * N:] == [2] * N


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_endovis18_scores_are_those_of_the_cleaned_labels(mode):
    protocol = "endovis18"
    c, ref = T._case(protocol), _ref(protocol)
    more = dict(graph=True) if mode == "graph" else {}
    with torch.no_grad():
        frame = video.VideoSegmenter(c["m"], boundary="deferred", **_kw(protocol), **more)
        later = video.VideoSegmenter(c["m"], scores="deferred", **_kw(protocol), **more)
        got, plain = [], []
        for q in c["seqs"]:
            got += frame.segment_sequence(q["fr"], gt=q["gt"])
            plain += later.segment_sequence(q["fr"], gt=q["gt"])
    labels = np.concatenate(ref["labels"])
    gts = np.concatenate([q["gt"].numpy() for q in c["seqs"]])
    res = later.endo_scores()
    assert res.count == 2 * N and res.sequences == [0] * N + [1] * N
    some = 0
    for k, (r, p) in enumerate(zip(got, plain)):
        assert len(r) == 3 and np.array_equal(r[0].cpu().numpy(), labels[k]) and np.array_equal(p.cpu().numpy(), labels[k]), k
        rd, rj = E.general_dice(gts[k], labels[k]), E.general_jaccard(gts[k], labels[k])
        for mine in ((r[1], r[2]), (res.dices[k], res.ious[k])):
            assert [cl for cl, _ in rd] == [cl for cl, _ in mine[0]] == [cl for cl, _ in mine[1]], k
            assert np.allclose([v for _, v in rd], [v for _, v in mine[0]], rtol=1e-12, atol=0)
            assert np.allclose([v for _, v in rj], [v for _, v in mine[1]], rtol=1e-12, atol=0)
        some += sum(v > 0 for _, v in rd)
    assert some > 0
    want = B.boundary_counts(gts, labels, c["nc"], 32, (0,))
    bs = frame.boundary_scores()
    assert bs.sequences == [0] * N + [1] * N and np.array_equal(bs.counts, want)
    assert np.array_equal(frame.clean_report().changed, np.concatenate(ref["stats"])[:, 1])


def test_cadis_confusion_matrix_is_that_of_the_cleaned_labels():
    protocol = "cadis"
    c, ref = T._case(protocol), _ref(protocol)
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], boundary="deferred", **_kw(protocol))
        got = []
        for q in c["seqs"]:
            got += seg.segment_sequence(q["fr"], gt=q["gt"])
    labels = np.concatenate(ref["labels"])
    gts = np.concatenate([q["gt"].numpy() for q in c["seqs"]])
    assert all(np.array_equal(r.cpu().numpy(), labels[k]) for k, r in enumerate(got))
    ncm = c["nc"] - 1
    assert seg.metric_classes == ncm
    ok = (gts >= 0) & (gts < ncm) & (labels < ncm)
    want = np.bincount(gts[ok] * ncm + labels[ok].astype(np.int64), minlength=ncm * ncm).reshape(ncm, ncm)
    assert np.array_equal(seg.confusion_matrix(), want.astype(np.float64)) and want.sum() > 0
    assert np.array_equal(seg.boundary_scores().counts, B.boundary_counts(gts, labels, c["nc"], 32, (c["nc"] - 1,)))


def test_keyword_validation():
    c = C._case("endovis18")
    m = c["m"]
    base = dict(out="labels", out_size=SIZE)
    for kw in (dict(clean_keep=(1,)), dict(clean_connectivity=4), dict(clean_max=16), dict(clean_area=1), dict(clean_area=(1 << 30) + 1),
               dict(clean_area=9.0), dict(clean_area=True), dict(clean_area=9, clean_keep=(64,)), dict(clean_area=9, clean_keep=(1.5,)),
               dict(clean_area=9, clean_connectivity=6), dict(clean_area=9, clean_max=0), dict(clean_area=9, clean_max=65537),
               dict(clean_area=9, out="logits", out_size=None)):
        with pytest.raises(StswinHipError, match="clean_"):
            video.VideoSegmenter(m, **{**base, **kw})
    with pytest.raises(StswinHipError, match="clean_"):
        video.VideoSegmenter(T._case("cadis")["m"], out="logits", protocol="cadis", clean_area=9)
    q = c["seqs"][0]
    with torch.no_grad():
        plain = video.VideoSegmenter(m, report="frame", **base)
        spelled = video.VideoSegmenter(m, report="frame", clean_area=None, clean_keep=None, clean_connectivity=8, clean_max=4096, **base)
        with pytest.raises(StswinHipError, match="clean_report"):
            plain.clean_report()
        a, b = plain.segment_sequence(q["fr"]), spelled.segment_sequence(q["fr"])
    assert spelled.cleaner is None and spelled.clean_area is None
    for f, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y) == 2 and torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        assert torch.equal(x[0].cpu(), q["labels"][f]) and torch.equal(x[1].cpu(), q["moments"][f])
    seg = video.VideoSegmenter(m, clean_area=9, clean_keep=3, clean_connectivity=4, clean_max=16, **base)
    assert (seg.clean_area, seg.clean_keep, seg.clean_connectivity, seg.clean_max) == (9, (3,), 4, 16)
