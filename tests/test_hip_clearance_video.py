"""VideoSegmenter(clearance=...): the tensor a result carries, or the log holds, is utils.instruments.instance_clearance of the labels
the same segmenter returns and of the host components of those labels (grouped where instance_groups is given).  Exact integers."""
import numpy as np
import pytest
import torch

import test_hip_clean_video as CV
import test_hip_components as C
import test_hip_parts as P
import test_hip_tracks as T
from stswincl_amd import video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I

pytestmark = pytest.mark.gpu

SIZE, N, K = C.SIZE, C.N, C.K
_MODES = {"eager": {}, "batch4": dict(batch=4), "graph": dict(graph=True)}
_WANT = {}


def _want(labels, c, groups=(), targets=None, max_distance=None):
    """The definition on a result's own labels uint8 [H][W] (device) and the host components of them; computed once per map."""
    lab = labels.cpu().numpy()
    key = (lab.tobytes(), c["nc"], groups, targets, max_distance)
    if key not in _WANT:
        comp = I.label_components(I.group_table(groups, c["nc"])[lab][None], c["nc"], 8, c["skip"], K)[0]
        _WANT[key] = I.instance_clearance(lab[None], comp, K, c["nc"], targets, max_distance)[0]
    return _WANT[key]


def _own(r, c, groups=(), targets=None, max_distance=None):
    """The last element of a clearance="frame" result is the definition of the result's own labels."""
    cl = r[-1]
    ok = cl.is_cuda and cl.dtype == torch.int64 and tuple(cl.shape) == (K, c["nc"], 3)
    return ok and np.array_equal(cl.cpu().numpy(), _want(r[0], c, groups, targets, max_distance))


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_frame_clearance_equals_the_definition_in_every_mode(protocol, grouped):
    c = T._case(protocol)
    s = c["seqs"][0]
    groups = P._groups(protocol) if grouped else ()
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, **(dict(instance_groups=groups) if grouped else {}))
    with torch.no_grad():
        was = video.VideoSegmenter(c["m"], **kw).segment_sequence(s["fr"])
        runs = {}
        for mode, mkw in _MODES.items():
            seg = video.VideoSegmenter(c["m"], clearance="frame", **kw, **mkw)
            runs[mode] = seg.segment_sequence(s["fr"])
            assert mode != "graph" or seg.captured
    measured = 0
    for f in range(N):
        e = runs["eager"][f]
        assert len(was[f]) == 4 and len(e) == 5 and all(torch.equal(a, b) for a, b in zip(e[:4], was[f])), f     # what was there is what it was
        assert torch.equal(e[0].cpu(), s["labels"][f]) and _own(e, c, groups), f
        for mode in ("batch4", "graph"):
            assert len(runs[mode][f]) == 5 and all(torch.equal(a, b) for a, b in zip(e, runs[mode][f])), (mode, f)
        measured += int((e[4][..., 0] > 0).sum())
        present = e[2][:, 2] > 0                                              # an instance of the rows is measured to something, or alone
        assert bool((~(e[4][..., 0] >= 0).any(dim=1) | present).all()), f
    assert measured > 0


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_deferred_clearance_joins_the_tracks(mode):
    protocol = "endovis18"
    c = T._case(protocol)
    a, b = c["seqs"]
    groups = P._groups(protocol)
    names = [f"class {k}" for k in range(c["nc"])]
    to, far = tuple(k for k in range(c["nc"]) if k not in groups[0]), 30
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, instances=K, tracks=True, instance_groups=groups, clearance_to=to, clearance_max=far)
    with torch.no_grad():
        frame = video.VideoSegmenter(c["m"], report="frame", clearance="frame", parts="frame", **kw)
        want = [frame.segment_sequence(q["fr"]) for q in (a, b)]
        seg = video.VideoSegmenter(c["m"], report="deferred", clearance="deferred", **kw, **_MODES[mode])
        assert len(seg.clearance_report()) == 0
        for f in range(N):                                                   # pushed frame by frame: some wait, parked, for the tracker
            for g, r in seg.push(a["fr"][f]):
                assert isinstance(r, torch.Tensor)                           # the results are unchanged
        seg.finish()
        seg.reset()
        got_b = seg.segment_sequence(b["fr"])
    assert all(torch.equal(r.cpu(), b["labels"][f]) for f, r in enumerate(got_b))
    rep = seg.clearance_report(names=names)
    inst, trk = seg.instance_report(names), seg.track_report(names)
    assert rep.sequences == inst.sequences == [0] * N + [1] * N and rep.frames == inst.frames == list(range(N)) * 2
    assert rep.names == names and rep.size == SIZE and (seg.clearance, seg.clearance_to, seg.clearance_max) == ("deferred", to, far)
    for n, res in enumerate(want):
        for f, r in enumerate(res):
            row = n * N + f
            assert len(r) == 8 and _own(r, c, groups, to, far), (n, f)       # (labels, moments, rows, total, ids, parts, contacts, clearance)
            assert np.array_equal(rep.clearance[row], r[-1].cpu().numpy()), (n, f)
            assert np.array_equal(rep.instances.rows[row], r[2].cpu().numpy()) and np.array_equal(rep.tracks.ids[row], r[4].cpu().numpy()), (n, f)
    assert (rep.d2[:, :, list(groups[0])] == -1).all() and int(rep.d2.max()) <= far * far and int(rep.measured.sum()) > 0
    rows = rep.as_rows()
    assert len(rows) == int(inst.present.sum()) and [r["track"] for r in rows] == [r["track"] for r in trk.as_rows()]
    one = next(r for r in rows if r["distance"])
    cls, dist = sorted(one["distance"].items())[0]
    r0 = [k for k in range(2 * N) if (rep.sequences[k], rep.frames[k]) == (one["sequence"], one["frame"])][0]
    (py, px), (qy, qx) = rep.nearest(r0, one["instance"], cls)
    assert round(dist * dist) == (py - qy) ** 2 + (px - qx) ** 2 and 0 < dist <= far
    seg.reset_metrics()
    assert len(seg.clearance_report()) == 0 and len(seg.instance_report()) == 0


@pytest.mark.parametrize("mode", ["eager", "batch4", "graph"])
def test_clearance_reads_the_cleaned_map(mode):
    protocol = "endovis18"
    c, ref = T._case(protocol), CV._ref(protocol)
    q = c["seqs"][0]
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, clean_area=ref["area"], clean_keep=CV.KEEP, report="frame", instances=K)
    with torch.no_grad():
        got = video.VideoSegmenter(c["m"], clearance="frame", **kw, **_MODES[mode]).segment_sequence(q["fr"])
    for f, r in enumerate(got):
        assert len(r) == 5 and np.array_equal(r[0].cpu().numpy(), ref["labels"][0][f]) and _own(r, c), f


def test_clearance_with_ground_truth_is_made_after_the_replay():
    for protocol in ("endovis18", "cadis"):
        c = T._case(protocol)
        s = c["seqs"][0]
        kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, tracks=True, clearance="frame")
        with torch.no_grad():
            seg = video.VideoSegmenter(c["m"], graph=True, **kw)
            free = seg.segment_sequence(s["fr"])
            assert seg.captured
            scored = seg.segment_sequence(s["fr"], gt=s["gt"])
            more = dict(scores="deferred") if protocol == "endovis18" else {}
            eager = video.VideoSegmenter(c["m"], batch=4, **more, **kw).segment_sequence(s["fr"], gt=s["gt"])
        for f in range(N):
            a, b, d = free[f], scored[f], eager[f]
            assert len(a) == 6 and len(d) == 6 and len(b) == (8 if protocol == "endovis18" else 6), (protocol, f)
            assert torch.equal(b[0].cpu(), s["labels"][f]) and _own(b, c), (protocol, f)
            assert torch.equal(a[-1], b[-1]) and torch.equal(a[-2], b[-2]) and all(torch.equal(x, y) for x, y in zip(a, d)), (protocol, f)


def test_keywords_and_refusals():
    c = C._case("endovis18")
    m = c["m"]
    base = dict(out="labels", out_size=SIZE, report="frame")
    for kwargs, what in ((dict(clearance="frame", **base), "instances"), (dict(clearance="deferred", **base), "instances"),
                         (dict(clearance_to=(1,), instances=4, **base), "clearance_to"), (dict(clearance_max=9, instances=4, **base), "clearance_max"),
                         (dict(out="logits", clearance="frame"), "clearance"), (dict(clearance="always", instances=4, **base), "clearance"),
                         (dict(clearance=True, instances=4, **base), "clearance"),
                         (dict(clearance="frame", clearance_to=(c["nc"],), instances=4, **base), "clearance_to"),
                         (dict(clearance="frame", clearance_to=(1.0,), instances=4, **base), "clearance_to"),
                         (dict(clearance="frame", clearance_max=-1, instances=4, **base), "clearance_max"),
                         (dict(clearance="frame", clearance_max=9.0, instances=4, **base), "clearance_max")):
        with pytest.raises(StswinHipError, match=what):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(instances=4, **base), dict(instances=4, clearance="frame", **base)):
        with pytest.raises(StswinHipError, match="clearance_report"):
            video.VideoSegmenter(m, **kwargs).clearance_report()
    q = c["seqs"][0]
    with torch.no_grad():                                                    # without the keyword, spelled or not: results of unchanged shape
        plain = video.VideoSegmenter(m, instances=K, **base).segment_sequence(q["fr"])
        spelled = video.VideoSegmenter(m, instances=K, clearance=None, clearance_to=None, clearance_max=None, **base)
        got = spelled.segment_sequence(q["fr"])
    assert spelled.clearance is None and spelled.chain.clr_ws is None and "clearance" not in spelled.chain.log.columns
    for f, (x, y) in enumerate(zip(plain, got)):
        assert len(x) == len(y) == 4 and all(torch.equal(u, v) for u, v in zip(x, y)), f
        assert torch.equal(x[0].cpu(), q["labels"][f]) and torch.equal(x[1].cpu(), q["moments"][f])
    seg = video.VideoSegmenter(m, out="overlay", report="deferred", instances=4, clearance="deferred", clearance_to=[3, 1], clearance_max=0)
    assert (seg.clearance, seg.clearance_to, seg.clearance_max) == ("deferred", (3, 1), 0)
