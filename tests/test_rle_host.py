"""utils.rle (the numpy definition of hip.rle_encode and the COCO / MOTS conversions) and the masks keyword of the report chain, on the
CPU: everything on integers, bit for bit."""
import numpy as np
import pytest
import torch

import rle_cases as RC
from stswincl_amd import hip
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I, rle as R
from stswincl_amd.video_report import ReportChain, Yield

MAPS = RC.small_maps()


@pytest.mark.parametrize("k", range(len(MAPS)))
def test_encode_is_the_plain_loop_and_decode_inverts_it(k):
    m = MAPS[k]
    H, W = m.shape
    runs, count = R.encode(m, 1024)
    want, n = RC.loop_encode(m, 1024)
    assert runs.dtype == count.dtype == np.int32 and runs.shape == (1, 1024, 2) and count.shape == (1,)
    assert int(count[0]) == n and np.array_equal(runs[0], want)
    assert runs[0, 0, 0] == 0 and not runs[0, n:].any()
    back = R.decode(runs[0], count[0], (H, W))
    assert back.shape == m.shape and np.array_equal(back, m.astype(np.int32))
    both, counts = R.encode(np.stack([m, m[::-1]]), 1024)                  # [n][H][W]: frame by frame
    assert np.array_equal(both[0], runs[0]) and counts[0] == count[0] and np.array_equal(both[1], RC.loop_encode(m[::-1], 1024)[0])


def test_a_run_continues_from_the_bottom_of_a_column_into_the_next():
    m = np.array([[0, 1, 1], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)        # columns 0 0 1 | 1 0 1 | 1 1 1
    runs, count = R.encode(m, 8)
    assert int(count[0]) == 4 and runs[0, :4].tolist() == [[0, 0], [2, 1], [4, 0], [5, 1]]
    m = np.array([[-1, -1], [-1, -1]], dtype=np.int32)
    runs, count = R.encode(m, 2)
    assert int(count[0]) == 1 and runs[0].tolist() == [[0, -1], [0, 0]]
    assert R.encode(np.array([[200, 255]], dtype=np.uint8), 2)[0][0].tolist() == [[0, 200], [1, 255]]     # zero-extended


@pytest.mark.parametrize("k", range(len(MAPS)))
def test_truncation_keeps_the_first_runs_and_the_full_count(k):
    m = MAPS[k]
    full, n = RC.loop_encode(m, m.size)
    for cap in sorted({1, max(1, n - 1), n, n + 1}):
        runs, count = R.encode(m, cap)
        assert int(count[0]) == n and np.array_equal(runs[0, :min(n, cap)], full[:min(n, cap)]) and not runs[0, n:].any()
        if cap < n:
            with pytest.raises(ValueError, match="runs"):
                R.decode(runs[0], count[0], m.shape)
            with pytest.raises(ValueError, match="runs"):
                R.mask_counts(runs[0], count[0], m.shape, (1,))
        else:
            assert np.array_equal(R.decode(runs[0], count[0], m.shape), m.astype(np.int32))


def test_encode_refusals():
    for bad in (np.zeros((2, 2), np.int64), np.zeros((2, 2), np.float32), np.zeros((0, 2), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            R.encode(bad, 4)
    for cap in (0, -1, (1 << 20) + 1, 2.5, 4.0, True, None, "4"):
        with pytest.raises(ValueError):
            R.encode(np.zeros((2, 2), np.uint8), cap)


@pytest.mark.parametrize("k", range(len(MAPS)))
def test_mask_counts_against_the_brute_force_rle_of_the_dense_mask(k):
    m = MAPS[k]
    runs, count = R.encode(m, m.size)
    present = np.unique(m).tolist()
    sets = [(v,) for v in present] + [tuple(present[:2]), tuple(present), (-7,), (present[0], 99)]
    for values in sets:
        got = R.mask_counts(runs[0], count[0], m.shape, values)
        assert got == RC.brute_counts(np.isin(m, values)), values
        assert sum(got) == m.size and np.array_equal(RC.counts_to_mask(got, *m.shape), np.isin(m, values))


VECTORS = [([5], "5"), ([3, 2, 40], "32X1"), ([3, 2, 40, 2], "32X10"), ([3, 2, 40, 1], "32X1O"), ([0, 1310720], "0PPPX1")]


@pytest.mark.parametrize("counts,string", VECTORS)
def test_the_compressed_string_s_vectors(counts, string):
    assert R.counts_to_string(counts) == string and R.string_to_counts(string) == counts


def test_the_compressed_string_round_trips():
    g = np.random.default_rng(5)
    cases = [[0], [0, 0, 0], [1 << 20, 3, (1 << 20) + 1, 1, 5], [7, 1 << 27, 2, 1, 1 << 27, (1 << 27) - 1], [31, 32, 15, 16, 1023, 1024, 0, 1]]
    cases += [g.integers(0, 1 << int(g.integers(1, 28)), int(g.integers(1, 40))).tolist() for _ in range(200)]
    cases += [[100, 5, 3, 90, 2, 1, 1, 1 << 21, 1]]                       # negative differences to the count two back
    for c in cases:
        s = R.counts_to_string(c)
        assert all(48 <= ord(ch) < 112 for ch in s) and R.string_to_counts(s) == c, c
    for bad in ("P", "0P", "\x00"):
        with pytest.raises(ValueError):
            R.string_to_counts(bad)


def test_against_pycocotools():
    M = pytest.importorskip("pycocotools.mask")
    for m in MAPS:
        runs, count = R.encode(m, m.size)
        for v in np.unique(m).tolist():
            mask = np.asfortranarray((m == v).astype(np.uint8))
            want = M.encode(mask)
            s = R.counts_to_string(R.mask_counts(runs[0], count[0], m.shape, (v,)))
            assert s.encode() == want["counts"] and list(want["size"]) == list(m.shape)
            assert np.array_equal(M.decode({"size": list(m.shape), "counts": s.encode()}), mask)


# ------------------------------------------------------------------------------------------------------------- MaskReport
def _two_frames():
    """A hand-built log of two 4 x 6 frames: their labels, 8-connected components and the host tracker's ids."""
    labels = np.zeros((2, 4, 6), dtype=np.uint8)
    labels[0, 0:2, 0:2] = 1
    labels[0, 2:4, 4:6] = 1
    labels[0, 0, 5] = 2
    labels[1, 0:2, 1:3] = 1            # the first blob moved a column; the second one and the class-2 pixel are gone
    labels[1, 3, 0] = 3
    comp, rows, total = I.label_components(labels, 4, 8, (0,), 4)
    t = I.InstanceTracker(4, 100, True, 1)
    got = [t.update(comp[f], rows[f], total[f]) for f in range(2)]
    return labels, comp.astype(np.int32), rows, total, np.stack([g[0] for g in got]), np.asarray([g[1] for g in got])


def test_mask_report_of_instances_with_tracks():
    labels, comp, rows, total, ids, started = _two_frames()
    runs, count = R.encode(comp, 32)
    inst = I.InstanceReport.from_rows(rows, total, (4, 6), frames=[0, 1], sequences=[0, 0])
    trk = I.TrackReport.from_ids(inst, ids, started)
    names = ["bg", "shaft", "wrist", "clasper"]
    rep = R.MaskReport(runs, count, (4, 6), "instances", [0, 1], [0, 0], tracks=trk, names=names)
    assert len(rep) == 2 and rep.size == (4, 6) and rep.source == "instances" and not rep.truncated.any() and rep.instances is inst
    for r in range(2):
        assert np.array_equal(rep.dense(r), comp[r])
        objs = rep.objects(r)
        assert [o["instance"] for o in objs] == list(range(int(total[r])))
        for o in objs:
            i = o["instance"]
            assert o["cls"] == int(rows[r, i, 0]) and o["name"] == names[o["cls"]] and o["track"] == int(ids[r, i]) and o["size"] == [4, 6]
            assert np.array_equal(RC.counts_to_mask(R.string_to_counts(o["counts"]), 4, 6), comp[r] == i)
    assert int(total[0]) == 3 and int(total[1]) == 2 and ids[0].tolist()[:3] == [0, 1, 2] and ids[1].tolist()[:2] == [0, 3]
    lines = rep.mots_lines(0)
    want = []
    for r in range(2):
        for o in rep.objects(r):
            want.append(f"{r} {o['cls'] * 1000 + o['track']} {o['cls']} 4 6 {o['counts']}")
    assert lines == want and len(lines) == 5 and lines[0].split()[:5] == ["0", "1000", "1", "4", "6"] and rep.mots_lines(1) == []
    # min_area drops the single pixels: the instance report decides who is present
    small = I.InstanceReport.from_rows(rows, total, (4, 6), min_area=2)
    assert [len(R.MaskReport(runs, count, (4, 6), "instances", instances=small).objects(r)) for r in range(2)] == [2, 1]
    # without reports: every ordinal of the map, class unknown
    bare = R.MaskReport(runs, count, (4, 6), "instances")
    assert [(o["instance"], o["cls"]) for o in bare.objects(0)] == [(0, None), (1, None), (2, None)] and "track" not in bare.objects(0)[0]
    with pytest.raises(ValueError, match="track"):
        bare.mots_lines(0)
    with pytest.raises(ValueError, match="track"):
        R.MaskReport(runs, count, (4, 6), "instances", instances=inst).mots_lines(0)


def test_mask_report_of_labels():
    labels = _two_frames()[0]
    runs, count = R.encode(labels, 32)
    rep = R.MaskReport(runs, count, (4, 6), "labels", [3, 4], [0, 1], skip=(0,), names=["bg", "shaft", "wrist", "clasper"])
    assert rep.frames == [3, 4] and rep.sequences == [0, 1]
    for r in range(2):
        assert np.array_equal(rep.dense(r), labels[r])
        objs = rep.objects(r)
        assert [o["cls"] for o in objs] == [c for c in np.unique(labels[r]).tolist() if c != 0] and "instance" not in objs[0]
        for o in objs:
            assert np.array_equal(RC.counts_to_mask(R.string_to_counts(o["counts"]), 4, 6), labels[r] == o["cls"])
    assert [o["name"] for o in rep.objects(0)] == ["shaft", "wrist"]
    assert [o["cls"] for o in R.MaskReport(runs, count, (4, 6), "labels", min_area=2, skip=(0,)).objects(0)] == [1]
    assert [o["cls"] for o in R.MaskReport(runs, count, (4, 6), "labels").objects(1)] == [0, 1, 3]


def test_mask_report_refusals():
    labels, comp, rows, total, ids, started = _two_frames()
    inst = I.InstanceReport.from_rows(rows, total, (4, 6))
    trk = I.TrackReport.from_ids(inst, ids, started)
    runs, count = R.encode(comp, 32)
    cut, n = R.encode(comp, int(count[1]))                                   # row 0 has more runs than row 1: truncated
    assert int(count[0]) > int(count[1]) and np.array_equal(n, count)
    rep = R.MaskReport(cut, n, (4, 6), "instances", tracks=trk)
    assert rep.truncated.tolist() == [True, False] and len(rep.objects(1)) == 2
    for call in (lambda: rep.objects(0), lambda: rep.dense(0), lambda: rep.mots_lines(0)):
        with pytest.raises(ValueError, match="runs"):
            call()
    far = I.TrackReport.from_ids(inst, np.where(ids >= 0, ids + 999, -1), started + 999)
    with pytest.raises(ValueError, match="1000"):
        R.MaskReport(runs, count, (4, 6), "instances", tracks=far).mots_lines(0)
    for bad in (dict(source="classes"), dict(frames=[0]), dict(sequences=[0, 0, 0]), dict(source="labels", instances=inst), dict(min_area=0), dict(min_area=None),
                dict(min_area="2")):
        with pytest.raises(ValueError):
            R.MaskReport(runs, count, (4, 6), **{"source": "instances", **bad})
    with pytest.raises(ValueError):
        R.MaskReport(runs[0, :, 0], count, (4, 6))
    with pytest.raises(ValueError):
        R.MaskReport(runs, count, (4, 6), "instances", instances=I.InstanceReport.from_rows(rows[:1], total[:1], (4, 6)))


# ------------------------------------------------------------------------------------------------------------- the chain
def _chain(**kw):
    args = dict(report=None, min_area=1, instances=None, connectivity=8, instance_skip=None, tracks=False, track_iou=100, track_same_class=True)
    out = kw.pop("out", "labels")
    extra = {k: kw.pop(k) for k in ("masks", "mask_runs") if k in kw}
    args.update(kw)
    return ReportChain("cpu", 12, "endovis18", out, *args.values(), **extra)


def test_report_chain_keyword_refusals():
    for kw in (dict(masks="always"), dict(masks=True), dict(masks="frame", out="logits"), dict(masks="deferred", out="logits"),
               dict(mask_runs=8), dict(masks="frame", mask_runs=0), dict(masks="frame", mask_runs=(1 << 20) + 1),
               dict(masks="deferred", mask_runs=64.0), dict(masks="frame", mask_runs=True)):
        with pytest.raises(StswinHipError, match="mask"):
            _chain(**kw)
    c = _chain(masks="frame")                                               # masks needs no report
    assert c.masks == "frame" and c.mask_runs == 16384 and c.report is None and "runs" not in c.log.columns
    c = _chain(masks="deferred", mask_runs=1 << 20, out="overlay")
    assert c.log.columns["runs"] == ((1 << 20, 2), torch.int32) and c.log.columns["count"] == ((), torch.int32)
    assert _chain().masks is None and "runs" not in _chain(report="deferred").log.columns


def test_device_log_rows_of_the_masks_group():
    labels = _two_frames()[0]
    runs, count = (torch.from_numpy(t) for t in R.encode(labels, 16))
    ys = [Yield(runs=runs[f:f + 1], count=count[f:f + 1]) for f in range(2)]
    # masks="frame": the pair is appended behind the result, nothing is logged
    c = _chain(masks="frame", mask_runs=16)
    res = c.released([0, 1], ["a", ("b", 1.0)], ys)
    assert res[0][0] == "a" and len(res[0]) == 3 and res[1][:2] == ("b", 1.0) and len(res[1]) == 4 and not c.log.keys
    assert torch.equal(res[0][1], runs[0]) and torch.equal(res[1][3], count[1]) and res[1][3].dim() == 0
    # masks="deferred": results unchanged, a row per frame, in (sequence, frame) order at download
    c = _chain(masks="deferred", mask_runs=16)
    assert c.released([1], ["x"], ys[1:]) == ["x"] and c.released([0], ["y"], ys[:1]) == ["y"]
    c.reset()
    c.released([0], ["z"], ys[1:])
    cols, sequences, frames = c.log.download("runs", "count")
    assert sequences == [0, 0, 1] and frames == [0, 1, 0]
    assert np.array_equal(cols["runs"], runs[[0, 1, 1]].numpy()) and np.array_equal(cols["count"], count[[0, 1, 1]].numpy())
    assert list(c.log.columns) == ["runs", "count"]                          # (report=None: the log has no columns for it)
    # report="deferred" beside masks="frame": the report's row is logged, the runs are appended
    c = _chain(report="deferred", masks="frame", mask_runs=16)
    y = ys[0]._replace(moments=torch.ones(1, 12, 10, dtype=torch.int64))
    res = c.released([5], ["r"], [y])
    assert len(res[0]) == 3 and torch.equal(res[0][1], runs[0]) and c.log.keys == [(0, 5)] and bool(c.log.data["moments"][0].all())
    # and the other way round
    c = _chain(report="frame", masks="deferred", mask_runs=16)
    res = c.released([5], ["r"], [y])
    assert len(res[0]) == 2 and torch.equal(res[0][1], y.moments[0]) and torch.equal(c.log.data["runs"][0], runs[0])
    assert list(c.log.columns) == ["runs", "count"]


def test_yield_carries_runs_and_count_per_clip():
    y = Yield(moments=torch.zeros(3, 2, 10), runs=torch.arange(24).view(3, 4, 2), count=torch.tensor([4, 1, 2]))
    b = y.clip(1)
    assert b.rows is None and tuple(b.runs.shape) == (1, 4, 2) and int(b.count[0]) == 1 and torch.equal(b.runs[0], y.runs[1])
    assert len(b.appended("r")) == 2 and len(b.appended("r", True, True)) == 4 and len(b.appended(("r", 1), False, True)) == 4


def test_the_abi_declares_the_encoder():
    for s in ("stswin_rle_encode", "stswin_rle_encode_scratch", "stswin_rle_geometry"):
        assert s in hip.declared_symbols()
    lib = hip.load()
    assert lib.stswin_abi_version() == 1 and hasattr(lib, "stswin_rle_encode")
    SH, TW, V = hip.rle_geometry()
    assert SH >= 1 and TW % V == 0 and lib.stswin_rle_geometry(3) == -1
    assert hip.rle_encode_scratch(2, SH + 1, 7) == 4 * 2 * 7 * 2 and lib.stswin_rle_encode_scratch(1, 16385, 1) == -1850
    with pytest.raises(StswinHipError):
        hip.rle_encode_scratch(0, 4, 4)
    with pytest.raises(StswinHipError, match="GPU"):
        hip.rle_encode(torch.zeros(1, 4, 4, dtype=torch.uint8), 8)


@pytest.mark.parametrize("H", [33, 34, 67, 70])
def test_the_horizontal_stripes_change_around_the_segment_edges(H):
    SH = 32                                                                  # (any segment height: the pattern is built around it)
    for dtype in (np.uint8, np.int32):
        m = RC.patterns(2, H, 11, dtype, SH)["hstripes"]
        changes = (np.nonzero((m[:, 1:] != m[:, :-1]).all(axis=(0, 2)))[0] + 1).tolist()
        assert changes == RC.hstripe_edges(H, SH) and {SH - 1, SH} <= set(changes) and (SH + 1 in changes or H == SH + 1)
        assert H < 2 * SH + 2 or {2 * SH - 1, 2 * SH, 2 * SH + 1} <= set(changes)
