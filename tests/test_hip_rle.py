"""hip.rle_encode (run-length masks of label and component maps) and VideoSegmenter(masks=...) against the numpy definition
utils.rle.encode: everything torch.equal, the zero tail and the full count of a truncated frame included.  The shapes are placed
around the kernel's geometry (stswin_rle_geometry)."""
import numpy as np
import pytest
import torch

import rle_cases as RC
import test_hip_components as C
import test_hip_tracks as T
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I, rle as R

pytestmark = pytest.mark.gpu

SH, TW, V = hip.rle_geometry()
SHAPES = [(1, 1, 1), (2, 1, TW + 1), (1, SH + 1, 1), (2, SH + 1, TW + 1), (3, 2 * SH + 3, 3 * TW + 5), (1, 3, V + 1),
          (2, SH + 2, 2 * TW)]            # the last one: W % 16 == 0 on an aligned pointer, the 16-byte body; the others the element body
DTYPES = [np.uint8, np.int32]


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


def _check(maps, cap, offset=0):
    """One call on `maps` (numpy [n][H][W]) placed `offset` bytes off a 512-byte boundary, outputs between sentinels: equal to the
    definition in full, the input untouched, a second call the same bits."""
    host = np.ascontiguousarray(maps)
    n = host.shape[0]
    dev, dev_buf = _padded(host.shape, torch.from_numpy(host).dtype, offset)
    dev.copy_(torch.from_numpy(host))
    assert dev.data_ptr() % 16 == offset % 16
    runs, runs_buf = _padded((n, cap, 2), torch.int32)
    count, count_buf = _padded((n,), torch.int32)
    got = hip.rle_encode(dev, cap, out=(runs, count))
    assert got[0] is runs and got[1] is count
    want_runs, want_count = R.encode(host, cap)
    assert torch.equal(count.cpu(), torch.from_numpy(want_count)), (count.cpu().tolist(), want_count.tolist())
    bad = (runs.cpu() != torch.from_numpy(want_runs)).nonzero()
    assert bad.numel() == 0, bad[:8].tolist()
    assert _sentinels_hold(runs, runs_buf) and _sentinels_hold(count, count_buf) and _sentinels_hold(dev, dev_buf)
    assert torch.equal(dev.cpu(), torch.from_numpy(host)), "the input changed"
    again = hip.rle_encode(dev, cap)                                       # fresh buffers, the wrapper's own workspace
    assert again[0].dtype == torch.int32 and tuple(again[0].shape) == (n, cap, 2) and tuple(again[1].shape) == (n,)
    assert torch.equal(again[0], runs) and torch.equal(again[1], count)
    return want_count


def test_geometry_is_the_library_s():
    geo = hip.load().stswin_rle_geometry
    assert (geo(0), geo(1), geo(2)) == (SH, TW, V) and geo(3) == -1 and geo(-1) == -1
    assert V == 16 and TW % 16 == 0 and SHAPES[-1][2] % 16 == 0 and all(s[2] % 4 for s in SHAPES[:-1] if s[2] > 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_pattern(shape, dtype):
    n, H, W = shape
    for name, maps in RC.patterns(n, H, W, dtype, SH).items():
        R_all = R.encode(maps, 1)[1]
        cap = int(R_all.max()) + 3                                         # every run and a zero tail
        counts = _check(maps, cap)
        if name == "constant":
            assert counts.tolist() == [1] * n
        if name == "checkerboard":
            assert counts.tolist() == [H * W] * n                          # (H W odd or even: neighbours in p always differ)
            if H * W > 2:
                _check(maps, H * W // 2)                                   # cap < R: the first cap runs, count stays full
                _check(maps, 1)
        if name == "mixed":
            assert len(set(counts.tolist())) == n
        if name == "vstripes" and H > 1 and W > 4:
            v = maps[0].T.ravel()
            carried = sum(int(v[x * H - 1] == v[x * H]) for x in range(1, W))
            assert 0 < carried < W - 1, "no run is carried from a column's bottom into the next one's top"
        if name == "hstripes":                                             # every column changes at, before and after the segment edges
            changes = (np.nonzero((maps[:, 1:] != maps[:, :-1]).all(axis=(0, 2)))[0] + 1).tolist()
            assert changes == RC.hstripe_edges(H, SH)
            assert all(e in changes for e in (SH - 1, SH, SH + 1, 2 * SH - 1, 2 * SH, 2 * SH + 1) if e < H), changes
        if cap > 4:
            _check(maps, cap - 4)                                         # R - 1: truncation by one run


def test_values_and_carries_of_the_patterns():
    big = RC.patterns(1, 40, 40, np.int32, SH)
    assert int(big["big"].max()) >= 1 << 20 and int(big["big"].min()) == -1 and int(big["vstripes"].max()) >= 1 << 20
    assert int(RC.patterns(1, 40, 40, np.uint8, SH)["blobs"].max()) == 255


@pytest.mark.parametrize("dtype,offset", [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.int32, 4), (np.int32, 8), (np.int32, 12)])
def test_maps_off_a_16_byte_boundary(dtype, offset):
    n, H, W = SHAPES[-1]
    maps = RC.patterns(n, H, W, dtype, SH, seed=offset)
    for name in ("blobs", "vstripes", "hstripes"):
        _check(maps[name], int(R.encode(maps[name], 1)[1].max()) + 1, offset)
    _check(maps["blobs"], int(R.encode(maps["blobs"], 1)[1].max()) + 1, 0)      # ... and on it: the same map through the 16-byte body


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_and_workspace_buffers_are_reused(dtype):
    n, H, W = 3, 2 * SH + 3, TW + 16
    cap = 600
    out = (torch.full((n, cap, 2), 77, dtype=torch.int32, device="cuda"), torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    ws = torch.full((hip.rle_encode_scratch(n, H, W) + 64,), 77, dtype=torch.uint8, device="cuda")
    assert hip.rle_encode_scratch(n, H, W) == 4 * n * W * 3
    for name, maps in RC.patterns(n, H, W, dtype, SH, seed=9).items():     # long lists, then short ones over them: the tail is cleared
        got = hip.rle_encode(torch.from_numpy(maps).cuda(), cap, out=out, workspace=ws)
        want = R.encode(maps, cap)
        assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1])), name
        assert bool((ws[-64:] == 77).all())
        ws[:-64].fill_(int(want[1][0]) % 251)                              # whatever the workspace holds: nothing in it survives


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_call_is_capturable(dtype):
    n, H, W = 2, SH + 5, TW + 32
    cap = 512
    pats = RC.patterns(n, H, W, dtype, SH, seed=4)
    maps = torch.empty(n, H, W, dtype=torch.from_numpy(pats["blobs"]).dtype, device="cuda")
    out = (torch.full((n, cap, 2), 77, dtype=torch.int32, device="cuda"), torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    ws = torch.empty(hip.rle_encode_scratch(n, H, W), dtype=torch.uint8, device="cuda")
    maps.copy_(torch.from_numpy(pats["blobs"]))
    hip.rle_encode(maps, cap, out=out, workspace=ws)                        # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.rle_encode(maps, cap, out=out, workspace=ws)
    for name in ("checkerboard", "constant", "blobs", "hstripes", "mixed"):
        maps.copy_(torch.from_numpy(pats[name]))
        graph.replay()
        want = R.encode(pats[name], cap)
        assert torch.equal(out[0].cpu(), torch.from_numpy(want[0])) and torch.equal(out[1].cpu(), torch.from_numpy(want[1])), name


def _buffers(n, H, W, cap):
    out = (torch.full((n, cap, 2), 77, dtype=torch.int32, device="cuda"), torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    return out, torch.full((hip.rle_encode_scratch(n, H, W),), 77, dtype=torch.uint8, device="cuda")


def test_wrapper_refusals():
    host = RC.patterns(2, 8, 16, np.uint8, SH)["blobs"]
    maps = torch.from_numpy(host).cuda()
    out, ws = _buffers(2, 8, 16, 32)

    def call(m=maps, cap=32, **kw):
        return hip.rle_encode(m, cap, **kw)

    for m in (maps.long(), maps.float(), maps[0], maps[None], maps[:, :, ::2], maps.cpu(), host, maps[:0]):
        with pytest.raises(StswinHipError, match="maps"):
            call(m=m, out=out, workspace=ws)
    for cap in (0, -1, (1 << 20) + 1, 32.0, True, None):
        with pytest.raises(StswinHipError, match="cap"):
            call(cap=cap)
    for bad in (out[0], (out[0],), (out[1], out[0]), (out[0].long(), out[1]), (out[0][:, :16], out[1]), (out[0], out[1][:1]),
                (out[0].view(2, 64), out[1]), (out[0].cpu(), out[1]), (out[0], out[1].short()), (out[0][:, :, :1].expand(2, 32, 2), out[1])):
        with pytest.raises(StswinHipError, match="out|runs|count"):
            call(out=bad, workspace=ws)
    for w in (ws[:-1], ws.view(torch.int32), ws.cpu(), ws.view(2, -1), torch.full((ws.numel() + 4,), 77, dtype=torch.uint8, device="cuda")[1:]):
        with pytest.raises(StswinHipError, match="workspace"):
            call(out=out, workspace=w)
    big = torch.full((8192,), 77, dtype=torch.uint8, device="cuda")
    for kw in (dict(m=big[:256].view(2, 8, 16), out=(big[:512].view(torch.int32).view(2, 32, 2), out[1]), workspace=ws),
               dict(m=big[:256].view(2, 8, 16), out=out, workspace=big),
               dict(out=(out[0], out[0].view(-1)[:2]), workspace=ws),
               dict(out=(big[:512].view(torch.int32).view(2, 32, 2), out[1]), workspace=big)):
        with pytest.raises(StswinHipError, match="shares memory"):
            call(**kw)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out + (ws, big)), "a refused call launched"
    want = R.encode(host, 32)
    got = call(out=out, workspace=ws)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1]))


def test_c_abi():
    lib = hip.load()
    assert lib.stswin_abi_version() == 1
    host = RC.patterns(2, 8, 16, np.int32, SH)["blobs"]
    maps = torch.from_numpy(host).cuda()
    bytes_ = maps.view(torch.uint8)
    out, ws = _buffers(2, 8, 16, 32)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    fn = lib.stswin_rle_encode

    def run(m=p(maps), eb=4, runs=p(out[0]), count=p(out[1]), n=2, H=8, W=16, cap=32, w=p(ws), wbytes=ws.numel()):
        return fn(m, eb, runs, count, n, H, W, cap, w, wbytes, st)

    for kw in (dict(n=0), dict(n=-1), dict(H=0), dict(W=-16), dict(H=16385), dict(W=16385)):
        assert run(**kw) == -1850, kw
    assert lib.stswin_rle_encode_scratch(1, 16385, 1) == -1850 and lib.stswin_rle_encode_scratch(0, 8, 16) == -1850
    for kw in (dict(m=None), dict(runs=None), dict(count=None), dict(w=None)):
        assert run(**kw) == -1851, kw
    for eb in (0, 2, 8, -1):
        assert run(eb=eb) == -1852
    for cap in (0, -1, (1 << 20) + 1):
        assert run(cap=cap) == -1853
    need = lib.stswin_rle_encode_scratch(2, 8, 16)
    assert need == hip.rle_encode_scratch(2, 8, 16) == 4 * 2 * 16 * 1
    assert run(wbytes=need - 1) == -1854 and run(w=p(ws) + 2) == -1854
    assert run(m=p(maps) + 2) == -1855 and run(m=p(maps) + 1) == -1855 and run(runs=p(out[0]) + 2) == -1855 and run(count=p(out[1]) + 1) == -1855
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out + (ws,)), "a refused call launched"
    assert run(wbytes=need) == 0
    want = R.encode(host, 32)
    assert torch.equal(out[0].cpu(), torch.from_numpy(want[0])) and torch.equal(out[1].cpu(), torch.from_numpy(want[1]))
    # the same bytes as a uint8 map [2][8][64], at any byte alignment
    assert run(m=p(bytes_), eb=1, W=64, wbytes=ws.numel()) == -1854              # (four times the columns: a larger table)
    out8, ws8 = _buffers(2, 8, 64, 32)
    assert fn(p(bytes_), 1, p(out8[0]), p(out8[1]), 2, 8, 64, 32, p(ws8), ws8.numel(), st) == 0
    want = R.encode(bytes_.cpu().numpy().reshape(2, 8, 64), 32)
    assert torch.equal(out8[0].cpu(), torch.from_numpy(want[0])) and torch.equal(out8[1].cpu(), torch.from_numpy(want[1]))


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE, N, K = C.SIZE, C.N, C.K
CAP = 2048


def _is_runs(runs, count, cap=CAP):
    return (runs.is_cuda and runs.dtype == torch.int32 and tuple(runs.shape) == (cap, 2) and count.is_cuda and count.dtype == torch.int32
            and count.dim() == 0)


def _encoded(m, cap=CAP):
    runs, count = R.encode(np.ascontiguousarray(m), cap)
    return torch.from_numpy(runs[0]), int(count[0])


def _same_runs(r, want):
    return torch.equal(r[-2].cpu(), want[0]) and int(r[-1]) == want[1]


def _components(labels, c):
    return I.label_components(labels.cpu().numpy()[None], c["nc"], 8, c["skip"], K)[0][0].astype(np.int32)


@pytest.mark.parametrize("mode", list(C._MODES))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_frame_masks(protocol, mode):
    c = C._case(protocol)
    m, s = c["m"], c["seqs"][0]
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, **C._MODES[mode])
    with torch.no_grad():
        # masks alone: the runs of the labels each result carries; the second sequence follows a reset()
        seg = video.VideoSegmenter(m, masks="frame", mask_runs=CAP, **kw)
        for q in c["seqs"]:
            got = seg.segment_sequence(q["fr"])
            assert len(got) == N
            for f, r in enumerate(got):
                assert len(r) == 3 and torch.equal(r[0].cpu(), q["labels"][f]) and _is_runs(r[1], r[2]), f
                assert _same_runs(r, _encoded(q["labels"][f].numpy())), f
        assert max(int(r[2]) for r in got) > 8, "the random model predicts one class: the masks test little"
        # with instances: the runs of the component map, behind what report="frame" appends
        inst = video.VideoSegmenter(m, report="frame", instances=K, masks="frame", mask_runs=CAP, **kw)
        got = inst.segment_sequence(s["fr"])
        for f, r in enumerate(got):
            assert len(r) == 6 and torch.equal(r[0].cpu(), s["labels"][f]) and torch.equal(r[1].cpu(), s["moments"][f]), f
            assert torch.equal(r[2].cpu(), s["rows"][f]) and int(r[3]) == int(s["total"][f]) and _is_runs(r[4], r[5]), f
            assert _same_runs(r, _encoded(_components(s["labels"][f], c))), f
        # with int64 ground truth the labels, and so the runs, come from the scoring launches: the same runs
        plain = video.VideoSegmenter(m, **kw).segment_sequence(s["fr"], gt=s["gt"])
        for seg_gt, maps in ((seg, [_encoded(s["labels"][f].numpy()) for f in range(N)]),
                             (inst, [_encoded(_components(s["labels"][f], c)) for f in range(N)])):
            for f, (r, p) in enumerate(zip(seg_gt.segment_sequence(s["fr"], gt=s["gt"]), plain)):
                p = p if isinstance(p, tuple) else (p,)
                assert torch.equal(r[0], p[0]) and list(r[1:len(p)]) == list(p[1:]) and _same_runs(r, maps[f]), f
        # masks=None: result tuples have the lengths they had
        assert all(isinstance(r, torch.Tensor) for r in video.VideoSegmenter(m, **kw).segment_sequence(s["fr"]))
        assert all(len(r) == 4 for r in video.VideoSegmenter(m, report="frame", instances=K, **kw).segment_sequence(s["fr"]))


@pytest.mark.parametrize("mode", list(C._MODES))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_masks_leave_the_tracked_results_as_they_are(protocol, mode):
    c = T._case(protocol)
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, tracks=True, **C._MODES[mode])
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], masks="frame", mask_runs=CAP, **kw)
        plain = video.VideoSegmenter(c["m"], **kw)
        for n, s in enumerate(c["seqs"]):                                   # parked frames included: ids are read after finish()
            got, want = seg.segment_sequence(s["fr"]), plain.segment_sequence(s["fr"])
            ids = T._want(protocol, n)[0]
            for f, (r, p) in enumerate(zip(got, want)):
                assert len(r) == 7 and len(p) == 5 and all(torch.equal(a, b) for a, b in zip(r, p)), f
                assert torch.equal(r[4].cpu(), torch.from_numpy(ids[f])), f
                assert _is_runs(r[5], r[6]) and _same_runs(r, _encoded(_components(s["labels"][f], c))), f


def test_segmenter_graph_runs_are_views_until_the_next_push():
    c = C._case("endovis18")
    s = c["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, graph=True, masks="frame", mask_runs=CAP)
        seen, held = {}, []
        for f in range(N):
            for g, r in seg.push(s["fr"][f]):
                seen[g] = tuple(t.clone() for t in r)
                held.append((g, r))
        for g, r in seg.finish():
            seen[g] = tuple(t.clone() for t in r)
    assert sorted(seen) == list(range(N)) and all(_same_runs(seen[f], _encoded(s["labels"][f].numpy())) for f in range(N))
    last = held[-1][1]
    replayed = [r for g, r in held if r[1].data_ptr() == last[1].data_ptr()]
    assert len(replayed) >= 2 and all(r[2].data_ptr() == last[2].data_ptr() and torch.equal(r[1], last[1]) for r in replayed)


@pytest.mark.parametrize("protocol,mode", [("endovis18", "eager"), ("endovis18", "batch4"), ("endovis18", "graph"), ("cadis", "graph"),
                                           ("cadis", "eager")])
def test_segmenter_deferred_masks(protocol, mode):
    c = T._case(protocol)
    a, b = c["seqs"]
    names = [f"class {k}" for k in range(c["nc"])]
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, instances=K, tracks=True, mask_runs=CAP, **C._MODES[mode])
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], report="deferred", masks="deferred", **kw)
        empty = seg.mask_report()
        assert len(empty) == 0 and empty.runs.shape == (0, CAP, 2) and empty.source == "instances"
        frame = video.VideoSegmenter(c["m"], report="frame", masks="frame", **kw)
        got = seg.segment_sequence(a["fr"]) + seg.segment_sequence(b["fr"])          # (segment_sequence ends with a reset())
        want = frame.segment_sequence(a["fr"]) + frame.segment_sequence(b["fr"])
        assert all(isinstance(r, torch.Tensor) for r in got)                          # the results are unchanged
        early = video.VideoSegmenter(c["m"], report="deferred", masks="deferred", **kw)
        early.push(a["fr"][:6])                                                       # released frames wait for the tracker
        assert early.chain.parked
        for report in (early.mask_report, early.track_report):
            with pytest.raises(StswinHipError, match="finish"):
                report()
    rep = seg.mask_report(names=names)
    assert rep.sequences == [0] * N + [1] * N and rep.frames == list(range(N)) * 2 and rep.size == SIZE
    assert not rep.truncated.any() and rep.source == "instances"
    trk = seg.track_report()
    for r in range(2 * N):                                                   # row for row what masks="frame" hands out
        w = want[r]
        assert torch.equal(torch.from_numpy(rep.runs[r]), w[-2].cpu()) and int(rep.count[r]) == int(w[-1]), r
        cc = _components((a, b)[r // N]["labels"][r % N], c)
        assert np.array_equal(rep.dense(r), cc), r
        objs = rep.objects(r)
        assert [o["instance"] for o in objs] == np.nonzero(trk.report.present[r])[0].tolist(), r
        for o in objs:
            assert o["cls"] == int(w[2][o["instance"], 0]) and o["name"] == names[o["cls"]] and o["track"] == int(w[4][o["instance"]])
            assert np.array_equal(RC.counts_to_mask(R.string_to_counts(o["counts"]), *SIZE), cc == o["instance"]), (r, o["instance"])
    for q in range(2):                                                       # the MOTS lines carry the ids of track_report()
        lines = [ln.split() for ln in rep.mots_lines(q)]
        ids = [(int(ln[0]), int(ln[1]) % 1000, int(ln[2])) for ln in lines]
        rows = [(w["frame"], w["track"], w["class"]) for w in trk.as_rows() if w["sequence"] == q]
        assert ids == rows and len(rows) >= 2 and all(ln[3:5] == [str(SIZE[0]), str(SIZE[1])] and int(ln[1]) // 1000 == int(ln[2]) for ln in lines)
    seg.reset_metrics()
    assert len(seg.mask_report()) == 0


def test_segmenter_deferred_label_masks_beside_a_frame_report():
    c = C._case("endovis18")
    a = c["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="overlay", report="frame", masks="deferred", mask_runs=CAP, batch=4)
        got = seg.segment_sequence(a["fr"], gt=a["gt"])
    for f, r in enumerate(got):                                              # (overlay, dice, iou, moments): the report's mode is its own
        assert len(r) == 4 and torch.equal(r[3].cpu(), a["moments"][f])
    rep = seg.mask_report()
    assert rep.source == "labels" and rep.frames == list(range(N)) and rep.instances is None and rep.skip == (0,)
    for f in range(N):
        lab = a["labels"][f].numpy()
        assert np.array_equal(rep.dense(f), lab)
        assert [o["cls"] for o in rep.objects(f)] == [v for v in np.unique(lab).tolist() if v != 0]
    with pytest.raises(StswinHipError, match="deferred"):
        seg.instrument_report()


def test_segmenter_mask_runs_below_the_largest_count():
    c = C._case("endovis18")
    a = c["seqs"][0]
    full = [_encoded(a["labels"][f].numpy()) for f in range(N)]
    cap = max(n for _, n in full) - 1
    assert cap >= 1
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, masks="deferred", mask_runs=cap, graph=True)
        seg.segment_sequence(a["fr"])
    rep = seg.mask_report()
    assert rep.count.tolist() == [n for _, n in full] and rep.truncated.tolist() == [n > cap for _, n in full] and rep.truncated.any()
    for f in range(N):
        assert torch.equal(torch.from_numpy(rep.runs[f]), full[f][0][:cap])
        if rep.truncated[f]:
            with pytest.raises(ValueError, match="runs"):
                rep.objects(f)
        else:
            assert np.array_equal(rep.dense(f), a["labels"][f].numpy())


def test_segmenter_masks_refusals():
    m = C._case("endovis18")["m"]
    for kwargs in (dict(out="logits", masks="frame"), dict(out="labels", masks="always"), dict(out="labels", masks=True),
                   dict(out="labels", mask_runs=4096), dict(out="labels", masks="frame", mask_runs=0),
                   dict(out="labels", masks="deferred", mask_runs=(1 << 20) + 1), dict(out="labels", masks="frame", mask_runs=1024.0)):
        with pytest.raises(StswinHipError, match="mask"):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(out="labels", masks="frame"), dict(out="labels", report="deferred"), dict(out="labels")):
        with pytest.raises(StswinHipError, match="masks"):
            video.VideoSegmenter(m, **kwargs).mask_report()
    seg = video.VideoSegmenter(m, out="overlay", masks="deferred")
    assert seg.masks == "deferred" and seg.mask_runs == 16384 and seg.report is None


@pytest.mark.parametrize("mode", list(C._MODES))
def test_segmenter_all_features_with_masks_equal_each_feature_alone(mode):
    """NV12 in and out, stored ground truth with deferred scores, the deferred report with instances, tracks and masks, all at once:
    bit for bit what the segmenters give that switch on one concern each."""
    c, x = T._case("endovis18"), T._all_features_inputs()
    m, kw = c["m"], C._MODES[mode]
    report = dict(report="deferred", min_area=3, instances=K, tracks=True)
    with torch.no_grad():
        full = video.VideoSegmenter(m, pixel_format="nv12", out="overlay", out_format="nv12", gt_table=x["table"], scores="deferred",
                                    masks="deferred", mask_runs=CAP, **report, **kw)
        got = [full.segment_sequence(x["nv12"][0]), full.segment_sequence(x["nv12"][1], gt=x["rgba"])]
        overlay = video.VideoSegmenter(m, pixel_format="nv12", out="overlay", out_format="nv12", **kw)
        scored = video.VideoSegmenter(m, out="labels", out_size=SIZE, gt_table=x["table"], scores="deferred", **kw)
        reported = video.VideoSegmenter(m, out="labels", out_size=SIZE, **report, **kw)
        masked = video.VideoSegmenter(m, out="labels", out_size=SIZE, report="frame", instances=K, masks="deferred", mask_runs=CAP, **kw)
        labels = []
        for s in range(2):
            want = overlay.segment_sequence(x["nv12"][s])
            assert len(got[s]) == len(want) == N
            assert all(isinstance(g, torch.Tensor) and torch.equal(g, w) for g, w in zip(got[s], want)), s
            scored.segment_sequence(x["rgb"][s], gt=x["rgba"] if s else None)
            reported.segment_sequence(x["rgb"][s])
            labels += [r[0].cpu() for r in masked.segment_sequence(x["rgb"][s])]
    a, b = full.endo_scores(), scored.endo_scores()
    assert a.count == b.count == N and a.dices == b.dices and a.ious == b.ious and a.frames == b.frames and full.unmatched() == scored.unmatched()
    assert np.array_equal(full.instrument_report().moments, reported.instrument_report().moments)
    a, b = full.track_report(), reported.track_report()
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.started, b.started) and a.as_rows() == b.as_rows()
    assert np.array_equal(a.report.rows, b.report.rows) and np.array_equal(a.report.total, b.report.total)
    a, b = full.mask_report(), masked.mask_report()
    assert a.sequences == b.sequences == [0] * N + [1] * N and a.frames == b.frames == list(range(N)) * 2 and a.size == b.size == SIZE
    assert np.array_equal(a.runs, b.runs) and np.array_equal(a.count, b.count) and a.tracks is not None and b.tracks is None
    for r in range(2 * N):
        assert np.array_equal(a.dense(r), _components(labels[r], c)), r
    assert len(a.mots_lines(0)) == int((full.track_report().ids[:N] >= 0).sum())
