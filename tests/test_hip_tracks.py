"""hip.track_instances (stswin_track_instances) and VideoSegmenter(tracks=True) on the GPU against the numpy definition
utils.instruments.InstanceTracker, bit for bit: every sequence of tests/tracks_cases.py through hip.label_components and the tracker's
launches, misaligned component maps, reused buffers, graph replay, the refusals and the C ABI's error codes; then the segmenter - eager,
batched and graph-captured, both protocols, with ground truth, parked frames and the deferred track log."""
import numpy as np
import pytest
import torch

import test_hip_components as C
import tracks_cases as TC
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I

pytestmark = pytest.mark.gpu


def _components(c, f, out=None):
    lab = torch.from_numpy(c["labels"][f:f + 1]).cuda()
    return hip.label_components(lab, c["nc"], c["connectivity"], c["skip"], c["K"], out=out)


def _kw(c):
    return dict(min_iou=c["min_iou"], same_class=c["same_class"], min_area=c["min_area"])


def _run(name, state=None, out=None, comp_out=None):
    """The case frame by frame through hip.label_components + hip.track_instances, every frame against the host tracker on the
    downloaded components, and the whole against the case's host run."""
    c = TC.case(name)
    H, W = c["labels"].shape[1:]
    if state is None:
        state = hip.TrackState(H, W, c["K"], "cuda")
    host = TC.tracker(c)
    for f in range(c["labels"].shape[0]):
        comp, rows, total = _components(c, f, comp_out)
        ids, started = hip.track_instances(comp[0], rows[0], total, state, out=out, **_kw(c))
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (c["K"],) and started.dtype == torch.int32 and tuple(started.shape) == (1,)
        want_ids, want_started = host.update(comp[0].cpu().numpy(), rows[0].cpu().numpy(), int(total[0]))
        assert torch.equal(ids.cpu(), torch.from_numpy(want_ids)), (name, f)
        assert int(started[0]) == want_started, (name, f)
        ref_ids, ref_started = TC.host_tracks(name)[f]
        assert np.array_equal(want_ids, ref_ids) and want_started == ref_started, (name, f)


@pytest.mark.parametrize("name", TC.NAMES)
def test_every_case(name):
    _run(name)


@pytest.mark.parametrize("name", ["moving_130", "threshold", "class_change_any"])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_component_maps_off_a_16_byte_boundary(name, offset):
    c = TC.case(name)
    H, W = c["labels"].shape[1:]
    base = torch.full((H * W + 8,), 77, dtype=torch.int32, device="cuda")
    comp = base[offset:offset + H * W].view(1, H, W)
    assert comp.data_ptr() % 16 == 4 * offset
    out = (comp, torch.empty(1, c["K"], 12, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
    _run(name, comp_out=out)
    assert bool((base[:offset] == 77).all()) and bool((base[offset + H * W:] == 77).all())


def test_state_and_out_buffers_are_reused():
    a, b = TC.case("enter_leave"), TC.case("split_merge")
    H, W = a["labels"].shape[1:]
    assert b["labels"].shape[1:] == (H, W) and a["K"] == b["K"]
    state = hip.TrackState(H, W, a["K"], "cuda")
    state.buffer.fill_(77)                                                 # stale counts, pairs and ids would show
    state.reset()
    out = (torch.full((a["K"],), 77, dtype=torch.int32, device="cuda"), torch.full((1,), 77, dtype=torch.int32, device="cuda"))
    _run("enter_leave", state, out)
    state.reset()
    _run("split_merge", state, out)
    state.reset()
    _run("enter_leave", state, out)
    assert state.bytes == hip.load().stswin_track_state_bytes(H, W, a["K"]) and state.buffer.data_ptr() % 16 == 0


@pytest.mark.parametrize("name", ["crossing", "chain"])
def test_the_call_is_capturable(name):
    c = TC.case(name)
    H, W, K = *c["labels"].shape[1:], c["K"]
    state = hip.TrackState(H, W, K, "cuda")
    cc = (torch.empty(1, H, W, dtype=torch.int32, device="cuda"), torch.empty(1, K, 12, dtype=torch.int64, device="cuda"),
          torch.empty(1, dtype=torch.int32, device="cuda"))
    out = (torch.full((K,), 77, dtype=torch.int32, device="cuda"), torch.full((1,), 77, dtype=torch.int32, device="cuda"))
    _components(c, 0, cc)
    hip.track_instances(cc[0][0], cc[1][0], cc[2], state, out=out, **_kw(c))      # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.track_instances(cc[0][0], cc[1][0], cc[2], state, out=out, **_kw(c))
    for _ in range(2):                                                      # the whole sequence, twice, through the one graph
        state.reset()
        for f, (want_ids, want_started) in enumerate(TC.host_tracks(name)):
            _components(c, f, cc)
            graph.replay()
            assert torch.equal(out[0].cpu(), torch.from_numpy(want_ids)) and int(out[1][0]) == want_started, f


def test_wrapper_refusals():
    c = TC.case("crossing")
    H, W, K = *c["labels"].shape[1:], c["K"]
    state = hip.TrackState(H, W, K, "cuda")
    comp, rows, total = _components(c, 0)
    comp, rows = comp[0], rows[0]
    torch.cuda.synchronize()
    state.buffer.fill_(77)
    out = (torch.full((K,), 77, dtype=torch.int32, device="cuda"), torch.full((1,), 77, dtype=torch.int32, device="cuda"))
    call = lambda comp=comp, rows=rows, total=total, state=state, **kw: hip.track_instances(comp, rows, total, state, **kw)
    for bad in (comp.long(), comp[None], comp.t(), comp.cpu(), comp[:, :W - 1], comp.cpu().numpy()):
        with pytest.raises(StswinHipError, match="components"):
            call(comp=bad, out=out)
    for bad in (rows.int(), rows[:K - 1], rows[:, :10], rows.cpu(), rows[None], rows.t().contiguous().t()):
        with pytest.raises(StswinHipError, match="rows"):
            call(rows=bad, out=out)
    for bad in (total.long(), total.cpu(), torch.zeros(2, dtype=torch.int32, device="cuda"), 3):
        with pytest.raises(StswinHipError, match="total"):
            call(total=bad, out=out)
    for bad in (None, state.buffer, hip.TrackState(H, W + 1, K, "cuda"), hip.TrackState(H, W, K + 1, "cuda")):
        with pytest.raises(StswinHipError):
            call(state=bad, out=out)
    for kw in (dict(min_iou=-1), dict(min_iou=1001), dict(min_iou=0.1), dict(min_iou=True), dict(same_class=1), dict(same_class=None),
               dict(min_area=0), dict(min_area=2.0)):
        with pytest.raises(StswinHipError):
            call(out=out, **kw)
    for bad in ((out[0].long(), out[1]), (out[0][:K - 1], out[1]), (out[0], out[1].long()), (out[0].cpu(), out[1]), (out[0],), out[0]):
        with pytest.raises(StswinHipError):
            call(out=bad)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(out=(comp.view(-1)[:K], out[1]))
    with pytest.raises(StswinHipError, match="shares memory"):
        call(out=(out[0], out[0][:1]))
    with pytest.raises(StswinHipError, match="shares memory"):
        call(out=(rows.view(torch.int32).view(-1)[:K], out[1]))
    with pytest.raises(StswinHipError, match="shares memory"):
        call(comp=state.buffer.view(torch.int32)[:H * W].view(H, W), out=out)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(total=out[1], out=out)
    for bad in (dict(H=0), dict(W=16385), dict(K=0), dict(K=1025), dict(K=8.0), dict(device="cpu")):
        with pytest.raises(StswinHipError):
            hip.TrackState(**{**dict(H=H, W=W, K=K, device="cuda"), **bad})
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (state.buffer,) + out), "a refused call launched"
    state.reset()
    ids, started = call(out=out, **_kw(c))
    assert torch.equal(ids.cpu(), torch.from_numpy(TC.host_tracks("crossing")[0][0])) and int(started[0]) == 2


def test_c_abi():
    for s in ("stswin_track_state_bytes", "stswin_track_reset", "stswin_track_instances"):
        assert s in hip.declared_symbols()
    lib = hip.load()
    assert lib.stswin_abi_version() == 1
    c = TC.case("crossing")
    H, W, K = *c["labels"].shape[1:], c["K"]
    comp, rows, total = _components(c, 0)
    need = lib.stswin_track_state_bytes(H, W, K)
    assert need == 4 * (4 + 3 * K + 2 * K * K + H * W) and need % 16 == 0
    assert lib.stswin_track_state_bytes(3, 5, 3) == 4 * (28 + 4 + 16)       # 4 + 9 + 18 = 31 -> 32 words, then 15 pixels -> 16
    buf = torch.full((need + 16,), 77, dtype=torch.uint8, device="cuda")
    out = (torch.full((K,), 77, dtype=torch.int32, device="cuda"), torch.full((2,), 77, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def run(comp=p(comp), rows=p(rows), total=p(total), state=p(buf), nbytes=need, H=H, W=W, K=K, iou=100, same=1, area=1, ids=p(out[0]),
            started=p(out[1])):
        return lib.stswin_track_instances(comp, rows, total, state, nbytes, H, W, K, iou, same, area, ids, started, st)

    def reset(state=p(buf), nbytes=need, H=H, W=W, K=K):
        return lib.stswin_track_reset(state, nbytes, H, W, K, st)

    for kw in (dict(H=0), dict(W=-1), dict(H=16385), dict(W=16385)):
        assert run(**kw) == -1840 and reset(**kw) == -1840, kw
    assert lib.stswin_track_state_bytes(0, 8, 8) == -1840 and lib.stswin_track_state_bytes(8, 16385, 8) == -1840
    for k in (0, -1, 1025):
        assert run(K=k) == -1841 and reset(K=k) == -1841 and lib.stswin_track_state_bytes(8, 8, k) == -1841
    for kw in (dict(comp=None), dict(rows=None), dict(total=None), dict(state=None), dict(ids=None), dict(started=None)):
        assert run(**kw) == -1842, kw
    assert reset(state=None) == -1842
    assert run(nbytes=need - 1) == -1843 and run(state=p(buf) + 4) == -1843 and reset(nbytes=need - 1) == -1843 and reset(state=p(buf) + 8) == -1843
    for kw in (dict(comp=p(comp) + 2), dict(rows=p(rows) + 4), dict(total=p(total) + 1), dict(ids=p(out[0]) + 2), dict(started=p(out[1]) + 3)):
        assert run(**kw) == -1844, kw
    for kw in (dict(iou=-1), dict(iou=1001), dict(same=2), dict(same=-1), dict(area=0)):
        assert run(**kw) == -1845, kw
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (buf,) + out), "a refused call launched"
    assert reset() == 0 and run() == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), torch.from_numpy(TC.host_tracks("crossing")[0][0])) and out[1].tolist() == [2, 77]
    assert bool((buf[need:] == 77).all())


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE, N, K = C.SIZE, C.N, C.K
_WANT = {}
_CASES = {}
CADIS_SEED = 5          # (the shared case's model, seed 4, gives its second sequence no birth after frame 0: see the condition below)


def _case(protocol):
    """endovis18: the shared case of tests/test_hip_components.py.  cadis: the same construction - two sequences, an int64 ground truth,
    the results of report="frame" alone and the host components of their label maps - with a model of another seed, whose sequences
    show births after frame 0.  Computed once, shared, never changed."""
    if protocol == "endovis18":
        return C._case(protocol)
    if protocol not in _CASES:
        m = C._model(protocol, seed=CADIS_SEED)
        nc, skip = 9, (8,)
        g = np.random.default_rng(17)
        seqs = []
        for s in range(2):
            fr = C._frames(N, seed=40 + s)
            with torch.no_grad():
                res = video.VideoSegmenter(m, out="labels", out_size=SIZE, protocol=protocol, report="frame").segment_sequence(fr)
            labels = np.stack([r[0].cpu().numpy() for r in res])
            _, rows, total = I.label_components(labels, nc, 8, skip, K)
            seqs.append(dict(fr=fr, labels=torch.from_numpy(labels), moments=torch.stack([r[1].cpu() for r in res]),
                             rows=torch.from_numpy(rows), total=torch.from_numpy(total), gt=torch.from_numpy(g.integers(0, nc - 1, (N, *SIZE)))))
        _CASES[protocol] = dict(m=m, nc=nc, skip=skip, seqs=seqs)
    return _CASES[protocol]


def _host_tracks(labels, c, min_area=1, iou=100, same=True):
    """int64 labels [n][H][W] of one sequence -> (ids int32 [n][K], started [n]) by the host components and the host tracker in frame
    order."""
    comp, rows, total = I.label_components(np.asarray(labels), c["nc"], 8, c["skip"], K)
    t = I.InstanceTracker(K, iou, same, min_area)
    got = [t.update(comp[f], rows[f], total[f]) for f in range(len(comp))]
    return np.stack([g[0] for g in got]), np.asarray([g[1] for g in got])


def _want(protocol, s, min_area=1):
    """The host tracks of the case's sequence s; computed once, never changed."""
    key = (protocol, s, min_area)
    if key not in _WANT:
        c = _case(protocol)
        _WANT[key] = _host_tracks(c["seqs"][s]["labels"].numpy(), c, min_area)
    return _WANT[key]


@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_the_random_model_s_sequences_show_matches_and_births(protocol):
    for s in range(2):
        ids, started = _want(protocol, s)
        births_later = int(started[-1]) - int(started[0])
        present = int((ids[1:] >= 0).sum())
        assert births_later >= 1, "no instance is born after frame 0: another seed"
        assert present - births_later >= 1, "no instance is matched: another seed"


@pytest.mark.parametrize("mode", list(C._MODES))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_frame_tracks(protocol, mode):
    c = _case(protocol)
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, **C._MODES[mode])
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], tracks=True, **kw)
        for n, s in enumerate(c["seqs"]):                                # the second sequence follows a reset(): ids start again at 0
            want = _want(protocol, n)[0]
            got = seg.segment_sequence(s["fr"])
            assert len(got) == N
            for f, r in enumerate(got):
                assert len(r) == 5 and torch.equal(r[0].cpu(), s["labels"][f]) and torch.equal(r[1].cpu(), s["moments"][f]), f
                assert torch.equal(r[2].cpu(), s["rows"][f]) and int(r[3]) == int(s["total"][f]), f
                assert r[4].is_cuda and r[4].dtype == torch.int32 and torch.equal(r[4].cpu(), torch.from_numpy(want[f])), f
            assert int(got[0][4].max()) == int(s["total"][0].clamp(max=K)) - 1 and int(got[0][4].min()) >= -1
        # tracks=False is today's path: element for element what instances=K gives
        s = c["seqs"][0]
        for f, r in enumerate(video.VideoSegmenter(c["m"], **kw).segment_sequence(s["fr"])):
            assert len(r) == 4 and torch.equal(r[0].cpu(), s["labels"][f]) and torch.equal(r[1].cpu(), s["moments"][f]), f
            assert torch.equal(r[2].cpu(), s["rows"][f]) and int(r[3]) == int(s["total"][f]), f
        # with int64 ground truth the labels, the instances and so the tracks come from the scoring launches
        got = seg.segment_sequence(s["fr"], gt=s["gt"])
        plain = video.VideoSegmenter(c["m"], **kw).segment_sequence(s["fr"], gt=s["gt"])
        want = _want(protocol, 0)[0]
        for f, (r, p) in enumerate(zip(got, plain)):
            assert len(r) == len(p) + 1 and all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for a, b in zip(r, p)), f
            assert torch.equal(r[-1].cpu(), torch.from_numpy(want[f])), f
        # another threshold, any class and the segmenter's min_area, against the result's own labels
        other = video.VideoSegmenter(c["m"], tracks=True, track_iou=400, track_same_class=False, min_area=4, **kw).segment_sequence(s["fr"])
        want = _host_tracks(np.stack([r[0].cpu().numpy() for r in other]), c, 4, 400, False)[0]
        assert all(torch.equal(r[4].cpu(), torch.from_numpy(want[f])) for f, r in enumerate(other))


@pytest.mark.parametrize("protocol,mode", [("endovis18", "eager"), ("cadis", "eager"), ("endovis18", "batch4"), ("endovis18", "graph")])
def test_parked_frames_get_their_ids_in_the_tensor_handed_out(protocol, mode):
    c = _case(protocol)
    s = c["seqs"][1]
    want = _want(protocol, 1)[0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, tracks=True,
                                   **C._MODES[mode])
        held, early = {}, []
        for f in range(N):
            for g, r in seg.push(s["fr"][f]):
                if any(h not in held for h in range(g)):                   # released before a predecessor: it cannot be tracked yet
                    early.append(g)
                held[g] = r[4] if g in early or mode != "graph" else r[4].clone()      # (a replayed step's ids are a view)
        for g, r in seg.finish():
            if any(h not in held for h in range(g)):
                early.append(g)
            held[g] = r[4]
    assert sorted(held) == list(range(N)) and len(early) >= 2
    for g in range(N):
        assert torch.equal(held[g].cpu(), torch.from_numpy(want[g])), (g, early)


@pytest.mark.parametrize("protocol,mode", [("endovis18", "eager"), ("endovis18", "batch4"), ("endovis18", "graph"), ("cadis", "graph")])
def test_segmenter_deferred_tracks(protocol, mode):
    c = _case(protocol)
    a, b = c["seqs"]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, protocol=protocol, report="deferred", min_area=3, instances=K,
                                   tracks=True, **C._MODES[mode])
        empty = seg.track_report()
        assert len(empty) == 0 and empty.ids.shape == (0, K) and empty.tracks == []
        got_a = seg.segment_sequence(a["fr"])
        seg.segment_sequence(b["fr"], gt=b["gt"])
    assert all(isinstance(r, torch.Tensor) and torch.equal(r.cpu(), a["labels"][f]) for f, r in enumerate(got_a))
    rep = seg.track_report()
    inst = I.InstanceReport.from_rows(torch.cat([a["rows"], b["rows"]]).numpy(), torch.cat([a["total"], b["total"]]).numpy(), SIZE,
                                      min_area=3, frames=list(range(N)) * 2, sequences=[0] * N + [1] * N)
    (ia, sa), (ib, sb) = _want(protocol, 0, 3), _want(protocol, 1, 3)
    want = I.TrackReport.from_ids(inst, np.concatenate([ia, ib]), np.concatenate([sa, sb]))
    assert np.array_equal(rep.ids, want.ids) and np.array_equal(rep.started, want.started) and rep.as_rows() == want.as_rows()
    assert len(rep.tracks) == len(want.tracks) == int(sa[-1]) + int(sb[-1])
    for t, w in zip(rep.tracks, want.tracks):
        assert {k: v for k, v in t.items() if not isinstance(v, np.ndarray)} == {k: v for k, v in w.items() if not isinstance(v, np.ndarray)}
        assert all(np.array_equal(t[k], w[k]) for k in ("frames", "centroids", "areas"))
    assert np.array_equal(seg.instance_report().rows, inst.rows)
    seg.reset_metrics()
    assert len(seg.track_report()) == 0


def test_segmenter_deferred_track_log_grows_past_its_first_rows():
    c = _case("endovis18")
    a = c["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="overlay", report="deferred", batch=4, instances=K, tracks=True)
        for _ in range(7):                                                # 70 rows: past the log's first 64
            seg.segment_sequence(a["fr"])
    rep = seg.track_report()
    ids, started = _want("endovis18", 0)
    assert len(rep) == 7 * N and rep.report.sequences == [s for s in range(7) for _ in range(N)]
    assert np.array_equal(rep.ids, np.tile(ids, (7, 1))) and np.array_equal(rep.started, np.tile(started, 7))
    assert len(rep.tracks) == 7 * int(started[-1])


def test_segmenter_tracks_refusals():
    m = _case("endovis18")["m"]
    for kwargs in (dict(out="labels", report="frame", tracks=True), dict(out="labels", tracks=True),
                   dict(out="labels", report="frame", instances=8, tracks=1), dict(out="labels", report="frame", instances=8, track_iou=200),
                   dict(out="labels", report="frame", instances=8, track_same_class=False),
                   dict(out="labels", report="frame", instances=8, tracks=True, track_iou=1001),
                   dict(out="labels", report="frame", instances=8, tracks=True, track_iou=-1),
                   dict(out="labels", report="frame", instances=8, tracks=True, track_iou=0.5),
                   dict(out="labels", report="frame", instances=8, tracks=True, track_same_class=1)):
        with pytest.raises(StswinHipError):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(out="labels", report="deferred", instances=8), dict(out="labels", report="frame", instances=8, tracks=True),
                   dict(out="labels")):
        with pytest.raises(StswinHipError, match="tracks"):
            video.VideoSegmenter(m, **kwargs).track_report()


def _all_features_inputs():
    """Two NV12 sequences made from the shared frames, and the second one's ground truth as an RGBA picture under the first 12
    colours of the default palette (a few pixels in a colour the table lacks: unmatched).  Computed once, never changed."""
    if "all" not in _CASES:
        from stswincl_amd.utils import groundtruth as G, visualize as V, yuv as Y
        c = _case("endovis18")
        nv12 = [Y.rgb_to_nv12(s["fr"], Y.to_yuv_matrix()) for s in c["seqs"]]
        rgb = [Y.yuv_to_rgb(x, "nv12", Y.to_rgb_matrix(), "replicate") for x in nv12]
        palette = V.default_palette()[:12]
        gt = c["seqs"][1]["gt"].numpy()
        rgba = np.concatenate([palette[gt], np.full((N, *SIZE, 1), 255, dtype=np.uint8)], axis=3)
        rgba[:, 5, 7:11, :3] = (1, 2, 3)
        _CASES["all"] = dict(nv12=nv12, rgb=rgb, rgba=rgba, table=G.colour_table(palette))
    return _CASES["all"]


@pytest.mark.parametrize("mode", list(C._MODES))
def test_segmenter_all_features_at_once_equal_each_feature_alone(mode):
    """Every option of the segmenter switched on together - NV12 in, NV12 overlays out, stored ground truth with deferred scores, the
    deferred report with instances and tracks - gives, bit for bit and row for row, what the segmenters give that switch on one
    concern each (and that the tests of those concerns pin)."""
    c, x = _case("endovis18"), _all_features_inputs()
    m, kw = c["m"], C._MODES[mode]
    report = dict(report="deferred", min_area=3, instances=K, tracks=True)
    with torch.no_grad():
        full = video.VideoSegmenter(m, pixel_format="nv12", out="overlay", out_format="nv12", gt_table=x["table"], scores="deferred",
                                    **report, **kw)
        got = [full.segment_sequence(x["nv12"][0]), full.segment_sequence(x["nv12"][1], gt=x["rgba"])]
        overlay = video.VideoSegmenter(m, pixel_format="nv12", out="overlay", out_format="nv12", **kw)
        scored = video.VideoSegmenter(m, out="labels", out_size=SIZE, gt_table=x["table"], scores="deferred", **kw)
        reported = video.VideoSegmenter(m, out="labels", out_size=SIZE, **report, **kw)
        for s in range(2):
            want = overlay.segment_sequence(x["nv12"][s])
            assert len(got[s]) == len(want) == N
            for f in range(N):
                assert isinstance(got[s][f], torch.Tensor) and got[s][f].shape == (SIZE[0] * 3 // 2, SIZE[1]), (s, f)
                assert got[s][f].dtype == torch.uint8 and torch.equal(got[s][f], want[f]), (s, f)
            scored.segment_sequence(x["rgb"][s], gt=x["rgba"] if s else None)
            reported.segment_sequence(x["rgb"][s])
    a, b = full.endo_scores(), scored.endo_scores()
    assert a.count == b.count == N and a.dices == b.dices and a.ious == b.ious and a.frames == b.frames == list(range(N))
    assert a.sequences == b.sequences == [0] * N and np.array_equal(a.dice, b.dice, equal_nan=True) and np.array_equal(a.iou, b.iou, equal_nan=True)
    assert full.unmatched() == scored.unmatched() == 4 * N
    a, b = full.instrument_report(), reported.instrument_report()
    assert a.sequences == b.sequences == [0] * N + [1] * N and a.frames == b.frames == list(range(N)) * 2
    assert np.array_equal(a.moments, b.moments) and a.size == b.size == SIZE and a.min_area == b.min_area == 3
    assert np.array_equal(a.presence(), b.presence()) and np.array_equal(a.box, b.box, equal_nan=True)
    assert np.array_equal(a.angle, b.angle, equal_nan=True)
    a, b = full.instance_report(), reported.instance_report()
    assert a.sequences == b.sequences == [0] * N + [1] * N and a.frames == b.frames == list(range(N)) * 2
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.total, b.total) and a.size == b.size and a.min_area == b.min_area
    assert np.array_equal(a.present, b.present) and np.array_equal(a.box, b.box, equal_nan=True)
    assert np.array_equal(a.angle, b.angle, equal_nan=True) and np.array_equal(a.counts(), b.counts())
    assert a.as_rows() == b.as_rows() and np.array_equal(a.truncated, b.truncated)
    a, b = full.track_report(), reported.track_report()
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.started, b.started) and a.as_rows() == b.as_rows()
    assert len(a.tracks) == len(b.tracks) >= 2 and int(a.ids.max()) >= 1
    for t, w in zip(a.tracks, b.tracks):
        assert {k: v for k, v in t.items() if not isinstance(v, np.ndarray)} == {k: v for k, v in w.items() if not isinstance(v, np.ndarray)}
        assert all(np.array_equal(t[k], w[k]) for k in ("frames", "centroids", "areas"))
