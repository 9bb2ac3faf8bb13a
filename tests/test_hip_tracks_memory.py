"""The tracker with a memory on the GPU - hip.track_instances on a hip.TrackState(..., max_gap=g) (stswin_track_memory) and
VideoSegmenter(tracks=True, track_max_gap=g) - against the numpy definition utils.instruments.MemoryTracker, bit for bit: every sequence
of tests/tracks_memory_cases.py and tests/tracks_cases.py through hip.label_components and the tracker's three launches at gaps 0
(through the memory kernels), 1 and 3, misaligned component maps, reused buffers, graph replay, the refusals and the C ABI's error
codes; then the segmenter - eager, batched and graph-captured, with the report per frame and deferred."""
import numpy as np
import pytest
import torch

import test_hip_components as C
import tracks_cases as TC
import tracks_memory_cases as MC
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I

pytestmark = pytest.mark.gpu

_NAMES = MC.NAMES + tuple(n for n in TC.NAMES if n != "overflow")


def _find(name):
    return MC.case(name) if name in MC.NAMES else TC.case(name)


def _components(c, f, out=None):
    lab = torch.from_numpy(c["labels"][f:f + 1]).cuda()
    return hip.label_components(lab, c["nc"], c["connectivity"], c["skip"], c["K"], out=out)


def _kw(c):
    return dict(min_iou=c["min_iou"], same_class=c["same_class"], min_area=c["min_area"])


def _state(c, gap):
    return hip.TrackState(*c["labels"].shape[1:], c["K"], "cuda", max_gap=gap, memory=True)


def _run(name, gap, state=None, out=None, comp_out=None):
    """The case frame by frame through hip.label_components + hip.track_instances, every frame against the host tracker on the
    downloaded components."""
    c = _find(name)
    if state is None:
        state = _state(c, gap)
    assert state.memory and state.max_gap == gap
    host = MC.tracker(c, gap)
    got = []
    for f in range(c["labels"].shape[0]):
        comp, rows, total = _components(c, f, comp_out)
        ids, started = hip.track_instances(comp[0], rows[0], total, state, out=out, **_kw(c))
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (c["K"],) and started.dtype == torch.int32 and tuple(started.shape) == (1,)
        want_ids, want_started = host.update(comp[0].cpu().numpy(), rows[0].cpu().numpy(), int(total[0]))
        assert torch.equal(ids.cpu(), torch.from_numpy(want_ids)), (name, gap, f)
        assert int(started[0]) == want_started, (name, gap, f)
        got.append((want_ids, want_started))
    return got


@pytest.mark.parametrize("gap", MC.GAPS)
@pytest.mark.parametrize("name", _NAMES)
def test_every_case(name, gap):
    got = _run(name, gap)
    if name in MC.NAMES:                                                    # (the device components are the host's: the whole host run too)
        for f, ((ids, started), (ref_ids, ref_started)) in enumerate(zip(got, MC.host_tracks(name, gap))):
            assert np.array_equal(ids, ref_ids) and started == ref_started, (name, gap, f)
    elif gap == 0:
        for f, ((ids, started), (ref_ids, ref_started)) in enumerate(zip(got, TC.host_tracks(name))):
            assert np.array_equal(ids, ref_ids) and started == ref_started, (name, f)


def test_flicker_and_empty_frame_keep_their_ids():
    got = _run("flicker", 2)
    assert [g[0][:2].tolist() for g in got] == [[0, 1], [1, -1], [0, 1], [1, -1], [1, -1], [0, 1]] and got[-1][1] == 2
    got = _run("empty_frame", 1)
    assert got[3][0][:2].tolist() == [0, 1] and got[3][1] == 2


@pytest.mark.parametrize("name", ["flicker", "odd_size", "overwritten_other"])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_component_maps_off_a_16_byte_boundary(name, offset):
    c = MC.case(name)
    H, W = c["labels"].shape[1:]
    base = torch.full((H * W + 8,), 77, dtype=torch.int32, device="cuda")
    comp = base[offset:offset + H * W].view(1, H, W)
    assert comp.data_ptr() % 16 == 4 * offset
    out = (comp, torch.empty(1, c["K"], 12, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
    _run(name, 3, comp_out=out)
    assert bool((base[:offset] == 77).all()) and bool((base[offset + H * W:] == 77).all())


@pytest.mark.parametrize("name", ["capacity", "slot_reuse"])
def test_state_and_out_buffers_are_reused(name):
    c = MC.case(name)
    H, W, K = *c["labels"].shape[1:], c["K"]
    state = _state(c, 3)
    state.buffer.fill_(77)                                                 # stale slots, counts, pairs and memory would show
    state.reset()
    out = (torch.full((K,), 77, dtype=torch.int32, device="cuda"), torch.full((1,), 77, dtype=torch.int32, device="cuda"))
    for _ in range(3):                                                     # (both sequences end with a lost track alive and remembered)
        _run(name, 3, state, out)
        state.reset()
    assert state.bytes == hip.load().stswin_track_memory_state_bytes(H, W, K) and state.buffer.data_ptr() % 16 == 0
    assert hip.TrackState(H, W, K, "cuda").bytes == hip.load().stswin_track_state_bytes(H, W, K)       # max_gap = 0: as it was
    assert not hip.TrackState(H, W, K, "cuda", max_gap=0).memory and hip.TrackState(H, W, K, "cuda", max_gap=2).memory


def test_the_call_is_capturable():
    c = MC.case("flicker")
    H, W, K = *c["labels"].shape[1:], c["K"]
    state = _state(c, 1)
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
        for f, (want_ids, want_started) in enumerate(MC.host_tracks("flicker", 1)):
            _components(c, f, cc)
            graph.replay()
            assert torch.equal(out[0].cpu(), torch.from_numpy(want_ids)) and int(out[1][0]) == want_started, f


def test_wrapper_refusals():
    c = MC.case("flicker")
    H, W, K = *c["labels"].shape[1:], c["K"]
    state = _state(c, 2)
    comp, rows, total = _components(c, 0)
    comp, rows = comp[0], rows[0]
    torch.cuda.synchronize()
    state.buffer.fill_(77)
    out = (torch.full((K,), 77, dtype=torch.int32, device="cuda"), torch.full((1,), 77, dtype=torch.int32, device="cuda"))
    call = lambda comp=comp, rows=rows, total=total, state=state, **kw: hip.track_instances(comp, rows, total, state, **kw)
    for bad in (comp.long(), comp[None], comp.cpu(), comp[:, :W - 1]):
        with pytest.raises(StswinHipError, match="components"):
            call(comp=bad, out=out)
    for bad in (rows.int(), rows[:K - 1], rows.cpu()):
        with pytest.raises(StswinHipError, match="rows"):
            call(rows=bad, out=out)
    for bad in (None, state.buffer, hip.TrackState(H, W + 1, K, "cuda", max_gap=2), hip.TrackState(H, W, K + 1, "cuda", max_gap=2)):
        with pytest.raises(StswinHipError):
            call(state=bad, out=out)
    for kw in (dict(min_iou=1001), dict(same_class=1), dict(min_area=0)):
        with pytest.raises(StswinHipError):
            call(out=out, **kw)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(comp=state.buffer.view(torch.int32)[-H * W:].view(H, W), out=out)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(total=out[1], out=out)
    for bad in (dict(max_gap=-1), dict(max_gap=1000001), dict(max_gap=1.0), dict(max_gap=True), dict(max_gap=None), dict(memory=1),
                dict(max_gap=2, K=1025), dict(max_gap=2, H=0), dict(max_gap=2, device="cpu")):
        with pytest.raises(StswinHipError):
            hip.TrackState(**{**dict(H=H, W=W, K=K, device="cuda"), **bad})
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (state.buffer,) + out), "a refused call launched"
    state.reset()
    ids, started = call(out=out, **_kw(c))
    assert torch.equal(ids.cpu(), torch.from_numpy(MC.host_tracks("flicker", 2)[0][0])) and int(started[0]) == 2


def test_c_abi():
    for s in ("stswin_track_memory_state_bytes", "stswin_track_memory_reset", "stswin_track_memory"):
        assert s in hip.declared_symbols()
    lib = hip.load()
    c = MC.case("flicker")
    H, W, K = *c["labels"].shape[1:], c["K"]
    comp, rows, total = _components(c, 0)
    need = lib.stswin_track_memory_state_bytes(H, W, K)
    assert need == 4 * (4 + 6 * K + 2 * K * K + H * W) and need % 16 == 0
    assert lib.stswin_track_memory_state_bytes(3, 5, 3) == 4 * (40 + 16)     # 4 + 18 + 18 = 40 words, then 15 pixels -> 16
    assert lib.stswin_track_memory_state_bytes(3, 5, 1) == 4 * (12 + 16)     # 4 + 6 + 2 = 12 words
    buf = torch.full((need + 16,), 77, dtype=torch.uint8, device="cuda")
    out = (torch.full((K,), 77, dtype=torch.int32, device="cuda"), torch.full((2,), 77, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def run(comp=p(comp), rows=p(rows), total=p(total), state=p(buf), nbytes=need, H=H, W=W, K=K, gap=2, iou=100, same=1, area=1,
            ids=p(out[0]), started=p(out[1])):
        return lib.stswin_track_memory(comp, rows, total, state, nbytes, H, W, K, gap, iou, same, area, ids, started, st)

    def reset(state=p(buf), nbytes=need, H=H, W=W, K=K):
        return lib.stswin_track_memory_reset(state, nbytes, H, W, K, st)

    for kw in (dict(H=0), dict(W=-1), dict(H=16385), dict(W=16385)):
        assert run(**kw) == -1860 and reset(**kw) == -1860, kw
    assert lib.stswin_track_memory_state_bytes(0, 8, 8) == -1860 and lib.stswin_track_memory_state_bytes(8, 16385, 8) == -1860
    for k in (0, -1, 1025):
        assert run(K=k) == -1861 and reset(K=k) == -1861 and lib.stswin_track_memory_state_bytes(8, 8, k) == -1861
    for kw in (dict(comp=None), dict(rows=None), dict(total=None), dict(state=None), dict(ids=None), dict(started=None)):
        assert run(**kw) == -1862, kw
    assert reset(state=None) == -1862
    assert run(nbytes=need - 1) == -1863 and run(state=p(buf) + 4) == -1863 and reset(nbytes=need - 1) == -1863 and reset(state=p(buf) + 8) == -1863
    for kw in (dict(comp=p(comp) + 2), dict(rows=p(rows) + 4), dict(total=p(total) + 1), dict(ids=p(out[0]) + 2), dict(started=p(out[1]) + 3)):
        assert run(**kw) == -1864, kw
    for kw in (dict(iou=-1), dict(iou=1001), dict(same=2), dict(same=-1), dict(area=0)):
        assert run(**kw) == -1865, kw
    for g in (-1, 1000001):
        assert run(gap=g) == -1866
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (buf,) + out), "a refused call launched"
    assert reset() == 0 and run() == 0 and run(gap=1000000) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu(), torch.from_numpy(MC.host_tracks("flicker", 2)[0][0])) and out[1].tolist() == [2, 77]
    assert bool((buf[need:] == 77).all())


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE, N, K = C.SIZE, C.N, C.K
GAP = 2
_AREAS = (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)
_HOST = {}


def _host(s):
    """Sequence s of the shared endovis18 case: its host components, and the smallest min_area of _AREAS at which an instance drops
    out and comes back within GAP frames - the memory then starts fewer tracks than the tracker without.  Computed once, never
    changed."""
    if s not in _HOST:
        c = C._case("endovis18")
        comp, rows, total = I.label_components(c["seqs"][s]["labels"].numpy(), c["nc"], 8, c["skip"], K)
        _HOST[s] = dict(comp=comp, rows=rows, total=total)
        if s == 0:
            for a in _AREAS:
                if _tracks(0, a, GAP)[1][-1] < _tracks(0, a, 0)[1][-1]:
                    _HOST["min_area"] = a
                    break
    return _HOST[s]


def _tracks(s, min_area, gap, iou=100, same=True):
    h = _host(s)
    t = I.MemoryTracker(K, gap, iou, same, min_area)
    got = [t.update(h["comp"][f], h["rows"][f], h["total"][f]) for f in range(N)]
    return np.stack([g[0] for g in got]), np.asarray([g[1] for g in got])


def _min_area():
    _host(0)
    assert "min_area" in _HOST, "no min_area of the list makes an instance of the random model's sequence flicker: another seed"
    return _HOST["min_area"]


@pytest.mark.parametrize("mode", list(C._MODES))
def test_segmenter_frame_tracks_with_a_gap(mode):
    c = C._case("endovis18")
    a = _min_area()
    kw = dict(out="labels", out_size=SIZE, report="frame", instances=K, tracks=True, min_area=a, **C._MODES[mode])
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], track_max_gap=GAP, **kw)
        for n, s in enumerate(c["seqs"]):                                # the second sequence follows a reset(): ids start again at 0
            want = _tracks(n, a, GAP)[0]
            got = seg.segment_sequence(s["fr"])
            assert len(got) == N
            for f, r in enumerate(got):
                assert len(r) == 5 and torch.equal(r[0].cpu(), s["labels"][f]) and torch.equal(r[2].cpu(), s["rows"][f]), f
                assert r[4].is_cuda and r[4].dtype == torch.int32 and torch.equal(r[4].cpu(), torch.from_numpy(want[f])), f
        assert seg.chain.state.memory and seg.chain.state.max_gap == GAP
        # another threshold and any class, on the first sequence again
        other = video.VideoSegmenter(c["m"], track_max_gap=1, track_iou=400, track_same_class=False, **kw).segment_sequence(c["seqs"][0]["fr"])
        want = _tracks(0, a, 1, 400, False)[0]
        assert all(torch.equal(r[4].cpu(), torch.from_numpy(want[f])) for f, r in enumerate(other))


@pytest.mark.parametrize("mode", list(C._MODES))
def test_segmenter_deferred_tracks_with_a_gap(mode):
    c = C._case("endovis18")
    a, b = c["seqs"]
    area = _min_area()
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, report="deferred", min_area=area, instances=K, tracks=True,
                                   track_max_gap=GAP, **C._MODES[mode])
        seg.segment_sequence(a["fr"])
        seg.segment_sequence(b["fr"], gt=b["gt"])
    rep = seg.track_report()
    inst = I.InstanceReport.from_rows(torch.cat([a["rows"], b["rows"]]).numpy(), torch.cat([a["total"], b["total"]]).numpy(), SIZE,
                                      min_area=area, frames=list(range(N)) * 2, sequences=[0] * N + [1] * N)
    (ia, sa), (ib, sb) = _tracks(0, area, GAP), _tracks(1, area, GAP)
    want = I.TrackReport.from_ids(inst, np.concatenate([ia, ib]), np.concatenate([sa, sb]))
    assert np.array_equal(rep.ids, want.ids) and np.array_equal(rep.started, want.started) and rep.as_rows() == want.as_rows()
    assert len(rep.tracks) == len(want.tracks) == int(sa[-1]) + int(sb[-1])
    assert any(t["seen"] < t["last"] - t["first"] + 1 for t in rep.tracks), "no track of the report bridges a gap"


@pytest.mark.parametrize("mode", list(C._MODES))
def test_segmenter_gap_0_is_the_segmenter_without_the_argument(mode):
    c = C._case("endovis18")
    s = c["seqs"][0]
    kw = dict(out="labels", out_size=SIZE, report="frame", instances=K, tracks=True, min_area=_min_area(), **C._MODES[mode])
    with torch.no_grad():
        zero = video.VideoSegmenter(c["m"], track_max_gap=0, **kw)
        got = [r[4].clone() for r in zero.segment_sequence(s["fr"])]
        plain = video.VideoSegmenter(c["m"], **kw)
        want = [r[4].clone() for r in plain.segment_sequence(s["fr"])]
    assert not zero.chain.state.memory and zero.chain.state.bytes == plain.chain.state.bytes == hip.load().stswin_track_state_bytes(*SIZE, K)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert any(not torch.equal(g, torch.from_numpy(w).cuda()) for g, w in zip(got, _tracks(0, kw["min_area"], GAP)[0])), "the gap changes nothing"


def test_segmenter_refusals():
    m = C._case("endovis18")["m"]
    base = dict(out="labels", report="frame", instances=8)
    for kwargs in (dict(track_max_gap=1), dict(tracks=True, track_max_gap=-1), dict(tracks=True, track_max_gap=1.0),
                   dict(tracks=True, track_max_gap=True), dict(tracks=True, track_max_gap=None), dict(tracks=True, track_max_gap=1000001)):
        with pytest.raises(StswinHipError, match="track_max_gap"):
            video.VideoSegmenter(m, **base, **kwargs)
    assert video.VideoSegmenter(m, **base, tracks=True, track_max_gap=3).track_max_gap == 3
    assert video.VideoSegmenter(m, **base, track_max_gap=0).track_max_gap == 0
