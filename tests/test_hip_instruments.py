"""stswin_label_moments / hip.label_moments and VideoSegmenter(report=...): every result is compared bit for bit (torch.equal) with
utils.instruments.label_moments, the numpy definition of the row."""
import numpy as np
import pytest
import torch

from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _want(labels, nc):
    return torch.from_numpy(I.label_moments(labels, nc))


def _check(labels, nc):
    got = hip.label_moments(_dev(labels), nc)
    assert got.dtype == torch.int64 and tuple(got.shape) == (labels.shape[0], nc, 10) and got.is_cuda
    want = _want(labels, nc)
    assert torch.equal(got.cpu(), want), (got.cpu() - want).nonzero()[:8].tolist()
    return want


def _blobs(n, H, W, nc, seed):
    """Piecewise-constant maps: a few rectangles and discs on background 0."""
    g = np.random.default_rng(seed)
    ys, xs = np.mgrid[:H, :W]
    lab = np.zeros((n, H, W), np.uint8)
    for f in range(n):
        for k in range(6):
            c = int(g.integers(1, max(nc, 2)))
            cy, cx = int(g.integers(0, H)), int(g.integers(0, W))
            r = int(g.integers(2, max(3, min(H, W) // 3)))
            if k % 2:
                lab[f][(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = c
            else:
                lab[f, max(cy - r, 0):cy + r // 2 + 1, max(cx - 2 * r, 0):cx + r + 1] = c
    return lab


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("nc", [1, 12, 64])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (3, 33, 130), (2, 3, 37)])
def test_random_labels(shape, nc):
    g = np.random.default_rng(nc + sum(shape))
    labels = g.integers(0, nc + 2, shape).astype(np.uint8)          # nc and nc + 1 are counted nowhere
    want = _check(labels, nc)
    assert int(want[:, :, 0].sum()) == int((labels < nc).sum())


def test_blob_maps_take_the_run_and_wave_paths():
    labels = _blobs(2, 64, 160, 12, seed=1)
    assert len(np.unique(labels)) >= 3
    _check(labels, 12)
    _check(labels, 2)                                                # most blobs are now labels >= nc
    _check(np.zeros((2, 64, 160), np.uint8), 12)                     # one label everywhere: every wave is uniform
    _check(np.full((1, 64, 160), 13, np.uint8), 12)                  # ... and it is counted nowhere


def test_checkerboard_changes_label_every_pixel():
    ys, xs = np.mgrid[:16, :64]
    labels = (3 + 2 * ((ys + xs) & 1)).astype(np.uint8)[None]
    _check(labels, 12)
    _check(np.ascontiguousarray(np.repeat(labels, 2, axis=2)[:, :, 1:97]), 12)      # runs of two, off the 16-pixel grid


def test_sums_past_32_bits():
    wide = np.full((1, 40, 16384), 5, np.uint8)
    want = _check(wide, 12)
    assert int(want[0, 5, 1]) > 2 ** 32 and int(want[0, 5, 4]) > 2 ** 36 and int(want[0, 5, 3]) > 2 ** 45
    tall = np.full((1, 2048, 8), 1, np.uint8)
    want = _check(tall, 2)
    assert int(want[0, 1, 5]) > 2 ** 34
    # the last rows and columns of the largest map the kernel takes: y^2 and x^2 at their largest
    edge = _dev(np.full((1, 16384, 16), 2, np.uint8))
    got = hip.label_moments(edge, 3).cpu()
    n = 16384
    assert got[0, 2].tolist() == [16 * n, n * 120, 16 * (n * (n - 1) // 2), n * 1240, 120 * (n * (n - 1) // 2),
                                  16 * ((n - 1) * n * (2 * n - 1) // 6), 16, n, 16, n]


def test_extents_corner_pixels_and_an_absent_class():
    labels = np.zeros((2, 37, 53), np.uint8)
    for y, x in ((0, 0), (0, 52), (36, 0), (36, 52)):
        labels[0, y, x] = 3
    labels[1, 10:20, 5:9] = 1
    want = _check(labels, 4)
    assert want[0, 3].tolist()[6:] == [53, 37, 53, 37] and int(want[0, 3, 0]) == 4
    assert not want[0, 2].any() and not want[1, 2].any() and not want[1, 3].any()          # absent: the row stays all zero
    assert want[1, 1].tolist()[6:] == [53 - 5, 37 - 10, 9, 20]


@pytest.mark.parametrize("W", [130, 128])
@pytest.mark.parametrize("offset", [1, 3, 8])
def test_any_pointer_alignment(offset, W):
    g = np.random.default_rng(offset + W)
    labels = _blobs(2, 19, W, 12, seed=offset + W)
    labels[g.random(labels.shape) < 0.05] = 7
    store = torch.zeros(offset + labels.size + 64, dtype=torch.uint8, device="cuda")
    view = store[offset:offset + labels.size].view(labels.shape)
    view.copy_(torch.from_numpy(labels))
    assert view.data_ptr() % 256 == offset and view.is_contiguous()
    assert torch.equal(hip.label_moments(view, 12).cpu(), _want(labels, 12))


def test_out_is_accumulated_never_cleared():
    a, b = _blobs(2, 33, 130, 12, seed=5)[:, None]
    da, db = _dev(a), _dev(b)
    ma, mb = _want(a, 12), _want(b, 12)
    out = hip.label_moments(da, 12)
    assert hip.label_moments(da, 12, out=out) is out
    twice = torch.cat([2 * ma[:, :, :6], ma[:, :, 6:]], dim=2)       # sums double, extents stay
    assert torch.equal(out.cpu(), twice)
    pool = torch.zeros(1, 12, 10, dtype=torch.int64, device="cuda")
    hip.label_moments(da, 12, out=pool)
    hip.label_moments(db, 12, out=pool)
    assert not torch.equal(ma, mb)
    assert torch.equal(pool.cpu(), torch.cat([(ma + mb)[:, :, :6], torch.maximum(ma, mb)[:, :, 6:]], dim=2))


def test_wrapper_refusals():
    labels = _dev(_blobs(2, 8, 16, 4, seed=2))
    ok = hip.label_moments(labels, 4).clone()
    out = torch.full((2, 4, 10), 99, dtype=torch.int64, device="cuda")
    bad_labels = (labels.long(), labels[0], labels.transpose(1, 2), labels.cpu(), labels[:0], labels.cpu().numpy())
    for lab in bad_labels:
        with pytest.raises(StswinHipError):
            hip.label_moments(lab, 4)
    for nc in (0, 65, -1, 4.0, None):
        with pytest.raises(StswinHipError):
            hip.label_moments(labels, nc)
    for o in (out.int(), out[:1], out[:, :3], out[:, :, :9], out.cpu(), out.transpose(0, 1), torch.zeros(2, 10, 4, dtype=torch.int64,
                                                                                                      device="cuda").transpose(1, 2)):
        with pytest.raises(StswinHipError):
            hip.label_moments(labels, 4, out=o)
    big = torch.zeros(2 * 40 * 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(StswinHipError, match="shares memory"):
        hip.label_moments(big.view(2, 40, 16), 4, out=big[:2 * 4 * 10 * 8].view(torch.int64).view(2, 4, 10))
    with pytest.raises(StswinHipError, match="16384"):
        hip.label_moments(torch.zeros(1, 1, 16385, dtype=torch.uint8, device="cuda"), 4)
    torch.cuda.synchronize()
    assert (out == 99).all(), "a refused call launched"
    assert torch.equal(hip.label_moments(labels, 4), ok)


def _raw():
    labels = _dev(_blobs(2, 8, 16, 4, seed=2))
    out = torch.full((2, 4, 10), 99, dtype=torch.int64, device="cuda")
    return hip.load().stswin_label_moments, labels, out, torch.cuda.current_stream().cuda_stream


def _untouched(out):
    torch.cuda.synchronize()
    assert (out == 99).all(), "a refused call launched"


def test_abi_refuses_sizes():
    fn, labels, out, st = _raw()
    p = lambda t: t.data_ptr()
    for n, H, W in ((0, 8, 16), (-1, 8, 16), (2, 0, 16), (2, 8, -16), (1, 16385, 1), (1, 1, 16385)):
        assert fn(p(labels), p(out), n, H, W, 4, st) == -1545
    _untouched(out)


def test_abi_refuses_null():
    fn, labels, out, st = _raw()
    assert fn(None, out.data_ptr(), 2, 8, 16, 4, st) == -1546
    assert fn(labels.data_ptr(), None, 2, 8, 16, 4, st) == -1546
    _untouched(out)


def test_abi_refuses_class_counts():
    fn, labels, out, st = _raw()
    for nc in (0, -3, 65):
        assert fn(labels.data_ptr(), out.data_ptr(), 2, 8, 16, nc, st) == -1547
    _untouched(out)
    out.zero_()
    assert fn(labels.data_ptr(), out.data_ptr(), 2, 8, 16, 4, st) == 0
    assert torch.equal(out.cpu(), _want(labels.cpu().numpy(), 4))
    assert "stswin_label_moments" in hip.declared_symbols() and hip.load().stswin_abi_version() == 1


def test_capturable_into_a_graph_with_its_clear():
    first = _blobs(2, 33, 130, 12, seed=7)
    labels = _dev(first)
    out = torch.zeros(2, 12, 10, dtype=torch.int64, device="cuda")
    hip.label_moments(labels, 12, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out.zero_()
        hip.label_moments(labels, 12, out=out)
    for seed in (8, 9):
        nxt = _blobs(2, 33, 130, 12, seed=seed)
        assert not np.array_equal(nxt, first)
        labels.copy_(torch.from_numpy(nxt))
        graph.replay()
        assert torch.equal(out.cpu(), _want(nxt, 12))
        assert torch.equal(out, hip.label_moments(labels, 12))      # eager


def test_one_full_size_frame():
    labels = _blobs(1, 1024, 1280, 12, seed=11)
    want = _check(labels, 12)
    assert int((want[0, :, 0] > 0).sum()) >= 3 and int(want[0, :, 0].sum()) == 1024 * 1280


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE = (72, 88)         # the frames' size and the output size (the model's input is 64 x 64): out="overlay" needs them equal
N = 10


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


def _frames(n, seed):
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (1, *SIZE, 3), dtype=np.int64)
    return np.clip(base + g.integers(-24, 25, (n, *SIZE, 3)), 0, 255).astype(np.uint8)


_CASES = {}


def _case(protocol):
    """Per protocol: the model, two sequences, an int64 ground truth, and the label maps of a plain out="labels" segmenter with their
    host moments - computed once, shared, never changed."""
    if protocol not in _CASES:
        m = _model(protocol, seed=4)
        nc = 9 if protocol == "cadis" else 12
        g = np.random.default_rng(17)
        seqs = []
        for s in range(2):
            fr = _frames(N, seed=40 + s)
            with torch.no_grad():
                res = video.VideoSegmenter(m, out="labels", out_size=SIZE, protocol=protocol).segment_sequence(fr)
            labels = np.stack([r.cpu().numpy() for r in res])
            seqs.append(dict(fr=fr, labels=torch.from_numpy(labels), moments=torch.from_numpy(I.label_moments(labels, nc)),
                             gt=torch.from_numpy(g.integers(0, nc - 1, (N, *SIZE)))))
        assert len(np.unique(seqs[0]["labels"].numpy())) >= 2, "the random model predicts one class: the moments test little"
        _CASES[protocol] = dict(m=m, nc=nc, seqs=seqs)
    return _CASES[protocol]


_MODES = {"eager": {}, "batch4": dict(batch=4), "graph": dict(graph=True)}


def _own_moments(r, nc):
    """The last element of a report="frame" result against the host moments of the result's own labels."""
    assert isinstance(r, tuple) and r[-1].is_cuda and r[-1].dtype == torch.int64 and tuple(r[-1].shape) == (nc, 10)
    return torch.equal(r[-1].cpu(), _want(r[0].cpu().numpy()[None], nc)[0])


@pytest.mark.parametrize("mode", list(_MODES))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_frame_report(protocol, mode):
    c = _case(protocol)
    m, nc = c["m"], c["nc"]
    kw = dict(out_size=SIZE, protocol=protocol, report="frame", **_MODES[mode])
    with torch.no_grad():
        seg = video.VideoSegmenter(m, out="labels", **kw)
        for s in c["seqs"]:                                              # the second sequence follows a reset(): graph replays go on
            got = seg.segment_sequence(s["fr"])
            assert len(got) == N
            for f, r in enumerate(got):
                assert len(r) == 2 and torch.equal(r[0].cpu(), s["labels"][f]), f
                assert _own_moments(r, nc) and torch.equal(r[1].cpu(), s["moments"][f]), f
        # with int64 ground truth the labels come from the scoring launches
        s = c["seqs"][0]
        got = seg.segment_sequence(s["fr"], gt=s["gt"])
        plain = video.VideoSegmenter(m, out="labels", out_size=SIZE, protocol=protocol, **_MODES[mode]).segment_sequence(s["fr"], gt=s["gt"])
        for f, (r, p) in enumerate(zip(got, plain)):
            if protocol == "cadis":                                      # the labels alone, then the moments
                assert len(r) == 2 and torch.equal(r[0], p)
            else:                                                        # (labels, dice, iou, moments)
                assert len(r) == 4 and torch.equal(r[0], p[0]) and r[1] == p[1] and r[2] == p[2]
            assert _own_moments(r, nc) and torch.equal(r[-1].cpu(), s["moments"][f]), f
        # out="overlay": the moments are those of the labels, not of the picture
        ov = video.VideoSegmenter(m, out="overlay", **kw).segment_sequence(s["fr"])
        ref = video.VideoSegmenter(m, out="overlay", out_size=SIZE, protocol=protocol, **_MODES[mode]).segment_sequence(s["fr"])
        for f, (r, p) in enumerate(zip(ov, ref)):
            assert len(r) == 2 and tuple(r[0].shape) == (*SIZE, 3) and torch.equal(r[0], p), f
            assert torch.equal(r[1].cpu(), s["moments"][f]), f


def test_segmenter_graph_results_are_views_until_the_next_push():
    c = _case("endovis18")
    s = c["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, report="frame", graph=True)
        seen = {}
        for f in range(N):
            for g, r in seg.push(s["fr"][f]):
                seen[g] = (r[0].clone(), r[1].clone())                   # the last replayed result is a view of the graph's buffers
        for g, r in seg.finish():
            seen[g] = (r[0].clone(), r[1].clone())
    assert sorted(seen) == list(range(N))
    for f in range(N):
        assert torch.equal(seen[f][0].cpu(), s["labels"][f]) and torch.equal(seen[f][1].cpu(), s["moments"][f]), f


@pytest.mark.parametrize("protocol,mode", [("endovis18", "eager"), ("endovis18", "batch4"), ("endovis18", "graph"), ("cadis", "graph")])
def test_segmenter_deferred_report(protocol, mode):
    c = _case(protocol)
    a, b = c["seqs"]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, protocol=protocol, report="deferred", min_area=3, **_MODES[mode])
        empty = seg.instrument_report()
        assert len(empty) == 0 and empty.presence().shape == (0, c["nc"])
        got_a = seg.segment_sequence(a["fr"])
        got_b = seg.segment_sequence(b["fr"], gt=b["gt"])                  # scored frames are logged as well
    for f in range(N):                                                    # the results are unchanged
        assert isinstance(got_a[f], torch.Tensor) and torch.equal(got_a[f].cpu(), a["labels"][f])
    rep = seg.instrument_report(names=[f"class {k}" for k in range(c["nc"])])
    assert rep.sequences == [0] * N + [1] * N and rep.frames == list(range(N)) * 2         # ordered by sequence and frame
    assert torch.equal(torch.from_numpy(rep.moments), torch.cat([a["moments"], b["moments"]]))
    want = I.InstrumentReport.from_moments(rep.moments, SIZE, min_area=3)
    assert rep.size == SIZE and rep.min_area == 3 and np.array_equal(rep.presence(), want.presence())
    assert np.array_equal(rep.presence(), rep.moments[:, :, 0] >= 3) and rep.as_rows()[0]["name"] == "class 0"
    assert np.array_equal(rep.box, want.box, equal_nan=True) and np.array_equal(rep.angle, want.angle, equal_nan=True)
    seg.reset_metrics()
    assert len(seg.instrument_report()) == 0
    with torch.no_grad():
        seg.segment_sequence(b["fr"])
    again = seg.instrument_report()
    assert again.sequences == [0] * N and torch.equal(torch.from_numpy(again.moments), b["moments"])


def test_segmenter_deferred_log_grows_past_its_first_rows():
    c = _case("endovis18")
    a = c["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="overlay", report="deferred", batch=4)
        for _ in range(7):                                                # 70 rows: past the log's first 64
            seg.segment_sequence(a["fr"])
    rep = seg.instrument_report()
    assert len(rep) == 70 and rep.sequences == [s for s in range(7) for _ in range(N)] and rep.frames == list(range(N)) * 7
    assert torch.equal(torch.from_numpy(rep.moments), a["moments"].repeat(7, 1, 1))


def test_segmenter_report_refusals():
    m = _case("endovis18")["m"]
    for kwargs in (dict(out="logits", report="frame"), dict(report="deferred"), dict(out="labels", report="later"),
                   dict(out="labels", report=True), dict(out="labels", report="frame", min_area=0),
                   dict(out="labels", report="deferred", min_area=-2), dict(out="labels", min_area=1.5)):
        with pytest.raises(StswinHipError):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(out="labels"), dict(out="labels", report="frame"), dict(out="logits")):
        with pytest.raises(StswinHipError, match="deferred"):
            video.VideoSegmenter(m, **kwargs).instrument_report()
