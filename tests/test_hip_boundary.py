"""hip.boundary_counts (exact contour distances per class: what NSD and the Hausdorff distance are made of) and
VideoSegmenter(boundary="deferred") against the numpy definition utils.boundary.boundary_counts: everything torch.equal.  The shapes are
placed around the kernel's geometry (stswin_boundary_geometry)."""
import numpy as np
import pytest
import torch

import boundary_cases as BC
import test_hip_components as C
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import boundary as B

pytestmark = pytest.mark.gpu

GEO = hip.boundary_geometry()
TH, TW, COLS, SEG = GEO
SHAPES = [(1, 1, 1), (2, 1, TW + 1), (1, TH + 1, 1), (2, TH + 1, TW + 1), (3, 2 * TH + 3, 3 * TW + 5), (1, SEG + TH + 3, TW + 1),
          (2, TH + 2, 2 * TW)]            # the last one: W % 16 == 0 on an aligned pointer
BINS = (2, 16, 256)
NCS = (2, 5, 64)
FILL = 77


def _padded(shape, dtype, offset=0):
    """A tensor of `shape` whose bytes start `offset` bytes behind a 512-byte boundary, inside a buffer of FILL: (view, buffer)."""
    n = int(np.prod(shape))
    size = torch.empty(0, dtype=dtype).element_size()
    assert offset % size == 0 and 512 % size == 0
    buf = torch.full((n + 1024 // size + offset // size,), FILL, dtype=dtype, device="cuda")
    lo = (-buf.data_ptr() % 512) // size + 512 // size + offset // size
    return buf[lo:lo + n].view(shape), buf


def _sentinels_hold(view, buf):
    n, lo = view.numel(), view.storage_offset()
    return bool((buf[:lo] == FILL).all()) and bool((buf[lo + n:] == FILL).all())


def _scratch(n, H, W, nc):
    """The workspace formula of the header: the class table uint64 [2][n][S][W] and the maps' classes uint64 [2][n], the planes uint16 [2][n][nc][H][W], the codes."""
    return 16 * n * (-(-H // SEG) * W + 1) + 2 * n * H * W * (2 * nc + 1)


def _skips(nc):
    return ((), (0,), (nc - 1,))


def _check(gt, pred, nc, bins, skip=(), offset=0, want=None):
    """One call on the pair (numpy), pred placed `offset` bytes off a 512-byte boundary, every buffer between sentinels: equal to the
    definition in full, the inputs untouched, a second call with the wrapper's own buffers the same bits."""
    n, H, W = gt.shape
    g, g_buf = _padded(gt.shape, torch.int64)
    p, p_buf = _padded(pred.shape, torch.uint8, offset)
    g.copy_(torch.from_numpy(gt))
    p.copy_(torch.from_numpy(pred))
    assert p.data_ptr() % 16 == offset % 16
    out, out_buf = _padded((n, nc, 2, 2 + bins), torch.int32)
    ws, ws_buf = _padded((hip.boundary_scratch(n, H, W, nc),), torch.uint8)
    got = hip.boundary_counts(g, p, nc, bins, skip, out=out, workspace=ws)
    assert got is out
    if want is None:
        want = B.boundary_counts(gt, pred, nc, bins, skip)
    bad = (out.cpu() != torch.from_numpy(want)).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), out.cpu()[tuple(bad[0])].item(), want[tuple(bad[0].tolist())])
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    assert all(_sentinels_hold(v, b) for v, b in ((g, g_buf), (p, p_buf), (out, out_buf), (ws, ws_buf)))
    assert torch.equal(g.cpu(), torch.from_numpy(gt)) and torch.equal(p.cpu(), torch.from_numpy(pred)), "an input changed"
    again = hip.boundary_counts(g, p, nc, bins, skip)
    assert again.dtype == torch.int32 and tuple(again.shape) == (n, nc, 2, 2 + bins) and torch.equal(again, out)
    return want


def test_geometry_is_the_library_s():
    geo = hip.load().stswin_boundary_geometry
    assert (geo(0), geo(1), geo(2), geo(3)) == GEO and geo(4) == -1 and geo(-1) == -1
    assert SEG % TH == 0 and SHAPES[5][1] > SEG + TH                       # the tile edges in y include a segment edge of the column pass
    assert SHAPES[4][2] > 2 * 64 + 9                                       # a far pair takes the wave's search past its second step
    # the grid below takes both bodies of the query pass: the LDS copy of the rows, and direct atomics above 8192 words
    assert 64 * (2 + 256) > 8192 >= 64 * (2 + 16) and 5 * (2 + 256) <= 8192


def _pattern_guards(name, gt, pred, nc, want16):
    """What a pattern is for, on the definition's rows at 16 bins without a skip set."""
    n, H, W = gt.shape
    top, a = nc - 1, 1 % nc
    if name == "far":
        d2 = (H - 1) ** 2 + (W - 1) ** 2
        assert want16[:, top, :, 0].tolist() == [[1, 1]] * n
        assert want16[:, top, :, 1].tolist() == [[d2, d2]] * n
        tail = B.boundary_counts(gt, pred, nc, 2)[:, top, :, -1]
        assert (tail > 0).all() if H * W > 1 else not tail.any()
        if d2 >= 15 * 15:
            assert (want16[:, top, :, -1] == 1).all()
    if name == "absent_pred":
        assert (want16[:, top, 0, 0] > 0).all() and (want16[:, top, 1, 0] == 0).all() and (want16[:, top, :, 1] == -1).all()
        assert not want16[:, top, :, 2:].any()
    if name == "absent_gt":
        assert (want16[:, top, 1, 0] > 0).all() and (want16[:, top, 0, 0] == 0).all() and (want16[:, top, :, 1] == -1).all()
        assert not want16[:, top, :, 2:].any()
    if name == "tile_edges" and (H > TH or W > TW):
        crossing = 0
        for c in {a, 2 if nc > 2 else a}:
            own, other = np.argwhere(B.contour(gt[0] == c)), np.argwhere(B.contour(pred[0] == c))
            if not len(own) or not len(other):                           # (a map of one tile row or column has edges in one direction)
                continue
            q = other[BC.nearest_pairs(own, other)]
            crossing += int(((own[:, 0] // TH != q[:, 0] // TH) | (own[:, 1] // TW != q[:, 1] // TW)).sum())
        assert crossing > 0, "no nearest pair lies across a tile edge"
    if name == "blobs" and H > TH and W > TW:
        both = (want16[:, :, 0, 0] > 0) & (want16[:, :, 1, 0] > 0) & (want16[:, :, :, 1].max(axis=2) > 1)
        assert (both.sum(axis=1) >= 2).all(), both.sum(axis=1)
        assert want16[..., -1].sum() > 0
    if name == "checker_vs_dot" and H * W > 2:
        assert want16[0, a, 0, 0] == (H * W) // 2 and want16[0, a, 1, 0] == 1
    if name == "full":
        assert want16[0, a, 0, 0] == (2 * (H + W) - 4 if H > 1 and W > 1 else H * W)
    if name == "out_of_range" and H * W >= 70:
        assert (gt == 255).any() and (gt == -1).any() and (gt == nc).any() and (pred == 255).any()


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_pattern(shape, nc):
    n, H, W = shape
    pats = BC.patterns(n, H, W, nc, GEO, seed=H + W)
    assert len(pats) == 10
    for name, (gt, pred) in pats.items():
        staged = B.contour_d2(gt, pred, nc)                                # the definition's half that bins and skip do not enter
        for bins in BINS:
            for skip in _skips(nc):
                want = _check(gt, pred, nc, bins, skip, want=B.counts_from_d2(*staged, bins, skip))
                if bins == 16 and skip == ():
                    _pattern_guards(name, gt, pred, nc, want)
                if skip:
                    assert not want[:, list(skip)].any()


@pytest.mark.parametrize("offset", [1, 2, 3, 8])
def test_maps_off_a_16_byte_boundary(offset):
    n, H, W = SHAPES[-1]
    pats = BC.patterns(n, H, W, 5, GEO, seed=offset)
    for name in ("blobs", "tile_edges", "out_of_range"):
        want = _check(*pats[name], 5, 16, (0,), offset)
        _check(*pats[name], 5, 16, (0,), 0, want)                          # ... and on it: the same maps, the same rows


def test_out_and_workspace_are_reused_over_dirty_contents():
    n, H, W, nc, bins = 3, 2 * TH + 3, TW + 16, 5, 16
    need = hip.boundary_scratch(n, H, W, nc)
    assert need == _scratch(n, H, W, nc) == hip.load().stswin_boundary_scratch(n, H, W, nc)
    assert hip.boundary_scratch(1, 1, 1, 1) == 32 + 6 and hip.boundary_scratch(2, 540, 960, 26) == 16 * 2 * (9 * 960 + 1) + 2 * 2 * 540 * 960 * 53
    out = torch.full((n, nc, 2, 2 + bins), FILL, dtype=torch.int32, device="cuda")
    ws = torch.full((need + 64,), FILL, dtype=torch.uint8, device="cuda")
    for k, (name, (gt, pred)) in enumerate(BC.patterns(n, H, W, nc, GEO, seed=9).items()):
        got = hip.boundary_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), nc, bins, (0,), out=out, workspace=ws)
        assert torch.equal(got.cpu(), torch.from_numpy(B.boundary_counts(gt, pred, nc, bins, (0,)))), name
        assert bool((ws[-64:] == FILL).all())
        ws[:-64].fill_((37 * k + 255) % 256)                               # whatever the workspace holds: nothing in it survives
        out.fill_(-(k + 1))


def test_the_call_is_capturable():
    n, H, W, nc, bins = 2, TH + 5, TW + 32, 5, 16
    pats = BC.patterns(n, H, W, nc, GEO, seed=4)
    gt = torch.empty(n, H, W, dtype=torch.int64, device="cuda")
    pred = torch.empty(n, H, W, dtype=torch.uint8, device="cuda")
    out = torch.full((n, nc, 2, 2 + bins), FILL, dtype=torch.int32, device="cuda")
    ws = torch.empty(hip.boundary_scratch(n, H, W, nc), dtype=torch.uint8, device="cuda")
    gt.copy_(torch.from_numpy(pats["blobs"][0]))
    pred.copy_(torch.from_numpy(pats["blobs"][1]))
    hip.boundary_counts(gt, pred, nc, bins, out=out, workspace=ws)           # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.boundary_counts(gt, pred, nc, bins, out=out, workspace=ws)
    for name in ("checker_vs_dot", "full", "blobs", "tile_edges", "absent_pred", "far"):
        gt.copy_(torch.from_numpy(pats[name][0]))
        pred.copy_(torch.from_numpy(pats[name][1]))
        graph.replay()
        assert torch.equal(out.cpu(), torch.from_numpy(B.boundary_counts(*pats[name], nc, bins))), name


def _buffers(n, H, W, nc, bins):
    return (torch.full((n, nc, 2, 2 + bins), FILL, dtype=torch.int32, device="cuda"),
            torch.full((hip.boundary_scratch(n, H, W, nc),), FILL, dtype=torch.uint8, device="cuda"))


def test_wrapper_refusals():
    n, H, W, nc, bins = 2, 8, 16, 3, 4
    hg, hp = BC.patterns(n, H, W, nc, GEO)["blobs"]
    gt, pred = torch.from_numpy(hg).cuda(), torch.from_numpy(hp).cuda()
    out, ws = _buffers(n, H, W, nc, bins)

    def call(g=gt, p=pred, nc=nc, bins=bins, skip=(), **kw):
        return hip.boundary_counts(g, p, nc, bins, skip, **kw)

    for g in (gt.int(), gt.float(), gt[0], gt[None], gt[:, :, ::2], gt.cpu(), hg, gt[:0]):
        with pytest.raises(StswinHipError, match="gt"):
            call(g=g, out=out, workspace=ws)
    for p in (pred.long(), pred.float(), pred[0], pred[:, :, ::2], pred.cpu(), hp, pred[:1], pred[:, :4]):
        with pytest.raises(StswinHipError, match="pred"):
            call(p=p, out=out, workspace=ws)
    for bad in (0, 65, -1, 3.0, True, None):
        with pytest.raises(StswinHipError, match="nc"):
            call(nc=bad)
    for bad in (1, 0, 257, 4.0, True, None):
        with pytest.raises(StswinHipError, match="bins"):
            call(bins=bad)
    for bad in ((64,), (-1,), (1.0,), (True,), "a"):
        with pytest.raises(StswinHipError, match="skip"):
            call(skip=bad)
    for bad in (out.long(), out[:1], out[:, :, :1], out.view(n, nc, 2 * (2 + bins)), out.cpu(), (out,), out[:, :, :, :1].expand(n, nc, 2, 2 + bins)):
        with pytest.raises(StswinHipError, match="out"):
            call(out=bad, workspace=ws)
    for w in (ws[:-1], ws.view(torch.int16), ws.cpu(), ws.view(2, -1), torch.full((ws.numel() + 4,), FILL, dtype=torch.uint8, device="cuda")[4:],
              torch.full((ws.numel() + 4,), FILL, dtype=torch.uint8, device="cuda")[1:]):
        with pytest.raises(StswinHipError, match="workspace"):
            call(out=out, workspace=w)
    big = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
    as_gt, as_pred = big[:n * H * W * 8].view(torch.int64).view(n, H, W), big[:n * H * W].view(n, H, W)
    as_out = big[:out.numel() * 4].view(torch.int32).view(out.shape)
    for kw in (dict(g=as_gt, p=as_pred), dict(g=as_gt, out=as_out, workspace=ws), dict(p=as_pred, out=out, workspace=big),
               dict(out=as_out, workspace=big), dict(g=as_gt, out=out, workspace=big)):
        with pytest.raises(StswinHipError, match="shares memory"):
            call(**kw)
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (out, ws, big)), "a refused call launched"
    assert torch.equal(call(out=out, workspace=ws).cpu(), torch.from_numpy(B.boundary_counts(hg, hp, nc, bins)))
    for shape in ((0, 8, 8, 2), (1, 16385, 8, 2), (1, 8, 0, 2)):
        with pytest.raises(StswinHipError, match="maps of"):
            hip.boundary_scratch(*shape)
    with pytest.raises(StswinHipError, match="nc"):
        hip.boundary_scratch(1, 8, 8, 65)


def test_c_abi():
    lib = hip.load()
    assert lib.stswin_abi_version() == 1
    n, H, W, nc, bins = 2, 8, 16, 3, 4
    hg, hp = BC.patterns(n, H, W, nc, GEO)["blobs"]
    gt, pred = torch.from_numpy(hg).cuda(), torch.from_numpy(hp).cuda()
    out, ws = _buffers(n, H, W, nc, bins)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    fn = lib.stswin_boundary_counts

    def run(g=p(gt), m=p(pred), o=p(out), n=n, H=H, W=W, nc=nc, bins=bins, skip=0, w=p(ws), wbytes=ws.numel()):
        return fn(g, m, o, n, H, W, nc, bins, skip, w, wbytes, st)

    for kw in (dict(n=0), dict(n=-1), dict(H=0), dict(W=-16), dict(H=16385), dict(W=16385)):
        assert run(**kw) == -1870, kw
    scratch = lib.stswin_boundary_scratch
    assert scratch(1, 16385, 1, 2) == -1870 and scratch(0, 8, 16, 2) == -1870 and scratch(1, 8, 16, 0) == -1872 and scratch(1, 8, 16, 65) == -1872
    for kw in (dict(g=None), dict(m=None), dict(o=None), dict(w=None)):
        assert run(**kw) == -1871, kw
    for bad in (0, -1, 65):
        assert run(nc=bad) == -1872
    for bad in (1, 0, -1, 257):
        assert run(bins=bad) == -1873
    need = scratch(n, H, W, nc)
    assert need == hip.boundary_scratch(n, H, W, nc) == _scratch(n, H, W, nc) == ws.numel()
    assert run(wbytes=need - 1) == -1874 and run(w=p(ws) + 4) == -1874 and run(w=p(ws) + 2) == -1874 and run(w=p(ws) + 1) == -1874
    assert run(g=p(gt) + 4) == -1875 and run(g=p(gt) + 1) == -1875 and run(o=p(out) + 2) == -1875 and run(o=p(out) + 1) == -1875
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (out, ws)), "a refused call launched"
    assert run() == 0
    assert torch.equal(out.cpu(), torch.from_numpy(B.boundary_counts(hg, hp, nc, bins)))
    assert run(skip=0b101) == 0                                              # bits 0 and 2; bits from nc on are ignored
    assert torch.equal(out.cpu(), torch.from_numpy(B.boundary_counts(hg, hp, nc, bins, (0, 2))))
    assert run(skip=-1 << 3) == 0
    assert torch.equal(out.cpu(), torch.from_numpy(B.boundary_counts(hg, hp, nc, bins)))
    assert run(m=p(pred) + 1, n=1) == 0                                     # pred at any address


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE, N = C.SIZE, C.N
SBINS = 16
_GT = {}


def _gt(protocol):
    """Per protocol a ground truth [2 sequences][N][*SIZE] of blobs: the plain segmenter's own label maps moved by (2, 3) pixels, an
    ellipse of class 1 over them and, every third frame, a second one of class 2 - close to the prediction along most contours and
    far from it at others.  Computed once, never changed."""
    if protocol not in _GT:
        c = C._case(protocol)
        both = []
        for s, q in enumerate(c["seqs"]):
            gt = np.roll(q["labels"].numpy().astype(np.int64), (2, 3), axis=(1, 2))
            for f in range(N):
                gt[f][BC._ellipse(*SIZE, 20 + f + 5 * s, 30 + 2 * f, 6, 9)] = 1
                if f % 3 == 0:
                    gt[f][BC._ellipse(*SIZE, 55, 60 - f, 5, 5)] = 2
            both.append(gt)
        _GT[protocol] = both
    return _GT[protocol]


def _same_result(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same_result(x, y) for x, y in zip(a, b))
    return a == b


def _label_of(r):
    return (r[0] if isinstance(r, tuple) else r).cpu().numpy()


@pytest.mark.parametrize("form", ["int64", "table"])
@pytest.mark.parametrize("mode", list(C._MODES))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_deferred_boundary(protocol, mode, form):
    c = C._case(protocol)
    nc, skip, gts = c["nc"], c["skip"], _gt(protocol)
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, **C._MODES[mode])
    if protocol == "endovis18" and mode != "eager":
        kw["scores"] = "deferred"                                           # (eager: scores="frame", the tuples with dice and iou)
    if form == "table":
        kw["gt_table"] = np.arange(256, dtype=np.uint8)
        gts = [g.astype(np.uint8) for g in gts]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], boundary="deferred", boundary_bins=SBINS, **kw)
        assert seg.boundary_skip == skip and len(seg.boundary_scores()) == 0
        plain = video.VideoSegmenter(c["m"], **kw)
        got, want = [], []
        for q, gt in zip(c["seqs"], gts):
            got += seg.segment_sequence(q["fr"], gt=torch.from_numpy(gt))
            want += plain.segment_sequence(q["fr"], gt=torch.from_numpy(gt))
    assert len(got) == len(want) == 2 * N and all(_same_result(a, b) for a, b in zip(got, want)), "the results changed"
    if protocol == "cadis":
        assert np.array_equal(seg.confusion_matrix(), plain.confusion_matrix()) and seg.confusion_matrix().sum() > 0
    elif kw.get("scores") == "deferred":
        a, b = seg.endo_scores(), plain.endo_scores()
        assert a.count == b.count == 2 * N and a.dices == b.dices and a.ious == b.ious and a.frames == b.frames and a.sequences == b.sequences
    labels = np.stack([_label_of(r) for r in want])
    assert np.array_equal(labels, np.concatenate([q["labels"].numpy() for q in c["seqs"]]))
    counts = B.boundary_counts(np.concatenate(gts).astype(np.int64), labels, nc, SBINS, skip)
    ref = B.BoundaryScores.from_counts(counts, [0] * N + [1] * N, list(range(N)) * 2)
    names = [f"class {k}" for k in range(nc)]
    res = seg.boundary_scores(names=names)
    assert res.sequences == [0] * N + [1] * N and res.frames == list(range(N)) * 2 and len(res) == 2 * N
    assert np.array_equal(res.counts, ref.counts)
    assert res.nsd(2) == ref.nsd(2) and res.hausdorff() == ref.hausdorff() and res.hausdorff_percentile(95) == ref.hausdorff_percentile(95)
    assert res.as_rows() == ref.as_rows(names=names) and res.as_rows()[0]["name"].startswith("class ")
    # the guard: the random model's labels against this ground truth score something in between
    between = {cl for row in ref.nsd(2) for cl, v in row if 0 < v < 1}
    assert len(between) >= 2, between
    with torch.no_grad():                                                  # reset() keeps the log, reset_metrics() clears it
        seg.reset()
        assert len(seg.boundary_scores()) == 2 * N
        seg.reset_metrics()
        assert len(seg.boundary_scores()) == 0
        seg.segment_sequence(c["seqs"][1]["fr"], gt=torch.from_numpy(gts[1]))
    res = seg.boundary_scores()
    assert res.sequences == [0] * N and res.frames == list(range(N)) and np.array_equal(res.counts, ref.counts[N:])


def test_segmenter_boundary_on_overlays_and_frames_without_gt():
    c = C._case("endovis18")
    q, gt = c["seqs"][0], _gt("endovis18")[0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="overlay", boundary="deferred", boundary_bins=SBINS, boundary_skip=(0, 3))
        plain = video.VideoSegmenter(c["m"], out="overlay")
        assert all(_same_result(a, b) for a, b in zip(seg.segment_sequence(q["fr"]), plain.segment_sequence(q["fr"])))
        assert len(seg.boundary_scores()) == 0                               # no gt, no row
        got, want = seg.segment_sequence(q["fr"], gt=torch.from_numpy(gt)), plain.segment_sequence(q["fr"], gt=torch.from_numpy(gt))
    assert all(_same_result(a, b) for a, b in zip(got, want))
    res = seg.boundary_scores()
    assert res.sequences == [0] * N and res.frames == list(range(N))
    assert np.array_equal(res.counts, B.boundary_counts(gt, q["labels"].numpy(), c["nc"], SBINS, (0, 3)))


def test_segmenter_boundary_refusals():
    m = C._case("endovis18")["m"]
    for kwargs in (dict(out="logits", boundary="deferred"), dict(out="labels", boundary="frame"), dict(out="labels", boundary=True),
                   dict(out="labels", boundary_bins=16), dict(out="labels", boundary="deferred", boundary_bins=1),
                   dict(out="labels", boundary="deferred", boundary_bins=257), dict(out="labels", boundary="deferred", boundary_bins=16.0),
                   dict(out="labels", boundary_skip=(0,)), dict(out="labels", boundary="deferred", boundary_skip=(64,))):
        with pytest.raises(StswinHipError, match="boundary"):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(out="labels"), dict(out="labels", scores="deferred"), dict(out="logits")):
        with pytest.raises(StswinHipError, match="boundary"):
            video.VideoSegmenter(m, **kwargs).boundary_scores()
    seg = video.VideoSegmenter(m, out="overlay", boundary="deferred")
    assert seg.boundary == "deferred" and seg.boundary_bins == 32 and seg.boundary_skip == (0,)
    cadis = C._case("cadis")
    assert video.VideoSegmenter(cadis["m"], out="labels", protocol="cadis", boundary="deferred").boundary_skip == (cadis["nc"] - 1,)
