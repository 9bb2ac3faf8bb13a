"""hip.label_components (connected instances of a label map and their moments rows) and VideoSegmenter(instances=K) against the numpy
definition utils.instruments.label_components: everything torch.equal, at both connectivities, truncation included.  The shapes are
placed around the kernel's tile and raster chunk (hip.CC_TILE, hip.CC_CHUNK)."""
import numpy as np
import pytest
import torch

from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I

pytestmark = pytest.mark.gpu

TH, TW = hip.CC_TILE
CHUNK = hip.CC_CHUNK
CONN = [4, 8]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _want(labels, nc, conn, skip=(), K=1024):
    return tuple(torch.from_numpy(t) for t in I.label_components(labels, nc, conn, skip, K))


def _same(got, want):
    for g, w, what in zip(got, want, ("components", "rows", "total")):
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), what
        assert torch.equal(g.cpu(), w), (what, (g.cpu() != w).nonzero()[:8].tolist())


def _check(labels, nc, conn, skip=(), K=1024):
    got = hip.label_components(_dev(labels), nc, conn, skip, K)
    assert all(t.is_cuda for t in got)
    want = _want(labels, nc, conn, skip, K)
    _same(got, want)
    return want


def _noise(shape, p, seed, classes=3):
    g = np.random.default_rng(seed)
    return np.where(g.random(shape) < p, g.integers(1, classes + 1, shape), 0).astype(np.uint8)


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
def test_geometry_constants_are_the_library_s():
    geo = hip.load().stswin_label_components_geometry
    assert (geo(0), geo(1)) == hip.CC_TILE and geo(2) == hip.CC_CHUNK and geo(3) == -1
    assert (CHUNK + 1) % 3 == 0, "the chunk + 1 shape below needs another factorisation"


SHAPES = [(1, 1, 1), (2, 1, TW + 1), (1, TH + 1, 1), (2, TH + 1, TW + 1), (3, 2 * TH + 3, 3 * TW + 5), (1, 3, (CHUNK + 1) // 3)]


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("nc", [1, 12, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_labels(shape, nc, conn):
    g = np.random.default_rng(nc + sum(shape))
    labels = g.integers(0, nc + 2, shape).astype(np.uint8)         # nc and nc + 1 belong to no component
    want = _check(labels, nc, conn)                                # (the larger shapes hold more than 1024 components: the first 1024)
    assert int((want[0] >= 0).sum()) == int((labels < nc).sum())


@pytest.mark.parametrize("conn", CONN)
def test_noise_on_the_three_by_three_tile_shape_stays_under_1024(conn):
    labels = _noise(SHAPES[4], 0.05, seed=5)
    want = _check(labels, 4, conn, skip=(0,))
    assert 16 < int(want[2].min()) and int(want[2].max()) < 1024
    cut = _check(labels, 4, conn, skip=(0,), K=16)                  # truncation keeps the first 16, whatever ran first
    assert torch.equal(cut[1], want[1][:, :16]) and torch.equal(cut[2], want[2]) and torch.equal(cut[0], want[0])


def _spiral(H, W):
    """A rectangular spiral one pixel wide, turns two pixels apart, from the outer corner inwards."""
    lab = np.zeros((H, W), np.uint8)
    inside = lambda v, u: 0 <= v < H and 0 <= u < W
    y, x, dy, dx = 0, 0, 0, 1
    lab[0, 0] = 1
    while True:
        moved = False
        while inside(y + dy, x + dx) and not lab[y + dy, x + dx] and not (inside(y + 2 * dy, x + 2 * dx) and lab[y + 2 * dy, x + 2 * dx]):
            y, x = y + dy, x + dx           # walk on while the pixel after the next is free: the turns stay one pixel apart
            lab[y, x] = 1
            moved = True
        if not moved:
            return lab[None]
        dy, dx = dx, -dy                    # right -> down -> left -> up


@pytest.mark.parametrize("conn", CONN)
def test_spiral_through_many_tiles_is_one_component(conn):
    H, W = 70, 150
    assert H >= 3 * TH and W > 2 * TW
    labels = _spiral(H, W)
    want = _check(labels, 2, conn, skip=(0,))
    assert int(want[2][0]) == 1 and int(want[1][0, 0, 2]) == int(labels.sum()) > 1000
    _check(labels, 2, conn)                                          # the gaps between the turns are a second spiral


@pytest.mark.parametrize("conn", CONN)
def test_comb_rings_and_a_tile_corner(conn):
    H, W = 2 * TH + 5, 2 * TW + 9
    comb = np.zeros((1, H, W), np.uint8)
    comb[0, :, ::2] = 3
    comb[0, H - 1, :] = 3                                            # the teeth join only in the last row
    want = _check(comb, 4, conn, skip=(0,))
    assert int(want[2][0]) == 1
    want = _check(comb, 4, conn)                                     # ... and the gaps between them do not join at all
    assert int(want[2][0]) == 1 + W // 2
    ys, xs = np.mgrid[:H, :W]
    rings = (1 + (np.maximum(abs(ys - H // 2), abs(xs - W // 2)) // 3) % 2).astype(np.uint8)[None]
    want = _check(rings, 3, conn)
    assert int(want[2][0]) > H // 6                                  # (the outer rings are cut into two by the frame)
    for dx in (-1, 0):                                               # two pixels that touch only across a tile corner, either diagonal
        corner = np.zeros((1, H, W), np.uint8)
        corner[0, TH - 1, TW + dx] = corner[0, TH, TW - 1 - dx] = 2
        want = _check(corner, 3, conn, skip=(0,))
        assert int(want[2][0]) == (1 if conn == 8 else 2)


@pytest.mark.parametrize("conn", CONN)
def test_frames_stay_apart(conn):
    labels = np.full((2, TH + 3, TW + 3), 4, np.uint8)
    want = _check(labels, 5, conn, K=4)
    assert want[2].tolist() == [1, 1] and want[1][:, 0, 1].tolist() == [0, 0]         # frame-local first pixel
    assert want[1][:, 0, 2].tolist() == [(TH + 3) * (TW + 3)] * 2 and not want[0].any()


def test_checkerboard():
    ys, xs = np.mgrid[:16, :64]
    labels = (1 + ((ys + xs) & 1)).astype(np.uint8)[None]
    want = _check(labels, 3, 8)
    assert int(want[2][0]) == 2 and want[1][0, :2, 2].tolist() == [512, 512]
    full = _check(labels, 3, 4)
    assert int(full[2][0]) == 1024 and bool((full[1][0, :, 2] == 1).all())              # K = 1024 exactly full
    assert torch.equal(full[0][0].reshape(-1), torch.arange(1024, dtype=torch.int32))
    cut = _check(labels, 3, 4, K=16)
    assert torch.equal(cut[1], full[1][:, :16]) and int(cut[2][0]) == 1024 and torch.equal(cut[0], full[0])


@pytest.mark.parametrize("conn", CONN)
def test_skip_and_class_range(conn):
    labels = _blobs(2, TH + 9, TW + 20, 6, seed=3)
    labels[1] = np.where(labels[1] > 0, 7, 0)                        # frame 1: the background and labels >= nc only
    want = _check(labels, 6, conn, skip=(0, 2), K=32)
    comp = want[0].numpy()
    assert (comp[np.isin(labels, (0, 2, 7))] == -1).all() and (comp[~np.isin(labels, (0, 2, 7))] >= 0).all()
    assert int(want[2][1]) == 0 and not want[1][1].any() and int(want[2][0]) > 0
    assert not np.isin(want[1][0, :int(want[2][0]), 0].numpy(), (0, 2)).any()
    _check(labels, 6, conn, skip=range(64))                          # everything skipped
    _check(labels, 64, conn, skip=(63, 0))


def test_sums_past_32_bits():
    H, W = 40, 16384
    got = hip.label_components(torch.full((1, H, W), 5, dtype=torch.uint8, device="cuda"), 12, 8, max_instances=2)
    sx, sy = W * (W - 1) // 2, H * (H - 1) // 2
    sxx, syy = (W - 1) * W * (2 * W - 1) // 6, (H - 1) * H * (2 * H - 1) // 6
    row = got[1][0, 0].tolist()
    assert row == [5, 0, H * W, H * sx, W * sy, H * sxx, sx * sy, W * syy, W, H, W, H]
    assert row[3] > 2 ** 32 and row[6] > 2 ** 36 and row[5] > 2 ** 45
    assert got[2].tolist() == [1] and not got[1][0, 1].any() and not got[0].any()
    tall = hip.label_components(torch.ones(1, 16384, 9, dtype=torch.uint8, device="cuda"), 2, 4, max_instances=1)
    n = 16384
    assert tall[1][0, 0].tolist() == [1, 0, 9 * n, n * 36, 9 * (n * (n - 1) // 2), n * 204, 36 * (n * (n - 1) // 2),
                                      9 * ((n - 1) * n * (2 * n - 1) // 6), 9, n, 9, n]


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
    for conn in CONN:
        _same(hip.label_components(view, 12, conn, (0,), 512), _want(labels, 12, conn, (0,), 512))


def _buffers(n, H, W, K):
    out = (torch.full((n, H, W), 77, dtype=torch.int32, device="cuda"), torch.full((n, K, 12), 77, dtype=torch.int64, device="cuda"),
           torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    ws = torch.full((hip.label_components_scratch(n, H, W) + 16,), 77, dtype=torch.uint8, device="cuda")
    return out, ws


@pytest.mark.parametrize("conn", CONN)
def test_buffers_are_reused_and_the_call_is_capturable(conn):
    n, H, W, K = 2, 2 * TH + 1, 2 * TW + 2, 64
    first = _noise((n, H, W), 0.01, seed=7) | _blobs(n, H, W, 4, seed=7)
    second = _blobs(n, H, W, 4, seed=8)                              # fewer components: stale rows would show
    labels = _dev(first)
    out, ws = _buffers(n, H, W, K)
    got = hip.label_components(labels, 4, conn, (0,), K, out=out, workspace=ws)
    assert all(g is o for g, o in zip(got, out))
    want_first, want_second = _want(first, 4, conn, (0,), K), _want(second, 4, conn, (0,), K)
    assert int(want_second[2].max()) < int(want_first[2].min())
    _same(out, want_first)
    labels.copy_(torch.from_numpy(second))
    hip.label_components(labels, 4, conn, (0,), K, out=out, workspace=ws)
    _same(out, want_second)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.label_components(labels, 4, conn, (0,), K, out=out, workspace=ws)
    for nxt, want in ((first, want_first), (second, want_second)):
        labels.copy_(torch.from_numpy(nxt))
        graph.replay()
        _same(out, want)
        _same(hip.label_components(labels, 4, conn, (0,), K), want)      # eager, fresh buffers


def test_wrapper_refusals():
    host = _blobs(2, 8, 16, 4, seed=2)
    labels = _dev(host)
    want = _want(host, 4, 8, (0,), 8)
    out, ws = _buffers(2, 8, 16, 8)
    call = lambda lab=labels, nc=4, conn=8, skip=(0,), K=8, **kw: hip.label_components(lab, nc, conn, skip, K, **kw)
    for lab in (labels.long(), labels[0], labels.transpose(1, 2), labels.cpu(), labels[:0], host):
        with pytest.raises(StswinHipError, match="labels"):
            call(lab=lab)
    with pytest.raises(StswinHipError, match="16384"):
        call(lab=torch.zeros(1, 1, 16385, dtype=torch.uint8, device="cuda"))
    for nc in (0, 65, -1, 4.0, None):
        with pytest.raises(StswinHipError, match="classes"):
            call(nc=nc)
    for conn in (0, 6, 16, None, 8.0, True):
        with pytest.raises(StswinHipError, match="connectivity"):
            call(conn=conn)
    for skip in ((64,), (-1,), (1.0,), ("0",)):
        with pytest.raises(StswinHipError, match="skip"):
            call(skip=skip)
    for K in (0, 1025, -1, 8.0, None):
        with pytest.raises(StswinHipError, match="max_instances"):
            call(K=K)
    bad_out = ((out[0].long(), out[1], out[2]), (out[0], out[1].int(), out[2]), (out[0], out[1], out[2].long()),
               (out[0][:1], out[1], out[2]), (out[0], out[1][:, :4], out[2]), (out[0], out[1][:, :, :10], out[2]),
               (out[0], out[1], out[2][:1]), (out[0].cpu(), out[1], out[2]), (out[0].transpose(1, 2), out[1], out[2]),
               (out[0], out[1]), out[0])
    for o in bad_out:
        with pytest.raises(StswinHipError):
            call(out=o, workspace=ws)
    for w in (ws[:hip.label_components_scratch(2, 8, 16) - 1], ws.int(), ws.cpu(), ws.view(2, -1)):
        with pytest.raises(StswinHipError, match="workspace"):
            call(out=out, workspace=w)
    big = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    lab_in = big[:256].view(2, 8, 16)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(lab=lab_in, out=(big[:1024].view(torch.int32).view(2, 8, 16), out[1], out[2]), workspace=ws)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(lab=lab_in, out=out, workspace=big)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(out=(out[0], out[1], out[0].view(-1)[:2]), workspace=ws)
    with pytest.raises(StswinHipError, match="shares memory"):
        call(out=(big[:1024].view(torch.int32).view(2, 8, 16), out[1], out[2]), workspace=big)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out + (ws,)), "a refused call launched"
    _same(call(), want)
    _same(call(out=out, workspace=ws), want)


def test_c_abi():
    assert "stswin_label_components" in hip.declared_symbols() and "stswin_label_components_scratch" in hip.declared_symbols()
    lib = hip.load()
    assert lib.stswin_abi_version() == 1
    host = _blobs(2, 8, 16, 4, seed=2)
    labels = _dev(host)
    out, ws = _buffers(2, 8, 16, 8)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    fn = lib.stswin_label_components

    def run(lab=p(labels), comp=p(out[0]), rows=p(out[1]), total=p(out[2]), n=2, H=8, W=16, nc=4, conn=8, skip=1, K=8, w=p(ws),
            wbytes=ws.numel()):
        return fn(lab, comp, rows, total, n, H, W, nc, conn, skip, K, w, wbytes, st)

    for kw in (dict(n=0), dict(n=-1), dict(H=0), dict(W=-16), dict(H=16385), dict(W=16385)):
        assert run(**kw) == -1830, kw
    assert lib.stswin_label_components_scratch(1, 16385, 1) == -1830 and lib.stswin_label_components_scratch(0, 8, 16) == -1830
    for kw in (dict(lab=None), dict(comp=None), dict(rows=None), dict(total=None), dict(w=None)):
        assert run(**kw) == -1831, kw
    for nc in (0, -3, 65):
        assert run(nc=nc) == -1832
    for conn in (0, 6, -8):
        assert run(conn=conn) == -1833
    for K in (0, -1, 1025):
        assert run(K=K) == -1834
    need = lib.stswin_label_components_scratch(2, 8, 16)
    assert need == hip.label_components_scratch(2, 8, 16) == 4 * 2 * (8 * 16 + 1)
    assert run(wbytes=need - 1) == -1835 and run(w=p(ws) + 1) == -1835
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out + (ws,)), "a refused call launched"
    assert run(wbytes=need) == 0
    _same(out, _want(host, 4, 8, (0,), 8))


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE = (72, 88)         # the frames' size and the output size (the model's input is 64 x 64)
N = 10
K = 64


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
    """Per protocol: the model, two sequences, an int64 ground truth, the results of report="frame" alone (today's path) and the host
    components of their label maps at 8-connectivity with the protocol's default skip - computed once, shared, never changed."""
    if protocol not in _CASES:
        m = _model(protocol, seed=4)
        nc = 9 if protocol == "cadis" else 12
        skip = (nc - 1,) if protocol == "cadis" else (0,)
        g = np.random.default_rng(17)
        seqs = []
        for s in range(2):
            fr = _frames(N, seed=40 + s)
            with torch.no_grad():
                res = video.VideoSegmenter(m, out="labels", out_size=SIZE, protocol=protocol, report="frame").segment_sequence(fr)
            labels = np.stack([r[0].cpu().numpy() for r in res])
            _, rows, total = I.label_components(labels, nc, 8, skip, K)
            seqs.append(dict(fr=fr, labels=torch.from_numpy(labels), moments=torch.stack([r[1].cpu() for r in res]),
                             rows=torch.from_numpy(rows), total=torch.from_numpy(total), gt=torch.from_numpy(g.integers(0, nc - 1, (N, *SIZE)))))
        assert int(seqs[0]["total"].max()) >= 2, "the random model predicts one blob: the instances test little"
        _CASES[protocol] = dict(m=m, nc=nc, skip=skip, seqs=seqs)
    return _CASES[protocol]


_MODES = {"eager": {}, "batch4": dict(batch=4), "graph": dict(graph=True)}


def _own_instances(r, c, conn=8, skip=None, k=K):
    """The last two elements of a report="frame", instances=k result against the host components of the result's own labels."""
    rows, total = r[-2], r[-1]
    assert rows.is_cuda and rows.dtype == torch.int64 and tuple(rows.shape) == (k, 12)
    assert total.is_cuda and total.dtype == torch.int32 and total.dim() == 0
    _, wrows, wtotal = _want(r[0].cpu().numpy()[None], c["nc"], conn, c["skip"] if skip is None else skip, k)
    return torch.equal(rows.cpu(), wrows[0]) and int(total) == int(wtotal[0])


@pytest.mark.parametrize("mode", list(_MODES))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_frame_instances(protocol, mode):
    c = _case(protocol)
    m = c["m"]
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", **_MODES[mode])
    with torch.no_grad():
        seg = video.VideoSegmenter(m, instances=K, **kw)
        for s in c["seqs"]:                                              # the second sequence follows a reset(): graph replays go on
            got = seg.segment_sequence(s["fr"])
            assert len(got) == N
            for f, r in enumerate(got):
                assert len(r) == 4 and torch.equal(r[0].cpu(), s["labels"][f]) and torch.equal(r[1].cpu(), s["moments"][f]), f
                assert torch.equal(r[2].cpu(), s["rows"][f]) and int(r[3]) == int(s["total"][f]), f
        # instances=None is today's path: the same results as the shared report="frame" run, nothing appended
        s = c["seqs"][0]
        for f, r in enumerate(video.VideoSegmenter(m, **kw).segment_sequence(s["fr"])):
            assert len(r) == 2 and torch.equal(r[0].cpu(), s["labels"][f]) and torch.equal(r[1].cpu(), s["moments"][f]), f
        # with int64 ground truth the labels, and so the instances, come from the scoring launches
        got = seg.segment_sequence(s["fr"], gt=s["gt"])
        plain = video.VideoSegmenter(m, **kw).segment_sequence(s["fr"], gt=s["gt"])
        for f, (r, p) in enumerate(zip(got, plain)):
            assert len(r) == len(p) + 2 and torch.equal(r[0], p[0]) and torch.equal(r[-3], p[-1]), f
            if protocol == "endovis18":                                  # (labels, dice, iou, moments, rows, total)
                assert len(r) == 6 and r[1] == p[1] and r[2] == p[2]
            assert torch.equal(r[-2].cpu(), s["rows"][f]) and int(r[-1]) == int(s["total"][f]), f
        # 4-connectivity, another skip set and a K that truncates, against the result's own labels
        other = video.VideoSegmenter(m, instances=2, connectivity=4, instance_skip=(1, 3), **kw).segment_sequence(s["fr"])
        assert all(_own_instances(r, c, 4, (1, 3), 2) for r in other)
        assert max(int(r[-1]) for r in other) > 2, "nothing was truncated"


def test_segmenter_graph_instances_are_views_until_the_next_push():
    c = _case("endovis18")
    s = c["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, report="frame", graph=True, instances=K)
        seen, held = {}, []
        for f in range(N):
            for g, r in seg.push(s["fr"][f]):
                seen[g] = tuple(t.clone() for t in r)
                held.append((g, r))
        for g, r in seg.finish():
            seen[g] = tuple(t.clone() for t in r)
    assert sorted(seen) == list(range(N))
    for f in range(N):
        assert torch.equal(seen[f][2].cpu(), s["rows"][f]) and int(seen[f][3]) == int(s["total"][f]), f
    # the replayed results of the steady state all look at the graph's buffers, which now hold the last replayed frame
    last = held[-1][1]
    replayed = [r for g, r in held if r[2].data_ptr() == last[2].data_ptr()]
    assert len(replayed) >= 2 and all(r[3].data_ptr() == last[3].data_ptr() for r in replayed)
    assert all(torch.equal(r[2], last[2]) for r in replayed)


@pytest.mark.parametrize("protocol,mode", [("endovis18", "eager"), ("endovis18", "batch4"), ("endovis18", "graph"), ("cadis", "graph")])
def test_segmenter_deferred_instances(protocol, mode):
    c = _case(protocol)
    a, b = c["seqs"]
    names = [f"class {k}" for k in range(c["nc"])]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="labels", out_size=SIZE, protocol=protocol, report="deferred", min_area=3, instances=K,
                                   **_MODES[mode])
        empty = seg.instance_report()
        assert len(empty) == 0 and empty.present.shape == (0, K)
        got_a = seg.segment_sequence(a["fr"])
        seg.segment_sequence(b["fr"], gt=b["gt"])                          # scored frames are logged as well
    for f in range(N):                                                    # the results are unchanged
        assert isinstance(got_a[f], torch.Tensor) and torch.equal(got_a[f].cpu(), a["labels"][f])
    rep = seg.instance_report(names=names)
    assert rep.sequences == [0] * N + [1] * N and rep.frames == list(range(N)) * 2         # ordered by sequence and frame
    want = I.InstanceReport.from_rows(torch.cat([a["rows"], b["rows"]]).numpy(), torch.cat([a["total"], b["total"]]).numpy(), SIZE,
                                      min_area=3, names=names, frames=list(range(N)) * 2, sequences=[0] * N + [1] * N)
    assert np.array_equal(rep.rows, want.rows) and np.array_equal(rep.total, want.total) and rep.size == SIZE and rep.min_area == 3
    assert np.array_equal(rep.present, want.present) and np.array_equal(rep.box, want.box, equal_nan=True)
    assert np.array_equal(rep.angle, want.angle, equal_nan=True) and np.array_equal(rep.counts(), want.counts())
    assert rep.as_rows() == want.as_rows() and np.array_equal(rep.truncated, want.truncated)
    moments = seg.instrument_report()                                     # the class report beside it is unchanged
    assert torch.equal(torch.from_numpy(moments.moments), torch.cat([a["moments"], b["moments"]]))
    seg.reset_metrics()
    assert len(seg.instance_report()) == 0
    with torch.no_grad():
        seg.segment_sequence(b["fr"])
    again = seg.instance_report()
    assert again.sequences == [0] * N and np.array_equal(again.rows, b["rows"].numpy())


def test_segmenter_deferred_instance_log_grows_past_its_first_rows():
    c = _case("endovis18")
    a = c["seqs"][0]
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="overlay", report="deferred", batch=4, instances=K)
        for _ in range(7):                                                # 70 rows: past the log's first 64
            seg.segment_sequence(a["fr"])
    rep = seg.instance_report()
    assert len(rep) == 7 * N and rep.sequences == [s for s in range(7) for _ in range(N)] and rep.frames == list(range(N)) * 7
    assert np.array_equal(rep.rows, a["rows"].repeat(7, 1, 1).numpy()) and np.array_equal(rep.total, a["total"].repeat(7).numpy())


def test_segmenter_instances_refusals():
    m = _case("endovis18")["m"]
    for kwargs in (dict(out="labels", instances=8), dict(out="logits", instances=8), dict(out="labels", report="frame", instances=0),
                   dict(out="labels", report="frame", instances=1025), dict(out="labels", report="deferred", instances=8.0),
                   dict(out="labels", report="frame", instances=True), dict(out="labels", report="frame", instances=8, connectivity=6),
                   dict(out="labels", report="frame", instances=8, instance_skip=(64,)), dict(out="labels", report="frame", connectivity=4),
                   dict(out="labels", report="frame", instance_skip=(0,))):
        with pytest.raises(StswinHipError):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(out="labels", report="deferred"), dict(out="labels", report="frame", instances=8), dict(out="labels")):
        with pytest.raises(StswinHipError, match="instances"):
            video.VideoSegmenter(m, **kwargs).instance_report()
    seg = video.VideoSegmenter(m, out="overlay", protocol="endovis18", report="frame", instances=1024)
    assert seg.instance_skip == (0,) and seg.connectivity == 8
