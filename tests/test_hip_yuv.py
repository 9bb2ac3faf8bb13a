"""GPU: stswin_yuv_to_rgb / stswin_rgb_to_nv12 (hip.yuv_to_rgb, hip.rgb_to_nv12) byte for byte against utils.yuv, and
VideoSegmenter(pixel_format="nv12" | "uyvy", out_format="nv12") against the segmenter that is pushed utils.yuv.yuv_to_rgb(frames)."""
import numpy as np
import pytest
import torch

from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import yuv as Y

pytestmark = pytest.mark.gpu

PAIRS = [(s, f) for s in ("bt709", "bt601") for f in (False, True)]
# (1, 2, 2): one thread; (2, 4, 6); (3, 34, 130): Ws is no multiple of 8 - the body of 2 pixels per thread, an nv12 frame of 6630 and an
# RGB frame of 13 260 bytes, so frames 1 and 2 start off every vector grid, 9 workgroups and more; (2, 36, 264): Ws % 8 == 0 - the body
# of 8 pixels per thread over 5 workgroups (nv12) with a partial last one
SHAPES = [(1, 2, 2), (2, 4, 6), (3, 34, 130), (2, 36, 264)]
# (Y, U, V) that leave the RGB range: R and B low / R and B high / G high / G low
PLANTED_YUV = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 255)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.uint8 and tuple(got.shape) == want.shape and torch.equal(got.cpu(), torch.from_numpy(want))


def _raw(m, t):
    """The three sums of a matrix for one triple before the clamp."""
    m = np.asarray(m).astype(np.int64)
    return [int((m[c, 0] * t[0] + m[c, 1] * t[1] + m[c, 2] * t[2] + m[c, 3]) >> 14) for c in range(3)]


def _shape_of(fmt, n, Hs, Ws):
    return (n, Hs * 3 // 2, Ws) if fmt == "nv12" else (n, Hs, Ws, 2)


def _plant(frames, fmt, f, y0, x0, t):
    """A 4 x 4 pixel region (2 x 2 where the frame is 2 x 2) of the constant (Y, U, V) t with its corner at the even (y0, x0)."""
    Hs = frames.shape[1] // 3 * 2 if fmt == "nv12" else frames.shape[1]
    h, w = min(4, Hs), min(4, frames.shape[2])
    if fmt == "nv12":
        frames[f, y0:y0 + h, x0:x0 + w] = t[0]
        frames[f, Hs + y0 // 2:Hs + (y0 + h) // 2, x0:x0 + w] = np.tile(np.array(t[1:], np.uint8), w // 2)
    else:
        frames[f, y0:y0 + h, x0:x0 + w, 1] = t[0]
        frames[f, y0:y0 + h, x0:x0 + w, 0] = np.tile(np.array(t[1:], np.uint8), w // 2)


def _yuv_case(fmt, n, Hs, Ws, seed):
    """Random bytes with the planted triples: -> (frames, [(frame, y, x, triple), ...] pixels whose chroma is the planted one under
    both chroma modes: an odd row and an even column inside a planted region)."""
    g = np.random.default_rng(seed)
    frames = g.integers(0, 256, _shape_of(fmt, n, Hs, Ws), dtype=np.uint8)
    spots = []
    corners = [(0, 0)] if Ws < 8 or Hs < 8 else [(0, 0), (Hs - 4, Ws - 4), (0, Ws - 4), (Hs - 4, 0)]      # the clamped edges too
    for i, t in enumerate(PLANTED_YUV[:max(n * len(corners), 1)]):
        f, (y0, x0) = (i // len(corners)) % n, corners[i % len(corners)]
        _plant(frames, fmt, f, y0, x0, t)
        spots.append((f, y0 + 1, x0, t))
    return frames, spots


def test_planted_triples_clamp_in_every_channel():
    for standard, full in PAIRS:
        raws = np.array([_raw(Y.to_rgb_matrix(standard, full), t) for t in PLANTED_YUV])
        assert (raws.min(axis=0) < 0).all() and (raws.max(axis=0) > 255).all(), (standard, full, raws)


@pytest.mark.parametrize("standard,full", PAIRS)
@pytest.mark.parametrize("chroma", ["replicate", "linear"])
@pytest.mark.parametrize("fmt", ["nv12", "uyvy"])
@pytest.mark.parametrize("n,Hs,Ws", SHAPES)
def test_yuv_to_rgb_against_the_host_statement(n, Hs, Ws, fmt, chroma, standard, full):
    frames, spots = _yuv_case(fmt, n, Hs, Ws, seed=Hs * Ws + full)
    m = Y.to_rgb_matrix(standard, full)
    want = Y.yuv_to_rgb(frames, fmt, m, chroma)
    for f, y, x, t in spots:                                     # the planted triples arrive unmixed and clamp where the sums say
        assert want[f, y, x].tolist() == [min(max(v, 0), 255) for v in _raw(m, t)], (f, y, x, t)
    if len(spots) == len(PLANTED_YUV):
        assert (want.reshape(-1, 3).min(0) == 0).all() and (want.reshape(-1, 3).max(0) == 255).all()
    assert _same(hip.yuv_to_rgb(_dev(frames), _dev(m), fmt, chroma), want)


def _clamping_to_yuv():
    """A matrix of three times the full-range BT.709 contrast around mid-grey: every output channel clamps both ways."""
    m = Y.to_yuv_matrix("bt709", True).astype(np.int64)
    m[:, :3] *= 3
    m[0, 3] -= 2 * 128 << 14
    return m.astype(np.int32)


PLANTED_RGB = [(0, 0, 0), (255, 255, 255), (0, 0, 255), (255, 255, 0), (255, 0, 0), (0, 255, 255)]


def _rgb_case(n, Hs, Ws, seed):
    g = np.random.default_rng(seed)
    rgb = g.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)
    for i, t in enumerate(PLANTED_RGB):                           # constant 2 x 2 blocks: the mean is the triple
        y0, x0 = 2 * (i % (Hs // 2)), 2 * (i % (Ws // 2))
        rgb[i % n, y0:y0 + 2, x0:x0 + 2] = t
    return rgb


@pytest.mark.parametrize("matrix", ["bt709", "bt709-full", "bt601", "bt601-full", "clamping"])
@pytest.mark.parametrize("n,Hs,Ws", SHAPES)
def test_rgb_to_nv12_against_the_host_statement(n, Hs, Ws, matrix):
    m = _clamping_to_yuv() if matrix == "clamping" else Y.to_yuv_matrix(matrix.split("-")[0], matrix.endswith("full"))
    rgb = _rgb_case(n, Hs, Ws, seed=Hs + Ws)
    want = Y.rgb_to_nv12(rgb, m)
    if matrix == "clamping":
        raws = np.array([_raw(m, t) for t in PLANTED_RGB])
        assert (raws.min(axis=0) < 0).all() and (raws.max(axis=0) > 255).all(), raws
        if Hs * Ws >= 4 * len(PLANTED_RGB):
            assert want[:, :Hs].min() == 0 and want[:, :Hs].max() == 255
            uv = want[:, Hs:].reshape(n, -1, 2)
            assert (uv.reshape(-1, 2).min(0) == 0).all() and (uv.reshape(-1, 2).max(0) == 255).all()
    assert _same(hip.rgb_to_nv12(_dev(rgb), _dev(m)), want)


# ---------------------------------------------------------------------------------------------------- alignment
def _offset_view(a: np.ndarray, off: int, fill: int = 0):
    """(buffer, view): a contiguous GPU tensor holding `a`, `off` bytes into a uint8 allocation with 32 more bytes behind it."""
    nbytes = a.size * a.itemsize
    buf = torch.full((off + nbytes + 32,), fill, dtype=torch.uint8, device="cuda")
    v = buf[off:off + nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off
    return buf, v


@pytest.mark.parametrize("which", ["in", "out", "both"])
@pytest.mark.parametrize("off", [1, 2, 3, 8])
@pytest.mark.parametrize("kernel", ["nv12", "uyvy", "rgb_to_nv12"])
def test_misaligned_pointers(kernel, off, which):
    """Ws % 8 == 0: at offset 0 these shapes take the wide body; the offsets (8: a uyvy input wants 16) must not."""
    n, Hs, Ws = 2, 6, 24
    if kernel == "rgb_to_nv12":
        src_host, m = _rgb_case(n, Hs, Ws, seed=off), Y.to_yuv_matrix("bt601", False)
        want = Y.rgb_to_nv12(src_host, m)
    else:
        src_host, m = _yuv_case(kernel, n, Hs, Ws, seed=off)[0], Y.to_rgb_matrix("bt601", False)
        want = Y.yuv_to_rgb(src_host, kernel, m, "linear")
    _, src = _offset_view(src_host, off if which in ("in", "both") else 0)
    o = off if which in ("out", "both") else 0
    buf, out = _offset_view(np.full(want.shape, 171, np.uint8), o, fill=171)
    mat = _offset_view(m, 4)[1]                                  # (the matrix only needs its own int alignment)
    got = hip.rgb_to_nv12(src, mat, out=out) if kernel == "rgb_to_nv12" else hip.yuv_to_rgb(src, mat, kernel, "linear", out=out)
    assert got is out and _same(got, want)
    assert (buf[:o] == 171).all() and (buf[o + want.size:] == 171).all(), "bytes around out were written"


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    nv12, _ = _yuv_case("nv12", 2, 8, 16, seed=1)
    uyvy, _ = _yuv_case("uyvy", 2, 8, 16, seed=2)
    rgb = _rgb_case(2, 8, 16, seed=3)
    a, b, c = _dev(nv12), _dev(uyvy), _dev(rgb)
    m, my = _dev(Y.to_rgb_matrix()), _dev(Y.to_yuv_matrix())
    ok = hip.yuv_to_rgb(a, m)
    sent = torch.full((2, 8, 16, 3), 99, dtype=torch.uint8, device="cuda")
    sent12 = torch.full((2, 12, 16), 99, dtype=torch.uint8, device="cuda")
    for args, kw in (((a.int(), m), {}), ((a[0], m), {}), ((a[:, :11].contiguous(), m), {}), ((a[:, :, :15].contiguous(), m), {}),
                     ((a[:, :, ::2], m), {}), ((a[:0], m), {}), ((a.cpu(), m), {}), ((b, m), {}), ((a, m, "uyvy"), {}),
                     ((b[:, :, :15].contiguous(), m, "uyvy"), {}), ((b[..., :1].contiguous(), m, "uyvy"), {}), ((a, m, "i420"), {}),
                     ((a, m, "nv12", "cubic"), {}), ((a, m.float()), {}), ((a, m[:2].contiguous()), {}), ((a, m.cpu()), {}),
                     ((a, m.t().contiguous().t()), {}), ((a, Y.to_rgb_matrix()), {}),
                     ((a, m), dict(out=sent[:1])), ((a, m), dict(out=sent.cpu())), ((a, m), dict(out=sent.int())),
                     ((a, m), dict(out=sent.transpose(1, 2)))):
        with pytest.raises(StswinHipError):
            hip.yuv_to_rgb(*args, **{"out": sent, **kw})
    for args, kw in (((c.int(), my), {}), ((c[0], my), {}), ((c[:, :7].contiguous(), my), {}), ((c[:, :, :15].contiguous(), my), {}),
                     ((c[..., :2].contiguous(), my), {}), ((c[:0], my), {}), ((c.cpu(), my), {}), ((c, my.long()), {}), ((c, my.cpu()), {}),
                     ((c, my), dict(out=sent12[:1])), ((c, my), dict(out=sent12.cpu())), ((c, my), dict(out=sent12.view(2, 16, 12)))):
        with pytest.raises(StswinHipError):
            hip.rgb_to_nv12(*args, **{"out": sent12, **kw})
    big = torch.full((4096,), 99, dtype=torch.uint8, device="cuda")
    big[:a.numel()] = a.view(-1)
    src = big[:a.numel()].view(2, 12, 16)
    with pytest.raises(StswinHipError, match="shares memory"):
        hip.yuv_to_rgb(src, m, out=big[300:300 + 768].view(2, 8, 16, 3))
    with pytest.raises(StswinHipError, match="shares memory"):
        hip.rgb_to_nv12(big[:768].view(2, 8, 16, 3), my, out=big[767:767 + 384].view(2, 12, 16))
    assert (big[a.numel():] == 99).all()
    # the C entry points' own codes
    lib, st = hip.load(), torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    f = lib.stswin_yuv_to_rgb
    assert f(p(a), p(m), p(sent), 0, 8, 16, 0, 0, st) == -1424
    assert f(p(a), p(m), p(sent), 2, -8, 16, 0, 0, st) == -1424
    assert f(p(a), p(m), p(sent), 2, 8, 0, 0, 0, st) == -1424
    assert f(None, p(m), p(sent), 2, 8, 16, 0, 0, st) == -1425
    assert f(p(a), None, p(sent), 2, 8, 16, 0, 0, st) == -1425
    assert f(p(a), p(m), None, 2, 8, 16, 0, 0, st) == -1425
    assert f(p(a), p(m), p(sent), 2, 7, 16, 0, 0, st) == -1426            # odd Hs: nv12 only
    assert f(p(a), p(m), p(sent), 2, 8, 15, 0, 0, st) == -1426
    assert f(p(b), p(m), p(sent), 2, 8, 15, 1, 0, st) == -1426
    assert f(p(a), p(m), p(sent), 2, 8, 16, -1, 0, st) == -1427
    assert f(p(a), p(m), p(sent), 2, 8, 16, 2, 0, st) == -1427
    assert f(p(a), p(m), p(sent), 2, 8, 16, 0, -1, st) == -1428
    assert f(p(a), p(m), p(sent), 2, 8, 16, 0, 2, st) == -1428
    assert f(p(src), p(m), p(src) + 383, 2, 8, 16, 0, 0, st) == -1429
    assert f(p(src), p(m), p(src), 2, 8, 16, 0, 0, st) == -1429
    f = lib.stswin_rgb_to_nv12
    assert f(p(c), p(my), p(sent12), 2, 8, 0, st) == -1424
    assert f(p(c), p(my), p(sent12), -2, 8, 16, st) == -1424
    assert f(None, p(my), p(sent12), 2, 8, 16, st) == -1425
    assert f(p(c), None, p(sent12), 2, 8, 16, st) == -1425
    assert f(p(c), p(my), None, 2, 8, 16, st) == -1425
    assert f(p(c), p(my), p(sent12), 2, 7, 16, st) == -1426
    assert f(p(c), p(my), p(sent12), 2, 8, 15, st) == -1426
    assert f(p(big), p(my), p(big) + 767, 2, 8, 16, st) == -1429
    torch.cuda.synchronize()
    assert (sent == 99).all() and (sent12 == 99).all() and (big[a.numel():] == 99).all(), "a refused call launched"
    assert torch.equal(a.cpu(), torch.from_numpy(nv12)) and torch.equal(c.cpu(), torch.from_numpy(rgb))
    # an odd height is a frame of the other kind for uyvy, and legal
    odd = _yuv_case("uyvy", 1, 7, 16, seed=4)[0]
    assert _same(hip.yuv_to_rgb(_dev(odd), m, "uyvy"), Y.yuv_to_rgb(odd, "uyvy", Y.to_rgb_matrix()))
    assert torch.equal(hip.yuv_to_rgb(a, m), ok)


# ---------------------------------------------------------------------------------------------------- graph capture, full size
@pytest.mark.parametrize("kernel", ["nv12", "uyvy", "rgb_to_nv12"])
def test_capturable_into_a_graph(kernel):
    n, Hs, Ws = 2, 34, 72
    if kernel == "rgb_to_nv12":
        m = Y.to_yuv_matrix()
        first, second = _rgb_case(n, Hs, Ws, seed=1), _rgb_case(n, Hs, Ws, seed=2)
        ref = lambda x: Y.rgb_to_nv12(x, m)
        run = lambda s, mm, o: hip.rgb_to_nv12(s, mm, out=o)
    else:
        m = Y.to_rgb_matrix()
        first, second = _yuv_case(kernel, n, Hs, Ws, seed=1)[0], _yuv_case(kernel, n, Hs, Ws, seed=2)[0]
        ref = lambda x: Y.yuv_to_rgb(x, kernel, m, "linear")
        run = lambda s, mm, o: hip.yuv_to_rgb(s, mm, kernel, "linear", out=o)
    src, mat = _dev(first), _dev(m)
    out = torch.zeros(ref(first).shape, dtype=torch.uint8, device="cuda")
    run(src, mat, out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(src, mat, out)
    src.copy_(torch.from_numpy(second))
    graph.replay()
    assert not np.array_equal(ref(first), ref(second)) and _same(out, ref(second))


def test_one_full_size_frame():
    Hs, Ws = 1024, 1280
    m, my = Y.to_rgb_matrix(), Y.to_yuv_matrix()
    for fmt in ("nv12", "uyvy"):
        frames = _yuv_case(fmt, 1, Hs, Ws, seed=7)[0]
        src = _dev(frames)
        for chroma in ("replicate", "linear"):
            assert _same(hip.yuv_to_rgb(src, _dev(m), fmt, chroma), Y.yuv_to_rgb(frames, fmt, m, chroma)), (fmt, chroma)
    rgb = _rgb_case(1, Hs, Ws, seed=8)
    assert _same(hip.rgb_to_nv12(_dev(rgb), _dev(my)), Y.rgb_to_nv12(rgb, my))


# ---------------------------------------------------------------------------------------------------- the segmenter
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


N, HS, WS = 10, 70, 90
STD = dict(yuv_standard="bt601", full_range=False)


@pytest.fixture(scope="module")
def clips():
    """Ten 70 x 90 frames made as YUV bytes: a still picture plus noise, in both raw layouts, their host RGB frames per chroma mode,
    ground truth at the frame size, and a cache of the RGB-pushed segmenters' results."""
    g = np.random.default_rng(17)
    raw = {}
    for fmt in ("nv12", "uyvy"):
        base = g.integers(0, 256, _shape_of(fmt, 1, HS, WS), dtype=np.int64)
        raw[fmt] = np.clip(base + g.integers(-24, 25, _shape_of(fmt, N, HS, WS)), 0, 255).astype(np.uint8)
    m = Y.to_rgb_matrix(**{"standard": STD["yuv_standard"], "full_range": STD["full_range"]})
    rgb = {(fmt, ch): Y.yuv_to_rgb(raw[fmt], fmt, m, ch) for fmt in raw for ch in ("replicate", "linear")}
    gt = g.integers(0, 12, (N, HS, WS))
    gt[:, 20:50, 10:60] = 3
    return dict(model=_model("endovis18", seed=4), raw=raw, rgb=rgb, gt=torch.from_numpy(gt), cache={})


def _reference(clips, fmt, chroma, gt, split=None, **kw):
    """The results of a segmenter of the same mode that is pushed the host-converted RGB frames (computed once per form)."""
    key = (fmt, chroma, gt, split, tuple(sorted(kw.items())))
    if key not in clips["cache"]:
        seg = video.VideoSegmenter(clips["model"], **kw)
        clips["cache"][key] = _run(seg, clips["rgb"][fmt, chroma], clips["gt"] if gt else None, split)
    return clips["cache"][key]


def _run(seg, frames, gt, split=None):
    """segment_sequence, or with `split` the sequence pushed in two calls; results in frame order, cloned."""
    with torch.no_grad():
        if split is None:
            return seg.segment_sequence(frames, gt=gt)
        seg.reset()
        res = []
        for lo, hi in ((0, split), (split, len(frames))):
            res += [(f, video._clone(r)) for f, r in seg.push(frames[lo:hi], gt=None if gt is None else gt[lo:hi])]
        res += [(f, video._clone(r)) for f, r in seg.finish()]
        return [r for _, r in sorted(res, key=lambda fr: fr[0])]


def _equal(got, want):
    assert len(got) == len(want) == N
    for f, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, tuple):
            assert isinstance(a, tuple) and torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], f
        else:
            assert isinstance(a, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), f


@pytest.mark.parametrize("where", ["cpu", "gpu"])
@pytest.mark.parametrize("fmt", ["nv12", "uyvy"])
def test_segmenter_online_labels_and_scores(clips, fmt, where):
    kw = dict(out="labels", out_size=(HS, WS))
    frames = clips["raw"][fmt] if where == "cpu" else _dev(clips["raw"][fmt])
    seg = video.VideoSegmenter(clips["model"], pixel_format=fmt, **STD, **kw)
    got = _run(seg, frames, clips["gt"])
    assert seg.frame_shape == (HS, WS) and isinstance(got[0], tuple)
    _equal(got, _reference(clips, fmt, "replicate", True, **kw))


@pytest.mark.parametrize("fmt", ["nv12", "uyvy"])
def test_segmenter_online_logits_and_overlays(clips, fmt):
    seg = video.VideoSegmenter(clips["model"], pixel_format=fmt, chroma="linear", **STD)
    with torch.no_grad():                                        # one frame per push, without [n]
        res = []
        for f in range(N):
            res += seg.push(clips["raw"][fmt][f] if f % 2 else _dev(clips["raw"][fmt][f]))
        res += seg.finish()
    _equal([r for _, r in sorted(res, key=lambda fr: fr[0])], _reference(clips, fmt, "linear", False))
    seg = video.VideoSegmenter(clips["model"], out="overlay", pixel_format=fmt, **STD)
    got = _run(seg, _dev(clips["raw"][fmt]), None)
    assert got[0].shape == (HS, WS, 3) and not seg._kept and not seg._frames
    _equal(got, _reference(clips, fmt, "replicate", False, out="overlay"))


@pytest.mark.parametrize("fmt", ["nv12", "uyvy"])
def test_segmenter_batch4(clips, fmt):
    for kw, gt in ((dict(out="overlay"), True), (dict(out="logits"), False)):
        seg = video.VideoSegmenter(clips["model"], batch=4, pixel_format=fmt, **STD, **kw)
        _equal(_run(seg, clips["raw"][fmt], clips["gt"] if gt else None), _reference(clips, fmt, "replicate", gt, batch=4, **kw))


@pytest.mark.parametrize("fmt", ["nv12", "uyvy"])
def test_segmenter_graph(clips, fmt):
    """Pushed in two calls, 9 frames and 1: frame 7 is the captured step, frame 8 a replay inside the first call, frame 9 a replay in
    the second."""
    for kw, gt, where in ((dict(out="overlay"), False, "cpu"), (dict(out="labels", out_size=(HS, WS)), True, "gpu"), (dict(out="logits"), False, "gpu")):
        seg = video.VideoSegmenter(clips["model"], graph=True, pixel_format=fmt, chroma="linear", **STD, **kw)
        frames = clips["raw"][fmt] if where == "cpu" else _dev(clips["raw"][fmt])
        got = _run(seg, frames, clips["gt"] if gt else None, split=9)
        assert seg._g is not None and seg._g[1].shape == (1, *frames.shape[1:]) and seg._g[7].shape == (1, HS, WS, 3)
        _equal(got, _reference(clips, fmt, "linear", gt, split=9, graph=True, **kw))


def test_segmenter_cadis(clips):
    m = _model("cadis", seed=4)
    g = np.random.default_rng(3)
    gt = torch.from_numpy(g.integers(0, 9, (N, 45, 58)))
    kw = dict(protocol="cadis", out="labels", out_size=(45, 58))
    with torch.no_grad():
        want_seg = video.VideoSegmenter(m, **kw)
        want = want_seg.segment_sequence(clips["rgb"]["nv12", "replicate"], gt=gt)
        seg = video.VideoSegmenter(m, pixel_format="nv12", **STD, **kw)
        got = seg.segment_sequence(clips["raw"]["nv12"], gt=gt)
    _equal(got, want)
    cm = want_seg.confusion_matrix()
    assert cm.sum() > 0 and np.array_equal(seg.confusion_matrix(), cm)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_segmenter_nv12_overlays(clips, fmt, graph):
    kw = dict(graph=True) if graph else {}
    split = 9 if graph else None
    want = _reference(clips, "nv12", "replicate", False, split=split, out="overlay", **kw)
    my = Y.to_yuv_matrix(STD["yuv_standard"], STD["full_range"])
    seg = video.VideoSegmenter(clips["model"], out="overlay", out_format="nv12", pixel_format=fmt, **STD, **kw)
    frames = clips["rgb"]["nv12", "replicate"] if fmt == "rgb" else clips["raw"]["nv12"]
    got = _run(seg, frames, None, split)
    assert len(got) == N
    for f in range(N):
        assert got[f].shape == (HS * 3 // 2, WS)
        assert _same(got[f], Y.rgb_to_nv12(want[f].cpu().numpy()[None], my)[0]), f
    if graph:
        assert seg._g[4].shape == (1, HS * 3 // 2, WS)           # made inside the captured step


def test_segmenter_refusals(clips):
    m = clips["model"]
    for kw in (dict(out_format="nv12"), dict(out="labels", out_format="nv12"), dict(pixel_format="i420"), dict(out="overlay", out_format="uyvy"),
               dict(pixel_format="nv12", chroma="cubic"), dict(pixel_format="nv12", yuv_standard="bt2020")):
        with pytest.raises(StswinHipError):
            video.VideoSegmenter(m, **kw)
    nv12, uyvy = clips["raw"]["nv12"], clips["raw"]["uyvy"]
    for fmt, bad in (("nv12", nv12[:1, :104]), ("nv12", nv12[:1, :, :89]), ("nv12", uyvy[:1]), ("nv12", clips["rgb"]["nv12", "replicate"][:1]),
                     ("nv12", nv12[:1].astype(np.int32)), ("uyvy", uyvy[:1, :, :89]), ("uyvy", nv12[:1]), ("uyvy", uyvy[:1, :, :, :1]),
                     ("rgb", nv12[:1]), ("rgb", uyvy[:1])):
        seg = video.VideoSegmenter(m, pixel_format=fmt)
        with pytest.raises(StswinHipError):
            seg.push(bad)
        assert seg.frame_shape is None and not seg._frames
    seg = video.VideoSegmenter(m, pixel_format="nv12")
    seg.push(nv12[0])
    with pytest.raises(StswinHipError):
        seg.push(nv12[:1, :102])                                 # another frame size
    rgb = clips["rgb"]["nv12", "replicate"]
    for bad in (rgb[:1, :69], rgb[:1, :, :89]):                  # an odd frame size cannot leave as NV12
        seg = video.VideoSegmenter(m, out="overlay", out_format="nv12")
        with pytest.raises(StswinHipError):
            seg.push(bad)
