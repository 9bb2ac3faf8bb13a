"""GPU: stswin_labels_overlay / hip.labels_overlay and VideoSegmenter(out="overlay"), every byte against tests/overlay_ref.py."""
import numpy as np
import pytest
import torch

import overlay_ref as O
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import visualize as V

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_case(n, H, W, seed, classes=5):
    """Few classes (regions and edges both occur), a random table over all 256 entries."""
    g = np.random.default_rng(seed)
    lab = g.integers(0, classes, (n, H, W)).astype(np.uint8)
    lab[g.random((n, H, W)) < 0.1] = 255
    frames = g.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    table = g.integers(0, 256, (256, 4), dtype=np.uint8)
    return lab, frames, table


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want))


def test_blend_is_exact_for_every_alpha_and_source_byte():
    lab = np.arange(256, dtype=np.uint8)[None, :, None].repeat(256, 2)                  # row = label = alpha
    frames = np.arange(256, dtype=np.uint8)[None, None, :, None].repeat(256, 1).repeat(3, 3)   # column = source byte
    table = np.zeros((256, 4), np.uint8)
    table[:, :3] = (0, 137, 255)
    table[:, 3] = np.arange(256)
    want = O.overlay(lab, table, frames)
    assert np.array_equal(want[0, 255], np.broadcast_to(np.array([0, 137, 255], np.uint8), (256, 3))) and np.array_equal(want[0, 0], frames[0, 0])
    assert _same(hip.labels_overlay(_dev(lab), _dev(table), _dev(frames)), want)


SHAPES = [(1, 1), (1, 7), (7, 1), (5, 13), (8, 16), (33, 67), (64, 80)]


@pytest.mark.parametrize("edge", [None, 255, 77])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_where_indexing_can_go_wrong(H, W, edge):
    lab, frames, table = _random_case(2, H, W, seed=H * 100 + W)
    got = hip.labels_overlay(_dev(lab), _dev(table), _dev(frames), edge_alpha=edge)
    assert got.shape == (2, H, W, 3) and _same(got, O.overlay(lab, table, frames, edge))


def _offset_view(a: np.ndarray, off: int) -> torch.Tensor:
    """A contiguous GPU tensor holding `a`, `off` bytes into its allocation."""
    buf = torch.empty(a.size + off, dtype=torch.uint8, device="cuda")
    v = buf[off:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 8 == off % 8
    return v


@pytest.mark.parametrize("which", ["labels", "frames", "out", "all", "none"])
@pytest.mark.parametrize("off", [1, 4])
@pytest.mark.parametrize("H,W", [(5, 13), (8, 16)])
def test_misaligned_pointers(H, W, off, which):
    lab, frames, table = _random_case(2, H, W, seed=H + W + off)
    want = O.overlay(lab, table, frames, 200)
    shift = lambda name: off if which in (name, "all") else 0
    out = _offset_view(np.full((2, H, W, 3), 99, np.uint8), shift("out"))
    got = hip.labels_overlay(_offset_view(lab, shift("labels")), _dev(table), _offset_view(frames, shift("frames")), 200, out)
    assert got is out and _same(got, want)
    tab = _offset_view(table, 1)                              # the table's own alignment does not matter either
    assert _same(hip.labels_overlay(_dev(lab), tab, _dev(frames), 200), want)


def test_edge_rule_at_row_and_frame_borders():
    table = V.overlay_table(V.default_palette(), alpha=100)
    table[:, 3] = 100
    g = np.random.default_rng(0)
    H, W = 6, 11
    frames = g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    tab = _dev(table)

    def marked(lab, edge_alpha=255):
        """The pixels the kernel treats as edge pixels: where the result differs from the no-edge result (colours and frame
        are chosen so that alpha 100 and edge_alpha never give the same three bytes)."""
        a = hip.labels_overlay(_dev(lab), tab, _dev(frames), edge_alpha).cpu().numpy()
        b = hip.labels_overlay(_dev(lab), tab, _dev(frames)).cpu().numpy()
        assert np.array_equal(a, O.overlay(lab, table, frames, edge_alpha)) and np.array_equal(b, O.overlay(lab, table, frames))
        return (a != b).any(-1)

    # column stripes: the last column of a row (label 2) and the first of the next row (label 1) differ, but are no neighbours
    stripes = np.ones((2, H, W), np.uint8)
    stripes[:, :, W - 3:] = 2
    want = np.zeros((2, H, W), bool)
    want[:, :, W - 4:W - 2] = True
    frames[:] = 7                                              # (7, 7, 7) differs from both stripe colours
    assert np.array_equal(marked(stripes), want)
    # two frames of different constant labels: no edge at all, also not where frame 0 ends and frame 1 begins
    const = np.ones((2, H, W), np.uint8)
    const[1] = 2
    assert not marked(const).any()
    # one differing pixel marks itself and its four neighbours
    single = np.ones((2, H, W), np.uint8)
    single[1, 3, 5] = 2
    cross = np.zeros((2, H, W), bool)
    cross[1, 3, 4:7] = cross[1, 2, 5] = cross[1, 4, 5] = True
    assert np.array_equal(marked(single), cross)
    # ... also in a corner, where two of them do not exist
    corner = np.ones((2, H, W), np.uint8)
    corner[0, H - 1, W - 1] = 2
    want = np.zeros((2, H, W), bool)
    want[0, H - 1, W - 2:] = want[0, H - 2, W - 1] = True
    assert np.array_equal(marked(corner), want)
    # edge_alpha = 0: outlines are pure frame; edge_alpha = None is the no-edge result (-1 at the C ABI)
    got = hip.labels_overlay(_dev(single), tab, _dev(frames), 0).cpu().numpy()
    assert np.array_equal(got[cross], frames[cross]) and np.array_equal(got, O.overlay(single, table, frames, 0))
    assert np.array_equal(O.overlay(single, table, frames, -1), O.overlay(single, table, frames))
    out = torch.empty(2, H, W, 3, dtype=torch.uint8, device="cuda")
    dl, df = _dev(single), _dev(frames)                       # (held: a temporary's memory is reused by the next allocation)
    rc = hip.load().stswin_labels_overlay(dl.data_ptr(), df.data_ptr(), tab.data_ptr(), out.data_ptr(), 2, H, W, -1,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and _same(out, O.overlay(single, table, frames))


def test_frames_argument_none_and_in_place():
    lab, frames, table = _random_case(2, 33, 67, seed=5)
    assert _same(hip.labels_overlay(_dev(lab), _dev(table), None, 255), O.overlay(lab, table, np.zeros_like(frames), 255))
    assert _same(hip.labels_overlay(_dev(lab), _dev(table)), O.overlay(lab, table))
    want = O.overlay(lab, table, frames, 90)
    for fr in (_dev(frames), _offset_view(frames, 1)):        # the wide and the byte body
        got = hip.labels_overlay(_dev(lab), _dev(table), fr, 90, out=fr)
        assert got is fr and _same(fr, want)


def test_refusals():
    lab, frames, table = (_dev(a) for a in _random_case(2, 8, 16, seed=1))
    ok = hip.labels_overlay(lab, table, frames)
    for args, kwargs in (((lab.int(), table, frames), {}), ((lab, table.int(), frames), {}), ((lab, table, frames.float()), {}),
                         ((lab[0], table, frames), {}), ((lab, table[:255], frames), {}), ((lab, table, frames[:1]), {}),
                         ((lab, table, frames[..., :2]), {}), ((lab, table, frames), dict(out=ok[:, :, :8])),
                         ((lab, table, frames), dict(out=ok.float())), ((lab[:, :, ::2], table, frames[:, :, ::2]), {}),
                         ((lab, table.cpu(), frames), {}), ((lab, table, frames), dict(edge_alpha=256)),
                         ((lab, table, frames), dict(edge_alpha=-2))):
        with pytest.raises(StswinHipError):
            hip.labels_overlay(*args, **kwargs)
    # out must not share memory with labels: the same tensor's bytes, or an overlapping window of one allocation
    buf = torch.zeros(2 * 8 * 16 * 3 + 64, dtype=torch.uint8, device="cuda")
    inside = buf[:2 * 8 * 16].view(2, 8, 16)
    with pytest.raises(StswinHipError, match="shares memory"):
        hip.labels_overlay(inside, table, frames, out=buf[64:].view(2, 8, 16, 3))
    # the C entry point's own codes
    fn, st = hip.load().stswin_labels_overlay, torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    assert fn(p(lab), p(frames), p(table), p(ok), 0, 8, 16, -1, st) == -1415
    assert fn(p(lab), p(frames), p(table), p(ok), 2, 8, -16, -1, st) == -1415
    assert fn(None, p(frames), p(table), p(ok), 2, 8, 16, -1, st) == -1416
    assert fn(p(lab), p(frames), None, p(ok), 2, 8, 16, -1, st) == -1416
    assert fn(p(lab), p(frames), p(table), None, 2, 8, 16, -1, st) == -1416
    assert fn(p(lab), p(frames), p(table), p(ok), 2, 8, 16, 256, st) == -1417
    assert fn(p(lab), p(frames), p(table), p(ok), 2, 8, 16, -2, st) == -1417


def test_capturable_into_a_graph():
    lab, frames, table = _random_case(1, 33, 67, seed=9)
    dl, df, dt = _dev(lab), _dev(frames), _dev(table)
    out = torch.zeros(1, 33, 67, 3, dtype=torch.uint8, device="cuda")
    hip.labels_overlay(dl, dt, df, 255, out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.labels_overlay(dl, dt, df, 255, out)
    lab2, frames2, _ = _random_case(1, 33, 67, seed=10)
    dl.copy_(torch.from_numpy(lab2))
    df.copy_(torch.from_numpy(frames2))
    graph.replay()
    assert _same(out, O.overlay(lab2, table, frames2, 255))


# ------------------------------------------------------------------------------------------------------- the segmenter
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


def _frames(n, hs, ws, seed):
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (1, hs, ws, 3), dtype=np.int64)
    return np.clip(base + g.integers(-24, 25, (n, hs, ws, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module", params=["endovis18", "cadis"])
def sequence(request):
    """A 10-frame sequence of 45 x 58 frames, its labels from out="labels" segmenters (without and with gt) and the table the
    overlay segmenter is expected to build."""
    protocol = request.param
    nc = 9 if protocol == "cadis" else 12
    m = _model(protocol, seed=4)
    n, size = 10, (45, 58)
    fr = _frames(n, *size, seed=12)
    g = torch.Generator().manual_seed(3)
    gt = torch.randint(0, nc - 1, (n, *size), generator=g).cuda()
    kw = dict(protocol=protocol, out_size=size)
    with torch.no_grad():
        labels = video.VideoSegmenter(m, out="labels", **kw).segment_sequence(fr)
        scored_seg = video.VideoSegmenter(m, out="labels", **kw)
        scored = scored_seg.segment_sequence(fr, gt=gt)
    transparent = (nc - 1,) if protocol == "cadis" else (0,)
    table = V.overlay_table(V.default_palette(), 128, transparent)
    assert len({int(l.max()) for l in labels} | {int(l.min()) for l in labels}) > 1, "the model predicts one class: nothing to draw"
    want = [O.overlay(labels[f].cpu().numpy()[None], table, fr[f:f + 1], 255)[0] for f in range(n)]
    return dict(protocol=protocol, m=m, fr=fr, gt=gt, size=size, labels=labels, scored=scored, scored_seg=scored_seg, table=table, want=want)


def test_segmenter_overlay_is_labels_overlay_of_its_own_labels_and_frame(sequence):
    s = sequence
    with torch.no_grad():
        seg = video.VideoSegmenter(s["m"], out="overlay", protocol=s["protocol"])
        assert seg.out_size is None
        got = {}
        order = []
        for f in range(len(s["fr"])):                        # online, one CPU frame per push: frames 0 .. 3 wait for their clips
            for g, r in seg.push(s["fr"][f]):
                got[g] = r.clone()
                order.append((f, g))
            assert set(seg._kept) <= set(range(f + 1)) - set(got) and len(seg._kept) <= seg.planner.slots
        for g, r in seg.finish():
            got[g] = r.clone()
        assert seg.out_size == s["size"] and not seg._kept and not seg._frames
    assert any(g < f for f, g in order), "no frame's result came after a later frame's push: the ordering is not exercised"
    tab = _dev(s["table"])
    for f in range(len(s["fr"])):
        assert got[f].shape == (*s["size"], 3) and _same(got[f], s["want"][f]), f
        direct = hip.labels_overlay(s["labels"][f][None], tab, _dev(s["fr"][f:f + 1]), 255)[0]
        assert torch.equal(got[f], direct), f
    assert np.array_equal(seg._table.cpu().numpy(), s["table"])


def test_segmenter_modes_and_frame_residence_give_equal_bytes(sequence):
    s = sequence
    kw = dict(out="overlay", protocol=s["protocol"])
    dev = torch.from_numpy(s["fr"]).cuda()
    with torch.no_grad():
        runs = {"batch4 cpu": video.VideoSegmenter(s["m"], batch=4, **kw).segment_sequence(s["fr"]),
                "batch4 gpu": video.VideoSegmenter(s["m"], batch=4, **kw).segment_sequence(dev),
                "online gpu": video.VideoSegmenter(s["m"], **kw).segment_sequence(dev),
                "graph cpu": video.VideoSegmenter(s["m"], graph=True, **kw).segment_sequence(s["fr"])}
        graphed = video.VideoSegmenter(s["m"], graph=True, **kw)
        gr = {}
        for f in range(len(dev)):                            # graph replay, one GPU frame per push
            for g, r in graphed.push(dev[f]):
                gr[g] = r.clone()
        gr.update((g, r.clone()) for g, r in graphed.finish())
        assert graphed._g is not None and graphed._g[4] is not None and graphed._g[4].shape == (1, *s["size"], 3)
        runs["graph gpu"] = [gr[f] for f in range(len(dev))]
    assert torch.equal(dev.cpu(), torch.from_numpy(s["fr"])), "the segmenter wrote into the pushed frames"
    for name, res in runs.items():
        for f in range(len(dev)):
            assert _same(res[f], s["want"][f]), (name, f)


def test_segmenter_with_gt_scores_as_labels_do(sequence):
    s = sequence
    kw = dict(out="overlay", protocol=s["protocol"])
    with torch.no_grad():
        eager = video.VideoSegmenter(s["m"], **kw)
        res = eager.segment_sequence(s["fr"], gt=s["gt"])
        graphed = video.VideoSegmenter(s["m"], graph=True, **kw)
        gres = graphed.segment_sequence(s["fr"], gt=s["gt"])
    for f in range(len(s["fr"])):
        if s["protocol"] == "cadis":
            assert _same(res[f], s["want"][f]) and _same(gres[f], s["want"][f]), f
        else:
            for r in (res[f], gres[f]):
                assert _same(r[0], s["want"][f]) and r[1] == s["scored"][f][1] and r[2] == s["scored"][f][2], f
    if s["protocol"] == "cadis":
        cm = s["scored_seg"].confusion_matrix()
        assert cm.sum() > 0 and np.array_equal(eager.confusion_matrix(), cm) and np.array_equal(graphed.confusion_matrix(), cm)


def test_segmenter_overlay_options_and_refusals(sequence):
    s = sequence
    m = s["m"]
    with torch.no_grad():
        seg = video.VideoSegmenter(m, out="overlay", protocol=s["protocol"], out_size=(40, 58))
        with pytest.raises(StswinHipError, match="differs from the frame size"):
            seg.push(s["fr"][0])
        cmap = {c: (10 * c, 255 - c, 3) for c in range(12)}
        custom = video.VideoSegmenter(m, out="overlay", protocol=s["protocol"], palette=cmap, alpha=255, transparent=(), edge_alpha=None)
        got = custom.segment_sequence(s["fr"])
    table = V.overlay_table(cmap, 255)
    for f in range(len(s["fr"])):
        lab = s["labels"][f].cpu().numpy()
        assert _same(got[f], O.overlay(lab[None], table, s["fr"][f:f + 1])[0]), f
        assert _same(got[f], V.mask_to_colormap(lab, cmap)), f           # opaque, no outlines: the host picture
    for kwargs in (dict(out="labels", palette=cmap), dict(out="logits", transparent=(0,)), dict(out="overlay", edge_alpha=256),
                   dict(out="overlay", alpha=300), dict(out="picture")):
        with pytest.raises(StswinHipError):
            video.VideoSegmenter(m, protocol=s["protocol"], **kwargs)
