"""hip.instance_clearance against the numpy definition (stswincl_amd/utils/instruments.py, instance_clearance).  Every comparison is
exact integer equality."""
import numpy as np
import pytest
import torch

import test_hip_confidence as Q
from stswincl_amd import hip
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I

pytestmark = pytest.mark.gpu

FRAMES = 2
FILL = 91


def _geo():
    return hip.instance_clearance_geometry()


def _blocky(shape, hi, cell, seed):
    """Random maps of upscaled random blocks, so that regions exist; values 0 .. hi - 1."""
    n, H, W = shape
    g = np.random.default_rng(seed)
    cells = g.integers(0, hi, (n, -(-H // cell[0]), -(-W // cell[1])))
    return np.ascontiguousarray(np.repeat(np.repeat(cells, cell[0], axis=1), cell[1], axis=2)[:, :H, :W].astype(np.uint8))


def _check(lab, comp, K, nc, targets=None, max_distance=None):
    """hip.instance_clearance of device labels and components equals the definition on their host copies -> the result, on the host."""
    want = I.instance_clearance(lab.cpu().numpy(), comp.cpu().numpy(), K, nc, targets, max_distance)
    got = hip.instance_clearance(lab, comp, K, nc, targets, max_distance)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (lab.shape[0], K, nc, 3)
    bad = (got.cpu() != torch.from_numpy(want)).nonzero()
    assert bad.numel() == 0, (K, nc, bad[:6].tolist(), got.cpu()[tuple(bad[0][:3])].tolist(), want[tuple(bad[0][:3])].tolist())
    return want


def _shapes():
    th, tw, _, seg = _geo()[:4]
    return [(1, 1), (1, 37), (37, 1), (th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (seg - 1, 21), (seg, 21), (seg + 1, 21),
            (2 * seg + 1, 21), (67, 131)]


IDS = ["1x1", "1x37", "37x1", "tile-1", "tile", "tile+1", "seg-1", "seg", "seg+1", "2seg+1", "67x131"]


# ------------------------------------------------------------------------------------------------ the kernel against the definition
@pytest.mark.parametrize("shape", range(len(IDS)), ids=IDS)
def test_kernel_equals_the_definition(shape):
    H, W = _shapes()[shape]
    measured = 0
    for K, nc in ((1, 12), (16, 1), (16, 12), (16, 64)):
        lab = torch.from_numpy(_blocky((FRAMES, H, W), nc + 2, (3, 7), seed=nc + K + H)).cuda()    # labels >= nc among them
        comp = hip.label_components(lab, nc, 8, (0,) if nc > 1 else (), 1024)[0]
        want = _check(lab, comp, K, nc)
        measured += int((want[..., 0] > 0).sum())
        assert not (want[..., 0] == 0).any()
    assert measured > 0 or H * W < 40


@pytest.mark.parametrize("nc,shape", [(1, (17, 65)), (12, (67, 131)), (64, (37, 67))], ids=["nc1", "nc12", "nc64"])
def test_more_components_than_instances(nc, shape):
    """K = 1024 of more components than that: blocks of 1 x 2 pixels at 4-connectivity; the ones past K are nobody's."""
    H, W = shape
    lab = torch.from_numpy(_blocky((1, H, W), nc + 2, (1, 2), seed=nc)).cuda()
    comp, _, total = hip.label_components(lab, nc, 4, (0,) if nc > 1 else (), 1024)
    if nc > 1:
        assert int(total.min()) > 1024, "fewer components than K: the truncation is not exercised"
    want = _check(lab, comp, 1024, nc)
    assert nc == 1 or int((want[..., 0] > 0).sum()) > 1024


def test_one_large_frame():
    H, W, nc, K = 540, 960, 6, 16
    lab = torch.from_numpy(_blocky((1, H, W), nc + 1, (27, 41), seed=5)).cuda()
    comp, _, total = hip.label_components(lab, nc, 8, (0,), 1024)
    assert int(total[0]) > K
    want = _check(lab, comp, K, nc)
    assert int((want[..., 0] > 0).sum()) >= K and int(want[..., 0].max()) > 81      # some past the lane's own reach


# ----------------------------------------------------------------------------------------------------------------- the search
def _two_blobs(gap, transposed, wide):
    """An instance of class 1, `wide` columns, and a blob of class 2 `gap` columns apart on a 5 x 260 map of background 0 (transposed:
    260 x 5)."""
    lab = np.zeros((1, 5, 260), np.uint8)
    lab[0, 1:4, 3:3 + wide] = 1
    lab[0, 2:4, 2 + wide + gap:4 + wide + gap] = 2
    return np.ascontiguousarray(lab.transpose(0, 2, 1)) if transposed else lab


@pytest.mark.parametrize("wide", [2, 9], ids=["one-by-one", "row-at-once"])
@pytest.mark.parametrize("transposed", [False, True], ids=["5x260", "260x5"])
@pytest.mark.parametrize("gap", [73, 137, 201])
def test_blobs_beyond_the_near_range(gap, transposed, wide):
    """wide = 2: a row of the instance leaves two pixels to the wave, which takes them one by one; wide = 9: nine, and the row searches
    at once (transposed: the top and the bottom row of three do)."""
    near, solo = _geo()[4:]
    assert gap > near + 64 and (gap - near - 1) // 64 == (73, 137, 201).index(gap) + 1      # that many steps of 64 columns past the first
    assert (wide <= solo) == (wide == 2) and 3 > solo
    lab = torch.from_numpy(_two_blobs(gap, transposed, wide)).cuda()
    comp, _, total = hip.label_components(lab, 3, 8, (0,), 8)
    assert int(total[0]) == 2 and int(comp[0, 2, 3] if not transposed else comp[0, 3, 2]) == 0
    for targets in (None, (2,), (1, 2)):
        want = _check(lab, comp, 8, 3, targets)
        assert int(want[0, 0, 2, 0]) == gap * gap and int(want[0, 1, 1, 0]) == (-1 if targets == (2,) else gap * gap)
        assert int(want[0, 0, 2, 0]) > (near + 64) ** 2
    e = 2 + wide                                                              # the instance's last column
    p, q = (2 * 260 + e, 2 * 260 + e + gap) if not transposed else (e * 5 + 2, (e + gap) * 5 + 2)
    assert want[0, 0, 2].tolist() == [gap * gap, p, q]
    cut = _check(lab, comp, 8, 3, None, gap)                                  # r^2 = d2 stays ...
    assert int(cut[0, 0, 2, 0]) == gap * gap
    cut = _check(lab, comp, 8, 3, None, gap - 1)                              # ... and anything below cuts it
    assert (cut[0, 0, 2] == -1).all() and int(cut[0, 0, 0, 0]) == 1


def test_a_class_only_beyond_the_instances_own_part():
    """A grouped arm, shaft (1) then clasper (3), with the organ (5) only to the right of the clasper: the shaft's pixels search
    across the arm's own clasper, and the clasper's are the nearest."""
    lab = np.zeros((1, 9, 140), np.uint8)
    lab[0, 3:6, 2:60], lab[0, 2:7, 60:70] = 1, 3
    lab[0, 1:8, 120:130] = 5
    lab[0, 7, 30] = 3                                                         # a clasper pixel of nobody's arm, nearer to the shaft
    nc, K = 6, 4
    t = torch.from_numpy(lab).cuda()
    grouped = torch.from_numpy(I.group_table(((1, 3),), nc)[lab]).cuda()
    comp = hip.label_components(grouped, nc, 8, (0,), K)[0]
    arm = int(comp[0, 4, 10])
    assert int(comp[0, 4, 65]) == arm
    want = _check(t, comp, K, nc)
    assert want[0, arm, 5].tolist() == [51 * 51, 2 * 140 + 69, 2 * 140 + 120] and (want[0, arm, 3] == -1).all() and (want[0, arm, 1] == -1).all()
    plain = hip.label_components(t, nc, 8, (0,), K)[0]                        # ungrouped: the shaft is measured to both claspers
    want = _check(t, plain, K, nc)
    assert int(want[0, int(plain[0, 4, 10]), 3, 0]) == 1 and int(want[0, int(plain[0, 4, 10]), 5, 0]) == 61 * 61


def test_checkerboard_at_4_connectivity():
    th, tw = _geo()[:2]
    H, W, nc, K = th + 1, tw + 1, 4, 1024
    ys, xs = np.mgrid[:H, :W]
    board = (1 + (ys + xs) % 2).astype(np.uint8)                              # every pixel its own component, every one on the query set
    other = (3 - board).astype(np.uint8)
    board[H - 1, W - 1] = other[H - 1, W - 1] = 3                             # one pixel of a third class, in nobody's instance below K
    lab = torch.from_numpy(np.stack([board, other])).cuda()
    comp, _, total = hip.label_components(lab, nc, 4, (), 1024)
    assert total.tolist() == [H * W] * 2
    want = _check(lab, comp, K, nc)
    assert int((want[0, :, 3, 0] > 0).sum()) == K
    few = (comp % 3).contiguous()                                             # the same pixels pooled into three instances that hold
    want = _check(lab, few, 3, nc)                                            # both colours: every pixel contends for the keys of class 3
    holder = (H * W - 1) % 3                                                  # the one that holds the pixel of class 3 too
    assert (want[:, :, 1:3] == -1).all() and (want[:, holder, 3] == -1).all() and int((want[0, :, 3, 0] > 0).sum()) == 2


def test_raw_ordinals_unrelated_to_the_labels():
    H, W = 67, 131
    g = np.random.default_rng(3)
    lab = torch.from_numpy(_blocky((FRAMES, H, W), 14, (2, 5), seed=9)).cuda()
    for K in (1, 16, 1024):
        raw = torch.from_numpy(np.repeat(g.integers(-1, K + 3, (FRAMES, H, -(-W // 3))), 3, axis=2)[:, :, :W].astype(np.int32).copy()).cuda()
        assert int(raw.min()) == -1 and int(raw.max()) >= K
        _check(lab, raw, K, 12)
    inner = torch.full((1, 9, 9), 2, dtype=torch.uint8, device="cuda")        # an instance that holds only inner pixels of a class
    inner[0, 0, 0] = 1
    raw = torch.full((1, 9, 9), -1, dtype=torch.int32, device="cuda")
    raw[0, 4, 4], raw[0, 0, 0] = 0, 1
    want = _check(inner, raw, 2, 3)
    assert (want[0, 0, 2] == -1).all() and want[0, 0, 1].tolist() == [32, 40, 0] and want[0, 1, 2].tolist() == [1, 0, 1]


def test_targets_and_max_distance():
    H, W, nc, K = 40, 90, 8, 16
    lab = torch.from_numpy(_blocky((FRAMES, H, W), nc + 1, (4, 9), seed=8)).cuda()
    comp = hip.label_components(lab, nc, 8, (0,), 64)[0]
    full = _check(lab, comp, K, nc)
    seen = sorted({int(v) for v in full[..., 0].reshape(-1) if v > 1})
    assert len(seen) >= 3
    for targets in ((0,), (3, 5), (7, 1, 2), ()):
        sub = _check(lab, comp, K, nc, targets)
        assert np.array_equal(sub[:, :, list(targets)], full[:, :, list(targets)]) and int((sub[..., 0] >= 0).sum()) <= int((full[..., 0] >= 0).sum())
    for r in (0, 1, 4, 9, 13, 1 << 20):
        cut = _check(lab, comp, K, nc, None, r)
        keep = (full[..., 0] >= 0) & (full[..., 0] <= r * r)
        assert np.array_equal(cut, np.where(keep[..., None], full, -1)), r


# ------------------------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("W", [48, 37])
def test_any_pointer_alignment_and_nothing_else_is_written(W):
    H, nc, K = 40, 12, 16
    labels = torch.from_numpy(_blocky((FRAMES, H, W), nc + 2, (3, 7), seed=W)).cuda()
    comps = hip.label_components(labels, nc, 8, (0,), 1024)[0]
    want = torch.from_numpy(I.instance_clearance(labels.cpu().numpy(), comps.cpu().numpy(), K, nc)).cuda()
    need = hip.instance_clearance_scratch(FRAMES, H, W, nc, K)
    for k, (lab_off, comp_off, ws_off) in enumerate(((0, 0, 0), (1, 0, 8), (0, 4, 0), (1, 4, 8), (3, 12, 8))):
        lab, lab_buf = Q._padded(labels.shape, torch.uint8, lab_off)
        lab.copy_(labels)
        cc, cc_buf = Q._padded(comps.shape, torch.int32, comp_off)
        cc.copy_(comps)
        assert lab.data_ptr() % 16 == lab_off and cc.data_ptr() % 16 == comp_off
        out, out_buf = Q._padded((FRAMES, K, nc, 3), torch.int64, 8 * (k % 2), fill=-5)
        ws, ws_buf = Q._padded((need,), torch.uint8, ws_off, fill=FILL)
        for again in range(2):                                                # a second call overwrites, whatever the workspace held
            got = hip.instance_clearance(lab, cc, K, nc, out=out, workspace=ws)
            assert got is out and torch.equal(out, want), (lab_off, comp_off, again)
            ws.fill_((37 * k + 255) % 256)
        ws.fill_(FILL)
        got = hip.instance_clearance(lab, cc, K, nc, (2, 3), 6, out=out, workspace=ws)      # other keywords into the same out
        assert torch.equal(got.cpu(), torch.from_numpy(I.instance_clearance(labels.cpu().numpy(), comps.cpu().numpy(), K, nc, (2, 3), 6)))
        assert Q._sentinels_hold(out, out_buf, -5) and Q._sentinels_hold(ws, ws_buf, FILL)
        assert Q._sentinels_hold(lab, lab_buf) and Q._sentinels_hold(cc, cc_buf) and torch.equal(lab, labels) and torch.equal(cc, comps)


def test_the_call_is_capturable():
    th, tw = _geo()[:2]
    n, H, W, nc, K = 2, th + 5, tw + 32, 6, 16
    maps = [_blocky((n, H, W), nc + 1, cell, seed=s) for cell, s in (((3, 7), 1), ((5, 4), 2), ((2, 11), 3))]
    lab = torch.empty(n, H, W, dtype=torch.uint8, device="cuda")
    comp = torch.empty(n, H, W, dtype=torch.int32, device="cuda")
    out = torch.full((n, K, nc, 3), FILL, dtype=torch.int64, device="cuda")
    ws = torch.empty(hip.instance_clearance_scratch(n, H, W, nc, K), dtype=torch.uint8, device="cuda")

    def load(m):
        lab.copy_(torch.from_numpy(m))
        comp.copy_(hip.label_components(lab, nc, 8, (0,), 64)[0])

    load(maps[0])
    hip.instance_clearance(lab, comp, K, nc, out=out, workspace=ws)           # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.instance_clearance(lab, comp, K, nc, out=out, workspace=ws)
    for m in maps[1:] + maps[:1]:                                             # replayed with changed inputs
        load(m)
        out.fill_(FILL)
        graph.replay()
        assert torch.equal(out.cpu(), torch.from_numpy(I.instance_clearance(m, comp.cpu().numpy(), K, nc)))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_wrapper_and_abi_refusals():
    lab = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    cc = torch.zeros(2, 8, 10, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 4, 3, 3, dtype=torch.int64, device="cuda")
    need = hip.instance_clearance_scratch(2, 8, 10, 3, 4)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    for a, b, kw, what in ((lab[0], cc[0], {}, "labels"), (lab.int(), cc, {}, "labels"), (lab, cc.long(), {}, "components"),
                           (lab, cc[:1], {}, "components"), (lab[:, :, ::2], cc[:, :, ::2], {}, "labels"), (lab.cpu(), cc, {}, "GPU"),
                           (lab, cc.cpu(), {}, "GPU"), ("labels", cc, {}, "labels"), (lab[:0], cc[:0], {}, "empty"),
                           (lab, cc, dict(K=0), "K"), (lab, cc, dict(K=1025), "K"), (lab, cc, dict(K=4.0), "K"), (lab, cc, dict(K=True), "K"),
                           (lab, cc, dict(nc=0), "nc"), (lab, cc, dict(nc=65), "nc"), (lab, cc, dict(nc=3.0), "nc"),
                           (lab, cc, dict(targets=(3,)), "targets"), (lab, cc, dict(targets=(-1,)), "targets"),
                           (lab, cc, dict(targets=(1.0,)), "targets"), (lab, cc, dict(targets=(True,)), "targets"),
                           (lab, cc, dict(max_distance=-1), "max_distance"), (lab, cc, dict(max_distance=2.0), "max_distance"),
                           (lab, cc, dict(max_distance=True), "max_distance"),
                           (lab, cc, dict(out=out[:, :3]), "out"), (lab, cc, dict(out=out.int()), "out"), (lab, cc, dict(out=out.cpu()), "out"),
                           (lab, cc, dict(out=(out,)), "out"), (lab, cc, dict(workspace=ws[:need - 1]), "workspace"),
                           (lab, cc, dict(workspace=ws[1:]), "workspace"), (lab, cc, dict(workspace=ws.int()), "workspace"),
                           (lab, cc, dict(workspace=ws.cpu()), "workspace"), (lab, cc, dict(workspace=ws.view(2, -1)), "workspace")):
        with pytest.raises(StswinHipError, match="instance_clearance.*" + what):
            hip.instance_clearance(a, b, **{"K": 4, "nc": 3, **kw})
    both = torch.zeros(640, dtype=torch.uint8, device="cuda")                  # out over the labels' own bytes, over the components', in the
    shared = both[:576].view(torch.int64).view(2, 4, 3, 3)                    # workspace
    for kw in (dict(labels=both[:160].view(2, 8, 10), out=shared), dict(components=both[:640].view(torch.int32).view(2, 8, 10), out=shared),
               dict(out=ws[:576].view(torch.int64).view(2, 4, 3, 3), workspace=ws), dict(labels=ws[8:168].view(2, 8, 10), workspace=ws)):
        with pytest.raises(StswinHipError, match="shares memory"):
            hip.instance_clearance(**{**dict(labels=lab, components=cc, K=4, nc=3), **kw})
    lib = hip.load()
    p = (lab.data_ptr(), cc.data_ptr(), out.data_ptr())
    tail = (ws.data_ptr(), ws.numel(), None)
    assert lib.stswin_instance_clearance(*p, 0, 8, 10, 3, 4, 7, -1, *tail) == -1920
    assert lib.stswin_instance_clearance(*p, 2, 8, 16385, 3, 4, 7, -1, *tail) == -1920
    assert lib.stswin_instance_clearance(*p, 2, 0, 10, 3, 4, 7, -1, *tail) == -1920
    assert lib.stswin_instance_clearance(p[0], None, p[2], 2, 8, 10, 3, 4, 7, -1, *tail) == -1921
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 3, 4, 7, -1, None, ws.numel(), None) == -1921
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 0, 4, 7, -1, *tail) == -1922
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 65, 4, 7, -1, *tail) == -1922
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 3, 0, 7, -1, *tail) == -1923
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 3, 1025, 7, -1, *tail) == -1923
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 3, 4, 7, -1, ws.data_ptr(), need - 1, None) == -1924
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 3, 4, 7, -1, ws.data_ptr() + 4, need, None) == -1924
    assert lib.stswin_instance_clearance(p[0], p[1] + 2, p[2], 2, 8, 10, 3, 4, 7, -1, *tail) == -1925
    assert lib.stswin_instance_clearance(p[0], p[1], p[2] + 4, 2, 8, 10, 3, 4, 7, -1, *tail) == -1925
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 3, 4, 7, -2, *tail) == -1926
    torch.cuda.synchronize()
    out.fill_(7)
    assert lib.stswin_instance_clearance(*p, 2, 8, 10, 3, 2000, 7, -1, *tail) == -1923
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                             # refused before anything was launched
    with pytest.raises(StswinHipError, match="instance_clearance"):
        hip.instance_clearance_scratch(1, 16385, 4, 3, 4)
