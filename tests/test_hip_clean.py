"""hip.labels_clean against the definition (stswincl_amd/utils/instruments.py, clean_labels) and hip.labels_score against the fused
counting launches and numpy.  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

import test_hip_components as C
import test_hip_confidence as Q
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I

pytestmark = pytest.mark.gpu

FRAMES = 3
# (nc, values, cell, connectivity, min_area, keep, max_small): nc in (1, 12, 64) with labels >= nc among the `values` distinct ones where
# values > nc, both connectivities, min_area in (2, 9, 200), keep empty and not, max_small in (1, 16, 4096).  The cases of 1 x 2 blocks
# at 4-connectivity hold more small components than max_small.
SWEEP = [(1, 3, (3, 7), 8, 2, (), 4096),
         (12, 3, (1, 2), 4, 9, (2,), 16),
         (12, 14, (3, 7), 8, 200, (), 4096),
         (64, 66, (1, 2), 4, 9, (0, 5), 1),
         (64, 5, (2, 3), 8, 9, (), 4096),
         (12, 14, (1, 1), 4, 2, (1, 3), 16),
         (12, 6, (4, 6), 4, 200, (1,), 4096)]


def _geo():
    return hip.labels_clean_geometry()


def _blocky(shape, hi, cell, seed):
    """Random maps of upscaled random blocks, so that runs exist; values 0 .. hi - 1."""
    n, H, W = shape
    g = np.random.default_rng(seed)
    cells = g.integers(0, hi, (n, -(-H // cell[0]), -(-W // cell[1])))
    return np.ascontiguousarray(np.repeat(np.repeat(cells, cell[0], axis=1), cell[1], axis=2)[:, :H, :W].astype(np.uint8))


def _check(lab, nc, min_area, conn=8, keep=(), max_small=4096):
    """hip.labels_clean of the host labels equals the definition -> (out, stats), the reference's, on the host."""
    want, wstats = I.clean_labels(lab, nc, min_area, conn, keep, max_small)
    dev = torch.from_numpy(lab).cuda()
    got, stats = hip.labels_clean(dev, nc, min_area, conn, keep, max_small)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == lab.shape
    assert stats.is_cuda and stats.dtype == torch.int32 and tuple(stats.shape) == (lab.shape[0], 2)
    assert stats.cpu().tolist() == wstats.tolist(), (nc, min_area, conn, keep, max_small)
    bad = (got.cpu() != torch.from_numpy(want)).nonzero()
    assert bad.numel() == 0, (nc, min_area, conn, keep, max_small, bad[:6].tolist())
    assert torch.equal(dev.cpu(), torch.from_numpy(lab))                     # the input is unchanged
    return want, wstats


def _shapes():
    g0, g1 = _geo()[:2]
    return [(1, 1), (1, 37), (37, 1), (g0 - 1, g1 - 1), (g0, g1), (g0 + 1, g1 + 1), (67, 131), (135, 240)]


@pytest.mark.parametrize("shape", range(8), ids=["1x1", "1x37", "37x1", "tile-1", "tile", "tile+1", "67x131", "135x240"])
def test_kernel_equals_the_definition(shape):
    H, W = _shapes()[shape]
    chunk = _geo()[2]
    assert shape != 7 or (H * W > 2 * chunk and H > 2 * _geo()[0] and W > _geo()[1])
    changed = truncated = 0
    for nc, values, cell, conn, min_area, keep, max_small in SWEEP:
        lab = _blocky((FRAMES, H, W), values, cell, seed=nc + min_area + H)
        assert values <= nc or H * W < 1000 or int(lab.max()) >= nc
        _, stats = _check(lab, nc, min_area, conn, keep, max_small)
        changed += int(stats[:, 1].sum())
        if cell == (1, 2) and H * W >= (37 if max_small == 1 else 3000):     # more small components than max_small: the truncation
            assert (stats[:, 0] > max_small).all(), (nc, max_small, stats.tolist())
            truncated += 1
    assert changed > 0 or H * W < 37
    assert truncated >= 1 or H * W < 37


def test_more_small_components_in_a_tile_than_the_table_has_slots():
    g0, g1, _, slots = _geo()
    H, W = g0 + 1, g1 + 1
    ys, xs = np.mgrid[:H, :W]
    board = (1 + (ys + xs) % 2).astype(np.uint8)                             # a checkerboard of two classes: at 4-connectivity every
    base = np.stack([board, 3 - board, board])                               # pixel is a small component of its own
    assert g0 * g1 > slots
    for max_small in (4096, 65536):
        out, stats = _check(base, 3, 2, 4, (), max_small)
        assert np.array_equal(out, base) and stats.tolist() == [[H * W, 0]] * 3
    lab = base.copy()
    lab[:, :8, :8] = 0                                                       # one stable block in the first tile's corner: its border
    out, stats = _check(lab, 3, 2, 4, (), 65536)                             # pixels vote, and the tile's table has long been full
    assert stats.tolist() == [[H * W - 64, 16]] * 3 and (out[:, 8, :8] == 0).all() and (out[:, :8, 8] == 0).all()
    lab = base.copy()
    lab[:, -8:, -8:] = 0                                                     # the same in the last pixels of the first tile and beyond
    out, stats = _check(lab, 3, 2, 4, (), 65536)
    assert stats.tolist() == [[H * W - 64, 16]] * 3


@pytest.mark.parametrize("W", [48, 37])
def test_any_pointer_alignment_and_nothing_else_is_written(W):
    H, nc = 40, 12
    host = _blocky((FRAMES, H, W), 5, (2, 3), seed=W)
    want, wstats = I.clean_labels(host, nc, 9, 8, (1,), 16)
    assert wstats[:, 1].sum() > 0
    labels = torch.from_numpy(host).cuda()
    need = hip.labels_clean_scratch(FRAMES, H, W, nc, 16)
    for lab_off, out_off, ws_off in ((0, 0, 0), (1, 0, 0), (0, 1, 4), (3, 2, 8), (0, 0, 12), (5, 5, 0)):
        lab, lab_buf = Q._padded(labels.shape, torch.uint8, lab_off)
        lab.copy_(labels)
        out, out_buf = Q._padded(labels.shape, torch.uint8, out_off, fill=201)
        ws, ws_buf = Q._padded((need,), torch.uint8, ws_off, fill=99)
        assert lab.data_ptr() % 16 == lab_off and out.data_ptr() % 16 == out_off and ws.data_ptr() % 16 == ws_off
        for _ in range(2):                                                   # a second call into the same outputs overwrites
            got, stats = hip.labels_clean(lab, nc, 9, 8, (1,), 16, out=out, workspace=ws)
            assert got is out
            assert torch.equal(out.cpu(), torch.from_numpy(want)) and stats.cpu().tolist() == wstats.tolist(), (lab_off, out_off, ws_off)
        assert Q._sentinels_hold(out, out_buf, 201) and Q._sentinels_hold(lab, lab_buf) and Q._sentinels_hold(ws, ws_buf, 99)
        assert torch.equal(lab, labels)


def test_wrapper_and_abi_refusals():
    lab = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(lab)
    ws = torch.zeros(hip.labels_clean_scratch(2, 8, 10, 3, 8), dtype=torch.uint8, device="cuda")
    for a, kw in ((lab[0], {}), (lab.int(), {}), (lab[:, :, ::2], {}), (lab.cpu(), {}), ("labels", {}), (lab, dict(nc=0)), (lab, dict(nc=65)),
                  (lab, dict(nc=True)), (lab, dict(min_area=1)), (lab, dict(min_area=(1 << 30) + 1)), (lab, dict(min_area=2.0)),
                  (lab, dict(connectivity=6)), (lab, dict(keep=(64,))), (lab, dict(keep=(1.0,))), (lab, dict(max_small=0)),
                  (lab, dict(max_small=65537)), (lab, dict(out=out[:1])), (lab, dict(out=out.int())), (lab, dict(out=out.cpu())),
                  (lab, dict(out=lab)), (lab, dict(workspace=ws[:-1])), (lab, dict(workspace=ws.int())), (lab, dict(workspace=ws.cpu())),
                  (lab, dict(workspace=torch.zeros(ws.numel() + 8, dtype=torch.uint8, device="cuda")[1:]))):
        with pytest.raises(StswinHipError, match="labels_clean"):
            hip.labels_clean(a, **{"nc": 3, "min_area": 2, "max_small": 8, **kw})
    both = torch.zeros(4 * 160, dtype=torch.uint8, device="cuda")
    with pytest.raises(StswinHipError, match="shares memory"):              # out over a part of the labels' own bytes
        hip.labels_clean(both[:160].view(2, 8, 10), 3, 2, out=both[80:240].view(2, 8, 10))
    with pytest.raises(StswinHipError, match="labels_clean"):
        hip.labels_clean_scratch(1, 16385, 4, 3)
    lib = hip.load()
    stats = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
    out.fill_(7)
    torch.cuda.synchronize()
    p = (lab.data_ptr(), out.data_ptr(), stats.data_ptr())
    tail = (ws.data_ptr(), ws.numel(), None)
    assert lib.stswin_labels_clean(*p, 0, 8, 10, 3, 8, 0, 2, 8, *tail) == -1900
    assert lib.stswin_labels_clean(*p, 2, 8, 16385, 3, 8, 0, 2, 8, *tail) == -1900
    assert lib.stswin_labels_clean_scratch(2, 0, 10, 3, 8) == -1900
    assert lib.stswin_labels_clean(None, p[1], p[2], 2, 8, 10, 3, 8, 0, 2, 8, *tail) == -1901
    assert lib.stswin_labels_clean(p[0], None, p[2], 2, 8, 10, 3, 8, 0, 2, 8, *tail) == -1901
    assert lib.stswin_labels_clean(p[0], p[1], None, 2, 8, 10, 3, 8, 0, 2, 8, *tail) == -1901
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 8, 0, 2, 8, None, ws.numel(), None) == -1901
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 0, 8, 0, 2, 8, *tail) == -1902
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 65, 8, 0, 2, 8, *tail) == -1902
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 6, 0, 2, 8, *tail) == -1903
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 8, 0, 1, 8, *tail) == -1904
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 8, 0, (1 << 30) + 1, 8, *tail) == -1904
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 8, 0, 2, 0, *tail) == -1905
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 8, 0, 2, 65537, *tail) == -1905
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 8, 0, 2, 8, ws.data_ptr(), ws.numel() - 1, None) == -1906
    assert lib.stswin_labels_clean(*p, 2, 8, 10, 3, 8, 0, 2, 8, ws.data_ptr() + 2, ws.numel() - 2, None) == -1906
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((stats == 7).all())               # refused before anything was launched


# ----------------------------------------------------------------------------------------------------------------- labels_score
def _numpy_counts(lab, gt, nc):
    out = np.zeros((lab.shape[0], 3, nc), dtype=np.int32)
    for f in range(lab.shape[0]):
        for c in range(nc):
            out[f, :, c] = ((gt[f] == c).sum(), (lab[f] == c).sum(), ((gt[f] == c) & (lab[f] == c)).sum())
    return out


def _numpy_cm(lab, gt, ncm):
    ok = (gt >= 0) & (gt < ncm) & (lab < ncm)
    return np.bincount(gt[ok] * ncm + lab[ok].astype(np.int64), minlength=ncm * ncm).reshape(ncm, ncm)


@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_score_equals_the_fused_launches_on_the_model_s_logits(protocol):
    c = C._case(protocol)
    nc, (H, W) = c["nc"], C.SIZE
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], out="logits", protocol=protocol)
        logits = torch.stack(seg.segment_sequence(c["seqs"][0]["fr"])[:FRAMES]).float().contiguous()
    gt = c["seqs"][0]["gt"][:FRAMES].clone()
    gt[:, 0, :5] = torch.tensor([-1, 255, nc, 64, 1000])                      # values outside the range are ignored
    gt = gt.cuda()
    labels, counts = hip.upsample_argmax(logits, H, W, gt)
    got, none = hip.labels_score(labels, gt, nc)
    assert none is None and got.dtype == torch.int32 and torch.equal(got, counts)
    assert np.array_equal(got.cpu().numpy(), _numpy_counts(labels.cpu().numpy(), gt.cpu().numpy(), nc))
    for align in (True, False):
        for ncm in (nc, nc - 1, 3):
            cm = torch.zeros(ncm, ncm, dtype=torch.int64, device="cuda")
            lab = hip.upsample_argmax_cm(logits, H, W, gt=gt, cm=cm, align_corners=align)
            mine = torch.zeros_like(cm)
            both = torch.zeros(FRAMES, 3, nc, dtype=torch.int32, device="cuda")
            got = hip.labels_score(lab, gt, nc, counts=both, cm=mine)
            assert got[0] is both and got[1] is mine and torch.equal(mine, cm), (align, ncm)
            assert np.array_equal(both.cpu().numpy(), _numpy_counts(lab.cpu().numpy(), gt.cpu().numpy(), nc))
            hip.labels_score(lab, gt, nc, cm=mine)                           # the matrix accumulates; counts are not touched
            assert torch.equal(mine, 2 * cm) and np.array_equal(both.cpu().numpy(), _numpy_counts(lab.cpu().numpy(), gt.cpu().numpy(), nc))


@pytest.mark.parametrize("shape", [(3, 67, 131), (2, 64, 80), (1, 1, 1)])
def test_score_equals_numpy_on_random_maps(shape):
    g = np.random.default_rng(shape[1])
    for nc, ncm in ((1, 1), (12, 9), (64, 64)):
        lab = g.integers(0, min(nc + 3, 256), shape).astype(np.uint8)
        gt = g.integers(-2, nc + 3, shape).astype(np.int64)
        gt.reshape(-1)[0] = (1 << 32) + 1                                    # no class, whatever its low bits say
        for off in (0, 1, 3):
            dl, _ = Q._padded(shape, torch.uint8, off)
            dl.copy_(torch.from_numpy(lab))
            dg = torch.from_numpy(gt).cuda()
            cm = torch.zeros(ncm, ncm, dtype=torch.int64, device="cuda")
            counts, _ = hip.labels_score(dl, dg, nc, cm=cm, counts=torch.zeros(shape[0], 3, nc, dtype=torch.int32, device="cuda"))
            assert np.array_equal(counts.cpu().numpy(), _numpy_counts(lab, gt, nc)), (nc, off)
            assert np.array_equal(cm.cpu().numpy(), _numpy_cm(lab, gt, ncm)), (nc, off)


def test_score_refusals():
    lab = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    gt = torch.zeros(2, 8, 10, dtype=torch.int64, device="cuda")
    cm = torch.zeros(3, 3, dtype=torch.int64, device="cuda")
    for a, b, kw in ((lab[0], gt[0], {}), (lab.int(), gt, {}), (lab, gt.int(), {}), (lab, gt[:1], {}), (lab.cpu(), gt, {}), (lab, gt.cpu(), {}),
                     (lab, gt, dict(nc=0)), (lab, gt, dict(nc=65)), (lab, gt, dict(counts=torch.zeros(2, 3, 4, dtype=torch.int32, device="cuda"))),
                     (lab, gt, dict(counts=torch.zeros(2, 3, 3, device="cuda"))), (lab, gt, dict(cm=cm.int())), (lab, gt, dict(cm=cm[:2])),
                     (lab, gt, dict(cm=torch.zeros(65, 65, dtype=torch.int64, device="cuda"))), (lab, gt, dict(cm=gt.view(-1)[:9].view(3, 3)))):
        with pytest.raises(StswinHipError, match="labels_score"):
            hip.labels_score(a, b, **{"nc": 3, **kw})
    lib = hip.load()
    counts = torch.zeros(2, 3, 3, dtype=torch.int32, device="cuda")
    p = (lab.data_ptr(), gt.data_ptr(), counts.data_ptr(), cm.data_ptr())
    assert lib.stswin_labels_score(*p, 3, 0, 8, 10, 3, None) == -1910
    assert lib.stswin_labels_score(*p, 3, 2, 8, 16385, 3, None) == -1910
    assert lib.stswin_labels_score(None, p[1], p[2], p[3], 3, 2, 8, 10, 3, None) == -1911
    assert lib.stswin_labels_score(p[0], None, p[2], p[3], 3, 2, 8, 10, 3, None) == -1911
    assert lib.stswin_labels_score(p[0], p[1], None, None, 3, 2, 8, 10, 3, None) == -1911
    assert lib.stswin_labels_score(*p, 3, 2, 8, 10, 0, None) == -1912
    assert lib.stswin_labels_score(*p, 65, 2, 8, 10, 3, None) == -1912
    assert lib.stswin_labels_score(p[0], p[1] + 4, p[2], p[3], 3, 2, 8, 10, 3, None) == -1913
    assert lib.stswin_labels_score(p[0], p[1], p[2] + 2, p[3], 3, 2, 8, 10, 3, None) == -1913
    assert lib.stswin_labels_score(p[0], p[1], p[2], p[3] + 4, 3, 2, 8, 10, 3, None) == -1913
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0 and int(cm.sum()) == 0                     # refused before anything was launched
    assert lib.stswin_labels_score(p[0], p[1], p[2], None, 65, 2, 8, 10, 3, None) == 0      # ncm is checked only with cm
    torch.cuda.synchronize()
    assert counts[:, :, 0].cpu().tolist() == [[80, 80, 80]] * 2
