"""utils.instruments.instance_clearance, the numpy definition of hip.instance_clearance, against an all-pairs brute force written
here; ClearanceReport; and what of the ABI and of VideoSegmenter(clearance=...) needs no GPU.  Exact integers throughout."""
import numpy as np
import pytest
import torch

from stswincl_amd import hip, video_report
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I


def _blocky(shape, lo, hi, cell, seed):
    """Random maps of upscaled random blocks; values lo .. hi - 1."""
    n, H, W = shape
    g = np.random.default_rng(seed)
    cells = g.integers(lo, hi, (n, -(-H // cell[0]), -(-W // cell[1])))
    return np.ascontiguousarray(np.repeat(np.repeat(cells, cell[0], axis=1), cell[1], axis=2)[:, :H, :W])


def brute(labels, components, K, nc, targets=None, max_distance=None):
    """The issue's sentences, literally: every pixel of the instance against every pixel of the class."""
    n, H, W = labels.shape
    out = np.full((n, K, nc, 3), -1, dtype=np.int64)
    targets = range(nc) if targets is None else targets
    for f in range(n):
        for i in range(K):
            P = np.argwhere(components[f] == i)                                  # raster order
            if not len(P):
                continue
            own = set(labels[f][components[f] == i].tolist())
            for c in targets:
                Q = np.argwhere(labels[f] == c)
                if not len(Q) or c in own:
                    continue
                d = ((P[:, None, :].astype(np.int64) - Q[None, :, :]) ** 2).sum(axis=2)
                d2 = int(d.min())
                if max_distance is not None and d2 > max_distance ** 2:
                    continue
                k = int(np.flatnonzero(d.min(axis=1) == d2)[0])
                j = int(np.flatnonzero(d[k] == d2)[0])
                out[f, i, c] = d2, P[k, 0] * W + P[k, 1], Q[j, 0] * W + Q[j, 1]
    return out


CASES = [((2, 24, 31), 6, (3, 4), 8), ((2, 17, 23), 4, (2, 3), 4), ((3, 9, 14), 12, (1, 2), 8), ((1, 1, 1), 3, (1, 1), 8),
         ((1, 1, 19), 3, (1, 3), 8), ((1, 19, 1), 3, (3, 1), 8)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_definition_equals_all_pairs(case):
    shape, nc, cell, conn = CASES[case]
    lab = _blocky(shape, 0, nc + 2, cell, seed=case + 20).astype(np.uint8)       # labels >= nc among them
    comp = I.label_components(lab, nc, conn, (0,), 1024)[0]
    measured = 0
    for K in (1, 5, 64):
        got = I.instance_clearance(lab, comp, K, nc)
        assert got.dtype == np.int64 and got.shape == (shape[0], K, nc, 3)
        assert np.array_equal(got, brute(lab, comp.astype(np.int64), K, nc)), K
        measured += int((got[..., 0] >= 0).sum())
        assert not (got[..., 0] == 0).any()                                      # an instance never holds the class it is measured to
    assert measured > 0 or shape[1] * shape[2] == 1
    sub = (0, nc - 1) if nc > 4 else (1,)
    got = I.instance_clearance(lab, comp, 5, nc, targets=sub)
    assert np.array_equal(got, brute(lab, comp.astype(np.int64), 5, nc, targets=sub))
    assert (got[:, :, [c for c in range(nc) if c not in sub]] == -1).all()


def test_ties_take_the_first_pixels_in_raster_order():
    lab = np.zeros((1, 7, 9), np.uint8)
    lab[0, 2:5, 3:6] = 1                                                         # a square, class 2 two pixels away on all four sides
    lab[0, 0, 4], lab[0, 6, 4], lab[0, 3, 1], lab[0, 3, 7] = 2, 2, 2, 2
    comp = np.where(lab == 1, 0, -1)
    got = I.instance_clearance(lab, comp, 2, 3)
    assert got[0, 0, 2].tolist() == [4, 2 * 9 + 4, 0 * 9 + 4]                    # p: the square's top row; q: the pixel above
    assert got[0, 0, 0].tolist() == [1, 2 * 9 + 3, 1 * 9 + 3]                    # background: the corner's upper neighbour, not its left
    assert (got[0, 0, 1] == -1).all() and (got[0, 1] == -1).all()                # own class; an empty ordinal
    assert np.array_equal(got, brute(lab, comp, 2, 3))
    lab[0, 2, 4] = 0                                                             # the top row's middle gone: p's candidates at d2 = 4 are
    comp = np.where(lab == 1, 0, -1)                                             # (3, 3) left, (3, 4) up, (3, 5) right, (4, 4) down
    got = I.instance_clearance(lab, comp, 1, 3)
    assert got[0, 0, 2].tolist() == [4, 3 * 9 + 3, 3 * 9 + 1]
    assert np.array_equal(got, brute(lab, comp, 1, 3))


def test_own_classes_of_a_grouped_instrument_are_not_measured():
    """Two shaft (1) - wrist (2) - clasper (3) chains on background 0, a needle (4) near the first one, an organ (5) below."""
    lab = np.zeros((1, 12, 16), np.uint8)
    lab[0, 1, 1:4], lab[0, 1, 4:6], lab[0, 1, 6:8] = 1, 2, 3
    lab[0, 3, 9] = 4
    lab[0, 6, 2:6], lab[0, 6, 6], lab[0, 5:8, 7] = 1, 2, 3
    lab[0, 10:, 3:9] = 5
    nc, K = 6, 4
    comp = I.label_components(I.group_table(((1, 2, 3),), nc)[lab], nc, 8, (0,), K)[0]
    got = I.instance_clearance(lab, comp, K, nc)
    assert np.array_equal(got, brute(lab, comp.astype(np.int64), K, nc))
    arm = int(comp[0, 1, 1])
    assert (got[0, arm, 1:4] == -1).all()                                        # shaft, wrist, clasper: its own, though the other arm has them
    assert got[0, arm, 4].tolist() == [8, 1 * 16 + 7, 3 * 16 + 9] and got[0, arm, 5, 0] == 81
    needle = int(comp[0, 3, 9])
    assert got[0, needle, 3].tolist() == [8, 3 * 16 + 9, 1 * 16 + 7] and (got[0, needle, 4] == -1).all()
    plain = I.label_components(lab, nc, 8, (0,), 8)[0]                           # ungrouped: a shaft is measured to the wrist it touches
    got = I.instance_clearance(lab, plain, 8, nc)
    assert got[0, int(plain[0, 1, 1]), 2].tolist() == [1, 1 * 16 + 3, 1 * 16 + 4]
    assert np.array_equal(got, brute(lab, plain.astype(np.int64), 8, nc))


def test_raw_ordinals_and_labels_outside_their_ranges():
    g = np.random.default_rng(11)
    lab = _blocky((2, 13, 22), 0, 9, (2, 3), seed=4).astype(np.int64)            # classes 0 .. 8 of which nc = 6 count
    for K in (1, 3):
        raw = np.repeat(g.integers(-1, K + 3, (2, 13, 8)), 3, axis=2)[:, :, :22]
        assert raw.min() == -1 and raw.max() >= K
        got = I.instance_clearance(lab, raw, K, 6)
        assert np.array_equal(got, brute(lab, raw, K, 6))
    one = I.instance_clearance(lab[0], raw[0], K, 6)                             # one [H][W] each
    assert np.array_equal(one, got[:1])


def test_max_distance_cuts_at_r_squared():
    lab = np.zeros((1, 8, 20), np.uint8)
    lab[0, 1, 1], lab[0, 5, 4], lab[0, 1, 15] = 1, 2, 3                          # 1 -> 2: d2 = 25; 1 -> 3: d2 = 196
    comp = np.where(lab == 1, 0, -1)
    free = I.instance_clearance(lab, comp, 1, 4)
    assert free[0, 0, :, 0].tolist() == [1, -1, 25, 196]
    assert np.array_equal(I.instance_clearance(lab, comp, 1, 4, max_distance=14), free)      # r^2 = d2: still in
    got = I.instance_clearance(lab, comp, 1, 4, max_distance=13)                              # r^2 = 169 < 196
    assert got[0, 0, :, 0].tolist() == [1, -1, 25, -1] and (got[0, 0, 3] == -1).all()
    assert I.instance_clearance(lab, comp, 1, 4, max_distance=5)[0, 0, :, 0].tolist() == [1, -1, 25, -1]
    assert I.instance_clearance(lab, comp, 1, 4, max_distance=4)[0, 0, :, 0].tolist() == [1, -1, -1, -1]
    assert (I.instance_clearance(lab, comp, 1, 4, max_distance=0) == -1).all()
    rnd = _blocky((2, 16, 21), 0, 6, (3, 3), seed=2).astype(np.uint8)
    cc = I.label_components(rnd, 6, 8, (0,), 64)[0]
    full = I.instance_clearance(rnd, cc, 8, 6)
    for r in (1, 2, 3, 5):                                                       # r^2 and r^2 - 1 on random maps: d2 <= r^2 stays, as it was
        cut = I.instance_clearance(rnd, cc, 8, 6, max_distance=r)
        keep = (full[..., 0] >= 0) & (full[..., 0] <= r * r)
        assert np.array_equal(cut, np.where(keep[..., None], full, -1)) and np.array_equal(cut, brute(rnd, cc.astype(np.int64), 8, 6, None, r))


def test_definition_refusals():
    lab, comp = np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 4), np.int32)
    for kw in (dict(labels=lab.astype(np.float32)), dict(components=comp[:, :2]), dict(K=0), dict(K=1025), dict(nc=0), dict(nc=65),
               dict(targets=(3,)), dict(targets=(-1,)), dict(targets=5), dict(max_distance=-1), dict(max_distance=1.5)):
        with pytest.raises(ValueError, match="instance_clearance"):
            I.instance_clearance(**{**dict(labels=lab, components=comp, K=2, nc=3), **kw})


# ----------------------------------------------------------------------------------------------------------- ClearanceReport
def test_clearance_report_rows_names_and_joins():
    lab = np.zeros((2, 9, 16), np.uint8)
    for f, dx in enumerate((0, 3)):                                              # the instrument moves three pixels to the right
        lab[f, 1, 1 + dx:4 + dx], lab[f, 1, 4 + dx:6 + dx], lab[f, 1, 6 + dx:8 + dx] = 1, 2, 3
        lab[f, 2, 7 + dx] = 4
        lab[f, 7, 12] = 5
    nc, K = 6, 4
    comp, rows, total = I.label_components(I.group_table(((1, 2, 3),), nc)[lab], nc, 8, (0,), K)
    cl = I.instance_clearance(lab, comp, K, nc)
    names = ["background", "instrument", "wrist", "clasper", "needle", "organ"]
    inst = I.InstanceReport.from_rows(rows, total, (9, 16), names=names)
    tracker = I.InstanceTracker(K)
    ids, started = zip(*(tracker.update(comp[f], rows[f], total[f]) for f in range(2)))
    trk = I.TrackReport.from_ids(inst, np.stack(ids), np.asarray(started))
    rep = I.ClearanceReport(cl, (9, 16), names, frames=[4, 5], sequences=[0, 0], tracks=trk)
    assert len(rep) == 2 and rep.instances is inst and rep.measured.shape == (2, K, nc) and np.array_equal(rep.clearance, cl)
    assert rep.distance(0, 0) == {0: 1.0, 4: 1.0, 5: np.sqrt(61.0)} and rep.distance(0, 3) == {}
    assert rep.nearest(0, 0, 5) == ((1, 7), (7, 12)) and rep.nearest(1, 0, 5) == ((1, 10), (7, 12)) and rep.nearest(0, 0, 1) is None
    assert rep.distance(1, 0)[5] == np.sqrt(40.0)
    got = rep.as_rows()
    assert [(r["frame"], r["instance"], r["class"], r["name"], r["track"]) for r in got] == [
        (4, 0, 1, "instrument", 0), (4, 1, 4, "needle", 1), (4, 2, 5, "organ", 2),
        (5, 0, 1, "instrument", 0), (5, 1, 4, "needle", 3), (5, 2, 5, "organ", 2)]
    assert got[1]["distance"][3] == 1.0 and got[1]["nearest"][3] == ((2, 7), (1, 7)) and sorted(got[1]["distance"]) == [0, 1, 2, 3, 5]
    bare = I.ClearanceReport(cl[0], (9, 16))                                     # one frame, nothing joined
    assert [(r["frame"], r["instance"]) for r in bare.as_rows()] == [(0, 0), (0, 1), (0, 2)] and "class" not in bare.as_rows()[0]
    for bad in (dict(clearance=cl[..., :2]), dict(clearance=cl.astype(np.float64)), dict(names=names[:3]), dict(frames=[1]), dict(size=(2, 2)),
                dict(instances=I.InstanceReport.from_rows(rows[:1], total[:1], (9, 16)))):
        with pytest.raises(ValueError, match="ClearanceReport"):
            I.ClearanceReport(**{**dict(clearance=cl, size=(9, 16)), **bad})


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_abi_declares_the_clearance_launches():
    names = ("stswin_instance_clearance", "stswin_instance_clearance_scratch", "stswin_instance_clearance_geometry")
    for s in names:
        assert s in hip.declared_symbols()
    lib = hip.load()
    assert lib.stswin_abi_version() == 1 and all(hasattr(lib, s) for s in names)
    geo = hip.instance_clearance_geometry()
    assert geo[:4] == hip.boundary_geometry() and geo[4] >= 1 and geo[5] >= 1 and lib.stswin_instance_clearance_geometry(6) == -1
    assert hip.instance_clearance_scratch(2, 70, 10, 5, 8) == 8 * 2 * (2 * 10 + 1 + 8 * 5 + 8) + 2 * 70 * 10 * (2 * 5 + 1)
    assert lib.stswin_instance_clearance_scratch(1, 16385, 4, 3, 8) == -1920 and lib.stswin_instance_clearance_scratch(0, 4, 4, 3, 8) == -1920
    assert lib.stswin_instance_clearance_scratch(1, 4, 4, 65, 8) == -1922 and lib.stswin_instance_clearance_scratch(1, 4, 4, 3, 1025) == -1923
    for bad in ((1, 16385, 4, 3, 8), (1, 4, 4, 0, 8), (1, 4, 4, 3, 0), (1, 4, 4, 3, 2.0)):
        with pytest.raises(StswinHipError, match="instance_clearance"):
            hip.instance_clearance_scratch(*bad)
    # refusals that need no GPU: the checks run before anything is launched
    assert lib.stswin_instance_clearance(None, None, None, 0, 8, 8, 3, 4, 7, -1, None, 0, None) == -1920
    assert lib.stswin_instance_clearance(None, None, None, 1, 8, 16385, 3, 4, 7, -1, None, 0, None) == -1920
    assert lib.stswin_instance_clearance(None, None, None, 1, 8, 8, 3, 4, 7, -1, None, 0, None) == -1921
    with pytest.raises(StswinHipError, match="GPU"):
        hip.instance_clearance(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.int32), 4, 3)


# ---------------------------------------------------------------------------------------------- the chain's refusals (no GPU needed)
def test_the_report_chain_refuses_what_clearance_cannot_be():
    def chain(**kw):
        base = dict(report="frame", min_area=1, instances=4, connectivity=8, instance_skip=None, tracks=False, track_iou=100,
                    track_same_class=True)
        return video_report.ReportChain("cpu", 12, "endovis18", kw.pop("out", "labels"), **{**base, **kw})
    for kw, what in ((dict(clearance="always"), "clearance"), (dict(clearance=True), "clearance"),
                     (dict(clearance_to=(1,)), "clearance_to"), (dict(clearance_max=5), "clearance_max"),
                     (dict(clearance="frame", out="logits"), "clearance"),
                     (dict(clearance="frame", instances=None, report=None), "instances"),
                     (dict(clearance="frame", clearance_to=(12,)), "clearance_to"), (dict(clearance="frame", clearance_to=(1.0,)), "clearance_to"),
                     (dict(clearance="deferred", clearance_max=-1), "clearance_max"), (dict(clearance="deferred", clearance_max=2.5), "clearance_max")):
        with pytest.raises(StswinHipError, match=what):
            chain(**kw)
    c = chain(clearance="deferred", clearance_to=[3, 1], clearance_max=40, instance_groups=((1, 2, 3),))
    assert c.clearance == "deferred" and c.clearance_to == (3, 1) and c.clearance_max == 40
    assert c.log.columns["clearance"] == ((4, 12, 3), torch.int64)
    assert "clearance" not in chain(clearance="frame").log.columns and chain().clearance is None
    y = video_report.Yield(clearance=torch.arange(6).view(1, 1, 2, 3))
    assert y.clip(0).clearance.shape == (1, 1, 2, 3) and y.parts is None
    r = y.appended(("labels",), report=False, clearance=True)
    assert len(r) == 2 and r[1].shape == (1, 2, 3)
