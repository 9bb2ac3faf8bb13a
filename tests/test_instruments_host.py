"""utils.instruments on the host: the numpy definition of the moments row against a brute-force double loop, and InstrumentReport on
closed forms.  No GPU."""
import math

import numpy as np
import pytest

from stswincl_amd.utils import instruments as I

TOL = 1e-9          # absolute: the report divides exact integers once in float64 and takes one square root


def _brute(labels, nc):
    n, H, W = labels.shape
    out = [[[0] * 10 for _ in range(nc)] for _ in range(n)]
    for f in range(n):
        for y in range(H):
            for x in range(W):
                c = int(labels[f, y, x])
                if c >= nc:
                    continue
                r = out[f][c]
                r[0] += 1
                r[1] += x
                r[2] += y
                r[3] += x * x
                r[4] += x * y
                r[5] += y * y
                r[6], r[7], r[8], r[9] = max(r[6], W - x), max(r[7], H - y), max(r[8], x + 1), max(r[9], y + 1)
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (3, 9, 20)])
def test_label_moments_is_the_double_loop(shape):
    g = np.random.default_rng(sum(shape))
    labels = g.integers(0, 6, shape).astype(np.uint8)          # 4 and 5 are >= nc: counted nowhere
    got = I.label_moments(labels, 4)
    assert got.dtype == np.int64 and got.shape == (shape[0], 4, 10)
    assert np.array_equal(got, _brute(labels, 4))
    assert got[:, :, 0].sum() == (labels < 4).sum()
    assert np.array_equal(I.label_moments(labels[0], 4), got[:1])          # one [H][W] map


def test_label_moments_refusals():
    for labels, nc in ((np.zeros((2, 3, 4), np.float32), 4), (np.zeros((3,), np.uint8), 4), (np.zeros((1, 2, 3), np.uint8), 0),
                       (np.zeros((1, 2, 3), np.uint8), 65), (np.zeros((1, 0, 3), np.uint8), 4)):
        with pytest.raises(ValueError):
            I.label_moments(labels, nc)


def _report(labels, nc, **kw):
    return I.InstrumentReport.from_moments(I.label_moments(labels, nc), labels.shape[-2:], **kw)


def test_filled_rectangle_and_its_transpose():
    x0, x1, y0, y1 = 100, 161, 40, 60                           # w = 61 > h = 20
    w, h = x1 - x0, y1 - y0
    lab = np.zeros((1, 128, 200), np.uint8)
    lab[0, y0:y1, x0:x1] = 2
    rep = _report(lab, 4)
    assert rep.present[0].tolist() == [True, False, True, False] and rep.area[0, 2] == w * h
    assert rep.box[0, 2].tolist() == [x0, y0, x1, y1]
    assert np.abs(rep.centroid[0, 2] - [(x0 + x1 - 1) / 2, (y0 + y1 - 1) / 2]).max() <= TOL
    assert np.abs(rep.axes[0, 2] - [math.sqrt((w * w - 1) / 12), math.sqrt((h * h - 1) / 12)]).max() <= TOL
    assert abs(rep.angle[0, 2]) <= TOL
    rep_t = _report(np.ascontiguousarray(lab.transpose(0, 2, 1)), 4)
    assert rep_t.box[0, 2].tolist() == [y0, x0, y1, x1]
    assert abs(rep_t.angle[0, 2] - math.pi / 2) <= TOL          # (-pi/2, pi/2]: the vertical axis is +pi/2
    assert np.abs(rep_t.axes[0, 2] - rep.axes[0, 2]).max() <= TOL
    assert np.abs(rep_t.centroid[0, 2] - rep.centroid[0, 2][::-1]).max() <= TOL


def test_diagonal_line_and_antidiagonal():
    lab = np.zeros((1, 64, 64), np.uint8)
    k = np.arange(50)
    lab[0, k + 5, k + 5] = 1
    rep = _report(lab, 2)
    assert abs(rep.angle[0, 1] - math.pi / 4) <= TOL
    assert rep.axes[0, 1, 1] == 0.0                              # one pixel wide: the determinant is exactly 0
    assert abs(rep.axes[0, 1, 0] - math.sqrt(2 * (50 * 50 - 1) / 12)) <= TOL
    assert rep.box[0, 1].tolist() == [5, 5, 55, 55]
    anti = _report(np.ascontiguousarray(lab[:, :, ::-1]), 2)
    assert abs(anti.angle[0, 1] + math.pi / 4) <= TOL


def test_single_far_pixel_does_not_cancel():
    lab = np.zeros((1, 1024, 1280), np.uint8)
    lab[0, 1023, 1279] = 7
    rep = _report(lab, 12)
    assert rep.centroid[0, 7].tolist() == [1279.0, 1023.0] and rep.axes[0, 7].tolist() == [0.0, 0.0]
    assert rep.angle[0, 7] == 0.0 and rep.box[0, 7].tolist() == [1279, 1023, 1280, 1024] and rep.area[0, 7] == 1
    # a 3-pixel horizontal sliver at the far corner: variance 2/3 whatever the offset
    lab[0, 1023, 1277:1279] = 7
    rep = _report(lab, 12)
    assert np.abs(rep.axes[0, 7] - [math.sqrt(2 / 3), 0.0]).max() <= TOL and rep.centroid[0, 7].tolist() == [1278.0, 1023.0]


def test_min_area_absent_classes_presence_and_rows():
    lab = np.zeros((3, 10, 12), np.uint8)
    lab[0, 2:4, 3:6] = 1                                          # 6 pixels
    lab[1, 0, 0] = 2                                              # 1 pixel
    lab[2, 5:9, 1:11] = 1                                         # 40 pixels
    mom = I.label_moments(lab, 3)
    rep = I.InstrumentReport.from_moments(mom, (10, 12), min_area=5, names=["bg", "shaft", "clasper"], frames=[7, 3, 8],
                                          sequences=[1, 0, 1])
    assert len(rep) == 3
    assert rep.presence().tolist() == [[True, True, False], [True, False, False], [True, True, False]]
    assert rep.presence().dtype == np.bool_
    assert rep.area.tolist() == [[114, 6, 0], [119, 0, 0], [80, 40, 0]]           # class 2 of frame 1: 1 < min_area, so absent
    assert np.isnan(rep.box[1, 2]).all() and np.isnan(rep.centroid[1, 2]).all() and np.isnan(rep.angle[1, 2])
    assert np.isnan(rep.axes[0, 2]).all() and not np.isnan(rep.box[rep.present]).any()
    assert I.InstrumentReport.from_moments(mom, (10, 12)).presence()[1].tolist() == [True, False, True]
    rows = rep.as_rows()
    assert [(r["sequence"], r["frame"], r["class"], r["name"]) for r in rows] == [
        (1, 7, 0, "bg"), (1, 7, 1, "shaft"), (0, 3, 0, "bg"), (1, 8, 0, "bg"), (1, 8, 1, "shaft")]        # the given row order
    assert rows[1]["area"] == 6 and rows[1]["box"] == (3, 2, 6, 4) and rows[1]["centroid"] == (4.0, 2.5) and rows[1]["present"]
    assert all(isinstance(v, float) for v in rows[1]["axes"]) and isinstance(rows[1]["angle"], float)
    every = rep.as_rows(absent=True)
    assert len(every) == 9 and every[5] == dict(sequence=0, frame=3, **{"class": 2}, name="clasper", present=False, area=0, box=None,
                                                centroid=None, angle=None, axes=None)
    assert "name" not in I.InstrumentReport.from_moments(mom, (10, 12)).as_rows()[0]
    one = I.InstrumentReport.from_moments(mom[2], (10, 12))                         # one frame's [nc][10]
    assert len(one) == 1 and one.frames == [0] and one.sequences == [0] and one.area.tolist() == [[80, 40, 0]]
    for kw in (dict(min_area=0), dict(min_area=1.5), dict(names=["a"]), dict(frames=[1]), dict(sequences=[0, 1])):
        with pytest.raises(ValueError):
            I.InstrumentReport.from_moments(mom, (10, 12), **kw)
    with pytest.raises(ValueError):
        I.InstrumentReport.from_moments(mom[:, :, :9], (10, 12))


def test_pooled_rows_are_a_sum_and_a_maximum():
    g = np.random.default_rng(3)
    a, b = (g.integers(0, 3, (1, 6, 9)).astype(np.uint8) for _ in range(2))
    ma, mb = I.label_moments(a, 3), I.label_moments(b, 3)
    both = I.label_moments(np.concatenate([a, b], axis=2), 3)       # b to the right of a: other x, so only count and the y terms pool
    assert np.array_equal(both[:, :, [0, 2, 5]], (ma + mb)[:, :, [0, 2, 5]])
    assert np.array_equal(both[:, :, [7, 9]], np.maximum(ma, mb)[:, :, [7, 9]])
