"""utils.instruments.label_components on the host: the numpy definition against an independent flood fill (and scipy.ndimage.label
where scipy is installed), pooling back to the moments row, deterministic truncation, InstanceReport on hand-computed cases, and the
refusals.  No GPU."""
import numpy as np
import pytest

from stswincl_amd.utils import instruments as I


def _flood(labels, nc, connectivity, skip=()):
    """Brute force: visit pixels in raster order, flood-fill every unvisited valid pixel with an explicit stack -> (components, rows
    unbounded as a list per frame, total)."""
    n, H, W = labels.shape
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    comp = np.full((n, H, W), -1, dtype=np.int32)
    rows, total = [], []
    for f in range(n):
        frame_rows = []
        for y0 in range(H):
            for x0 in range(W):
                c = int(labels[f, y0, x0])
                if c >= nc or c in skip or comp[f, y0, x0] >= 0:
                    continue
                i = len(frame_rows)
                r = [c, y0 * W + x0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
                comp[f, y0, x0] = i
                stack = [(y0, x0)]
                while stack:
                    y, x = stack.pop()
                    r[2] += 1
                    r[3] += x
                    r[4] += y
                    r[5] += x * x
                    r[6] += x * y
                    r[7] += y * y
                    r[8], r[9], r[10], r[11] = max(r[8], W - x), max(r[9], H - y), max(r[10], x + 1), max(r[11], y + 1)
                    for dy, dx in steps:
                        v, u = y + dy, x + dx
                        if 0 <= v < H and 0 <= u < W and comp[f, v, u] < 0 and int(labels[f, v, u]) == c:
                            comp[f, v, u] = i
                            stack.append((v, u))
                frame_rows.append(r)
        rows.append(frame_rows)
        total.append(len(frame_rows))
    return comp, rows, np.array(total, dtype=np.int32)


def _padded(rows, K):
    out = np.zeros((len(rows), K, 12), dtype=np.int64)
    for f, fr in enumerate(rows):
        for i, r in enumerate(fr[:K]):
            out[f, i] = r
    return out


def _scipy_components(labels, nc, connectivity, skip=()):
    """scipy.ndimage.label per class, the components of all classes renumbered by first pixel."""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else None
    n, H, W = labels.shape
    comp = np.full((n, H, W), -1, dtype=np.int32)
    total = np.zeros(n, dtype=np.int32)
    for f in range(n):
        firsts = []
        for c in range(nc):
            if c in skip:
                continue
            lab, k = ndimage.label(labels[f] == c, structure=structure)
            for j in range(1, k + 1):
                m = lab == j
                firsts.append((int(np.flatnonzero(m)[0]), m))
        for i, (_, m) in enumerate(sorted(firsts, key=lambda t: t[0])):
            comp[f][m] = i
        total[f] = len(firsts)
    return comp, total


def _noise(shape, p, seed):
    """Classes 1 .. 3 sprinkled with density p over a background of class 0."""
    g = np.random.default_rng(seed)
    return (g.integers(1, 4, shape) * (g.random(shape) < p)).astype(np.uint8)


NOISE_SEED = 37         # the (1, 37, 150) map at p = 0.05 on which scipy counts 241 components at 8-connectivity and 248 at 4


def _u_shape():
    lab = np.zeros((1, 9, 11), dtype=np.uint8)
    lab[0, 1:8, 2] = lab[0, 1:8, 8] = lab[0, 7, 2:9] = 1        # two arms that join only at the bottom
    return lab


def _diagonal_blobs():
    lab = np.zeros((1, 8, 8), dtype=np.uint8)
    lab[0, 1:4, 1:4] = lab[0, 4:7, 4:8] = 2                     # (3, 3) and (4, 4) touch only diagonally
    return lab


CASES = {
    "random-2x9x13": lambda: np.random.default_rng(1).integers(0, 3, (2, 9, 13)).astype(np.uint8),
    "random-1x37x150": lambda: np.random.default_rng(2).integers(0, 3, (1, 37, 150)).astype(np.uint8),
    "u-shape": _u_shape,
    "diagonal-blobs": _diagonal_blobs,
}


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", sorted(CASES))
def test_definition_is_the_flood_fill(case, connectivity):
    labels = CASES[case]()
    nc = 3
    comp, rows, total = I.label_components(labels, nc, connectivity, max_instances=1024)
    assert comp.dtype == np.int32 and rows.dtype == np.int64 and total.dtype == np.int32
    assert comp.shape == labels.shape and rows.shape == (labels.shape[0], 1024, 12) and total.shape == (labels.shape[0],)
    bcomp, brows, btotal = _flood(labels, nc, connectivity)
    assert np.array_equal(total, btotal) and np.array_equal(comp, bcomp)
    assert np.array_equal(rows, _padded(brows, 1024))
    if case == "u-shape":
        assert total[0] == 2                                        # the U, and the background around and inside it
    if case == "diagonal-blobs":
        assert total[0] == (2 if connectivity == 8 else 3)          # background + one instance at 8, two at 4


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", sorted(CASES))
def test_definition_is_scipy_per_class(case, connectivity):
    labels = CASES[case]()
    comp, _, total = I.label_components(labels, 3, connectivity, skip=(0,), max_instances=1024)
    scomp, stotal = _scipy_components(labels, 3, connectivity, skip=(0,))
    assert np.array_equal(total, stotal) and np.array_equal(comp, scomp)
    if case == "diagonal-blobs":
        assert total[0] == (1 if connectivity == 8 else 2)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_instances_pool_to_the_class_moments(connectivity):
    labels = CASES["random-2x9x13"]()
    nc = 3
    _, rows, total = I.label_components(labels, nc, connectivity, max_instances=1024)
    assert (total <= 1024).all()
    mom = I.label_moments(labels, nc)
    for f in range(labels.shape[0]):
        for c in range(nc):
            mine = rows[f, :total[f]][rows[f, :total[f], 0] == c]
            assert np.array_equal(mine[:, 2:8].sum(axis=0), mom[f, c, :6])
            assert np.array_equal(mine[:, 8:12].max(axis=0) if len(mine) else np.zeros(4, dtype=np.int64), mom[f, c, 6:])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_truncation_keeps_the_first_rows(connectivity):
    labels = _noise((1, 37, 150), 0.05, NOISE_SEED)
    full = I.label_components(labels, 4, connectivity, skip=(0,), max_instances=1024)
    cut = I.label_components(labels, 4, connectivity, skip=(0,), max_instances=16)
    _, btotal = _flood(labels, 4, connectivity, skip=(0,))[1:]
    assert full[2][0] == btotal[0] == (241 if connectivity == 8 else 248)
    assert np.array_equal(cut[1], full[1][:, :16])
    assert np.array_equal(cut[2], full[2]) and np.array_equal(cut[0], full[0])
    assert cut[0].max() == full[2][0] - 1                           # the map is complete: ordinals past K are in it


@pytest.mark.parametrize("connectivity", [4, 8])
def test_noise_map_counts_are_scipy_s(connectivity):
    labels = _noise((1, 37, 150), 0.05, NOISE_SEED)
    comp, _, total = I.label_components(labels, 4, connectivity, skip=(0,), max_instances=1)
    scomp, stotal = _scipy_components(labels, 4, connectivity, skip=(0,))
    assert total[0] == stotal[0] == (241 if connectivity == 8 else 248) and np.array_equal(comp, scomp)


def test_skipped_and_out_of_range_labels_are_in_no_component():
    labels = np.array([[[0, 1, 1, 5], [2, 2, 0, 1]]], dtype=np.uint8)
    comp, rows, total = I.label_components(labels, 3, 4, skip=(0, 2), max_instances=4)
    assert np.array_equal(comp[0], [[-1, 0, 0, -1], [-1, -1, -1, 1]])
    assert total[0] == 2 and np.array_equal(rows[0, :2, :3], [[1, 1, 2], [1, 7, 1]]) and not rows[0, 2:].any()
    comp, rows, total = I.label_components(labels, 3, 8, skip=(0, 1, 2), max_instances=4)
    assert (comp == -1).all() and total[0] == 0 and not rows.any()
    one = I.label_components(labels[0], 3, 4, skip=(0, 2), max_instances=4)          # one [H][W] map is one frame
    assert one[0].shape == (1, 2, 4) and one[2][0] == 2


def _two_rectangles():
    lab = np.zeros((1, 20, 30), dtype=np.uint8)
    lab[0, 2:6, 3:11] = 1          # 4 x 8 = 32 pixels, box (3, 2, 11, 6), centroid (6.5, 3.5)
    lab[0, 10:13, 20:22] = 1       # 3 x 2 = 6 pixels, box (20, 10, 22, 13), centroid (20.5, 11)
    return lab


def test_instance_report_on_two_rectangles():
    lab = _two_rectangles()
    _, rows, total = I.label_components(lab, 2, 8, skip=(0,), max_instances=4)
    rep = I.InstanceReport.from_rows(rows, total, (20, 30), names=["background", "shaft"])
    assert len(rep) == 1 and rep.present[0].tolist() == [True, True, False, False]
    assert rep.cls[0].tolist() == [1, 1, -1, -1] and rep.first[0].tolist() == [2 * 30 + 3, 10 * 30 + 20, -1, -1]
    assert rep.area[0].tolist() == [32, 6, 0, 0]
    assert rep.box[0, 0].tolist() == [3, 2, 11, 6] and rep.box[0, 1].tolist() == [20, 10, 22, 13]
    assert rep.centroid[0, 0].tolist() == [6.5, 3.5] and rep.centroid[0, 1].tolist() == [20.5, 11.0]
    assert rep.angle[0, 0] == 0.0 and abs(rep.angle[0, 1]) == pytest.approx(np.pi / 2)      # wide, and tall
    assert rep.axes[0, 0].tolist() == pytest.approx([np.sqrt(63 / 12), np.sqrt(15 / 12)], abs=1e-12)
    assert np.isnan(rep.box[0, 2:]).all() and not rep.truncated[0]
    assert rep.counts().tolist() == [[0, 2]]
    listed = rep.as_rows()
    assert [r["instance"] for r in listed] == [0, 1] and listed[0]["name"] == "shaft"
    assert listed[1] == {"sequence": 0, "frame": 0, "instance": 1, "class": 1, "name": "shaft", "area": 6, "box": (20, 10, 22, 13),
                         "centroid": (20.5, 11.0), "angle": listed[1]["angle"], "axes": listed[1]["axes"]}
    # the same arithmetic as InstrumentReport: one instance of a class is that class's row
    single = np.where(lab == 1, 1, 0).astype(np.uint8)
    single[0, 10:13, 20:22] = 0
    ir = I.InstrumentReport.from_moments(I.label_moments(single, 2), (20, 30))
    assert ir.box[0, 1].tolist() == rep.box[0, 0].tolist() and ir.axes[0, 1].tolist() == rep.axes[0, 0].tolist()
    assert ir.angle[0, 1] == rep.angle[0, 0] and ir.centroid[0, 1].tolist() == rep.centroid[0, 0].tolist()


def test_instance_report_min_area_truncated_and_frames():
    lab = np.concatenate([_two_rectangles(), np.zeros((1, 20, 30), dtype=np.uint8)])
    _, rows, total = I.label_components(lab, 2, 8, skip=(0,), max_instances=1)
    rep = I.InstanceReport.from_rows(rows, total, (20, 30), min_area=7, frames=[4, 5], sequences=[2, 2])
    assert rep.truncated.tolist() == [True, False] and rep.total.tolist() == [2, 0]
    assert rep.counts(2).tolist() == [[0, 1], [0, 0]]
    assert [(r["sequence"], r["frame"], r["instance"], r["area"]) for r in rep.as_rows()] == [(2, 4, 0, 32)]
    _, rows, total = I.label_components(lab, 2, 8, skip=(0,), max_instances=4)
    rep = I.InstanceReport.from_rows(rows, total, (20, 30), min_area=7)
    assert rep.present.sum() == 1 and rep.area[0].tolist() == [32, 0, 0, 0] and rep.counts(2).tolist() == [[0, 1], [0, 0]]
    assert I.InstanceReport.from_rows(rows[0], total[0], (20, 30)).present.sum() == 2        # one frame's [K][12] and a scalar total


def test_refusals():
    lab = np.zeros((1, 4, 4), dtype=np.uint8)
    bad = [
        dict(labels=lab.astype(np.float32)), dict(labels=np.zeros((4,), dtype=np.uint8)), dict(labels=np.zeros((1, 1, 4, 4), dtype=np.uint8)),
        dict(nc=0), dict(nc=65), dict(connectivity=6), dict(connectivity=0), dict(skip=(64,)), dict(skip=(-1,)),
        dict(max_instances=0), dict(max_instances=1025),
    ]
    for kw in bad:
        args = dict(labels=lab, nc=2, connectivity=8, skip=(), max_instances=4)
        args.update(kw)
        with pytest.raises(ValueError, match="label_components"):
            I.label_components(**args)
    _, rows, total = I.label_components(lab, 2, max_instances=4)
    for kw in (dict(rows=rows[:, :, :10]), dict(total=np.zeros(3, dtype=np.int32)), dict(min_area=0), dict(frames=[0, 1]),
               dict(rows=rows.astype(np.float64))):
        args = dict(rows=rows, total=total, size=(4, 4))
        args.update(kw)
        with pytest.raises(ValueError, match="InstanceReport"):
            I.InstanceReport.from_rows(**args)
