"""The numpy side of VideoSegmenter(instance_groups=..., parts=...): utils.instruments.group_table, instance_parts and PartsReport
(CPU, no GPU needed), and the two entry points in the header.  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

from stswincl_amd import hip
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import instruments as I


def _loop(lab, comp, K, nc):
    """instance_parts pixel by pixel, in Python integers."""
    n, H, W = lab.shape
    parts = np.zeros((n, K, nc, 10), np.int64)
    contacts = np.zeros((n, K, nc), np.int64)
    for f in range(n):
        for y in range(H):
            for x in range(W):
                i, c = int(comp[f, y, x]), int(lab[f, y, x])
                if not 0 <= i < K:
                    continue
                if c < nc:
                    row = parts[f, i, c]
                    for k, v in enumerate((1, x, y, x * x, x * y, y * y)):
                        row[k] += v
                    for k, v in enumerate((W - x, H - y, x + 1, y + 1)):
                        row[6 + k] = max(row[6 + k], v)
                for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and int(comp[f, v, u]) != i and int(lab[f, v, u]) < nc:
                        contacts[f, i, int(lab[f, v, u])] += 1
    return parts, contacts


def _blocky(rng, shape, hi, cell=(3, 4)):
    n, H, W = shape
    cells = rng.integers(0, hi, (n, -(-H // cell[0]), -(-W // cell[1])))
    return np.repeat(np.repeat(cells, cell[0], axis=1), cell[1], axis=2)[:, :H, :W]


# ------------------------------------------------------------------------------------------------------------ instance_parts
@pytest.mark.parametrize("nc", [1, 3, 12])
def test_instance_parts_against_a_plain_loop(nc):
    rng = np.random.default_rng(nc)
    for shape in ((2, 12, 17), (1, 1, 1), (2, 1, 9), (1, 7, 1)):
        lab = _blocky(rng, shape, nc + 2).astype(np.uint8)                    # labels >= nc among them
        lab[0, 0, 0] = 255
        comp, _, total = I.label_components(lab, nc, 8, (0,) if nc > 1 else (), 1024)
        for K in (1, max(int(total.max()) - 1, 1), int(total.max()) + 3):      # below and above the number of components
            for c in (comp, rng.integers(-1, K + 3, shape).astype(np.int32)):  # and raw ordinals: -1 and >= K, unrelated to the labels
                got, want = I.instance_parts(lab, c, K, nc), _loop(lab, c, K, nc)
                assert got[0].dtype == got[1].dtype == np.int64 and got[0].shape == (shape[0], K, nc, 10) and got[1].shape == (shape[0], K, nc)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (shape, K)
    one = I.instance_parts(lab[0], comp[0], 4, nc)                            # one frame [H][W]
    assert np.array_equal(one[0], I.instance_parts(lab[:1], comp[:1], 4, nc)[0])


def test_parts_sum_to_the_rows_of_label_components():
    rng = np.random.default_rng(7)
    nc, K = 6, 32
    lab = _blocky(rng, (3, 12, 17), nc).astype(np.uint8)
    table = I.group_table(((1, 2, 3),), nc)
    for conn in (4, 8):
        comp, rows, total = I.label_components(table[lab], nc, conn, (0,), K)
        parts, contacts = I.instance_parts(lab, comp, K, nc)
        assert int(total.max()) >= 2 and (parts[:, :, 1:4, 0] > 0).sum(axis=2).max() >= 2, "no instance has two parts"
        assert np.array_equal(parts[..., :6].sum(axis=2), rows[:, :, 2:8])
        assert np.array_equal(parts[..., 6:].max(axis=2), rows[:, :, 8:])
        assert contacts.max() <= 4 * 12 * 17 and contacts.min() >= 0
        # an instance is maximal at 4-connectivity or finer: nothing of its own (grouped) class lies across a pixel edge
        for f, i in zip(*np.nonzero(rows[:, :, 2])):
            own = [c for c in range(nc) if table[c] == rows[f, i, 0]]
            assert int(contacts[f, i, own].sum()) == 0


def test_definition_refusals():
    lab, comp = np.zeros((1, 4, 5), np.uint8), np.zeros((1, 4, 5), np.int32)
    for a, b, K, nc in ((lab, comp[:, :3], 4, 3), (lab.astype(np.float32), comp, 4, 3), (lab, comp, 0, 3), (lab, comp, 1025, 3),
                        (lab, comp, 4, 0), (lab, comp, 4, 65), (lab, comp.astype(np.float64), 4, 3)):
        with pytest.raises(ValueError, match="instance_parts"):
            I.instance_parts(a, b, K, nc)


# ------------------------------------------------------------------------------------------------------------------ grouping
def test_group_table():
    t = I.group_table(((3, 1, 2), (7, 5)), 12)
    assert t.dtype == np.uint8 and t.shape == (256,)
    want = np.arange(256)
    want[[1, 2, 3]] = 1
    want[[5, 7]] = 5
    assert np.array_equal(t, want) and (t[12:] >= 12).all()
    assert np.array_equal(I.group_table((), 12), np.arange(256)) and np.array_equal(I.group_table([[0, 11]], 12)[[0, 11]], [0, 0])


def test_malformed_groups_are_refused():
    for groups in (((1,),), ((1, 1),), ((1, 2), (2, 3)), ((1, 12),), ((-1, 2),), ((1, 2.0),), ((True, 2),), 5, (1, 2)):
        with pytest.raises(ValueError, match="instance_groups"):
            I.group_table(groups, 12)
    with pytest.raises(ValueError, match="skipped"):
        I.check_groups(((0, 1),), 12, skip=(0,))
    assert I.check_groups([[1, 2, 3], (5, 4)], 12, skip=(0,)) == ((1, 2, 3), (5, 4))


def test_grouped_components_are_whole_instruments():
    """Two shaft (1) - wrist (2) - clasper (3) chains on background 0, a needle (4) in the first one's clasper."""
    lab = np.zeros((1, 9, 16), np.uint8)
    lab[0, 1, 1:4], lab[0, 1, 4:6], lab[0, 1, 6:8] = 1, 2, 3
    lab[0, 2, 7] = 4
    lab[0, 6, 2:6], lab[0, 6, 6], lab[0, 5:8, 7] = 1, 2, 3
    nc, K = 5, 8
    assert int(I.label_components(lab, nc, 8, (0,), K)[2][0]) == 7            # ungrouped: seven unrelated components
    table = I.group_table(((1, 2, 3),), nc)
    comp, rows, total = I.label_components(table[lab], nc, 8, (0,), K)
    assert int(total[0]) == 3 and rows[0, :3, 0].tolist() == [1, 4, 1] and rows[0, :3, 2].tolist() == [7, 1, 8]
    assert len(set(comp[0, 1, 1:8].tolist())) == 1 and comp[0, 1, 1] == 0 and comp[0, 6, 2] == 2 and comp[0, 2, 7] == 1
    parts, contacts = I.instance_parts(lab, comp, K, nc)
    assert parts[0, 0, :, 0].tolist() == [0, 3, 2, 2, 0] and parts[0, 2, :, 0].tolist() == [0, 4, 1, 3, 0]
    assert contacts[0, 0].tolist() == [2 * 7 + 2 - 1, 0, 0, 0, 1]            # the chain's outline less the needle's edge; the needle
    assert contacts[0, 1].tolist() == [3, 0, 0, 1, 0]                         # touches the clasper (3) and background
    assert contacts[0, 2, 0] == 4 * 8 - 2 * 7 and contacts[0, 2, 1:].sum() == 0   # eight pixels, seven edges between them


# --------------------------------------------------------------------------------------------------------------- PartsReport
def _hand_made():
    lab = np.zeros((2, 9, 16), np.uint8)
    for f, dx in enumerate((0, 3)):                                          # the instrument moves three pixels to the right
        lab[f, 1, 1 + dx:4 + dx], lab[f, 1, 4 + dx:6 + dx], lab[f, 1, 6 + dx:8 + dx] = 1, 2, 3
        lab[f, 2, 7 + dx] = 4
    nc, K = 5, 4
    comp, rows, total = I.label_components(I.group_table(((1, 2, 3),), nc)[lab], nc, 8, (0,), K)
    return lab, comp, rows, total, nc, K


def test_parts_report_on_a_hand_made_frame():
    lab, comp, rows, total, nc, K = _hand_made()
    parts, contacts = I.instance_parts(lab, comp, K, nc)
    names = ["background", "instrument", "wrist", "clasper", "needle"]
    inst = I.InstanceReport.from_rows(rows, total, (9, 16), names=names)
    tracker = I.InstanceTracker(K)
    ids, started = zip(*(tracker.update(comp[f], rows[f], total[f]) for f in range(2)))
    trk = I.TrackReport.from_ids(inst, np.stack(ids), np.asarray(started))
    rep = I.PartsReport(parts, contacts, (9, 16), names, frames=[4, 5], sequences=[0, 0], tracks=trk)
    assert len(rep) == 2 and rep.instances is inst and rep.has.shape == (2, K, nc)
    assert rep.area[0, 0].tolist() == [0, 3, 2, 2, 0] and rep.has[0, 1].tolist() == [False] * 4 + [True]
    assert rep.parts(0, 0)[1] == dict(area=3, box=(1, 1, 4, 2), centroid=(2.0, 1.0), angle=0.0, axes=(np.sqrt(2 / 3), 0.0))
    assert sorted(rep.parts(0, 0)) == [1, 2, 3] and rep.parts(0, 2) == {}
    assert np.isnan(rep.centroid[0, 0, 4]).all() and np.isnan(rep.box[0, 1, 1]).all()
    assert rep.touches(0, 0) == {0: 15, 4: 1} and rep.touches(0, 1) == {0: 3, 3: 1} and rep.touches(0, 3) == {}
    assert np.array_equal(rep.direction(0, 0, 1, 3), [1.0, 0.0]) and np.array_equal(rep.direction(0, 0, 3, 1), [-1.0, 0.0])
    assert np.isnan(rep.direction(0, 0, 1, 4)).all() and np.isnan(rep.direction(0, 0, 1, 1)).all()
    d = rep.centroid[0, 1, 4] - rep.centroid[0, 0, 1]                         # across instances the centroids are the caller's to join
    assert d.tolist() == [5.0, 1.0]
    got = rep.as_rows()
    assert [(r["frame"], r["instance"], r["class"], r["name"], r["track"]) for r in got] == [
        (4, 0, 1, "instrument", 0), (4, 1, 4, "needle", 1), (5, 0, 1, "instrument", 0), (5, 1, 4, "needle", 2)]   # (no overlap: a new track)
    assert got[2]["parts"][3]["centroid"] == (9.5, 1.0) and got[3]["touches"] == {0: 3, 3: 1}
    bare = I.PartsReport(parts[0], contacts[0], (9, 16))                     # one frame, nothing joined
    assert [(r["frame"], r["instance"]) for r in bare.as_rows()] == [(0, 0), (0, 1)] and "class" not in bare.as_rows()[0]
    for bad in (dict(parts=parts[..., :9]), dict(contacts=contacts[:, :2]), dict(names=names[:3]), dict(frames=[1]),
                dict(instances=I.InstanceReport.from_rows(rows[:1], total[:1], (9, 16)))):
        with pytest.raises(ValueError, match="PartsReport"):
            I.PartsReport(**{**dict(parts=parts, contacts=contacts, size=(9, 16)), **bad})


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_abi_declares_the_parts_launch():
    for s in ("stswin_instance_parts", "stswin_instance_parts_geometry"):
        assert s in hip.declared_symbols()
    lib = hip.load()
    assert lib.stswin_abi_version() == 1 and hasattr(lib, "stswin_instance_parts") and hasattr(lib, "stswin_instance_parts_geometry")
    th, tw, slots = hip.instance_parts_geometry()
    assert th >= 1 and tw >= 16 and 1 <= slots < th * tw and lib.stswin_instance_parts_geometry(3) == -1
    # refusals that need no GPU: the checks run before anything is launched
    assert lib.stswin_instance_parts(None, None, None, None, 1, 8, 8, 3, 4, None) == -1891
    assert lib.stswin_instance_parts(None, None, None, None, 0, 8, 8, 3, 4, None) == -1890
    assert lib.stswin_instance_parts(None, None, None, None, 1, 8, 16385, 3, 4, None) == -1890
    with pytest.raises(StswinHipError, match="GPU"):
        hip.instance_parts(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.int32), 4, 3)
