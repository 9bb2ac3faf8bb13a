"""utils.instruments.clean_labels, the definition hip.labels_clean is tested against: an independent check against scipy.ndimage on
binary maps, constructed cases, argument errors, and the ABI of the four entry points.  No GPU needed."""
import numpy as np
import pytest
from scipy import ndimage

from stswincl_amd import hip
from stswincl_amd.utils import instruments as I


def _blocky(shape, hi, cell, seed):
    n, H, W = shape
    g = np.random.default_rng(seed)
    cells = g.integers(0, hi, (n, -(-H // cell[0]), -(-W // cell[1])))
    return np.ascontiguousarray(np.repeat(np.repeat(cells, cell[0], axis=1), cell[1], axis=2)[:, :H, :W].astype(np.uint8))


def _scipy_binary(lab, min_area, connectivity):
    """Binary maps: flip every component of area < min_area that has a 4-neighbour in a component of area >= min_area."""
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    out = lab.copy()
    small_count, changed = [], []
    for f in range(lab.shape[0]):
        big = np.zeros(lab.shape[1:], dtype=bool)
        smalls = []
        for c in (0, 1):
            comp, k = ndimage.label(lab[f] == c, structure)
            area = np.bincount(comp.ravel(), minlength=k + 1)
            for i in range(1, k + 1):
                if area[i] >= min_area:
                    big |= comp == i
                else:
                    smalls.append(comp == i)
        near = ndimage.binary_dilation(big, ndimage.generate_binary_structure(2, 1))       # big itself and its 4-neighbours
        flipped = 0
        for m in smalls:
            if (m & near).any():
                out[f][m] = 1 - lab[f][m]
                flipped += int(m.sum())
        small_count.append(len(smalls))
        changed.append(flipped)
    return out, np.stack([small_count, changed], axis=1).astype(np.int32)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("cell,min_area", [((1, 1), 4), ((2, 3), 20), ((3, 2), 7)])
def test_binary_maps_equal_scipy(connectivity, cell, min_area):
    lab = _blocky((3, 29, 41), 2, cell, seed=min_area + connectivity)
    got, stats = I.clean_labels(lab, 2, min_area, connectivity)
    want, want_stats = _scipy_binary(lab, min_area, connectivity)
    assert got.dtype == np.uint8 and stats.dtype == np.int32 and stats.shape == (3, 2)
    assert np.array_equal(got, want)
    assert np.array_equal(stats, want_stats)
    assert stats[:, 1].sum() > 0


def test_a_ring_with_a_hole_is_filled():
    lab = np.zeros((1, 9, 9), dtype=np.uint8)
    lab[0, 2:7, 2:7] = 3
    lab[0, 4, 4] = 0                                                          # the hole: one pixel of the background class
    out, stats = I.clean_labels(lab, 5, 4)
    want = lab.copy()
    want[0, 4, 4] = 3
    assert np.array_equal(out, want) and stats.tolist() == [[1, 1]]


def test_equal_border_takes_the_smaller_class():
    lab = np.zeros((1, 6, 8), dtype=np.uint8)
    lab[0, :, :4] = 4
    lab[0, :, 4:] = 2
    lab[0, 2:4, 3:5] = 1                                                      # 2 x 2 speck astride the border: 4 edges to each class
    out, stats = I.clean_labels(lab, 5, 5)
    assert (out[0, 2:4, 3:5] == 2).all() and stats.tolist() == [[1, 4]]
    lab[0, 2:4, 2] = 1                                                        # two more pixels on the side of class 4: 6 edges against 4
    out, _ = I.clean_labels(lab, 5, 8)
    assert (out[0, 2:4, 2:5] == 4).all()


def test_a_kept_class_survives_and_votes():
    lab = np.zeros((1, 7, 9), dtype=np.uint8)
    lab[0, 3, 1:8] = 2                                                        # a thread: thin, 7 pixels
    lab[0, 2, 4] = 1                                                          # a speck on it: 3 edges to class 0, 1 to the thread
    out, stats = I.clean_labels(lab, 3, 10, keep=(2,))
    assert (out[0, 3, 1:8] == 2).all() and out[0, 2, 4] == 0 and stats.tolist() == [[1, 1]]
    out, stats = I.clean_labels(lab, 3, 10)                                   # not kept: the thread is a speck too and goes
    assert (out == 0).all() and stats.tolist() == [[2, 8]]
    lab[0] = 2                                                                # only the kept class around: it votes
    lab[0, 2, 4] = 1
    lab[0, :, 0] = 0
    out, _ = I.clean_labels(lab, 3, 3, keep=(2,))
    assert out[0, 2, 4] == 2


def test_labels_past_nc_neither_change_nor_vote():
    lab = np.full((1, 5, 5), 9, dtype=np.uint8)
    lab[0, 2, 2] = 1
    out, stats = I.clean_labels(lab, 4, 3)
    assert np.array_equal(out, lab) and stats.tolist() == [[1, 0]]
    lab[0, 0, :] = 0                                                          # five stable pixels of class 0, none beside the speck
    lab[0, 1, 2] = 9
    out, stats = I.clean_labels(lab, 4, 3)
    assert np.array_equal(out, lab) and stats.tolist() == [[1, 0]]


def test_no_stable_voter_no_swap():
    lab = np.array([[[1, 2]]], dtype=np.uint8)
    out, stats = I.clean_labels(lab, 3, 2)
    assert np.array_equal(out, lab) and stats.tolist() == [[2, 0]]
    one = np.full((1, 3, 3), 1, dtype=np.uint8)
    out, stats = I.clean_labels(one, 3, 100)
    assert np.array_equal(out, one) and stats.tolist() == [[1, 0]]


def test_truncation_keeps_the_first_in_raster_order():
    lab = np.zeros((2, 12, 40), dtype=np.uint8)
    lab[:, 1::3, 1::4] = 1                                                    # isolated specks on a stable background, raster order
    full, stats = I.clean_labels(lab, 2, 2, 4)
    per_frame = int((lab[0] == 1).sum())
    assert stats.tolist() == [[per_frame, per_frame]] * 2 and (full == 0).all()
    cap = 7
    out, stats = I.clean_labels(lab, 2, 2, 4, max_small=cap)
    assert (stats[:, 0] > cap).all() and stats.tolist() == [[per_frame, cap]] * 2
    ys, xs = np.nonzero(lab[0] == 1)                                          # (np.nonzero lists in raster order)
    want = lab.copy()
    want[:, ys[:cap], xs[:cap]] = 0
    assert np.array_equal(out, want)


def test_argument_errors():
    lab = np.zeros((1, 4, 4), dtype=np.uint8)
    bad = [dict(labels=lab.astype(np.float32)), dict(labels=lab[0]), dict(labels=lab[None]), dict(nc=0), dict(nc=65), dict(nc=True),
           dict(min_area=1), dict(min_area=(1 << 30) + 1), dict(min_area=2.0), dict(min_area=True), dict(connectivity=6),
           dict(keep=(64,)), dict(keep=(-1,)), dict(keep=(1.5,)), dict(max_small=0), dict(max_small=65537), dict(max_small=4.0)]
    for kw in bad:
        args = dict(labels=lab, nc=3, min_area=2)
        args.update(kw)
        with pytest.raises(ValueError, match="clean_labels"):
            I.clean_labels(**args)
    I.clean_labels(lab, 64, 1 << 30, 4, (0, 63), 65536)
    I.clean_labels(lab.astype(np.int64), 1, 2, 8, (), 1)


def test_abi():
    names = ("stswin_labels_clean", "stswin_labels_clean_scratch", "stswin_labels_clean_geometry", "stswin_labels_score")
    for s in names:
        assert s in hip.declared_symbols()
    lib = hip.load()
    assert lib.stswin_abi_version() == 1 and all(hasattr(lib, s) for s in names)
    g = hip.labels_clean_geometry()
    assert g == (32, 128, 2048, 256) and lib.stswin_labels_clean_geometry(4) == -1
    assert hip.labels_clean_scratch(2, 10, 10, 5, 8) == 4 * (2 * 2 * 100 + 2 * 1 + 2 + 2 * 2 * 8 + 2 * 8 * 5)
    assert lib.stswin_labels_clean_scratch(1, 16385, 4, 3, 8) == -1900 and lib.stswin_labels_clean_scratch(0, 4, 4, 3, 8) == -1900
    # argument errors are reported before anything is launched: no GPU is touched here
    assert lib.stswin_labels_clean(None, None, None, 1, 4, 4, 3, 8, 0, 2, 8, None, 0, None) == -1901
    assert lib.stswin_labels_clean(None, None, None, 0, 4, 4, 3, 8, 0, 2, 8, None, 0, None) == -1900
    assert lib.stswin_labels_score(None, None, None, None, 0, 1, 4, 4, 3, None) == -1911
    assert lib.stswin_labels_score(None, None, None, None, 0, 1, 0, 4, 3, None) == -1910
