"""Synthetic sequences for the instance tracker (utils.instruments.InstanceTracker, hip.track_instances), shared by
tests/test_tracks_host.py and tests/test_hip_tracks.py.  Every case is a sequence of label maps, so the GPU tests can run it through
hip.label_components; the shapes lie around the 16 x 64 tile of the component kernels (hip.CC_TILE).  A case is a dict: name, labels
uint8 [frames][H][W], nc, connectivity, skip, K, min_iou, same_class, min_area."""
import functools

import numpy as np

from stswincl_amd import hip
from stswincl_amd.utils import instruments as I

TH, TW = hip.CC_TILE


def _put(lab, f, y, x, h, w, c):
    """Class c into the rectangle [y, y + h) x [x, x + w) of frame f, clipped to the map."""
    H, W = lab.shape[1:]
    y0, x0, y1, x1 = max(y, 0), max(x, 0), min(y + h, H), min(x + w, W)
    if y0 < y1 and x0 < x1:
        lab[f, y0:y1, x0:x1] = c


def _case(name, labels, K=8, nc=3, connectivity=8, skip=(0,), min_iou=100, same_class=True, min_area=1):
    return dict(name=name, labels=labels, K=K, nc=nc, connectivity=connectivity, skip=tuple(skip), min_iou=min_iou, same_class=same_class,
                min_area=min_area)


def _moving(W):
    """Two blobs of class 1 - (TH + 3) x (TW + 5) and 1 x 1 - and a 1 x (TW + 1) line of class 2, each translating for 8 frames.  The
    single pixel moves further than its size: it ends and is born again in every frame."""
    lab = np.zeros((8, 2 * TH + 8, W), dtype=np.uint8)
    for f in range(8):
        _put(lab, f, 1, 1 + 2 * f, TH + 3, TW + 5, 1)
        _put(lab, f, TH + 9, 2 + 3 * f, 1, TW + 1, 2)
        _put(lab, f, TH + 14, 100 + 3 * f, 1, 1, 1)
    return lab


def _enter_leave():
    lab = np.zeros((6, 20, TW + 6), dtype=np.uint8)
    for f in range(6):
        _put(lab, f, 3, TW - 6 + 4 * f, 6, 6, 1)        # leaves on the right: clipped in frame 2, gone from frame 3
        _put(lab, f, 12, -14 + 4 * f, 6, 6, 1)          # enters on the left in frame 3
    return lab


def _split_merge():
    """A bar splits into a small left and a large right piece, which then merge again: the id stays with the right piece throughout,
    although the left one comes first in raster order."""
    lab = np.zeros((3, 20, TW + 6), dtype=np.uint8)
    for f in range(3):
        _put(lab, f, 5, 5, 4, 36, 1)
    _put(lab, 1, 5, 15, 4, 3, 0)
    return lab


def _crossing():
    """Two blobs of one class, one moving down and one moving up: from frame 4 on the other one holds the first pixel."""
    lab = np.zeros((7, 30, TW + 6), dtype=np.uint8)
    for f in range(7):
        _put(lab, f, 2 + 2 * f, 5, 8, 8, 1)
        _put(lab, f, 14 - 2 * f, 30, 8, 8, 1)
    return lab


def _chain():
    """Frame 0: i0 = 4 x 20, i1 = 8 x 8.  Frame 1: j0 = 4 x 28 over i0 and six columns of i1, j1 = 4 pixels inside i1.  (i0, j0) 80 / 112
    is the best pair, i1 prefers j0 (24 / 152) to j1 (4 / 64), j1 has only i1: the first round of mutual bests matches (i0, j0) alone,
    the second (i1, j1).  min_iou = 50 keeps 4 / 64 a candidate."""
    lab = np.zeros((2, 12, TW + 6), dtype=np.uint8)
    _put(lab, 0, 2, 0, 4, 20, 1)
    _put(lab, 0, 2, 22, 8, 8, 1)
    _put(lab, 1, 2, 0, 4, 28, 1)
    _put(lab, 1, 9, 24, 1, 4, 1)
    return lab


def _tie():
    """Row 0: (ov, u) = (1, 2) and (2, 4), two pairs of equal preference that share nothing.  Row 3: a 4-pixel instance over a
    1-pixel one (1 / 4) and over two of a 6-pixel one (2 / 8): equal, so the smaller previous ordinal wins although it overlaps less."""
    lab = np.zeros((2, 6, 24), dtype=np.uint8)
    _put(lab, 0, 0, 0, 1, 1, 1)
    _put(lab, 0, 0, 5, 1, 2, 1)
    _put(lab, 1, 0, 0, 1, 2, 1)
    _put(lab, 1, 0, 5, 1, 4, 1)
    _put(lab, 0, 3, 10, 1, 1, 1)
    _put(lab, 0, 3, 12, 1, 6, 1)
    _put(lab, 1, 3, 10, 1, 4, 1)
    return lab


def _threshold():
    """min_iou = 100.  Row 0: 5 and 6 pixels that share one, u = 10: 1000 ov == 100 u, a candidate.  Row 3: 5 and 7 pixels that share
    one, u = 11: one pixel under it."""
    lab = np.zeros((2, 5, 23), dtype=np.uint8)              # (115 pixels: no multiple of four)
    _put(lab, 0, 0, 0, 1, 5, 1)
    _put(lab, 1, 0, 4, 1, 6, 1)
    _put(lab, 0, 3, 0, 1, 5, 1)
    _put(lab, 1, 3, 4, 1, 7, 1)
    return lab


def _class_change():
    lab = np.zeros((3, 9, 25), dtype=np.uint8)              # (225 pixels: no multiple of four)
    for f in range(3):
        _put(lab, f, 1, 2 + f, 4, 6, 1 if f < 2 else 2)      # changes class in frame 2
        _put(lab, f, 6, 12, 3, 5, 2)
    return lab


def _min_area():
    """min_area = 5: a 4-pixel blob takes no part until it has grown to 6 pixels in frame 2; the large blob is followed throughout."""
    lab = np.zeros((3, 10, 24), dtype=np.uint8)
    for f in range(3):
        _put(lab, f, 1, 2, 2, 2 if f < 2 else 3, 1)
        _put(lab, f, 5, 8 + f, 4, 8, 1)
    return lab


def _truncation():
    """Four blobs in every frame and K = 2: only the first two in raster order have rows, the pixels of the others count nowhere."""
    lab = np.zeros((3, 20, TW + 6), dtype=np.uint8)
    for f in range(3):
        for b in range(4):
            _put(lab, f, 1 + 4 * b, 3 + 9 * b + f, 3, 6, 1 + b % 2)
    return lab


def _full_k():
    """Two TH x TW checkerboards of classes 1 and 2 at 4-connectivity, the second shifted by one pixel: 1024 one-pixel instances on both
    sides, each over the instance of the other class."""
    y, x = np.mgrid[0:TH, 0:TW]
    return np.stack([1 + (y + x) % 2, 1 + (y + x + 1) % 2]).astype(np.uint8)


def _overflow():
    """40 x 16384.  Frame 0 is one instance of 655360 pixels.  Frame 1 splits it into rows 0 .. 19 (ov 327680) and rows 21 .. 39 (ov
    311296), both with u = 655360.  ov u' = 50 * 2^32 and ov' u = 95 * 2^31: as 32-bit products 0 and 2^31, the wrong way round."""
    lab = np.ones((2, 40, 16384), dtype=np.uint8)
    lab[1, 20] = 0
    return lab


def _empty_frame():
    lab = np.zeros((4, 12, 24), dtype=np.uint8)
    for f in (0, 1, 3):
        _put(lab, f, 1, 2 + f, 3, 5, 1)
        _put(lab, f, 6, 10 + f, 4, 4, 2)
    return lab


@functools.lru_cache(maxsize=None)
def cases():
    return (
        _case("moving_130", _moving(2 * TW + 2)),
        _case("moving_128", _moving(2 * TW)),
        _case("enter_leave", _enter_leave()),
        _case("split_merge", _split_merge()),
        _case("crossing", _crossing()),
        _case("chain", _chain(), min_iou=50),
        _case("tie", _tie()),
        _case("threshold", _threshold()),
        _case("class_change_same", _class_change()),
        _case("class_change_any", _class_change(), same_class=False),
        _case("min_area", _min_area(), min_area=5),
        _case("truncation", _truncation(), K=2),
        _case("full_k_same", _full_k(), K=1024, connectivity=4, skip=()),
        _case("full_k_any", _full_k(), K=1024, connectivity=4, skip=(), same_class=False),
        _case("overflow", _overflow(), K=4),
        _case("empty_frame", _empty_frame()),
    )


NAMES = tuple(c["name"] for c in cases())


def case(name):
    return cases()[NAMES.index(name)]


def _host_components_fast(lab):
    """label_components of a map whose non-zero rows are whole rows of one class (the 40 x 16384 case, which the per-pixel definition
    takes minutes for): every maximal band of non-zero rows is one instance.  -> (components, [(class, first, area)])."""
    H, W = lab.shape
    comp = np.full((H, W), -1, dtype=np.int32)
    found, y = [], 0
    while y < H:
        if lab[y, 0] == 0:
            y += 1
            continue
        y1 = y
        while y1 < H and lab[y1, 0] == lab[y, 0]:
            y1 += 1
        comp[y:y1] = len(found)
        found.append((int(lab[y, 0]), y * W, (y1 - y) * W))
        y = y1
    return comp, found


@functools.lru_cache(maxsize=None)
def host_components(name):
    """Per frame (components int32 [H][W], rows int64 [K][12], total) of the case by the numpy definition."""
    c = case(name)
    lab = c["labels"]
    if name == "overflow":                       # whole rows of one class: bands (only class, first pixel and area of the rows are filled)
        assert all((fr == fr[:, :1]).all() for fr in lab)
        out = []
        for fr in lab:
            comp, found = _host_components_fast(fr)
            rows = np.zeros((c["K"], I.INSTANCE_ROW), dtype=np.int64)
            for i, (cl, first, area) in enumerate(found[:c["K"]]):
                rows[i, :3] = cl, first, area
            out.append((comp, rows, len(found)))
        return tuple(out)
    comp, rows, total = I.label_components(lab, c["nc"], c["connectivity"], c["skip"], c["K"])
    return tuple((comp[f], rows[f], int(total[f])) for f in range(lab.shape[0]))


def tracker(c):
    return I.InstanceTracker(c["K"], c["min_iou"], c["same_class"], c["min_area"])


@functools.lru_cache(maxsize=None)
def host_tracks(name):
    """Per frame (ids int32 [K], started) of the case by utils.instruments.InstanceTracker over host_components."""
    t = tracker(case(name))
    return tuple(t.update(comp, rows, total) for comp, rows, total in host_components(name))
