"""Synthetic sequences for the tracker with a memory (utils.instruments.MemoryTracker, hip.track_instances on a
hip.TrackState(..., max_gap=g)), shared by tests/test_tracks_memory_host.py and tests/test_hip_tracks_memory.py.  Built like the cases of
tests/tracks_cases.py - sequences of label maps around the 16 x 64 tile of the component kernels, at most 40 x 140 pixels - with frames
in which an instrument is out of view.  A case is the dict of tracks_cases; the gap it is run with is the caller's."""
import functools

import numpy as np

from stswincl_amd.utils import instruments as I
from tracks_cases import TH, TW, _case, _put

GAPS = (0, 1, 3)            # what the GPU tests run every case with (0: the memory kernels with nothing to remember)


def _flicker():
    """A, (TH + 2) x (TW + 3) of class 1 over four tiles, is there in frames 0, 2 and 5; B, a 2 x 26 bar of class 2, always.  A comes
    first in raster order: B is ordinal 1 beside it and ordinal 0 alone."""
    lab = np.zeros((6, TH + 8, TW + 10), dtype=np.uint8)
    for f in range(6):
        if f in (0, 2, 5):
            _put(lab, f, 2, 3, TH + 2, TW + 3, 1)
        _put(lab, f, TH + 5, 5, 2, 26, 2)
    return lab


def _expiry_exact():
    """One blob in frames 0, 3 and 7 of a 9 x 25 map (225 pixels): out of view for two frames, then for three."""
    lab = np.zeros((8, 9, 25), dtype=np.uint8)
    for f in (0, 3, 7):
        _put(lab, f, 2, 4, 4, 6, 1)
    return lab


def _overwritten(cls_b):
    """A, 6 x 10 of class 1 at columns 2 .. 11, is there in frames 0 and 3.  B, 6 x 10 of class cls_b, stands at columns 40 .. 49 in
    frames 0, 1 and 3 and in frame 2 at columns 3 .. 12: on A's remembered place, all of it but column 2, and off its own."""
    lab = np.zeros((4, 10, TW + 6), dtype=np.uint8)
    for f in (0, 3):
        _put(lab, f, 2, 2, 6, 10, 1)
    for f in (0, 1, 3):
        _put(lab, f, 2, 40, 6, 10, cls_b)
    _put(lab, 2, 2, 3, 6, 10, cls_b)
    return lab


_PLACES = (2, 20, 38, 56)


def _capacity():
    """K = 2.  4 x 8 blobs of class 1 at four places of one row band: frame 0 places 0 and 1, frame 1 place 2, frame 2 place 3,
    frame 3 place 2 again, frame 4 places 0 and 3."""
    lab = np.zeros((5, 8, TW + 6), dtype=np.uint8)
    for f, places in enumerate(((0, 1), (2,), (3,), (2,), (0, 3))):
        for p in places:
            _put(lab, f, 2, _PLACES[p], 4, 8, 1)
    return lab


def _slot_reuse():
    """A at place 0 in frame 0, nothing in frames 1 and 2, B at place 1 from frame 3 on, C at place 0 - where A was - in frame 4."""
    lab = np.zeros((5, 8, TW + 6), dtype=np.uint8)
    _put(lab, 0, 2, _PLACES[0], 4, 8, 1)
    for f in (3, 4):
        _put(lab, f, 2, _PLACES[1], 4, 8, 1)
    _put(lab, 4, 2, _PLACES[0], 4, 8, 1)
    return lab


def _tie_by_id():
    """Frame 0: X at columns 16 .. 18, track 0.  Frame 1: Y at columns 10 .. 12 joins to its left, so Y is ordinal 0 with track 1 and X
    ordinal 1 with track 0.  Frame 2: Z at columns 12 .. 16 shares one pixel with each, (ov, u) = (1, 7) twice: the smaller track id is
    X's, the smaller previous ordinal Y's."""
    lab = np.zeros((3, 5, 24), dtype=np.uint8)
    for f in (0, 1):
        _put(lab, f, 2, 16, 1, 3, 1)
    _put(lab, 1, 2, 10, 1, 3, 1)
    _put(lab, 2, 2, 12, 1, 5, 1)
    return lab


def _min_area_gap():
    """min_area = 5: a blob of 6 pixels has 4 in frame 1 and 6 again in frame 2; a 4 x 8 blob is followed throughout."""
    lab = np.zeros((3, 10, 24), dtype=np.uint8)
    for f in range(3):
        _put(lab, f, 1, 2, 2, 2 if f == 1 else 3, 1)
        _put(lab, f, 5, 8 + f, 4, 8, 1)
    return lab


def _odd_size():
    """7 x 23 = 161 pixels: a blob that holds the map's last pixel is away in frame 1, one at the first pixel stays."""
    lab = np.zeros((3, 7, 23), dtype=np.uint8)
    for f in range(3):
        _put(lab, f, 0, 0, 2, 3, 1)
        if f != 1:
            _put(lab, f, 4, 19, 3, 4, 2)
    return lab


def _full_k(evict):
    """The TH x TW checkerboard of classes 1 and 2 at 4-connectivity, 1024 one-pixel instances, in frames 0 and 2 and nothing in frame 1.
    evict: a row below the board, empty but for a 1 x 4 bar of class 3 in frame 1 - a 1025th track beside 1024 lost ones of one age, so
    the one of the smallest id ends and its pixel is born again in frame 2."""
    y, x = np.mgrid[0:TH, 0:TW]
    lab = np.zeros((3, TH + (1 if evict else 0), TW), dtype=np.uint8)
    lab[0, :TH] = lab[2, :TH] = 1 + (y + x) % 2
    if evict:
        _put(lab, 1, TH, 0, 1, 4, 3)
    return lab


@functools.lru_cache(maxsize=None)
def cases():
    return (
        _case("flicker", _flicker()),
        _case("expiry_exact", _expiry_exact()),
        _case("overwritten_same", _overwritten(1)),
        _case("overwritten_other", _overwritten(2)),
        _case("capacity", _capacity(), K=2),
        _case("slot_reuse", _slot_reuse()),
        _case("tie_by_id", _tie_by_id()),
        _case("min_area_gap", _min_area_gap(), min_area=5),
        _case("odd_size", _odd_size()),
        _case("full_k", _full_k(False), K=1024, connectivity=4),
        _case("full_k_evict", _full_k(True), K=1024, nc=4, connectivity=4),
    )


NAMES = tuple(c["name"] for c in cases())


def case(name):
    return cases()[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def host_components(name):
    """Per frame (components int32 [H][W], rows int64 [K][12], total) of the case by the numpy definition."""
    c = case(name)
    comp, rows, total = I.label_components(c["labels"], c["nc"], c["connectivity"], c["skip"], c["K"])
    return tuple((comp[f], rows[f], int(total[f])) for f in range(c["labels"].shape[0]))


def tracker(c, max_gap):
    return I.MemoryTracker(c["K"], max_gap, c["min_iou"], c["same_class"], c["min_area"])


def run(c, components, max_gap):
    """Per frame (ids int32 [K], started) of utils.instruments.MemoryTracker over `components` (the host_components of either module)."""
    t = tracker(c, max_gap)
    return tuple(t.update(comp, rows, total) for comp, rows, total in components)


@functools.lru_cache(maxsize=None)
def host_tracks(name, max_gap):
    return run(case(name), host_components(name), max_gap)
