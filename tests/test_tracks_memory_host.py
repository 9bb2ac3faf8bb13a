"""utils.instruments.MemoryTracker, the numpy definition of the tracker with a memory: against InstanceTracker at max_gap = 0 on the
cases of tests/tracks_cases.py, against expectations stated here by hand on the cases of tests/tracks_memory_cases.py, its refusals,
and TrackReport over ids with gaps.  No GPU."""
import numpy as np
import pytest

import tracks_cases as TC
import tracks_memory_cases as MC
from stswincl_amd.utils import instruments as I


def _ids(name, gap):
    """Per frame the ids of the participants' ordinals (up to the last one that takes part) and started."""
    out = []
    for ids, started in MC.host_tracks(name, gap):
        n = int(np.nonzero(ids >= 0)[0].max()) + 1 if (ids >= 0).any() else 0
        out.append((ids[:n].tolist(), started))
    return out


# Every case of tracks_cases runs (`overflow` too: its components come from the module's own fast path), and none differs: where two
# pairs are equally preferred in them (`tie`), track ids ascend with the previous ordinals.
@pytest.mark.parametrize("name", TC.NAMES)
def test_gap_0_is_the_instance_tracker(name):
    got = MC.run(TC.case(name), TC.host_components(name), 0)
    want = TC.host_tracks(name)
    assert len(got) == len(want)
    for f, ((ids, started), (want_ids, want_started)) in enumerate(zip(got, want)):
        assert ids.dtype == np.int32 and np.array_equal(ids, want_ids) and started == want_started, (name, f)


@pytest.mark.parametrize("gap", [1, 3])
def test_empty_frame_keeps_its_ids(gap):
    got = MC.run(TC.case("empty_frame"), TC.host_components("empty_frame"), gap)
    assert [g[0][:3].tolist() for g in got] == [[0, 1, -1], [0, 1, -1], [-1, -1, -1], [0, 1, -1]]
    assert [g[1] for g in got] == [2, 2, 2, 2]
    assert TC.host_tracks("empty_frame")[3][0][:2].tolist() == [2, 3] and TC.host_tracks("empty_frame")[3][1] == 4      # (without)


@pytest.mark.parametrize("name", [n for n in TC.NAMES if n != "empty_frame"])
def test_a_gap_starts_no_track_less_where_nothing_flickers(name):
    for gap in (1, 3):
        assert MC.run(TC.case(name), TC.host_components(name), gap)[-1][1] == TC.host_tracks(name)[-1][1], gap


def test_flicker():
    assert _ids("flicker", 0) == [([0, 1], 2), ([1], 2), ([2, 1], 3), ([1], 3), ([1], 3), ([3, 1], 4)]
    assert _ids("flicker", 1) == [([0, 1], 2), ([1], 2), ([0, 1], 2), ([1], 2), ([1], 2), ([2, 1], 3)]      # kept over frame 1, not over 3 - 4
    for gap in (2, 3):
        assert _ids("flicker", gap) == [([0, 1], 2), ([1], 2), ([0, 1], 2), ([1], 2), ([1], 2), ([0, 1], 2)]


def test_expiry_exact():
    none = ([], None)
    strip = lambda got: [(ids, started) if ids else none for ids, started in got]
    assert strip(_ids("expiry_exact", 1)) == [([0], 1), none, none, ([1], 2), none, none, none, ([2], 3)]
    assert strip(_ids("expiry_exact", 2)) == [([0], 1), none, none, ([0], 1), none, none, none, ([1], 2)]     # away for 2: back; for 3: new
    assert strip(_ids("expiry_exact", 3)) == [([0], 1), none, none, ([0], 1), none, none, none, ([0], 1)]
    assert [s for _, s in _ids("expiry_exact", 2)] == [1, 1, 1, 1, 1, 1, 1, 2]


def test_overwritten():
    # B jumps onto A's remembered place (ov 54 of u 66) and inherits id 0; its own track 1 waits where B was, and when A comes back
    # it finds B's mask under id 0 while B returns to its place: the documented property.
    for gap in (1, 3):
        assert _ids("overwritten_same", gap) == [([0, 1], 2), ([1], 2), ([0], 2), ([0, 1], 2)]
    assert _ids("overwritten_same", 0) == [([0, 1], 2), ([1], 2), ([2], 3), ([2, 3], 4)]
    # B of another class is born as 2 there and takes the pixels: A's remembered mask shrinks to column 2, 6 pixels, and A's return
    # (u = 60 + 60 - 6 = 114, 6000 < 11400) is no candidate any more - a new id 3; B goes back to its own track 1.
    for gap in (1, 3):
        assert _ids("overwritten_other", gap) == [([0, 1], 2), ([1], 2), ([2], 3), ([3, 1], 4)]
    t = MC.tracker(MC.case("overwritten_other"), 3)
    for f, (comp, rows, total) in enumerate(MC.host_components("overwritten_other")):
        t.update(comp, rows, total)
        if f == 1:
            assert int((t.mem == 0).sum()) == 60
        if f == 2:
            assert int((t.mem == 0).sum()) == 6 and t.live[0] == (1, 60, 2) and int((t.mem == 2).sum()) == 60


def test_capacity():
    # K = 2.  Frame 1: tracks 0 and 1 are lost with one age beside the new 2 - the smaller id, 0, ends.  Frame 2: 1 (age 2) and 2
    # (age 1) beside the new 3 - the older, 1, ends.  Frame 3 finds 2 again; frame 4 finds 3 again and place 0 born anew.
    assert _ids("capacity", 3) == [([0, 1], 2), ([2], 3), ([3], 4), ([2], 4), ([4, 3], 5)]
    assert _ids("capacity", 0) == [([0, 1], 2), ([2], 3), ([3], 4), ([4], 5), ([5, 6], 7)]
    t = MC.tracker(MC.case("capacity"), 3)
    lives = []
    for comp, rows, total in MC.host_components("capacity"):
        t.update(comp, rows, total)
        lives.append(sorted(t.live))
    assert lives == [[0, 1], [1, 2], [2, 3], [2, 3], [3, 4]]


def test_slot_reuse():
    # gap 1: A's track ends in frame 2; what is at its place in frame 4 is new although B was born in between
    assert _ids("slot_reuse", 1) == [([0], 1), ([], 1), ([], 1), ([1], 2), ([2, 1], 3)]
    assert _ids("slot_reuse", 3) == [([0], 1), ([], 1), ([], 1), ([1], 2), ([0, 1], 2)]       # (alive for three frames: back)


def test_tie_by_id():
    for gap in MC.GAPS:
        assert _ids("tie_by_id", gap) == [([0], 1), ([1, 0], 2), ([0], 2)]
    c = MC.case("tie_by_id")
    t = TC.tracker(c)                                                      # the tracker without memory breaks the tie by the ordinal
    got = [t.update(comp, rows, total) for comp, rows, total in MC.host_components("tie_by_id")]
    assert got[2][0][0] == 1 and got[2][1] == 2


def test_min_area_gap():
    assert _ids("min_area_gap", 1) == [([0, 1], 2), ([-1, 1], 2), ([0, 1], 2)]
    assert _ids("min_area_gap", 0) == [([0, 1], 2), ([-1, 1], 2), ([2, 1], 3)]


def test_odd_size():
    assert MC.case("odd_size")["labels"][0].size % 4 == 1 and MC.case("odd_size")["labels"][0, -1, -1] == 2
    assert _ids("odd_size", 1) == [([0, 1], 2), ([0], 2), ([0, 1], 2)]
    assert _ids("odd_size", 0) == [([0, 1], 2), ([0], 2), ([0, 2], 3)]


def test_full_k():
    every = np.arange(1024, dtype=np.int32)
    for gap in (1, 3):
        (a, sa), (b, sb), (c, sc) = MC.host_tracks("full_k", gap)
        assert np.array_equal(a, every) and (b == -1).all() and np.array_equal(c, every) and (sa, sb, sc) == (1024, 1024, 1024)
        (a, sa), (b, sb), (c, sc) = MC.host_tracks("full_k_evict", gap)      # track 0 made room for the bar's 1024; its pixel is 1025
        assert np.array_equal(a, every) and b[0] == 1024 and (b[1:] == -1).all() and (sa, sb, sc) == (1024, 1025, 1026)
        assert c[0] == 1025 and np.array_equal(c[1:], every[1:])
    (a, sa), (b, sb), (c, sc) = MC.host_tracks("full_k", 0)
    assert np.array_equal(c, every + 1024) and sc == 2048


def test_refusals():
    for kw in (dict(K=0), dict(K=1025), dict(K=2.5), dict(K=True), dict(max_gap=-1), dict(max_gap=1.5), dict(max_gap=True),
               dict(max_gap=1000001), dict(min_iou=-1), dict(min_iou=1001), dict(min_iou=0.5), dict(min_area=0), dict(min_area=1.5)):
        with pytest.raises(ValueError, match="MemoryTracker"):
            I.MemoryTracker(**{**dict(K=4, max_gap=1), **kw})
    with pytest.raises(TypeError):
        I.MemoryTracker(4)                                                 # max_gap has no default: a MemoryTracker is asked for one
    t = I.MemoryTracker(4, 1)
    rows = np.zeros((4, I.INSTANCE_ROW), dtype=np.int64)
    comp = np.full((3, 5), -1, dtype=np.int32)
    for bad in (comp[0], comp.astype(np.float32), comp[:, :0]):
        with pytest.raises(ValueError, match="components"):
            t.update(bad, rows, 0)
    for bad in (rows[:3], rows[:, :5], rows.astype(np.float64)):
        with pytest.raises(ValueError, match="rows"):
            t.update(comp, bad, 0)
    t.update(comp, rows, 0)
    with pytest.raises(ValueError, match="reset"):
        t.update(np.full((3, 6), -1, dtype=np.int32), rows, 0)
    t.reset()
    assert t.update(np.full((3, 6), -1, dtype=np.int32), rows, 0)[1] == 0


def test_track_report_takes_ids_with_gaps():
    c = MC.case("flicker")
    comps = MC.host_components("flicker")
    n, (H, W) = len(comps), comps[0][0].shape
    rep = I.InstanceReport.from_rows(np.stack([r for _, r, _ in comps]), np.asarray([t for _, _, t in comps]), (H, W),
                                     frames=list(range(n)), sequences=[0] * n)
    got = MC.host_tracks("flicker", 2)
    tr = I.TrackReport.from_ids(rep, np.stack([g[0] for g in got]), np.asarray([g[1] for g in got]))
    assert [t["track"] for t in tr.tracks] == [0, 1]
    a, b = tr.tracks
    assert (a["first"], a["last"], a["seen"]) == (0, 5, 3) and a["seen"] < a["last"] - a["first"] + 1 and a["frames"].tolist() == [0, 2, 5]
    assert (b["first"], b["last"], b["seen"]) == (0, 5, 6) and a["class"] == 1 and b["class"] == 2
    assert a["areas"].tolist() == [(TC.TH + 2) * (TC.TW + 3)] * 3 and tr.started.tolist() == [2] * 6
    assert c["K"] == 8 and tr.ids.shape == (6, 8)
