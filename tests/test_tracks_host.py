"""utils.instruments.InstanceTracker and TrackReport on the host: the tracker against an independent brute-force statement (overlaps by
np.unique of pairs, preferences as fractions.Fraction, one sorted sweep), every case of tests/tracks_cases.py shown to hold the point it
was built for, TrackReport on a hand-made log, and the refusals.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import tracks_cases as TC
from stswincl_amd.utils import instruments as I


def _brute(c, frames):
    """The definition, stated another way.  -> per frame a dict: ids, started, and what happened: matches [(i, j)], births, ends, the
    candidates [(pref, i, j, ov, u)] in order of preference, `late` matches (not the most preferred candidate of both their row and
    their column among all candidates: a second round's), ties (pairs of candidates of equal Fraction), on_threshold / under_threshold
    pairs, truncated (total > K)."""
    K, out = c["K"], []
    prev_map, prev = None, {}                      # ordinal -> (class, area, id)
    nxt = 0
    for comp, rows, total in frames:
        n = min(total, K)
        cur = {j: (int(rows[j][0]), int(rows[j][2])) for j in range(n) if int(rows[j][2]) >= c["min_area"]}
        cand, on_thr, under_thr = [], [], []
        if prev_map is not None:
            a, b = prev_map.reshape(-1).astype(np.int64), comp.reshape(-1).astype(np.int64)
            keep = (a >= 0) & (a < K) & (b >= 0) & (b < K)
            pairs, counts = np.unique(np.stack([a[keep], b[keep]]), axis=1, return_counts=True)
            for (i, j), ov in zip(pairs.T.tolist(), counts.tolist()):
                if i not in prev or j not in cur:
                    continue
                u = prev[i][1] + cur[j][1] - ov
                if c["same_class"] and prev[i][0] != cur[j][0]:
                    continue
                if Fraction(ov, u) >= Fraction(c["min_iou"], 1000):
                    cand.append((Fraction(ov, u), i, j, ov, u))
                    if Fraction(ov, u) == Fraction(c["min_iou"], 1000):
                        on_thr.append((i, j))
                elif Fraction(ov, u + 1) < Fraction(c["min_iou"], 1000) <= Fraction(ov + 1, u):     # within a pixel of it
                    under_thr.append((i, j))
        cand.sort(key=lambda t: (-t[0], t[1], t[2]))
        ids = np.full(K, -1, dtype=np.int32)
        ui, uj, matches, late = set(), set(), [], []
        for pref, i, j, ov, u in cand:             # one sweep in order of preference
            if i in ui or j in uj:
                continue
            ui.add(i), uj.add(j)
            ids[j] = prev[i][2]
            matches.append((i, j))
            if next(t for t in cand if t[1] == i)[2] != j or next(t for t in cand if t[2] == j)[1] != i:
                late.append((i, j))
        births = [j for j in sorted(cur) if j not in uj]
        for j in births:
            ids[j] = nxt
            nxt += 1
        ties = [(s, t) for k, s in enumerate(cand) for t in cand[k + 1:] if s[0] == t[0]]
        out.append(dict(ids=ids, started=nxt, matches=matches, births=births, ends=[i for i in sorted(prev) if i not in ui], cand=cand,
                        late=late, ties=ties, on_threshold=on_thr, under_threshold=under_thr, truncated=total > K, cur=cur, prev=dict(prev)))
        prev_map, prev = comp, {j: (cur[j][0], cur[j][1], int(ids[j])) for j in cur}
    return out


_BRUTE = {}


def _events(name):
    if name not in _BRUTE:
        _BRUTE[name] = _brute(TC.case(name), TC.host_components(name))
    return _BRUTE[name]


@pytest.mark.parametrize("name", TC.NAMES)
def test_tracker_is_the_brute_force_statement(name):
    want = _events(name)
    got = TC.host_tracks(name)
    assert len(got) == len(want)
    for f, ((ids, started), w) in enumerate(zip(got, want)):
        assert ids.dtype == np.int32 and ids.shape == (TC.case(name)["K"],)
        assert np.array_equal(ids, w["ids"]), (name, f)
        assert started == w["started"], (name, f)


def _id_of_pixel(name, f, y, x):
    comp = TC.host_components(name)[f][0]
    return int(TC.host_tracks(name)[f][0][comp[y, x]])


@pytest.mark.parametrize("name", ["moving_130", "moving_128"])
def test_moving_blobs_keep_their_ids(name):
    ev = _events(name)
    assert [len(e["cur"]) for e in ev] == [3] * 8
    for f in range(8):
        assert _id_of_pixel(name, f, 2, 2 + 2 * f) == 0 and _id_of_pixel(name, f, TC.TH + 9, 3 + 3 * f) == 1
        assert _id_of_pixel(name, f, TC.TH + 14, 100 + 3 * f) == 2 + f           # the single pixel never overlaps itself
    assert all(len(e["matches"]) == 2 and len(e["births"]) == 1 and len(e["ends"]) == 1 for e in ev[1:])


def test_enter_and_leave():
    ev = _events("enter_leave")
    assert [len(e["cur"]) for e in ev] == [1, 1, 1, 1, 1, 1]
    assert [e["started"] for e in ev] == [1, 1, 1, 2, 2, 2]
    assert ev[3]["ends"] == [0] and ev[3]["births"] == [0] and not ev[3]["matches"]


def test_split_and_merge_follow_the_larger_piece():
    ev = _events("split_merge")
    assert ev[1]["matches"] == [(0, 1)] and ev[1]["births"] == [0]               # the right piece is larger: the left one is born
    assert list(TC.host_tracks("split_merge")[1][0][:2]) == [1, 0]
    assert ev[2]["matches"] == [(1, 0)] and ev[2]["ends"] == [0]
    assert TC.host_tracks("split_merge")[2][0][0] == 0 and ev[2]["started"] == 2


def test_crossing_swaps_the_ordinals_and_not_the_ids():
    ev = _events("crossing")
    assert all(e["matches"] == [(0, 0), (1, 1)] for e in ev[1:4] + ev[5:]) and sorted(ev[4]["matches"]) == [(0, 1), (1, 0)]
    for f in range(7):
        assert _id_of_pixel("crossing", f, 2 + 2 * f, 5) == 0 and _id_of_pixel("crossing", f, 14 - 2 * f, 30) == 1
    assert ev[-1]["started"] == 2


def test_chain_needs_a_second_round():
    e = _events("chain")[1]
    assert [(t[1], t[2], t[3], t[4]) for t in e["cand"]] == [(0, 0, 80, 112), (1, 0, 24, 152), (1, 1, 4, 64)]
    assert e["matches"] == [(0, 0), (1, 1)] and e["late"] == [(1, 1)] and not e["births"]
    assert list(TC.host_tracks("chain")[1][0][:2]) == [0, 1]


def test_exact_ties():
    e = _events("tie")[1]
    got = {(t[1], t[2]): (t[3], t[4]) for t in e["cand"]}
    assert got == {(0, 0): (1, 2), (1, 1): (2, 4), (2, 2): (1, 4), (3, 2): (2, 8)}
    assert len(e["ties"]) == 2
    assert e["matches"] == [(0, 0), (1, 1), (2, 2)] and e["ends"] == [3]        # 1 / 4 == 2 / 8: the smaller i, not the larger overlap
    assert list(TC.host_tracks("tie")[1][0][:3]) == [0, 1, 2]


def test_threshold_boundary():
    e = _events("threshold")[1]
    assert e["on_threshold"] == [(0, 0)] and e["under_threshold"] == [(1, 1)]
    assert e["matches"] == [(0, 0)] and e["births"] == [1] and e["ends"] == [1]


def test_class_change():
    same, anyc = _events("class_change_same")[2], _events("class_change_any")[2]
    assert same["matches"] == [(1, 1)] and same["births"] == [0] and same["started"] == 3
    assert sorted(anyc["matches"]) == [(0, 0), (1, 1)] and not anyc["births"] and anyc["started"] == 2


def test_min_area():
    ev = _events("min_area")
    got = TC.host_tracks("min_area")
    assert [list(g[0][:2]) for g in got] == [[-1, 0], [-1, 0], [1, 0]]
    assert [sorted(e["cur"]) for e in ev] == [[1], [1], [0, 1]] and TC.host_components("min_area")[0][2] == 2


def test_truncation():
    ev = _events("truncation")
    assert all(e["truncated"] and sorted(e["cur"]) == [0, 1] for e in ev)
    assert all(e["matches"] == [(0, 0), (1, 1)] for e in ev[1:]) and ev[-1]["started"] == 2
    assert all(TC.host_components("truncation")[f][2] == 4 and TC.host_components("truncation")[f][0].max() == 3 for f in range(3))


def test_full_k():
    same, anyc = _events("full_k_same"), _events("full_k_any")
    assert len(same[0]["cur"]) == len(same[1]["cur"]) == 1024
    assert not same[1]["cand"] and len(same[1]["births"]) == 1024 and same[1]["started"] == 2048
    assert len(anyc[1]["matches"]) == 1024 and anyc[1]["started"] == 1024
    assert np.array_equal(TC.host_tracks("full_k_any")[1][0], np.arange(1024))


def test_overflow_case_shows_a_32_bit_product():
    e = _events("overflow")[1]
    (_, i0, j0, ov0, u0), (_, i1, j1, ov1, u1) = e["cand"]
    assert (i0, j0, i1, j1) == (0, 0, 0, 1) and ov0 * u1 > ov1 * u0 > 1 << 32
    assert (ov0 * u1) % (1 << 32) < (ov1 * u0) % (1 << 32)                       # wrapped, the products say the opposite
    assert e["matches"] == [(0, 0)] and e["births"] == [1]


def test_empty_frame_ends_everything():
    ev = _events("empty_frame")
    assert ev[1]["matches"] == [(0, 0), (1, 1)]
    assert not ev[2]["cur"] and ev[2]["ends"] == [0, 1] and ev[2]["started"] == 2
    assert not ev[3]["cand"] and ev[3]["births"] == [0, 1] and ev[3]["started"] == 4


def test_the_cases_together_hold_every_kind_of_event():
    ev = [e for name in TC.NAMES for e in _events(name)]
    for what in ("matches", "births", "ends", "ties", "late", "on_threshold", "under_threshold"):
        assert any(e[what] for e in ev), what
    assert any(e["truncated"] for e in ev)


def test_reset_starts_again_at_zero():
    c = TC.case("crossing")
    t = TC.tracker(c)
    frames = TC.host_components("crossing")
    first = [t.update(*fr) for fr in frames]
    t.reset()
    second = [t.update(*fr) for fr in frames]
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(first, second)) and second[0][1] == 2


def _hand_log():
    """Two sequences on a 10 x 20 map, K = 3: rows by hand (class, first, then the ten moments of a single row of pixels)."""
    def row(c, y, x0, w):
        xs = np.arange(x0, x0 + w)
        return [c, y * 20 + x0, w, xs.sum(), y * w, (xs * xs).sum(), (xs * y).sum(), y * y * w, 20 - x0, 10 - y, x0 + w, y + 1]

    rows = np.zeros((4, 3, 12), dtype=np.int64)
    rows[0, 0], rows[0, 1] = row(1, 1, 2, 4), row(2, 5, 3, 6)
    rows[1, 0], rows[1, 1] = row(2, 4, 4, 6), row(1, 6, 2, 5)
    rows[2, 0] = row(1, 2, 0, 3)
    rows[3, 0], rows[3, 1] = row(1, 2, 1, 3), row(2, 7, 7, 2)
    rep = I.InstanceReport.from_rows(rows, [2, 2, 1, 2], (10, 20), frames=[0, 1, 0, 1], sequences=[0, 0, 1, 1])
    ids = np.array([[0, 1, -1], [1, 0, -1], [0, -1, -1], [0, 1, -1]], dtype=np.int32)
    return rep, ids, np.array([2, 2, 1, 2])


def test_track_report_on_a_hand_made_log():
    rep, ids, started = _hand_log()
    tr = I.TrackReport.from_ids(rep, ids, started)
    assert len(tr) == 4 and np.array_equal(tr.ids, ids) and tr.ids.dtype == np.int32 and list(tr.started) == [2, 2, 1, 2]
    assert [(t["sequence"], t["track"], t["class"], t["first"], t["last"], t["seen"]) for t in tr.tracks] == [
        (0, 0, 1, 0, 1, 2), (0, 1, 2, 0, 1, 2), (1, 0, 1, 0, 1, 2), (1, 1, 2, 1, 1, 1)]
    t = tr.tracks[0]
    assert list(t["frames"]) == [0, 1] and list(t["areas"]) == [4, 5]
    assert np.array_equal(t["centroids"], np.array([[3.5, 1.0], [4.0, 6.0]]))
    assert np.array_equal(t["centroids"][1], rep.centroid[1, 1])
    rows = tr.as_rows()
    assert [r["track"] for r in rows] == [0, 1, 1, 0, 0, 0, 1]
    assert [{k: v for k, v in r.items() if k != "track"} for r in rows] == rep.as_rows()


def test_refusals():
    rep, ids, started = _hand_log()
    with pytest.raises(ValueError):
        I.TrackReport.from_ids(rep, ids[:3], started)
    with pytest.raises(ValueError):
        I.TrackReport.from_ids(rep, ids[:, :2], started)
    with pytest.raises(ValueError):
        I.TrackReport.from_ids(rep, ids.astype(np.float32), started)
    with pytest.raises(ValueError):
        I.TrackReport.from_ids(rep, ids, started[:3])
    with pytest.raises(ValueError):
        I.TrackReport.from_ids(rep.rows, ids, started)
    bad = ids.copy()
    bad[0, 2] = 5                                                   # an id where the report holds no instance
    with pytest.raises(ValueError):
        I.TrackReport.from_ids(rep, bad, started)
    for kw in (dict(K=0), dict(K=1025), dict(K=True), dict(K=4, min_iou=-1), dict(K=4, min_iou=1001), dict(K=4, min_iou=0.5),
               dict(K=4, min_area=0)):
        with pytest.raises(ValueError):
            I.InstanceTracker(**kw)
    t = I.InstanceTracker(3)
    comp = np.full((10, 20), -1, dtype=np.int32)
    rows = np.zeros((3, 12), dtype=np.int64)
    with pytest.raises(ValueError):
        t.update(comp[0], rows, 0)
    with pytest.raises(ValueError):
        t.update(comp.astype(np.float32), rows, 0)
    with pytest.raises(ValueError):
        t.update(comp, rows[:2], 0)
    t.update(comp, rows, 0)
    with pytest.raises(ValueError):
        t.update(comp[:5], rows, 0)                                 # another shape within a sequence
