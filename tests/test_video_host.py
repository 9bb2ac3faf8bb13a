"""Host side of stswincl_amd.video (no GPU): the Pillow resize restatement the ingest kernel is checked against, the host
coefficient tables, the reference's clip rule and release schedule, the frame-feature ring plan, the device log (on the CPU) and
the tracker's frame order over the planner's release order."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_ref as R  # noqa: E402

from stswincl_amd import video  # noqa: E402
from stswincl_amd.hip import StswinHipError  # noqa: E402

SIZES = [(1024, 1280, 512, 640), (1080, 1920, 512, 640), (540, 960, 512, 640), (256, 320, 512, 640), (37, 53, 16, 20),
         (540, 640, 512, 640), (512, 960, 512, 640), (512, 640, 512, 640)]     # (one axis changes: one pass)


@pytest.mark.parametrize("hs,ws,h,w", SIZES)
def test_resize_ref_is_bit_exact_with_pillow(hs, ws, h, w):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(hs * 7 + ws)
    img = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    img[: hs // 8] = 255                                   # saturated and dark bands: the clip of the fixed-point sum
    img[hs // 8: hs // 4] = 0
    got = R.resize(img, h, w)
    want = np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n_in,n_out", [(1280, 640), (1920, 640), (960, 640), (320, 640), (53, 20), (37, 16), (1024, 512),
                                        (1080, 512), (540, 512), (256, 512)])
def test_device_tables_match_the_restatement(n_in, n_out):
    """video.bilinear_coeffs (vectorised, what the kernel gets) equals the per-index restatement of Resample.c."""
    b, k = video.bilinear_coeffs(n_in, n_out)
    xmin, n, kk = R.coeffs(n_in, n_out)
    assert b.dtype == np.int32 and k.dtype == np.int32
    assert np.array_equal(b[:, 0], xmin) and np.array_equal(b[:, 1], n)
    assert np.array_equal(k, kk)
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all()
    assert np.abs(k.astype(np.int64).sum(1) - (1 << 22)).max() <= k.shape[1]


def test_value_table_is_the_references_division():
    u = np.arange(256)
    assert np.array_equal(video.VALUE_TABLE, (u.astype(float) / 255.).astype(np.float32))
    assert np.array_equal(video.VALUE_TABLE, u.astype(np.float32) / np.float32(255))


def _reference_clip(frame, t=4):
    """seg18/dataset/Endovis2018_new.py:119-124."""
    if t > frame:
        return list(range(frame + t - 1, frame - 1, -1))
    return list(range(frame - t + 1, frame + 1))


@pytest.mark.parametrize("n", [7, 8, 250])
def test_clip_rule_and_release_schedule(n):
    for f in range(n):
        assert list(video.clip_frames(f)) == _reference_clip(f)
    p = video.ClipPlanner(batch=1)
    released = {}
    for f in range(n):
        released[f] = [g for st in p.push(1) for g in st.clips]
    assert [g for st in p.finish() for g in st.clips] == []
    expect = {0: [], 1: [], 2: [], 3: [0], 4: [1, 4], 5: [2, 5], 6: [3, 6]}
    for f in range(n):
        assert released[f] == expect.get(f, [f]), f
        # a clip is released as soon as its frames are there, never earlier
        for g in released[f]:
            assert max(_reference_clip(g)) == f
    assert sorted(g for v in released.values() for g in v) == list(range(n))


def _simulate(n, batch, chunks, slots=None):
    """Run the planner over a sequence pushed in `chunks`, replaying its plan on a simulated ring; -> clips in run order."""
    p = video.ClipPlanner(batch=batch, slots=slots)
    ring = [None] * p.slots
    done = []
    steps = []
    f = 0
    for c in chunks:
        steps += p.push(c)
        f += c
    assert f == n
    steps += p.finish()
    processed = set()
    for st in steps:
        assert 1 <= len(st.clips) <= batch
        assert len(st.stores) == len(st.new)
        assert not processed & set(st.new)
        processed |= set(st.new)
        read = set()
        for g, src in zip(st.clips, st.sources):
            got = []
            for e in src:
                if e >= 0:
                    read.add(e)
                    got.append(ring[e])
                else:
                    got.append(st.new[-1 - e])
            assert got == _reference_clip(g), (g, got, st)
        stored = [s for s in st.stores if s >= 0]
        assert len(stored) == len(set(stored))
        assert not read & set(stored), f"step stores into a slot it reads: {st}"
        assert all(0 <= s < p.slots for s in stored)
        for fr, s in zip(st.new, st.stores):
            if s >= 0:
                ring[s] = fr
        done += st.clips
        tab = st.table()
        assert len(tab) == 4 * len(st.clips) + len(st.new)
    assert processed == set(range(n))
    return done


def test_ring_plan_never_overwrites_a_slot_still_needed():
    """Property test over random sequence lengths, batch sizes and push chunkings: every clip is run once, reads exactly the
    reference's frames (from the ring or this step's new frames), and no store hits a slot that the same step reads or that a
    later clip still needs (a later read of an overwritten slot would return the wrong frame)."""
    rnd = random.Random(1234)
    for _ in range(300):
        n = rnd.randint(7, 90)
        batch = rnd.randint(1, 9)
        chunks = []
        left = n
        while left:
            c = min(left, rnd.choice([1, 1, 1, 2, 3, 5, 16, 64]))
            chunks.append(c)
            left -= c
        done = _simulate(n, batch, chunks)
        assert sorted(done) == list(range(n))


@pytest.mark.parametrize("batch", [1, 2, 4, 8])
def test_ring_wraps_and_steady_state_is_one_frame(batch):
    p = video.ClipPlanner(batch=batch)
    assert p.slots == max(7, batch + 3)
    steps = []
    for _ in range(60):
        steps += p.push(1)
    used = {s for st in steps for s in st.stores if s >= 0}
    assert used == set(range(p.slots)) or len(used) >= 7          # the cursor walks the whole ring
    if batch == 1:
        for st in steps[-40:]:
            assert len(st.new) == 1 and st.clips == st.new and sum(e < 0 for e in st.sources[0]) == 1
    _simulate(60, batch, [1] * 60)


def test_finish_refuses_a_sequence_too_short_for_the_rule():
    p = video.ClipPlanner(batch=1)
    p.push(6)
    with pytest.raises(StswinHipError, match="too short"):
        p.finish()
    p.reset()
    p.push(7)
    assert p.finish() == []


def test_ring_smaller_than_needed_is_refused():
    with pytest.raises(StswinHipError):
        video.ClipPlanner(batch=6, slots=8)


# ------------------------------------------------------------------------------------------------ the device log, on the CPU
def _log():
    import torch
    from stswincl_amd.video_report import DeviceLog
    return torch, DeviceLog("cpu", {"rows": ((2, 3), torch.int64), "ids": ((2,), torch.int32), "total": ((), torch.int32)})


def _row(torch, v):
    return dict(rows=torch.full((1, 2, 3), v, dtype=torch.int64), ids=torch.tensor([[v, -v]], dtype=torch.int32),
                total=torch.tensor([v + 1000], dtype=torch.int32))


def test_device_log_empty_download_has_the_columns_shapes_and_dtypes():
    torch, log = _log()
    cols, sequences, frames = log.download()
    assert list(cols) == ["rows", "ids", "total"] and sequences == [] and frames == []
    assert cols["rows"].shape == (0, 2, 3) and cols["rows"].dtype == np.int64
    assert cols["ids"].shape == (0, 2) and cols["ids"].dtype == np.int32
    assert cols["total"].shape == (0,) and cols["total"].dtype == np.int32
    assert list(log.download("ids")[0]) == ["ids"]


def test_device_log_grows_past_64_and_128_rows_and_keeps_its_contents():
    torch, log = _log()
    for f in range(130):
        assert log.append(f, **_row(torch, f)) == f
        assert log.capacity == (64 if f < 64 else 128 if f < 128 else 256)         # zeros of max(64, 2 n) rows
        assert all(t.shape[0] == log.capacity for t in log.data.values())
    cols, sequences, frames = log.download()
    assert frames == list(range(130)) and sequences == [0] * 130
    assert np.array_equal(cols["rows"], np.arange(130)[:, None, None].repeat(2, 1).repeat(3, 2))
    assert np.array_equal(cols["ids"], np.stack([np.arange(130), -np.arange(130)], 1)) and np.array_equal(cols["total"], np.arange(130) + 1000)
    assert int(log.data["rows"][130:].abs().sum()) == 0                        # what was never written is zero


def test_device_log_writes_a_row_after_later_rows_were_appended():
    torch, log = _log()
    log.append(0, **_row(torch, 0))
    late = log.append(4, rows=_row(torch, 4)["rows"], total=_row(torch, 4)["total"])         # (a parked frame: its ids come later)
    for f in (1, 2):
        log.append(f, **_row(torch, f))
    assert log.download("ids")[0]["ids"].tolist() == [[0, 0], [1, -1], [2, -2], [0, 0]]
    log.write(late, ids=torch.tensor([4, -4], dtype=torch.int32))              # [K], as the tracker hands it out
    cols, _, frames = log.download()
    assert frames == [0, 1, 2, 4] and cols["ids"].tolist() == [[0, 0], [1, -1], [2, -2], [4, -4]]
    assert cols["total"].tolist() == [1000, 1001, 1002, 1004] and cols["rows"][:, 0, 0].tolist() == [0, 1, 2, 4]


def test_device_log_orders_by_sequence_and_frame_and_counts_only_sequences_that_logged():
    torch, log = _log()
    for f in (0, 1, 4, 2, 5, 3):                                               # release order, not frame order
        log.append(f, **_row(torch, f))
    log.end_sequence()
    log.end_sequence()                                                         # a sequence that logged nothing uses up no ordinal
    log.end_sequence()
    for f in (1, 0, 2):
        log.append(f, **_row(torch, 10 + f))
    cols, sequences, frames = log.download()
    assert sequences == [0] * 6 + [1] * 3 and frames == [0, 1, 2, 3, 4, 5, 0, 1, 2]
    assert cols["total"].tolist() == [1000, 1001, 1002, 1003, 1004, 1005, 1010, 1011, 1012]
    assert cols["ids"][:, 0].tolist() == [0, 1, 2, 3, 4, 5, 10, 11, 12]
    log.end_sequence()
    assert log.sequence == 2


def test_device_log_clear_forgets_the_rows_and_restarts_the_ordinal():
    torch, log = _log()
    for f in range(70):
        log.append(f, **_row(torch, f))
    log.end_sequence()
    log.clear()
    assert log.sequence == 0 and log.download()[1:] == ([], []) and log.download()[0]["rows"].shape == (0, 2, 3)
    log.end_sequence()                                                         # nothing logged since clear()
    log.append(3, **_row(torch, 7))
    cols, sequences, frames = log.download()
    assert sequences == [0] and frames == [3] and cols["total"].tolist() == [1007] and log.capacity == 128


# ------------------------------------------------------------------------------------------------ the tracker's frame order
@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("batch", [1, 2, 3, 4])
@pytest.mark.parametrize("rule", video.RULES)
def test_track_sequencer_over_the_planner_s_release_order(rule, batch, chunk):
    """Driven with ClipPlanner's real release order: every frame is tracked exactly once, in frame order; at batch 1 exactly the
    frames VideoSegmenter's docstring names are parked; nothing is parked after finish()."""
    from stswincl_amd.video_report import TrackSequencer
    seq = TrackSequencer()
    for n in range(video.min_frames(rule), video.min_frames(rule) + 10):
        p = video.ClipPlanner(batch=batch, rule=rule)
        seq.reset()
        assert seq.next == 0 and not seq.parked
        tracked, parked, released = [], [], []
        steps = []
        for lo in range(0, n, chunk):
            steps += p.push(min(chunk, n - lo))
        for st in steps + p.finish():
            for g in st.clips:
                released.append(g)
                now = seq.release(g)
                assert (now == []) == (g != len(tracked)) and now[:1] in ([], [g])       # parked unless its predecessor is tracked
                if not now:
                    parked.append(g)
                    assert g in seq.parked
                tracked += now
                assert sorted(seq.parked) == sorted(set(released) - set(tracked))
        assert sorted(released) == list(range(n))
        assert tracked == list(range(n)), (rule, batch, n)
        assert not seq.parked and seq.next == n
        if batch == 1:
            assert parked == ([5, 6] if rule == "cadis" else [4, 5]), (rule, n)
        else:
            assert len(parked) >= 2
