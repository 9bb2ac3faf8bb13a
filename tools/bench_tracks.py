#!/usr/bin/env python3
"""Cost of following the instances from frame to frame (stswin_track_instances, VideoSegmenter(tracks=True)):

  tracks         the two launches of hip.track_instances alone (K = 256, min_iou 100, same class), one frame per call: 1024x1280 with
                 12 classes (EndoVis18) and 540x960 with 26 classes (CaDIS).  Measured as tools/bench_components.py measures its
                 launches: device events around replays of a captured hipGraph that holds one call per component map, `buffer_sets`
                 int32 maps with their rows and totals, together larger than the 256 MB last-level cache, so that every current map
                 comes from HBM; the state (with the previous map) and the outputs are one set, reused by every call, as the segmenter
                 reuses them.  The maps are hip.label_components of that tool's label maps: 16 scenes, each for `SHIFTS` = 4 frames
                 in which it moves 4 pixels to the right per frame, then a cut to the next scene, 64 distinct frames repeated over
                 the sets; `matched_per_cycle` and `started_per_cycle` say what the tracker made of one cycle of 64.  The ids of that
                 cycle are compared with utils.instruments.InstanceTracker before timing
  components     the launches of hip.label_components on the label maps of the same run (cold label maps, one set of outputs), the
                 yardstick beside it; tracks_over_components is the ratio
  host           the route a user has without the kernel: download the component map, rows and total, then
                 utils.instruments.InstanceTracker.update, wall time per frame, the median of `--host-frames` frames
  online         frames/s of VideoSegmenter(graph=True, out="labels", report="deferred", instances=256), bf16 autocast, GPU-resident
                 1024x1280 frames, one frame per push, push -> synchronise, with tracks=False (the parent's path: the yardstick) and
                 tracks=True, and with instances=None (what instances themselves cost, the same day), taking turns in windows of
                 `--frames` frames; the median window of each with its range (the yardstick's range is the run-to-run spread the
                 difference is read against), tracks_over_instances and instances_over_report

    python tools/bench_tracks.py [--reps 300] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_tracks_line.json

--max-gap g (g >= 1) adds the tracker with a memory (stswin_track_memory, VideoSegmenter(track_max_gap=g)) to the same run: per case
`memory_us_per_frame`, its three launches at max_gap = g on a state of their own, over the same cold maps in the same rotation as
`tracks_us_per_frame` (the two launches at max_gap = 0) and after one cycle against utils.instruments.MemoryTracker, with
memory_over_tracks; online gains the path `gap` (tracks=True, track_max_gap=g) beside `tracks`, with gap_over_tracks.  The line then
goes to profiles/bench_tracks_memory_line.json.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_instruments import CASES, COLD_BYTES, DISTINCT, _windows, instrument_maps  # noqa: E402
from online_loop import endovis_model, noisy_frames, take_turns  # noqa: E402
from stswincl_amd import hip, video  # noqa: E402
from stswincl_amd.utils import instruments  # noqa: E402

K = 256
SKIP = (0,)
SHIFTS = 4              # frames per scene
STEP = 4                # pixels a scene moves per frame


def launch_cost(case, a):
    (H, W), nc = CASES[case]
    gen = np.random.default_rng(a.seed)
    distinct = instrument_maps(gen, DISTINCT, H, W, nc)
    speck = gen.random(distinct.shape) < a.noise
    distinct[speck] = gen.integers(1, nc, distinct.shape).astype(np.uint8)[speck]
    distinct = np.stack([np.roll(scene, STEP * j, axis=1) for scene in distinct for j in range(SHIFTS)])
    cycle = len(distinct)
    dev = torch.from_numpy(distinct).cuda()
    comp, rows, total = hip.label_components(dev, nc, 8, SKIP, K)
    sets = max(2, -(-COLD_BYTES // (4 * H * W)))
    sets = -(-sets // cycle) * cycle                              # whole cycles: the captured sequence repeats exactly
    comps = comp.repeat(sets // cycle, 1, 1).contiguous()
    state = hip.TrackState(H, W, K, "cuda")
    out = (torch.empty(K, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
    host = instruments.InstanceTracker(K)
    matched = 0
    for i in range(cycle):                                        # one cycle against the definition
        ids, started = hip.track_instances(comps[i], rows[i], total[i:i + 1], state, out=out)
        want_ids, want_started = host.update(comp[i].cpu().numpy(), rows[i].cpu().numpy(), int(total[i]))
        if not np.array_equal(ids.cpu().numpy(), want_ids) or int(started[0]) != want_started:
            raise SystemExit(f"FAIL: the kernel and utils.instruments.InstanceTracker differ at {case}, frame {i}")
        if i:
            matched += int((want_ids >= 0).sum()) - (want_started - before)
        before = want_started
    state.reset()

    def tracks(k):
        hip.track_instances(comps[k], rows[k % cycle], total[k % cycle:k % cycle + 1], state, out=out)

    w = _windows(tracks, sets, a.reps, a.windows)
    us = float(np.median(w))
    totals = total.tolist()
    res = {"frame": [H, W], "classes": nc, "labels": f"synthetic bars and discs, single-pixel noise p = {a.noise}, {DISTINCT} scenes of {SHIFTS} frames, {STEP} pixels a frame",
           "max_instances": K, "total": [min(totals), int(np.median(totals)), max(totals)], "frames_per_cycle": cycle, "matched_per_cycle": matched,
           "started_per_cycle": before,
           "buffer_sets": sets, "buffer_bytes": sets * 4 * H * W, "state_bytes": state.bytes,
           "tracks_us_per_frame": round(us, 2), "tracks_us_range": [round(min(w), 2), round(max(w), 2)]}
    if a.max_gap:
        mstate = hip.TrackState(H, W, K, "cuda", max_gap=a.max_gap)
        mhost = instruments.MemoryTracker(K, a.max_gap)
        for i in range(cycle):                                    # one cycle against the definition
            ids, started = hip.track_instances(comps[i], rows[i], total[i:i + 1], mstate, out=out)
            want_ids, want_started = mhost.update(comp[i].cpu().numpy(), rows[i].cpu().numpy(), int(total[i]))
            if not np.array_equal(ids.cpu().numpy(), want_ids) or int(started[0]) != want_started:
                raise SystemExit(f"FAIL: the kernels and utils.instruments.MemoryTracker differ at {case}, frame {i}")
        mstate.reset()

        def memory(k):
            hip.track_instances(comps[k], rows[k % cycle], total[k % cycle:k % cycle + 1], mstate, out=out)

        w = _windows(memory, sets, a.reps, a.windows)
        mus = float(np.median(w))
        res.update({"max_gap": a.max_gap, "memory_started_per_cycle": want_started, "memory_state_bytes": mstate.bytes,
                    "memory_us_per_frame": round(mus, 2), "memory_us_range": [round(min(w), 2), round(max(w), 2)],
                    "memory_over_tracks": round(mus / us, 3)})
        del mstate
    del comps
    torch.cuda.empty_cache()
    lsets = max(2, -(-COLD_BYTES // (H * W)))
    labels = dev.repeat(-(-lsets // cycle), 1, 1)[:lsets].contiguous()
    cout = (torch.empty(1, H, W, dtype=torch.int32, device="cuda"), torch.empty(1, K, 12, dtype=torch.int64, device="cuda"),
            torch.empty(1, dtype=torch.int32, device="cuda"))
    ws = torch.empty(hip.label_components_scratch(1, H, W), dtype=torch.uint8, device="cuda")

    def components(k):
        hip.label_components(labels[k:k + 1], nc, 8, SKIP, K, out=cout, workspace=ws)

    w = _windows(components, lsets, a.reps, a.windows)
    cus = float(np.median(w))
    res.update({"components_us_per_frame": round(cus, 2), "components_us_range": [round(min(w), 2), round(max(w), 2)],
                "tracks_over_components": round(us / cus, 3)})
    torch.cuda.synchronize()
    host.reset()
    times = []
    for i in range(a.host_frames):
        t0 = time.perf_counter()
        host.update(comp[i % cycle].cpu().numpy(), rows[i % cycle].cpu().numpy(), int(total[i % cycle]))
        times.append((time.perf_counter() - t0) * 1e6)
    hus = float(np.median(times))
    res.update({"host_route": "download + utils.instruments.InstanceTracker", "host_us_per_frame": round(hus, 1),
                "host_us_range": [round(min(times), 1), round(max(times), 1)], "tracks_over_host": round(us / hus, 5)})
    return res


def online(a):
    (H, W), classes = (1024, 1280), 12
    model, name = endovis_model(a.seed, classes)
    n = 16
    frames = noisy_frames(np.random.default_rng(a.seed), n, H, W)
    paths = {"instances": dict(instances=K), "tracks": dict(instances=K, tracks=True), "report": {}}
    if a.max_gap:
        paths["gap"] = dict(instances=K, tracks=True, track_max_gap=a.max_gap)
    res = {"model": name, "frame": [H, W], "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows, "max_instances": K}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {p: video.VideoSegmenter(model, graph=True, out="labels", out_size=(H, W), report="deferred", **kw) for p, kw in paths.items()}
        fps = take_turns(segs, lambda p, k: segs[p].push(frames[k % n]), a.frames, a.online_windows)
        t0 = time.perf_counter()
        rep = segs["tracks"].track_report()
        res["track_report_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res.update(fps)
    res["reported_frames"] = len(rep)
    res["tracks_in_the_sequence"] = len(rep.tracks)
    res["tracks_over_instances"] = round(res["tracks_frames_per_s"] / res["instances_frames_per_s"], 4)
    res["instances_over_report"] = round(res["instances_frames_per_s"] / res["report_frames_per_s"], 4)
    if a.max_gap:
        res["max_gap"] = a.max_gap
        res["gap_over_tracks"] = round(res["gap_frames_per_s"] / res["tracks_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--noise", type=float, default=0.0001, help="density of the single-pixel noise on the label maps")
    ap.add_argument("--host-frames", type=int, default=5)
    ap.add_argument("--frames", type=int, default=48, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--max-gap", type=int, default=0, help="g >= 1: measure the tracker with a memory at max_gap = g as well")
    ap.add_argument("--out", default=None, help="profiles/bench_tracks_line.json, with --max-gap profiles/bench_tracks_memory_line.json")
    a = ap.parse_args()
    if not 0 <= a.max_gap <= hip.TRACK_MAX_GAP:
        raise SystemExit(f"--max-gap is 0 .. {hip.TRACK_MAX_GAP}")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bench_tracks_memory_line.json" if a.max_gap else "bench_tracks_line.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tracks.py measures on the GPU: no device found")
    res = {"launch": []}
    for case in CASES:
        res["launch"].append(dict(case=case, **launch_cost(case, a)))
        torch.cuda.empty_cache()
    if not a.no_online:
        res["online"] = online(a)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
