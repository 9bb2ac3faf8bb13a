#!/usr/bin/env python3
"""Cost of splitting the instrument report into connected instances (stswin_label_components, VideoSegmenter(instances=K)):

  components     the launches of hip.label_components alone (K = 256, 8-connectivity, class 0 skipped), one frame per call: 1024x1280
                 with 12 classes (EndoVis18) and 540x960 with 26 classes (CaDIS).  Measured as tools/bench_instruments.py measures
                 the moments launch: device events around replays of a captured hipGraph that holds one call per label map,
                 `buffer_sets` maps, together larger than the 256 MB last-level cache, so that every label map comes from HBM; the
                 outputs and the workspace are one set, reused by every call, as the segmenter reuses them.  The label maps are that
                 tool's synthetic bars and discs plus a sprinkle of single-pixel noise (p = `--noise`), 16 distinct frames repeated
                 over the sets; `total` is their number of components (min, median, max over the 16).  The first map's total and
                 areas are compared with the host route's before timing
  moments        hip.label_moments on the same maps, timed the same way: the one-byte-per-pixel floor of a pass over the map
  host           the route a user has without the kernel: download the label map, then scipy.ndimage.label per class (the numpy
                 definition utils.instruments.label_components where scipy is not installed: `host_route` says which), wall time
                 per frame, the median of `--host-frames` frames
  online         frames/s of VideoSegmenter(graph=True, out="labels", report="deferred"), bf16 autocast, GPU-resident 1024x1280
                 frames, one frame per push, push -> synchronise, with instances=None (the parent's path: the yardstick) and
                 instances=256, taking turns in windows of `--frames` frames; the median window of each with its range and
                 instances_over_none

    python tools/bench_components.py [--reps 300] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_components_line.json
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

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def host_route(labels_dev, nc):
    """Download one label map [H][W] and label it per class on the host -> (total, areas sorted)."""
    lab = labels_dev.cpu().numpy()
    if ndimage is None:
        _, rows, total = instruments.label_components(lab, nc, 8, SKIP, 1024)
        return int(total[0]), sorted(rows[0, :int(total[0]), 2].tolist())
    areas = []
    for c in range(nc):
        if c in SKIP:
            continue
        comp, k = ndimage.label(lab == c, structure=np.ones((3, 3), dtype=int))
        if k:
            areas += np.bincount(comp.reshape(-1))[1:].tolist()
    return len(areas), sorted(areas)


def launch_cost(case, a):
    (H, W), nc = CASES[case]
    gen = np.random.default_rng(a.seed)
    per_set = H * W
    sets = max(2, -(-COLD_BYTES // per_set))
    distinct = instrument_maps(gen, DISTINCT, H, W, nc)
    speck = gen.random(distinct.shape) < a.noise
    distinct[speck] = gen.integers(1, nc, distinct.shape).astype(np.uint8)[speck]
    labels = torch.from_numpy(distinct).cuda().repeat(-(-sets // DISTINCT), 1, 1)[:sets].contiguous()
    out = (torch.empty(1, H, W, dtype=torch.int32, device="cuda"), torch.empty(1, K, 12, dtype=torch.int64, device="cuda"),
           torch.empty(1, dtype=torch.int32, device="cuda"))
    ws = torch.empty(hip.label_components_scratch(1, H, W), dtype=torch.uint8, device="cuda")
    totals = [int(hip.label_components(labels[i:i + 1], nc, 8, SKIP, K, out=out, workspace=ws)[2][0]) for i in range(DISTINCT)]
    _, rows, total = hip.label_components(labels[:1], nc, 8, SKIP, 1024)
    want_total, want_areas = host_route(labels[0], nc)
    if int(total[0]) != want_total or (want_total <= 1024 and sorted(rows[0, :want_total, 2].tolist()) != want_areas):
        raise SystemExit(f"FAIL: the kernel and the host route differ at {case}: {int(total[0])} components against {want_total}")

    def components(k):
        hip.label_components(labels[k:k + 1], nc, 8, SKIP, K, out=out, workspace=ws)

    w = _windows(components, sets, a.reps, a.windows)
    us = float(np.median(w))
    res = {"frame": [H, W], "classes": nc, "labels": f"synthetic bars and discs, single-pixel noise p = {a.noise}", "max_instances": K,
           "total": [min(totals), int(np.median(totals)), max(totals)], "buffer_sets": sets, "buffer_bytes": sets * per_set,
           "components_us_per_frame": round(us, 2), "components_us_range": [round(min(w), 2), round(max(w), 2)]}
    moms = torch.zeros(sets, nc, 10, dtype=torch.int64, device="cuda")

    def moments(k):
        hip.label_moments(labels[k:k + 1], nc, out=moms[k:k + 1])

    w = _windows(moments, sets, a.reps, a.windows)
    mus = float(np.median(w))
    res.update({"moments_us_per_frame": round(mus, 2), "moments_us_range": [round(min(w), 2), round(max(w), 2)],
                "components_over_moments": round(us / mus, 2)})
    torch.cuda.synchronize()
    host = []
    for i in range(a.host_frames):
        t0 = time.perf_counter()
        host_route(labels[i % sets], nc)
        host.append((time.perf_counter() - t0) * 1e6)
    hus = float(np.median(host))
    res.update({"host_route": "download + scipy.ndimage.label per class" if ndimage is not None else "download + numpy definition",
                "host_us_per_frame": round(hus, 1), "host_us_range": [round(min(host), 1), round(max(host), 1)],
                "components_over_host": round(us / hus, 5)})
    return res


def online(a):
    (H, W), classes = (1024, 1280), 12
    model, name = endovis_model(a.seed, classes)
    n = 16
    frames = noisy_frames(np.random.default_rng(a.seed), n, H, W)
    paths = {"none": None, "instances": K}
    res = {"model": name, "frame": [H, W], "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows, "max_instances": K}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {p: video.VideoSegmenter(model, graph=True, out="labels", out_size=(H, W), report="deferred", instances=k)
                for p, k in paths.items()}
        fps = take_turns(segs, lambda p, k: segs[p].push(frames[k % n]), a.frames, a.online_windows)
        t0 = time.perf_counter()
        rep = segs["instances"].instance_report()
        res["instance_report_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res.update(fps)
    res["reported_frames"] = len(rep)
    res["total_per_frame"] = [int(rep.total.min()), int(np.median(rep.total)), int(rep.total.max())] if len(rep) else [0, 0, 0]
    res["instances_over_none"] = round(res["instances_frames_per_s"] / res["none_frames_per_s"], 4)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_components_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_components.py measures on the GPU: no device found")
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
