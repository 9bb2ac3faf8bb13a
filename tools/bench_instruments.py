#!/usr/bin/env python3
"""Cost of the per-frame instrument report (stswin_label_moments, VideoSegmenter(report=...)):

  launch         the moments launch alone, one frame per launch: 1024x1280 with 12 classes (EndoVis18) and 540x960 with 26 classes
                 (CaDIS).  Device events around replays of a captured hipGraph that holds one launch of hip.label_moments per
                 (labels, out) buffer set, `buffer_sets` sets, together larger than the 256 MB last-level cache, so that every label
                 map comes from HBM and no host call sits between two launches; >= `--reps` launches per window, the median of
                 `--windows` windows, min and max in us_range.  It is the period of back-to-back launches, an upper bound of the
                 kernel's own time.  bytes_per_frame = the label map, TB_per_s = that over the period.  The label maps are synthetic
                 (background with a few bars and discs, 16 distinct frames repeated over the sets): no checkpoint ships with the
                 package.  The result of the first and the last set is compared with utils.instruments.label_moments before timing
  torch          the same ten statistics by the torch formulation a user would write without the kernel - per class a mask, masked
                 sums over index grids, masked amax for the extent - on the same label maps, timed the same way over `--torch-sets`
                 sets (it reads the map and the grids some 15 times per class, so the last-level cache is its friend); its result is
                 compared with the kernel's before timing.  kernel_over_torch = launch us / torch us
  online         frames/s of VideoSegmenter(graph=True, out="labels"), bf16 autocast, GPU-resident 1024x1280 frames, one frame per
                 push, push -> synchronise, with report=None, "frame" and "deferred".  The three segmenters take turns in windows of
                 `--frames` frames within one run; the median window of each is reported with its range, deferred_over_none and
                 frame_over_none beside them, and the time of the one instrument_report() download at the end.  The deferred rows must
                 equal the moments of report="frame": otherwise the tool prints FAIL and exits non-zero.

    python tools/bench_instruments.py [--reps 500] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_instruments_line.json
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

from online_loop import endovis_model, noisy_frames, take_turns  # noqa: E402
from stswincl_amd import hip, video  # noqa: E402
from stswincl_amd.utils import instruments  # noqa: E402

CASES = {"endovis18": ((1024, 1280), 12), "cadis": ((540, 960), 26)}
COLD_BYTES = 320 << 20          # more than the 256 MB last-level cache
DISTINCT = 16


def instrument_maps(gen, n, H, W, classes):
    """Label maps as a segmenter writes them: background 0, per frame a few thick bars that enter from the border (shafts) and discs."""
    ys, xs = np.mgrid[:H, :W].astype(np.float32)
    lab = np.zeros((n, H, W), np.uint8)
    for f in range(n):
        for _ in range(int(gen.integers(2, 5))):
            c = int(gen.integers(1, classes))
            x0, y0 = (float(gen.uniform(0, W)), float(gen.choice([0, H - 1]))) if gen.random() < 0.5 else (float(gen.choice([0, W - 1])), float(gen.uniform(0, H)))
            x1, y1 = float(gen.uniform(0.3 * W, 0.7 * W)), float(gen.uniform(0.3 * H, 0.7 * H))
            dx, dy = x1 - x0, y1 - y0
            t = np.clip(((xs - x0) * dx + (ys - y0) * dy) / (dx * dx + dy * dy), 0, 1)
            d2 = (xs - (x0 + t * dx)) ** 2 + (ys - (y0 + t * dy)) ** 2
            lab[f][d2 <= float(gen.uniform(0.02, 0.05) * H) ** 2] = c
            lab[f][(xs - x1) ** 2 + (ys - y1) ** 2 <= float(gen.uniform(0.03, 0.07) * H) ** 2] = int(gen.integers(1, classes))
    return lab


def _windows(fn, sets, reps, windows):
    """us per call of fn(k), k cycling over the buffer sets: one cycle captured into a graph, replayed."""
    sync = torch.cuda.synchronize
    for k in range(min(sets, 8)):
        fn(k)
    sync()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(sets):
            fn(k)
    replays = max(1, -(-reps // sets))
    graph.replay()
    sync()
    res = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        sync()
        res.append(e0.elapsed_time(e1) * 1e3 / (replays * sets))
    return res


def torch_moments(labels, nc, xs, ys):
    """The row of utils.instruments.label_moments in torch ops, per class: labels uint8 [H][W], xs / ys int64 index grids."""
    H, W = labels.shape
    rows = []
    for c in range(nc):
        m = labels == c
        mi = m.to(torch.int64)
        x, y = xs * mi, ys * mi
        zero = torch.zeros((), dtype=torch.int64, device=labels.device)
        rows.append(torch.stack([mi.sum(), x.sum(), y.sum(), (x * xs).sum(), (x * ys).sum(), (y * ys).sum(),
                                 torch.where(m, W - xs, zero).amax(), torch.where(m, H - ys, zero).amax(),
                                 torch.where(m, xs + 1, zero).amax(), torch.where(m, ys + 1, zero).amax()]))
    return torch.stack(rows)


def launch_cost(case, a):
    (H, W), nc = CASES[case]
    gen = np.random.default_rng(a.seed)
    per_set = H * W
    sets = max(2, -(-COLD_BYTES // per_set))
    distinct = instrument_maps(gen, DISTINCT, H, W, nc)
    labels = torch.from_numpy(distinct).cuda().repeat(-(-sets // DISTINCT), 1, 1)[:sets].contiguous()
    outs = torch.zeros(sets, nc, 10, dtype=torch.int64, device="cuda")
    for i in (0, sets - 1):
        got = hip.label_moments(labels[i:i + 1], nc)
        if not torch.equal(got.cpu(), torch.from_numpy(instruments.label_moments(distinct[i % DISTINCT], nc))):
            raise SystemExit(f"FAIL: the kernel and the numpy statement differ at {case}")

    def kernel(k):
        hip.label_moments(labels[k:k + 1], nc, out=outs[k:k + 1])     # (accumulates: the contract; nobody reads outs)

    w = _windows(kernel, sets, a.reps, a.windows)
    us = float(np.median(w))
    res = {"frame": [H, W], "classes": nc, "classes_present": int((got[0, :, 0] > 0).sum()), "labels": "synthetic bars and discs",
           "buffer_sets": sets, "buffer_bytes": sets * per_set, "bytes_per_frame": per_set, "us_per_frame": round(us, 2),
           "us_range": [round(min(w), 2), round(max(w), 2)], "TB_per_s": round(per_set / us / 1e6, 3)}
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    tsets = min(sets, a.torch_sets)
    if not torch.equal(torch_moments(labels[0], nc, xs, ys), hip.label_moments(labels[:1], nc)[0]):
        raise SystemExit(f"FAIL: the torch formulation and the kernel differ at {case}")
    sink = torch.zeros(tsets, nc, 10, dtype=torch.int64, device="cuda")

    def baseline(k):
        sink[k].copy_(torch_moments(labels[k], nc, xs, ys))

    w = _windows(baseline, tsets, tsets, max(3, a.windows // 2))
    tus = float(np.median(w))
    res.update({"torch_us_per_frame": round(tus, 1), "torch_us_range": [round(min(w), 1), round(max(w), 1)], "torch_buffer_sets": tsets,
                "kernel_over_torch": round(us / tus, 5)})
    return res


def online(a):
    (H, W), classes = (1024, 1280), 12
    model, name = endovis_model(a.seed, classes)
    n = 16
    frames = noisy_frames(np.random.default_rng(a.seed), n, H, W)
    paths = ("none", "frame", "deferred")
    res = {"model": name, "frame": [H, W], "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {p: video.VideoSegmenter(model, graph=True, out="labels", out_size=(H, W), report=None if p == "none" else p) for p in paths}
        frame_moments = {}

        def push(p, k):
            out = segs[p].push(frames[k % n])
            if p == "frame":
                for f, (_, mom) in out:
                    frame_moments[f] = mom.clone()                       # stays on the device: no download in the timed loop

        fps = take_turns(segs, push, a.frames, a.online_windows)
        t0 = time.perf_counter()
        rep = segs["deferred"].instrument_report()
        res["instrument_report_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res.update(fps)
    same = rep.frames == sorted(frame_moments) and all(np.array_equal(rep.moments[r], frame_moments[f].cpu().numpy())
                                                       for r, f in enumerate(rep.frames))
    res["reported_frames"] = len(rep)
    res["classes_present_per_frame"] = round(float(rep.presence().sum(1).mean()), 2) if len(rep) else 0.0
    res["reports_equal"] = bool(same)
    res["deferred_over_none"] = round(res["deferred_frames_per_s"] / res["none_frames_per_s"], 4)
    res["frame_over_none"] = round(res["frame_frames_per_s"] / res["none_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--torch-sets", type=int, default=8, help="buffer sets (and calls per window) of the torch formulation")
    ap.add_argument("--frames", type=int, default=48, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_instruments_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instruments.py measures on the GPU: no device found")
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
    if not a.no_online and not res["online"]["reports_equal"]:
        raise SystemExit("FAIL: report='deferred' and report='frame' give different moments")


if __name__ == "__main__":
    main()
