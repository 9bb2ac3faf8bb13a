#!/usr/bin/env python3
"""Cost of ground truth in its stored form (stswin_gt_decode, VideoSegmenter(gt_table=..., scores="deferred")):

  launch         the decode launch alone, one frame per launch: 1024x1280 RGBA under 12 colours (EndoVis18 test labels) and 540x960
                 raw ids (CaDIS), each to uint8 and to int64.  Device events around replays of a captured hipGraph that holds one
                 launch of hip.gt_decode per (in, out) buffer set, `buffer_sets` sets, together larger than the 256 MB last-level
                 cache, so that every operand comes from HBM and no host call sits between two launches; >= `--reps` launches per
                 window, the median of `--windows` windows, min and max in us_range.  It is the period of back-to-back launches, an
                 upper bound of the kernel's own time.  bytes_per_frame = what the kernel has to move (stored bytes in, indices out),
                 TB_per_s = that over the period.  The result of the first and the last set is compared with
                 utils.groundtruth.decode_colours / decode_ids before timing
  evaluation     EndoVis18 evaluation frames/s with ground truth on every frame: VideoSegmenter(graph=True, out="labels"), bf16
                 autocast, GPU-resident frames, ground truth as RGBA pictures in host memory (where a PNG decoder leaves them), one
                 frame per push, push -> synchronise.  Three segmenters take turns in windows of `--frames` frames within one run,
                 the median window of each is reported with its range:
                   host_int64_frame   today's path: utils.groundtruth.decode_colours on the host, the int64 index map uploaded,
                                      scores="frame" (a download and a synchronise per scored frame)
                   stored_deferred    gt_table + scores="deferred": the RGBA bytes uploaded, decoded and counted on the device, the
                                      score log downloaded once at the end (endo_scores_ms)
                   no_gt              the same segmenter without ground truth: the ceiling
                 The per-frame Dice / IoU lists of the two scored paths must be equal, and stored_deferred must not be slower than
                 host_int64_frame: otherwise the tool prints FAIL and exits non-zero.

    python tools/bench_gt_decode.py [--reps 500] [--windows 7] [--frames 48]     -> one JSON line, also written to profiles/bench_gt_decode_line.json
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
from stswincl_amd.utils import groundtruth  # noqa: E402
from stswincl_amd.utils.visualize import default_palette  # noqa: E402

CASES = {"endovis18_rgba": ((1024, 1280), 4), "cadis_ids": ((540, 960), 1)}
COLOURS = 12
COLD_BYTES = 320 << 20          # more than the 256 MB last-level cache


def blob_labels(gen, n, H, W, classes):
    """Ground truth as it looks: a coarse random class map, enlarged (regions of ~32 pixels)."""
    coarse = gen.integers(0, classes, (n, -(-H // 32), -(-W // 32))).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, 32, 1), 32, 2)[:, :H, :W])


def rgba_pictures(gen, labels):
    """labels [n][H][W] -> the RGBA pictures a colour-coded label file decodes to (opaque alpha)."""
    rgb = default_palette()[:COLOURS][labels]
    return np.ascontiguousarray(np.concatenate([rgb, np.full(labels.shape + (1,), 255, np.uint8)], axis=-1))


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


def launch_cost(case, dtype, a):
    (H, W), ch = CASES[case]
    gen = np.random.default_rng(a.seed)
    out_bytes = 8 if dtype == torch.int64 else 1
    per_set = H * W * (ch + out_bytes)
    sets = max(2, -(-COLD_BYTES // per_set))
    if ch == 1:
        raw = gen.integers(0, 36, (sets, H, W), dtype=np.uint8)
        raw[gen.random((sets, H, W)) < 0.05] = 255
        host, table = raw, groundtruth.remap_table({c: c % 8 for c in range(36)}, ignore_to=8)
        want = lambda i: groundtruth.decode_ids(host[i], table)
    else:
        host, table = rgba_pictures(gen, blob_labels(gen, sets, H, W, COLOURS)), groundtruth.colour_table(default_palette()[:COLOURS])
        want = lambda i: groundtruth.decode_colours(host[i], table)[0]
    src, tab = torch.from_numpy(host).cuda(), torch.from_numpy(table).cuda()
    outs = torch.empty(sets, H, W, dtype=dtype, device="cuda")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    unmatched = counts if ch != 1 else None
    for i in (0, sets - 1):
        got = hip.gt_decode(src[i:i + 1], tab, dtype, unmatched, outs[i:i + 1])
        if not torch.equal(got[0].cpu(), torch.from_numpy(want(i)).to(dtype)) or int(counts.item()) != 0:
            raise SystemExit(f"FAIL: the kernel and the numpy statement differ at {case} -> {dtype}")

    def kernel(k):
        hip.gt_decode(src[k:k + 1], tab, dtype, unmatched, outs[k:k + 1])

    w = _windows(kernel, sets, a.reps, a.windows)
    us = float(np.median(w))
    return {"frame": [H, W], "channels": ch, "out": str(dtype).replace("torch.", ""), "buffer_sets": sets, "buffer_bytes": sets * per_set,
            "bytes_per_frame": per_set, "us_per_frame": round(us, 2), "us_range": [round(min(w), 2), round(max(w), 2)],
            "TB_per_s": round(per_set / us / 1e6, 3)}


def evaluation(a):
    (H, W), classes = (1024, 1280), COLOURS
    model, name = endovis_model(a.seed, classes)
    gen = np.random.default_rng(a.seed)
    n = 16
    frames = noisy_frames(gen, n, H, W)
    stored = rgba_pictures(gen, blob_labels(gen, n, H, W, classes))            # host memory: what a PNG decoder hands over
    table = groundtruth.colour_table(default_palette()[:COLOURS])
    res = {"model": name, "frame": [H, W], "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows,
           "gt_bytes_uploaded_per_frame": {"host_int64_frame": H * W * 8, "stored_deferred": H * W * 4}}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        kw = dict(graph=True, out="labels", out_size=(H, W))
        segs = {"host_int64_frame": video.VideoSegmenter(model, **kw),
                "stored_deferred": video.VideoSegmenter(model, gt_table=table, scores="deferred", **kw),
                "no_gt": video.VideoSegmenter(model, **kw)}
        frame_scores = {}                                    # host_int64_frame: frame index -> (dice list, iou list)

        def push(p, k):
            k %= n
            if p == "host_int64_frame":
                gt = torch.from_numpy(groundtruth.decode_colours(stored[k], table)[0].astype(np.int64))
                for f, (_, dice, iou) in segs[p].push(frames[k], gt=gt):
                    frame_scores[f] = (dice, iou)
            elif p == "stored_deferred":
                segs[p].push(frames[k], gt=stored[k])
            else:
                segs[p].push(frames[k])

        fps = take_turns(segs, push, a.frames, a.online_windows)
        t0 = time.perf_counter()
        scores = segs["stored_deferred"].endo_scores()
        res["endo_scores_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res.update(fps)
    same = scores.frames == sorted(frame_scores) and all(scores.dices[r] == frame_scores[f][0] and scores.ious[r] == frame_scores[f][1]
                                                          for r, f in enumerate(scores.frames))
    res["scored_frames"] = scores.count
    res["dice"], res["iou"] = round(float(scores.dice), 6), round(float(scores.iou), 6)
    res["unmatched"] = segs["stored_deferred"].unmatched()
    res["scores_equal"] = bool(same)
    res["stored_over_host"] = round(res["stored_deferred_frames_per_s"] / res["host_int64_frame_frames_per_s"], 4)
    res["stored_over_no_gt"] = round(res["stored_deferred_frames_per_s"] / res["no_gt_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--frames", type=int, default=48, help="frames per evaluation window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-evaluation", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_gt_decode_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gt_decode.py measures on the GPU: no device found")
    res = {"launch": []}
    for case in CASES:
        for dtype in (torch.uint8, torch.int64):
            res["launch"].append(dict(case=case, **launch_cost(case, dtype, a)))
            torch.cuda.empty_cache()
    if not a.no_evaluation:
        res["evaluation"] = evaluation(a)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    if not a.no_evaluation:
        ev = res["evaluation"]
        if not ev["scores_equal"]:
            raise SystemExit("FAIL: scores='deferred' and scores='frame' give different per-frame lists")
        if ev["stored_deferred_frames_per_s"] < ev["host_int64_frame_frames_per_s"]:
            raise SystemExit("FAIL: gt_table + scores='deferred' is slower than the host decode + int64 upload + scores='frame'")


if __name__ == "__main__":
    main()
