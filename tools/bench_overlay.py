#!/usr/bin/env python3
"""Cost of the colour overlay (stswin_labels_overlay, VideoSegmenter(out="overlay")) at 1024x1280 (EndoVis18 frames) and 540x960
(CaDIS frames), one frame per launch, labels of 12 / 9 classes in blobs, outlines on:

  kernel_us_per_frame    device events around replays of a captured hipGraph that holds one launch of hip.labels_overlay per set of
                         (labels, frame, out) buffers, `buffer_sets` sets, together larger than the 256 MB last-level cache, so that
                         every operand comes from HBM and no host call sits between two launches (the Python call alone takes longer
                         than the kernel); >= `--reps` launches per window, the median of `--windows` windows, min and max in
                         kernel_us_range.  It is the period of back-to-back launches, an upper bound of the kernel's own time.
                         kernel_GB_per_s = the 7 bytes per pixel the kernel has to move over that time
  torch_us_per_frame     the same bytes (checked with torch.equal before timing) from a plain torch formulation on the same buffers
                         in the same run, captured and replayed the same way: palette gather, neighbour compares, integer blend.  The
                         single-pass kernel must be faster than this multi-pass formulation: otherwise the tool prints FAIL and exits
                         non-zero
  online_graph           frames/s of VideoSegmenter(graph=True) with out="overlay" against out="labels", same process, same
                         GPU-resident frames, bf16 autocast, one frame per push, push -> synchronise; the two segmenters take turns in
                         windows of `--frames` frames, the median window of each is reported

    python tools/bench_overlay.py [--reps 500] [--windows 7] [--frames 64]      -> one JSON line, also written to profiles/bench_overlay_line.json
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
from stswincl_amd.utils.visualize import default_palette, overlay_table  # noqa: E402

SIZES = {"endovis18": ((1024, 1280), 12), "cadis": ((540, 960), 9)}
COLD_BYTES = 320 << 20          # more than the 256 MB last-level cache


def blob_labels(gen, n, H, W, classes):
    """Labels as a segmenter gives them: a coarse random class map, enlarged (regions of ~32 pixels with straight outlines)."""
    coarse = gen.integers(0, classes, (n, -(-H // 32), -(-W // 32))).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, 32, 1), 32, 2)[:, :H, :W])


def torch_overlay(labels, table_i32, frames, edge_alpha):
    """stswin_labels_overlay in plain torch ops (int32 arithmetic)."""
    entry = table_i32[labels.long()]                                        # palette gather [n][H][W][4]
    alpha = entry[..., 3]
    if edge_alpha is not None:
        edge = torch.zeros_like(labels, dtype=torch.bool)
        d = labels[:, :, 1:] != labels[:, :, :-1]
        edge[:, :, 1:] |= d
        edge[:, :, :-1] |= d
        d = labels[:, 1:] != labels[:, :-1]
        edge[:, 1:] |= d
        edge[:, :-1] |= d
        alpha = torch.where(edge, edge_alpha, alpha)
    alpha = alpha[..., None]
    v = alpha * entry[..., :3] + (255 - alpha) * frames.int() + 127
    return torch.div(v, 255, rounding_mode="floor").to(torch.uint8)


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


def launch_cost(protocol, a):
    (H, W), classes = SIZES[protocol]
    gen = np.random.default_rng(a.seed)
    per_set = H * W * 7
    sets = max(2, -(-COLD_BYTES // per_set))
    labels = torch.from_numpy(blob_labels(gen, sets, H, W, classes)).cuda()
    frames = torch.from_numpy(gen.integers(0, 256, (sets, H, W, 3), dtype=np.uint8)).cuda()
    outs = torch.empty(sets, H, W, 3, dtype=torch.uint8, device="cuda")
    table = torch.from_numpy(overlay_table(default_palette(), 128, (0,))).cuda()
    table_i32 = table.int()
    edge = 255
    for i in (0, sets - 1):
        got = hip.labels_overlay(labels[i:i + 1], table, frames[i:i + 1], edge, outs[i:i + 1])
        if not torch.equal(got, torch_overlay(labels[i:i + 1], table_i32, frames[i:i + 1], edge)):
            raise SystemExit(f"FAIL: the kernel and the torch formulation give different bytes at {H}x{W}")

    def kernel(k):
        hip.labels_overlay(labels[k:k + 1], table, frames[k:k + 1], edge, outs[k:k + 1])

    def plain(k):
        outs[k:k + 1].copy_(torch_overlay(labels[k:k + 1], table_i32, frames[k:k + 1], edge))

    kw = _windows(kernel, sets, a.reps, a.windows)
    tw = _windows(plain, sets, max(a.reps // 5, sets), a.windows)
    kus, tus = float(np.median(kw)), float(np.median(tw))
    return {"frame": [H, W], "buffer_sets": sets, "buffer_bytes": sets * per_set, "edge_alpha": edge, "kernel_us_per_frame": round(kus, 2),
            "kernel_us_range": [round(min(kw), 2), round(max(kw), 2)], "kernel_GB_per_s": round(per_set / kus / 1e3, 1),
            "torch_us_per_frame": round(tus, 2), "torch_us_range": [round(min(tw), 2), round(max(tw), 2)],
            "torch_over_kernel": round(tus / kus, 1), "kernel_faster": bool(kus < tus)}


def online(protocol, a):
    (H, W), classes = SIZES[protocol]
    torch.manual_seed(a.seed)
    if protocol == "cadis":
        from stswincl_amd.net.Ours.base_cata_np import TswinPlusv5
        model, name = TswinPlusv5(classes).cuda().eval(), f"base_cata_np.TswinPlusv5({classes})"
    else:
        model, name = endovis_model(a.seed, classes)
    n = 16
    frames = noisy_frames(np.random.default_rng(a.seed), n, H, W)
    res = {"model": name, "frame": [H, W], "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {out: video.VideoSegmenter(model, graph=True, out=out, out_size=(H, W), protocol=protocol) for out in ("labels", "overlay")}
        res.update(take_turns(segs, lambda out, k: segs[out].push(frames[k % n]), a.frames, a.online_windows, protocol))
    res["overlay_over_labels"] = round(res["overlay_frames_per_s"] / res["labels_frames_per_s"], 4)
    res["overlay_extra_us_per_frame"] = round(1e6 / res["overlay_frames_per_s"] - 1e6 / res["labels_frames_per_s"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--frames", type=int, default=64, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_overlay_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlay.py measures on the GPU: no device found")
    res = {"launch": {p: launch_cost(p, a) for p in SIZES}}
    torch.cuda.empty_cache()
    if not a.no_online:
        res["online_graph"] = {p: online(p, a) for p in SIZES}
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    slow = [p for p, r in res["launch"].items() if not r["kernel_faster"]]
    if slow:
        raise SystemExit(f"FAIL: the single-pass kernel is not faster than the multi-pass torch formulation at {slow}")


if __name__ == "__main__":
    main()
