#!/usr/bin/env python3
"""Cost of frames in the form a video source delivers them (stswin_yuv_to_rgb, stswin_rgb_to_nv12,
VideoSegmenter(pixel_format="nv12" | "uyvy", out_format="nv12")):

  launch         each launch alone, one frame per launch, at 1024x1280 and 540x960: nv12 replicate, nv12 linear, uyvy replicate and
                 rgb -> nv12.  Device events around replays of a captured hipGraph that holds one launch per (in, out) buffer set,
                 `buffer_sets` sets, together larger than the 256 MB last-level cache, so that every operand comes from HBM and no
                 host call sits between two launches; >= `--reps` launches per window, the median of `--windows` windows, min and max
                 in us_range.  It is the period of back-to-back launches, an upper bound of the kernel's own time.  bytes_per_frame =
                 what the kernel has to move (raw bytes in, RGB out, or the reverse), TB_per_s = that over the period.  The result of
                 the first and the last set is compared with utils.yuv before timing
  online         VideoSegmenter(graph=True, out="labels"), bf16 autocast, frames in host memory (where a decoder or a capture card
                 leaves them), one frame per push, push -> synchronise.  pixel_format "rgb" (today's path: the host has converted, 3
                 bytes per pixel go up), "nv12" (1.5) and "uyvy" (2) show the same pictures; the three segmenters take turns in
                 windows of `--frames` frames within one run, the median window of each is reported with its range
  overlay        the same for out="overlay" on GPU-resident RGB frames: out_format "rgb" against "nv12"

A raw-format run must not be slower than the rgb run of the same session by more than the spread between the rgb run's own windows
(max - min): otherwise the tool prints FAIL and exits non-zero.

    python tools/bench_yuv.py [--reps 500] [--windows 7] [--frames 48]     -> one JSON line, also written to profiles/bench_yuv_line.json
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

from online_loop import endovis_model, take_turns  # noqa: E402
from stswincl_amd import hip, video  # noqa: E402
from stswincl_amd.utils import yuv  # noqa: E402

SIZES = ((1024, 1280), (540, 960))
CASES = (("nv12", "replicate"), ("nv12", "linear"), ("uyvy", "replicate"), ("rgb_to_nv12", None))
COLD_BYTES = 320 << 20          # more than the 256 MB last-level cache


def raw_shape(fmt, n, H, W):
    return (n, H * 3 // 2, W) if fmt == "nv12" else (n, H, W, 2)


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


def launch_cost(size, fmt, chroma, a):
    H, W = size
    gen = np.random.default_rng(a.seed)
    raw_bytes = H * W * (3 if fmt == "nv12" or fmt == "rgb_to_nv12" else 4) // 2
    per_set = raw_bytes + 3 * H * W
    sets = max(2, -(-COLD_BYTES // per_set))
    if fmt == "rgb_to_nv12":
        m = yuv.to_yuv_matrix()
        host = gen.integers(0, 256, (sets, H, W, 3), dtype=np.uint8)
        outs = torch.empty(raw_shape("nv12", sets, H, W), dtype=torch.uint8, device="cuda")
        want = lambda i: yuv.rgb_to_nv12(host[i:i + 1], m)
        run = lambda k: hip.rgb_to_nv12(src[k:k + 1], mat, out=outs[k:k + 1])
    else:
        m = yuv.to_rgb_matrix()
        host = gen.integers(0, 256, raw_shape(fmt, sets, H, W), dtype=np.uint8)
        outs = torch.empty(sets, H, W, 3, dtype=torch.uint8, device="cuda")
        want = lambda i: yuv.yuv_to_rgb(host[i:i + 1], fmt, m, chroma)
        run = lambda k: hip.yuv_to_rgb(src[k:k + 1], mat, fmt, chroma, out=outs[k:k + 1])
    src, mat = torch.from_numpy(host).cuda(), torch.from_numpy(m).cuda()
    for i in (0, sets - 1):
        if not torch.equal(run(i).cpu(), torch.from_numpy(want(i))):
            raise SystemExit(f"FAIL: the kernel and the numpy statement differ at {fmt} {chroma} {H}x{W}")
    w = _windows(run, sets, a.reps, a.windows)
    us = float(np.median(w))
    return {"case": fmt if chroma is None else f"{fmt}_{chroma}", "frame": [H, W], "buffer_sets": sets, "buffer_bytes": sets * per_set,
            "bytes_per_frame": per_set, "us_per_frame": round(us, 2), "us_range": [round(min(w), 2), round(max(w), 2)],
            "TB_per_s": round(per_set / us / 1e6, 3)}


def _pictures(a, n, H, W):
    """The same n pictures as nv12, as uyvy (each chroma row twice) and as the RGB frames both convert to (replicate)."""
    gen = np.random.default_rng(a.seed)
    base = gen.integers(0, 256, raw_shape("nv12", 1, H, W), dtype=np.int64)
    nv12 = np.clip(base + gen.integers(-24, 25, raw_shape("nv12", n, H, W)), 0, 255).astype(np.uint8)
    uyvy = np.empty(raw_shape("uyvy", n, H, W), dtype=np.uint8)
    uyvy[..., 1] = nv12[:, :H]
    uyvy[..., 0] = np.repeat(nv12[:, H:], 2, axis=1)
    rgb = yuv.yuv_to_rgb(nv12, "nv12", yuv.to_rgb_matrix(), "replicate")
    assert np.array_equal(rgb, yuv.yuv_to_rgb(uyvy, "uyvy", yuv.to_rgb_matrix(), "replicate"))
    return {"rgb": rgb, "nv12": nv12, "uyvy": uyvy}


def _turns(segs, frames, a, name):
    """Every segmenter pushes its own form of the same pictures, one frame per push, push -> synchronise; windows take turns."""
    n = len(next(iter(frames.values())))
    last = {}

    def push(p, k):
        for f, r in segs[p].push(frames[p][k % n]):
            last[p] = (f, r)

    return take_turns(segs, push, a.frames, a.online_windows, prefix=name + "_"), last


def _criterion(res, name, base, others):
    lo, hi = res[f"{name}_{base}_frames_per_s_range"]
    ok = True
    for p in others:
        res[f"{name}_{p}_over_{base}"] = round(res[f"{name}_{p}_frames_per_s"] / res[f"{name}_{base}_frames_per_s"], 4)
        ok = ok and res[f"{name}_{p}_frames_per_s"] >= res[f"{name}_{base}_frames_per_s"] - (hi - lo)
    res[f"{name}_within_{base}_spread"] = bool(ok)
    return ok


def segmenter(a):
    (H, W), classes, n = (1024, 1280), 12, 16
    model, name = endovis_model(a.seed, classes)
    pics = _pictures(a, n, H, W)
    res = {"model": name, "frame": [H, W], "autocast": "bf16", "frames_per_window": a.frames,
           "windows": a.online_windows, "bytes_uploaded_per_frame": {"rgb": 3 * H * W, "nv12": H * W * 3 // 2, "uyvy": 2 * H * W}}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        kw = dict(graph=True, out="labels", out_size=(H, W))
        segs = {p: video.VideoSegmenter(model, pixel_format=p, **kw) for p in ("rgb", "nv12", "uyvy")}
        r, last = _turns(segs, pics, a, "online")
        res.update(r)
        same = all(last[p][0] == last["rgb"][0] and torch.equal(last[p][1], last["rgb"][1]) for p in ("nv12", "uyvy"))
        res["online_labels_equal"] = bool(same)
        del segs
        gpu = torch.from_numpy(pics["rgb"]).cuda()
        segs = {p: video.VideoSegmenter(model, graph=True, out="overlay", out_format=p) for p in ("rgb", "nv12")}
        r, last = _turns(segs, {"rgb": gpu, "nv12": gpu}, a, "overlay")
        res.update(r)
        want = yuv.rgb_to_nv12(last["rgb"][1].cpu().numpy()[None], yuv.to_yuv_matrix())[0]
        res["overlay_nv12_equal"] = bool(last["nv12"][0] == last["rgb"][0] and np.array_equal(last["nv12"][1].cpu().numpy(), want))
    ok = _criterion(res, "online", "rgb", ("nv12", "uyvy"))
    ok = _criterion(res, "overlay", "rgb", ("nv12",)) and ok
    return res, ok and res["online_labels_equal"] and res["overlay_nv12_equal"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--frames", type=int, default=48, help="frames per segmenter window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-segmenter", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_yuv_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv.py measures on the GPU: no device found")
    res = {"launch": []}
    for size in SIZES:
        for fmt, chroma in CASES:
            res["launch"].append(launch_cost(size, fmt, chroma, a))
            torch.cuda.empty_cache()
    ok = True
    if not a.no_segmenter:
        res["segmenter"], ok = segmenter(a)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    if not ok:
        raise SystemExit("FAIL: a raw-format run is slower than the rgb run by more than the rgb run's own spread, or its results differ")


if __name__ == "__main__":
    main()
