#!/usr/bin/env python3
"""Cost of cleaning the label map (stswin_labels_clean, stswin_labels_score, VideoSegmenter(clean_area=A)), one run on one MI355X:

  launch         per frame size - 540x960 and 1024x1280 - the launches of hip.labels_clean (12 classes, clean_area = 64, the defaults
                 otherwise) alone, one frame per call, on the label maps of a real forward pass: the random-weight model of the other
                 video tools segments noisy frames and its labels, `distinct` maps, are repeated into `buffer_sets` frames, together
                 larger than the 256 MB last-level cache.  Measured as tools/bench_parts.py measures its launch: device events around
                 replays of a captured hipGraph that holds one call per buffer set.  Beside it, from the same run and on the same maps,
                 the launches of hip.label_components (K = 64) and hip.instance_parts on its component map: the cost the chain already
                 pays for the same union-find and the same border walk; `clean_over_components` is the ratio
  host           the same maps the way a pipeline without the kernel would start: download one map, scipy.ndimage.label per class and
                 the areas by bincount - without the relabelling, so a lower bound of the host route - wall clock per frame
  score          hip.labels_score (counts) on existing labels against the fused route it replaces when the labels are cleaned first:
                 hip.upsample_argmax with gt, and without gt (what still runs in front of the cleaning)
  online         frames/s of VideoSegmenter(out="labels", report="deferred", instances=16), bf16 autocast, GPU-resident 1024x1280
                 frames, one frame per push, push -> synchronise, without and with clean_area, eager and graph=True, taking turns in
                 windows of `--frames` frames; the median window of each with its range

    python tools/bench_clean.py [--reps 200] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_clean_line.json
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

from bench_confidence import _spread  # noqa: E402
from bench_instruments import COLD_BYTES, DISTINCT, _windows  # noqa: E402
from online_loop import endovis_model, noisy_frames  # noqa: E402
from stswincl_amd import hip, video  # noqa: E402

try:
    from scipy import ndimage
except ImportError:          # the host yardstick is optional
    ndimage = None

CLASSES = 12
K = 64
AREA = 64
SIZES = {"540x960": (540, 960), "1024x1280": (1024, 1280)}


def model_labels(model, frames, size):
    """The label maps [n][*size] of a forward pass over `frames`, and the logits they were made from."""
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        labels = video.VideoSegmenter(model, out="labels", out_size=size).segment_sequence(frames)
        logits = video.VideoSegmenter(model, out="logits").segment_sequence(frames)
    return torch.stack(labels).contiguous(), torch.stack(logits).contiguous()


def host_route(labels_dev, nc, area):
    """Download one label map [H][W], label it per class on the host and take the areas -> the number of components below `area`."""
    lab = labels_dev.cpu().numpy()
    small = 0
    for c in range(nc):
        comp, k = ndimage.label(lab == c, np.ones((3, 3), dtype=int))
        if k:
            small += int((np.bincount(comp.ravel(), minlength=k + 1)[1:] < area).sum())
    return small


def launch_cost(model, frames, a):
    res = {"classes": CLASSES, "clean_area": AREA, "connectivity": 8, "max_small": 4096, "instances": K,
           "maps": "labels of a forward pass of the random-weight model over noisy frames"}
    for name, (H, W) in SIZES.items():
        sets = max(2, -(-COLD_BYTES // (2 * H * W)))
        distinct, logits = model_labels(model, frames, (H, W))
        lab = distinct.repeat(-(-sets // distinct.shape[0]), 1, 1)[:sets].contiguous()
        out = torch.empty(1, H, W, dtype=torch.uint8, device="cuda")
        ws = torch.empty(hip.labels_clean_scratch(1, H, W, CLASSES), dtype=torch.uint8, device="cuda")
        cc_out = (torch.empty(1, H, W, dtype=torch.int32, device="cuda"), torch.empty(1, K, 12, dtype=torch.int64, device="cuda"),
                  torch.empty(1, dtype=torch.int32, device="cuda"))
        cc_ws = torch.empty(hip.label_components_scratch(1, H, W), dtype=torch.uint8, device="cuda")
        ip_out = (torch.empty(1, K, CLASSES, 10, dtype=torch.int64, device="cuda"), torch.empty(1, K, CLASSES, dtype=torch.int64, device="cuda"))
        stats = hip.labels_clean(distinct, CLASSES, AREA)[1].cpu().numpy()
        clean = lambda i: hip.labels_clean(lab[i:i + 1], CLASSES, AREA, out=out, workspace=ws)                          # noqa: E731
        comps = lambda i: hip.label_components(lab[i:i + 1], CLASSES, 8, (0,), K, out=cc_out, workspace=cc_ws)         # noqa: E731
        parts = lambda i: hip.instance_parts(lab[i:i + 1], cc_out[0], K, CLASSES, out=ip_out)                           # noqa: E731
        r = {"frame": [H, W], "buffer_sets": sets, "distinct": int(distinct.shape[0]),
             "small_components_per_frame": [int(stats[:, 0].min()), int(np.median(stats[:, 0])), int(stats[:, 0].max())],
             "changed_pixels_per_frame": [int(stats[:, 1].min()), int(np.median(stats[:, 1])), int(stats[:, 1].max())]}
        r["clean_us"], r["clean_us_range"] = _spread(_windows(clean, sets, a.reps, a.windows))
        r["components_us"], r["components_us_range"] = _spread(_windows(comps, sets, a.reps, a.windows))
        r["parts_us"], r["parts_us_range"] = _spread(_windows(parts, sets, a.reps, a.windows))
        r["clean_over_components"] = round(r["clean_us"] / r["components_us"], 4)
        if ndimage is not None:
            t = []
            for i in range(min(a.host_frames, distinct.shape[0])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_route(distinct[i], CLASSES, AREA)
                t.append((time.perf_counter() - t0) * 1e6)
            r["host_scipy_us"], r["host_scipy_us_range"] = _spread(t)
            r["host_over_clean"] = round(r["host_scipy_us"] / r["clean_us"], 1)
        # the score launch on existing labels against the fused label + count launch, and the label launch that stays
        n = logits.shape[0]
        gt = torch.randint(0, CLASSES, (n, 1, H, W), device="cuda")
        labels1 = [distinct[i:i + 1] for i in range(n)]
        counts = torch.zeros(1, 3, CLASSES, dtype=torch.int32, device="cuda")
        r["score_us"], r["score_us_range"] = _spread(_windows(lambda i: hip.labels_score(labels1[i], gt[i], CLASSES, counts=counts), n, a.reps, a.windows))
        r["argmax_gt_us"], r["argmax_gt_us_range"] = _spread(_windows(lambda i: hip.upsample_argmax(logits[i:i + 1], H, W, gt[i]), n, a.reps, a.windows))
        r["argmax_us"], r["argmax_us_range"] = _spread(_windows(lambda i: hip.upsample_argmax(logits[i:i + 1], H, W), n, a.reps, a.windows))
        r["score_note"] = f"{n} frames in turn: these maps stay in the last-level cache"
        res[name] = r
        del lab, distinct, logits, gt
        torch.cuda.empty_cache()
    return res


def _turns(segs, frames, per_window, windows, rule="endovis18"):
    """tools/online_loop.take_turns for segmenters of either mode: path -> VideoSegmenter; every path first runs its eager steps (and a
    few more: a graph's capture and first replays), then the paths take turns in `windows` windows of `per_window` one-frame pushes."""
    n = frames.shape[0]
    pushed = {p: 0 for p in segs}
    fps = {p: [] for p in segs}

    def run(p, count):
        for _ in range(count):
            segs[p].push(frames[pushed[p] % n])
            pushed[p] += 1
            torch.cuda.synchronize()

    for p in segs:
        run(p, video.min_frames(rule) + 4)
    for _ in range(windows):
        for p in segs:
            t0 = time.perf_counter()
            run(p, per_window)
            fps[p].append(per_window / (time.perf_counter() - t0))
    res = {}
    for p, seg in segs.items():
        assert seg.captured == seg.graph, p
        res[f"{p}_frames_per_s"] = round(float(np.median(fps[p])), 2)
        res[f"{p}_frames_per_s_range"] = [round(min(fps[p]), 2), round(max(fps[p]), 2)]
    return res


def online(model, name, frames, a):
    size = SIZES["1024x1280"]
    res = {"model": name, "frame": list(size), "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows, "instances": 16}
    kw = dict(out="labels", out_size=size, report="deferred", instances=16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {f"{mode}_{path}": video.VideoSegmenter(model, graph=mode == "graph", **kw, **more)
                for mode in ("eager", "graph") for path, more in (("plain", {}), ("clean", dict(clean_area=AREA)))}
        res.update(_turns(segs, frames, a.frames, a.online_windows))
        rep = segs["graph_clean"].clean_report()
    res["reported_frames"] = len(rep)
    res["changed_pixels_median"] = int(np.median(rep.changed))
    for mode in ("eager", "graph"):
        res[f"{mode}_clean_over_plain"] = round(res[f"{mode}_clean_frames_per_s"] / res[f"{mode}_plain_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--frames", type=int, default=48, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=4, help="maps timed on the host route")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_clean_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clean.py measures on the GPU: no device found")
    model, name = endovis_model(a.seed, CLASSES)
    frames = noisy_frames(np.random.default_rng(a.seed), DISTINCT, *SIZES["1024x1280"])
    res = {"launch": launch_cost(model, frames, a)}
    torch.cuda.empty_cache()
    if not a.no_online:
        res["online"] = online(model, name, frames, a)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
