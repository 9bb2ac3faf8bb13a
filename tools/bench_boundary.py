#!/usr/bin/env python3
"""Cost of the boundary scores (stswin_boundary_counts, VideoSegmenter(boundary="deferred")), one run on one MI355X at 1024x1280:

  launch_blobs   the five launches of hip.boundary_counts alone (bins = 32, skip the background), one pair of maps per call: ground
                 truths of 8 classes as a segmenter's maps look (tools/bench_instruments.py instrument_maps) against the same maps
                 moved by (2, 3) pixels with every instrument of one class removed.  Measured as tools/bench_masks.py measures its
                 launches: device events around replays of a captured hipGraph that holds one call per pair of `buffer_sets` pairs,
                 together larger than the 256 MB last-level cache, so that a call's first read of its maps comes from HBM; one output
                 row and one workspace, as the segmenter has them.  The first and the last pair are compared with the host recipe
                 before timing
  launch_worst   the same call on the widest search there is: the ground truth a checkerboard of two classes, every pixel a contour
                 pixel, the prediction one pixel in the far corner, so that every query walks its whole row
  host           what the call replaces, on the same box: the label map's .cpu() (a synchronising download) plus the scipy recipe
                 (binary_erosion, distance_transform_edt per class and direction, the histogram), wall time per frame, the median of
                 `--host-frames` frames, for the blob maps and for the worst case
  evaluation     frames/s of VideoSegmenter(graph=True, out="labels", gt_table=..., scores="deferred"), bf16 autocast, GPU-resident
                 frames, stored RGBA ground truth from host memory, one frame per push, push -> synchronise, without (the parent's
                 path: the yardstick) and with boundary="deferred", taking turns in windows of `--frames` frames; the median window
                 of each with its range.  The ground truth is random regions and the seeded model is untrained: contours far from each
                 other, longer searches than a trained model's

Every step that uses the GPU runs in a child process of its own under its own time limit, and a step that fails ends the run.

    python tools/bench_boundary.py [--reps 100] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_boundary_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZE, CLASSES, BINS, SKIP = (1024, 1280), 8, 32, (0,)
STEPS = {"launch_blobs": 240, "launch_worst": 240, "evaluation": 420}          # seconds


def scipy_counts(gt, pred, nc, bins, skip):
    """The host recipe for one pair of maps [H][W] -> int32 [nc][2][2 + bins] (scipy: tools only)."""
    from scipy import ndimage
    out = np.zeros((nc, 2, 2 + bins), dtype=np.int32)
    for c in range(nc):
        if c in skip:
            continue
        edges = [m & ~ndimage.binary_erosion(m) for m in (gt == c, pred == c)]
        for d in range(2):
            own, other = edges[d], edges[1 - d]
            out[c, d, 0], out[c, d, 1] = own.sum(), -1
            if out[c, d, 0] and other.any():
                dist = ndimage.distance_transform_edt(~other)[own]
                d2 = np.rint(dist * dist).astype(np.int64)
                k = np.ceil(dist).astype(np.int64)
                k -= (k > 0) & ((k - 1) ** 2 >= d2)
                k += k * k < d2
                out[c, d, 1] = d2.max()
                out[c, d, 2:] = np.bincount(np.minimum(k, bins - 1), minlength=bins)
    return out


def _spread(w, digits=2):
    return round(float(np.median(w)), digits), [round(min(w), digits), round(max(w), digits)]


def launch(a, worst):
    import torch
    from bench_instruments import COLD_BYTES, _windows, instrument_maps
    from stswincl_amd import hip
    H, W = SIZE
    gen = np.random.default_rng(a.seed)
    if worst:
        sets = 2
        y, x = np.mgrid[:H, :W]
        gt = np.ascontiguousarray(np.broadcast_to((y + x) % 2, (sets, H, W)), dtype=np.int64)
        pred = np.zeros((sets, H, W), dtype=np.uint8)
        pred[:, H - 1, W - 1] = 1
        skip, what = (), "a checkerboard of two classes against one far pixel"
    else:
        sets = max(2, -(-COLD_BYTES // (H * W * 9)))
        lab = instrument_maps(gen, sets, H, W, CLASSES)
        pred = np.roll(lab, (2, 3), axis=(1, 2))
        pred[pred == CLASSES - 1] = 0
        gt, skip, what = lab.astype(np.int64), SKIP, f"instrument maps of {CLASSES} classes against themselves moved by (2, 3), one class removed"
    g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(np.ascontiguousarray(pred)).cuda()
    out = torch.empty(1, CLASSES, 2, 2 + BINS, dtype=torch.int32, device="cuda")
    ws = torch.empty(hip.boundary_scratch(1, H, W, CLASSES), dtype=torch.uint8, device="cuda")
    for i in (0, sets - 1):
        got = hip.boundary_counts(g[i:i + 1], p[i:i + 1], CLASSES, BINS, skip, out=out, workspace=ws).cpu().numpy()[0]
        if not np.array_equal(got, scipy_counts(gt[i], pred[i], CLASSES, BINS, skip)):
            raise SystemExit(f"FAIL: the kernel and the scipy recipe differ on pair {i}")
    contour = [int(got[:, 0, 0].sum()), int(got[:, 1, 0].sum())]
    reps = max(2, a.reps // 10) if worst else a.reps
    us, span = _spread(_windows(lambda k: hip.boundary_counts(g[k:k + 1], p[k:k + 1], CLASSES, BINS, skip, out=out, workspace=ws), sets,
                                reps, a.windows))
    times = []
    for i in range(a.host_frames):
        t0 = time.perf_counter()
        scipy_counts(gt[i % sets], p[i % sets].cpu().numpy(), CLASSES, BINS, skip)
        times.append((time.perf_counter() - t0) * 1e3)
    host, host_span = _spread(times)
    return {"frame": [H, W], "maps": what, "classes": CLASSES, "bins": BINS, "skip": list(skip), "buffer_sets": sets,
            "contour_pixels_gt_pred": contour, "workspace_bytes": ws.numel(), "us_per_frame": us, "us_range": span,
            "host_ms_per_frame": host, "host_ms_range": host_span, "host_route": "map.cpu() + scipy binary_erosion + distance_transform_edt",
            "kernel_over_host": round(us / (host * 1e3), 6)}


def evaluation(a):
    import torch
    from bench_gt_decode import COLOURS, blob_labels, rgba_pictures
    from online_loop import endovis_model, noisy_frames, take_turns
    from stswincl_amd import video
    from stswincl_amd.utils import groundtruth
    from stswincl_amd.utils.visualize import default_palette
    H, W = SIZE
    model, name = endovis_model(a.seed, COLOURS)
    gen = np.random.default_rng(a.seed)
    n = 16
    frames = noisy_frames(gen, n, H, W)
    stored = rgba_pictures(gen, blob_labels(gen, n, H, W, COLOURS))            # host memory: what a PNG decoder hands over
    table = groundtruth.colour_table(default_palette()[:COLOURS])
    res = {"model": name, "frame": [H, W], "classes": COLOURS, "bins": BINS, "autocast": "bf16", "frames_per_window": a.frames,
           "windows": a.online_windows, "ground_truth": "random regions of 32 pixels, stored RGBA on the host"}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        kw = dict(graph=True, out="labels", out_size=(H, W), gt_table=table, scores="deferred")
        segs = {"scores": video.VideoSegmenter(model, **kw), "boundary": video.VideoSegmenter(model, boundary="deferred", boundary_bins=BINS, **kw)}
        res.update(take_turns(segs, lambda p, k: segs[p].push(frames[k % n], gt=stored[k % n]), a.frames, a.online_windows))
        t0 = time.perf_counter()
        scores = segs["boundary"].boundary_scores()
        res["boundary_scores_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["scored_frames"] = len(scores)
    res["nsd_2"] = round(scores.aggregate(scores.nsd(2)).mean, 6)
    res["log_bytes_per_frame"] = COLOURS * 2 * (2 + BINS) * 4
    res["boundary_over_scores"] = round(res["boundary_frames_per_s"] / res["scores_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="calls per timed window (a tenth of it in the worst case)")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--frames", type=int, default=48, help="frames per evaluation window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-evaluation", action="store_true")
    ap.add_argument("--step", choices=list(STEPS), help="(internal) run one step in this process and print its JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_boundary_line.json"))
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_boundary.py measures on the GPU: no device found")
        res = evaluation(a) if a.step == "evaluation" else launch(a, a.step == "launch_worst")
        print("STEP " + json.dumps(res))
        return
    res = {}
    passed = [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in ("reps", "windows", "host_frames", "frames", "online_windows", "seed")]
    for step, limit in STEPS.items():
        if step == "evaluation" and a.no_evaluation:
            continue
        try:                                       # a fresh process per GPU step, under the step's own time limit
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + passed, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"FAIL: step {step} ran longer than {limit} s; nothing more is started")
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"FAIL: step {step} ended with status {p.returncode}; nothing more is started")
        res[step] = json.loads(lines[-1][5:])
        print(f"[bench_boundary] {step}: {lines[-1][5:]}", file=sys.stderr, flush=True)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
