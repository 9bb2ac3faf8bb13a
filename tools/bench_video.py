#!/usr/bin/env python3
"""Video inference throughput and per-frame latency: the reference's evaluation protocol (seg18/test.py:147-175, one model(clip) per
frame) against stswincl_amd.video.VideoSegmenter online (eager and graph replay) and offline (batch 4).

A seeded synthetic sequence of 1024x1280 uint8 frames, TswinPlus(12, (64, 80)) in eval mode under bf16 autocast.  Every variant
warms up, then runs --frames frames; each frame is timed from its push to a device synchronise (host clock), as test.py:152-160
times each frame.  (a) gets GPU-resident 512x640 fp32 clips built beforehand: the host PIL resize of the reference is left out, to
be fair to the baseline.  (b) and (c) push one uint8 frame (GPU-resident) at a time; (d) pushes the whole sequence and times
push + finish per frame on average.  Also the ingest kernel alone: us per frame and GB/s from algorithmic bytes (uint8 read
+ uint8 intermediate written and read + fp32 written).

    python tools/bench_video.py [--frames 64] [--warmup 8]    -> one JSON line
    python tools/bench_video.py --only a|b ...                 (one variant, no ingest timing: for a kernel trace of it)

--protocol cadis (segcata/cata_test.py:115-170): 540x960 frames, base_cata_np.TswinPlusv5(9), the CaDIS clip rule and
normalisation; (b) - (d) segment with gt into the pooled 8-class confusion matrix (labels at 540x960, align_corners=False), and
the upsample + argmax + confusion kernel is timed alone on one frame's logits (us per frame).
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

from stswincl_amd import video  # noqa: E402
from stswincl_amd.net.Ours.base18 import TswinPlus  # noqa: E402


def _stats(times_s):
    t = np.asarray(times_s) * 1e3
    return {"frames_per_s": round(len(t) / (t.sum() / 1e3), 2), "p50_ms": round(float(np.percentile(t, 50)), 3),
            "p90_ms": round(float(np.percentile(t, 90)), 3), "frames": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default=None, choices=["a", "b", "c", "d"], help="run one variant only (e.g. under rocprofv3)")
    ap.add_argument("--protocol", default="endovis18", choices=list(video.RULES))
    a = ap.parse_args()
    # the warm-up covers the graph capture, which comes with the first steady-state frame (7, or 8 under the CaDIS rule)
    a.warmup = max(a.warmup, video.min_frames(a.protocol) + 1)
    n = a.warmup + a.frames
    torch.manual_seed(a.seed)
    cadis = a.protocol == "cadis"
    if cadis:
        from stswincl_amd.net.Ours.base_cata_np import TswinPlusv5
        model, name, fin = TswinPlusv5(9).cuda().eval(), "base_cata_np.TswinPlusv5(9)", (540, 960)
    else:
        model, name, fin = TswinPlus(12, (64, 80)).cuda().eval(), "TswinPlus(12, (64, 80))", (1024, 1280)
    g = np.random.default_rng(a.seed)
    base = g.integers(0, 256, (1, *fin, 3), dtype=np.int64)
    frames = torch.from_numpy(np.clip(base + g.integers(-24, 25, (n, *fin, 3)), 0, 255).astype(np.uint8)).cuda()
    out = {"config": {"model": name, "frames_in": list(fin), "model_in": [512, 640], "autocast": "bf16", "timed_frames": a.frames,
                      "warmup": a.warmup, "protocol": a.protocol}}
    sync = torch.cuda.synchronize
    # CaDIS: ground truth for every frame (with the ignore label 8), the segmenters count it into their confusion matrix
    gts = torch.from_numpy(g.integers(0, 9, (n, *fin))).cuda() if cadis else None
    kw = dict(protocol="cadis", out="labels") if cadis else {}

    def gt_of(f0, f1):
        return gts[f0:f1] if cadis else None

    run = (lambda v: a.only in (None, v))
    # ingest kernel alone
    if a.only is None:
        one = frames[:1]
        for _ in range(5):
            video.ingest(one, (512, 640), protocol=a.protocol)
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 50
        e0.record()
        for _ in range(reps):
            video.ingest(one, (512, 640), protocol=a.protocol)
        e1.record()
        sync()
        us = e0.elapsed_time(e1) * 1e3 / reps
        nbytes = fin[0] * fin[1] * 3 + 2 * fin[0] * 640 * 3 + 512 * 640 * 3 * 4
        out["ingest"] = {"us_per_frame": round(us, 2), "algorithmic_bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
        if cadis:
            from stswincl_amd import hip
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                lg = model(video.ingest(frames[:4], (512, 640), protocol="cadis")[None])
            cm = torch.zeros(8, 8, dtype=torch.int64, device="cuda")
            for form, labels in (("cm_only", False), ("cm_and_labels", True)):
                for _ in range(5):
                    hip.upsample_argmax_cm(lg, *fin, gt=gts[:1], cm=cm, align_corners=False, labels=labels)
                sync()
                e0.record()
                for _ in range(reps):
                    hip.upsample_argmax_cm(lg, *fin, gt=gts[:1], cm=cm, align_corners=False, labels=labels)
                e1.record()
                sync()
                out["upsample_argmax_cm_" + form] = {"us_per_frame": round(e0.elapsed_time(e1) * 1e3 / reps, 2),
                                                     "logits": [str(lg.dtype), *lg.shape[1:]]}

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        # (a) the reference protocol: model(clip) per frame on GPU-resident 512x640 fp32 clips
        images = video.ingest(frames, (512, 640), protocol=a.protocol) if run("a") else None
        if run("a"):
            clips = [images[list(video.clip_frames(f, rule=a.protocol))][None].contiguous() for f in range(n)]
            sync()
            times = []
            for f in range(n):
                t0 = time.perf_counter()
                model(clips[f])
                sync()
                if f >= a.warmup:
                    times.append(time.perf_counter() - t0)
            del clips
            out["a_reference_model_clip"] = _stats(times)

        # (b) online eager, (c) online graph replay: one frame per push, latency = push -> synchronise
        for key, graph in (("b_online_eager", False), ("c_online_graph", True)):
            if not run(key[0]):
                continue
            seg = video.VideoSegmenter(model, graph=graph, **kw)
            times = []
            for f in range(n):
                t0 = time.perf_counter()
                seg.push(frames[f], gt_of(f, f + 1))
                sync()
                if f >= a.warmup:
                    times.append(time.perf_counter() - t0)
            seg.finish()
            sync()
            out[key] = _stats(times)
            del seg

        # (d) offline, batch 4: the whole sequence (one warm-up pass first)
        if not run("d"):
            print(json.dumps(out))
            return
        seg = video.VideoSegmenter(model, batch=4, **kw)
        seg.segment_sequence(frames[:a.warmup + 8], gt_of(0, a.warmup + 8))
        sync()
        t0 = time.perf_counter()
        res = seg.segment_sequence(frames, gt_of(0, n))
        sync()
        dt = time.perf_counter() - t0
        out["d_offline_batch4"] = {"frames_per_s": round(len(res) / dt, 2), "mean_ms": round(dt * 1e3 / len(res), 3), "frames": len(res)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
