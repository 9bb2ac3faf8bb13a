#!/usr/bin/env python3
"""Cost of the run-length masks (stswin_rle_encode, VideoSegmenter(masks=...)), one run on one MI355X at 1024x1280:

  maps           the label maps that the bench model - the seeded TswinPlus(12, (64, 80)) of the online measurement - makes of its
                 `DISTINCT` = 16 noisy frames, and hip.label_components of them (K = 256, skip the background): the uint8 and the int32
                 map of the same frames.  `count` is [min, median, max] of their runs; the first and the last map are compared with
                 utils.rle.encode before timing
  encode         the three launches of hip.rle_encode alone (cap = 16384), one map per call, on the uint8 and on the int32 maps.
                 Measured as tools/bench_tracks.py measures its launches: device events around replays of a captured hipGraph that
                 holds one call per map of `buffer_sets` maps, together larger than the 256 MB last-level cache, so that a call's first
                 read of its map comes from HBM (the second one, of the third launch, finds it in the caches); one set of outputs
                 and one workspace, as the segmenter has them
  components, tracks   hip.label_components on the cold label maps and hip.track_instances on the cold component maps of the same
                 run, for scale; encode_int32_over_components is the ratio the design note answers for
  host           what the call replaces: the map's .cpu() (a synchronising download) plus utils.rle.encode on the host, wall time
                 per frame, the median of `--host-frames` frames, for both maps
  online         frames/s of VideoSegmenter(graph=True, out="labels", report="deferred", instances=256, tracks=True), bf16 autocast,
                 GPU-resident frames, one frame per push, push -> synchronise, without (the parent's path: the yardstick) and with
                 masks="deferred", taking turns in windows of `--frames` frames; the median window of each with its range (the
                 yardstick's range is the run-to-run spread the difference is read against), and `largest_count`, the largest number
                 of runs of a frame in the mask log, against the default mask_runs = 16384

    python tools/bench_masks.py [--reps 300] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_masks_line.json
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

from bench_instruments import COLD_BYTES, DISTINCT, _windows  # noqa: E402
from online_loop import endovis_model, noisy_frames, take_turns  # noqa: E402
from stswincl_amd import hip, video  # noqa: E402
from stswincl_amd.utils import rle  # noqa: E402

K = 256
SKIP = (0,)
CAP = 16384
SIZE, CLASSES = (1024, 1280), 12


def _spread(w):
    return round(float(np.median(w)), 2), [round(min(w), 2), round(max(w), 2)]


def launch_cost(model, frames, a):
    H, W = SIZE
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        labels = torch.stack(video.VideoSegmenter(model, out="labels", out_size=SIZE, batch=4).segment_sequence(frames))
    comp, rows, total = hip.label_components(labels, CLASSES, 8, SKIP, K)
    n = labels.shape[0]
    res = {"frame": [H, W], "maps": f"the bench model's labels of {n} noisy frames and their components (K = {K})", "cap": CAP,
           "instances": [int(total.min()), int(total.median()), int(total.max())]}
    out = (torch.empty(1, CAP, 2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
    ws = torch.empty(hip.rle_encode_scratch(1, H, W), dtype=torch.uint8, device="cuda")
    for name, maps in (("uint8", labels), ("int32", comp)):
        counts = hip.rle_encode(maps, CAP)[1].cpu().numpy()
        for i in (0, n - 1):
            got = hip.rle_encode(maps[i:i + 1], CAP, out=out, workspace=ws)
            want = rle.encode(maps[i].cpu().numpy(), CAP)
            if not np.array_equal(got[0].cpu().numpy(), want[0]) or not np.array_equal(got[1].cpu().numpy(), want[1]):
                raise SystemExit(f"FAIL: the kernel and utils.rle.encode differ on {name} map {i}")
        sets = max(2, -(-COLD_BYTES // (maps.element_size() * H * W)))
        cold = maps.repeat(-(-sets // n), 1, 1)[:sets].contiguous()
        us, span = _spread(_windows(lambda k: hip.rle_encode(cold[k:k + 1], CAP, out=out, workspace=ws), sets, a.reps, a.windows))
        res.update({f"count_{name}": [int(counts.min()), int(np.median(counts)), int(counts.max())], f"buffer_sets_{name}": sets,
                    f"encode_{name}_us_per_frame": us, f"encode_{name}_us_range": span})
        if name == "uint8":                       # the component launches on the same cold label maps
            cout = (torch.empty(1, H, W, dtype=torch.int32, device="cuda"), torch.empty(1, K, 12, dtype=torch.int64, device="cuda"),
                    torch.empty(1, dtype=torch.int32, device="cuda"))
            cws = torch.empty(hip.label_components_scratch(1, H, W), dtype=torch.uint8, device="cuda")
            us, span = _spread(_windows(lambda k: hip.label_components(cold[k:k + 1], CLASSES, 8, SKIP, K, out=cout, workspace=cws), sets,
                                        a.reps, a.windows))
            res.update({"components_us_per_frame": us, "components_us_range": span})
        else:                                     # the tracker on the same cold component maps
            state = hip.TrackState(H, W, K, "cuda")
            tout = (torch.empty(K, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
            us, span = _spread(_windows(lambda k: hip.track_instances(cold[k], rows[k % n], total[k % n:k % n + 1], state, out=tout), sets,
                                        a.reps, a.windows))
            res.update({"tracks_us_per_frame": us, "tracks_us_range": span})
        del cold
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        times = []
        for i in range(a.host_frames):
            t0 = time.perf_counter()
            rle.encode(maps[i % n].cpu().numpy(), CAP)
            times.append((time.perf_counter() - t0) * 1e6)
        res.update({f"host_{name}_us_per_frame": round(float(np.median(times)), 1), f"host_{name}_us_range": [round(min(times), 1), round(max(times), 1)]})
    res["host_route"] = "map.cpu() + utils.rle.encode"
    res["encode_int32_over_components"] = round(res["encode_int32_us_per_frame"] / res["components_us_per_frame"], 3)
    res["encode_int32_over_tracks"] = round(res["encode_int32_us_per_frame"] / res["tracks_us_per_frame"], 3)
    res["encode_int32_over_host"] = round(res["encode_int32_us_per_frame"] / res["host_int32_us_per_frame"], 5)
    return res


def online(model, name, frames, a):
    n = frames.shape[0]
    chain = dict(report="deferred", instances=K, tracks=True)
    paths = {"chain": {}, "masks": dict(masks="deferred", mask_runs=CAP)}
    res = {"model": name, "frame": list(SIZE), "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows, "max_instances": K,
           "mask_runs": CAP}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {p: video.VideoSegmenter(model, graph=True, out="labels", out_size=SIZE, **chain, **kw) for p, kw in paths.items()}
        res.update(take_turns(segs, lambda p, k: segs[p].push(frames[k % n]), a.frames, a.online_windows))
        t0 = time.perf_counter()
        rep = segs["masks"].mask_report()
        res["mask_report_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["reported_frames"] = len(rep)
    res["largest_count"] = int(rep.count.max())
    res["truncated_frames"] = int(rep.truncated.sum())
    res["log_bytes_per_frame"] = 8 * CAP + 4
    res["masks_over_chain"] = round(res["masks_frames_per_s"] / res["chain_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--host-frames", type=int, default=5)
    ap.add_argument("--frames", type=int, default=48, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_masks_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_masks.py measures on the GPU: no device found")
    model, name = endovis_model(a.seed, CLASSES)
    frames = noisy_frames(np.random.default_rng(a.seed), DISTINCT, *SIZE)
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
