#!/usr/bin/env python3
"""Cost of the confidence launches (stswin_upsample_confidence, stswin_confidence_sums, VideoSegmenter(confidence=...)), one run on
one MI355X:

  launch         per output size - 1024x1280 (align_corners=True, the EndoVis form) and 540x960 (align_corners=False, the CaDIS form),
                 both from fp32 logits [12][512][640] - the map launch and the two launches of the sums (K = 12 over the uint8 labels,
                 K = 256 over an int32 component map) alone, one frame per call.  Measured as tools/bench_masks.py measures its
                 launches: device events around replays of a captured hipGraph that holds one call per frame of `buffer_sets` frames of
                 seeded random logits, together larger than the 256 MB last-level cache, so that a call reads its logits from HBM.  The
                 first frame's map is compared with utils.confidence before timing (every byte within one step; the tests hold the
                 tight bound)
  torch          what the launches replace, on the same cold frames: F.interpolate -> softmax(1) -> max(1) -> the byte, captured and
                 replayed the same way, and torch.bincount with weights (count, sum of conf, conf < low: three calls) in eager mode
                 between device events (bincount sizes its result on the host, so it cannot be captured); `sums_eager_us` is our
                 launches timed in that same eager way, the like-for-like figure
  online         frames/s of VideoSegmenter(graph=True, out="labels"), bf16 autocast, GPU-resident 1024x1280 frames, one frame per
                 push, push -> synchronise, without (the parent's path: the yardstick) and with confidence="deferred", taking turns in
                 windows of `--frames` frames; the median window of each with its range (the yardstick's range is the run-to-run
                 spread the difference is read against)

    python tools/bench_confidence.py [--reps 300] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_confidence_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_instruments import COLD_BYTES, DISTINCT, _windows, instrument_maps  # noqa: E402
from online_loop import endovis_model, noisy_frames, take_turns  # noqa: E402
from stswincl_amd import hip, video  # noqa: E402
from stswincl_amd.utils import confidence  # noqa: E402

CLASSES, LOGITS = 12, (512, 640)
K = 256
LOW = 128
SIZES = {"1024x1280": ((1024, 1280), True), "540x960": ((540, 960), False)}


def _spread(w):
    return round(float(np.median(w)), 2), [round(min(w), 2), round(max(w), 2)]


def _eager_windows(fn, sets, reps, windows):
    """us per call of fn(k) launched from the host, k cycling over the buffer sets, between device events."""
    for k in range(min(sets, 8)):
        fn(k)
    torch.cuda.synchronize()
    res = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i % sets)
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / reps)
    return res


def _torch_map(logits, size, align):
    p = F.interpolate(logits, size=size, mode="bilinear", align_corners=align).softmax(1).max(1).values
    return (p * 255.0 + 0.5).to(torch.uint8)


def _torch_sums(maps, conf, k, low):
    m, q = maps.reshape(-1).long(), conf.reshape(-1)
    keep = (m >= 0) & (m < k)
    m, q = m[keep], q[keep]
    return torch.stack((torch.bincount(m, minlength=k), torch.bincount(m, weights=q.double(), minlength=k).long(),
                        torch.bincount(m, weights=(q < low).double(), minlength=k).long()), 1)


def launch_cost(a):
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    frame_bytes = 4 * CLASSES * LOGITS[0] * LOGITS[1]
    sets = max(2, -(-COLD_BYTES // frame_bytes))
    logits = (torch.randn(sets, CLASSES, *LOGITS, device="cuda", generator=gen) * 3).clamp_(-16, 16)
    res = {"logits": [CLASSES, *LOGITS], "dtype": "fp32", "buffer_sets": sets, "low": LOW, "instances": K,
           "maps": "labels of the seeded random logits; components of synthetic instrument maps"}
    for name, (size, align) in SIZES.items():
        H, W = size
        labels = hip.upsample_argmax_cm(logits, H, W, align_corners=align)
        conf = hip.upsample_confidence(logits, labels, align)
        want = 255.0 * confidence.upsample_probability(logits[:1].cpu().numpy(), labels[:1].cpu().numpy(), align)
        if float(np.abs(conf[:1].cpu().numpy() - want).max()) > 1.0:
            raise SystemExit(f"FAIL: the kernel and utils.confidence differ at {name}")
        inst = torch.from_numpy(instrument_maps(np.random.default_rng(a.seed), DISTINCT, H, W, CLASSES)).cuda()
        comp = hip.label_components(inst, CLASSES, 8, (0,), K)[0]
        comp = comp.repeat(-(-sets // DISTINCT), 1, 1)[:sets].contiguous()
        for maps, k, what in ((labels, CLASSES, "class"), (comp, K, "instance")):
            if not torch.equal(hip.confidence_sums(maps[:2], conf[:2], k, LOW), torch.stack([_torch_sums(maps[i], conf[i], k, LOW) for i in range(2)])):
                raise SystemExit(f"FAIL: the kernel and torch.bincount differ on the {what} sums at {name}")
        out_conf = torch.empty(1, H, W, dtype=torch.uint8, device="cuda")
        out_c = torch.empty(1, CLASSES, 3, dtype=torch.int64, device="cuda")
        out_i = torch.empty(1, K, 3, dtype=torch.int64, device="cuda")
        r = {"frame": [H, W], "align_corners": align}
        r["map_us"], r["map_us_range"] = _spread(_windows(lambda i: hip.upsample_confidence(logits[i:i + 1], labels[i:i + 1], align, out=out_conf),
                                                          sets, a.reps, a.windows))
        r["torch_map_us"], r["torch_map_us_range"] = _spread(_windows(lambda i: _torch_map(logits[i:i + 1], size, align), sets, a.reps, a.windows))
        for maps, k, out, what in ((labels, CLASSES, out_c, "class"), (comp, K, out_i, "instance")):
            ours = lambda i: hip.confidence_sums(maps[i:i + 1], conf[i:i + 1], k, LOW, out=out)      # noqa: E731
            r[f"{what}_sums_us"], r[f"{what}_sums_us_range"] = _spread(_windows(ours, sets, a.reps, a.windows))
            r[f"{what}_sums_eager_us"], r[f"{what}_sums_eager_us_range"] = _spread(_eager_windows(ours, sets, a.reps, a.windows))
            r[f"torch_{what}_sums_eager_us"], r[f"torch_{what}_sums_eager_us_range"] = _spread(
                _eager_windows(lambda i: _torch_sums(maps[i], conf[i], k, LOW), sets, a.reps, a.windows))
        r["map_over_torch"] = round(r["map_us"] / r["torch_map_us"], 4)
        res[name] = r
        del labels, conf, comp
        torch.cuda.empty_cache()
    res["torch_route"] = "F.interpolate -> softmax(1) -> max(1) -> uint8; torch.bincount x 3 (minlength = K, weights)"
    return res


def online(model, name, frames, a):
    n = frames.shape[0]
    size = SIZES["1024x1280"][0]
    paths = {"labels": {}, "confidence": dict(confidence="deferred", confidence_low=LOW)}
    res = {"model": name, "frame": list(size), "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {p: video.VideoSegmenter(model, graph=True, out="labels", out_size=size, **kw) for p, kw in paths.items()}
        res.update(take_turns(segs, lambda p, k: segs[p].push(frames[k % n]), a.frames, a.online_windows))
        rep = segs["confidence"].confidence_report()
    res["reported_frames"] = len(rep)
    res["mean_confidence"] = round(float(np.nanmean(rep.mean)), 4)
    res["confidence_over_labels"] = round(res["confidence_frames_per_s"] / res["labels_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--frames", type=int, default=48, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_confidence_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_confidence.py measures on the GPU: no device found")
    res = {"launch": launch_cost(a)}
    torch.cuda.empty_cache()
    if not a.no_online:
        model, name = endovis_model(a.seed, CLASSES)
        res["online"] = online(model, name, noisy_frames(np.random.default_rng(a.seed), DISTINCT, *SIZES["1024x1280"][0]), a)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
