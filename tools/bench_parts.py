#!/usr/bin/env python3
"""Cost of the parts launch (stswin_instance_parts, VideoSegmenter(instance_groups=..., parts=...)), one run on one MI355X:

  launch         per frame size - 1024x1280 and 540x960 - hip.instance_parts (K = 64, 12 classes) alone, one frame per call, on
                 synthetic instrument maps made here (bars and discs of several classes on background; their classes grouped, so an
                 instance has parts) and the components hip.label_components takes of the grouped maps.  Measured as
                 tools/bench_confidence.py measures its launches: device events around replays of a captured hipGraph that holds one
                 call per frame of `buffer_sets` frames, together larger than the 256 MB last-level cache, so that a call reads its
                 maps from HBM.  The first frames' result is compared with the torch formulation before timing
  yardstick      hip.confidence_sums over the same int32 component maps with the label maps as its uint8 operand: the same 5 bytes
                 per pixel read, one table of K x 3 sums - the byte-equivalent launch; `parts_over_sums` is the ratio
  torch          what the launch replaces, on the same cold frames, on the device: index_add_ / scatter_reduce_ over components * nc +
                 labels for the moments, shifted compares and bincount for the contacts, in eager mode between device events
                 (bincount sizes its result on the host, so it cannot be captured); `parts_eager_us` is our launch timed in that same
                 eager way, the like-for-like figure, `parts_over_torch` their ratio
  online         frames/s of VideoSegmenter(graph=True, out="labels", report="deferred", instances=K), bf16 autocast, GPU-resident
                 1024x1280 frames, one frame per push, push -> synchronise, without (the yardstick) and with instance_groups and
                 parts="deferred", taking turns in windows of `--frames` frames; the median window of each with its range

    python tools/bench_parts.py [--reps 300] [--windows 7] [--frames 48]   -> one JSON line, also written to profiles/bench_parts_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_confidence import _eager_windows, _spread  # noqa: E402
from bench_instruments import COLD_BYTES, DISTINCT, _windows, instrument_maps  # noqa: E402
from online_loop import endovis_model, noisy_frames, take_turns  # noqa: E402
from stswincl_amd import hip, video  # noqa: E402
from stswincl_amd.utils.instruments import group_table  # noqa: E402

CLASSES = 12
K = 64
LOW = 128
GROUPS = (tuple(range(1, CLASSES)),)          # every class but the background is a part of an instrument
SIZES = {"1024x1280": (1024, 1280), "540x960": (540, 960)}
_SHIFTS = (((slice(1, None), slice(None)), (slice(None, -1), slice(None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None))),
           ((slice(None), slice(1, None)), (slice(None), slice(None, -1))), ((slice(None), slice(None, -1)), (slice(None), slice(1, None))))


def _torch_parts(lab, comp, k, nc, xs, ys):
    """utils.instruments.instance_parts of one frame in torch ops on the device: lab uint8 [H][W], comp int32 [H][W], xs / ys int64 grids."""
    H, W = lab.shape
    c, l = comp.long(), lab.long()
    own, cls = (c >= 0) & (c < k), l < nc
    m = own & cls
    key, x, y = (c * nc + l)[m], xs[m], ys[m]
    parts = torch.zeros(k * nc, 10, dtype=torch.int64, device=lab.device)
    parts[:, :6].index_add_(0, key, torch.stack((torch.ones_like(x), x, y, x * x, x * y, y * y), 1))
    parts[:, 6:].scatter_reduce_(0, key[:, None].expand(-1, 4), torch.stack((W - x, H - y, x + 1, y + 1), 1), "amax")
    contacts = torch.zeros(k * nc, dtype=torch.int64, device=lab.device)
    for p, q in _SHIFTS:
        e = own[p] & (c[q] != c[p]) & cls[q]
        contacts += torch.bincount((c[p] * nc + l[q])[e], minlength=k * nc)
    return parts.view(k, nc, 10), contacts.view(k, nc)


def launch_cost(a):
    table = torch.from_numpy(group_table(GROUPS, CLASSES)).cuda()
    res = {"classes": CLASSES, "instances": K, "groups": [list(g) for g in GROUPS],
           "maps": "synthetic instrument maps; components of the grouped maps at 8-connectivity"}
    for name, (H, W) in SIZES.items():
        sets = max(2, -(-COLD_BYTES // (5 * H * W)))
        lab = torch.from_numpy(instrument_maps(np.random.default_rng(a.seed), DISTINCT, H, W, CLASSES)).cuda()
        comp = hip.label_components(hip.gt_decode(lab, table), CLASSES, 8, (0,), K)[0]
        lab = lab.repeat(-(-sets // DISTINCT), 1, 1)[:sets].contiguous()
        comp = comp.repeat(-(-sets // DISTINCT), 1, 1)[:sets].contiguous()
        ys, xs = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        got = hip.instance_parts(lab[:2], comp[:2], K, CLASSES)
        for f in range(2):
            want = _torch_parts(lab[f], comp[f], K, CLASSES, xs, ys)
            if not (torch.equal(got[0][f], want[0]) and torch.equal(got[1][f], want[1])):
                raise SystemExit(f"FAIL: the kernel and the torch formulation differ at {name}")
        out = (torch.empty(1, K, CLASSES, 10, dtype=torch.int64, device="cuda"), torch.empty(1, K, CLASSES, dtype=torch.int64, device="cuda"))
        out_s = torch.empty(1, K, 3, dtype=torch.int64, device="cuda")
        ours = lambda i: hip.instance_parts(lab[i:i + 1], comp[i:i + 1], K, CLASSES, out=out)             # noqa: E731
        yard = lambda i: hip.confidence_sums(comp[i:i + 1], lab[i:i + 1], K, LOW, out=out_s)                # noqa: E731
        r = {"frame": [H, W], "buffer_sets": sets, "instances_in_frame_0": int(comp[0].max()) + 1,
             "keys_in_frame_0": int((got[0][0][..., 0] > 0).sum())}
        r["parts_us"], r["parts_us_range"] = _spread(_windows(ours, sets, a.reps, a.windows))
        r["sums_us"], r["sums_us_range"] = _spread(_windows(yard, sets, a.reps, a.windows))
        r["parts_eager_us"], r["parts_eager_us_range"] = _spread(_eager_windows(ours, sets, a.reps, a.windows))
        r["torch_eager_us"], r["torch_eager_us_range"] = _spread(
            _eager_windows(lambda i: _torch_parts(lab[i], comp[i], K, CLASSES, xs, ys), sets, max(a.reps // 10, 8), a.windows))
        r["parts_over_sums"] = round(r["parts_us"] / r["sums_us"], 4)
        r["parts_over_torch"] = round(r["parts_eager_us"] / r["torch_eager_us"], 4)
        res[name] = r
        del lab, comp, xs, ys
        torch.cuda.empty_cache()
    res["torch_route"] = "index_add_ and scatter_reduce_(amax) over components * nc + labels; four shifted compares and bincount"
    return res


def online(model, name, frames, a):
    n = frames.shape[0]
    size = SIZES["1024x1280"]
    paths = {"instances": {}, "parts": dict(instance_groups=GROUPS, parts="deferred")}
    res = {"model": name, "frame": list(size), "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {p: video.VideoSegmenter(model, graph=True, out="labels", out_size=size, report="deferred", instances=K, **kw)
                for p, kw in paths.items()}
        res.update(take_turns(segs, lambda p, k: segs[p].push(frames[k % n]), a.frames, a.online_windows))
        rep = segs["parts"].parts_report()
    res["reported_frames"] = len(rep)
    res["parts_over_instances"] = round(res["parts_frames_per_s"] / res["instances_frames_per_s"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--frames", type=int, default=48, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_parts_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_parts.py measures on the GPU: no device found")
    res = {"launch": launch_cost(a)}
    torch.cuda.empty_cache()
    if not a.no_online:
        model, name = endovis_model(a.seed, CLASSES)
        res["online"] = online(model, name, noisy_frames(np.random.default_rng(a.seed), DISTINCT, *SIZES["1024x1280"]), a)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
