#!/usr/bin/env python3
"""Cost of the clearance launches (stswin_instance_clearance, VideoSegmenter(clearance=...)), one run on one MI355X:

  launch         per frame size - 1024x1280 and 540x960 - hip.instance_clearance (K = 64, 12 classes, every class a target, no
                 limit) alone, one frame per call, on the synthetic instrument maps of tools/bench_parts.py (bars and discs of several
                 classes on background; their classes grouped, so an instance has own classes) and the components
                 hip.label_components takes of the grouped maps.  Measured as tools/bench_parts.py measures its launch: device events
                 around replays of a captured hipGraph that holds one call per frame of `buffer_sets` frames, together larger than
                 the 256 MB last-level cache, so that a call reads its maps from HBM.  The first frames' result is compared with the
                 numpy definition before timing
  yardstick      hip.boundary_counts in the same run over the same maps (a frame as int64 ground truth against the next frame): the
                 same passes - fill, mark, classes per segment, column distances, query - over two maps instead of one, with contour
                 pixels of one class as its query set where clearance has the instances' border pixels times the classes they do not
                 hold; `clearance_over_boundary` is the ratio
  host           for scale, what a pipeline without the kernel would do: download one frame's labels and components and run the numpy
                 definition (utils.instruments.instance_clearance), wall clock, `--host-frames` frames per size
  online         frames/s of VideoSegmenter(graph=True, out="labels", report="deferred", instances=K, instance_groups=...), bf16
                 autocast, GPU-resident 1024x1280 frames, one frame per push, push -> synchronise, without (the yardstick) and with
                 clearance="deferred", taking turns in windows of `--frames` frames; the median window of each with its range
  ab             with --parent DIR (a built checkout of the parent commit): the keyword-less segmenter of that tree against this
                 tree's, each in a fresh child process of this tool (--child TREE), the two taking turns `--ab-rounds` times; per side
                 the median of all its windows with their range, and `new_over_parent`

    python tools/bench_clearance.py [--reps 300] [--windows 7] [--frames 48] [--parent DIR]
        -> one JSON line, also written to profiles/bench_clearance_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --child TREE: the package of another tree (the parent commit's), the helpers of this one
TREE = os.path.abspath(sys.argv[sys.argv.index("--child") + 1]) if "--child" in sys.argv[1:-1] else ROOT
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, TREE)

from stswincl_amd import hip, video  # noqa: E402  (first: the helper modules below put this tree in front of the path themselves)
from stswincl_amd.utils import instruments as I  # noqa: E402
from bench_confidence import _spread  # noqa: E402
from bench_instruments import COLD_BYTES, DISTINCT, _windows, instrument_maps  # noqa: E402
from online_loop import endovis_model, noisy_frames, take_turns  # noqa: E402

CLASSES = 12
K = 64
BINS = 32
GROUPS = (tuple(range(1, CLASSES)),)          # every class but the background is a part of an instrument
SIZES = {"1024x1280": (1024, 1280), "540x960": (540, 960)}


def launch_cost(a):
    table = torch.from_numpy(I.group_table(GROUPS, CLASSES)).cuda()
    res = {"classes": CLASSES, "instances": K, "groups": [list(g) for g in GROUPS], "targets": "all", "max_distance": None,
           "maps": "synthetic instrument maps; components of the grouped maps at 8-connectivity"}
    for name, (H, W) in SIZES.items():
        sets = max(2, -(-COLD_BYTES // (5 * H * W)))
        lab = torch.from_numpy(instrument_maps(np.random.default_rng(a.seed), DISTINCT, H, W, CLASSES)).cuda()
        comp = hip.label_components(hip.gt_decode(lab, table), CLASSES, 8, (0,), K)[0]
        host = []
        got = hip.instance_clearance(lab[:a.host_frames], comp[:a.host_frames], K, CLASSES)
        for f in range(a.host_frames):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = I.instance_clearance(lab[f].cpu().numpy(), comp[f].cpu().numpy(), K, CLASSES)
            host.append((time.perf_counter() - t0) * 1e3)
            if not np.array_equal(got[f].cpu().numpy(), want[0]):
                raise SystemExit(f"FAIL: the kernel and the numpy definition differ at {name}, frame {f}")
        lab = lab.repeat(-(-sets // DISTINCT), 1, 1)[:sets].contiguous()
        comp = comp.repeat(-(-sets // DISTINCT), 1, 1)[:sets].contiguous()
        gt = lab.long()
        out = torch.empty(1, K, CLASSES, 3, dtype=torch.int64, device="cuda")
        ws = torch.empty(hip.instance_clearance_scratch(1, H, W, CLASSES, K), dtype=torch.uint8, device="cuda")
        out_b = torch.empty(1, CLASSES, 2, 2 + BINS, dtype=torch.int32, device="cuda")
        ws_b = torch.empty(hip.boundary_scratch(1, H, W, CLASSES), dtype=torch.uint8, device="cuda")
        ours = lambda i: hip.instance_clearance(lab[i:i + 1], comp[i:i + 1], K, CLASSES, out=out, workspace=ws)        # noqa: E731
        yard = lambda i: hip.boundary_counts(gt[i:i + 1], lab[(i + 1) % sets:(i + 1) % sets + 1], CLASSES, BINS, (0,),   # noqa: E731
                                             out=out_b, workspace=ws_b)
        first = got[0].cpu().numpy()
        r = {"frame": [H, W], "buffer_sets": sets, "instances_in_frame_0": int(comp[0].max()) + 1,
             "pairs_in_frame_0": int((first[..., 0] >= 0).sum()), "largest_d2_in_frame_0": int(first[..., 0].max())}
        r["clearance_us"], r["clearance_us_range"] = _spread(_windows(ours, sets, a.reps, a.windows))
        r["boundary_us"], r["boundary_us_range"] = _spread(_windows(yard, sets, a.reps, a.windows))
        r["clearance_over_boundary"] = round(r["clearance_us"] / r["boundary_us"], 4)
        r["host_ms"], r["host_ms_range"] = _spread(host) if host else (None, None)
        res[name] = r
        del lab, comp, gt
        torch.cuda.empty_cache()
    res["host_route"] = "download of labels and components, then utils.instruments.instance_clearance (numpy)"
    return res


def online(model, name, frames, a):
    n = frames.shape[0]
    size = SIZES["1024x1280"]
    paths = {"instances": {}, "clearance": dict(clearance="deferred")}
    res = {"model": name, "frame": list(size), "autocast": "bf16", "frames_per_window": a.frames, "windows": a.online_windows}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        segs = {p: video.VideoSegmenter(model, graph=True, out="labels", out_size=size, report="deferred", instances=K,
                                        instance_groups=GROUPS, **kw) for p, kw in paths.items()}
        res.update(take_turns(segs, lambda p, k: segs[p].push(frames[k % n]), a.frames, a.online_windows))
        rep = segs["clearance"].clearance_report()
    res["reported_frames"] = len(rep)
    res["measured_pairs"] = int(rep.measured.sum())
    res["clearance_over_instances"] = round(res["clearance_frames_per_s"] / res["instances_frames_per_s"], 4)
    return res


def child(a):
    """--child TREE: the keyword-less segmenter of the package at TREE, its windows as one JSON line."""
    model, _ = endovis_model(a.seed, CLASSES)
    frames = noisy_frames(np.random.default_rng(a.seed), DISTINCT, *SIZES["1024x1280"])
    n = frames.shape[0]
    fps = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        seg = video.VideoSegmenter(model, graph=True, out="labels", out_size=SIZES["1024x1280"], report="deferred", instances=K,
                                   instance_groups=GROUPS)
        for k in range(video.min_frames("endovis18") + 4):
            seg.push(frames[k % n])
            torch.cuda.synchronize()
        for w in range(a.online_windows):
            t0 = time.perf_counter()
            for k in range(a.frames):
                seg.push(frames[(w * a.frames + k) % n])
                torch.cuda.synchronize()
            fps.append(a.frames / (time.perf_counter() - t0))
    assert seg.captured
    print(json.dumps({"tree": os.path.dirname(os.path.dirname(os.path.abspath(video.__file__))), "frames_per_s": fps}))


def ab(a):
    """The keyword-less segmenter of the tree at --parent against this tree's: fresh child processes, taking turns."""
    sides = {"parent": os.path.abspath(a.parent), "new": ROOT}
    fps = {s: [] for s in sides}
    for _ in range(a.ab_rounds):
        for side, tree in sides.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--online-windows", str(a.online_windows),
                   "--seed", str(a.seed), "--child", tree, "--no-online"]
            text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            line = json.loads([t for t in text.splitlines() if t.startswith("{")][-1])
            if os.path.realpath(line["tree"]) != os.path.realpath(tree):
                raise SystemExit(f"FAIL: the child of {tree} imported the package of {line['tree']}")
            fps[side] += line["frames_per_s"]
    res = {"rounds": a.ab_rounds, "frames_per_window": a.frames, "windows_per_round": a.online_windows, "path": "no clearance keyword"}
    for side in sides:
        res[f"{side}_frames_per_s"], res[f"{side}_frames_per_s_range"] = _spread(fps[side])
    res["new_over_parent"] = round(res["new_frames_per_s"] / res["parent_frames_per_s"], 4)
    lo = max(res["parent_frames_per_s_range"][0], res["new_frames_per_s_range"][0])
    hi = min(res["parent_frames_per_s_range"][1], res["new_frames_per_s_range"][1])
    res["ranges_overlap"] = lo <= hi
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--frames", type=int, default=48, help="frames per online window")
    ap.add_argument("--online-windows", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=1, help="frames per size the host route is timed on (and the kernel checked on)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-online", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the keyword-less A/B against it")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_clearance_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clearance.py measures on the GPU: no device found")
    if a.child is not None:
        return child(a)
    res = {}
    if a.parent is not None:                  # first: the only process on the device while the children run
        res["ab"] = ab(a)
    res["launch"] = launch_cost(a)
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
