#!/usr/bin/env python3
"""Cost of the contrastive pre-training input (stswincl_amd/contrast/views.py) per batch of 8 samples x 6 views x 4 frames from
270 x 480 uint8 frames, at two output sizes: `bench` = 256 x 256, what `bench.py --workload contrast` times, and `native` = 256 x 448,
the reference's get_transform default.  Per configuration:

  device_us_per_batch       the two launches (horizontal pass; vertical pass + table + mask), device events around `--reps` batches
                            that cycle through 8 drawn parameter sets whose tables are already on the device and through two input
                            batches and two output buffers (operands larger than the last-level cache: cold); the median of
                            `--windows` such windows, min and max in device_us_range
  host_ms_per_batch         ContrastViews.sample + ContrastViews.tables on the host, one process; median of the windows
  call_ms_per_batch         cv(frames, labels, params, out=...) to a device synchronise: tables, pinned upload and launches together
  upload_bytes_per_batch    uint8 frames + uint8 labels + the int32 tables; reference_upload_bytes_per_batch is the batch the
                            reference's loader ships: 24 fp32 frames and 6 uint8 masks per sample at the output size

With --step-json FILE (the JSON line `python bench.py --workload contrast` printed in the same session on the same box) each
configuration also holds ratio = (device + host time per batch) / step time; the input must stay below the step: with a ratio >= 1
the tool prints FAIL and exits non-zero.  The reference's loader (torchvision) cannot run here: no speed-up over it is claimed.

    python tools/bench_contrast_input.py [--reps 200] [--windows 7] [--step-json contrast_line.json]
        -> one JSON line, also written to profiles/bench_contrast_input_line.json
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stswincl_amd import hip  # noqa: E402
from stswincl_amd.contrast.views import ContrastViews  # noqa: E402

B, SOURCE = 8, (270, 480)
CONFIGS = (("bench", (256, 256)), ("native", (256, 448)))


def measure(name, out_hw, a):
    cv = ContrastViews(out=out_hw, source=SOURCE)
    gen = torch.Generator().manual_seed(a.seed)
    inputs = [(torch.randint(0, 256, (B, cv.n_frames, *SOURCE, 3), dtype=torch.uint8, generator=gen).cuda(),
               torch.randint(0, 12, (B, cv.n_labels, *SOURCE), dtype=torch.uint8, generator=gen).cuda()) for _ in range(2)]
    outs = [(torch.empty(cv.views, B, 4, 3, *out_hw, device="cuda"), torch.empty(cv.views, B, 1, *out_hw, device="cuda")) for _ in range(2)]
    rng = random.Random(a.seed)
    sets = [cv.sample(B, rng) for _ in range(8)]
    sync = torch.cuda.synchronize
    dev = inputs[0][0].device
    ws, lut, V = cv._workspace(B, dev), cv._lut(dev), cv.views * B
    resident = [torch.from_numpy(cv.tables(p)).cuda() for p in sets]

    def launches(i):
        (fr, lb), (img, msk) = inputs[i % 2], outs[i % 2]
        hip.contrast_views(fr.view(-1, *SOURCE, 3), lb.view(-1, *SOURCE), ws["tmp"], img.view(V, 4, 3, *out_hw), msk.view(V, 1, *out_hw),
                           resident[i % len(resident)], lut, cv.ksize)

    for i in range(16):
        launches(i)
    sync()
    windows = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            launches(i)
        e1.record()
        sync()
        windows.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    device_us = float(np.median(windows))

    host_windows = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        for _ in range(a.host_reps):
            cv.tables(cv.sample(B, rng))
        host_windows.append((time.perf_counter() - t0) * 1e3 / a.host_reps)
    host_ms = float(np.median(host_windows))

    for i in range(8):
        cv(*inputs[i % 2], sets[i % len(sets)], out=outs[i % 2])
    sync()
    t0 = time.perf_counter()
    for i in range(a.host_reps):
        cv(*inputs[i % 2], sets[i % len(sets)], out=outs[i % 2])
    sync()
    call_ms = (time.perf_counter() - t0) * 1e3 / a.host_reps

    fr, lb = inputs[0]
    table_bytes = int(resident[0].numel() * 4)
    res = {"out": list(out_hw), "ksize": cv.ksize, "device_us_per_batch": round(device_us, 2),
           "device_us_range": [round(min(windows), 2), round(max(windows), 2)], "host_ms_per_batch": round(host_ms, 3),
           "host_ms_range": [round(min(host_windows), 3), round(max(host_windows), 3)], "call_ms_per_batch": round(call_ms, 3),
           "upload_bytes_per_batch": int(fr.numel() + lb.numel() + table_bytes), "table_bytes_per_batch": table_bytes,
           "reference_upload_bytes_per_batch": int(B * 24 * 3 * out_hw[0] * out_hw[1] * 4 + B * 6 * out_hw[0] * out_hw[1]),
           "output_bytes_per_batch": int(sum(t.numel() * 4 for t in outs[0])),
           "first_parameter_set": [[p.i, p.j, p.h, p.w, int(p.hflip)] for p in sets[0][0]]}
    del inputs, outs, resident, cv
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="batches per timed device window")
    ap.add_argument("--host-reps", type=int, default=20, help="batches per timed host window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_contrast_input_line.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contrast_input.py measures on the GPU: no device found")
    res = {"config": {"batch": B, "views": 6, "frames_per_view": 4, "frames_per_sample": 17, "labels_per_sample": 6, "source": list(SOURCE),
                      "reps": a.reps, "host_reps": a.host_reps, "windows": a.windows, "device": torch.cuda.get_device_name(0)}}
    for name, out_hw in CONFIGS:
        res[name] = measure(name, out_hw, a)
    failed = []
    if a.step_json:
        with open(a.step_json) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        step = json.loads(line)
        step_ms = float(step["ms_per_step"])
        res["step_ms"] = round(step_ms, 3)
        res["step_metric"] = step.get("metric")
        for name, _ in CONFIGS:
            r = res[name]
            r["input_ms_per_batch"] = round(r["device_us_per_batch"] / 1e3 + r["host_ms_per_batch"], 3)
            r["ratio"] = round(r["input_ms_per_batch"] / step_ms, 4)
            r["device_ratio"] = round(r["device_us_per_batch"] / 1e3 / step_ms, 4)
            r["below_step"] = bool(r["input_ms_per_batch"] < step_ms)
            if not r["below_step"]:
                failed.append(name)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    if failed:
        raise SystemExit(f"FAIL: the input of {failed} takes as long as the contrastive step ({res['step_ms']} ms) or longer: the input, "
                         "not the step, would bound pre-training")


if __name__ == "__main__":
    main()
