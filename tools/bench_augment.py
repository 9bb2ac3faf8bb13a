#!/usr/bin/env python3
"""Cost of the training-input augmenter (stswincl_amd/augment.py) per batch of 4 clips x 4 frames at 512x640, mixed parameters:

  device_us_per_batch       the three launches (horizontal pass, vertical pass + label, table + rotate + convert), device events around
                            `--reps` batches that cycle through 8 drawn parameter sets whose tables are already on the device; the
                            median of `--windows` such windows, min and max in device_us_range
  host_ms_per_batch         ClipAugmenter.sample + ClipAugmenter.tables on the host, one process
  call_ms_per_batch         aug(frames, labels, params, out=...) to a device synchronise: tables, pinned upload and launches together
  upload_bytes_per_batch    uint8 frames + uint8 labels + the int32 tables (the reference ships float64 images and int64 one-hot labels)
  pillow_numpy_host_ms_per_batch   the same batch through tests/augment_ref.py's Pillow path + its numpy rotate and conversion, one process
                            on this box.  NOT the reference's loader (albumentations / cv2 are not installed): no speed-up is claimed.

With --step-json FILE (the JSON line `python bench.py` printed in the same session on the same box) the line also holds the
training step time and ratio = (device + host time per batch) / step time; the augmenter must stay below the step: with ratio >= 1
the tool prints FAIL and exits non-zero.

With --p-noise P (the reference's CaDIS value is 0.5; default 0: no sample has noise and the numbers are those of the three
launches) the parameter sets are drawn with that probability of CaDIS's Gaussian noise, a noisy set costs a fourth launch, and the
line also holds, from the same process:

  noise                     the noise launch alone with all 4 clips noisy (15.7 MB read and as much written): device us per launch
                            and the TB/s that is, `cold` over a ring of crop buffers larger than the 256 MiB Infinity Cache, so that
                            every launch reads from and writes to HBM, and `warm` over one buffer
  no_noise                  device_us_per_batch and call_ms_per_batch of the same geometry without any noise key

    python tools/bench_augment.py [--reps 1000] [--windows 7] [--step-json bench_line.json] [--p-noise 0.5]
    -> one JSON line, also written to profiles/bench_augment_line.json (with --p-noise: profiles/bench_augment_noise_line.json)
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from stswincl_amd import hip  # noqa: E402
from stswincl_amd.augment import ClipAugmenter, ClipParams  # noqa: E402

L3_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000, help="batches per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows; the median is reported, min and max beside it")
    ap.add_argument("--host-batches", type=int, default=8, help="batches through the Pillow / numpy host pipeline")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-json", default=None)
    ap.add_argument("--p-noise", type=float, default=0.0, help="probability of CaDIS's Gaussian noise per sample (the reference: 0.5)")
    ap.add_argument("--out", default=None, help="default: profiles/bench_augment_line.json, with --p-noise bench_augment_noise_line.json")
    ap.add_argument("--no-host-pipeline", action="store_true")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bench_augment_noise_line.json" if a.p_noise else "bench_augment_line.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU: no device found")
    import augment_ref as ar
    B, T, hw = 4, 4, (512, 640)
    aug = ClipAugmenter(p_noise=a.p_noise)
    clips = [ar.seeded_clip(a.seed + b, T, *hw) for b in range(B)]
    frames = np.stack([c[0] for c in clips])
    labels = np.stack([c[1] for c in clips])
    dframes, dlabels = torch.from_numpy(frames).cuda(), torch.from_numpy(labels).cuda()
    out = (torch.empty(B, T, 3, *hw, device="cuda"), torch.empty(B, *hw, dtype=torch.int64, device="cuda"))
    rng, gen = random.Random(a.seed), np.random.default_rng(a.seed)
    sets = [aug.sample(B, rng=rng, gen=gen) for _ in range(8)]
    sync = torch.cuda.synchronize

    # the launches alone: 8 table sets resident on the device
    ws = aug._workspace(B, dframes.device)
    lut, label_lut = aug._lut(dframes.device)
    thr, k_min = aug._thresholds(dframes.device), aug.noise_law[1]

    def device_windows(sets):
        resident = []
        for params in sets:
            t1, t2 = aug.tables(params)
            resident.append((torch.from_numpy(t1).cuda(), torch.from_numpy(t2).cuda(), any(p.noise is not None for p in params)))

        def launches(i):
            t1, t2, noisy = resident[i % len(resident)]
            hip.augment_crop(dframes, dlabels, ws["tmp"], ws["crop"], ws["label_crop"], t1, aug.ksize)
            if noisy:
                hip.augment_noise(ws["crop"], t2, thr, k_min)
            hip.augment_finish(ws["crop"], ws["label_crop"], out[0], out[1], t2, lut, label_lut)

        return timed_windows(launches)

    def timed_windows(fn, reps=a.reps):
        for i in range(16):
            fn(i)
        sync()
        windows = []
        for _ in range(a.windows):                   # several windows of `reps` batches: the median is reported, the range shows the spread
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                fn(i)
            e1.record()
            sync()
            windows.append(e0.elapsed_time(e1) * 1e3 / reps)
        return windows

    def call_ms(sets):
        for i in range(8):
            aug(dframes, dlabels, sets[i % len(sets)], out=out)
        sync()
        t0 = time.perf_counter()
        for i in range(a.reps):
            aug(dframes, dlabels, sets[i % len(sets)], out=out)
        sync()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    windows = device_windows(sets)
    device_us = float(np.median(windows))

    # host: drawing and table building
    host_windows = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            aug.tables(aug.sample(B, rng=rng, gen=gen))
        host_windows.append((time.perf_counter() - t0) * 1e3 / a.reps)
    host_ms = float(np.median(host_windows))

    # the whole call
    whole_ms = call_ms(sets)

    t1, t2 = aug.tables(sets[0])
    res = {"config": {"batch": B, "frames": T, "source": list(hw), "crop": list(aug.crop), "base_w": aug.base_w, "ksize": aug.ksize,
                      "reps": a.reps, "p_noise": a.p_noise,
                      "parameter_sets": [[p.long_size, p.x1, p.y1, int(p.hflip), int(p.vflip), p.alpha is not None,
                                          p.angle is not None, p.noise is not None] for p in sets[0]]},
           "device_us_per_batch": round(device_us, 2), "device_us_range": [round(min(windows), 2), round(max(windows), 2)],
           "host_ms_per_batch": round(host_ms, 3), "host_ms_range": [round(min(host_windows), 3), round(max(host_windows), 3)], "call_ms_per_batch": round(whole_ms, 3),
           "upload_bytes_per_batch": int(frames.nbytes + labels.nbytes + t1.nbytes + t2.nbytes),
           "reference_upload_bytes_per_batch": int(B * T * 3 * hw[0] * hw[1] * 8 + B * 12 * hw[0] * hw[1] * 8)}
    if a.p_noise:
        res["noisy_samples"] = [sum(p.noise is not None for p in params) for params in sets]
        quiet = [[ClipParams(**{**p.__dict__, "noise": None}) for p in params] for params in sets]
        quiet_windows = device_windows(quiet)
        res["no_noise"] = {"device_us_per_batch": round(float(np.median(quiet_windows)), 2),
                           "device_us_range": [round(min(quiet_windows), 2), round(max(quiet_windows), 2)],
                           "call_ms_per_batch": round(call_ms(quiet), 3)}
        # the noise launch alone, every clip noisy.  cold: a ring of crop buffers larger than the Infinity Cache, every launch on the
        # next one, so that its bytes come from and go to HBM; warm: one buffer, which stays in the cache
        crop_bytes = ws["crop"].numel()
        _, t2 = aug.tables([ClipParams(**{**p.__dict__, "noise": 1 + b}) for b, p in enumerate(sets[0])])
        t2 = torch.from_numpy(t2).cuda()
        ring = [torch.randint(0, 256, ws["crop"].shape, dtype=torch.uint8, device="cuda") for _ in range(L3_BYTES * 3 // 2 // crop_bytes + 1)]
        res["noise"] = {"bytes_read_and_written": 2 * crop_bytes, "ring_buffers": len(ring)}
        for name, bufs in (("cold", ring), ("warm", ring[:1])):
            w = timed_windows(lambda i: hip.augment_noise(bufs[i % len(bufs)], t2, thr, k_min), reps=max(len(ring) * 4, a.reps // 4))
            us = float(np.median(w))
            res["noise"][name] = {"device_us_per_launch": round(us, 2), "device_us_range": [round(min(w), 2), round(max(w), 2)],
                                  "tb_per_s": round(2 * crop_bytes / us / 1e6, 3)}
        del ring
    if not a.no_host_pipeline:
        n = 0
        t0 = time.perf_counter()
        for k in range(a.host_batches):
            params = sets[k % len(sets)]
            for b, p in enumerate(params):
                crops, lab = ar.scale_crop_pillow(frames[b], labels[b], p, aug.crop)
                crops, lab = ar.rotate(crops, lab, p.angle, ar.value_table(p.alpha, p.beta))
                ar.to_float(crops), ar.label_table()[lab]
            n += 1
        res["pillow_numpy_host_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3 / n, 1)
    if a.step_json:
        with open(a.step_json) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        step = json.loads(line)
        step_ms = float(step["ms_per_step"])
        res["step_ms"] = round(step_ms, 3)
        res["step_metric"] = step.get("metric")
        res["augment_ms_per_batch"] = round(device_us / 1e3 + host_ms, 3)
        res["ratio"] = round((device_us / 1e3 + host_ms) / step_ms, 4)
        res["below_step"] = bool(device_us / 1e3 + host_ms < step_ms)
    text = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    if a.step_json and not res["below_step"]:
        raise SystemExit(f"FAIL: the augmenter takes {res['augment_ms_per_batch']} ms per batch, the training step {res['step_ms']} ms: "
                         "the input, not the step, would bound training")


if __name__ == "__main__":
    main()
