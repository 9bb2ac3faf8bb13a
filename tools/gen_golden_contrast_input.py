#!/usr/bin/env python3
"""Record tests/golden/resized_crop_coord.npz: what the reference's RandomResizedCropCoord + RandomHorizontalFlipCoord
(pixcontrast_18/contrast/data/transform_coord.py) draw for the six views of a sample, seed by seed.

    python tools/gen_golden_contrast_input.py --reference /path/to/reference

The reference module is imported from its file, at generation time only, with a stub `torchvision` in sys.modules (torchvision is
not a dependency; the stub's resized_crop / hflip record their arguments instead of touching pixels) and with its `random` name bound
to a counting wrapper around a random.Random(seed).  The fixture holds numbers only:

    <case>/source, out, scale, ratio      the transform's configuration
    <case>/seeds     [N]                  random.Random(seed)
    <case>/ijhw      [N][6][4]  int32     i, j, h, w per view, views in the dataset's order (transform[0] .. transform[5])
    <case>/flip      [N][6]     bool
    <case>/coord     [N][6][4]  float32   the `coord` tensor after the flip
    <case>/attempts  [N][6]     int32     (scale, ratio) pairs drawn by get_params
    <case>/fallback  [N][6]     bool      ten rejections: the central crop, no randint drawn
    <case>/check     [N]        uint32    getrandbits(32) of the generator after the six views: the stream position

Cases: `default` (270 x 480, scale (0.09, 0.49): some attempts are rejected, the fallback is never reached) and `wide` (40 x 200: the
fallback is reached)."""
from __future__ import annotations

import argparse
import importlib.util
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"default": dict(source=(270, 480), out=(256, 448), scale=(0.09, 0.49), ratio=(3. / 4., 4. / 3.), seeds=range(300)),
         "wide": dict(source=(40, 200), out=(16, 32), scale=(0.09, 0.49), ratio=(3. / 4., 4. / 3.), seeds=range(300))}


class CountingRandom:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.uniforms = self.randints = 0

    def uniform(self, a, b):
        self.uniforms += 1
        return self.rng.uniform(a, b)

    def randint(self, a, b):
        self.randints += 1
        return self.rng.randint(a, b)

    def random(self):
        return self.rng.random()


def load_reference(ref: str, calls: list):
    from PIL import Image
    fn = types.ModuleType("torchvision.transforms.functional")
    fn._is_pil_image = lambda img: isinstance(img, Image.Image)
    fn.resized_crop = lambda img, i, j, h, w, size, interpolation: calls.append(("crop", i, j, h, w)) or img
    fn.hflip = lambda img: calls.append(("hflip",)) or img
    tr = types.ModuleType("torchvision.transforms")
    tr.functional = fn
    tv = types.ModuleType("torchvision")
    tv.transforms = tr
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional")}
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})
    try:
        path = os.path.join(ref, "pixcontrast_18", "contrast", "data", "transform_coord.py")
        spec = importlib.util.spec_from_file_location("_reference_transform_coord", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def record(tc, calls, case):
    from PIL import Image
    (Hs, Ws), (H, W) = case["source"], case["out"]
    img = Image.new("RGB", (Ws, Hs))
    lab = Image.new("L", (Ws, Hs))
    seeds = list(case["seeds"])
    n = len(seeds)
    ijhw, flip = np.zeros((n, 6, 4), np.int32), np.zeros((n, 6), bool)
    coord, attempts = np.zeros((n, 6, 4), np.float32), np.zeros((n, 6), np.int32)
    fallback, check = np.zeros((n, 6), bool), np.zeros(n, np.uint32)
    for s, seed in enumerate(seeds):
        tc.random = rng = CountingRandom(seed)
        for v in range(6):                                       # one Compose per view, as get_transform builds them
            crop = tc.RandomResizedCropCoord(H, W, scale=case["scale"], ratio=case["ratio"])
            flipper = tc.RandomHorizontalFlipCoord()
            del calls[:]
            u0, r0 = rng.uniforms, rng.randints
            out = crop(img, img, img, img, lab)
            out = flipper(*out)
            crops = [c for c in calls if c[0] == "crop"]
            assert len(crops) == 5 and len(set(crops)) == 1
            ijhw[s, v] = crops[0][1:]
            flip[s, v] = any(c[0] == "hflip" for c in calls)
            coord[s, v] = out[5].numpy()
            attempts[s, v] = (rng.uniforms - u0) // 2
            fallback[s, v] = rng.randints == r0
        check[s] = rng.rng.getrandbits(32)
    return dict(source=np.array(case["source"]), out=np.array(case["out"]), scale=np.array(case["scale"], np.float64),
                ratio=np.array(case["ratio"], np.float64), seeds=np.array(seeds), ijhw=ijhw, flip=flip, coord=coord, attempts=attempts,
                fallback=fallback, check=check)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds pixcontrast_18/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "resized_crop_coord.npz"))
    a = ap.parse_args()
    calls = []
    tc = load_reference(a.reference, calls)
    arrays = {}
    for name, case in CASES.items():
        rec = record(tc, calls, case)
        print(f"{name}: {len(rec['seeds'])} seeds, views with rejected attempts {int((rec['attempts'] > 1).sum())}, "
              f"fallbacks {int(rec['fallback'].sum())}, flips {int(rec['flip'].sum())}")
        arrays.update({f"{name}/{k}": v for k, v in rec.items()})
    assert (arrays["default/attempts"] > 1).any() and not arrays["default/fallback"].any() and arrays["wide/fallback"].any()
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
