#!/usr/bin/env python3
"""Record tests/golden/overlay_colormap.npz: what the reference's segcata/utils/cadis_visualization.py makes of a seeded synthetic
CaDIS mask under each of its three experiments.

    python tools/gen_golden_overlay.py --reference /path/to/reference

The reference module is imported from its file, at generation time only, with empty stub modules for `cv2` and `albumentations`
where they are not installed (it imports them for its plotting functions; nothing recorded here calls them).  The fixture holds
numbers only:

    mask                  [24][40]    uint8   values 0 .. 35 and 255, seed 0
    exp<k>/remapped       [24][40]    uint8   remap_experiment<k>(mask)[0]
    exp<k>/keys           [n]         int32   the colormap dict remap_experiment<k> returns, in the dict's order ...
    exp<k>/colors         [n][3]      uint8   ... and its colours
    exp<k>/rgb            [24][40][3] uint8   mask_to_colormap(remapped, colormap)

for k = 1, 2, 3."""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (24, 40)


def synthetic_mask(seed: int = 0) -> np.ndarray:
    """Every CaDIS class 0 .. 35 and the ignore value 255 at least once, the rest drawn with a bias to 255 so that it is not rare."""
    rng = np.random.RandomState(seed)
    values = np.concatenate([np.arange(36), [255]])
    flat = rng.choice(values, size=SHAPE[0] * SHAPE[1], p=np.concatenate([np.full(36, 0.9 / 36), [0.1]]))
    flat[rng.permutation(flat.size)[:len(values)]] = values
    return flat.reshape(SHAPE).astype(np.uint8)


def load_reference(ref: str):
    stubs = {}
    for name in ("cv2", "albumentations"):
        try:
            importlib.import_module(name)
        except ImportError:
            stubs[name] = types.ModuleType(name)
    sys.modules.update(stubs)
    try:
        path = os.path.join(ref, "segcata", "utils", "cadis_visualization.py")
        spec = importlib.util.spec_from_file_location("_reference_cadis_visualization", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name in stubs:
            sys.modules.pop(name, None)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds segcata/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "overlay_colormap.npz"))
    a = ap.parse_args()
    cv = load_reference(a.reference)
    mask = synthetic_mask()
    assert set(np.unique(mask).tolist()) == set(range(36)) | {255}
    arrays = {"mask": mask}
    for k in (1, 2, 3):
        # (int64 input: the reference sizes its remap array by mask.max() + 1, which wraps in uint8)
        remapped, _, colormap = getattr(cv, f"remap_experiment{k}")(mask.astype(np.int64))
        rgb = cv.mask_to_colormap(remapped, colormap)
        keys = np.array([int(key) for key in colormap], dtype=np.int32)
        colors = np.array([np.asarray(c) for c in colormap.values()], dtype=np.int64)
        assert remapped.shape == SHAPE and rgb.shape == SHAPE + (3,) and rgb.dtype == np.uint8
        assert colors.min() >= 0 and colors.max() <= 255
        arrays.update({f"exp{k}/remapped": remapped.astype(np.uint8), f"exp{k}/keys": keys, f"exp{k}/colors": colors.astype(np.uint8),
                       f"exp{k}/rgb": rgb})
        print(f"experiment {k}: {len(keys)} colormap keys {keys.tolist()}, remapped values {np.unique(remapped).tolist()}")
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
