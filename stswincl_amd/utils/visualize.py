"""Host helpers of the colour overlay (hip.labels_overlay, VideoSegmenter(out="overlay")): palettes and the uint8 [256][4] table
the kernel reads.  numpy only, no GPU needed.

The kernel's definition, per pixel and channel (include/stswin_hip.h, stswin_labels_overlay): with s the frame byte and (c, a) =
table[label] the label's colour and alpha,

    out = (a * c + (255 - a) * s + 127) // 255

so alpha 255 paints the colour, alpha 0 passes the frame through, both exactly.

The reference draws its pictures on the host: seg18/test.py:162-169 (label2rgb + imsave) and
segcata/utils/cadis_visualization.py:86-113 (get_remapped_colormap, mask_to_colormap).  This module ships no dataset palette: a CaDIS
user passes what their checkout's get_remapped_colormap(class_remapping) returns to palette_from_colormap()."""
from __future__ import annotations

from typing import Iterable, Mapping, Optional

import numpy as np


def default_palette() -> np.ndarray:
    """uint8 [256][3], the project's palette: the bit-interleave colormap.  Label i gives its bits 0, 1, 2 to the top bit of r, g, b,
    its bits 3, 4, 5 to the next lower bit, and so on:

        r = sum_j bit(i, 3 j)     << (7 - j)
        g = sum_j bit(i, 3 j + 1) << (7 - j)
        b = sum_j bit(i, 3 j + 2) << (7 - j)        j = 0, 1, 2

    (8 bits of i: j stops at 2, where only r and g still receive a bit).  The map label -> (r, g, b) is injective: 256 distinct
    colours, label 0 black."""
    i = np.arange(256, dtype=np.int64)
    pal = np.zeros((256, 3), dtype=np.int64)
    for j in range(3):
        for ch in range(3):
            pal[:, ch] |= ((i >> (3 * j + ch)) & 1) << (7 - j)
    return pal.astype(np.uint8)


def palette_from_colormap(mapping) -> np.ndarray:
    """uint8 [k][3] palette from a {label: (r, g, b)} dict (the form the reference's get_remapped_colormap returns; k = largest label
    + 1, so a 255 key gives 256 rows; labels the dict lacks are black) or from an [n][3] array."""
    if isinstance(mapping, Mapping):
        if not mapping:
            raise ValueError("palette_from_colormap: an empty colormap")
        keys = [int(k) for k in mapping]
        if min(keys) < 0 or max(keys) > 255:
            raise ValueError(f"palette_from_colormap: labels must be 0 .. 255, got {min(keys)} .. {max(keys)}")
        pal = np.zeros((max(keys) + 1, 3), dtype=np.uint8)
        for k, color in mapping.items():
            pal[int(k)] = _color(color)
        return pal
    arr = np.asarray(mapping)
    if arr.ndim != 2 or arr.shape[1] != 3 or not 1 <= arr.shape[0] <= 256:
        raise ValueError(f"palette_from_colormap: expected a dict or an [n][3] array with n <= 256, got shape {arr.shape}")
    return np.stack([_color(c) for c in arr])


def _color(color) -> np.ndarray:
    c = np.asarray(color)
    if c.shape != (3,) or (c < 0).any() or (c > 255).any() or (c != np.floor(c)).any():
        raise ValueError(f"a colour is three integers 0 .. 255, got {color!r}")
    return c.astype(np.uint8)


def overlay_table(palette, alpha: int = 128, transparent: Iterable[int] = (), alphas: Optional[Mapping[int, int]] = None) -> np.ndarray:
    """uint8 [256][4] = (r, g, b, a) per label value: the palette's colours with `alpha`; `transparent` labels get alpha 0 (the frame
    shows through), `alphas` {label: alpha} overrides single labels (after `transparent`), and labels beyond the palette are
    (0, 0, 0, 0)."""
    pal = palette_from_colormap(palette)
    table = np.zeros((256, 4), dtype=np.uint8)
    table[:len(pal), :3] = pal
    table[:len(pal), 3] = _alpha(alpha)
    for lab in transparent:
        table[_label(lab), 3] = 0
    for lab, a in (alphas or {}).items():
        table[_label(lab), 3] = _alpha(a)
    return table


def _alpha(a) -> int:
    if int(a) != a or not 0 <= a <= 255:
        raise ValueError(f"an alpha is an integer 0 .. 255, got {a!r}")
    return int(a)


def _label(lab) -> int:
    if int(lab) != lab or not 0 <= lab <= 255:
        raise ValueError(f"a label is an integer 0 .. 255, got {lab!r}")
    return int(lab)


def mask_to_colormap(mask: np.ndarray, colormap: Mapping) -> np.ndarray:
    """RGB picture uint8 [H][W][3] of a label mask [H][W] under a {label: (r, g, b)} dict, with the semantics of the reference's
    function of the same name (cadis_visualization.py:103-113): a pixel takes the colour of the key equal to its value, black where
    no key is.  A host convenience and the tests' reference; on the GPU the same picture is hip.labels_overlay with alpha 255."""
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError(f"mask_to_colormap: mask must be [H][W], got shape {mask.shape}")
    values, index = np.unique(mask, return_inverse=True)
    colors = np.zeros((len(values), 3), dtype=np.uint8)
    for i, v in enumerate(values.tolist()):
        if v in colormap:
            colors[i] = _color(colormap[v])
    return colors[index.reshape(mask.shape)]
