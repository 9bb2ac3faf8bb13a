"""Ground truth in the form the files hold it: the tables hip.gt_decode and VideoSegmenter(gt_table=...) read, and the numpy
statement of what the kernel computes.  numpy only, no GPU needed.

Two stored forms (include/stswin_hip.h, stswin_gt_decode):

  * colour-coded, uint8 [H][W][3 | 4] (the EndoVis18 test labels, seg18/dataset/Endovis2018_new.py:130-136 with `lb_json`'s colour
    list): a table uint8 [k][4] = (r, g, b, label), k <= 256.  A pixel takes the label of the LAST row whose colour equals its first
    three channels exactly; a fourth channel is not looked at; a pixel that equals no row becomes 0 and is counted as unmatched.
    The reference zeroes such pixels without a word: a labels.json of another dataset or an antialiased mask shows up in the count.
  * id-coded, uint8 [H][W] (the CaDIS labels, segcata/dataset/CATA_new_512.py:97, 237): a table uint8 [256], out = table[u].  One
    table carries both the experiment's remap and the move of the ignore value 255 to the last class.

This module ships no dataset's colours or remap: pass what your checkout's labels.json or class_remapping dictionary holds."""
from __future__ import annotations

from typing import Mapping, Optional, Tuple

import numpy as np


def _byte(v, what: str) -> int:
    if isinstance(v, (bool, np.bool_)) or int(v) != v or not 0 <= v <= 255:
        raise ValueError(f"{what} is an integer 0 .. 255, got {v!r}")
    return int(v)


def colour_table(colours, labels=None) -> np.ndarray:
    """uint8 [k][4] = (r, g, b, label) from a list of k (r, g, b) (labels default to 0 .. k - 1, the position in the list: `lb_json`'s
    colour list as the reference reads it; or pass one label per colour) or from a {label: (r, g, b)} dict in the dict's order.
    1 <= k <= 256.  Where two rows hold one colour the later row decides."""
    if isinstance(colours, Mapping):
        if labels is not None:
            raise ValueError("colour_table: a {label: colour} dict brings its own labels")
        labels, colours = list(colours.keys()), list(colours.values())
    colours = [tuple(np.asarray(c).tolist()) for c in colours]
    if not 1 <= len(colours) <= 256:
        raise ValueError(f"colour_table: 1 .. 256 colours, got {len(colours)}")
    labels = list(range(len(colours))) if labels is None else list(labels)
    if len(labels) != len(colours):
        raise ValueError(f"colour_table: {len(colours)} colours and {len(labels)} labels")
    table = np.zeros((len(colours), 4), dtype=np.uint8)
    for row, (c, lab) in enumerate(zip(colours, labels)):
        if len(c) != 3:
            raise ValueError(f"colour_table: a colour is (r, g, b), got {c!r}")
        table[row] = [_byte(v, "a colour channel") for v in c] + [_byte(lab, "a label")]
    return table


def remap_table(mapping: Mapping, default: int = 0, ignore_to: Optional[int] = None) -> np.ndarray:
    """uint8 [256]: the new value of every raw id.  `mapping` is {raw: new} or {new: [raw, ...]} (the shape of the reference's
    class_remapping dictionaries; a dict with any list, tuple or array value is read this way).  Raw ids the mapping does not name
    become `default`, except 255, which stays 255 (the reference's remap passes the ignore value through).  ignore_to then replaces
    every 255 of the finished table, raw 255 and the ids the mapping sends to 255 alike: ignore_to = class_num - 1 is
    `mask[mask == 255] = class_num - 1` after the remap."""
    table = np.full(256, _byte(default, "default"), dtype=np.uint8)
    table[255] = 255
    grouped = any(isinstance(v, (list, tuple, set, frozenset, np.ndarray)) for v in mapping.values())
    seen = set()
    for key, val in mapping.items():
        raws = (list(val) if isinstance(val, (list, tuple, set, frozenset, np.ndarray)) else [val]) if grouped else [key]
        new = _byte(key if grouped else val, "a new id")
        for raw in raws:
            raw = _byte(raw, "a raw id")
            if raw in seen:
                raise ValueError(f"remap_table: raw id {raw} is mapped twice")
            seen.add(raw)
            table[raw] = new
    if ignore_to is not None:
        table[table == 255] = _byte(ignore_to, "ignore_to")
    return table


def _check_colour_table(table) -> np.ndarray:
    table = np.asarray(table)
    if table.dtype != np.uint8 or table.ndim != 2 or table.shape[1] != 4 or not 1 <= table.shape[0] <= 256:
        raise ValueError(f"a colour table is uint8 [1 .. 256][4], got {table.dtype} {table.shape}")
    return table


def decode_colours(img, table) -> Tuple[np.ndarray, object]:
    """(labels uint8 [...][H][W], unmatched) of colour-coded ground truth uint8 [...][H][W][3 | 4] under a colour_table: the rule at
    the top of this module.  unmatched is the number of pixels that equal no row: an int for one image [H][W][c], an int64 array
    [n] for [n][H][W][c]."""
    table = _check_colour_table(table)
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (3, 4) or img.shape[-1] not in (3, 4):
        raise ValueError(f"decode_colours: img must be uint8 [H][W][3 | 4] or [n][H][W][3 | 4], got {img.dtype} {img.shape}")
    # one 24-bit number per colour; a dict filled in row order keeps the last row of each colour; the image's numbers are then
    # looked up in the sorted distinct ones
    word = lambda a: a[..., 0].astype(np.uint32) | (a[..., 1].astype(np.uint32) << 8) | (a[..., 2].astype(np.uint32) << 16)
    label_of = {int(w): int(lab) for w, lab in zip(word(table), table[:, 3])}
    known = np.array(sorted(label_of), dtype=np.uint32)
    label = np.array([label_of[int(w)] for w in known], dtype=np.uint8)
    if img.shape[-1] == 4 and img.flags.c_contiguous:          # the same number straight from the four bytes
        words = (img.view("<u4")[..., 0] & np.uint32(0xffffff)).astype(np.uint32, copy=False)
    else:
        words = word(img)
    at = np.minimum(np.searchsorted(known, words), len(known) - 1)
    missing = known[at] != words
    labels = label[at]
    labels[missing] = 0
    if img.ndim == 3:
        return labels, int(missing.sum())
    return labels, missing.reshape(img.shape[0], -1).sum(1).astype(np.int64)


def decode_ids(img, table) -> np.ndarray:
    """labels uint8 = table[img] of id-coded ground truth uint8 [...] under a remap_table."""
    table, img = np.asarray(table), np.asarray(img)
    if table.dtype != np.uint8 or table.shape != (256,):
        raise ValueError(f"a remap table is uint8 [256], got {table.dtype} {table.shape}")
    if img.dtype != np.uint8:
        raise ValueError(f"decode_ids: img must be uint8, got {img.dtype}")
    return table[img]
