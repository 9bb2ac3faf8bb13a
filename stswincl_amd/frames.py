"""What every uint8-frame input path shares (video.py, augment.py, contrast/views.py): the clip length and the protocols' names, the
value tables, Pillow's BILINEAR coefficients, their per-device caches (module state: one copy) and the pinned staging buffers."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .hip import StswinHipError

T = 4                   # frames per clip (the model asserts T == 4)
RULES = ("endovis18", "cadis")


def check_rule(rule: str) -> None:
    if rule not in RULES:
        raise StswinHipError(f"clip rule must be one of {RULES}, got {rule!r}")


# float32(u / 255.) of the reference (astype(float) / 255., then .float()): equal to the fp32 division u / 255.f for all 256 values,
# not to u * (1 / 255.f) (126 differ)
VALUE_TABLE = (np.arange(256, dtype=np.float64) / 255.).astype(np.float32)
PRECISION_BITS = 22

# CaDIS (CATA_new_512.py:21-22, 228-229): float32 MEAN / STD arrays, `imgs / 255.` in float64, `(imgs - mean) / std` promoted to
# float64, `.float()` at cata_test.py:125
CADIS_MEAN = np.array([0.40789654, 0.44719302, 0.47026115], dtype=np.float32)
CADIS_STD = np.array([0.28863828, 0.27408164, 0.27809835], dtype=np.float32)
CADIS_SIZE = (540, 960)   # the CaDIS frames' size, which cata_test.py:129 resizes the logits back to


def cadis_value_table() -> np.ndarray:
    """fp32 [3][256]: the CaDIS value of byte u in RGB plane c, computed in float64 as the reference does, then cast."""
    u = np.arange(256, dtype=np.float64) / 255.
    return ((u[None, :] - CADIS_MEAN.astype(np.float64)[:, None]) / CADIS_STD.astype(np.float64)[:, None]).astype(np.float32)


def bilinear_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's BILINEAR coefficients for one axis (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc), in float64:
    -> (bounds int32 [out][2] = (first tap, taps), weights int32 [out][ksize] with 22 fraction bits)."""
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = fs                                            # the triangle filter's support is 1
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5), in_size).astype(np.int64)
    n = xmax - xmin
    x = np.arange(ksize)
    t = np.abs((x[None, :] + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs))
    w = np.where((t < 1.0) & (x[None, :] < n[:, None]), 1.0 - t, 0.0)
    ww = np.zeros(out_size)
    for k in range(ksize):                                   # the sequential float64 sum of the C loop
        ww += w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.trunc(np.where(w < 0, -0.5, 0.5) + w * (1 << PRECISION_BITS)).astype(np.int32)
    return np.stack([xmin, n], 1).astype(np.int32), np.ascontiguousarray(kk)


_TABLES = {}            # (in, out, device) -> (bounds, weights) on the device
_LUTS = {}


def tables(in_size: int, out_size: int, device):
    key = (in_size, out_size, str(device))
    tab = _TABLES.get(key)
    if tab is None:
        b, k = bilinear_coeffs(in_size, out_size)
        assert int((b[:, 0] + b[:, 1]).max()) <= in_size and int(b[:, 0].min()) >= 0
        tab = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device))
        _TABLES[key] = tab
    return tab


def value_lut(device, protocol: str = "endovis18"):
    """The value table of a protocol on a device: a persistent tensor (a captured graph reads it)."""
    key = (protocol, str(device))
    t = _LUTS.get(key)
    if t is None:
        t = _LUTS[key] = torch.from_numpy(cadis_value_table() if protocol == "cadis" else VALUE_TABLE).to(device)
    return t


class Pinned:
    """Pinned host staging buffers for host -> device copies that do not block the host: a buffer is reused only after the copy
    that last read it has run (its event)."""

    def __init__(self, count: int = 4):
        self.bufs = [None] * count
        self.events = [None] * count
        self.i = 0

    def upload(self, arr: np.ndarray, dst: torch.Tensor) -> torch.Tensor:
        i = self.i = (self.i + 1) % len(self.bufs)
        if self.events[i] is not None:
            self.events[i].synchronize()
        flat = np.ascontiguousarray(arr).reshape(-1)
        buf = self.bufs[i]
        if buf is None or buf.numel() < flat.nbytes:
            buf = self.bufs[i] = torch.empty(flat.nbytes, dtype=torch.uint8).pin_memory()
        buf[:flat.nbytes].numpy().view(flat.dtype)[:] = flat
        dst.view(torch.uint8).view(-1).copy_(buf[:flat.nbytes], non_blocking=True)
        ev = self.events[i] = torch.cuda.Event()
        ev.record()
        return dst
