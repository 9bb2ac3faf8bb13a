"""Contrastive pre-training input: build the six views on the GPU from uint8 frames.

The reference's `pretrainDataset.__getitem__` (pixcontrast_18/contrast/data/dataset.py:43-70) runs six `RandomResizedCropCoord +
RandomHorizontalFlipCoord + ToTensor + Normalize` pipelines (contrast/data/transform.py:20-87, transform_coord.py:81-224) per sample
on the host - 24 Pillow BILINEAR and 6 NEAREST resizes - and ships 24 fp32 frames.  ContrastViews takes the sample as the dataset
loads it, 17 distinct uint8 frames and 6 uint8 labels at the source size, and returns what `ConsistencyLoss.forward` receives:

    cv = ContrastViews()                                             # 270 x 480 -> 256 x 448
    params = cv.sample(B, rng=random.Random(seed))                   # B x 6 ViewParams, the reference's draws in its order
    views = cv(frames_u8, labels_u8, params)                         # (im_1 .. im_6, mask_1 .. mask_6), or out=: static buffers
    loss = model(*views)

Frame order of a sample (uint8 [17][Hs][Ws][3]): `image, prev1, prev2, prev3, prev4`, then for each of the three negatives
`neg, p1, p2, p3` - `_load_data`'s return order without the duplicate `image_v`.  DEFAULT_FRAME_MAP gives each view's four frames in
the order `append_img_1` stacks them (oldest first).  Label order (uint8 [6][Hs][Ws]): `label, label_v, label_1, label_neg1,
label_neg2, label_neg3`, the dataset's return order.  A caller with another layout passes its own frame_map / label_map.

What is exact: the crop + BILINEAR / NEAREST resize (Pillow bit for bit), the flip, the value table (value_table(): torch CPU fp32
arithmetic, the definition of ToTensor + Normalize), and the random stream - with the `random` state the reference has after
`get_neg`'s draws (which stay on the dataset side), sample() returns the reference's crops, flips and `coord`.
"""
from __future__ import annotations

import functools
import math
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..frames import PRECISION_BITS, Pinned, T, bilinear_coeffs
from ..augment import bilinear_ksize, nearest_index
from ..hip import StswinHipError

VIEWS = 6
MAX_KSIZE = 16          # taps per output index the library's tables hold (include/stswin_hip.h, stswin_contrast_views)
_ONE = 1 << PRECISION_BITS
_HEAD = 8

# dataset.py:56-68: view k is transform[k] over four frames, stacked by append_img_1 oldest first.  Frames: 0 image, 1 .. 4 prev1 ..
# prev4, 5 .. 8 neg1 + its three predecessors, 9 .. 12 neg2's, 13 .. 16 neg3's.
DEFAULT_FRAME_MAP = ((3, 2, 1, 0), (3, 2, 1, 0), (4, 3, 2, 1), (8, 7, 6, 5), (12, 11, 10, 9), (16, 15, 14, 13))
DEFAULT_LABEL_MAP = (0, 1, 2, 3, 4, 5)


@dataclass
class ViewParams:
    """One view's transform: the crop rows [i, i + h) x columns [j, j + w) of the source, the flips, and the reference's `coord`
    (fp32 [4]: x0, y0, x1, y1 of the crop in [0, 1], x0 and x2 swapped by a horizontal flip)."""
    i: int
    j: int
    h: int
    w: int
    hflip: bool = False
    vflip: bool = False
    coord: Optional[np.ndarray] = None


def value_table(mean: Sequence[float] = (0.485, 0.456, 0.406), std: Sequence[float] = (0.229, 0.224, 0.225)) -> np.ndarray:
    """fp32 [3][256]: the value of byte u in plane c after ToTensor and Normalize, in fp32 steps evaluated with torch's CPU ops:
    ((float32(u) / float32(255)) - float32(mean[c])) / float32(std[c]).  ToTensor is `.to(float32).div(255)`, Normalize is
    `.sub_(mean).div_(std)` with fp32 mean / std tensors; torchvision is not a dependency, so this derivation is the definition.
    NOT frames.cadis_value_table(), which follows a float64 pipeline."""
    u = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    m = torch.as_tensor(list(mean), dtype=torch.float32)
    s = torch.as_tensor(list(std), dtype=torch.float32)
    if m.numel() != 3 or s.numel() != 3:
        raise StswinHipError(f"mean and std must have one value per RGB plane, got {tuple(mean)} and {tuple(std)}")
    return u[None, :].repeat(3, 1).sub_(m[:, None]).div_(s[:, None]).numpy()


@functools.lru_cache(maxsize=4096)
def _axis(length: int, out_size: int):
    """Tables of an axis of `length` source pixels resized to out_size, relative to the crop's origin: (bounds [out][2], weights
    [out][k], nearest [out]).  Pillow skips the pass of an unscaled axis: one tap of weight 2^22."""
    if length == out_size:
        idx = np.arange(out_size, dtype=np.int32)
        b, k, near = np.stack([idx, np.ones_like(idx)], 1), np.full((out_size, 1), _ONE, np.int32), idx
    else:
        b, k = bilinear_coeffs(length, out_size)
        near = nearest_index(length, out_size).astype(np.int32)
    for a in (b, k, near):
        a.setflags(write=False)
    return b, k, near


def axis_tables(offset: int, length: int, out_size: int, ksize: int):
    """The tables of source pixels [offset, offset + length) resized to out_size, in source coordinates: (bounds int32 [out][2],
    weights int32 [out][ksize], nearest int32 [out])."""
    b, k, near = _axis(int(length), int(out_size))
    if k.shape[1] > ksize:
        raise StswinHipError(f"scale {length} -> {out_size} needs {k.shape[1]} taps, the tables hold {ksize}")
    bounds = b.copy()
    bounds[:, 0] += offset
    coef = np.zeros((out_size, ksize), np.int32)
    coef[:, :k.shape[1]] = k
    return bounds, coef, near + np.int32(offset)


class ContrastViews:
    """cv = ContrastViews(out=(256, 448), source=(270, 480), scale=(0.09, 0.49), ratio=(3/4, 4/3), hflip_p=0.5, mean=..., std=...,
                          frame_map=DEFAULT_FRAME_MAP, label_map=DEFAULT_LABEL_MAP)

    sample(B, rng) draws B x 6 ViewParams; params(i, j, h, w, hflip, vflip) makes one explicitly; identity() is the whole source.
    cv(frames, labels, params, out=None): uint8 frames [B][NF][Hs][Ws][3] and uint8 labels [B][NL][Hs][Ws] on the GPU (NF = 17 and
    NL = 6 with the default maps) -> (im_1 .. im_6, mask_1 .. mask_6): fp32 images [B][4][3][H][W] and fp32 masks [B][1][H][W], the
    arguments of ConsistencyLoss.forward in its order.  They are views of two view-major buffers, images [6][B][4][3][H][W] and
    masks [6][B][1][H][W]; out=(images, masks) writes into given ones and, after the first call for a batch size, allocates nothing:
    the form for GraphedStep's before_step.  Two launches and one pinned upload of the tables per batch, on the current stream, no
    synchronisation.

    Refuses (StswinHipError): CPU tensors, a wrong dtype, shape or device, fewer frames or labels than the maps index, a crop
    outside the source, a source / output pair that needs more taps than the tables hold."""

    def __init__(self, out: Sequence[int] = (256, 448), source: Sequence[int] = (270, 480), scale: Sequence[float] = (0.09, 0.49),
                 ratio: Sequence[float] = (3. / 4., 4. / 3.), hflip_p: float = 0.5, mean: Sequence[float] = (0.485, 0.456, 0.406),
                 std: Sequence[float] = (0.229, 0.224, 0.225), frame_map=DEFAULT_FRAME_MAP, label_map=DEFAULT_LABEL_MAP):
        self.out = (int(out[0]), int(out[1]))
        self.source = (int(source[0]), int(source[1]))
        if min(self.out) < 1 or min(self.source) < 1:
            raise StswinHipError(f"out and source must be positive (H, W) sizes, got {tuple(out)} and {tuple(source)}")
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.hflip_p = float(hflip_p)
        self.frame_map = np.asarray(frame_map, dtype=np.int64)
        self.label_map = np.asarray(label_map, dtype=np.int64)
        if self.frame_map.ndim != 2 or self.frame_map.shape[1] != T or self.label_map.shape != (self.frame_map.shape[0],):
            raise StswinHipError(f"frame_map must be [views][{T}] frame indices and label_map [views] label indices, got shapes "
                                 f"{self.frame_map.shape} and {self.label_map.shape}")
        if self.frame_map.min() < 0 or self.label_map.min() < 0:
            raise StswinHipError("frame_map and label_map hold indices into a sample's frames and labels: none may be negative")
        self.views = self.frame_map.shape[0]
        self.n_frames = int(self.frame_map.max()) + 1
        self.n_labels = int(self.label_map.max()) + 1
        self.ksize = max(bilinear_ksize(self.source[0], self.out[0]), bilinear_ksize(self.source[1], self.out[1]))  # the most taps any crop needs
        if self.ksize > MAX_KSIZE:
            raise StswinHipError(f"source {self.source} -> out {self.out} needs {self.ksize} taps per output pixel, the tables hold "
                                 f"{MAX_KSIZE}: resize the source on the host first")
        self.table = value_table(mean, std)
        self._ws = {}
        self._luts = {}
        self._pinned = Pinned()

    # ----------------------------------------------------------------------------------------- parameters
    def _coord(self, i: int, j: int, h: int, w: int, hflip: bool, vflip: bool) -> np.ndarray:
        height, width = self.source
        c = [float(j) / (width - 1), float(i) / (height - 1), float(j + w - 1) / (width - 1), float(i + h - 1) / (height - 1)] \
            if width > 1 and height > 1 else [0.0, 0.0, 0.0, 0.0]
        if hflip:
            c[0], c[2] = c[2], c[0]
        if vflip:
            c[1], c[3] = c[3], c[1]
        return np.asarray(c, dtype=np.float32)

    def check(self, p: ViewParams) -> ViewParams:
        (Hs, Ws) = self.source
        if not (p.h >= 1 and p.w >= 1 and 0 <= p.i and p.i + p.h <= Hs and 0 <= p.j and p.j + p.w <= Ws):
            raise StswinHipError(f"the crop must lie inside the source {Hs} x {Ws}: 0 <= i, i + h <= {Hs}, 0 <= j, j + w <= {Ws}, h, w >= 1; "
                                 f"got i = {p.i}, j = {p.j}, h = {p.h}, w = {p.w}")
        return p

    def params(self, i: int, j: int, h: int, w: int, hflip: bool = False, vflip: bool = False) -> ViewParams:
        i, j, h, w, hflip, vflip = int(i), int(j), int(h), int(w), bool(hflip), bool(vflip)
        return self.check(ViewParams(i, j, h, w, hflip, vflip, self._coord(i, j, h, w, hflip, vflip)))

    def identity(self) -> ViewParams:
        """The whole source, resized to the output size, no flip."""
        return self.params(0, 0, *self.source)

    def _draw(self, rng) -> ViewParams:
        height, width = self.source
        area = height * width
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            target = rng.uniform(*self.scale) * area
            aspect = math.exp(rng.uniform(*log_ratio))
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= width and 0 < h <= height:
                i = rng.randint(0, height - h)
                j = rng.randint(0, width - w)
                break
        else:                                                   # ten rejections: the central crop of the nearest allowed ratio
            in_ratio = float(width) / float(height)
            if in_ratio < min(self.ratio):
                w = width
                h = int(round(w / min(self.ratio)))
            elif in_ratio > max(self.ratio):
                h = height
                w = int(round(h * max(self.ratio)))
            else:
                w, h = width, height
            i, j = (height - h) // 2, (width - w) // 2
        hflip = rng.random() < self.hflip_p
        return ViewParams(i, j, h, w, hflip, False, self._coord(i, j, h, w, hflip, False))

    def sample(self, B: int, rng: Optional[random.Random] = None) -> List[List[ViewParams]]:
        """B samples x `views` ViewParams, drawn from rng (a random.Random; default: the `random` module, as the reference) with
        RandomResizedCropCoord.get_params' calls in its order - per attempt uniform(*scale), uniform(*log_ratio); on acceptance
        randint(0, height - h), randint(0, width - w); after ten rejections the central-crop fallback, no draw - then one
        random() < hflip_p for the flip; view after view, sample after sample, as the dataset calls transform[0] .. transform[5].
        The dataset's `get_neg` draws (one sample(), three randint) precede each sample's views and stay with the dataset: from the
        `random` state the reference has after get_neg, one sample's parameters equal the reference's."""
        rng = random if rng is None else rng
        return [[self._draw(rng) for _ in range(self.views)] for _ in range(B)]

    # ----------------------------------------------------------------------------------------- host tables
    def view_tables(self, p: ViewParams) -> dict:
        """One view's tables (numpy): r0, r1, flags, hbounds, hcoef, vbounds, vcoef, lx, ly, in source coordinates."""
        self.check(p)
        H, W = self.out
        hb, hk, lx = axis_tables(p.j, p.w, W, self.ksize)
        vb, vk, ly = axis_tables(p.i, p.h, H, self.ksize)
        return dict(r0=int(vb[:, 0].min()), r1=int((vb[:, 0] + vb[:, 1]).max()), flags=(1 if p.hflip else 0) | (2 if p.vflip else 0),
                    hbounds=hb, hcoef=hk, vbounds=vb, vcoef=vk, lx=lx, ly=ly)

    def stride(self) -> int:
        """Words per table row, as the library states them."""
        return hip.contrast_views_table_stride(self.out[0], self.out[1], self.ksize)

    def tables(self, params: Sequence[Sequence[ViewParams]], n_frames: Optional[int] = None, n_labels: Optional[int] = None) -> np.ndarray:
        """-> int32 [views * B][stride], view-major (row view * B + sample): the rows of stswin_contrast_views' table, with the frame
        and label indices made global (sample * n_frames + frame_map[view][t], sample * n_labels + label_map[view])."""
        n_frames = self.n_frames if n_frames is None else n_frames
        n_labels = self.n_labels if n_labels is None else n_labels
        B, s = len(params), self.stride()
        tab = np.zeros((self.views * B, s), np.int32)
        for b, sample in enumerate(params):
            if len(sample) != self.views:
                raise StswinHipError(f"params must hold {self.views} ViewParams per sample, sample {b} has {len(sample)}")
            for v, p in enumerate(sample):
                c = self.view_tables(p)
                row = tab[v * B + b]
                row[:4] = (c["r0"], c["r1"], c["flags"], b * n_labels + self.label_map[v])
                row[4:_HEAD] = b * n_frames + self.frame_map[v]
                o = _HEAD
                for k in ("hbounds", "hcoef", "vbounds", "vcoef", "lx", "ly"):
                    row[o:o + c[k].size] = c[k].reshape(-1)
                    o += c[k].size
                if o != s:
                    raise StswinHipError(f"a table row has {o} words, the library expects {s}")
        return tab

    # ----------------------------------------------------------------------------------------- device
    def _workspace(self, B: int, dev):
        key = (B, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            V = self.views * B
            ws = self._ws[key] = dict(table=torch.empty(V, self.stride(), dtype=torch.int32, device=dev),
                                      tmp=torch.empty(V * T * self.source[0] * self.out[1] * 3, dtype=torch.uint8, device=dev))
        return ws

    def _lut(self, dev):
        key = str(dev)
        t = self._luts.get(key)
        if t is None:
            t = self._luts[key] = torch.from_numpy(self.table).to(dev)
        return t

    def _check_inputs(self, frames, labels, params) -> int:
        Hs, Ws = self.source
        form = (f"frames must be contiguous uint8 [B][>= {self.n_frames}][{Hs}][{Ws}][3] and labels contiguous uint8 "
                f"[B][>= {self.n_labels}][{Hs}][{Ws}], both on the GPU")
        for t, what in ((frames, "frames"), (labels, "labels")):
            if not isinstance(t, torch.Tensor):
                raise StswinHipError(f"{form}; got {type(t).__name__} for {what}")
            if not t.is_cuda:
                raise StswinHipError(f"{form}; {what} is on the CPU (there is no CPU path: move the uint8 batch with .cuda())")
            if t.dtype != torch.uint8:
                raise StswinHipError(f"{form}; {what} is {t.dtype}")
            if not t.is_contiguous():
                raise StswinHipError(f"{form}; {what} is not contiguous")
        if frames.dim() != 5 or frames.shape[4] != 3 or tuple(frames.shape[2:4]) != (Hs, Ws):
            raise StswinHipError(f"{form}; frames is {tuple(frames.shape)}")
        B = frames.shape[0]
        if labels.dim() != 4 or labels.shape[0] != B or tuple(labels.shape[2:]) != (Hs, Ws):
            raise StswinHipError(f"{form}; frames is {tuple(frames.shape)} and labels {tuple(labels.shape)}")
        if frames.shape[1] < self.n_frames:
            raise StswinHipError(f"{form}; frame_map indexes frame {self.n_frames - 1} of a sample, frames holds {frames.shape[1]} per sample")
        if labels.shape[1] < self.n_labels:
            raise StswinHipError(f"{form}; label_map indexes label {self.n_labels - 1} of a sample, labels holds {labels.shape[1]} per sample")
        if labels.device != frames.device:
            raise StswinHipError(f"{form}; frames on {frames.device}, labels on {labels.device}")
        if B < 1 or len(params) != B:
            raise StswinHipError(f"params must hold one list of {self.views} ViewParams per sample: {B}, got {len(params)}")
        return B

    def _outputs(self, out, B: int, dev):
        H, W = self.out
        if out is None:
            return (torch.empty(self.views, B, T, 3, H, W, dtype=torch.float32, device=dev),
                    torch.empty(self.views, B, 1, H, W, dtype=torch.float32, device=dev))
        form = f"out must be (contiguous fp32 [{self.views}][{B}][{T}][3][{H}][{W}], contiguous fp32 [{self.views}][{B}][1][{H}][{W}]) on {dev}"
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out):
            raise StswinHipError(form)
        img, msk = out
        if img.dtype != torch.float32 or tuple(img.shape) != (self.views, B, T, 3, H, W) or msk.dtype != torch.float32 or \
                tuple(msk.shape) != (self.views, B, 1, H, W) or not img.is_contiguous() or not msk.is_contiguous() or \
                img.device != dev or msk.device != dev:
            raise StswinHipError(f"{form}; got {img.dtype} {tuple(img.shape)} on {img.device} and {msk.dtype} {tuple(msk.shape)} on {msk.device}")
        return img, msk

    def __call__(self, frames: torch.Tensor, labels: torch.Tensor, params: Sequence[Sequence[ViewParams]], out=None) -> Tuple[torch.Tensor, ...]:
        B = self._check_inputs(frames, labels, params)
        dev = frames.device
        tab = self.tables(params, frames.shape[1], labels.shape[1])
        images, masks = self._outputs(out, B, dev)
        ws = self._workspace(B, dev)
        # one asynchronous copy from pinned memory; calls may follow each other without a synchronise (Pinned waits for the
        # copy that last read a staging buffer before it rewrites it; the device table is rewritten in stream order)
        self._pinned.upload(tab, ws["table"])
        V = self.views * B
        hip.contrast_views(frames.view(-1, *frames.shape[2:]), labels.view(-1, *labels.shape[2:]), ws["tmp"],
                           images.view(V, T, 3, *self.out), masks.view(V, 1, *self.out), ws["table"], self._lut(dev), self.ksize)
        return tuple(images[v] for v in range(self.views)) + tuple(masks[v] for v in range(self.views))
