"""Training input: augment uint8 clips and labels on the GPU.

The reference's training `__getitem__` (seg18/dataset/Endovis2018_new.py:61-107, 145-182; segcata/dataset/CATA_new_512.py:115-152,
160-239) runs per clip on the host - eight Pillow resizes, pad, crop, flips, brightness / contrast, a 12-channel rotate, / 255., a
one-hot - and ships float64 images and int64 one-hot labels.  ClipAugmenter takes the clip as it is stored, uint8 frames
[B][T][Hs][Ws][3] and uint8 labels [B][Hs][Ws] on the GPU, and returns the model's input fp32 [B][T][3][Hc][Wc] and the class-index
labels int64 [B][Hc][Wc] that OhemCELoss2D receives after the scripts' argmax.  The host draws the random parameters and builds
small per-sample tables; the pixels never leave the device.

    aug = ClipAugmenter(crop=(512, 640), base_w=672, protocol="endovis18")
    params = aug.sample(B, rng=random.Random(seed), gen=numpy.random.default_rng(seed))
    images, labels = aug(frames_u8, labels_u8, params)                  # or out=(images, labels): static buffers, no allocation

What is exact and what is ours:
  * scale, pad, crop (`_random_scale`): drawn from a random.Random with the reference's calls in its order, computed as Pillow does
    (BILINEAR bit for bit, NEAREST with its accumulated float64 index, ImageOps.expand(fill=0), crop).
  * flips, brightness / contrast, rotation: the reference uses albumentations, whose random stream cannot be reproduced without the
    library; they are drawn from a numpy Generator of ours (sample() documents the order).  Brightness / contrast is the uint8 table
    value_table(); the rotation is fixed-point arithmetic modelled on cv2.warpAffine (rotate_tables()), not pinned to cv2.
  * Gaussian noise (CaDIS, CATA_new_512.py:178-183: skimage's random_noise(mode='gaussian', var=0.001, clip=True) on half of the
    clips, stored as (255 * clip(u / 255. + n, 0, 1)).astype('uint8')): for a byte that is clamp(u + floor(255 n), 0, 255), an integer
    offset with the law of noise_thresholds(), exact.  The stream is ours: Philox4x32-10 keyed by ClipParams.noise and counted by the
    byte index (the reference's is unseeded and never repeats).  Off unless p_noise is given; the reference's CaDIS value is 0.5.
  * the conversion: float32(u / 255.) (CaDIS: frames.cadis_value_table() per plane) and the label table (CaDIS: 255 -> class_num - 1).
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .frames import PRECISION_BITS, Pinned, T, bilinear_coeffs, check_rule, value_lut
from .hip import StswinHipError

AB_BITS = 10            # fraction bits of the rotation's position tables
INTER_BITS = 5          # fraction bits of a source position
_ONE = 1 << PRECISION_BITS


@dataclass
class ClipParams:
    """One sample's transform.  alpha / beta None: no value table; angle None: no rotation (degrees, positive counter-clockwise);
    noise None: no Gaussian noise, else the 64-bit key of the sample's noise stream."""
    long_size: int
    x1: int
    y1: int
    hflip: bool = False
    vflip: bool = False
    alpha: Optional[float] = None
    beta: Optional[float] = None
    angle: Optional[float] = None
    noise: Optional[int] = None


def geometry(long_size: int, src_hw, crop_hw) -> Tuple[int, int, int, int]:
    """(ow, oh, padw, padh) of `_random_scale`, which compares the short side with the crop WIDTH before it pads."""
    (h, w), (crop_h, crop_w) = src_hw, crop_hw
    if h > w:
        oh, ow = long_size, int(1.0 * w * long_size / h + 0.5)
        short = ow
    else:
        ow, oh = long_size, int(1.0 * h * long_size / w + 0.5)
        short = oh
    padw = padh = 0
    if short < crop_w:
        padh = crop_h - oh if oh < crop_h else 0
        padw = crop_w - ow if ow < crop_w else 0
    return ow, oh, padw, padh


def nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """Pillow's NEAREST source index (libImaging ImagingScaleAffine): the float64 position starts at scale / 2 and is advanced by
    `+= scale` per output pixel, then truncated.  The closed form floor((x + 0.5) * scale) rounds differently on most sizes."""
    scale = float(in_size) / out_size
    steps = np.full(out_size, scale, np.float64)
    steps[0] = scale * 0.5
    return np.add.accumulate(steps).astype(np.int64)


def bilinear_ksize(in_size: int, out_size: int) -> int:
    return int(math.ceil(max(float(in_size) / out_size, 1.0))) * 2 + 1


def axis_tables(in_size: int, out_size: int, start: int, count: int, ksize: int):
    """The tables of window indices start .. start + count of an axis scaled in_size -> out_size and padded behind out_size:
    (bounds int32 [count][2], weights int32 [count][ksize], nearest int32 [count]); an index in the padding has no taps and nearest
    -1; an unscaled axis has one tap of weight 2^22 (Pillow skips the pass)."""
    idx = start + np.arange(count)
    valid = idx < out_size
    src = idx[valid]
    bounds = np.zeros((count, 2), np.int32)
    coef = np.zeros((count, ksize), np.int32)
    near = np.full(count, -1, np.int32)
    if in_size == out_size:
        bounds[valid, 0], bounds[valid, 1], coef[valid, 0] = src, 1, _ONE
        near[valid] = src
    else:
        b, k = bilinear_coeffs(in_size, out_size)
        if k.shape[1] > ksize:
            raise StswinHipError(f"scale {in_size} -> {out_size} needs {k.shape[1]} taps, the tables hold {ksize}")
        bounds[valid] = b[src]
        coef[valid, :k.shape[1]] = k[src]
        near[valid] = nearest_index(in_size, out_size)[src]
    return bounds, coef, near


def value_table(alpha: Optional[float], beta: Optional[float]) -> np.ndarray:
    """uint8 [256], brightness / contrast (A.RandomBrightnessContrast with brightness_by_max): clip(round(alpha * u + beta * 255), 0,
    255), alpha = 1 + the contrast draw, beta = the brightness draw; float64, rounding floor(x + 0.5).  Both None: identity."""
    if alpha is None and beta is None:
        return np.arange(256, dtype=np.uint8)
    u = np.arange(256, dtype=np.float64)
    v = np.floor(float(1.0 if alpha is None else alpha) * u + float(0.0 if beta is None else beta) * 255.0 + 0.5)
    return np.clip(v, 0, 255).astype(np.uint8)


def rotate_tables(angle: float, H: int, W: int):
    """Position tables of the inverse rotation by `angle` degrees about ((W-1)/2, (H-1)/2), int32 with AB_BITS fraction bits:
    (colx [W], coly [W], rowx [H], rowy [H]).  With a = cos, b = sin, cx, cy the centre:
        colx[x] = rint(a x 2^10)    rowx[y] = rint((-b y + cx - a cx + b cy) 2^10) + 16
        coly[x] = rint(b x 2^10)    rowy[y] = rint(( a y + cy - b cx - a cy) 2^10) + 16
    (rint = round half to even, cv2's saturate_cast<int>; 16 = half of 1/32 pixel).  Modelled on cv2.warpAffine, not pinned to it."""
    r = math.radians(float(angle))
    a, b = math.cos(r), math.sin(r)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    m02 = cx - a * cx + b * cy
    m12 = cy - b * cx - a * cy
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    scale = float(1 << AB_BITS)
    rnd = (1 << AB_BITS) // (1 << INTER_BITS) // 2
    colx = np.rint(a * xs * scale)
    coly = np.rint(b * xs * scale)
    rowx = np.rint((-b * ys + m02) * scale) + rnd
    rowy = np.rint((a * ys + m12) * scale) + rnd
    return tuple(t.astype(np.int32) for t in (colx, coly, rowx, rowy))


MAX_THRESHOLDS = 1024   # what stswin_augment_noise keeps in LDS


def _phi(z: float) -> float:
    return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))


def _law(var: float):
    """[(k, t_k)] for the k whose threshold lies strictly between 0 and 2^32, strictly ascending: far out in the tails neighbours
    round to the same value, and there each is moved to one past its outer neighbour's (upwards below 2^31, downwards above), so that
    every offset in range keeps a probability of at least 2^-32."""
    s = 255.0 * math.sqrt(var)
    reach = int(math.ceil(9.0 * s)) + 2                     # Phi(-9) 2^32 < 1e-9: every k further out rounds to 0 or 2^32
    t = [(k, int(math.floor(_phi((k + 1) / s) * 4294967296.0 + 0.5))) for k in range(-reach, reach + 1)]
    ks, ts = [k for k, v in t if 0 < v < 1 << 32], [v for _, v in t if 0 < v < 1 << 32]
    for j in range(1, len(ts)):
        if ts[j] < 1 << 31:
            ts[j] = max(ts[j], ts[j - 1] + 1)
    for j in range(len(ts) - 2, -1, -1):
        if ts[j] >= 1 << 31:
            ts[j] = min(ts[j], ts[j + 1] - 1)
    return list(zip(ks, ts))


def noise_thresholds(var: float) -> Tuple[np.ndarray, int]:
    """The law of the integer offset K = floor(255 n), n ~ N(0, var), at 2^-32 resolution -> (uint32 thr ascending, k_min): with r a
    uniform 32-bit number K = k_min + #{j : thr[j] <= r}.  P(K <= k) = Phi((k + 1) / s), s = 255 sqrt(var), so the threshold of k is
    t_k = floor(Phi((k + 1) / s) 2^32 + 0.5) (float64, Phi from math.erf); the k with 0 < t_k < 2^32 are kept and k_min is the first.
    var = 0.001 (the reference's): 103 thresholds, k_min = -52, mean -0.5, variance s^2 + 1/12.  Strictly ascending: where neighbours
    far out in the tails round to the same value, each is moved to one past its outer neighbour's (for 0.001 the first two, 1 and 1,
    become 1 and 2, the last two 2^32 - 2 and 2^32 - 1), so that no offset in range has probability 0."""
    var = float(var)
    if not (math.isfinite(var) and var > 0.0):
        raise StswinHipError(f"noise_var must be a positive number, got {var!r}")

    def fits(v):                                            # (the k within one sigma alone have 2 s distinct thresholds)
        return 255.0 * math.sqrt(v) <= MAX_THRESHOLDS and len(_law(v)) <= MAX_THRESHOLDS

    if not fits(var):
        lo, hi = 0.0, min(var, (MAX_THRESHOLDS / 255.0) ** 2)      # the number of thresholds grows with var: bisect for the largest that fits
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        raise StswinHipError(f"noise_var {var!r} needs more than {MAX_THRESHOLDS} thresholds, which is what the kernel holds: the "
                             f"largest var that fits is {lo:.6g}")
    kept = _law(var)
    return np.array([v for _, v in kept], dtype=np.uint32), kept[0][0]


_PROTOCOL_DEFAULTS = {      # (p_hflip, p_vflip, p_bc) of the reference's A.Compose: Endovis2018_new.py:73-78, CATA_new_512.py:211-219
    "endovis18": (0.0, 0.5, 0.5),
    "cadis": (0.5, 0.5, 0.0),
}


def _noise_key(noise) -> Optional[int]:
    if noise is None:
        return None
    key = int(noise)
    if not 0 <= key < 1 << 64:
        raise StswinHipError(f"noise must be None or a 64-bit key in [0, 2**64), got {noise!r}")
    return key


class ClipAugmenter:
    """aug = ClipAugmenter(crop=(512, 640), base_w=672, protocol="endovis18" | "cadis", class_num=None, source=None, p_hflip=None,
                           p_vflip=None, p_bc=None, brightness_limit=0.2, contrast_limit=0.2, p_rotate=0.5, rotate_limit=90.0,
                           p_noise=0.0, noise_var=0.001)

    crop = (Hc, Wc), base_w the reference's base_size['w'], source = (Hs, Ws) the stored frames' size (default: the crop size, as
    EndoVis18's Processed_train).  The probabilities default to the protocol's A.Compose; class_num (cadis: required) is the 255 ->
    class_num - 1 label rule's.  p_noise is the probability of CaDIS's Gaussian noise of variance noise_var (on the / 255. scale); it
    is 0.0 by default for BOTH protocols - the reference's CaDIS transform uses 0.5, EndoVis18's has none.

    sample(B, rng, gen) draws B ClipParams; params(...) makes one explicitly; identity() is the no-augmentation one.
    aug(frames, labels, params, out=None): uint8 frames [B][4][Hs][Ws][3] and uint8 labels [B][Hs][Ws] on the GPU -> (fp32 images
    [B][4][3][Hc][Wc], int64 labels [B][Hc][Wc]).  With out=(images, labels) it writes into the given buffers and, after the first
    call for a batch size, allocates nothing: the form for GraphedStep's before_step.  Three launches and one pinned upload of the
    tables per batch, on the current stream, no synchronisation.

    Refuses (StswinHipError, with the expected form): CPU tensors, a wrong dtype or layout, frames and labels of different sizes or
    not of the source size, T != 4, a long_size outside the range base_w allows, crop coordinates outside the scaled image."""

    def __init__(self, crop: Sequence[int] = (512, 640), base_w: int = 672, protocol: str = "endovis18", class_num: Optional[int] = None,
                 source: Optional[Sequence[int]] = None, p_hflip: Optional[float] = None, p_vflip: Optional[float] = None,
                 p_bc: Optional[float] = None, brightness_limit: float = 0.2, contrast_limit: float = 0.2, p_rotate: float = 0.5,
                 rotate_limit: float = 90.0, p_noise: float = 0.0, noise_var: float = 0.001):
        check_rule(protocol)
        self.protocol = protocol
        self.crop = (int(crop[0]), int(crop[1]))
        self.source = (int(source[0]), int(source[1])) if source is not None else self.crop
        self.base_w = int(base_w)
        if protocol == "cadis" and class_num is None:
            raise StswinHipError("protocol='cadis' needs class_num (9, 18 or 26: the label 255 becomes class_num - 1)")
        self.class_num = 12 if class_num is None else int(class_num)
        d = _PROTOCOL_DEFAULTS[protocol]
        self.p_hflip = d[0] if p_hflip is None else float(p_hflip)
        self.p_vflip = d[1] if p_vflip is None else float(p_vflip)
        self.p_bc = d[2] if p_bc is None else float(p_bc)
        self.brightness_limit, self.contrast_limit = float(brightness_limit), float(contrast_limit)
        self.p_rotate, self.rotate_limit = float(p_rotate), float(rotate_limit)
        self.p_noise, self.noise_var = float(p_noise), float(noise_var)
        self.noise_law = noise_thresholds(self.noise_var)
        self.long_range = (int(self.base_w * 0.5), int(self.base_w * 2.0))
        if self.long_range[0] < 1:
            raise StswinHipError(f"base_w must be >= 2, got {base_w}")
        ow, oh, _, _ = geometry(self.long_range[0], self.source, self.crop)
        if min(ow, oh) < 1:
            raise StswinHipError(f"base_w {base_w} scales the source {self.source} down to nothing")
        self.ksize = max(bilinear_ksize(self.source[1], ow), bilinear_ksize(self.source[0], oh))       # the most taps any scale needs
        self._ws = {}
        self._luts = {}
        self._thr = {}
        self._pinned = Pinned()

    # ----------------------------------------------------------------------------------------- parameters
    def params(self, long_size: int, x1: int, y1: int, hflip: bool = False, vflip: bool = False, alpha: Optional[float] = None,
               beta: Optional[float] = None, angle: Optional[float] = None, noise: Optional[int] = None) -> ClipParams:
        p = ClipParams(int(long_size), int(x1), int(y1), bool(hflip), bool(vflip), alpha, beta, angle, _noise_key(noise))
        self.scaled(p)
        return p

    def identity(self) -> ClipParams:
        """No augmentation: scale to the source size, crop at the origin (needs source == crop)."""
        return self.params(max(self.source), 0, 0)

    def scaled(self, p: ClipParams) -> Tuple[int, int, int, int]:
        """(ow, oh, padw, padh) of p, after checking it against the source and the crop."""
        lo, hi = self.long_range
        if not lo <= p.long_size <= hi:
            raise StswinHipError(f"long_size must be in [{lo}, {hi}] (base_w {self.base_w}), got {p.long_size}")
        ow, oh, padw, padh = geometry(p.long_size, self.source, self.crop)
        w, h = ow + padw, oh + padh
        if not (0 <= p.x1 <= w - self.crop[1] and 0 <= p.y1 <= h - self.crop[0]):
            raise StswinHipError(f"crop origin must satisfy 0 <= x1 <= {w - self.crop[1]} and 0 <= y1 <= {h - self.crop[0]} (the scaled "
                                 f"and padded image is {h} x {w}, the crop {self.crop[0]} x {self.crop[1]}), got x1 = {p.x1}, y1 = {p.y1}")
        return ow, oh, padw, padh

    def sample(self, B: int, rng: Optional[random.Random] = None, gen: Optional[np.random.Generator] = None) -> List[ClipParams]:
        """B parameter sets.  Per sample, from rng (a random.Random; default: the `random` module, as the reference): long_size =
        randint(int(base_w * 0.5), int(base_w * 2.0)), x1 = randint(0, w - Wc), y1 = randint(0, h - Hc) - `_random_scale`'s calls in
        its order, so the same seed gives the reference's geometry.  Then from gen (a numpy Generator; default: a fresh default_rng()),
        always seven draws in this order: u_hflip, u_vflip, u_bc, contrast ~ U(-limit, limit), brightness ~ U(-limit, limit), u_rotate,
        angle ~ U(-limit, limit); a transform applies when its u < p.  With p_noise != 0 two more follow, always both: u_noise =
        gen.random() and key = gen.integers(0, 2**64, dtype=uint64); the sample gets the key when u_noise < p_noise.  This is NOT
        albumentations' stream."""
        rng = random if rng is None else rng
        gen = np.random.default_rng() if gen is None else gen
        out = []
        for _ in range(B):
            long_size = rng.randint(*self.long_range)
            ow, oh, padw, padh = geometry(long_size, self.source, self.crop)
            if ow + padw < self.crop[1] or oh + padh < self.crop[0]:
                raise StswinHipError(f"long_size {long_size} scales the source {self.source} to {oh} x {ow}, padded {oh + padh} x "
                                     f"{ow + padw}: smaller than the crop {self.crop}")
            x1 = rng.randint(0, ow + padw - self.crop[1])
            y1 = rng.randint(0, oh + padh - self.crop[0])
            u = gen.random(3)
            contrast = gen.uniform(-self.contrast_limit, self.contrast_limit)
            brightness = gen.uniform(-self.brightness_limit, self.brightness_limit)
            u_rot = gen.random()
            angle = gen.uniform(-self.rotate_limit, self.rotate_limit)
            noise = None
            if self.p_noise != 0.0:
                u_noise = gen.random()
                key = int(gen.integers(0, 2 ** 64, dtype=np.uint64))
                noise = key if u_noise < self.p_noise else None
            bc = u[2] < self.p_bc
            out.append(ClipParams(long_size, x1, y1, bool(u[0] < self.p_hflip), bool(u[1] < self.p_vflip),
                                  1.0 + float(contrast) if bc else None, float(brightness) if bc else None,
                                  float(angle) if u_rot < self.p_rotate else None, noise))
        return out

    # ----------------------------------------------------------------------------------------- host tables
    def crop_tables(self, p: ClipParams) -> dict:
        """Stage 1's tables of one sample (numpy): r0, r1, flags, hbounds, hcoef, vbounds, vcoef, lx, ly."""
        ow, oh, _, _ = self.scaled(p)
        (Hs, Ws), (Hc, Wc) = self.source, self.crop
        hb, hk, lx = axis_tables(Ws, ow, p.x1, Wc, self.ksize)
        vb, vk, ly = axis_tables(Hs, oh, p.y1, Hc, self.ksize)
        rows = vb[:, 1] > 0
        r0 = int(vb[rows, 0].min()) if rows.any() else 0
        r1 = int((vb[rows, 0] + vb[rows, 1]).max()) if rows.any() else 0
        return dict(r0=r0, r1=r1, flags=(1 if p.hflip else 0) | (2 if p.vflip else 0), hbounds=hb, hcoef=hk, vbounds=vb, vcoef=vk, lx=lx, ly=ly)

    def strides(self) -> Tuple[int, int]:
        """Words per sample of the two stages' table rows, as the library states them (the one place both tables() and the device
        workspace take them from)."""
        Hc, Wc = self.crop
        return hip.augment_crop_table_stride(Hc, Wc, self.ksize), hip.augment_finish_table_stride(Hc, Wc)

    def tables(self, params: Sequence[ClipParams]) -> Tuple[np.ndarray, np.ndarray]:
        """-> (int32 [B][stride1], int32 [B][stride2]): the rows of stswin_augment_crop's and stswin_augment_finish's tables.  Both are
        views of one flat array (`.base`): stage 1's rows, then stage 2's - the layout of the device table, uploaded in one copy."""
        Hc, Wc = self.crop
        s1, s2 = self.strides()
        B = len(params)
        flat = np.zeros(B * (s1 + s2), np.int32)
        t1, t2 = flat[:B * s1].reshape(B, s1), flat[B * s1:].reshape(B, s2)
        for b, p in enumerate(params):
            c = self.crop_tables(p)
            t1[b, :4] = (c["r0"], c["r1"], c["flags"], 0)
            o = 4
            for k in ("hbounds", "hcoef", "vbounds", "vcoef", "lx", "ly"):
                t1[b, o:o + c[k].size] = c[k].reshape(-1)
                o += c[k].size
            if o != s1:
                raise StswinHipError(f"stage 1's table row has {o} words, the library expects {s1}")
            key = _noise_key(p.noise)
            if key is not None:                                    # (int32 words: the halves' bit patterns)
                t2[b, 1:4] = np.array([key & 0xffffffff, key >> 32, 1], np.uint32).view(np.int32)
            o = 4
            if p.angle is not None:
                t2[b, 0] = 1
                for t in rotate_tables(p.angle, Hc, Wc):
                    t2[b, o:o + t.size] = t
                    o += t.size
            o = 4 + 2 * (Hc + Wc)
            if o + 64 != s2:
                raise StswinHipError(f"stage 2's table row has {o + 64} words, the library expects {s2}")
            t2[b, o:] = value_table(p.alpha, p.beta).view(np.int32)
        return t1, t2

    # ----------------------------------------------------------------------------------------- device
    def _workspace(self, B: int, dev):
        key = (B, str(dev))
        ws = self._ws.get(key)
        if ws is None:
            (Hs, Ws), (Hc, Wc) = self.source, self.crop
            s1, s2 = self.strides()
            table = torch.empty(B * (s1 + s2), dtype=torch.int32, device=dev)
            ws = self._ws[key] = dict(table=table, t1=table[:B * s1].view(B, s1), t2=table[B * s1:].view(B, s2),
                                      tmp=torch.empty(B * T * Hs * Wc * 3, dtype=torch.uint8, device=dev),
                                      crop=torch.empty(B, T, Hc, Wc, 3, dtype=torch.uint8, device=dev),
                                      label_crop=torch.empty(B, Hc, Wc, dtype=torch.uint8, device=dev))
        return ws

    def _lut(self, dev):
        key = str(dev)
        t = self._luts.get(key)
        if t is None:
            lab = np.arange(256, dtype=np.int64)
            if self.protocol == "cadis":
                lab[255] = self.class_num - 1                      # CATA_new_512.py:237
            t = self._luts[key] = (value_lut(dev, self.protocol), torch.from_numpy(lab).to(dev))
        return t

    def _thresholds(self, dev):
        key = str(dev)
        t = self._thr.get(key)
        if t is None:
            t = self._thr[key] = torch.from_numpy(self.noise_law[0].view(np.int32).copy()).to(dev)
        return t

    def _check_inputs(self, frames, labels, params):
        (Hs, Ws) = self.source
        form = f"frames must be contiguous uint8 [B][{T}][{Hs}][{Ws}][3] and labels contiguous uint8 [B][{Hs}][{Ws}], both on the GPU"
        for t, what in ((frames, "frames"), (labels, "labels")):
            if not isinstance(t, torch.Tensor):
                raise StswinHipError(f"{form}; got {type(t).__name__} for {what}")
            if not t.is_cuda:
                raise StswinHipError(f"{form}; {what} is on the CPU (there is no CPU path: move the uint8 batch with .cuda())")
            if t.dtype != torch.uint8:
                raise StswinHipError(f"{form}; {what} is {t.dtype}")
            if not t.is_contiguous():
                raise StswinHipError(f"{form}; {what} is not contiguous")
        if frames.dim() != 5 or frames.shape[4] != 3:
            raise StswinHipError(f"{form}; frames is {tuple(frames.shape)}")
        if frames.shape[1] != T:
            raise StswinHipError(f"{form}; the model takes clips of T = {T} frames, frames is {tuple(frames.shape)}")
        B = frames.shape[0]
        if labels.dim() != 3 or labels.shape[0] != B or tuple(labels.shape[1:]) != tuple(frames.shape[2:4]):
            raise StswinHipError(f"{form}; frames is {tuple(frames.shape)} and labels {tuple(labels.shape)}: the sizes differ")
        if tuple(frames.shape[2:4]) != (Hs, Ws):
            raise StswinHipError(f"{form}; the frames are {tuple(frames.shape[2:4])}, the augmenter's source size is {(Hs, Ws)}")
        if labels.device != frames.device:
            raise StswinHipError(f"{form}; frames on {frames.device}, labels on {labels.device}")
        if len(params) != B:
            raise StswinHipError(f"params must hold one ClipParams per sample: {B}, got {len(params)}")
        return B

    def crop_stage(self, frames: torch.Tensor, labels: torch.Tensor, params: Sequence[ClipParams]):
        """Stage 1 alone -> (uint8 crops [B][4][Hc][Wc][3], uint8 label crops [B][Hc][Wc]): views of the augmenter's workspace, which
        the next call overwrites."""
        B = self._check_inputs(frames, labels, params)
        ws = self._upload(B, frames.device, params)
        return hip.augment_crop(frames, labels, ws["tmp"], ws["crop"], ws["label_crop"], ws["t1"], self.ksize)

    def _upload(self, B: int, dev, params):
        """Build both stages' tables and copy them to the device table in one asynchronous copy from pinned memory.  Calls may follow
        each other without a synchronise: Pinned rotates staging buffers and, before it rewrites one, waits for the event
        recorded behind the copy that last read it; the device table itself is rewritten in stream order, behind the launches of the
        earlier call that read it."""
        t1, _ = self.tables(params)
        ws = self._workspace(B, dev)
        self._pinned.upload(t1.base, ws["table"])
        return ws

    def _outputs(self, out, B: int, dev):
        Hc, Wc = self.crop
        if out is None:
            return (torch.empty(B, T, 3, Hc, Wc, dtype=torch.float32, device=dev), torch.empty(B, Hc, Wc, dtype=torch.int64, device=dev))
        form = f"out must be (contiguous fp32 [{B}][{T}][3][{Hc}][{Wc}], contiguous int64 [{B}][{Hc}][{Wc}]) on {dev}"
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out):
            raise StswinHipError(form)
        img, lab = out
        if img.dtype != torch.float32 or tuple(img.shape) != (B, T, 3, Hc, Wc) or lab.dtype != torch.int64 or tuple(lab.shape) != (B, Hc, Wc) \
                or not img.is_contiguous() or not lab.is_contiguous() or img.device != dev or lab.device != dev:
            raise StswinHipError(f"{form}; got {img.dtype} {tuple(img.shape)} on {img.device} and {lab.dtype} {tuple(lab.shape)} on {lab.device}")
        return img, lab

    def finish_stage(self, crop: torch.Tensor, label_crop: torch.Tensor, params: Sequence[ClipParams], out=None):
        """Stage 2 alone on uint8 crops [B][4][Hc][Wc][3] and label crops [B][Hc][Wc] (only alpha, beta and angle of params are used)."""
        Hc, Wc = self.crop
        hip.tensor_form(crop, torch.uint8, (None, T, Hc, Wc, 3), "crop", "finish_stage")
        B, dev = crop.shape[0], crop.device
        hip.tensor_form(label_crop, torch.uint8, (B, Hc, Wc), "label_crop", "finish_stage", dev)
        if len(params) != B:
            raise StswinHipError(f"params must hold one ClipParams per sample: {B}, got {len(params)}")
        images, labels_out = self._outputs(out, B, dev)
        ws = self._upload(B, dev, params)
        lut, label_lut = self._lut(dev)
        return hip.augment_finish(crop, label_crop, images, labels_out, ws["t2"], lut, label_lut)

    def noise_stage(self, crop: torch.Tensor, params: Sequence[ClipParams]) -> torch.Tensor:
        """The noise pass alone, in place on uint8 crops [B][4][Hc][Wc][3] (only `noise` of params is used); returns crop."""
        Hc, Wc = self.crop
        hip.tensor_form(crop, torch.uint8, (None, T, Hc, Wc, 3), "crop", "noise_stage")
        B, dev = crop.shape[0], crop.device
        if len(params) != B:
            raise StswinHipError(f"params must hold one ClipParams per sample: {B}, got {len(params)}")
        ws = self._upload(B, dev, params)
        return hip.augment_noise(crop, ws["t2"], self._thresholds(dev), self.noise_law[1])

    def __call__(self, frames: torch.Tensor, labels: torch.Tensor, params: Sequence[ClipParams], out=None):
        B = self._check_inputs(frames, labels, params)
        dev = frames.device
        images, labels_out = self._outputs(out, B, dev)
        ws = self._upload(B, dev, params)
        lut, label_lut = self._lut(dev)
        thr = self._thresholds(dev)
        hip.augment_crop(frames, labels, ws["tmp"], ws["crop"], ws["label_crop"], ws["t1"], self.ksize)
        if any(p.noise is not None for p in params):
            hip.augment_noise(ws["crop"], ws["t2"], thr, self.noise_law[1])
        return hip.augment_finish(ws["crop"], ws["label_crop"], images, labels_out, ws["t2"], lut, label_lut)
