"""Float64 contract of the kernels that turn logits into what the project reports (stswincl_amd/csrc/headops.hip):
stswin_upsample_argmax (EndoVis: labels + Dice / IoU counts), stswin_upsample_argmax_cm (CaDIS: labels + confusion matrix) and
stswin_labels_score (the same integers from an existing label map).

Shared by tests/test_labels_ref.py (CPU: the reference against float64 F.interpolate, an fp32 emulation of the kernels' association
against the bound, the cases' properties, planted defects) and tests/test_hip_labels_contract.py (GPU: the kernels against it).
Nothing here calls the library: plain torch, run on the device of its operands.  Finite logits only: infinities and NaN are outside
this contract (the kernels start their running maximum at -3e38 and compare with `>`).

  upsample   the header's formulas per axis (n_in -> n_out), in float64 from integer numerators, so one rounding per coordinate and
             an exact floor:
                 align = 1:  src = dst (n_in - 1) / (n_out - 1), 0 when n_out == 1
                 align = 0:  src = max((n_in / n_out)(dst + 0.5) - 0.5, 0) = max((n_in (2 dst + 1) - n_out) / (2 n_out), 0)
                 i0 = min(floor(src), n_in - 1),  i1 = min(i0 + 1, n_in - 1),  w = src - i0
             v = (1 - wy) ((1 - wx) s[y0][x0] + wx s[y0][x1]) + wy ((1 - wx) s[y1][x0] + wx s[y1][x1])
  bound      what an fp32 evaluation of the same expressions may differ by, per pixel and class, u = 2^-24:
                 8 u A + 4 u (fx + 1) Dx + 4 u (fy + 1) Dy
             A: the largest |source value|, Dx / Dy: the largest difference of horizontally / vertically adjacent source values, all
             three over the 4 x 4 source neighbourhood rows y0 - 1 .. y0 + 2, columns x0 - 1 .. x0 + 2 (clamped to the map), so a
             coordinate that rounds across a cell border is covered.  Where from:
               the coordinate: the scale is one rounded division (u), the product one more (u), align = 0 subtracts 0.5 (u of the
                 result) after the product's error grew by the 0.5 added to dst: |f32 src - src| <= 3 u (src + 1) <= 4 u (src + 1);
                 src - i0 is exact.  v is piecewise linear and continuous in src with slope <= Dx (Dy), also across a cell border.
               the value: 1 - w rounds once (u), so each of the four inner products carries 2 u, an inner sum one more u A: 3 u A;
                 the outer products add 2 u each and the last sum u A: 6 u A in first order, 8 u A with room for the second order.
             Nothing in it is tuned on a GPU.  The exact regime (below) has bound 0: every coordinate, weight, product and sum is
             a dyadic number with a handful of bits, exact in fp32 and in float64.
  verdict    delta = 2 max_c bound per pixel (the winner and its rival may each be off by their bound); the allowed set is
             {c : v_c >= max_c v - delta}; a pixel is decided when the set has one member.  A kernel label must lie in the allowed
             set, so on a decided pixel it is that member.  With bound 0 the label must be the FIRST maximum of v.
  counts     int64 [F][3][nc]: |gt == c|, |labels == c|, |gt == c and labels == c| for c < nc, gt compared as int64.
  confusion  int64 [ncm][ncm]: cm[gt][label] over the pixels with 0 <= gt < ncm and label < ncm, gt compared as int64.
"""
from __future__ import annotations

import dataclasses

import torch
import torch.nn.functional as TF

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
CAP = 0.02                   # at most this share of a non-exact case's pixels may be undecided (asserted on the reference alone)
SENTINEL = 0xA5              # the byte around and under the label maps: no class index (nc <= 64)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BLOCK_ENDOVIS, BLOCK_CM, BLOCK_SCORE = 256, 1024, 4096      # output pixels of one frame per workgroup


# ------------------------------------------------------------------------------------------------------------------- the contract
def axis(n_in, n_out, align, device=None):
    """-> (src float64, i0, i1 long, w float64), each [n_out], of one axis."""
    d = torch.arange(n_out, dtype=torch.int64, device=device)
    if align:
        s = (d * (n_in - 1)).to(F64) / (n_out - 1) if n_out > 1 else torch.zeros(n_out, dtype=F64, device=device)
    else:
        s = (((2 * d + 1) * n_in - n_out).to(F64) / (2 * n_out)).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return s, i0, i1, s - i0.to(F64)


def upsample(logits, H, W, align):
    """The stored logits [F][nc][h][w] (fp32 or bf16) -> float64 v [F][nc][H][W]."""
    src = logits.to(F64)
    h, w = src.shape[2:]
    _, y0, y1, wy = axis(h, H, align, src.device)
    _, x0, x1, wx = axis(w, W, align, src.device)
    wy = wy.view(H, 1)
    r0, r1 = src[:, :, y0], src[:, :, y1]                                    # [F][nc][H][w]
    return (1.0 - wy) * ((1.0 - wx) * r0[..., x0] + wx * r0[..., x1]) + wy * ((1.0 - wx) * r1[..., x0] + wx * r1[..., x1])


def _window_max(t, rows, cols):
    out = None
    for yy in rows:
        r = t[:, :, yy]
        for xx in cols:
            g = r[..., xx]
            out = g if out is None else torch.maximum(out, g)
    return out


def bound(logits, H, W, align, exact=False):
    """-> float64 [F][nc][H][W]; exact=True (the exact regime, held to an fp32 emulation by the CPU test): zeros."""
    src = logits.to(F64)
    F_, nc, h, w = src.shape
    if exact:
        return torch.zeros(F_, nc, H, W, dtype=F64, device=src.device)
    sy, y0, _, _ = axis(h, H, align, src.device)
    sx, x0, _, _ = axis(w, W, align, src.device)
    rows = [(y0 + k).clamp(0, h - 1) for k in (-1, 0, 1, 2)]
    cols = [(x0 + k).clamp(0, w - 1) for k in (-1, 0, 1, 2)]
    A = _window_max(src.abs(), rows, cols)
    zero = torch.zeros_like(A)
    Dx = _window_max((src[..., 1:] - src[..., :-1]).abs(), rows, [(x0 + k).clamp(0, w - 2) for k in (-1, 0, 1)]) if w > 1 else zero
    Dy = _window_max((src[:, :, 1:] - src[:, :, :-1]).abs(), [(y0 + k).clamp(0, h - 2) for k in (-1, 0, 1)], cols) if h > 1 else zero
    return 8 * U * A + 4 * U * (sx + 1.0) * Dx + 4 * U * (sy.view(H, 1) + 1.0) * Dy


def verdict(v, bnd):
    """-> (allowed bool [F][nc][H][W], decided bool [F][H][W], first long [F][H][W]: the first maximum of v, delta [F][H][W])."""
    nc = v.shape[1]
    delta = 2.0 * bnd.amax(1)
    top = v.amax(1)
    allowed = v >= (top - delta).unsqueeze(1)
    idx = torch.arange(nc, device=v.device).view(1, nc, 1, 1)
    first = torch.where(v == top.unsqueeze(1), idx, torch.full_like(idx, nc)).amin(1)
    return allowed, allowed.sum(1) == 1, first, delta


def offenders(labels, allowed, first, exact):
    """-> bool [F][H][W]: the labels the contract does not permit (outside the allowed set; exact: not the first maximum)."""
    lab = labels.long()
    if exact:
        return lab != first
    nc = allowed.shape[1]
    inside = allowed.gather(1, lab.clamp_max(nc - 1).unsqueeze(1)).squeeze(1)
    return (lab >= nc) | ~inside


def outside(logits, labels, H, W, align):
    """For the tests that have their own logits: -> (labels outside their allowed set, undecided pixels)."""
    allowed, decided, first, _ = verdict(upsample(logits, H, W, align), bound(logits, H, W, align))
    return int(offenders(labels, allowed, first, False).sum()), int((~decided).sum())


def counts(labels, gt, nc):
    """-> int64 [F][3][nc], no narrowing of gt."""
    c = torch.arange(nc, dtype=torch.int64, device=labels.device).view(1, nc, 1, 1)
    g = gt.to(torch.int64).unsqueeze(1) == c
    p = labels.to(torch.int64).unsqueeze(1) == c
    return torch.stack([g.sum((2, 3)), p.sum((2, 3)), (g & p).sum((2, 3))], 1)


def confusion(labels, gt, ncm):
    """-> int64 [ncm][ncm], rows gt, columns label, no narrowing of gt."""
    g, p = gt.to(torch.int64).reshape(-1), labels.to(torch.int64).reshape(-1)
    keep = (g >= 0) & (g < ncm) & (p < ncm)
    return torch.bincount(g[keep] * ncm + p[keep], minlength=ncm * ncm).view(ncm, ncm)


def where(case, f, y, x):
    """Which workgroup and lane of either kernel owns pixel (f, y, x) - for a failure's message."""
    HW, px = case.H * case.W, y * case.W + x
    b256, b1024 = -(-HW // BLOCK_ENDOVIS), -(-HW // BLOCK_CM)
    return (f"frame {f} y {y} x {x}: upsample_argmax block {f * b256 + px // 256} lane {px % 256}; "
            f"upsample_argmax_cm block {f * b1024 + px // 1024} pass {px % 1024 // 256} lane {px % 256}")


# ------------------------------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass(frozen=True)
class Case:
    F: int
    nc: int
    h: int
    w: int
    H: int
    W: int
    align: int
    dtype: torch.dtype
    regime: str
    seed: int

    @property
    def exact(self):
        return self.regime == "exact"

    @property
    def name(self):
        return (f"{self.regime} {self.F}x{self.nc}x{self.h}x{self.w}->{self.H}x{self.W} align{self.align} "
                f"{'bf16' if self.dtype == BF else 'f32'}")


# F, h, w, H, W, then (nc, regime) for align 0 fp32, align 0 bf16, align 1 fp32, align 1 bf16.  nc <= 12 only where the source has
# enough pixels for every class to win somewhere; `smooth` only where its coarse map (h / 8 x w / 8) has.
_SHAPES = [
    # 24 pixels: everything clamped, one partial block per frame, so the frame index of a block is exercised
    (3, 1, 1, 4, 6, [(2, "normal"), (64, "large"), (2, "large"), (1, "normal")]),
    # a non-dyadic ratio; 7777 pixels = 31 blocks of 256 and 8 of 1024 with a ragged last one
    (2, 23, 37, 101, 77, [(12, "normal"), (64, "smooth"), (9, "large"), (2, "smooth")]),
    # coordinates near the right and bottom clamps
    (2, 8, 10, 67, 131, [(9, "large"), (12, "normal"), (64, "smooth"), (12, "large")]),
    # down-sampling
    (1, 16, 20, 13, 9, [(12, "large"), (2, "smooth"), (9, "normal"), (64, "normal")]),
    # x8
    (1, 3, 5, 40, 24, [(2, "normal"), (64, "normal"), (1, "large"), (2, "normal")]),
    # H W = 1025: one pixel in the second 1024-block of the CM kernel and in the fifth 256-block
    (1, 5, 7, 25, 41, [(64, "large"), (9, "normal"), (2, "large"), (9, "large")]),
    # the production source size at a quarter of the output: the largest case, 32 400 pixels
    (1, 64, 80, 135, 240, [(12, "smooth"), (64, "normal"), (9, "smooth"), (12, "large")]),
]
# ratios at which every coordinate and weight is exact in fp32: identity, x2 and x4 with align = 0, (n - 1) -> 2 (n - 1) with align = 1
_EXACT = [(2, 5, 7, 5, 7, 0), (2, 5, 7, 5, 7, 1), (2, 5, 7, 10, 14, 0), (2, 6, 6, 24, 24, 0), (2, 5, 9, 9, 17, 1)]
_EXACT_NC = [(9, 2), (2, 12), (12, 9), (9, 12), (2, 9)]                       # (fp32, bf16)


def cases():
    out = []
    for F_, h, w, H, W, slots in _SHAPES:
        for k, (nc, regime) in enumerate(slots):
            out.append(Case(F_, nc, h, w, H, W, k // 2, BF if k % 2 else F32, regime, 0))
    for (F_, h, w, H, W, align), ncs in zip(_EXACT, _EXACT_NC):
        for k, nc in enumerate(ncs):
            out.append(Case(F_, nc, h, w, H, W, align, BF if k else F32, "exact", 0))
    out = [dataclasses.replace(c, seed=i) for i, c in enumerate(out)]       # (the CPU test holds every case's properties at these seeds)
    assert len({c.name for c in out}) == len(out)
    return out


def make_logits(c):
    """The stored logits of a case, on the CPU (one generator per case, so a case does not depend on the others)."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    shape = (c.F, c.nc, c.h, c.w)
    if c.regime == "normal":
        x = 3.0 * torch.randn(shape, generator=g)
    elif c.regime == "large":
        x = 3.0e4 * torch.randn(shape, generator=g)
    elif c.regime == "smooth":                                               # a coarse map resized up, plus noise
        coarse = 3.0 * torch.randn(c.F, c.nc, max(c.h // 8, 1), max(c.w // 8, 1), generator=g)
        x = TF.interpolate(coarse, (c.h, c.w), mode="bilinear") + 0.3 * torch.randn(shape, generator=g)
    else:
        x = torch.randint(-2, 3, shape, generator=g).to(F32)
    return x.to(c.dtype)


def edge_values(nc):
    return [-1, nc - 1, nc, 63, 64, 255, 1 << 31, 1 << 32, (1 << 32) + 3, -(1 << 32) + 2, I64_MIN, I64_MAX]


def ground_truth(c, labels):
    """int64 [F][H][W] on the device of `labels`: the label itself on about half of the pixels (so the intersections are not empty),
    classes 0 .. nc + 1 elsewhere, and the twelve edge values in every run of 256 pixels of every frame - so in every workgroup of the
    three kernels (256, 1024, 4096 pixels), the last partial one included; a run shorter than twelve takes as many as fit, 2^32 + 3
    first."""
    g = torch.Generator().manual_seed(5000 + c.seed)
    HW = c.H * c.W
    rnd = torch.randint(0, c.nc + 2, (c.F, HW), generator=g)
    own = torch.rand(c.F, HW, generator=g) < 0.5
    gt = torch.where(own, labels.detach().cpu().reshape(c.F, HW).long(), rnd)
    edge = edge_values(c.nc)
    for f in range(c.F):
        for p0 in range(0, HW, 256):
            n = min(256, HW - p0)
            k = min(n, len(edge))
            pos = p0 + torch.randperm(n, generator=g)[:k]
            gt[f, pos] = torch.tensor([edge[(8 + i) % len(edge)] for i in range(k)], dtype=torch.int64)
    return gt.view(c.F, c.H, c.W).to(labels.device)
