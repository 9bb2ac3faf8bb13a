"""Float64 reference of the decode head's resampling and pooling kernels (stswincl_amd/csrc/headops.hip: bilinear, logits_upsample,
rows_broadcast, the sum-only colstats; rowops.hip: maxpool3x3s2), on token matrices [F*h*w][C] as the kernels take them.

Shared by tests/test_resample_ref.py (CPU: the reference against float64 F.interpolate / F.max_pool2d and autograd through them) and
tests/test_hip_resample_contract.py (GPU: every kernel against it).  Nothing here calls the library: plain torch, run on the device
of its inputs.  Written from the definitions:

  bilinear, align_corners=False, per axis (n_in -> n_out), all in float64:
        s = max((d + 0.5) * n_in / n_out - 0.5, 0),  i0 = min(floor(s), n_in - 1),  i1 = min(i0 + 1, n_in - 1),  w = s - i0
        out[d] = (1 - w) * in[i0] + w * in[i1];  two axes: rows first, then columns (the order is immaterial in exact arithmetic).
  its adjoint: the two 1-D interpolation matrices A_y [H][h], A_x [W][w]; up = A_y x A_x^T per channel, so up^T(g) = A_y^T g A_x.
        The forward gathers through (i0, i1, w); the adjoint multiplies by the dense transposes and shares nothing with a gather.
  logits: the same operator from tokens [F*h*w][pitch >= nc] (columns >= nc are padding) to NCHW [F][nc][H][W] and back.
  rows_broadcast: out[r] = (base[r] if given) + v[r // (M / groups)] * scale.
  group_sums: per statistic group (bn_ref.group_rows: contiguous or interleaved units) the column sums - AdaptiveAvgPool2d(1)'s
        numerator.
  max pool 3 x 3, stride 2, pad 1: values from bn_ref.maxpool3x3s2; the tap is the FIRST maximum of the window at (2 yo - 1, 2 xo - 1)
        in (ky, kx) scan order, tap = ky * 3 + kx, out-of-map taps never win (what nn.MaxPool2d(return_indices=True) returns).
"""
from __future__ import annotations

import torch

from bn_ref import errors, group_rows, maxpool3x3s2, maxpool3x3s2_bwd  # noqa: F401  (re-exported: one reference module per suite)

F64 = torch.float64

# (h, w, H, W) of the GPU contract; the CPU tests hold the reference to F.interpolate at the same geometries.
BILINEAR_GEOMS = [(1, 1, 4, 6),          # everything clamped
                  (1, 5, 3, 11), (2, 2, 3, 5),
                  (5, 7, 13, 9),         # up in one axis, a near-1 ratio in the other
                  (8, 8, 16, 16),
                  (16, 20, 32, 40),      # the x2 of base18.py:54-55
                  (6, 10, 6, 10),        # identity
                  (13, 9, 5, 7)]         # down-sampling
LOGITS_GEOMS = [(5, 6, 40, 48), (4, 5, 30, 37), (16, 20, 128, 160), (1, 1, 8, 8)]
FRAMES = [1, 3]


def source(n_in, n_out, device=None):
    """-> (i0, i1 long [n_out], w float64 [n_out]) of one axis."""
    d = torch.arange(n_out, dtype=F64, device=device)
    s = ((d + 0.5) * n_in / n_out - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0.to(F64)


def interp_matrix(n_in, n_out, device=None):
    """The 1-D interpolation as a dense float64 matrix [n_out][n_in] (two entries per row; one where i1 == i0)."""
    i0, i1, w = source(n_in, n_out, device)
    A = torch.zeros(n_out, n_in, dtype=F64, device=device)
    r = torch.arange(n_out, device=device)
    A.index_put_((r, i0), 1.0 - w, accumulate=True)
    A.index_put_((r, i1), w, accumulate=True)
    return A


def bilinear_fwd(x, F, h, w, H, W):
    """tokens x [F*h*w][C] -> [F*H*W][C], float64."""
    C = x.shape[1]
    xi = x.to(F64).reshape(F, h, w, C)
    y0, y1, wy = source(h, H, x.device)
    x0, x1, wx = source(w, W, x.device)
    wy, wx = wy.view(1, H, 1, 1), wx.view(1, 1, W, 1)
    rows = (1.0 - wy) * xi[:, y0] + wy * xi[:, y1]                       # [F][H][w][C]
    out = (1.0 - wx) * rows[:, :, x0] + wx * rows[:, :, x1]              # [F][H][W][C]
    return out.reshape(F * H * W, C)


def bilinear_bwd(g, F, h, w, H, W):
    """The exact adjoint: g [F*H*W][C] -> [F*h*w][C], float64, through the transposed interpolation matrices."""
    C = g.shape[1]
    Ay, Ax = interp_matrix(h, H, g.device), interp_matrix(w, W, g.device)
    gi = g.to(F64).reshape(F, H, W, C)
    return torch.einsum("yi,fyxc,xj->fijc", Ay, gi, Ax).reshape(F * h * w, C)


def logits_up_fwd(tok, F, h, w, H, W, nc):
    """tokens [F*h*w][pitch >= nc] -> NCHW [F][nc][H][W], float64."""
    return bilinear_fwd(tok[:, :nc], F, h, w, H, W).reshape(F, H, W, nc).permute(0, 3, 1, 2).contiguous()


def logits_up_bwd(g, F, h, w, H, W):
    """NCHW g [F][nc][H][W] -> tokens [F*h*w][nc], float64."""
    nc = g.shape[1]
    return bilinear_bwd(g.to(F64).permute(0, 2, 3, 1).reshape(F * H * W, nc), F, h, w, H, W)


def rows_broadcast(v, M, groups, scale, base=None):
    """out [M][C] = (base) + v[group of the row] * scale, float64; groups are contiguous blocks of M / groups rows."""
    assert groups > 0 and M % groups == 0 and v.shape[0] == groups
    out = (v.to(F64) * scale).repeat_interleave(M // groups, dim=0)
    return out if base is None else base.to(F64) + out


def group_sums(x, groups, unit=0):
    """-> float64 [groups][C] column sums of every statistic group."""
    idx = group_rows(x.shape[0], groups, unit, x.device)
    return x.to(F64)[idx.reshape(-1)].view(groups, -1, x.shape[1]).sum(1)


def maxpool3x3s2_taps(z, frames, H, W):
    """First-maximum taps of nn.MaxPool2d(3, 2, 1) on tokens z [frames*H*W][C] -> uint8 [frames*Hp*Wp][C], tap = ky * 3 + kx."""
    C = z.shape[1]
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    zi = z.to(F64).view(frames, H, W, C)
    pad = torch.full((frames, 2 * Hp + 1, 2 * Wp + 1, C), float("-inf"), dtype=F64, device=z.device)
    pad[:, 1:H + 1, 1:W + 1] = zi                                        # pad[y + 1][x + 1] = z[y][x]: window row 2 yo - 1 + ky -> 2 yo + ky
    win = torch.stack([pad[:, ky:ky + 2 * Hp:2, kx:kx + 2 * Wp:2] for ky in range(3) for kx in range(3)])    # [9][F][Hp][Wp][C]
    mx = win.max(0).values
    t = torch.arange(9, device=z.device).view(9, 1, 1, 1, 1)
    first = torch.where(win == mx, t, torch.full_like(t, 9)).min(0).values
    assert int(first.max()) <= 8
    return first.to(torch.uint8).reshape(frames * Hp * Wp, C)
