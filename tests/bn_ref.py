"""Float64 reference of the token-layout BatchNorm (stswincl_amd/csrc/headops.hip, include/stswin_hip.h) in the kernels' call forms.

Shared by tests/test_bn_ref.py (CPU: the reference against float64 autograd of nn.BatchNorm2d) and tests/test_hip_bn_contract.py
(GPU: every BatchNorm kernel against it).  Nothing here calls the library: it is plain torch, run on whatever device its inputs live
on.  Written from nn.BatchNorm2d's semantics:

  x     [M][C] tokens, M = groups x group_rows.  Statistic group g owns rows g * group_rows ... (contiguous, unit = 0) or the units of
        `unit` rows g, g + G, g + 2G, ... (interleaved, unit > 0: frame t of every clip when clips are stored clip-major).
  y     = act((x - mean_g) * rstd_g * gamma + beta [+ resid]),  mean / biased variance of the group, rstd = (var + eps)^-1/2.
  running statistics: one nn.BatchNorm2d call per group, group 0 first (base18.py:86-89):
        running = (1 - momentum) * running + momentum * stat, with the UNBIASED variance (n / (n - 1)).
  backward: dyr = dy * (y > 0 if relu), s1_g = sum dyr, s2_g = sum dyr * xhat (xhat = (x - mean) * rstd),
        training: dx = gamma * rstd * (dyr - (s1_g + xhat * s2_g) / n)   (n = rows of the group over all ranks: rows_total)
        eval:     dx = gamma * rstd * dyr
        dresid = dyr, dbeta = sum_g s1_g, dgamma = sum_g s2_g (group_sums = [dbeta; dgamma]).
"""
from __future__ import annotations

import torch

F64 = torch.float64


def group_rows(M, groups, unit=0, device=None):
    """[groups][M / groups] physical row indices of every statistic group (in the order the group's rows are visited)."""
    assert groups > 0 and M % groups == 0
    gr = M // groups
    if unit <= 0:
        return torch.arange(M, device=device).view(groups, gr)
    assert M % (groups * unit) == 0
    # unit u belongs to group u % groups; a group's units in increasing order
    return torch.arange(M, device=device).view(M // (groups * unit), groups, unit).transpose(0, 1).reshape(groups, gr)


def _grouped(t, idx):
    return t[idx.reshape(-1)].view(*idx.shape, t.shape[-1])          # [groups][group_rows][C]


def _scatter(v, idx, M):
    out = torch.empty(M, v.shape[-1], dtype=v.dtype, device=v.device)
    out[idx.reshape(-1)] = v.reshape(-1, v.shape[-1])
    return out


def stats(x, groups=1, unit=0):
    """-> (mean, biased var) float64 [groups][C]: two-pass, the mean subtracted before squaring."""
    xg = _grouped(x.to(F64), group_rows(x.shape[0], groups, unit, x.device))
    mean = xg.mean(1)
    var = ((xg - mean.unsqueeze(1)) ** 2).mean(1)
    return mean, var


def running_update(mean, var, running_mean, running_var, n, momentum=0.1):
    """nn.BatchNorm2d's running statistics after one call per group (group 0 first), n rows per group: float64 [C] each."""
    rm, rv = running_mean.to(F64).clone(), running_var.to(F64).clone()
    unb = n / max(n - 1, 1)
    for g in range(mean.shape[0]):
        rm = (1 - momentum) * rm + momentum * mean[g]
        rv = (1 - momentum) * rv + momentum * var[g] * unb
    return rm, rv


def forward(x, gamma, beta, *, groups=1, unit=0, resid=None, relu=True, eps=1e-5, momentum=0.1, training=True,
            running_mean=None, running_var=None):
    """The forward in float64.  training: batch statistics (and, with running_mean / running_var, their updated values);
    eval: the running statistics for every group.  Returns a dict: mean, var (biased), rstd [groups][C], y [M][C] and, when given
    running statistics in training, running_mean / running_var [C]."""
    M, C = x.shape
    idx = group_rows(M, groups, unit, x.device)
    if training:
        mean, var = stats(x, groups, unit)
    else:
        mean = running_mean.to(F64).view(1, C).expand(groups, C)
        var = running_var.to(F64).view(1, C).expand(groups, C)
    rstd = (var + eps).rsqrt()
    xg = _grouped(x.to(F64), idx)
    z = (xg - mean.unsqueeze(1)) * (rstd * gamma.to(F64)).unsqueeze(1) + beta.to(F64)
    y = _scatter(z, idx, M)
    if resid is not None:
        y = y + resid.to(F64)
    if relu:
        y = y.clamp_min(0)
    res = {"mean": mean, "var": var, "rstd": rstd, "y": y}
    if training and running_mean is not None:
        res["running_mean"], res["running_var"] = running_update(mean, var, running_mean, running_var, M // groups, momentum)
    return res


def backward(dy, x, mean, rstd, gamma, *, groups=1, unit=0, mask=None, training=True, rows_total=0):
    """The backward in float64 from given statistics (mean / rstd [groups][C], as the forward used them).

    mask: the ReLU mask (y > 0) as a bool [M][C], or None for no ReLU; a GPU test passes the mask of the KERNEL's output, so that an
    output rounded to 0 or across 0 is a selection, not an arithmetic error.  rows_total: rows of a group over all ranks (SyncBatchNorm:
    s1 / s2 summed over the ranks, divided by the global count); 0 = the local group rows.
    Returns dx, dresid (= dyr) [M][C], s1, s2 [groups][C] and group_sums [2][C] (dbeta; dgamma)."""
    M, C = x.shape
    idx = group_rows(M, groups, unit, x.device)
    dyr = dy.to(F64)
    if mask is not None:
        dyr = torch.where(mask, dyr, torch.zeros((), dtype=F64, device=dyr.device))
    xhat = (_grouped(x.to(F64), idx) - mean.to(F64).unsqueeze(1)) * rstd.to(F64).unsqueeze(1)
    dg = _grouped(dyr, idx)
    s1, s2 = dg.sum(1), (dg * xhat).sum(1)
    a = (gamma.to(F64) * rstd.to(F64)).unsqueeze(1)
    if training:
        n = rows_total if rows_total > 0 else M // groups
        dxg = a * (dg - (s1.unsqueeze(1) + xhat * s2.unsqueeze(1)) / n)
    else:
        dxg = a * dg
    return {"dx": _scatter(dxg, idx, M), "dresid": dyr, "s1": s1, "s2": s2, "group_sums": torch.stack([s1.sum(0), s2.sum(0)])}


def maxpool3x3s2(z, frames, H, W):
    """nn.MaxPool2d(3, 2, 1) of tokens z [frames*H*W][C] -> [frames*Hp*Wp][C] (float64)."""
    C = z.shape[1]
    zi = z.to(F64).view(frames, H, W, C).permute(0, 3, 1, 2)
    p = torch.nn.functional.max_pool2d(zi, 3, 2, 1)
    return p.permute(0, 2, 3, 1).reshape(-1, C)


def maxpool3x3s2_bwd(dout, arg, frames, H, W):
    """Scatter of dout [frames*Hp*Wp][C] through the winning taps arg (uint8, tap = ky * 3 + kx of the 3 x 3 window at
    (2 yo - 1, 2 xo - 1)) into [frames*H*W][C], float64 (the taps are the selection, given)."""
    C = dout.shape[1]
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    a = arg.to(torch.long).view(frames, Hp, Wp, C)
    yo = torch.arange(Hp, device=dout.device).view(1, Hp, 1, 1)
    xo = torch.arange(Wp, device=dout.device).view(1, 1, Wp, 1)
    yy = 2 * yo - 1 + a // 3
    xx = 2 * xo - 1 + a % 3
    assert bool(((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).all()), "a tap outside the map"
    f = torch.arange(frames, device=dout.device).view(frames, 1, 1, 1)
    c = torch.arange(C, device=dout.device).view(1, 1, 1, C)
    flat = ((f * H + yy) * W + xx) * C + c
    out = torch.zeros(frames * H * W * C, dtype=F64, device=dout.device)
    out.index_add_(0, flat.reshape(-1), dout.to(F64).view(frames, Hp, Wp, C).reshape(-1))
    return out.view(frames * H * W, C)


def errors(got, ref):
    """(max |got - ref| / max |ref|, ||got - ref|| / ||ref||), float64 on ref's device."""
    g = got.to(device=ref.device, dtype=F64)
    r = ref.to(F64)
    diff = g - r
    return float(diff.abs().max()) / max(float(r.abs().max()), 1e-300), float(diff.norm() / r.norm().clamp_min(1e-300))
