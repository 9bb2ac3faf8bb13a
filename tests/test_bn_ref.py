"""tests/bn_ref.py (the float64 reference of the BatchNorm kernels) checked on the CPU before any kernel is held against it: against
nn.BatchNorm2d in float64 called once per statistic group (base18.py:86-89), forward, running statistics and autograd gradients, for
contiguous and interleaved groups, residual and ReLU, training and eval, and two ranks of a SyncBatchNorm split."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_ref as R

F64 = torch.float64


def _module(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=g, dtype=F64))
        bn.bias.copy_(0.3 * torch.randn(C, generator=g, dtype=F64))
        bn.running_mean.copy_(0.2 * torch.randn(C, generator=g, dtype=F64))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g, dtype=F64))
    return bn


def _torch_bn(x, bn, frames, h, w, groups, unit_frames, resid, relu, training):
    """nn.BatchNorm2d on NCHW frames, one call per statistic group in group order; tokens in, tokens out."""
    C = x.shape[1]
    xi = x.view(frames, h, w, C).permute(0, 3, 1, 2)
    bn.train(training)
    idx = R.group_rows(frames, groups, unit_frames)           # frames of each group (a "row" of this index is one frame)
    out = [None] * frames
    for g in range(groups):
        fr = idx[g]
        yg = bn(xi[fr])
        for j, f in enumerate(fr.tolist()):
            out[f] = yg[j:j + 1]
    y = torch.cat(out, 0).permute(0, 2, 3, 1).reshape(-1, C)
    if resid is not None:
        y = y + resid
    return F.relu(y) if relu else y


@pytest.mark.parametrize("frames,h,w,C,groups,unit_frames,res,relu,training",
                         [(4, 6, 5, 16, 1, 0, False, True, True), (4, 6, 5, 16, 4, 0, True, True, True),
                          (6, 4, 4, 8, 3, 1, False, True, True), (8, 3, 5, 8, 2, 2, True, False, True),
                          (4, 6, 5, 16, 2, 0, True, True, False), (6, 4, 4, 8, 3, 1, False, True, False)])
def test_forward_and_backward_equal_float64_batchnorm2d(frames, h, w, C, groups, unit_frames, res, relu, training):
    torch.manual_seed(frames * C + groups)
    M = frames * h * w
    x = (torch.randn(M, C, dtype=F64) * 2 + 3).requires_grad_(True)
    r = torch.randn(M, C, dtype=F64).requires_grad_(True) if res else None
    dy = torch.randn(M, C, dtype=F64)
    bn = _module(C, C + groups)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    unit = unit_frames * h * w
    want = _torch_bn(x, bn, frames, h, w, groups, unit_frames, r, relu, training)
    (want * dy).sum().backward()
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    got = R.forward(x.detach(), gamma, beta, groups=groups, unit=unit, resid=r.detach() if res else None, relu=relu,
                    training=training, running_mean=rm0, running_var=rv0)
    assert torch.allclose(got["y"], want.detach(), rtol=0, atol=1e-12)
    if training:
        assert torch.allclose(got["running_mean"], bn.running_mean, rtol=0, atol=1e-14)
        assert torch.allclose(got["running_var"], bn.running_var, rtol=1e-13, atol=0)
    mask = got["y"] > 0 if relu else None
    b = R.backward(dy, x.detach(), got["mean"], got["rstd"], gamma, groups=groups, unit=unit, mask=mask, training=training)
    assert torch.allclose(b["dx"], x.grad, rtol=1e-10, atol=1e-12), float((b["dx"] - x.grad).abs().max())
    assert torch.allclose(b["group_sums"][0], bn.bias.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(b["group_sums"][1], bn.weight.grad, rtol=1e-10, atol=1e-12)
    if res:
        assert torch.allclose(b["dresid"], r.grad, rtol=0, atol=0)


def test_interleaved_groups_are_the_frames_of_every_clip():
    """unit > 0: group g owns the units g, g + G, ... ; the frame-major reorder of the same data with contiguous groups gives the
    same statistics, outputs and gradients."""
    clips, T, hw, C = 3, 4, 6, 8
    x = torch.randn(clips * T * hw, C, dtype=F64) * 3 + 1
    dy = torch.randn_like(x)
    gamma, beta = torch.rand(C, dtype=F64) + 0.5, torch.randn(C, dtype=F64)
    fm = lambda t: t.view(clips, T, hw, C).transpose(0, 1).reshape(-1, C)            # noqa: E731
    a = R.forward(x, gamma, beta, groups=T, unit=hw)
    b = R.forward(fm(x), gamma, beta, groups=T)
    assert torch.allclose(a["mean"], b["mean"], rtol=0, atol=1e-14) and torch.allclose(a["var"], b["var"], rtol=1e-14, atol=0)
    assert torch.allclose(fm(a["y"]), b["y"], rtol=0, atol=1e-13)
    ga = R.backward(dy, x, a["mean"], a["rstd"], gamma, groups=T, unit=hw, mask=a["y"] > 0)
    gb = R.backward(fm(dy), fm(x), b["mean"], b["rstd"], gamma, groups=T, mask=b["y"] > 0)
    assert torch.allclose(fm(ga["dx"]), gb["dx"], rtol=0, atol=1e-13)
    assert torch.allclose(ga["group_sums"], gb["group_sums"], rtol=0, atol=1e-12)


def test_rows_total_is_two_ranks_of_one_batch():
    """SyncBatchNorm: global statistics, s1 / s2 summed over two ranks, divided by the global rows - the gradient of the whole batch."""
    M, C = 96, 8
    x = torch.randn(M, C, dtype=F64) * 2 - 1
    dy = torch.randn(M, C, dtype=F64)
    gamma, beta = torch.rand(C, dtype=F64) + 0.5, torch.randn(C, dtype=F64)
    full = R.forward(x, gamma, beta)
    want = R.backward(dy, x, full["mean"], full["rstd"], gamma, mask=full["y"] > 0)
    halves = []
    for sl in (slice(0, M // 2), slice(M // 2, M)):
        part = R.backward(dy[sl], x[sl], full["mean"], full["rstd"], gamma, mask=full["y"][sl] > 0)
        halves.append(part)
    assert torch.allclose(halves[0]["s1"] + halves[1]["s1"], want["s1"], rtol=1e-13, atol=1e-13)
    # with the all-reduced sums, each rank's dx is the whole batch's: checked through the formula with rows_total
    s1 = halves[0]["s1"] + halves[1]["s1"]
    s2 = halves[0]["s2"] + halves[1]["s2"]
    xhat = (x - full["mean"]) * full["rstd"]
    dyr = dy * (full["y"] > 0)
    dx = gamma * full["rstd"] * (dyr - (s1 + xhat * s2) / M)
    assert torch.allclose(dx, want["dx"], rtol=0, atol=1e-13)


def test_maxpool_reference_and_its_tap_scatter():
    """maxpool3x3s2 against F.max_pool2d, and the tap scatter against autograd through it (taps = the first maximum in (ky, kx)
    order, from max_pool2d's indices)."""
    frames, H, W, C = 2, 7, 6, 4
    z = torch.randn(frames * H * W, C, dtype=F64).requires_grad_(True)
    p = R.maxpool3x3s2(z, frames, H, W)
    zi = z.detach().view(frames, H, W, C).permute(0, 3, 1, 2)
    want, ind = F.max_pool2d(zi, 3, 2, 1, return_indices=True)
    assert torch.equal(p.detach(), want.permute(0, 2, 3, 1).reshape(-1, C))
    dout = torch.randn_like(p)
    (p * dout).sum().backward()
    Hp, Wp = want.shape[2:]
    yy, xx = ind // W, ind % W
    yo = torch.arange(Hp).view(1, 1, Hp, 1)
    xo = torch.arange(Wp).view(1, 1, 1, Wp)
    tap = ((yy - (2 * yo - 1)) * 3 + (xx - (2 * xo - 1))).permute(0, 2, 3, 1).reshape(-1, C).to(torch.uint8)
    got = R.maxpool3x3s2_bwd(dout, tap, frames, H, W)
    assert torch.allclose(got, z.grad, rtol=0, atol=1e-15)
