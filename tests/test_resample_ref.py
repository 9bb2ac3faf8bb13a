"""tests/resample_ref.py (the float64 reference of the resampling and pooling kernels) checked on the CPU before any kernel is held
against it: against F.interpolate(mode="bilinear", align_corners=False) in float64 and autograd through it at every geometry of the
GPU contract, the adjoint identity, the identity resize, and the first-maximum taps against F.max_pool2d(return_indices=True)."""
import pytest
import torch
import torch.nn.functional as F

import resample_ref as R

F64 = torch.float64
GEOMS = [(f, *g) for g in R.BILINEAR_GEOMS + R.LOGITS_GEOMS for f in R.FRAMES]
IDS = [f"f{f}-{h}x{w}-{H}x{W}" for f, h, w, H, W in GEOMS]


def _nchw(t, frames, h, w):
    return t.view(frames, h, w, t.shape[1]).permute(0, 3, 1, 2)


def _tok(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("frames,h,w,H,W", GEOMS, ids=IDS)
def test_bilinear_equals_float64_interpolate_and_its_autograd(frames, h, w, H, W):
    torch.manual_seed(h * 1000 + w * 100 + H + W)
    C = 5
    x = torch.randn(frames * h * w, C, dtype=F64, requires_grad=True)
    y = F.interpolate(_nchw(x, frames, h, w), size=(H, W), mode="bilinear", align_corners=False)
    g = torch.randn(frames * H * W, C, dtype=F64)
    (_tok(y) * g).sum().backward()
    assert float((R.bilinear_fwd(x.detach(), frames, h, w, H, W) - _tok(y.detach())).abs().max()) < 1e-13
    assert float((R.bilinear_bwd(g, frames, h, w, H, W) - x.grad).abs().max()) < 1e-12


@pytest.mark.parametrize("frames,h,w,H,W", GEOMS, ids=IDS)
def test_adjoint_identity(frames, h, w, H, W):
    """<up(x), g> == <x, up^T(g)> to 1e-12 (relative to the product of the norms)."""
    torch.manual_seed(h + 7 * w + 13 * H + 29 * W)
    C = 3
    x = torch.randn(frames * h * w, C, dtype=F64)
    g = torch.randn(frames * H * W, C, dtype=F64)
    lhs = (R.bilinear_fwd(x, frames, h, w, H, W) * g).sum()
    rhs = (x * R.bilinear_bwd(g, frames, h, w, H, W)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float(x.norm() * g.norm())


@pytest.mark.parametrize("h,w", [(6, 10), (1, 1), (13, 9)])
def test_identity_resize_returns_the_input_exactly(h, w):
    x = torch.randn(2 * h * w, 4, dtype=F64)
    assert torch.equal(R.bilinear_fwd(x, 2, h, w, h, w), x)
    assert torch.equal(R.bilinear_bwd(x, 2, h, w, h, w), x)
    assert torch.equal(R.interp_matrix(h, h), torch.eye(h, dtype=F64))


def test_interp_matrix_rows_are_convex_weights():
    for n_in, n_out in [(1, 4), (5, 11), (7, 9), (13, 5), (16, 128), (5, 37)]:
        A = R.interp_matrix(n_in, n_out)
        assert float((A.sum(1) - 1).abs().max()) < 1e-15 and float(A.min()) >= 0 and int((A != 0).sum(1).max()) <= 2


@pytest.mark.parametrize("nc,pitch", [(1, 1), (9, 9), (9, 64), (12, 64), (26, 64)])
@pytest.mark.parametrize("frames,h,w,H,W", [(2, 4, 5, 30, 37), (1, 1, 1, 8, 8), (3, 5, 6, 40, 48)])
def test_logits_forms_equal_interpolate(nc, pitch, frames, h, w, H, W):
    torch.manual_seed(nc + pitch + H)
    tok = torch.randn(frames * h * w, pitch, dtype=F64)
    x = tok[:, :nc].clone().requires_grad_(True)
    y = F.interpolate(_nchw(x, frames, h, w), size=(H, W), mode="bilinear", align_corners=False)
    g = torch.randn(frames, nc, H, W, dtype=F64)
    (y * g).sum().backward()
    got = R.logits_up_fwd(tok, frames, h, w, H, W, nc)
    assert got.shape == (frames, nc, H, W) and float((got - y.detach()).abs().max()) < 1e-13
    assert float((R.logits_up_bwd(g, frames, h, w, H, W) - x.grad).abs().max()) < 1e-12


def test_rows_broadcast_and_group_sums():
    torch.manual_seed(3)
    v = torch.randn(3, 8, dtype=F64)
    base = torch.randn(3 * 7, 8, dtype=F64)
    out = R.rows_broadcast(v, 21, 3, 1 / 37)
    for r in range(21):
        assert torch.equal(out[r], v[r // 7] * (1 / 37))
    assert torch.equal(R.rows_broadcast(v, 21, 3, 0.5, base=base), base + R.rows_broadcast(v, 21, 3, 0.5))
    # group_sums is the adjoint of rows_broadcast (contiguous groups); interleaved units against an explicit loop
    assert float((R.group_sums(base, 3) - base.view(3, 7, 8).sum(1)).abs().max()) < 1e-14
    x = torch.randn(2 * 3 * 4, 8, dtype=F64)                  # 2 rounds x 3 groups x units of 4 rows
    want = torch.stack([sum(x[(k * 3 + g) * 4:(k * 3 + g + 1) * 4].sum(0) for k in range(2)) for g in range(3)])
    assert float((R.group_sums(x, 3, unit=4) - want).abs().max()) < 1e-14


def _inputs(kind, n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, dtype=F64, generator=g)
    if kind == "relu":
        x = x.clamp_min(0)
    elif kind == "levels":                                    # four levels: almost every window has ties
        x = torch.randint(0, 4, (n, C), generator=g).to(F64) - 1.5
    elif kind == "const":
        x = torch.full((n, C), 0.25, dtype=F64)
    return x


@pytest.mark.parametrize("kind", ["random", "relu", "levels", "const"])
@pytest.mark.parametrize("frames,H,W", [(1, 1, 1), (2, 2, 2), (1, 1, 9), (3, 37, 53), (2, 16, 16)])
def test_taps_equal_max_pool2d_indices_with_forced_ties(kind, frames, H, W):
    C = 6
    z = _inputs(kind, frames * H * W, C, frames + H + W)
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    val, ind = F.max_pool2d(_nchw(z, frames, H, W), 3, 2, 1, return_indices=True)       # ind: y * W + x of the first maximum
    taps = R.maxpool3x3s2_taps(z, frames, H, W).view(frames, Hp, Wp, C).permute(0, 3, 1, 2).long()
    yo = torch.arange(Hp).view(1, 1, Hp, 1)
    xo = torch.arange(Wp).view(1, 1, 1, Wp)
    assert torch.equal((2 * yo - 1 + taps // 3) * W + (2 * xo - 1 + taps % 3), ind)
    assert torch.equal(R.maxpool3x3s2(z, frames, H, W), _tok(val))
    # the scatter through the taps is the adjoint of the pooling as autograd sees it
    zz = _nchw(z, frames, H, W).clone().requires_grad_(True)
    g = torch.randn(frames * Hp * Wp, C, dtype=F64)
    (_tok(F.max_pool2d(zz, 3, 2, 1)) * g).sum().backward()
    got = R.maxpool3x3s2_bwd(g, R.maxpool3x3s2_taps(z, frames, H, W), frames, H, W)
    assert torch.equal(got, _tok(zz.grad))


def test_forced_ties_distinguish_first_from_last_maximum():
    """On a constant map the first maximum is the first in-map tap of every window, never the last one."""
    z = torch.full((5 * 5, 2), 1.0, dtype=F64)
    taps = R.maxpool3x3s2_taps(z, 1, 5, 5).view(3, 3, 2)
    assert int(taps[0, 0, 0]) == 4 and int(taps[0, 1, 0]) == 3 and int(taps[1, 0, 0]) == 1 and int(taps[1, 1, 0]) == 0
