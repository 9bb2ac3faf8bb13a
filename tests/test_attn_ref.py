"""tests/attn_ref.py (the float64 reference of the attention kernels) checked on the CPU before any kernel is held against it:
against the oracle's window_attention (swin_512.py:109-141), against float64 autograd of its own forward, across the three
bias_windows forms, and against the fp32 helpers the older kernel tests use."""
import pytest
import torch

import attn_ref as R
from oracle import stswin_oracle as O

F64 = torch.float64


def _case(ws, C, heads, nW, B, seed, T=2):
    g = torch.Generator().manual_seed(seed)
    N = ws * ws
    nB_ = B * nW
    qkv = torch.randn(nB_ * T * N, 3 * C, generator=g, dtype=F64)
    qkv[:, :C] *= (C // heads) ** -0.5
    bias = torch.randn(heads, N, N, generator=g, dtype=F64) * 0.5          # [heads][query][key]
    dout = torch.randn(nB_ * T * N, C, generator=g, dtype=F64)
    return qkv, bias, dout, nB_, N


def _shift_mask(ws, nW):
    side = int(round(nW ** 0.5))
    return O.shift_attn_mask(side * ws, side * ws, ws, ws // 2).to(F64)      # [nW][N][N] in {0, -100}, symmetric


@pytest.mark.parametrize("ws,C,heads,shift", [(4, 32, 2, 2), (4, 32, 2, 0), (2, 24, 3, 1)])
def test_forward_equals_the_oracle_window_attention(ws, C, heads, shift):
    """O.window_attention projects x with qkv.weight, scales q, adds table[index] tiled over the frames and the mask, and
    projects the result: with an identity projection and the same table, its output is attn_ref's on the pre-scaled q | k | v."""
    torch.manual_seed(ws * C + shift)
    T, N, B = 2, ws * ws, 2
    nW = 4
    d = C // heads
    x = torch.randn(B * nW, T, N, C, dtype=F64)
    w = torch.randn(3 * C, C, dtype=F64) / C ** 0.5
    b = torch.randn(3 * C, dtype=F64) * 0.1
    table = torch.randn((2 * ws - 1) ** 2, heads, dtype=F64) * 0.5
    sd = {"a.qkv.weight": w, "a.qkv.bias": b, "a.relative_position_bias_table": table,
          "a.relative_position_index": O.relative_position_index(ws), "a.proj.weight": torch.eye(C, dtype=F64),
          "a.proj.bias": torch.zeros(C, dtype=F64)}
    mask = _shift_mask(ws, nW) if shift else None
    want = O.window_attention(x, sd, "a.", heads, ws, mask).reshape(-1, C)
    qkv = x.reshape(-1, C) @ w.t() + b
    qkv[:, :C] *= d ** -0.5
    biasT = O.expanded_rel_bias(sd, "a.", ws, heads).transpose(1, 2)
    maskT = mask.transpose(1, 2) if mask is not None else None
    got = R.attention(qkv, biasT, maskT, T=T, ws=ws, heads=heads, C=C, nW=nW)["out"]
    assert torch.allclose(got, want, rtol=0, atol=1e-12), float((got - want).abs().max())


@pytest.mark.parametrize("ws,C,heads,nW,scale", [(4, 32, 2, 4, 1.0), (4, 64, 4, 4, 0.25), (2, 24, 3, 1, 0.7)])
def test_backward_equals_float64_autograd(ws, C, heads, nW, scale):
    """The written-out backward against torch.autograd through the forward (dq carries `scale`, dbias is the gradient of the
    per-head [N][N] table in the transposed layout, colsum the column sums of the scaled dq)."""
    qkv, bias, dout, nB_, N = _case(ws, C, heads, nW, 2, ws * C + nW)
    mask = torch.where(torch.rand(nW, N, N, generator=torch.Generator().manual_seed(5)) < 0.25, -100.0, 0.0).to(F64)
    qr = qkv.clone().requires_grad_(True)
    bT = bias.transpose(1, 2).contiguous().requires_grad_(True)
    mT = mask.transpose(1, 2).contiguous()
    out = R.attention(qr, bT, mT, T=2, ws=ws, heads=heads, C=C, nW=nW)["out"]
    (out * dout).sum().backward()
    got = R.attention(qkv, bias.transpose(1, 2), mT, T=2, ws=ws, heads=heads, C=C, nW=nW, dout=dout, scale=scale)
    want_dq = qr.grad[:, :C] * scale
    for name, a, b in (("dq", got["dq"], want_dq), ("dk", got["dk"], qr.grad[:, C:2 * C]), ("dv", got["dv"], qr.grad[:, 2 * C:]),
                       ("dbiasT", got["dbiasT"], bT.grad), ("colsum", got["colsum"], want_dq.sum(0))):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12), (name, float((a - b).abs().max()))
    assert torch.equal(got["dqkv"], torch.cat([got["dq"], got["dk"], got["dv"]], 1))


@pytest.mark.parametrize("ws,heads,nW", [(4, 2, 9), (2, 3, 16)])
def test_the_three_bias_forms_agree(ws, heads, nW):
    """biasT + maskT ("1"), the per-window pre-summed table ("nW") and the slot table + index ("U", slots deduplicated the way
    ops.unique_windows does) encode the same bias + mask: same scores, output and gradients - bitwise, the additions are the same."""
    C = 8 * heads
    qkv, bias, dout, nB_, N = _case(ws, C, heads, nW, 3, ws * nW)
    side = int(round(nW ** 0.5))
    mask = O.shift_attn_mask(side * ws, side * ws, ws, max(ws // 2, 1)).to(F64)
    biasT, maskT = bias.transpose(1, 2).contiguous(), mask.transpose(1, 2).contiguous()
    per_window = biasT.unsqueeze(0) + maskT.unsqueeze(1)                              # [nW][heads][key][query]
    umask, inv = torch.unique(mask.reshape(nW, -1), dim=0, return_inverse=True)
    assert 1 < umask.shape[0] < nW                                                   # a real deduplication
    slots = biasT.unsqueeze(0) + umask.reshape(-1, N, N).transpose(1, 2).unsqueeze(1)
    kw = dict(T=2, ws=ws, heads=heads, C=C, nW=nW, dout=dout, scale=0.5)
    r1 = R.attention(qkv, biasT, maskT, **kw)
    rw = R.attention(qkv, per_window, None, **kw)
    ru = R.attention(qkv, slots, None, bias_index=inv.to(torch.int32), **kw)
    for key in ("out", "dqkv", "dbiasT", "colsum"):
        assert torch.equal(r1[key], rw[key]) and torch.equal(r1[key], ru[key]), key
    # a window given the wrong slot changes the result: the index is really used
    bad = inv.clone()
    bad[bad == bad[-1]] = (bad[-1] + 1) % umask.shape[0]
    assert not torch.allclose(R.attention(qkv, slots, None, bias_index=bad, **kw)["out"], r1["out"])


def test_matches_the_fp32_helpers_of_the_older_kernel_tests():
    """test_hip_attention._ref and test_hip_fp8._ref_attn (fp32) against attn_ref on the same inputs: fp32 rounding apart."""
    from test_hip_attention import _ref
    from test_hip_fp8 import _ref_attn
    ws, C, heads, nW = 4, 64, 4, 4
    qkv, bias, dout, nB_, N = _case(ws, C, heads, nW, 2, 3)
    mask = _shift_mask(ws, nW)
    want = R.attention(qkv, bias.transpose(1, 2), mask.transpose(1, 2), T=2, ws=ws, heads=heads, C=C, nW=nW)["out"]
    scl = float(want.abs().max())
    for helper in (_ref, _ref_attn):
        for m in (mask, None):
            got = helper(qkv.float(), bias.float(), m.float() if m is not None else None, nB_, nW, 2, N, heads, C)
            w = want if m is not None else R.attention(qkv, bias.transpose(1, 2), None, T=2, ws=ws, heads=heads, C=C, nW=nW)["out"]
            assert float((got.double() - w).abs().max()) <= 2e-6 * scl


def test_e4m3_round_trip_and_scales():
    """e4m3_quantise: one amax / 448 scale per (problem, head block), every dequantised value within half an e4m3 step (2^-4
    relative; 2^-10 of the scale in the subnormal range) of its input, and the block maximum exactly representable."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 48, generator=g)
    x[3, 5] = 9.0
    q8, sc = R.e4m3_quantise(x, 16, 12)
    assert q8.dtype == torch.uint8 and sc.shape == (4, 4)
    amax = x.abs().reshape(4, 16, 4, 12).amax(dim=(1, 3))
    assert torch.allclose(sc, amax / 448.0, rtol=1e-6, atol=0)
    y = R.e4m3_dequantise(q8, sc, 16, 12)
    full = sc.double().repeat_interleave(16, 0).repeat_interleave(12, 1)
    tol = torch.maximum(x.double().abs() * 2.0 ** -4, full * 2.0 ** -10) * 1.0001
    assert bool(((y - x.double()).abs() <= tol).all())
    assert float(y[3, 5]) == pytest.approx(9.0, rel=1e-6)
