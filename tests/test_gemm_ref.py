"""tests/gemm_ref.py (the float64 reference and the derived bound of the gemm_nt contract) held to independent definitions on the CPU:
ref() against float64 F.linear / F.gelu(approximate='none') / autograd composed by hand per flag; bound()'s product term against the
fp32 torch product of the same operands at the shapes of tests/test_hip_gemm_nt_contract.py (the bound is not vacuously small); and
the bf16 epilogue's GELU polynomial, evaluated in float32 from the coefficients parsed out of stswincl_amd/csrc/common.h, against
float64 erf - the constants bound() uses are the ones the header documents."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_bits_are_the_headers():
    from stswincl_amd import hip
    for name in ("GELU", "RESID", "MUL_DGELU", "OUT_F32", "ACCUM", "RELU", "MUL_R", "C2_DGELU"):
        assert getattr(G, name) == getattr(hip, "GF_" + name), name


def _operands(seed, rows, M, N, Kseg, S, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(rows, Kseg, generator=g).to(dtype)
    B = (torch.randn(N, S * Kseg, generator=g) / (S * Kseg) ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g)
    R = torch.randn(rows, N, generator=g).to(dtype)
    return A, B, bias, R


def _autograd_dgelu(x):
    x = x.clone().requires_grad_(True)
    F.gelu(x, approximate="none").sum().backward()
    return x.grad


def test_gelu_and_its_derivative_are_torchs():
    x = torch.linspace(-9, 9, 20001, dtype=F64)
    assert float((G.gelu(x) - F.gelu(x, approximate="none")).abs().max()) < 1e-14      # (a few float64 ulps of |x| <= 9)
    assert float((G.dgelu(x) - _autograd_dgelu(x)).abs().max()) < 1e-14
    # the two curvature constants of bound(): max |gelu'| = 1.129 < GELU_SLOPE; gelu''(0) = 2 pdf(0) = 0.798 (GELU2_MAX is the issue's)
    assert 1.128 < float(G.dgelu(x).abs().max()) < G.GELU_SLOPE
    assert abs(2.0 / math.sqrt(2 * math.pi) - 0.7979) < 1e-4


@pytest.mark.parametrize("flags,with_bias,c2", [(0, False, False), (0, True, False), (G.GELU, True, True), (G.GELU | G.C2_DGELU, True, True),
                                                (G.RESID, True, False), (G.MUL_R, False, False), (G.MUL_DGELU, False, False),
                                                (G.RELU, True, False), (G.RESID | G.RELU, True, False),
                                                (G.OUT_F32 | G.ACCUM, False, False)])
def test_ref_plain_linear_forms(flags, with_bias, c2):
    M, N, K = 37, 24, 64
    A, B, bias, R = _operands(3, M, M, N, K, 1)
    prev = torch.randn(M, N, generator=torch.Generator().manual_seed(9))
    r = G.ref(A, B, M=M, bias=bias if with_bias else None, scale=0.25, scale_cols=10, R=R, flags=flags, c_prev=prev)
    lin = F.linear(A.double(), B.double(), bias.double() if with_bias else None)
    lin[:, :10] *= 0.25
    assert torch.allclose(r["pre"], lin, rtol=0, atol=1e-13)
    if c2:
        want2 = _autograd_dgelu(lin) if flags & G.C2_DGELU else lin
        assert torch.allclose(r["c2"], want2, rtol=0, atol=1e-13)
    v = F.gelu(lin, approximate="none") if flags & G.GELU else lin
    if flags & G.RESID:
        v = v + R.double()
    if flags & G.MUL_R:
        v = v * R.double()
    if flags & G.MUL_DGELU:
        v = v * _autograd_dgelu(R.double())
    if flags & G.RELU:
        v = F.relu(v)
    assert torch.allclose(r["out"], v, rtol=0, atol=1e-13)
    assert torch.allclose(r["store"], v + prev.double() if flags & G.ACCUM else v, rtol=0, atol=1e-13)


def test_ref_gather_with_padding_rows_segments_and_gathered_residual():
    M, N, K, S, rows = 33, 20, 64, 3, 50
    A, B, bias, R = _operands(4, rows, M, N, K, S)
    g = torch.Generator().manual_seed(5)
    amap = torch.randint(-1, rows, (S, M), generator=g, dtype=torch.int32)
    amap[:, 5] = -1
    amap[1, :] = -1                                # a tap that is padding for every row
    rmap = torch.randperm(rows, generator=g)[:M].to(torch.int32)
    r = G.ref(A, B, M=M, S=S, a_rows=amap, bias=bias, R=R, r_rows=rmap, flags=G.RESID)
    want = torch.zeros(M, N, dtype=F64)
    for m in range(M):
        row = torch.cat([A[amap[s, m]].double() if amap[s, m] >= 0 else torch.zeros(K, dtype=F64) for s in range(S)])
        want[m] = B.double() @ row + bias.double() + R[rmap[m]].double()
    assert torch.allclose(r["out"], want, rtol=0, atol=1e-13)
    assert float(r["out"][5].sub(bias.double() + R[rmap[5]].double()).abs().max()) < 1e-13      # an all-padding row: bias + residual
    # block sums (what the column-sum table holds) and their scatter-free definition
    bs = G.block_sums(r["out"], 16)
    assert bs.shape == (3, N) and torch.allclose(bs[2], r["out"][32:].sum(0), rtol=0, atol=1e-12)
    assert torch.allclose(bs.sum(0), r["out"].sum(0), rtol=0, atol=1e-12)


def test_bf16_store_term_is_half_an_ulp_of_the_binade():
    """Correct rounding of the reference itself stays within the store term - and would NOT stay within 2^-9 * |ref|, the form the
    contract's issue states (the error at the top of a binade only)."""
    x = torch.cat([torch.linspace(-8, 8, 100001, dtype=F64), torch.tensor([0.0, 0.289930522, 1.0, 1.00390624, 2.0 ** -20], dtype=F64)])
    err = (x.to(torch.bfloat16).double() - x).abs()
    h = G.half_ulp_bf16(x.abs())
    assert bool((err <= h).all()) and bool((h <= 2.0 ** -8 * x.abs()).all()) and bool((h > 2.0 ** -9 * x.abs())[x != 0].all())
    assert float(h[100001]) == 0.0 and float(G.half_ulp_bf16(torch.tensor(1.0))) == 2.0 ** -8 and float(G.half_ulp_bf16(torch.tensor(0.99))) == 2.0 ** -9
    assert float((err / x.abs().clamp(min=1e-300)).max()) > 1.9 * 2.0 ** -9          # correct rounding loses up to 2^-8 relative


# (M, N, Kseg, S, dtype) of the GPU contract's cases: bound()'s product term must hold the fp32 torch product of the same operands
BOUND_SHAPES = [(8, 261, 576, 1, "bf16"), (200, 136, 128, 1, "bf16"), (37, 48, 192, 1, "bf16"), (200, 136, 320, 1, "bf16"),
                (200, 136, 96, 1, "f32"), (37, 48, 32, 1, "f32"), (300, 192, 128, 1, "bf16"), (4100, 48, 64, 1, "bf16"),
                (256, 128, 128, 9, "bf16"), (32800, 64, 64, 1, "bf16"), (300, 64, 32, 1, "f32"), (600, 264, 320, 1, "bf16"),
                (600, 264, 64, 3, "bf16"), (257, 512, 128, 1, "bf16"), (3900, 3848, 64, 1, "bf16"), (256, 256, 2048, 1, "bf16"),
                (300, 264, 448, 5, "bf16"), (256, 256, 256, 9, "bf16")]


def test_bound_holds_the_fp32_cpu_product_and_is_not_vacuous(capsys):
    worst = 0.0
    for M, N, Kseg, S, dt in BOUND_SHAPES:
        dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        g = torch.Generator().manual_seed(M + N + Kseg)
        A = torch.randn(M, S * Kseg, generator=g).to(dtype)
        B = (torch.randn(N, S * Kseg, generator=g) / (S * Kseg) ** 0.5).to(dtype)
        bias = torch.randn(N, generator=g)
        r = G.ref(A, B, M=M, bias=bias)
        e0 = G.e0(r)
        got = F.linear(A.float(), B.float(), bias)
        ratio = float(((got.double() - r["out"]).abs() / e0).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (M, N, Kseg, S, dt, ratio)
        # not vacuous either way: E0 stays below one bf16 ulp of a typical output, and far above fp64 noise
        assert float(e0.max()) < 2.0 ** -8 * float(r["out"].abs().max())
    with capsys.disabled():
        print(f"\n[gemm_ref] fp32 CPU product vs E0: largest err / bound = {worst:.3f} over {len(BOUND_SHAPES)} shapes")
    assert worst > 1e-4


def _poly_constants():
    with open(os.path.join(ROOT, "stswincl_amd", "csrc", "common.h")) as f:
        text = f.read()
    m = re.search(r"#define\s+STSWIN_PHI_COEFFS\s+(.*)", text)
    coeffs = [np.float32(c.rstrip("f")) for c in re.split(r"\s*,\s*", m.group(1).strip())]
    assert len(coeffs) == 8
    body = text[text.index("phi_poly2(f32x2 x)"):]
    zs = re.search(r"z\s*=\s*x\s*\*\s*([0-9.eE+-]+)f\s*;", body)
    assert zs and zs.group(1) == "0.2525381361380527"
    body = body[:body.index("\n}")]
    # the result is clamped to [0, 1] (what makes the tails exact): _phi_poly2 below mirrors the function as written
    assert re.search(r"__builtin_elementwise_min\(__builtin_elementwise_max\(r, \(f32x2\)\{0\.f, 0\.f\}\), \(f32x2\)\{1\.f, 1\.f\}\)", body)
    return coeffs, np.float32(zs.group(1))


def _fma32(a, b, c):
    """float32 fma: the product of two float32 values is exact in float64, the sum rounds once more than an fma does only in
    double-rounding ties (2^-29 of the cases, one float32 ulp)."""
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(np.float32)


def _phi_poly2(x, coeffs, zscale):
    z = np.clip((x * zscale).astype(np.float32), np.float32(-1), np.float32(1))
    s = (z * z).astype(np.float32)
    q = np.full_like(s, coeffs[7])
    for i in range(6, -1, -1):
        q = _fma32(q, s, coeffs[i])
    return np.clip(_fma32(z, q, np.float32(0.5)), np.float32(0), np.float32(1))


def test_bf16_gelu_polynomial_meets_its_documented_bounds(capsys):
    coeffs, zscale = _poly_constants()
    edge = 2.8 * math.sqrt(2.0)
    assert abs(float(zscale) * edge - 1.0) < 1e-7                 # the header's factor is 1 / (2.8 sqrt 2)
    x = np.concatenate([np.linspace(-8, 8, 1 << 21), [edge, -edge, np.nextafter(edge, 0), -np.nextafter(edge, 0), 0.0]]).astype(np.float32)
    phi = _phi_poly2(x, coeffs, zscale)
    gelu_fast = (x * phi).astype(np.float32)
    h = ((x * x).astype(np.float32) * np.float32(-0.72134752044448170368)).astype(np.float32)
    dens = np.exp2(h.astype(np.float64)).astype(np.float32)       # (v_exp_f32: correctly rounded here, 1 ulp on the device)
    dgelu_fast = _fma32((x * np.float32(0.39894228040143267794)).astype(np.float32), dens, phi)
    xd = torch.from_numpy(x.astype(np.float64))
    Phi = 0.5 * (1.0 + torch.erf(xd / math.sqrt(2.0)))
    e_phi = float((torch.from_numpy(phi.astype(np.float64)) - Phi).abs().max())
    e_xphi = float((torch.from_numpy(gelu_fast.astype(np.float64)) - xd * Phi).abs().max())
    e_d = float((torch.from_numpy(dgelu_fast.astype(np.float64)) - G.dgelu(xd)).abs().max())
    with capsys.disabled():
        print(f"\n[gemm_ref] phi_poly2 in float32 on {x.size} points of [-8, 8]: |Phi err| = {e_phi:.4e}  |x Phi err| = {e_xphi:.4e}  "
              f"|gelu' err| = {e_d:.4e}")
    assert e_phi <= 3.9e-5 and G.POLY_PHI_ERR == 3.9e-5
    assert e_xphi <= 1.6e-4 and G.POLY_XPHI_ERR == 1.6e-4
    assert e_d <= 4.0e-5 < G.DGELU_ERR_BF16
    # the tails beyond the clamp are exact: Phi = 0 / 1, so gelu = 0 / x and gelu' = 0 / 1 up to the (underflowing) density term
    far = np.array([4.0, 5.5, 8.0, 100.0], dtype=np.float32)
    assert np.all(_phi_poly2(far, coeffs, zscale) == np.float32(1.0))
    assert np.all(_phi_poly2(-far, coeffs, zscale) == np.float32(0.0))
    z_edge = np.float32(np.float32(edge) * zscale)
    assert abs(float(z_edge) - 1.0) <= 2.0 ** -23
