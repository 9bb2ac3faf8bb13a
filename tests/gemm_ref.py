"""Float64 reference of stswin_gemm_nt / stswin_gemm_nt_splitk (stswincl_amd/csrc/gemm.hip) and a derived PER-ELEMENT error bound.

Shared by tests/test_gemm_ref.py (CPU: the reference against float64 F.linear / F.gelu / autograd, the bound against an fp32 product,
the bf16 path's GELU polynomial against erf) and tests/test_hip_gemm_nt_contract.py (GPU: every product kernel family against it).
Nothing here calls the library: plain torch in float64, on the operands the kernel multiplies (the bf16- or fp32-rounded A, B, R
cast to float64).

ref(): the contract of include/stswin_hip.h in the order epi_piece (gemm.hip) applies it
      v     = sum_s A[a_rows[s][m], :Kseg] . B[n, s*Kseg:(s+1)*Kseg]           (row index -1: a row of zeros)
      v    += bias[n];   v *= scale for n < scale_cols
      C2    = v,  or gelu'(v) with GF_C2_DGELU
      v     = gelu_erf(v)                          (GF_GELU)
      v    += R[r_rows[m]]  |  v *= R[..]  |  v *= gelu'(R[..])                 (GF_RESID | GF_MUL_R | GF_MUL_DGELU)
      v     = max(v, 0)                            (GF_RELU)
      column sums, and per block of rows the sums and sums of squares, of v - BEFORE the output rounding
      C[c_rows[m]] = v,  or += v with GF_ACCUM     (the caller scatters: ref returns rows in m order)

bound(): worst case, derived, nothing in it is measured on a GPU.  u = 2^-23 (see below), absdot = |A| @ |B|^T, nk = S*Kseg.
  product   E0 = (nk + 4) * u * (absdot + |bias|), times |scale| on the scaled columns.  Products of bf16 values are exact in fp32,
            so only the nk - 1 additions of the accumulation, the bias add and the scaling round (nk + 1 operations; + 4 leaves room for
            the split-K combine's extra additions).  Neither the accumulation order nor whether the MFMA rounds to nearest or truncates
            inside a 32-wide (bf16) / 4-wide (fp32) block is specified: every partial sum is bounded by absdot, each operation loses at
            most one ulp of it one-sidedly, u = 2^-23 - the bound of ANY order under truncation.  The fp32 kernels
            (mfma_f32_16x16x4f32) round their products too: product k loses at most u * |a_k b_k|, all of them together u * absdot - one
            of the + 4 - so the same form with the same u covers them.
  GELU      1-Lipschitz up to max|gelu'| = 1.129 -> 1.13 * E0, plus the evaluation: bf16 path 1.6e-4 absolute (phi_poly2 in common.h:
            |x * Phi error| <= 1.6e-4, asserted by tests/test_gemm_ref.py from the header's coefficients); fp32 path erff:
            4 * 2^-24 * |gelu|.
  gelu'     as C2 or as the factor of GF_MUL_DGELU, bf16 path: 4.5e-5 absolute on the factor = 3.9e-5 of the polynomial's Phi + x * pdf(x)
            through the hardware exp2 (|x pdf| <= 0.242, v_exp_f32 and the argument's rounding stay below 6e-6).  fp32 path (erff and
            __expf): 2e-6 (0.5 * a few ulp of erff + 0.242 * the relative error of exp, ~1e-6).  Where the argument is v itself
            (GF_C2_DGELU) its error E0 passes through gelu'': + GELU2_MAX * E0.  The issue this contract was written for states
            max|gelu''| <= 0.4; the true maximum is gelu''(0) = 2 pdf(0) = 0.798.  The smaller, STRICTER constant is kept as stated.
  R         v + R adds nothing to the error; v * R scales it by |R|; v * gelu'(R): E * (|f| + ef) + |v| * ef with ef the factor error.
  ReLU      1-Lipschitz: unchanged.
  store     bf16: round-to-nearest to 8 significant bits = + half a bf16 ulp of the binade of |ref| + E, i.e. 2^(floor(log2(|ref| + E)) - 8):
            between 2^-9 and 2^-8 of the value.  (The issue this contract was written for states the term as 2^-9 * (|ref| + E); that is
            the rounding error at the TOP of a binade only - 0.2899 rounds to 0.2891, 1.5e-3 relative - and a correctly rounded result
            exceeds it: tests/test_gemm_ref.py shows both.  half_ulp_bf16 is the exact form and never above 2^-8 relative.)
            fp32: nothing.  GF_ACCUM: + E0 once more for the read-modify-write.
  sums      sum_m E[m, n] + (rows + 2) * 2^-24 * sum_m |ref[m, n]| for a sum over `rows` rows in any order (blocks first or not), the
            accumulator's prior value included; squares: the same with 2 |ref| E and ref^2.
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64

# stswin_gemm_nt flag bits (include/stswin_hip.h; tests/test_gemm_ref.py holds them to the header)
GELU, RESID, MUL_DGELU, OUT_F32, ACCUM, RELU = 1, 2, 4, 8, 16, 32
MUL_R, C2_DGELU = 8192, 16384

U = 2.0 ** -23
POLY_PHI_ERR = 3.9e-5          # |Phi error| of phi_poly2            (common.h; asserted in tests/test_gemm_ref.py)
POLY_XPHI_ERR = 1.6e-4         # |x * Phi error|
DGELU_ERR_BF16 = 4.5e-5        # gelu' on the bf16 path: polynomial + hardware exp2
DGELU_ERR_F32 = 2e-6           # gelu' on the fp32 path: erff + __expf
GELU_SLOPE = 1.13              # max |gelu'| = 1.129
GELU2_MAX = 0.4                # as stated by the issue (stricter than the true 0.798, see above)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def half_ulp_bf16(x):
    """Half a unit in the last place of bf16 (8 significant bits) in the binade of x >= 0: the round-to-nearest error of any value of
    magnitude <= x.  0 at x = 0."""
    x = x.to(F64)
    _, e = torch.frexp(x)                          # x = m * 2^e, 0.5 <= m < 1: floor(log2 x) = e - 1
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - 9), torch.zeros_like(x))


def gather_rows(A, rows, M):
    """A[rows] with -1 -> zeros (rows None: the first M rows); float64 [M][A.shape[1]]."""
    A = A.to(F64)
    if rows is None:
        return A[:M]
    idx = rows.long()
    return torch.where((idx >= 0)[:, None], A[idx.clamp(min=0)], torch.zeros((), dtype=F64))


def _products(A, B, M, Kseg, S, a_rows):
    """-> (dot, absdot) float64 [M][N]."""
    Bd = B.to(F64)
    dot = torch.zeros(M, B.shape[0], dtype=F64)
    absdot = torch.zeros_like(dot)
    for s in range(S):
        seg = gather_rows(A, None if a_rows is None else a_rows[s], M)[:, :Kseg]
        Bs = Bd[:, s * Kseg:(s + 1) * Kseg]
        dot += seg @ Bs.t()
        absdot += seg.abs() @ Bs.abs().t()
    return dot, absdot


def block_sums(x, rows):
    """[ceil(M / rows)][N]: column sums of x over consecutive blocks of `rows` rows."""
    M, N = x.shape
    nb = (M + rows - 1) // rows
    pad = torch.zeros(nb * rows, N, dtype=x.dtype)
    pad[:M] = x
    return pad.view(nb, rows, N).sum(1)


def ref(A, B, *, M, S=1, a_rows=None, bias=None, scale=1.0, scale_cols=0, R=None, r_rows=None, flags=0, c_prev=None):
    """Float64 contract.  A [rows][>= Kseg], B [N][S*Kseg], a_rows int [S][M] or None, R [rows][N] (gathered by r_rows or its first M
    rows), c_prev [M][N]: the output rows' previous contents (GF_ACCUM).  Returns a dict of float64 tensors in m order:
    pre (v after bias and scale), c2, out (v before rounding and before any accumulate), store (what C[c_rows[m]] holds afterwards),
    absdot; plus the operands bound() needs."""
    N, Ktot = B.shape
    assert Ktot % S == 0
    Kseg = Ktot // S
    dot, absdot = _products(A, B, M, Kseg, S, a_rows)
    v = dot.clone()
    bd = None
    if bias is not None:
        bd = bias.to(F64)
        v = v + bd
    if scale_cols > 0:
        v[:, :scale_cols] = v[:, :scale_cols] * float(scale)
    pre = v.clone()
    c2 = dgelu(pre) if flags & C2_DGELU else pre
    if flags & GELU:
        v = gelu(v)
    act = v.clone()
    Rg = None
    if flags & (RESID | MUL_R | MUL_DGELU):
        Rg = gather_rows(R, r_rows, M)
        if flags & RESID:
            v = v + Rg
        elif flags & MUL_R:
            v = v * Rg
        else:
            v = v * dgelu(Rg)
    if flags & RELU:
        v = v.clamp(min=0)
    store = v if not (flags & ACCUM) else c_prev.to(F64) + v
    return {"pre": pre, "c2": c2, "act": act, "out": v, "store": store, "absdot": absdot, "bias": bd, "R": Rg, "nk": S * Kseg,
            "scale": float(scale), "scale_cols": int(scale_cols), "flags": int(flags)}


def e0(r):
    """The product stage's bound [M][N] from ref()'s result."""
    e = (r["nk"] + 4) * U * (r["absdot"] + (r["bias"].abs() if r["bias"] is not None else 0.0))
    if r["scale_cols"] > 0:
        e = e.clone()
        e[:, :r["scale_cols"]] *= abs(r["scale"])
    return e


def bound(r, *, bf16, out_f32=False):
    """Per-element bounds from ref()'s result r: {E0, c2, out (before the store), store}.  bf16: the operand / epilogue path (False: the
    exact-fp32 kernels); out_f32: C is fp32 (GF_OUT_F32, or the fp32 path)."""
    flags = r["flags"]
    E0 = e0(r)
    ef = DGELU_ERR_BF16 if bf16 else DGELU_ERR_F32
    round_store = (lambda ref_, E: E + half_ulp_bf16(ref_.abs() + E)) if bf16 else (lambda ref_, E: E)
    Ec2 = (ef + GELU2_MAX * E0) if flags & C2_DGELU else E0
    Ec2 = round_store(r["c2"], Ec2)
    E = E0
    if flags & GELU:
        E = GELU_SLOPE * E0 + (POLY_XPHI_ERR if bf16 else 4 * 2.0 ** -24 * r["act"].abs())
    if flags & MUL_R:
        E = E * r["R"].abs()
    elif flags & MUL_DGELU:
        f = dgelu(r["R"]).abs()
        E = E * (f + ef) + r["act"].abs() * ef
    Eout = E
    Es = Eout if (out_f32 or not bf16) else round_store(r["store"], Eout)
    if flags & ACCUM:
        Es = Es + E0
    return {"E0": E0, "c2": Ec2, "out": Eout, "store": Es}


def sum_bound(out, Eout, rows, prior=None):
    """Bound of block sums over `rows` rows of `out` [M][N] (rows <= 0: the whole column) -> (sums' bound, squares' bound), both
    [ceil(M / rows)][N].  prior: the accumulator's previous value (colsum is +=)."""
    rows = out.shape[0] if rows <= 0 else rows
    a = block_sums(out.abs(), rows)
    if prior is not None:
        a = a + prior.to(F64).abs()
    n = min(rows, out.shape[0])
    bs = block_sums(Eout, rows) + (n + 2) * 2.0 ** -24 * a
    bq = block_sums(2 * out.abs() * Eout, rows) + (n + 2) * 2.0 ** -24 * block_sums(out * out, rows)
    return bs, bq


def worst(got, want, bnd, tile=256):
    """-> (largest err / bound, offenders, description of the worst element with its tile-local position)."""
    err = (got.to(F64) - want).abs()
    bnd = bnd.to(F64).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)       # (0 / 0 = exact at a zero bound; x / 0 = inf)
    bad = int((~(err <= bnd)).sum())           # (NaN counts as an offender)
    flat = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")).flatten()
    k = int(flat.argmax())
    ncol = got.shape[-1]
    i, j = k // ncol, k % ncol
    return float(flat[k]), bad, (f"row {i} col {j} (tile-local {i % tile}, {j % tile}): got {float(got.flatten()[k]):.9g} want "
                                 f"{float(want.flatten()[k]):.9g} bound {float(bnd.flatten()[k]):.3g}")
