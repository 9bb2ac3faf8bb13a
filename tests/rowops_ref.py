"""Float64 references of the row kernels of stswincl_amd/csrc/rowops.hip - ln_fwd_kernel, ln_bwd_kernel, colsum_kernel, slab_fold_kernel /
slab_fold_multi_kernel, bias_scatter_kernel - with the launch geometry of the LayerNorm backward, the depth of every reduction, derived
PER-ELEMENT error bounds and the case lists of the contract tests.

Shared by tests/test_rowops_ref.py (CPU: the references against float64 autograd, the geometry against a transcription of the
launcher's rule, the bounds against an fp32 emulation of each kernel's association and against planted defects) and
tests/test_hip_rowops_contract.py (GPU: every kernel against them).  Nothing here calls the library: plain torch in float64 on the operands as
stored (bf16 or fp32 cast to float64), on whichever device the operands live.

Contract decisions
  dxsum   sums the fp32 values of dx BEFORE they are rounded to the output type (with accumulate: add + LN'(dy) in fp32): the better bias
          gradient; in fp32 storage the two readings coincide.  include/stswin_hip.h says the same.
  eps     crosses the ABI as a float: the reference uses float32(eps).
  mean, rstd of the backward are the ones the forward kernel wrote (as bn_ref.backward does): the backward is judged on its own arithmetic.

Bounds.  u = 2^-24 (round to nearest, fp32 VALU; the library is built with -ffp-contract=off: no fused multiply-adds), gam(k) = k u / (1 - k u)
for k roundings in a row.  A sum of n terms through a chain of `depth` additions is off by at most gam(depth) * sum |terms|.  Nothing is measured.
  e_rsqrt  the ROCm documentation shipped with the toolchain does not state the error of the device rsqrtf; 2 ulp = 4 u is ASSUMED (the OpenCL
           full-profile bound for rsqrt, which the device library's implementation is written to).
  division by C: hipcc's default is the correctly rounded fp32 division (-fhip-fp32-correctly-rounded-divide-sqrt): one u.
  forward  d1 = pieces * PACK + 6: a lane adds its pieces' elements in order, then six butterfly levels.
    dmean = gam(d1 + 1) * mean|x|                                        the sum, the division
    dvar  = dmean^2 + gam(d1 + 4) * (var + dmean^2)                      sum (x - m)^2 = C var + C (m - mean)^2 exactly (the cross term is
                                                                         zero); per term: the subtraction twice (squared), the product;
                                                                         then the sum and the division
    drs   = (1 - darg)^-1/2 - 1 + e_rsqrt (1 + ...),  darg = dvar / (var + eps) + u    the addition of eps; the rsqrt
    dy    = |gamma| rstd (dmean + (|x - mean| + dmean) (drs + gam(3))) (1 + u) + u |y| + rounding of y to T
            (the subtraction, the product with rstd, the product with gamma: gam(3); the addition of beta: u |y|, carried (1 + u) onto the rest)
  backward, per row (mean, rstd exact inputs):  xh = (x - mean) rstd: gam(2) |xh|;  g = dy gamma: u |g|
    ds1 = gam(d1 + 2) mean|g|            ds2 = gam(d1 + 5) mean|g xh|         (term, sum, division)
    dval = rstd (u |g| + ds1 + u |g - s1| + gam(3) |xh s2| + |xh| ds2 + u |g - s1 - xh s2|) (1 + u) + u |val|
    dfin = dval + u |fin| when accumulating (old + val), then the one rounding to T
  sums: gam(depth + k) * (sum |terms| + |old|) + the propagated per-term error, k = roundings in forming one term (dgamma: 3, dbeta: 0,
    dxsum: 0 + the terms' own dfin before the rounding to T); depth from the kernels:
    parameter gradients  rows_per_wave * ceil(groups / grid) + (waves - 1) + fold
    fold                 ceil(nslabs / QL) + (QL - 1) (+ 1 when accumulating),  QL = 64 at nslabs >= 96, else 16
    colsum               ceil(min(M, 512) / 8) + 8 + fold over ceil(M / 512) slabs
    bias_scatter         ceil(pairs / 64) * nslabs + 6 + 1
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from gemm_ref import half_ulp_bf16

F64 = torch.float64
BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
RSQRT_ULP = 2.0                     # assumed (module docstring)
E_RSQRT = RSQRT_ULP * 2 * U
FOLD_QUEUE_MAX = 12                 # rowops.hip
GRID_CAP = 1024


def gam(k):
    return k * U / (1.0 - k * U)


def pack_of(dtype):
    return 8 if dtype == BF else 4


def pieces(C, pk):
    return (C // pk + 63) // 64


def np_inst(C, pk, backward=False):
    """The NP template argument the launchers pick (None: refused with -1104)."""
    n = pieces(C, pk)
    for cap in (1, 2, 4, 8) + (() if backward else (16,)):
        if n <= cap:
            return cap
    return None


def eps32(eps):
    return float(torch.tensor(eps, dtype=F32))


def round_to(v, dtype):
    """Half an ulp of the storage type at |v| (0 for fp32: the value is already one)."""
    return half_ulp_bf16(v) if dtype == BF else torch.zeros_like(v)


# ------------------------------------------------------------------------------------------------------------------ geometry and depths
def ln_bwd_geometry(M, C, pk):
    """(rows_per_wave, waves, groups, grid) of stswin_layernorm_bwd, from the rule rowops.hip states under "Geometry:": 8 rows per wave from
    M = 16384, 4 from 4096, else 2; 8 waves where four would leave the grid at <= 512 workgroups, the 8-wave grid is still >= 128 and the row
    fits two pieces per lane; the grid is capped at 1024 (a workgroup then walks several row groups)."""
    rpw = 8 if M >= 16384 else (4 if M >= 4096 else 2)
    four = -(-M // (4 * rpw))
    waves = 8 if (four <= 512 and M >= 8 * rpw * 128 and pieces(C, pk) <= 2) else 4
    groups = -(-M // (waves * rpw))
    return rpw, waves, groups, min(groups, GRID_CAP)


def ln_bwd_scratch(M, C):
    rpw = 8 if M >= 16384 else (4 if M >= 4096 else 2)
    return min(-(-M // (4 * rpw)), GRID_CAP) * 3 * C


def fold_ql(nslabs):
    return 64 if nslabs >= 96 else 16


def row_depth(C, pk):
    return pieces(C, pk) * pk + 6


def fold_depth(nslabs, accumulate=True):
    ql = fold_ql(nslabs)
    return -(-nslabs // ql) + (ql - 1) + (1 if accumulate else 0)


def param_depth(M, C, pk):
    rpw, waves, groups, grid = ln_bwd_geometry(M, C, pk)
    return rpw * -(-groups // grid) + (waves - 1) + fold_depth(grid, True)


def colsum_depth(M):
    return -(-min(M, 512) // 8) + 8 + fold_depth(-(-M // 512), True)


def scatter_depth(pairs, nslabs):
    return -(-pairs // 64) * nslabs + 6 + 1


# ------------------------------------------------------------------------------------------------------------------ gather / scatter
def merge_rows(frames, H, W):
    """The patch-merging row map [4 * M]: segment s = (dy, dx) in [(0,0),(1,0),(0,1),(1,1)] of output token r reads this source token."""
    Ho, Wo = H // 2, W // 2
    r = torch.arange(frames * Ho * Wo)
    xo, yo, f = r % Wo, (r // Wo) % Ho, r // (Wo * Ho)
    return torch.cat([(f * H + 2 * yo + dy) * W + 2 * xo + dx for dy, dx in ((0, 0), (1, 0), (0, 1), (1, 1))]).to(torch.int32)


def gathered(x, rows, M, S, Cseg):
    """The normalised matrix [M][S * Cseg] in float64: row r = concat_s x[rows[s * M + r]][:Cseg]."""
    x = x.to(F64)
    if rows is None:
        assert S == 1
        return x[:M, :Cseg]
    idx = rows.long().view(S, M)
    return torch.cat([x[idx[s], :Cseg] for s in range(S)], dim=1)


def scatter(full, rows, S, Cseg, n_src, fill=float("nan")):
    """The inverse of gathered() for a [M][S * Cseg] matrix -> [n_src][Cseg]; source rows no map entry names hold `fill`."""
    M = full.shape[0]
    if rows is None:
        return full
    out = torch.full((n_src, Cseg), fill, dtype=full.dtype, device=full.device)
    idx = rows.long().view(S, M)
    for s in range(S):
        out[idx[s]] = full[:, s * Cseg:(s + 1) * Cseg]
    return out


# ------------------------------------------------------------------------------------------------------------------ LayerNorm forward
def ln_forward(x, gamma, beta, eps, rows=None, S=1, Cseg=None, M=None):
    """-> y [M][C], mean [M], var [M] (biased), rstd [M], float64."""
    Cseg = x.shape[1] if Cseg is None else Cseg
    M = (x.shape[0] if rows is None else rows.numel() // S) if M is None else M
    X = gathered(x, rows, M, S, Cseg)
    mean = X.mean(1)
    var = ((X - mean[:, None]) ** 2).mean(1)
    rstd = (var + eps32(eps)) ** -0.5
    y = (X - mean[:, None]) * rstd[:, None] * gamma.to(F64) + beta.to(F64)
    return y, mean, var, rstd


def fwd_bound(x, gamma, beta, eps, dtype, rows=None, S=1, Cseg=None, M=None):
    """-> {y [M][C], mean [M], rstd [M]}: the forms of the module docstring."""
    Cseg = x.shape[1] if Cseg is None else Cseg
    y, mean, var, rstd = ln_forward(x, gamma, beta, eps, rows, S, Cseg, M)
    X = gathered(x, rows, y.shape[0], S, Cseg)
    d1 = row_depth(S * Cseg, pack_of(dtype))
    dmean = gam(d1 + 1) * X.abs().mean(1)
    dvar = dmean ** 2 + gam(d1 + 4) * (var + dmean ** 2)
    darg = (dvar / (var + eps32(eps)) + U).clamp(max=0.5)
    drs = ((1 - darg) ** -0.5 - 1) * (1 + E_RSQRT) + E_RSQRT
    dev = (X - mean[:, None]).abs()
    e = gamma.to(F64).abs() * rstd[:, None] * (dmean[:, None] + (dev + dmean[:, None]) * (drs[:, None] + gam(3))) * (1 + U) + U * y.abs()
    e = e + round_to(y.abs() + e, dtype)
    return {"y": e, "mean": dmean, "rstd": rstd * drs}


# ------------------------------------------------------------------------------------------------------------------ LayerNorm backward
def bwd_core(dy, x, gamma, mean, rstd, rows=None, S=1, Cseg=None, M=None):
    """Everything the references and the bounds of the backward share, in the normalised layout [M][C], float64."""
    Cseg = x.shape[1] if Cseg is None else Cseg
    M = dy.shape[0] if M is None else M
    X = gathered(x, rows, M, S, Cseg)
    d = dy.to(F64)[:M, :S * Cseg]
    mu, rs = mean.to(F64)[:M, None], rstd.to(F64)[:M, None]
    xh = (X - mu) * rs
    g = d * gamma.to(F64)
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    val = rs * (g - s1 - xh * s2)
    return {"d": d, "xh": xh, "g": g, "s1": s1, "s2": s2, "rs": rs, "val": val, "S": S, "Cseg": Cseg}


def ln_backward(dy, x, gamma, mean, rstd, rows=None, S=1, Cseg=None, add=None, n_src=None, M=None, core=None):
    """-> dx, dgamma, dbeta, dxsum in float64.  dx is in the SOURCE layout [n_src][Cseg] (scattered back through `rows`; rows no map entry
    names are NaN), = add + LN'(dy) where `add` (source layout, read through the same map) is given.  dgamma / dbeta / dxsum are the sums
    alone: the caller adds what the accumulators held.  dxsum sums the unrounded dx."""
    c = core if core is not None else bwd_core(dy, x, gamma, mean, rstd, rows, S, Cseg, M)
    fin = c["val"] if add is None else gathered(add, rows, c["val"].shape[0], c["S"], c["Cseg"]) + c["val"]
    n_src = x.shape[0] if n_src is None else n_src
    return scatter(fin, rows, c["S"], c["Cseg"], n_src), (c["d"] * c["xh"]).sum(0), c["d"].sum(0), fin.sum(0)


def sum_bound(abs_sum, depth, k, old_abs=0.0, prop=0.0):
    """gam(depth + k) * (sum |terms| + propagated + |old|) + propagated."""
    return gam(depth + k) * (abs_sum + prop + old_abs) + prop


def bwd_bound(core, dtype, M, rows=None, add=None, n_src=None, old=None):
    """-> {dx [n_src][Cseg] (NaN where unnamed), dgamma, dbeta, dxsum [C]}.  old: {name: what the accumulator held} (float64 or None)."""
    c = core
    C = c["S"] * c["Cseg"]
    pk = pack_of(dtype)
    d1 = row_depth(C, pk)
    g, xh, s1, s2, rs, val = c["g"], c["xh"], c["s1"], c["s2"], c["rs"], c["val"]
    ds1 = gam(d1 + 2) * g.abs().mean(1, keepdim=True)
    ds2 = gam(d1 + 5) * (g * xh).abs().mean(1, keepdim=True)
    inner = U * g.abs() + ds1 + U * (g - s1).abs() + gam(3) * (xh * s2).abs() + xh.abs() * ds2 + U * (g - s1 - xh * s2).abs()
    dval = rs.abs() * inner * (1 + U) + U * val.abs()
    if add is None:
        fin, dfin = val, dval
    else:
        fin = gathered(add, rows, val.shape[0], c["S"], c["Cseg"]) + val
        dfin = dval + U * (fin.abs() + dval)
    ddx = dfin + round_to(fin.abs() + dfin, dtype)
    depth = param_depth(M, C, pk)
    old = old or {}
    o = lambda k: (old[k].to(F64).abs() if old.get(k) is not None else 0.0)   # noqa: E731
    n_src = val.shape[0] if n_src is None else n_src
    return {"dx": scatter(ddx, rows, c["S"], c["Cseg"], n_src),
            "dgamma": sum_bound((c["d"] * xh).abs().sum(0), depth, 3, o("dgamma")),
            "dbeta": sum_bound(c["d"].abs().sum(0), depth, 0, o("dbeta")),
            "dxsum": sum_bound(fin.abs().sum(0), depth, 0, o("dxsum"), prop=dfin.sum(0))}


# ------------------------------------------------------------------------------------------------------------------ sums
def colsum(y, M):
    return y.to(F64)[:M].sum(0)


def colsum_bound(y, M, old=None):
    return sum_bound(y.to(F64)[:M].abs().sum(0), colsum_depth(M), 0, 0.0 if old is None else old.to(F64).abs())


def fold_view(ws, slab_stride, ws_batch_stride, nslabs, seg_len, nseg, batch):
    """ws (flat) -> [batch][nslabs][nseg * seg_len] as a strided view."""
    return torch.as_strided(ws, (batch, nslabs, nseg * seg_len), (ws_batch_stride, slab_stride, 1), ws.storage_offset())


def fold(ws, slab_stride, ws_batch_stride, nslabs, seg_len, nseg, batch):
    """-> [nseg][batch][seg_len] float64: out_s[b][j] = sum_p ws[b * ws_batch_stride + p * slab_stride + s * seg_len + j]."""
    v = fold_view(ws, slab_stride, ws_batch_stride, nslabs, seg_len, nseg, batch).to(F64)
    return v.sum(1).view(batch, nseg, seg_len).permute(1, 0, 2)


def fold_bound(ws, slab_stride, ws_batch_stride, nslabs, seg_len, nseg, batch, old=None, accumulate=True):
    """old: [nseg][batch][seg_len] or None."""
    v = fold_view(ws, slab_stride, ws_batch_stride, nslabs, seg_len, nseg, batch).to(F64).abs()
    a = v.sum(1).view(batch, nseg, seg_len).permute(1, 0, 2)
    return sum_bound(a, fold_depth(nslabs, accumulate), 0, old.to(F64).abs() if (accumulate and old is not None) else 0.0)


def bias_scatter(dbiasT, index, table_rows, nslabs):
    """dbiasT [nslabs][heads][N(key j)][N(query i)], index int64 [N * N] (pair i * N + j) -> (sum, sum of |.|, pairs per row): the first
    two [table_rows][heads] float64."""
    ns, heads, N, _ = dbiasT.shape
    assert ns == nslabs
    v = dbiasT.to(F64).permute(0, 3, 2, 1).reshape(nslabs, N * N, heads)         # [slab][i * N + j][h]
    out = torch.zeros(table_rows, heads, dtype=F64, device=dbiasT.device)
    ab = torch.zeros_like(out)
    out.index_add_(0, index.reshape(-1), v.sum(0))
    ab.index_add_(0, index.reshape(-1), v.abs().sum(0))
    return out, ab, torch.bincount(index.reshape(-1), minlength=table_rows)[:table_rows]


def bias_scatter_bound(ab, counts, nslabs, old):
    depth = torch.tensor([scatter_depth(int(n), nslabs) for n in counts.tolist()], dtype=F64, device=ab.device)[:, None]
    return depth * U / (1 - depth * U) * (ab + old.to(F64).abs())


# ------------------------------------------------------------------------------------------------------------------ judging
def worst(got, want, bnd, pk=None, C=None):
    """-> (largest err / bound, offenders, description of the worst element).  Elements whose bound is NaN (unnamed rows) are skipped."""
    got, want = got.to(F64), want.to(F64)
    live = ~torch.isnan(bnd)
    err = torch.where(live, (got - want).abs(), torch.zeros_like(want))
    b = torch.where(live, bnd, torch.ones_like(bnd))
    bad = (err > b) | (live & ~torch.isfinite(got))
    ratio = torch.where(b > 0, err / b.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(live & ~torch.isfinite(got), torch.full_like(ratio, float("inf")), ratio)
    if ratio.numel() == 0:
        return 0.0, 0, "-"
    k = int(ratio.argmax())
    idx = [int(i) for i in torch.unravel_index(torch.tensor(k), ratio.shape)] if ratio.dim() else []
    where = f"{idx}: got {float(got.flatten()[k]):.9g}, want {float(want.flatten()[k]):.9g}, bound {float(bnd.flatten()[k]):.3g}"
    if pk is not None and idx:
        c = idx[-1]
        where += f" (piece {c // (64 * pk)}, lane {(c // pk) % 64}, element {c % pk})"
    return float(ratio.flatten()[k]), int(bad.sum()), where


# ------------------------------------------------------------------------------------------------------------------ operands
REGIMES = ("normal", "offset300", "const", "spike")


def make_x(regime, M, C, dtype, gen):
    """The four regimes of x, as stored.  offset300: |mean| / std about 300 (separates two-pass from one-pass statistics); const: every third
    row is one value (variance 0, rstd = eps^-1/2: the result hangs on eps and on the exact mean); spike: one column 5000 x the rest."""
    x = torch.randn(M, C, generator=gen)
    if regime == "normal":
        x = x * 2 + 0.5
    elif regime == "offset300":
        x = x + 300.0
    elif regime == "const":
        x = x * 2 + 0.5
        x[::3] = x[::3, :1]
    elif regime == "spike":
        x[:, C // 3] *= 5000.0
    else:
        raise ValueError(regime)
    return x.to(dtype)


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class FwdCase:
    name: str
    dtype: torch.dtype
    M: int
    C: int
    NP: int                      # the instantiation the launcher's switch picks
    regime: str = "normal"
    S: int = 1
    Cseg: int = 0                # 0: C
    form: str = "plain"          # plain | gather | xslice


@dataclasses.dataclass(frozen=True)
class BwdCase:
    name: str
    dtype: torch.dtype
    M: int
    C: int
    NP: int
    geometry: tuple              # (rows_per_wave, waves, groups, grid) the launch must show
    S: int = 1
    Cseg: int = 0
    form: str = "plain"          # plain | gather


@dataclasses.dataclass(frozen=True)
class ColsumCase:
    name: str
    dtype: torch.dtype
    M: int
    N: int


@dataclasses.dataclass(frozen=True)
class FoldCase:
    name: str
    nslabs: int
    seg_len: int
    nseg: int
    batch: int
    accumulate: int
    null_out1: bool
    QL: int
    loops4: int                  # passes of the four-loads-in-flight loop of slab lane 0


def _dn(dt):
    return "bf16" if dt == BF else "f32"


FWD_C = {BF: (8, 64, 520, 1536, 2568, 4096, 4104), F32: (4, 64, 260, 768, 1284, 2048, 2052)}
FWD_ALL_REGIMES = {BF: (64, 520, 1536, 2568, 4104), F32: (64, 260, 768, 1284, 2052)}       # one C per NP
GATHER = dict(frames=2, H=4, W=6)                                                            # S = 4: M = 12 of 48 source tokens


def cases_fwd():
    out = []
    for dt in (BF, F32):
        pk = pack_of(dt)
        for C in FWD_C[dt]:
            for M in (1, 3, 37):
                regs = REGIMES if (C in FWD_ALL_REGIMES[dt] and M == 37) else ("normal",)
                for rg in regs:
                    out.append(FwdCase(f"{_dn(dt)} {M}x{C} {rg}", dt, M, C, np_inst(C, pk), rg))
        for Cseg in (16, 24):
            out.append(FwdCase(f"{_dn(dt)} gather S=4 Cseg={Cseg}", dt, 12, 4 * Cseg, np_inst(4 * Cseg, pk), "normal", 4, Cseg, "gather"))
        out.append(FwdCase(f"{_dn(dt)} 37x{FWD_C[dt][2]} x column slice", dt, 37, FWD_C[dt][2], 2, "normal", 1, 0, "xslice"))
    return out


BWD_M = (1, 7, 9, 2047, 2048, 4095, 4096, 8192, 8193, 16383, 16384, 16385, 32768, 32769, 32800)
BWD_M_F32 = (2048, 4096, 8192, 16384, 32769, 32800)                     # the 8-wave and the wrapped sizes


def cases_bwd():
    out = []

    def add(dt, M, C, S=1, Cseg=0, form="plain"):
        pk = pack_of(dt)
        out.append(BwdCase(f"{_dn(dt)} {M}x{C}" + (f" {form} S={S}" if S > 1 else ""), dt, M, C, np_inst(C, pk, True), ln_bwd_geometry(M, C, pk),
                           S, Cseg, form))
    for M in BWD_M:
        add(BF, M, 64)
    for M in BWD_M_F32:
        add(F32, M, 64)
    add(BF, 2050, 1536)                                                 # three pieces: 4 waves although 2050 rows would take 8
    add(BF, 2048, 1024)                                                 # two pieces per lane in 8 waves
    add(F32, 2048, 512)
    for C in (520, 1536, 2568, 3272):
        add(BF, 37, C)
    for C in (260, 1284, 2048):
        add(F32, 37, C)
    for dt in (BF, F32):
        add(dt, 12, 64, 4, 16, "gather")
        add(dt, 12, 96, 4, 24, "gather")
    return out


def cases_colsum():
    out = []
    for dt in (BF, F32):
        pk = pack_of(dt)
        for M in (1, 8, 511, 512, 513, 1030):
            for N in (pk, 264, 32 * pk, 33 * pk):
                out.append(ColsumCase(f"{_dn(dt)} {M}x{N}", dt, M, N))
    return out


FOLD_NSLABS = (1, 15, 16, 17, 48, 49, 65, 95, 96, 97, 192, 193, 257, 1024)
FOLD_SEG = (4, 60, 64, 260)


def cases_fold():
    """Every (nslabs, seg_len, nseg) with two of the four (batch, accumulate) pairs, alternating, so that every nslabs and every seg_len
    meets both batches and both modes; a NULL out1 at every nseg = 3 case with batch = 3."""
    out, i = [], 0
    for ns in FOLD_NSLABS:
        ql = fold_ql(ns)
        loops4 = len(range(0, max(0, ns - 3 * ql), 4 * ql))
        for sl in FOLD_SEG:
            for nseg in (1, 2, 3):
                for batch, acc in (((1, 1), (3, 0)) if i % 2 == 0 else ((1, 0), (3, 1))):
                    out.append(FoldCase(f"{ns} slabs x {nseg}x{sl} batch {batch} acc {acc}", ns, sl, nseg, batch, acc, nseg == 3 and batch == 3, ql,
                                        loops4))
                i += 1
    return out


# ------------------------------------------------------------------------------------------------------------------ operands of the cases
def seed(c):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % (1 << 31))


def fwd_operands(c):
    """x as stored (source layout), gamma, beta, rows."""
    g = seed(c)
    Cseg = c.Cseg or c.C
    if c.form == "gather":
        n_src = GATHER["frames"] * GATHER["H"] * GATHER["W"]
        rows = merge_rows(**GATHER)
        x = make_x(c.regime, n_src, Cseg, c.dtype, g)
    else:
        rows, x = None, make_x(c.regime, c.M, Cseg, c.dtype, g)
    return x, 1 + 0.1 * torch.randn(c.C, generator=g), 0.1 * torch.randn(c.C, generator=g), rows


def bwd_operands(c):
    g = seed(c)
    Cseg = c.Cseg or c.C
    rows = merge_rows(**GATHER) if c.form == "gather" else None
    n_src = GATHER["frames"] * GATHER["H"] * GATHER["W"] + 3 if rows is not None else c.M      # three source rows no map entry names
    x = make_x("normal", n_src, Cseg, c.dtype, g)
    gamma = 1 + 0.1 * torch.randn(c.C, generator=g)
    dy = torch.randn(c.M, c.C, generator=g).to(c.dtype)
    add = torch.randn(n_src, Cseg, generator=g).to(c.dtype)
    return x, gamma, dy, add, rows, n_src


def fold_operands(c, integers=False, device="cpu"):
    """-> ws (flat, NaN in the padding between slabs and batches), slab_stride, ws_batch_stride, old [nseg][batch][seg_len]."""
    g = seed(c)
    width = c.nseg * c.seg_len
    stride = width + 8
    bstride = c.nslabs * stride + 12
    ws = torch.full((c.batch * bstride + 4,), float("nan"))
    v = fold_view(ws, stride, bstride, c.nslabs, c.seg_len, c.nseg, c.batch)
    shape = (c.batch, c.nslabs, width)
    v.copy_(torch.randint(-8, 9, shape, generator=g).float() if integers else torch.randn(shape, generator=g))
    old = torch.randint(-8, 9, (c.nseg, c.batch, c.seg_len), generator=g).float() if integers else torch.randn(c.nseg, c.batch, c.seg_len, generator=g)
    return ws.to(device), stride, bstride, old.to(device)
