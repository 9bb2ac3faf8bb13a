"""Float64 reference of stswin_gemm_tn (stswincl_amd/csrc/gemm.hip: every weight gradient of the training step), the row ranges of its
contraction splits, a derived PER-ELEMENT error bound, and the case list of the contract tests.

Shared by tests/test_gemm_tn_ref.py (CPU: the reference against float64 autograd, the partition against the launcher's rule, the bound
against an fp32 emulation of every combine form and against four planted defects, at every case below) and
tests/test_hip_gemm_tn_contract.py (GPU: every kernel and combine form against it).  Nothing here calls the library: plain torch in
float64, on the operands the kernel multiplies (the bf16- or fp32-rounded At, Bt cast to float64).

ref(): the contract of include/stswin_hip.h
      C[i][j] = c_prev[i][j] + sum_m At[at_rows[m]][i] * Bt[bt_rows[m]][j]          (row index -1 in either map: a row of zeros)
      bseg > 0:  column j reads column j % bseg of row bt_rows[(j // bseg) * Mk + m]  (tap j // bseg has its own row map)
      tapminor:  GEMM column j = s * bseg + c is stored at c * S + s, S = Nj // bseg  (conv.weight.grad's own [cout][cin][k][k] layout)

partition(): both kernel bodies cut the contraction into units of `unit` rows (32: the 256x256 ring and the fp32 128x128 kernel, 64: the
      bf16 128x128 kernel), per = ceil(units / splits), split s takes the units [s * per, min(units, (s + 1) * per)).  corrected_splits()
      is what stswin_gemm_tn turns a requested count into: at most one split per unit, then ceil(units / per) - no split without a unit.

bound(): worst case, derived, nothing in it is measured on a GPU.  u = 2^-23 and any-order truncation, as tests/gemm_ref.py argues: neither
      the accumulation order nor whether the MFMA rounds to nearest or truncates inside a block is specified, every partial sum is bounded
      by the sum of absolute products, each operation loses at most one ulp of it one-sidedly.  P_s / A_s: the float64 partial sum / the
      partial sum of absolute products over the rows of split s.
  accumulation  E_s = (rows_s + 2) * u * A_s.  Products of bf16 values are exact in fp32; the fp32 instantiation (mfma_f32_16x16x4f32)
                rounds its products, all of them together u * A_s - one of the + 2.
  bf16 slabs    (only where the variant word reports STSWIN_VAR_TN_SLABS_BF16) each partial is rounded to bf16 once:
                H_s = half_ulp_bf16(|P_s| + E_s).  Zero for every other form.
  combine       fp32 atomics, fp32 slabs + tn_reduce, the fused in-launch combine, tn_combine, or the one atomic add per element at
                splits == 1: at most splits + 1 additions (the partials onto zero, the sum onto c_prev), every intermediate bounded by
                T = |c_prev| + sum_s (|P_s| + E_s + H_s):  (splits + 2) * u * T.
                (H_s inside T is a term the issue's formula does not list: the combine adds the ROUNDED partials, whose magnitude is up to
                 |P_s| + E_s + H_s.  It is second order - (splits + 2) * 2^-23 * 2^-8 of a partial - and derived, not measured.)
  total         sum_s (E_s + H_s) + combine.
  rows kernel   (Mk <= 8: one thread adds Mk outer-product terms onto c_prev, rounding each product and each add)
                (2 * Mk + 2) * u * (sum_m |a b| + |c_prev|).
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from gemm_ref import U, half_ulp_bf16

F64 = torch.float64
BF, F32 = torch.bfloat16, torch.float32

# stswin_last_variant(1) codes and bits, bits of `splits` (include/stswin_hip.h; tests/test_gemm_tn_ref.py holds them to the header)
RING_PLAIN, RING_ATROWS, RING_BTROWS, RING_BSEG, K128, K128_W4, ROWS, VAR_F32 = 20, 21, 22, 23, 30, 31, 32, 100
SLABS_F32, SLABS_BF16, TAPMINOR, FUSED = 0x1000, 0x2000, 0x4000, 0x8000
BIT_W4, BIT_RING = 1 << 30, 1 << 29                    # tuning bits of `splits`, as tools/tn_sweep.py uses them
KERNEL_NAMES = {RING_PLAIN: "ring", RING_ATROWS: "ring_atrows", RING_BTROWS: "ring_btrows", RING_BSEG: "ring_bseg", K128: "128x128",
                K128_W4: "128x128_w4", ROWS: "rows", K128 + VAR_F32: "128x128_f32", K128_W4 + VAR_F32: "128x128_w4_f32"}


# ------------------------------------------------------------------------------------------------------------------ operands
def gather(X, rows, Mk):
    """X[rows] with -1 -> zeros (rows None: the first Mk rows); float64 [Mk][X.shape[1]]."""
    X = X.to(F64)
    if rows is None:
        return X[:Mk]
    idx = rows.long()
    assert idx.numel() == Mk
    return torch.where((idx >= 0)[:, None], X[idx.clamp(min=0)], torch.zeros((), dtype=F64))


def operands(At, Bt, *, Mk, Nj=None, at_rows=None, bt_rows=None, bseg=0):
    """The two [Mk][.] float64 matrices the contraction runs over: A [Mk][Ni] and B [Mk][Nj] (bseg: the taps side by side)."""
    A = gather(At, at_rows, Mk)
    if bseg > 0:
        assert bt_rows is not None
        Nj = bt_rows.numel() // Mk * bseg if Nj is None else Nj
        assert Nj % bseg == 0 and bt_rows.numel() == (Nj // bseg) * Mk
        B = torch.cat([gather(Bt[:, :bseg], bt_rows[t * Mk:(t + 1) * Mk], Mk) for t in range(Nj // bseg)], dim=1)
    else:
        B = gather(Bt, bt_rows, Mk)
        if Nj is not None:
            B = B[:, :Nj]
    return A, B


def tapminor_index(Nj, bseg):
    """idx with stored[:, idx[j]] = gemm[:, j]: GEMM column j = s * bseg + c goes to c * S + s."""
    S = Nj // bseg
    j = torch.arange(Nj)
    return (j % bseg) * S + j // bseg


def to_tapminor(X, bseg):
    out = torch.empty_like(X)
    out[..., tapminor_index(X.shape[-1], bseg)] = X
    return out


def ref(At, Bt, *, Mk, at_rows=None, bt_rows=None, bseg=0, c_prev=None, tapminor=False, Nj=None):
    """Float64 contract -> C [Ni][Nj].  At [rows][Ni], Bt [rows][Nj] (bseg > 0: [rows][>= bseg], Nj = taps * bseg from bt_rows), maps int
    [Mk] (bseg: [taps * Mk]) or None, c_prev [Ni][Nj] in the STORED layout or None (overwrite)."""
    A, B = operands(At, Bt, Mk=Mk, Nj=Nj, at_rows=at_rows, bt_rows=bt_rows, bseg=bseg)
    C = A.t() @ B
    if tapminor:
        assert bseg > 0
        C = to_tapminor(C, bseg)
    return C if c_prev is None else c_prev.to(F64) + C


# ------------------------------------------------------------------------------------------------------------------ partition
def corrected_splits(Mk, splits, unit):
    """The split count stswin_gemm_tn launches for a requested one: clamped to the units, then no split left without a unit."""
    units = (Mk + unit - 1) // unit
    splits = max(1, min(int(splits), units))
    per = (units + splits - 1) // splits
    return (units + per - 1) // per


def partition(Mk, splits, unit):
    """[(m0, m1)] per split: the contraction rows the kernels give split s (see the module docstring).  A split beyond the last unit
    gets an empty range (m0 == m1) - the launcher never asks for one (corrected_splits)."""
    units = (Mk + unit - 1) // unit
    per = (units + splits - 1) // splits
    out = []
    for s in range(splits):
        u0, u1 = min(units, s * per), min(units, (s + 1) * per)
        out.append((min(Mk, u0 * unit), min(Mk, u1 * unit)))
    return out


def partials(A, B, ranges):
    """-> (P, Ab) float64 [splits][Ni][Nj]: partial sums and partial sums of absolute products over each row range."""
    P = torch.stack([A[m0:m1].t() @ B[m0:m1] for m0, m1 in ranges])
    Ab = torch.stack([A[m0:m1].abs().t() @ B[m0:m1].abs() for m0, m1 in ranges])
    return P, Ab


def bound(P, Ab, ranges, *, c_prev=None, slab_bf16=False, rows_kernel=False):
    """Per-element bound [Ni][Nj] from partials() (already in the stored layout) and the previous contents (None: overwrite)."""
    cp = torch.zeros_like(P[0]) if c_prev is None else c_prev.to(F64).abs()
    if rows_kernel:
        Mk = ranges[-1][1] - ranges[0][0]
        return (2 * Mk + 2) * U * (Ab.sum(0) + cp)
    splits = len(ranges)
    rows = torch.tensor([m1 - m0 for m0, m1 in ranges], dtype=F64, device=P.device)[:, None, None]
    E = (rows + 2) * U * Ab
    H = half_ulp_bf16(P.abs() + E) if slab_bf16 else torch.zeros_like(E)
    T = cp + (P.abs() + E + H).sum(0)
    return (E + H).sum(0) + (splits + 2) * U * T


def worst(got, want, bnd, P, *, tile, tapminor_bseg=0):
    """-> (largest err / bound, offenders, description of the worst element: its tile-local position in GEMM order and the split whose
    partial sum comes closest to the error - a lost or doubled partial shows there)."""
    err = (got.to(F64) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    bad = int((~(err <= bnd)).sum())                     # (NaN counts as an offender)
    flat = torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")).flatten()
    k = int(flat.argmax())
    Nj = got.shape[-1]
    i, j = k // Nj, k % Nj
    jg = j
    if tapminor_bseg:                                    # stored column c * S + s -> GEMM column s * bseg + c
        S = Nj // tapminor_bseg
        jg = (j % S) * tapminor_bseg + j // S
    e = float(err[i, j]) if bool(torch.isfinite(err[i, j])) else float("inf")
    s_near = int((P[:, i, j].abs() - e).abs().argmin())
    return float(flat[k]), bad, (f"row {i} col {j} (GEMM col {jg}, tile-local {i % tile}, {jg % tile}; nearest partial: split {s_near} of "
                                 f"{P.shape[0]}, |P_s| = {float(P[s_near, i, j].abs()):.4g}): got {float(got[i, j]):.9g} want "
                                 f"{float(want[i, j]):.9g} err {e:.3g} bound {float(bnd[i, j]):.3g}")


# ------------------------------------------------------------------------------------------------------------------ cases
def conv3x3_rowmap(H, W, dil):
    """int32 [9][H * W]: tap t = ky * 3 + kx of a 3x3 convolution with dilation = padding = dil reads input pixel
    (y + (ky - 1) * dil, x + (kx - 1) * dil) for output pixel m = y * W + x; -1 where that is padding.  Plain torch."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    rows = []
    for ky in range(3):
        for kx in range(3):
            yy, xx = y + (ky - 1) * dil, x + (kx - 1) * dil
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            rows.append(torch.where(ok, yy * W + xx, torch.full_like(yy, -1)).flatten())
    return torch.stack(rows).to(torch.int32)


@dataclasses.dataclass(frozen=True)
class Case:
    """One gemm_tn problem of the contract.  kernel: the code stswin_last_variant(1) must report (VAR_F32 included); req: the low bits of
    `splits` handed to the library (0: automatic); splits: the count it must report; bits: tuning bits of `splits`; maps: '' | 'a' | 'b' |
    'ab'; bseg > 0: Bt is an [H * W][bseg] image gathered through the first Nj / bseg taps of conv3x3_rowmap(*img, 2); form: what is
    ASKED for - '' (workspace, the library's default), 'atomics' (no workspace), 'f32slabs' (STSWIN_TN_F32_SLABS=1), 'nocombine'
    (STSWIN_TN_NO_COMBINE + stswin_tn_combine; 'nocombine+f32': with STSWIN_TN_F32_SLABS=1), 'unfused' (STSWIN_TN_FUSED=0)."""
    name: str
    kernel: int
    Mk: int
    Ni: int
    Nj: int
    splits: int
    req: int = 0
    bits: int = 0
    f32: bool = False
    maps: str = ""
    bseg: int = 0
    img: Optional[tuple] = None
    tapminor: bool = False
    form: str = ""

    @property
    def ring(self):
        return self.kernel in (RING_PLAIN, RING_ATROWS, RING_BTROWS, RING_BSEG)

    @property
    def rows(self):
        return self.kernel == ROWS

    @property
    def unit(self):
        return 32 if self.ring or self.f32 else 64

    @property
    def tile(self):
        return 256 if self.ring else 128

    @property
    def expect(self):
        """The combine form that must run: 'rows' | 'none' (splits == 1: no partials) | 'atomics' | 'f32' | 'bf16' (slabs + tn_reduce) |
        'fused' | 'explicit-f32' | 'explicit-bf16' (slabs + stswin_tn_combine)."""
        if self.rows:
            return "rows"
        if self.splits == 1:
            return "none"
        if self.form == "atomics":
            return "atomics"
        f32 = self.f32 or self.form in ("f32slabs", "nocombine+f32")
        if self.form.startswith("nocombine"):
            return "explicit-f32" if f32 else "explicit-bf16"
        if f32:
            return "f32"
        return "fused" if self.ring and self.form != "unfused" else "bf16"

    @property
    def slab_bf16(self):
        return self.expect in ("bf16", "fused", "explicit-bf16")

    @property
    def has_slabs(self):
        return self.expect in ("f32", "bf16", "fused", "explicit-f32", "explicit-bf16")

    @property
    def tapminor_honoured(self):
        """Only where slabs are combined by the library itself (stswin_tn_combine takes no permutation)."""
        return self.tapminor and self.expect in ("f32", "bf16", "fused")

    @property
    def word(self):
        """The raw stswin_last_variant(1) word."""
        if self.rows:
            return ROWS
        return (self.kernel | (self.splits << 16) | (SLABS_BF16 if self.slab_bf16 else SLABS_F32 if self.has_slabs else 0) |
                (FUSED if self.expect == "fused" else 0) | (TAPMINOR if self.tapminor_honoured else 0))

    def ranges(self):
        return partition(self.Mk, self.splits, self.unit)


def _k128_cases():
    out = []
    for f32 in (False, True):
        k, t = K128 + (VAR_F32 if f32 else 0), "f32" if f32 else "bf16"
        u = 32 if f32 else 64

        def c(name, Mk, Ni, Nj, req, **kw):
            out.append(Case(f"128x128 {t} {name}", kw.pop("kernel", k), Mk, Ni, Nj, corrected_splits(Mk, req, u) if req else 1, req=req,
                            f32=f32, **kw))
        c("one unit", 64, 128, 128, 0)
        c("splits=4 clamped", 33, 48, 64, 4)
        for Mk in (200, 201):
            c(f"ragged Mk={Mk} splits=3", Mk, 136, 264, 3)
            c(f"ragged Mk={Mk} auto", Mk, 136, 264, 0)
            for maps in ("a", "b", "ab"):
                c(f"maps {maps} Mk={Mk}", Mk, 136, 264, 3, maps=maps)
        for bseg, Nj in ((64, 576), (136, 408)):
            for tm in (False, True):
                c(f"bseg={bseg} Nj={Nj}" + (" tapminor" if tm else ""), 200, 136, Nj, 3, maps="b", bseg=bseg, img=(10, 20), tapminor=tm)
        c("bseg=64 tapminor, one split: not honoured", 200, 136, 576, 0, maps="b", bseg=64, img=(10, 20), tapminor=True)
        c("atomics", 200, 136, 264, 3, form="atomics")
        c("atomics bseg=64 tapminor: not honoured", 200, 136, 576, 3, maps="b", bseg=64, img=(10, 20), tapminor=True, form="atomics")
        c("no_combine + tn_combine", 201, 136, 264, 3, form="nocombine")
        if not f32:
            c("fp32 slabs", 200, 136, 264, 3, form="f32slabs")
            c("fp32 slabs bseg=136 tapminor", 200, 136, 408, 3, maps="b", bseg=136, img=(10, 20), tapminor=True, form="f32slabs")
            c("fp32 slabs, no_combine + tn_combine", 200, 136, 264, 3, form="nocombine+f32")
        # four waves
        k4 = K128_W4 + (VAR_F32 if f32 else 0)
        for Mk in (200, 201):
            c(f"w4 plain Mk={Mk}", Mk, 136, 264, 3, kernel=k4, bits=BIT_W4)
            c(f"w4 maps ab Mk={Mk}", Mk, 136, 264, 3, kernel=k4, bits=BIT_W4, maps="ab")
        c("w4 bseg=64", 200, 136, 576, 3, kernel=k4, bits=BIT_W4, maps="b", bseg=64, img=(10, 20))
    return out


def _ring_cases():
    out = []

    def c(name, kernel, Mk, Ni, Nj, rs, forms=("", "unfused"), **kw):
        for form in forms:
            out.append(Case(f"ring {name} rs={rs}" + (f" {form}" if form else ""), kernel, Mk, Ni, Nj, corrected_splits(Mk, rs, 32), req=rs,
                            bits=BIT_RING, form=form, **kw))
    c("96x256x256", RING_PLAIN, 96, 256, 256, 3, forms=("", "unfused", "f32slabs", "atomics", "nocombine"))
    c("96x256x256", RING_PLAIN, 96, 256, 256, 1, forms=("",))
    c("ragged 100x264x520", RING_PLAIN, 100, 264, 520, 2)
    c("1000x256x512", RING_PLAIN, 1000, 256, 512, 5)
    c("40x256x256", RING_PLAIN, 40, 256, 256, 8)
    c("at_rows 96x264x520", RING_ATROWS, 96, 264, 520, 3, maps="a")
    c("bt_rows 96x264x520", RING_BTROWS, 96, 264, 520, 3, maps="b")
    for tm in (False, True):
        t = " tapminor" if tm else ""
        c("bseg=128 96x256x1152" + t, RING_BSEG, 96, 256, 1152, 2, forms=("", "unfused", "f32slabs", "atomics"), maps="b", bseg=128,
          img=(8, 12), tapminor=tm)
        c("bseg=128 96x256x1152" + t, RING_BSEG, 96, 256, 1152, 1, forms=("",), maps="b", bseg=128, img=(8, 12), tapminor=tm)
    # the ring declines a row map with Mk % 32 != 0: the 128x128 kernel runs, with the requested split count
    out.append(Case("ring declined: at_rows Mk=100 rs=2", K128, 100, 264, 520, corrected_splits(100, 2, 64), req=2, bits=BIT_RING, maps="a"))
    return out


def cases():
    out = [Case("rows 1x8x8", ROWS, 1, 8, 8, 1), Case("rows 8x72x264", ROWS, 8, 72, 264, 1),
           Case("rows declined: at_rows 8x72x264", K128, 8, 72, 264, 1, maps="a")]
    out += _k128_cases() + _ring_cases()
    out.append(Case("automatic dispatch 22528x512x512", RING_PLAIN, 22528, 512, 512, 44))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def problem(c: Case, seed=0):
    """The operands of a case from a seed, on the CPU: dict(At, Bt, at_rows, bt_rows).  Every source buffer is TALLER than Mk and random
    throughout (a kernel that reads a row past the ragged tail adds it); every map has -1 rows, one of them in the last unit."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * c.Mk + c.Ni + c.Nj + c.bseg + len(c.maps))
    dt = F32 if c.f32 else BF
    Mk = c.Mk
    rows_a = Mk + (29 if "a" in c.maps else 7)
    At = torch.randn(rows_a, c.Ni, generator=g).to(dt)
    at_rows = bt_rows = None
    if "a" in c.maps:
        at_rows = torch.randint(0, rows_a, (Mk,), generator=g, dtype=torch.int32)
        at_rows[min(3, Mk - 1)] = -1
        at_rows[max(Mk - 2, 0)] = -1                      # (never row Mk - 1 itself: the tests plant "row Mk - 1 left out")
    if c.bseg > 0:
        H, W = c.img
        assert H * W == Mk and "b" in c.maps
        bt_rows = conv3x3_rowmap(H, W, 2)[:c.Nj // c.bseg].contiguous().flatten()
        assert int((bt_rows.view(-1, Mk)[:, Mk - c.unit:] < 0).sum()) > 0
        Bt = torch.randn(Mk + 11, c.bseg, generator=g).to(dt)
    elif "b" in c.maps:
        rows_b = Mk + 31
        bt_rows = torch.randint(0, rows_b, (Mk,), generator=g, dtype=torch.int32)
        bt_rows[min(5, Mk - 1)] = -1
        bt_rows[max(Mk - 3, 0)] = -1
        Bt = torch.randn(rows_b, c.Nj, generator=g).to(dt)
    else:
        Bt = torch.randn(Mk + 7, c.Nj, generator=g).to(dt)
    return {"At": At, "Bt": Bt, "at_rows": at_rows, "bt_rows": bt_rows}
