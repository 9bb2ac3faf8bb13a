"""The window-attention kernels (stswincl_amd/csrc/attention.hip) against the float64 reference of tests/attn_ref.py, per kernel x
call form x score regime x persistent partition (include/stswin_hip.h, a6 section).

Every case compares EVERY window with the reference evaluated on the operands the kernel multiplies (the bf16-rounded q | k | v
and dO; for the fp8-stored kernels the dequantised e4m3 values x scale) and prints its measured errors: the largest error over the
largest reference value ("max") and the relative L2 norm ("l2") of every output.

Call forms: the three bias_windows forms ("1": biasT + maskT; "nW": per-window pre-summed table; "U": slot table + bias_index,
what ops.SwinBlockFn passes) with the real SW-MSA masks (O.shift_attn_mask); scale in {1, d^-0.5} on the backward (dq carries it);
colsum_out on and off; dbiasT and colsum_out PRE-FILLED with non-zero values, so the result must be prefill + gradient (the ABI says
+=).

Regimes (score distributions):
  uniform   - 0.5 randn q | k | v, q pre-scaled: score std ~0.5, every softmax row nearly flat (the older tests' inputs);
  peaked    - score std ~6: rows close to one-hot;
  cross     - designed scores: each query's dominant key (+12 over a unit-normal background) lies in the OTHER frame of the pair, for
              every third query in the last key tile - the case where the 8-wave backward's two half-wave groups (one frame's keys
              each) must merge their (max, sum) pairs with the rescale, and where the forward's running max lives in the far tile;
  maskpeak  - designed scores with the real SW-MSA mask: where a query has masked keys, its largest RAW score (100 + 4..14) sits on
              one of them, beside an unmasked key of 4..14: the additive -100 leaves that masked key competitive, so a kernel that
              skipped masked keys or treated them as -inf would be wrong here;
  outlier   - fp8-stored kernels: q | k | v from the fp8 QKV GEMM with one 6x outlier token per window (as tests/test_hip_fp8.py).
Designed scores need a key basis: k = orthogonal rows x sqrt(d), q = S k / d (exact up to the bf16 rounding of q and k, which the
reference sees), so they run where a window has no more tokens than the head dimension (both production stages).

Bounds (max, l2), where each comes from:
  fp32 kernels: fp32 products and __expf / expf - ~1e-6 relative, bounded at a few 1e-6..1e-5;
  bf16 kernels: P and dS are rounded to bf16 (2^-9 relative) before the second products, the outputs to bf16 (2^-9);
  fp8 forward (fp8=True): q, k, v, P quantised in registers to e4m3 (2^-4 relative), against the bf16 operands;
  fp8-stored (f8) kernels: exact e4m3 operands; the forward rounds P to e4m3 (x 128): 2^-4; the backward recomputes P in fp32 and
  rounds P / dS to bf16 like the bf16 kernels.
Each bound is at most 2x the value measured on MI355X for that kernel family and regime (the printed lines; table BOUND), and never
looser than the older test of the same kernel (tests/test_hip_attention.py, test_hip_fp8.py).  Only the fp32 kernels need wider
bounds in a new regime ("maskpeak": raw scores above 100 make fp32's absolute rounding of a score ~1e-5); the bf16 and fp8 kernels
measure the same relative errors in every regime, because their error is the bf16 / e4m3 rounding of P, dS and the outputs.

Partitions: the backward kernels size their persistent grids from stswin_cu_budget() (stswin_set_cu_budget); dqkv has no sum across
workgroups, so it must be bitwise the same for every budget, while dbiasT / colsum are folded from per-workgroup slabs and are held to
the reference.  Window counts: the bench step's stage-1 count (512 windows: B = 4 clips, frame pairs as batch, 64 windows of a 64 x 64
map - taken from ops.ATTN_TAP on a bench-size forward) and counts whose problems leave a ragged last round of the grid."""
import time

import pytest
import torch

import attn_ref as R
from oracle import stswin_oracle as O
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
T = 2
BENCH_STAGE1_WINDOWS = 512           # ops.ATTN_TAP at bench size (512 x 512 frames, B = 4): Bp = 8 frame pairs x nW = 64 (stage-1 layers 0, 2)

GEOM = {"s1": (8, 512, 4),           # stage 1: ws 8, C 512, 4 heads (128 tokens, head dim 128)
        "s2": (4, 1024, 4),          # stage 2: ws 4, C 1024, 4 heads (32 tokens, head dim 256)
        "red": (8, 128, 4)}          # reduced width (dispatch_attn CASE(128, 32))

# (max, l2) per (kernel family, regime) and output: 1.9 x the largest value measured on MI355X over the family's kernels and call
# forms (rounded to two digits), capped where an older test of the same kernel is tighter (f8 forward: l2 3e-2, max 8e-2; fp8-mode
# forward: l2 6e-2, max 0.12).  Measured: bf16 ~2.4e-3 l2 for every output and regime (bf16 rounding of P, dS and the stored
# result: 2^-9); f32 2e-7..3e-6, and up to 1.6e-5 in "maskpeak" - its raw scores of ~110 carry an fp32 rounding of ~110 x 2^-24 =
# 7e-6 into the exponent, i.e. into every probability of the row; dbias, summed in fp32 over 32+ windows, 2e-7..9e-6 of its
# scale; f8 forward 1.8e-2 l2 (P in e4m3: 2^-4 per element); fp8-mode forward 5.5e-2 l2.
BOUND = {
    ("bf16", "cross"): {"colsum": (1.1e-03, 4.7e-03), "dbias": (1.6e-05, 9.0e-06), "dk": (8.2e-03, 4.5e-03), "dq": (9.2e-03, 4.5e-03), "dv": (7.0e-03, 3.6e-03), "out": (8.9e-03, 3.1e-03)},
    ("bf16", "maskpeak"): {"colsum": (6.0e-04, 4.6e-03), "dbias": (9.8e-06, 7.9e-06), "dk": (6.8e-03, 4.4e-03), "dq": (7.0e-03, 4.4e-03), "dv": (7.3e-03, 3.9e-03), "out": (9.2e-03, 3.7e-03)},
    ("bf16", "peaked"): {"colsum": (1.0e-03, 4.8e-03), "dbias": (2.4e-06, 1.3e-06), "dk": (9.2e-03, 4.5e-03), "dq": (7.2e-03, 4.7e-03), "dv": (6.2e-03, 4.1e-03), "out": (8.4e-03, 4.1e-03)},
    ("bf16", "uniform"): {"colsum": (1.7e-03, 5.3e-03), "dbias": (4.0e-07, 5.7e-07), "dk": (7.7e-03, 4.5e-03), "dq": (6.9e-03, 4.5e-03), "dv": (7.0e-03, 4.5e-03), "out": (8.9e-03, 4.4e-03)},
    ("f32", "cross"): {"colsum": (7.2e-07, 5.8e-06), "dbias": (1.2e-05, 6.3e-06), "dk": (6.1e-06, 5.7e-06), "dq": (5.1e-06, 5.7e-06), "dv": (1.3e-06, 5.0e-07), "out": (1.7e-06, 5.0e-07)},
    ("f32", "maskpeak"): {"colsum": (2.6e-06, 1.9e-05), "dbias": (2.7e-05, 1.9e-05), "dk": (3.1e-05, 2.0e-05), "dq": (2.6e-05, 1.8e-05), "dv": (1.5e-05, 5.6e-06), "out": (2.8e-05, 5.7e-06)},
    ("f32", "peaked"): {"colsum": (5.8e-07, 3.2e-06), "dbias": (4.2e-06, 3.1e-06), "dk": (5.3e-06, 3.1e-06), "dq": (6.6e-06, 3.1e-06), "dv": (3.2e-06, 1.7e-06), "out": (5.6e-06, 1.7e-06)},
    ("f32", "uniform"): {"colsum": (2.4e-07, 6.6e-07), "dbias": (8.1e-07, 6.8e-07), "dk": (8.6e-07, 6.0e-07), "dq": (9.2e-07, 6.0e-07), "dv": (4.6e-07, 3.8e-07), "out": (5.3e-07, 3.8e-07)},
    ("f8", "cross"): {"colsum": (9.6e-04, 4.6e-03), "dbias": (1.1e-05, 4.4e-06), "dk": (6.4e-03, 4.5e-03), "dq": (6.8e-03, 4.5e-03), "dv": (7.9e-03, 3.6e-03), "out": (4.6e-02, 1.5e-02)},
    ("f8", "outlier"): {"colsum": (5.8e-04, 5.1e-03), "dbias": (2.0e-06, 2.1e-06), "dk": (6.9e-03, 4.5e-03), "dq": (9.4e-03, 4.5e-03), "dv": (7.5e-03, 4.2e-03), "out": (6.1e-02, 3.0e-02)},
    ("fp8fwd", "uniform"): {"out": (1.2e-01, 6.0e-02)},
    ("qkv", "peaked"): {"out": (8.0e-03, 4.1e-03), "qkv": (4.6e-03, 3.2e-03)},
    ("qkv", "uniform"): {"out": (9.1e-03, 4.2e-03), "qkv": (5.6e-03, 3.2e-03)},
}
OWN_COLSUM_BOUND = 1.5e-7   # colsum against the fp64 column sums of the kernel's own dq output, on the scale max |dq| sqrt(rows)
                            # (the same bf16 values summed in fp32 in another order; measured <= 7.1e-8)


def _bound(fam, regime, what):
    return BOUND[(fam, regime)][what]


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[attention contract] wall time {time.perf_counter() - t0:.1f} s")


@pytest.fixture
def cu_budget():
    """set_cu_budget(k) inside a test, 0 (the whole device) restored whatever happens."""
    try:
        yield hip.set_cu_budget
    finally:
        hip.set_cu_budget(0)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _mask(ws, nW):
    """the real SW-MSA mask of a square map of nW windows: [nW][N][N] (query, key) in {0, -100}"""
    side = int(round(nW ** 0.5))
    assert side * side == nW
    return O.shift_attn_mask(side * ws, side * ws, ws, ws // 2)


def _bias_form(form, bias, mask, nW):
    """bias [heads][N][N], mask [nW][N][N] (query, key; fp32) -> (biasT, maskT, bias_index) on the GPU in the kernels' layout"""
    bT = bias.transpose(1, 2).contiguous()
    mT = mask.transpose(1, 2).contiguous()
    if form == "1":
        return bT.cuda(), mT.cuda(), None
    if form == "nW":
        return (bT[None] + mT[:, None]).contiguous().cuda(), None, None
    umask, inv = torch.unique(mask.reshape(nW, -1), dim=0, return_inverse=True)
    table = (bT[None] + umask.reshape(-1, *mask.shape[1:]).transpose(1, 2)[:, None]).contiguous()
    assert table.shape[0] < nW or nW <= 4
    return table.cuda(), None, inv.to(torch.int32).cuda()


def _designed_qkv(S, d, g):
    """S [nB_][heads][TN][TN] wanted scores (float64) -> q | k | v rows (float64) with q_s k^T = S (before rounding): k rows
    orthogonal, |k| = sqrt(d) (a pool of random orthogonal bases, rows permuted per problem), v unit normal."""
    nB_, heads, ntok, _ = S.shape
    assert ntok <= d
    pool = torch.linalg.qr(torch.randn(16, d, d, generator=g, dtype=F64))[0]
    pick = torch.randint(0, 16, (nB_ * heads,), generator=g)
    perm = torch.argsort(torch.rand(nB_ * heads, d, generator=g), dim=1)[:, :ntok]
    k = pool[pick].gather(1, perm[:, :, None].expand(-1, -1, d)).reshape(nB_, heads, ntok, d) * d ** 0.5
    q = S @ k / d
    v = torch.randn(nB_, heads, ntok, d, generator=g, dtype=F64)
    rows = lambda x: x.transpose(1, 2).reshape(nB_ * ntok, heads * d)      # noqa: E731
    return torch.cat([rows(q), rows(k), rows(v)], 1)


def _qkv(regime, ws, C, heads, nB_, mask, seed):
    """float64 q (pre-scaled) | k | v rows [nB_ T N][3C] of a regime"""
    g = torch.Generator().manual_seed(seed)
    N, d = ws * ws, C // heads
    ntok, rows = T * N, nB_ * T * ws * ws
    if regime in ("uniform", "peaked"):
        sd = 0.5 if regime == "uniform" else 6.0 ** 0.5          # score std = sd^2 (q carries d^-0.5)
        x = torch.randn(rows, 3 * C, generator=g, dtype=F64)
        x[:, :2 * C] *= sd
        x[:, 2 * C:] *= 0.5 if regime == "uniform" else 1.0
        x[:, :C] *= d ** -0.5
        return x
    S = torch.randn(nB_, heads, ntok, ntok, generator=g, dtype=F64)
    i = torch.arange(ntok)
    t_i, n_i = i // N, i % N
    if regime == "cross":
        other = (T - 1) - t_i                                   # (T = 2: the other frame of the pair)
        tgt = other * N + (n_i * 7 + 3) % N
        last = (other == T - 1) & (n_i % 3 == 0)                # ... for every third frame-0 query: a key of the last 32-key tile
        tgt = torch.where(last, ntok - 1 - (n_i * 5) % min(32, N), tgt)
        assert bool((tgt // N != t_i).all())
        S[:, :, i, tgt] += 12.0
    elif regime == "maskpeak":
        nW = mask.shape[0]
        m = mask.repeat(1, T, T)                                # [nW][TN][TN] (query, key)
        for w in range(nW):
            masked = m[w] < 0
            for q_ in range(ntok):
                keys = torch.nonzero(masked[q_]).flatten()
                free = torch.nonzero(~masked[q_]).flatten()
                j2 = free[(q_ * 11 + w) % len(free)]
                sel = slice(w, nB_, nW)
                S[sel, :, q_, j2] = 4.0 + 10.0 * torch.rand(nB_ // nW, heads, 1, generator=g, dtype=F64).squeeze(-1)
                if len(keys):
                    j1 = keys[(q_ * 5 + w) % len(keys)]
                    S[sel, :, q_, j1] = 104.0 + 10.0 * torch.rand(nB_ // nW, heads, 1, generator=g, dtype=F64).squeeze(-1)
    else:
        raise ValueError(regime)
    return _designed_qkv(S, d, g)


def _setup(gname, regime, nB_, nW, seed, dtype):
    ws, C, heads = GEOM[gname]
    N = ws * ws
    mask = _mask(ws, nW)
    g = torch.Generator().manual_seed(seed + 1)
    bias = torch.randn(heads, N, N, generator=g) * 0.5
    x = _qkv(regime, ws, C, heads, nB_, mask, seed).to(dtype)
    dout = torch.randn(nB_ * T * N, C, generator=g).to(dtype)
    return ws, C, heads, N, mask, bias, x, dout


def _report(tag, errs, fam, regime):
    """print one line of measured errors, then assert every one against its bound"""
    print(f"{tag}: " + " | ".join(f"{k} max {e[0]:.2e} l2 {e[1]:.2e}" for k, e in errs.items()), flush=True)
    bad = [(k, e, _bound(fam, regime, k)) for k, e in errs.items() if not (e[0] <= _bound(fam, regime, k)[0] and e[1] <= _bound(fam, regime, k)[1])]
    assert not bad, f"{tag}: {bad}"


def _colsum_err(cs, pre, ref_cs, dq_ref, dq_got, rows):
    """colsum against prefill + the reference, on the natural scale of a column sum of rows dq values (max |dq| sqrt(rows)); and
    against the column sums of the kernel's own dq output (the same values summed in fp32 in another order: ~1e-6)"""
    scl = float(dq_ref.abs().max()) * rows ** 0.5
    got = cs.to(F64) - pre.to(F64)
    e_ref = float((got - ref_cs).abs().max()) / scl
    e_own = float((got - dq_got.to(F64).sum(0)).abs().max()) / scl
    return e_ref, float((got - ref_cs).norm() / ref_cs.norm()), e_own


# ------------------------------------------------------------------------------------------------------------------ forward
FWD_CASES = [(dt, gname, form, regime) for dt in ("f32", "bf16") for gname in ("s1", "s2", "red") for form in ("1", "nW", "U")
             for regime in (("uniform", "peaked") if gname == "red" else ("uniform", "peaked", "cross", "maskpeak"))]


@pytest.mark.parametrize("dt,gname,form,regime", FWD_CASES)
def test_forward(dt, gname, form, regime):
    """stswin_win_attn_fwd (attn_fwd_kernel; the training forward of the two-kernel path) in fp32 and bf16"""
    nW, nB_ = 16, 32
    dtype = F32 if dt == "f32" else BF
    ws, C, heads, N, mask, bias, x, _ = _setup(gname, regime, nB_, nW, 11, dtype)
    biasT, maskT, bidx = _bias_form(form, bias, mask, nW)
    out = hip.win_attn_fwd(x.cuda(), biasT, maskT, nB_=nB_, nW=nW, T=T, ws=ws, heads=heads, C=C, bias_index=bidx)
    ref = R.attention(x.cuda(), biasT, maskT, T=T, ws=ws, heads=heads, C=C, nW=nW, bias_index=bidx)["out"]
    _report(f"fwd {dt} {gname} form={form} {regime}", {"out": R.errors(out, ref)}, dt, regime)


@pytest.mark.parametrize("gname,form", [(gname, form) for gname in ("s1", "s2", "red") for form in ("1", "nW", "U")])
def test_forward_fp8_mode(gname, form):
    """stswin_win_attn_fwd_fp8 (fp8=True: q, k, v and P quantised to e4m3 in registers), uniform regime only: against the bf16
    operands, which is what the mode approximates (peaked rows would measure the quantisation of one logit, not the kernel)"""
    nW, nB_ = 16, 32
    ws, C, heads, N, mask, bias, x, _ = _setup(gname, "uniform", nB_, nW, 12, BF)
    x[5::T * N] *= 6.0                                         # an outlier row per window: the per-problem amax absorbs it
    biasT, maskT, bidx = _bias_form(form, bias, mask, nW)
    out = hip.win_attn_fwd(x.cuda(), biasT, maskT, nB_=nB_, nW=nW, T=T, ws=ws, heads=heads, C=C, bias_index=bidx, fp8=True)
    ref = R.attention(x.cuda(), biasT, maskT, T=T, ws=ws, heads=heads, C=C, nW=nW, bias_index=bidx)["out"]
    _report(f"fwd fp8-mode {gname} form={form} uniform", {"out": R.errors(out, ref)}, "fp8fwd", "uniform")


@pytest.mark.parametrize("form,regime", [(f, r) for f in ("1", "nW", "U") for r in ("uniform", "peaked")])
def test_qkv_fused_forward(form, regime):
    """stswin_win_attn_qkv_fwd (stage 1 only): the attention part against the reference on the q * scale | k | v rows the kernel
    hands out (bf16, the values it multiplies), and those rows against the float64 projection of the same bf16 tokens / weights.
    form "1" is the unshifted block (no mask); "nW" / "U" carry the SW-MSA mask in the table."""
    from stswincl_amd import ops
    ws, C, heads = GEOM["s1"]
    N, d = ws * ws, C // heads
    Bc, H, W = 2, 16, 32
    nW = (H // ws) * (W // ws)
    nB_ = Bc * nW
    g = torch.Generator().manual_seed(21)
    x = torch.randn(Bc * T * H * W, C, generator=g).to(BF)
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5 * (1.0 if regime == "uniform" else 6.0 ** 0.5)).to(BF)
    bq = torch.randn(3 * C, generator=g) * 0.1
    bias = torch.randn(heads, N, N, generator=g) * 0.5
    shift = 0 if form == "1" else ws // 2
    mask = O.shift_attn_mask(H, W, ws, shift) if shift else torch.zeros(nW, N, N)
    rmap = ops.window_rowmap(Bc, T, H, W, ws, shift, "cuda")
    if form == "1":
        biasT, bidx = bias.transpose(1, 2).contiguous().cuda(), None
    else:
        biasT, _, bidx = _bias_form(form, bias, mask, nW)
    out, qkv = hip.win_attn_qkv_fwd(x.cuda(), rmap, w.cuda(), bq.cuda(), biasT, nB_=nB_, nW=nW, T=T, ws=ws, heads=heads, C=C,
                                    scale=d ** -0.5, bias_index=bidx)
    ref = R.attention(qkv, biasT, None, T=T, ws=ws, heads=heads, C=C, nW=nW, bias_index=bidx)
    proj = x.cuda().to(F64)[rmap.long()] @ w.cuda().to(F64).t() + bq.cuda().to(F64)
    proj[:, :C] *= d ** -0.5
    e_qkv = R.errors(qkv, proj)
    s = R.scores(qkv, biasT, None, T=T, ws=ws, heads=heads, C=C, nW=nW, bias_index=bidx)
    _report(f"qkv-fused s1 form={form} {regime} (score std {float((s - s.mean(-1, keepdim=True)).std()):.1f})",
            {"out": R.errors(out, ref["out"]), "qkv": e_qkv}, "qkv", regime)


@pytest.mark.parametrize("gname,form,regime", [(g_, f, r) for g_ in ("s1", "s2") for f in ("1", "nW", "U") for r in ("outlier", "cross")])
def test_forward_f8(gname, form, regime):
    """stswin_win_attn_fwd_f8 (fp8-stored q | k | v, both products on the fp8 MFMA) against the reference on the dequantised
    operands: what is left is the e4m3 rounding of P (x 128) and fp32 summation order"""
    ws, C, heads = GEOM[gname]
    nW, nB_ = 16, 32
    q8, sc, deq, bias, mask, _ = _f8_inputs(gname, regime, nB_, nW, 13)
    biasT, maskT, bidx = _bias_form(form, bias, mask, nW)
    out = hip.win_attn_fwd_f8(q8, sc, biasT, maskT, nB_=nB_, nW=nW, T=T, ws=ws, heads=heads, C=C, bias_index=bidx)
    ref = R.attention(deq, biasT, maskT, T=T, ws=ws, heads=heads, C=C, nW=nW, bias_index=bidx)["out"]
    _report(f"fwd f8 {gname} form={form} {regime}", {"out": R.errors(out, ref)}, "f8", regime)


# ------------------------------------------------------------------------------------------------------------------ backward
def _run_bwd(kernel, monkeypatch, x, dout, biasT, maskT, bidx, nB_, nW, ws, heads, C, scale, dbT, cs, q8=None, sc=None):
    if kernel == "f8":
        return hip.win_attn_bwd_f8(q8, sc, dout.cuda(), biasT, maskT, dbT, nB_=nB_, nW=nW, T=T, ws=ws, heads=heads, C=C, scale=scale,
                                   colsum_out=cs, bias_index=bidx)
    monkeypatch.setenv("STSWIN_ATTN_BWD4", "1" if kernel == "bwd4" else "0")
    return hip.win_attn_bwd(x.cuda(), dout.cuda(), biasT, maskT, dbT, nB_=nB_, nW=nW, T=T, ws=ws, heads=heads, C=C, scale=scale,
                            colsum_out=cs, bias_index=bidx)


def _f8_inputs(gname, regime, nB_, nW, seed):
    """(q8, scales, dequantised float64 q | k | v on the GPU, bias, mask, dout) for the fp8-stored kernels: regime "outlier" = the
    fp8 QKV GEMM's own output (one 6x token per window), otherwise a designed q | k | v quantised by attn_ref.e4m3_quantise"""
    ws, C, heads = GEOM[gname]
    N, d = ws * ws, C // heads
    rows = nB_ * T * N
    g = torch.Generator().manual_seed(seed)
    if regime == "outlier":
        xt = torch.randn(rows, C, generator=g).to(BF)
        xt[5::T * N] *= 6.0
        w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).to(BF)
        b = torch.randn(3 * C, generator=g) * 0.1
        q8, sc = hip.gemm_nt_qkv_fp8(xt.cuda(), w.cuda(), M=rows, bias=b.cuda(), scale=d ** -0.5, scale_cols=C, rows_per_problem=T * N,
                                     head_dim=d)
    else:
        q8, sc = R.e4m3_quantise(_qkv(regime, ws, C, heads, nB_, _mask(ws, nW), seed), T * N, d)
        q8, sc = q8.cuda(), sc.cuda()
    deq = R.e4m3_dequantise(q8, sc, T * N, d)
    bias = torch.randn(heads, N, N, generator=g) * 0.5
    dout = torch.randn(rows, C, generator=g).to(BF)
    return q8, sc, deq, bias, _mask(ws, nW), dout


def _check_bwd(tag, fam, regime, kernel, monkeypatch, gname, nB_, nW, form, scale_kind, colsum, seed):
    ws, C, heads = GEOM[gname]
    N, d = ws * ws, C // heads
    scale = 1.0 if scale_kind == "1" else d ** -0.5
    q8 = sc = None
    if kernel == "f8":
        q8, sc, xref, bias, mask, dout = _f8_inputs(gname, regime, nB_, nW, seed)
        x = None
    else:
        ws, C, heads, N, mask, bias, x, dout = _setup(gname, regime, nB_, nW, seed, F32 if fam == "f32" else BF)
        xref = x.cuda()
    biasT, maskT, bidx = _bias_form(form, bias, mask, nW)
    ref = R.attention(xref, biasT, maskT, T=T, ws=ws, heads=heads, C=C, nW=nW, bias_index=bidx, dout=dout.cuda(), scale=scale)
    gpre = torch.Generator().manual_seed(seed + 7)
    pre_db = (torch.randn(heads, N, N, generator=gpre) * float(ref["dbiasT"].abs().max())).cuda()
    pre_cs = (torch.randn(C, generator=gpre) * float(ref["colsum"].abs().max())).cuda()
    dbT = pre_db.clone()
    cs = pre_cs.clone() if colsum else None
    dqkv = _run_bwd(kernel, monkeypatch, x, dout, biasT, maskT, bidx, nB_, nW, ws, heads, C, scale, dbT, cs, q8, sc)
    errs = {"dq": R.errors(dqkv[:, :C], ref["dq"]), "dk": R.errors(dqkv[:, C:2 * C], ref["dk"]),
            "dv": R.errors(dqkv[:, 2 * C:], ref["dv"]), "dbias": R.errors(dbT.to(F64) - pre_db.to(F64), ref["dbiasT"])}
    extra = ""
    if colsum:
        e_ref, l2, e_own = _colsum_err(cs, pre_cs, ref["colsum"], ref["dq"], dqkv[:, :C], nB_ * T * N)
        errs["colsum"] = (e_ref, l2)
        extra = f" (colsum vs own dq {e_own:.1e})"
    # prefill + gradient: an overwrite leaves an error of the prefill's size (~1 x the gradient scale)
    _report(f"{tag}{extra}", errs, fam, regime)
    if colsum:
        assert e_own < OWN_COLSUM_BOUND, f"{tag}: colsum is not the column sums of the kernel's dq ({e_own})"
    return dqkv, dbT, cs, ref


BWD_VARIANTS = {            # name -> (kernel, geometry, family)
    "bwd8-s1-bf16": ("bwd8", "s1", "bf16"),          # production stage 1: attn_bwd8_kernel
    "bwd4-s1-bf16": ("bwd4", "s1", "bf16"),          # STSWIN_ATTN_BWD4=1: attn_bwd_kernel<bf16, 128, 128, 64>
    "bwd-s2-bf16": ("bwd", "s2", "bf16"),            # stage 2: attn_bwd_kernel<bf16, 32, 256, 16>
    "bwd-s1-f32": ("bwd", "s1", "f32"),
    "bwd-s2-f32": ("bwd", "s2", "f32"),
    "bwd-red-bf16": ("bwd", "red", "bf16"),          # attn_bwd_kernel<bf16, 128, 32, 0>
    "bwd-red-f32": ("bwd", "red", "f32"),
    "f8-s1": ("f8", "s1", "f8"),                     # stswin_win_attn_bwd_f8 stage 1: attn_bwd8_kernel<64, true, true>
    "f8-s2": ("f8", "s2", "f8"),                     # ... stage 2: attn_bwd_kernel<bf16, 32, 256, 16, true>
}
CALL_FORMS = [("1", "d", True), ("nW", "1", False), ("U", "d", True), ("U", "1", True)]   # (bias form, scale, colsum_out)


def _regimes(name):
    kernel, gname, fam = BWD_VARIANTS[name]
    if fam == "f8":
        return ("outlier", "cross")
    return ("uniform", "peaked") if gname == "red" else ("uniform", "peaked", "cross", "maskpeak")


BWD_CASES = [(name, form, sk, cs, regime) for name in BWD_VARIANTS for (form, sk, cs) in CALL_FORMS for regime in _regimes(name)]


@pytest.mark.parametrize("name,form,scale_kind,colsum,regime", BWD_CASES)
def test_backward(name, form, scale_kind, colsum, regime, monkeypatch):
    """dq (x scale), dk, dv, dbiasT (+=) and the dq column sums (+=) of every backward kernel, 32 windows (128 problems)"""
    kernel, gname, fam = BWD_VARIANTS[name]
    _check_bwd(f"{name} form={form} scale={scale_kind} colsum={int(colsum)} {regime}", fam, regime, kernel, monkeypatch, gname, 32, 16,
               form, scale_kind, colsum, 31)


PART_VARIANTS = ["bwd8-s1-bf16", "bwd4-s1-bf16", "bwd-s2-bf16", "f8-s1", "f8-s2"]


@pytest.mark.parametrize("name", ["bwd8-s1-bf16", "bwd4-s1-bf16", "f8-s1"])
def test_backward_at_the_bench_window_count(name, monkeypatch):
    """stage 1 at the bench step's window count (512 windows x 4 heads = 2048 problems, 8 per workgroup of the full device), U
    form with the real 64-window stage-1 mask, scale d^-0.5: every window against the reference"""
    kernel, gname, fam = BWD_VARIANTS[name]
    regime = "cross" if fam != "f8" else "outlier"
    _check_bwd(f"{name} bench windows={BENCH_STAGE1_WINDOWS} {regime}", fam, regime, kernel, monkeypatch, gname, BENCH_STAGE1_WINDOWS,
               64, "U", "d", True, 41)


@pytest.mark.parametrize("name", PART_VARIANTS)
def test_backward_ragged_last_round(name, monkeypatch):
    """window counts whose problems are not a multiple of the persistent grid: stage 1 100 windows = 400 problems on 256
    workgroups, stage 2 264 windows = 264 groups of 4 on 256 workgroups - some workgroups run one problem less"""
    kernel, gname, fam = BWD_VARIANTS[name]
    nB_ = 100 if gname == "s1" else 264                    # (x 128 / x 32 rows: multiples of 256, as the fp8 QKV GEMM wants)
    regime = "cross" if fam != "f8" else "outlier"
    _check_bwd(f"{name} ragged windows={nB_} {regime}", fam, regime, kernel, monkeypatch, gname, nB_, 4, "U", "d", True, 51)


@pytest.mark.parametrize("name", PART_VARIANTS)
def test_backward_under_cu_budgets(name, monkeypatch, cu_budget):
    """The same backward call with stswin_set_cu_budget(k) for k in 256, 160, 37, 4 (grids of 256 .. 4 workgroups, up to 32
    problems per workgroup): dqkv bitwise equal to the default grid's (every problem is computed whole by one workgroup), dbiasT and
    colsum (folded from per-workgroup slabs in another grouping) held to the reference"""
    kernel, gname, fam = BWD_VARIANTS[name]
    regime = "cross" if fam != "f8" else "outlier"
    base = None
    for k in (0, 256, 160, 37, 4):
        cu_budget(k)
        got = _check_bwd(f"{name} cu_budget={k} {regime}", fam, regime, kernel, monkeypatch, gname, 32, 16, "U", "d", True, 61)
        if base is None:
            base = got
        else:
            assert torch.equal(got[0], base[0]), f"dqkv differs under cu_budget {k}"
