"""The BatchNorm kernels (stswincl_amd/csrc/headops.hip: colstats, bn_finalize, cs_group_reduce, bn_table_finalize,
bn_running_update, bn_apply, bn_bwd in phase 0 and phases 1 + 2, bn_relu_pool) against the float64 reference of tests/bn_ref.py,
called through the hip.* entry points, fp32 and bf16.

Every case compares every row and channel with the reference evaluated on the operands the kernel reads (the stored fp32 / bf16 x)
and prints its measured errors.  Metrics:
  mean     max |mean - ref| / ref std (the std of the group: an absolute error in units of the deviation);
  rstd     max |rstd / ref - 1|;   rm / rv  running mean (units of std) / running var (relative);
  y, dx    (max, l2) as tests/attn_ref.py: largest error over the largest reference value, relative L2 norm;
  s        s1 / s2 / group_sums of bn_bwd, (max, l2).
The backward is checked from the kernel's own mean / rstd (the reference gets them as inputs) and with the ReLU mask of the kernel's
output (a value rounded to 0 is a selection, not an arithmetic error).

Shapes: M from 37 rows up to the stem (4 x 256 x 320 rows, 64 channels), layer1 (8 frames of 128 x 160, interleaved units), ASPP at
32 x 32 with 24 groups; C of 64, 128, 256 and 48 (48 bf16 channels are 6 column pieces: a partial column block, pick_cpb < 32).
Regimes: "normal" (|mean| / std <= 1), "ratio30", "ratio300" (|mean| / std ~ 30 / 300: where pivot-shifted and raw sums differ),
"const" (8 constant channels: var 0, rstd = eps^-1/2), "relu0" (post-ReLU-like: ~half the values exactly 0).

Bounds: at most 2x the error measured on MI355X for the kernel, dtype and regime (table BOUND).  The raw-sum paths (bn_finalize
raw=True, bn_table_finalize) compute E[x^2] - E[x]^2: at |mean| / std = 300 that loses ~300^2 x 2^-24 of the variance in fp32 sums,
which is why their "ratio300" bounds are wide and why production takes them only from convolution outputs (|mean| / std ~ 1).
"""
import time

import pytest
import torch

import bn_ref as R
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS, MOM = 1e-5, 0.1
REGIMES = ["normal", "ratio30", "ratio300", "const", "relu0"]

# Bounds per key of _check: 1.8 x the largest error measured on MI355X over the key's cases, rounded up to two digits (<= 2x).
# Measured (fp32 | bf16): y / dx / pool ~1e-7 | ~3e-3 max, 1.7e-3 l2 (the bf16 rounding of the stored result, 2^-9); mean 5e-7 std,
# rstd 2e-6 relative from the pivot-shifted sums in every regime but ratio300 (mean 2e-5 std: fp32 rounding of |mean| / std = 300);
# raw sums (bn_finalize raw, bn_table_finalize): rstd 1.6e-2 (f32) / 9e-3 (bf16) at ratio300, 1.5e-4 at ratio30, 1.2e-2 on a
# constant channel (E[x^2] - E[x]^2 in fp32 leaves ~mean^2 x 2^-24 against eps); running var 5e-7..5e-3 likewise; the epilogue
# table of a bf16 GEMM 3.6e-4 rstd (fp32 accumulators against the bf16-rounded output the reference sees).
BOUND = {
    ('apply', 'bf16'): (6.5e-03, 3.1e-03),
    ('apply', 'f32'): (1.7e-05, 1.5e-05),
    ('cs_group_reduce',): (3.0e-07,),
    ('dx', 'bf16', 'eval', 'ord'): (5.7e-03, 3.1e-03),
    ('dx', 'bf16', 'eval', 'ratio300'): (5.0e-03, 3.1e-03),
    ('dx', 'bf16', 'train', 'ord'): (5.6e-03, 3.3e-03),
    ('dx', 'bf16', 'train', 'ratio300'): (5.8e-03, 3.1e-03),
    ('dx', 'f32', 'eval', 'ord'): (1.5e-07, 6.7e-08),
    ('dx', 'f32', 'eval', 'ratio300'): (1.4e-07, 7.4e-08),
    ('dx', 'f32', 'train', 'ord'): (2.8e-07, 1.1e-07),
    ('dx', 'f32', 'train', 'ratio300'): (4.7e-06, 4.2e-06),
    ('dx_ranks', 'bf16'): (6.0e-03, 3.1e-03),
    ('dx_ranks', 'f32'): (2.7e-07, 9.7e-08),
    ('finalize', 'bf16', 'const'): (5.3e-07, 1.3e-06, 5.2e-05, 5.7e-07),
    ('finalize', 'bf16', 'ord'): (1.4e-06, 5.1e-06, 5.5e-07, 1.6e-06),
    ('finalize', 'bf16', 'ratio30'): (2.8e-06, 4.0e-06, 1.5e-05, 9.1e-07),
    ('finalize', 'bf16', 'ratio300'): (3.4e-05, 8.3e-07, 1.6e-04, 7.6e-07),
    ('finalize', 'f32', 'const'): (1.1e-06, 4.4e-06, 4.6e-05, 1.1e-06),
    ('finalize', 'f32', 'ord'): (9.5e-07, 3.0e-06, 5.0e-07, 8.9e-07),
    ('finalize', 'f32', 'ratio30'): (3.2e-06, 3.3e-06, 1.8e-05, 1.1e-06),
    ('finalize', 'f32', 'ratio300'): (3.0e-05, 3.6e-06, 1.8e-04, 8.1e-07),
    ('finalize_raw', 'bf16', 'const'): (2.5e-07, 4.2e-07, 4.0e-04, 1.6e-06),
    ('finalize_raw', 'bf16', 'ord'): (2.4e-07, 3.7e-07, 5.4e-07, 1.1e-06),
    ('finalize_raw', 'bf16', 'ratio30'): (4.5e-06, 2.0e-04, 1.6e-05, 6.3e-05),
    ('finalize_raw', 'bf16', 'ratio300'): (4.1e-05, 1.7e-02, 1.6e-04, 6.0e-03),
    ('finalize_raw', 'f32', 'const'): (6.8e-05, 2.2e-02, 2.0e-04, 1.6e-06),
    ('finalize_raw', 'f32', 'ord'): (2.6e-07, 4.6e-07, 5.6e-07, 1.4e-06),
    ('finalize_raw', 'f32', 'ratio30'): (6.1e-06, 2.7e-04, 1.8e-05, 1.7e-04),
    ('finalize_raw', 'f32', 'ratio300'): (7.8e-05, 2.9e-02, 1.8e-04, 8.2e-03),
    ('gemm_table', 'bf16'): (3.7e-04, 6.6e-04, 5.7e-05, 2.5e-04),
    ('gemm_table', 'f32'): (2.3e-07, 3.6e-07, 4.0e-07, 6.7e-07),
    ('pool', 'bf16'): (5.8e-03, 3.1e-03),
    ('pool', 'f32'): (1.9e-07, 9.6e-08),
    ('pool_dx', 'bf16'): (1.1e-02, 4.0e-03),
    ('pool_dx', 'f32'): (3.5e-07, 1.1e-07),
    ('pool_gs', 'bf16'): (3.0e-03, 3.0e-03),
    ('pool_gs', 'f32'): (4.2e-07, 3.6e-07),
    ('s', 'bf16'): (4.1e-07, 3.1e-07),
    ('s', 'f32'): (6.0e-07, 4.0e-07),
    ('table', 'const'): (1.9e-07, 8.1e-03, 4.0e-04, 1.6e-06),
    ('table', 'ord'): (1.8e-07, 3.0e-07, 5.7e-07, 1.3e-06),
    ('table', 'ratio30'): (6.8e-06, 1.5e-04, 1.7e-05, 8.3e-05),
    ('table', 'ratio300'): (6.2e-05, 1.8e-02, 1.8e-04, 6.7e-03),
}
MEASURED = {}


def _bound(key):
    return BOUND[key]


def _check(key, *vals):
    """record the measured errors of `key` and hold them to BOUND[key] (same arity)"""
    MEASURED.setdefault(key, [0.0] * len(vals))
    MEASURED[key] = [max(a, b) for a, b in zip(MEASURED[key], vals)]
    print(f"[bn] {key}: " + " ".join(f"{v:.2e}" for v in vals))
    b = _bound(key)
    b = b if isinstance(b, tuple) else (b,)
    assert all(v <= bb for v, bb in zip(vals, b)), (key, vals, b)


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[bn contract] wall time {time.perf_counter() - t0:.1f} s; measured maxima:")
    for k, v in sorted(MEASURED.items(), key=str):
        print(f"[bn]   {k}: " + " ".join(f"{x:.2e}" for x in v))


# ------------------------------------------------------------------------------------------------------------------ inputs
def _data(M, C, regime, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = 0.5 + 1.5 * torch.rand(C, device="cuda", generator=g)
    sign = torch.where(torch.rand(C, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    ratio = {"ratio30": 30.0, "ratio300": 300.0}.get(regime, 1.0)
    mu = sign * sd * ratio * (0.5 + 0.5 * torch.rand(C, device="cuda", generator=g))
    x = mu + sd * torch.randn(M, C, device="cuda", generator=g)
    if regime == "const":
        x[:, ::max(C // 8, 1)] = torch.linspace(-2.5, 2.5, len(range(0, C, max(C // 8, 1))), device="cuda")
    if regime == "relu0":
        x = (x - mu).clamp_min(0)
    return x.to(dt)


def _randn(*shape, seed):
    return torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _params(C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    gamma = 1 + 0.3 * torch.randn(C, device="cuda", generator=g)
    beta = 0.3 * torch.randn(C, device="cuda", generator=g)
    rm = 0.2 * torch.randn(C, device="cuda", generator=g)
    rv = 0.5 + torch.rand(C, device="cuda", generator=g)
    return gamma, beta, rm, rv


def _fam(dt):
    return "f32" if dt == F32 else "bf16"


def _stat_errors(mean, rstd, ref):
    sd = ref["var"].sqrt().clamp_min(EPS ** 0.5)
    em = float(((mean.double() - ref["mean"]).abs() / sd).max())
    er = float((rstd.double() / ref["rstd"] - 1).abs().max())
    return em, er


def _running_errors(rm, rv, ref):
    sd = ref["var"].sqrt().clamp_min(EPS ** 0.5).max(0).values
    return float(((rm.double() - ref["running_mean"]).abs() / sd).max()), float((rv.double() / ref["running_var"] - 1).abs().max())


def _kind(regime):
    """bound classes: the regimes whose errors differ in kind ("normal" and "relu0" share one)"""
    return regime if regime in ("ratio30", "ratio300", "const") else "ord"


# ------------------------------------------------------------------------------------------------------------------ shapes
# (name, M, C, groups, unit)
SHAPES = [
    ("m37", 37, 64, 1, 0),
    ("c48", 4 * 6 * 5, 48, 4, 0),
    ("c128", 16 * 32 * 32, 128, 4, 1024),
    ("aspp", 48 * 32 * 32, 256, 24, 1024),
    ("layer1", 8 * 128 * 160, 64, 4, 128 * 160),
    ("stem", 4 * 256 * 320, 64, 1, 0),
]
SMALL = SHAPES[:3]


# ------------------------------------------------------------------------------------------------------------------ forward statistics
# every regime at the small shapes, the production shapes with the three regimes whose errors grow with the rows
FWD_CASES = [(s, r) for s in SHAPES for r in REGIMES if s in SMALL or r in ("normal", "ratio30", "ratio300")]


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,regime", FWD_CASES, ids=[f"{s[0]}-{r}" for s, r in FWD_CASES])
def test_colstats_finalize_apply(dt, shape, regime):
    """colstats -> bn_finalize (pivot) -> bn_apply (residual + ReLU), and bn_finalize from raw sums (raw=True): mean, rstd, running
    statistics and y."""
    name, M, C, G, unit = shape
    seed = M + C + len(regime)
    x = _data(M, C, regime, dt, seed)
    gamma, beta, rm0, rv0 = _params(C, seed)
    resid = _randn(M, C, seed=seed + 2).to(dt)
    ref = R.forward(x, gamma, beta, groups=G, unit=unit, resid=resid, relu=True, running_mean=rm0, running_var=rv0)
    rm, rv = rm0.clone(), rv0.clone()
    s, ss = hip.colstats(x, groups=G, unit=unit)
    mean, rstd = hip.bn_finalize(x, s, ss, rm, rv, G, EPS, MOM, unit=unit)
    fam, kind = _fam(dt), _kind(regime)
    _check(("finalize", fam, kind), *_stat_errors(mean, rstd, ref), *_running_errors(rm, rv, ref))
    y = torch.empty_like(x)
    hip.bn_apply(x, mean, rstd, gamma, beta, y, resid=resid, groups=G, relu=True, unit=unit)
    # y against the reference evaluated with the kernel's statistics: the apply arithmetic alone
    idx = R.group_rows(M, G, unit, x.device)
    z = (x.double()[idx] - mean.double().unsqueeze(1)) * (rstd.double() * gamma.double()).unsqueeze(1) + beta.double()
    want = torch.empty(M, C, dtype=F64, device="cuda")
    want[idx.reshape(-1)] = z.reshape(-1, C)
    want = (want + resid.double()).clamp_min(0)
    _check(("apply", fam), *R.errors(y, want))
    # raw sums (a GEMM epilogue's form): float64 plain sums rounded to fp32
    xs = x.double()[idx]
    rm2, rv2 = rm0.clone(), rv0.clone()
    mean2, rstd2 = hip.bn_finalize(x, xs.sum(1).float(), (xs * xs).sum(1).float(), rm2, rv2, G, EPS, MOM, unit=unit, raw=True)
    _check(("finalize_raw", fam, kind), *_stat_errors(mean2, rstd2, ref), *_running_errors(rm2, rv2, ref))
    if regime == "const":                                 # var 0: rstd = eps^-1/2 (to fp32 rounding), y = relu(beta + resid)
        c0 = torch.arange(0, C, max(C // 8, 1), device="cuda")
        assert float((rstd[:, c0].double() * EPS ** 0.5 - 1).abs().max()) < 1e-6


def _block_table(y, nbk):
    """[2][nbk][N] fp32 table of per-128-row-block sums / sums of squares (float64, rounded once) - what gemm_nt(stats_out=) writes"""
    M, N = y.shape
    yd = torch.zeros(nbk * 128, N, dtype=F64, device=y.device)
    yd[:M] = y.double()
    b = yd.view(nbk, 128, N)
    return torch.stack([b.sum(1), (b * b).sum(1)]).float().contiguous()


TABLE_SHAPES = [("t256", 256 * 4, 64, 4, 0), ("t_il", 16 * 32 * 32, 128, 4, 1024), ("aspp24", 48 * 32 * 32, 256, 24, 1024),
                ("t_c48", 512 * 3, 48, 3, 0)]


TABLE_CASES = [(s, r, True) for s in TABLE_SHAPES for r in REGIMES] + [(s, "normal", False) for s in TABLE_SHAPES]


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,regime,running", TABLE_CASES,
                         ids=[f"{s[0]}-{r}-{'running' if run else 'norun'}" for s, r, run in TABLE_CASES])
def test_table_finalize_from_host_block_sums(dt, shape, regime, running):
    """bn_table_finalize (one launch up to 8 groups; the per-group kernel + bn_running_update above) and cs_group_reduce ->
    bn_finalize(raw=True), from a table of float64 128-row block sums rounded to fp32."""
    name, M, C, G, unit = shape
    seed = M + C + 7 * len(regime)
    x = _data(M, C, regime, dt, seed)
    gamma, beta, rm0, rv0 = _params(C, seed)
    ref = R.forward(x, gamma, beta, groups=G, unit=unit, relu=False, running_mean=rm0, running_var=rv0)
    tab = _block_table(x, 2 * ((M + 255) // 256))
    rm, rv = (rm0.clone(), rv0.clone()) if running else (None, None)
    mean, rstd = hip.bn_table_finalize(tab, M, rm, rv, G, EPS, MOM, unit=unit)
    fam, kind = _fam(dt), _kind(regime)
    errs = _stat_errors(mean, rstd, ref)
    if running:
        errs = errs + _running_errors(rm, rv, ref)
        _check(("table", kind), *errs)
    else:
        _check(("table", kind), *errs, 0.0, 0.0)
    s, ss = hip.cs_group_reduce(tab, M, G, unit)
    idx = R.group_rows(M, G, unit, x.device)
    xs = x.double()[idx]
    es = float(((s.double() - xs.sum(1)).abs() / xs.abs().sum(1).clamp_min(1e-30)).max())
    _check(("cs_group_reduce",), es)
    rm2, rv2 = rm0.clone(), rv0.clone()
    mean2, rstd2 = hip.bn_finalize(x, s, ss, rm2, rv2, G, EPS, MOM, unit=unit, raw=True)
    _check(("finalize_raw", fam, kind), *_stat_errors(mean2, rstd2, ref), *_running_errors(rm2, rv2, ref))


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,K,G,unit", [(4 * 1024, 64, 192, 4, 0), (16 * 1024, 256, 256, 8, 1024),
                                          (24 * 1024, 128, 128, 24, 1024)])
def test_table_finalize_from_a_real_gemm_epilogue(dt, M, N, K, G, unit):
    """One gemm_nt(stats_out=) launch: the statistics of its output from the epilogue table (bn_table_finalize, and
    cs_group_reduce -> bn_finalize raw) against the float64 statistics of the stored output."""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    A = (torch.randn(M, K, device="cuda", generator=g) + 0.3).to(dt)
    B = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(dt)
    out = torch.empty(M, N, dtype=dt, device="cuda")
    tab = hip.stats_table(M, N, "cuda")
    hip.gemm_nt(A, B, out, M=M, stats_out=tab)
    gamma, beta, rm0, rv0 = _params(N, M)
    # statistics of the fp32 accumulators (what the table sums) against those of the rounded output: the rounding of `out`
    ref = R.forward(out, gamma, beta, groups=G, unit=unit, relu=False, running_mean=rm0, running_var=rv0)
    rm, rv = rm0.clone(), rv0.clone()
    mean, rstd = hip.bn_table_finalize(tab, M, rm, rv, G, EPS, MOM, unit=unit)
    _check(("gemm_table", _fam(dt)), *_stat_errors(mean, rstd, ref), *_running_errors(rm, rv, ref))
    s, ss = hip.cs_group_reduce(tab, M, G, unit)
    mean2, rstd2 = hip.bn_finalize(out, s, ss, None, None, G, EPS, MOM, unit=unit, raw=True)
    _check(("gemm_table", _fam(dt)), *_stat_errors(mean2, rstd2, ref), 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------------ backward
BWD_SHAPES = [("m37", 37, 64, 1, 0), ("c48", 4 * 6 * 5, 48, 4, 0), ("c128", 16 * 32 * 32, 128, 4, 1024),
              ("aspp", 48 * 32 * 32, 256, 24, 1024), ("stem", 4 * 256 * 320, 64, 1, 0)]


def _bn_fwd(x, gamma, beta, G, unit, resid=None):
    s, ss = hip.colstats(x, groups=G, unit=unit)
    mean, rstd = hip.bn_finalize(x, s, ss, None, None, G, EPS, MOM, unit=unit)
    y = torch.empty_like(x)
    hip.bn_apply(x, mean, rstd, gamma, beta, y, resid=resid, groups=G, relu=True, unit=unit)
    return mean, rstd, y


MODES = [(True, True), (True, False), (False, False)]        # (training, residual)
BWD_CASES = [(s, r, m) for s in BWD_SHAPES for r in ("normal", "ratio300", "relu0") for m in MODES
             if s[0] not in ("aspp", "stem") or (r == "normal" and m[0])]


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,regime,mode", BWD_CASES,
                         ids=[f"{s[0]}-{r}-{'train' if m[0] else 'eval'}{'_res' if m[1] else ''}" for s, r, m in BWD_CASES])
def test_bn_bwd(dt, shape, regime, mode):
    """bn_bwd phase 0 against phases 1 + 2 (bitwise), against the float64 backward (dx, dresid, s1 / s2, group_sums), with the ReLU
    mask from the stored y (residual) or recomputed from x (y = None, beta)."""
    name, M, C, G, unit = shape
    training, res = mode
    seed = M + C + len(regime) + 3 * training + res
    x = _data(M, C, regime, dt, seed)
    gamma, beta, rm0, rv0 = _params(C, seed)
    resid = _randn(M, C, seed=seed + 2).to(dt) if res else None
    if training:
        mean, rstd, y = _bn_fwd(x, gamma, beta, G, unit, resid)
    else:
        mean = rm0.view(1, C).expand(G, C).contiguous()
        rstd = torch.rsqrt(rv0 + EPS).view(1, C).expand(G, C).contiguous()
        y = torch.empty_like(x)
        hip.bn_apply(x, mean, rstd, gamma, beta, y, resid=resid, groups=G, relu=True, unit=unit)
    dy = _randn(M, C, seed=seed + 5).to(dt)
    yk = y if res else None
    dx = torch.empty_like(x)
    dres = torch.empty_like(x)
    gs = torch.empty(2, C, dtype=F32, device="cuda")
    s1, s2 = hip.bn_bwd(dy, x, yk, mean, rstd, gamma, dx, dres, G, True, training, beta=beta, unit=unit, group_sums=gs)
    # phases 1 + 2: the same bits
    dx2, dres2 = torch.empty_like(x), torch.empty_like(x)
    t1, t2 = hip.bn_bwd(dy, x, yk, mean, rstd, gamma, dx2, dres2, G, True, training, phase=1, beta=beta, unit=unit)
    hip.bn_bwd(dy, x, yk, mean, rstd, gamma, dx2, dres2, G, True, training, phase=2, sums=(t1, t2), beta=beta, unit=unit)
    assert torch.equal(dx, dx2) and torch.equal(dres, dres2) and torch.equal(s1, t1) and torch.equal(s2, t2)
    mask = y > 0
    ref = R.backward(dy, x, mean, rstd, gamma, groups=G, unit=unit, mask=mask, training=training)
    fam = _fam(dt)
    _check(("dx", fam, "train" if training else "eval", _kind(regime)), *R.errors(dx, ref["dx"]))
    assert torch.equal(dres.double(), ref["dresid"])
    _check(("s", fam), *R.errors(torch.stack([s1, s2]), torch.stack([ref["s1"], ref["s2"]])))
    _check(("s", fam), *R.errors(gs, ref["group_sums"]))


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,C,G,unit", [(37, 64, 1, 0), (4 * 6 * 5, 48, 4, 0), (16 * 32 * 32, 128, 4, 1024), (4 * 256 * 320, 64, 1, 0)])
def test_bn_bwd_relu_mask_from_y_equals_mask_from_x(dt, M, C, G, unit):
    """y stored vs y = None (mask recomputed from x, mean, rstd, gamma, beta): bitwise the same dx / s1 / s2, with many outputs exactly
    0 (channels with beta = 0 whose x equals the given mean: x * (rstd gamma) + (0 - mean * rstd gamma) = 0 exactly)."""
    seed = M + C
    x = _data(M, C, "normal", dt, seed)
    gamma, beta, _, _ = _params(C, seed)
    mean = _randn(G, C, seed=seed + 3).to(dt).float()
    rstd = 0.5 + _randn(G, C, seed=seed + 4).abs()
    zc = torch.arange(0, C, 3, device="cuda")
    beta[zc] = 0.0
    idx = R.group_rows(M, G, unit, x.device)
    rows = idx[:, ::2]                                        # half of each group's rows: x = the group's mean
    xv = x.view(M, C)
    for g in range(G):
        xv[rows[g].unsqueeze(1), zc.unsqueeze(0)] = mean[g, zc].to(dt)
    y = torch.empty_like(x)
    hip.bn_apply(x, mean, rstd, gamma, beta, y, resid=None, groups=G, relu=True, unit=unit)
    zero = (y == 0)
    assert int(zero[:, zc].sum()) >= rows.numel() * zc.numel()
    dy = _randn(M, C, seed=seed + 5).to(dt)
    outs = []
    for yy in (y, None):
        dx = torch.empty_like(x)
        s1, s2 = hip.bn_bwd(dy, x, yy, mean, rstd, gamma, dx, None, G, True, True, beta=beta, unit=unit)
        outs.append((dx, s1, s2))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0].float()).all())


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,C,G", [(2 * 37, 64, 1), (2 * 4 * 1024, 128, 4), (2 * 4 * 256 * 320 // 2, 64, 1)])
def test_bn_bwd_rows_total_two_ranks(dt, M, C, G):
    """SyncBatchNorm by hand: two ranks hold a half of every group each; global statistics; phase 1 on each rank, s1 / s2 all-reduced
    (summed), phase 2 with rows_total = the global group rows: every rank's dx is its rows of the whole batch's gradient."""
    seed = M + C
    x = _data(M, C, "normal", dt, seed)
    gamma, beta, _, _ = _params(C, seed)
    dy = _randn(M, C, seed=seed + 5).to(dt)
    ref_f = R.forward(x, gamma, beta, groups=G, relu=True)
    mean, rstd = ref_f["mean"].float(), ref_f["rstd"].float()
    # rank r holds rows [g][r * n/2 : (r+1) * n/2] of every group g (contiguous groups per rank)
    idx = R.group_rows(M, G, 0, x.device)
    n = M // G
    parts = [idx[:, r * n // 2:(r + 1) * n // 2].reshape(-1) for r in range(2)]
    loc = []
    for p in parts:
        xr, dyr = x[p].contiguous(), dy[p].contiguous()
        y = torch.empty_like(xr)
        hip.bn_apply(xr, mean, rstd, gamma, beta, y, resid=None, groups=G, relu=True)
        loc.append((xr, dyr, y, hip.bn_bwd(dyr, xr, None, mean, rstd, gamma, torch.empty_like(xr), None, G, True, True, phase=1,
                                           beta=beta)))
    s1 = loc[0][3][0] + loc[1][3][0]
    s2 = loc[0][3][1] + loc[1][3][1]
    mask = torch.empty(M, C, dtype=torch.bool, device="cuda")
    dx = torch.empty(M, C, dtype=dt, device="cuda")
    for p, (xr, dyr, y, _) in zip(parts, loc):
        dxr = torch.empty_like(xr)
        hip.bn_bwd(dyr, xr, None, mean, rstd, gamma, dxr, None, G, True, True, phase=2, sums=(s1, s2), rows_total=n, beta=beta)
        dx[p] = dxr
        mask[p] = y > 0
    ref = R.backward(dy, x, mean, rstd, gamma, groups=G, mask=mask, training=True)
    _check(("dx_ranks", _fam(dt)), *R.errors(dx, ref["dx"]))


# ------------------------------------------------------------------------------------------------------------------ bn_relu_pool
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("frames,H,W,G,unit_frames", [(3, 17, 13, 1, 0), (4, 16, 24, 4, 0), (8, 32, 16, 4, 1), (4, 256, 320, 1, 0)])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_relu_pool_forward_and_backward(dt, frames, H, W, G, unit_frames, training):
    """bn_relu_pool (BatchNorm + ReLU + MaxPool2d(3, 2, 1)) against the reference followed by a float64 max pool, and its backward
    (max-pool scatter through the kernel's taps, then bn_bwd(group_sums=) with the mask recomputed from x) against the float64 one."""
    C = 64
    M = frames * H * W
    unit = unit_frames * H * W
    seed = M + G + training
    x = _data(M, C, "normal", dt, seed)
    gamma, beta, rm0, rv0 = _params(C, seed)
    if training:
        s, ss = hip.colstats(x, groups=G, unit=unit)
        mean, rstd = hip.bn_finalize(x, s, ss, None, None, G, EPS, MOM, unit=unit)
    else:
        mean = rm0.view(1, C).expand(G, C).contiguous()
        rstd = torch.rsqrt(rv0 + EPS).view(1, C).expand(G, C).contiguous()
    out, arg = hip.bn_relu_pool(x, mean, rstd, gamma, beta, frames, H, W, groups=G, unit=unit)
    idx = R.group_rows(M, G, unit, x.device)
    z = torch.empty(M, C, dtype=F64, device="cuda")
    z[idx.reshape(-1)] = ((x.double()[idx] - mean.double().unsqueeze(1)) * (rstd.double() * gamma.double()).unsqueeze(1)
                          + beta.double()).reshape(-1, C)
    want = R.maxpool3x3s2(z.clamp_min(0), frames, H, W)
    fam = _fam(dt)
    _check(("pool", fam), *R.errors(out, want))
    assert int(arg.max()) <= 8
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dout = _randn(frames * Hp * Wp, C, seed=seed + 6).to(dt)
    dz = torch.empty_like(x)
    hip.maxpool3x3s2(dout, dz, arg, frames, H, W, Hp, Wp, backward=True)
    dx = torch.empty_like(x)
    gs = torch.empty(2, C, dtype=F32, device="cuda")
    hip.bn_bwd(dz, x, None, mean, rstd, gamma, dx, None, G, True, training, beta=beta, unit=unit, group_sums=gs)
    pm = rstd * gamma                                          # the kernel's own fp32 mask expression (selection, given)
    xg = x.float()[idx]
    mk = torch.empty(M, C, dtype=torch.bool, device="cuda")
    mk[idx.reshape(-1)] = (xg * pm.unsqueeze(1) + (beta - mean * pm).unsqueeze(1) > 0).reshape(-1, C)
    dz_ref = R.maxpool3x3s2_bwd(dout, arg, frames, H, W)
    ref = R.backward(dz_ref, x, mean, rstd, gamma, groups=G, unit=unit, mask=mk, training=training)
    _check(("pool_dx", fam), *R.errors(dx, ref["dx"]))
    _check(("pool_gs", fam), *R.errors(gs, ref["group_sums"]))
