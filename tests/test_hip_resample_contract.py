"""The kernels that move the decode head between resolutions (stswincl_amd/csrc/headops.hip: bilinear forward and gather-form
backward, logits_upsample forward and backward, rows_broadcast, the sum-only colstats<T, false>; rowops.hip: the stand-alone
maxpool3x3s2 forward) against the float64 reference of tests/resample_ref.py, called through the raw hip.* entry points, fp32 and bf16.

Every case compares every element with the reference evaluated on the operands the kernel reads (the stored fp32 / bf16 values
widened to float64) and prints its measured errors.  Metrics:
  fwd / bwd / bcast / pool_bwd   (max, l2) as tests/bn_ref.py: largest error over the largest reference value, relative L2 norm;
  sums                           max over the columns of |sum - ref| / sum |x| of the column.
Exact, without a tolerance: the identity resize (bit-equal, forward and backward), max-pool values and first-maximum taps, every
sentinel (columns outside a column slice, pad columns >= nc of the logit tokens, the words behind a dense destination) and the
bitwise repeat of the pooled sums.

Shapes are the smallest at which each kernel can still go wrong: one pack (C = 8 bf16 / 4 fp32), six packs (48), 64; one and three
frames; everything-clamped 1 x 1 sources, non-dyadic and near-1 ratios, the production x2 and x8, a down-sampling ratio; element
counts far from a multiple of 256 (1 x 1 -> 4 x 6 with one pack: 24 threads of one block) and several blocks; source and destination
as C-wide column slices at offset 48 of 448-wide buffers (the decode concat).  The backward windows are checked on a random g and on g
that is non-zero in one output row, one output column and the four corners only: there a window one pixel short loses a whole term;
and, fp32 only, on a sweep of every ratio a -> b with 1 <= a, b <= 20.

Bounds: at most 2x the error measured on MI355X for the kernel, dtype and regime (table BOUND).  What explains the measured values:
an fp32 bilinear result is a four-term convex combination whose coordinate error is ~n_out x 2^-23; a bf16 result adds one rounding
of the stored value (half an ulp: up to 2^-8 of the value, 2^-9 on average).
"""
import time

import pytest
import torch

import resample_ref as R
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PITCH, OFFSET = 448, 48                   # the decode concat: a C-wide slice at column 48 of a 448-wide buffer
SENTINEL = -24576.0                       # exact in bf16; large enough to wreck any result that reads it

# Bounds per key of _check: 1.8 x the largest error measured on MI355X over the key's cases, rounded up to two digits (<= 2x).
# Measured (max, l2), fp32 | bf16:
#   bilinear_fwd 1.02e-6, 6.62e-7 | 3.07e-3, 1.67e-3     bilinear_bwd 1.10e-6, 1.18e-6 | 3.74e-3, 2.90e-3
#   logits_fwd   7.11e-7, 2.93e-7 | 3.49e-3, 1.68e-3     logits_bwd   4.80e-7, 5.23e-7 | 3.46e-3, 2.28e-3
#   bcast        5.47e-8, 3.03e-8 | 3.37e-3, 2.23e-3     bcast_acc    5.13e-8, 3.84e-8 | 3.55e-3, 2.07e-3
#   pool_bwd     1.04e-7, 2.65e-8 | 3.72e-3, 1.57e-3
#   the sweep over every ratio a -> b up to 20, fp32: bilinear_bwd 2.23e-6, 1.21e-6; logits_bwd 1.86e-6, 1.27e-6 (coordinates up to
#   20 times a rounded ratio: ~20 x 2^-23 = 2.4e-6)
#   sums: fp32 2.46e-7 (normal), 2.87e-7 (ratio300); bf16 1.71e-7 (normal), 0 (ratio300)
# fp32 bilinear: the largest values come from 13 x 9 -> 5 x 7, 5 x 7 -> 13 x 9 and 4 x 5 -> 30 x 37, whose ratios are rounded to fp32
# before they multiply the coordinate: the fp32 source coordinate is off by up to 5.7e-7 / 2.7e-7 / 4.1e-7 there (computed on the
# host, ~n x 2^-23), per axis, times the difference of two neighbours over the largest value (~1); dyadic ratios give exact
# coordinates and stay at 1e-7.  bf16: one rounding of the stored result, at most 2^-8 = 3.9e-3 of the
# largest value (the l2 of a backward on a g with four non-zero pixels is the rounding of a handful of values, hence above 2^-9).
# Sums relative to sum |x|: a few fp32 roundings of partial sums in any order.  bf16 x at |mean| / std ~ 300 are multiples of 0.5 ... 4
# below 1024; their sums over 4100 rows stay below 2^24 units, so every fp32 partial sum is exact in ANY order: the bound is 0.
BOUND = {
    ('bcast', 'bf16'): (6.1e-03, 4.1e-03),
    ('bcast', 'f32'): (9.9e-08, 5.5e-08),
    ('bcast_acc', 'bf16'): (6.4e-03, 3.8e-03),
    ('bcast_acc', 'f32'): (9.3e-08, 7.0e-08),
    ('bilinear_bwd', 'bf16'): (6.8e-03, 5.3e-03),
    ('bilinear_bwd', 'f32'): (2.0e-06, 2.2e-06),
    ('bilinear_bwd_sweep', 'f32'): (4.1e-06, 2.2e-06),
    ('bilinear_fwd', 'bf16'): (5.6e-03, 3.1e-03),
    ('bilinear_fwd', 'f32'): (1.9e-06, 1.2e-06),
    ('logits_bwd', 'bf16'): (6.3e-03, 4.2e-03),
    ('logits_bwd', 'f32'): (8.7e-07, 9.5e-07),
    ('logits_bwd_sweep', 'f32'): (3.4e-06, 2.3e-06),
    ('logits_fwd', 'bf16'): (6.3e-03, 3.1e-03),
    ('logits_fwd', 'f32'): (1.3e-06, 5.3e-07),
    ('pool_bwd', 'bf16'): (6.7e-03, 2.9e-03),
    ('pool_bwd', 'f32'): (1.9e-07, 4.8e-08),
    ('sums', 'bf16', 'normal'): (3.1e-07,),
    ('sums', 'bf16', 'ratio300'): (0.0,),
    ('sums', 'f32', 'normal'): (4.5e-07,),
    ('sums', 'f32', 'ratio300'): (5.2e-07,),
}
MEASURED = {}


def _bound(key):
    return BOUND[key]


def _check(key, *vals):
    """record the measured errors of `key` and hold them to BOUND[key] (same arity)"""
    MEASURED.setdefault(key, [0.0] * len(vals))
    MEASURED[key] = [max(a, b) for a, b in zip(MEASURED[key], vals)]
    print(f"[resample] {key}: " + " ".join(f"{v:.2e}" for v in vals))
    b = _bound(key)
    b = b if isinstance(b, tuple) else (b,)
    assert len(b) == len(vals) and all(v <= bb for v, bb in zip(vals, b)), (key, vals, b)


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[resample contract] wall time {time.perf_counter() - t0:.1f} s; measured maxima:")
    for k, v in sorted(MEASURED.items(), key=str):
        print(f"[resample]   {k}: " + " ".join(f"{x:.2e}" for x in v))


# ------------------------------------------------------------------------------------------------------------------ helpers
def _fam(dt):
    return "f32" if dt == F32 else "bf16"


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(rows, cols, dt, seed):
    return torch.randn(rows, cols, device="cuda", generator=_gen(seed)).to(dt)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _widths(dt):
    """one pack, six packs of bf16 (twelve of fp32), 64"""
    return [4 if dt == F32 else 8, 48, 64]


class Slot:
    """A [rows][C] matrix for a kernel to read or write: dense (with SENTINEL words behind its end), or columns OFFSET .. OFFSET + C
    of a [rows][PITCH] buffer filled with SENTINEL.  unchanged() tells whether every word outside the matrix still holds its bits."""

    def __init__(self, rows, C, dt, pitched, data=None):
        self.rows, self.C, self.pitched = rows, C, pitched
        if pitched:
            self.buf = torch.full((rows, PITCH), SENTINEL, dtype=dt, device="cuda")
            self.t = self.buf[:, OFFSET:OFFSET + C]
        else:
            self.buf = torch.full((rows * C + 64,), SENTINEL, dtype=dt, device="cuda")
            self.t = self.buf[:rows * C].view(rows, C)
        if data is not None:
            self.t.copy_(data)
        self.before = self.buf.clone()

    def unchanged(self, whole=False):
        a, b = _bits(self.buf), _bits(self.before)
        if whole:
            return torch.equal(a, b)
        if self.pitched:
            return torch.equal(a[:, :OFFSET], b[:, :OFFSET]) and torch.equal(a[:, OFFSET + self.C:], b[:, OFFSET + self.C:])
        return torch.equal(a[self.rows * self.C:], b[self.rows * self.C:])


# ------------------------------------------------------------------------------------------------------------------ bilinear
def _structured(kind, F_, H, W, C, dt, seed):
    """g [F*H*W][C]: random, or random values in one output row / one output column / the four corners and zero elsewhere"""
    g = _randn(F_ * H * W, C, dt, seed)
    if kind == "random":
        return g
    keep = torch.zeros(F_, H, W, 1, dtype=torch.bool, device="cuda")
    if kind == "row":
        keep[:, (seed * 7) % H] = True
    elif kind == "col":
        keep[:, :, (seed * 5) % W] = True
    elif kind == "last":                                  # the last output row and column: the far edge of every window
        keep[:, H - 1] = True
        keep[:, :, W - 1] = True
    else:
        for y in (0, H - 1):
            for x in (0, W - 1):
                keep[:, y, x] = True
    return torch.where(keep.expand(F_, H, W, C).reshape(F_ * H * W, C), g, torch.zeros((), dtype=dt, device="cuda"))


G_KINDS = ["random", "row", "col", "last", "corners"]
BIL_CASES = [(g, f) for g in R.BILINEAR_GEOMS for f in R.FRAMES]


@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom,frames", BIL_CASES, ids=[f"{g[0]}x{g[1]}-{g[2]}x{g[3]}-f{f}" for g, f in BIL_CASES])
def test_bilinear_forward_and_backward(geom, frames, dt, pitched):
    """stswin_bilinear, both directions, every width: all elements against the reference; nothing outside the destination written,
    the source left as it was; the identity resize bit-equal."""
    h, w, H, W = geom
    fam = _fam(dt)
    for C in _widths(dt):
        seed = 1000 * h + 100 * w + 10 * H + W + C + frames
        src = Slot(frames * h * w, C, dt, pitched, _randn(frames * h * w, C, dt, seed))
        dst = Slot(frames * H * W, C, dt, pitched)
        hip.bilinear(src.t, dst.t, frames, h, w, H, W)
        assert dst.unchanged(), "forward wrote outside its destination"
        assert src.unchanged(whole=True), "forward wrote to its source"
        ref = R.bilinear_fwd(src.t, frames, h, w, H, W)
        if (h, w) == (H, W):
            assert torch.equal(_bits(dst.t.contiguous()), _bits(src.t.contiguous())), "identity resize is not bit-equal"
        _check(("bilinear_fwd", fam), *R.errors(dst.t, ref))
        for kind in G_KINDS:
            g = Slot(frames * H * W, C, dt, pitched, _structured(kind, frames, H, W, C, dt, seed + len(kind)))
            dx = Slot(frames * h * w, C, dt, pitched)
            hip.bilinear(g.t, dx.t, frames, h, w, H, W, backward=True)
            assert dx.unchanged(), "backward wrote outside its destination"
            assert g.unchanged(whole=True), "backward wrote to its source"
            if (h, w) == (H, W):
                assert torch.equal(_bits(dx.t.contiguous()), _bits(g.t.contiguous())), "identity backward is not bit-equal"
            _check(("bilinear_bwd", fam), *R.errors(dx.t, R.bilinear_bwd(g.t, frames, h, w, H, W)))


SWEEP = range(1, 21)


@pytest.mark.parametrize("kernel", ["bilinear", "logits"])
def test_backward_windows_over_every_ratio_up_to_20(kernel):
    """The gather windows of both backward kernels at every ratio a -> b, 1 <= a, b <= 20, in both axes at once (a x b -> b x a):
    up- and down-sampling, dyadic or not, everything clamped (a = 1) and the identity.  fp32, one frame, a random g: a pixel missing
    from a window is a missing term of order 1, seven orders above the bound."""
    worst = [0.0, 0.0]
    for a in SWEEP:
        for b in SWEEP:
            h, w, H, W = a, b, b, a
            if kernel == "bilinear":
                g = _randn(H * W, 4, F32, 100 * a + b)
                dx = torch.empty(h * w, 4, dtype=F32, device="cuda")
                hip.bilinear(g, dx, 1, h, w, H, W, backward=True)
                ref = R.bilinear_bwd(g, 1, h, w, H, W)
            else:
                g = _randn(H * W, 3, F32, 100 * a + b).t().contiguous().view(1, 3, H, W)
                dx = torch.empty(h * w, 3, dtype=F32, device="cuda")
                hip.logits_upsample(dx, g, 1, h, w, H, W, 3, backward=True)
                ref = R.logits_up_bwd(g, 1, h, w, H, W)
            e = R.errors(dx, ref)
            worst = [max(x, y) for x, y in zip(worst, e)]
            assert e[0] <= _bound((kernel + "_bwd_sweep", "f32"))[0], (kernel, a, b, e)
    _check((kernel + "_bwd_sweep", "f32"), *worst)


# ------------------------------------------------------------------------------------------------------------------ logits_upsample
NCS = [1, 9, 12, 26]
LOG_CASES = [(g, f) for g in R.LOGITS_GEOMS for f in R.FRAMES]


@pytest.mark.parametrize("wide", [False, True], ids=["pitch_nc", "pitch64"])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom,frames", LOG_CASES, ids=[f"{g[0]}x{g[1]}-{g[2]}x{g[3]}-f{f}" for g, f in LOG_CASES])
def test_logits_upsample_forward_and_backward(geom, frames, dt, wide):
    """stswin_logits_upsample between tokens [F*h*w][pitch] (pitch = nc, or 64 with SENTINEL pad columns) and NCHW [F][nc][H][W]."""
    h, w, H, W = geom
    fam = _fam(dt)
    for nc in NCS:
        pitch = 64 if wide else nc
        seed = 100 * h + 10 * W + nc + frames
        rows = frames * h * w
        tok = torch.full((rows, pitch), SENTINEL, dtype=dt, device="cuda")
        tok[:, :nc] = _randn(rows, nc, dt, seed)
        tok0 = tok.clone()
        out = Slot(1, frames * nc * H * W, dt, False)
        nchw = out.t.view(frames, nc, H, W)
        hip.logits_upsample(tok, nchw, frames, h, w, H, W, nc)
        assert out.unchanged(), "forward wrote behind the NCHW tensor"
        assert torch.equal(_bits(tok), _bits(tok0)), "forward wrote to its source"
        _check(("logits_fwd", fam), *R.errors(nchw, R.logits_up_fwd(tok, frames, h, w, H, W, nc)))
        for kind in G_KINDS:
            g = _structured(kind, frames, H, W, nc, dt, seed + len(kind)).view(frames, H, W, nc).permute(0, 3, 1, 2).contiguous()
            g0 = g.clone()
            dtok = torch.full((rows, pitch), SENTINEL, dtype=dt, device="cuda")
            hip.logits_upsample(dtok, g, frames, h, w, H, W, nc, backward=True)
            assert torch.equal(_bits(g), _bits(g0)), "backward wrote to its source"
            if pitch > nc:
                assert bool((dtok[:, nc:] == SENTINEL).all()), "backward wrote a pad column"
            _check(("logits_bwd", fam), *R.errors(dtok[:, :nc], R.logits_up_bwd(g, frames, h, w, H, W)))


# ------------------------------------------------------------------------------------------------------------------ rows_broadcast
GROUP_ROWS = [1, 5, 37, 300]
SCALES = [1.0, 1.0 / 37.0]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_rows_broadcast(dt, groups, pitched, accumulate):
    """stswin_rows_broadcast: out[r] (+)= v[r // group_rows] * scale.  accumulate is a read-modify-write in the storage dtype: its
    reference is the float64 sum of the stored value and v * scale (the scale as the kernel gets it: rounded to fp32)."""
    fam = _fam(dt)
    for C in _widths(dt):
        for gr in GROUP_ROWS:
            for scale in SCALES:
                M = groups * gr
                seed = 10 * M + C + accumulate
                v = torch.randn(groups, C, device="cuda", generator=_gen(seed))
                out = Slot(M, C, dt, pitched, _randn(M, C, dt, seed + 1))
                base = out.t.clone()
                hip.rows_broadcast(v, out.t, groups, scale=scale, accumulate=accumulate)
                assert out.unchanged(), "wrote outside its destination"
                s32 = float(torch.tensor(scale, dtype=F32))
                ref = R.rows_broadcast(v, M, groups, s32, base=base if accumulate else None)
                if dt == F32 and not accumulate and scale == 1.0:
                    assert torch.equal(out.t, v.repeat_interleave(gr, dim=0)), "a copy is not exact"
                _check(("bcast_acc" if accumulate else "bcast", fam), *R.errors(out.t, ref))


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_rows_broadcast_first_m_rows_only(dt):
    """M < out.shape[0]: the rows behind M keep their bits"""
    v = torch.randn(3, 64, device="cuda", generator=_gen(5))
    out = torch.full((40, 64), SENTINEL, dtype=dt, device="cuda")
    hip.rows_broadcast(v, out, 3, M=33)
    assert bool((out[33:] == SENTINEL).all())
    _check(("bcast", _fam(dt)), *R.errors(out[:33], R.rows_broadcast(v, 33, 3, 1.0)))


# ------------------------------------------------------------------------------------------------------------------ pooled sums
def _data(M, C, regime, dt, seed):
    """as tests/test_hip_bn_contract.py: "normal" |mean| / std <= 1, "ratio300" |mean| / std ~ 300"""
    g = _gen(seed)
    sd = 0.5 + 1.5 * torch.rand(C, device="cuda", generator=g)
    sign = torch.where(torch.rand(C, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    ratio = {"ratio300": 300.0}.get(regime, 1.0)
    mu = sign * sd * ratio * (0.5 + 0.5 * torch.rand(C, device="cuda", generator=g))
    return (mu + sd * torch.randn(M, C, device="cuda", generator=g)).to(dt)


# (groups, rows per group, unit): contiguous groups, and one interleaved case (units of 64 rows, four per group)
SUM_CASES = [(G, gr, 0) for G in (1, 3) for gr in (1, 37, 1024, 4100)] + [(3, 256, 64)]


@pytest.mark.parametrize("regime", ["normal", "ratio300"])
@pytest.mark.parametrize("C", [48, 64, 256])
@pytest.mark.parametrize("groups,gr,unit", SUM_CASES, ids=[f"g{G}-r{gr}-u{u}" for G, gr, u in SUM_CASES])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_pooled_sums(dt, groups, gr, unit, C, regime):
    """hip.colstats(squares=False), the numerator of nn.AdaptiveAvgPool2d(1): plain fp32 sums without a pivot (colstats<T, false>),
    relative to the column's sum of |x|; the same bits on a second call."""
    M = groups * gr
    x = _data(M, C, regime, dt, M + C + len(regime))
    s, ss = hip.colstats(x, groups=groups, squares=False, unit=unit)
    s2, _ = hip.colstats(x, groups=groups, squares=False, unit=unit)
    assert ss is None and s.shape == (groups, C)
    assert torch.equal(_bits(s), _bits(s2)), "two calls on the same input differ"
    ref = R.group_sums(x, groups, unit)
    idx = R.group_rows(M, groups, unit, x.device)
    mag = x.double().abs()[idx.reshape(-1)].view(groups, gr, C).sum(1)
    _check(("sums", _fam(dt), regime), float(((s.double() - ref).abs() / mag.clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------------------------------------------ max pool
def _pool_input(kind, rows, C, dt, seed):
    x = _randn(rows, C, dt, seed)
    if kind == "relu":                                        # half the values exactly 0
        return x.clamp_min(0)
    if kind == "levels":                                      # four levels: almost every window has ties
        return (torch.randint(0, 4, (rows, C), device="cuda", generator=_gen(seed)).float() - 1.5).to(dt)
    return x


POOL_GEOMS = [(1, 1), (2, 2), (1, 9), (37, 53), (16, 16)]


def _pool_case(frames, H, W, C, dt, kind, pitched):
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    seed = 100 * H + W + C + frames + len(kind)
    src = Slot(frames * H * W, C, dt, pitched, _pool_input(kind, frames * H * W, C, dt, seed))
    dst = Slot(frames * Hp * Wp, C, dt, pitched)
    arg = torch.full((frames * Hp * Wp * C + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    a = arg[:frames * Hp * Wp * C].view(frames * Hp * Wp, C)
    hip.maxpool3x3s2(src.t, dst.t, a, frames, H, W, Hp, Wp)
    assert dst.unchanged() and src.unchanged(whole=True) and bool((arg[frames * Hp * Wp * C:] == 0xEE).all())
    assert torch.equal(dst.t.double(), R.maxpool3x3s2(src.t, frames, H, W)), "a pooled value is not the maximum of its window"
    assert torch.equal(a, R.maxpool3x3s2_taps(src.t, frames, H, W)), "a tap is not the first maximum in (ky, kx) order"
    dout = Slot(frames * Hp * Wp, C, dt, pitched, _randn(frames * Hp * Wp, C, dt, seed + 1))
    dz = Slot(frames * H * W, C, dt, pitched)
    hip.maxpool3x3s2(dout.t, dz.t, a, frames, H, W, Hp, Wp, backward=True)
    assert dz.unchanged() and dout.unchanged(whole=True)
    _check(("pool_bwd", _fam(dt)), *R.errors(dz.t, R.maxpool3x3s2_bwd(dout.t, a, frames, H, W)))


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("H,W", POOL_GEOMS, ids=[f"{H}x{W}" for H, W in POOL_GEOMS])
@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_maxpool_forward_values_and_taps(dt, H, W, frames, C):
    """stswin_maxpool3x3s2 forward (maxpool_fwd_kernel): values and taps exactly; the taps fed to the backward form reproduce the
    float64 scatter.  Random, post-ReLU and four-level inputs."""
    for kind in ("random", "relu", "levels"):
        _pool_case(frames, H, W, C, dt, kind, False)


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
def test_maxpool_column_slices(dt):
    """source and destination as column slices of 448-wide buffers"""
    _pool_case(3, 37, 53, 64, dt, "levels", True)
    _pool_case(1, 1, 9, 8, dt, "relu", True)
