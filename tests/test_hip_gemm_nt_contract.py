"""stswin_gemm_nt / stswin_gemm_nt_splitk (stswincl_amd/csrc/gemm.hip), every product kernel family, against the float64 contract of
tests/gemm_ref.py - per ELEMENT, with the derived bound of that module (nothing here is tuned on a GPU).

Every case asserts
  * which kernel ran (stswin_last_variant(0)): a case that lands in another family fails;
  * |got - ref| <= bound for every element of C, C2, the column sums and the statistics tables; a failure names the worst element
    with its tile-local position and the number of offenders; one line per case is printed with the largest err / bound;
  * nothing else was written: C, C2 and the fp32 C are views into larger buffers pre-filled with a finite sentinel (scratch: NaN) -
    the rows past M, the columns left and right of the slice and the rows c_rows does not name are bit-identical afterwards;
  * the inputs (A, B, R, bias, row maps) are bit-identical afterwards;
  * a second call gives the same bits (column sums through fp32 atomics excepted).

Column-sum tables: kernels whose workgroups split their rows in 128 (the register-epilogue ring, the 128-row tiles) fill one table row per
128 output rows; the 256x64 tiles and the ring's LDS epilogue put the sum of 256 rows into the even row and zero into the odd one
(include/stswin_hip.h, STSWIN_GF_CS_PARTIAL) - checked as such.  The library's tuning-only variants are out of scope: where
stswin_tuning_build() is 0 their flags are ignored, and none is used here."""
import pytest
import torch

import gemm_ref as G
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
F64 = torch.float64
SENT = 12345.0
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
V128 = (hip.VAR_NT_128x128, hip.VAR_NT_128x128_W4, hip.VAR_NT_128x64, hip.VAR_NT_RING256_REGEPI,
        hip.VAR_NT_128x128 + hip.VAR_F32, hip.VAR_NT_128x128_W4 + hip.VAR_F32)       # families with one table row per 128 output rows
NAMES = {hip.VAR_NT_ROWS: "rows", hip.VAR_NT_128x128: "128x128", hip.VAR_NT_128x128_W4: "128x128_w4", hip.VAR_NT_128x64: "128x64",
         hip.VAR_NT_256x64: "256x64", hip.VAR_NT_RING256_REGEPI: "ring256_regepi", hip.VAR_NT_RING256_LDSEPI: "ring256_ldsepi",
         hip.VAR_NT_SPLITK: "splitk", hip.VAR_NT_128x128 + hip.VAR_F32: "128x128_f32", hip.VAR_NT_128x128_W4 + hip.VAR_F32: "128x128_w4_f32",
         hip.VAR_NT_256x64 + hip.VAR_F32: "256x64_f32"}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def run_case(expect, M, N, Kseg, *, monkeypatch=None, **kw):
    """_run_case; colsum='atomic' forces the fp32-atomics form of the column sums for this case only (the wrapper's table threshold,
    monkeypatched as tests/test_hip_gemm.py does)."""
    if kw.get("colsum") == "atomic":
        with monkeypatch.context() as mp:
            mp.setattr(hip, "_CS_PARTIAL_MIN_M", 1 << 30)
            return _run_case(expect, M, N, Kseg, **kw)
    return _run_case(expect, M, N, Kseg, **kw)


def _run_case(expect, M, N, Kseg, *, S=1, dtype=BF, flags=0, mode="", bias=None, r=None, rmap=False, amap=None, cmap=False, scale_cols=0,
             scale=0.25, c2=False, colsum=None, stats=False, col0=0, seed=0, splits=None):
    """One gemm_nt problem from a seed, checked as the module docstring says.  bias: None | 'n' (unit normal) | 'wide' (spread over
    [-6, 6]: the GELU polynomial's clamp at |x| = 3.96 and its tails); r: None | 'n' | 'wide' (the R operand; the flags say what it is
    for); rmap / cmap: gather R rows / scatter C rows through a permutation into a taller buffer; amap: None | 'rand' (with -1 rows) |
    an int32 [S][M] map; colsum: None | 'table' | 'atomic'; col0: the outputs and R are column slices starting there."""
    dev = DEV
    g = torch.Generator().manual_seed(1000 * seed + M + N + Kseg + S)
    out_f32 = bool(flags & hip.GF_OUT_F32) or dtype == F32
    odt = F32 if out_f32 else dtype
    a_rows = None
    rows_a = M
    if isinstance(amap, str):
        rows_a = M + 37
        a_rows = torch.randint(-1, rows_a, (S, M), generator=g, dtype=torch.int32)
        a_rows[:, min(5, M - 1)] = -1
    elif amap is not None:
        a_rows = amap.cpu()
    A = torch.randn(rows_a, Kseg, generator=g).to(dtype)
    B = (torch.randn(N, S * Kseg, generator=g) / (S * Kseg) ** 0.5).to(dtype)
    bv = None
    if bias == "n":
        bv = torch.randn(N, generator=g)
    elif bias == "wide":
        bv = (torch.rand(N, generator=g) * 12.0 - 6.0)
    pitch = (col0 + N + 8 + 7) // 8 * 8
    rows_r = M + 50 if rmap else M
    Rfull = r_rows = None
    if r is not None:
        Rfull = torch.full((rows_r, pitch), SENT).to(dtype)
        Rfull[:, col0:col0 + N] = (torch.randn(rows_r, N, generator=g) if r == "n" else torch.rand(rows_r, N, generator=g) * 12.0 - 6.0).to(dtype)
        if rmap:
            r_rows = torch.randperm(rows_r, generator=g)[:M].to(torch.int32)
    rows_c = M + 45 if cmap else M
    c_rows = torch.randperm(rows_c, generator=g)[:M].to(torch.int32) if cmap else None
    orow = c_rows.long() if cmap else torch.arange(M)
    Cinit = torch.full((rows_c + 3, pitch), SENT).to(odt)
    c_prev = None
    if flags & hip.GF_ACCUM:
        c_prev = torch.randn(M, N, generator=g)
        Cinit[orow, col0:col0 + N] = c_prev
    C2init = torch.full((rows_c + 3, pitch), SENT).to(dtype) if c2 else None
    cs0 = torch.randn(N, generator=g) if colsum else None                  # (the ABI says +=: a non-zero accumulator)
    nb256 = (M + 255) // 256

    Ad, Bd = A.to(dev), B.to(dev)
    bd = bv.to(dev) if bv is not None else None
    Rd = Rfull.to(dev) if Rfull is not None else None
    ard = a_rows.to(dev) if a_rows is not None else None
    crd = c_rows.to(dev) if c_rows is not None else None
    rrd = r_rows.to(dev) if r_rows is not None else None

    def launch():
        Cb = Cinit.to(dev, copy=True)
        C2b = C2init.to(dev, copy=True) if c2 else None
        csd = cs0.to(dev, copy=True) if colsum else None
        tab = hip.stats_table(M, N, dev).fill_(float("nan")) if stats else None
        hip.scratch(dev, 1).fill_(float("nan"))            # column-sum table / split-K slabs: stale contents must not leak
        hip.gemm_nt(Ad, Bd, Cb[:rows_c, col0:col0 + N], M=M, a_rows=ard, c_rows=crd, bias=bd, resid=Rd[:, col0:col0 + N] if Rd is not None else None,
                    r_rows=rrd, out2=C2b[:rows_c, col0:col0 + N] if c2 else None, S=S, scale=scale if scale_cols else 1.0, scale_cols=scale_cols,
                    flags=flags, colsum_out=csd, stats_out=tab)
        v = hip.last_variant(0)
        return v, Cb.cpu(), C2b.cpu() if c2 else None, csd.cpu() if colsum else None, tab.cpu() if stats else None

    v, Cb, C2b, csd, tab = launch()
    what = f"{NAMES.get(expect, expect)} M={M} N={N} K={Kseg} S={S} {mode or 'plain'}"
    assert v["kernel"] == expect, f"{what}: ran {NAMES.get(v['kernel'], v['kernel'])}"
    if splits is not None:
        assert v["splits"] == splits, f"{what}: {v['splits']} splits, planned {splits}"

    # inputs untouched
    assert _same_bits(Ad.cpu(), A) and _same_bits(Bd.cpu(), B), f"{what}: an operand was written"
    assert bd is None or torch.equal(bd.cpu(), bv), f"{what}: bias was written"
    assert Rd is None or _same_bits(Rd.cpu(), Rfull), f"{what}: R was written"
    for d_, h_ in ((ard, a_rows), (crd, c_rows), (rrd, r_rows)):
        assert d_ is None or torch.equal(d_.cpu(), h_), f"{what}: a row map was written"

    # nothing but C[c_rows[m]][col0 : col0 + N] was written
    touched = torch.zeros(rows_c + 3, pitch, dtype=torch.bool)
    touched[orow, col0:col0 + N] = True
    for name, buf, init in (("C", Cb, Cinit), ("C2", C2b, C2init)):
        if buf is not None:
            stray = (_bits(buf) != _bits(init)) & ~touched
            assert not bool(stray.any()), (f"{what}: {int(stray.sum())} elements of {name} outside the result were written, first at "
                                           f"{tuple(int(x) for x in stray.nonzero()[0])} of a {tuple(buf.shape)} buffer, slice at column {col0}")

    ref = G.ref(A, B, M=M, S=S, a_rows=a_rows, bias=bv, scale=scale, scale_cols=scale_cols, R=Rfull[:, col0:col0 + N] if Rfull is not None else None,
                r_rows=r_rows, flags=flags, c_prev=c_prev)
    bnd = G.bound(ref, bf16=dtype == BF, out_f32=out_f32)
    line = [what]
    fails = []

    def check(name, got, want, b, tile=256):
        ratio, bad, where = G.worst(got, want, b, tile)
        line.append(f"{name} {ratio:.3f}")
        if bad:
            fails.append(f"{name}: {bad} of {got.numel()} elements beyond their bound, worst err / bound = {ratio:.3g} at {where}")

    check("C", Cb[orow, col0:col0 + N], ref["store"], bnd["store"])
    if c2:
        check("C2", C2b[orow, col0:col0 + N], ref["c2"], bnd["c2"])
    if colsum:
        bs, _ = G.sum_bound(ref["out"], bnd["out"], 0, prior=cs0)
        check("colsum", csd[None], cs0.to(F64)[None] + ref["out"].sum(0, keepdim=True), bs)
    if stats:
        blk = 128 if expect in V128 else 256
        bs, bq = G.sum_bound(ref["out"], bnd["out"], blk)
        want = torch.zeros(2, 2 * nb256, N, dtype=F64)
        wb = torch.zeros_like(want)
        step = blk // 128
        nb = bs.shape[0]
        want[0, 0:nb * step:step], want[1, 0:nb * step:step] = G.block_sums(ref["out"], blk), G.block_sums(ref["out"] ** 2, blk)
        wb[0, 0:nb * step:step], wb[1, 0:nb * step:step] = bs, bq
        check("sums", tab[0], want[0], wb[0])               # (rows without output rows: exactly zero, the odd last row included)
        check("squares", tab[1], want[1], wb[1])
    print("[gemm_nt] " + "  ".join(line))
    assert not fails, what + ": " + "; ".join(fails)

    # the same bits again
    v2, Cb2, C2b2, csd2, tab2 = launch()
    assert v2 == v
    assert _same_bits(Cb2, Cb), f"{what}: a second call gave other bits in C"
    assert C2b is None or _same_bits(C2b2, C2b), f"{what}: a second call gave other bits in C2"
    assert tab is None or _same_bits(tab2, tab), f"{what}: a second call gave another statistics table"
    if colsum == "table" and N % 4 == 0:
        assert _same_bits(csd2, csd), f"{what}: a second call gave other column sums"
    return v


RF, MR, MD = hip.GF_RESID, hip.GF_MUL_R, hip.GF_MUL_DGELU
GELU, RELU, C2D = hip.GF_GELU, hip.GF_RELU, hip.GF_C2_DGELU
O32, ACC = hip.GF_OUT_F32, hip.GF_ACCUM
BIG, NONARROW, DEEP, W4, NODEEP, NOREGEPI = hip.GF_BIG, hip.GF_NONARROW, hip.GF_DEEP, hip.GF_WAVES4, hip.GF_NODEEP, hip.GF_NOREGEPI


# ---------------------------------------------------------------------------------------------------- M <= 8: one wave per column
@pytest.mark.parametrize("K", [64, 576])          # 576: a second trip of the 512-wide k loop, for eight lanes only
@pytest.mark.parametrize("N", [64, 261])          # 261: not a multiple of the 4 columns of a workgroup
@pytest.mark.parametrize("M", [1, 8])
def test_rows_kernel(M, N, K):
    run_case(hip.VAR_NT_ROWS, M, N, K, seed=1)
    run_case(hip.VAR_NT_ROWS, M, N, K, bias="n", mode="bias", seed=2)
    run_case(hip.VAR_NT_ROWS, M, N, K, bias="n", flags=RELU, mode="bias relu", seed=3)


# ---------------------------------------------------------------------------------------------------- 128x128 tiles
def _epi_piece_cases(expect, M, N, K, base, monkeypatch, dtype=BF):
    """Every flag of epi_piece at least once on a tiled family."""
    kw = dict(dtype=dtype)
    run_case(expect, M, N, K, flags=base, seed=1, **kw)
    run_case(expect, M, N, K, flags=base, bias="n", mode="bias", seed=2, **kw)
    run_case(expect, M, N, K, flags=base | GELU, bias="wide", c2=True, mode="bias gelu c2", seed=3, **kw)
    run_case(expect, M, N, K, flags=base | GELU | C2D, bias="wide", c2=True, mode="bias gelu c2=gelu'", seed=4, **kw)
    run_case(expect, M, N, K, flags=base | RF, bias="n", r="n", rmap=True, cmap=True, mode="bias resid r_rows c_rows", seed=5, **kw)
    run_case(expect, M, N, K, flags=base | MR, r="n", colsum="table", mode="mul_r colsum", seed=6, **kw)
    run_case(expect, M, N, K, flags=base | MD, r="wide", colsum="atomic", monkeypatch=monkeypatch, mode="mul_dgelu colsum(atomic)", seed=7, **kw)
    run_case(expect, M, N, K, flags=base | RELU, bias="n", scale_cols=100, mode="bias scale100 relu", seed=8, **kw)
    run_case(expect, M, N, K, flags=base | O32, bias="n", mode="bias out_f32", seed=9, **kw)
    run_case(expect, M, N, K, flags=base | O32 | ACC, mode="out_f32 accum", seed=10, **kw)
    run_case(expect, M, N, K, flags=base, bias="n", stats=True, mode="bias stats", seed=11, **kw)


def test_tile_128x128_bf16_every_epilogue_flag(monkeypatch):
    _epi_piece_cases(hip.VAR_NT_128x128, 200, 136, 128, NONARROW, monkeypatch)


def test_tile_128x128_bf16_small_ragged_and_slices():
    E = hip.VAR_NT_128x128
    run_case(E, 37, 48, 192, seed=1)
    run_case(E, 37, 48, 192, bias="n", mode="bias", seed=2)
    run_case(E, 37, 48, 192, flags=RF, r="n", mode="resid", seed=3)
    run_case(E, 37, 48, 64, S=3, amap="rand", bias="n", mode="gather bias", seed=4)
    # C, C2 and R as slices that start 4 columns into a wider buffer: 8-byte, not 16-byte aligned
    run_case(E, 200, 136, 128, flags=NONARROW | GELU, bias="wide", c2=True, col0=4, mode="slice+4 bias gelu c2", seed=5)
    run_case(E, 200, 136, 128, flags=NONARROW | RF, bias="n", r="n", col0=4, mode="slice+4 bias resid", seed=6)


def test_tile_128x128_four_waves():
    E = hip.VAR_NT_128x128_W4
    run_case(E, 200, 136, 128, flags=W4, seed=1)
    run_case(E, 200, 136, 128, flags=W4, bias="n", mode="bias", seed=2)
    run_case(E, 200, 136, 128, flags=W4 | RF, bias="n", r="n", cmap=True, mode="bias resid c_rows", seed=3)
    run_case(E, 37, 48, 192, flags=W4 | GELU, bias="wide", c2=True, mode="bias gelu c2", seed=4)


@pytest.mark.parametrize("K", [64, 128, 320])     # 1, 2 and 5 stages of the 3-stage ring
def test_tile_128x128_deep_ring(K):
    E, fl = hip.VAR_NT_128x128, NONARROW | DEEP
    run_case(E, 200, 136, K, flags=fl, seed=1)
    run_case(E, 200, 136, K, flags=fl, bias="n", mode="bias", seed=2)
    run_case(E, 200, 136, K, flags=fl | RF, bias="n", r="n", rmap=True, mode="bias resid r_rows", seed=3)
    run_case(E, 37, 48, K, flags=fl | MR, r="n", mode="mul_r", seed=4)


@pytest.mark.parametrize("K", [32, 96, 160])
def test_tile_128x128_fp32(K, monkeypatch):
    E = hip.VAR_NT_128x128 + hip.VAR_F32
    if K == 96:
        _epi_piece_cases(E, 200, 136, K, 0, monkeypatch, dtype=F32)
    else:
        run_case(E, 200, 136, K, dtype=F32, seed=1)
        run_case(E, 200, 136, K, dtype=F32, bias="n", mode="bias", seed=2)
        run_case(E, 37, 48, K, dtype=F32, flags=RF, bias="n", r="n", cmap=True, mode="bias resid c_rows", seed=3)
    E4 = hip.VAR_NT_128x128_W4 + hip.VAR_F32
    run_case(E4, 200, 136, K, dtype=F32, flags=W4, bias="n", mode="bias", seed=4)
    run_case(E4, 37, 48, K, dtype=F32, flags=W4 | RF, r="n", mode="resid", seed=5)


# ---------------------------------------------------------------------------------------------------- 128x64 tiles
def test_tile_128x64_double_buffer(monkeypatch):
    E = hip.VAR_NT_128x64
    _epi_piece_cases(E, 300, 192, 128, 0, monkeypatch)
    run_case(E, 4100, 48, 64, seed=1)
    run_case(E, 4100, 48, 64, flags=RELU, bias="n", mode="bias relu", seed=2)
    run_case(E, 4100, 48, 64, flags=RF, r="n", rmap=True, cmap=True, mode="resid r_rows c_rows", seed=3)


@pytest.mark.parametrize("flags,name", [(0, "ring4"), (NODEEP, "nodeep")])
def test_tile_128x64_long_k_dilated_convolution(flags, name):
    """S * Kseg >= 1024: the 4-stage ring (GF_NODEEP: the double buffer) over the tap map of a dilated 3x3 convolution - padding rows -1."""
    E = hip.VAR_NT_128x64
    tap = hip.conv3x3_rowmap(1, 16, 16, 2, DEV)
    assert tap.shape == (9, 256) and int((tap < 0).sum()) > 0
    run_case(E, 256, 128, 128, S=9, amap=tap, flags=flags, mode=name + " taps", seed=1)
    run_case(E, 256, 128, 128, S=9, amap=tap, flags=flags | RELU, bias="n", mode=name + " taps bias relu", seed=2)
    run_case(E, 256, 128, 128, S=9, amap=tap, flags=flags | RF, r="n", mode=name + " taps resid", seed=3)
    far = hip.conv3x3_rowmap(1, 16, 16, 12, DEV)        # dilation 12 on 16 x 16: whole taps are padding for whole row tiles
    run_case(E, 256, 128, 128, S=9, amap=far, flags=flags | hip.GF_TAPSKIP, bias="n", mode=name + " far taps, tapskip", seed=4)


# ---------------------------------------------------------------------------------------------------- 256x64 tiles
def test_tile_256x64_bf16_beyond_128_row_tiles():
    E = hip.VAR_NT_256x64
    run_case(E, 32800, 64, 64, seed=1)
    run_case(E, 32800, 64, 64, bias="n", stats=True, mode="bias stats", seed=2)
    run_case(E, 32800, 40, 64, flags=RF, bias="n", r="n", mode="bias resid", seed=3)
    run_case(E, 32800, 40, 64, flags=DEEP, bias="n", mode="deep bias", seed=4)
    run_case(E, 32800, 64, 64, flags=DEEP | RF, r="n", colsum="table", mode="deep resid colsum", seed=5)


def test_tile_256x64_fp32():
    E = hip.VAR_NT_256x64 + hip.VAR_F32
    run_case(E, 300, 64, 32, dtype=F32, seed=1)
    run_case(E, 300, 64, 32, dtype=F32, bias="n", mode="bias", seed=2)
    run_case(E, 300, 40, 32, dtype=F32, flags=RF, bias="n", r="n", cmap=True, mode="bias resid c_rows", seed=3)


# ---------------------------------------------------------------------------------------------------- 256x256 ring, register epilogue
@pytest.mark.parametrize("M", [37, 257, 600])     # 257: a one-row tail tile
def test_ring_register_epilogue_ragged_shapes(M):
    E = hip.VAR_NT_RING256_REGEPI
    for N in (256, 264, 512):                      # 264: an 8-column tail
        run_case(E, M, N, 128, flags=BIG, seed=1)
        run_case(E, M, N, 128, flags=BIG, bias="n", mode="bias", seed=2)
        run_case(E, M, N, 128, flags=BIG | RF, bias="n", r="n", mode="bias resid", seed=3)


def test_ring_is_dispatched_when_a_round_is_filled():
    """The production rule: 16 x 16 = 256 tiles of 256x256 fill one round of the 256 CUs (>= 90 %) - no GF_BIG."""
    run_case(hip.VAR_NT_RING256_REGEPI, 3900, 3848, 64, bias="n", mode="bias (natural dispatch)", seed=1)


@pytest.mark.parametrize("K", [64, 128, 192, 320])          # nt = 2 (general loop), 4, 6, 10 (steady loop + drain / R-early)
def test_ring_stages_by_epilogue_by_r_addressing(K):
    E, M, N = hip.VAR_NT_RING256_REGEPI, 600, 264
    run_case(E, M, N, K, flags=BIG, seed=1)
    for rmap in (False, True):                     # without r_rows: R blocks requested into vacated stage buffers; with: they must not be
        tag = " r_rows" if rmap else ""
        run_case(E, M, N, K, flags=BIG | RF, r="n", rmap=rmap, mode="resid" + tag, seed=2)
        run_case(E, M, N, K, flags=BIG | MR, r="n", rmap=rmap, mode="mul_r" + tag, seed=3)
        run_case(E, M, N, K, flags=BIG | MD, r="wide", rmap=rmap, mode="mul_dgelu" + tag, seed=4)


def test_ring_tap_segments_take_the_general_loop():
    E = hip.VAR_NT_RING256_REGEPI
    run_case(E, 600, 264, 64, S=3, amap="rand", flags=BIG, bias="n", mode="gather bias", seed=1)
    run_case(E, 600, 264, 64, S=3, amap="rand", flags=BIG | RF, r="n", cmap=True, rmap=True, mode="gather resid r_rows c_rows", seed=2)


def test_ring_every_epilogue_body(monkeypatch):
    """The 13 `case` labels of epilogue_reg's switch and two combinations that fall to its generic body."""
    E, M, N, K = hip.VAR_NT_RING256_REGEPI, 600, 264, 128
    run_case(E, M, N, K, flags=BIG, mode="0", seed=1)
    run_case(E, M, N, K, flags=BIG, bias="n", mode="BIAS", seed=2)
    for sc in (96, 100, 264):                      # a multiple of 8 inside a tile, not a multiple of the 4-column fragment, N
        run_case(E, M, N, K, flags=BIG, bias="n", scale_cols=sc, mode=f"BIAS SCALE({sc})", seed=3)
    run_case(E, M, N, K, flags=BIG | GELU, bias="wide", c2=True, mode="BIAS GELU C2", seed=4)
    run_case(E, M, N, K, flags=BIG | GELU, bias="wide", mode="BIAS GELU", seed=5)
    run_case(E, M, N, K, flags=BIG | RF, bias="n", r="n", mode="BIAS RESID", seed=6)
    run_case(E, M, N, K, flags=BIG | RF, r="n", cmap=True, rmap=True, mode="RESID r_rows c_rows", seed=7)
    run_case(E, M, N, K, flags=BIG | GELU | C2D, bias="wide", c2=True, mode="BIAS GELU C2 C2D", seed=8)
    run_case(E, M, N, K, flags=BIG | MR, r="n", colsum="table", mode="MULR COLSUM", seed=9)
    run_case(E, M, N, K, flags=BIG | MD, r="wide", colsum="table", mode="DGELU COLSUM", seed=10)
    run_case(E, M, N, K, flags=BIG, colsum="table", mode="COLSUM", seed=11)
    run_case(E, M, N, K, flags=BIG, stats=True, mode="COLSUM COLSQ (odd block count)", seed=12)
    run_case(E, 700, N, K, flags=BIG, bias="n", stats=True, mode="BIAS COLSUM COLSQ", seed=13)
    run_case(E, M, N, K, flags=BIG | RELU, bias="n", mode="generic: BIAS RELU", seed=14)
    run_case(E, M, N, K, flags=BIG | RF, bias="n", r="n", scale_cols=100, mode="generic: BIAS SCALE RESID", seed=15)
    run_case(E, M, N, K, flags=BIG | MR, r="n", colsum="atomic", monkeypatch=monkeypatch, mode="MULR COLSUM (atomics)", seed=16)


# ---------------------------------------------------------------------------------------------------- 256x256 ring, LDS epilogue
def test_ring_lds_epilogue(monkeypatch):
    E, M, K = hip.VAR_NT_RING256_LDSEPI, 600, 128
    run_case(E, M, 264, K, flags=BIG | O32, bias="n", mode="bias out_f32", seed=1)
    run_case(E, M, 264, K, flags=BIG | O32 | ACC, mode="out_f32 accum", seed=2)
    run_case(E, M, 260, K, flags=BIG, bias="n", mode="bias N%8", seed=3)
    run_case(E, M, 260, K, flags=BIG | RF, r="n", rmap=True, cmap=True, mode="resid r_rows c_rows N%8", seed=4)
    run_case(E, M, 264, K, flags=BIG | NOREGEPI, mode="noregepi", seed=5)
    run_case(E, M, 264, K, flags=BIG | NOREGEPI | GELU, bias="wide", c2=True, mode="noregepi bias gelu c2", seed=6)
    run_case(E, M, 264, K, flags=BIG | NOREGEPI | MD, r="wide", colsum="table", mode="noregepi mul_dgelu colsum", seed=7)
    run_case(E, M, 264, K, flags=BIG | NOREGEPI | MR | RELU, r="n", mode="noregepi mul_r relu", seed=8)
    # slices that start 4 columns into a wider bf16 buffer: the dispatch must send them to the LDS epilogue
    run_case(E, M, 264, K, flags=BIG | GELU, bias="wide", c2=True, col0=4, mode="slice+4 bias gelu c2", seed=9)
    run_case(E, M, 264, K, flags=BIG | RF, bias="n", r="n", col0=4, mode="slice+4 bias resid", seed=10)
    run_case(E, 257, 264, 64, flags=BIG | RF, r="n", col0=4, mode="slice+4 resid", seed=11)


# ---------------------------------------------------------------------------------------------------- split-K
def _planned_splits(M, N, Kseg, S):
    need = hip.load().stswin_gemm_nt_splitk_scratch(M, N, Kseg, S)       # (host-only: splits * M * N floats)
    assert need > 0 and need % (M * N) == 0
    return need // (M * N)


def test_split_k_smallest_candidates():
    E = hip.VAR_NT_SPLITK
    assert _planned_splits(256, 256, 2048, 1) == 4 and _planned_splits(300, 264, 448, 5) == 4 and _planned_splits(256, 256, 256, 9) == 4
    run_case(E, 256, 256, 2048, splits=4, seed=1)
    run_case(E, 256, 256, 2048, bias="n", col0=8, splits=4, mode="bias slice+8", seed=2)
    run_case(E, 300, 264, 448, S=5, amap="rand", splits=4, mode="gather, ragged last split", seed=3)
    run_case(E, 300, 264, 448, S=5, amap="rand", flags=RELU, bias="n", splits=4, mode="gather bias relu", seed=4)
    tap = hip.conv3x3_rowmap(1, 16, 16, 2, DEV)
    run_case(E, 256, 256, 256, S=9, amap=tap, flags=RELU, bias="n", splits=4, mode="taps bias relu", seed=5)
