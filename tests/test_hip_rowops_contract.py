"""The row kernels of stswincl_amd/csrc/rowops.hip - ln_fwd_kernel<T, 1..16>, ln_bwd_kernel<T, NP, 4|8, ACC, DXS>, colsum_kernel,
slab_fold_kernel, slab_fold_multi_kernel (the deferred queue), bias_scatter_kernel and the four multi-launch repack forms - against the
float64 contract of tests/rowops_ref.py, per ELEMENT, with the derived bounds of that module (nothing here is tuned on a GPU).
tests/test_rowops_ref.py shows on the CPU that at every case an fp32 emulation of the kernels' association stays inside those bounds and
that the planted defects (a lost row, an overwritten partial, a skipped or doubled slab, ...) land outside.

Every case is called through the raw entry points (hip.load().stswin_*) and asserts
  * |got - ref| <= bound for every element; a failure names the worst element, its piece and lane, and the number of offenders; one line per
    case is printed with the largest err / bound;
  * every output is finite;
  * nothing else was written: outputs are row and column slices of taller, wider buffers holding a finite sentinel, and the inputs are
    bit-identical afterwards;
  * the scratch buffer is NaN before each launch; after a LayerNorm backward exactly `grid` slabs of [3][C] are non-NaN in their first two
    (three with dxsum) vectors - the geometry that ran, held to rowops_ref.ln_bwd_geometry - nothing is non-NaN behind them, and the float64
    sum of the slabs equals the folded output within the fold's own bound (a wrong kernel is told from a wrong fold);
  * a second call gives the same bits.
The references run in float64 on the device the operands are on (plain torch, the same code the CPU test checks against autograd)."""
import time

import pytest
import torch

import rowops_ref as R
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
DEV = "cuda"
SENT = 12345.0
EPS = 1e-5
NAN = float("nan")


def _id(c):
    return c.name.replace(" ", "_")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dt(dtype):
    return 0 if dtype == BF else 1


def _st():
    return hip._stream()


def _scratch(floats):
    """The whole per-device scratch buffer (outside deferred_folds), NaN everywhere."""
    ws = hip.scratch(DEV, floats)
    ws.fill_(NAN)
    return ws


def _framed(inner, top=1, left=0, right=0, bottom=2, sentinel=SENT):
    """inner [r][c] inside a taller, wider sentinel buffer -> (buffer, view of the inner block)."""
    r, c = inner.shape
    buf = torch.full((r + top + bottom, c + left + right), sentinel, dtype=inner.dtype, device=DEV)
    buf[top:top + r, left:left + c] = inner.to(DEV)
    return buf, buf[top:top + r, left:left + c]


def _untouched_outside(buf, init, top, left, r, c, tag):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[top:top + r, left:left + c] = True
    stray = (_bits(buf) != _bits(init)) & ~inside
    assert not bool(stray.any()), f"{tag}: {int(stray.sum())} elements outside the result were written, first at {stray.nonzero()[0].tolist()}"


def _judge(tag, what, got, want, bnd, pk, fails, line):
    assert bool(torch.isfinite(got[~torch.isnan(bnd)]).all()), f"{tag}: {what} is not finite"
    ratio, bad, where = R.worst(got, want, bnd, pk)
    line.append(f"{what} {ratio:.3f}")
    if bad:
        fails.append(f"{tag}: {what}: {bad} of {got.numel()} elements beyond their bound, worst err / bound = {ratio:.3g} at {where}")


def _merge_map(rows):
    """The gathered cases' row map as hip.merge_rowmap builds it on the device - held to the reference's own (rows)."""
    if rows is None:
        return None
    m = hip.merge_rowmap(R.GATHER["frames"], R.GATHER["H"], R.GATHER["W"]).flatten()
    assert m.dtype == torch.int32 and torch.equal(m.cpu(), rows)
    return m


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n[rowops] wall time of this file: {time.time() - t0:.1f} s")


# ====================================================================================================== LayerNorm forward
def _fwd_launch(c, d, x_view, rows, stats=True):
    pk = R.pack_of(c.dtype)
    Cseg = c.Cseg or c.C
    ybuf, y = _framed(torch.full((c.M, c.C), NAN, dtype=c.dtype), 1, pk, pk, 2)
    mbuf = torch.full((2, c.M + 8), SENT, device=DEV)
    mbuf[:, 4:4 + c.M] = NAN
    init = (ybuf.clone(), mbuf.clone())
    rc = hip.load().stswin_layernorm_fwd(_dt(c.dtype), x_view.data_ptr(), x_view.stride(0), hip._p(rows), c.S, Cseg, y.data_ptr(), y.stride(0),
                                         d["gamma"].data_ptr(), d["beta"].data_ptr(), mbuf[0, 4:].data_ptr() if stats else None,
                                         mbuf[1, 4:].data_ptr() if stats else None, c.M, EPS, _st())
    assert rc == 0, f"{c.name}: stswin_layernorm_fwd returned {rc}"
    return ybuf, y, mbuf, init


@pytest.mark.parametrize("c", R.cases_fwd(), ids=_id)
def test_layernorm_forward(c):
    x, gamma, beta, rows = R.fwd_operands(c)
    pk = R.pack_of(c.dtype)
    Cseg = c.Cseg or c.C
    d = {"gamma": gamma.to(DEV), "beta": beta.to(DEV)}
    rows_d = _merge_map(rows)
    if c.form in ("gather", "xslice"):                          # x is a column slice of a wider matrix: ldx > Cseg
        xbuf = torch.randn(x.shape[0], Cseg + pk).to(c.dtype)
        xbuf[:, :Cseg] = x
        xbuf = xbuf.to(DEV)
        xv = xbuf[:, :Cseg]
    else:
        xbuf = x.to(DEV)
        xv = xbuf
    xinit = xbuf.clone()
    runs = [_fwd_launch(c, d, xv, rows_d) for _ in range(2)]
    ybuf, y, mbuf, init = runs[0]
    tag = f"fwd {c.name}"
    y64, mean, var, rstd = R.ln_forward(xv, d["gamma"], d["beta"], EPS, rows_d, c.S, Cseg, c.M)
    b = R.fwd_bound(xv, d["gamma"], d["beta"], EPS, c.dtype, rows_d, c.S, Cseg, c.M)
    fails, line = [], [f"[rowops] fwd {c.name} NP={c.NP} (by the launcher's switch):"]
    _judge(tag, "y", y, y64, b["y"], pk, fails, line)
    _judge(tag, "mean", mbuf[0, 4:4 + c.M], mean, b["mean"], None, fails, line)
    _judge(tag, "rstd", mbuf[1, 4:4 + c.M], rstd, b["rstd"], None, fails, line)
    print(" ".join(line))
    assert not fails, "; ".join(fails)
    _untouched_outside(ybuf, init[0], 1, pk, c.M, c.C, tag)
    _untouched_outside(mbuf, init[1], 0, 4, 2, c.M, tag)
    assert _same(xbuf, xinit) and _same(d["gamma"], gamma.to(DEV)) and _same(d["beta"], beta.to(DEV)), f"{tag}: an input was written"
    assert rows is None or torch.equal(rows_d.cpu(), rows)
    assert _same(runs[1][0], ybuf) and _same(runs[1][2], mbuf), f"{tag}: a second call gave other bits"
    # mean == NULL (save_stats=False): the same y, no statistics written
    yb3, _, mb3, init3 = _fwd_launch(c, d, xv, rows_d, stats=False)
    assert _same(yb3, ybuf) and _same(mb3, init3[1]), f"{tag}: without statistics"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_layernorm_forward_wrapper_out_row_block_and_no_stats(dtype):
    """hip.layernorm_fwd(out=a row block of a taller buffer, save_stats=False) gives the bits of the plain call and writes nothing else."""
    g = torch.Generator().manual_seed(5)
    M, C = 37, 264
    x = R.make_x("normal", M, C, dtype, g).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    y, mean, rstd = hip.layernorm_fwd(x, gamma, beta, M=M)
    tall = torch.full((M + 9, C), SENT, dtype=dtype, device=DEV)
    init = tall.clone()
    y2, m2, r2 = hip.layernorm_fwd(x, gamma, beta, M=M, out=tall[4:4 + M], save_stats=False)
    assert m2 is None and r2 is None and y2.data_ptr() == tall[4:].data_ptr()
    assert _same(tall[4:4 + M], y) and _same(tall[:4], init[:4]) and _same(tall[4 + M:], init[4 + M:])
    y64, m64, _, r64 = R.ln_forward(x, gamma, beta, EPS)
    b = R.fwd_bound(x, gamma, beta, EPS, dtype)
    for got, want, bnd in ((y, y64, b["y"]), (mean, m64, b["mean"]), (rstd, r64, b["rstd"])):
        assert R.worst(got, want, bnd)[1] == 0


# ====================================================================================================== LayerNorm backward
MODES = ("overwrite", "in place", "add")


def _bwd_launch(c, d, mode, dxs, old_dx, olds, expect_rc=0):
    """One raw call -> (dx buffer, dx view, parameter buffer, scratch, the buffers' initial contents)."""
    pk = R.pack_of(c.dtype)
    Cseg = c.Cseg or c.C
    n_src = d["x"].shape[0]
    start = old_dx if mode == "in place" else torch.full((n_src, Cseg), SENT, dtype=c.dtype)
    dxbuf, dx = _framed(start, 1, pk, pk, 2)
    pbuf = torch.full((3, c.C + 8), SENT, device=DEV)
    pbuf[:, 4:4 + c.C] = olds
    init = (dxbuf.clone(), pbuf.clone())
    lib = hip.load()
    ws = _scratch(lib.stswin_layernorm_bwd_scratch(c.M, c.C))
    common = (_dt(c.dtype), d["dy"].data_ptr(), d["dy"].stride(0), d["x"].data_ptr(), d["x"].stride(0), hip._p(d["rows"]), c.S, Cseg,
              d["gamma"].data_ptr(), d["mean"].data_ptr(), d["rstd"].data_ptr())
    tail = (pbuf[0, 4:].data_ptr(), pbuf[1, 4:].data_ptr(), c.M)
    dxsum = pbuf[2, 4:].data_ptr() if dxs else None
    if mode == "add":
        rc = lib.stswin_layernorm_bwd_add(*common, d["add"].data_ptr(), d["add"].stride(0), dx.data_ptr(), dx.stride(0), *tail, dxsum,
                                          ws.data_ptr(), _st())
    else:
        rc = lib.stswin_layernorm_bwd(*common, dx.data_ptr(), dx.stride(0), *tail, 1 if mode == "in place" else 0, dxsum, ws.data_ptr(), _st())
    assert rc == expect_rc, f"{c.name} ({mode}): returned {rc}"
    return dxbuf, dx, pbuf, ws, init


def _check_scratch(c, tag, ws, pbuf, olds, dxs, fails, line):
    """The geometry that ran, read from the NaN-filled scratch; the slabs' float64 sum against the folded outputs."""
    C = c.C
    rpw, waves, groups, grid = c.geometry
    scr = hip.load().stswin_layernorm_bwd_scratch(c.M, C)
    assert scr == R.ln_bwd_scratch(c.M, C), f"{tag}: stswin_layernorm_bwd_scratch = {scr}"
    live = ~torch.isnan(ws[:scr].view(-1, 3, C))
    full2 = live[:, :2].all(2).all(1)
    any_ = live.any(2).any(1)
    seen = int(full2.sum())
    assert seen == grid and bool(full2[:grid].all()) and not bool(any_[grid:].any()), \
        f"{tag}: {seen} slabs were written ({int(any_.sum())} touched), the geometry {c.geometry} has {grid}"
    third = live[:grid, 2]
    assert bool(third.all()) if dxs else not bool(third.any()), f"{tag}: the dxsum vector of the slabs ({'wanted' if dxs else 'not wanted'})"
    assert bool(torch.isnan(ws[scr:]).all()), f"{tag}: scratch was written past stswin_layernorm_bwd_scratch(M, C)"
    slabs = ws[:grid * 3 * C].view(grid, 3, C)
    for k, what in enumerate(("dgamma", "dbeta", "dxsum")[:3 if dxs else 2]):
        want = olds[k].double() + slabs[:, k].double().sum(0)
        bnd = R.sum_bound(slabs[:, k].double().abs().sum(0), R.fold_depth(grid, True), 0, olds[k].double().abs())
        ratio, bad, where = R.worst(pbuf[k, 4:4 + C], want, bnd)
        if bad:
            fails.append(f"{tag}: the fold of {what}: {bad} elements beyond the fold's bound over {grid} slabs, worst {ratio:.3g} at {where}")
    line.append(f"grid={seen}")


@pytest.mark.parametrize("c", R.cases_bwd(), ids=_id)
def test_layernorm_backward(c):
    x, gamma, dy, add, rows, n_src = R.bwd_operands(c)
    pk = R.pack_of(c.dtype)
    Cseg = c.Cseg or c.C
    # x, dy and add with pitches of their own (add's differs from dx's)
    host = {"x": x, "dy": dy, "add": add, "gamma": gamma, "rows": rows}
    d, inits = {}, {}
    for k, extra in (("x", pk), ("dy", 0), ("add", 3 * pk)):
        buf = torch.randn(host[k].shape[0], host[k].shape[1] + extra).to(c.dtype)
        buf[:, :host[k].shape[1]] = host[k]
        inits[k] = buf.to(DEV)
        d[k] = inits[k].clone()[:, :host[k].shape[1]]
    d["gamma"] = gamma.to(DEV)
    d["rows"] = _merge_map(rows)
    _, d["mean"], d["rstd"] = hip.layernorm_fwd(d["x"], d["gamma"], torch.zeros(c.C, device=DEV), M=c.M, rows=d["rows"], S=c.S, Cseg=Cseg)
    stats0 = (d["mean"].clone(), d["rstd"].clone())
    g = R.seed(c)
    olds = torch.randn(3, c.C, generator=g).to(DEV)
    old_dx = torch.randn(n_src, Cseg, generator=g).to(c.dtype)
    core = R.bwd_core(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], d["rows"], c.S, Cseg, c.M)
    named = torch.zeros(n_src, dtype=torch.bool, device=DEV)
    if rows is None:
        named[:c.M] = True
    else:
        named[d["rows"].long()] = True
    fails = []
    for mode in MODES:
        a = {"overwrite": None, "in place": old_dx.to(DEV), "add": d["add"]}[mode]
        dx64, dg, db, dxs64 = R.ln_backward(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], d["rows"], c.S, Cseg, add=a, n_src=n_src, core=core)
        bnd = R.bwd_bound(core, c.dtype, c.M, d["rows"], a, n_src, {"dgamma": olds[0], "dbeta": olds[1], "dxsum": olds[2]})
        for dxs in (True, False):
            tag = f"bwd {c.name} ({mode}, {'dxsum' if dxs else 'no dxsum'})"
            runs = [_bwd_launch(c, d, mode, dxs, old_dx, olds) for _ in range(2)]
            dxbuf, dx, pbuf, ws, init = runs[1]                    # (the scratch is the second launch's)
            line = [f"[rowops] {tag} NP={c.NP} rows/wave={c.geometry[0]} waves={c.geometry[1]} groups={c.geometry[2]}"]
            _check_scratch(c, tag, ws, pbuf, olds, dxs, fails, line)
            _judge(tag, "dx", dx, dx64, bnd["dx"], pk, fails, line)
            _judge(tag, "dgamma", pbuf[0, 4:4 + c.C], olds[0].double() + dg, bnd["dgamma"], pk, fails, line)
            _judge(tag, "dbeta", pbuf[1, 4:4 + c.C], olds[1].double() + db, bnd["dbeta"], pk, fails, line)
            if dxs:
                _judge(tag, "dxsum", pbuf[2, 4:4 + c.C], olds[2].double() + dxs64, bnd["dxsum"], pk, fails, line)
            else:
                assert _same(pbuf[2], init[1][2]), f"{tag}: dxsum was written"
            print(" ".join(line))
            _untouched_outside(dxbuf, init[0], 1, pk, n_src, Cseg, tag)
            assert _same(dx[~named], init[0][1:1 + n_src, pk:pk + Cseg][~named]), f"{tag}: a source row no map entry names was written"
            _untouched_outside(pbuf, init[1], 0, 4, 3, c.C, tag)
            assert _same(runs[0][0], dxbuf) and _same(runs[0][2], pbuf), f"{tag}: a second call gave other bits"
    assert not fails, "; ".join(fails)
    for k in ("x", "dy", "add"):
        assert _same(d[k]._base if d[k]._base is not None else d[k], inits[k]), f"bwd {c.name}: {k} was written"
    assert _same(d["gamma"], gamma.to(DEV)) and _same(d["mean"], stats0[0]) and _same(d["rstd"], stats0[1])
    assert rows is None or torch.equal(d["rows"].cpu(), rows)


# ====================================================================================================== refusals of the LayerNorm entries
def _ln_buffers(dtype, M, C, ld=None):
    ld = C if ld is None else ld
    z = lambda *s: torch.full(s, 1.0, dtype=dtype, device=DEV)       # noqa: E731
    f = lambda *s: torch.full(s, SENT, device=DEV)                   # noqa: E731
    return {"x": z(M, ld), "dy": z(M, ld), "add": z(M, ld), "y": torch.full((M, ld), SENT, dtype=dtype, device=DEV),
            "dx": torch.full((M, ld), SENT, dtype=dtype, device=DEV), "gamma": f(C), "beta": f(C), "mean": f(M), "rstd": f(M), "dg": f(C), "db": f(C),
            "dxs": f(C), "ws": hip.scratch(DEV, 3 * 4 * C * M)}


REFUSALS = [("fwd", F32, 4100, {}, -1104), ("bwd", F32, 2052, {}, -1104), ("bwd", BF, 3280, {}, -1106),
            ("fwd", BF, 12, {}, -1105), ("fwd", F32, 6, {}, -1105), ("fwd", BF, 64, {"ldx": 68}, -1105), ("fwd", BF, 64, {"ldy": 68}, -1105),
            ("bwd", BF, 12, {}, -1105), ("bwd", BF, 64, {"ldx": 68}, -1105), ("bwd", BF, 64, {"lddy": 68}, -1105), ("bwd", F32, 64, {"lddx": 66}, -1105),
            ("bwd_add", BF, 64, {"ldadd": 68}, -1105), ("bwd", BF, 64, {"ws": None}, -1111), ("bwd_add", BF, 64, {"ws": None}, -1111),
            ("bwd_add", BF, 64, {"add": None}, -1105)]


@pytest.mark.parametrize("entry,dtype,C,how,code", REFUSALS, ids=[f"{e}-{'bf16' if t == BF else 'f32'}-C{c}-{'-'.join(h) or 'C'}-{k}"
                                                                   for e, t, c, h, k in REFUSALS])
def test_layernorm_refusals_leave_every_output_untouched(entry, dtype, C, how, code):
    M = 5
    b = _ln_buffers(dtype, M, C, ld=72 if C == 64 else None)
    ld = b["x"].stride(0)
    outs = ("y", "dx", "mean", "rstd", "dg", "db", "dxs")
    if entry != "fwd":
        b["mean"].fill_(0.5)
        b["rstd"].fill_(1.0)
    before = {k: b[k].clone() for k in outs}
    lib = hip.load()
    ws = None if ("ws" in how and how["ws"] is None) else b["ws"].data_ptr()
    if entry == "fwd":
        rc = lib.stswin_layernorm_fwd(_dt(dtype), b["x"].data_ptr(), how.get("ldx", ld), None, 1, C, b["y"].data_ptr(), how.get("ldy", ld),
                                      b["gamma"].data_ptr(), b["beta"].data_ptr(), b["mean"].data_ptr(), b["rstd"].data_ptr(), M, EPS, _st())
    else:
        common = (_dt(dtype), b["dy"].data_ptr(), how.get("lddy", ld), b["x"].data_ptr(), how.get("ldx", ld), None, 1, C, b["gamma"].data_ptr(),
                  b["mean"].data_ptr(), b["rstd"].data_ptr())
        for acc in ((0, 1) if entry == "bwd" else (1,)):
            if entry == "bwd":
                rc = lib.stswin_layernorm_bwd(*common, b["dx"].data_ptr(), how.get("lddx", ld), b["dg"].data_ptr(), b["db"].data_ptr(), M, acc,
                                              b["dxs"].data_ptr(), ws, _st())
            else:
                add = None if ("add" in how and how["add"] is None) else b["add"].data_ptr()
                rc = lib.stswin_layernorm_bwd_add(*common, add, how.get("ldadd", ld), b["dx"].data_ptr(), how.get("lddx", ld), b["dg"].data_ptr(),
                                                  b["db"].data_ptr(), M, b["dxs"].data_ptr(), ws, _st())
            assert rc == code, f"returned {rc}"
    assert rc == code, f"returned {rc}"
    torch.cuda.synchronize()
    for k in outs:
        assert _same(b[k], before[k]), f"the refused call wrote {k}"


# ====================================================================================================== colsum
@pytest.mark.parametrize("c", R.cases_colsum(), ids=_id)
def test_colsum(c):
    pk = R.pack_of(c.dtype)
    g = R.seed(c)
    ybuf = torch.randn(c.M + 2, c.N + pk, generator=g).to(c.dtype)
    ybuf[c.M:] = NAN                                               # the M argument is smaller than the rows of y
    ybuf = ybuf.to(DEV)
    yinit = ybuf.clone()
    y = ybuf[:, :c.N]                                              # a column slice: ldy > N
    old = torch.randn(c.N, generator=g).to(DEV)
    lib = hip.load()
    outs = []
    for _ in range(2):
        obuf = torch.full((c.N + 8,), SENT, device=DEV)
        obuf[4:4 + c.N] = old
        ws = _scratch(lib.stswin_colsum_scratch(c.M, c.N))
        rc = lib.stswin_colsum(_dt(c.dtype), y.data_ptr(), y.stride(0), obuf[4:].data_ptr(), c.M, c.N, ws.data_ptr(), _st())
        assert rc == 0, f"colsum {c.name}: returned {rc}"
        outs.append(obuf)
    obuf = outs[0]
    nb = -(-c.M // 512)
    assert lib.stswin_colsum_scratch(c.M, c.N) == nb * c.N
    assert not bool(torch.isnan(ws[:nb * c.N]).any()) and bool(torch.isnan(ws[nb * c.N:]).all()), f"colsum {c.name}: {nb} slabs of {c.N} expected"
    got = obuf[4:4 + c.N]
    assert bool(torch.isfinite(got).all())
    ratio, bad, where = R.worst(got, old.double() + R.colsum(y, c.M), R.colsum_bound(y, c.M, old), pk)
    print(f"[rowops] colsum {c.name} row blocks={nb}: {ratio:.3f}")
    assert bad == 0, f"colsum {c.name}: {bad} of {c.N} beyond their bound, worst {ratio:.3g} at {where}"
    assert bool((obuf[:4] == SENT).all()) and bool((obuf[4 + c.N:] == SENT).all()), f"colsum {c.name}: written outside out"
    assert _same(ybuf, yinit), f"colsum {c.name}: y was written"
    assert _same(outs[1], obuf), f"colsum {c.name}: a second call gave other bits"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_colsum_empty_and_refusals(dtype):
    pk = R.pack_of(dtype)
    lib = hip.load()
    y = torch.ones(16, 4 * pk + pk, dtype=dtype, device=DEV)
    out = torch.full((4 * pk,), SENT, device=DEV)
    ws = hip.scratch(DEV, 1024)
    assert lib.stswin_colsum(_dt(dtype), y.data_ptr(), y.stride(0), out.data_ptr(), 0, 4 * pk, ws.data_ptr(), _st()) == 0
    assert lib.stswin_colsum(_dt(dtype), y.data_ptr(), y.stride(0), out.data_ptr(), 16, 4 * pk - 2, ws.data_ptr(), _st()) == -1107
    assert lib.stswin_colsum(_dt(dtype), y.data_ptr(), y.stride(0) - 2, out.data_ptr(), 16, 4 * pk, ws.data_ptr(), _st()) == -1107
    assert lib.stswin_colsum(_dt(dtype), y.data_ptr(), y.stride(0), out.data_ptr(), 16, 4 * pk, None, _st()) == -1111
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ====================================================================================================== slab_fold
def _fold_launch(c, ws, stride, bstride, old, obs, null_out1):
    """-> the output buffer [nseg][8 + batch * obs] after one raw call; out_s starts 4 floats in, batch b at b * obs."""
    obuf = torch.full((c.nseg, 8 + c.batch * obs), SENT, device=DEV)
    view = obuf[:, 4:4 + c.batch * obs].view(c.nseg, c.batch, obs)[:, :, :c.seg_len]
    view.copy_(old if c.accumulate else torch.full_like(old, NAN))
    if null_out1:
        obuf[1] = SENT
    ptr = [obuf[s, 4:].data_ptr() if s < c.nseg else None for s in range(3)]
    if null_out1:
        ptr[1] = None
    rc = hip.load().stswin_slab_fold(ws.data_ptr(), stride, bstride, c.nslabs, c.seg_len, c.nseg, ptr[0], ptr[1], ptr[2], obs, c.batch,
                                     c.accumulate, _st())
    assert rc == 0, f"fold {c.name}: returned {rc}"
    return obuf, view


@pytest.mark.parametrize("nslabs", R.FOLD_NSLABS)
def test_slab_fold(nslabs):
    worst_ratio, fails = 0.0, []
    for c in [c for c in R.cases_fold() if c.nslabs == nslabs]:
        obs = c.seg_len + 4                                        # the outputs' batch stride is wider than a segment
        for integers in (True, False):
            ws, stride, bstride, old = R.fold_operands(c, integers, DEV)
            winit = ws.clone()
            args = (stride, bstride, c.nslabs, c.seg_len, c.nseg, c.batch)
            runs = [_fold_launch(c, ws, stride, bstride, old, obs, c.null_out1) for _ in range(2)]
            obuf, got = runs[0]
            tag = f"fold {c.name} ({'integers' if integers else 'normal'})"
            want = R.fold(ws, *args) + (old.double() if c.accumulate else 0)
            keep = [s for s in range(c.nseg) if not (c.null_out1 and s == 1)]
            assert bool(torch.isfinite(got[keep]).all()), f"{tag}: not finite"
            if integers:                                           # every order of summation is exact: bit for bit the float64 sum
                if not torch.equal(got[keep].double(), want[keep]):
                    fails.append(f"{tag}: {int((got[keep].double() != want[keep]).sum())} sums of integers are not exact")
            else:
                bnd = R.fold_bound(ws, *args, old=old, accumulate=bool(c.accumulate))
                ratio, bad, where = R.worst(got[keep], want[keep], bnd[keep])
                worst_ratio = max(worst_ratio, ratio)
                if bad:
                    fails.append(f"{tag}: {bad} beyond their bound, worst {ratio:.3g} at {where}")
            # nothing else: the frame, the padding between the batches, the whole row of a NULL out1
            frame = obuf.clone()
            frame[:, 4:4 + c.batch * obs].view(c.nseg, c.batch, obs)[:, :, :c.seg_len] = SENT
            if c.null_out1:
                assert bool((obuf[1] == SENT).all()), f"{tag}: the row of the NULL out1 was written"
            assert bool((frame[keep] == SENT).all()), f"{tag}: written outside the segments"
            assert _same(ws, winit), f"{tag}: the slabs were written"
            assert _same(runs[1][0], obuf), f"{tag}: a second call gave other bits"
    c0 = [c for c in R.cases_fold() if c.nslabs == nslabs][0]
    print(f"[rowops] fold {nslabs} slabs QL={c0.QL} four-load passes={c0.loops4}: {worst_ratio:.3f} (integers exact)")
    assert not fails, "; ".join(fails[:5]) + f" ({len(fails)} in all)"


def test_slab_fold_refusals_and_empty_calls():
    lib = hip.load()
    ws = torch.ones(4096, device=DEV)
    out = torch.full((3, 64), SENT, device=DEV)
    o = [out[s].data_ptr() for s in range(3)]
    assert lib.stswin_slab_fold(ws.data_ptr(), 64, 0, 4, 8, 4, o[0], o[1], o[2], 0, 1, 1, _st()) == -1110          # nseg = 4
    assert lib.stswin_slab_fold(ws.data_ptr(), 64, 0, 4, 6, 1, o[0], None, None, 0, 1, 1, _st()) == -1110           # seg_len = 6
    assert lib.stswin_slab_fold(ws.data_ptr(), 6, 0, 4, 4, 1, o[0], None, None, 0, 1, 1, _st()) == -1110            # slab_stride = 6
    assert lib.stswin_slab_fold(ws.data_ptr(), 64, 0, 4, 8, 0, o[0], o[1], o[2], 0, 1, 1, _st()) == 0               # nseg = 0
    assert lib.stswin_slab_fold(ws.data_ptr(), 64, 0, 0, 8, 3, o[0], o[1], o[2], 0, 1, 0, _st()) == 0               # nslabs = 0
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ====================================================================================================== the deferred queue
def _deferred_program():
    """13 folds - one more than the queue holds - through the public entry points: layernorm_bwd with and without dxsum (5 and 128 slabs),
    colsum, and raw stswin_slab_fold calls on regions from hip.scratch (17, 96, 200 and 3 x 40 slabs).  -> the outputs, in order."""
    lib = hip.load()
    g = torch.Generator().manual_seed(77)
    outs = []

    def region(floats):                     # (immediate mode: the start of the whole buffer; queued mode: a region of its own)
        return hip.scratch(DEV, floats)[:floats]

    def ln(M, C, dxs, dtype):
        x = R.make_x("normal", M, C, dtype, g).to(DEV)
        gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
        dy = torch.randn(M, C, generator=g).to(dtype).to(DEV)
        _, mean, rstd = hip.layernorm_fwd(x, gamma, torch.zeros(C, device=DEV), M=M)
        acc = [torch.randn(C, generator=g).to(DEV) for _ in range(3 if dxs else 2)]
        hip.layernorm_bwd(dy, x, gamma, mean, rstd, acc[0], acc[1], M=M, dxsum=acc[2] if dxs else None)
        outs.extend(acc)

    def raw(nslabs, seg_len, nseg, batch, accumulate):
        width = nseg * seg_len
        bstride = nslabs * width + 4 if batch > 1 else 0
        ws = region(batch * (nslabs * width + 4))
        ws.copy_(torch.randn(ws.numel(), generator=g))
        o = torch.randn(nseg, batch, seg_len, generator=g).to(DEV)
        rc = lib.stswin_slab_fold(ws.data_ptr(), width, bstride, nslabs, seg_len, nseg, o[0].data_ptr(), o[1].data_ptr() if nseg > 1 else None,
                                  o[2].data_ptr() if nseg > 2 else None, seg_len, batch, accumulate, _st())
        assert rc == 0
        outs.append(o)

    ln(37, 64, True, BF)                     # 1
    raw(17, 60, 2, 1, 1)                     # 2
    ln(4096, 64, False, BF)                  # 3: 128 slabs, 64 slab lanes
    y = torch.randn(1030, 264, generator=g).to(DEV)
    o = torch.randn(264, generator=g).to(DEV)
    hip.colsum(y, o)                         # 4
    outs.append(o)
    raw(96, 64, 3, 1, 0)                     # 5
    raw(40, 260, 1, 3, 1)                    # 6: batch = 3
    ln(37, 260, False, F32)                  # 7
    raw(200, 4, 3, 1, 1)                     # 8
    ln(4096, 64, True, F32)                  # 9
    raw(15, 64, 1, 1, 0)                     # 10
    yb = torch.randn(513, 64, generator=g).to(BF).to(DEV)
    ob = torch.randn(64, generator=g).to(DEV)
    hip.colsum(yb, ob)                       # 11
    outs.append(ob)
    raw(193, 60, 2, 1, 1)                    # 12
    raw(49, 4, 1, 1, 1)                      # 13: the queue is full - the first twelve are launched, this one waits for the end of the block
    return outs


def test_deferred_folds_overflow_the_queue_and_match_immediate_mode(monkeypatch):
    assert R.FOLD_QUEUE_MAX == 12
    lib = hip.load()
    immediate = _deferred_program()
    torch.cuda.synchronize()
    runs, regions = [], []
    real_scratch = hip.scratch

    def recording(device, floats):
        t = real_scratch(device, floats)
        if hip._DEFER[0]:
            regions.append((t.data_ptr(), t.numel() * 4))
        return t
    monkeypatch.setattr(hip, "scratch", recording)
    try:
        for _ in range(2):
            del regions[:]
            hip.scratch(DEV, 64).fill_(NAN)            # (the whole buffer: no stale slab can stand in for a missing one)
            with hip.deferred_folds():
                outs = _deferred_program()
            torch.cuda.synchronize()
            runs.append(outs)
            assert len(regions) == 13
            spans = sorted(regions)
            for (a, n), (b, _) in zip(spans, spans[1:]):
                assert a + n <= b, "two queued folds were handed overlapping scratch regions"
    finally:                                           # a failure must not leave the thread in queued mode
        hip._DEFER[0], hip._DEFER[1] = False, 0
        lib.stswin_fold_defer(0, _st())
    assert len(immediate) == len(runs[0]) == len(runs[1])
    for i, (a, b, c) in enumerate(zip(immediate, runs[0], runs[1])):
        assert bool(torch.isfinite(b).all()), f"output {i} of the queued run is not finite"
        assert _same(a, b), f"output {i}: the queued folds give other bits than the immediate ones"
        assert _same(b, c), f"output {i}: the second queued run gave other bits"
    # immediate mode is back: a fold launched now is visible at once
    ws = torch.ones(4 * 8, device=DEV)
    o = torch.zeros(8, device=DEV)
    assert lib.stswin_slab_fold(ws.data_ptr(), 8, 0, 4, 8, 1, o.data_ptr(), None, None, 0, 1, 0, _st()) == 0
    assert float(o.min()) == 4.0 == float(o.max())


# ====================================================================================================== bias_scatter
@pytest.mark.parametrize("nslabs", [1, 3])
def test_bias_scatter_raw(nslabs):
    """One table row owns 200 pairs (the lane loop runs four times), another owns none (its bits stay)."""
    g = torch.Generator().manual_seed(nslabs)
    N, heads, table_rows = 16, 3, 10
    index = torch.zeros(N * N, dtype=torch.int64)
    index[200:] = torch.randint(2, table_rows, (N * N - 200,), generator=g)
    index = index[torch.randperm(N * N, generator=g)].to(DEV)
    order, offs = hip.scatter_lists(index, table_rows)
    assert int(offs[1]) == 200 and int(offs[2]) == 200
    dbias = torch.randn(nslabs, heads, N, N, generator=g).to(DEV)
    old = torch.randn(table_rows, heads, generator=g).to(DEV)
    lib = hip.load()
    bufs = []
    for _ in range(2):
        buf = torch.full((table_rows * heads + 8,), SENT, device=DEV)
        buf[4:-4] = old.flatten()
        rc = lib.stswin_bias_scatter(dbias.data_ptr(), order.data_ptr(), offs.data_ptr(), buf[4:].data_ptr(), N, heads, table_rows, nslabs, _st())
        assert rc == 0
        bufs.append(buf)
    got = bufs[0][4:-4].view(table_rows, heads)
    s, ab, counts = R.bias_scatter(dbias, index, table_rows, nslabs)
    ratio, bad, where = R.worst(got, old.double() + s, R.bias_scatter_bound(ab, counts, nslabs, old))
    print(f"[rowops] bias_scatter nslabs={nslabs} pairs per row {counts.tolist()}: {ratio:.3f}")
    assert bad == 0, f"{bad} beyond their bound, worst {ratio:.3g} at {where}"
    assert _same(got[1], old[1]), "the row without pairs changed"
    assert bool((bufs[0][:4] == SENT).all()) and bool((bufs[0][-4:] == SENT).all()) and _same(bufs[1], bufs[0])
    keep = bufs[0].clone()
    assert lib.stswin_bias_scatter(dbias.data_ptr(), None, offs.data_ptr(), bufs[0][4:].data_ptr(), N, heads, table_rows, nslabs, _st()) == -1109
    assert lib.stswin_bias_scatter(dbias.data_ptr(), order.data_ptr(), None, bufs[0][4:].data_ptr(), N, heads, table_rows, nslabs, _st()) == -1109
    torch.cuda.synchronize()
    assert _same(bufs[0], keep)


# ====================================================================================================== the multi-launch forms
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_linear_pack_multi_is_bitwise_the_single_form(dt):
    """65 weights of different shapes in one call (two launches: 64 + 1), one of them without a transpose."""
    g = torch.Generator().manual_seed(11)
    shapes = [(4, 260), (132, 68), (64, 64), (8, 8), (68, 4), (200, 64), (64, 132)]
    entries, want = [], []
    for i in range(65):
        n, k = shapes[i % len(shapes)]
        w = torch.randn(n, k, generator=g).to(DEV)
        tr = i != 7
        want.append(hip.linear_pack(w, dt, want_tr=tr))
        entries.append((w, torch.full((n, k), NAN, dtype=dt, device=DEV), torch.full((k, n), NAN, dtype=dt, device=DEV) if tr else None))
    hip.linear_pack_multi(entries, dt)
    for i, ((w, fwd, tr), (f1, t1)) in enumerate(zip(entries, want)):
        assert _same(fwd, f1), f"entry {i} {tuple(w.shape)}: W"
        assert (tr is None and t1 is None) or _same(tr, t1), f"entry {i} {tuple(w.shape)}: W^T"


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_conv_pack_multi_is_bitwise_the_single_form(dt):
    """33 convolution weights (1x1 and 3x3, padded channel maps with -1) in one call (32 + 1), one without a dgrad matrix."""
    g = torch.Generator().manual_seed(12)
    entries, want = [], []
    for i in range(33):
        co, ci, k = [(8, 12, 1), (70, 20, 3), (64, 64, 1), (5, 130, 3)][i % 4]
        w = torch.randn(co, ci, k, k, generator=g).to(DEV)
        omap = torch.cat([torch.arange(co // 2), torch.full((3,), -1), torch.arange(co // 2, co), torch.full((1 + i % 3,), -1)]).to(torch.int32).to(DEV)
        imap = torch.cat([torch.full((2,), -1), torch.arange(ci), torch.full((i % 2,), -1)]).to(torch.int32).to(DEV)
        dgrad = i != 5
        want.append(hip.conv_pack(w, dt, omap, imap, want_dgrad=dgrad))
        S, cop, cip = k * k, omap.numel(), imap.numel()
        entries.append((w, torch.full((cop, S * cip), NAN, dtype=dt, device=DEV),
                        torch.full((cip, S * cop), NAN, dtype=dt, device=DEV) if dgrad else None, omap, imap))
    hip.conv_pack_multi(entries, dt)
    for i, (e, (f1, d1)) in enumerate(zip(entries, want)):
        assert _same(e[1], f1), f"entry {i} {tuple(e[0].shape)}: forward matrix"
        assert (e[2] is None and d1 is None) or _same(e[2], d1), f"entry {i} {tuple(e[0].shape)}: dgrad matrix"


def test_bias_expand_multi_is_bitwise_the_single_form():
    """17 tables (16 + 1), N in {16, 64}, some with a mask and some without."""
    g = torch.Generator().manual_seed(13)
    entries, want = [], []
    for i in range(17):
        N, heads = (16, 64)[i % 2], 2 + i % 3
        nW = (0, 2, 3)[i % 3]
        ws = int(N ** 0.5)
        table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).to(DEV)
        index = torch.randint(0, (2 * ws - 1) ** 2, (N * N,), generator=g).to(DEV)
        mask = torch.randn(nW, N, N, generator=g).to(DEV) if nW else None
        want.append(hip.bias_expand(table, index, mask, N, heads))
        entries.append((table, index, mask, torch.full_like(want[-1], NAN), N, heads))
    hip.bias_expand_multi(entries)
    for i, (e, w) in enumerate(zip(entries, want)):
        assert _same(e[3], w), f"entry {i}: N={e[4]} heads={e[5]} mask={'yes' if e[2] is not None else 'no'}"


def test_vec_gather_multi_is_bitwise_the_single_form():
    g = torch.Generator().manual_seed(14)
    n = 300
    imap = torch.randint(-1, 200, (n,), generator=g).to(torch.int32).to(DEV)
    vs = [torch.randn(200, generator=g).to(DEV) for _ in range(4)]
    fills = [0.0, 1.5, -2.0, 7.0]
    want = [hip.vec_gather(v, imap, f) for v, f in zip(vs, fills)]
    got = hip.vec_gather_multi(vs, imap, fills)
    outs = [torch.full((n,), NAN, device=DEV) for _ in range(4)]
    back = hip.vec_gather_multi(vs, imap, fills, outs=outs)
    for k in range(4):
        assert _same(got[k], want[k]) and _same(outs[k], want[k]) and back[k] is outs[k], k
    assert bool((imap < 0).any())
