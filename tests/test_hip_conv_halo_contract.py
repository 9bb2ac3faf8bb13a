"""The four kernels of stswincl_amd/csrc/conv_halo.hip (stswin_conv3x3_c64 forward and input gradient, stswin_conv3x3_c64_wgrad,
stswin_stem_conv, stswin_stem_wgrad) against the float64 contract of tests/conv_halo_ref.py - per ELEMENT, with the derived bounds of
that module (nothing here is tuned on a GPU).  The cases are conv_halo_ref.cases(): the smallest shapes at which each path of the
launcher's schedule runs (tests/test_conv_halo_ref.py asserts every case's properties on the CPU and shows that nine planted defects
land outside twice the bound).

Every case asserts
  * |got - ref| <= bound for every element; a failure names the worst element (frame / y / x / channel, tile or unit, workgroup,
    position in the run - for a gradient: the output element and the workgroup whose partial is nearest to the error) and the number of
    offenders; one line per case is printed with the largest err / bound;
  * the statistics table, NaN-filled before the call: every row up to M / 128 finite; conv3x3_c64: every 128-row block within its
    bound of the sums of the fp32 values BEFORE the bf16 store; stem_conv: per the schedule, the row of a run's first block within the
    bound, the run's other rows exactly 0.0, per-frame sums within the summed bounds;
  * nothing else is written: y, dw and the table sit inside larger buffers filled with a finite sentinel, compared bitwise around
    them; x, dy, rec, wmat and resid are bit-identical afterwards; the weight-gradient scratch is NaN before every launch;
  * a second call gives the same bits; accumulate equals the float64 c_prev + dW within the bound;
  * operands are built by the test from the header's definitions (conv_halo_ref.conv_wmats, a dense record buffer and W); hip.conv_pack
    is held to conv_wmats bitwise on its own; refusals launch nothing and hip.*_ok agree with the launchers."""
import pytest
import torch

import conv_halo_ref as R
import gemm_tn_ref as T
from stswincl_amd import hip

pytestmark = pytest.mark.gpu
F64, BF = torch.float64, torch.bfloat16
DEV = "cuda"
SENT = 12345.0
GUARD = 4096                                               # sentinel elements on either side of every output
NAN = float("nan")
CONV = R.conv_cases()
WGRAD = R.wgrad_cases()
STEM = R.stem_cases()
_REF = {}                                                  # key -> operands and float64 terms: computed once, never changed


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Guarded:
    """A contiguous tensor of `shape` inside a larger flat buffer of a finite sentinel; init: NaN, or the values to start from."""

    def __init__(self, shape, dtype, init=NAN):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.flat = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.view = self.flat[GUARD:GUARD + n].view(*shape)
        if isinstance(init, float):
            self.view.fill_(init)
        else:
            self.view.copy_(init.to(DEV).view(*shape))
        self.sent = _bits(torch.full((1,), SENT, dtype=dtype))[0].item()

    def check_guards(self, what):
        b = _bits(self.flat)
        stray = torch.cat([b[:GUARD], b[GUARD + self.n:]]) != self.sent
        assert not bool(stray.any()), f"{what}: {int(stray.sum())} elements outside the result were written"


def _dev(p):
    return {k: v.to(DEV) for k, v in p.items()}


def _untouched(p, d, tag):
    for k, v in p.items():
        assert torch.equal(_bits(d[k].cpu()), _bits(v)), f"{tag}: operand {k} was written"


def _table(M):
    return Guarded((2, 2 * ((M + 255) // 256), 64), torch.float32)


def _fail_pixel(kind, c, sched, tag, got, want, bnd, fails, what="y"):
    ratio, bad, k = R.worst(got, want, bnd)
    if bad:
        fails.append(f"{tag}: {what}: {bad} of {got.numel()} elements beyond their bound, worst err / bound = {ratio:.3g} at "
                     f"{R.describe_pixel(kind, c, sched, k)}: got {float(got.flatten()[k]):.9g} want {float(want.flatten()[k]):.9g} "
                     f"bound {float(bnd.flatten()[k]):.3g}")
    return ratio


def _fail_rows(tag, what, got, want, bnd, fails, row_names):
    ratio, bad, k = R.worst(got, want, bnd)
    if bad:
        fails.append(f"{tag}: {what}: {bad} of {got.numel()} table elements beyond their bound, worst err / bound = {ratio:.3g} at "
                     f"{row_names(k // 64)} channel {k % 64}: got {float(got.flatten()[k]):.9g} want {float(want.flatten()[k]):.9g} "
                     f"bound {float(bnd.flatten()[k]):.3g}")
    return ratio


# ---------------------------------------------------------------------------------------------------- conv3x3_c64
def _conv_ref(c, sign, flavour):
    key = (c.name, sign, flavour)
    if key not in _REF:
        p = R.conv_problem(c, flavour)
        d = _dev(p)
        y0, A = R.conv3x3_terms(d["x"], d["fwd"] if sign > 0 else d["dgrad"], c.F, c.H, c.W, sign)
        _REF[key] = (p, d, y0, A)
    return _REF[key]


@pytest.mark.parametrize("flavour", R.FLAVOURS)
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("c", CONV, ids=lambda c: c.name)
def test_conv3x3_c64(c, sign, flavour):
    p, d, y0, A = _conv_ref(c, sign, flavour)
    sched = c.schedule()
    M = c.F * c.H * c.W
    wmat = d["fwd"] if sign > 0 else d["dgrad"]
    blocks = torch.arange(M, device=DEV).view(M // 128, 128)
    line, fails = [f"{c.name} sign {sign:+d} {flavour}"], []
    for resid in (None, d["resid"]):
        ref, Epre, Est = R.out_bound(y0, A, 576, resid)
        s1, s2, b1, b2 = R.stats_ref_and_bound(ref, Epre, blocks)
        for stats in (False, True):
            tag = f"{c.name} sign {sign:+d} {flavour} resid={resid is not None} stats={stats}"
            runs = []
            for _ in range(2):
                y, tab = Guarded((M, 64), BF), _table(M) if stats else None
                hip.conv3x3_c64(d["x"], wmat, y.view, c.F, c.H, c.W, sign=sign, resid=resid, stats_out=tab.view if stats else None)
                y.check_guards(tag + " y")
                if stats:
                    tab.check_guards(tag + " table")
                runs.append((y.view.clone(), tab.view.clone() if stats else None))
            got, table = runs[0]
            assert torch.equal(_bits(runs[1][0]), _bits(got)), f"{tag}: a second call gave other output bits"
            assert bool(torch.isfinite(got.float()).all()), f"{tag}: {int((~torch.isfinite(got.float())).sum())} outputs are not finite"
            r = _fail_pixel("conv", c, sched, tag, got, ref, Est, fails)
            line.append(f"{'r' if resid is not None else '-'}{'s' if stats else '-'} y {r:.3f}")
            if stats:
                assert torch.equal(_bits(runs[1][1]), _bits(table)), f"{tag}: a second call gave other table bits"
                assert table.shape[1] == M // 128
                assert bool(torch.isfinite(table).all()), f"{tag}: {int((~torch.isfinite(table)).sum())} table elements were not written"
                name = lambda b: (f"block {b} (tile {b // 2}, workgroup {sched.where(b // 2)[0]}, position "         # noqa: E731
                                  f"{sched.where(b // 2)[1]} of its run)")
                r1 = _fail_rows(tag, "sums", table[0], s1, b1, fails, name)
                r2 = _fail_rows(tag, "sums of squares", table[1], s2, b2, fails, name)
                line.append(f"sum {r1:.3g} sq {r2:.3g}")
    print("[conv_halo] " + "  ".join(line))
    _untouched(p, d, c.name)
    assert not fails, "; ".join(fails)


# ---------------------------------------------------------------------------------------------------- the two weight gradients
def _wgrad_ref(c):
    if c.name not in _REF:
        p = R.wgrad_problem(c)
        d = _dev(p)
        P, Ab = R.conv3x3_wgrad_partials(d["dy"], d["x"], c.F, c.H, c.W, c.schedule())
        _REF[c.name] = (p, d, P, Ab)
    return _REF[c.name]


def _stem_view(rec, c):
    Ho, Wo = R.stem_geometry(c.H, c.W)
    return torch.as_strided(rec, (c.F * (Ho + 3) * (Wo + 3), 64), (16, 1))


def _run_wgrad(c, tag, launch, need, cols, P, Ab, prev, tapminor, line, fails):
    """Overwrite a NaN-filled dw and accumulate onto prev, twice each, through launch(dw, accumulate, scratch, floats) -> rc."""
    sched = c.schedule()
    assert need >= sched.grid * 64 * cols, f"{tag}: the scratch query {need} is below grid * 64 * {cols}"
    st = (lambda X: T.to_tapminor(X, 64)) if tapminor else (lambda X: X)
    Ps, Abs_ = st(P), st(Ab)
    want0 = Ps.sum(0)
    for accumulate in (False, True):
        runs = []
        for _ in range(2):
            dw = Guarded((64, cols), torch.float32, prev if accumulate else NAN)
            ws = Guarded((need,), torch.float32)           # NaN: no stale partial may be read
            rc = launch(dw.view, accumulate, ws.view, need)
            assert rc == 0, f"{tag}: returned {rc}"
            dw.check_guards(tag + " dw")
            ws.check_guards(tag + " scratch")
            runs.append(dw.view.clone())
        got = runs[0]
        t = f"{tag} ({'accumulate' if accumulate else 'overwrite'})"
        assert torch.equal(_bits(runs[1]), _bits(got)), f"{t}: a second call gave other bits"
        assert bool(torch.isfinite(got).all()), f"{t}: {int((~torch.isfinite(got)).sum())} elements are not finite"
        cp = prev.to(DEV) if accumulate else None
        bnd = R.slab_bound(Ps, Abs_, R.row_ranges(sched), c_prev=cp)
        want = want0 if cp is None else cp.double() + want0
        ratio, bad, where = T.worst(got, want, bnd, Ps, tile=64, tapminor_bseg=64 if tapminor else 0)
        line.append(f"{'tm ' if tapminor else ''}{'acc' if accumulate else 'ow'} {ratio:.3g}")
        if bad:
            fails.append(f"{t}: {bad} of {got.numel()} elements beyond their bound, worst err / bound = {ratio:.3g} at {where} "
                         f"(split = workgroup, {sched.per} units each)")


@pytest.mark.parametrize("c", WGRAD, ids=lambda c: c.name)
def test_conv3x3_c64_wgrad(c):
    p, d, P, Ab = _wgrad_ref(c)
    lib = hip.load()
    need = lib.stswin_conv3x3_c64_wgrad_scratch(c.F, c.H, c.W)
    line, fails = [c.name], []
    for tapminor in (False, True):
        def launch(dw, accumulate, ws, floats):
            return lib.stswin_conv3x3_c64_wgrad(d["dy"].data_ptr(), d["x"].data_ptr(), dw.data_ptr(), 1 if tapminor else 0,
                                                1 if accumulate else 0, ws.data_ptr(), floats, c.F, c.H, c.W, hip._stream())
        _run_wgrad(c, f"{c.name} tapminor={tapminor}", launch, need, 576, P, Ab, p["prev"], tapminor, line, fails)
    print("[conv_halo] " + "  ".join(line))
    _untouched(p, d, c.name)
    assert not fails, "; ".join(fails)


def _stem_ref(c, flavour):
    key = (c.name, flavour)
    if key not in _REF:
        p = R.stem_problem(c, flavour)
        d = _dev(p)
        y0, A = R.stem_terms(d["rec"], d["w"], c.F, c.H, c.W)
        _REF[key] = (p, d, y0, A)
    return _REF[key]


@pytest.mark.parametrize("c", STEM, ids=lambda c: c.name)
def test_stem_wgrad(c):
    p, d, _, _ = _stem_ref(c, "signed")
    key = (c.name, "wgrad")
    if key not in _REF:
        _REF[key] = R.stem_wgrad_partials(d["dy"], d["rec"], c.F, c.H, c.W, c.schedule())
    P, Ab = _REF[key]
    lib = hip.load()
    Ho, Wo = R.stem_geometry(c.H, c.W)
    need = lib.stswin_stem_wgrad_scratch(c.F, Ho, Wo)
    line, fails = [c.name + " wgrad"], []

    def launch(dw, accumulate, ws, floats):
        return lib.stswin_stem_wgrad(d["dy"].data_ptr(), d["rec"].data_ptr(), dw.data_ptr(), 1 if accumulate else 0, ws.data_ptr(), floats,
                                     c.F, c.H, c.W, hip._stream())
    _run_wgrad(c, c.name + " wgrad", launch, need, 256, P, Ab, p["prev"], False, line, fails)
    print("[conv_halo] " + "  ".join(line))
    _untouched(p, d, c.name)
    assert not fails, "; ".join(fails)


# ---------------------------------------------------------------------------------------------------- stem_conv
@pytest.mark.parametrize("flavour", R.FLAVOURS)
@pytest.mark.parametrize("c", STEM, ids=lambda c: c.name)
def test_stem_conv(c, flavour):
    p, d, y0, A = _stem_ref(c, flavour)
    sched = c.schedule()
    Ho, Wo = R.stem_geometry(c.H, c.W)
    M = c.F * Ho * Wo
    ref, Epre, Est = R.out_bound(y0, A, 256)
    units = R.stem_unit_pixels(c.F, c.H, c.W, DEV)
    runs_ = sched.stretches()
    s1, s2, b1, b2 = R.stats_by_runs(ref, Epre, runs_, units)
    blk = (units[:, 0] // 128).cpu()                       # table row of every unit
    first = torch.tensor([int(blk[u0]) for u0, _ in runs_])
    others = torch.tensor([int(blk[u]) for u0, u1 in runs_ for u in range(u0 + 1, u1)], dtype=torch.long)
    frame_of_run = torch.tensor([int(units[u0, 0]) // (Ho * Wo) for u0, _ in runs_], device=DEV)
    Arec = _stem_view(d["rec"], c)
    line, fails = [f"{c.name} {flavour}"], []
    for stats in (False, True):
        tag = f"{c.name} {flavour} stats={stats}"
        runs = []
        for _ in range(2):
            y, tab = Guarded((M, 64), BF), _table(M) if stats else None
            hip.stem_conv(Arec, d["w"], y.view, c.F, c.H, c.W, stats_out=tab.view if stats else None)
            y.check_guards(tag + " y")
            if stats:
                tab.check_guards(tag + " table")
            runs.append((y.view.clone(), tab.view.clone() if stats else None))
        got, table = runs[0]
        assert torch.equal(_bits(runs[1][0]), _bits(got)), f"{tag}: a second call gave other output bits"
        r = _fail_pixel("stem", c, sched, tag, got, ref, Est, fails)
        line.append(f"{'s' if stats else '-'} y {r:.3f}")
        if stats:
            assert torch.equal(_bits(runs[1][1]), _bits(table)), f"{tag}: a second call gave other table bits"
            used = table[:, :M // 128]
            assert bool(torch.isfinite(used).all()), f"{tag}: {int((~torch.isfinite(used)).sum())} table elements up to row M / 128 were not written"
            assert bool(torch.isnan(table[:, M // 128:]).all()), f"{tag}: a table row past M / 128 was written"
            z = used[:, others.to(DEV)]
            assert bool((z == 0).all()), f"{tag}: {int((z != 0).sum())} elements of the rows after a run's first block are not 0.0"
            name = lambda i: (f"run {i} (units {runs_[i][0]}..{runs_[i][1] - 1}, workgroup {sched.where(runs_[i][0])[0]}, from position "  # noqa: E731
                              f"{sched.where(runs_[i][0])[1]} of its run, table row {int(first[i])})")
            r1 = _fail_rows(tag, "run sums", used[0][first.to(DEV)], s1, b1, fails, name)
            r2 = _fail_rows(tag, "run sums of squares", used[1][first.to(DEV)], s2, b2, fails, name)
            # per frame: what the table's consumers add up
            rows_pf = M // 128 // c.F
            got_f = used.double().view(2, c.F, rows_pf, 64).sum(2)
            fsum = lambda v: torch.zeros(c.F, 64, dtype=F64, device=DEV).index_add_(0, frame_of_run, v)      # noqa: E731
            fname = lambda f: f"frame {f}"                                                                   # noqa: E731
            _fail_rows(tag, "frame sums", got_f[0], fsum(s1), fsum(b1), fails, fname)
            _fail_rows(tag, "frame sums of squares", got_f[1], fsum(s2), fsum(b2), fails, fname)
            line.append(f"sum {r1:.3g} sq {r2:.3g}")
    print("[conv_halo] " + "  ".join(line))
    _untouched(p, d, c.name)
    assert not fails, "; ".join(fails)


# ---------------------------------------------------------------------------------------------------- operands of the library's own
def test_conv_pack_makes_the_matrices_of_the_header():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 64, 3, 3, generator=g)
    ident = torch.arange(64, dtype=torch.int32, device=DEV)
    fwd, dg = hip.conv_pack(w.to(DEV), BF, ident, ident)
    wf, wd = R.conv_wmats(w)
    assert torch.equal(_bits(fwd.cpu()), _bits(wf.to(BF))), "conv_pack fwd is not [cout][tap][cin]"
    assert torch.equal(_bits(dg.cpu()), _bits(wd.to(BF))), "conv_pack dgrad is not [cin][tap][cout]"


# ---------------------------------------------------------------------------------------------------- refusals launch nothing
def _pixels(n):
    return torch.randn(n, 64, generator=torch.Generator().manual_seed(n)).to(BF).to(DEV)


def test_conv3x3_c64_refusals_and_ok():
    lib = hip.load()
    x, wm = _pixels(8192), torch.randn(64, 576, generator=torch.Generator().manual_seed(1)).to(BF).to(DEV)
    for H in (1, 2, 3, 4, 8, 16, 32):
        for W in (8, 16, 24, 32, 48, 64, 96, 128, 256):
            y, tab = Guarded((H * W, 64), BF, SENT), Guarded((2, 2 * ((H * W + 255) // 256), 64), torch.float32, SENT)
            rc = lib.stswin_conv3x3_c64(x.data_ptr(), wm.data_ptr(), y.view.data_ptr(), None, tab.view.data_ptr(), 1, H, W, 1, hip._stream())
            ok = hip.conv3x3_c64_ok(1, H, W, 64, 64, 3, 1, 1, 1, BF)
            want = 0 if ok else -1701 if (H * W) % 256 else -1702
            assert rc == want, f"H {H} W {W}: returned {rc}, expected {want} (conv3x3_c64_ok says {ok})"
            if not ok:
                sent = torch.full((1,), SENT, dtype=BF)
                assert bool((_bits(y.flat) == _bits(sent)[0].item()).all()), f"H {H} W {W}: refused, yet y was written"
                assert bool((tab.flat == SENT).all()), f"H {H} W {W}: refused, yet the table was written"
    for args in ((0, 2, 128, 1), (1, 2, 128, 0), (1, 2, 128, 3), (1, 0, 128, 1)):
        y = Guarded((256, 64), BF, SENT)
        assert lib.stswin_conv3x3_c64(x.data_ptr(), wm.data_ptr(), y.view.data_ptr(), None, None, *args, hip._stream()) == -1701
        assert bool((y.flat.float() == torch.full((1,), SENT, dtype=BF).float().item()).all())


def test_conv3x3_c64_wgrad_refusals_and_ok():
    lib = hip.load()
    dy, x = _pixels(4096), _pixels(4097)[:4096]

    def call(H, W, dw, ws, floats, frames=1):
        return lib.stswin_conv3x3_c64_wgrad(dy.data_ptr(), x.data_ptr(), dw, 0, 0, ws, floats, frames, H, W, hip._stream())
    for H in (1, 2, 3, 4, 8, 16):
        for W in (8, 16, 24, 32, 48, 64, 96, 128, 256):
            need = max(lib.stswin_conv3x3_c64_wgrad_scratch(1, H, W), 64 * 576)
            dw, ws = Guarded((64, 576), torch.float32, SENT), Guarded((need,), torch.float32)
            rc = call(H, W, dw.view.data_ptr(), ws.view.data_ptr(), need)
            ok = hip.conv3x3_c64_wgrad_ok(1, H, W)
            want = 0 if ok else -1711 if (H * W) % 128 else -1712
            assert rc == want, f"H {H} W {W}: returned {rc}, expected {want} (conv3x3_c64_wgrad_ok says {ok})"
            if not ok:
                assert bool((dw.flat == SENT).all()) and bool(torch.isnan(ws.view).all()), f"H {H} W {W}: refused, yet something was written"
    need = lib.stswin_conv3x3_c64_wgrad_scratch(1, 4, 128)
    assert need == 4 * 64 * 576
    dw, ws = Guarded((64, 576), torch.float32, SENT), Guarded((need,), torch.float32)
    for rc, want in ((call(4, 128, dw.view.data_ptr(), ws.view.data_ptr(), need - 1), -1713), (call(4, 128, dw.view.data_ptr(), None, need), -1713),
                     (call(4, 128, None, ws.view.data_ptr(), need), -1711), (call(4, 128, dw.view.data_ptr(), ws.view.data_ptr(), need, frames=0), -1711)):
        assert rc == want, f"returned {rc}, expected {want}"
    assert bool((dw.flat == SENT).all()) and bool(torch.isnan(ws.view).all()), "refused, yet something was written"


def test_stem_refusals_and_ok():
    lib = hip.load()
    g = torch.Generator().manual_seed(2)
    wm = torch.randn(64, 256, generator=g).to(BF).to(DEV)
    for H in (1, 2, 5):
        for W in (253, 254, 255, 256, 257, 258, 383, 384, 385, 511, 512, 513):
            Ho, Wo = R.stem_geometry(H, W)
            rec = torch.randn((Ho + 3) * (Wo + 3) * 16 + 64, generator=g).to(BF).to(DEV)
            dy = _pixels(Ho * Wo)
            ok = hip.stem_wgrad_ok(H, W, BF)
            assert ok == (Wo % 128 == 0)
            y = Guarded((Ho * Wo, 64), BF, SENT)
            rc = lib.stswin_stem_conv(rec.data_ptr(), wm.data_ptr(), y.view.data_ptr(), None, 1, H, W, hip._stream())
            assert rc == (0 if ok else -1732), f"stem_conv H {H} W {W}: returned {rc} (stem_wgrad_ok says {ok})"
            need = max(lib.stswin_stem_wgrad_scratch(1, Ho, Wo), 64 * 256)
            dw, ws = Guarded((64, 256), torch.float32, SENT), Guarded((need,), torch.float32)
            rc = lib.stswin_stem_wgrad(dy.data_ptr(), rec.data_ptr(), dw.view.data_ptr(), 0, ws.view.data_ptr(), need, 1, H, W, hip._stream())
            assert rc == (0 if ok else -1722), f"stem_wgrad H {H} W {W}: returned {rc} (stem_wgrad_ok says {ok})"
            if not ok:
                assert bool((y.flat.float() == y.flat.float()[0]).all()), f"H {H} W {W}: stem_conv refused, yet y was written"
                assert bool((dw.flat == SENT).all()) and bool(torch.isnan(ws.view).all()), f"H {H} W {W}: stem_wgrad refused, yet something was written"
    H, W = 5, 256
    Ho, Wo = R.stem_geometry(H, W)
    rec, dy = torch.randn((Ho + 3) * (Wo + 3) * 16 + 64, generator=g).to(BF).to(DEV), _pixels(Ho * Wo)
    need = lib.stswin_stem_wgrad_scratch(1, Ho, Wo)
    assert need == Ho * 64 * 256
    dw, ws = Guarded((64, 256), torch.float32, SENT), Guarded((need,), torch.float32)

    def call(dwp, wsp, floats, frames=1):
        return lib.stswin_stem_wgrad(dy.data_ptr(), rec.data_ptr(), dwp, 0, wsp, floats, frames, H, W, hip._stream())
    for rc, want in ((call(dw.view.data_ptr(), ws.view.data_ptr(), need - 1), -1723), (call(dw.view.data_ptr(), None, need), -1723),
                     (call(None, ws.view.data_ptr(), need), -1721), (call(dw.view.data_ptr(), ws.view.data_ptr(), need, frames=0), -1721)):
        assert rc == want, f"stem_wgrad returned {rc}, expected {want}"
    assert bool((dw.flat == SENT).all()) and bool(torch.isnan(ws.view).all()), "stem_wgrad refused, yet something was written"
    assert lib.stswin_stem_conv(rec.data_ptr(), wm.data_ptr(), None, None, 1, H, W, hip._stream()) == -1731
    assert lib.stswin_stem_conv(rec.data_ptr(), wm.data_ptr(), dw.view.data_ptr(), None, 0, H, W, hip._stream()) == -1731
    assert bool((dw.flat == SENT).all())
