"""tests/conv_halo_ref.py (the float64 reference, the schedules and the derived bounds of the conv_halo.hip contract) held to independent
definitions on the CPU:
  * the halo forms against float64 F.conv2d / F.conv_transpose2d / torch.nn.grad.conv2d_weight; the general 4 x 4 stem form, fed a
    space-to-depth image and packed weights written here in torch from the header's text, against the float64 7 x 7 / 2 / 3 convolution
    and its weight gradient; headops._stem_pack / _stem_unpack against that packing (checked, not used as the definition);
  * every schedule function against the launcher's expressions, transcribed literally; every case has the properties it records;
  * the bounds hold for an fp32 emulation of each kernel (tap-by-tap fp32 accumulation, residual add, bf16 store, block- / run-wise
    statistics, unit-by-unit slabs and their fold) at EVERY case of conv_halo_ref.cases() - the largest err / bound is printed;
  * the bounds have teeth: nine planted defects, put into that emulation, each leave an element outside TWICE the bound (a kernel with
    the defect also has its own rounding error, up to one bound, which may point the other way) at every case where the defect can
    occur; the least margin per defect is printed.  Where a defect applies:
      bottom halo row not zeroed            conv cases with more than one frame (sign = +1)
      pad column missing                    every conv case (sign = +1)
      input gradient in forward tap order   every conv case (sign = -1)
      residual added after the rounding     every conv case, 'signed' operands (with 'nonneg' operands both roundings stay within one
                                            binade of the result: the double rounding cannot exceed twice half an ulp)
      ring row one lap stale                wgrad / stem cases whose in-frame stretches outgrow the ring (properties: wraps / overwrites)
      first unit after a change dropped     wgrad / stem cases with a run that crosses a frame / strip
      stem t and ch exchanged               every stem case, forward and weight gradient
      statistics from the stored values     every conv / stem case, 'nonneg' operands: A = |ref| there, the derived bound of a table row
                                            is at its tightest relative to the sums and the bf16 rounding errors of 128+ rows add up to
                                            more than twice of it.  With 'signed' operands A is ~15 |ref| and the largest ratio is
                                            0.9 - 1.6 of the bound at the conv cases, 2.5 - 3.3 at the stem cases: not reliably beyond
                                            twice the bound, so it is printed per case instead of asserted or quietly dropped.
      run sums in the wrong table row       every conv / stem case"""
import pytest
import torch
import torch.nn.functional as F

import conv_halo_ref as R

F64, BF = torch.float64, torch.bfloat16
CONV, WGRAD, STEM = R.conv_cases(), R.wgrad_cases(), R.stem_cases()
ident = lambda c: c.name                                   # noqa: E731


# ------------------------------------------------------------------------------------------------------------------ ref == torch
def _nchw(t, Fr, H, W):
    return t.double().view(Fr, H, W, -1).permute(0, 3, 1, 2)


def _tokens(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("Fr,H,W", [(2, 4, 64), (3, 16, 16), (1, 6, 128)])
def test_halo_forms_are_torchs_convolutions(Fr, H, W):
    g = torch.Generator().manual_seed(H)
    x, dy = (torch.randn(Fr * H * W, 64, generator=g).to(BF) for _ in range(2))
    w = torch.randn(64, 64, 3, 3, generator=g).to(BF)
    fwd, dg = R.conv_wmats(w)
    assert torch.equal(fwd.view(64, 9, 64)[5, 7, 3], w[5, 3, 2, 1]) and torch.equal(dg.view(64, 9, 64)[3, 7, 5], w[5, 3, 2, 1])
    xi = _nchw(x, Fr, H, W)
    y, A = R.conv3x3_terms(x, fwd, Fr, H, W, 1)
    assert float((y - _tokens(F.conv2d(xi, w.double(), padding=1))).abs().max()) < 1e-11
    assert bool((A >= y.abs()).all())
    dx, _ = R.conv3x3_terms(x, dg, Fr, H, W, -1)
    assert float((dx - _tokens(F.conv_transpose2d(xi, w.double(), padding=1))).abs().max()) < 1e-11
    s = R.wgrad_schedule(Fr, H, W) if W >= 32 else R.Sched(Fr * H * W // 128, H * W // 128, 1, Fr * H * W // 128, [(u, u + 1) for u in range(Fr * H * W // 128)])
    P, Ab = R.conv3x3_wgrad_partials(dy, x, Fr, H, W, s)
    gw = torch.nn.grad.conv2d_weight(xi, (64, 64, 3, 3), _nchw(dy, Fr, H, W), padding=1)
    assert float((P.sum(0) - gw.permute(0, 2, 3, 1).reshape(64, 576)).abs().max()) < 1e-10
    assert float((R.to_tapminor(P.sum(0), 64) - gw.reshape(64, 576)).abs().max()) < 1e-10       # nn.Conv2d.weight's own layout
    assert bool((Ab.sum(0) >= P.sum(0).abs()).all())


def s2d(img):
    """include/stswin_hip.h, stswin_stem_s2d, in torch: records [F][Ho + 3][Wo + 3][16], record (sy, sx)[(dy*2 + dx)*3 + c] =
    img[c][2(sy-2) + dy][2(sx-2) + dx], zero outside the image, positions 12..15 zero; 64 trailing zeros."""
    Fr, _, H, W = img.shape
    Ho, Wo = R.stem_geometry(H, W)
    big = torch.zeros(Fr, 3, 2 * (Ho + 3), 2 * (Wo + 3), dtype=img.dtype)
    big[:, :, 4:4 + H, 4:4 + W] = img
    rec = torch.zeros(Fr, Ho + 3, Wo + 3, 16, dtype=img.dtype)
    for dy in range(2):
        for dx in range(2):
            rec[..., (dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3] = big[:, :, dy::2, dx::2].permute(0, 2, 3, 1)
    return torch.cat([rec.flatten(), torch.zeros(64, dtype=img.dtype)])


def stem_pack(w):
    """(64, 3, 7, 7) -> [64][4][4][16]: W[co][c][2s + dy - 1][2t + dx - 1] at (s, t, (dy*2 + dx)*3 + c), zero where the window has no tap."""
    out = torch.zeros(w.shape[0], 4, 4, 16, dtype=w.dtype)
    for s in range(4):
        for t in range(4):
            for dy in range(2):
                for dx in range(2):
                    ky, kx = 2 * s + dy - 1, 2 * t + dx - 1
                    if 0 <= ky < 7 and 0 <= kx < 7:
                        out[:, s, t, (dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3] = w[:, :, ky, kx]
    return out.reshape(-1, 256)


@pytest.mark.parametrize("Fr,H,W", [(2, 5, 255), (1, 6, 256), (1, 1, 511)])
def test_general_stem_form_is_the_7x7_stride_2_convolution(Fr, H, W):
    g = torch.Generator().manual_seed(W)
    img = torch.randn(Fr, 3, H, W, generator=g).to(BF)
    w = torch.randn(64, 3, 7, 7, generator=g).to(BF)
    Ho, Wo = R.stem_geometry(H, W)
    dy = torch.randn(Fr * Ho * Wo, 64, generator=g).to(BF)
    rec, wm = s2d(img), stem_pack(w)
    y, _ = R.stem_terms(rec, wm, Fr, H, W)
    want = F.conv2d(img.double(), w.double(), stride=2, padding=3)
    assert want.shape[2:] == (Ho, Wo)
    assert float((y - _tokens(want)).abs().max()) < 1e-11
    P, _ = R.stem_wgrad_partials(dy, rec, Fr, H, W, R.stem_schedule(Fr, H, W))
    gw = torch.nn.grad.conv2d_weight(img.double(), (64, 3, 7, 7), _nchw(dy, Fr, Ho, Wo), stride=2, padding=3)
    dW = P.sum(0)
    window = stem_pack(torch.ones_like(gw)) > 0            # (elsewhere W is structurally zero and its gradient is not conv1's)
    assert int(window.sum()) == 64 * 147 and float(((dW - stem_pack(gw)) * window).abs().max()) < 1e-10
    from stswincl_amd import headops as Hd                  # (importing it needs no GPU)
    assert torch.equal(Hd._stem_pack(w.float(), BF), wm)
    assert float((Hd._stem_unpack(dW) - gw).abs().max()) < 1e-10


# ------------------------------------------------------------------------------------------------------------------ schedules
def _kernel_runs(units, grid, per):
    """The kernels' own expressions: u0 = blockIdx.x * per, u1 = u0 + per < units ? u0 + per : units; u0 >= u1 returns."""
    out = []
    for b in range(grid):
        u0 = b * per
        u1 = u0 + per if u0 + per < units else units
        out.append((u0, u1) if u0 < u1 else None)
    return out


def _tiles_once(s, allow_empty):
    seen = [u for r in s.runs for u in range(*r)]
    assert seen == list(range(s.units)) and len(s.runs) == s.grid
    assert allow_empty or all(b > a for a, b in s.runs)


def test_forward_schedule_is_the_launchers():
    for W in (16, 32, 64, 128):
        for H in range(256 // W, 4096 // W + 1, 256 // W):
            for Fr in (1, 2, 3, 7, 100, 103, 154, 300):
                if Fr * H * W > 300 * 4096:
                    continue
                s = R.fwd_schedule(Fr, H, W)
                ntiles = Fr * H * W // 256                                  # ch_launch: a.M / 256, grid = min(ntiles, 256)
                grid = ntiles if ntiles < 256 else 256
                per = (ntiles + grid - 1) // grid                           # the kernel: (ntiles + gridDim.x - 1) / gridDim.x
                assert (s.units, s.grid, s.per, s.upf) == (ntiles, grid, per, (H * W) >> 8)
                assert [r if r[1] > r[0] else None for r in s.runs] == _kernel_runs(ntiles, grid, per)
                _tiles_once(s, allow_empty=True)


def test_weight_gradient_schedules_are_the_launchers():
    for W in (32, 64, 128):
        for H in range(128 // W, 2048 // W + 1, 128 // W):
            for Fr in (1, 2, 5, 86, 113, 147, 255, 256, 257):
                s = R.wgrad_schedule(Fr, H, W)
                nunits = Fr * H * W // 128
                g0 = nunits if nunits < 256 else 256
                per = (nunits + g0 - 1) // g0
                grid = (nunits + per - 1) // per
                assert (s.units, s.grid, s.per, s.upf) == (nunits, grid, per, (H * W) >> 7)
                assert s.runs == _kernel_runs(nunits, grid, per)            # every workgroup has a unit: every slab is written
                _tiles_once(s, allow_empty=False)
                assert g0 * 64 * 576 >= grid * 64 * 576                     # stswin_conv3x3_c64_wgrad_scratch covers the slabs
    assert [R.ring_slots(w) for w in (128, 64, 32)] == [4, 8, 16]           # ChWg::RING: TYU = 1, 2, 4 -> 4, 8, 16 >= 2 TYU + 2
    for Fr, H, W in ((2, 1, 255), (1, 5, 767), (3, 173, 256), (4, 257, 512), (16, 512, 512), (5, 513, 256)):
        s = R.stem_schedule(Fr, H, W)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        nunits = Fr * (Wo // 128) * Ho
        g0 = nunits if nunits < 256 else 256
        per = (nunits + g0 - 1) // g0
        grid = (nunits + per - 1) // per
        assert (s.units, s.grid, s.per, s.upf) == (nunits, grid, per, Ho) and s.runs == _kernel_runs(nunits, grid, per)
        _tiles_once(s, allow_empty=False)
        # the kernel's unit -> pixel rule, and its statistics runs: a run ends when `next` is false (end of the run or of the strip)
        nxh = Wo >> 7
        pix = R.stem_unit_pixels(Fr, H, W)
        st = []
        for u0, u1 in s.runs:
            start = u0
            for u in range(u0, u1):
                strip, oy = u // Ho, u % Ho
                f, x0 = strip // nxh, (strip % nxh) << 7
                assert int(pix[u, 0]) == (f * Ho + oy) * Wo + x0 and int(pix[u, 127]) == int(pix[u, 0]) + 127
                if not (u + 1 < u1 and oy + 1 < Ho):
                    st.append((start, u + 1))
                    start = u + 1
        assert st == s.stretches()
        assert sorted(pix.flatten().tolist()) == list(range(Fr * Ho * Wo))


@pytest.mark.parametrize("c", R.cases(), ids=ident)
def test_case_has_the_properties_it_records(c):
    have = R.properties(c)
    assert c.props and all(k in have for k, _ in c.props)
    assert {k: have[k] for k, _ in c.props} == dict(c.props), f"{c.name} ({c.why}): the schedule gives {have}"
    pixels = c.F * c.H * c.W if c.kind != "stem" else c.F * have["Ho"] * have["Wo"]
    assert pixels <= 200_000


def test_case_list_is_the_issues():
    by = {c.name: R.properties(c) for c in R.cases()}
    for n in ("conv_3x2x128", "conv_3x4x64", "conv_3x8x32", "conv_3x16x16"):
        assert by[n]["upf"] == 1 and by[n]["per"] == 1
    assert by["conv_300x16x16"]["per"] == 2 and by["conv_300x16x16"]["empty"] == 106
    assert by["conv_6x86x128"]["per"] == 2 and by["conv_6x86x128"]["cross"] > 0
    for n in ("conv_103x10x128", "conv_103x20x64", "conv_103x40x32", "conv_103x80x16"):
        assert (by[n]["units"], by[n]["upf"], by[n]["per"], by[n]["cross"]) == (515, 5, 3, 68) and by[n]["refill0"] > 0 and by[n]["short_last"]
    for n in ("conv_154x10x128", "conv_154x80x16"):
        assert by[n]["per"] == 4 and by[n]["refill1"] > 0
    for n in ("wgrad_86x3x128", "wgrad_86x6x64", "wgrad_86x12x32"):
        assert (by[n]["units"], by[n]["per"], by[n]["cross"]) == (258, 2, 43)
    for n in ("wgrad_147x7x128", "wgrad_147x14x64", "wgrad_147x28x32"):
        assert (by[n]["units"], by[n]["per"], by[n]["cross"], by[n]["wraps"]) == (1029, 5, 117, True)
    assert [by[f"wgrad_{g}x1x128"]["grid"] for g in (1, 15, 16, 17, 48, 49, 64, 65, 113)] == [1, 15, 16, 17, 48, 49, 64, 65, 113]
    assert by["stem_2x1x255"]["Ho"] == 1 and by["stem_2x2x256"]["Ho"] == 1 and by["stem_1x5x767"]["Wo"] == 384
    assert (by["stem_3x173x256"]["Ho"], by["stem_3x173x256"]["per"], by["stem_3x173x256"]["cross"]) == (87, 2, 1)
    assert (by["stem_2x259x512"]["Ho"], by["stem_2x259x512"]["per"], by["stem_2x259x512"]["strips"]) == (130, 3, 2)
    assert (by["stem_4x257x512"]["Ho"], by["stem_4x257x512"]["per"], by["stem_4x257x512"]["cross"]) == (129, 5, 6)


# ------------------------------------------------------------------------------------------------------------------ emulation, defects
@pytest.fixture(scope="module")
def record():
    table = {"emu": {}, "teeth": {}}
    yield table
    print("\n[conv_halo bound] largest err / bound of the fp32 emulation: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(table["emu"].items())))
    for k, (v, name) in sorted(table["teeth"].items()):
        print(f"[conv_halo teeth] {k}: least margin (largest |defect - ref| / bound of a case) {v:.3g} at {name}")


def _note(record, kind, key, ratio, name=None):
    if kind == "emu":
        record["emu"][key] = max(record["emu"].get(key, 0.0), ratio)
    elif key not in record["teeth"] or ratio < record["teeth"][key][0]:
        record["teeth"][key] = (ratio, name)


def _ratio(got, want, bnd):
    return R.worst(got, want, bnd)[0]


def _blocks(M):
    return torch.arange(M).view(M // 128, 128)


def emu_conv_acc(p, c, sign, defect=None):
    """fp32: the taps one after the other onto the accumulator -> [M][64] before the residual."""
    Fr, H, W = c.F, c.H, c.W
    X = p["x"].float().view(Fr, H, W, 64)
    Xp = F.pad(X, (0, 0, 1, 1, 1, 1))
    if defect == "bottom":
        Xp[:-1, H + 1, 1:W + 1] = X[1:, 0]
    if defect == "padcol":
        Xp[:, 1:, 0] = Xp[:, :-1, W].clone()
    wm = (p["fwd"] if sign > 0 else p["dgrad"]).float()
    sg = 1 if defect == "taporder" else sign
    step, out = max(1, 8192 // (H * W)), []              # (whole frames, ~8192 pixels at a time)
    for f0 in range(0, Fr, step):
        acc = torch.zeros(min(step, Fr - f0) * H * W, 64)
        for tap, (dy, dx) in enumerate(R.TAPS):
            acc += Xp[f0:f0 + step, 1 + sg * dy:1 + sg * dy + H, 1 + sg * dx:1 + sg * dx + W].reshape(-1, 64) @ wm[:, tap * 64:(tap + 1) * 64].t()
        out.append(acc)
    return torch.cat(out)


def emu_conv_finish(acc, resid, defect=None):
    """fp32: the residual, the bf16 store, 128-row block sums -> (y bf16, s1, s2)."""
    if resid is not None and defect == "resid_after":
        y = (acc.to(BF).float() + resid.float()).to(BF)
    else:
        if resid is not None:
            acc = acc + resid.float()
        y = acc.to(BF)
    v = y.float() if defect == "stored" else acc
    s1, s2 = v.view(-1, 128, 64).sum(1), (v * v).view(-1, 128, 64).sum(1)
    if defect == "wrongrow":                               # the two blocks of a tile exchanged
        s1, s2 = s1.view(-1, 2, 64).flip(1).reshape(-1, 64), s2.view(-1, 2, 64).flip(1).reshape(-1, 64)
    return y, s1, s2


@pytest.mark.parametrize("c", CONV, ids=ident)
def test_conv3x3_bound_against_emulation_and_defects(c, record):
    M = c.F * c.H * c.W
    ps, pn = R.conv_problem(c, "signed"), R.conv_problem(c, "nonneg")
    refs, accs = {}, {}
    for sign in (1, -1):
        y0, A = R.conv3x3_terms(ps["x"], ps["fwd"] if sign > 0 else ps["dgrad"], c.F, c.H, c.W, sign)
        accs[sign] = emu_conv_acc(ps, c, sign)
        for resid in (None, ps["resid"]):
            ref, Epre, Est = R.out_bound(y0, A, 576, resid)
            st = R.stats_ref_and_bound(ref, Epre, _blocks(M))
            refs[(sign, resid is not None)] = (ref, Est, st)
            y, s1, s2 = emu_conv_finish(accs[sign], resid)
            r = (_ratio(y, ref, Est), _ratio(s1, st[0], st[2]), _ratio(s2, st[1], st[3]))
            assert max(r) < 1.0, f"{c.name} sign {sign} resid {resid is not None}: the emulation leaves the bound: y, sums, squares {r}"
            _note(record, "emu", "conv y", r[0]), _note(record, "emu", "conv sums", r[1]), _note(record, "emu", "conv squares", r[2])
    # ---- planted defects
    ref, Est, st = refs[(1, False)]
    teeth = {}
    if c.F > 1:
        teeth["bottom halo row not zeroed"] = _ratio(emu_conv_acc(ps, c, 1, "bottom").to(BF), ref, Est)
    teeth["pad column missing"] = _ratio(emu_conv_acc(ps, c, 1, "padcol").to(BF), ref, Est)
    teeth["input gradient in forward tap order"] = _ratio(emu_conv_acc(ps, c, -1, "taporder").to(BF), refs[(-1, False)][0], refs[(-1, False)][1])
    teeth["residual added after the rounding"] = _ratio(emu_conv_finish(accs[1], ps["resid"], "resid_after")[0], refs[(1, True)][0], refs[(1, True)][1])
    _, w1, w2 = emu_conv_finish(accs[1], None, "wrongrow")
    teeth["run sums in the wrong table row (conv)"] = max(_ratio(w1, st[0], st[2]), _ratio(w2, st[1], st[3]))
    # statistics from the stored values: 'nonneg' operands (module docstring); the clean emulation holds there too
    y0, A = R.conv3x3_terms(pn["x"], pn["fwd"], c.F, c.H, c.W, 1)
    accn = emu_conv_acc(pn, c, 1)
    for resid in (None, pn["resid"]):
        refn, Epre, Estn = R.out_bound(y0, A, 576, resid)
        stn = R.stats_ref_and_bound(refn, Epre, _blocks(M))
        y, s1, s2 = emu_conv_finish(accn, resid)
        r = (_ratio(y, refn, Estn), _ratio(s1, stn[0], stn[2]), _ratio(s2, stn[1], stn[3]))
        assert max(r) < 1.0, f"{c.name} nonneg resid {resid is not None}: the emulation leaves the bound: {r}"
        _, d1, d2 = emu_conv_finish(accn, resid, "stored")
        teeth[f"statistics from the stored values (conv{', resid' if resid is not None else ''})"] = max(_ratio(d1, stn[0], stn[2]), _ratio(d2, stn[1], stn[3]))
    _, d1, d2 = emu_conv_finish(accs[1], None, "stored")
    print(f"[conv_halo] {c.name}: statistics from the stored values with 'signed' operands: {max(_ratio(d1, st[0], st[2]), _ratio(d2, st[1], st[3])):.3g} "
          "of the bound (not asserted: see the module docstring)")
    for k, v in teeth.items():
        _note(record, "teeth", k, v, c.name)
    short = {k: round(v, 2) for k, v in teeth.items() if not v > 2.0}
    assert not short, f"{c.name}: defects that stay within twice the bound everywhere: {short}"


def _unit_products(DY, B, sched):
    """fp32 [units][64][n]: every unit's 128-pixel product, then each workgroup's slab as the sum over its units one after the other,
    then the fold over slabs in order."""
    n = B.shape[1]
    Uprod = torch.bmm(DY.view(-1, 128, 64).transpose(1, 2), B.view(-1, 128, n))
    slabs = torch.zeros(sched.grid, 64, n)
    for k in range(sched.per):
        part = Uprod[k::sched.per]
        slabs[:part.shape[0]] += part
    tot = torch.zeros(64, n)
    for s in slabs:
        tot += s
    return tot


def _first_after_change(sched):
    return [a for (a, b) in sched.stretches() if a not in {r[0] for r in sched.runs}]


def emu_wgrad(p, c, sched, prev, defect=None):
    Fr, H, W = c.F, c.H, c.W
    X = p["x"].float().view(Fr, H, W, 64)
    B = torch.cat([R.shifted(X, dy, dx).reshape(-1, 64) for dy, dx in R.TAPS], dim=1)
    DY = p["dy"].float().clone()
    if defect == "dropped":
        for u in _first_after_change(sched):
            DY[u * 128:(u + 1) * 128] = 0
    if defect == "stale":
        tyu, ring = 128 // W, R.ring_slots(W)
        Xs = torch.zeros_like(X)
        Xs[:, ring:] = X[:, :H - ring]
        Bs = torch.cat([R.shifted(Xs, dy, dx).reshape(-1, 64) for dy, dx in R.TAPS], dim=1).view(-1, 9, 64)
        B = B.view(-1, 9, 64).clone()
        tapdy = torch.tensor([dy for dy, _ in R.TAPS])
        for a, b in sched.stretches():
            for u in range(a + 1, b):                      # the rows y0 + 1 .. y0 + TYU that arrive for unit u land on slots in use
                if (u - a) * tyu + tyu + 2 > ring:
                    y0 = (u % sched.upf) * tyu
                    rows = y0 + torch.arange(128) // W     # image row of every pixel of the unit
                    m = (rows[:, None] + tapdy[None, :]) >= y0 + 1
                    blk = B[u * 128:(u + 1) * 128]
                    blk[m] = Bs[u * 128:(u + 1) * 128][m]
        B = B.view(-1, 576)
    tot = _unit_products(DY, B, sched)
    return tot if prev is None else prev + tot


@pytest.mark.parametrize("c", WGRAD, ids=ident)
def test_wgrad_bound_against_emulation_and_defects(c, record):
    p, sched = R.wgrad_problem(c), c.schedule()
    P, Ab = R.conv3x3_wgrad_partials(p["dy"], p["x"], c.F, c.H, c.W, sched)
    want = P.sum(0)
    for prev in (None, p["prev"]):
        bnd = R.wgrad_bound(P, Ab, sched, c_prev=prev)
        r = _ratio(emu_wgrad(p, c, sched, prev), want if prev is None else prev.double() + want, bnd)
        assert r < 1.0, f"{c.name}: the emulation leaves the bound: {r}"
        _note(record, "emu", "wgrad", r)
    # tap-minor is a permutation of the same elements (gemm_tn_ref.to_tapminor): bound and defects carry over element by element
    bnd = R.wgrad_bound(P, Ab, sched, c_prev=p["prev"])     # (accumulate: the wider of the two)
    have = R.properties(c)
    teeth = {}
    if have["cross"]:
        teeth["first unit after a frame change dropped (wgrad)"] = _ratio(emu_wgrad(p, c, sched, None, "dropped"), want, bnd)
    if have["wraps"]:
        teeth["ring row one lap stale (wgrad)"] = _ratio(emu_wgrad(p, c, sched, None, "stale"), want, bnd)
    for k, v in teeth.items():
        _note(record, "teeth", k, v, c.name)
    short = {k: round(v, 2) for k, v in teeth.items() if not v > 2.0}
    assert not short, f"{c.name}: defects that stay within twice the bound everywhere: {short}"


def _exchange_t_ch(wm):
    """[..][s][t * 16 + ch] read as [..][s][ch * 4 + t]."""
    return wm.reshape(-1, 4, 4, 16).transpose(2, 3).reshape(-1, 256)


def emu_stem(p, c, sched, defect=None):
    """-> (y bf16, table of sums, table of squares [M / 128][64]) as stem_conv writes them: run sums in the row of the run's first block."""
    Ho, Wo = R.stem_geometry(c.H, c.W)
    M = c.F * Ho * Wo
    Rr = p["rec"][:-64].float().view(c.F, Ho + 3, Wo + 3, 16)
    wm = (_exchange_t_ch(p["w"]) if defect == "exchange" else p["w"]).float().view(64, 4, 4, 16)
    acc = torch.zeros(M, 64)
    for s in range(4):
        for t in range(4):
            acc += Rr[:, s:s + Ho, t:t + Wo].reshape(-1, 16) @ wm[:, s, t].t()
    y = acc.to(BF)
    v = y.float() if defect == "stored" else acc
    units = R.stem_unit_pixels(c.F, c.H, c.W)
    t1, t2 = torch.zeros(M // 128, 64), torch.zeros(M // 128, 64)
    for a, b in sched.stretches():
        rows = units[a:b].flatten()
        row = int(units[a, 0]) // 128
        if defect == "wrongrow":
            row = (row + 1) % (M // 128)
        t1[row] += v[rows].sum(0)
        t2[row] += (v[rows] * v[rows]).sum(0)
    return y, t1, t2


def stem_tables(c, sched, ref, Epre):
    """The float64 table and its bound (0 in the rows that must be exactly 0.0)."""
    Ho, Wo = R.stem_geometry(c.H, c.W)
    rows = c.F * Ho * Wo // 128
    units = R.stem_unit_pixels(c.F, c.H, c.W)
    runs = sched.stretches()
    vals = R.stats_by_runs(ref, Epre, runs, units)
    first = torch.tensor([int(units[a, 0]) // 128 for a, _ in runs])
    out = [torch.zeros(rows, 64, dtype=F64) for _ in range(4)]
    for o, v in zip(out, vals):
        o[first] = v
    return out


def emu_stem_wgrad(p, c, sched, prev, defect=None):
    Ho, Wo = R.stem_geometry(c.H, c.W)
    Rr = p["rec"][:-64].float().view(c.F, Ho + 3, Wo + 3, 16)
    idx = R.stem_unit_pixels(c.F, c.H, c.W).flatten()

    def cols(Rx):
        return torch.cat([Rx[:, s:s + Ho, t:t + Wo].reshape(-1, 16) for s in range(4) for t in range(4)], dim=1)[idx]
    B, DY = cols(Rr), p["dy"].float()[idx].clone()
    if defect == "dropped":
        for u in _first_after_change(sched):
            DY[u * 128:(u + 1) * 128] = 0
    if defect == "stale":                                  # the row oy + 3 that arrives for unit u lands on a slot of its own stretch
        Rs = torch.zeros_like(Rr)
        Rs[:, 8:] = Rr[:, :-8]
        Bs = cols(Rs)
        B = B.clone()
        for a, b in sched.stretches():
            for u in range(a + 5, b):
                B[u * 128:(u + 1) * 128, 192:] = Bs[u * 128:(u + 1) * 128, 192:]
    tot = _unit_products(DY, B, sched)
    if defect == "exchange":
        tot = _exchange_t_ch(tot)
    return tot if prev is None else prev + tot


@pytest.mark.parametrize("c", STEM, ids=ident)
def test_stem_bounds_against_emulation_and_defects(c, record):
    sched, have = c.schedule(), R.properties(c)
    teeth = {}
    for flavour in R.FLAVOURS:
        p = R.stem_problem(c, flavour)
        y0, A = R.stem_terms(p["rec"], p["w"], c.F, c.H, c.W)
        ref, Epre, Est = R.out_bound(y0, A, 256)
        T1, T2, B1, B2 = stem_tables(c, sched, ref, Epre)
        y, t1, t2 = emu_stem(p, c, sched)
        r = (_ratio(y, ref, Est), _ratio(t1, T1, B1), _ratio(t2, T2, B2))
        assert max(r) < 1.0, f"{c.name} {flavour}: the emulation leaves the bound: y, sums, squares {r}"
        _note(record, "emu", "stem y", r[0]), _note(record, "emu", "stem sums", r[1]), _note(record, "emu", "stem squares", r[2])
        _, d1, d2 = emu_stem(p, c, sched, "stored")
        stored = max(_ratio(d1, T1, B1), _ratio(d2, T2, B2))
        if flavour == "nonneg":
            teeth["statistics from the stored values (stem)"] = stored
        else:
            print(f"[conv_halo] {c.name}: statistics from the stored values with 'signed' operands: {stored:.3g} of the bound "
                  "(not asserted: see the module docstring)")
            teeth["stem t and ch exchanged (forward)"] = _ratio(emu_stem(p, c, sched, "exchange")[0], ref, Est)
            _, w1, w2 = emu_stem(p, c, sched, "wrongrow")
            teeth["run sums in the wrong table row (stem)"] = max(_ratio(w1, T1, B1), _ratio(w2, T2, B2))
            # ---- weight gradient
            P, Ab = R.stem_wgrad_partials(p["dy"], p["rec"], c.F, c.H, c.W, sched)
            want = P.sum(0)
            for prev in (None, p["prev"]):
                bnd = R.wgrad_bound(P, Ab, sched, c_prev=prev)
                rr = _ratio(emu_stem_wgrad(p, c, sched, prev), want if prev is None else prev.double() + want, bnd)
                assert rr < 1.0, f"{c.name}: the weight-gradient emulation leaves the bound: {rr}"
                _note(record, "emu", "stem wgrad", rr)
            teeth["stem t and ch exchanged (wgrad)"] = _ratio(emu_stem_wgrad(p, c, sched, None, "exchange"), want, bnd)
            if have["cross"]:
                teeth["first unit after a strip change dropped (stem wgrad)"] = _ratio(emu_stem_wgrad(p, c, sched, None, "dropped"), want, bnd)
            if have["overwrites"]:
                teeth["ring row one lap stale (stem wgrad)"] = _ratio(emu_stem_wgrad(p, c, sched, None, "stale"), want, bnd)
    for k, v in teeth.items():
        _note(record, "teeth", k, v, c.name)
    short = {k: round(v, 2) for k, v in teeth.items() if not v > 2.0}
    assert not short, f"{c.name}: defects that stay within twice the bound everywhere: {short}"
