"""tests/rowops_ref.py on the CPU: the float64 references against float64 autograd through F.layer_norm (accumulate and gathered forms
included), the geometry function against a transcription of the launcher's rule at every switch point, the derived bounds against an fp32
emulation of each kernel's documented association (a condition: err / bound < 1 at every case) and against planted defects (each at least one
element outside the bound at every case it applies to; the counts are printed)."""
import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R
from oracle import stswin_oracle as O

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
EPS = 1e-5
IDX = torch.arange(64)


def _gen(*k):
    return torch.Generator().manual_seed(abs(hash(tuple(str(x) for x in k))) % (1 << 31))


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def lanes(X, pk):
    """[M][C] -> [M][pieces][64][pk], zeros past C (adding a zero is exact: the same as the kernel's skipped lanes)."""
    M, C = X.shape
    P = R.pieces(C, pk)
    out = torch.zeros(M, P * 64 * pk, dtype=X.dtype)
    out[:, :C] = X
    return out.view(M, P, 64, pk)


def row_sum(X, pk):
    """A lane adds the elements of its pieces in order; six butterfly levels (a + b == b + a: every lane ends with the same bits)."""
    T = lanes(X, pk)
    acc = torch.zeros(X.shape[0], 64, dtype=F32)
    for p in range(T.shape[1]):
        for e in range(pk):
            acc = acc + T[:, p, :, e]
    for d in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[:, IDX ^ d]
    return acc[:, 0]


def emu_fwd(x, gamma, beta, eps, dtype, rows, S, Cseg, M):
    pk = R.pack_of(dtype)
    X = R.gathered(x, rows, M, S, Cseg).float()
    C = torch.tensor(float(S * Cseg), dtype=F32)
    mu = row_sum(X, pk) / C
    d = X - mu[:, None]
    rs = torch.rsqrt(row_sum(d * d, pk) / C + torch.tensor(eps, dtype=F32))
    y = (d * rs[:, None] * gamma + beta).to(dtype)
    return y, mu, rs


def emu_fold(slabs, old=None):
    """slab_fold_kernel: lane q adds the slabs q, q + QL, ... onto zero; lane 0 adds the lane sums in lane order; then old + a."""
    ns, n = slabs.shape
    ql = R.fold_ql(ns)
    V = torch.zeros(-(-ns // ql) * ql, n, dtype=F32)
    V[:ns] = slabs
    V = V.view(-1, ql, n)
    a = torch.zeros(ql, n, dtype=F32)
    for j in range(V.shape[0]):
        a = a + V[j]
    t = a[0]
    for k in range(1, ql):
        t = t + a[k]
    return t if old is None else old + t


def emu_param_sum(terms, geometry, old):
    """ln_bwd_kernel's parameter gradients: a wave adds its rows in order, over every row group its workgroup walks; the waves are added in
    order; one slab per workgroup; the fold."""
    rpw, nw, groups, grid = geometry
    M, C = terms.shape
    K = -(-groups // grid)
    T = torch.zeros(K * grid * nw * rpw, C, dtype=F32)
    T[:M] = terms
    T = T.view(K, grid, nw, rpw, C)
    acc = torch.zeros(grid, nw, C, dtype=F32)
    for k in range(K):
        for i in range(rpw):
            acc = acc + T[k, :, :, i]
    slab = acc[:, 0]
    for w in range(1, nw):
        slab = slab + acc[:, w]
    return emu_fold(slab, old)


def emu_bwd(dy, x, gamma, mean, rstd, dtype, rows, S, Cseg, M, add, old):
    pk = R.pack_of(dtype)
    C = S * Cseg
    X = R.gathered(x, rows, M, S, Cseg).float()
    d = dy.float()
    mu, rs = mean[:, None], rstd[:, None]
    xh = (X - mu) * rs
    g = d * gamma
    Cf = torch.tensor(float(C), dtype=F32)
    s1 = (row_sum(g, pk) / Cf)[:, None]
    s2 = (row_sum(g * xh, pk) / Cf)[:, None]
    val = rs * (g - s1 - xh * s2)
    fin = val if add is None else R.gathered(add, rows, M, S, Cseg).float() + val
    geo = R.ln_bwd_geometry(M, C, pk)
    return (fin.to(dtype), emu_param_sum(d * xh, geo, old["dgamma"]), emu_param_sum(d, geo, old["dbeta"]), emu_param_sum(fin, geo, old["dxsum"]))


def emu_colsum(y, M, old):
    N = y.shape[1]
    nb = -(-M // 512)
    Y = torch.zeros(nb * 512, N, dtype=F32)
    Y[:M] = y[:M].float()
    Y = Y.view(nb, 64, 8, N)                                # row r0 + rl + 8 i
    acc = torch.zeros(nb, 8, N, dtype=F32)
    for i in range(64):
        acc = acc + Y[:, i]
    t = torch.zeros(nb, N, dtype=F32)
    for k in range(8):
        t = t + acc[:, k]
    return emu_fold(t, old)


# ------------------------------------------------------------------------------------------------------------------ references vs autograd
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("form", ["plain", "accumulate", "gather", "gather+add"])
def test_references_agree_with_float64_autograd(dtype, form):
    g = _gen(form, dtype)
    gather = form.startswith("gather")
    if gather:
        fr, H, W, Cseg, S = 2, 4, 6, 24, 4
        x = R.make_x("normal", fr * H * W, Cseg, dtype, g)
        rows = R.merge_rows(fr, H, W)
        M = fr * H * W // 4
        ids = torch.arange(fr * H * W, dtype=F32).reshape(1, fr, H * W, 1)
        assert torch.equal(rows, O.patch_merge_gather(ids, H, W).reshape(-1, 4).t().contiguous().flatten().to(torch.int32))
    else:
        M, Cseg, S, rows = 37, 264, 1, None
        x = R.make_x("normal", M, Cseg, dtype, g)
    C = S * Cseg
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g).to(dtype)
    add = torch.randn(x.shape[0], Cseg, generator=g).to(dtype) if "a" in form.replace("gather", "") else None
    xr = x.to(F64).requires_grad_(True)
    gr, br = gamma.to(F64).requires_grad_(True), beta.to(F64).requires_grad_(True)
    Xr = O.patch_merge_gather(xr.view(1, 2, -1, Cseg), 4, 6).reshape(M, C) if gather else xr
    yr = F.layer_norm(Xr, (C,), gr, br, R.eps32(EPS))
    (yr * dy.to(F64)).sum().backward()
    y, mean, var, rstd = R.ln_forward(x, gamma, beta, EPS, rows, S, Cseg)
    assert torch.allclose(y, yr.detach(), rtol=1e-12, atol=1e-12)
    dx, dg, db, dxs = R.ln_backward(dy, x, gamma, mean, rstd, rows, S, Cseg, add=add)
    want = xr.grad + (add.to(F64) if add is not None else 0)
    assert not bool(torch.isnan(dx).any()), "the merge map names every source row"
    assert torch.allclose(dx, want, rtol=1e-11, atol=1e-11)
    assert torch.allclose(dg, gr.grad, rtol=1e-11, atol=1e-11) and torch.allclose(db, br.grad, rtol=1e-11, atol=1e-11)
    full = R.gathered(want, rows, M, S, Cseg)
    assert torch.allclose(dxs, full.sum(0), rtol=1e-11, atol=1e-11)


def test_scatter_marks_rows_no_map_entry_names():
    rows = torch.tensor([3, 1, 5, 0], dtype=torch.int32)          # S = 2, M = 2
    full = torch.arange(8, dtype=F64).view(2, 4)
    out = R.scatter(full, rows, 2, 2, 7)
    assert torch.isnan(out[[2, 4, 6]]).all() and torch.equal(out[3], full[0, :2]) and torch.equal(out[0], full[1, 2:])
    assert torch.equal(R.gathered(out, rows, 2, 2, 2), full)


def test_sum_references():
    g = _gen("sums")
    ws = torch.randn(3 * 1000 + 50, generator=g)
    got = R.fold(ws, 40, 1000, 20, 12, 3, 3)
    for s in range(3):
        for b in range(3):
            want = sum(ws[b * 1000 + p * 40 + s * 12:b * 1000 + p * 40 + s * 12 + 12].double() for p in range(20))
            assert torch.allclose(got[s, b], want, rtol=1e-13, atol=1e-13)
    N, heads, rows_t = 4, 2, 9
    index = torch.randint(0, rows_t, (N * N,), generator=g)
    d = torch.randn(3, heads, N, N, generator=g)
    out, ab, cnt = R.bias_scatter(d, index, rows_t, 3)
    want = torch.zeros(rows_t, heads, dtype=F64)
    for i in range(N):
        for j in range(N):
            want[index[i * N + j]] += d[:, :, j, i].double().sum(0)
    assert torch.allclose(out, want, rtol=1e-13, atol=1e-13) and int(cnt.sum()) == N * N


# ------------------------------------------------------------------------------------------------------------------ geometry
def _rule(M, C, pk):
    """Transcribed from rowops.hip (ln_bwd_rows_per_wave, ln_bwd_waves without its A/B switch, ln_bwd_grid)."""
    np_ = (C // pk + 63) // 64
    rpw = 8 if M >= 16384 else (4 if M >= 4096 else 2)
    nw = 8 if ((M + 4 * rpw - 1) // (4 * rpw) <= 512 and M >= 8 * rpw * 128 and np_ <= 2) else 4
    groups = (M + nw * rpw - 1) // (nw * rpw)
    return rpw, nw, groups, (groups if groups < 1024 else 1024)


def test_geometry_at_every_switch_point():
    pts = [1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, 32800, 65536]
    seen = set()
    for M in pts:
        for C, pk in ((64, 8), (64, 4), (1024, 8), (1032, 8), (512, 4), (516, 4), (1536, 8), (3272, 8)):
            assert R.ln_bwd_geometry(M, C, pk) == _rule(M, C, pk), (M, C, pk)
            seen.add(R.ln_bwd_geometry(M, C, pk)[:2])
    assert seen == {(2, 4), (2, 8), (4, 8), (4, 4), (8, 8), (8, 4)}
    want = {2047: (2, 4), 2048: (2, 8), 4095: (2, 8), 4096: (4, 8), 8192: (4, 8), 8193: (4, 4), 16383: (4, 4), 16384: (8, 8), 16385: (8, 4),
            32768: (8, 4)}
    for M, rw in want.items():
        assert R.ln_bwd_geometry(M, 64, 8)[:2] == rw, M
    assert R.ln_bwd_geometry(32768, 64, 8)[2:] == (1024, 1024) and R.ln_bwd_geometry(32769, 64, 8)[2:] == (1025, 1024)
    assert R.ln_bwd_geometry(2050, 1536, 8)[1] == 4 and R.ln_bwd_geometry(2050, 64, 8)[1] == 8
    assert {c.geometry[:2] for c in R.cases_bwd()} == seen, "the case list shows all six geometries"
    for c in R.cases_bwd():
        assert c.geometry[3] * 3 * c.C <= R.ln_bwd_scratch(c.M, c.C)
    assert R.np_inst(4104, 8) == 16 and R.np_inst(2052, 4) == 16 and R.np_inst(4100, 4) is None and R.np_inst(2052, 4, True) is None
    assert {c.NP for c in R.cases_fwd()} == {1, 2, 4, 8, 16} and {c.NP for c in R.cases_bwd()} == {1, 2, 4, 8}
    assert {(c.QL, min(c.loops4, 2)) for c in R.cases_fold()} == {(16, 0), (16, 1), (64, 0), (64, 1), (64, 2)}


# ------------------------------------------------------------------------------------------------------------------ emulation within bound
@pytest.mark.parametrize("c", R.cases_fwd(), ids=lambda c: c.name.replace(" ", "_"))
def test_forward_emulation_within_bound_and_defects_outside(c):
    x, gamma, beta, rows = R.fwd_operands(c)
    Cseg = c.Cseg or c.C
    y, mean, var, rstd = R.ln_forward(x, gamma, beta, EPS, rows, c.S, Cseg, c.M)
    b = R.fwd_bound(x, gamma, beta, EPS, c.dtype, rows, c.S, Cseg, c.M)
    ey, emu, ers = emu_fwd(x, gamma, beta, EPS, c.dtype, rows, c.S, Cseg, c.M)
    pk = R.pack_of(c.dtype)
    ratios = [R.worst(ey, y, b["y"], pk), R.worst(emu, mean, b["mean"]), R.worst(ers, rstd, b["rstd"])]
    print(f"[rowops-emu] fwd {c.name} NP={c.NP}: y {ratios[0][0]:.3f} mean {ratios[1][0]:.3f} rstd {ratios[2][0]:.3f}")
    for (ratio, bad, where), what in zip(ratios, ("y", "mean", "rstd")):
        assert bad == 0 and ratio < 1, f"{c.name}: emulated {what} beyond its bound: {bad} elements, worst {ratio:.3g} at {where}"

    def outside(yy, mm, rr):
        return R.worst(yy, y, b["y"])[1] + R.worst(mm, mean, b["mean"])[1] + R.worst(rr, rstd, b["rstd"])[1]

    X = R.gathered(x, rows, c.M, c.S, Cseg)
    e32 = R.eps32(EPS)
    found = {}
    m2 = X[:, :-1].mean(1) if c.C > 1 else X.mean(1)                              # a column dropped from the statistics
    v2 = ((X[:, :-1] - m2[:, None]) ** 2).mean(1)
    r2 = (v2 + e32) ** -0.5
    found["column dropped"] = outside((X - m2[:, None]) * r2[:, None] * gamma.double() + beta.double(), m2, r2)
    found["gamma shifted"] = R.worst((X - mean[:, None]) * rstd[:, None] * gamma.double().roll(1) + beta.double(), y, b["y"])[1]
    if c.regime == "offset300":                                                   # one-pass variance, in fp32 as a kernel would
        Xf = X.float()
        m1 = row_sum(Xf, pk) / c.C
        v1 = row_sum(Xf * Xf, pk) / c.C - m1 * m1
        found["one-pass variance (rstd)"] = R.worst(torch.rsqrt(v1.clamp(min=0) + EPS), rstd, b["rstd"])[1]
    if c.regime == "const":
        found["eps = 1e-6 (rstd)"] = R.worst((var + 1e-6) ** -0.5, rstd, b["rstd"])[1]
    if rows is not None:
        wrong = rows.view(c.S, c.M).roll(-1, 0).flatten()
        y3, m3, _, r3 = R.ln_forward(x, gamma, beta, EPS, wrong, c.S, Cseg, c.M)
        found["segment through the next map"] = outside(y3, m3, r3)
    print(f"[rowops-defect] fwd {c.name}: " + ", ".join(f"{k}: {v}" for k, v in found.items()))
    for k, v in found.items():
        assert v >= 1, f"{c.name}: the planted defect '{k}' stays inside the bound"


_MEAN_RSTD = {}


@pytest.mark.parametrize("c", R.cases_bwd(), ids=lambda c: c.name.replace(" ", "_"))
def test_backward_emulation_within_bound_and_defects_outside(c):
    x, gamma, dy, add, rows, n_src = R.bwd_operands(c)
    Cseg = c.Cseg or c.C
    pk = R.pack_of(c.dtype)
    _, mean, rstd = emu_fwd(x, gamma, torch.zeros(c.C), EPS, c.dtype, rows, c.S, Cseg, c.M)       # fp32 statistics, as the kernel would get
    g = R.seed(c)
    old = {k: torch.randn(c.C, generator=g) for k in ("dgamma", "dbeta", "dxsum")}
    core = R.bwd_core(dy, x, gamma, mean, rstd, rows, c.S, Cseg, c.M)
    line = [f"[rowops-emu] bwd {c.name} geometry={c.geometry}:"]
    for a in (None, add):
        dx, dg, db, dxs = R.ln_backward(dy, x, gamma, mean, rstd, rows, c.S, Cseg, add=a, n_src=n_src, core=core)
        b = R.bwd_bound(core, c.dtype, c.M, rows, a, n_src, old)
        edx, edg, edb, edxs = emu_bwd(dy, x, gamma, mean, rstd, c.dtype, rows, c.S, Cseg, c.M, a, old)
        edx = R.scatter(edx.double(), rows, c.S, Cseg, n_src)
        for got, want, bnd, what in ((edx, dx, b["dx"], "dx"), (edg, old["dgamma"].double() + dg, b["dgamma"], "dgamma"),
                                     (edb, old["dbeta"].double() + db, b["dbeta"], "dbeta"), (edxs, old["dxsum"].double() + dxs, b["dxsum"], "dxsum")):
            ratio, bad, where = R.worst(got, want, bnd, pk)
            line.append(f"{'acc' if a is not None else 'ow'} {what} {ratio:.3f}")
            assert bad == 0 and ratio < 1, f"{c.name}: emulated {what} beyond its bound: {bad} elements, worst {ratio:.3g} at {where}"
    print(" ".join(line))
    # planted defects, judged with the accumulate form's reference and bound (dx, b and the sums of the last pass)
    found = {}
    t = core["d"] * core["xh"]
    found["last row missing from dgamma"] = R.worst(old["dgamma"].double() + t[:-1].sum(0), old["dgamma"].double() + dg, b["dgamma"])[1]
    rpw, nw, groups, grid = c.geometry
    if groups > grid:
        keep = torch.ones(c.M, dtype=torch.bool)
        for blk in range(groups - grid):                                          # these workgroups walk a second group: the first is lost
            keep[blk * nw * rpw:(blk + 1) * nw * rpw] = False
        found["second row group overwrites the first"] = R.worst(old["dgamma"].double() + t[keep].sum(0), old["dgamma"].double() + dg, b["dgamma"])[1]
    full = R.gathered(add, rows, c.M, c.S, Cseg) + core["rs"] * (core["g"] - core["s1"])
    found["s2 term dropped from dx"] = R.worst(R.scatter(full, rows, c.S, Cseg, n_src), dx, b["dx"])[1]
    if rows is not None:
        full = add.double()[:c.M].repeat(1, c.S) + core["val"]
        found["add read through r"] = R.worst(R.scatter(full, rows, c.S, Cseg, n_src), dx, b["dx"])[1]
    if c.dtype == BF:
        fin = R.gathered(add, rows, c.M, c.S, Cseg) + core["val"]
        found["dxsum of the rounded values"] = R.worst(old["dxsum"].double() + fin.to(BF).double().sum(0), old["dxsum"].double() + dxs, b["dxsum"])[1]
    print(f"[rowops-defect] bwd {c.name}: " + ", ".join(f"{k}: {v}" for k, v in found.items()))
    for k, v in found.items():
        assert v >= 1, f"{c.name}: the planted defect '{k}' stays inside the bound"


@pytest.mark.parametrize("c", R.cases_colsum(), ids=lambda c: c.name.replace(" ", "_"))
def test_colsum_emulation_within_bound_and_defects_outside(c):
    g = R.seed(c)
    y = torch.randn(c.M + 2, c.N, generator=g).to(c.dtype)
    old = torch.randn(c.N, generator=g)
    want, bnd = old.double() + R.colsum(y, c.M), R.colsum_bound(y, c.M, old)
    ratio, bad, where = R.worst(emu_colsum(y, c.M, old), want, bnd)
    print(f"[rowops-emu] colsum {c.name}: {ratio:.3f}")
    assert bad == 0 and ratio < 1, f"{c.name}: {bad} beyond the bound, worst {ratio:.3g} at {where}"
    found = {"a row skipped": R.worst(want - y[c.M // 2].double(), want, bnd)[1], "a row added twice": R.worst(want + y[c.M - 1].double(), want, bnd)[1],
             "M ignored": R.worst(want + y[c.M].double(), want, bnd)[1]}
    print(f"[rowops-defect] colsum {c.name}: " + ", ".join(f"{k}: {v}" for k, v in found.items()))
    assert all(v >= 1 for v in found.values()), found


def test_fold_emulation_within_bound_and_defects_outside():
    worst_by_ql, counts = {}, {}
    for c in R.cases_fold():
        ws, stride, bstride, old = R.fold_operands(c)
        args = (stride, bstride, c.nslabs, c.seg_len, c.nseg, c.batch)
        ref = R.fold(ws, *args)
        want = ref + old.double() if c.accumulate else ref
        bnd = R.fold_bound(ws, *args, old=old, accumulate=bool(c.accumulate))
        v = R.fold_view(ws, *args)
        emu = torch.stack([torch.stack([emu_fold(v[b, :, s * c.seg_len:(s + 1) * c.seg_len], old[s, b] if c.accumulate else None)
                                        for b in range(c.batch)]) for s in range(c.nseg)])
        ratio, bad, where = R.worst(emu, want, bnd)
        assert bad == 0 and ratio < 1, f"{c.name}: {bad} beyond the bound, worst {ratio:.3g} at {where}"
        key = (c.QL, min(c.loops4, 2))
        worst_by_ql[key] = max(worst_by_ql.get(key, 0.0), ratio)
        vd = v.double()
        per = lambda t: t.view(c.batch, c.nseg, c.seg_len).permute(1, 0, 2)       # noqa: E731
        found = {"a slab skipped": R.worst(want - per(vd[:, c.nslabs // 2]), want, bnd)[1],
                 "a slab added twice": R.worst(want + per(vd[:, c.nslabs - 1]), want, bnd)[1]}
        if c.nslabs > c.QL:
            found["slab QL read for slab 0"] = R.worst(want + per(vd[:, c.QL] - vd[:, 0]), want, bnd)[1]
        if c.batch > 1:
            found["batch stride ignored"] = R.worst(want - ref + ref[:, :1], want, bnd)[1]
        for k, n in found.items():
            assert n >= 1, f"{c.name}: the planted defect '{k}' stays inside the bound"
            counts[k] = counts.get(k, 0) + n
        # integer-valued slabs: every order of summation is exact in fp32
        wsi, stride, bstride, oldi = R.fold_operands(c, integers=True)
        vi = R.fold_view(wsi, *args)
        exact = R.fold(wsi, *args) + (oldi.double() if c.accumulate else 0)
        emi = torch.stack([torch.stack([emu_fold(vi[b, :, s * c.seg_len:(s + 1) * c.seg_len], oldi[s, b] if c.accumulate else None)
                                        for b in range(c.batch)]) for s in range(c.nseg)])
        assert torch.equal(emi.double(), exact), c.name
    for k, r in sorted(worst_by_ql.items()):
        print(f"[rowops-emu] fold QL={k[0]} four-load passes {'2+' if k[1] == 2 else k[1]}: {r:.3f}")
    print("[rowops-defect] fold (summed over the cases): " + ", ".join(f"{k}: {v}" for k, v in counts.items()))


def test_depths():
    assert R.row_depth(64, 8) == 14 and R.row_depth(4104, 8) == 9 * 8 + 6 and R.row_depth(260, 4) == 2 * 4 + 6
    assert R.fold_depth(95) == 6 + 15 + 1 and R.fold_depth(96) == 2 + 63 + 1 and R.fold_depth(1024, False) == 16 + 63
    assert R.param_depth(32800, 64, 8) == 8 * 2 + 3 + 16 + 63 + 1 and R.param_depth(1, 64, 8) == 2 + 3 + 1 + 15 + 1
    assert R.colsum_depth(1030) == 64 + 8 + 1 + 15 + 1 and R.colsum_depth(1) == 1 + 8 + 1 + 15 + 1
    assert R.scatter_depth(200, 3) == 4 * 3 + 7 and R.scatter_depth(0, 1) == 7
