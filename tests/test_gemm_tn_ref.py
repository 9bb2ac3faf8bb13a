"""tests/gemm_tn_ref.py (the float64 reference, the split partition and the derived bound of the gemm_tn contract) held to independent
definitions on the CPU, at every case of tests/test_hip_gemm_tn_contract.py:
  * ref() against float64 autograd: the weight gradient of F.linear (plain, both row maps with -1 rows) and of a dilated 3x3 F.conv2d
    through a row map built in plain torch (bseg; tapminor = weight.grad in its own [cout][cin][k][k] layout);
  * partition() / corrected_splits() against the launcher's rule;
  * the bound holds for an fp32 emulation of every combine form (sequential fp32 accumulation per split in partition order, partials
    rounded to bf16 where they are bf16, added in fp32 in split order) - the largest err / bound per form is printed;
  * the bound has teeth: four planted defects (contraction row Mk - 1 left out; a -1 map row read as row 0; a tile's second tap read
    through the first tap's map; the tap-minor permutation not applied) each leave elements outside it, at every case."""
import pytest
import torch
import torch.nn.functional as F

import gemm_tn_ref as T

F64 = torch.float64
CASES = T.cases()
IDS = [c.name.replace(" ", "_") for c in CASES]


def test_codes_and_bits_are_the_headers():
    from stswincl_amd import hip                          # (hip.X is the header's STSWIN_X; importing it needs no GPU)
    for name, value in (("VAR_TN_RING_PLAIN", T.RING_PLAIN), ("VAR_TN_RING_ATROWS", T.RING_ATROWS), ("VAR_TN_RING_BTROWS", T.RING_BTROWS),
                        ("VAR_TN_RING_BSEG", T.RING_BSEG), ("VAR_TN_128x128", T.K128), ("VAR_TN_128x128_W4", T.K128_W4), ("VAR_TN_ROWS", T.ROWS),
                        ("VAR_F32", T.VAR_F32), ("VAR_TN_SLABS_F32", T.SLABS_F32), ("VAR_TN_SLABS_BF16", T.SLABS_BF16),
                        ("VAR_TN_TAPMINOR", T.TAPMINOR), ("VAR_TN_FUSED", T.FUSED)):
        assert getattr(hip, name) == value, name
    # the tuning bits are documented in prose only ("bits 28-30 ... forbid / force the 256x256 ring kernel, 4-wave 128x128 variant")
    assert T.BIT_RING == 1 << 29 and T.BIT_W4 == 1 << 30
    assert not (T.BIT_RING | T.BIT_W4) & (hip.TN_OVERWRITE | hip.TN_NO_COMBINE | hip.TN_OUT_TAPMINOR)


def test_every_kernel_code_and_combine_form_has_a_case():
    kernels = {c.kernel for c in CASES}
    assert kernels >= {20, 21, 22, 23, 30, 31, 32, 130, 131}
    assert {c.expect for c in CASES} >= {"rows", "none", "atomics", "f32", "bf16", "fused", "explicit-f32", "explicit-bf16"}
    assert any(c.tapminor_honoured for c in CASES) and any(c.tapminor and not c.tapminor_honoured for c in CASES)


# ------------------------------------------------------------------------------------------------------------------ ref == autograd
def _pad_gather(X, rows):
    """X[rows] with -1 -> zeros, as an autograd-visible torch expression of its own (index into X with a zero row appended)."""
    Xp = torch.cat([X, torch.zeros(1, X.shape[1], dtype=X.dtype)])
    return Xp[torch.where(rows < 0, torch.full_like(rows, X.shape[0]), rows).long()]


@pytest.mark.parametrize("maps", ["", "a", "b", "ab"])
def test_ref_is_the_weight_gradient_of_linear(maps):
    g = torch.Generator().manual_seed(5)
    Mk, cout, cin = 37, 24, 40
    dy = torch.randn(Mk + 9, cout, generator=g).bfloat16()
    x = torch.randn(Mk + 13, cin, generator=g).bfloat16()
    ar = torch.randint(-1, Mk + 9, (Mk,), generator=g, dtype=torch.int32) if "a" in maps else None
    br = torch.randint(-1, Mk + 13, (Mk,), generator=g, dtype=torch.int32) if "b" in maps else None
    for r in (ar, br):
        if r is not None:
            r[4] = -1
    w = torch.zeros(cout, cin, dtype=F64, requires_grad=True)
    xin = _pad_gather(x.double(), br) if br is not None else x.double()[:Mk]
    dyin = _pad_gather(dy.double(), ar) if ar is not None else dy.double()[:Mk]
    F.linear(xin, w).backward(dyin)
    prev = torch.randn(cout, cin, generator=g)
    got = T.ref(dy, x, Mk=Mk, at_rows=ar, bt_rows=br)
    assert float((got - w.grad).abs().max()) < 1e-12
    assert float((T.ref(dy, x, Mk=Mk, at_rows=ar, bt_rows=br, c_prev=prev) - (prev.double() + w.grad)).abs().max()) < 1e-12


@pytest.mark.parametrize("dil", [1, 2])
def test_ref_is_the_weight_gradient_of_a_dilated_convolution(dil):
    g = torch.Generator().manual_seed(6)
    H, W, cin, cout = 6, 7, 16, 24
    x = torch.randn(1, cin, H, W, generator=g).bfloat16()
    dy = torch.randn(1, cout, H, W, generator=g).bfloat16()
    w = torch.zeros(cout, cin, 3, 3, dtype=F64, requires_grad=True)
    F.conv2d(x.double(), w, padding=dil, dilation=dil).backward(dy.double())
    rowmap = T.conv3x3_rowmap(H, W, dil)
    assert rowmap.shape == (9, H * W) and int((rowmap < 0).sum()) > 0
    At = dy[0].permute(1, 2, 0).reshape(H * W, cout).contiguous()       # NHWC tokens
    Bt = torch.cat([x[0].permute(1, 2, 0).reshape(H * W, cin), torch.randn(5, cin, generator=g).bfloat16()])     # (taller than Mk)
    kw = dict(Mk=H * W, bt_rows=rowmap.flatten(), bseg=cin)
    gemm_order = T.ref(At, Bt, **kw)                                     # [cout][tap][cin]
    assert float((gemm_order - w.grad.permute(0, 2, 3, 1).reshape(cout, 9 * cin)).abs().max()) < 1e-12
    tapminor = T.ref(At, Bt, tapminor=True, **kw)                        # [cout][cin][ky][kx]: weight.grad as it lies in memory
    assert float((tapminor - w.grad.reshape(cout, cin * 9)).abs().max()) < 1e-12
    prev = torch.randn(cout, cin * 9, generator=g)
    assert float((T.ref(At, Bt, tapminor=True, c_prev=prev, **kw) - (prev.double() + w.grad.reshape(cout, -1))).abs().max()) < 1e-12
    # the permutation is the one the header states: GEMM column s * bseg + c -> c * S + s
    s, c_ = 5, 11
    assert torch.equal(tapminor[:, c_ * 9 + s], gemm_order[:, s * cin + c_])


# ------------------------------------------------------------------------------------------------------------------ partition
@pytest.mark.parametrize("unit", [32, 64])
def test_partition_tiles_the_contraction_without_an_empty_split(unit):
    for Mk in (1, 31, 32, 33, 64, 100, 200, 201, 1000, 16576):
        units = -(-Mk // unit)
        for req in range(1, 70):
            s = T.corrected_splits(Mk, req, unit)
            assert 1 <= s <= min(req, units)
            per = -(-units // s)
            assert -(-units // per) == s                  # the rule of stswin_gemm_tn: ceil(units / per) splits of per units
            r = T.partition(Mk, s, unit)
            assert len(r) == s and r[0][0] == 0 and r[-1][1] == Mk
            assert all(m1 > m0 for m0, m1 in r), (Mk, req, s, r)
            assert all(r[i][1] == r[i + 1][0] for i in range(s - 1))
            assert all(m0 % unit == 0 for m0, _ in r) and all((m1 - m0) == per * unit for m0, m1 in r[:-1])


def test_partition_examples_of_the_launcher():
    # 259 units over 64 splits: ceil = 5 each fills 52 splits, 12 would stay empty (gemm.hip) -> 52
    assert T.corrected_splits(259 * 64, 64, 64) == 52
    assert any(m0 == m1 for m0, m1 in T.partition(259 * 64, 64, 64)) and all(m1 > m0 for m0, m1 in T.partition(259 * 64, 52, 64))
    # 4 units over 3 splits: 2 each -> 2 splits
    assert T.corrected_splits(200, 3, 64) == 2 and T.partition(200, 2, 64) == [(0, 128), (128, 200)]
    assert T.corrected_splits(200, 3, 32) == 3 and T.partition(200, 3, 32) == [(0, 96), (96, 192), (192, 200)]
    assert T.corrected_splits(33, 4, 64) == 1 and T.corrected_splits(33, 4, 32) == 2
    # the ring's stages of 32: 32 stages over 5 -> 7 per split -> stays 5; 2 stages over 8 -> 2; 4 over 2 -> 2, the last one ragged
    assert T.corrected_splits(1000, 5, 32) == 5 and T.partition(1000, 5, 32)[-1] == (896, 1000)
    assert T.corrected_splits(40, 8, 32) == 2 and T.partition(40, 2, 32) == [(0, 32), (32, 40)]
    assert T.partition(100, 2, 32) == [(0, 64), (64, 100)]
    # the automatic 22528 x 512 x 512 dispatch at 256 compute units: 4 tiles, 704 stages -> min(256 / 4, 704 / 16) = 44 splits of 16
    assert T.corrected_splits(22528, min(256 // 4, 704 // 16), 32) == 44
    assert next(c for c in CASES if c.Mk == 22528).splits == 44


def test_case_split_counts_follow_the_rule():
    for c in CASES:
        if c.req:
            assert c.splits == T.corrected_splits(c.Mk, c.req, c.unit), c.name
        assert all(m1 > m0 for m0, m1 in c.ranges()) and c.ranges()[-1][1] == c.Mk, c.name
    by = {c.name: c for c in CASES}
    assert by["128x128 bf16 ragged Mk=200 splits=3"].splits == 2 and by["128x128 f32 ragged Mk=200 splits=3"].splits == 3
    assert by["128x128 bf16 splits=4 clamped"].splits == 1 and by["ring 40x256x256 rs=8"].splits == 2
    assert by["ring 1000x256x512 rs=5"].splits == 5


# ------------------------------------------------------------------------------------------------------------------ bound
def _setup(c):
    """Everything of a case the two bound tests share, in float64: operands, partials in the stored layout, c_prev."""
    p = T.problem(c)
    A, B = T.operands(p["At"], p["Bt"], Mk=c.Mk, Nj=c.Nj, at_rows=p["at_rows"], bt_rows=p["bt_rows"], bseg=c.bseg)
    P, Ab = T.partials(A, B, c.ranges())
    if c.tapminor_honoured:
        P, Ab = T.to_tapminor(P, c.bseg), T.to_tapminor(Ab, c.bseg)
    prev = torch.randn(c.Ni, c.Nj, generator=torch.Generator().manual_seed(c.Mk + c.Nj))
    return p, A, B, P, Ab, prev


def _stored(c, X):
    return T.to_tapminor(X, c.bseg) if c.tapminor_honoured else X


def _emulate(c, A, B, prev):
    """An fp32 run of the case's combine form; prev: fp32 [Ni][Nj] or None (overwrite)."""
    A32, B32 = A.float(), B.float()                      # (exact: the operands are bf16 / fp32 values)
    zero = torch.zeros(c.Ni, c.Nj)
    if c.rows:
        v = zero.clone() if prev is None else prev.clone()
        for m in range(c.Mk):
            v += A32[m][:, None] * B32[m][None, :]
        return v
    slabs = []
    for m0, m1 in c.ranges():
        acc = zero.clone()
        for m in range(m0, m1):
            acc += A32[m][:, None] * B32[m][None, :]
        slabs.append(acc.bfloat16().float() if c.slab_bf16 else acc)
    if c.has_slabs:                                      # tn_reduce / the fused combine: the partials onto zero, then onto C
        s = zero.clone()
        for x in slabs:
            s += x
        s = _stored(c, s)
        return s if prev is None else prev + s
    v = zero.clone() if prev is None else prev.clone()   # atomics: every partial straight onto C (here: in split order)
    for x in slabs:
        v += x
    return v


@pytest.fixture(scope="module")
def headroom():
    table = {}
    yield table
    print("\n[gemm_tn bound] largest err / bound of the fp32 emulation per combine form: " +
          "  ".join(f"{k} {v:.3f}" for k, v in sorted(table.items())))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bound_holds_for_an_fp32_emulation(c, headroom):
    p, A, B, P, Ab, prev = _setup(c)
    want0 = P.sum(0)
    for cp in (None, prev):
        got = _emulate(c, A, B, cp)
        want = want0 if cp is None else cp.double() + want0
        bnd = T.bound(P, Ab, c.ranges(), c_prev=cp, slab_bf16=c.slab_bf16, rows_kernel=c.rows)
        ratio, bad, where = T.worst(got, want, bnd, P, tile=c.tile, tapminor_bseg=c.bseg if c.tapminor_honoured else 0)
        headroom[c.expect] = max(headroom.get(c.expect, 0.0), ratio)
        assert bad == 0 and ratio < 1.0, f"{c.name} ({'overwrite' if cp is None else 'accumulate'}): {bad} elements beyond the bound, worst {where}"


def _defects(c, p, A, B):
    """{name: delta of the GEMM-order float64 result} for the defects that apply to the case; (d) is handled by the caller."""
    Mk, out = c.Mk, {}
    out["a: row Mk-1 left out"] = -torch.outer(A[Mk - 1], B[Mk - 1])
    if "a" in c.maps:
        m = int((p["at_rows"] < 0).nonzero().max())
        out["b: at_rows -1 read as row 0"] = torch.outer(p["At"][0].double(), B[m])
    elif c.bseg > 0:
        t, m = (int(v) for v in (p["bt_rows"].view(-1, Mk) < 0).nonzero()[-1])
        d = torch.zeros(c.Ni, c.Nj, dtype=F64)
        d[:, t * c.bseg:(t + 1) * c.bseg] = torch.outer(A[m], p["Bt"][0, :c.bseg].double())
        out["b: bt_rows -1 read as row 0"] = d
    elif "b" in c.maps:
        m = int((p["bt_rows"] < 0).nonzero().max())
        out["b: bt_rows -1 read as row 0"] = torch.outer(A[m], p["Bt"][0, :c.Nj].double())
    if c.bseg > 0:
        maps = p["bt_rows"].view(-1, Mk)
        j0 = next(j for j in range(0, c.Nj, c.tile) if (min(j + c.tile, c.Nj) - 1) // c.bseg != j // c.bseg)
        tap0 = j0 // c.bseg
        cols = torch.arange(j0, min(j0 + c.tile, c.Nj))
        cols = cols[cols // c.bseg == tap0 + 1]
        wrong = T.gather(p["Bt"][:, :c.bseg], maps[tap0], Mk)[:, cols % c.bseg]
        d = torch.zeros(c.Ni, c.Nj, dtype=F64)
        d[:, cols] = A.t() @ (wrong - B[:, cols])
        out["c: second tap of a tile through the first tap's map"] = d
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bound_has_teeth(c):
    p, A, B, P, Ab, prev = _setup(c)
    bnd = T.bound(P, Ab, c.ranges(), c_prev=prev, slab_bf16=c.slab_bf16, rows_kernel=c.rows)     # (accumulate: the wider of the two)
    assert bool((bnd >= T.bound(P, Ab, c.ranges(), slab_bf16=c.slab_bf16, rows_kernel=c.rows)).all())
    deltas = {k: _stored(c, d) for k, d in _defects(c, p, A, B).items()}
    if c.tapminor_honoured:
        deltas["d: tap-minor permutation not applied"] = (A.t() @ B) - P.sum(0)
    assert "a: row Mk-1 left out" in deltas and (not c.maps or len(deltas) >= 2) and (c.bseg == 0 or len(deltas) >= 3)
    for name, d in deltas.items():
        # (2 x: a kernel with the defect also has its own rounding error, up to one bound, which may point the other way)
        outside = int((d.abs() > 2 * bnd).sum())
        print(f"[gemm_tn teeth] {c.name}: {name}: {outside} of {d.numel()} elements outside, largest |delta| / bound "
              f"{float((d.abs() / bnd).max()):.3g}")
        assert outside > 0, f"{c.name}: defect ({name}) stays inside the bound everywhere"
