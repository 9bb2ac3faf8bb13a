"""The pixel-contrast loss kernels (stswincl_amd/csrc/contrast.hip) against the float64 reference of tests/contrast_ref.py, every call
form at the shapes where tiling goes wrong (case tables: tests/contrast_cases.py; tests/test_contrast_ref.py shows on the CPU that
each table catches a dropped / extra / shifted bank row, swapped maps, a wrong block and a wrongly skipped negative term).

Every kernel is called through the C ABI with caller-owned outputs that are filled with NaN (ints: a sentinel) before the call, as is
the cached bank workspace hip._BANK_WS; after the call no NaN may remain in an output, and a refused call must leave them all.
Exact cases (integer operands) are compared without tolerance; rounding cases against the fp32 summation bounds of contrast_cases.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import contrast_cases as CC
import contrast_ref as R
from stswincl_amd import hip
from stswincl_amd.contrast.models import PixPro_swin_v5 as P

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = ["bf16", "f32"]


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _gm(gmap):
    flat = [int(v) for row in gmap for v in row]
    return (ctypes.c_int * len(flat))(*flat)


def _f64(t):
    return t.detach().cpu().double().numpy()


def _relnorm(got, ref):
    return float(np.linalg.norm(_f64(got) - ref) / np.linalg.norm(ref))


@functools.lru_cache(maxsize=None)
def _bank_case(kind, name, dtype):
    case = next(c for c in CC.EXACT_BANK + CC.ROUND_BANK if c.name == name)
    d = CC.bank_inputs(case, dtype, kind)
    inv_tau = CC.INV_TAU if kind == "round" else 0.5
    ref = R.bank_scores(CC.wide(d["Q"]), d["lq"], CC.wide(d["bank"]), d["lb"], d["gmap"], case.q_block, case.bank_block, inv_tau)
    return case, d, inv_tau, ref


def _bank_fwd(case, d, inv_tau, unit, want_lse, gmap=None, groups=None, C=None):
    """Raw call: Q = a column slice of a wider matrix (ldq > C), bank with row pitch C + case.ldb_pad -> (rc, pos, all, rowmax, lse, ws)."""
    gmap = d["gmap"] if gmap is None else gmap
    groups = len(gmap[0]) if groups is None else groups
    C = d["C"] if C is None else C
    Qw = d["Qw"].cuda()
    Q = Qw[:, d["off"]:d["off"] + d["C"]]
    assert Qw.stride(0) > d["C"] and Q.data_ptr() % 16 == 0 and (Qw.stride(0) * Qw.element_size()) % 16 == 0
    bank = torch.full((d["maps"] * d["seg"], d["C"] + case.ldb_pad), NAN, dtype=Qw.dtype, device="cuda")
    bank[:, :d["C"]] = d["bank"].reshape(-1, d["C"]).cuda()
    lq, lb = d["lq"].cuda(), d["lb"].cuda()
    M = d["M"]
    pos, tot = _nan(M, groups), _nan(M, groups)
    rmax, lse = (_nan(M), _nan(M)) if want_lse else (None, None)
    ws = hip._bank_workspace(Q.device, 4 * M * groups * 8)
    hip._BANK_WS[Q.device].fill_(NAN)
    fn = hip.load().stswin_contrast_bank_fwd_unit if unit else hip.load().stswin_contrast_bank_fwd
    rc = fn(hip._dt(Q), hip._p(Q), Qw.stride(0), hip._p(lq), M, C, case.q_sets, case.q_block, hip._p(bank), bank.stride(0), hip._p(lb),
            d["maps"], d["seg"], case.bank_block, groups, _gm(gmap), inv_tau, hip._p(pos), hip._p(tot), hip._p(rmax), hip._p(lse),
            hip._p(ws), ws.numel(), hip._stream())
    torch.cuda.synchronize()
    return rc, pos, tot, rmax, lse, ws


# ---------------------------------------------------------------------------------------------------------------- bank_fwd
@pytest.mark.parametrize("unit", [False, True], ids=["plain", "unit"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c.name for c in CC.EXACT_BANK])
def test_bank_fwd_exact(name, dtype, unit):
    """Integer operands: pos, all and the row maximum (inv_tau = 0.5) equal the reference bit for bit.  The plain entry also forms the
    online log-sum-exp (NaN-free; its accuracy is the rounding cases' business), the unit entry runs without it (the operands are
    not unit rows)."""
    case, d, inv_tau, ref = _bank_case("exact", name, dtype)
    assert float(np.abs(ref.absum).max()) < 2 ** 24
    rc, pos, tot, rmax, lse, _ = _bank_fwd(case, d, inv_tau, unit, want_lse=not unit)
    assert rc == 0
    assert np.array_equal(_f64(pos), ref.pos), "pos"
    assert np.array_equal(_f64(tot), ref.all), "all"
    if not unit:
        assert np.array_equal(_f64(rmax), ref.rowmax), "rowmax"
        assert bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("unit", [False, True], ids=["online", "fixed-reference"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c.name for c in CC.ROUND_BANK])
def test_bank_fwd_rounding(name, dtype, unit):
    """Unit rows rounded to the dtype, a key of score ~1 in the last row of every (ragged) bank block, inv_tau = 20: pos / all within
    (C + bank_block + 64) 2^-24 absum element by element (absum over the label-equal rows for pos), rowmax within
    (C + 1) 2^-24 inv_tau max_p sum_c |q_c k_pc|, lse within LSE_ALLOW.

    The lse allowance is measured, not derived (hardware exp2 / log; lse ~ 20, fp32 spacing 1.9e-6): largest |lse - float64 reference|
    over this table on MI355X 3.57e-6 (contrast_cases.LSE_MEASURED_MAX: r-1100 bf16, fixed-reference form; online form 3.03e-6);
    allowance 4 x that rounded up to a power of two = 2^-16 = 1.53e-5 (contrast_cases.LSE_ALLOW).  Losing the planted key moves lse by
    more than 1 (tests/test_contrast_ref.py)."""
    case, d, inv_tau, ref = _bank_case("round", name, dtype)
    rc, pos, tot, rmax, lse, _ = _bank_fwd(case, d, inv_tau, unit, want_lse=True)
    assert rc == 0
    e_pos, e_all = np.abs(_f64(pos) - ref.pos), np.abs(_f64(tot) - ref.all)
    e_max, e_lse = np.abs(_f64(rmax) - ref.rowmax), np.abs(_f64(lse) - ref.lse)
    b_pos, b_all = CC.sum_bound(d["C"], case.bank_block, ref.abspos), CC.sum_bound(d["C"], case.bank_block, ref.absum)
    b_max = CC.rowmax_bound(d["C"], inv_tau, ref.amax)
    print(f"[contrast] {name} {dtype} {'fixed' if unit else 'online'}: pos {e_pos.max():.2e} (bound {b_pos.max():.2e}) all {e_all.max():.2e} "
          f"({b_all.max():.2e}) rowmax {e_max.max():.2e} ({b_max.max():.2e}) lse {e_lse.max():.3e} (allow {CC.LSE_ALLOW:.2e})")
    assert not np.isnan(e_pos).any() and (e_pos <= b_pos).all(), "pos"
    assert not np.isnan(e_all).any() and (e_all <= b_all).all(), "all"
    assert not np.isnan(e_max).any() and (e_max <= b_max).all(), "rowmax"
    assert not np.isnan(e_lse).any() and float(e_lse.max()) <= CC.LSE_ALLOW, "lse"


def test_bank_fwd_long_block_is_three_splits_with_a_ragged_last_one():
    for case in (c for c in CC.EXACT_BANK + CC.ROUND_BANK if c.bank_block == 1100 and c.groups == 1):
        M = case.q_sets * case.nblk * case.q_block
        assert CC.planned_splits(M, case.q_sets, case.q_block, 1100, case.groups) == (3, 384)


@pytest.mark.parametrize("what", ["f32-C96", "C320", "groups9", "gmap=maps"])
def test_bank_fwd_refusals_leave_the_outputs_untouched(what):
    dtype = "f32" if what == "f32-C96" else "bf16"
    case, d, inv_tau, _ = _bank_case("exact", "240x129", dtype)
    d = dict(d)
    gmap, C = d["gmap"], d["C"]
    if what == "f32-C96":
        C = 96
    elif what == "C320":
        C = 320
    elif what == "groups9":
        gmap = [list(range(5)) + [0, 1, 2, 3]]
    else:
        gmap = [[0, 1, 2, 3, d["maps"]]]
    for unit in (False, True):
        rc, pos, tot, rmax, lse, ws = _bank_fwd(case, d, inv_tau, unit, True, gmap=gmap, C=C)
        assert rc != 0
        assert all(bool(torch.isnan(t).all()) for t in (pos, tot, rmax, lse, ws))
    if what in ("groups9", "gmap=maps"):                       # the wrapper raises
        with pytest.raises(hip.StswinHipError):
            hip.contrast_bank_fwd(d["Q"].contiguous().cuda(), d["lq"].cuda(), d["bank"].cuda(), d["lb"].cuda(), q_sets=1, q_block=case.q_block,
                                  bank_block=case.bank_block, gmap=gmap)
    else:
        Q = torch.zeros(d["M"], C, dtype=CC.DT[dtype], device="cuda")
        bank = torch.zeros(d["maps"], d["seg"], C, dtype=CC.DT[dtype], device="cuda")
        with pytest.raises(hip.StswinHipError):
            hip.contrast_bank_fwd(Q, d["lq"].cuda(), bank, d["lb"].cuda(), q_sets=1, q_block=case.q_block, bank_block=case.bank_block,
                                  gmap=d["gmap"])


# ---------------------------------------------------------------------------------------------------------------- legacy contrast_fwd
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW,C", [(63, 64), (240, 256), (63, 256), (240, 64)])
def test_legacy_contrast_fwd_exact(HW, C, dtype):
    g = torch.Generator().manual_seed(HW + C)
    N = 2
    q = torch.randint(-2, 3, (N * HW, C), generator=g).to(CC.DT[dtype])
    keys = torch.randint(-2, 3, (5, N * HW, C), generator=g).to(CC.DT[dtype])
    lq = torch.randint(0, 4, (N * HW,), generator=g, dtype=torch.int32)
    lk = torch.randint(0, 4, (5, N * HW), generator=g, dtype=torch.int32)
    ref = R.bank_scores(CC.wide(q), lq, CC.wide(keys), lk, [[0, 1, 2, 3, 4]], HW, HW)
    qg, kg, lqg, lkg = q.cuda(), keys.cuda(), lq.cuda(), lk.cuda()
    pos, tot = _nan(N, HW, 5), _nan(N, HW, 5)
    K5 = (ctypes.c_void_p * 5)(*[kg[j].data_ptr() for j in range(5)])
    L5 = (ctypes.c_void_p * 5)(*[lkg[j].data_ptr() for j in range(5)])
    rc = hip.load().stswin_contrast_fwd(hip._dt(qg), hip._p(qg), C, K5, C, hip._p(lqg), L5, hip._p(pos), hip._p(tot), N, HW, C, hip._stream())
    assert rc == 0
    assert np.array_equal(_f64(pos).reshape(N * HW, 5), ref.pos) and np.array_equal(_f64(tot).reshape(N * HW, 5), ref.all)


# ---------------------------------------------------------------------------------------------------------------- class_sums
def _class_sums(bank, lb, bank_block, ncls):
    maps, seg, C = bank.shape
    nb = seg // bank_block
    ksum = _nan(maps, nb, ncls + 1, C)
    need = hip.load().stswin_contrast_class_sums_scratch(maps, seg, bank_block, C, ncls)
    assert need > 0
    scr = hip.scratch(bank.device, need)
    scr.fill_(NAN)
    rc = hip.load().stswin_contrast_class_sums(hip._dt(bank), hip._p(bank), bank.stride(1), hip._p(lb), maps, seg, bank_block, C, ncls,
                                               hip._p(ksum), hip._p(scr), hip._stream())
    torch.cuda.synchronize()
    return rc, ksum


@pytest.mark.parametrize("C,ncls,bank_block,nb,dtype", CC.CLASS_SUMS)
def test_class_sums_exact(C, ncls, bank_block, nb, dtype):
    bank, lb = CC.class_sums_inputs(C, ncls, bank_block, nb, dtype)
    ref = R.class_sums(CC.wide(bank), lb, bank_block, ncls)
    rc, ksum = _class_sums(bank.cuda(), lb.cuda(), bank_block, ncls)
    assert rc == 0
    assert np.array_equal(_f64(ksum), ref)
    if ncls > 1:
        assert not ref[0, 0, ncls - 1].any() and not bool(ksum[0, 0, ncls - 1].any())       # the absent class: exactly 0.0


def test_class_sums_refuses_64_classes():
    bank, lb = CC.class_sums_inputs(64, 63, 8, 1, "f32")
    rc, ksum = _class_sums(bank.cuda(), lb.cuda(), 8, 64)
    assert rc == -1521 and bool(torch.isnan(ksum).all())
    with pytest.raises(hip.StswinHipError):
        hip.contrast_class_sums(bank.cuda(), lb.cuda(), 8, 64)


# ---------------------------------------------------------------------------------------------------------------- bank_dq
def _bank_dq(dpos, dneg, cnt, lq, ksum, gmap, q_block, bank_block, pad=0):
    M, groups = dpos.shape
    _, nb, ncls1, C = ksum.shape
    dq = _nan(M, C + pad)
    t = [torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous().cuda() for a in (dpos, dneg, cnt, ksum)]
    lqg = torch.as_tensor(np.asarray(lq), dtype=torch.int32).cuda()
    rc = hip.load().stswin_contrast_bank_dq(hip._p(t[0]), hip._p(t[1]), hip._p(t[2]), hip._p(lqg), hip._p(t[3]), hip._p(dq), C + pad, M, C,
                                            len(gmap), q_block, nb * bank_block, bank_block, ncls1 - 1, groups, _gm(gmap), hip._stream())
    torch.cuda.synchronize()
    return rc, dq


@pytest.mark.parametrize("case", CC.BANK_DQ, ids=str)
def test_bank_dq_exact(case):
    """Integer class sums and small-integer dpos / dneg: dq equals the reference bit for bit (|dq| < 2^24); rows whose negative set is
    empty carry dneg = 1e30 and must not see it; the row pitch of dq is C + 4 (the pad stays NaN)."""
    q_sets, nblk, q_block, nb, bank_block, C, groups, ncls = case
    bank, lb, lq, gmap, dpos, dneg = CC.bank_dq_inputs(*case)
    cnt = R.label_counts(lq, lb, gmap, q_block, bank_block, ncls)
    assert (cnt == bank_block).any()
    dneg = np.where(cnt == bank_block, 1e30, CC.wide(dneg))
    ksum = R.class_sums(bank, lb, bank_block, ncls)
    ref = R.bank_dq(dpos, dneg, cnt, lq, ksum, gmap, q_block, bank_block)
    assert float(np.abs(ref).max()) < 2 ** 24
    rc, dq = _bank_dq(dpos, dneg, cnt, lq, ksum, gmap, q_block, bank_block, pad=4)
    assert rc == 0
    assert np.array_equal(_f64(dq[:, :C]), ref) and bool(torch.isnan(dq[:, C:]).all())


def test_bank_dq_empty_negative_set_contributes_nothing_with_rounded_class_sums():
    """Unit-row bank, class sums from the class_sums kernel (Ktot - Kcls is then rounding residue, not 0): where cnt == bank_block the
    term is skipped even with dneg = 1e30.  Bound: dq is an fp32 sum of 2 groups products of fp32 factors, each (Ktot - Kcls) rounded
    once: (2 groups + 3) 2^-24 sum_g |dpos| |Kcls| + |dneg| (|Ktot| + |Kcls|)."""
    case = CC.BANK_DQ[0]
    q_sets, nblk, q_block, nb, bank_block, C, groups, ncls = case
    bank, lb, lq, gmap, dpos, dneg = CC.bank_dq_inputs(*case, exact=False)
    cnt = R.label_counts(lq, lb, gmap, q_block, bank_block, ncls)
    full = cnt == bank_block
    assert full.any()
    dneg = np.where(full, 1e30, CC.wide(dneg))
    rc, ksum = _class_sums(bank.cuda(), lb.cuda(), bank_block, ncls)
    assert rc == 0
    ks = _f64(ksum)
    # the kernel adds a block's rows to the class and to the total in one order, so its Ktot - Kcls of a one-class block is exactly 0;
    # a total that carries a residue (as sums formed any other way would) makes a term that is not skipped show as 1e30 x 2^-12
    ks[..., ncls, :] = (ks[..., ncls, :] + 2.0 ** -12).astype(np.float32).astype(np.float64)
    ref = R.bank_dq(dpos, dneg, cnt, lq, ks, gmap, q_block, bank_block)
    mag = np.zeros_like(ref)
    for m in range(ref.shape[0]):
        b = (m % (nblk * q_block)) // q_block if nb > 1 else 0
        for g, mp in enumerate(gmap[m // (nblk * q_block)]):
            kc, kt = np.abs(ks[mp, b, int(lq[m])]), np.abs(ks[mp, b, ncls])
            mag[m] += abs(float(dpos[m, g])) * kc + (0.0 if full[m, g] else abs(dneg[m, g]) * (kt + kc))
    rc, dq = _bank_dq(dpos, dneg, cnt, lq, ks, gmap, q_block, bank_block)
    assert rc == 0
    err = np.abs(_f64(dq) - ref)
    print(f"[contrast] bank_dq rounded: max err {err.max():.2e}, bound min {((2 * groups + 3) * CC.U24 * mag).min():.2e}")
    assert not np.isnan(err).any() and (err <= (2 * groups + 3) * CC.U24 * mag).all()


def test_bank_dq_refuses_mismatched_block_counts():
    dpos = np.ones((3 * 4, 2))
    ksum = np.zeros((2, 2, 4, 8))                               # 2 bank blocks for 3 query blocks
    rc, dq = _bank_dq(dpos, dpos, dpos, np.zeros(12, np.int32), ksum, [[0, 1]], 4, 5)
    assert rc == -1532 and bool(torch.isnan(dq).all())


# ---------------------------------------------------------------------------------------------------------------- end to end
def _e2e_reference(Qr, lq, bank, lb, gmap, q_block, bank_block, ncls):
    sc = R.bank_scores(Qr, lq, bank, lb, gmap, q_block, bank_block)
    cnt = R.label_counts(lq, lb, gmap, q_block, bank_block, ncls)
    loss, dpos, dneg = R.pair_loss(sc.pos, sc.all, cnt, len(gmap), bank_block)
    return loss, R.bank_dq(dpos, dneg, cnt, lq, R.class_sums(bank, lb, bank_block, ncls), gmap, q_block, bank_block)


E2E_BOUND = {"f32": 1e-5, "bf16": 2.0 ** -8}                    # bf16: the one rounding left is the final cast of the gradient, 2^-9 an element


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_through_contrast_bank_fn(dtype):
    g = torch.Generator().manual_seed(5)
    q_sets, nblk, qb, C, ncls, gmap = 2, 2, 63, 128, 12, [[1, 2, 3, 4, 5], [0, 2, 3, 4, 5]]
    q = F.normalize(torch.randn(q_sets * nblk * qb, C, generator=g), dim=1).to(CC.DT[dtype])
    bank = F.normalize(torch.randn(6, nblk * qb, C, generator=g), dim=2).to(CC.DT[dtype])
    lb = torch.randint(0, ncls, (6, nblk * qb), generator=g, dtype=torch.int32)
    lq = torch.randint(0, ncls, (q_sets * nblk * qb,), generator=g, dtype=torch.int32)
    lb[2, :qb] = lq[0]                                          # an empty negative set
    ref_loss, ref_dq = _e2e_reference(CC.wide(q), lq, CC.wide(bank), lb, gmap, qb, qb, ncls)
    qg = q.cuda().requires_grad_(True)
    loss, _, _ = P.bank_contrast_loss(qg, lq.cuda(), bank.cuda(), lb.cuda(), gmap, qb, qb, ncls)
    loss.backward()
    e = _relnorm(qg.grad, ref_dq)
    print(f"[contrast] ContrastBankFn {dtype}: loss rel {abs(float(loss) - ref_loss) / abs(ref_loss):.2e}, grad rel-norm {e:.2e}")
    assert qg.grad.dtype == CC.DT[dtype] and e < E2E_BOUND[dtype]
    assert abs(float(loss) - ref_loss) <= 2e-5 * abs(ref_loss)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_through_pair_loss_fn(dtype):
    g = torch.Generator().manual_seed(6)
    b, HW, C, ncls, gmap = 2, 63, 64, 12, [[1, 2, 3, 4, 5], [0, 2, 3, 4, 5]]
    X = (torch.randn(2 * b * HW, C, generator=g) * 2).to(CC.DT[dtype])
    bank = F.normalize(torch.randn(6, b * HW, C, generator=g), dim=2).to(CC.DT[dtype])
    lb = torch.randint(0, ncls, (6, b * HW), generator=g, dtype=torch.int32)
    Y, _ = R.rownorm_scatter(CC.wide(X), 2, HW, b)
    Yr = torch.from_numpy(Y).to(CC.DT[dtype]).double().numpy()  # the query matrix is stored in the compute dtype
    lq = lb[:2].reshape(-1)
    ref_loss, ref_dq = _e2e_reference(Yr, lq, CC.wide(bank), lb, gmap, HW, HW, ncls)
    ref_dx = R.rownorm_scatter_bwd(CC.wide(X), ref_dq, 2, HW, b)
    xg = X.cuda().requires_grad_(True)
    loss, _, _ = P.pair_loss_tokens(xg, bank.cuda(), lb.cuda(), b, HW, ncls)
    loss.backward()
    e = _relnorm(xg.grad, ref_dx)
    print(f"[contrast] PairLossFn {dtype}: loss rel {abs(float(loss) - ref_loss) / abs(ref_loss):.2e}, grad rel-norm {e:.2e}")
    assert xg.grad.dtype == CC.DT[dtype] and e < E2E_BOUND[dtype]
    assert abs(float(loss) - ref_loss) <= 2e-5 * abs(ref_loss)


# ---------------------------------------------------------------------------------------------------------------- label_counts
def _label_counts(lq, lb, q_sets, q_block, bank_block, ncls, gmap):
    M, (maps, seg), groups = lq.numel(), lb.shape, len(gmap[0])
    hist = torch.full((maps, max(seg // bank_block, 1), ncls), -7, dtype=torch.int32, device="cuda")
    cnt = _nan(M, groups)
    lqg, lbg = lq.cuda(), lb.cuda()
    rc = hip.load().stswin_label_counts(hip._p(lqg), hip._p(lbg), M, maps, seg, q_sets, q_block, bank_block, ncls, groups, _gm(gmap),
                                        hip._p(hist), hip._p(cnt), hip._stream())
    torch.cuda.synchronize()
    return rc, cnt


@pytest.mark.parametrize("ncls", [1, 12, 64])
@pytest.mark.parametrize("q_sets,nblk,q_block,nb,bank_block", [(2, 3, 67, 3, 45), (1, 5, 61, 1, 300), (2, 1, 333, 1, 77)])
def test_label_counts_exact(q_sets, nblk, q_block, nb, bank_block, ncls):
    g = torch.Generator().manual_seed(ncls + q_block)
    M, seg, gmap = q_sets * nblk * q_block, nb * bank_block, [[1, 2, 3], [0, 2, 3]][:q_sets]
    assert M % 256
    lq = torch.randint(0, ncls, (M,), generator=g, dtype=torch.int32)
    lb = torch.randint(0, ncls, (4, seg), generator=g, dtype=torch.int32)
    lq[1::7], lq[2::11] = -3, ncls + 5                         # clamped to 0 resp. ncls - 1
    lb[:, 3::5], lb[:, 1::13] = -3, ncls + 5
    rc, cnt = _label_counts(lq, lb, q_sets, q_block, bank_block, ncls, gmap)
    assert rc == 0
    assert np.array_equal(_f64(cnt), R.label_counts(lq, lb, gmap, q_block, bank_block, ncls).astype(np.float64))


@pytest.mark.parametrize("M,q_block,seg,bank_block", [(2 * 3 * 10 + 2, 10, 30, 10), (2 * 3 * 10, 10, 20, 10)],
                         ids=["M % (q_sets q_block)", "2 bank blocks for 3 query blocks"])
def test_label_counts_refuses_malformed_geometry(M, q_block, seg, bank_block):
    lq = torch.zeros(M, dtype=torch.int32)
    lb = torch.zeros(4, seg, dtype=torch.int32)
    rc, cnt = _label_counts(lq, lb, 2, q_block, bank_block, 12, [[1, 2, 3], [0, 2, 3]])
    assert rc == -1543 and bool(torch.isnan(cnt).all())


# ---------------------------------------------------------------------------------------------------------------- pair_loss
@pytest.mark.parametrize("groups", [1, 8])
@pytest.mark.parametrize("per_set,visible", [(7, 9), (1024, 300), (1025, 1), (1025, 63)])
@pytest.mark.parametrize("q_sets", [1, 2])
def test_pair_loss_and_its_backward(q_sets, per_set, visible, groups):
    g = torch.Generator().manual_seed(per_set + groups)
    M = q_sets * per_set
    cnt = torch.randint(0, visible + 1, (M, groups), generator=g).float()
    cnt[0], cnt[1] = 0.0, float(visible)                       # empty positive sets, empty negative sets
    pos = torch.randn(M, groups, generator=g) * cnt * 0.3
    tot = pos + torch.randn(M, groups, generator=g) * (visible - cnt) * 0.3
    ref, rdp, rdn = R.pair_loss(CC.wide(pos), CC.wide(tot), CC.wide(cnt), q_sets, visible, dloss=1.5)
    pg, tg, cg, dl = pos.cuda(), tot.cuda(), cnt.cuda(), torch.full((1,), 1.5, device="cuda")
    out = []
    for _ in range(2):
        loss, dpos, dneg = _nan(1), _nan(M, groups), _nan(M, groups)
        assert hip.load().stswin_pair_loss(hip._p(pg), hip._p(tg), hip._p(cg), M, groups, q_sets, visible, hip._p(loss), hip._stream()) == 0
        assert hip.load().stswin_pair_loss_bwd(hip._p(pg), hip._p(tg), hip._p(cg), hip._p(dl), M, groups, q_sets, visible, hip._p(dpos),
                                               hip._p(dneg), hip._stream()) == 0
        out.append((loss, dpos, dneg))
    (loss, dpos, dneg), again = out
    assert all(torch.equal(a, b) for a, b in zip(out[0], again))          # fixed-order sums: equal bits
    e_l, e_p, e_n = abs(float(loss) - ref), np.abs(_f64(dpos) - rdp).max(), np.abs(_f64(dneg) - rdn).max()
    print(f"[contrast] pair_loss {q_sets}x{per_set} g{groups} v{visible}: loss rel {e_l / abs(ref):.2e} dpos {e_p / np.abs(rdp).max():.2e} "
          f"dneg {e_n / np.abs(rdn).max():.2e}")
    assert e_l <= 2e-6 * abs(ref) + 1e-7
    assert e_p <= 1e-5 * np.abs(rdp).max() + 1e-12 and e_n <= 1e-5 * np.abs(rdn).max() + 1e-12


# ---------------------------------------------------------------------------------------------------------------- rownorm_scatter
@pytest.mark.parametrize("dtype,views,b,hw,C", [("f32", 2, 3, 7, 256), ("bf16", 6, 1, 5, 64), ("bf16", 1, 3, 7, 1024), ("f32", 1, 1, 9, 1024),
                                                ("bf16", 2, 3, 7, 256), ("f32", 6, 1, 5, 64)])
def test_rownorm_scatter_and_its_backward(dtype, views, b, hw, C):
    """Forward bit-equal to F.normalize in fp32 followed by the cast.  Backward element by element against float64, with max|ref| taken
    PER ROW (the zero row's gradient is 1e12 dy: a matrix-wide maximum would check nothing): fp32 |dx - ref| <= 2^-20 max|ref|, bf16
    |dx - ref| <= 2^-8 |ref| + 2^-20 max|ref|."""
    g = torch.Generator().manual_seed(views + C)
    Rr = views * b * hw
    assert Rr % 4
    Xw = torch.full((Rr, C + 8), NAN).to(CC.DT[dtype])
    Xw[:, :C] = (torch.randn(Rr, C, generator=g) * 3).to(CC.DT[dtype])
    Xw[5, :C] = 0                                              # a zero row: y = 0, no NaN
    Xg = Xw.cuda()
    X = Xg[:, :C]
    Y = torch.full((Rr, C), NAN, dtype=X.dtype, device="cuda")
    inv = _nan(Rr)
    assert hip.load().stswin_rownorm_scatter(hip._dt(X), hip._p(X), Xg.stride(0), hip._p(Y), C, hip._p(inv), Rr, C, views, hw, b, hip._stream()) == 0
    want = F.normalize(X.float(), dim=1).view(b, views, hw, C).permute(1, 0, 2, 3).reshape(Rr, C).to(X.dtype)
    assert torch.equal(Y, want)
    ref_y, ref_inv = R.rownorm_scatter(CC.wide(Xw[:, :C]), views, hw, b)
    assert np.abs(_f64(Y) - ref_y).max() <= (2.0 ** -8 if dtype == "bf16" else 2.0 ** -23) and np.allclose(_f64(inv), ref_inv, rtol=2.0 ** -21)
    dY = torch.randn(Rr, C, generator=g)
    dX = torch.full((Rr, C), NAN, dtype=X.dtype, device="cuda")
    dYg = dY.cuda()
    assert hip.load().stswin_rownorm_scatter_bwd(hip._dt(X), hip._p(X), Xg.stride(0), hip._p(inv), hip._p(dYg), C, hip._p(dX), C, Rr, C, views, hw,
                                                 b, hip._stream()) == 0
    ref = R.rownorm_scatter_bwd(CC.wide(Xw[:, :C]), CC.wide(dY), views, hw, b)
    err, rowmax = np.abs(_f64(dX) - ref), np.abs(ref).max(1, keepdims=True)
    bound = 2.0 ** -20 * rowmax + (2.0 ** -8 * np.abs(ref) if dtype == "bf16" else 0.0)
    print(f"[contrast] rownorm_bwd {dtype} C{C} v{views}: max err / row max {(err / rowmax).max():.2e}")
    assert not np.isnan(err).any() and (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------- labels_resize
@pytest.mark.parametrize("Hs,Ws,h,w", [(64, 80, 8, 10), (50, 37, 7, 9), (7, 9, 16, 20), (512, 512, 32, 32)])
def test_labels_resize_equals_the_reference_and_atens_nearest(Hs, Ws, h, w):
    g = torch.Generator().manual_seed(Hs)
    masks = [torch.randint(0, 12, (2, 1, Hs, Ws), generator=g).float() for _ in range(3)]
    masks[0][0, 0, :Hs // 2] = 3.9
    masks[1][1, 0, :, :Ws // 2] = -0.5
    masks[2][0, 0, Hs // 2:] = 255.0
    mg = [m.cuda() for m in masks]
    lb = torch.full((3, 2 * h * w), -77, dtype=torch.int32, device="cuda")
    arr = (ctypes.c_void_p * 3)(*[m.data_ptr() for m in mg])
    assert hip.load().stswin_labels_resize(arr, 3, 2, Hs, Ws, h, w, hip._p(lb), hip._stream()) == 0
    aten = torch.stack([F.interpolate(m, size=[h, w], mode="nearest").reshape(-1).to(torch.int32) for m in masks], 0)
    assert np.array_equal(lb.cpu().numpy(), R.labels_resize([m.numpy() for m in masks], h, w)) and torch.equal(lb.cpu(), aten)
