"""tests/contrast_ref.py (the float64 reference of the pixel-contrast loss kernels) checked on the CPU before any kernel is held
against it: against the dense oracle and torch autograd of its loss in float64, against the recorded reference outputs, and - for the
case tables of tests/test_hip_contrast_contract.py (tests/contrast_cases.py) - sensitivity: each way a tiled kernel goes subtly wrong,
applied to the reference, moves a checked output by more than 4 x the tolerance of the case (any change where the check is exact)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import contrast_cases as CC
import contrast_ref as R
import golden_util as gu
from oracle import stswin_oracle as O

F64 = torch.float64


def _rand_case(seed, q_sets, nblk, q_block, nb, bank_block, C, maps, ncls=6):
    g = torch.Generator().manual_seed(seed)
    M, seg = q_sets * nblk * q_block, nb * bank_block
    q = F.normalize(torch.randn(M, C, generator=g, dtype=F64), dim=1)
    bank = F.normalize(torch.randn(maps, seg, C, generator=g, dtype=F64), dim=2)
    lq = torch.randint(0, ncls, (M,), generator=g)
    lb = torch.randint(0, ncls, (maps, seg), generator=g)
    lb[0, :bank_block] = lq[q_sets * nblk * q_block - 1]        # an empty negative set for some rows of the last set's map 0 users
    lb[1, :bank_block] = lq[0]
    return q, lq, bank, lb


GEOMS = [  # q_sets, nblk, q_block, nb, bank_block, C, gmap
    (1, 3, 7, 3, 9, 16, [[0, 1, 2, 3, 4]]),
    (2, 2, 5, 2, 11, 24, [[1, 2, 3], [0, 2, 3]]),
    (2, 3, 4, 1, 13, 8, [[1, 2], [0, 2]]),                    # one bank block for every query block
    (1, 1, 6, 1, 1, 8, [[1]]),
]


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}x{g[2]}-{g[3]}x{g[4]}")
def test_scores_loss_and_gradient_agree_with_the_oracle_in_float64(geom):
    """pos / all / rowmax / lse against oracle.bank_scores; loss and d loss / d q (pair_loss's analytic derivative through class_sums and
    bank_dq) against torch autograd of oracle.bank_contrast_loss."""
    q_sets, nblk, q_block, nb, bank_block, C, gmap = geom
    maps = max(max(r) for r in gmap) + 1
    q, lq, bank, lb = _rand_case(C, q_sets, nblk, q_block, nb, bank_block, C, maps)
    if nb == nblk:
        sc = R.bank_scores(q, lq, bank, lb, gmap, q_block, bank_block, inv_tau=7.0)
        op, on, om, ol = O.bank_scores(q, lq, bank, lb, gmap, q_block, bank_block, inv_tau=7.0)
        for got, want in ((sc.pos, op), (sc.all - sc.pos, on), (sc.rowmax, om), (sc.lse, ol)):
            np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=1e-13)
    else:                                                      # the forward spells this geometry as ONE query block per set
        sc = R.bank_scores(q, lq, bank, lb, gmap, nblk * q_block, bank_block)
    qo = q.clone().requires_grad_(True)
    lo = O.bank_contrast_loss(qo, lq, bank, lb, gmap, q_block, bank_block)
    lo.backward()
    cnt = R.label_counts(lq, lb, gmap, q_block, bank_block, 6)
    loss, dpos, dneg = R.pair_loss(sc.pos, sc.all, cnt, q_sets, bank_block)
    dq = R.bank_dq(dpos, dneg, cnt, lq, R.class_sums(bank, lb, bank_block, 6), gmap, q_block, bank_block)
    assert (cnt == bank_block).any() or bank_block == 1
    assert abs(loss - float(lo.detach())) <= 1e-12 * abs(float(lo.detach()))
    np.testing.assert_allclose(dq, qo.grad.numpy(), rtol=1e-9, atol=1e-12 * float(qo.grad.abs().max()))


def test_pair_loss_derivative_is_the_autograd_derivative():
    g = torch.Generator().manual_seed(1)
    M, groups, visible = 14, 3, 9
    cnt = torch.randint(0, visible + 1, (M, groups), generator=g).double()
    cnt[0], cnt[1] = 0.0, float(visible)
    pos = (torch.randn(M, groups, generator=g, dtype=F64) * cnt * 0.3).requires_grad_(True)
    neg = (torch.randn(M, groups, generator=g, dtype=F64) * (visible - cnt) * 0.3).requires_grad_(True)
    P = pos.sum(-1) / (cnt.sum(-1) + 1e-6)
    N = (neg / ((visible - cnt) + 1e-6)).sum(-1)
    ref = (-torch.log(torch.exp(P) / (torch.exp(P) + torch.exp(N)) + 1e-6)).view(2, -1).mean(1).sum()
    (3.0 * ref).backward()
    loss, dpos, dneg = R.pair_loss(pos.detach(), (pos + neg).detach(), cnt, 2, visible, dloss=3.0)
    assert abs(loss - float(ref)) <= 1e-13 * abs(float(ref))
    np.testing.assert_allclose(dpos, pos.grad.numpy(), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(dneg, neg.grad.numpy(), rtol=1e-10, atol=1e-15)


@pytest.mark.parametrize("views,HW,samples,C", [(2, 5, 3, 64), (6, 3, 2, 8), (1, 7, 1, 16)])
def test_rownorm_scatter_is_normalize_and_its_autograd(views, HW, samples, C):
    g = torch.Generator().manual_seed(views)
    R_ = views * HW * samples
    x = torch.randn(R_, C, generator=g, dtype=F64) * 3
    x[1] = 0
    xr = x.clone().requires_grad_(True)
    y = F.normalize(xr, dim=1).view(samples, views, HW, C).permute(1, 0, 2, 3).reshape(R_, C)
    dy = torch.randn(R_, C, generator=g, dtype=F64)
    y.backward(dy)
    Y, inv = R.rownorm_scatter(x, views, HW, samples)
    np.testing.assert_allclose(Y, y.detach().numpy(), rtol=1e-14, atol=0)
    assert inv[1] == 1e12 and not Y[R.out_row(1, views, HW, samples)].any()
    np.testing.assert_allclose(R.rownorm_scatter_bwd(x, dy, views, HW, samples), xr.grad.numpy(), rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("Hs,Ws,h,w", [(64, 80, 8, 10), (50, 37, 7, 9), (7, 9, 16, 20), (512, 512, 32, 32)])
def test_labels_resize_is_atens_nearest(Hs, Ws, h, w):
    g = torch.Generator().manual_seed(Hs)
    masks = [torch.randint(0, 12, (2, 1, Hs, Ws), generator=g).float() for _ in range(3)]
    masks[0][0, 0, :Hs // 2] = 3.9
    masks[1][1, 0, :, :Ws // 2] = -0.5                        # truncates to 0, where a floor would give -1
    masks[2][0, 0, Hs // 2:] = 255.0
    want = torch.stack([F.interpolate(m, size=[h, w], mode="nearest").reshape(-1).to(torch.int32) for m in masks], 0)
    got = R.labels_resize([m.numpy() for m in masks], h, w)
    assert np.array_equal(got, want.numpy())
    assert {3, 0, 255} <= set(np.unique(got).tolist()) and got.min() == 0


def test_label_counts_clamps_like_the_documented_rule():
    lq = np.array([-3, 0, 2, 8, 1, 2], np.int64)
    lb = np.array([[0, -1, 2, 9, 2, 2], [1, 1, 0, 0, 7, 2]], np.int64)
    cnt = R.label_counts(lq, lb, [[0, 1]], 3, 3, 3)
    assert cnt.tolist() == [[2, 1], [2, 1], [1, 0], [3, 2], [0, 0], [3, 2]]


# ---------------------------------------------------------------------------------------------------------------- recorded outputs
def test_reference_reproduces_the_recorded_regression_loss_and_gradient():
    g = gu.load("regression_loss.npz")
    n, c, h, w = [int(v) for v in g["shape"]]
    HW = h * w
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(n * HW, c).double()          # noqa: E731
    feats = [tok(F.normalize(gu.det_tensor(f"regression/f{i}", (n, c, h, w)), dim=1)) for i in range(6)]
    labs = [torch.from_numpy(g[f"l{i}"]).reshape(n * HW).long() for i in range(6)]
    bank, lb, gmap = torch.stack(feats[1:], 0), torch.stack(labs[1:], 0), [[0, 1, 2, 3, 4]]
    sc = R.bank_scores(feats[0], labs[0], bank, lb, gmap, HW, HW)
    cnt = R.label_counts(labs[0], lb, gmap, HW, HW, 12)
    loss, dpos, dneg = R.pair_loss(sc.pos, sc.all, cnt, 1, HW)
    dq = R.bank_dq(dpos, dneg, cnt, labs[0], R.class_sums(bank, lb, HW, 12), gmap, HW, HW)
    assert abs(loss - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    want = torch.from_numpy(g["dq"]).permute(0, 2, 3, 1).reshape(n * HW, c).double().numpy()
    assert np.linalg.norm(dq - want) <= 1e-4 * np.linalg.norm(want)


def test_reference_reproduces_the_recorded_consistency_loss():
    """The loss tail of the recorded ConsistencyLoss step: embeddings from the oracle's encoders (none of the loss code), then
    labels_resize, label_counts, bank_scores and pair_loss of the reference with both directions as two query sets."""
    g = gu.load("consistency.npz")
    sd = gu.det_fill(gu.skeleton_sd(g["keys"], g["shapes"], g["dtypes"]))
    hh, ww = [int(v) for v in g["hw"]]
    ims = [gu.det_tensor(f"consistency/im{i}", (2, 4, 3, hh, ww)) for i in range(6)]
    masks = [torch.floor(gu.det_tensor(f"consistency/mask{i}", (2, 1, hh // 8, ww // 8), "uniform", 12.0))
             .clamp(0, 11).repeat_interleave(8, 2).repeat_interleave(8, 3) for i in range(6)]
    with torch.no_grad():
        preds = [O.pixel_embed(ims[i], sd, "pixpro.", False) for i in range(2)]
        O.momentum_update(sd, "pixpro.", [str(k) for k in g["param_keys"]], O.ema_momentum(int(g["k0"]), int(g["big_k"])))
        keys = [O.pixel_embed(im, sd, "pixpro.", True) for im in ims]
    n, c, h, w = preds[0].shape
    HW = h * w
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(n * HW, c).double()          # noqa: E731
    lb = R.labels_resize([m.numpy() for m in masks], h, w)
    q, lq = torch.cat([tok(preds[0]), tok(preds[1])], 0), np.concatenate([lb[0], lb[1]])
    bank, gmap = torch.stack([tok(k) for k in keys], 0), [[1, 2, 3, 4, 5], [0, 2, 3, 4, 5]]
    sc = R.bank_scores(q, lq, bank, lb, gmap, HW, HW)
    loss, _, _ = R.pair_loss(sc.pos, sc.all, R.label_counts(lq, lb, gmap, HW, HW, 12), 2, HW)
    assert abs(loss - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _mutated(monkeypatch, name, nb, fn, gmap):
    """fn(gmap) under mutation `name` of the reference (None where the mutation does not exist for this geometry)."""
    patch, gm = CC.mutations(R)[name]
    if name == "next-block" and nb == 1:
        return None
    if gm is not None:
        if gm(gmap) == [list(r) for r in gmap]:
            return None
        return fn(gm(gmap))
    with monkeypatch.context() as mp:
        for k, v in patch(nb).items():
            mp.setattr(R, k, v)
        return fn(gmap)


FWD_MUTATIONS = ["drop-last-row", "one-row-past", "labels-one-row-off", "gmap-swapped", "next-block"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("kind,case", [("exact", c) for c in CC.EXACT_BANK] + [("round", c) for c in CC.ROUND_BANK], ids=lambda v: getattr(v, "name", v))
def test_every_mutation_moves_a_checked_output_of_bank_fwd(kind, case, dtype, monkeypatch):
    d = CC.bank_inputs(case, dtype, kind)
    Q, bank = CC.wide(d["Q"]), CC.wide(d["bank"])
    inv_tau = CC.INV_TAU if kind == "round" else 0.5
    run = lambda gm: R.bank_scores(Q, d["lq"], bank, d["lb"], gm, case.q_block, case.bank_block, inv_tau)      # noqa: E731
    base = run(d["gmap"])
    if case.bank_block == 1100:
        assert CC.planned_splits(d["M"], case.q_sets, case.q_block, 1100, case.groups) == (3, 384) and 1100 - 2 * 384 not in (0, 384)
    for name in FWD_MUTATIONS:
        mut = _mutated(monkeypatch, name, case.nblk, run, d["gmap"])
        if mut is None:
            continue
        if kind == "exact":
            moved = any(not np.array_equal(a, b) for a, b in ((base.pos, mut.pos), (base.all, mut.all), (base.rowmax, mut.rowmax)))
        else:
            with np.errstate(invalid="ignore"):
                moved = bool((np.abs(mut.pos - base.pos) > 4 * CC.sum_bound(d["C"], case.bank_block, base.abspos)).any() or
                             (np.abs(mut.all - base.all) > 4 * CC.sum_bound(d["C"], case.bank_block, base.absum)).any() or
                             (np.abs(mut.rowmax - base.rowmax) > 4 * CC.rowmax_bound(d["C"], inv_tau, base.amax)).any() or
                             (np.abs(mut.lse - base.lse) > 4 * CC.LSE_ALLOW).any())
            if name == "drop-last-row":                       # the planted key: losing it moves lse by far more than the allowance
                assert float(np.nanmax(np.abs(mut.lse - base.lse))) > 1.0 > 4 * CC.LSE_ALLOW
                assert float(base.rowmax.max()) > 0.98 * inv_tau and inv_tau >= 20
        assert moved, (case.name, dtype, name)


@pytest.mark.parametrize("C,ncls,bank_block,nb,dtype", CC.CLASS_SUMS)
def test_every_mutation_moves_class_sums(C, ncls, bank_block, nb, dtype, monkeypatch):
    bank, lb = CC.class_sums_inputs(C, ncls, bank_block, nb, dtype)
    run = lambda gm: R.class_sums(CC.wide(bank), lb, bank_block, ncls)         # noqa: E731
    base = run(None)
    assert not base[0, 0, ncls - 1].any() or ncls == 1         # the absent class: an exactly-zero row
    assert float(np.abs(base).max()) < 2 ** 24
    for name in ["drop-last-row", "one-row-past", "labels-one-row-off", "next-block"]:
        mut = _mutated(monkeypatch, name, nb, run, [[0]])
        assert mut is None or not np.array_equal(mut, base), (name,)


@pytest.mark.parametrize("case", CC.BANK_DQ, ids=str)
def test_every_mutation_moves_bank_dq(case, monkeypatch):
    q_sets, nblk, q_block, nb, bank_block, C, groups, ncls = case
    bank, lb, lq, gmap, dpos, dneg = CC.bank_dq_inputs(*case)
    cnt = R.label_counts(lq, lb, gmap, q_block, bank_block, ncls)
    assert (cnt == bank_block).any() and ((cnt == bank_block - 1).any() or groups == 1)
    dneg = np.where(cnt == bank_block, 1e30, CC.wide(dneg))
    run = lambda gm: R.bank_dq(dpos, dneg, cnt, lq, R.class_sums(bank, lb, bank_block, ncls), gm, q_block, bank_block)      # noqa: E731
    base = run(gmap)
    assert float(np.abs(base).max()) < 2 ** 24
    for name in ["drop-last-row", "labels-one-row-off", "gmap-swapped", "next-block", "skip-negative-at-visible-1"]:
        if name == "skip-negative-at-visible-1" and not (cnt == bank_block - 1).any():
            continue
        mut = _mutated(monkeypatch, name, nb, run, gmap)
        assert mut is None or not np.array_equal(mut, base), (name,)
