"""Float64 reference of the pixel-contrast loss kernels (stswincl_amd/csrc/contrast.hip), written from the definitions in
include/stswin_hip.h: no tiling, no splits, no project imports, nothing shared with oracle/.

Every function takes exactly the operands its kernel takes - values ALREADY rounded to the storage dtype, then widened - as numpy
arrays (anything np.asarray accepts) and computes in float64 / int64:

  bank_scores      stswin_contrast_bank_fwd / _unit (and, with one query set of per-sample blocks, stswin_contrast_fwd)
  class_sums       stswin_contrast_class_sums
  bank_dq          stswin_contrast_bank_dq
  label_counts     stswin_label_counts
  pair_loss        stswin_pair_loss and stswin_pair_loss_bwd (analytic derivative)
  rownorm_scatter  stswin_rownorm_scatter and _bwd (with the clip-major -> view-major row map)
  labels_resize    stswin_labels_resize

Geometry (the header's): the M query rows are q_sets equal sets of nblk = M / (q_sets q_block) blocks of q_block rows; the bank is
[maps][seg][C] with nb = seg / bank_block blocks per map; a query of block b of set s sees, as its group g, rows
[b' bank_block, (b' + 1) bank_block) of map gmap[s][g], b' = b if nb > 1 else 0.

The three module-level hooks _bank_rows, _label_rows and _negative_set_empty are the places a kernel's indexing can go wrong;
tests/test_contrast_ref.py replaces them to show that the GPU tests would notice (they are not part of the reference's interface).
"""
from collections import namedtuple

import numpy as np

F64 = np.float64
Scores = namedtuple("Scores", "pos all rowmax lse absum abspos amax")


def geometry(M, q_sets, q_block, seg, bank_block):
    """-> (nblk, nb); raises on a geometry the header does not define."""
    if q_sets < 1 or q_block < 1 or bank_block < 1 or M % (q_sets * q_block) or seg % bank_block:
        raise ValueError(f"M = {M} is not {q_sets} sets of {q_block}-row blocks, or seg = {seg} not blocks of {bank_block}")
    nblk, nb = M // (q_sets * q_block), seg // bank_block
    if nb != nblk and nb != 1:
        raise ValueError(f"{nb} bank blocks for {nblk} query blocks")
    return nblk, nb


def _bank_rows(mp, blk, seg, bank_block):
    """Flat row numbers (into the [maps * seg] row list) of the rows of map mp a query of bank block blk sees."""
    return mp * seg + blk * bank_block + np.arange(bank_block)


def _label_rows(mp, blk, seg, bank_block):
    """Flat numbers of the labels that belong to _bank_rows(...): the same rows."""
    return mp * seg + blk * bank_block + np.arange(bank_block)


def _negative_set_empty(cnt, visible):
    """The negative set of a (query, group) is empty when every visible row carries the query's label."""
    return cnt == visible


def _visible(bank, lb, mp, blk, bank_block):
    maps, seg, C = bank.shape
    total = maps * seg
    K = bank.reshape(total, C)[_bank_rows(mp, blk, seg, bank_block) % total]
    L = lb.reshape(total)[_label_rows(mp, blk, seg, bank_block) % total]
    return K, L


def bank_scores(Q, lq, bank, lb, gmap, q_block, bank_block, inv_tau=1.0):
    """pos[m][g] = sum_p S[m][p] [lq[m] == lb[p]] and all[m][g] = sum_p S[m][p] over the visible rows p of group g, S = q_m . k_p;
    rowmax[m] / lse[m] = max / log-sum-exp of inv_tau S[m][p] over the visible rows of ALL groups; absum[m][g] = sum_p sum_c |q_mc k_pc|
    (the magnitude an fp32 summation error scales with), abspos the same over the label-equal rows only, amax[m] = max_p sum_c |q_mc k_pc|
    over the visible rows of all groups (the same for a single score).  An empty visible set has rowmax = lse = -inf."""
    Q, bank = np.asarray(Q, F64), np.asarray(bank, F64)
    lq, lb = np.asarray(lq, np.int64), np.asarray(lb, np.int64)
    M, C = Q.shape
    maps, seg, _ = bank.shape
    q_sets, groups = len(gmap), len(gmap[0])
    nblk, nb = geometry(M, q_sets, q_block, seg, bank_block)
    pos, tot, absum, abspos = (np.zeros((M, groups), F64) for _ in range(4))
    rowmax, lse, amax = np.zeros(M, F64), np.zeros(M, F64), np.zeros(M, F64)
    for s in range(q_sets):
        for b in range(nblk):
            r0 = (s * nblk + b) * q_block
            sl = slice(r0, r0 + q_block)
            scores, mags = [], []
            for g, mp in enumerate(gmap[s]):
                if not 0 <= mp < maps:
                    raise ValueError(f"gmap entry {mp} for {maps} maps")
                K, L = _visible(bank, lb, mp, b if nb > 1 else 0, bank_block)
                S = Q[sl] @ K.T
                A = np.abs(Q[sl]) @ np.abs(K).T
                same = lq[sl, None] == L[None, :]
                pos[sl, g], tot[sl, g] = (S * same).sum(1), S.sum(1)
                abspos[sl, g], absum[sl, g] = (A * same).sum(1), A.sum(1)
                scores.append(S)
                mags.append(A)
            Z = float(inv_tau) * np.concatenate(scores, 1)
            amax[sl] = np.concatenate(mags, 1).max(1, initial=0.0)
            rowmax[sl] = Z.max(1, initial=-np.inf)
            with np.errstate(divide="ignore", invalid="ignore"):
                lse[sl] = np.where(np.isfinite(rowmax[sl]), rowmax[sl] + np.log(np.exp(Z - rowmax[sl, None]).sum(1)), -np.inf)
    return Scores(pos, tot, rowmax, lse, absum, abspos, amax)


def class_sums(bank, lb, bank_block, ncls):
    """ksum [maps][seg / bank_block][ncls + 1][C]: per bank block the sum of the rows of each class, slot ncls = the sum of all rows;
    a row whose label lies outside [0, ncls) counts in the total only."""
    bank, lb = np.asarray(bank, F64), np.asarray(lb, np.int64)
    maps, seg, C = bank.shape
    if seg % bank_block:
        raise ValueError("seg % bank_block")
    nb = seg // bank_block
    ksum = np.zeros((maps, nb, ncls + 1, C), F64)
    for mp in range(maps):
        for b in range(nb):
            K, L = _visible(bank, lb, mp, b, bank_block)
            for c in range(ncls):
                ksum[mp, b, c] = K[L == c].sum(0)
            ksum[mp, b, ncls] = K.sum(0)
    return ksum


def bank_dq(dpos, dneg, cnt, lq, ksum, gmap, q_block, bank_block):
    """dq[m] = sum_g dpos[m][g] Kcls + dneg[m][g] (Ktot - Kcls) with Kcls = ksum[gmap[s][g]][blk][lq[m]] (zero for a label outside
    [0, ncls)) and Ktot = ksum[..][ncls]; the dneg term is skipped where cnt[m][g] == bank_block (an empty negative set)."""
    dpos, dneg, cnt, ksum = (np.asarray(a, F64) for a in (dpos, dneg, cnt, ksum))
    lq = np.asarray(lq, np.int64)
    M, groups = dpos.shape
    _, nb, ncls1, C = ksum.shape
    ncls, q_sets = ncls1 - 1, len(gmap)
    nblk, _ = geometry(M, q_sets, q_block, nb * bank_block, bank_block)
    dq = np.zeros((M, C), F64)
    for m in range(M):
        s, b = m // (nblk * q_block), (m % (nblk * q_block)) // q_block
        for g, mp in enumerate(gmap[s]):
            tab = ksum[mp, b if nb > 1 else 0]
            kc = tab[lq[m]] if 0 <= lq[m] < ncls else np.zeros(C, F64)
            dq[m] += dpos[m, g] * kc
            if not _negative_set_empty(cnt[m, g], bank_block):
                dq[m] += dneg[m, g] * (tab[ncls] - kc)
    return dq


def label_counts(lq, lb, gmap, q_block, bank_block, ncls):
    """cnt[m][g] (int64) = visible rows of group g whose label equals lq[m], both clamped to [0, ncls - 1] first."""
    lq = np.clip(np.asarray(lq, np.int64), 0, ncls - 1)
    lb = np.clip(np.asarray(lb, np.int64), 0, ncls - 1)
    M, (maps, seg), q_sets = lq.shape[0], lb.shape, len(gmap)
    nblk, nb = geometry(M, q_sets, q_block, seg, bank_block)
    cnt = np.zeros((M, len(gmap[0])), np.int64)
    for m in range(M):
        s, b = m // (nblk * q_block), (m % (nblk * q_block)) // q_block
        for g, mp in enumerate(gmap[s]):
            b0 = (b if nb > 1 else 0) * bank_block
            cnt[m, g] = int((lb[mp, b0:b0 + bank_block] == lq[m]).sum())
    return cnt


def pair_loss(pos, tot, cnt, q_sets, visible, dloss=1.0):
    """loss = sum over the query sets of mean(-log(e^P / (e^P + e^N) + 1e-6)), P = sum_g pos_g / (sum_g cnt_g + 1e-6),
    N = sum_g (all_g - pos_g) / (visible - cnt_g + 1e-6) -> (loss, d loss / d pos, d loss / d (all - pos)), the derivatives times dloss."""
    pos, tot, cnt = (np.asarray(a, F64) for a in (pos, tot, cnt))
    M, _ = pos.shape
    if M % q_sets:
        raise ValueError("M % q_sets")
    per_set = M // q_sets
    csum = cnt.sum(1)
    den_n = (visible - cnt) + 1e-6
    P = pos.sum(1) / (csum + 1e-6)
    N = ((tot - pos) / den_n).sum(1)
    s = 1.0 / (1.0 + np.exp(N - P))                       # e^P / (e^P + e^N)
    term = -np.log(s + 1e-6)
    loss = float(term.reshape(q_sets, per_set).mean(1).sum())
    dP = -(s * (1.0 - s)) / (s + 1e-6) * (float(dloss) / per_set)       # d term / d P; d term / d N = -d term / d P
    dpos = np.repeat((dP / (csum + 1e-6))[:, None], pos.shape[1], 1)
    dneg = -dP[:, None] / den_n
    return loss, dpos, dneg


def out_row(r, views, HW, samples):
    """Row of the view-major [views][samples * HW] matrix that clip-major row r = (sample * views + view) * HW + pixel lands in."""
    clip, px = divmod(int(r), HW)
    sample, view = divmod(clip, views)
    return (view * samples + sample) * HW + px


def rownorm_scatter(X, views, HW, samples):
    """Y[out_row(r)] = X[r] / max(||X[r]||_2, 1e-12) -> (Y, inv) with inv[r] = 1 / max(||X[r]||, 1e-12)."""
    X = np.asarray(X, F64)
    R, _ = X.shape
    if R != views * HW * samples:
        raise ValueError("R != views * samples * HW")
    inv = 1.0 / np.maximum(np.sqrt((X * X).sum(1)), 1e-12)
    Y = np.zeros_like(X)
    for r in range(R):
        Y[out_row(r, views, HW, samples)] = X[r] * inv[r]
    return Y, inv


def rownorm_scatter_bwd(X, dY, views, HW, samples):
    """dX[r] = inv (dy - y (y . dy)) with y = X[r] inv and dy = dY[out_row(r)] (a row at the 1e-12 floor has y = 0: dX = inv dy)."""
    X, dY = np.asarray(X, F64), np.asarray(dY, F64)
    Y, inv = rownorm_scatter(X, views, HW, samples)
    dX = np.zeros_like(X)
    for r in range(X.shape[0]):
        o = out_row(r, views, HW, samples)
        dX[r] = inv[r] * (dY[o] - Y[o] * float(Y[o] @ dY[o]))
    return dX


def labels_resize(masks, h, w):
    """float label maps [N][1][Hs][Ws] -> int32 [maps][N * h * w]: source index min(floor(dst * scale), in - 1) with the fp32 scale
    (float)in / (float)out and an fp32 product, then truncation toward zero."""
    out = []
    for m in masks:
        m = np.asarray(m, np.float32)
        N, _, Hs, Ws = m.shape
        sy, sx = np.float32(Hs) / np.float32(h), np.float32(Ws) / np.float32(w)
        ys = [min(int(np.floor(np.float32(y) * sy)), Hs - 1) for y in range(h)]
        xs = [min(int(np.floor(np.float32(x) * sx)), Ws - 1) for x in range(w)]
        out.append(np.trunc(m[:, 0][:, ys][:, :, xs]).astype(np.int32).reshape(N * h * w))
    return np.stack(out, 0)
