"""Case tables, inputs and tolerances of tests/test_hip_contrast_contract.py, kept apart from it (no GPU, no project imports) so that
tests/test_contrast_ref.py can show on the CPU, for the very same inputs, that a subtly wrong kernel would be caught.

Inputs are torch CPU tensors in the storage dtype; wide(t) gives the float64 numpy array tests/contrast_ref.py takes.
  exact cases    Q / bank entries are integers in [-2, 2]: every dtype stores them exactly, every score and sum is an integer
                 below 2^24, so fp32 sums in ANY order are exact - the comparison has no tolerance.  They carry the geometry edges.
  rounding cases L2-normalised random rows rounded to the dtype, a key equal to a query (score ~1) planted in the LAST row of every
                 bank block (with bank_block % 128 != 0: the last row of the last, ragged, bank tile), inv_tau = 20.
"""
from collections import namedtuple

import numpy as np
import torch

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
SPLITS_MAX = 64                     # the launcher's cap on bank splits
U24 = 2.0 ** -24                    # unit round-off of fp32


def wide(t):
    return t.detach().cpu().to(torch.float64).numpy()


# ---------------------------------------------------------------------------------------------------------------- bank_fwd
# name, q_sets, nblk, q_block, bank_block, groups, gmap (None: sets use maps [0..g) resp. [1..g]), C per dtype, ldb pad (raw entry)
BankCase = namedtuple("BankCase", "name q_sets nblk q_block bank_block groups gmap C_bf16 C_f32 ldb_pad")


def _bc(name, q_sets, nblk, q_block, bank_block, groups, C_bf16, C_f32, gmap=None, ldb_pad=0):
    return BankCase(name, q_sets, nblk, q_block, bank_block, groups, gmap, C_bf16, C_f32, ldb_pad)


# q_block 1 / 63 / 128 / 129 / 240, bank_block 1 / 63 / 127 / 128 / 129 / 1100, groups 1 / 5 / 8, every C, two sets sharing maps,
# blocks smaller than the 128-row tile with several blocks (63), one query block against a whole segment (1100: 3 splits, the last
# one ragged - planned_splits below), bank row pitch > C through the raw entry point
EXACT_BANK = [
    _bc("one-row", 1, 1, 1, 1, 1, 64, 32, gmap=[[1]]),
    _bc("sets-share-maps-63", 2, 3, 63, 63, 5, 256, 256, gmap=[[1, 2, 3, 4, 5], [0, 2, 3, 4, 5]]),
    _bc("128x127", 1, 2, 128, 127, 5, 128, 64, ldb_pad=8),
    _bc("129x128", 1, 2, 129, 128, 8, 192, 128),
    _bc("240x129", 1, 1, 240, 129, 5, 64, 32, ldb_pad=16),
    _bc("block-vs-segment-1100", 1, 1, 63, 1100, 1, 192, 64),
    _bc("two-sets-1100", 2, 1, 240, 1100, 8, 256, 256, gmap=[[0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 2, 1, 0]]),
    _bc("q1-blocks-129", 1, 3, 1, 129, 5, 128, 128),
    _bc("two-sets-129x63", 2, 2, 129, 63, 1, 64, 32, gmap=[[1], [0]]),
]
ROUND_BANK = [
    _bc("r-1100", 1, 1, 63, 1100, 1, 256, 256),
    _bc("r-129", 2, 2, 129, 129, 5, 192, 32, gmap=[[1, 2, 3, 4, 5], [0, 2, 3, 4, 5]]),
    _bc("r-63", 1, 3, 63, 63, 8, 128, 64),
    _bc("r-127", 1, 1, 240, 127, 5, 64, 128, ldb_pad=8),
]
INV_TAU = 20.0
NCLS = 5

# log-sum-exp: the kernel uses the hardware exp2 / log, so the allowance is MEASURED (MI355X, float64 reference, every ROUND_BANK
# case, both dtypes, both forms; lse ~ 20, where fp32 numbers are 1.9e-6 apart): the largest error seen is 3.57e-6 (r-1100 bf16,
# fixed-reference form; online form 3.03e-6), 4 x that = 1.43e-5, rounded up to a power of two = 2^-16 = 1.53e-5.
LSE_MEASURED_MAX = 3.57e-6
LSE_ALLOW = 2.0 ** -16


def gmap_of(case):
    if case.gmap is not None:
        return [list(r) for r in case.gmap]
    return [list(range(s, s + case.groups)) for s in range(case.q_sets)]


def bank_inputs(case, dtype, kind):
    """-> dict(Qw [M][ldq] (the wider matrix), Q = its column slice, lq, bank, lb, gmap, C, M, seg, maps)."""
    C = case.C_bf16 if dtype == "bf16" else case.C_f32
    gmap = gmap_of(case)
    maps = max(max(r) for r in gmap) + 1
    M, seg = case.q_sets * case.nblk * case.q_block, case.nblk * case.bank_block
    g = torch.Generator().manual_seed(sum(map(ord, case.name + dtype + kind)))
    ldq = C + (8 if dtype == "bf16" else 4) * 3                     # a column slice at a 16-byte aligned offset of a wider matrix
    off = ldq - C - (8 if dtype == "bf16" else 4)
    if kind == "exact":
        Qw = torch.randint(-2, 3, (M, ldq), generator=g).to(DT[dtype])
        bank = torch.randint(-2, 3, (maps, seg, C), generator=g).to(DT[dtype])
    else:
        Qw = torch.randn(M, ldq, generator=g)
        Qw[:, off:off + C] = torch.nn.functional.normalize(Qw[:, off:off + C], dim=1)
        Qw = Qw.to(DT[dtype])
        bank = torch.nn.functional.normalize(torch.randn(maps, seg, C, generator=g), dim=2).to(DT[dtype])
        for b in range(case.nblk):                                  # the planted key: query row 0 of block b (set 0) as the last row
            bank[:, (b + 1) * case.bank_block - 1] = Qw[b * case.q_block, off:off + C]
    lq = torch.randint(0, NCLS, (M,), generator=g, dtype=torch.int32)
    lb = torch.randint(0, NCLS, (maps, seg), generator=g, dtype=torch.int32)
    if case.bank_block > 2:
        lb[gmap[0][0], :case.bank_block // 2] = lq[0]               # block 0 of group 0: a large positive set for query 0
    else:                                                           # neighbouring rows never share a label; query 0 matches its first key
        lb = (torch.arange(maps * seg, dtype=torch.int32) % NCLS).view(maps, seg)
        lq[0] = lb[gmap[0][0], 0]
    return dict(Qw=Qw, off=off, Q=Qw[:, off:off + C], lq=lq, bank=bank, lb=lb, gmap=gmap, C=C, M=M, seg=seg, maps=maps)


def planned_splits(M, q_sets, q_block, bank_block, groups, workspace_floats=1 << 22):
    """CPU copy of the launcher's split planner (contrast_bank_fwd_impl) -> (splits, rows per split)."""
    nblk = M // (q_sets * q_block)
    row_tiles = q_sets * nblk * ((q_block + 127) // 128)
    tiles_total = (bank_block + 127) // 128
    splits, best = 1, -1
    for sp in range(1, min(max(tiles_total // 2, 1), SPLITS_MAX) + 1):
        rounds = (row_tiles * groups * sp + 255) // 256
        cost = rounds * ((tiles_total + sp - 1) // sp + 2)
        if best < 0 or cost < best:
            best, splits = cost, sp
    while splits > 1 and 4 * M * groups * splits > workspace_floats:
        splits -= 1
    return splits, ((bank_block + splits - 1) // splits + 127) // 128 * 128


def sum_bound(C, bank_block, absum):
    """|fp32 sum - exact| for a sum of bank_block scores of C exact products each, combined over at most SPLITS_MAX partials."""
    return (C + bank_block + SPLITS_MAX) * U24 * absum


def rowmax_bound(C, inv_tau, amax):
    """One score is an fp32 sum of C exact products (error <= C u sum_c |q_c k_c|), then one rounded product with inv_tau."""
    return (C + 1) * U24 * inv_tau * amax


# ---------------------------------------------------------------------------------------------------------------- class_sums
# C, ncls, bank_block, nb, dtype: C % 64 != 0 (12), 512, ncls 1 / 63, bank_block 1000 = several row chunks per block
CLASS_SUMS = [(12, 1, 1, 3, "f32"), (64, 12, 63, 1, "bf16"), (192, 63, 64, 3, "bf16"), (256, 12, 65, 3, "f32"),
              (512, 63, 1000, 1, "f32"), (512, 12, 1000, 3, "bf16"), (12, 63, 65, 1, "bf16"), (256, 1, 64, 1, "f32")]


def class_sums_inputs(C, ncls, bank_block, nb, dtype):
    """Integer bank rows, maps = 2.  Block 0 of map 0 lacks class ncls - 1 (with ncls = 1: holds class 0 only); the last block of
    map 1 is all one class; map 0 also holds the labels -1 and ncls + 2, which class_sums counts in the total only."""
    g = torch.Generator().manual_seed(C * 1000 + ncls * 10 + bank_block + nb)
    seg = nb * bank_block
    bank = torch.randint(-2, 3, (2, seg, C), generator=g).to(DT[dtype])
    lb = torch.randint(0, ncls, (2, seg), generator=g, dtype=torch.int32)
    blk0 = lb[0, :bank_block]
    blk0[blk0 == ncls - 1] = max(ncls - 2, 0)
    lb[1, seg - bank_block:] = ncls // 2
    lb[0, 0::3] = torch.where(torch.arange(0, seg, 3) % 2 == 0, -1, ncls + 2).to(torch.int32)
    return bank, lb


# ---------------------------------------------------------------------------------------------------------------- bank_dq
# q_sets, nblk, q_block, nb, bank_block, C, groups, ncls: one bank block per query block / one for all, both set counts
BANK_DQ = [(1, 3, 5, 3, 7, 64, 5, 12), (2, 3, 5, 1, 9, 256, 3, 12), (2, 2, 4, 2, 6, 12, 8, 63), (1, 2, 7, 2, 4, 512, 1, 2)]


def bank_dq_inputs(q_sets, nblk, q_block, nb, bank_block, C, groups, ncls, exact=True):
    """bank (integers, or unit rows when not exact), labels with one group of query row 0 wholly of its class (cnt == bank_block: the
    row's dneg there is 1e30) and another all but one row (cnt == bank_block - 1), small-integer dpos / dneg."""
    g = torch.Generator().manual_seed(q_sets * 7 + nblk * 5 + C + groups)
    maps, M, seg = groups + q_sets - 1, q_sets * nblk * q_block, nb * bank_block
    gmap = [list(range(s, s + groups)) for s in range(q_sets)]
    bank = torch.randint(-2, 3, (maps, seg, C), generator=g).float() if exact else \
        torch.nn.functional.normalize(torch.randn(maps, seg, C, generator=g), dim=2)
    lq = torch.randint(0, ncls, (M,), generator=g, dtype=torch.int32)
    lb = torch.randint(0, ncls, (maps, seg), generator=g, dtype=torch.int32)
    lb[gmap[0][0], :bank_block] = lq[0]
    if groups > 1:
        lb[gmap[0][-1], :bank_block - 1] = lq[0]
        lb[gmap[0][-1], bank_block - 1] = (int(lq[0]) + 1) % ncls
    dpos = torch.randint(-3, 4, (M, groups), generator=g).float()
    dneg = torch.randint(1, 4, (M, groups), generator=g).float()
    return bank, lb, lq, gmap, dpos, dneg


# ---------------------------------------------------------------------------------------------------------------- mutations
# (the ways a tiled kernel goes subtly wrong; tests/test_contrast_ref.py applies each to the reference)
def mutations(R):
    """name -> (patch dict for the hooks of contrast_ref R, gmap transform or None)."""
    rows = R._bank_rows

    def swap(gmap):
        gm = [list(r) for r in gmap]
        if len(gm[0]) > 1:
            gm[0][0], gm[0][1] = gm[0][1], gm[0][0]
        elif len(gm) > 1:
            gm[0][0], gm[1][0] = gm[1][0], gm[0][0]
        return gm

    def next_block(nb):
        return lambda mp, blk, seg, bb: rows(mp, (blk + 1) % nb, seg, bb)

    return {
        "drop-last-row": (lambda nb: dict(_bank_rows=lambda mp, blk, seg, bb: rows(mp, blk, seg, bb)[:-1],
                                          _label_rows=lambda mp, blk, seg, bb: rows(mp, blk, seg, bb)[:-1]), None),
        "one-row-past": (lambda nb: dict(_bank_rows=lambda mp, blk, seg, bb: np.append(rows(mp, blk, seg, bb), mp * seg + (blk + 1) * bb),
                                         _label_rows=lambda mp, blk, seg, bb: np.append(rows(mp, blk, seg, bb), mp * seg + (blk + 1) * bb)),
                         None),
        "labels-one-row-off": (lambda nb: dict(_label_rows=lambda mp, blk, seg, bb: rows(mp, blk, seg, bb) + 1), None),
        "gmap-swapped": (lambda nb: {}, swap),
        "next-block": (lambda nb: dict(_bank_rows=next_block(nb), _label_rows=next_block(nb)), None),
        "skip-negative-at-visible-1": (lambda nb: dict(_negative_set_empty=lambda cnt, vis: cnt >= vis - 1), None),
    }
