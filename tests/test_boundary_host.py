"""utils.boundary on the CPU: boundary_counts against the scipy recipe (binary_erosion + distance_transform_edt, the one MONAI's
surface metrics use) on every pattern of boundary_cases, hand-computed cases, the exact ceiling, BoundaryScores against a plain
restatement."""
import math

import numpy as np
import pytest

import boundary_cases as BC
from stswincl_amd.utils import boundary as B

GEO = (32, 64, 64, 64)           # the patterns only need some tile size here (the GPU tests pass the library's)
SHAPES = [(1, 1, 1), (2, 1, 70), (1, 70, 1), (2, 37, 53), (1, 65, 130)]


def _scipy_counts(gt, pred, nc, bins, skip=()):
    """The recipe: edges = mask & ~binary_erosion(mask); distances of the own edge pixels in distance_transform_edt(~other edges);
    squared and rounded (a float64 root of an integer below 2^30, squared, rounds back to the integer); the ceiling by integer
    correction."""
    from scipy import ndimage
    n = gt.shape[0]
    out = np.zeros((n, nc, 2, 2 + bins), dtype=np.int32)
    for f in range(n):
        for c in range(nc):
            if c in skip:
                continue
            edges = []
            for m in (gt[f] == c, pred[f] == c):
                edges.append(m & ~ndimage.binary_erosion(m))
            for d in range(2):
                own, other = edges[d], edges[1 - d]
                out[f, c, d, 0] = own.sum()
                out[f, c, d, 1] = -1
                if own.any() and other.any():
                    dist = ndimage.distance_transform_edt(~other)[own]
                    d2 = np.rint(dist * dist).astype(np.int64)
                    k = np.ceil(dist).astype(np.int64)
                    k -= (k > 0) & ((k - 1) ** 2 >= d2)
                    k += k * k < d2
                    out[f, c, d, 1] = d2.max()
                    out[f, c, d, 2:] = np.bincount(np.minimum(k, bins - 1), minlength=bins)
    return out


def _brute(gt, pred, nc, bins):
    """The statement itself, pixel by pixel (tiny maps only)."""
    n, H, W = gt.shape
    out = np.zeros((n, nc, 2, 2 + bins), dtype=np.int32)

    def edge(m, c, y, x):
        return m[y, x] == c and any(not (0 <= v < H and 0 <= u < W) or m[v, u] != c for v, u in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)))

    for f in range(n):
        for c in range(nc):
            pts = [[(y, x) for y in range(H) for x in range(W) if edge(m[f], c, y, x)] for m in (gt, pred)]
            for d in range(2):
                out[f, c, d, 0] = len(pts[d])
                out[f, c, d, 1] = -1
                if pts[d] and pts[1 - d]:
                    for y, x in pts[d]:
                        d2 = min((y - v) ** 2 + (x - u) ** 2 for v, u in pts[1 - d])
                        out[f, c, d, 1] = max(out[f, c, d, 1], d2)
                        k = 0
                        while k * k < d2:
                            k += 1
                        out[f, c, d, 2 + min(k, bins - 1)] += 1
    return out


@pytest.mark.parametrize("nc", [2, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_definition_is_the_scipy_recipe_on_every_pattern(shape, nc):
    n, H, W = shape
    pats = BC.patterns(n, H, W, nc, GEO, seed=H + W)
    assert sorted(pats) == sorted(["blobs", "equal", "far", "checker_vs_dot", "border", "absent_pred", "absent_gt", "out_of_range",
                                   "tile_edges", "full"])
    for name, (gt, pred) in pats.items():
        assert gt.dtype == np.int64 and pred.dtype == np.uint8 and gt.shape == pred.shape == shape
        for bins, skip in ((16, ()), (2, (0,)), (256, (nc - 1,))):
            got = B.boundary_counts(gt, pred, nc, bins, skip)
            assert got.dtype == np.int32 and got.shape == (n, nc, 2, 2 + bins)
            assert np.array_equal(got, _scipy_counts(gt, pred, nc, bins, skip)), (name, bins, skip)
            assert not got[:, list(skip)].any()
        if name == "out_of_range" and H * W >= 70:
            assert (gt == 255).any() and (gt == -1).any()


@pytest.mark.parametrize("shape", [(2, 9, 13), (1, 1, 7), (1, 12, 5)])
def test_brute_force_scipy_and_the_definition_agree_on_blobs(shape):
    n, H, W = shape
    tails = 0
    for seed in range(3):
        gt, pred = BC.blob_maps(n, H, W, 4, seed, blobs=4)
        want = _brute(gt, pred, 4, 3)
        assert np.array_equal(B.boundary_counts(gt, pred, 4, 3), want) and np.array_equal(_scipy_counts(gt, pred, 4, 3), want)
        tails += int(want[..., -1].sum())
    assert tails > 0 or H * W < 10


def test_tail_bins_hold_counts_at_16_bins_on_the_blob_maps():
    for n, H, W in SHAPES[3:]:
        gt, pred = BC.patterns(n, H, W, 5, GEO, seed=H + W)["blobs"]
        got = B.boundary_counts(gt, pred, 5, 16)
        assert got[..., -1].sum() > 0 and np.array_equal(got, _scipy_counts(gt, pred, 5, 16))


def test_two_parallel_lines_three_apart():
    gt, pred = np.zeros((1, 9, 20), dtype=np.int64), np.zeros((1, 9, 20), dtype=np.uint8)
    gt[0, 2, :] = 1
    pred[0, 5, :] = 1
    got = B.boundary_counts(gt, pred, 2, 8, skip=(0,))
    assert got[0, 1, :, 0].tolist() == [20, 20] and got[0, 1, :, 1].tolist() == [9, 9]
    assert got[0, 1, 0, 2:].tolist() == [0, 0, 0, 20, 0, 0, 0, 0] and not got[0, 0].any()
    s = B.BoundaryScores.from_counts(got)
    assert s.nsd(2) == [[[1, 0.0]]] and s.nsd(3) == [[[1, 1.0]]] and s.hausdorff() == [[[1, 3.0]]]
    assert s.hausdorff_percentile(95) == [[[1, 3.0]]]


def test_equal_maps():
    gt, _ = BC.blob_maps(2, 30, 40, 5, 3)
    got = B.boundary_counts(gt, gt.astype(np.uint8), 5)
    s = B.BoundaryScores.from_counts(got)
    for f in range(2):
        assert len(s.nsd(0)[f]) >= 2
        assert all(v == 1.0 for _, v in s.nsd(0)[f]) and all(v == 0.0 for _, v in s.hausdorff()[f])
    assert np.array_equal(got[:, :, 0], got[:, :, 1]) and (got[..., 1] <= 0).all()


def test_ceiling_is_exact_next_to_large_squares():
    ks = np.array([1, 2, 3, 1000, 4097, 16383, 23169, 32767], dtype=np.int64)
    for k in ks.tolist():
        got = B.ceil_sqrt(np.array([k * k - 1, k * k, k * k + 1])).tolist()
        assert got == [k if k * k - 1 > (k - 1) ** 2 else k - 1, k, k + 1], k
        assert got == [math.isqrt(v - 1) + 1 if v else 0 for v in (k * k - 1, k * k, k * k + 1)]
    assert B.ceil_sqrt(np.array([0, 1, 2, 3, 4, 5])).tolist() == [0, 1, 2, 2, 2, 3]
    # a far pair at the largest size class: d2 from the definition, bins clip it into the tail
    gt, pred = np.zeros((1, 3, 4000), dtype=np.int64), np.zeros((1, 3, 4000), dtype=np.uint8)
    gt[0, 0, 0] = pred[0, 2, 3999] = 1
    got = B.boundary_counts(gt, pred, 2, 256, skip=(0,))
    assert got[0, 1, :, 1].tolist() == [3999 ** 2 + 4] * 2 and got[0, 1, :, -1].tolist() == [1, 1]


def _plain(counts, sequences, values):
    """The aggregates, restated: values[f] = {class: value} for the scored classes of row f."""
    nc = counts.shape[1]
    nseq = max(sequences) + 1
    frame_means, each, tool = [], [0.0] * nc, [0] * nc
    for f, v in enumerate(values):
        for c, x in v.items():
            each[c] += x
            tool[c] += 1
        frame_means.append(sum(v.values()) / len(v) if v else float("nan"))
    per_seq = []
    for s in range(nseq):
        rows = [m for m, q in zip(frame_means, sequences) if q == s]
        per_seq.append(sum(rows) / len(rows) if rows else float("nan"))
    return (sum(frame_means) / len(frame_means), per_seq, [e / t if t else float("nan") for e, t in zip(each, tool)], tool,
            [f for f, v in enumerate(values) if not v])


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= 1e-12 * np.abs(b))))


def test_scores_and_aggregates_match_a_plain_restatement():
    nc, bins = 5, 8
    maps = [BC.patterns(1, 37, 53, nc, GEO, seed=s) for s in range(2)]
    pairs = [maps[0]["blobs"], maps[0]["absent_pred"], maps[1]["blobs"], maps[0]["far"], maps[1]["equal"]]
    empty = (np.zeros((1, 37, 53), dtype=np.int64), np.ones((1, 37, 53), dtype=np.uint8))       # gt: background alone
    pairs.append(empty)
    counts = np.concatenate([B.boundary_counts(g, p, nc, bins, skip=(0,)) for g, p in pairs])
    sequences, frames = [0, 0, 0, 1, 1, 2], [0, 1, 2, 0, 1, 0]
    s = B.BoundaryScores.from_counts(counts, sequences, frames)
    assert len(s) == 6 and s.classes == nc and s.bins == bins and s.frames == frames and s.empty_frames == [5]
    for f in range(6):
        assert s.scored(f) == [c for c in range(1, nc) if counts[f, c, 0, 0] > 0]
    tau = 2
    nsd = [{c: (counts[f, c, 0, 2:3 + tau].sum() + counts[f, c, 1, 2:3 + tau].sum()) / (counts[f, c, 0, 0] + counts[f, c, 1, 0])
            for c in s.scored(f)} for f in range(6)]
    hd = [{c: math.sqrt(max(counts[f, c, 0, 1], counts[f, c, 1, 1])) if counts[f, c, 1, 0] else math.inf for c in s.scored(f)}
          for f in range(6)]
    assert s.nsd(tau) == [[[c, float(v)] for c, v in row.items()] for row in nsd]
    assert s.hausdorff() == [[[c, v] for c, v in row.items()] for row in hd]
    assert nsd[1][nc - 1] == 0.0 and hd[1][nc - 1] == math.inf and counts[1, nc - 1, 0, 1] == -1      # absent in the prediction
    assert hd[3][nc - 1] == math.sqrt(36 ** 2 + 52 ** 2)

    def pct(f, c, q):                                        # nearest rank per direction, whole pixels, inf in the tail bin
        worst = 0.0
        for d in range(2):
            r = counts[f, c, d]
            if r[1] < 0:
                return math.inf
            k = next(k for k in range(bins) if r[2:3 + k].sum() * 100 >= q * r[0])
            worst = max(worst, math.inf if k == bins - 1 else float(k))
        return worst

    for q in (50, 95, 100):
        assert s.hausdorff_percentile(q) == [[[c, pct(f, c, q)] for c in s.scored(f)] for f in range(6)], q
    assert s.hausdorff_percentile(100)[3] == [[nc - 1, math.inf]]                               # the far pair sits in the tail bin
    for lists, values in ((s.nsd(tau), nsd), (s.hausdorff(), hd)):
        agg, want = s.aggregate(lists), _plain(counts, sequences, values)
        assert _same(agg.mean, want[0]) and _same(agg.per_sequence, want[1]) and _same(agg.each, want[2])
        assert agg.tool_each.tolist() == want[3] == s.tool_each.tolist() and agg.empty_frames == want[4] == [5]
        assert math.isnan(agg.mean) and math.isnan(agg.per_sequence[2]) and math.isnan(agg.each[0])
    assert math.isinf(s.aggregate(s.hausdorff()).per_sequence[0]) and 0 < s.aggregate(s.nsd(tau)).per_sequence[0] < 1
    rows = s.as_rows(names=[f"class {c}" for c in range(nc)], tau=tau)
    assert len(rows) == sum(len(r) for r in nsd)
    assert rows[0] == {"sequence": 0, "frame": 0, "class": s.scored(0)[0], "name": f"class {s.scored(0)[0]}",
                       "gt_pixels": int(counts[0, s.scored(0)[0], 0, 0]), "pred_pixels": int(counts[0, s.scored(0)[0], 1, 0]),
                       "nsd": float(nsd[0][s.scored(0)[0]]), "hausdorff": hd[0][s.scored(0)[0]],
                       "hausdorff_percentile": pct(0, s.scored(0)[0], 95)}
    for bad in (-1, bins - 1, 1.5, True):
        with pytest.raises(ValueError, match="tau"):
            s.nsd(bad)
    with pytest.raises(ValueError, match="counts"):
        B.BoundaryScores.from_counts(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="sequence"):
        B.BoundaryScores.from_counts(counts, sequences[:-1])


def test_definition_refusals():
    gt, pred = np.zeros((1, 4, 4), dtype=np.int64), np.zeros((1, 4, 4), dtype=np.uint8)
    for kw in (dict(nc=0), dict(nc=65), dict(bins=1), dict(bins=257)):
        with pytest.raises(ValueError, match="nc|bins"):
            B.boundary_counts(gt, pred, **{"nc": 2, **kw})
    with pytest.raises(ValueError, match="shape"):
        B.boundary_counts(gt, pred[:, :2], 2)
    with pytest.raises(ValueError, match="integer"):
        B.boundary_counts(gt.astype(np.float32), pred, 2)
