"""Shared constructions of the run-length tests (tests/test_rle_host.py, tests/test_hip_rle.py): the definition of utils.rle.encode as a
plain loop, a brute-force binary RLE of a dense mask, and the map patterns.  numpy only."""
import numpy as np


def loop_encode(m, cap):
    """One map [H][W] -> (runs, count) by a plain Python loop over m.T.ravel()."""
    v = m.T.ravel().tolist()
    starts = [p for p in range(len(v)) if p == 0 or v[p] != v[p - 1]]
    runs = np.zeros((cap, 2), dtype=np.int32)
    for i, p in enumerate(starts[:cap]):
        runs[i] = (p, v[p])
    return runs, len(starts)


def brute_counts(mask):
    """COCO's uncompressed counts of a dense binary mask [H][W]: column-major, alternating off / on, the first run off (may be 0)."""
    out, cur, n = [], 0, 0
    for b in mask.T.ravel().tolist():
        if bool(b) != bool(cur):
            out.append(n)
            cur, n = 1 - cur, 0
        n += 1
    return out + [n]


def counts_to_mask(counts, H, W):
    """The dense mask bool [H][W] of uncompressed counts."""
    assert sum(counts) == H * W and all(c >= 0 for c in counts), counts
    v = np.repeat(np.arange(len(counts)) % 2 == 1, counts)
    return v.reshape(W, H).T


def small_maps():
    """The host tests' maps: H x W in {1x1, 1x7, 7x1, 5x9, 33x17}, int32 with values in {-1, 0, 1, 2} and uint8 up to 255."""
    g = np.random.default_rng(3)
    out = []
    for H, W in ((1, 1), (1, 7), (7, 1), (5, 9), (33, 17)):
        out.append(g.integers(-1, 3, (H, W)).astype(np.int32))
        out.append(np.repeat(g.integers(-1, 3, (H, (W + 2) // 3)), 3, axis=1)[:, :W].astype(np.int32))     # longer runs
        out.append(g.integers(0, 256, (H, W)).astype(np.uint8))
        out.append(np.where(g.random((H, W)) < 0.3, 255, 0).astype(np.uint8))
    return out


def _as(m, dtype, big):
    """Values {-1, 0, 1, 2, ...} in the element type: uint8 wraps -1 to 255; `big` puts int32 values at and above 2^20."""
    if dtype == np.uint8:
        return (m & 255).astype(np.uint8)
    return np.where(m > 0, m + big, m).astype(np.int32)


def hstripe_edges(H, SH):
    """The rows at which the `hstripes` pattern changes value, ascending: row 1, the rows before, on and after the first two segment
    edges, and the last row - those of them that a map of H rows has."""
    return sorted({e for e in (1, SH - 1, SH, SH + 1, 2 * SH - 1, 2 * SH, 2 * SH + 1, H - 1) if 0 < e < H})


def patterns(n, H, W, dtype, SH, seed=0):
    """name -> maps [n][H][W] of `dtype`.  SH: the rows of a segment of the kernel (stripes end on, before and after its edges)."""
    g = np.random.default_rng(seed + 131 * H + W)
    ys, xs = np.mgrid[:H, :W]
    out = {}
    out["constant"] = np.full((n, H, W), 3, dtype=dtype)
    # alternating in p = x H + y, so that the bottom of a column differs from the top of the next for even H too: R = H W
    out["checkerboard"] = _as(np.broadcast_to((xs * H + ys) % 2 * 3 - 1, (n, H, W)).copy(), dtype, 0)   # -1 / 2 (uint8: 255 / 2)
    # vertical stripes one column wide in which every other column pair shares a value: with H odd or even, the bottom of a column
    # and the top of the next are equal for half of the pairs, so runs carry over
    v = np.broadcast_to(((xs + 1) // 2) % 3, (n, H, W)).copy()
    v[:, H - 1, ::4] = 2                                  # ... and some bottoms differ from their own column but equal the next top
    v[:, 0, 1::4] = 2
    out["vstripes"] = _as(v, dtype, 1 << 20)
    h = np.zeros((n, H, W), dtype=np.int64)
    for k, edge in enumerate(hstripe_edges(H, SH)):       # ascending: the band from row `edge` to the next edge has its own value,
        h[:, edge:] = np.where((xs[edge:] % 5 == 0) & (k % 2 == 1), 7, (k + 1) % 3)     # every fifth column of every other band another
    out["hstripes"] = _as(h, dtype, 0)
    blobs = np.kron(g.integers(-1, 3, (n, (H + 4) // 5, (W + 6) // 7)), np.ones((5, 7), dtype=np.int64))[:, :H, :W]
    out["blobs"] = _as(blobs, dtype, 0)                   # coarse random blobs with values {-1, 0, 1, 2} (uint8: 255 for -1)
    out["big"] = _as(blobs, dtype, (1 << 20) + 12345)     # int32 values >= 2^20
    if n > 1:                                             # frames of one call with different counts
        mixed = out["blobs"].copy()
        mixed[0] = out["constant"][0]
        mixed[-1] = out["checkerboard"][-1]
        out["mixed"] = mixed
    return out
