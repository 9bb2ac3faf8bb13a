"""Named pairs of label maps for the boundary scores (utils.boundary.boundary_counts, hip.boundary_counts): what each pattern is for is
asserted by the tests that use it.  numpy only."""
import numpy as np


def _ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[0:H, 0:W]
    return ((y - cy) / max(ry, 0.5)) ** 2 + ((x - cx) / max(rx, 0.5)) ** 2 <= 1.0


def blob_maps(n, H, W, nc, seed, blobs=7, moved=True):
    """(gt, pred): `blobs` ellipses on a background of class 0, of the classes (1 + 3 k) mod (nc - 1) and the last one, a small one, of
    class nc - 1, which no other has; pred holds every second one moved by a few pixels and resized, and the last one half the image
    away: distances for the tail bins."""
    g = np.random.default_rng(seed)
    gt, pred = np.zeros((n, H, W), dtype=np.int64), np.zeros((n, H, W), dtype=np.int64)
    for f in range(n):
        for k in range(blobs):
            last = k == blobs - 1
            c = nc - 1 if last else (1 + 3 * k) % max(1, nc - 1)
            cy, cx = g.integers(0, H), g.integers(0, W)
            ry, rx = g.integers(1, max(2, H // 5)), g.integers(1, max(2, W // 5))
            if last:
                ry, rx = min(ry, 3), min(rx, 3)
            gt[f][_ellipse(H, W, cy, cx, ry, rx)] = c
            if moved and k % 2:
                cy, cx, ry, rx = cy + g.integers(-4, 5), cx + g.integers(-6, 7), ry + g.integers(0, 3), rx + g.integers(-1, 2)
            if moved and last:
                cy, cx = (cy + H // 2) % H, (cx + W // 2) % W
            pred[f][_ellipse(H, W, cy, cx, ry, rx)] = c
    return gt, pred.astype(np.uint8)


def patterns(n, H, W, nc, geometry, seed=0):
    """name -> (gt int64 [n][H][W], pred uint8 [n][H][W]) for maps of nc >= 2 classes; geometry = hip.boundary_geometry()."""
    TH, TW = geometry[0], geometry[1]
    a = 1 % nc                                                       # the classes the line patterns draw in
    b = 2 if nc > 2 else a
    top = nc - 1
    out = {}
    out["blobs"] = blob_maps(n, H, W, nc, seed)
    eq = blob_maps(n, H, W, nc, seed + 1, moved=False)
    out["equal"] = eq
    gt, pred = np.zeros((n, H, W), dtype=np.int64), np.zeros((n, H, W), dtype=np.uint8)
    gt[:, 0, 0] = top
    pred[:, H - 1, W - 1] = top
    out["far"] = (gt, pred)
    y, x = np.mgrid[0:H, 0:W]
    gt = np.ascontiguousarray(np.broadcast_to(((y + x) % 2) * a, (n, H, W)), dtype=np.int64)
    pred = np.zeros((n, H, W), dtype=np.uint8)
    pred[:, H - 1, W - 1] = a
    out["checker_vs_dot"] = (gt, pred)
    gt, pred = np.zeros((n, H, W), dtype=np.int64), np.zeros((n, H, W), dtype=np.uint8)
    for m, t in ((gt, 2), (pred, 1)):                                # a frame of class a along the image border, t pixels thick
        m[:, :t, :] = m[:, -t:, :] = m[:, :, :t] = m[:, :, -t:] = a
    out["border"] = (gt, pred)
    gt, pred = blob_maps(n, H, W, nc, seed + 2)
    only = _ellipse(H, W, H // 2, W // 2, max(1, H // 4), max(1, W // 4))
    g2, p2 = gt.copy(), pred.copy()
    g2[g2 == top] = 0
    p2[p2 == top] = 0
    g2[:, only] = top
    out["absent_pred"] = (g2, p2)                                    # class top in the ground truth alone
    g3, p3 = gt.copy(), pred.copy()
    g3[g3 == top] = 0
    p3[p3 == top] = 0
    p3[:, only] = top
    out["absent_gt"] = (g3, p3)
    gt, pred = blob_maps(n, H, W, nc, seed + 3)
    gt, pred = gt.copy(), pred.copy()
    gt[:, : (H + 1) // 2, : (W + 2) // 3] = 255                      # values that are no class: they bound their neighbours' contours
    gt[:, H // 2:, W // 2:][:, ::2, ::3] = -1
    gt[:, 0, W - 1] = nc
    pred[:, H // 3:, : (W + 1) // 2][:, ::3, ::2] = 255
    if nc < 255:
        pred[:, H - 1, 0] = nc
    out["out_of_range"] = (gt, pred)
    gt, pred = np.zeros((n, H, W), dtype=np.int64), np.zeros((n, H, W), dtype=np.uint8)
    for e in range(TW, W, TW):                                       # class a: gt ends on the last column of a tile, pred starts the next
        gt[:, : max(1, H - 2), max(0, e - 2):e] = a
        pred[:, min(1, H - 1):, e:e + 2] = a
    for e in range(TH, H, TH):                                       # class b: gt on the last row of a tile, pred on the row behind the edge
        gt[:, e - 1, W // 3:] = b
        pred[:, min(H - 1, e + 1), : max(1, 2 * W // 3)] = b
        pred[:, e, : max(1, W // 5)] = b
    gt[:, H - 1, W - 1] = top                                        # something everywhere, also where no tile edge exists
    pred[:, 0, 0] = top
    out["tile_edges"] = (gt, pred)
    gt, pred = np.full((n, H, W), a, dtype=np.int64), np.full((n, H, W), a, dtype=np.uint8)
    pred[1::2, H // 2, W // 2] = 0                                   # every second frame: a hole, one more contour
    out["full"] = (gt, pred)
    return out


def nearest_pairs(own, other):
    """Pixel lists [k][2], [m][2] -> per own pixel the index of a nearest pixel of other (brute force)."""
    d = own[:, None, :].astype(np.int64) - other[None, :, :].astype(np.int64)
    return (d * d).sum(axis=2).argmin(axis=1)
