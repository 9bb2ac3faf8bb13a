"""Seeded mask pairs for the CaDIS metric fixture (tests/golden/cata_metrics.npz): built identically by tools/gen_golden.py, which
feeds them to the REFERENCE's segcata/utils/cata_metrics.py, and by tests/test_cata_host.py, so the fixture holds seeds and results
only."""
import numpy as np

CLASS_COUNTS = (8, 17, 25)          # cata_test.py:45, experiments 1 / 2 / 3


def mask_pairs(ncm: int, seed: int, frames: int = 3, h: int = 48, w: int = 64):
    """-> [(gt, pred)] int64 masks with values in [-1, ncm + 2] and 255: the ignore label ncm (the remapped 255 of
    CATA_new_512.py:237), predictions equal to ncm, negatives, values above the class count, and two classes (1 and ncm - 2) absent
    from both ground truth and prediction, so that their per-class values are NaN."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(frames):
        g = rng.integers(-1, ncm + 3, (h, w))
        p = rng.integers(0, ncm + 1, (h, w))
        g[: h // 6, : w // 3] = ncm                   # an ignore region
        g[-2:, :] = 255
        agree = rng.random((h, w)) < 0.4              # enough true positives for non-trivial IoU
        p[agree] = np.clip(g[agree], 0, ncm)
        for c in (1, ncm - 2):
            g[g == c] = ncm
            p[p == c] = 0
        out.append((g.astype(np.int64), p.astype(np.int64)))
    return out
