"""numpy statement of CaDIS's Gaussian noise as stswincl_amd.augment computes it (stswin_augment_noise): the reference of the noise
pass between the two stages of tests/augment_ref.py.

The reference transform (segcata/dataset/CATA_new_512.py:178-183) stores (255 * clip(u / 255. + n, 0, 1)).astype('uint8') with
n ~ N(0, var), var = 0.001.  For a byte u that is clamp(u + floor(255 n), 0, 255): the integer offset K = floor(255 n) has
P(K <= k) = Phi((k + 1) / s), s = 255 sqrt(var).  Defined here, not pinned to skimage (not available): the law at 2^-32 resolution
(thresholds) and the random stream, Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", Random123) keyed by
the sample's 64-bit key and counted by the byte index - the reference's own stream is unseeded."""
from __future__ import annotations

import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments per round
_MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]           # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [x.astype(np.uint32) for x in c]


def thresholds(var: float = 0.001):
    """-> (uint32 thr ascending, k_min): t_k = floor(Phi((k + 1) / s) 2^32 + 0.5) for the k with 0 < t_k < 2^32; with r uniform on
    32 bits, K = k_min + #{j : thr[j] <= r}.  Strictly ascending: a threshold that rounds to its outer neighbour's value is moved to one
    past it, so every offset in range keeps a probability >= 2^-32."""
    s = 255.0 * math.sqrt(var)
    ks, ts = [], []
    for k in range(-int(12 * s) - 4, int(12 * s) + 5):
        t = int(math.floor(0.5 * (1.0 + math.erf((k + 1) / s / math.sqrt(2.0))) * 2.0 ** 32 + 0.5))
        if 0 < t < 2 ** 32:
            ks.append(k)
            ts.append(t)
    assert ks == list(range(ks[0], ks[0] + len(ks)))
    t = np.array(ts, dtype=np.int64)                       # ties far out in the tails are separated by one, away from the nearer end
    low = t < 2 ** 31
    t[low] = np.maximum.accumulate(t[low] - np.arange(low.sum())) + np.arange(low.sum())
    high = t[~low][::-1]
    t[~low] = (np.minimum.accumulate(high + np.arange(high.size)) - np.arange(high.size))[::-1]
    return t.astype(np.uint32), ks[0]


def pmf(var: float = 0.001):
    """The law the thresholds state, exactly: -> (k values int64 [n + 1], probabilities float64 [n + 1]), P(K = k_min + j) =
    (thr[j] - thr[j - 1]) / 2^32 with thr[-1] = 0 and thr[n] = 2^32 (j thresholds are <= r)."""
    thr, k_min = thresholds(var)
    edges = np.concatenate([[0], thr.astype(np.int64), [1 << 32]])
    return np.arange(k_min, k_min + len(thr) + 1, dtype=np.int64), np.diff(edges) / 2.0 ** 32


def clamped_pmf(u: int, var: float = 0.001) -> np.ndarray:
    """P(clamp(u + K, 0, 255) = v) for v = 0 .. 255."""
    ks, p = pmf(var)
    out = np.zeros(256)
    np.add.at(out, np.clip(u + ks, 0, 255), p)
    return out


def offsets(n: int, key: int, var: float = 0.001) -> np.ndarray:
    """K of bytes 0 .. n - 1 of a sample with the 64-bit `key` (int64 [n]); n a multiple of 4.  Bytes 4c .. 4c + 3 take the four
    output words of counter (c, 0, 0, 0) under the key (low half, high half)."""
    assert n % 4 == 0 and 0 <= key < 1 << 64
    thr, k_min = thresholds(var)
    w = philox4x32_10((np.arange(n // 4, dtype=np.uint64), 0, 0, 0), (key & 0xffffffff, key >> 32))
    r = np.stack(w, axis=1).reshape(-1)
    return k_min + np.searchsorted(thr, r, side="right").astype(np.int64)


def add_noise(crops_u8: np.ndarray, key: int, var: float = 0.001) -> np.ndarray:
    """One sample: uint8 crops of any shape, taken as its bytes in C order -> the same shape with the noise of `key` added."""
    a = np.ascontiguousarray(crops_u8)
    assert a.dtype == np.uint8
    v = a.reshape(-1).astype(np.int64) + offsets(a.size, key, var)
    return np.clip(v, 0, 255).astype(np.uint8).reshape(a.shape)
