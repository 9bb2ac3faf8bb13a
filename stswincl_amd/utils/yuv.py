"""YUV frames as a video source delivers them <-> RGB: the host statement (numpy, int64) of stswin_yuv_to_rgb / stswin_rgb_to_nv12
(include/stswin_hip.h), which the kernels reproduce to the bit.

A conversion is an int32 [3][4] matrix: per output channel three coefficients in units of 2^-14 and an offset that already holds the
rounding half, applied to a triple t as

    clamp((m[c][0] t0 + m[c][1] t1 + m[c][2] t2 + m[c][3]) >> 14, 0, 255)          (>> is the arithmetic shift: a floor)

to_rgb_matrix takes (Y, U, V) to (R, G, B), to_yuv_matrix (R, G, B) to (Y, U, V), for BT.709 or BT.601 in limited (Y 16 .. 235,
chroma 16 .. 240) or full range.

Layouts (Hs and Ws even):
    nv12  uint8 [n][3 Hs / 2][Ws]: rows 0 .. Hs-1 luma, then Hs / 2 rows of Ws / 2 interleaved (U, V) pairs
    uyvy  uint8 [n][Hs][Ws][2]: the four bytes of pixel pair (2k, 2k+1) are U, Y0, V, Y1

Chroma reconstruction, C[j][k] one chroma plane: "replicate" gives pixel (y, x) C[y >> 1][x >> 1] (nv12) or C[y][x >> 1] (uyvy).
"linear" (MPEG-2 siting: co-sited with the even columns, vertically centred between two rows) first interpolates nv12 vertically,
row 2j: (3 C[j][k] + C[max(j-1, 0)][k] + 2) >> 2, row 2j+1: (3 C[j][k] + C[min(j+1, Hs/2 - 1)][k] + 2) >> 2 (uyvy: the row's own
chroma), then horizontally, x = 2k: V[k], x = 2k+1: (V[k] + V[min(k+1, Ws/2 - 1)] + 1) >> 1.

The arithmetic is this project's own (14-bit matrix, floor); it is not pinned to swscale or to a hardware decoder's converter.
"""
from __future__ import annotations

import numpy as np

SHIFT = 14
STANDARDS = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}        # Kr, Kb
FORMATS = ("nv12", "uyvy")
CHROMA = ("replicate", "linear")


def _constants(standard: str, full_range: bool):
    if standard not in STANDARDS:
        raise ValueError(f"standard must be one of {sorted(STANDARDS)}, got {standard!r}")
    kr, kb = STANDARDS[standard]
    ys, cs, y_off = (1.0, 1.0, 0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16)
    return kr, 1.0 - kr - kb, kb, ys, cs, y_off


def to_rgb_matrix(standard: str = "bt709", full_range: bool = False) -> np.ndarray:
    """int32 [3][4]: (Y, U, V) -> (R, G, B)."""
    kr, kg, kb, ys, cs, y_off = _constants(standard, full_range)
    coef = np.array([[1.0 / ys, 0.0, 2.0 * (1.0 - kr) / cs],
                     [1.0 / ys, -2.0 * kb * (1.0 - kb) / kg / cs, -2.0 * kr * (1.0 - kr) / kg / cs],
                     [1.0 / ys, 2.0 * (1.0 - kb) / cs, 0.0]], dtype=np.float64)
    m = np.rint(coef * (1 << SHIFT)).astype(np.int64)
    off = -(m[:, 0] * y_off + (m[:, 1] + m[:, 2]) * 128) + (1 << (SHIFT - 1))
    return np.concatenate([m, off[:, None]], axis=1).astype(np.int32)


def to_yuv_matrix(standard: str = "bt709", full_range: bool = False) -> np.ndarray:
    """int32 [3][4]: (R, G, B) -> (Y, U, V).  Each chroma row's coefficients sum to 0 and the luma row's to rint(ys 2^14) (the green
    coefficient takes what rounding leaves), so every grey gives U = V = 128 exactly."""
    kr, kg, kb, ys, cs, y_off = _constants(standard, full_range)
    coef = np.array([[ys * kr, ys * kg, ys * kb],
                     [-cs * kr / (2.0 * (1.0 - kb)), -cs * kg / (2.0 * (1.0 - kb)), cs * 0.5],
                     [cs * 0.5, -cs * kg / (2.0 * (1.0 - kr)), -cs * kb / (2.0 * (1.0 - kr))]], dtype=np.float64)
    m = np.rint(coef * (1 << SHIFT)).astype(np.int64)
    sums = np.array([int(np.rint(ys * (1 << SHIFT))), 0, 0], dtype=np.int64)
    m[:, 1] += sums - m.sum(axis=1)
    off = np.array([y_off, 128, 128], dtype=np.int64) * (1 << SHIFT) + (1 << (SHIFT - 1))
    return np.concatenate([m, off[:, None]], axis=1).astype(np.int32)


def apply_matrix(matrix, t0, t1, t2) -> np.ndarray:
    """The three output channels of a matrix for triples (t0, t1, t2) (arrays of one shape): uint8 [..., 3]."""
    m = np.asarray(matrix).astype(np.int64)
    if m.shape != (3, 4):
        raise ValueError(f"a conversion matrix is int32 [3][4], got {m.shape}")
    t0, t1, t2 = (np.asarray(t).astype(np.int64) for t in (t0, t1, t2))
    out = [np.clip((m[c, 0] * t0 + m[c, 1] * t1 + m[c, 2] * t2 + m[c, 3]) >> SHIFT, 0, 255) for c in range(3)]
    return np.stack(out, axis=-1).astype(np.uint8)


def _horizontal(v: np.ndarray, chroma: str) -> np.ndarray:
    """int64 [n][rows][Ws / 2] chroma per pair -> [n][rows][Ws] per pixel."""
    if chroma == "replicate":
        return np.repeat(v, 2, axis=2)
    nxt = np.concatenate([v[:, :, 1:], v[:, :, -1:]], axis=2)
    out = np.empty(v.shape[:2] + (2 * v.shape[2],), dtype=np.int64)
    out[:, :, 0::2] = v
    out[:, :, 1::2] = (v + nxt + 1) >> 1
    return out


def _vertical(c: np.ndarray, chroma: str) -> np.ndarray:
    """nv12: int64 [n][Hs / 2][k] chroma rows -> [n][Hs][k]."""
    if chroma == "replicate":
        return np.repeat(c, 2, axis=1)
    up = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    down = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((c.shape[0], 2 * c.shape[1], c.shape[2]), dtype=np.int64)
    out[:, 0::2] = (3 * c + up + 2) >> 2
    out[:, 1::2] = (3 * c + down + 2) >> 2
    return out


def yuv_to_rgb(frames, fmt: str, matrix, chroma: str = "replicate") -> np.ndarray:
    """nv12 uint8 [n][3 Hs / 2][Ws] or uyvy uint8 [n][Hs][Ws][2] -> RGB uint8 [n][Hs][Ws][3]."""
    frames = np.asarray(frames)
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {FORMATS}, got {fmt!r}")
    if chroma not in CHROMA:
        raise ValueError(f"chroma must be one of {CHROMA}, got {chroma!r}")
    if frames.dtype != np.uint8:
        raise ValueError(f"frames must be uint8, got {frames.dtype}")
    if fmt == "nv12":
        if frames.ndim != 3 or frames.shape[1] % 3 or frames.shape[2] % 2 or frames.size == 0:
            raise ValueError(f"nv12 frames are uint8 [n][3 Hs / 2][Ws] with Hs and Ws even, got {frames.shape}")
        n, Ws = frames.shape[0], frames.shape[2]
        Hs = frames.shape[1] // 3 * 2
        y = frames[:, :Hs].astype(np.int64)
        uv = frames[:, Hs:].astype(np.int64).reshape(n, Hs // 2, Ws // 2, 2)
        u, v = (_horizontal(_vertical(uv[..., i], chroma), chroma) for i in range(2))
    else:
        if frames.ndim != 4 or frames.shape[3] != 2 or frames.shape[2] % 2 or frames.size == 0:
            raise ValueError(f"uyvy frames are uint8 [n][Hs][Ws][2] with Ws even, got {frames.shape}")
        n, Hs, Ws = frames.shape[:3]
        q = frames.astype(np.int64).reshape(n, Hs, Ws // 2, 4)
        y = q[..., 1::2].reshape(n, Hs, Ws)
        u, v = _horizontal(q[..., 0], chroma), _horizontal(q[..., 2], chroma)
    return apply_matrix(matrix, y, u, v)


def rgb_to_nv12(rgb, matrix) -> np.ndarray:
    """RGB uint8 [n][Hs][Ws][3] (Hs, Ws even) -> nv12 uint8 [n][3 Hs / 2][Ws]: luma per pixel from row 0 of the matrix, chroma from
    rows 1 and 2 applied to the 2 x 2 block's per-channel mean (sum of four + 2) >> 2."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3 or rgb.shape[1] % 2 or rgb.shape[2] % 2 or rgb.size == 0:
        raise ValueError(f"rgb must be uint8 [n][Hs][Ws][3] with Hs and Ws even, got {rgb.dtype} {rgb.shape}")
    n, Hs, Ws, _ = rgb.shape
    p = rgb.astype(np.int64)
    out = np.empty((n, Hs * 3 // 2, Ws), dtype=np.uint8)
    out[:, :Hs] = apply_matrix(matrix, p[..., 0], p[..., 1], p[..., 2])[..., 0]
    mean = (p.reshape(n, Hs // 2, 2, Ws // 2, 2, 3).sum(axis=(2, 4)) + 2) >> 2
    out[:, Hs:] = apply_matrix(matrix, mean[..., 0], mean[..., 1], mean[..., 2])[..., 1:].reshape(n, Hs // 2, Ws)
    return out
