"""CPU: utils.yuv, the host statement of stswin_yuv_to_rgb / stswin_rgb_to_nv12 - the matrices, Pillow where Pillow has the same
matrix, the round trip, the layouts and the chroma reconstruction - and the two entry points' place in the ABI."""
import ctypes

import numpy as np
import pytest
from PIL import Image

from stswincl_amd import hip
from stswincl_amd.utils import yuv

PAIRS = [(s, f) for s in ("bt709", "bt601") for f in (False, True)]
# the largest |rgb -> yuv -> rgb - rgb| over all 2^24 triples, established by test_round_trip_exhaustive itself: 8-bit YUV cannot
# hold every RGB triple (limited range has 219 x 224 x 224 codes for 2^24 colours), so 0 is out of reach
ROUND_TRIP = {False: 2, True: 1}


@pytest.fixture(scope="module")
def triples():
    """All 2^24 byte triples as a uint8 picture [4096][4096][3] (read-only)."""
    v = np.arange(256, dtype=np.uint8)
    t = np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(4096, 4096, 3))
    t.setflags(write=False)
    return t


def _apply(m, t):
    return yuv.apply_matrix(m, t[..., 0], t[..., 1], t[..., 2])


def test_recorded_matrices():
    assert yuv.to_rgb_matrix("bt601", True).tolist() == [[16384, 0, 22970, -2931968], [16384, -5638, -11700, 2227456],
                                                         [16384, 29032, 0, -3707904]]
    assert yuv.to_yuv_matrix("bt709", False).tolist() == [[2991, 10064, 1016, 270336], [-1649, -5547, 7196, 2105344],
                                                          [7196, -6536, -660, 2105344]]
    for m in (yuv.to_rgb_matrix(), yuv.to_yuv_matrix()):
        assert m.dtype == np.int32 and m.shape == (3, 4)
    assert np.array_equal(yuv.to_rgb_matrix(), yuv.to_rgb_matrix("bt709", False))
    with pytest.raises(ValueError):
        yuv.to_rgb_matrix("bt2020")


@pytest.mark.parametrize("standard,full", PAIRS)
def test_matrix_rows_and_greys(standard, full):
    m = yuv.to_yuv_matrix(standard, full).astype(np.int64)
    ys = 1.0 if full else 219.0 / 255.0
    assert m[1, :3].sum() == 0 and m[2, :3].sum() == 0
    assert m[0, :3].sum() == int(np.rint(ys * (1 << 14)))
    # int32 on the device: the largest magnitude any row can reach
    for mat in (m, yuv.to_rgb_matrix(standard, full).astype(np.int64)):
        assert (np.abs(mat[:, :3]).sum(axis=1) * 255 + np.abs(mat[:, 3])).max() < 1 << 31
    g = np.arange(256)
    grey = yuv.apply_matrix(m, g, g, g)
    assert (grey[:, 1] == 128).all() and (grey[:, 2] == 128).all()
    if full:
        assert np.array_equal(grey[:, 0], g)
        back = _apply(yuv.to_rgb_matrix(standard, True), grey)
        assert np.array_equal(back, np.stack([g, g, g], -1))
    else:
        assert grey[0, 0] == 16 and grey[255, 0] == 235


def test_against_pillow_bt601_full_range_exhaustive(triples):
    """Pillow's YCbCr is BT.601 full range (JFIF) from 6-bit-fraction tables: at most one code value from the 14-bit matrix."""
    want = np.asarray(Image.fromarray(triples, "YCbCr").convert("RGB")).astype(np.int16)
    d = int(np.abs(_apply(yuv.to_rgb_matrix("bt601", True), triples).astype(np.int16) - want).max())
    print("to_rgb against Pillow: largest difference", d)
    assert d <= 1
    want = np.asarray(Image.fromarray(triples, "RGB").convert("YCbCr")).astype(np.int16)
    d = int(np.abs(_apply(yuv.to_yuv_matrix("bt601", True), triples).astype(np.int16) - want).max())
    print("to_yuv against Pillow: largest difference", d)
    assert d <= 1


@pytest.mark.parametrize("standard,full", PAIRS)
def test_round_trip_exhaustive(triples, standard, full):
    back = _apply(yuv.to_rgb_matrix(standard, full), _apply(yuv.to_yuv_matrix(standard, full), triples))
    d = int(np.abs(back.astype(np.int16) - triples.astype(np.int16)).max())
    print(standard, "full" if full else "limited", "round trip: largest error", d)
    assert d == ROUND_TRIP[full]


# ---------------------------------------------------------------------------------------------------- layouts, chroma
def _slow_yuv_to_rgb(frames, fmt, m, chroma):
    """The definition written out pixel by pixel in Python integers."""
    m = [[int(x) for x in row] for row in np.asarray(m)]
    if fmt == "nv12":
        n, Ws = frames.shape[0], frames.shape[2]
        Hs = frames.shape[1] // 3 * 2
    else:
        n, Hs, Ws = frames.shape[:3]
    out = np.zeros((n, Hs, Ws, 3), np.uint8)
    fr = frames.astype(np.int64).tolist()

    def plane(f, y, k, c):                      # chroma c of pair k for luma row y, after the vertical step
        if fmt == "uyvy":
            return fr[f][y][2 * k][0] if c == 0 else fr[f][y][2 * k + 1][0]
        C = lambda j: fr[f][Hs + j][2 * k + c]
        j = y >> 1
        if chroma == "replicate":
            return C(j)
        other = max(j - 1, 0) if y % 2 == 0 else min(j + 1, Hs // 2 - 1)
        return (3 * C(j) + C(other) + 2) >> 2

    for f in range(n):
        for y in range(Hs):
            for x in range(Ws):
                lum = fr[f][y][x] if fmt == "nv12" else fr[f][y][x][1]
                k = x >> 1
                uv = []
                for c in range(2):
                    if chroma == "replicate" or x % 2 == 0:
                        uv.append(plane(f, y, k, c))
                    else:
                        uv.append((plane(f, y, k, c) + plane(f, y, min(k + 1, Ws // 2 - 1), c) + 1) >> 1)
                for c in range(3):
                    v = (m[c][0] * lum + m[c][1] * uv[0] + m[c][2] * uv[1] + m[c][3]) >> 14
                    out[f, y, x, c] = min(max(v, 0), 255)
    return out


@pytest.mark.parametrize("chroma", ["replicate", "linear"])
@pytest.mark.parametrize("fmt", ["nv12", "uyvy"])
@pytest.mark.parametrize("Hs,Ws", [(2, 2), (4, 6), (6, 10)])
def test_layouts_and_chroma_against_the_definition(Hs, Ws, fmt, chroma):
    g = np.random.default_rng(Hs * Ws)
    shape = (2, Hs * 3 // 2, Ws) if fmt == "nv12" else (2, Hs, Ws, 2)
    frames = g.integers(0, 256, shape, dtype=np.uint8)
    m = yuv.to_rgb_matrix("bt709", False)
    got = yuv.yuv_to_rgb(frames, fmt, m, chroma)
    assert got.dtype == np.uint8 and got.shape == (2, Hs, Ws, 3)
    assert np.array_equal(got, _slow_yuv_to_rgb(frames, fmt, m, chroma))


def test_hand_built_frames():
    ident = np.array([[1 << 14, 0, 0, 0], [0, 1 << 14, 0, 0], [0, 0, 1 << 14, 0]], np.int32)     # (Y, U, V) shows through as (R, G, B)
    # nv12 4 x 6: luma 0 .. 23, chroma rows [(10, 110), (20, 120), (40, 140)] and [(50, 150), (90, 190), (170, 250)]
    nv12 = np.zeros((1, 6, 6), np.uint8)
    nv12[0, :4] = np.arange(24).reshape(4, 6)
    nv12[0, 4] = [10, 110, 20, 120, 40, 140]
    nv12[0, 5] = [50, 150, 90, 190, 170, 250]
    rep = yuv.yuv_to_rgb(nv12, "nv12", ident, "replicate")
    assert np.array_equal(rep[0, :, :, 0], np.arange(24).reshape(4, 6))
    assert rep[0, :2, :, 1].tolist() == [[10, 10, 20, 20, 40, 40]] * 2 and rep[0, 2:, :, 1].tolist() == [[50, 50, 90, 90, 170, 170]] * 2
    assert rep[0, 0, :, 2].tolist() == [110, 110, 120, 120, 140, 140]
    lin = yuv.yuv_to_rgb(nv12, "nv12", ident, "linear")
    # vertical: row 0 clamps upwards (its own chroma), row 1 = (3 a + b + 2) >> 2, row 2 = (3 b + a + 2) >> 2, row 3 clamps downwards
    u = [[10, 20, 40], [(30 + 50 + 2) >> 2, (60 + 90 + 2) >> 2, (120 + 170 + 2) >> 2],
         [(150 + 10 + 2) >> 2, (270 + 20 + 2) >> 2, (510 + 40 + 2) >> 2], [50, 90, 170]]
    for y in range(4):
        a, b, c = u[y]
        assert lin[0, y, :, 1].tolist() == [a, (a + b + 1) >> 1, b, (b + c + 1) >> 1, c, c], y      # the last column clamps to the right
    assert np.array_equal(lin[..., 0], rep[..., 0])
    # uyvy 2 x 4: bytes U Y0 V Y1
    uyvy = np.array([[[[10, 1], [110, 2], [21, 3], [121, 4]], [[50, 5], [150, 6], [90, 7], [190, 8]]]], np.uint8)
    rep = yuv.yuv_to_rgb(uyvy, "uyvy", ident, "replicate")
    assert rep[0, :, :, 0].tolist() == [[1, 2, 3, 4], [5, 6, 7, 8]]
    assert rep[0, :, :, 1].tolist() == [[10, 10, 21, 21], [50, 50, 90, 90]] and rep[0, 0, :, 2].tolist() == [110, 110, 121, 121]
    lin = yuv.yuv_to_rgb(uyvy, "uyvy", ident, "linear")
    assert lin[0, :, :, 1].tolist() == [[10, 16, 21, 21], [50, 70, 90, 90]]                          # rows do not mix
    # 2 x 2: one pair, every neighbour clamps to itself
    one = np.array([[[7, 8], [9, 10], [33, 44]]], np.uint8)
    for chroma in ("replicate", "linear"):
        assert yuv.yuv_to_rgb(one, "nv12", ident, chroma).tolist() == [[[[7, 33, 44], [8, 33, 44]], [[9, 33, 44], [10, 33, 44]]]]


def test_refused_host_forms():
    m = yuv.to_rgb_matrix()
    for frames, fmt in ((np.zeros((1, 5, 4), np.uint8), "nv12"), (np.zeros((1, 6, 3), np.uint8), "nv12"), (np.zeros((6, 4), np.uint8), "nv12"),
                        (np.zeros((1, 4, 3, 2), np.uint8), "uyvy"), (np.zeros((1, 4, 4, 3), np.uint8), "uyvy"), (np.zeros((1, 6, 4), np.int32), "nv12"),
                        (np.zeros((1, 6, 4), np.uint8), "i420")):
        with pytest.raises(ValueError):
            yuv.yuv_to_rgb(frames, fmt, m)
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb(np.zeros((1, 6, 4), np.uint8), "nv12", m, "cubic")
    for rgb in (np.zeros((1, 3, 4, 3), np.uint8), np.zeros((1, 4, 5, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            yuv.rgb_to_nv12(rgb, yuv.to_yuv_matrix())


@pytest.mark.parametrize("standard,full", PAIRS)
def test_rgb_to_nv12_layout_and_constant_blocks(standard, full):
    g = np.random.default_rng(5)
    blocks = g.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    rgb = np.repeat(np.repeat(blocks, 2, 1), 2, 2)                          # constant 2 x 2 blocks: the mean is the colour itself
    to_yuv, to_rgb = yuv.to_yuv_matrix(standard, full), yuv.to_rgb_matrix(standard, full)
    nv12 = yuv.rgb_to_nv12(rgb, to_yuv)
    assert nv12.dtype == np.uint8 and nv12.shape == (2, 15, 14)
    want = _apply(to_yuv, blocks)
    assert np.array_equal(nv12[:, :10], np.repeat(np.repeat(want[..., 0], 2, 1), 2, 2))
    assert np.array_equal(nv12[:, 10:].reshape(2, 5, 7, 2), want[..., 1:])
    back = yuv.yuv_to_rgb(nv12, "nv12", to_rgb, "replicate")
    assert int(np.abs(back.astype(np.int16) - rgb.astype(np.int16)).max()) <= ROUND_TRIP[full]
    # a block that is not constant: chroma from the per-channel mean (sum + 2) >> 2, luma per pixel
    px = g.integers(0, 256, (1, 2, 2, 3), dtype=np.uint8)
    mean = (px.astype(np.int64).sum(axis=(1, 2)) + 2) >> 2
    got = yuv.rgb_to_nv12(px, to_yuv)
    assert np.array_equal(got[0, :2], _apply(to_yuv, px)[0, :, :, 0])
    assert got[0, 2].tolist() == _apply(to_yuv, mean)[0, 1:].tolist()


# ---------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_exported_and_typed():
    lib = hip.load()
    i, p = ctypes.c_int, ctypes.c_void_p
    for name, argtypes in (("stswin_yuv_to_rgb", [p, p, p, i, i, i, i, i, p]), ("stswin_rgb_to_nv12", [p, p, p, i, i, i, p])):
        assert name in hip.declared_symbols()
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes
    assert (hip.YUV_NV12, hip.YUV_UYVY, hip.YUV_REPLICATE, hip.YUV_LINEAR) == (0, 1, 0, 1)
