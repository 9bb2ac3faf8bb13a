"""Host side of the contrastive pre-training input (stswincl_amd/contrast/views.py), no GPU: the per-axis tables against Pillow for
every crop length the source allows, the random stream against the recorded draws of the reference's RandomResizedCropCoord +
RandomHorizontalFlipCoord (tests/golden/resized_crop_coord.npz, tools/gen_golden_contrast_input.py), the table rows applied in numpy
the way the kernels apply them against the CPU statement tests/contrast_views_ref.py, the value table, the frame map, the refusals."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrast_views_ref as cr  # noqa: E402
from stswincl_amd import video  # noqa: E402
from stswincl_amd.contrast import views as cv  # noqa: E402
from stswincl_amd.contrast.views import ContrastViews, ViewParams  # noqa: E402
from stswincl_amd.hip import StswinHipError  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resized_crop_coord.npz")


def apply_axis(strip: np.ndarray, bounds: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """One pass of the resampler along axis 0 of uint8 strip [n][...]: out[x] = clip((2^21 + sum_t strip[first + t] k[x][t]) >> 22)."""
    ks = coef.shape[1]
    t = np.arange(ks)
    idx = np.minimum(bounds[:, :1] + t[None, :], strip.shape[0] - 1)
    k = np.where(t[None, :] < bounds[:, 1:2], coef, 0).astype(np.int64)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= strip.shape[0]).all()
    acc = (strip[idx].astype(np.int64) * k.reshape(k.shape + (1,) * (strip.ndim - 1))).sum(1) + (1 << 21)
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- tables against Pillow
@pytest.mark.parametrize("axis,src,out", [("x", 480, 448), ("y", 270, 256)])
def test_axis_tables_equal_pillow_for_every_crop_length(axis, src, out):
    from PIL import Image
    rng = np.random.default_rng(src)
    strip = rng.integers(0, 256, (src, 3), dtype=np.uint8)                     # the pixels along the axis, RGB
    lstrip = rng.integers(0, 256, src, dtype=np.uint8)
    if axis == "x":
        im, lim = Image.fromarray(np.stack([strip, strip])), Image.fromarray(np.stack([lstrip, lstrip]))
    else:
        im, lim = Image.fromarray(np.stack([strip, strip], 1)), Image.fromarray(np.stack([lstrip, lstrip], 1))
    ksize = cv.bilinear_ksize(src, out)
    assert ksize == 5
    taps = {}
    for length in range(1, src + 1):
        for off in sorted({0, src - length}):
            box, size = ((off, 0, off + length, 2), (out, 2)) if axis == "x" else ((0, off, 2, off + length), (2, out))
            want = np.array(im.crop(box).resize(size, Image.BILINEAR))
            lwant = np.array(lim.crop(box).resize(size, Image.NEAREST))
            want, lwant = (want[0], lwant[0]) if axis == "x" else (want[:, 0], lwant[:, 0])
            bounds, coef, near = cv.axis_tables(off, length, out, ksize)
            assert bounds.dtype == coef.dtype == near.dtype == np.int32 and coef.shape == (out, ksize)
            assert np.array_equal(apply_axis(strip, bounds, coef), want), (axis, length, off)
            assert near.min() >= off and near.max() < off + length
            assert np.array_equal(lstrip[near], lwant), (axis, length, off)
            taps[length] = (cv._axis(length, out)[1].shape[1], int(bounds[:, 1].max()))      # (table width, most taps in use)
    assert taps[out] == (1, 1)                                                  # the unscaled length (pass skipped: one tap of 2^22)
    assert np.array_equal(cv.axis_tables(3, out, out, ksize)[1][:, 0], np.full(out, 1 << 22))
    assert taps[1] == (3, 1)                                                    # length 1: every output pixel is the one source pixel
    assert all(taps[n][0] == 3 and taps[n][1] <= 3 for n in range(1, out))      # upscaling: Pillow's 3-tap tables
    assert all(taps[n][0] == 5 and 2 <= taps[n][1] <= 5 for n in range(out + 1, src + 1))      # downscaling: the 5-tap tables
    assert max(taps[n][1] for n in range(out + 1, src + 1)) == 3


def emulate(c: ContrastViews, frames: np.ndarray, labels: np.ndarray, tab: np.ndarray, B: int):
    """The kernels' computation from the table rows alone, in numpy: frames [F][Hs][Ws][3], labels [L][Hs][Ws] -> images
    [V][4][3][H][W], masks [V][1][H][W]."""
    H, W = c.out
    ks = c.ksize
    imgs, masks = [], []
    for row in tab:
        r0, r1, flags, lab = row[:4]
        o = 8
        parts = []
        for n in (2 * W, ks * W, 2 * H, ks * H, W, H):
            parts.append(row[o:o + n])
            o += n
        assert o == row.size
        hb, hk, vb, vk, lx, ly = parts[0].reshape(W, 2), parts[1].reshape(W, ks), parts[2].reshape(H, 2), parts[3].reshape(H, ks), parts[4], parts[5]
        assert vb[:, 0].min() >= r0 and (vb[:, 0] + vb[:, 1]).max() <= r1
        fr = []
        for f in row[4:8]:
            tmp = np.zeros((frames.shape[1], W, 3), np.uint8)
            tmp[r0:r1] = apply_axis(frames[f, r0:r1].transpose(1, 0, 2), hb, hk).transpose(1, 0, 2)          # the horizontal pass, rows [r0, r1)
            a = apply_axis(tmp, vb, vk)
            m = labels[lab][ly[:, None], lx[None, :]]
            if flags & 1:
                a, m = a[:, ::-1], m[:, ::-1]
            if flags & 2:
                a, m = a[::-1], m[::-1]
            fr.append(np.stack([c.table[ch][a[..., ch]] for ch in range(3)]))
        imgs.append(np.stack(fr))
        masks.append(m.astype(np.float32)[None])
    return np.stack(imgs), np.stack(masks)


def test_table_rows_applied_in_numpy_equal_the_cpu_statement():
    c = ContrastViews(out=(16, 32), source=(24, 40))
    assert c.ksize == 5 and c.n_frames == 17 and c.n_labels == 6
    B = 2
    data = [cr.seeded_sample(s, 17, 6, 24, 40) for s in range(B)]
    frames, labels = np.stack([d[0] for d in data]), np.stack([d[1] for d in data])
    params = [[c.params(0, 0, 24, 40), c.params(3, 5, 16, 10, hflip=True), c.params(8, 8, 1, 32, vflip=True), c.params(0, 39, 24, 1),
               c.params(4, 4, 16, 32, hflip=True, vflip=True), c.params(23, 0, 1, 1)],
              c.sample(1, random.Random(3))[0]]
    tab = c.tables(params)
    assert tab.shape == (12, c.stride()) and tab.dtype == np.int32
    assert np.array_equal(tab[0 * B + 1, 4:8], 17 + np.array(cv.DEFAULT_FRAME_MAP[0])) and tab[5 * B + 1, 3] == 6 + 5      # global indices
    imgs, masks = emulate(c, frames.reshape(-1, 24, 40, 3), labels.reshape(-1, 24, 40), tab, B)
    want = cr.views(frames, labels, params, c.out)
    for v in range(6):
        assert np.array_equal(imgs[v * B:(v + 1) * B], want[v].numpy()), v
        assert np.array_equal(masks[v * B:(v + 1) * B], want[6 + v].numpy()), v


# ---------------------------------------------------------------------------------------------- the random stream
@pytest.mark.parametrize("case", ["default", "wide"])
def test_sample_equals_the_recorded_reference_draws(case):
    g = np.load(GOLDEN)
    get = lambda k: g[f"{case}/{k}"]                                                   # noqa: E731
    c = ContrastViews(out=tuple(get("out")), source=tuple(get("source")), scale=tuple(get("scale")), ratio=tuple(get("ratio")))
    assert len(get("seeds")) >= 200
    if case == "default":
        assert (get("attempts") > 1).any() and not get("fallback").any()             # seeds that reject attempts; the fallback is out of reach
        assert (c.out, c.source, c.scale, c.hflip_p) == ((256, 448), (270, 480), (0.09, 0.49), 0.5)
    else:
        assert get("fallback").any() and not get("fallback").all()
    for s, seed in enumerate(get("seeds")):
        rng = random.Random(int(seed))
        (ps,) = c.sample(1, rng)
        assert len(ps) == 6
        for v, p in enumerate(ps):
            assert (p.i, p.j, p.h, p.w) == tuple(int(x) for x in get("ijhw")[s, v]), (seed, v)
            assert p.hflip == bool(get("flip")[s, v]) and p.vflip is False, (seed, v)
            assert p.coord.dtype == np.float32 and np.array_equal(p.coord.view(np.uint32), get("coord")[s, v].view(np.uint32)), (seed, v)
            c.check(p)
        assert rng.getrandbits(32) == int(get("check")[s]), seed                       # the same number of draws was consumed
    fb = np.argwhere(get("fallback"))
    if len(fb):                                                                       # the central crop of the widest allowed ratio
        s, v = fb[0]
        assert tuple(get("ijhw")[s, v]) == (0, (200 - 53) // 2, 40, 53)


def test_sample_draws_sample_after_sample_from_one_stream():
    c = ContrastViews()
    rng = random.Random(11)
    a = c.sample(3, rng)
    rng = random.Random(11)
    b = [c.sample(1, rng)[0] for _ in range(3)]
    assert [[(p.i, p.j, p.h, p.w, p.hflip) for p in s] for s in a] == [[(p.i, p.j, p.h, p.w, p.hflip) for p in s] for s in b]


# ---------------------------------------------------------------------------------------------- smaller checks
def test_value_table_is_the_torch_fp32_formula():
    t = cv.value_table()
    assert t.dtype == np.float32 and t.shape == (3, 256)
    u = torch.arange(256, dtype=torch.uint8)
    for c, (m, s) in enumerate(zip(cr.MEAN, cr.STD)):
        want = ((u.to(torch.float32) / torch.tensor(255, dtype=torch.float32)) - torch.tensor(m, dtype=torch.float32)) / torch.tensor(s, dtype=torch.float32)
        assert np.array_equal(t[c].view(np.uint32), want.numpy().view(np.uint32)), c
    assert np.array_equal(t.view(np.uint32), cr.value_table().view(np.uint32))
    f64 = ((np.arange(256) / 255.)[None, :] - np.array(cr.MEAN)[:, None]) / np.array(cr.STD)[:, None]
    assert np.abs(t - f64).max() < 1e-6                                              # (the same quantity, other rounding)
    assert (t != video.cadis_value_table()).any()                                     # not the CaDIS table
    other = cv.value_table(video.CADIS_MEAN, video.CADIS_STD)
    assert (other != video.cadis_value_table()).any()                                 # ... nor its float64 derivation with equal constants
    assert np.array_equal(ContrastViews().table, t)


def test_default_frame_map_is_the_datasets_index_pattern():
    # frames: 0 image, 1 image_1, 2 image_2, 3 image_3, 4 image_4, 5-8 neg1 p1 p2 p3, 9-12 neg2's, 13-16 neg3's (image_v is image)
    want = [[3, 2, 1, 0],            # transform[0](image, image_1, image_2, image_3)   -> append(img3, img2, img1, img)
            [3, 2, 1, 0],            # transform[1](image_1, image_2, image_3, image_v) -> append(img3, img2, img1, img_v)
            [4, 3, 2, 1],            # transform[2](image_1 .. image_4)                 -> append(img4, img3, img2, img1)
            [8, 7, 6, 5],            # transform[3](neg1, p1, p2, p3)                   -> append(p3, p2, p1, neg)
            [12, 11, 10, 9],
            [16, 15, 14, 13]]
    assert [list(r) for r in cv.DEFAULT_FRAME_MAP] == want == [list(r) for r in cr.FRAME_MAP]
    assert list(cv.DEFAULT_LABEL_MAP) == [0, 1, 2, 3, 4, 5]
    c = ContrastViews()
    assert (c.views, c.n_frames, c.n_labels, c.ksize) == (6, 17, 6, 5)
    ident = ContrastViews(frame_map=np.arange(24).reshape(6, 4))
    assert ident.n_frames == 24


def test_params_identity_and_coord():
    c = ContrastViews()
    p = c.identity()
    assert (p.i, p.j, p.h, p.w, p.hflip, p.vflip) == (0, 0, 270, 480, False, False)
    assert np.array_equal(p.coord, np.array([0, 0, 1, 1], np.float32))
    q = c.params(10, 20, 100, 200, hflip=True)
    assert np.array_equal(q.coord, np.array([219 / 479, 10 / 269, 20 / 479, 109 / 269], np.float32))
    t = c.view_tables(q)
    assert (t["r0"], t["r1"], t["flags"]) == (10, 110, 1) and t["lx"].min() >= 20 and t["lx"].max() < 220
    t = c.view_tables(c.params(0, 0, 270, 480))
    assert (t["r0"], t["r1"]) == (0, 270) and int(t["vbounds"][:, 1].max()) == 3 and t["vcoef"].shape == (256, 5)


def test_refusals_on_the_host():
    c = ContrastViews(out=(16, 32), source=(24, 40))
    for bad in ((-1, 0, 4, 4), (0, -1, 4, 4), (21, 0, 4, 4), (0, 37, 4, 4), (0, 0, 25, 4), (0, 0, 4, 41), (0, 0, 0, 4), (0, 0, 4, 0)):
        with pytest.raises(StswinHipError, match="the crop must lie inside the source 24 x 40"):
            c.params(*bad)
    with pytest.raises(StswinHipError, match="the crop must lie inside"):
        c.tables([[ViewParams(20, 0, 16, 10)] * 6])
    with pytest.raises(StswinHipError, match="6 ViewParams per sample"):
        c.tables([[c.identity()] * 5])
    with pytest.raises(StswinHipError, match=r"needs 27 taps per output pixel, the tables hold 16"):
        ContrastViews(out=(16, 32), source=(200, 40))
    with pytest.raises(StswinHipError, match="needs 5 taps, the tables hold 3"):
        cv.axis_tables(0, 24, 16, 3)
    with pytest.raises(StswinHipError, match="frame_map must be"):
        ContrastViews(frame_map=[[0, 1, 2]] * 6)
    with pytest.raises(StswinHipError, match="none may be negative"):
        ContrastViews(frame_map=[[0, 1, 2, -1]] * 6)
    frames, labels = torch.zeros(1, 17, 24, 40, 3, dtype=torch.uint8), torch.zeros(1, 6, 24, 40, dtype=torch.uint8)
    with pytest.raises(StswinHipError, match=r"uint8 \[B\]\[>= 17\]\[24\]\[40\]\[3\].*frames is on the CPU"):
        c(frames, labels, [[c.identity()] * 6])
    with pytest.raises(StswinHipError, match="got ndarray for frames"):
        c(frames.numpy(), labels, [[c.identity()] * 6])
