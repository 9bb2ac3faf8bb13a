"""Host side of the training-input augmenter (stswincl_amd/augment.py), no GPU: the numpy reference tests/augment_ref.py against
Pillow and against the recorded outputs of the reference's `_random_scale` (tests/golden/random_scale.npz), and the per-sample
tables ClipAugmenter builds for the kernels - inside their sources for every reachable size, and, applied in numpy the way the
kernels apply them, equal to the reference."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ar  # noqa: E402
from stswincl_amd import augment  # noqa: E402
from stswincl_amd.augment import ClipAugmenter  # noqa: E402
from stswincl_amd.hip import StswinHipError  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_scale.npz")
SRC = (512, 640)
CROP = (512, 640)
BASE_W = 672
LONG_SIZES = range(int(BASE_W * 0.5), int(BASE_W * 2.0) + 1)            # 336 .. 1344: every size _random_scale can reach


def _clip(seed, T=2, hw=SRC):
    return ar.seeded_clip(seed, T, *hw)


# long_size, x1, y1: 336 pads both ways, 500 pads, the others do not; 640 is the identity scale
PILLOW_CASES = [(336, 0, 0), (500, 0, 0), (640, 0, 0), (672, 17, 9), (900, 100, 50), (1344, 704, 563)]


@pytest.mark.parametrize("long_size,x1,y1", PILLOW_CASES)
def test_reference_equals_pillow(long_size, x1, y1):
    pytest.importorskip("PIL")
    frames, label = _clip(long_size)
    ow, oh, padw, padh = ar.geometry(long_size, SRC, CROP)
    assert (padw > 0 or padh > 0) == (long_size < 640)
    for hflip, vflip in ((False, False), (True, True)):
        p = ar.P(long_size, x1, y1, hflip=hflip, vflip=vflip)
        crops, lab = ar.scale_crop(frames, label, p, CROP)
        pcrops, plab = ar.scale_crop_pillow(frames, label, p, CROP)
        assert np.array_equal(crops, pcrops) and np.array_equal(lab, plab)
        if padw:
            assert not (pcrops[:, :, :padw] if hflip else pcrops[:, :, ow:]).any()


def test_nearest_tables_equal_pillow_for_every_reachable_size():
    Image = pytest.importorskip("PIL.Image")
    cols = Image.fromarray(np.broadcast_to(np.arange(SRC[1], dtype=np.int32)[None, :], (2, SRC[1])).copy())       # mode I: the pixel is its index
    rows = Image.fromarray(np.broadcast_to(np.arange(SRC[0], dtype=np.int32)[:, None], (SRC[0], 2)).copy())
    closed_form_differs = 0
    for long_size in LONG_SIZES:
        ow, oh, _, _ = ar.geometry(long_size, SRC, CROP)
        want_x = np.array(cols.resize((ow, 2), Image.NEAREST))[0]
        want_y = np.array(rows.resize((2, oh), Image.NEAREST))[:, 0]
        for fn in (ar.nearest_index, augment.nearest_index):
            assert np.array_equal(fn(SRC[1], ow), want_x), (long_size, ow)
            assert np.array_equal(fn(SRC[0], oh), want_y), (long_size, oh)
        closed_form_differs += not np.array_equal(np.floor((np.arange(ow) + 0.5) * (SRC[1] / ow)).astype(np.int64), want_x)
    assert closed_form_differs > 0            # (why the tables accumulate as Pillow does)


def test_geometry_and_sampling_follow_the_reference():
    for long_size in LONG_SIZES:
        assert augment.geometry(long_size, SRC, CROP) == ar.geometry(long_size, SRC, CROP)
    for hw in ((80, 64), (64, 80), (64, 64)):
        for long_size in range(40, 170):
            assert augment.geometry(long_size, hw, (64, 80)) == ar.geometry(long_size, hw, (64, 80))
    aug = ClipAugmenter()
    got = aug.sample(16, rng=random.Random(7), gen=np.random.default_rng(7))
    rng = random.Random(7)
    for p in got:
        assert (p.long_size, p.x1, p.y1) == ar.draw_geometry(rng, BASE_W, SRC, CROP)
    again = aug.sample(16, rng=random.Random(7), gen=np.random.default_rng(7))
    assert got == again
    assert not any(p.hflip for p in got)                                    # EndoVis18: no horizontal flip
    assert any(p.vflip for p in got) and any(p.alpha is not None for p in got) and any(p.angle is not None for p in got)
    assert all(0.8 <= p.alpha <= 1.2 and -0.2 <= p.beta <= 0.2 for p in got if p.alpha is not None)
    assert all(-90 <= p.angle <= 90 for p in got if p.angle is not None)
    cadis = ClipAugmenter(protocol="cadis", class_num=18).sample(32, rng=random.Random(7), gen=np.random.default_rng(7))
    assert any(p.hflip for p in cadis) and all(p.alpha is None and p.beta is None for p in cadis)
    off = ClipAugmenter(p_vflip=0, p_bc=0, p_rotate=0).sample(8, rng=random.Random(1), gen=np.random.default_rng(1))
    assert all(not p.vflip and p.alpha is None and p.angle is None for p in off)


def test_reference_and_sampler_reproduce_the_recorded_random_scale():
    g = np.load(GOLDEN)
    src, crop, base_w, t = tuple(g["source"]), tuple(g["crop"]), int(g["base_w"]), int(g["t"])
    aug = ClipAugmenter(crop=crop, base_w=base_w, source=src, p_vflip=0, p_bc=0, p_rotate=0)
    kinds = set()
    for seed in g["seeds"]:
        long_size, ow, oh, x1, y1 = (int(v) for v in g[f"{seed}/geometry"])
        p = aug.sample(1, rng=random.Random(int(seed)), gen=np.random.default_rng(0))[0]
        assert (p.long_size, p.x1, p.y1) == (long_size, x1, y1)
        assert aug.scaled(p)[:2] == (ow, oh) == ar.geometry(long_size, src, crop)[:2]
        frames, label = ar.seeded_clip(int(seed), t, *src)
        crops, mask = ar.scale_crop(frames, label, p, crop)
        assert np.array_equal(crops, g[f"{seed}/crops"]) and np.array_equal(mask, g[f"{seed}/mask"])
        kinds.add("up" if ow > src[1] else "down")
        if ow < crop[1] or oh < crop[0]:
            kinds.add("pad")
    assert kinds == {"up", "down", "pad"}


def test_host_tables_stay_inside_their_sources():
    """For every reachable size: the whole axis (every column and row of the scaled and padded image, whichever window a crop origin
    picks), then the tables of the two extreme crop origins as the kernels receive them."""
    from stswincl_amd import video
    aug = ClipAugmenter()
    assert aug.ksize == 5
    for long_size in LONG_SIZES:
        ow, oh, padw, padh = augment.geometry(long_size, SRC, CROP)
        for in_size, out_size, pad in ((SRC[1], ow, padw), (SRC[0], oh, padh)):
            near = augment.nearest_index(in_size, out_size)
            assert near.shape == (out_size,) and near.min() >= 0 and near.max() < in_size and (np.diff(near) >= 0).all()
            if in_size != out_size:
                b, k = video.bilinear_coeffs(in_size, out_size)
                assert b.shape == (out_size, 2) and k.shape[1] <= aug.ksize
                assert b[:, 0].min() >= 0 and b[:, 1].min() >= 1 and (b[:, 0] + b[:, 1]).max() <= in_size
            bounds, coef, anear = augment.axis_tables(in_size, out_size, 0, out_size + pad, aug.ksize)      # the whole padded axis
            inside = np.arange(out_size + pad) < out_size
            assert bounds[inside, 0].min() >= 0 and bounds[inside, 1].min() >= 1 and (bounds[inside, 0] + bounds[inside, 1]).max() <= in_size
            assert np.array_equal(anear[inside], near) and (anear[~inside] == -1).all() and not bounds[~inside].any() and not coef[~inside].any()
            assert (coef[inside].sum(1) > 0).all() and coef.shape[1] == aug.ksize
        for x1, y1 in {(0, 0), (ow + padw - CROP[1], oh + padh - CROP[0])}:
            c = aug.crop_tables(aug.params(long_size, x1, y1))
            for bounds, coef, near, size in ((c["hbounds"], c["hcoef"], c["lx"], SRC[1]), (c["vbounds"], c["vcoef"], c["ly"], SRC[0])):
                taps = bounds[:, 1] > 0
                assert bounds[taps, 0].min() >= 0 and (bounds[taps, 0] + bounds[taps, 1]).max() <= size
                assert bounds[:, 1].max() <= aug.ksize and coef.shape[1] == aug.ksize
                assert not coef[~taps].any() and (near[~taps] == -1).all()
                assert near[taps].min() >= 0 and near[taps].max() < size
                assert (coef[taps].sum(1) > 0).all()
            rows = c["vbounds"][:, 1] > 0
            assert 0 <= c["r0"] <= c["r1"] <= SRC[0]
            assert c["vbounds"][rows, 0].min() >= c["r0"] and (c["vbounds"][rows, 0] + c["vbounds"][rows, 1]).max() <= c["r1"]


# ---------------------------------------------------------------------------------------------- the tables, applied as the kernels do
def _taps(a, bounds, coef):
    """Pillow's pass along axis 0 of `a` with per-index taps: clip((2^21 + sum u k) >> 22)."""
    acc = np.full((bounds.shape[0],) + a.shape[1:], 1 << 21, np.int64)
    for j in range(coef.shape[1]):
        on = j < bounds[:, 1]
        src = np.where(on, np.minimum(bounds[:, 0] + j, a.shape[0] - 1), 0)
        acc += a[src].astype(np.int64) * np.where(on, coef[:, j], 0).reshape((-1,) + (1,) * (a.ndim - 1))
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def emulate(aug, frames, label, p, protocol="endovis18", class_num=12):
    """One sample through the words of ClipAugmenter.tables(), in numpy, in the kernels' order."""
    t1, t2 = aug.tables([p])
    t1, t2 = t1[0], t2[0]
    (Hs, Ws), (Hc, Wc), ks = aug.source, aug.crop, aug.ksize
    r0, r1, flags = (int(v) for v in t1[:3])
    o = 4
    hb = t1[o:o + 2 * Wc].reshape(Wc, 2); o += 2 * Wc
    hk = t1[o:o + ks * Wc].reshape(Wc, ks); o += ks * Wc
    vb = t1[o:o + 2 * Hc].reshape(Hc, 2); o += 2 * Hc
    vk = t1[o:o + ks * Hc].reshape(Hc, ks); o += ks * Hc
    lx = t1[o:o + Wc]; ly = t1[o + Wc:o + Wc + Hc]
    assert o + Wc + Hc == t1.size
    tmp = np.full((frames.shape[0], Hs, Wc, 3), 0xAB, np.uint8)                      # rows outside [r0, r1) are never written ...
    tmp[:, r0:r1] = _taps(frames[:, r0:r1].transpose(2, 0, 1, 3), hb, hk).transpose(1, 2, 0, 3)
    crops = _taps(tmp.transpose(1, 0, 2, 3), vb, vk).transpose(1, 0, 2, 3)            # ... and must never be read
    lab = np.where((ly[:, None] >= 0) & (lx[None, :] >= 0), label[np.maximum(ly, 0)[:, None], np.maximum(lx, 0)[None, :]], 0).astype(np.uint8)
    if flags & 1:
        crops, lab = crops[:, :, ::-1], lab[:, ::-1]
    if flags & 2:
        crops, lab = crops[:, ::-1], lab[::-1]
    bc = t2[4 + 2 * (Hc + Wc):].view(np.uint8)
    assert bc.size == 256
    v = bc[crops].astype(np.int64)
    if t2[0] & 1:
        colx, coly = t2[4:4 + Wc].astype(np.int64), t2[4 + Wc:4 + 2 * Wc].astype(np.int64)
        rowx, rowy = t2[4 + 2 * Wc:4 + 2 * Wc + Hc].astype(np.int64), t2[4 + 2 * Wc + Hc:4 + 2 * Wc + 2 * Hc].astype(np.int64)
        X, Y = (rowx[:, None] + colx[None, :]) >> 5, (rowy[:, None] + coly[None, :]) >> 5
        fx, fy = (X & 31)[None, :, :, None], (Y & 31)[None, :, :, None]
        x0, x1, y0, y1 = (ar.reflect101(X >> 5, Wc), ar.reflect101((X >> 5) + 1, Wc), ar.reflect101(Y >> 5, Hc), ar.reflect101((Y >> 5) + 1, Hc))
        v = ((32 - fx) * (32 - fy) * v[:, y0, x0] + fx * (32 - fy) * v[:, y0, x1] + (32 - fx) * fy * v[:, y1, x0] + fx * fy * v[:, y1, x1] + 512) >> 10
        lab = lab[ar.reflect101((Y + 16) >> 5, Hc), ar.reflect101((X + 16) >> 5, Wc)]
    return ar.to_float(v.astype(np.uint8), protocol), ar.label_table(protocol, class_num)[lab]


SMALL = dict(crop=(64, 80), base_w=84, source=(64, 80))
SMALL_CASES = [
    dict(long_size=42, x1=0, y1=0),                                                  # the extreme downscale: 5 taps, padding
    dict(long_size=80, x1=0, y1=0),                                                  # identity scale
    dict(long_size=80, x1=0, y1=0, vflip=True, alpha=1.15, beta=-0.1),
    dict(long_size=121, x1=16, y1=22, hflip=True, angle=31.0),
    dict(long_size=168, x1=88, y1=70, hflip=True, vflip=True, alpha=0.8, beta=0.2, angle=-90.0),
    dict(long_size=59, x1=0, y1=0, hflip=True, angle=77.5),
    dict(long_size=100, x1=20, y1=0, angle=0.0),
    dict(long_size=100, x1=0, y1=16, angle=90.0),
]


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_tables_applied_as_the_kernels_do_equal_the_reference(case, protocol):
    aug = ClipAugmenter(protocol=protocol, class_num=18, **SMALL)
    frames, label = ar.seeded_clip(3, 4, *SMALL["source"])
    label[::7, ::5] = 255
    p = aug.params(**case)
    img, lab = emulate(aug, frames, label, p, protocol, 18)
    want_img, want_lab = ar.augment_one(frames, label, p, SMALL["crop"], protocol, 18)
    assert np.array_equal(img, want_img) and np.array_equal(lab, want_lab)
    assert img.dtype == np.float32 and lab.dtype == np.int64
    if protocol == "cadis":
        assert (lab == 17).any() and not (lab == 255).any()


def test_tables_at_full_size_with_a_non_square_source():
    aug = ClipAugmenter()
    frames, label = _clip(11, T=1)
    for case in (dict(long_size=336, x1=0, y1=0, vflip=True), dict(long_size=1344, x1=704, y1=563, angle=12.0, alpha=1.1, beta=0.05)):
        p = aug.params(**case)
        img, lab = emulate(aug, frames, label, p)
        want_img, want_lab = ar.augment_one(frames, label, p, CROP)
        assert np.array_equal(img, want_img) and np.array_equal(lab, want_lab)
    tall = ClipAugmenter(crop=(80, 64), base_w=84, source=(100, 70))                 # h > w: the other branch of the geometry
    frames, label = ar.seeded_clip(5, 4, 100, 70)
    p = tall.params(130, 10, 30, hflip=True, angle=-20.0)
    img, lab = emulate(tall, frames, label, p)
    want_img, want_lab = ar.augment_one(frames, label, p, (80, 64))
    assert np.array_equal(img, want_img) and np.array_equal(lab, want_lab)


# ---------------------------------------------------------------------------------------------- value table, rotation
def test_value_table_and_rotation_tables():
    """The value table and the rotation are this project's own definition, stated twice (stswincl_amd/augment.py for the device tables,
    tests/augment_ref.py for the reference): the table-equality loops below only show that the two statements agree.  The independent
    assertions are the hand-computed table entries (51, 255, 2), the multiples of 90 degrees against numpy.rot90 (orientation, centre and
    the exactness of the fixed-point positions), the table-only copy, and the reflect-101 index list."""
    for alpha, beta in ((None, None), (1.2, 0.2), (0.8, -0.2), (1.0, 0.1), (1.07, None)):
        assert np.array_equal(augment.value_table(alpha, beta), ar.value_table(alpha, beta))
    assert np.array_equal(ar.value_table(None, None), np.arange(256))
    assert ar.value_table(1.0, 0.2)[0] == 51 and ar.value_table(1.0, 0.2)[255] == 255 and ar.value_table(0.5, 0.0)[3] == 2   # 1.5 -> 2
    for angle in (0.0, 90.0, -90.0, 1.5, 31.0, -77.25):
        for a, b in zip(augment.rotate_tables(angle, 512, 640), ar.rotate_tables(angle, 512, 640)):
            assert a.dtype == np.int32 and np.array_equal(a, b)
    # multiples of 90 degrees on a square are exact copies: positive = counter-clockwise
    frames, label = ar.seeded_clip(2, 4, 32, 32)
    ident = np.arange(256, dtype=np.uint8)
    for angle, k in ((0.0, 0), (90.0, 1), (-90.0, -1), (180.0, 2)):
        img, lab = ar.rotate(frames, label, angle, ident)
        assert np.array_equal(img, np.rot90(frames, k, axes=(1, 2))) and np.array_equal(lab, np.rot90(label, k))
    img, lab = ar.rotate(frames, label, None, ar.value_table(1.2, -0.1))
    assert np.array_equal(img, ar.value_table(1.2, -0.1)[frames]) and np.array_equal(lab, label)
    # a small angle stays within one grey level step of its neighbours' range, and reflect-101 never repeats the edge pixel
    assert np.array_equal(ar.reflect101(np.array([-2, -1, 0, 5, 6, 7, 12]), 6), [2, 1, 0, 5, 4, 3, 2])


def test_refusals_on_the_host():
    aug = ClipAugmenter()
    with pytest.raises(StswinHipError, match="crop origin must satisfy"):
        aug.params(672, 40, 0)                                        # 672 x 538: x1 <= 32
    with pytest.raises(StswinHipError, match="crop origin must satisfy"):
        aug.params(336, 1, 0)                                         # padded to the crop size: only (0, 0)
    with pytest.raises(StswinHipError, match=r"long_size must be in \[336, 1344\]"):
        aug.params(200, 0, 0)
    with pytest.raises(StswinHipError, match="class_num"):
        ClipAugmenter(protocol="cadis")
    with pytest.raises(StswinHipError):
        ClipAugmenter(protocol="other")
    import torch
    p = [aug.identity()]
    with pytest.raises(StswinHipError, match="on the CPU"):
        aug(torch.zeros(1, 4, 512, 640, 3, dtype=torch.uint8), torch.zeros(1, 512, 640, dtype=torch.uint8), p)
