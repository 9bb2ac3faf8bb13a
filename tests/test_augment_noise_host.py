"""Host side of CaDIS's Gaussian noise (stswincl_amd/augment.py: noise_thresholds, ClipParams.noise, the table words), no GPU: the
reference Philox of tests/augment_noise_ref.py against the published known answers, the law against the reference transform's own
expression, the draws of sample() and the three words tables() writes."""
import math
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_noise_ref as nr  # noqa: E402
import augment_ref as ar  # noqa: E402
from stswincl_amd import augment  # noqa: E402
from stswincl_amd.augment import ClipAugmenter, ClipParams, noise_thresholds  # noqa: E402
from stswincl_amd.hip import StswinHipError  # noqa: E402

VAR = 0.001
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_reference_philox_reproduces_the_known_answers():
    for counter, key, want in KAT:
        assert " ".join("%08x" % int(w) for w in nr.philox4x32_10(counter, key)) == want
    c = np.array([k[0] for k in KAT[:2]], dtype=np.uint32).T                     # vectorised over counters, one key
    got = nr.philox4x32_10(tuple(c), (0, 0))
    assert " ".join("%08x" % int(w[0]) for w in got) == KAT[0][2]


def test_thresholds_of_the_reference_variance():
    thr, k_min = noise_thresholds(VAR)
    assert thr.dtype == np.uint32 and thr.shape == (103,) and k_min == -52
    assert (np.diff(thr.astype(np.int64)) > 0).all()                          # strictly ascending
    ref_thr, ref_k_min = nr.thresholds(VAR)
    assert ref_k_min == k_min and np.array_equal(ref_thr, thr)
    s2 = 255.0 ** 2 * VAR
    edges = np.concatenate([[0], thr.astype(np.int64), [1 << 32]])
    p = np.diff(edges) / 2.0 ** 32                                            # P(K = k_min + j): j thresholds are <= r
    ks = np.arange(k_min, k_min + len(thr) + 1, dtype=np.float64)
    mean = float((p * ks).sum())
    variance = float((p * (ks - mean) ** 2).sum())
    assert abs(p.sum() - 1.0) < 1e-12
    assert abs(mean + 0.5) < 1e-6, mean
    assert abs(variance - (s2 + 1.0 / 12.0)) < 1e-6, variance


def test_thresholds_are_strictly_ascending_and_the_formula_s_up_to_separated_ties():
    """t_k = floor(Phi((k + 1) / s) 2^32 + 0.5) gives 1 for k = -52 and -51 (Phi 2^32 = 0.55 and 1.21) and 2^32 - 1 for k = 49 and
    50: the ties are separated by one, every other threshold is the formula's."""
    thr, k_min = noise_thresholds(VAR)
    s = 255.0 * math.sqrt(VAR)
    plain = np.array([int(math.floor(0.5 * (1.0 + math.erf((k + 1) / s / math.sqrt(2.0))) * 2.0 ** 32 + 0.5))
                      for k in range(k_min, k_min + len(thr))], dtype=np.int64)
    t = thr.astype(np.int64)
    assert (np.diff(t) > 0).all() and 0 < t[0] and t[-1] < 1 << 32
    assert plain[:3].tolist() == [1, 1, 3] and t[:3].tolist() == [1, 2, 3]
    assert plain[-3:].tolist() == [4294967293, 4294967295, 4294967295] and t[-3:].tolist() == [4294967293, 4294967294, 4294967295]
    assert np.array_equal(t[2:-2], plain[2:-2])
    for var in (0.0004, 0.01, 0.09):                                         # more ties in longer tails: still strict, never more than a few units off
        thr, k_min = noise_thresholds(var)
        ref, ref_k_min = nr.thresholds(var)
        assert k_min == ref_k_min and np.array_equal(thr, ref) and (np.diff(thr.astype(np.int64)) > 0).all(), var


def test_thresholds_refuse_what_the_kernel_cannot_hold():
    with pytest.raises(StswinHipError, match=r"more than 1024 thresholds.*largest var that fits is 0\.\d+"):
        noise_thresholds(1.0)
    with pytest.raises(StswinHipError, match="more than 1024"):
        noise_thresholds(1e9)
    with pytest.raises(StswinHipError, match="positive"):
        noise_thresholds(0.0)
    with pytest.raises(StswinHipError, match="more than 1024"):
        ClipAugmenter(noise_var=1.0)
    m = None
    try:
        noise_thresholds(1.0)
    except StswinHipError as e:
        m = float(str(e).rsplit(" ", 1)[1])
    assert len(noise_thresholds(m)[0]) <= 1024 < len(nr.thresholds(m * 1.01)[0])      # the var it names fits, a little more does not


@pytest.mark.parametrize("u", [0, 3, 128, 250, 255])
def test_the_law_is_the_reference_transform_s(u):
    """The reference's own expression on 2^20 normal draws of a fixed-seed generator: every output value's frequency within five
    binomial standard errors (+ 1e-6) of the clamped law."""
    n = 1 << 20
    rng = np.random.default_rng(1000 + u)
    out = (255 * np.clip(u / 255. + rng.normal(0, VAR ** .5, n), 0, 1)).astype('uint8')
    freq = np.bincount(out, minlength=256) / n
    p = nr.clamped_pmf(u, VAR)
    assert abs(p.sum() - 1.0) < 1e-12
    margin = 5.0 * np.sqrt(p * (1.0 - p) / n) + 1e-6
    bad = np.nonzero(np.abs(freq - p) > margin)[0]
    assert bad.size == 0, [(int(v), float(freq[v]), float(p[v])) for v in bad]
    thr, k_min = noise_thresholds(VAR)                                        # and the device's counting rule states the same law
    r = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k = k_min + np.searchsorted(thr, r, side="right")
    freq_k = np.bincount(np.clip(u + k, 0, 255), minlength=256) / n
    assert (np.abs(freq_k - p) <= margin).all()


def _seven_draws(aug, rng, gen, noise):
    """The documented order: three from rng, seven from gen, then (noise) u_noise and the key."""
    long_size, x1, y1 = ar.draw_geometry(rng, aug.base_w, aug.source, aug.crop)
    u = gen.random(3)
    contrast = gen.uniform(-aug.contrast_limit, aug.contrast_limit)
    brightness = gen.uniform(-aug.brightness_limit, aug.brightness_limit)
    u_rot = gen.random()
    angle = gen.uniform(-aug.rotate_limit, aug.rotate_limit)
    key = None
    if noise:
        u_noise = gen.random()
        k = int(gen.integers(0, 2 ** 64, dtype=np.uint64))
        key = k if u_noise < aug.p_noise else None
    bc = u[2] < aug.p_bc
    return ClipParams(long_size, x1, y1, bool(u[0] < aug.p_hflip), bool(u[1] < aug.p_vflip), 1.0 + float(contrast) if bc else None,
                      float(brightness) if bc else None, float(angle) if u_rot < aug.p_rotate else None, key)


@pytest.mark.parametrize("protocol,class_num", [("endovis18", None), ("cadis", 18)])
def test_sample_without_noise_makes_exactly_the_seven_draws(protocol, class_num):
    aug = ClipAugmenter(protocol=protocol, class_num=class_num)
    assert aug.p_noise == 0.0 and aug.noise_var == 0.001                       # the default is off for both protocols
    got = aug.sample(6, rng=random.Random(11), gen=np.random.default_rng(11))
    rng, gen = random.Random(11), np.random.default_rng(11)
    want = [_seven_draws(aug, rng, gen, noise=False) for _ in range(6)]
    assert got == want and all(p.noise is None for p in got)
    assert ClipParams(1, 2, 3) == ClipParams(1, 2, 3, False, False, None, None, None, None)


def test_sample_with_noise_keeps_the_seven_draws_and_adds_two():
    aug = ClipAugmenter(protocol="cadis", class_num=18, p_noise=0.5)
    B = 16
    got = aug.sample(B, rng=random.Random(5), gen=np.random.default_rng(5))
    rng, gen = random.Random(5), np.random.default_rng(5)
    want = [_seven_draws(aug, rng, gen, noise=True) for _ in range(B)]
    assert got == want
    keys = [p.noise for p in got if p.noise is not None]
    assert 0 < len(keys) < B and len(set(keys)) == len(keys) and all(0 <= k < 1 << 64 for k in keys) and max(keys) >= 1 << 32
    # the first sample's seven draws are those of a sampler without noise (later samples start two draws further on)
    plain = ClipAugmenter(protocol="cadis", class_num=18).sample(1, rng=random.Random(5), gen=np.random.default_rng(5))[0]
    first = ClipParams(**{**got[0].__dict__, "noise": None})
    assert first == plain
    # both extra draws are made whether or not the noise applies: the generator is at the same place after B samples
    g_all, g_none = np.random.default_rng(9), np.random.default_rng(9)
    ClipAugmenter(protocol="cadis", class_num=18, p_noise=1.0).sample(4, rng=random.Random(9), gen=g_all)
    ClipAugmenter(protocol="cadis", class_num=18, p_noise=1e-300).sample(4, rng=random.Random(9), gen=g_none)
    assert g_all.random() == g_none.random()


def test_tables_carry_the_key_of_a_noisy_sample_only():
    aug = ClipAugmenter(crop=(64, 80), base_w=84, protocol="cadis", class_num=18, source=(64, 80))
    keys = [None, 0x0123456789abcdef, 0xffffffff80000001, None, 0x80000000fffffffe, 0]
    base = [aug.params(100 + b, b, 2 * b, hflip=bool(b & 1), angle=(12.5 * b if b % 3 else None), alpha=1.1 if b == 4 else None,
                       beta=0.05 if b == 4 else None) for b in range(len(keys))]
    noisy = [aug.params(p.long_size, p.x1, p.y1, p.hflip, p.vflip, p.alpha, p.beta, p.angle, noise=k) for p, k in zip(base, keys)]
    a1, a2 = aug.tables(base)
    n1, n2 = aug.tables(noisy)
    assert n1.shape == a1.shape and n2.shape == a2.shape and n1.dtype == n2.dtype == np.int32
    assert n1.strides == a1.strides and n2.strides == a2.strides and n1.base.shape == a1.base.shape and n2.base is n1.base
    assert (a2[:, 1:4] == 0).all()
    for b, k in enumerate(keys):
        words = n2[b, 1:4].view(np.uint32)
        assert tuple(int(w) for w in words) == ((0, 0, 0) if k is None else (k & 0xffffffff, k >> 32, 1)), (b, k)
    rest = np.ones(n2.shape[1], bool)
    rest[1:4] = False
    assert np.array_equal(n1, a1) and np.array_equal(n2[:, rest], a2[:, rest])           # nothing else moves, word 0 included
    assert n2[2, 2] < 0 and n2[4, 1] < 0                                       # the high bit of a half is the int32 word's sign


def test_noise_keys_are_checked_on_the_host():
    aug = ClipAugmenter()
    for bad in (-1, 1 << 64):
        with pytest.raises(StswinHipError, match="64-bit key"):
            aug.params(672, 0, 0, noise=bad)
        with pytest.raises(StswinHipError, match="64-bit key"):
            aug.tables([ClipParams(672, 0, 0, noise=bad)])
    assert aug.params(672, 0, 0, noise=np.uint64(7)).noise == 7 and aug.params(672, 0, 0).noise is None
    assert math.isclose(255.0 * math.sqrt(aug.noise_var), 8.0638, abs_tol=1e-4) and augment.MAX_THRESHOLDS == 1024


def test_the_entry_point_refuses_before_it_launches():
    """Every refusal of stswin_augment_noise returns its documented code without touching a pointer (none of these is a device
    address) or a device (there is none here)."""
    import ctypes

    from stswincl_amd import hip
    lib = hip.load()
    assert "stswin_augment_noise" in hip.declared_symbols()
    assert lib.stswin_augment_noise.argtypes[2] is ctypes.c_long and lib.stswin_augment_noise.argtypes[7] is ctypes.c_long
    stride = hip.augment_finish_table_stride(1, 1)
    assert stride == 72

    def call(crop=64, table=64, stride=stride, thr=64, n_thr=103, k_min=-52, B=2, sample_bytes=1152):
        return lib.stswin_augment_noise(crop, table, stride, thr, n_thr, k_min, B, sample_bytes, None)

    for kw in (dict(B=0), dict(B=-1), dict(sample_bytes=0), dict(sample_bytes=-4), dict(sample_bytes=1150), dict(sample_bytes=(1 << 34) + 4)):
        assert call(**kw) == -1808, kw
    for kw in (dict(crop=None), dict(table=None), dict(thr=None)):
        assert call(**kw) == -1809, kw
    for kw in (dict(n_thr=0), dict(n_thr=-1), dict(n_thr=1025)):
        assert call(**kw) == -1810, kw
    for kw in (dict(stride=stride - 1), dict(stride=4), dict(stride=0)):
        assert call(**kw) == -1819, kw
