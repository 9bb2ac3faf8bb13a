"""CaDIS's Gaussian noise on the GPU (stswin_augment_noise through hip.augment_noise and ClipAugmenter) against the numpy statement
tests/augment_noise_ref.py: Philox4x32-10 counted by the byte index, the law as thresholds, clamp.  Integer arithmetic throughout, so
every comparison is torch.equal over all bytes."""
import numpy as np
import pytest
import torch

import augment_noise_ref as nr
import augment_ref as ar
from stswincl_amd import hip
from stswincl_amd.augment import ClipAugmenter, noise_thresholds
from stswincl_amd.hip import StswinHipError

pytestmark = pytest.mark.gpu

HW = (64, 80)
KEYS = (0xffffffff80000001, None, 0x80000000fffffffe)            # a high bit in either half: negative int32 table words
GUARD = 64
_LAW = {}


def law():
    if not _LAW:
        thr, k_min = noise_thresholds(0.001)
        _LAW["thr"], _LAW["k_min"] = torch.from_numpy(thr.view(np.int32).copy()).cuda(), k_min
    return _LAW["thr"], _LAW["k_min"]


def table(keys, stride=None):
    """Stage-2 rows with only the head that the noise pass reads; every other word is set, to show that it is not looked at."""
    stride = hip.augment_finish_table_stride(1, 1) if stride is None else stride
    t = np.full((len(keys), stride), 0x5a5a5a5a, np.uint32)
    for b, k in enumerate(keys):
        t[b, 1:4] = (0, 0, 0) if k is None else (k & 0xffffffff, k >> 32, 1)
    return torch.from_numpy(t.view(np.int32)).cuda()


def run_raw(data: np.ndarray, keys, offset=0):
    """data uint8 [B][sample_bytes] -> the kernel's output, from a view `offset` bytes into an allocation with guard bytes around it."""
    B, sb = data.shape
    buf = torch.full((GUARD + offset + B * sb + GUARD,), 0xa5, dtype=torch.uint8, device="cuda")
    view = buf[GUARD + offset:GUARD + offset + B * sb].view(B, sb)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + GUARD + offset
    view.copy_(torch.from_numpy(data))
    thr, k_min = law()
    res = hip.augment_noise(view, table(keys), thr, k_min)
    assert res is view
    out = buf.cpu()
    assert (out[:GUARD + offset] == 0xa5).all() and (out[GUARD + offset + B * sb:] == 0xa5).all()          # nothing outside the samples
    return out[GUARD + offset:GUARD + offset + B * sb].view(B, sb)


def want_raw(data, keys):
    return torch.from_numpy(np.stack([d if k is None else nr.add_noise(d, k) for d, k in zip(data, keys)]))


# 420 = 4 * 5 * 7 * 3: 4-byte units in front of and behind the 16-byte body, sample bases 1 and 2 not 16-byte aligned; 61 440: more
# than one workgroup per sample.  Offset 4: a view inside an allocation; offset 1: no 4-byte alignment, every unit byte by byte.
@pytest.mark.parametrize("sample_bytes,offset", [(420, 0), (1152, 0), (61440, 0), (420, 4), (1152, 4), (61440, 4), (420, 1), (4, 12)])
def test_raw_bytes_equal_the_reference(sample_bytes, offset):
    data = np.random.default_rng(sample_bytes + offset).integers(0, 256, (3, sample_bytes), dtype=np.uint8)
    got = run_raw(data, KEYS, offset)
    assert torch.equal(got, want_raw(data, KEYS))
    assert torch.equal(got[1], torch.from_numpy(data[1]))                    # the switched-off sample is its input
    assert not torch.equal(got[0], torch.from_numpy(data[0])) or sample_bytes == 4


def test_all_0_and_all_255_clamp_and_show_the_counter_to_byte_mapping():
    n = 1152
    key = 0x0123456789abcdef
    k = nr.offsets(n, key)
    assert k.min() < 0 < k.max()
    data = np.stack([np.zeros(n, np.uint8), np.full(n, 255, np.uint8)])
    got = run_raw(data, (key, key))
    assert torch.equal(got[0], torch.from_numpy(np.maximum(k, 0).astype(np.uint8)))           # 0 where K <= 0, K elsewhere
    assert torch.equal(got[1], torch.from_numpy((255 + np.minimum(k, 0)).astype(np.uint8)))


def test_the_key_alone_decides_the_noise():
    data = np.full((3, 1152), 128, np.uint8)
    got = run_raw(data, (7, 7, 8))
    assert torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2])
    again = run_raw(data, (8, 7, 7), offset=4)                               # another launch, another alignment, another sample slot
    assert torch.equal(again[0], got[2]) and torch.equal(again[1], got[0])


def small_aug(**kw):
    return ClipAugmenter(crop=HW, base_w=84, protocol="cadis", class_num=18, source=HW, **kw)


def small_batch(seeds):
    clips = [ar.seeded_clip(s, 4, *HW, classes=18) for s in seeds]
    frames, labels = np.stack([c[0] for c in clips]), np.stack([c[1] for c in clips])
    labels[:, 3::11, 5::7] = 255                                             # (CaDIS's ignore label)
    return frames, labels, torch.from_numpy(frames).cuda(), torch.from_numpy(labels).cuda()


def test_noise_stage_in_place_and_the_four_frames_differ():
    aug = small_aug()
    crop = torch.full((2, 4, *HW, 3), 128, dtype=torch.uint8, device="cuda")
    params = [aug.params(80, 0, 0, noise=3), aug.params(80, 0, 0)]
    res = aug.noise_stage(crop, params)
    assert res is crop
    got = crop.cpu()
    assert torch.equal(got[0], torch.from_numpy(nr.add_noise(np.full((4, *HW, 3), 128, np.uint8), 3)))
    assert (got[1] == 128).all()
    for i in range(4):
        for j in range(i + 1, 4):
            assert not torch.equal(got[0, i], got[0, j])


def reference(frames, labels, params, noise=True):
    imgs, labs = [], []
    for f, l, p in zip(frames, labels, params):
        crops, lab = ar.scale_crop(f, l, p, HW)
        if noise and p.noise is not None:
            crops = nr.add_noise(crops, p.noise)                             # flips -> noise -> rotate -> normalise
        crops, lab = ar.rotate(crops, lab, p.angle, ar.value_table(p.alpha, p.beta))
        imgs.append(ar.to_float(crops, "cadis"))
        labs.append(ar.label_table("cadis", 18)[lab])
    return torch.from_numpy(np.stack(imgs)), torch.from_numpy(np.stack(labs))


def mixed_params(aug):
    return [aug.params(120, 10, 5, hflip=True, angle=-21.0, noise=0xfedcba9876543210), aug.params(60, 0, 0, vflip=True, angle=48.5),
            aug.params(84, 2, 1, hflip=True, vflip=True, noise=0x00000001ffffffff), aug.params(168, 88, 70)]


def test_end_to_end_cadis():
    aug = small_aug()
    params = mixed_params(aug)
    frames, labels, dframes, dlabels = small_batch([0, 1, 2, 3])
    img, lab = aug(dframes, dlabels, params)
    want_img, want_lab = reference(frames, labels, params)
    assert img.dtype == torch.float32 and lab.dtype == torch.int64
    assert torch.equal(img.cpu(), want_img) and torch.equal(lab.cpu(), want_lab)
    plain_img, plain_lab = reference(frames, labels, params, noise=False)
    assert torch.equal(want_lab, plain_lab)                                  # labels are unaffected by noise
    for b, p in enumerate(params):
        assert torch.equal(want_img[b], plain_img[b]) == (p.noise is None), b
    assert int(lab.max()) == 17


def test_out_allocates_nothing_and_a_batch_without_a_key_skips_the_pass():
    aug = small_aug()
    frames, labels, dframes, dlabels = small_batch([4, 5, 6, 7])
    out = (torch.zeros(4, 4, 3, *HW, device="cuda"), torch.zeros(4, *HW, dtype=torch.int64, device="cuda"))
    aug(dframes, dlabels, [aug.params(100, 1, 1, noise=1)] + [aug.params(100, 1, 1)] * 3, out=out)       # (the first call makes the workspace)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    params = mixed_params(aug)
    res = aug(dframes, dlabels, params, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert res[0] is out[0] and res[1] is out[1]
    want_img, want_lab = reference(frames, labels, params)
    assert torch.equal(out[0].cpu(), want_img) and torch.equal(out[1].cpu(), want_lab)
    quiet = [aug.params(p.long_size, p.x1, p.y1, p.hflip, p.vflip, p.alpha, p.beta, p.angle) for p in params]
    aug(dframes, dlabels, quiet, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    crops = aug._workspace(4, dframes.device)["crop"].cpu()                  # what stage 2 read: stage 1's bytes, untouched
    for b, p in enumerate(quiet):
        assert torch.equal(crops[b], torch.from_numpy(ar.scale_crop(frames[b], labels[b], p, HW)[0])), b
    want_img, want_lab = reference(frames, labels, quiet)
    assert torch.equal(out[0].cpu(), want_img) and torch.equal(out[1].cpu(), want_lab)


def test_refusals_leave_the_buffer_alone():
    thr, k_min = law()
    data = torch.full((2, 1152), 77, dtype=torch.uint8, device="cuda")
    tab = table((5, 6))
    with pytest.raises(StswinHipError, match="augment_noise: crop must be a contiguous uint8"):
        hip.augment_noise(data.cpu(), tab, thr, k_min)
    with pytest.raises(StswinHipError, match="augment_noise: crop must be a contiguous uint8"):
        hip.augment_noise(data.to(torch.int8), tab, thr, k_min)
    with pytest.raises(StswinHipError, match="augment_noise: crop must be a contiguous uint8"):
        hip.augment_noise(data[:, ::2], tab, thr, k_min)
    with pytest.raises(StswinHipError, match="multiple of 4 bytes"):
        hip.augment_noise(data[:, :1150].contiguous(), tab, thr, k_min)
    with pytest.raises(StswinHipError, match=r"1 \.\. 1024 thresholds, got 1025"):
        hip.augment_noise(data, tab, torch.zeros(1025, dtype=torch.int32, device="cuda"), k_min)
    with pytest.raises(StswinHipError, match="augment_noise: thr"):
        hip.augment_noise(data, tab, thr.cpu(), k_min)
    with pytest.raises(StswinHipError, match="augment_noise: table"):
        hip.augment_noise(data, tab[:1], thr, k_min)
    with pytest.raises(StswinHipError, match="table rows must hold >= 72 words"):
        hip.augment_noise(data, table((5, 6), stride=71), thr, k_min)
    aug = small_aug()
    crop = torch.full((2, 4, *HW, 3), 77, dtype=torch.uint8, device="cuda")
    with pytest.raises(StswinHipError, match="one ClipParams per sample: 2, got 1"):
        aug.noise_stage(crop, [aug.params(80, 0, 0, noise=1)])
    with pytest.raises(StswinHipError, match="noise_stage: crop"):
        aug.noise_stage(crop[:, :3].contiguous(), [aug.params(80, 0, 0, noise=1)] * 2)
    torch.cuda.synchronize()
    assert (data == 77).all() and (crop == 77).all()
