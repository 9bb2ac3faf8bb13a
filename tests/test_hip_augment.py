"""The training-input augmenter on the GPU (stswincl_amd/augment.py over stswin_augment_crop / stswin_augment_finish) against the
numpy reference tests/augment_ref.py.  The arithmetic is integer until the last table lookup, so every comparison is torch.equal
over all pixels: no tolerance, no sampled subset."""
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
import pil_resize_ref as pr
from stswincl_amd import hip, video
from stswincl_amd.augment import ClipAugmenter, ClipParams
from stswincl_amd.hip import StswinHipError

pytestmark = pytest.mark.gpu

SRC = (512, 640)
CROP = (512, 640)
_CLIPS = {}


def clip(seed):
    if seed not in _CLIPS:
        frames, label = ar.seeded_clip(seed, 4, *SRC)
        label[3::41, 5::37] = 255                                            # (CaDIS's ignore label)
        _CLIPS[seed] = (frames, label)
    return _CLIPS[seed]


def batch(seeds):
    frames = np.stack([clip(s)[0] for s in seeds])
    labels = np.stack([clip(s)[1] for s in seeds])
    return frames, labels, torch.from_numpy(frames).cuda(), torch.from_numpy(labels).cuda()


def check_stage1(aug, params, seeds=None):
    seeds = list(range(len(params))) if seeds is None else seeds
    frames, labels, dframes, dlabels = batch(seeds)
    crops, lab = aug.crop_stage(dframes, dlabels, params)
    assert crops.dtype == torch.uint8 and tuple(crops.shape) == (len(params), 4, *CROP, 3)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (len(params), *CROP)
    crops, lab = crops.cpu(), lab.cpu()
    for b, p in enumerate(params):
        want_crops, want_lab = ar.scale_crop(frames[b], labels[b], p, CROP)
        assert torch.equal(crops[b], torch.from_numpy(want_crops)), (b, p)
        assert torch.equal(lab[b], torch.from_numpy(want_lab)), (b, p)


# ---------------------------------------------------------------------------------------------- stage 1
def test_stage1_upscale_downscale_identity():
    aug = ClipAugmenter()
    assert aug.ksize == 5
    check_stage1(aug, [aug.params(900, 100, 50), aug.params(336, 0, 0), aug.params(640, 0, 0), aug.params(1344, 704, 563)])


def test_stage1_crop_at_each_corner_of_the_scaled_image():
    aug = ClipAugmenter()
    ow, oh, _, _ = aug.scaled(aug.params(1000, 0, 0))
    assert (ow, oh) == (1000, 800)
    check_stage1(aug, [aug.params(1000, x1, y1) for x1, y1 in ((0, 0), (ow - 640, 0), (0, oh - 512), (ow - 640, oh - 512))], seeds=[1, 1, 2, 2])


def test_stage1_each_flip_combination():
    aug = ClipAugmenter()
    check_stage1(aug, [aug.params(672, 17, 9, hflip=h, vflip=v) for h in (False, True) for v in (False, True)], seeds=[0, 0, 0, 0])
    check_stage1(aug, [aug.params(500, 0, 0, hflip=True, vflip=True), aug.params(500, 0, 0, vflip=True)], seeds=[3, 3])      # padding moves with the flip


def test_stage1_mixed_parameters_in_one_batch():
    aug = ClipAugmenter()
    params = aug.sample(5, rng=random.Random(2018), gen=np.random.default_rng(2018))
    params[1] = aug.params(336, 0, 0, hflip=True)
    assert len({p.long_size for p in params}) == 5
    check_stage1(aug, params, seeds=[0, 1, 2, 3, 0])


# ---------------------------------------------------------------------------------------------- stage 2
def check_stage2(aug, params, seed):
    rng = np.random.default_rng(seed)
    B = len(params)
    crops = rng.integers(0, 256, (B, 4, *CROP, 3), dtype=np.uint8)
    labs = rng.integers(0, 12, (B, *CROP), dtype=np.uint8)
    img, lab = aug.finish_stage(torch.from_numpy(crops).cuda(), torch.from_numpy(labs).cuda(), params)
    assert img.dtype == torch.float32 and tuple(img.shape) == (B, 4, 3, *CROP) and lab.dtype == torch.int64
    img, lab = img.cpu(), lab.cpu()
    for b, p in enumerate(params):
        want, want_lab = ar.rotate(crops[b], labs[b], p.angle, ar.value_table(p.alpha, p.beta))
        assert torch.equal(img[b], torch.from_numpy(ar.to_float(want))), (b, p)
        assert torch.equal(lab[b], torch.from_numpy(want_lab.astype(np.int64))), (b, p)
    return crops, img


def test_stage2_rotations():
    aug = ClipAugmenter()
    crops, img = check_stage2(aug, [aug.params(640, 0, 0, angle=a) for a in (0.0, 90.0, -90.0, 1.5, 37.0)], seed=1)
    assert torch.equal(img[0], torch.from_numpy(ar.to_float(crops[0])))       # 0 degrees is a copy
    # 37 degrees: the corners of the output read across the border (reflected indices), which the reference check above covers
    colx, coly, rowx, rowy = (t.astype(np.int64) for t in ar.rotate_tables(37.0, *CROP))
    assert ((rowx[0] + colx[0]) >> 10) < 0 or ((rowy[0] + coly[0]) >> 10) < 0


def test_stage2_value_table_with_and_without_rotation():
    aug = ClipAugmenter()
    check_stage2(aug, [aug.params(640, 0, 0, alpha=1.2, beta=0.2), aug.params(640, 0, 0, alpha=0.8, beta=-0.2, angle=-63.0),
                       aug.params(640, 0, 0), aug.params(640, 0, 0, alpha=1.1, beta=-0.05, angle=90.0)], seed=2)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("protocol,class_num", [("endovis18", 12), ("cadis", 18)])
def test_end_to_end(protocol, class_num):
    aug = ClipAugmenter(protocol=protocol, class_num=class_num)
    params = [aug.params(415, 0, 0, hflip=True, alpha=1.13, beta=0.07, angle=-21.0), aug.params(1101, 333, 222, vflip=True, angle=48.5),
              aug.params(700, 10, 20)]
    frames, labels, dframes, dlabels = batch([0, 1, 2])
    img, lab = aug(dframes, dlabels, params)
    want_img, want_lab = ar.augment(frames, labels, params, CROP, protocol, class_num)
    assert img.dtype == torch.float32 and lab.dtype == torch.int64
    assert torch.equal(img.cpu(), torch.from_numpy(want_img)) and torch.equal(lab.cpu(), torch.from_numpy(want_lab))
    if protocol == "cadis":
        assert int(lab.max()) == class_num - 1 and (labels == 255).any()                 # 255 -> class_num - 1
        crops = ar.scale_crop(frames[2], labels[2], params[2], CROP)[0]                     # sample 2: no table, no rotation
        table = torch.from_numpy(video.cadis_value_table())
        for c in range(3):                                                                  # the per-plane table of the inference path
            assert torch.equal(img[2, :, c].cpu(), table[c][torch.from_numpy(crops[..., c].astype(np.int64))])


def test_out_writes_in_place_and_allocates_nothing():
    aug = ClipAugmenter()
    frames, labels, dframes, dlabels = batch([2, 3])
    out = (torch.zeros(2, 4, 3, *CROP, device="cuda"), torch.zeros(2, *CROP, dtype=torch.int64, device="cuda"))
    first = aug.sample(2, rng=random.Random(1), gen=np.random.default_rng(1))
    aug(dframes, dlabels, first, out=out)                                        # (the first call of a batch size makes the workspace)
    torch.cuda.synchronize()
    ptrs = (out[0].data_ptr(), out[1].data_ptr())
    before = torch.cuda.memory_allocated()
    params = [aug.params(820, 30, 40, vflip=True, alpha=0.9, beta=0.1, angle=15.0), aug.params(512, 0, 0, angle=-80.0)]
    res = aug(dframes, dlabels, params, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert res[0] is out[0] and res[1] is out[1] and (out[0].data_ptr(), out[1].data_ptr()) == ptrs
    want_img, want_lab = ar.augment(frames, labels, params, CROP)
    assert torch.equal(out[0].cpu(), torch.from_numpy(want_img)) and torch.equal(out[1].cpu(), torch.from_numpy(want_lab))


def test_back_to_back_calls_without_a_synchronise():
    """More calls in flight than the augmenter has pinned staging buffers (4), nothing between them that waits for the device: no
    call's tables may be overwritten before its copy has read them."""
    aug = ClipAugmenter()
    frames, labels, dframes, dlabels = batch([0, 1])
    rng, gen = random.Random(5), np.random.default_rng(5)
    sets = [aug.sample(2, rng=rng, gen=gen) for _ in range(7)]
    outs = [(torch.empty(2, 4, 3, *CROP, device="cuda"), torch.empty(2, *CROP, dtype=torch.int64, device="cuda")) for _ in sets]
    aug(dframes, dlabels, sets[0], out=outs[0])
    torch.cuda.synchronize()
    for params, out in zip(sets, outs):
        aug(dframes, dlabels, params, out=out)
    torch.cuda.synchronize()
    for params, out in zip(sets, outs):
        want_img, want_lab = ar.augment(frames, labels, params, CROP)
        assert torch.equal(out[0].cpu(), torch.from_numpy(want_img)) and torch.equal(out[1].cpu(), torch.from_numpy(want_lab)), params


# ---------------------------------------------------------------------------------------------- identity, model, training
def test_identity_parameters_equal_ingest_and_give_the_same_logits():
    from stswincl_amd.net.Ours.base18 import TswinPlus
    aug = ClipAugmenter()
    frames, labels, dframes, dlabels = batch([1])
    img, lab = aug(dframes, dlabels, [aug.identity()])
    ingested = video.ingest(dframes[0], CROP)
    assert torch.equal(img[0], ingested)
    assert torch.equal(lab.cpu(), torch.from_numpy(labels.astype(np.int64)))
    host = torch.from_numpy(np.stack([pr.transform(f, *CROP) for f in frames[0]]))[None]          # the reference's host transform
    assert torch.equal(img.cpu(), host)
    torch.manual_seed(0)
    m = TswinPlus(12).cuda().eval()
    with torch.no_grad():
        a = m(img).clone()
        b = m(host.cuda())
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_one_training_step_from_augmented_input():
    from stswincl_amd.net.Ours.base18 import TswinPlus
    from stswincl_amd.utils.losses import OhemCELoss2D
    hw = (128, 128)
    aug = ClipAugmenter(crop=hw, base_w=134, source=hw)
    clips = [ar.seeded_clip(s, 4, *hw) for s in (1, 2)]
    dframes = torch.from_numpy(np.stack([c[0] for c in clips])).cuda()
    dlabels = torch.from_numpy(np.stack([c[1] for c in clips])).cuda()
    params = aug.sample(2, rng=random.Random(3), gen=np.random.default_rng(3))
    img, lab = aug(dframes, dlabels, params)
    want_img, want_lab = ar.augment(np.stack([c[0] for c in clips]), np.stack([c[1] for c in clips]), params, hw)
    assert torch.equal(img.cpu(), torch.from_numpy(want_img)) and torch.equal(lab.cpu(), torch.from_numpy(want_lab))
    torch.manual_seed(0)
    m = TswinPlus(12, (16, 16)).cuda().train()
    loss = OhemCELoss2D(128 * 128 // 16)(m(img), lab)
    assert torch.isfinite(loss)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    aug = ClipAugmenter()
    frames, labels, dframes, dlabels = batch([0])
    ok = [aug.identity()]
    with pytest.raises(StswinHipError, match=r"uint8 \[B\]\[4\]\[512\]\[640\]\[3\].*labels is on the CPU"):
        aug(dframes, dlabels.cpu(), ok)
    with pytest.raises(StswinHipError, match=r"uint8 \[B\]\[4\]\[512\]\[640\]\[3\].*frames is on the CPU"):
        aug(dframes.cpu(), dlabels, ok)
    with pytest.raises(StswinHipError, match="frames is torch.float32"):
        aug(dframes.float(), dlabels, ok)
    with pytest.raises(StswinHipError, match="labels is torch.int64"):
        aug(dframes, dlabels.long(), ok)
    with pytest.raises(StswinHipError, match="not contiguous"):
        aug(dframes.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2), dlabels, ok)
    with pytest.raises(StswinHipError, match=r"\[B\]\[4\]\[512\]\[640\]\[3\].*frames is \(1, 4, 3, 512, 640\)"):
        aug(dframes.permute(0, 1, 4, 2, 3).contiguous(), dlabels, ok)
    with pytest.raises(StswinHipError, match="the sizes differ"):
        aug(dframes, dlabels[:, :256].contiguous(), ok)
    with pytest.raises(StswinHipError, match="source size"):
        aug(dframes[:, :, :256].contiguous(), dlabels[:, :256].contiguous(), ok)
    with pytest.raises(StswinHipError, match="T = 4"):
        aug(dframes[:, :3].contiguous(), dlabels, ok)
    with pytest.raises(StswinHipError, match="one ClipParams per sample"):
        aug(dframes, dlabels, ok * 2)
    with pytest.raises(StswinHipError, match="crop origin must satisfy 0 <= x1 <= 32 and 0 <= y1 <= 26"):
        aug(dframes, dlabels, [ClipParams(672, 33, 0)])
    with pytest.raises(StswinHipError, match="crop origin must satisfy"):
        aug(dframes, dlabels, [ClipParams(336, 0, 5)])
    with pytest.raises(StswinHipError, match="out must be"):
        aug(dframes, dlabels, ok, out=(torch.zeros(1, 4, 3, 512, 640, device="cuda"), torch.zeros(1, 512, 640, device="cuda")))
    ws = aug._workspace(1, dframes.device)
    lut, label_lut = aug._lut(dframes.device)
    img, lab = torch.empty(1, 4, 3, *CROP, device="cuda"), torch.empty(1, *CROP, dtype=torch.int64, device="cuda")
    with pytest.raises(StswinHipError, match=r"augment_finish: lut .* on the GPU"):
        hip.augment_finish(ws["crop"], ws["label_crop"], img, lab, ws["t2"], lut.cpu(), label_lut)               # a host pointer must not reach the kernel
    with pytest.raises(StswinHipError, match="augment_finish: label_lut"):
        hip.augment_finish(ws["crop"], ws["label_crop"], img, lab, ws["t2"], lut, label_lut.cpu())
    with pytest.raises(StswinHipError, match="augment_crop: table"):
        ws = aug._workspace(1, dframes.device)
        hip.augment_crop(dframes, dlabels, ws["tmp"], ws["crop"], ws["label_crop"], ws["t2"], aug.ksize)      # the other stage's (shorter) table
