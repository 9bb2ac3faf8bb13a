"""CaDIS evaluation on the MI355X (segcata/cata_test.py:115-170): the upsample + argmax + confusion-matrix kernel against torch and
against a bincount of its own labels, 64-bit accumulation, the per-channel ingest against the Pillow restatement and the CaDIS
table, the segmenter under protocol="cadis" against model(clip) per frame, its modes against each other, and the pooled matrix
against utils.cata_metrics.ConfusionMatrix."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import labels_ref
import pil_resize_ref as R
from stswincl_amd import hip, video
from stswincl_amd.net.Ours.base_cata_np import TswinPlusv5
from stswincl_amd.utils.cata_metrics import ConfusionMatrix

pytestmark = pytest.mark.gpu

TIE_BOUND = 2e-4          # labels may differ from torch's on this fraction of pixels (exact near-ties), as for upsample_argmax


def _gt(F_, H, W, ncm, nc, seed):
    """Ground truth with the ignore label ncm, negatives and values above the model's classes."""
    g = torch.from_numpy(np.random.default_rng(seed).integers(-1, nc + 4, (F_, H, W)))
    g[:, : H // 5, : W // 4] = ncm
    return g.long().cuda()


def _bincount(gt, labels, ncm):
    gt, p = gt.reshape(-1).long(), labels.reshape(-1).long()
    keep = (gt >= 0) & (gt < ncm) & (p >= 0) & (p < ncm)
    return torch.bincount(gt[keep] * ncm + p[keep], minlength=ncm * ncm).reshape(ncm, ncm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nc", [9, 18, 26])
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("h,w,H,W", [(64, 80, 540, 960), (23, 37, 101, 77)])
def test_kernel_matches_torch_and_counts_its_own_labels(dtype, nc, align, h, w, H, W):
    torch.manual_seed(nc * 7 + h)
    F_ = 2
    logits = (torch.randn(F_, nc, h, w, device="cuda") * 3).to(dtype)
    ncm = nc - 1
    gt = _gt(F_, H, W, ncm, nc, seed=nc + H)
    cm = torch.zeros(ncm, ncm, dtype=torch.int64, device="cuda")
    labels = hip.upsample_argmax_cm(logits, H, W, gt=gt, cm=cm, align_corners=align)
    want = F.softmax(F.interpolate(logits.float(), (H, W), mode="bilinear", align_corners=align), dim=1).argmax(1)
    assert labels.dtype == torch.uint8 and labels.shape == (F_, H, W)
    differ = (labels.long() != want).float().mean().item()
    print(f"[cata] {dtype} nc {nc} align {align} {h}x{w}->{H}x{W}: {differ:.2e} of labels differ from torch")
    assert differ < TIE_BOUND
    assert labels_ref.outside(logits, labels, H, W, int(align))[0] == 0      # every label is one its float64 values allow
    assert torch.equal(cm, _bincount(gt, labels, ncm))
    assert int(cm.sum()) > 0
    # the same matrix without the label write, and the label-only form
    cm2 = torch.zeros_like(cm)
    assert hip.upsample_argmax_cm(logits, H, W, gt=gt, cm=cm2, align_corners=align, labels=False) is None
    assert torch.equal(cm2, cm)
    assert torch.equal(hip.upsample_argmax_cm(logits, H, W, align_corners=align), labels)
    if align:
        assert torch.equal(hip.upsample_argmax(logits, H, W)[0], labels)      # the EndoVis kernel's formula


def test_matrix_accumulates_over_launches_in_64_bits():
    torch.manual_seed(5)
    logits = torch.randn(3, 9, 64, 80, device="cuda")
    gt = _gt(3, 540, 960, 8, 9, seed=3)
    base = (1 << 31) - 8
    cm = torch.full((8, 8), base, dtype=torch.int64, device="cuda")
    once = torch.zeros(8, 8, dtype=torch.int64, device="cuda")
    for _ in range(3):
        hip.upsample_argmax_cm(logits, 540, 960, gt=gt, cm=cm, align_corners=False, labels=False)
    hip.upsample_argmax_cm(logits, 540, 960, gt=gt, cm=once, align_corners=False, labels=False)
    assert int(once.max()) > 8
    assert torch.equal(cm, base + 3 * once)
    assert int(cm.min()) >= base                                             # no bin wrapped past 2^31


def test_refusals():
    lg = torch.zeros(1, 9, 8, 8, device="cuda")
    gt = torch.zeros(1, 16, 16, dtype=torch.int64, device="cuda")
    with pytest.raises(hip.StswinHipError):
        hip.upsample_argmax_cm(lg, 16, 16, gt=gt)                            # gt without a matrix
    with pytest.raises(hip.StswinHipError):
        hip.upsample_argmax_cm(lg, 16, 16, gt=gt, cm=torch.zeros(8, 8, dtype=torch.int32, device="cuda"))
    with pytest.raises(hip.StswinHipError):
        hip.upsample_argmax_cm(torch.zeros(1, 65, 8, 8, device="cuda"), 16, 16)
    with pytest.raises(hip.StswinHipError):
        hip.upsample_argmax_cm(lg, 16, 16, labels=False)


def _frames(n, hs, ws, seed):
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (1, hs, ws, 3), dtype=np.int64)
    fr = base + g.integers(-24, 25, (n, hs, ws, 3))
    return np.clip(fr, 0, 255).astype(np.uint8)


def _cadis_host(frames, h, w):
    """CATA_new_512.py's test transform on the host: PIL BILINEAR to (w, h), then the CaDIS table per channel."""
    tab = video.cadis_value_table()
    out = []
    for f in frames:
        u = R.resize(f, h, w)
        out.append(np.stack([tab[c][u[..., c]] for c in range(3)]))
    return torch.from_numpy(np.stack(out))


@pytest.mark.parametrize("hs,ws,h,w", [(540, 960, 512, 640), (37, 53, 16, 20)])
def test_per_channel_ingest_is_bit_exact(hs, ws, h, w):
    fr = _frames(3, hs, ws, seed=hs + ws)
    fr[0, :8] = 255
    fr[0, 8:16] = 0
    dev = torch.from_numpy(fr).cuda()
    got = video.ingest(dev, (h, w), protocol="cadis")
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), _cadis_host(fr, h, w))
    # the one-table entry point still gives float32(u / 255.)
    assert torch.equal(video.ingest(dev, (h, w)).cpu(), torch.from_numpy(np.stack([R.transform(f, h, w) for f in fr])))


def _model(nc, res, seed=0):
    torch.manual_seed(seed)
    m = TswinPlusv5(nc, res)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def full_size():
    m = _model(9, (64, 80), seed=2)
    fr = _frames(12, 540, 960, seed=11)
    images = _cadis_host(fr, 512, 640).cuda()
    return m, fr, images


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_segmenter_gives_the_logits_of_model_clip(full_size, mode):
    m, fr, images = full_size
    assert tuple(m.swin.input_resolution) == (64, 80)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
        seg = video.VideoSegmenter(m, protocol="cadis")
        res = dict(seg.push(fr))
        res.update(seg.finish())
        assert sorted(res) == list(range(12))
        for f in range(12):
            want = m(images[list(video.clip_frames(f, rule="cadis"))][None])[0]
            assert res[f].dtype == want.dtype and torch.equal(res[f], want), f


def test_modes_agree_and_the_matrix_pools_sequences():
    m = _model(9, (16, 16), seed=3)
    n, size = 12, (150, 170)
    seqs = [_frames(n, 200, 240, seed=20), _frames(n + 3, 200, 240, seed=21)]
    gts = [_gt(len(s), *size, 8, 9, seed=30 + i) for i, s in enumerate(seqs)]
    with torch.no_grad():
        online = video.VideoSegmenter(m, out="labels", out_size=size, protocol="cadis")
        on = {}
        for f in range(n):
            for g, r in online.push(seqs[0][f], gt=gts[0][f:f + 1]):
                on[g] = r.clone()
        on.update((g, r.clone()) for g, r in online.finish())
        batched = video.VideoSegmenter(m, batch=4, out="labels", out_size=size, protocol="cadis")
        off = batched.segment_sequence(seqs[0], gt=gts[0])
        graphed = video.VideoSegmenter(m, graph=True, out="labels", out_size=size, protocol="cadis")
        gr = graphed.segment_sequence(torch.from_numpy(seqs[0]).cuda(), gt=gts[0])
        plain = video.VideoSegmenter(m, graph=True, out="labels", out_size=size, protocol="cadis")
        pl = plain.segment_sequence(seqs[0])                                  # labels inside the captured step
        assert graphed._g is not None and plain._g is not None and plain._g[4] is not None
        assert sorted(on) == list(range(n))
        for f in range(n):
            assert on[f].dtype == torch.uint8 and on[f].shape == size
            assert torch.equal(off[f], on[f]) and torch.equal(gr[f], on[f]) and torch.equal(pl[f], on[f]), f
        cm = online.confusion_matrix()
        assert cm.dtype == np.float64 and cm.shape == (8, 8) and cm.sum() > 0
        assert np.array_equal(batched.confusion_matrix(), cm) and np.array_equal(graphed.confusion_matrix(), cm)
        assert not plain.confusion_matrix().any()

        # a second sequence: reset() keeps the matrix, the pool equals the numpy ConfusionMatrix over both
        ref = ConfusionMatrix(8)
        for f in range(n):
            ref.update_confusion_matrix(gts[0][f].cpu().numpy(), on[f].cpu().numpy())
        second = graphed.segment_sequence(seqs[1], gt=gts[1])
        for f in range(len(seqs[1])):
            ref.update_confusion_matrix(gts[1][f].cpu().numpy(), second[f].cpu().numpy())
        assert np.array_equal(graphed.confusion_matrix(), ref.get_confusion_matrix())
        # the drop-in's device path counts the same from the logits
        logits = video.VideoSegmenter(m, protocol="cadis").segment_sequence(seqs[1])
        dev = ConfusionMatrix(8)
        dev.update_from_logits(torch.stack(logits), gts[1], size)
        one = ConfusionMatrix(8)
        for f in range(len(seqs[1])):
            one.update_confusion_matrix(gts[1][f].cpu().numpy(), second[f].cpu().numpy())
        assert np.array_equal(dev.get_confusion_matrix(), one.get_confusion_matrix())
        graphed.reset_metrics()
        assert not graphed.confusion_matrix().any()


def test_cadis_refusals():
    m = _model(9, (8, 8), seed=5)
    with torch.no_grad():
        seg = video.VideoSegmenter(m, protocol="cadis", out_size=(64, 64))
        seg.push(_frames(7, 64, 64, seed=1))
        with pytest.raises(hip.StswinHipError, match=">= 8 frames"):
            seg.finish()
    with pytest.raises(hip.StswinHipError):
        video.VideoSegmenter(m, protocol="cata")
    with pytest.raises(hip.StswinHipError):
        video.VideoSegmenter(m, align_corners=False)                        # (an EndoVis segmenter resizes with align_corners=True)
    assert video.VideoSegmenter(m, protocol="cadis").out_size == (540, 960)
    assert video.VideoSegmenter(m, protocol="cadis").metric_classes == 8
