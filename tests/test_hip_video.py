"""stswincl_amd.video on the MI355X: the frame-ingest kernel against the Pillow restatement, the clip assembly against torch
indexing, the segmenter against the fp32 oracle and against model(clip) per frame, and online / offline / graph replay against
each other (seg18/test.py:147-175 over seg18/dataset/Endovis2018_new.py:109-127)."""
import numpy as np
import pytest
import torch

import pil_resize_ref as R
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.net.Ours.base18 import TswinPlus

pytestmark = pytest.mark.gpu

SIZES = [(1024, 1280, 512, 640), (1080, 1920, 512, 640), (540, 960, 512, 640), (256, 320, 512, 640), (37, 53, 16, 20),
         (540, 640, 512, 640), (512, 960, 512, 640), (512, 640, 512, 640)]     # (one axis changes: one pass)

# Same answer as model(clip), 10 frames 1024x1280 -> 512x640, TswinPlus(12, (64, 80)): the segmenter runs the ResNet on one to four
# frames per launch, model(clip) on four.  Measured on one MI355X: bitwise in fp32 and in bf16.  (bf16 before the segmenter planned its
# GEMMs as for the clip's four frames, hip.splitk_as_rows: 4.42e-3 relative L2, against 6.11e-3 for the clip path's own bf16-vs-fp32
# deviation - one frame's layer4 convolutions took the split-K kernel, four frames' do not.)
MEASURED = {"fp32": 0.0, "bf16": 0.0}


def _frames(n, hs, ws, seed):
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (1, hs, ws, 3), dtype=np.int64)
    fr = base + g.integers(-24, 25, (n, hs, ws, 3))                # a sequence: frames close to each other
    return np.clip(fr, 0, 255).astype(np.uint8)


def _host_transform(frames, h, w):
    return torch.from_numpy(np.stack([R.transform(f, h, w) for f in frames]))


def _clip(images, f):
    return images[list(video.clip_frames(f))][None]


def _model(nc, res, seed=0):
    torch.manual_seed(seed)
    m = TswinPlus(nc, res)
    for mod in m.modules():                              # non-trivial running statistics: eval-mode BatchNorm is not the identity
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    return m.cuda().eval()


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hs,ws,h,w", SIZES)
def test_ingest_is_bit_exact_with_pillow_and_the_value_table(n, hs, ws, h, w):
    fr = _frames(n, hs, ws, seed=hs + ws + n)
    fr[0, :8] = 255
    fr[0, 8:16] = 0
    got = video.ingest(torch.from_numpy(fr).cuda(), (h, w))
    want = _host_transform(fr, h, w)
    assert got.dtype == torch.float32 and got.shape == (n, 3, h, w)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("amp", [False, True])
def test_ingested_frames_give_the_logits_of_the_host_transform(amp):
    m = _model(12, (8, 8))
    fr = _frames(4, 80, 96, seed=5)
    img_dev = video.ingest(torch.from_numpy(fr).cuda(), (64, 64))
    img_host = _host_transform(fr, 64, 64).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        a = m(img_dev[None])
        b = m(img_host[None])
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_clip_assembly_is_torch_indexing(B, dtype):
    g = torch.Generator().manual_seed(B)
    S, L, C, n_new = 7, 40, 512, 3
    ring = torch.randn(S, L, C, generator=g).to(dtype).cuda()
    fresh = torch.randn(n_new, L, C, generator=g).to(dtype).cuda()
    rnd = np.random.default_rng(B)
    stores = [int(s) for s in rnd.choice(S, size=n_new, replace=False)]
    stores[-1] = -1                                          # a new frame that is not kept
    readable = [s for s in range(S) if s not in stores]
    src = [int(rnd.choice(readable)) if rnd.random() < 0.6 else -1 - int(rnd.integers(n_new)) for _ in range(4 * B)]
    src[0], src[-1] = readable[-1], -1 - (n_new - 1)        # the last slot (wrap) and the last new frame are read
    table = torch.tensor(src + stores, dtype=torch.int32).cuda()
    ring0 = ring.clone()
    clips = torch.empty(B, 4, L, C, dtype=dtype, device="cuda")
    hip.clip_assemble(ring, fresh, clips, table, B, n_new)
    both = torch.cat([ring0, fresh])
    idx = torch.tensor([e if e >= 0 else S + (-1 - e) for e in src])
    assert torch.equal(clips.cpu(), both.cpu()[idx].view(B, 4, L, C))
    want_ring = ring0.clone()
    for j, s in enumerate(stores):
        if s >= 0:
            want_ring[s] = fresh[j]
    assert torch.equal(ring.cpu(), want_ring.cpu())


def test_segmenter_matches_the_fp32_oracle():
    """8 frames of 64x64, TswinPlus(12, (8, 8)), fp32 path: every frame's logits against oracle.tswin_plus on the reference's
    clip of that frame (1e-3 relative, the project's gate)."""
    from oracle import stswin_oracle as O
    m = _model(12, (8, 8), seed=1)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    fr = _frames(8, 64, 64, seed=8)
    images = _host_transform(fr, 64, 64)
    seg = video.VideoSegmenter(m)
    res = seg.segment_sequence(fr)
    assert len(res) == 8
    for f in range(8):
        with torch.no_grad():
            ref = O.tswin_plus(_clip(images, f), sd, training=False)[0]
        e = float((res[f].cpu() - ref).norm() / ref.norm())
        assert e < 1e-3, (f, e)


@pytest.fixture(scope="module")
def full_size():
    m = _model(12, (64, 80), seed=2)
    fr = _frames(10, 1024, 1280, seed=10)
    images = video.ingest(torch.from_numpy(fr).cuda(), (512, 640))
    return m, fr, images


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_segmenter_gives_the_logits_of_model_clip(full_size, mode):
    m, fr, images = full_size
    amp = mode == "bf16"
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        seg = video.VideoSegmenter(m)
        res = dict(seg.push(fr))
        res.update(seg.finish())
        diffs, devs = [], []
        for f in range(10):
            want = m(_clip(images, f))[0]
            diffs.append(_rel(res[f], want))
            if amp and f in (0, 5):
                with torch.autocast("cuda", enabled=False):
                    devs.append(_rel(want, m(_clip(images, f))[0]))
    print(f"[video] {mode}: segmenter vs model(clip) max rel {max(diffs):.3e}" + (f"; clip path bf16 vs fp32 {min(devs):.3e}" if devs else ""))
    assert max(diffs) == MEASURED[mode] == 0.0
    if devs:
        assert min(devs) > 0.0


def test_online_offline_and_graph_agree():
    m = _model(12, (16, 16), seed=3)
    fr = _frames(20, 200, 240, seed=20)                       # -> 128x128
    with torch.no_grad():
        online = video.VideoSegmenter(m)
        on = {}
        for f in range(20):
            for g, r in online.push(fr[f]):
                on[g] = r.clone()
        on.update((g, r.clone()) for g, r in online.finish())
        off = video.VideoSegmenter(m, batch=4).segment_sequence(fr)
        graphed = video.VideoSegmenter(m, graph=True)
        gr = {}
        for f in range(20):
            for g, r in graphed.push(torch.from_numpy(fr[f]).cuda()):
                gr[g] = r.clone()
        gr.update((g, r.clone()) for g, r in graphed.finish())
        # whole sequences through the graph: many replays inside one push, CPU frames copied from pinned memory
        whole = video.VideoSegmenter(m, graph=True).segment_sequence(fr)
        one_push = video.VideoSegmenter(m, graph=True)
        res = one_push.push(torch.from_numpy(fr).cuda())
        last = res[-1][1].clone()
        res = {g: r.clone() for g, r in res}
        res.update((g, r.clone()) for g, r in one_push.finish())
    assert graphed._g is not None and one_push._g is not None
    assert sorted(on) == sorted(gr) == sorted(res) == list(range(20)) and len(off) == len(whole) == 20
    for f in range(20):
        assert torch.equal(off[f], on[f]), f                   # fp32: bitwise, as the bound above
        assert torch.equal(gr[f], on[f]), f
        assert torch.equal(whole[f], on[f]), f
        assert torch.equal(res[f], on[f]), f
    assert torch.equal(last, on[19])


def test_graph_replay_gives_the_eager_labels():
    m = _model(12, (8, 8), seed=6)
    fr = _frames(12, 80, 96, seed=12)
    with torch.no_grad():
        eager = video.VideoSegmenter(m, out="labels", out_size=(96, 80)).segment_sequence(fr)
        graphed = video.VideoSegmenter(m, out="labels", out_size=(96, 80), graph=True)
        got = graphed.segment_sequence(fr)
    assert graphed._g is not None and graphed._g[4] is not None      # the labels are computed inside the captured step
    for f in range(12):
        assert got[f].dtype == torch.uint8 and torch.equal(got[f], eager[f]), f


def test_labels_and_scores_match_predict_and_score():
    from stswincl_amd.utils.EndoMetric import predict_and_score
    m = _model(12, (8, 8), seed=4)
    fr = _frames(9, 64, 64, seed=9)
    gt = torch.from_numpy(np.random.default_rng(0).integers(0, 12, (9, 96, 80))).long()
    with torch.no_grad():
        logits = video.VideoSegmenter(m).segment_sequence(fr)
        res = video.VideoSegmenter(m, out="labels", out_size=(96, 80)).segment_sequence(fr, gt=gt)
        plain = video.VideoSegmenter(m, out="labels", out_size=(96, 80)).segment_sequence(fr)
    for f in range(9):
        labels, dices, ious = predict_and_score(logits[f][None], (96, 80), gt[f:f + 1].cuda())
        lab, dc, io = res[f]
        assert lab.dtype == torch.uint8 and torch.equal(lab, labels[0]) and torch.equal(plain[f], labels[0])
        assert dc == dices[0] and io == ious[0]


def test_refusals():
    m = _model(12, (8, 8), seed=5)
    fr = _frames(2, 64, 64, seed=1)
    m.train()
    with pytest.raises(StswinHipError, match="eval"):
        video.VideoSegmenter(m)
    m.eval()
    seg = video.VideoSegmenter(m)
    m.train()
    with pytest.raises(StswinHipError, match="eval"):
        seg.push(fr)
    m.eval()
    with pytest.raises(StswinHipError, match="GPU"):
        video.VideoSegmenter(TswinPlus(12, (8, 8)).eval())
    seg.push(fr)
    with pytest.raises(StswinHipError, match="frame size"):
        seg.push(_frames(1, 64, 72, seed=2))
