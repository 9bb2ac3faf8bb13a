"""hip.instance_parts against the numpy definition (stswincl_amd/utils/instruments.py, instance_parts), and
VideoSegmenter(instance_groups=..., parts=...).  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

import test_hip_components as C
import test_hip_confidence as Q
import test_hip_tracks as T
from stswincl_amd import hip, video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import confidence as CF, instruments as I, rle

pytestmark = pytest.mark.gpu

FRAMES = 3
NCS = (1, 12, 64)


def _geo():
    return hip.instance_parts_geometry()


def _blocky(shape, hi, cell, seed):
    """Random maps of upscaled random blocks, so that runs exist; values 0 .. hi - 1."""
    n, H, W = shape
    g = np.random.default_rng(seed)
    cells = g.integers(0, hi, (n, -(-H // cell[0]), -(-W // cell[1])))
    return np.ascontiguousarray(np.repeat(np.repeat(cells, cell[0], axis=1), cell[1], axis=2)[:, :H, :W].astype(np.uint8))


def _check(lab, comp, K, nc):
    """hip.instance_parts of device labels and components equals the definition on their host copies -> (parts, contacts), on the host."""
    want = I.instance_parts(lab.cpu().numpy(), comp.cpu().numpy(), K, nc)
    got = hip.instance_parts(lab, comp, K, nc)
    assert all(t.is_cuda and t.dtype == torch.int64 for t in got)
    assert tuple(got[0].shape) == (lab.shape[0], K, nc, 10) and tuple(got[1].shape) == (lab.shape[0], K, nc)
    for g, w, what in zip(got, want, ("parts", "contacts")):
        bad = (g.cpu() != torch.from_numpy(w)).nonzero()
        assert bad.numel() == 0, (what, K, nc, bad[:6].tolist(), g.cpu()[tuple(bad[0])].item(), w[tuple(bad[0])].item())
    return want


def _shapes():
    g0, g1, _ = _geo()
    return [(1, 1), (1, 37), (37, 1), (g0 - 1, g1 - 1), (g0, g1), (g0 + 1, g1 + 1), (67, 131), (540, 960)]


# ------------------------------------------------------------------------------------------------ the kernel against the definition
@pytest.mark.parametrize("shape", range(8), ids=["1x1", "1x37", "37x1", "tile-1", "tile", "tile+1", "67x131", "540x960"])
def test_kernel_equals_the_definition(shape):
    H, W = _shapes()[shape]
    big = H * W > 100000
    some = 0
    for nc, K in [(nc, K) for nc in NCS for K in (1, 16, 1024)]:
        # K = 1024 wants more components than K: blocks of 1 x 2 pixels at 4-connectivity, where the map has room for them
        cell, conn = ((1, 2), 4) if K == 1024 else ((5, 9) if big else (3, 7), 8)
        lab = torch.from_numpy(_blocky((FRAMES, H, W), nc + 2, cell, seed=nc + K + H)).cuda()      # labels >= nc among them
        comp, _, total = hip.label_components(lab, nc, conn, (0,) if nc > 1 else (), 1024)
        if K == 1024 and nc >= 12 and H * W >= 4000:
            assert int(total.min()) > K, "fewer components than K: the truncation is not exercised"
        parts, contacts = _check(lab, comp, K, nc)
        assert int(contacts.max()) <= 4 * H * W
        some += int(parts[..., 0].sum()) > 0
    assert some or H * W == 1
    if big:                                                                  # every pixel of every tile in an instance below K
        lab = torch.from_numpy(_blocky((FRAMES, H, W), 14, (27, 41), seed=5)).cuda()
        comp, _, total = hip.label_components(lab, 12, 8, (), 1024)
        assert int(total.max()) <= 1024
        parts, _ = _check(lab, comp, 1024, 12)
        assert int(parts[..., 0].sum()) == int((lab < 12).sum())
    if (H, W) == (67, 131):                                                  # raw ordinals, unrelated to the labels: -1 and >= K
        g = np.random.default_rng(3)
        lab = torch.from_numpy(_blocky((FRAMES, H, W), 14, (2, 5), seed=9)).cuda()
        for K in (1, 16, 1024):
            raw = torch.from_numpy(np.repeat(g.integers(-1, K + 3, (FRAMES, H, -(-W // 3))), 3, axis=2)[:, :, :W].astype(np.int32).copy()).cuda()
            assert int(raw.min()) == -1 and int(raw.max()) >= K
            _check(lab, raw, K, 12)


def test_keys_past_the_on_chip_table_go_straight_to_the_outputs():
    g0, g1, slots = _geo()
    H, W, nc, K = g0 + 1, g1 + 1, 3, 1024
    ys, xs = np.mgrid[:H, :W]
    board = (1 + (ys + xs) % 2).astype(np.uint8)                             # a checkerboard of two classes: at 4-connectivity every
    lab = torch.from_numpy(np.stack([board, 3 - board, board])).cuda()       # pixel is its own component
    comp, _, total = hip.label_components(lab, nc, 4, (), 1024)
    assert total.tolist() == [H * W] * 3
    first = comp[0, :g0, :g1].cpu().numpy()                                  # the first tile: more distinct keys than the table has slots
    keys = np.unique(first[(first >= 0) & (first < K)].astype(np.int64) * nc + board[:g0, :g1][(first >= 0) & (first < K)])
    assert len(keys) > slots
    parts, contacts = _check(lab, comp, K, nc)
    assert int(parts[0, :, :, 0].sum()) == K and int(contacts[0].sum()) > 2 * K


# ------------------------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("W", [48, 37])
def test_any_pointer_alignment_and_nothing_else_is_written(W):
    H, nc, K = 40, 12, 16
    labels = torch.from_numpy(_blocky((FRAMES, H, W), nc + 2, (3, 7), seed=W)).cuda()
    comps = hip.label_components(labels, nc, 8, (0,), 1024)[0]
    assert labels.data_ptr() % 16 == 0 and comps.data_ptr() % 16 == 0        # fresh tensors: W = 48 takes the body with 16-byte loads
    want = hip.instance_parts(labels, comps, K, nc)
    ref = I.instance_parts(labels.cpu().numpy(), comps.cpu().numpy(), K, nc)
    assert torch.equal(want[0].cpu(), torch.from_numpy(ref[0])) and torch.equal(want[1].cpu(), torch.from_numpy(ref[1]))
    for lab_off, comp_off in ((0, 0), (1, 0), (0, 4), (1, 4), (3, 12)):
        lab, lab_buf = Q._padded(labels.shape, torch.uint8, lab_off)
        lab.copy_(labels)
        cc, cc_buf = Q._padded(comps.shape, torch.int32, comp_off)
        cc.copy_(comps)
        assert lab.data_ptr() % 16 == lab_off and cc.data_ptr() % 16 == comp_off
        pt, pt_buf = Q._padded((FRAMES, K, nc, 10), torch.int64, fill=-5)
        ct, ct_buf = Q._padded((FRAMES, K, nc), torch.int64, fill=-5)
        for _ in range(2):                                                   # a second call overwrites, it does not add
            got = hip.instance_parts(lab, cc, K, nc, out=(pt, ct))
            assert got[0] is pt and got[1] is ct
            assert torch.equal(pt, want[0]) and torch.equal(ct, want[1]), (lab_off, comp_off)
        assert Q._sentinels_hold(pt, pt_buf, -5) and Q._sentinels_hold(ct, ct_buf, -5)
        assert Q._sentinels_hold(lab, lab_buf) and Q._sentinels_hold(cc, cc_buf) and torch.equal(lab, labels) and torch.equal(cc, comps)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_wrapper_and_abi_refusals():
    lab = torch.zeros(2, 8, 10, dtype=torch.uint8, device="cuda")
    cc = torch.zeros(2, 8, 10, dtype=torch.int32, device="cuda")
    pt = torch.zeros(2, 4, 3, 10, dtype=torch.int64, device="cuda")
    ct = torch.zeros(2, 4, 3, dtype=torch.int64, device="cuda")
    for a, b, kw in ((lab[0], cc[0], {}), (lab.int(), cc, {}), (lab, cc.long(), {}), (lab, cc[:1], {}), (lab[:, :, ::2], cc[:, :, ::2], {}),
                     (lab, cc, dict(K=0)), (lab, cc, dict(K=1025)), (lab, cc, dict(K=4.0)), (lab, cc, dict(K=True)), (lab, cc, dict(nc=0)),
                     (lab, cc, dict(nc=65)), (lab, cc, dict(out=pt)), (lab, cc, dict(out=(pt, ct[:, :3]))), (lab, cc, dict(out=(pt.int(), ct))),
                     (lab, cc, dict(out=(pt, ct.cpu()))), (lab, cc, dict(out=(pt, pt.view(-1)[:24].view(2, 4, 3)))),
                     (lab.cpu(), cc, {}), (lab, cc.cpu(), {}), ("labels", cc, {})):
        with pytest.raises(StswinHipError, match="instance_parts"):
            hip.instance_parts(a, b, **{"K": 4, "nc": 3, **kw})
    both = torch.zeros(2 * 4 * 3 * 10 * 8, dtype=torch.uint8, device="cuda")   # out over the labels' own bytes
    with pytest.raises(StswinHipError, match="shares memory"):
        hip.instance_parts(both[:160].view(2, 8, 10), cc, 4, 3, out=(both.view(torch.int64).view(2, 4, 3, 10), ct))
    lib = hip.load()
    args = (lab.data_ptr(), cc.data_ptr(), pt.data_ptr(), ct.data_ptr())
    assert lib.stswin_instance_parts(*args, 0, 8, 10, 3, 4, None) == -1890
    assert lib.stswin_instance_parts(*args, 2, 8, 16385, 3, 4, None) == -1890
    assert lib.stswin_instance_parts(*args, 2, 0, 10, 3, 4, None) == -1890
    assert lib.stswin_instance_parts(args[0], None, args[2], args[3], 2, 8, 10, 3, 4, None) == -1891
    assert lib.stswin_instance_parts(*args[:3], None, 2, 8, 10, 3, 4, None) == -1891
    assert lib.stswin_instance_parts(*args, 2, 8, 10, 0, 4, None) == -1892
    assert lib.stswin_instance_parts(*args, 2, 8, 10, 65, 4, None) == -1892
    assert lib.stswin_instance_parts(*args, 2, 8, 10, 3, 0, None) == -1893
    assert lib.stswin_instance_parts(*args, 2, 8, 10, 3, 1025, None) == -1893
    assert lib.stswin_instance_parts(args[0], args[1] + 2, args[2], args[3], 2, 8, 10, 3, 4, None) == -1894
    assert lib.stswin_instance_parts(args[0], args[1], args[2] + 4, args[3], 2, 8, 10, 3, 4, None) == -1894
    assert lib.stswin_instance_parts(args[0], args[1], args[2], args[3] + 4, 2, 8, 10, 3, 4, None) == -1894
    torch.cuda.synchronize()
    pt.fill_(7)
    ct.fill_(7)
    assert lib.stswin_instance_parts(*args, 2, 8, 10, 3, 2000, None) == -1893
    torch.cuda.synchronize()
    assert bool((pt == 7).all()) and bool((ct == 7).all())                   # refused before anything was launched


# ------------------------------------------------------------------------------------------------------- the segmenter
SIZE, N, K = C.SIZE, C.N, C.K
LOW = 128
_MODES = {"eager": {}, "batch2": dict(batch=2), "graph": dict(graph=True)}
_GROUPS = {}


def _groups(protocol):
    """One group per protocol, from the tracks case's first sequence: the classes it predicts outside the skipped one, all but the
    rarest (which stays a class the instruments can touch) - chosen once, never changed."""
    if protocol not in _GROUPS:
        c = T._case(protocol)
        counts = np.bincount(c["seqs"][0]["labels"].numpy().reshape(-1), minlength=c["nc"])
        counts[list(c["skip"])] = 0
        seen = [int(k) for k in np.argsort(-counts, kind="stable") if counts[k] > 0]
        assert len(seen) >= 2, "the random model predicts one class: nothing to group"
        _GROUPS[protocol] = (tuple(sorted(seen[:-1] if len(seen) > 2 else seen)),)
    return _GROUPS[protocol]


def _own_parts(r, nc, components):
    """The last two elements of a parts="frame" result are instance_parts of the result's own labels and the given components [H][W]."""
    pt, ct = r[-2], r[-1]
    ok = pt.is_cuda and ct.is_cuda and pt.dtype == ct.dtype == torch.int64 and tuple(pt.shape) == (K, nc, 10) and tuple(ct.shape) == (K, nc)
    want = I.instance_parts(r[0].cpu().numpy()[None], components[None], K, nc)
    return ok and np.array_equal(pt.cpu().numpy(), want[0][0]) and np.array_equal(ct.cpu().numpy(), want[1][0])


@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_grouped_instances_equal_the_numpy_chain_on_the_grouped_labels(protocol):
    c = T._case(protocol)
    groups = _groups(protocol)
    table = I.group_table(groups, c["nc"])
    merged = 0
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, tracks=True, masks="frame", mask_runs=2048,
              confidence="frame", confidence_low=LOW)
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], instance_groups=groups, **kw)
        plain = video.VideoSegmenter(c["m"], **kw)
        for s in c["seqs"]:
            got, was = seg.segment_sequence(s["fr"]), plain.segment_sequence(s["fr"])
            grouped = table[s["labels"].numpy()]
            comp, rows, total = I.label_components(grouped, c["nc"], 8, c["skip"], K)
            ids = T._host_tracks(grouped, c)[0]
            runs, count = rle.encode(comp.astype(np.int32), 2048)
            for f, (r, p) in enumerate(zip(got, was)):
                assert len(r) == len(p) == 10
                # the labels, the per-class moments, the confidence map and the class sums are those without the keyword
                assert all(torch.equal(r[k], p[k]) for k in (0, 1, 7, 8)) and torch.equal(r[0].cpu(), s["labels"][f]), f
                assert np.array_equal(r[2].cpu().numpy(), rows[f]) and int(r[3]) == int(total[f]), f
                assert np.array_equal(r[4].cpu().numpy(), ids[f]), f
                assert np.array_equal(r[5].cpu().numpy(), runs[f]) and int(r[6]) == int(count[f]), f
                assert np.array_equal(r[9].cpu().numpy(), CF.confidence_sums(comp[f:f + 1].astype(np.int32), r[7].cpu().numpy()[None], K, LOW)[0]), f
                assert set(rows[f, :min(int(total[f]), K), 0].tolist()) <= set(range(c["nc"])) - {k for g in groups for k in g[1:]}
                merged += int(p[3]) - int(total[f])
    assert merged > 0, "no frame has two grouped classes side by side: the grouping tests little"
    assert seg.instance_groups == groups and plain.instance_groups is None


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("protocol", ["endovis18", "cadis"])
def test_segmenter_frame_parts_agree_across_modes(protocol, grouped):
    c = T._case(protocol)
    s = c["seqs"][0]
    extra = dict(instance_groups=_groups(protocol)) if grouped else {}
    table = I.group_table(extra.get("instance_groups", ()), c["nc"])
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, report="frame", instances=K, **extra)
    with torch.no_grad():
        was = video.VideoSegmenter(c["m"], **kw).segment_sequence(s["fr"])
        runs = {}
        for mode, mkw in _MODES.items():
            seg = video.VideoSegmenter(c["m"], parts="frame", **kw, **mkw)
            runs[mode] = seg.segment_sequence(s["fr"])
            assert mode != "graph" or seg.captured
    comp = I.label_components(table[s["labels"].numpy()], c["nc"], 8, c["skip"], K)[0]
    touching = 0
    for f in range(N):
        e = runs["eager"][f]
        assert len(e) == 6 and all(torch.equal(a, b) for a, b in zip(e[:4], was[f])), f       # what was there is what it was
        assert _own_parts(e, c["nc"], comp[f]), f
        for mode in ("batch2", "graph"):
            assert len(runs[mode][f]) == 6 and all(torch.equal(a, b) for a, b in zip(e, runs[mode][f])), (mode, f)
        assert np.array_equal(e[4][..., :6].sum(dim=1).cpu().numpy(), e[2][:, 2:8].cpu().numpy()), f      # the parts make up the rows
        touching += int(e[5].sum())
        if grouped:
            assert int((e[4][..., 0] > 0).sum(dim=1).max()) >= 1
    assert touching > 0


def test_segmenter_parts_with_ground_truth_are_made_after_the_replay():
    c = T._case("endovis18")
    s = c["seqs"][0]
    groups = _groups("endovis18")
    table = I.group_table(groups, c["nc"])
    kw = dict(out="labels", out_size=SIZE, report="frame", instances=K, tracks=True, instance_groups=groups, parts="frame")
    with torch.no_grad():
        seg = video.VideoSegmenter(c["m"], graph=True, **kw)
        free = seg.segment_sequence(s["fr"])
        assert seg.captured
        scored = seg.segment_sequence(s["fr"], gt=s["gt"])
        eager = video.VideoSegmenter(c["m"], scores="deferred", batch=2, **kw).segment_sequence(s["fr"], gt=s["gt"])
    comp = I.label_components(table[s["labels"].numpy()], c["nc"], 8, c["skip"], K)[0]
    for f in range(N):
        a, b, d = free[f], scored[f], eager[f]
        assert len(a) == 7 and len(b) == 9 and len(d) == 7, f                # (labels, dice, iou, moments, rows, total, ids, parts, contacts)
        assert torch.equal(b[0].cpu(), s["labels"][f]) and _own_parts(b, c["nc"], comp[f]), f
        assert torch.equal(a[-2], b[-2]) and torch.equal(a[-1], b[-1]) and torch.equal(a[-3], b[-3]), f
        assert all(torch.equal(x, y) for x, y in zip(a, d)), f


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_segmenter_deferred_parts_join_the_tracks(mode):
    protocol = "endovis18"
    c = T._case(protocol)
    a, b = c["seqs"]
    groups = _groups(protocol)
    names = [f"class {k}" for k in range(c["nc"])]
    kw = dict(out="labels", out_size=SIZE, protocol=protocol, instances=K, tracks=True, instance_groups=groups)
    with torch.no_grad():
        frame = video.VideoSegmenter(c["m"], report="frame", parts="frame", **kw)
        want = [frame.segment_sequence(q["fr"]) for q in (a, b)]
        seg = video.VideoSegmenter(c["m"], report="deferred", parts="deferred", **kw, **_MODES[mode])
        assert len(seg.parts_report()) == 0
        early = []
        for f in range(N):                                                   # pushed frame by frame: some are released before their
            for g, r in seg.push(a["fr"][f]):                                # predecessors and wait, parked, for the tracker
                assert isinstance(r, torch.Tensor)                           # the results are unchanged
                early += [g] if seg.chain.parked else []
        seg.finish()
        seg.reset()
        assert len(early) >= 1
        got_b = seg.segment_sequence(b["fr"])
    assert all(torch.equal(r.cpu(), b["labels"][f]) for f, r in enumerate(got_b))
    rep = seg.parts_report(names=names)
    inst, trk = seg.instance_report(names), seg.track_report(names)
    assert rep.sequences == inst.sequences == [0] * N + [1] * N and rep.frames == inst.frames == list(range(N)) * 2
    assert rep.names == names and rep.size == SIZE
    for n, res in enumerate(want):
        for f, r in enumerate(res):
            row = n * N + f
            assert np.array_equal(rep.moments[row], r[-2].cpu().numpy()) and np.array_equal(rep.contacts[row], r[-1].cpu().numpy()), (n, f)
            assert np.array_equal(rep.instances.rows[row], r[2].cpu().numpy()) and np.array_equal(rep.tracks.ids[row], r[4].cpu().numpy()), (n, f)
    assert np.array_equal(rep.instances.rows, inst.rows) and np.array_equal(rep.tracks.ids, trk.ids)
    rows = rep.as_rows()
    assert len(rows) == int(inst.present.sum()) and [r["track"] for r in rows] == [r["track"] for r in trk.as_rows()]
    assert all(sum(p["area"] for p in r["parts"].values()) == w["area"] for r, w in zip(rows, inst.as_rows()))
    assert any(len(r["parts"]) >= 2 for r in rows), "no instrument is made of two classes: the parts test little"
    two = next(r for r in rows if len(r["parts"]) >= 2)
    x, y = sorted(two["parts"])[:2]
    r0 = [k for k in range(2 * N) if (rep.sequences[k], rep.frames[k]) == (two["sequence"], two["frame"])][0]
    d = rep.direction(r0, two["instance"], x, y)
    assert np.isnan(d).all() or abs(float(np.hypot(*d)) - 1.0) < 1e-12
    seg.reset_metrics()
    assert len(seg.parts_report()) == 0 and len(seg.instance_report()) == 0


def test_segmenter_parts_and_groups_refusals():
    m = C._case("endovis18")["m"]
    base = dict(out="labels", report="frame")
    for kwargs, what in ((dict(parts="frame", **base), "parts"), (dict(parts="deferred", **base), "parts"),
                         (dict(instance_groups=((1, 2),), **base), "instance_groups"),
                         (dict(out="logits", parts="frame"), "parts"), (dict(out="logits", parts="frame", report="frame", instances=4), "parts"),
                         (dict(parts="always", instances=4, **base), "parts"), (dict(parts=True, instances=4, **base), "parts"),
                         (dict(instance_groups=((1,),), instances=4, **base), "instance_groups"),
                         (dict(instance_groups=((1, 1),), instances=4, **base), "instance_groups"),
                         (dict(instance_groups=((1, 2), (2, 3)), instances=4, **base), "instance_groups"),
                         (dict(instance_groups=((1, 12),), instances=4, **base), "instance_groups"),
                         (dict(instance_groups=((0, 1),), instances=4, **base), "instance_groups"),
                         (dict(instance_groups=((1, 2),), instances=4, instance_skip=(0, 2), **base), "instance_groups"),
                         (dict(instance_groups=5, instances=4, **base), "instance_groups")):
        with pytest.raises(StswinHipError, match=what):
            video.VideoSegmenter(m, **kwargs)
    for kwargs in (dict(instances=4, **base), dict(instances=4, parts="frame", **base)):
        with pytest.raises(StswinHipError, match="parts_report"):
            video.VideoSegmenter(m, **kwargs).parts_report()
    seg = video.VideoSegmenter(m, out="overlay", report="deferred", instances=4, parts="deferred", instance_groups=[[3, 1, 2]])
    assert seg.parts == "deferred" and seg.instance_groups == ((3, 1, 2),) and seg.chain.group_table[3].item() == 1
