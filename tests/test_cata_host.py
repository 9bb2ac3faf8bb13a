"""Host side of the CaDIS evaluation (segcata/cata_test.py:115-170, no GPU): the cata_metrics drop-in against the reference's own
results (tests/golden/cata_metrics.npz), the CaDIS clip rule, release schedule and ring plan, the per-channel value table, the
import aliases and model, and the segcata loader names."""
import random

import numpy as np
import pytest
import torch

import cata_ref_inputs as ci
import golden_util as gu
from stswincl_amd import video
from stswincl_amd.hip import StswinHipError
from stswincl_amd.utils import LoadModel as L
from stswincl_amd.utils import cata_metrics as M


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("ncm", ci.CLASS_COUNTS)
def test_cata_metrics_equal_the_reference(ncm):
    g = gu.load("cata_metrics.npz")
    pairs = ci.mask_pairs(ncm, int(g[f"{ncm}/seed"]))
    gts, preds = [a for a, _ in pairs], [b for _, b in pairs]
    acc = M.ConfusionMatrix(ncm)
    for a, b in pairs:
        acc.update_confusion_matrix(a, b)
    cm = acc.get_confusion_matrix()
    assert cm.dtype == np.float64 and np.array_equal(cm, g[f"{ncm}/cm"])
    pa, pac, pac_c, miou, miou_c = M.segmentation_metrics(gts, preds, num_classes=ncm)
    for name, v in (("pa", pa), ("pac", pac), ("pac_c", pac_c), ("miou", miou), ("miou_c", miou_c)):
        _same(v, g[f"{ncm}/{name}"])
    _same(M.iou_per_class_metrics(gts, preds, num_classes=ncm), g[f"{ncm}/iou_per_class"])
    assert np.isnan(g[f"{ncm}/miou_c"]).sum() == 2                  # the fixture covers absent classes
    _same(M.pixel_accuracy(cm), pa)
    _same(M.pixel_accuracy_class(cm)[1], pac_c)
    _same(M.mean_intersection_over_union(cm)[1], miou_c)
    _same(M.per_class_intersection_over_union(cm), miou_c)
    acc.reset()
    assert not acc.get_confusion_matrix().any()


def _reference_clip(frame, t=4):
    """segcata/dataset/CATA_new_512.py:155-158 (step 1)."""
    if frame > t:
        return list(range(frame - (t - 1), frame + 1))
    return list(range(frame + (t - 1), frame - 1, -1))


def test_cadis_clip_rule_and_release_schedule():
    for f in range(41):
        assert list(video.clip_frames(f, rule="cadis")) == _reference_clip(f), f
    p = video.ClipPlanner(batch=1, rule="cadis")
    released = {f: [g for st in p.push(1) for g in st.clips] for f in range(40)}
    assert [g for st in p.finish() for g in st.clips] == []
    expect = {0: [], 1: [], 2: [], 3: [0], 4: [1], 5: [2, 5], 6: [3, 6], 7: [4, 7]}
    for f in range(40):
        assert released[f] == expect.get(f, [f]), f
        for g in released[f]:
            assert max(_reference_clip(g)) == f
    assert sorted(g for v in released.values() for g in v) == list(range(40))


def test_endovis_schedule_is_unchanged():
    assert video.ClipPlanner(batch=1).rule == "endovis18"
    for f in range(30):
        assert video.ready_at(f) == video.ready_at(f, "endovis18")
        assert video.clip_frames(f) == video.clip_frames(f, rule="endovis18")
    assert [video.ready_at(f) for f in range(9)] == [[], [], [], [0], [1, 4], [2, 5], [3, 6], [7], [8]]
    assert video.min_frames() == 7 and video.min_frames("cadis") == 8


def _simulate(n, batch, chunks):
    p = video.ClipPlanner(batch=batch, rule="cadis")
    ring = [None] * p.slots
    done, processed = [], set()
    for st in [st for c in chunks for st in p.push(c)] + p.finish():
        assert not processed & set(st.new)
        processed |= set(st.new)
        read = set()
        for g, src in zip(st.clips, st.sources):
            got = []
            for e in src:
                if e >= 0:
                    read.add(e)
                    got.append(ring[e])
                else:
                    got.append(st.new[-1 - e])
            assert got == _reference_clip(g), (g, got, st)
        stored = [s for s in st.stores if s >= 0]
        assert len(stored) == len(set(stored)) and not read & set(stored)
        for fr, s in zip(st.new, st.stores):
            if s >= 0:
                ring[s] = fr
        done += st.clips
    assert processed == set(range(n))
    return done


@pytest.mark.parametrize("batch", [1, 2, 3, 4, 5, 6])
def test_cadis_ring_never_overwrites_a_slot_still_needed(batch):
    rnd = random.Random(77 + batch)
    for _ in range(60):
        n = rnd.randint(8, 70)
        chunks, left = [], n
        while left:
            c = min(left, rnd.choice([1, 1, 1, 2, 3, 5, 16]))
            chunks.append(c)
            left -= c
        assert sorted(_simulate(n, batch, chunks)) == list(range(n))


def test_cadis_refuses_a_seven_frame_sequence():
    p = video.ClipPlanner(batch=1, rule="cadis")
    p.push(7)
    with pytest.raises(StswinHipError, match="too short.*>= 8 frames"):
        p.finish()
    p.reset()
    p.push(8)
    assert [g for st in p.finish() for g in st.clips] == []
    with pytest.raises(StswinHipError):
        video.ClipPlanner(rule="cata")


def test_cadis_value_table_is_the_references_transform():
    mean = np.array([0.40789654, 0.44719302, 0.47026115], dtype=np.float32)
    std = np.array([0.28863828, 0.27408164, 0.27809835], dtype=np.float32)
    u = np.arange(256)
    want = np.stack([((u / 255.) - np.float64(mean[c])) / np.float64(std[c]) for c in range(3)]).astype(np.float32)
    got = video.cadis_value_table()
    assert got.dtype == np.float32 and got.shape == (3, 256)
    assert np.array_equal(got, want)
    # the reference's own expression on an image (CATA_new_512.py:228-229, then .float())
    img = np.broadcast_to(u.astype(np.uint8)[:, None], (256, 3))
    ref = ((img / 255.) - mean[None, :]) / std[None, :]
    assert np.array_equal(torch.from_numpy(ref).float().numpy().T, want)


def test_compat_aliases_and_the_cadis_model():
    import sys
    from stswincl_amd import compat
    from stswincl_amd.net.Ours import ASPP, base18, swin_512
    from stswincl_amd.net.Ours import base_cata_np
    compat.install()
    assert sys.modules["utils.cata_metrics"] is M
    assert sys.modules["net.Ours.base_cata_np"] is base_cata_np
    assert sys.modules["net.Ours.swin_tem_cata"] is swin_512
    assert sys.modules["net.Ours.ASPP_swin"] is ASPP
    m = base_cata_np.TswinPlusv5(9)
    assert tuple(m.swin.input_resolution) == (64, 80)
    assert list(m.state_dict().keys()) == list(base18.TswinPlus(9).state_dict().keys())
    from stswincl_amd.contrast.models.Ours import base as cl_base
    assert tuple(cl_base.TswinPlusv5(9).swin.input_resolution) == (32, 56)


def test_segcata_loader_names_match_the_reference(tmp_path):
    """tests/golden/cata_metrics.npz holds what segcata/utils/LoadModel.py's load_model_test did to golden_util.toy_seg_model() per
    file layout, and for load_model_cata (which returns None and loads nothing) the keys of the state-dict it built."""
    g = gu.load("cata_metrics.npz")
    files = {}
    for case, obj in gu.toy_checkpoints(gu.toy_seg_model()).items():
        files[case] = str(tmp_path / (case + ".pth"))
        torch.save(obj, files[case])
    for case, path in files.items():
        for fn in ("load_model_test", "load_model_cata"):
            tag = f"{fn}/{case}"
            m = gu.toy_seg_model()
            before = {k: v.clone() for k, v in m.state_dict().items()}
            assert getattr(L, fn)(m, path, log=False) is m
            after = m.state_dict()
            changed = [k for k in after if not torch.equal(after[k], before[k])]
            if fn == "load_model_test":
                assert changed == [k for k in g[tag + "/changed"].tolist() if k], tag
                assert float(sum(v.double().sum() for v in after.values())) == pytest.approx(float(g[tag + "/checksum"]), rel=1e-12)
            else:
                built = set(g[tag + "/built"].tolist())
                assert not bool(g[tag + "/returns_model"])
                # the merge of the reference's dict: every model key it holds, except the one the toy files give another shape
                assert changed == [k for k in after if k in built and not k.endswith("attn_mask")], tag
