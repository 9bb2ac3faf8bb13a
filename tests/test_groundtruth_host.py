"""Host side of "ground truth as stored" (CPU): stswincl_amd/utils/groundtruth.py against the recorded remaps and pictures of the
reference's three CaDIS experiments (tests/golden/overlay_colormap.npz), and utils.EndoMetric.EndoScores against a literal val_map
loop over general_dice / general_jaccard."""
import ctypes
import os

import numpy as np
import pytest

from stswincl_amd import hip
from stswincl_amd.utils import EndoMetric as EM
from stswincl_amd.utils import groundtruth as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay_colormap.npz")
CLASSES = {1: 9, 2: 18, 3: 26}          # class_num of the three experiments: the last class is the moved ignore value


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _pairs(golden, k):
    """{raw: new} as the fixture recorded it (every raw id 0 .. 35 and 255 occurs in the mask)."""
    mask, remapped = golden["mask"], golden[f"exp{k}/remapped"]
    pairs = {}
    for raw, new in zip(mask.ravel().tolist(), remapped.ravel().tolist()):
        assert pairs.setdefault(raw, new) == new
    return pairs


@pytest.mark.parametrize("k", [1, 2, 3])
def test_remap_table_reproduces_the_recorded_remap(golden, k):
    mask, remapped = golden["mask"], golden[f"exp{k}/remapped"]
    pairs = _pairs(golden, k)
    table = G.remap_table(pairs)
    assert table.dtype == np.uint8 and table.shape == (256,)
    got = G.decode_ids(mask, table)
    assert got.dtype == np.uint8 and np.array_equal(got, remapped)
    # the same table from the {new: [raw, ...]} form of the reference's class_remapping dictionaries
    grouped = {}
    for raw, new in pairs.items():
        grouped.setdefault(new, []).append(raw)
    assert np.array_equal(G.remap_table(grouped), table)
    # ignore_to = class_num - 1 is `mask[mask == 255] = class_num - 1` after the remap
    last = CLASSES[k] - 1
    moved = G.decode_ids(mask, G.remap_table(pairs, ignore_to=last))
    want = remapped.copy()
    want[remapped == 255] = last
    assert (remapped == 255).any() and np.array_equal(moved, want) and moved.max() == last
    assert last == {1: 8, 2: 17, 3: 25}[k]


def test_remap_table_rules():
    t = G.remap_table({3: 1, 4: 2}, default=7)
    assert t[3] == 1 and t[4] == 2 and t[0] == 7 and t[254] == 7 and t[255] == 255
    assert G.remap_table({3: 1}, ignore_to=9)[255] == 9
    t = G.remap_table({0: [0, 1], 1: (2,), 255: [5, 6]}, ignore_to=2)
    assert t[:7].tolist() == [0, 0, 1, 0, 0, 2, 2] and t[255] == 2
    assert G.remap_table({255: 4})[255] == 4
    for bad in ({256: 1}, {1: 256}, {1: [2], 3: [2]}, {-1: 0}, {1: 1.5}):
        with pytest.raises(ValueError):
            G.remap_table(bad)
    with pytest.raises(ValueError):
        G.remap_table({1: 2}, ignore_to=300)
    with pytest.raises(ValueError):
        G.decode_ids(np.zeros((2, 2), np.int64), t)
    with pytest.raises(ValueError):
        G.decode_ids(np.zeros((2, 2), np.uint8), t[:10])


@pytest.mark.parametrize("k", [1, 2, 3])
def test_decode_colours_inverts_the_recorded_picture(golden, k):
    rgb, remapped = golden[f"exp{k}/rgb"], golden[f"exp{k}/remapped"]
    cmap = dict(zip(golden[f"exp{k}/keys"].tolist(), golden[f"exp{k}/colors"].tolist()))
    got, unmatched = G.decode_colours(rgb, G.colour_table(cmap))
    assert got.dtype == np.uint8 and got.shape == remapped.shape
    if k == 1:                              # that colormap has no 255 key: those pixels are black, which no row holds
        ignored = remapped == 255
        assert 255 not in cmap and int(ignored.sum()) == 99
        assert np.array_equal(got[~ignored], remapped[~ignored]) and not got[ignored].any() and unmatched == 99
    else:
        assert np.array_equal(got, remapped) and unmatched == 0
    # the batched form counts per frame
    both, counts = G.decode_colours(np.stack([rgb, rgb[::-1]]), G.colour_table(cmap))
    assert np.array_equal(both[0], got) and np.array_equal(both[1], got[::-1])
    assert counts.dtype == np.int64 and counts.tolist() == [unmatched, unmatched]


def test_colour_table_rules():
    t = G.colour_table([(0, 0, 0), (10, 20, 30), (0, 0, 255)])
    assert t.dtype == np.uint8 and t.tolist() == [[0, 0, 0, 0], [10, 20, 30, 1], [0, 0, 255, 2]]
    assert G.colour_table([(1, 2, 3), (4, 5, 6)], labels=[7, 255]).tolist() == [[1, 2, 3, 7], [4, 5, 6, 255]]
    assert G.colour_table({5: (1, 2, 3), 2: [4, 5, 6]}).tolist() == [[1, 2, 3, 5], [4, 5, 6, 2]]
    assert np.array_equal(G.colour_table(np.array([[1, 2, 3], [4, 5, 6]])), G.colour_table([(1, 2, 3), (4, 5, 6)]))
    # a duplicate colour takes the later row; a colour one off in one channel matches nothing; a fourth channel is not looked at
    dup = G.colour_table([(9, 9, 9), (1, 2, 3), (9, 9, 9)], labels=[4, 5, 6])
    img = np.array([[[9, 9, 9], [1, 2, 3], [9, 9, 8], [1, 2, 4]]], dtype=np.uint8)
    got, unmatched = G.decode_colours(img, dup)
    assert got.tolist() == [[6, 5, 0, 0]] and unmatched == 2
    rgba = np.concatenate([img, np.array([[[0], [77], [255], [3]]], dtype=np.uint8)], axis=2)
    got4, unmatched4 = G.decode_colours(rgba, dup)
    assert np.array_equal(got4, got) and unmatched4 == 2
    assert len(G.colour_table([(i, 0, 0) for i in range(256)])) == 256
    for bad in ([], [(i % 256, i // 256, 0) for i in range(257)], [(1, 2)], [(1, 2, 256)], [(1, 2, -1)], [(1.5, 2, 3)]):
        with pytest.raises(ValueError):
            G.colour_table(bad)
    with pytest.raises(ValueError):
        G.colour_table([(1, 2, 3)], labels=[1, 2])
    with pytest.raises(ValueError):
        G.colour_table([(1, 2, 3)], labels=[256])
    with pytest.raises(ValueError):
        G.colour_table({1: (1, 2, 3)}, labels=[1])
    for bad_img in (img.astype(np.int64), img[..., :2], img[0, 0]):
        with pytest.raises(ValueError):
            G.decode_colours(bad_img, dup)
    with pytest.raises(ValueError):
        G.decode_colours(img, dup[:, :3])


def _val_map(gts, preds, seq_of, classes):
    """The reference's val_map loop (seg18/test.py:140-203, per-class division of seg18/train_swin.py:230-232), restated over label
    maps: general_dice / general_jaccard per frame, float64 sums in frame order."""
    nseq = max(seq_of) + 1
    metrics, metrics_seq, count_seq = np.zeros((2,)), np.zeros((2, nseq)), np.zeros((nseq,))
    dice_each, iou_each, tool_each = np.zeros((classes,)), np.zeros((classes,)), np.zeros((classes,))
    count, dices, ious = 0, [], []
    for y, p, s in zip(gts, preds, seq_of):
        dice, iou = EM.general_dice(y, p), EM.general_jaccard(y, p)
        dices.append(dice)
        ious.append(iou)
        for i in range(len(dice)):
            dice_each[dice[i][0]] += dice[i][1]
            iou_each[dice[i][0]] += iou[i][1]
            tool_each[dice[i][0]] += 1
        frame_dice = np.mean([d[1] for d in dice])
        frame_iou = np.mean([j[1] for j in iou])
        metrics += (frame_dice, frame_iou)
        metrics_seq[0][s] += frame_dice
        metrics_seq[1][s] += frame_iou
        count_seq[s] += 1
        count += 1
    metrics /= count
    metrics_seq /= count_seq
    dice_each /= tool_each
    iou_each /= tool_each
    return dict(dices=dices, ious=ious, dice=metrics[0], iou=metrics[1], dice_seq=metrics_seq[0], iou_seq=metrics_seq[1],
                dice_each=dice_each, iou_each=iou_each, tool_each=tool_each, count=count)


def _counts(gts, preds, classes):
    """int32 [F][3][nc]: |gt|, |pred|, |gt & pred| per class, what hip.upsample_argmax returns with gt."""
    out = np.zeros((len(gts), 3, classes), dtype=np.int32)
    for f, (y, p) in enumerate(zip(gts, preds)):
        for c in range(classes):
            out[f, :, c] = ((y == c).sum(), (p == c).sum(), ((y == c) & (p == c)).sum())
    return out


def _random_maps(seed, empty_frame=None):
    """3 sequences x 5 frames of 24 x 40 maps, 12 classes, class 7 absent from every gt; frame `empty_frame`'s gt all background."""
    g = np.random.default_rng(seed)
    values = np.array([c for c in range(12) if c != 7])
    gts = values[g.integers(0, len(values), (15, 24, 40))]
    preds = np.where(g.random((15, 24, 40)) < 0.6, gts, g.integers(0, 12, (15, 24, 40)))
    gts[3][gts[3] == 4] = 0                 # a present-class set that differs between frames
    if empty_frame is not None:
        gts[empty_frame] = 0
    return gts, preds, [f // 5 for f in range(15)]


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.mark.filterwarnings("ignore:Mean of empty slice", "ignore:invalid value encountered")
@pytest.mark.parametrize("empty_frame", [None, 7])
def test_endo_scores_from_counts_is_val_map_exactly(empty_frame):
    gts, preds, seq_of = _random_maps(5, empty_frame)
    want = _val_map(gts, preds, seq_of, 12)
    got = EM.EndoScores.from_counts(_counts(gts, preds, 12), seq_of)
    assert got.dices == want["dices"] and got.ious == want["ious"]
    assert got.count == 15 and got.sequences == seq_of
    for name in ("dice", "iou", "dice_seq", "iou_seq", "dice_each", "iou_each", "tool_each"):
        assert _same(getattr(got, name), want[name]), name
    assert np.isnan(got.dice_each[7]) and np.isnan(got.dice_each[0]) and got.tool_each[7] == 0      # no frame has them: 0 / 0
    if empty_frame is None:
        assert got.empty_frames == [] and np.isfinite([got.dice, got.iou]).all() and np.isfinite(got.dice_seq).all()
        assert 0 < got.iou < got.dice < 1
    else:                                    # np.mean([]) of that frame: the totals and its sequence are NaN, the others are not
        assert got.empty_frames == [7] and got.dices[7] == [] and np.isnan(got.dice) and np.isnan(got.iou)
        assert np.isnan(got.dice_seq).tolist() == [False, True, False] and np.isnan(got.iou_seq).tolist() == [False, True, False]
    assert np.isfinite(np.delete(got.dice_each, [0, 7])).all()


def test_endo_scores_from_counts_forms_and_refusals():
    gts, preds, seq_of = _random_maps(6)
    counts = _counts(gts, preds, 12)
    a = EM.EndoScores.from_counts(counts)                       # one sequence by default
    assert a.sequences == [0] * 15 and a.dice_seq.shape == (1,) and a.dice_seq[0] == a.dice
    import torch
    b = EM.EndoScores.from_counts(torch.from_numpy(counts), seq_of)
    assert b.dices == EM.EndoScores.from_counts(counts, seq_of).dices and b.dice_seq.shape == (3,)
    none = EM.EndoScores.from_counts(np.zeros((0, 3, 12), np.int32))
    assert none.count == 0 and none.dices == [] and np.isnan(none.dice) and none.dice_seq.shape == (0,)
    for bad in (lambda: EM.EndoScores.from_counts(counts[:, :2]), lambda: EM.EndoScores.from_counts(counts, seq_of[:3]),
                lambda: EM.EndoScores.from_counts(counts, [-1] * 15)):
        with pytest.raises(ValueError):
            bad()


def test_header_declares_the_entry_point_and_the_library_exports_it():
    assert "stswin_gt_decode" in hip.declared_symbols()
    fn = hip.load().stswin_gt_decode                          # (raises when the library lacks a declared symbol)
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    assert callable(hip.gt_decode)
