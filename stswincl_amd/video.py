"""Video inference: segment whole sequences with TswinPlus, computing each frame's ResNet features once.

The reference evaluates a sequence with batch 1 and one 4-frame clip per labelled frame (seg18/test.py:147-175 over
seg18/dataset/Endovis2018_new.py:109-127): frames f-3 .. f, and f+3, f+2, f+1, f for f < 4 (the rule is `t > frame`).  Each
frame is resized with PIL BILINEAR on the host, divided by 255 and sent to the model as an fp32 clip, so every frame runs
through the ResNet feeder four times.  In eval mode BatchNorm uses its running statistics: a frame's ResNet features do not
depend on the clip around it.  VideoSegmenter therefore

  * ingests the new uint8 frames on the GPU (stswin_frame_ingest: Pillow's resampler, bit-exact, and the /255 table),
  * runs the ResNet on the new frames only and keeps their tokens in a device ring of frame-feature slots,
  * assembles the clips (B, 4, h*w, 512) from ring slots and new frames (stswin_clip_assemble, one launch that also stores the
    new frames' tokens into their slots) and runs Swin / ASPP / head on them (TswinPlus.forward_frame_tokens).

    from stswincl_amd.video import VideoSegmenter
    seg = VideoSegmenter(model.eval(), out="labels", out_size=(1024, 1280))
    for frame in decoder:                                  # uint8 [Hs][Ws][3] or [n][Hs][Ws][3], CPU or GPU
        for f, labels in seg.push(frame):                  # frames whose clip is complete, in release order
            ...
    for f, labels in seg.finish():                         # end of the sequence
        ...
    seg.reset()                                            # next sequence: frame indices restart at 0

Which clips are ready after each frame, which slots they read and which slots the new frames take is decided on the host by
ClipPlanner (pure Python).  With batch 1 a clip is released when its last frame arrives: frame 3 -> {0}, 4 -> {1, 4}, 5 -> {2, 5},
6 -> {3, 6}, f >= 7 -> {f}.  A sequence needs at least 7 frames (frame 3's clip reads frame 6).

protocol="cadis" evaluates as segcata/cata_test.py:115-170 does over segcata/dataset/CATA_new_512.py:155-158, 192-195, 228-237:
the clip rule is `f > t` (frames f+3 .. f for f <= 4: frame 3 -> {0}, 4 -> {1}, 5 -> {2, 5}, 6 -> {3, 6}, 7 -> {4, 7}, f >= 8 -> {f};
at least 8 frames), the input values are (u / 255. - MEAN[c]) / STD[c] per channel (a [3][256] table), the labels come from a
bilinear resize with align_corners=False to the original 540 x 960, and with gt the segmenter accumulates one confusion matrix
over every frame of every sequence (stswin_upsample_argmax_cm; reset_metrics() clears it, confusion_matrix() reads it).
"""
from __future__ import annotations

from collections import deque, namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .frames import (CADIS_MEAN, CADIS_SIZE, CADIS_STD, RULES, T, VALUE_TABLE, bilinear_coeffs, cadis_value_table,  # noqa: F401
                     PRECISION_BITS as _PRECISION_BITS, Pinned as _Pinned, check_rule as _check_rule, tables as _tables, value_lut as _lut)
from .hip import StswinHipError
from .video_report import DeviceLog, LabelCleaner, ReportChain, Yield

PIXEL_FORMATS = ("rgb", "nv12", "uyvy")
_FRAME_FORMS = {"rgb": "uint8 RGB [n][Hs][Ws][3]", "nv12": "uint8 NV12 [n][3 Hs / 2][Ws]", "uyvy": "uint8 UYVY [n][Hs][Ws][2]"}


def clip_frames(f: int, t: int = T, rule: str = "endovis18") -> Tuple[int, ...]:
    """The frames of frame f's clip in clip order: Endovis2018_new.py:119-124 (`t > f` reads forward), or under rule="cadis"
    CATA_new_512.py:155-158 (`f > t`: frame t = 4 reads forward too)."""
    forward = f <= t if rule == "cadis" else t > f
    if forward:
        return tuple(range(f + t - 1, f - 1, -1))
    return tuple(range(f - t + 1, f + 1))


def ready_at(f: int, rule: str = "endovis18") -> List[int]:
    """The clips whose last missing frame is frame f, in release order."""
    out = []
    last_forward = T if rule == "cadis" else T - 1     # the last clip that reads forward, f + 3 .. f
    if T - 1 <= f <= last_forward + T - 1:             # clip f - 3 reads f - 3 .. f
        out.append(f - (T - 1))
    if f > last_forward:
        out.append(f)
    return out


def min_frames(rule: str = "endovis18") -> int:
    """The shortest sequence the rule can segment (the last clip that reads forward reads frame min_frames - 1)."""
    return 2 * T if rule == "cadis" else 2 * T - 1


class Step:
    """One launch group: ResNet on `new` (frame indices), `clips` (frame indices) assembled from `sources` (per clip, T entries:
    ring slot >= 0 or new frame -1 - j) and the new frames stored into `stores` (slot per new frame, -1 = not kept)."""

    __slots__ = ("new", "stores", "clips", "sources")

    def __init__(self, new, stores, clips, sources):
        self.new, self.stores, self.clips, self.sources = new, stores, clips, sources

    def table(self) -> List[int]:
        """The int32 slot table of stswin_clip_assemble: B*4 sources, then the stores."""
        return [e for src in self.sources for e in src] + list(self.stores)

    def __repr__(self):
        return f"Step(new={self.new}, stores={self.stores}, clips={self.clips}, sources={self.sources})"


class ClipPlanner:
    """Host-side schedule of a VideoSegmenter: which clips are ready, which ring slots they read, which slots new frames take.

    Frames are counted from 0 per sequence.  Ready clips are run `batch` at a time (finish() runs the rest).  A frame stays in the
    ring while a clip that still has to run reads it: the clips of frames >= F (F = frames pushed) read frames >= F - 3, so the
    ring holds those and the frames of ready clips not yet run.  No step stores into a slot it reads."""

    def __init__(self, batch: int = 1, slots: Optional[int] = None, rule: str = "endovis18"):
        if batch < 1:
            raise StswinHipError(f"batch must be >= 1, got {batch}")
        _check_rule(rule)
        self.rule = rule
        self.batch = batch
        self.slots = slots if slots is not None else max(2 * T - 1, batch + T - 1)
        if self.slots < max(2 * T - 1, batch + T - 1):
            raise StswinHipError(f"a ring of {self.slots} slots is too small for batch {batch}: needs >= {max(2 * T - 1, batch + T - 1)}")
        self.reset()

    def reset(self) -> None:
        self.seen = 0
        self.unprocessed: List[int] = []
        self.slot_of = {}
        self.pending = deque()
        self.cursor = 0

    def push(self, n: int = 1) -> List[Step]:
        steps = []
        for _ in range(n):
            f = self.seen
            self.seen += 1
            self.unprocessed.append(f)
            self.pending.extend(ready_at(f, self.rule))
            while len(self.pending) >= self.batch:
                steps.append(self._step([self.pending.popleft() for _ in range(self.batch)]))
        return steps

    def finish(self) -> List[Step]:
        short = [g for g in range(min(T + 1, self.seen)) if max(clip_frames(g, rule=self.rule)) >= self.seen]
        if short:
            raise StswinHipError(f"a sequence of {self.seen} frames is too short: the clip of frame {short[0]} reads frames "
                                 f"{clip_frames(short[0], rule=self.rule)} (the reference's rule needs >= {min_frames(self.rule)} frames)")
        steps = []
        while self.pending:
            steps.append(self._step([self.pending.popleft() for _ in range(min(self.batch, len(self.pending)))]))
        return steps

    def _step(self, clips: List[int]) -> Step:
        new, self.unprocessed = self.unprocessed, []
        pos = {fr: j for j, fr in enumerate(new)}
        sources = []
        for g in clips:
            src = []
            for fr in clip_frames(g, rule=self.rule):
                if fr in pos:
                    src.append(-1 - pos[fr])
                elif fr in self.slot_of:
                    src.append(self.slot_of[fr])
                else:                                                   # (a planner bug, not a user error)
                    raise AssertionError(f"frame {fr} of clip {g} is neither new nor in the ring")
            sources.append(src)
        needed = {fr for g in self.pending for fr in clip_frames(g, rule=self.rule)}
        needed.update(range(max(0, self.seen - (T - 1)), self.seen))
        read = {e for src in sources for e in src if e >= 0}
        for fr in [fr for fr in self.slot_of if fr not in needed]:
            del self.slot_of[fr]
        taken = set(self.slot_of.values()) | read
        stores = []
        for fr in new:
            if fr not in needed:
                stores.append(-1)
                continue
            for k in range(self.slots):
                s = (self.cursor + k) % self.slots
                if s not in taken:
                    break
            else:
                raise AssertionError(f"frame-feature ring of {self.slots} slots is full")
            self.cursor = (s + 1) % self.slots
            taken.add(s)
            self.slot_of[fr] = s
            stores.append(s)
        return Step(new, stores, clips, sources)


# ----------------------------------------------------------------------------------------------- frame ingest
def ingest(frames: torch.Tensor, size: Tuple[int, int], out: Optional[torch.Tensor] = None, protocol: str = "endovis18") -> torch.Tensor:
    """uint8 RGB frames [n][Hs][Ws][3] on the GPU -> fp32 images [n][3][H][W] (the stem's input): PIL.Image.resize((W, H),
    Image.BILINEAR) bit for bit, then float32(u / 255.) (protocol="cadis": the per-plane cadis_value_table()).  One or two launches
    (horizontal pass into a uint8 intermediate when the width changes, vertical pass + conversion)."""
    H, W = size
    n, Hs, Ws, _ = frames.shape
    dev = frames.device
    if out is None:
        out = torch.empty(n, 3, H, W, dtype=torch.float32, device=dev)
    htab = _tables(Ws, W, dev) if Ws != W else None
    vtab = _tables(Hs, H, dev) if Hs != H else None
    tmp = torch.empty(n * Hs * W * 3, dtype=torch.uint8, device=dev) if Ws != W else None
    return hip.frame_ingest(frames, out, _lut(dev, protocol), htab, vtab, tmp)


# ----------------------------------------------------------------------------------------------- the segmenter
class VideoSegmenter:
    """Segment video sequences with an eval-mode TswinPlus, one result per frame, each frame's ResNet features computed once.

    seg = VideoSegmenter(model, batch=1, out="logits" | "labels" | "overlay", out_size=None, graph=False, report=None, instances=None,
                         tracks=False, masks=None, boundary=None, confidence=None, instance_groups=None, parts=None, clean_area=None,
                         clearance=None)

    push(frames, gt=None) takes uint8 RGB frames [n][Hs][Ws][3] (or one [Hs][Ws][3]; torch tensor on the model's GPU or the CPU, or
    a numpy array; NV12 or UYVY frames with pixel_format, below) and returns [(frame_index, result), ...] for the frames whose clip is now complete.  finish() runs what is
    left at the end of the sequence; reset() starts the next one (frame indices restart at 0).  segment_sequence(frames, gt=None)
    is reset + push + finish, results in frame order.  Frames are resized to the model's input size (H, W) = 8 x
    swin.input_resolution.

    result: out="logits": the fp32 (bf16 under autocast) logits (nc, H, W) that model(clip) gives for the frame's clip;
    out="labels": uint8 labels (out_size, default (H, W)) of the bilinear (align_corners=True) resize + argmax
    (hip.upsample_argmax).  With gt (int64 [n][*out_size], one per pushed frame) the result is (labels or logits, dice, iou) with the
    per-frame [[class, value], ...] lists of utils.EndoMetric.predict_and_score.

    batch = B > 1 runs ready clips B at a time (offline throughput; the last results come with finish()).  graph=True (batch 1)
    captures the steady-state step - ingest, ResNet on the new frame, clip assembly, Swin / ASPP / head, logits or labels - once
    after the warm-up frames and replays it for every later frame; the host only copies the frame (a CPU frame from pinned memory)
    and the slot table into the captured buffers.  As with torch.cuda.graphs, the result of the last replayed step of a push is a
    view of the graph's output buffer that the next push overwrites (clone what you keep); earlier replayed results of the same
    push are copies, and segment_sequence returns copies.

    protocol="cadis" (segcata/cata_test.py:115-170): the CaDIS clip rule and per-channel normalisation, labels of a bilinear
    resize with align_corners=False (pass align_corners=True for the training-time validation form, train_cata_swin.py:203) to
    out_size, default (540, 960).  With gt the result is the labels (or logits) alone, and every pixel of the frame is counted into a
    device int64 confusion matrix of metric_classes classes (default: the model's classes - 1, the last one being the remapped ignore
    label, CATA_new_512.py:237) that pools all frames of all sequences, as cata_test.py does: reset() keeps it, reset_metrics() clears
    it, confusion_matrix() returns it as float64 numpy (utils.cata_metrics.ConfusionMatrix.get_confusion_matrix()).

    out="overlay" (palette=None, alpha=128, transparent=None, edge_alpha=255): the result is uint8 [Hs][Ws][3], the pushed frame itself
    with the protocol's labels blended in (hip.labels_overlay: colour table utils.visualize.overlay_table(palette or
    default_palette(), alpha, transparent), outlines of edge_alpha where the label changes, None for none).  `transparent` labels show
    the frame unchanged: default (0,), the background, for endovis18 and (classes - 1,), the remapped ignore label, for cadis.  out_size
    is the frame size (another one raises at the first push).  With gt: (overlay, dice, iou) for endovis18, the overlay alone for cadis,
    counted as for out="labels".  The segmenter keeps the GPU uint8 copy of a frame from its ResNet pass until its own clip's result
    (frames f < 4 wait several steps; a frame pushed as a GPU tensor is referenced, not copied, as it is until its ResNet pass for
    every output form: leave it unchanged until its result has come back); under graph=True the captured step ends with the label
    and the overlay launch on the static frame buffer, and the result is a view of the graph's output buffer as above.

    gt_table (utils.groundtruth.colour_table or remap_table; both protocols): gt is then the ground truth as the files hold it, uint8
    [n][*out_size][3 | 4] colour-coded with a [k][4] table or uint8 [n][*out_size] raw ids with a [256] table, on the CPU or the GPU.
    The bytes are uploaded as they are and decoded to the int64 index map on the device (hip.gt_decode) when they are pushed; scoring
    then proceeds as with an int64 gt.  unmatched() is the pooled number of colour-coded pixels that no table row holds.

    pixel_format="nv12" | "uyvy" (yuv_standard="bt709" | "bt601", full_range=False, chroma="replicate" | "linear"): push takes the
    frames as a decoder or a capture card delivers them, uint8 [n][3 Hs / 2][Ws] (NV12: Hs luma rows, then Hs / 2 rows of (U, V) pairs)
    or uint8 [n][Hs][Ws][2] (UYVY: U, Y0, V, Y1 per pixel pair), one frame without [n], on the CPU or the GPU, Hs (NV12) and Ws even;
    frame_shape stays (Hs, Ws).  The raw bytes are uploaded as they are (1.5 or 2 bytes per pixel) and one launch (hip.yuv_to_rgb,
    defined to the bit by utils.yuv.yuv_to_rgb with utils.yuv.to_rgb_matrix(yuv_standard, full_range)) makes the RGB frame that
    everything downstream reads, so the results are those of pushing utils.yuv.yuv_to_rgb(frames) as RGB.  A raw frame pushed as a GPU
    tensor is read by that launch only: it is free again after its ResNet pass, for out="overlay" too (the segmenter keeps the RGB
    frame it made).  Under graph=True the static input buffer holds the raw frame and the captured step begins with the conversion.
    out_format="nv12" (out="overlay" only; any pixel_format; an odd frame size raises at the first push): the result is the overlay as
    NV12, uint8 [3 Hs / 2][Ws] = utils.yuv.rgb_to_nv12 of the RGB overlay with utils.yuv.to_yuv_matrix(yuv_standard, full_range), made
    by one more launch (hip.rgb_to_nv12), the last captured one under graph=True.

    scores="deferred" (endovis18): a scored frame's counts go into a device log instead of to the host - no download and no
    synchronisation per frame - and push returns the labels (logits, overlay) alone, as cadis does; under graph=True the counting
    launch runs after the replayed step.  endo_scores() downloads the log once and returns utils.EndoMetric.EndoScores: the per-frame
    lists that scores="frame" (the default) returns, and the reference's val_map aggregates, per sequence too: a sequence's ordinal
    is the number of earlier sequences that scored a frame since reset_metrics(), which clears the log.

    report="frame" | "deferred" (out="labels" | "overlay", both protocols; min_area=1): wherever a step's label map is made - the scoring
    launches with ground truth included - one more launch (hip.label_moments, before the overlay launch: it reads the labels) takes
    each frame's per-class moments, int64 [nc][10] with nc the model's classes: count, sum x, sum y, sum x^2, sum xy, sum y^2 and the
    extent (utils.instruments states the row).  report="frame": a result r becomes (r, moments), a tuple r + (moments,), the moments on
    the device - no download and no synchronisation (utils.instruments.InstrumentReport.from_moments(moments.cpu(), out_size) reads
    them).  Under graph=True the captured step holds the clearing of the moments buffer (a fill kernel) and the moments launch behind
    the label launch, and the moments of the last replayed step of a push are a view of that buffer, as the labels are; with ground
    truth the labels, and so the moments, are made after the replay.  report="deferred": results are unchanged and the rows go into a
    device log (copied from the graph's buffer after a replay); instrument_report() downloads the log once and returns the
    InstrumentReport - presence, area, box, centroid, principal axis per frame and class, classes below min_area pixels absent - over
    every frame released since reset_metrics(), rows ordered by sequence and frame, a sequence's ordinal being the number of earlier
    sequences that released a frame.  Class names are the caller's (instrument_report(names=...)).

    instances=K (1 .. 1024; needs report; connectivity=8 | 4, instance_skip=None): the report split into connected instances, for
    frames that hold two shafts or two claspers.  Wherever the moments launch runs - the scoring paths with ground truth included -
    the launches of hip.label_components follow it on the same label map: the components of every class not in instance_skip
    (default: what `transparent` defaults to, (0,) for endovis18 and (classes - 1,) for cadis), numbered per frame by their first pixel
    in raster order, the first K with a row int64 [12] = class, first pixel y W + x and the ten integers of the moments row
    (utils.instruments.label_components defines them; K truncates deterministically and `total` still counts every component).
    report="frame": a result r becomes r + (moments, rows, total), rows int64 [K][12] and total an int32 scalar tensor, both on the
    device - no download and no synchronisation.  Under graph=True the captured step holds the launches behind the moments launch;
    the component map and the workspace are the segmenter's own, allocated by the eager warm-up frames, and rows and total of the
    last replayed step of a push are views of the graph's buffers, as the moments are; with ground truth they are made after the
    replay, as the labels are.  report="deferred": rows and totals go into a device log that grows as the moments log does;
    instance_report(names=None) downloads it once and returns utils.instruments.InstanceReport over every frame released since
    reset_metrics(), with instrument_report()'s order, sequence ordinals and reset() / reset_metrics() behaviour.  instances=None:
    every result, launch and captured graph is what it is without the keyword.

    tracks=True (needs instances=K; track_iou=100 in thousandths, track_same_class=True; min_area is the segmenter's): the instances
    followed from frame to frame, so that a shaft keeps one id while its ordinal changes.  Behind the component launches of a frame run
    the two of hip.track_instances (utils.instruments.InstanceTracker defines the result): an instance takes the id of the instance of
    the previous frame it overlaps best, a new id otherwise; ids restart at 0 with every sequence (reset() resets the state with a fill
    kernel), and an instance that was absent for a frame comes back under a new id.  The tracker takes frames in frame order, which is
    not the order of release (endovis18 releases 0, 1, 4, 2, 5, 3, 6, ..., cadis 0, 1, 2, 5, 3, 6, 4, 7, ..., a batch in the planner's
    order): a released frame whose predecessor has not been tracked is parked - its component map copied into a pool that grows as
    needed, its rows and total kept - and tracked in the push that releases the predecessor.  report="frame": a result gains ids,
    int32 [K] on the device, as its last element (-1: no instance or below min_area).  For a parked frame - frames 4 and 5 of an
    endovis18 sequence, 5 and 6 of a cadis one, more with batch > 1 - the tensor is handed out at release holding -2 and is written
    on the stream when the frame is tracked, at the latest by finish(): no synchronisation, read it after that push.  Under graph=True
    the captured steady step holds the tracker's launches behind the component launches and ids is a view of the graph's buffer until
    the next push, as rows and total are; the state is allocated by the warm-up frames; with ground truth the tracker follows the
    eager component launches after the replay.  report="deferred": ids and the running number of tracks go into a device log beside
    the instance log (a parked frame's row when it is tracked); track_report(names=None) downloads once and returns
    utils.instruments.TrackReport over every frame released since reset_metrics(), in instance_report()'s order.  tracks=False:
    every result, launch and captured graph is what it is without the keyword.

    track_max_gap=g (tracks=True; an int >= 0, frames): with g >= 1 a track that no instance was matched to stays alive for up to g
    frames, and instances are matched against the mask each track had when it was last seen, kept per pixel on the device: a shaft
    that drops below min_area for a frame, or is hidden by smoke for two, comes back under its id.  The tracker's launches are then the
    three of the tracker with a memory (utils.instruments.MemoryTracker defines the result; hip.TrackState(..., max_gap=g)), under
    graph=True three in the captured steady step; frame order, parking, both report modes, masks, ground truth and batch > 1 are as
    above.  Deliberately, an instrument of the same class that moves onto a lost track's remembered place inherits its id, and there
    is still no motion model.  track_max_gap=0: every result, launch and captured graph is what it is without the keyword.

    masks="frame" | "deferred" (out="labels" | "overlay", both protocols; does not need report; mask_runs=16384): the masks themselves in
    the form their consumers read, run-length encoded in column-major order (COCO's `counts`, the rle field of MOTS files), so that
    storing what was segmented needs no download of a map per frame.  Behind the tracker's launches - or the component launches, or the
    moments launch, or the label launch, whatever the chain ends with - run the three of hip.rle_encode (utils.rle.encode defines the
    result) on the chain's int32 component map with instances=K, the only thing that tells two shafts apart, and on the uint8 label map
    otherwise, wherever a step's label map is made, the scoring paths with ground truth included: runs int32 [mask_runs][2] = (start p =
    x H + y, value) in ascending p, zero behind the last run, and count, an int32 scalar tensor that counts every run although only the
    first mask_runs are kept (a truncated frame shows as count > mask_runs).  mask_runs defaults to 16384, 128 KB per frame against
    the 1.3 MB (labels) or 5.2 MB (components) of a 1024 x 1280 map; the basis is an estimate, not a measurement of surgical video - a
    map of a handful of instruments crosses each of its W columns a few times, a few thousand runs - and tools/bench_masks.py
    records the largest count it sees.  The deferred log holds 8 mask_runs bytes per frame and grows by doubling from 64 rows, so its
    first row allocates 8 MB at the default and 512 MB at mask_runs = 1048576: choose mask_runs by the counts, not by the limit.  The
    log holds columns only for what is deferred (masks="deferred" beside report=None or "frame" logs runs and counts alone).  The encoder needs nothing from the tracker: a frame the tracker parks is encoded when its
    labels exist.  masks="frame": a result r becomes r + (runs, count) behind whatever report="frame" appends, both on the device - no
    download and no synchronisation.  Under graph=True the captured steady step holds the encoder's launches behind the tracker's;
    the workspace is the segmenter's own, allocated by the warm-up frames, and runs and count of the last replayed step of a push are
    views of the graph's buffers, as rows and total are; with ground truth they are made after the replay.  masks="deferred": results
    are unchanged and runs and counts go into the device log beside the report's (report and masks choose their modes independently;
    a row is logged when either is deferred); mask_report(names=None) downloads once and returns utils.rle.MaskReport over every frame
    released since reset_metrics(), in instrument_report()'s order and with its sequence ordinals - dense(r), objects(r) with each
    object's COCO RLE, mots_lines(sequence) - joined with instance_report() when instances and report="deferred" are set and with
    track_report() when tracks is.  masks=None: every result, launch and captured graph is what it is without the keyword.

    boundary="deferred" (out="labels" | "overlay", both protocols, every scores mode; boundary_bins=32, boundary_skip=None): the contours
    scored beside the regions.  For every frame pushed with gt - int64, or as stored with gt_table - the five launches of
    hip.boundary_counts (utils.boundary.boundary_counts defines the result) follow the launch that makes the frame's labels, on the same
    stream and in the segmenter's own workspace, about 2 H W (2 classes + 1) bytes, allocated once per frame size: per class and direction the
    size of the contour, the largest squared distance to the other map's contour and the contour pixels per whole-pixel distance up to
    boundary_bins - 2, exact integers.  The row goes into a device log beside the score log, with its sequence ordinals: no download
    and no synchronisation, and the results of push are unchanged.  Under graph=True scored labels are made after the replay, and so
    are the rows; the captured step is what it is without the keyword.  boundary_scores(names=None) downloads the log once and returns
    utils.boundary.BoundaryScores: nsd(tau), the normalised surface distance of ROBUST-MIS and "Metrics Reloaded" (MONAI's
    compute_surface_dice at whole-pixel tolerances), hausdorff(), hausdorff_percentile(q) and their aggregates, over the classes
    present in the ground truth and not in boundary_skip (default: what `transparent` defaults to, (0,) for endovis18 and (classes - 1,)
    for cadis; a ground-truth value that is no class of the model, such as an ignore label that was not remapped, belongs to no
    contour but still bounds its neighbours' contours).  reset() keeps the log, reset_metrics() clears it.  boundary=None: every
    result, launch and captured graph is what it is without the keyword.

    confidence="frame" | "deferred" (out="labels" | "overlay", both protocols, every scores mode, batch > 1 and graph=True; needs neither
    report nor masks; confidence_low=128): how sure the model was of the labels it gave - the softmax probability the reference has
    between its resize and its argmax and throws away (seg18/test.py:153-158), which the label launches skip.  Wherever a step's label
    map is made, the scoring paths with ground truth included, one launch (hip.upsample_confidence; utils.confidence states the
    result) reads the logits the labels came from once more and writes conf uint8 [*out_size] = min(255, floor(255 p + 0.5)), p the
    probability of the pixel's label; then hip.confidence_sums takes per class the number of pixels, the sum of conf and the number
    of pixels with conf < confidence_low (0 .. 256), int64 [nc][3], and with instances=K the same per instance ordinal over the chain's
    component map, int64 [K][3], behind the component launches and before the next clip's components overwrite the map (where the
    masks are encoded: nothing depends on the tracker, a parked frame is summed when its labels exist, and ordinals join with track ids
    by row on the host).  confidence="frame": a result r becomes r + (conf, class_sums[, instance_sums]) behind whatever report and
    masks append, all on the device - no download and no synchronisation.  Under graph=True the launches are part of the captured
    steady step and the three tensors of the last replayed step of a push are views of the graph's buffers, as the labels are; with
    ground truth they are made after the replay.  confidence="deferred": results are unchanged and the sums, not the map, go into the
    device log; confidence_report(names=None) downloads once and returns utils.confidence.ConfidenceReport - mean = sum / (255 count)
    and low_fraction per class, and per instance, NaN where absent - over every frame released since reset_metrics(), in
    instrument_report()'s order and with its sequence ordinals; mask_report() passes it to the MaskReport when masks is deferred too,
    and objects(r) then carry "score", the mean probability of the instance (of the class without instances).  confidence=None: every
    result, launch and captured graph is what it is without the keyword.

    instance_groups=((1, 2, 3), ...) (needs instances=K): the classes that are parts of one instrument - EndoVis18's shaft, wrist and
    clasper, CaDIS's finer label sets; the ids are the caller's own - so that instances=K reports whole instruments.  A sequence of
    groups, each at least two distinct classes 0 .. classes - 1, the groups disjoint, none of their classes in instance_skip.  A
    group's representative is its smallest class.  One launch in front of the component launches (hip.gt_decode, id-coded, with the
    persistent table utils.instruments.group_table(groups, classes)) writes the grouped labels into a buffer of the chain's own, and
    the components, rows and total of a frame are exactly utils.instruments.label_components(group_table[labels], ...): the class
    column of a row holds the representative, which the caller's names call "instrument".  The tracker (track_same_class compares
    representatives), the masks and the per-instance confidence sums read the component map and follow by construction; the
    per-class moments of report= stay on the ungrouped labels.  instance_groups=None: every result, launch and captured graph is
    what it is without the keyword.

    parts="frame" | "deferred" (needs instances=K; with or without instance_groups; both protocols, every scores mode, batch > 1 and
    graph=True): what each instance is made of and what it touches.  Wherever the component launches run, the scoring paths with
    ground truth included, hip.instance_parts (utils.instruments.instance_parts states the result) takes over the labels (ungrouped)
    and the chain's component map, per instance ordinal i < K and class c, parts int64 [K][nc][10], the ten integers of the moments
    over the pixels of instance i with label c, and contacts int64 [K][nc], the pixel edges between instance i and pixels of class c
    outside it (needle in clasper, instrument on kidney; borders between an instance's own parts are not counted) - behind the
    component launches and before the next clip's components overwrite the map, where the masks are encoded: nothing depends on the
    tracker, a parked frame is summed when its labels exist.  parts="frame": a result r becomes r + (parts, contacts) behind whatever
    report, masks and confidence append, on the device.  Under graph=True the launch is part of the captured steady step and the two
    tensors of the last replayed step of a push are views of the graph's buffers; with ground truth they are made after the replay.
    parts="deferred": results are unchanged and both tensors go into the device log; parts_report(names=None) downloads once and
    returns utils.instruments.PartsReport - per instance the area, box, centroid and principal axis of every class it holds,
    touches(r, i) class -> edges, direction(r, i, a, b) the unit vector from part a's centroid to part b's (shaft -> clasper: the
    heading) - over every frame released since reset_metrics(), in instrument_report()'s order and with its sequence ordinals,
    joined by row with instance_report() under report="deferred" and with track_report() under tracks=True.  parts=None: every
    result, launch and captured graph is what it is without the keyword.

    clearance="frame" | "deferred" (needs instances=K; with or without instance_groups; both protocols, every scores mode, batch > 1,
    graph=True and clean_area, whose cleaned map it then reads; clearance_to=None, clearance_max=None): how near each instance comes to
    what it does not touch - clasper to small intestine, needle driver to kidney, an instrument to the pupil - where contacts of
    parts= says nothing until the two regions meet.  Wherever hip.instance_parts would run - behind the component launches and before
    the next clip's components overwrite the map, the scoring paths with ground truth included; nothing depends on the tracker - the
    six launches of hip.instance_clearance (utils.instruments.instance_clearance states the result) take over the labels (ungrouped)
    and the chain's component map, per instance ordinal i < K and class c, clearance int64 [K][nc][3] = (d2, p, q): the exact squared
    Euclidean distance in pixels between the instance and the nearest pixel of the class, and the raster indices y W + x of the two
    pixels that realise it, the first in raster order; (-1, -1, -1) where the instance or the class is absent, the class is not in
    clearance_to (a sequence of classes; default all), the distance exceeds clearance_max pixels, or the instance holds a pixel of the
    class itself: own classes - with instance_groups an arm's shaft, wrist and clasper - are not measured, so neither is the distance
    between two instruments of one class.  clearance="frame": a result r becomes r + (clearance,) behind whatever report, masks,
    confidence and parts append, on the device.  Under graph=True the launches are part of the captured steady step, the workspace is
    the segmenter's own, allocated by the warm-up frames (it only grows, retired ones are kept), and the tensor of the last replayed
    step of a push is a view of the graph's buffer; with ground truth it is made after the replay.  clearance="deferred": results are
    unchanged and the tensor goes into the device log; clearance_report(names=None) downloads once and returns
    utils.instruments.ClearanceReport - distance(r, i) class -> pixels, nearest(r, i, c) the two pixels as ((y, x), (y, x)) - over
    every frame released since reset_metrics(), in instrument_report()'s order and with its sequence ordinals, joined by row with
    instance_report() under report="deferred" and with track_report() under tracks=True.  clearance=None: every result, launch and
    captured graph is what it is without the keyword; clearance_to or clearance_max without it is refused.

    clean_area=A (2 .. 2^30 pixels; out="labels" | "overlay", both protocols, every scores mode, batch > 1 and graph=True; a model of 1 ..
    64 classes; clean_keep=None, clean_connectivity=8 | 4, clean_max=4096): the label map cleaned before anything reads it - specks out,
    small holes filled.  Wherever a step's label map is made, the launches of hip.labels_clean (utils.instruments.clean_labels states
    the result) follow the label launch and precede everything else: a connected component of any class with fewer than A pixels,
    unless its class is in clean_keep (the classes that are thin by nature - thread, needle; the ids are the caller's), takes the class
    that most of its pixel edges towards stable pixels lead to; a speck among specks stays, and of a frame's small components the first
    clean_max in raster order can change.  With the keyword the labels are the cleaned labels everywhere: the returned labels or
    overlay, the moments, grouped labels, components, tracks, masks, parts and contacts come from the cleaned map (the tracker's parking
    is as it was: the cleaning sits in front of the chain), and confidence is the probability of the cleaned label.  With ground truth
    the scores are those of the cleaned labels: the label launch runs without gt, then the cleaning, then one launch of
    hip.labels_score takes the counts scores="frame" builds its lists from, scores="deferred" logs and protocol="cadis" adds to the
    confusion matrix, and boundary="deferred" reads the cleaned labels.  Under graph=True the cleaning launches are part of the captured
    steady step; the workspace is the segmenter's own, allocated by the warm-up frames (it only grows, retired ones are kept), the
    cleaned map is a fresh tensor per eager step and the graph's buffer under replay, so the labels of the last replayed step of a push
    are a view of the graph's buffer, as they are without the keyword.  The cleaning's stats - the frame's small components, not
    bounded by clean_max, and the pixels whose label changed - go into a small device log, one row per released frame, copied out of
    the graph's buffer after a replay: no download and no synchronisation per frame.  clean_report() downloads it once and returns
    video_report.CleanReport over every frame released since reset_metrics(), in instrument_report()'s order and with its sequence
    ordinals.  clean_area=None: every result, launch and captured graph is what it is without the keyword.

    Runs under torch.no_grad().  Refuses (StswinHipError): a model in train mode, a model or frames not on the GPU, a frame size
    that differs from the earlier frames'."""

    def __init__(self, model, batch: int = 1, out: str = "logits", out_size: Optional[Sequence[int]] = None, graph: bool = False,
                 protocol: str = "endovis18", metric_classes: Optional[int] = None, align_corners: Optional[bool] = None,
                 palette=None, alpha: int = 128, transparent: Optional[Sequence[int]] = None, edge_alpha: Optional[int] = 255,
                 gt_table=None, scores: str = "frame", pixel_format: str = "rgb", yuv_standard: str = "bt709", full_range: bool = False,
                 chroma: str = "replicate", out_format: str = "rgb", report: Optional[str] = None, min_area: int = 1,
                 instances: Optional[int] = None, connectivity: int = 8, instance_skip: Optional[Sequence[int]] = None,
                 tracks: bool = False, track_iou: int = 100, track_same_class: bool = True, masks: Optional[str] = None,
                 mask_runs: int = 16384, track_max_gap: int = 0, boundary: Optional[str] = None, boundary_bins: int = 32,
                 boundary_skip: Optional[Sequence[int]] = None, confidence: Optional[str] = None, confidence_low: int = 128,
                 instance_groups=None, parts: Optional[str] = None, clean_area: Optional[int] = None, clean_keep: Optional[Sequence[int]] = None,
                 clean_connectivity: int = 8, clean_max: int = 4096, clearance: Optional[str] = None,
                 clearance_to: Optional[Sequence[int]] = None, clearance_max: Optional[int] = None):
        if out not in ("logits", "labels", "overlay"):
            raise StswinHipError(f"out must be 'logits', 'labels' or 'overlay', got {out!r}")
        if pixel_format not in PIXEL_FORMATS:
            raise StswinHipError(f"pixel_format must be one of {PIXEL_FORMATS}, got {pixel_format!r}")
        if out_format not in ("rgb", "nv12"):
            raise StswinHipError(f"out_format must be 'rgb' or 'nv12', got {out_format!r}")
        if out_format == "nv12" and out != "overlay":
            raise StswinHipError("out_format='nv12' belongs to out='overlay'")
        if chroma not in ("replicate", "linear"):
            raise StswinHipError(f"chroma must be 'replicate' or 'linear', got {chroma!r}")
        if yuv_standard not in ("bt709", "bt601"):
            raise StswinHipError(f"yuv_standard must be 'bt709' or 'bt601', got {yuv_standard!r}")
        if out != "overlay" and (palette is not None or transparent is not None):
            raise StswinHipError("palette and transparent belong to out='overlay'")
        if graph and batch != 1:
            raise StswinHipError("graph replay runs the online step: batch must be 1")
        _check_rule(protocol)
        if protocol == "endovis18" and (align_corners is False or metric_classes is not None):
            raise StswinHipError("align_corners=False and metric_classes belong to protocol='cadis'")
        if scores not in ("frame", "deferred"):
            raise StswinHipError(f"scores must be 'frame' or 'deferred', got {scores!r}")
        if scores == "deferred" and protocol != "endovis18":
            raise StswinHipError("scores='deferred' belongs to protocol='endovis18' (protocol='cadis' pools its counts in confusion_matrix())")
        self.model = model
        self._check_train()
        if any(not p.is_cuda for p in model.parameters()):
            raise StswinHipError("VideoSegmenter needs the model on the GPU (model.cuda()); there is no CPU path")
        self.device = next(model.parameters()).device
        ir = tuple(model.swin.input_resolution)
        self.size = (8 * ir[0], 8 * ir[1])
        self.batch = batch
        self.out = out
        self.protocol = protocol
        self.cadis = protocol == "cadis"
        default_size = CADIS_SIZE if self.cadis else self.size
        if out == "overlay":
            default_size = None           # the frame size, known at the first push
        self.out_size = tuple(out_size) if out_size is not None else default_size
        self.align_corners = True if align_corners is None and not self.cadis else bool(align_corners)
        self.metric_classes = None
        if self.cadis:
            self.metric_classes = metric_classes if metric_classes is not None else model.classifier[-1].out_channels - 1
            if not 1 <= self.metric_classes <= 64:
                raise StswinHipError(f"metric_classes must be 1 .. 64, got {self.metric_classes}")
        self._cm = None
        self.scores = scores
        classes = model.classifier[-1].out_channels
        self._score_log = DeviceLog(self.device, {"counts": ((3, classes), torch.int32)})     # scores="deferred": a row per scored frame
        self.chain = ReportChain(self.device, classes, protocol, out, report, min_area, instances, connectivity, instance_skip, tracks,
                                 track_iou, track_same_class, masks, mask_runs, track_max_gap, confidence, confidence_low,
                                 self.align_corners, parts, instance_groups, clearance, clearance_to, clearance_max)
        self.clearance, self.clearance_to, self.clearance_max = clearance, self.chain.clearance_to, clearance_max
        self.confidence, self.confidence_low = confidence, confidence_low
        self.parts, self.instance_groups = parts, self.chain.instance_groups
        self.report, self.min_area, self.instances, self.connectivity, self.instance_skip = report, min_area, instances, connectivity, self.chain.instance_skip
        self.tracks, self.track_iou, self.track_same_class = tracks, track_iou, track_same_class
        self.track_max_gap = track_max_gap
        self.masks, self.mask_runs = masks, mask_runs
        if boundary not in (None, "deferred"):
            raise StswinHipError(f"boundary must be None or 'deferred', got {boundary!r}")
        if boundary is None and (boundary_bins != 32 or boundary_skip is not None):
            raise StswinHipError("boundary_bins and boundary_skip belong to boundary='deferred'")
        if boundary is not None and out == "logits":
            raise StswinHipError("boundary='deferred' measures the label map: out must be 'labels' or 'overlay'")
        if isinstance(boundary_bins, bool) or not isinstance(boundary_bins, int) or not 2 <= boundary_bins <= 256:
            raise StswinHipError(f"boundary_bins must be an int 2 .. 256, got {boundary_bins!r}")
        if boundary is not None and not 1 <= classes <= 64:
            raise StswinHipError(f"boundary: the model has {classes} classes, hip.boundary_counts takes 1 .. 64")
        if boundary is not None:
            if boundary_skip is None:         # the background, or the remapped ignore label: what `transparent` defaults to
                boundary_skip = (classes - 1,) if self.cadis else (0,)
            try:
                boundary_skip = tuple(boundary_skip)
            except TypeError:
                boundary_skip = (boundary_skip,)
            if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 63 for c in boundary_skip):
                raise StswinHipError(f"boundary_skip holds classes 0 .. 63, got {boundary_skip!r}")
        self.boundary, self.boundary_bins, self.boundary_skip = boundary, boundary_bins, boundary_skip
        self._classes = classes
        if clean_area is None and (clean_keep is not None or clean_connectivity != 8 or clean_max != 4096):
            raise StswinHipError("clean_keep, clean_connectivity and clean_max belong to clean_area=A")
        # clean_area: the launches of hip.labels_clean behind every label launch, its workspace and the log of its stats
        self.cleaner = None if clean_area is None else LabelCleaner(self.device, classes, out, clean_area, clean_keep, clean_connectivity, clean_max)
        self.clean_area, self.clean_connectivity, self.clean_max = clean_area, clean_connectivity, clean_max
        self.clean_keep = self.cleaner.keep if self.cleaner is not None else None
        # boundary="deferred": a row per frame pushed with gt, beside _score_log; the call's output row and workspace are the segmenter's
        self._boundary_log = DeviceLog(self.device, {"counts": ((classes, 2, 2 + boundary_bins), torch.int32)})
        self._boundary_out = self._boundary_ws = None
        self._gt_table = None
        self._unmatched = None
        if gt_table is not None:
            t = torch.as_tensor(gt_table)
            if t.dtype != torch.uint8 or not (tuple(t.shape) == (256,) or (t.dim() == 2 and t.shape[1] == 4 and 1 <= t.shape[0] <= 256)):
                raise StswinHipError("gt_table must be uint8 [1 .. 256][4] (utils.groundtruth.colour_table) or uint8 [256] "
                                     f"(utils.groundtruth.remap_table), got {t.dtype} {tuple(t.shape)}")
            self._gt_table = t.contiguous().to(self.device)
            self._unmatched = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._table = None
        if out == "overlay":
            from .utils.visualize import default_palette, overlay_table
            if transparent is None:       # the background, or the remapped ignore label
                transparent = (model.classifier[-1].out_channels - 1,) if self.cadis else (0,)
            if edge_alpha is not None and (not isinstance(edge_alpha, int) or not 0 <= edge_alpha <= 255):
                raise StswinHipError(f"edge_alpha must be None or an int 0 .. 255, got {edge_alpha!r}")
            try:
                table = overlay_table(default_palette() if palette is None else palette, alpha, transparent)
            except ValueError as e:
                raise StswinHipError(f"out='overlay': {e}") from e
            self._table = torch.from_numpy(table).to(self.device)       # persistent: a captured graph reads it
        self.edge_alpha = edge_alpha
        self.pixel_format, self.chroma, self.out_format = pixel_format, chroma, out_format
        self._to_rgb = self._to_yuv = None                               # persistent: a captured graph reads them
        if pixel_format != "rgb" or out_format == "nv12":
            from .utils import yuv
            if pixel_format != "rgb":
                self._to_rgb = torch.from_numpy(yuv.to_rgb_matrix(yuv_standard, bool(full_range))).to(self.device)
            if out_format == "nv12":
                self._to_yuv = torch.from_numpy(yuv.to_yuv_matrix(yuv_standard, bool(full_range))).to(self.device)
        self.graph = graph
        self.planner = ClipPlanner(batch, rule=protocol)
        self.frame_shape = None
        self._ring = None
        self._pinned = _Pinned()
        self._g = None
        self.reset()

    @property
    def captured(self) -> bool:
        """graph=True: the steady step has been captured (later steady steps replay it)."""
        return self._g is not None

    def _check_train(self):
        if self.model.training:
            raise StswinHipError("VideoSegmenter needs the model in eval mode (model.eval()): in train mode BatchNorm uses batch "
                                 "statistics and a frame's features depend on its clip")

    def reset(self) -> None:
        self.planner.reset()
        self._frames = {}                 # frame index -> (uint8 tensor [k][Hs][Ws][3] (or raw nv12 / uyvy), GPU or CPU, row) until its ResNet pass
        self._kept = {}                   # out="overlay": frame index -> GPU uint8 [1][Hs][Ws][3] from its ResNet pass until its clip's result
        self._gt = {}
        self._score_log.end_sequence()    # scores="deferred": the sequence that ends here uses up its ordinal if it has rows in the log
        self.chain.reset()                # report="deferred": likewise, with its own ordinal; tracks: ids restart at 0
        self._boundary_log.end_sequence()  # boundary="deferred": likewise
        if self.cleaner is not None:
            self.cleaner.log.end_sequence()  # clean_area: likewise

    def reset_metrics(self) -> None:
        """Clear what an evaluation pools and reset() keeps: the confusion matrix (protocol="cadis"), the score log and its sequence
        ordinal (scores="deferred"), the instrument log and its ordinal (report="deferred"), the count of unmatched ground-truth
        pixels (gt_table); masks="deferred", confidence="deferred", parts="deferred" and clearance="deferred" log into the instrument log; the boundary log
        and its ordinal (boundary="deferred"); the log of the cleaning's stats and its ordinal (clean_area)."""
        if self.cleaner is not None:
            self.cleaner.log.clear()
        if self._cm is not None:
            self._cm.zero_()
        self._score_log.clear()
        self._boundary_log.clear()
        self.chain.log.clear()
        if self._unmatched is not None:
            self._unmatched.zero_()

    def unmatched(self) -> int:
        """gt_table: the pixels of colour-coded ground truth pushed so far whose colour no table row holds (they count as class 0),
        pooled over frames and sequences until reset_metrics().  One download."""
        if self._gt_table is None:
            raise StswinHipError("unmatched() belongs to gt_table")
        return int(self._unmatched.item())

    def endo_scores(self):
        """scores="deferred": one download of the score log -> utils.EndoMetric.EndoScores over every frame scored since
        reset_metrics(): the per-frame lists scores="frame" returns, and val_map's aggregates.  Row r of its lists is frame
        .frames[r] of sequence .sequences[r], rows ordered by sequence and frame."""
        if self.scores != "deferred":
            raise StswinHipError("endo_scores() belongs to scores='deferred'")
        from .utils.EndoMetric import EndoScores
        cols, sequences, frames = self._score_log.download()            # ordered by sequence and frame: the reference sums in frame order
        res = EndoScores.from_counts(cols["counts"], sequences)
        res.frames = frames
        return res

    def boundary_scores(self, names: Optional[Sequence[str]] = None):
        """boundary="deferred": one download of the boundary log -> utils.boundary.BoundaryScores over every frame pushed with gt since
        reset_metrics() - nsd(tau), hausdorff(), hausdorff_percentile(q), their aggregates - rows ordered by sequence and frame
        (.sequences[r], .frames[r]) as endo_scores() orders them.  names: the caller's class names, the default of as_rows()."""
        if self.boundary != "deferred":
            raise StswinHipError("boundary_scores() belongs to boundary='deferred'")
        from .utils.boundary import BoundaryScores
        cols, sequences, frames = self._boundary_log.download()
        res = BoundaryScores.from_counts(cols["counts"], sequences, frames)
        res.names = list(names) if names is not None else None
        return res

    def clean_report(self):
        """clean_area=A: one download of the stats log -> video_report.CleanReport over every frame released since reset_metrics() - per
        frame the small components of its raw label map (small[r] > clean_max: a truncated frame) and the pixels whose label changed -
        rows ordered by sequence and frame (.sequences[r], .frames[r]) as instrument_report() orders them."""
        if self.cleaner is None:
            raise StswinHipError("clean_report() belongs to clean_area=A")
        return self.cleaner.report()

    def _boundary(self, frame: int, gt: torch.Tensor, lab: torch.Tensor) -> None:
        """boundary="deferred": the five launches of hip.boundary_counts on a scored frame's gt and labels [1][*out_size], behind the
        launch that made the labels, and the row's copy into the log: no download, no synchronisation."""
        need = hip.boundary_scratch(1, *lab.shape[1:], self._classes)
        if self._boundary_ws is None or self._boundary_ws.numel() < need:         # once per frame size
            self._boundary_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._boundary_out = torch.empty(1, self._classes, 2, 2 + self.boundary_bins, dtype=torch.int32, device=self.device)
        hip.boundary_counts(gt.contiguous(), lab, self._classes, self.boundary_bins, self.boundary_skip, out=self._boundary_out,
                            workspace=self._boundary_ws)
        self._boundary_log.append(frame, counts=self._boundary_out)

    def instrument_report(self, names: Optional[Sequence[str]] = None):
        """report="deferred": one download of the instrument log -> utils.instruments.InstrumentReport (min_area as given to the
        segmenter) over every frame released since reset_metrics(), rows ordered by sequence and frame (.sequences[r], .frames[r]).
        names: the caller's class names, for as_rows()."""
        if self.report != "deferred":
            raise StswinHipError("instrument_report() belongs to report='deferred'")
        from .utils.instruments import InstrumentReport
        cols, sequences, frames = self.chain.log.download("moments")
        try:
            return InstrumentReport.from_moments(cols["moments"], self.out_size or (0, 0), self.min_area, names, frames, sequences)
        except ValueError as e:
            raise StswinHipError(f"instrument_report: {e}") from e

    def track_report(self, names: Optional[Sequence[str]] = None):
        """report="deferred" with tracks=True: one download of the track log -> utils.instruments.TrackReport over instance_report(names):
        every frame released since reset_metrics(), in its order and with its sequence ordinals; ids restart at 0 with every sequence."""
        if self.report != "deferred" or not self.tracks:
            raise StswinHipError("track_report() belongs to report='deferred' with tracks=True")
        if self.chain.parked:
            raise StswinHipError("track_report(): released frames still wait for their predecessors (finish() the sequence first)")
        from .utils.instruments import TrackReport
        rep = self.instance_report(names)
        cols = self.chain.log.download("ids", "started")[0]        # (in the rows' order: the same keys)
        try:
            return TrackReport.from_ids(rep, cols["ids"], cols["started"])
        except ValueError as e:
            raise StswinHipError(f"track_report: {e}") from e

    def mask_report(self, names: Optional[Sequence[str]] = None):
        """masks="deferred": one download of the mask log -> utils.rle.MaskReport over every frame released since reset_metrics(), rows
        ordered by sequence and frame as instrument_report()'s; with instances=K and report="deferred" joined with instance_report(names),
        with tracks=True with track_report(names) too (objects(r) then carry class and track, mots_lines() works)."""
        if self.masks != "deferred":
            raise StswinHipError("mask_report() belongs to masks='deferred'")
        if self.tracks and self.chain.parked:
            raise StswinHipError("mask_report(): released frames still wait for their predecessors (finish() the sequence first)")
        from .utils.instruments import InstanceReport, TrackReport
        from .utils.rle import MaskReport
        joined = self.instances is not None and self.report == "deferred"
        scored = self.confidence == "deferred"   # objects(r) then carry a score: the instance's (the class's) mean probability
        wanted = ("runs", "count") + (("rows", "total") if joined else ()) + (("ids", "started") if joined and self.tracks else ())
        wanted += self._confidence_columns() if scored else ()
        cols, sequences, frames = self.chain.log.download(*wanted)          # the one download: every column the report is made of
        size = self.out_size or (0, 0)         # (out="overlay" before its first frame: no size yet, and no row that would need one)
        skip = self.instance_skip if self.instance_skip is not None else (self.chain.classes - 1,) if self.cadis else (0,)
        inst = trk = conf = None
        try:
            if joined:
                inst = InstanceReport.from_rows(cols["rows"], cols["total"], size, self.min_area, names, frames, sequences)
                if self.tracks:
                    trk = TrackReport.from_ids(inst, cols["ids"], cols["started"])
            if scored:
                from .utils.confidence import ConfidenceReport
                conf = ConfidenceReport.from_sums(cols["class_sums"], cols.get("instance_sums"), self.confidence_low, names, frames, sequences)
            return MaskReport(cols["runs"], cols["count"], size, "labels" if self.instances is None else "instances", frames, sequences,
                              inst, trk, self.min_area, skip, names, confidence=conf)
        except ValueError as e:
            raise StswinHipError(f"mask_report: {e}") from e

    def _confidence_columns(self) -> Tuple[str, ...]:
        return ("class_sums",) + (("instance_sums",) if self.instances is not None else ())

    def confidence_report(self, names: Optional[Sequence[str]] = None):
        """confidence="deferred": one download of the confidence log -> utils.confidence.ConfidenceReport over every frame released since
        reset_metrics() - per class, and per instance with instances=K, the mean probability of its pixels and the share of them below
        confidence_low - rows ordered by sequence and frame as instrument_report()'s, with its sequence ordinals.  names: the caller's
        class names, for as_rows()."""
        if self.confidence != "deferred":
            raise StswinHipError("confidence_report() belongs to confidence='deferred'")
        from .utils.confidence import ConfidenceReport
        cols, sequences, frames = self.chain.log.download(*self._confidence_columns())
        try:
            return ConfidenceReport.from_sums(cols["class_sums"], cols.get("instance_sums"), self.confidence_low, names, frames, sequences)
        except ValueError as e:
            raise StswinHipError(f"confidence_report: {e}") from e

    def parts_report(self, names: Optional[Sequence[str]] = None):
        """parts="deferred": one download of the parts log -> utils.instruments.PartsReport over every frame released since
        reset_metrics() - per instance the area, box, centroid and axis of every class it holds, the classes it touches and
        direction() from one part to another - rows ordered by sequence and frame as instrument_report()'s, with its sequence
        ordinals; with report="deferred" joined by row with instance_report(names), with tracks=True with track_report(names) too."""
        if self.parts != "deferred":
            raise StswinHipError("parts_report() belongs to parts='deferred'")
        if self.tracks and self.chain.parked:
            raise StswinHipError("parts_report(): released frames still wait for their predecessors (finish() the sequence first)")
        from .utils.instruments import InstanceReport, PartsReport, TrackReport
        joined = self.report == "deferred"
        wanted = ("parts", "contacts") + (("rows", "total") if joined else ()) + (("ids", "started") if joined and self.tracks else ())
        cols, sequences, frames = self.chain.log.download(*wanted)          # the one download: every column the report is made of
        size = self.out_size or (0, 0)
        inst = trk = None
        try:
            if joined:
                inst = InstanceReport.from_rows(cols["rows"], cols["total"], size, self.min_area, names, frames, sequences)
                if self.tracks:
                    trk = TrackReport.from_ids(inst, cols["ids"], cols["started"])
            return PartsReport(cols["parts"], cols["contacts"], size, names, frames, sequences, inst, trk)
        except ValueError as e:
            raise StswinHipError(f"parts_report: {e}") from e

    def clearance_report(self, names: Optional[Sequence[str]] = None):
        """clearance="deferred": one download of the clearance log -> utils.instruments.ClearanceReport over every frame released since
        reset_metrics() - per instance the distance to every class measured and the two pixels that realise it - rows ordered by
        sequence and frame as instrument_report()'s, with its sequence ordinals; with report="deferred" joined by row with
        instance_report(names), with tracks=True with track_report(names) too."""
        if self.clearance != "deferred":
            raise StswinHipError("clearance_report() belongs to clearance='deferred'")
        if self.tracks and self.chain.parked:
            raise StswinHipError("clearance_report(): released frames still wait for their predecessors (finish() the sequence first)")
        from .utils.instruments import ClearanceReport, InstanceReport, TrackReport
        joined = self.report == "deferred"
        wanted = ("clearance",) + (("rows", "total") if joined else ()) + (("ids", "started") if joined and self.tracks else ())
        cols, sequences, frames = self.chain.log.download(*wanted)          # the one download: every column the report is made of
        size = self.out_size or (0, 0)
        inst = trk = None
        try:
            if joined:
                inst = InstanceReport.from_rows(cols["rows"], cols["total"], size, self.min_area, names, frames, sequences)
                if self.tracks:
                    trk = TrackReport.from_ids(inst, cols["ids"], cols["started"])
            return ClearanceReport(cols["clearance"], size, names, frames, sequences, inst, trk)
        except ValueError as e:
            raise StswinHipError(f"clearance_report: {e}") from e

    def instance_report(self, names: Optional[Sequence[str]] = None):
        """report="deferred" with instances=K: one download of the instance log -> utils.instruments.InstanceReport (min_area as given
        to the segmenter) over every frame released since reset_metrics(), rows ordered by sequence and frame as instrument_report()'s.
        names: the caller's class names, for as_rows()."""
        if self.report != "deferred" or self.instances is None:
            raise StswinHipError("instance_report() belongs to report='deferred' with instances=K")
        from .utils.instruments import InstanceReport
        cols, sequences, frames = self.chain.log.download("rows", "total")
        try:
            return InstanceReport.from_rows(cols["rows"], cols["total"], self.out_size or (0, 0), self.min_area, names, frames, sequences)
        except ValueError as e:
            raise StswinHipError(f"instance_report: {e}") from e

    def confusion_matrix(self) -> np.ndarray:
        """protocol="cadis": the pooled confusion matrix, float64 [metric_classes][metric_classes], rows gt, columns prediction."""
        if not self.cadis:
            raise StswinHipError("confusion_matrix() belongs to protocol='cadis'")
        if self._cm is None:
            return np.zeros((self.metric_classes, self.metric_classes))
        return self._cm.cpu().numpy().astype(np.float64)

    # ----------------------------------------------------------------------------------------- public
    def push(self, frames, gt=None) -> List[Tuple[int, object]]:
        self._check_train()
        fr = self._as_frames(frames)
        n = fr.shape[0]
        if gt is not None and self._gt_table is not None:
            gt = self._decode_gt(gt, n)
        elif gt is not None:
            gt = torch.as_tensor(gt)
            if gt.dim() == 2:
                gt = gt[None]
            if gt.shape[0] != n or tuple(gt.shape[1:]) != self.out_size:
                raise StswinHipError(f"gt must be [{n}][{self.out_size[0]}][{self.out_size[1]}], got {tuple(gt.shape)}")
            gt = gt.to(self.device, torch.int64)
        f0 = self.planner.seen
        for j in range(n):
            self._frames[f0 + j] = (fr, j)
            if gt is not None:
                self._gt[f0 + j] = gt[j:j + 1]
        return self._run_all(self.planner.push(n))

    def finish(self) -> List[Tuple[int, object]]:
        self._check_train()
        res = self._run_all(self.planner.finish())
        if self.chain.parked:
            raise StswinHipError(f"internal error: frames {sorted(self.chain.parked)} were released and never tracked")
        return res

    def segment_sequence(self, frames, gt=None) -> list:
        self.reset()
        res = self.push(frames, gt) + self.finish()
        if self.graph:
            res = [(f, _clone(r)) for f, r in res]
        self.reset()
        return [r for _, r in sorted(res, key=lambda fr: fr[0])]

    # ----------------------------------------------------------------------------------------- internals
    def _decode_gt(self, gt, n: int) -> torch.Tensor:
        """gt_table: stored ground truth (uint8, colour- or id-coded, CPU or GPU) -> int64 class indices [n][*out_size] on the device:
        the bytes are uploaded as they are and decoded by one launch (hip.gt_decode), which also pools the unmatched pixels."""
        gt = torch.as_tensor(gt)
        colour = self._gt_table.dim() == 2
        if gt.dim() == (3 if colour else 2):
            gt = gt[None]
        want = f"[{n}][{self.out_size[0]}][{self.out_size[1]}]" + ("[3 | 4]" if colour else "") if self.out_size else "of the output size"
        if (gt.dtype != torch.uint8 or gt.dim() != (4 if colour else 3) or gt.shape[0] != n or tuple(gt.shape[1:3]) != self.out_size
                or (colour and gt.shape[3] not in (3, 4))):
            raise StswinHipError(f"with gt_table, gt must be uint8 {want}, got {gt.dtype} {tuple(gt.shape)}")
        if gt.is_cuda and gt.device != self.device:
            raise StswinHipError(f"gt on {gt.device}, the model on {self.device}")
        gt = gt.contiguous()
        if not gt.is_cuda:
            gt = self._pinned.upload(gt.numpy(), torch.empty(gt.shape, dtype=torch.uint8, device=self.device))
        H, W = self.out_size
        flat = gt.view(1, n * H, W, gt.shape[3]) if colour else gt.view(1, n * H, W)    # one "frame": one pooled unmatched count
        return hip.gt_decode(flat, self._gt_table, torch.int64, self._unmatched if colour else None).view(n, H, W)

    def _as_frames(self, frames) -> torch.Tensor:
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(frames)
        form = _FRAME_FORMS[self.pixel_format]
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            raise StswinHipError(f"frames must be {form} (torch tensor or numpy array)")
        dims = 3 if self.pixel_format == "nv12" else 4
        if frames.dim() == dims - 1:
            frames = frames[None]
        if frames.dim() != dims or (dims == 4 and frames.shape[3] != (2 if self.pixel_format == "uyvy" else 3)):
            raise StswinHipError(f"frames must be {form}, got {tuple(frames.shape)}")
        if self.pixel_format == "nv12":
            if frames.shape[1] % 3 or frames.shape[2] % 2:
                raise StswinHipError(f"frames must be {form} with Hs and Ws even, got {tuple(frames.shape)}")
            shape = (frames.shape[1] // 3 * 2, frames.shape[2])
        else:
            shape = tuple(frames.shape[1:3])
            if shape[1] % 2 and self.pixel_format == "uyvy":
                raise StswinHipError(f"frames must be {form} with Ws even, got {tuple(frames.shape)}")
        if self.out_format == "nv12" and (shape[0] % 2 or shape[1] % 2):
            raise StswinHipError(f"out_format='nv12' needs an even frame size, got {shape}")
        if self.frame_shape is None:
            if self.out == "overlay":
                if self.out_size is None:
                    self.out_size = shape
                elif self.out_size != shape:
                    raise StswinHipError(f"out='overlay' blends onto the pushed frame: out_size {self.out_size} differs from the frame "
                                         f"size {shape}")
            self.frame_shape = shape
        elif shape != self.frame_shape:
            raise StswinHipError(f"frame size {shape} differs from the earlier frames' {self.frame_shape}")
        if frames.is_cuda and frames.device != self.device:
            raise StswinHipError(f"frames on {frames.device}, the model on {self.device}")
        return frames.contiguous()           # (CPU frames stay on the host until their step copies them from pinned memory)

    def _put_frames(self, src: torch.Tensor, r0: int, k: int, dst: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Rows r0 .. r0+k of a pushed frame tensor on the GPU: a view of it, or (CPU frames, or a static buffer `dst`) a copy."""
        part = src[r0:r0 + k]
        if dst is None:
            if part.is_cuda:
                return part
            dst = torch.empty(part.shape, dtype=torch.uint8, device=self.device)
        if part.is_cuda:
            return dst.copy_(part)
        return self._pinned.upload(part.numpy(), dst)

    def _static_image(self, raw: torch.Tensor, u8: torch.Tensor) -> torch.Tensor:
        """The graph step's first launches: the static input buffer (raw pixel formats: converted into the static RGB buffer u8, which
        the overlay blends onto) -> the fp32 image."""
        if self._to_rgb is not None:
            hip.yuv_to_rgb(raw, self._to_rgb, self.pixel_format, self.chroma, out=u8)
        return ingest(u8, self.size, protocol=self.protocol)

    def _upload_table(self, values: List[int], dst: Optional[torch.Tensor] = None) -> torch.Tensor:
        if dst is None:
            dst = torch.empty(len(values), dtype=torch.int32, device=self.device)
        return self._pinned.upload(np.asarray(values, dtype=np.int32), dst)

    def _ingest_new(self, new: List[int]) -> torch.Tensor:
        """The new frames' fp32 images [n][3][H][W]: one ingest launch per run of rows of one pushed tensor (raw pixel formats: one
        hip.yuv_to_rgb launch before it).  out="overlay" keeps the device RGB tensor that the ingest read, one view per frame, for the
        frame's own clip: the copy made of CPU frames, the pushed tensor itself for GPU RGB frames, the converted frames for raw ones."""
        out = torch.empty(len(new), 3, *self.size, dtype=torch.float32, device=self.device)
        j = 0
        while j < len(new):
            src, r0 = self._frames.pop(new[j])
            k = 1
            while j + k < len(new) and self._frames[new[j + k]][0] is src and self._frames[new[j + k]][1] == r0 + k:
                self._frames.pop(new[j + k])
                k += 1
            dev = self._put_frames(src, r0, k)
            if self._to_rgb is not None:                     # raw frames: the RGB frames are made here, the raw bytes are done with
                dev = hip.yuv_to_rgb(dev, self._to_rgb, self.pixel_format, self.chroma)
            ingest(dev, self.size, out[j:j + k], self.protocol)
            if self._table is not None:
                for i in range(k):
                    self._kept[new[j + i]] = dev[i:i + 1]
            j += k
        return out

    def _compute(self, img: Optional[torch.Tensor], table: torch.Tensor, B: int, n_new: int, labels: bool = False, frames=None,
                 tracked: bool = False):
        """ResNet on the new frames' images, clip assembly, Swin / ASPP / head: -> logits (B, nc, H, W), and with labels = True the
        labels (B, *out_size), or for out="overlay" the overlay (B, *out_size, 3) on `frames`, one uint8 [1][Hs][Ws][3] per clip, and
        with report what the labels yield per clip (_finish_labels; `tracked`: the graph's steady step, the tracker's launches in it),
        and with clean_area the cleaning's stats (B, 2): the labels are then the cleaned ones, made behind the label launch.
        Every launch on the current stream, no host synchronisation (graph-capturable)."""
        m = self.model
        hip.arena_reset(self.device)
        h, w = self.size[0] // 8, self.size[1] // 8
        tok = None
        if n_new:
            # the GEMMs plan as for model(clip)'s launch over the clip's T frames: the same kernels, a frame's features the same bits
            with hip.splitk_as_rows(T):
                tok, h2, w2 = m.resnet.forward_tokens(img, groups=1)
            if (h2, w2) != (h, w):
                raise StswinHipError(f"the ResNet gives {h2}x{w2} features, the model's swin.input_resolution is {(h, w)}")
        dt = tok.dtype if tok is not None else self._ring.dtype
        L = h * w
        if self._ring is None:
            self._ring = torch.empty(self.planner.slots, L, 512, dtype=dt, device=self.device)
        elif self._ring.dtype != dt:
            raise StswinHipError(f"the compute dtype changed within the segmenter ({self._ring.dtype} -> {dt}): keep autocast as it "
                                 "was, or make a new VideoSegmenter")
        clips = torch.empty(B, T, L, 512, dtype=dt, device=self.device)
        hip.clip_assemble(self._ring, tok, clips, table, B, n_new)
        logits = m.forward_frame_tokens(clips, h, w, self.size[0], self.size[1])
        if labels:
            lab, stats = self._clean(self._labels(logits))
            return (logits,) + self._finish_labels(lab, frames, steady=tracked, logits=logits) + (stats,)
        return logits, None, None, None

    def _clean(self, lab: Optional[torch.Tensor]):
        """clean_area: a step's (a clip's) labels -> (the cleaned labels, the stats), behind the label launch and in front of
        everything that reads the labels; without the keyword (or without labels) the labels themselves and None."""
        if self.cleaner is None or lab is None:
            return lab, None
        return self.cleaner.clean(lab)

    def _score_cleaned(self, g: int, logits: torch.Tensor, gt: torch.Tensor):
        """clean_area with ground truth: the label launch without gt, the cleaning launches, then hip.labels_score counts the cleaned
        labels as the fused launches count their own -> (labels, stats, (dice, iou) or ())."""
        lab, stats = self._clean(self._labels(logits))
        gt = gt.contiguous()
        if self.cadis:
            if self._cm is None:
                self._cm = torch.zeros(self.metric_classes, self.metric_classes, dtype=torch.int64, device=self.device)
            hip.labels_score(lab, gt, self._classes, cm=self._cm)
            return lab, stats, ()
        counts = hip.labels_score(lab, gt, self._classes)[0]
        if self.scores == "deferred":
            self._score_log.append(g, counts=counts)
            return lab, stats, ()
        from .utils.EndoMetric import _frame_lists
        dices, ious = _frame_lists(counts.cpu().numpy().astype(np.float64))
        return lab, stats, (dices[0], ious[0])

    def _finish_labels(self, lab: torch.Tensor, frames, clips: Optional[List[int]] = None, steady: bool = False,
                       logits: Optional[torch.Tensor] = None):
        """Labels (B, *out_size) of a step, or of the one clip `clips` names (made by a scoring launch) -> (the result form of out="labels"
        | "overlay", what the report chain makes of them per clip).  The one statement of the order: moments, (grouping,) components,
        (tracks), masks, confidence (on `logits`, the ones the labels were made from), parts, overlay."""
        ys = self.chain.labelled(lab, clips, steady, logits=logits)
        return lab if self._table is None else self._overlay(lab, frames), ys

    def _overlay(self, labels: torch.Tensor, frames) -> torch.Tensor:
        """labels (B, *out_size) blended onto the clips' own frames: one launch per clip (the frames live in separate tensors);
        out_format="nv12": one more launch turns the overlays (B, Hs, Ws, 3) into NV12 (B, 3 Hs / 2, Ws)."""
        out = torch.empty(*labels.shape, 3, dtype=torch.uint8, device=self.device)
        for b, fr in enumerate(frames):
            hip.labels_overlay(labels[b:b + 1], self._table, fr, self.edge_alpha, out[b:b + 1])
        if self._to_yuv is not None:
            return hip.rgb_to_nv12(out, self._to_yuv)
        return out

    def _labels(self, logits: torch.Tensor, gt: Optional[torch.Tensor] = None, want: bool = True) -> Optional[torch.Tensor]:
        if not self.cadis:
            return hip.upsample_argmax(logits, *self.out_size)[0]
        cm = None
        if gt is not None:
            if self._cm is None:
                self._cm = torch.zeros(self.metric_classes, self.metric_classes, dtype=torch.int64, device=self.device)
            cm = self._cm
        return hip.upsample_argmax_cm(logits, *self.out_size, gt=gt, cm=cm, align_corners=self.align_corners, labels=want)

    def _steady(self, st: Step) -> bool:
        return len(st.new) == 1 and len(st.clips) == 1 and st.clips[0] == st.new[0] and st.clips[0] >= min_frames(self.protocol)

    def _run_all(self, steps: List[Step]) -> List[Tuple[int, object]]:
        res = []
        with torch.no_grad():
            for i, st in enumerate(steps):
                r, replayed = self._run(st)
                if replayed and i + 1 < len(steps):        # the next replay of this call overwrites the graph's output buffers
                    r = [(f, _clone(x)) for f, x in r]
                res += r
        return res

    def _run(self, st: Step):
        B, n_new = len(st.clips), len(st.new)
        want_labels = self.out != "logits" and not any(g in self._gt for g in st.clips)
        if self.graph and self._steady(st):
            logits, labels, extras, stats, replayed, frames = self._run_graph(st, want_labels)
        else:
            img = self._ingest_new(st.new) if n_new else None
            frames = [self._kept.pop(g) for g in st.clips] if self._table is not None else None
            logits, labels, extras, stats = self._compute(img, self._upload_table(st.table()), B, n_new, want_labels, frames)
            replayed = False
        return self._results(st.clips, logits, labels, frames, extras, stats), replayed

    def _run_graph(self, st: Step, want_labels: bool):
        src, r = self._frames.pop(st.new[0])
        g = self._g
        tracked = self.tracks and want_labels     # the tracker's launches are part of the step: the steady state is in frame order
        if tracked:
            self.chain.step_is_steady(st.new[0])
        if g is None or g.want_labels != want_labels:
            # first steady-state step (or first of the other output form): one eager warm-up on the static buffers (on a side stream,
            # as graph.py's GraphedStep does), then the capture; this step's result is the warm-up's
            u8 = torch.empty(1, *self.frame_shape, 3, dtype=torch.uint8, device=self.device)
            # raw pixel formats: the static input buffer holds the raw frame, the step begins with its conversion into u8
            raw = u8 if self._to_rgb is None else torch.empty(1, *src.shape[1:], dtype=torch.uint8, device=self.device)
            frames = [u8] if self._table is not None else None     # the steady step's clip is the new frame's: blend onto the static buffer
            table = torch.empty(T + 1, dtype=torch.int32, device=self.device)
            self._put_frames(src, r, 1, raw)
            self._upload_table(st.table(), table)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                logits, labels, extras, stats = self._compute(self._static_image(raw, u8), table, 1, 1, want_labels, frames, tracked)
                logits = logits.clone()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            hip.note_capture()
            graph = torch.cuda.CUDAGraph()
            autocast = torch.is_autocast_enabled()
            with torch.cuda.graph(graph):
                out, out_labels, out_extras, out_stats = self._compute(self._static_image(raw, u8), table, 1, 1, want_labels, frames, tracked)
            self._g = Captured(graph, raw, table, out, out_labels, want_labels, autocast, u8, out_extras, out_stats)
            return logits, labels, extras, stats, False, frames
        if torch.is_autocast_enabled() != g.autocast:
            raise StswinHipError("autocast differs from the state the step was captured under: make a new VideoSegmenter")
        self._put_frames(src, r, 1, g.raw)
        self._upload_table(st.table(), g.table)
        g.graph.replay()
        return g.out, g.labels, g.extras, g.stats, True, [g.u8] if self._table is not None else None

    def _results(self, clips: List[int], logits: torch.Tensor, labels: Optional[torch.Tensor], frames=None,
                 extras: Optional[List[Yield]] = None, stats: Optional[torch.Tensor] = None) -> List[Tuple[int, object]]:
        """`labels`: the step's labels (out="overlay": its overlays), with report their `extras` per clip and with clean_area the
        cleaning's `stats`, or None when some clip has ground truth or out="logits": each clip's labels then come from its own
        (scoring) launch."""
        if labels is not None:
            results = list(labels)
            if stats is not None:
                self.cleaner.released(clips, stats)
        else:
            results, extras = [], []
            for b, g in enumerate(clips):
                gt = self._gt.pop(g, None)
                scored = ()
                if gt is None:
                    lab, stats = self._clean(self._labels(logits[b:b + 1]) if self.out != "logits" else None)
                elif self.cleaner is not None:     # the scores are those of the cleaned labels
                    lab, stats, scored = self._score_cleaned(g, logits[b:b + 1], gt)
                elif self.cadis:
                    lab = self._labels(logits[b:b + 1], gt, want=self.out != "logits")
                elif self.scores == "deferred":       # the counts stay on the device: no download, no synchronisation
                    lab, counts = hip.upsample_argmax(logits[b:b + 1], *self.out_size, gt)
                    self._score_log.append(g, counts=counts)
                else:
                    from .utils.EndoMetric import predict_and_score
                    lab, dices, ious = predict_and_score(logits[b:b + 1], self.out_size, gt)
                    scored = (dices[0], ious[0])
                if self.cleaner is not None:
                    self.cleaner.released([g], stats)
                if gt is not None and self.boundary is not None:
                    self._boundary(g, gt, lab)
                r, y = logits[b], None
                if self.out != "logits":
                    out, ys = self._finish_labels(lab, frames and frames[b:b + 1], [g], logits=logits[b:b + 1])
                    r, y = out[0], ys and ys[0]
                results.append((r,) + scored if scored else r)
                extras.append(y)
        return list(zip(clips, self.chain.released(clips, results, extras)))


# The graph's steady step: the static buffers it reads (raw: the pushed frame; u8: the RGB frame, the same tensor for pixel_format="rgb";
# the slot table) and writes (out: the logits; with want_labels the labels or overlays and the report chain's extras), its autocast state
# and with clean_area the cleaning's stats
Captured = namedtuple("Captured", "graph raw table out labels want_labels autocast u8 extras stats")


def _clone(r):
    if isinstance(r, torch.Tensor):
        return r.clone()
    if isinstance(r, tuple):
        return tuple(_clone(x) for x in r)
    return r
