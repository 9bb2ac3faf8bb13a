"""What a VideoSegmenter makes of its label maps beside the result (its docstring states the keywords): the chain moments -> instances
-> tracks -> masks -> confidence -> parts -> clearance with its buffers (ReportChain), its record (Yield), the tracker's frame order (TrackSequencer) and the device log;
and what it does to them before anything reads them: the cleaning of clean_area (LabelCleaner) and its report (CleanReport)."""
from __future__ import annotations

from collections import namedtuple
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import hip
from .hip import StswinHipError


class DeviceLog:
    """An append-only log on a device: column tensors [capacity][*row shape] that share their rows, and on the host one key
    (sequence ordinal, frame index) per row; a sequence's ordinal is the number of earlier sequences that logged a row since clear().
    Appending is a device copy, no synchronisation; full columns double (zeros of max(64, 2 n) rows, the first n copied).
    `groups`: dicts name -> (row shape, dtype), in the order in which a row's values are copied; a group's columns grow together."""

    def __init__(self, device, *groups: Dict[str, Tuple[Tuple[int, ...], torch.dtype]]):
        self.device, self.groups, self.columns = device, groups, {name: c for g in groups for name, c in g.items()}
        self.data: Dict[str, torch.Tensor] = {}
        self.capacity = 0
        self.clear()

    def clear(self) -> None:                  # forget every row, restart the ordinal (the device tensors are kept and overwritten)
        self.keys: List[Tuple[int, int]] = []
        self.sequence = 0

    def end_sequence(self) -> None:           # the running sequence ends: the next one gets the next ordinal if this one logged a row
        if self.keys and self.keys[-1][0] == self.sequence:
            self.sequence += 1

    def append(self, frame: int, **values: torch.Tensor) -> int:
        """One row for `frame` of the running sequence -> its index.  A column without a value is left for write()."""
        n = len(self.keys)
        self.keys.append((self.sequence, frame))
        grow = n == self.capacity
        if grow:
            self.capacity = max(64, 2 * n)
        for group in self.groups:
            for name, (shape, dtype) in group.items() if grow else ():
                grown = torch.zeros(self.capacity, *shape, dtype=dtype, device=self.device)
                if n:
                    grown[:n].copy_(self.data[name][:n])
                self.data[name] = grown
            self.write(n, **{name: values.get(name) for name in group})
        return n

    def write(self, row: int, **values: torch.Tensor) -> None:
        """Values of an appended row, now or later (a parked frame's track row), in the columns' order."""
        for name in self.columns:
            if values.get(name) is not None:
                dst = self.data[name][row:row + 1]
                dst.copy_(values[name].reshape(dst.shape))

    def download(self, *names: str):
        """-> (name -> numpy array [rows][*row shape], sequences, frames) for the columns named (default: all), rows ordered by
        (sequence, frame) - the log itself is in release order; without rows the empty arrays of the columns' shapes."""
        n = len(self.keys)
        order = sorted(range(n), key=self.keys.__getitem__)
        cols = {}
        for name in names or self.columns:
            shape, dtype = self.columns[name]
            cols[name] = self.data[name][:n].cpu().numpy()[order] if n else torch.zeros(0, *shape, dtype=dtype).numpy()
        return cols, [self.keys[r][0] for r in order], [self.keys[r][1] for r in order]


class CleanReport:
    """VideoSegmenter(clean_area=A).clean_report(): what the cleaning did per released frame, rows ordered by sequence and frame.
    frames[r], sequences[r]: the row's frame index and its sequence's ordinal; small[r]: the small components of the frame's raw label
    map (not bounded by clean_max: small[r] > max_small is a truncated frame); changed[r]: the pixels whose label changed."""

    def __init__(self, stats, frames, sequences, max_small: int):
        self.frames, self.sequences, self.max_small = list(frames), list(sequences), max_small
        self.small, self.changed = stats[:, 0].copy(), stats[:, 1].copy()

    def __len__(self):
        return len(self.frames)

    def as_rows(self) -> List[dict]:
        return [dict(sequence=s, frame=f, small=int(k), changed=int(c), truncated=bool(k > self.max_small))
                for s, f, k, c in zip(self.sequences, self.frames, self.small, self.changed)]


class LabelCleaner:
    """clean_area of a VideoSegmenter: the launches of hip.labels_clean on every label map the segmenter makes, in front of everything
    that reads the labels.  Owns the workspace (it only grows; the ones it replaced are kept, a captured step may still use them) and
    the device log of the stats, one row per released frame.  The cleaned map and the stats are fresh per step (under capture: the
    graph's), as the labels they replace are."""

    def __init__(self, device, classes: int, out: str, area, keep, connectivity, max_small):
        if area is None:
            raise StswinHipError("internal error: a LabelCleaner without clean_area")
        if out == "logits":
            raise StswinHipError("clean_area cleans the label map: out must be 'labels' or 'overlay'")
        if isinstance(area, bool) or not isinstance(area, int) or not 2 <= area <= 1 << 30:
            raise StswinHipError(f"clean_area must be None or an int 2 .. 2^30 (pixels; 1 would change nothing), got {area!r}")
        if not 1 <= classes <= 64:
            raise StswinHipError(f"clean_area: the model has {classes} classes, hip.labels_clean takes 1 .. 64")
        if keep is None:
            keep = ()
        try:
            keep = tuple(keep)
        except TypeError:
            keep = (keep,)
        if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 63 for c in keep):
            raise StswinHipError(f"clean_keep holds classes 0 .. 63, got {keep!r}")
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise StswinHipError(f"clean_connectivity must be 4 or 8, got {connectivity!r}")
        if isinstance(max_small, bool) or not isinstance(max_small, int) or not 1 <= max_small <= 65536:
            raise StswinHipError(f"clean_max must be an int 1 .. 65536, got {max_small!r}")
        self.device, self.classes = device, classes
        self.area, self.keep, self.connectivity, self.max_small = area, keep, connectivity, max_small
        self.ws = None
        self.retired = []
        self.log = DeviceLog(device, dict(stats=((2,), torch.int32)))

    def clean(self, labels: torch.Tensor):
        """labels [B][H][W] -> (the cleaned labels, stats int32 [B][2]): no allocation but the outputs, no synchronisation."""
        need = hip.labels_clean_scratch(*labels.shape, self.classes, self.max_small)
        if self.ws is None or self.ws.numel() < need:
            if self.ws is not None:
                self.retired.append(self.ws)
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return hip.labels_clean(labels, self.classes, self.area, self.connectivity, self.keep, self.max_small, workspace=self.ws)

    def released(self, frames: Sequence[int], stats: torch.Tensor) -> None:
        """The clips of `frames` are released: their stats rows [B][2] into the log (a device copy each)."""
        for b, g in enumerate(frames):
            self.log.append(g, stats=stats[b:b + 1])

    def report(self) -> CleanReport:
        cols, sequences, frames = self.log.download("stats")
        return CleanReport(cols["stats"], frames, sequences, self.max_small)


class Yield(namedtuple("Yield", "moments rows total ids started runs count conf class_sums instance_sums parts contacts clearance",
                       defaults=(None,) * 13)):
    """What the labels [B][*out_size] of a step (or of one clip, B = 1) yield on the device: moments int64 [B][nc][10]; with instances
    rows int64 [B][K][12] and total int32 [B]; once tracked ids int32 [B][K] and started int32 [B][1]; with masks runs int32
    [B][cap][2] and count int32 [B]; with confidence conf uint8 [B][*out_size], class_sums int64 [B][nc][3] and, with instances,
    instance_sums int64 [B][K][3]; with parts parts int64 [B][K][nc][10] and contacts int64 [B][K][nc]; with clearance clearance int64 [B][K][nc][3].  Absent fields are
    None."""
    __slots__ = ()

    def clip(self, b: int) -> "Yield":
        """Clip b's part [1][...]."""
        return Yield(*(None if t is None else t[b:b + 1] for t in self))

    def appended(self, result, report: bool = True, masks: bool = False, confidence: bool = False, parts: bool = False,
                 clearance: bool = False):
        """report="frame": a clip's result r -> r + (moments, rows, total, ids), what there is of them; masks="frame": then
        + (runs, count); confidence="frame": then + (conf, class_sums[, instance_sums]); parts="frame": then + (parts, contacts);
        clearance="frame": then + (clearance,); all on the device."""
        extra = tuple(t[0] for t in self[:4] if t is not None) if report else ()
        if masks:
            extra += (self.runs[0], self.count[0])
        if confidence:
            extra += tuple(t[0] for t in (self.conf, self.class_sums, self.instance_sums) if t is not None)
        if parts:
            extra += (self.parts[0], self.contacts[0])
        if clearance:
            extra += (self.clearance[0],)
        return result + extra if isinstance(result, tuple) else (result,) + extra

    def logged(self, log: DeviceLog, frame: int, tracked: bool = True, report: bool = True, masks: bool = False,
               confidence: bool = False, parts: bool = False, clearance: bool = False) -> int:
        """report="deferred", masks="deferred", confidence="deferred", parts="deferred" and / or clearance="deferred": a clip's row in the log -> its index
        (tracked = False: ids and started are written when it is tracked); the columns of what is not deferred are left alone.  Of the
        confidence the sums are logged, not the map."""
        values = dict(moments=self.moments, rows=self.rows, total=self.total, ids=self.ids if tracked else None,
                      started=self.started if tracked else None) if report else {}
        if masks:
            values.update(runs=self.runs, count=self.count)
        if confidence:
            values.update(class_sums=self.class_sums, instance_sums=self.instance_sums)
        if parts:
            values.update(parts=self.parts, contacts=self.contacts)
        if clearance:
            values.update(clearance=self.clearance)
        return log.append(frame, **values)


class TrackSequencer:
    """The tracker's frame-order rule.  The tracker takes the frames of a sequence in frame order, which is not the order of release
    (endovis18 releases 0, 1, 4, 2, 5, 3, 6, ..., cadis 0, 1, 2, 5, 3, 6, 4, 7, ..., a batch in the planner's order): a released frame
    whose predecessor has not been tracked is parked, and tracked when the predecessor is."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:                                  # a new sequence: frame 0 is next, nothing is parked
        self.next = 0
        self.parked = set()

    def release(self, frame: int) -> List[int]:
        """Frame `frame` is released -> the frames to track now, in order: the frame itself and the parked frames that drain behind
        it, or [] when the frame is parked."""
        if frame != self.next:
            self.parked.add(frame)
            return []
        now = [frame]
        self.next += 1
        while self.next in self.parked:
            self.parked.remove(self.next)
            now.append(self.next)
            self.next += 1
        return now


class ReportChain:
    """report / instances / tracks / masks / confidence of a VideoSegmenter: hip.label_moments, then the launches of
    hip.label_components, then those of hip.track_instances, then those of hip.rle_encode (on the component map with instances, else on
    the labels), then hip.upsample_confidence on the logits the labels came from and hip.confidence_sums over the labels (and over
    the component map with instances), then hip.instance_parts and hip.instance_clearance over the labels and the component map, on every
    label map the segmenter makes.  With instance_groups the component launches read the grouped labels, which hip.gt_decode makes of the labels with the
    persistent table of utils.instruments.group_table; everything else reads the labels themselves.  The segmenter calls labelled() where a step's labels exist and
    released() where its frames are handed out (step_is_steady() is the check in front of the graph's steady step, which tracks inside
    itself).  Owns what persists across steps: the component map, the grouped labels and the workspaces (they only grow; the ones they replaced are kept, a
    captured step may still use them), the tracker's state, the parked frames, the pool of their map copies, and the deferred log."""

    def __init__(self, device, classes: int, protocol: str, out: str, report, min_area, instances, connectivity, instance_skip, tracks,
                 track_iou, track_same_class, masks=None, mask_runs=16384, track_max_gap=0, confidence=None, confidence_low=128,
                 align_corners=True, parts=None, instance_groups=None, clearance=None, clearance_to=None, clearance_max=None):
        if clearance not in (None, "frame", "deferred"):
            raise StswinHipError(f"clearance must be None, 'frame' or 'deferred', got {clearance!r}")
        if clearance is None and (clearance_to is not None or clearance_max is not None):
            raise StswinHipError("clearance_to and clearance_max belong to clearance='frame' or 'deferred'")
        if clearance is not None and out == "logits":
            raise StswinHipError("clearance belongs to out='labels' and out='overlay' (the distances are taken over the label map)")
        if clearance is not None and instances is None:
            raise StswinHipError("clearance says how near the instances come to what they do not touch: it needs instances=K")
        if clearance is not None:
            if not 1 <= classes <= 64:
                raise StswinHipError(f"clearance: the model has {classes} classes, hip.instance_clearance takes 1 .. 64")
            if clearance_to is not None:
                try:
                    clearance_to = tuple(clearance_to)
                except TypeError:
                    clearance_to = (clearance_to,)
                if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < classes for c in clearance_to):
                    raise StswinHipError(f"clearance_to holds classes 0 .. {classes - 1}, got {clearance_to!r}")
            if clearance_max is not None and (isinstance(clearance_max, bool) or not isinstance(clearance_max, int) or clearance_max < 0):
                raise StswinHipError(f"clearance_max must be None or an int >= 0 (pixels), got {clearance_max!r}")
        if parts not in (None, "frame", "deferred"):
            raise StswinHipError(f"parts must be None, 'frame' or 'deferred', got {parts!r}")
        if parts is not None and out == "logits":
            raise StswinHipError("parts belongs to out='labels' and out='overlay' (the parts are taken over the label map)")
        if parts is not None and instances is None:
            raise StswinHipError("parts says what the instances are made of and what they touch: it needs instances=K")
        if instance_groups is not None and instances is None:
            raise StswinHipError("instance_groups belongs to instances=K")
        if report not in (None, "frame", "deferred"):
            raise StswinHipError(f"report must be None, 'frame' or 'deferred', got {report!r}")
        if report is not None and out == "logits":
            raise StswinHipError("report belongs to out='labels' and out='overlay' (the moments are taken over the label map)")
        if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 1:
            raise StswinHipError(f"min_area must be an int >= 1, got {min_area!r}")
        if report is not None and not 1 <= classes <= 64:
            raise StswinHipError(f"report: the model has {classes} classes, hip.label_moments takes 1 .. 64")
        if instances is None:
            if connectivity != 8 or instance_skip is not None:
                raise StswinHipError("connectivity and instance_skip belong to instances=K")
        else:
            if report is None:
                raise StswinHipError("instances=K splits the instrument report: it needs report='frame' or 'deferred'")
            if isinstance(instances, bool) or not isinstance(instances, int) or not 1 <= instances <= 1024:
                raise StswinHipError(f"instances must be None or an int 1 .. 1024, got {instances!r}")
            if isinstance(connectivity, bool) or connectivity not in (4, 8):
                raise StswinHipError(f"connectivity must be 4 or 8, got {connectivity!r}")
            if instance_skip is None:     # the background, or the remapped ignore label: what `transparent` defaults to
                instance_skip = (classes - 1,) if protocol == "cadis" else (0,)
            instance_skip = tuple(instance_skip)
            if any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 63 for c in instance_skip):
                raise StswinHipError(f"instance_skip holds classes 0 .. 63, got {instance_skip!r}")
            if instance_groups is not None:
                from .utils.instruments import check_groups
                try:
                    instance_groups = check_groups(instance_groups, classes, instance_skip)
                except ValueError as e:
                    raise StswinHipError(str(e)) from e
        if not isinstance(tracks, bool):
            raise StswinHipError(f"tracks must be a bool, got {tracks!r}")
        if not tracks and (track_iou != 100 or track_same_class is not True):
            raise StswinHipError("track_iou and track_same_class belong to tracks=True")
        if isinstance(track_max_gap, bool) or not isinstance(track_max_gap, int) or not 0 <= track_max_gap <= hip.TRACK_MAX_GAP:
            raise StswinHipError(f"track_max_gap must be an int 0 .. {hip.TRACK_MAX_GAP} (frames), got {track_max_gap!r}")
        if not tracks and track_max_gap != 0:
            raise StswinHipError("track_max_gap belongs to tracks=True")
        if tracks:
            if instances is None:
                raise StswinHipError("tracks=True follows the instances from frame to frame: it needs instances=K")
            if isinstance(track_iou, bool) or not isinstance(track_iou, int) or not 0 <= track_iou <= 1000:
                raise StswinHipError(f"track_iou must be an int 0 .. 1000 (thousandths), got {track_iou!r}")
            if not isinstance(track_same_class, bool):
                raise StswinHipError(f"track_same_class must be a bool, got {track_same_class!r}")
        if masks not in (None, "frame", "deferred"):
            raise StswinHipError(f"masks must be None, 'frame' or 'deferred', got {masks!r}")
        if masks is not None and out == "logits":
            raise StswinHipError("masks belongs to out='labels' and out='overlay' (the runs are taken over the label map)")
        if isinstance(mask_runs, bool) or not isinstance(mask_runs, int) or not 1 <= mask_runs <= hip.RLE_MAX_RUNS:
            raise StswinHipError(f"mask_runs must be an int 1 .. {hip.RLE_MAX_RUNS}, got {mask_runs!r}")
        if masks is None and mask_runs != 16384:
            raise StswinHipError("mask_runs belongs to masks='frame' or 'deferred'")
        if confidence not in (None, "frame", "deferred"):
            raise StswinHipError(f"confidence must be None, 'frame' or 'deferred', got {confidence!r}")
        if isinstance(confidence_low, bool) or not isinstance(confidence_low, int) or not 0 <= confidence_low <= 256:
            raise StswinHipError(f"confidence_low must be an int 0 .. 256, got {confidence_low!r}")
        if confidence is None and confidence_low != 128:
            raise StswinHipError("confidence_low belongs to confidence='frame' or 'deferred'")
        if confidence is not None and out == "logits":
            raise StswinHipError("confidence belongs to out='labels' and out='overlay' (it is the probability of the label map's labels)")
        if confidence is not None and not 1 <= classes <= 64:
            raise StswinHipError(f"confidence: the model has {classes} classes, hip.upsample_confidence takes 1 .. 64")
        self.device, self.classes, self.report, self.min_area = device, classes, report, min_area
        self.confidence, self.confidence_low, self.align_corners = confidence, confidence_low, bool(align_corners)
        self.parts, self.instance_groups = parts, instance_groups
        self.clearance, self.clearance_to, self.clearance_max = clearance, clearance_to, clearance_max
        self.clr_ws = None                    # clearance: the workspace (retired ones go where the component map's do)
        self.group_table = self.grouped = None        # instance_groups: the class -> representative table (persistent: a captured graph
        if instance_groups is not None:               # reads it) and the grouped labels, a buffer that only grows, as cc_map does
            from .utils.instruments import group_table
            self.group_table = torch.from_numpy(group_table(instance_groups, classes)).to(device)
        self.masks, self.mask_runs = masks, mask_runs
        self.rle_ws = None                    # masks: the encoder's workspace (retired ones go where the component map's do)
        self.instances, self.connectivity, self.instance_skip = instances, connectivity, instance_skip
        self.tracks, self.track_iou, self.track_same_class = tracks, track_iou, track_same_class
        self.track_max_gap = track_max_gap    # tracks: > 0 takes the tracker with a memory (hip.TrackState(..., max_gap))
        self.cc_map = self.cc_ws = None       # instances: the component map and the workspace ...
        self.cc_retired = []                  # ... and the smaller ones they replaced
        self.state = None                     # tracks: the hip.TrackState of the running sequence (made by the first tracked frame)
        self.order = TrackSequencer()
        self.parked = {}                      # frame -> a released frame that waits for the tracker: cc (a copy of its component map),
        self.pool = []                        # rows [K][12], total [1], ids and started (handed out holding -2), log_row; the copies' pool
        logged = report == "deferred"         # the log holds the columns of what is deferred, nothing else: one row per released frame
        self.log = DeviceLog(device,          # (a parked frame's ids and started later)
                             dict(rows=((instances, 12), torch.int64), total=((), torch.int32)) if logged and instances is not None else {},
                             dict(ids=((instances,), torch.int32), started=((), torch.int32)) if logged and tracks else {},
                             dict(moments=((classes, 10), torch.int64)) if logged else {},
                             dict(runs=((mask_runs, 2), torch.int32), count=((), torch.int32)) if masks == "deferred" else {},
                             dict(class_sums=((classes, 3), torch.int64)) if confidence == "deferred" else {},
                             dict(instance_sums=((instances, 3), torch.int64)) if confidence == "deferred" and instances is not None else {},
                             dict(parts=((instances, classes, 10), torch.int64), contacts=((instances, classes), torch.int64))
                             if parts == "deferred" else {},
                             dict(clearance=((instances, classes, 3), torch.int64)) if clearance == "deferred" else {})

    def reset(self) -> None:
        """The sequence ends: its ordinal in the log, ids restart at 0 (a fill kernel on the stream), what is parked is dropped."""
        self.log.end_sequence()
        if self.state is not None:
            self.state.reset()
        self.pool += [p.cc for p in self.parked.values()]
        self.parked = {}
        self.order.reset()

    def labelled(self, labels: torch.Tensor, frames: Optional[Sequence[int]] = None, steady: bool = False,
                 logits: Optional[torch.Tensor] = None) -> Optional[List[Yield]]:
        """A step's labels [B][*out_size] exist -> what they yield, per clip (None without report, masks and confidence): the moments,
        one launch behind the clearing of their buffer (a fill kernel, also when captured: no memset node), the component launches behind it, and the
        tracker's behind those for clips whose frame indices `frames` names (labels made per clip: the component map is that clip's
        until the next clip's labels) or in the graph's steady step (`steady`: one frame, in frame order); released() tracks the rest.
        The encoder's launches come last: they need nothing from the tracker, so a frame that is parked is encoded here, before the
        next clip's components overwrite the map.  So do the confidence launches, on the `logits` [B][nc][h][w] the labels were made
        from: the map, its sums over the labels and, with instances, over the component map.  And so do the parts launch and the clearance launches, on the
        labels (ungrouped) and the component map."""
        if self.report is None and self.masks is None and self.confidence is None:
            return None
        moments = rows = total = ids = started = None
        if self.report is not None:
            moments = hip.label_moments(labels, self.classes)
        if self.instances is not None:
            rows, total = self._components(labels)
        if steady:
            ids, started = (t[None] for t in self._track_now(self._map(0), rows[0], total))
        y = Yield(moments, rows, total, ids, started)
        ys = [y.clip(b) for b in range(labels.shape[0])]
        if self.tracks and frames is not None:
            ys = [self._track(g, b, c) for b, (g, c) in enumerate(zip(frames, ys))]
        if self.masks is not None:
            B, H, W = labels.shape
            runs, count = self._runs(self.cc_map[:B * H * W].view(B, H, W) if self.instances is not None else labels)
            ys = [c._replace(runs=runs[b:b + 1], count=count[b:b + 1]) for b, c in enumerate(ys)]
        if self.confidence is not None:
            if logits is None:
                raise StswinHipError("internal error: confidence needs the logits the labels were made from")
            B, H, W = labels.shape
            conf = hip.upsample_confidence(logits.contiguous(), labels, self.align_corners)
            sums = hip.confidence_sums(labels, conf, self.classes, self.confidence_low)
            inst = None
            if self.instances is not None:
                inst = hip.confidence_sums(self.cc_map[:B * H * W].view(B, H, W), conf, self.instances, self.confidence_low)
            ys = [c._replace(conf=conf[b:b + 1], class_sums=sums[b:b + 1], instance_sums=None if inst is None else inst[b:b + 1])
                  for b, c in enumerate(ys)]
        if self.parts is not None:
            B, H, W = labels.shape
            pt, ct = hip.instance_parts(labels, self.cc_map[:B * H * W].view(B, H, W), self.instances, self.classes)
            ys = [c._replace(parts=pt[b:b + 1], contacts=ct[b:b + 1]) for b, c in enumerate(ys)]
        if self.clearance is not None:
            B, H, W = labels.shape
            cl = self._clearance(labels, self.cc_map[:B * H * W].view(B, H, W))
            ys = [c._replace(clearance=cl[b:b + 1]) for b, c in enumerate(ys)]
        return ys

    def released(self, frames: Sequence[int], results: list, ys: Optional[List[Yield]]) -> list:
        """The clips of `frames` are released with `results` and what their labels yielded: clips not tracked yet are, in the step's
        order; then report="frame", masks="frame", confidence="frame" and parts="frame" append to each result (on the device), and a
        row is logged when any of them is "deferred".  -> the results."""
        if self.report is None and self.masks is None and self.confidence is None:
            return results
        if self.tracks:
            ys = [y if y.ids is not None else self._track(g, b, y) for b, (g, y) in enumerate(zip(frames, ys))]
        if "frame" in (self.report, self.masks, self.confidence, self.parts, self.clearance):
            results = [y.appended(r, self.report == "frame", self.masks == "frame", self.confidence == "frame", self.parts == "frame",
                                  self.clearance == "frame") for r, y in zip(results, ys)]
        if "deferred" in (self.report, self.masks, self.confidence, self.parts, self.clearance):
            for g, y in zip(frames, ys):
                row = y.logged(self.log, g, g not in self.parked, self.report == "deferred", self.masks == "deferred",
                               self.confidence == "deferred", self.parts == "deferred", self.clearance == "deferred")
                if g in self.parked and self.report == "deferred":
                    self.parked[g].log_row = row
        return results

    def step_is_steady(self, frame: int) -> None:
        """tracks: the graph's steady step holds the tracker's launches, so its frame must be the tracker's next one."""
        at = self.order.next
        if self.state is None or self.order.parked or self.order.release(frame) != [frame]:
            raise StswinHipError(f"internal error: the steady step of frame {frame} found the tracker at frame {at}")

    def _map(self, b: int) -> torch.Tensor:                   # clip b's component map [H][W], a view of the chain's own
        hw = self.hw[0] * self.hw[1]
        return self.cc_map[b * hw:(b + 1) * hw].view(self.hw)

    def _components(self, labels: torch.Tensor):
        """(rows int64 [B][K][12], total int32 [B]) of labels [B][H][W]; with instance_groups of the grouped labels, group_table[labels],
        made by one launch in front (hip.gt_decode, id-coded).  The component map, the grouped labels and the workspace only ever grow,
        so the warm-up frames allocate what the captured step then uses; rows and total are fresh per step (under capture: the graph's)."""
        B, H, W = labels.shape
        if self.group_table is not None:
            if self.grouped is None or self.grouped.numel() < B * H * W:
                if self.grouped is not None:
                    self.cc_retired.append(self.grouped)
                self.grouped = torch.empty(B * H * W, dtype=torch.uint8, device=self.device)
            labels = hip.gt_decode(labels, self.group_table, torch.uint8, out=self.grouped[:B * H * W].view(B, H, W))
        need = hip.label_components_scratch(B, H, W)
        if self.cc_ws is None or self.cc_ws.numel() < need or self.cc_map.numel() < B * H * W:
            self.cc_retired += [t for t in (self.cc_ws, self.cc_map) if t is not None]
            self.cc_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.cc_map = torch.empty(B * H * W, dtype=torch.int32, device=self.device)
        self.hw = (H, W)
        rows = torch.empty(B, self.instances, 12, dtype=torch.int64, device=self.device)
        total = torch.empty(B, dtype=torch.int32, device=self.device)
        hip.label_components(labels, self.classes, self.connectivity, self.instance_skip, self.instances,
                             out=(self.cc_map[:B * H * W].view(B, H, W), rows, total), workspace=self.cc_ws)
        return rows, total

    def _runs(self, maps: torch.Tensor):
        """(runs int32 [B][cap][2], count int32 [B]) of maps [B][H][W], uint8 labels or the int32 component map.  The workspace only
        ever grows, as the component launches' does; runs and count are fresh per step (under capture: the graph's)."""
        need = hip.rle_encode_scratch(*maps.shape)
        if self.rle_ws is None or self.rle_ws.numel() < need:
            if self.rle_ws is not None:
                self.cc_retired.append(self.rle_ws)
            self.rle_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        runs = torch.empty(maps.shape[0], self.mask_runs, 2, dtype=torch.int32, device=self.device)
        count = torch.empty(maps.shape[0], dtype=torch.int32, device=self.device)
        return hip.rle_encode(maps, self.mask_runs, out=(runs, count), workspace=self.rle_ws)

    def _clearance(self, labels: torch.Tensor, components: torch.Tensor) -> torch.Tensor:
        """clearance int64 [B][K][nc][3] of labels and components [B][H][W].  The workspace only ever grows, as the component launches'
        does; the result is fresh per step (under capture: the graph's)."""
        need = hip.instance_clearance_scratch(*labels.shape, self.classes, self.instances)
        if self.clr_ws is None or self.clr_ws.numel() < need:
            if self.clr_ws is not None:
                self.cc_retired.append(self.clr_ws)
            self.clr_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(labels.shape[0], self.instances, self.classes, 3, dtype=torch.int64, device=self.device)
        return hip.instance_clearance(labels, components, self.instances, self.classes, self.clearance_to, self.clearance_max, out=out,
                                      workspace=self.clr_ws)

    def _track(self, frame: int, b: int, y: Yield) -> Yield:
        """y with the ids [1][K] and started [1][1] of released frame `frame`, whose components clip b of the map holds.  A frame the
        sequencer parks has its map copied out and its tensors handed out holding -2; the call that tracks its predecessor tracks it."""
        cc = self._map(b)
        if self.state is None or (self.state.H, self.state.W) != tuple(cc.shape):
            self.state = hip.TrackState(cc.shape[0], cc.shape[1], self.instances, self.device, max_gap=self.track_max_gap)
        ids = torch.empty(self.instances, dtype=torch.int32, device=self.device)
        started = torch.empty(1, dtype=torch.int32, device=self.device)
        now = self.order.release(frame)
        if not now:
            keep = self.pool.pop() if self.pool and self.pool[-1].shape == cc.shape else torch.empty_like(cc)
            keep.copy_(cc)
            ids.fill_(-2)
            started.fill_(-2)
            self.parked[frame] = SimpleNamespace(cc=keep, rows=y.rows[0], total=y.total, ids=ids, started=started, log_row=None)
        else:
            self._track_now(cc, y.rows[0], y.total, ids, started)
            for g in now[1:]:
                p = self.parked.pop(g)
                self._track_now(p.cc, p.rows, p.total, p.ids, p.started)
                self.pool.append(p.cc)
                if p.log_row is not None:
                    self.log.write(p.log_row, ids=p.ids, started=p.started)
        return y._replace(ids=ids[None], started=started[None])

    def _track_now(self, cc, rows, total, *out):
        return hip.track_instances(cc, rows, total, self.state, self.track_iou, self.track_same_class, self.min_area, out=out or None)
