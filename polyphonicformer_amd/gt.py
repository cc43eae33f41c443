"""A training step's ground truth from what a loader can cheaply hand over: one segment-index map per frame.

The reference (polyphonic_former_video.py:103-183, polyphonic_former.py:60-95) uploads every frame's bitmasks as fp32
`[G][H][W]` (`BitmapMasks.to_tensor`), pads, interpolates down by the assign stride and splits things from stuff; `losses.StepGT`
then derives a contiguous copy, a hardened copy, the valid map and a zero-padded stack with torch passes.  The loader's masks of a
frame are disjoint, so the stack is one byte per pixel -- the index of the pixel's segment in the loader's list, 255 where there is
none -- and every tensor the step holds is a function of that map, the label list and the depth map: one `ph_gt_prepare` call
(csrc/ph_gtprep.hip).

    maps = [gt.index_map_from_bitmasks(m) for m in gt_masks]                     # loader worker, numpy
    prepared = gt.prepare_gt(maps, gt_labels, pad_hw, num_thing_classes, gt_depth=depth, gt_instance_ids=ids, want_hard=True)
    step.forward_backward_prepared(feats, img_metas, prepared)                   # train.TrainStep / train.VideoTrainStep
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import losses as Lo

NO_SEGMENT = 255


def index_map_from_bitmasks(masks):
    """host numpy, for a loader worker.  masks: uint8 / bool [G][H][W] or a BitmapMasks-like object with `.masks` -> uint8 [H][W], the
    index of the mask that covers the pixel or 255.  A mask that is empty (cropped away) stays in the list: its index does not occur
    in the map.  ValueError when two masks overlap or there are more than 254."""
    m = np.asarray(getattr(masks, "masks", masks))
    if m.ndim != 3:
        raise ValueError(f"index_map_from_bitmasks: masks must be [G][H][W], got shape {m.shape}")
    if m.shape[0] > _lib.PH_GTPREP_MAX_SEGMENTS:
        raise ValueError(f"index_map_from_bitmasks: {m.shape[0]} masks, an index map holds at most {_lib.PH_GTPREP_MAX_SEGMENTS}")
    on = m != 0
    if m.shape[0] and int(on.sum(0, dtype=np.int32).max()) > 1:
        raise ValueError("index_map_from_bitmasks: two masks overlap; an index map needs disjoint masks")
    out = np.full(m.shape[1:], NO_SEGMENT, np.uint8)
    for i in range(m.shape[0]):
        out[on[i]] = i
    return out


def split_rows(labels, num_thing_classes):
    """polyphonic_former_video.py:125-133 on one frame's host label list: -> (indices of the things, indices of the stuff segments),
    both in loader order.  A negative label is a segment the loader dropped from its list without renumbering the map."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    if lab.size > _lib.PH_GTPREP_MAX_SEGMENTS:
        raise ValueError(f"prepare_gt: {lab.size} segments in a frame, an index map holds at most {_lib.PH_GTPREP_MAX_SEGMENTS}")
    return np.flatnonzero((lab >= 0) & (lab < num_thing_classes)), np.flatnonzero(lab >= num_thing_classes)


def row_table(labels, num_thing_classes, gmax):
    """the `row_of` table of one frame (include/polyhead.h ph_gt_prepare): int32 [256], things to rows 0 .., stuff to rows gmax ..,
    everything else -1"""
    th, st = split_rows(labels, num_thing_classes)
    row = np.full(256, -1, np.int32)
    row[th] = np.arange(th.size, dtype=np.int32)
    row[st] = gmax + np.arange(st.size, dtype=np.int32)
    return row


def gt_prepare(seg, row_of, nseg, depth, src_hw, pad_hw, assign_hw, gmax, smax, nearest=False, want_hard=(False, False), out=None):
    """one raw `ph_gt_prepare` call.  seg uint8 [F, Hs, Ws], row_of int32 [F, 256] and depth fp32 [F, Hp, Wp] (or None) on the device,
    nseg host ints.  -> dict(things, stuff, things_hard, stuff_hard, valid, depth); `out` supplies buffers to write into instead of
    new ones."""
    F_, (Hs, Ws), (Hp, Wp), (aH, aW) = len(nseg), src_hw, pad_hw, assign_hw
    dev = seg.device
    if not seg.is_cuda:
        raise _lib.PolyheadError("gt_prepare: the index maps must live on the GPU: libpolyhead has no CPU path")
    if seg.dtype != torch.uint8 or not seg.is_contiguous() or tuple(seg.shape) != (F_, Hs, Ws):
        raise ValueError(f"gt_prepare: seg must be contiguous uint8 [{F_}, {Hs}, {Ws}]")
    if row_of.dtype != torch.int32 or not row_of.is_contiguous() or tuple(row_of.shape) != (F_, 256):
        raise ValueError(f"gt_prepare: row_of must be contiguous int32 [{F_}, 256]")
    if depth is not None and (depth.dtype != torch.float32 or not depth.is_contiguous() or tuple(depth.shape) != (F_, Hp, Wp)):
        raise ValueError(f"gt_prepare: depth must be contiguous fp32 [{F_}, {Hp}, {Wp}]")
    o = dict(out or {})
    shapes = dict(things=(F_, gmax, aH, aW), stuff=(F_, smax, aH, aW), things_hard=(F_, gmax, aH, aW) if want_hard[0] else None,
                  stuff_hard=(F_, smax, aH, aW) if want_hard[1] else None, valid=(F_, aH, aW), depth=(F_, aH, aW) if depth is not None else None)
    for k, shp in shapes.items():
        if shp is None:
            o[k] = None
        elif o.get(k) is None:
            o[k] = torch.empty(shp, dtype=torch.float32, device=dev)
        elif tuple(o[k].shape) != shp or o[k].dtype != torch.float32 or not o[k].is_contiguous() or o[k].device != dev:
            raise ValueError(f"gt_prepare: out['{k}'] must be contiguous fp32 {shp} on {dev}")
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    for f0 in range(0, F_, _lib.PH_GTPREP_MAX_FRAMES):
        f1 = min(F_, f0 + _lib.PH_GTPREP_MAX_FRAMES)
        s = lambda t: None if t is None else t[f0:f1]
        _lib.check(_lib.load().ph_gt_prepare(
            _lib.ptr(seg[f0:f1]), _lib.ptr(row_of[f0:f1]), (C.c_int32 * (f1 - f0))(*[int(n) for n in nseg[f0:f1]]), p(s(depth)), f1 - f0, Hs, Ws,
            Hp, Wp, aH, aW, gmax, smax, _lib.PH_GTBOX_NEAREST if nearest else _lib.PH_GTBOX_BILINEAR, p(s(o["things"])), p(s(o["stuff"])),
            p(s(o["things_hard"])), p(s(o["stuff_hard"])), _lib.ptr(s(o["valid"])), p(s(o["depth"])), _lib.stream_ptr()), "ph_gt_prepare")
    return o


class PreparedGT:
    """what `prepare_gt` leaves on the device, and the lists the reference has at polyphonic_former_video.py:185 as views of it
    (nothing is copied): gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, gt_instance_ids (filtered to things, :127)."""

    def __init__(self, bufs, G, S, labels_h, sem_cls_h, ids_h, small_dev):
        self.things, self.stuff, self.things_hard = bufs["things"], bufs["stuff"], bufs["things_hard"]
        self.valid, self.depth = bufs["valid"], bufs["depth"]
        self.B, self.G, self.S = len(G), list(G), list(S)
        self.H, self.W = self.valid.shape[-2:]
        self.labels_h, self.sem_cls_h, self.ids_h = labels_h, sem_cls_h, ids_h
        # the small integer lists in one int64 device tensor: labels of the things, classes of the stuff, instance ids, per frame each
        parts = torch.split(small_dev, self.G + self.S + (self.G if ids_h is not None else []))
        B = self.B
        self.gt_labels, self.gt_sem_cls = list(parts[:B]), list(parts[B:2 * B])
        self.gt_instance_ids = list(parts[2 * B:]) if ids_h is not None else None
        self.gt_masks = [self.things[b, :self.G[b]] for b in range(B)]
        self.gt_sem_seg = [self.stuff[b, :self.S[b]] for b in range(B)]
        self.gt_depth = None if self.depth is None else self.depth[:, None]

    def step_gt(self, hard, with_stuff=True):
        """the `losses.StepGT` of the prepared buffers (hardened things masks when `hard`): no torch pass over the masks, no
        device-to-host read.  A new object per call: it collects one step's status words.  with_stuff=False: the things alone, as
        the video step holds its reference frames -- `StepGT(masks, labels, None, None, None, False)` in every field but one: `valid`
        stays the prepared map, which marks the pixels of things OR stuff, where the list form marks the things alone (a things-only
        map would be a pass over the masks).  The track branch, that form's user, matches over all pixels and reads no valid map
        (train.track_sample); do not hand the object to a loss that does."""
        if hard and self.things_hard is None:
            raise ValueError("PreparedGT.step_gt(True): the hardened masks were not prepared; call prepare_gt(..., want_hard=True)")
        return Lo.StepGT.from_prepared(
            self.things_hard if hard else self.things, self.G, self.labels_h, self.gt_labels, self.valid,
            stuff=self.stuff if with_stuff else None, S=self.S, sem_cls_h=self.sem_cls_h, depth=self.depth if with_stuff else None)


def prepare_gt(index_maps, gt_labels, pad_hw, num_thing_classes, mask_assign_stride=4, gt_depth=None, gt_instance_ids=None, want_hard=False,
               nearest=False, device="cuda"):
    """index_maps: per frame a host uint8 [Hs][Ws] map (`index_map_from_bitmasks`; sizes may differ between frames, none above
    pad_hw); gt_labels / gt_instance_ids: per frame the loader's host arrays, one entry per segment; gt_depth: [B][1][Hp][Wp] or
    [B][Hp][Wp] at the padded size, host or device.  Builds the row tables on the host (polyphonic_former_video.py:125-133: labels
    < num_thing_classes are things rows in loader order, the rest stuff rows in loader order; a negative label maps to no row),
    uploads maps and tables and makes one `ph_gt_prepare` call.  nearest: the semantic_kitti mode of :122.  -> PreparedGT"""
    dev = torch.device(device)
    B = len(index_maps)
    if B == 0 or len(gt_labels) != B or (gt_instance_ids is not None and len(gt_instance_ids) != B):
        raise ValueError("prepare_gt: one index map, label list and id list per frame")
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    aH, aW = Hp // mask_assign_stride, Wp // mask_assign_stride                                # :104-105
    maps = [np.asarray(m) for m in index_maps]
    for m in maps:
        if m.ndim != 2 or m.dtype != np.uint8:
            raise ValueError("prepare_gt: an index map is uint8 [Hs][Ws]")
    Hs, Ws = max(m.shape[0] for m in maps), max(m.shape[1] for m in maps)
    if all(m.shape == (Hs, Ws) for m in maps):
        seg = np.stack(maps)
    else:                                                                                      # frames of different sizes: 255 beyond each
        seg = np.full((B, Hs, Ws), NO_SEGMENT, np.uint8)
        for b, m in enumerate(maps):
            seg[b, :m.shape[0], :m.shape[1]] = m
    labs = [np.asarray(l).reshape(-1).astype(np.int64) for l in gt_labels]
    split = [split_rows(l, num_thing_classes) for l in labs]
    G, S = [int(t.size) for t, _ in split], [int(s.size) for _, s in split]
    gmax, smax = max(max(G), 1), max(S)                                                        # StepGT.pad has at least one row
    rows = np.stack([row_table(l, num_thing_classes, gmax) for l in labs])
    labels_h = [l[t] for l, (t, _) in zip(labs, split)]
    sem_cls_h = [l[s] for l, (_, s) in zip(labs, split)]
    ids_h = None
    if gt_instance_ids is not None:
        ids_h = [np.asarray(i).reshape(-1).astype(np.int64)[t] for i, (t, _) in zip(gt_instance_ids, split)]       # :127
    small = np.concatenate(labels_h + sem_cls_h + (ids_h or []) + [np.zeros(0, np.int64)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
    depth = None
    if gt_depth is not None:
        depth = gt_depth if torch.is_tensor(gt_depth) else torch.from_numpy(np.ascontiguousarray(gt_depth))
        depth = depth.to(dev, non_blocking=True).float().reshape(B, Hp, Wp).contiguous()
    bufs = gt_prepare(up(seg), up(rows), [l.size for l in labs], depth, (Hs, Ws), (Hp, Wp), (aH, aW), gmax, smax, nearest=nearest,
                      want_hard=(bool(want_hard), False))
    return PreparedGT(bufs, G, S, labels_h, sem_cls_h, ids_h, up(small))
