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

Or from what the files hold, with no mask on the host at all: the raw panoptic id map and the raw depth map of each frame plus the
augmentation's parameters (csrc/ph_gtseg.hip: `ph_gt_segments` finds the segments and their boxes, `ph_gt_index_maps` takes the id map
and the depth through resize, flip, crop and pad, and `ph_gt_prepare` runs on the result where it lies).

    tables = gt.segment_tables(raw_maps, class_map)                              # depends on the files alone: a loader may cache it
    prepared = gt.prepare_gt_from_panoptic(raw_maps, raw_depth, aug, num_thing_classes, pad_hw, class_map, tables=tables, want_hard=True)
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
    depth = None
    if gt_depth is not None:
        depth = gt_depth if torch.is_tensor(gt_depth) else torch.from_numpy(np.ascontiguousarray(gt_depth))
        depth = depth.to(dev, non_blocking=True).float().reshape(B, Hp, Wp).contiguous()
    return _prepared(_up(seg, dev), gt_labels, gt_instance_ids, depth, (Hs, Ws), (Hp, Wp), (aH, aW), num_thing_classes, nearest, want_hard)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)


def _prepared(seg, gt_labels, gt_instance_ids, depth, src_hw, pad_hw, assign_hw, num_thing_classes, nearest, want_hard):
    """the row tables of the label lists, the `ph_gt_prepare` call on device index maps seg [B, Hs, Ws] and depth [B, Hp, Wp] (or None),
    and the PreparedGT around its buffers"""
    dev = seg.device
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
    bufs = gt_prepare(seg, _up(rows, dev), [l.size for l in labs], depth, src_hw, pad_hw, assign_hw, gmax, smax, nearest=nearest,
                      want_hard=(bool(want_hard), False))
    return PreparedGT(bufs, G, S, labels_h, sem_cls_h, ids_h, _up(small, dev))


# ---- from the dataset's panoptic id maps (csrc/ph_gtseg.hip): the loader keeps `ps_id` as the file holds it and drops the bitmask stack --

class SegmentTable:
    """one frame's segments at file resolution, what loading.py:201-220 and bitmasks2bboxes leave: ids int64 [n] (the mapped panoptic
    ids, ascending: `gt_instance_ids`; `ids // divisor` is `gt_labels`), boxes fp32 [n][4] (`gt_bboxes`: xmin, ymin, xmax, ymax,
    inclusive), areas int64 [n]"""

    def __init__(self, ids, boxes, areas):
        self.ids, self.boxes, self.areas = ids, boxes, areas


_STATUS_WORDS = ((_lib.PH_GTSEG_ETOOMANY, f"more than {_lib.PH_GTPREP_MAX_SEGMENTS} segments"),
                 (_lib.PH_GTSEG_EUNMAPPED, "an id whose class the class map sends to -1"),
                 (_lib.PH_GTSEG_EOUTSIDE, "an id whose class lies outside the class map"))


def _raw_maps(raw, dev, what):
    """host or device id maps -> (contiguous device tensor [F, Hs, Ws], PH_GTSEG_* dtype).  uint16 travels as int16 bits."""
    if not torch.is_tensor(raw):
        a = np.asarray(raw) if not isinstance(raw, (list, tuple)) else np.stack([np.asarray(r) for r in raw])
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        elif a.dtype != np.int32:
            raise ValueError(f"{what}: int32 or uint16, got {a.dtype}")
        raw = torch.from_numpy(np.ascontiguousarray(a))
    if raw.dtype not in (torch.int32, torch.int16, getattr(torch, "uint16", torch.int16)):
        raise ValueError(f"{what}: int32 or uint16 (int16 bits), got {raw.dtype}")
    if raw.dim() != 3 or raw.shape[0] == 0:
        raise ValueError(f"{what}: [frames][Hs][Ws] with at least one frame, got shape {tuple(raw.shape)}")
    raw = raw.to(dev, non_blocking=True).contiguous()
    if not raw.is_cuda:
        raise _lib.PolyheadError(f"{what}: the maps must live on the GPU: libpolyhead has no CPU path")
    return raw, _lib.PH_GTSEG_I32 if raw.dtype == torch.int32 else _lib.PH_GTSEG_U16


def _class_map(class_map):
    cm = np.ascontiguousarray(np.asarray(class_map).reshape(-1), dtype=np.int32)
    return cm, cm.ctypes.data_as(C.POINTER(C.c_int32))


def gt_segments(raw, dtype, class_map, raw_divisor, divisor, no_obj_class, tables=None, status=None, workspace=None):
    """one raw `ph_gt_segments` call per 64 frames on device maps [F, Hs, Ws] -> (tables int32 [F, PH_GTSEG_TABLE_WORDS], status int32
    [F]) on the device; no host read.  tables / status / workspace: buffers to write into instead of new ones."""
    F_, Hs, Ws = raw.shape
    cm, cmp_ = _class_map(class_map)
    lib = _lib.load()
    if tables is None:
        tables = torch.empty((F_, _lib.PH_GTSEG_TABLE_WORDS), dtype=torch.int32, device=raw.device)
    if status is None:
        status = torch.empty(F_, dtype=torch.int32, device=raw.device)
    for f0 in range(0, F_, _lib.PH_GTPREP_MAX_FRAMES):
        n = min(F_, f0 + _lib.PH_GTPREP_MAX_FRAMES) - f0
        need = lib.ph_gt_segments_workspace_bytes(n, cm.size, raw_divisor)
        ws = workspace
        if ws is None and need:
            ws = torch.empty(need, dtype=torch.uint8, device=raw.device)
        _lib.check(lib.ph_gt_segments(_lib.ptr(raw[f0:f0 + n]), dtype, n, Hs, Ws, cmp_, cm.size, raw_divisor, divisor, no_obj_class,
                                      _lib.ptr(tables[f0:f0 + n]), _lib.ptr(status[f0:f0 + n]), _lib.ptr(ws), ws.numel() if ws is not None else 0,
                                      _lib.stream_ptr()), "ph_gt_segments")
    return tables, status


def segment_tables(raw_maps, class_map, raw_divisor=1000, divisor=10000, no_obj_class=255, device="cuda"):
    """raw_maps: [frames][Hs][Ws] int32 or uint16, host or device, the panoptic ids as the file holds them (class * raw_divisor +
    instance); class_map: raw class -> training class, -1 for a class the dataset does not have, the no-object class to no_obj_class
    (to_coco, datasets/cityscapes_dvps.py:89-109).  Runs `ph_gt_segments` and makes ONE small download (6 KB a frame, the call's only
    synchronisation) -> per frame a SegmentTable.  ValueError, naming the frame, when a frame has more than 254 segments or an id
    outside the class map.  A frame's table depends on the file alone -- not on the augmentation -- so a loader may compute it once per
    file and cache it (`prepare_gt_from_panoptic(..., tables=...)`)."""
    raw, dtype = _raw_maps(raw_maps, torch.device(device), "segment_tables")
    tables, status = gt_segments(raw, dtype, class_map, raw_divisor, divisor, no_obj_class)
    host = torch.cat((status[:, None], tables), 1).cpu().numpy()
    out = []
    for f, row in enumerate(host):
        if row[0]:
            why = "; ".join(w for bit, w in _STATUS_WORDS if row[0] & bit)
            raise ValueError(f"segment_tables: frame {f}: {why} (status {int(row[0])})")
        t = row[2:2 + int(row[1]) * _lib.PH_GTSEG_ROW_WORDS].reshape(-1, _lib.PH_GTSEG_ROW_WORDS)
        out.append(SegmentTable(t[:, 0].astype(np.int64), t[:, 1:5].astype(np.float32), t[:, 5].astype(np.int64)))
    return out


def nearest_index(old, new):
    """the source index of every destination index of a nearest resize old -> new, int32 [new]: OpenCV's INTER_NEAREST,
    min(floor(dst * (1.0 / (double(new) / old))), old - 1) in double"""
    inv = 1.0 / (float(new) / float(old))
    return np.minimum(np.floor(np.arange(new, dtype=np.float64) * inv), old - 1).astype(np.int32)


def nearest_tables(src_hw, resized_hw, flip, crop_offset, crop_hw):
    """host: the resize to resized_hw, the horizontal flip (bool) and the crop (offset (y, x), size (h, w), clipped by the resized image
    as the reference's slice is) of one frame composed into two index tables -> (src_y int32 [Hc], src_x int32 [Wc], scale_factor fp32
    (w, h, w, h) as mmdet's Resize leaves it, (Hc, Wc)).  crop_offset = None: no crop.

    The resize rule is OpenCV's INTER_NEAREST as its documentation states it (`nearest_index`); it is RESTATED here, not checked against
    the library.  A loader that has cv2 gets the exact tables by resizing an `arange` row and column with the call it resizes its
    images with; `ph_gt_index_maps` takes the tables and not the rule for that reason."""
    (H, W), (nh, nw) = src_hw, resized_hw
    sy, sx = nearest_index(H, nh), nearest_index(W, nw)
    if flip:
        sx = sx[::-1]
    if crop_offset is not None:
        (oy, ox), (ch, cw) = crop_offset, crop_hw
        sy, sx = sy[oy:oy + ch], sx[ox:ox + cw]
    scale = np.array([nw / W, nh / H, nw / W, nh / H], dtype=np.float32)
    return np.ascontiguousarray(sy), np.ascontiguousarray(sx), scale, (int(sy.size), int(sx.size))


def transform_boxes(boxes, scale_factor, resized_hw, flip, crop_offset, crop_hw):
    """the file-resolution boxes of a SegmentTable through the augmentation, in fp32 numpy as the reference: mmdet's `_resize_bboxes`
    (times scale_factor, clipped to the resized shape), `bbox_flip` (horizontal) and the crop of datasets/pipelines/transforms.py:232-248
    (shifted, clipped to the cropped shape) -> (boxes fp32 [n][4], valid bool [n]).  valid is the crop's test -- the BOX keeps a
    positive width and height -- so a crop never keeps a segment one pixel wide or high in the file, and a kept one may have no pixel
    left in the crop.  crop_offset = None: no crop, every segment is valid."""
    nh, nw = resized_hw
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4) * np.asarray(scale_factor, dtype=np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, nw)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, nh)
    if flip:
        f = b.copy()
        f[:, 0] = nw - b[:, 2]
        f[:, 2] = nw - b[:, 0]
        b = f
    if crop_offset is None:
        return b, np.ones(b.shape[0], bool)
    (oy, ox), (ch, cw) = crop_offset, crop_hw
    b = b - np.array([ox, oy, ox, oy], dtype=np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, min(cw, nw - ox))
    b[:, 1::2] = np.clip(b[:, 1::2], 0, min(ch, nh - oy))
    return b, (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])


def gt_index_maps(raw, dtype, raw_depth, class_map, raw_divisor, divisor, no_obj_class, kept_ids, src_y, src_x, pad_hw, scale_mean=None,
                  depth_div=256.0, depth_max=80.0, out=None):
    """one raw `ph_gt_index_maps` call per 64 frames.  raw [F, Hs, Ws] and raw_depth (uint16 as int16 bits, or None) on the device;
    kept_ids: per frame the host list of kept mapped ids, ascending; src_y int32 [F, Hc] and src_x int32 [F, Wc] on the host (-1:
    none); scale_mean host fp32 [F].  Uploads the three tables in one copy -> (seg uint8 [F, Hc, Wc], depth fp32 [F, Hp, Wp] or None)
    on the device; `out` = (seg, depth) supplies the buffers."""
    F_, Hs, Ws = raw.shape
    dev = raw.device
    src_y, src_x = np.ascontiguousarray(src_y, dtype=np.int32), np.ascontiguousarray(src_x, dtype=np.int32)
    if src_y.ndim != 2 or src_x.ndim != 2 or src_y.shape[0] != F_ or src_x.shape[0] != F_ or len(kept_ids) != F_:
        raise ValueError("gt_index_maps: one kept list, src_y row and src_x row per frame")
    (Hc, Wc), (Hp, Wp) = (src_y.shape[1], src_x.shape[1]), pad_hw
    kept = np.zeros((F_, 256), np.int32)
    kept_n = np.zeros(F_, np.int32)
    for f, k in enumerate(kept_ids):
        k = np.asarray(k).reshape(-1)
        if k.size > _lib.PH_GTPREP_MAX_SEGMENTS:
            raise ValueError(f"gt_index_maps: frame {f} keeps {k.size} segments, an index map holds at most {_lib.PH_GTPREP_MAX_SEGMENTS}")
        if k.size > 1 and not (np.diff(k) > 0).all():
            raise ValueError(f"gt_index_maps: frame {f}: the kept ids must ascend")
        kept[f, :k.size], kept_n[f] = k, k.size
    host = np.concatenate((kept.ravel(), src_y.ravel(), src_x.ravel()))
    d = _up(host, dev)
    kept_d, sy_d, sx_d = d[:kept.size], d[kept.size:kept.size + src_y.size], d[kept.size + src_y.size:]
    cm, cmp_ = _class_map(class_map)
    seg, depth = out if out is not None else (None, None)
    if seg is None:
        seg = torch.empty((F_, Hc, Wc), dtype=torch.uint8, device=dev)
    if raw_depth is not None:
        if raw_depth.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or tuple(raw_depth.shape) != (F_, Hs, Ws) or \
                not raw_depth.is_contiguous() or raw_depth.device != dev:
            raise ValueError(f"gt_index_maps: raw_depth must be contiguous uint16 (int16 bits) [{F_}, {Hs}, {Ws}] on {dev}")
        if depth is None:
            depth = torch.empty((F_, Hp, Wp), dtype=torch.float32, device=dev)
        sm = np.ones(F_, np.float32) if scale_mean is None else np.ascontiguousarray(scale_mean, dtype=np.float32).reshape(F_)
    lib = _lib.load()
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    for f0 in range(0, F_, _lib.PH_GTPREP_MAX_FRAMES):
        n = min(F_, f0 + _lib.PH_GTPREP_MAX_FRAMES) - f0
        hy, hx, hn = src_y[f0:f0 + n], src_x[f0:f0 + n], kept_n[f0:f0 + n]
        _lib.check(lib.ph_gt_index_maps(
            _lib.ptr(raw[f0:f0 + n]), dtype, _lib.ptr(raw_depth[f0:f0 + n]) if raw_depth is not None else None, n, Hs, Ws, cmp_, cm.size,
            raw_divisor, divisor, no_obj_class, _lib.ptr(kept_d[f0 * 256:]), i32(hn), C.c_void_p(hy.ctypes.data), C.c_void_p(hx.ctypes.data),
            _lib.ptr(sy_d[f0 * Hc:]), _lib.ptr(sx_d[f0 * Wc:]), Hc, Wc, Hp, Wp, depth_div, depth_max,
            sm[f0:f0 + n].ctypes.data_as(C.POINTER(C.c_float)) if raw_depth is not None else None, _lib.ptr(seg[f0:f0 + n]),
            _lib.ptr(depth[f0:f0 + n]) if raw_depth is not None else None, _lib.stream_ptr()), "ph_gt_index_maps")
    return seg, depth if raw_depth is not None else None


def prepare_gt_from_panoptic(raw_maps, raw_depth, aug, num_thing_classes, pad_hw, class_map, raw_divisor=1000, divisor=10000,
                             no_obj_class=255, mask_assign_stride=4, want_hard=False, nearest=False, tables=None, depth_div=256.0,
                             depth_max=80.0, device="cuda"):
    """The step's ground truth from what the files hold.  raw_maps: [B][Hs][Ws] int32 / uint16 panoptic id maps, raw_depth: [B][Hs][Ws]
    uint16 or None, host or device; aug: per frame (resized_hw, flip, crop_offset, crop_hw) as `nearest_tables` takes them; class_map,
    raw_divisor, divisor, no_obj_class as `segment_tables`; tables: the frames' cached SegmentTables.

    1. the segment tables, cached or computed (`segment_tables`: the one synchronisation; none when `tables` is given);  2. on the host
    the boxes through the augmentation and the reference's filter (`transform_boxes`);  3. the kept ids -- they are `gt_instance_ids`, and
    `// divisor` gives `gt_labels`;  4. `ph_gt_index_maps`: the id maps and the depth through the augmentation;  5. `ph_gt_prepare` on
    those device maps; nothing is uploaded twice.  -> PreparedGT, as `prepare_gt` on the loader's bitmask path gives it."""
    dev = torch.device(device)
    raw, dtype = _raw_maps(raw_maps, dev, "prepare_gt_from_panoptic")
    B, Hs, Ws = raw.shape
    if B == 0 or len(aug) != B or (tables is not None and len(tables) != B):
        raise ValueError("prepare_gt_from_panoptic: one augmentation (and cached table) per frame")
    depth_d = None
    if raw_depth is not None:
        depth_d, ddt = _raw_maps(raw_depth, dev, "prepare_gt_from_panoptic: raw_depth")
        if ddt != _lib.PH_GTSEG_U16 or tuple(depth_d.shape) != (B, Hs, Ws):
            raise ValueError(f"prepare_gt_from_panoptic: raw_depth is uint16 [{B}][{Hs}][{Ws}]")
    if tables is None:
        tables = segment_tables(raw, class_map, raw_divisor, divisor, no_obj_class, device=dev)
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    kept, sys_, sxs, means = [], [], [], []
    for tab, (resized_hw, flip, crop_offset, crop_hw) in zip(tables, aug):
        sy, sx, scale, _ = nearest_tables((Hs, Ws), resized_hw, flip, crop_offset, crop_hw)
        _, valid = transform_boxes(tab.boxes, scale, resized_hw, flip, crop_offset, crop_hw)
        kept.append(tab.ids[valid])
        sys_.append(sy); sxs.append(sx); means.append(scale.mean())
    Hc, Wc = max(s.size for s in sys_), max(s.size for s in sxs)
    if Hc > Hp or Wc > Wp:
        raise ValueError(f"prepare_gt_from_panoptic: the augmented frames are {Hc} x {Wc}, above pad_hw {Hp} x {Wp}")
    src_y, src_x = np.full((B, Hc), -1, np.int32), np.full((B, Wc), -1, np.int32)          # a smaller frame: no pixel beyond it
    for b in range(B):
        src_y[b, :sys_[b].size], src_x[b, :sxs[b].size] = sys_[b], sxs[b]
    seg, depth = gt_index_maps(raw, dtype, depth_d, class_map, raw_divisor, divisor, no_obj_class, kept, src_y, src_x, (Hp, Wp),
                               scale_mean=np.asarray(means, np.float32), depth_div=depth_div, depth_max=depth_max)
    aH, aW = Hp // mask_assign_stride, Wp // mask_assign_stride
    return _prepared(seg, [k // divisor for k in kept], kept, depth, (Hc, Wc), (Hp, Wp), (aH, aW), num_thing_classes, nearest, want_hard)
