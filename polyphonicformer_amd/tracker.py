"""The trackers of the video association step (the consumer of the one multi-GPU exchange):
drop-in for `QuasiDenseEmbedTracker` (polyphonic/video/qdtrack/trackers/quasi_dense_embed_tracker.py:8-207) in three forms.

The tracker is *host logic*: stateful, strictly sequential in frame order, data-dependent control flow over
<= max_per_img detections and a memory of a few hundred rows.  The array form keeps that memory as a struct of arrays
(`_TrackTable`) and formulates de-duplication, affinity and greedy assignment as array operations; constructor
kwargs, the `match(bboxes, labels, track_feats, frame_id)` signature / return value and the registry name are the
reference's, and the integer ids are pinned to the reference class's own output (tests/golden/tracker.npz).  With the
embeddings on a GPU the same class hands each frame to `NativeHostTracker` (csrc/ph_tracker.hip: bookkeeping in C++, the
memory in a device pool); `NativeDeviceTracker` (csrc/ph_dtracker.hip) keeps the bookkeeping on the device too, and
`NativeDeviceTrackerBank` is S of those in one buffer, one frame of each per launch sequence (live cameras).
With frames sharded over GPUs (`dist.shard_frames`) every rank all-gathers the per-frame records
(`dist.allgather_track_records`) and replays `match` in frame order; integer track ids are then identical to the
single-process run (`replay_tracking`, tests/test_tracker.py and tests/test_dist_gloo.py)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .engine import _OwnsHandles, _cfg_error
from .registry import Registry

TRACKERS = Registry("trackers")
MATCH_METRICS = {"bisoftmax": 0, "softmax": 1, "cosine": 2}       # ph_tracker_cfg.metric / ph_track_affinity's metric code


def painted_ids(ids):
    """the ids `match` returns as they are painted onto the masks (polyphonic_former_video.py:399-402): ids + 1, then -1 -> 0.
    numpy or torch; a new array"""
    ids = ids + 1
    ids[ids == -1] = 0
    return ids


def _idx_to(dev, idx):
    """a host index tensor to the device the embeddings live on: through pinned memory and asynchronously when that is a GPU
    (six such transfers per frame in `match`; pageable ones cost 30-100 us each on the GPU box), a no-op on the CPU"""
    if torch.device(dev).type != "cuda":
        return idx
    return idx.pin_memory().to(dev, non_blocking=True)


def bbox_overlaps(b1, b2, eps=1e-6):
    """IoU matrix of xyxy boxes [n,4] x [m,4] (what mmdet.core.bbox_overlaps(mode='iou') returns)"""
    n, m = b1.shape[0], b2.shape[0]
    if n == 0 or m == 0:
        return b1.new_zeros((n, m))
    x1 = torch.maximum(b1[:, None, 0], b2[None, :, 0])
    y1 = torch.maximum(b1[:, None, 1], b2[None, :, 1])
    x2 = torch.minimum(b1[:, None, 2], b2[None, :, 2])
    y2 = torch.minimum(b1[:, None, 3], b2[None, :, 3])
    inter = (x2 - x1).clamp(min=0) * (y2 - y1).clamp(min=0)
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    return inter / (a1[:, None] + a2[None, :] - inter).clamp(min=eps)


def _iou_np(b1, b2, eps=1e-6):
    """`bbox_overlaps` on numpy float32 arrays: the same fp32 operations in the same order (bit-identical values), at numpy's
    per-call cost -- the tracker's bookkeeping is ~60 tiny array operations per frame"""
    n, m = b1.shape[0], b2.shape[0]
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=np.float32)
    x1 = np.maximum(b1[:, None, 0], b2[None, :, 0])
    y1 = np.maximum(b1[:, None, 1], b2[None, :, 1])
    x2 = np.minimum(b1[:, None, 2], b2[None, :, 2])
    y2 = np.minimum(b1[:, None, 3], b2[None, :, 3])
    inter = np.maximum(x2 - x1, np.float32(0)) * np.maximum(y2 - y1, np.float32(0))
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    return inter / np.maximum(a1[:, None] + a2[None, :] - inter, np.float32(eps))


def _rows_to(dev, rows):
    """numpy row indices -> an index tensor where the embeddings live"""
    return _idx_to(dev, torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)))


class _TrackTable:
    """The tracker's memory as a struct of arrays: one row per live tracklet, in creation order (the order the
    affinity columns are laid out in, which decides ties), plus the most recent frames' unmatched detections
    ("backdrops", newest frame first).  Rows are updated / appended / expired with index operations; nothing here is
    per-object Python state.  ids / boxes / labels / last-seen frames are numpy arrays on the host, the embeddings a torch
    tensor on the device the track head left them on."""

    def __init__(self, backdrop_frames):
        self.ids = np.zeros((0,), dtype=np.int64)
        self.box = np.zeros((0, 5), dtype=np.float32)
        self.emb = torch.zeros((0, 0))                            # lives where the track head left its embeddings (device)
        self.lab = np.zeros((0,), dtype=np.int64)
        self.seen = np.zeros((0,), dtype=np.int64)                # frame a row was last matched in
        self.backdrop_frames = backdrop_frames
        self.backdrops = []                                       # [(box, emb, lab)], newest first

    def __len__(self):
        return int(self.ids.shape[0])

    def columns(self):
        """(ids, labels, embeds) of everything a detection can be matched to: tracklets, then backdrops (id -1)"""
        ids, lab, emb = [self.ids], [self.lab], [self.emb]
        for (bb, be, bl) in self.backdrops:
            ids.append(np.full((be.shape[0],), -1, dtype=np.int64))
            lab.append(bl)
            emb.append(be)
        emb = [e for e in emb if e.shape[0]]
        return np.concatenate(ids), np.concatenate(lab), (torch.cat(emb, 0) if len(emb) > 1 else (emb[0] if emb else self.emb))

    def absorb(self, ids, box, emb, lab, frame, momentum):
        """matched detections refresh their rows (embedding = exponential moving average), unknown ids append rows"""
        if ids.shape[0] == 0:
            return
        pos = {t: r for r, t in enumerate(self.ids.tolist())}
        row = np.array([pos.get(t, -1) for t in ids.tolist()], dtype=np.int64)
        old, new = row >= 0, row < 0
        dev = emb.device
        if old.any():
            r = row[old]
            rd = _rows_to(dev, r)
            self.emb[rd] = (1 - momentum) * self.emb[rd] + momentum * emb[_rows_to(dev, np.flatnonzero(old))]
            self.box[r], self.lab[r], self.seen[r] = box[old], lab[old], frame
        if new.any():
            k = int(new.sum())
            self.ids = np.concatenate([self.ids, ids[new]])
            self.box = np.concatenate([self.box, box[new]], 0)
            self.emb = torch.cat([self.emb.reshape(-1, emb.shape[1]).to(dev), emb[_rows_to(dev, np.flatnonzero(new))]], 0)
            self.lab = np.concatenate([self.lab, lab[new]])
            self.seen = np.concatenate([self.seen, np.full((k,), frame, dtype=np.int64)])

    def expire(self, frame, max_age):
        live = (frame - self.seen) < max_age
        if not live.all():
            self.ids, self.box, self.emb, self.lab, self.seen = (self.ids[live], self.box[live],
                                                                  self.emb[_rows_to(self.emb.device, np.flatnonzero(live))],
                                                                  self.lab[live], self.seen[live])

    def push_backdrop(self, box, emb, lab):
        self.backdrops.insert(0, (box, emb, lab))
        del self.backdrops[self.backdrop_frames:]
        if self.backdrop_frames == 0:
            self.backdrops = []


def native_tracker_cfg(init_score_thr=0.8, obj_score_thr=0.5, match_score_thr=0.5, memo_tracklet_frames=10, memo_backdrop_frames=1,
                       memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True,
                       match_metric="bisoftmax", **_):
    """a ph_tracker_cfg from QuasiDenseEmbedTracker's kwargs (1 - momentum evaluated in double, as `(1 - momentum) * tensor` does)"""
    return _lib.TrackerCfg(init_score_thr, obj_score_thr, match_score_thr, memo_momentum, 1 - memo_momentum, nms_conf_thr,
                           nms_backdrop_iou_thr, nms_class_iou_thr, memo_tracklet_frames, memo_backdrop_frames, 1 if with_cats else 0,
                           MATCH_METRICS[match_metric])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class NativeHostTracker(_OwnsHandles):
    """One stream's C++ tracker object (ph_tracker_*, csrc/ph_tracker.hip): bookkeeping in C++ on the host, the embeddings in the
    device pool `mem` this object owns; per frame two small uploads, six launches and ONE synchronising download (the
    [detections x memory] scores).  Same integer ids as the array form.  `cfg`: a ph_tracker_cfg (`native_tracker_cfg`)."""
    _destroy_symbol = "ph_tracker_destroy"

    def __init__(self, cfg, device, capacity, max_dets):
        lib = _lib.load()
        self.device = device
        nbytes = lib.ph_tracker_device_bytes(capacity, max_dets)
        self.mem = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        h = lib.ph_tracker_create(C.byref(cfg), _lib.ptr(self.mem), nbytes, capacity, max_dets)
        if not h:
            raise _cfg_error("ph_tracker_create failed")
        self._h = C.c_void_p(h)

    @property
    def handle(self):
        """the ph_tracker handle; None once destroyed"""
        return self._h

    @property
    def num_tracklets(self):
        return int(_lib.load().ph_tracker_num_tracklets(self._h))

    @property
    def rows(self):
        return int(_lib.load().ph_tracker_rows(self._h))

    def match(self, box, lab, emb, frame_id):
        """one frame: box [n, 5] / lab [n] numpy arrays on the host, emb [n, 256] on the device -> (kept, ids): the rows of the kept
        detections in descending-score order and their int64 ids"""
        box, lab = np.ascontiguousarray(box, dtype=np.float32), np.ascontiguousarray(lab, dtype=np.int64)
        emb = emb.detach().float().contiguous()
        n = box.shape[0]
        kept, ids = np.empty((max(n, 1),), dtype=np.int32), np.empty((max(n, 1),), dtype=np.int64)
        k = _lib.load().ph_tracker_match(self._h, _vp(box), _vp(lab), _lib.ptr(emb), n, int(frame_id), _vp(kept), _vp(ids), _lib.stream_ptr())
        if k < 0:
            _lib.check(k, "ph_tracker_match")
        return kept[:k].astype(np.int64), ids[:k].copy()

    def match_frames(self, boxes, labels, embeds, first_frame_id):
        """a step's frames in ONE native call (`ph_tracker_match_frames`): boxes [sum n, 5] float32 / labels [sum n] int64 numpy arrays
        on the host, embeds: per frame a [n, 256] device tensor (frames without detections: n = 0, skipped like the reference's loop).
        Returns per frame the int64 ids of its kept detections in `match`'s order, and the number of frames matched."""
        nf = len(embeds)
        counts = np.asarray([int(e.shape[0]) for e in embeds], dtype=np.int32)
        tot = int(counts.sum())
        embs = [e.detach().float().contiguous() for e in embeds]
        ptrs = (C.c_void_p * nf)(*[e.data_ptr() if e.shape[0] else None for e in embs])
        box = np.ascontiguousarray(boxes, dtype=np.float32)
        lab = np.ascontiguousarray(labels, dtype=np.int64)
        kept, ids, kc = np.empty((max(tot, 1),), dtype=np.int32), np.empty((max(tot, 1),), dtype=np.int64), np.empty((nf,), dtype=np.int32)
        m = _lib.load().ph_tracker_match_frames(self._h, _vp(box), _vp(lab), ptrs, _vp(counts), nf, int(first_frame_id), _vp(kept), _vp(ids),
                                                _vp(kc), _lib.stream_ptr())
        if m < 0:
            _lib.check(m, "ph_tracker_match_frames")
        o = np.concatenate([[0], np.cumsum(counts)])
        return [ids[o[f]:o[f] + kc[f]].copy() for f in range(nf)], int(m)


@TRACKERS.register_module()
class QuasiDenseEmbedTracker(object):
    """Quasi-dense embedding tracker with the constructor kwargs, `match` signature and integer-id semantics of
    polyphonic/video/qdtrack/trackers/quasi_dense_embed_tracker.py:8-207 (pinned by tests/golden/tracker.npz, which the
    reference class produced).  This build's formulation: detections are de-duplicated with one triangular IoU test,
    the memory is a `_TrackTable`, the affinity matrix is computed once and the greedy one-to-one assignment walks the
    detections in score order with a `taken` mask over tracklet columns.  The reference also carries a per-tracklet
    velocity that nothing reads (its `match` ignores `memo_vs`); it is not kept.
    Where the arithmetic runs: boxes, labels, ids and the control flow on the host, as numpy float32 / int64 arrays (the same
    IEEE operations as the torch CPU ops they replace -- same values, a third of the per-call cost; the frame's ~60 tiny array
    operations were 0.6 ms of a 2 ms video frame); the EMBEDDINGS (detections and memory) stay on the device the track head
    produced them on, and the [detections x memory] affinity matrix is computed there (`ph_track_affinity`, csrc/ph_track.hip)
    -- one D2H of that matrix per frame feeds the greedy walk.  With CPU inputs (the CPU tests, gloo) the affinity runs as
    torch CPU ops; no process-global state is touched either way."""

    def __init__(self, init_score_thr=0.8, obj_score_thr=0.5, match_score_thr=0.5, memo_tracklet_frames=10,
                 memo_backdrop_frames=1, memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3,
                 nms_class_iou_thr=0.7, with_cats=True, match_metric='bisoftmax'):
        if not (0 <= memo_momentum <= 1.0) or memo_tracklet_frames < 0 or memo_backdrop_frames < 0:
            raise AssertionError("bad memo configuration")
        if match_metric not in MATCH_METRICS:
            raise AssertionError(f"unknown match_metric {match_metric}")
        self.init_score_thr, self.obj_score_thr, self.match_score_thr = init_score_thr, obj_score_thr, match_score_thr
        self.memo_tracklet_frames, self.memo_backdrop_frames = memo_tracklet_frames, memo_backdrop_frames
        self.memo_momentum, self.nms_conf_thr = memo_momentum, nms_conf_thr
        self.nms_backdrop_iou_thr, self.nms_class_iou_thr, self.with_cats = nms_backdrop_iou_thr, nms_class_iou_thr, with_cats
        self.match_metric = match_metric
        self._num_tracklets = 0
        self.table = _TrackTable(memo_backdrop_frames)
        self._native = None           # a NativeHostTracker from the first frame whose embeddings are on a GPU

    @property
    def num_tracklets(self):
        return self._num_tracklets if self._native is None else self._native.num_tracklets

    @num_tracklets.setter
    def num_tracklets(self, v):
        self._num_tracklets = v

    @property
    def empty(self):
        return len(self.table) == 0 if self._native is None else self._native.rows == 0

    # -- the native form (embeddings on a GPU): one C call per frame ----------------------------------------------
    NATIVE_CAPACITY, NATIVE_MAX_DETS = 4096, 128
    native = True                 # False: the array form below also for GPU embeddings (tests compare the two)

    def native_tracker(self, dev):
        """the `NativeHostTracker` of this stream, created on first use on the embeddings' device"""
        if self._native is None:
            if len(self.table) or self._num_tracklets:
                raise _lib.PolyheadError("QuasiDenseEmbedTracker: a tracker that started on CPU embeddings cannot continue on the GPU")
            # the constructor's kwargs are this object's attributes of the same names; `native_tracker_cfg` ignores the others
            self._native = NativeHostTracker(native_tracker_cfg(**vars(self)), dev, self.NATIVE_CAPACITY, self.NATIVE_MAX_DETS)
        if dev != self._native.device:
            raise _lib.PolyheadError("QuasiDenseEmbedTracker: the embeddings moved to another device mid-stream")
        return self._native

    def native_ready(self, n, emb, box_width=5):
        """True if `match` of n detections ([n, box_width] boxes) with these embeddings takes the native path"""
        return bool(self.native and emb.is_cuda and n <= self.NATIVE_MAX_DETS and box_width == 5 and emb.shape[1] == 256
                    and (self._native is not None or (len(self.table) == 0 and self._num_tracklets == 0)))

    def match_frames(self, boxes, labels, embeds, first_frame_id):
        """a step's frames in ONE native call (`NativeHostTracker.match_frames`, its arguments and return value)"""
        dev = next((e.device for e in embeds if e.shape[0]), None)
        if dev is None:
            return [np.empty((0,), dtype=np.int64) for _ in embeds], 0
        return self.native_tracker(dev).match_frames(boxes, labels, embeds, first_frame_id)

    def _match_native(self, bboxes, labels, track_feats, frame_id):
        # boxes / labels: torch tensors (any device) or host numpy arrays (`replay_tracking` downloads a whole step's at once)
        box = bboxes if isinstance(bboxes, np.ndarray) else bboxes.detach().cpu().float().numpy()
        lab = labels if isinstance(labels, np.ndarray) else labels.detach().cpu().long().numpy()
        box, lab = np.ascontiguousarray(box, dtype=np.float32), np.ascontiguousarray(lab, dtype=np.int64)
        kept, ids = self.native_tracker(track_feats.device).match(box, lab, track_feats, frame_id)
        return torch.from_numpy(box[kept]), torch.from_numpy(lab[kept]), torch.from_numpy(ids)

    # -- pieces of `match` ---------------------------------------------------------------------------------
    def _dedup(self, box):
        """a detection is dropped when ANY higher-scored detection (kept or not) overlaps it by more than the IoU
        threshold of its own score class (:147-155).  box: numpy float32 [n, 5], descending score"""
        f32 = np.float32
        iou = _iou_np(box[:, :4], box[:, :4])
        thr = np.where(box[:, 4] < f32(self.obj_score_thr), f32(self.nms_backdrop_iou_thr), f32(self.nms_class_iou_thr))
        return ~(np.tril(iou, -1) > thr[:, None]).any(1), iou

    def _affinity(self, emb, lab, memo_emb, memo_lab):
        """[detections x memory columns] match scores (:165-182), returned on the host (torch fp32).  Labels: numpy or torch"""
        lab, memo_lab = torch.as_tensor(lab), torch.as_tensor(memo_lab)
        # the fused kernel keeps a detection row in one workgroup: n <= 128 detections, m <= 4096 memory columns (max_per_img is
        # 100 and the memory a few hundred columns in the shipped configs).  Beyond that the same formula runs as torch ops ON
        # THE DEVICE the embeddings live on (below) -- the reference has no limit, a long video must not abort mid-stream
        if emb.is_cuda and emb.shape[0] <= 128 and memo_emb.shape[0] <= 4096:
            lib = _lib.load()
            n, m = emb.shape[0], memo_emb.shape[0]
            dev = emb.device
            score = torch.empty((n, m), dtype=torch.float32, device=dev)
            ws = torch.empty((lib.ph_track_affinity_workspace_bytes(n, m),), dtype=torch.uint8, device=dev)
            # named, so that the four operands are alive (and distinct blocks of the caching allocator) until the launch is queued
            e, me = emb.contiguous(), memo_emb.contiguous()
            both = torch.cat([lab.reshape(-1), memo_lab.reshape(-1)]).to(torch.int32)          # ONE pinned transfer for both label vectors
            both = both.to(dev) if both.is_cuda else both.pin_memory().to(dev, non_blocking=True)
            l, ml = both[:n], both[n:]
            _lib.check(lib.ph_track_affinity(_lib.ptr(e), _lib.ptr(l), _lib.ptr(me), _lib.ptr(ml), n, m, MATCH_METRICS[self.match_metric],
                                             1 if self.with_cats else 0, _lib.ptr(score), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "ph_track_affinity")
            host = torch.empty((n, m), dtype=torch.float32, pin_memory=True)
            host.copy_(score, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return host
        if self.match_metric == 'cosine':
            unit = torch.nn.functional.normalize
            s = unit(emb, p=2, dim=1) @ unit(memo_emb, p=2, dim=1).t()
        else:
            dot = emb @ memo_emb.t()
            s = dot.softmax(dim=1)
            if self.match_metric == 'bisoftmax':
                s = (s + dot.softmax(dim=0)) / 2
        if self.with_cats:
            s = s * (lab.to(s.device)[:, None] == memo_lab.to(s.device)[None, :]).float()
        return s.cpu()

    def _assign(self, score, det_conf, memo_ids):
        """greedy, in detection (score) order: best still-free column; a tracklet column is consumed by a confident
        detection, a weak detection that resembles a tracklet is marked -2 (neither a new track nor a backdrop),
        matches to backdrop columns assign nothing (:183-197).  numpy: score fp32 [n, m], det_conf fp32 [n], memo_ids int64 [m]"""
        f32 = np.float32
        n = score.shape[0]
        out = np.full((n,), -1, dtype=np.int64)
        taken = np.zeros(score.shape[1], dtype=bool)
        match_thr, obj_thr, conf_thr = f32(self.match_score_thr), f32(self.obj_score_thr), f32(self.nms_conf_thr)
        for i in range(n):
            row = np.where(taken, f32(0), score[i])
            j = int(row.argmax())                                  # first maximal column, like torch.max(0)
            conf = row[j]
            if not conf > match_thr or memo_ids[j] < 0:
                continue
            if det_conf[i] > obj_thr:
                out[i] = memo_ids[j]
                taken[j] = True
            elif conf > conf_thr:
                out[i] = -2
        return out

    def match(self, bboxes, labels, track_feats, frame_id, asso_tau=-1):
        """bboxes [n,5] (x1,y1,x2,y2,score), labels [n], track_feats [n,256] -> (bboxes, labels, ids) of the kept
        detections in descending-score order; ids >= 0 track, -1 unmatched, -2 suppressed."""
        return self._match(bboxes, labels, track_feats, frame_id)

    def _match(self, bboxes, labels, track_feats, frame_id):
        if self.native_ready(bboxes.shape[0], track_feats, bboxes.shape[1]):
            return self._match_native(bboxes, labels, track_feats, frame_id)
        if self._native is not None:
            # the native tracker owns the memory and the id counter from its first frame on: the array form below would start a second,
            # empty state (ids from 0 again, colliding with live native ids) and the native memory would miss this frame
            raise _lib.PolyheadError(f"QuasiDenseEmbedTracker: the native tracker has started and this frame does not fit it (device embeddings of "
                                f"width 256, [n, 5] boxes, n <= {self.NATIVE_MAX_DETS}; got n = {bboxes.shape[0]}, boxes {tuple(bboxes.shape)}, "
                                f"embeddings {tuple(track_feats.shape)} on {track_feats.device}); build the tracker with native=False for such streams")
        box_t, lab_t, emb = bboxes.detach().cpu().float(), labels.detach().cpu().long(), track_feats.detach().float()   # emb: stays put
        dev = emb.device
        order = box_t[:, 4].sort(descending=True)[1].numpy()      # torch's order among equal scores (what the goldens were pinned with)
        box, lab = box_t.numpy()[order], lab_t.numpy()[order]
        keep, iou = self._dedup(box)
        kept = order[keep]                                        # one gather of the embeddings for both steps
        box, lab, emb = box[keep], lab[keep], emb[_rows_to(dev, kept)]
        ids = np.full((box.shape[0],), -1, dtype=np.int64)
        if box.shape[0] and not self.empty:
            memo_ids, memo_lab, memo_emb = self.table.columns()
            ids = self._assign(self._affinity(emb, lab, memo_emb, memo_lab).numpy(), box[:, 4], memo_ids)
        born = (ids == -1) & (box[:, 4] > np.float32(self.init_score_thr))
        k = int(born.sum())
        ids[born] = np.arange(self._num_tracklets, self._num_tracklets + k, dtype=np.int64)
        self._num_tracklets += k
        self._remember(ids, box, emb, lab, frame_id, iou[keep][:, keep])
        return torch.from_numpy(box), torch.from_numpy(lab), torch.from_numpy(ids)

    def _remember(self, ids, box, emb, lab, frame_id, iou):
        """:47-102: tracked detections go to the table; the still-unmatched ones that no higher-scored detection covers
        become this frame's backdrops; tracklets unseen for `memo_tracklet_frames` frames are forgotten.  `iou`: the kept
        detections' pairwise IoU (the de-duplication's matrix restricted to them -- the same values)"""
        tracked = ids > -1
        self.table.absorb(ids[tracked], box[tracked], emb[_rows_to(emb.device, np.flatnonzero(tracked))], lab[tracked], frame_id,
                          self.memo_momentum)
        loose = ids == -1
        covered = (np.tril(iou, -1) > np.float32(self.nms_backdrop_iou_thr)).any(1)
        bd = loose & ~covered
        self.table.push_backdrop(box[bd], emb[_rows_to(emb.device, np.flatnonzero(bd))], lab[bd])
        self.table.expire(frame_id, self.memo_tracklet_frames)


def replay_tracking(records, tracker_cfg=None, tracker=None, first_count=1):
    """records: [(frame_id, bboxes[n,5], labels[n], embeds[n,256])] of ALL frames (any order); replays `match` in
    frame order like polyphonic_former_video.py:391-402 (frame_id = running count from 1, ids painted by `painted_ids`).
    A stream that arrives in batches passes its persistent `tracker` and `first_count` = 1 + the number of non-empty frames
    replayed so far.  Returns {frame_id: ids tensor}."""
    if tracker is None:
        tracker = QuasiDenseEmbedTracker(**(tracker_cfg or {}))
    out, cnt = {}, first_count
    records = sorted(records, key=lambda r: r[0])
    if records and all(r[1].is_cuda and r[2].is_cuda for r in records):
        # device records (after an RCCL all-gather): ONE download of the step's boxes and labels instead of two per frame
        ns = [int(r[1].shape[0]) for r in records]
        if sum(ns):
            bl = torch.cat([torch.cat([r[1].float(), r[2].float()[:, None]], 1) for r in records if r[1].shape[0]], 0).cpu().numpy()
            o = np.cumsum([0] + ns)
            records = [(r[0], bl[o[i]:o[i + 1], :5], bl[o[i]:o[i + 1], 5].astype(np.int64), r[3]) for i, r in enumerate(records)]
    if records and all(isinstance(r[1], np.ndarray) and tracker.native_ready(r[1].shape[0], r[3], r[1].shape[1]) for r in records):
        # device embeddings, host boxes: the whole step in ONE native call (a Python round trip per frame was half of the 0.13 ms a
        # frame's replay cost)
        per_frame, matched = tracker.match_frames(np.concatenate([r[1] for r in records], 0), np.concatenate([r[2] for r in records], 0),
                                                  [r[3] for r in records], cnt)
        return {r[0]: torch.from_numpy(painted_ids(ids)) for r, ids in zip(records, per_frame)}
    for fid, bb, lab, emb in records:
        if bb.shape[0] > 0:
            if isinstance(bb, np.ndarray) and not tracker.native_ready(bb.shape[0], emb, bb.shape[1]):
                bb, lab = torch.from_numpy(bb), torch.from_numpy(lab)           # the array form reads torch boxes and labels
            _, _, ids = tracker.match(bboxes=bb, labels=lab, track_feats=emb, frame_id=cnt)
            cnt += 1
            ids = painted_ids(ids)
        else:
            ids = torch.zeros((0,), dtype=torch.long)
        out[fid] = ids
    return out


class NativeDeviceTracker(_OwnsHandles):
    """The tracker whose state lives in ONE device buffer this object owns (ph_dtracker_*, csrc/ph_dtracker.hip): `reset` and `run`
    are launches only on the current stream (capturable), `status()` and `tables()` synchronising reads.  `cfg`: a ph_tracker_cfg
    (`native_tracker_cfg`)."""
    _destroy_symbol = "ph_dtracker_destroy"

    def __init__(self, cfg, device, capacity=4096, max_dets=128, first_frame_id=1):
        lib, dev = _lib.load(), torch.device(device)
        self.cfg, self.device, self.capacity, self.max_dets = _lib.TrackerCfg.from_buffer_copy(bytes(cfg)), dev, capacity, max_dets
        nbytes = lib.ph_dtracker_device_bytes(C.byref(self.cfg), capacity, max_dets)
        if nbytes == 0:
            raise _cfg_error("ph_dtracker_device_bytes")
        self.mem = torch.empty((nbytes,), dtype=torch.uint8, device=dev)             # zeroing contract: none (`reset` below)
        self._h = C.c_void_p()
        _lib.check(lib.ph_dtracker_create(C.byref(self.cfg), _lib.ptr(self.mem), nbytes, capacity, max_dets, C.byref(self._h)),
                   "ph_dtracker_create")
        self.layout = _lib.DtrackerLayout()
        _lib.check(lib.ph_dtracker_get_layout(self._h, C.byref(self.layout)), "ph_dtracker_get_layout")
        self.io = _lib.DtrackerIO()
        self._keep = None
        self.reset(first_frame_id)

    def reset(self, first_frame_id=1):
        """one launch: empty tables, full free stack, the frame counter at `first_frame_id`, status 0"""
        _lib.check(_lib.load().ph_dtracker_reset(self._h, int(first_frame_id), _lib.stream_ptr()), "ph_dtracker_reset")

    def run(self, boxes, labels, counts, embeds, refuse=None, out=None):
        """B frames in order: boxes fp32 [B, n, 5], labels int32 [B, n], counts int32 [B], embeds fp32 [B, n, 256], refuse int32 [B] or
        None, contiguous on the device -> (kept int32 [B, max_dets], ids int64 [B, max_dets], kept_counts int32 [B]) on the device
        (`out`: the same three, to write into); launches only"""
        return self._launch(boxes, labels, counts, embeds, refuse, out, "run")

    def _launch(self, boxes, labels, counts, embeds, refuse, out, how, active=None):
        B, dev = counts.shape[0], self.device
        if how == "step" and B != self.streams:
            raise _lib.PolyheadError(f"NativeDeviceTrackerBank.step: {self.streams} streams, tables of {B}")
        for t, dt, nm in ((boxes, torch.float32, "boxes"), (labels, torch.int32, "labels"), (counts, torch.int32, "counts"),
                          (embeds, torch.float32, "embeds")) + (((refuse, torch.int32, "refuse"),) if refuse is not None else ()):
            if t.dtype != dt or not t.is_contiguous() or t.device != dev or t.shape[0] != B:
                raise _lib.PolyheadError(f"{type(self).__name__}.{how}: {nm} must be {dt} contiguous [{B}, ...] on {dev}")
        if out is None:
            out = (torch.empty((B, self.max_dets), dtype=torch.int32, device=dev), torch.empty((B, self.max_dets), dtype=torch.int64, device=dev),
                   torch.empty((B,), dtype=torch.int32, device=dev))
        io = self.io
        io.boxes, io.box_stride = boxes.data_ptr(), boxes[0].numel()
        io.labels, io.label_stride = labels.data_ptr(), labels[0].numel()
        io.counts, io.count_stride = counts.data_ptr(), 1
        io.refuse, io.refuse_stride = (None, 0) if refuse is None else (refuse.data_ptr(), 1)
        io.embeds, io.embed_stride = embeds.data_ptr(), embeds[0].numel()
        io.kept_out, io.ids_out, io.kept_counts = (o.data_ptr() for o in out)
        self._keep = (boxes, labels, counts, embeds, refuse, out, active)      # alive until the launches have run (static under graph capture)
        if how == "step":
            _lib.check(_lib.load().ph_dtracker_step(self._h, C.byref(io), None if active is None else _lib.ptr(active), _lib.stream_ptr()),
                       "ph_dtracker_step")
        else:
            _lib.check(_lib.load().ph_dtracker_run(self._h, C.byref(io), B, _lib.stream_ptr()), "ph_dtracker_run")
        return out

    def _piece(self, offset, dtype, shape, s=0):
        """a piece of stream s's block (`layout` is stream 0's; a bank's blocks are `layout.total_bytes` apart)"""
        n = int(torch.tensor([], dtype=dtype).element_size()) * int(math.prod(shape))
        at = int(s) * int(self.layout.total_bytes) + int(offset)
        return self.mem[at:at + n].view(dtype).reshape(shape)

    def status(self, s=0):
        """the status record (of stream s of a bank) as a dict of ints (_lib.DTRK_STATUS); synchronises"""
        return dict(zip(_lib.DTRK_STATUS, self._piece(self.layout.status, torch.int64, (_lib.PH_DTRK_ST_WORDS,), s).cpu().tolist()))

    def tables(self, s=0):
        """the live tracklet rows in creation order (ids, labels, seen, boxes, slots, and `pool`: their embedding rows) plus the
        backdrop generations, newest first, as host tensors (of stream s of a bank); synchronises.  For tests and checkpointing"""
        l, Cn, N, G = self.layout, self.capacity, self.max_dets, self.layout.generations
        rows = self.status(s)["rows"]
        P = lambda off, dt, shape: self._piece(off, dt, shape, s)
        tr = dict(ids=P(l.trk_id, torch.int64, (Cn,))[:rows].cpu(), labels=P(l.trk_label, torch.int32, (Cn,))[:rows].cpu(),
                  seen=P(l.trk_seen, torch.int64, (Cn,))[:rows].cpu(), boxes=P(l.trk_box, torch.float32, (Cn, 5))[:rows].cpu(),
                  slots=P(l.trk_slot, torch.int32, (Cn,))[:rows].cpu())
        pool = P(l.pool, torch.float32, (Cn, 256))
        tr["pool"] = pool[tr["slots"].long().to(self.device)].cpu()
        counts = P(l.bd_count, torch.int32, (G,)).cpu().tolist()
        lab, slot, box = (P(l.bd_label, torch.int32, (G, N)).cpu(), P(l.bd_slot, torch.int32, (G, N)).cpu(),
                          P(l.bd_box, torch.float32, (G, N, 5)).cpu())
        tr["backdrops"] = [dict(labels=lab[g, :c], slots=slot[g, :c], boxes=box[g, :c]) for g, c in enumerate(counts)]
        return tr


class NativeDeviceTrackerBank(NativeDeviceTracker):
    """`streams` (1 .. 64) device trackers in ONE buffer, advanced by one frame each in one launch sequence (ph_dtracker_bank_* /
    ph_dtracker_step, csrc/ph_dtracker.hip): the trackers of S live cameras whose current frames share a launch.  Stream s's block lies
    at s * `layout.total_bytes` of `mem`; `status(s)` and `tables(s)` are NativeDeviceTracker's, per stream.  `reset` and `step` are
    launches only on the current stream (capturable)."""

    def __init__(self, cfg, device, streams, capacity=4096, max_dets=128, first_frame_id=1):
        lib, dev = _lib.load(), torch.device(device)
        self.cfg, self.device, self.capacity, self.max_dets = _lib.TrackerCfg.from_buffer_copy(bytes(cfg)), dev, capacity, max_dets
        self.streams = int(streams)
        nbytes = lib.ph_dtracker_bank_bytes(C.byref(self.cfg), capacity, max_dets, self.streams)
        if nbytes == 0:
            raise _cfg_error("ph_dtracker_bank_bytes")
        self.mem = torch.empty((nbytes,), dtype=torch.uint8, device=dev)             # zeroing contract: none (`reset` below)
        self._h = C.c_void_p()
        _lib.check(lib.ph_dtracker_bank_create(C.byref(self.cfg), _lib.ptr(self.mem), nbytes, capacity, max_dets, self.streams, C.byref(self._h)),
                   "ph_dtracker_bank_create")
        self.layout = _lib.DtrackerLayout()
        _lib.check(lib.ph_dtracker_get_layout(self._h, C.byref(self.layout)), "ph_dtracker_get_layout")
        n, stride = C.c_int(), C.c_uint64()
        _lib.check(lib.ph_dtracker_get_streams(self._h, C.byref(n), C.byref(stride)), "ph_dtracker_get_streams")
        assert (n.value, stride.value) == (self.streams, self.layout.total_bytes)
        self.io = _lib.DtrackerIO()
        self._keep = None
        self.reset(None, first_frame_id)

    def block(self, s):
        """stream s's whole block (state and scratch) as a uint8 view of `mem`"""
        return self._piece(0, torch.uint8, (int(self.layout.total_bytes),), s)

    def reset(self, streams=None, first_frame_id=1):
        """one launch: the named streams (an iterable of indices; None: all) start a new sequence, the others are untouched"""
        mask = 0
        for s in (range(self.streams) if streams is None else streams):
            if not 0 <= int(s) < self.streams:
                raise _lib.PolyheadError(f"NativeDeviceTrackerBank.reset: stream {s} of {self.streams}")
            mask |= 1 << int(s)
        mask -= (mask >> 63) << 64                               # the 64 bits as the ABI's int64
        _lib.check(_lib.load().ph_dtracker_reset_streams(self._h, mask, int(first_frame_id), _lib.stream_ptr()), "ph_dtracker_reset_streams")

    def _active(self, active):
        """`active` as the int32 [streams] device words ph_dtracker_step reads (None stays None: every stream has a frame)"""
        if active is None:
            return None
        if not torch.is_tensor(active):
            active = torch.tensor([1 if a else 0 for a in active], dtype=torch.int32)
            if self.device.type == "cuda":
                active = active.pin_memory().to(self.device, non_blocking=True)
        if active.dtype != torch.int32 or tuple(active.shape) != (self.streams,) or not active.is_contiguous() or active.device != self.device:
            raise _lib.PolyheadError(f"NativeDeviceTrackerBank: active must be int32 contiguous [{self.streams}] on {self.device}")
        return active

    def step(self, boxes, labels, counts, embeds, refuse=None, active=None, out=None):
        """one frame of every stream: `NativeDeviceTracker.run`'s tables with the leading dimension indexing STREAMS ([S, n, 5] ..),
        `active`: int32 [S] on the device (or a host sequence) or None -- a zero word's stream has no frame in this step and keeps every
        bit of its state; its kept_counts entry is 0.  Returns (kept [S, max_dets], ids [S, max_dets], kept_counts [S]); launches only"""
        active = self._active(active)
        return self._launch(boxes, labels, counts, embeds, refuse, out, "step", active)

    def run(self, *a, **kw):
        raise _lib.PolyheadError("NativeDeviceTrackerBank.run: a bank's frames are side by side, not in order: step()")
