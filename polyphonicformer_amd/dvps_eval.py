"""SURVEY.md 8(f) row N2 -- the output / evaluation wire format of the video path, host side.

* `save_record` / `record_name`: what `CityscapesDVPSDataset.pre_eval` writes per frame
  (datasets/cityscapes_dvps.py:325-338): `{"panseg": uint32 sem * 10000 + track_id, "depth": float32}` as
  `{seq:06d}_{img:06d}.pth`, so the unmodified reference evaluator (polyphonic/apis/video_evaluate.py) can score
  this build's outputs.
* `vpq_eval`, `evaluate_clip`, `video_evaluate`: the DVPQ metric itself (datasets/utils.py:31-106,
  polyphonic/apis/video_evaluate.py:14-111), restated on sorted-unique integer arrays instead of Python dicts
  (same pairing, same accumulation order: the per-class sums are bit-identical to the reference's) -- used by the
  tests to check the writer against goldens produced by the reference evaluator, and usable on its own.
* `compute_errors`: the depth error metrics (datasets/utils.py:109-137).
* `clip_tallies`, `depth_errors_from_tallies`, `dvpq_from_frames`: the same metric from per-frame tallies (pure numpy), and
  `DeviceEvaluator` / `video_evaluate_device`, which get those tallies from ph_dvpq_frames without downloading a map.
Everything up to `DeviceEvaluator` is numpy / torch.save and importable without a GPU or the library."""
import os

import numpy as np
import torch

INSTANCE_DIVISOR = 10000          # datasets/utils.py:5
_EPSILON = 1e-15                  # video_evaluate.py:11


def record_name(seq_id, img_id):
    return "{:06d}_{:06d}.pth".format(int(seq_id), int(img_id))


def wire_record(result):
    """result: dict(sem=int map, track=int map, depth=float map) as PolyphonicVideo.simple_test returns them
    (polyphonic_former_video.py:397-405)"""
    pan = result["sem"].astype(np.int64) * INSTANCE_DIVISOR + result["track"].astype(np.int64)
    return {"panseg": pan.astype(np.uint32), "depth": result["depth"].astype(np.float32)}


def save_record(save_dir, seq_id, img_id, result, sub="pred"):
    d = os.path.join(save_dir, sub)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, record_name(seq_id, img_id))
    torch.save(wire_record(result), path)
    return path


def vpq_eval(pred_ids, gt_ids, num_classes=19, max_ins=INSTANCE_DIVISOR, ign_id=255):
    """-> (iou_per_class, tp_per_class, fn_per_class, fp_per_class), float64 [num_classes + 1]"""
    pred = np.asarray(pred_ids).astype(np.int64).ravel()
    gt = np.asarray(gt_ids).astype(np.int64).ravel()
    pu, pinv, parea = np.unique(pred, return_inverse=True, return_counts=True)
    gu, ginv, garea = np.unique(gt, return_inverse=True, return_counts=True)
    # intersections, sorted by (gt id, pred id) = the reference's key order gt * 1e9 + pred
    iu, iarea = np.unique(ginv.astype(np.int64) * len(pu) + pinv, return_counts=True)
    gi, pi = iu // len(pu), iu % len(pu)
    return vpq_from_tables(gu, garea, pu, parea, gi, pi, iarea, num_classes=num_classes, max_ins=max_ins, ign_id=ign_id)


def vpq_from_tables(gu, garea, pu, parea, gi, pi, iarea, num_classes=19, max_ins=INSTANCE_DIVISOR, ign_id=255):
    """the metric from the tables `vpq_eval` builds with np.unique: the sorted gt ids `gu` with their areas, the sorted pred ids
    `pu` with theirs, and the intersections (gu[gi], pu[pi]) -> iarea sorted by (gt id, pred id).  int64 arrays."""
    num_cat = num_classes + 1
    iou_c, tp_c, fn_c, fp_c = (np.zeros(num_cat, dtype=np.float64) for _ in range(4))
    gcat, pcat = gu // max_ins, pu // max_ins
    is_void = gu == ign_id * max_ins
    is_ign = gcat == ign_id
    void_ov = np.zeros(len(pu), dtype=np.int64)
    np.add.at(void_ov, pi[is_void[gi]], iarea[is_void[gi]])
    ign_ov = np.zeros(len(pu), dtype=np.int64)
    np.add.at(ign_ov, pi[is_ign[gi]], iarea[is_ign[gi]])
    same = gcat[gi] == pcat[pi]
    union = garea[gi] + parea[pi] - iarea - void_ov[pi]
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = iarea / union
    tp = same & (iou > 0.5)
    g_matched = np.zeros(len(gu), dtype=bool)
    p_matched = np.zeros(len(pu), dtype=bool)
    for k in np.nonzero(tp)[0]:                   # ascending key order, like the reference's dict iteration
        c = int(gcat[gi[k]])
        tp_c[c] += 1
        iou_c[c] += iou[k]
        g_matched[gi[k]] = True
        p_matched[pi[k]] = True
    for k in np.nonzero(~g_matched & ~is_ign)[0]:
        fn_c[int(gcat[k])] += 1
    for k in np.nonzero(~p_matched)[0]:
        if ign_ov[k] / parea[k] > 0.5:
            continue
        fp_c[int(pcat[k])] += 1
    return iou_c, tp_c, fn_c, fp_c


def evaluate_clip(pred_records, gt_records, depth_thr, num_classes):
    """video_evaluate.py:14-37: frames of a clip side by side (axis 1); pixels whose relative depth error exceeds
    `depth_thr` are relabelled to class `num_classes` before the panoptic comparison"""
    pred_pan = np.concatenate([r["panseg"] for r in pred_records], axis=1)
    gt_pan = np.concatenate([r["panseg"] for r in gt_records], axis=1)
    pred_dep = np.concatenate([r["depth"] for r in pred_records], axis=1)
    gt_dep = np.concatenate([r["depth"] for r in gt_records], axis=1)
    if depth_thr > 0.:
        m = gt_dep > 0.
        sel = pred_pan[m]
        bad = (np.abs(pred_dep[m] - gt_dep[m]) / gt_dep[m]) > depth_thr
        sel[bad] = num_classes * INSTANCE_DIVISOR
        pred_pan[m] = sel
    return vpq_eval(pred_pan, gt_pan, num_classes=num_classes)


def _pth_names(d):
    return sorted(f for f in os.listdir(d) if ".pth" in f and not f.startswith("._"))


def video_evaluate(eval_dir, num_classes, num_things, windows=(1, 2, 3, 4), depth_thrs=(0, 0.5, 0.25, 0.1)):
    """video_evaluate.py:40-111 -> {(k, lambda): (DVPQ, DVPQ_thing, DVPQ_stuff)} in percent; clips never span
    two sequences"""
    gt_dir, pred_dir = os.path.join(eval_dir, "gt"), os.path.join(eval_dir, "pred")
    gts = [os.path.join(gt_dir, f) for f in _pth_names(gt_dir)]
    preds = [os.path.join(pred_dir, f) for f in _pth_names(pred_dir)]
    cache = {}

    def load(p):
        if p not in cache:
            cache[p] = torch.load(p, weights_only=False)
        return cache[p]

    out = {}
    n = len(preds)
    for k in windows:
        for thr in depth_thrs:
            res = []
            for idx in range(n):
                if idx + k - 1 >= n:
                    break
                s0 = int(os.path.basename(preds[idx]).split("_")[0])
                s1 = int(os.path.basename(preds[idx + k - 1]).split("_")[0])
                if s0 != s1:
                    continue
                pr = [{kk: np.array(v) for kk, v in load(preds[idx + j]).items()} for j in range(k)]
                gr = [load(gts[idx + j]) for j in range(k)]
                res.append(evaluate_clip(pr, gr, thr, num_classes))
            if not res:
                continue
            iou, tp, fn, fp = (np.stack([r[j] for r in res]).sum(axis=0)[:num_classes] for j in range(4))
            sq = iou / (tp + _EPSILON)
            rq = tp / (tp + 0.5 * fn + 0.5 * fp + _EPSILON)
            pq = np.nan_to_num(sq * rq)
            out[(k, thr)] = (float(pq.mean() * 100), float(pq[:num_things].mean() * 100), float(pq[num_things:].mean() * 100))
    return out


def compute_errors(pred, gt):
    """datasets/utils.py:109-137"""
    pred, gt = pred[gt > 0.], gt[gt > 0.]
    thresh = np.maximum(gt / pred, pred / gt)
    return dict(abs_rel=np.mean(np.abs(gt - pred) / gt), sq_rel=np.mean(((gt - pred) ** 2) / gt),
                rmse=np.sqrt(((gt - pred) ** 2).mean()), rmse_log=np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean()),
                a1=(thresh < 1.25).mean(), a2=(thresh < 1.25 ** 2).mean(), a3=(thresh < 1.25 ** 3).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# The same metric from per-frame tallies.  A clip is its frames side by side, so a clip's (gt id, pred id) intersection counts are
# the sums of its frames' counts, and a depth threshold only relabels the pred id of the pixels that violate it.  A frame's table
# has rows (gt id, pred id, mask of violated thresholds, pixel count) -- ph_dvpq_frames (include/polyhead.h) builds it on the
# device; everything below is numpy on those few rows.
def frame_table(pred, gt, depth_thrs=()):
    """the table of one frame on the host, rows ascending in (gt id, pred id, mask): what ph_dvpq_frames writes.  `pred`, `gt`:
    wire records; bit j of the mask: gt depth > 0 and the fp32 relative error exceeds depth_thrs[j] as in `evaluate_clip`"""
    g = np.asarray(gt["panseg"]).astype(np.uint32).ravel()
    p = np.asarray(pred["panseg"]).astype(np.uint32).ravel()
    gd = np.asarray(gt["depth"], dtype=np.float32).ravel()
    pd = np.asarray(pred["depth"], dtype=np.float32).ravel()
    m = np.zeros(g.shape, dtype=np.uint32)
    pos = gd > 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(pd - gd) / gd
    for j, thr in enumerate(depth_thrs):
        m |= (pos & (rel > np.float32(thr))).astype(np.uint32) << np.uint32(j)
    rows, counts = np.unique(np.stack([g, p, m], axis=1), axis=0, return_counts=True)
    return np.concatenate([rows.astype(np.uint32), counts.astype(np.uint32)[:, None]], axis=1)


def clip_tallies(frame_tables, thr_index, num_classes, max_ins=INSTANCE_DIVISOR, ign_id=255):
    """`evaluate_clip` from the frames' tables: merge them, relabel the rows whose mask has bit `thr_index` set to class
    `num_classes` (None: no relabelling), add up equal (gt id, pred id) pairs and score them with `vpq_from_tables`"""
    rows = np.concatenate([np.asarray(t).reshape(-1, 4) for t in frame_tables], axis=0).astype(np.int64)
    g, p, m, c = rows[:, 0], rows[:, 1].copy(), rows[:, 2], rows[:, 3]
    if thr_index is not None:
        p[((m >> int(thr_index)) & 1) == 1] = num_classes * max_ins
    gu, ginv = np.unique(g, return_inverse=True)
    pu, pinv = np.unique(p, return_inverse=True)
    ginv, pinv = ginv.reshape(-1), pinv.reshape(-1)
    garea = np.zeros(len(gu), dtype=np.int64)
    np.add.at(garea, ginv, c)
    parea = np.zeros(len(pu), dtype=np.int64)
    np.add.at(parea, pinv, c)
    iu, iinv = np.unique(ginv.astype(np.int64) * len(pu) + pinv, return_inverse=True)
    iarea = np.zeros(len(iu), dtype=np.int64)
    np.add.at(iarea, iinv.reshape(-1), c)
    return vpq_from_tables(gu, garea, pu, parea, iu // len(pu), iu % len(pu), iarea, num_classes=num_classes, max_ins=max_ins,
                           ign_id=ign_id)


def depth_tallies(pred, gt):
    """the depth record of one frame on the host in fp64 (ph_dvpq_frames' depth_out row): count of gt > 0 pixels, the four sums
    of `compute_errors` with fp64 terms, the three threshold counts compared in fp32"""
    pred, gt = np.asarray(pred, dtype=np.float32).ravel(), np.asarray(gt, dtype=np.float32).ravel()
    pred, gt = pred[gt > 0.], gt[gt > 0.]
    with np.errstate(divide="ignore", invalid="ignore"):
        thresh = np.maximum(gt / pred, pred / gt)
        g, p = gt.astype(np.float64), pred.astype(np.float64)
        d2 = (g - p) ** 2
        return np.array([len(gt), (np.abs(g - p) / g).sum(), (d2 / g).sum(), d2.sum(), ((np.log(g) - np.log(p)) ** 2).sum(),
                         (thresh < 1.25).sum(), (thresh < 1.25 ** 2).sum(), (thresh < 1.25 ** 3).sum()], dtype=np.float64)


def depth_errors_from_tallies(rows):
    """`compute_errors` from depth records [..., 8] (one per frame, added here in order)"""
    t = np.asarray(rows, dtype=np.float64).reshape(-1, 8).sum(axis=0)
    n = t[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(abs_rel=t[1] / n, sq_rel=t[2] / n, rmse=np.sqrt(t[3] / n), rmse_log=np.sqrt(t[4] / n), a1=t[5] / n, a2=t[6] / n,
                    a3=t[7] / n)


def dvpq_from_frames(frames, num_classes, num_things, windows=(1, 2, 3, 4), depth_thrs=(0, 0.5, 0.25, 0.1), thr_bits=None):
    """`video_evaluate` from [(seq id, img id, table)]: frames ordered by (seq, img) as the file names order them, clips never span
    two sequences.  thr_bits: {threshold: mask bit}; a threshold of 0 means no relabelling"""
    frames = sorted(frames, key=lambda f: (int(f[0]), int(f[1])))
    if thr_bits is None:
        thr_bits = {t: j for j, t in enumerate(t for t in depth_thrs if t > 0.)}
    out = {}
    n = len(frames)
    for k in windows:
        for thr in depth_thrs:
            res = []
            for idx in range(n):
                if idx + k - 1 >= n:
                    break
                if int(frames[idx][0]) != int(frames[idx + k - 1][0]):
                    continue
                res.append(clip_tallies([frames[idx + j][2] for j in range(k)], thr_bits[thr] if thr > 0. else None, num_classes))
            if not res:
                continue
            iou, tp, fn, fp = (np.stack([r[j] for r in res]).sum(axis=0)[:num_classes] for j in range(4))
            sq = iou / (tp + _EPSILON)
            rq = tp / (tp + 0.5 * fn + 0.5 * fp + _EPSILON)
            pq = np.nan_to_num(sq * rq)
            out[(k, thr)] = (float(pq.mean() * 100), float(pq[:num_things].mean() * 100), float(pq[num_things:].mean() * 100))
    return out


class DeviceEvaluator:
    """DVPQ and the depth errors of a video run from maps that stay on the device.  `add_frames` makes one native call per batch
    (ph_dvpq_frames: launches only) into a ring of output slots and starts their download; nothing synchronises until a slot comes
    round again or `summarize` collects.  `summarize()` returns exactly `video_evaluate`'s dict."""

    def __init__(self, num_classes, num_things, windows=(1, 2, 3, 4), depth_thrs=(0, .5, .25, .1), capacity=8192, ring=4):
        from . import _lib
        self.num_classes, self.num_things = int(num_classes), int(num_things)
        self.windows, self.depth_thrs, self.capacity = tuple(windows), tuple(depth_thrs), int(capacity)
        pos = [t for t in dict.fromkeys(self.depth_thrs) if t > 0.]
        if len(pos) > _lib.PH_DVPQ_MAX_THR:
            raise ValueError(f"at most {_lib.PH_DVPQ_MAX_THR} depth thresholds above 0")
        self.thr_bits = {t: j for j, t in enumerate(pos)}
        self.ring = max(1, int(ring))
        self._slots = [None] * self.ring
        self._next = 0
        self._ws = {}                  # (device, B, H, W) -> (cfg, workspace): calls on one stream run in order and may share it
        self.frames = []               # (seq id, img id, table [n][4] uint32)
        self.depth_rows = []           # (seq id, img id, record [8] float64)

    def _plan(self, dev, B, H, W):
        from . import _lib
        key = (str(dev), B, H, W)
        if key not in self._ws:
            cfg = _lib.DvpqCfg(B=B, H=H, W=W, capacity=self.capacity, nthr=len(self.thr_bits))
            for t, j in self.thr_bits.items():
                cfg.thr[j] = t
            need = _lib.load().ph_dvpq_workspace_bytes(_lib.C.byref(cfg))
            if need == 0:
                _lib.check(-1, "ph_dvpq_workspace_bytes")
            self._ws[key] = (cfg, torch.empty(need, dtype=torch.uint8, device=dev), need)
        return self._ws[key]

    @staticmethod
    def _panseg(d):
        """uint32 ids as an int32 tensor, or None when the dict carries sem + track"""
        if "panseg" in d:
            t = d["panseg"]
            if t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                t = t.to(torch.int64).to(torch.int32)          # wraps like astype(uint32)
            return t.contiguous()
        return None

    def add_frames(self, seq_ids, img_ids, pred, gt):
        """pred: dict(panseg=[B, H, W] ids | sem=uint8 + track=float64 maps, depth=float32); gt: dict(panseg | sem + track, depth);
        device tensors.  One native call, no synchronisation."""
        from . import _lib
        depth = pred["depth"]
        if depth.dim() == 2:
            pred = {k: v[None] for k, v in pred.items()}
            gt = {k: v[None] for k, v in gt.items()}
            depth = pred["depth"]
        B, H, W = depth.shape
        if len(seq_ids) != B or len(img_ids) != B:
            raise ValueError("one (seq id, img id) per frame")
        dev = depth.device
        slot = self._next
        self._collect(slot)
        cfg, ws, need = self._plan(dev, B, H, W)
        pp = self._panseg(pred)
        ps = pt = None
        if pp is None:
            ps, pt = pred["sem"].to(torch.uint8).contiguous(), pred["track"].to(torch.float64).contiguous()
        gp = self._panseg(gt)
        if gp is None:
            gp = (gt["sem"].to(torch.int64) * INSTANCE_DIVISOR + gt["track"].to(torch.int64)).to(torch.int32).contiguous()
        pd, gd = depth.to(torch.float32).contiguous(), gt["depth"].to(torch.float32).contiguous()
        for t in (pp, ps, pt, gp, gd):
            if t is not None and tuple(t.shape) != (B, H, W):
                raise ValueError(f"every map must be [{B}, {H}, {W}], got {tuple(t.shape)}")
        table = torch.empty(B, 4 + 4 * self.capacity, dtype=torch.int32, device=dev)
        drec = torch.empty(B, 8, dtype=torch.float64, device=dev)
        io = _lib.DvpqIO(pred_panseg=_lib.ptr(pp), pred_sem=_lib.ptr(ps), pred_track=_lib.ptr(pt), pred_depth=_lib.ptr(pd), gt_panseg=_lib.ptr(gp),
                         gt_depth=_lib.ptr(gd), table_out=_lib.ptr(table), depth_out=_lib.ptr(drec))
        _lib.check(_lib.load().ph_dvpq_frames(_lib.C.byref(cfg), _lib.C.byref(io), _lib.ptr(ws), need, _lib.stream_ptr()), "ph_dvpq_frames")
        h_table = torch.empty(table.shape, dtype=torch.int32, pin_memory=True)
        h_drec = torch.empty(drec.shape, dtype=torch.float64, pin_memory=True)
        h_table.copy_(table, non_blocking=True)
        h_drec.copy_(drec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        # the inputs stay referenced until the slot is collected: the launches may not have run yet
        self._slots[slot] = (ev, h_table, h_drec, [int(s) for s in seq_ids], [int(i) for i in img_ids], (pp, ps, pt, pd, gp, gd, table, drec))
        self._next = (slot + 1) % self.ring

    def _collect(self, slot):
        s = self._slots[slot]
        if s is None:
            return
        self._slots[slot] = None
        ev, h_table, h_drec, seqs, imgs, _ = s
        ev.synchronize()
        tab = h_table.numpy().view(np.uint32)
        for b, (sq, im) in enumerate(zip(seqs, imgs)):
            n, over = int(tab[b, 0]), int(tab[b, 1])
            if over:
                raise RuntimeError(f"frame ({sq}, {im}) has more than capacity = {self.capacity} distinct (gt id, pred id, mask) keys: "
                                   "raise DeviceEvaluator's capacity")
            self.frames.append((sq, im, tab[b, 4:4 + 4 * n].reshape(n, 4).copy()))
            self.depth_rows.append((sq, im, h_drec[b].numpy().copy()))

    def collect(self):
        for i in range(self.ring):
            self._collect((self._next + i) % self.ring)

    def depth_errors(self):
        self.collect()
        rows = sorted(self.depth_rows, key=lambda r: (r[0], r[1]))
        return depth_errors_from_tallies(np.stack([r[2] for r in rows]))

    def summarize(self, with_depth=False):
        """-> `video_evaluate`'s dict {(k, lambda): (DVPQ, DVPQ_thing, DVPQ_stuff)}; with_depth: (that, `compute_errors`' dict)"""
        self.collect()
        res = dvpq_from_frames(self.frames, self.num_classes, self.num_things, self.windows, self.depth_thrs, self.thr_bits)
        return (res, self.depth_errors()) if with_depth else res


def video_evaluate_device(eval_dir, num_classes, num_things, windows=(1, 2, 3, 4), depth_thrs=(0, 0.5, 0.25, 0.1), capacity=8192, batch=8,
                          device="cuda", with_depth=False):
    """`video_evaluate` on the device: the same gt/ and pred/ .pth files, uploaded and scored through `DeviceEvaluator`"""
    gt_dir, pred_dir = os.path.join(eval_dir, "gt"), os.path.join(eval_dir, "pred")
    gts, preds = _pth_names(gt_dir), _pth_names(pred_dir)
    ev = DeviceEvaluator(num_classes, num_things, windows, depth_thrs, capacity)

    def up(recs, key, dtype):
        return torch.from_numpy(np.stack([np.asarray(r[key]).astype(dtype) for r in recs])).to(device)

    i = 0
    while i < len(preds):
        pr = [torch.load(os.path.join(pred_dir, preds[i]), weights_only=False)]
        gr = [torch.load(os.path.join(gt_dir, gts[i]), weights_only=False)]
        names = [preds[i]]
        i += 1
        while i < len(preds) and len(pr) < batch:           # a batch is frames of one size
            p = torch.load(os.path.join(pred_dir, preds[i]), weights_only=False)
            if np.asarray(p["panseg"]).shape != np.asarray(pr[0]["panseg"]).shape:
                break
            pr.append(p)
            gr.append(torch.load(os.path.join(gt_dir, gts[i]), weights_only=False))
            names.append(preds[i])
            i += 1
        ids = [n.split(".")[0].split("_") for n in names]
        ev.add_frames([int(a[0]) for a in ids], [int(a[1]) for a in ids],
                      dict(panseg=up(pr, "panseg", np.int64), depth=up(pr, "depth", np.float32)),
                      dict(panseg=up(gr, "panseg", np.int64), depth=up(gr, "depth", np.float32)))
    return ev.summarize(with_depth)
