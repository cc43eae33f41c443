"""Training-side losses of the hot path on libpolyhead's loss kernels (csrc/ph_loss.hip).

Registry names, constructor kwargs and attributes are the reference's: `FocalLoss`, `CrossEntropyLoss`, `DiceLoss`
(vendored mmdet, mmdet/models/losses/*.py) and `DepthLoss` (polyphonic/losses/depth_loss.py).  The modules hold the
configuration; `stage_losses` is what `KernelUpdateHead.loss` (kernel_update_head.py:355-441) runs: four `*_sums` passes
(mask BCE + dice, rank, depth, focal), a handful of scalars combined on the device in fp64 in a fixed order, and -- when
asked -- four `*_grad` passes that write d(sum of the stage's losses) / d(mask_pred, cls_score, depth_pred), the first
step of the backward pass.  The reference does the same arithmetic as ~40 ATen launches with boolean-mask gathers.
These functions evaluate values and d(losses)/d(predictions) without an autograd graph of their own; `train.py` wraps them
into one autograd node per head and stage (`_Objective`), behind which the hand-written backward of the forward kernels runs."""
import torch
import torch.nn as nn

from . import _lib
from .registry import LOSSES

DEPTH_MODES = {"sigmoid": 0, "monodepth": 1}


def _gpu(t, name):
    if not t.is_cuda:
        raise _lib.PolyheadError(f"{name} must live on the GPU: libpolyhead has no CPU path")


def _f32(t):
    return t.detach().contiguous().float()


# ---- the launches: sums (fixed-order fp64 records, combined here), gradients and targets (into the caller's buffers) ----------
def _run(name, *args):
    """queue libpolyhead's `name` on torch's current stream: tensors (None: NULL) go as pointers, everything else as it is"""
    _lib.check(getattr(_lib.load(), name)(*(_lib.ptr(a) if a is None or torch.is_tensor(a) else a for a in args), _lib.stream_ptr()), name)


def mask_loss_sums(pred, target, weight, pos_rows, nsplit=None):
    """pred / target / weight [R, HW] fp32, pos_rows int32 [P] -> float64 [P, 5] (BCE sum, count, a, b, c), fixed order"""
    P, HW = pos_rows.numel(), pred.shape[1]
    nsplit = nsplit or max(1, min(64, 2048 // max(P, 1)))
    out = torch.empty((P, nsplit, 5), dtype=torch.float64, device=pred.device)
    _run("ph_mask_loss_sums", pred, target, weight, pos_rows, P, HW, nsplit, out)
    return out.sum(1)


def rank_loss_sum(pred, rank_target, ignore):
    B, N, H, W = pred.shape
    out = torch.empty((B * _lib.load().ph_rank_loss_blocks(H * W),), dtype=torch.float64, device=pred.device)
    _run("ph_rank_loss_sum", pred, rank_target, B, N, H * W, ignore, out)
    return out.sum()


def depth_loss_sums(pred, target, weight, mode):
    total = pred.numel()
    out = torch.empty((_lib.load().ph_depth_loss_blocks(total), 5), dtype=torch.float64, device=pred.device)
    _run("ph_depth_loss_sums", pred, target, weight, total, mode, out)
    return out.sum(0)


def seg_focal_sum(pred, target, gamma, alpha):
    """pred [B, L, HW] fp32 (class-major, as conv_seg writes it), target int32 [B, HW] (== L: pixel not selected)"""
    B, L, HW = pred.shape
    out = torch.empty((B * _lib.load().ph_rank_loss_blocks(HW),), dtype=torch.float64, device=pred.device)
    _run("ph_seg_focal_sum", pred, target, B, L, HW, gamma, alpha, out)
    return out.sum()


def focal_loss_sum(pred, labels, weight, gamma, alpha):
    R, L = pred.shape
    out = torch.empty((_lib.load().ph_focal_loss_blocks(R * L),), dtype=torch.float64, device=pred.device)
    _run("ph_focal_loss_sum", pred, labels, weight, R, L, gamma, alpha, out)
    return out.sum()


def mask_loss_grad(pred, target, weight, pos_rows, coef, grad):
    """grad [R, HW] += d(BCE + dice) / d pred on the positive rows; coef float32 [P, 3] as ph_mask_loss_grad reads it"""
    _run("ph_mask_loss_grad", pred, target, weight, pos_rows, pos_rows.numel(), pred.shape[1], coef, grad)


def rank_loss_grad(pred, rank_target, B, N, HW, ignore, scale, grad):
    """grad [B * N, HW] = scale * d(rank cross entropy) / d pred; rank_target int32 [B, HW] or None (every pixel ignored)"""
    _run("ph_rank_loss_grad", pred, rank_target, B, N, HW, ignore, scale, grad)


def depth_loss_grad(pred, target, weight, mode, coef, grad):
    """grad = d DepthLoss / d pred, element for element; coef: the four coefficients of `_depth_from_sums`"""
    _run("ph_depth_loss_grad", pred, target, weight, pred.numel(), mode, *coef, grad)


def focal_loss_grad(pred, labels, weight, gamma, alpha, scale, grad):
    _run("ph_focal_loss_grad", pred, labels, weight, pred.shape[0], pred.shape[1], gamma, alpha, scale, grad)


def seg_focal_grad(pred, target, gamma, alpha, scale, grad):
    _run("ph_seg_focal_grad", pred, target, *pred.shape, gamma, alpha, scale, grad)


def rank_target(mask_targets, pos_u8, B, N, HW, ignore, out):
    """out int32 [B, HW]: pixel -> index (within its image) of the LAST positive row whose target covers it, else `ignore`"""
    _run("ph_rank_target", mask_targets, pos_u8, B, N, HW, ignore, out)


def seg_target(sem_seg, sem_cls, S, pos_masks, pos_labels, P, L, out):
    """out int64 [H, W] of one image: background L, the S stuff masks in order, then the P assigned thing masks in order"""
    _run("ph_seg_target", sem_seg, sem_cls, S, pos_masks, pos_labels, P, L, out.numel(), out)


# ---- loss modules (configuration holders with the reference's names) -----------------------------------------------------------
class _Loss(nn.Module):
    def __init__(self, use_sigmoid=False, loss_weight=1.0, reduction="mean", **kw):
        super().__init__()
        self.use_sigmoid, self.loss_weight, self.reduction = use_sigmoid, loss_weight, reduction
        self.cfg = dict(kw)


# the process group the focal normaliser is averaged over (None: the default group); train.TrainStep(group=...) sets it for
# the duration of its step so that a sub-group step neither averages over foreign ranks nor waits for them
_REDUCE_GROUP = [None]


class reduce_group:
    def __init__(self, group):
        self.group = group

    def __enter__(self):
        _REDUCE_GROUP.append(self.group)

    def __exit__(self, *exc):
        _REDUCE_GROUP.pop()
        return False


class FocalLoss(_Loss):
    """mmdet FocalLoss (focal_loss.py:160-244), the sigmoid form: forward(pred [R, L], target [R], weight [R, L], avg_factor)"""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0, activated=False, **kw):
        super().__init__(use_sigmoid, loss_weight, reduction, **kw)
        if not use_sigmoid or activated:
            raise NotImplementedError("libpolyhead: sigmoid focal loss on logits only (the shipped configs)")
        self.gamma, self.alpha = gamma, alpha

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        _gpu(pred, "pred")
        pred = _f32(pred)
        red = reduction_override or self.reduction
        if red not in ("mean", "sum") or (red == "sum" and avg_factor is not None):
            raise NotImplementedError("libpolyhead FocalLoss: reduction 'mean' (optionally with avg_factor) or 'sum'")
        if weight is None:
            w = torch.ones_like(pred)
        else:
            w = _f32(weight)
            if w.dim() == 1:                   # one weight per row, as mmdet reshapes it (focal_loss.py:60-69)
                w = w.view(-1, 1)
            w = w.expand_as(pred).contiguous()
        s = focal_loss_sum(pred, target.long().contiguous(), w, self.gamma, self.alpha)
        if avg_factor is not None:
            s = s / avg_factor
        elif red == "mean":
            s = s / pred.numel()
        return (self.loss_weight * s).float()


class CrossEntropyLoss(_Loss):
    """mmdet CrossEntropyLoss (cross_entropy_loss.py:163-251): the stage uses the sigmoid form on selected pixels (loss_mask)
    and the softmax form over the mask channels (loss_rank); both are evaluated inside `stage_losses`"""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None, ignore_index=None,
                 loss_weight=1.0, **kw):
        super().__init__(use_sigmoid, loss_weight, reduction, **kw)
        if use_mask or class_weight is not None:
            raise NotImplementedError("libpolyhead: use_mask / class_weight are not part of the shipped configs")
        self.ignore_index = ignore_index

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, ignore_index=None, **kw):
        """mmdet CrossEntropyLoss.forward on the device's loss kernels, the two forms the path uses:
        use_sigmoid: binary cross entropy of mask logits [R, P] against soft targets [R, P] (every pixel selected) --
          mean over all elements (cross_entropy_loss.py:56-105), what `loss_mask` evaluates;
        softmax: cross entropy over dim 1 of [B, N, H, W] (or [B, N, P]) logits against an index map [B, H, W] with
          `ignore_index` pixels contributing zero -- mean over all pixels (:9-53), what `loss_rank` evaluates.
        The heads themselves go through `stage_losses` / `rpn_losses`, which fuse these with the other losses."""
        red = reduction_override or self.reduction
        if weight is not None or avg_factor is not None or red != "mean":
            raise NotImplementedError("libpolyhead CrossEntropyLoss: mean reduction without weights (the shipped configs)")
        _gpu(cls_score, "cls_score")
        if self.use_sigmoid:
            z, t = _f32(cls_score).reshape(cls_score.shape[0], -1), _f32(label).reshape(cls_score.shape[0], -1)
            sel = torch.ones_like(z)
            sums = mask_loss_sums(z, t, sel, torch.arange(z.shape[0], device=z.device, dtype=torch.int32))
            return (self.loss_weight * sums[:, 0].sum() / z.numel()).float()
        ii = self.ignore_index if ignore_index is None else ignore_index
        z = _f32(cls_score)
        B, N = z.shape[:2]
        HW = z[0, 0].numel()
        tgt = label.reshape(B, HW).to(torch.int32).contiguous()
        s = rank_loss_sum(z.reshape(B, N, HW, 1), tgt, -100 if ii is None else int(ii))
        return (self.loss_weight * s / (B * HW)).float()


class DiceLoss(_Loss):
    """mmdet DiceLoss (dice_loss.py:49-136), sigmoid activation inside, eps 1e-3"""

    def __init__(self, use_sigmoid=True, activate=True, reduction="mean", loss_weight=1.0, eps=1e-3, **kw):
        super().__init__(use_sigmoid, loss_weight, reduction, **kw)
        if not (use_sigmoid and activate):
            raise NotImplementedError("libpolyhead: DiceLoss with the sigmoid inside (the shipped configs)")
        self.eps, self.activate = eps, activate

    def forward(self, pred, target, weight=None, reduction_override=None, avg_factor=None):
        """mmdet DiceLoss.forward (dice_loss.py:7-47,96-136): pred [R, P] logits, target [R, P]; per-row
        1 - 2 sum(p t) / ((sum(p^2) + eps) + (sum(t^2) + eps)) with p = sigmoid(pred), mean over the rows"""
        red = reduction_override or self.reduction
        if weight is not None or avg_factor is not None or red != "mean":
            raise NotImplementedError("libpolyhead DiceLoss: mean reduction without weights (the shipped configs)")
        _gpu(pred, "pred")
        z, t = _f32(pred).reshape(pred.shape[0], -1), _f32(target).reshape(pred.shape[0], -1)
        sums = mask_loss_sums(z, t, torch.ones_like(z), torch.arange(z.shape[0], device=z.device, dtype=torch.int32))
        dice = 1.0 - 2.0 * sums[:, 2] / (sums[:, 3] + sums[:, 4] + 2.0 * self.eps)          # dice_loss.py:33-38
        return (self.loss_weight * dice.mean()).float()


def _depth_value_from_sums(s, loss_weight, w3):
    """DepthLoss from the five sums (depth_loss.py:19-32), an fp64 scalar tensor, 0 where no pixel is labelled.  All on the
    device: the host never reads n"""
    n = s[0]
    si = s[1] / n - s[2] / (n * n)                      # as the reference writes it: sum(log_minus) / n^2, not its square
    sq = torch.sqrt(s[3] / n)
    ab = s[4] / n
    loss = (loss_weight / 3.0) * (w3[0] * si + w3[1] * sq + w3[2] * ab)
    return torch.where(n == 0, torch.zeros_like(loss), loss)


def _depth_from_sums(s, loss_weight, w3):
    """(that value, the four coefficients of the gradient pass): those the host forms, so it reads n and the sq_rel root"""
    loss, n = _depth_value_from_sums(s, loss_weight, w3), float(s[0])
    if n == 0.0:
        return loss, (0.0, 0.0, 0.0, 0.0)
    K, sq = loss_weight / 3.0, float(torch.sqrt(s[3] / s[0]))
    return loss, (K * w3[0] * 2.0 / n, -K * w3[0] / (n * n), (K * w3[1] / (n * sq)) if sq > 0 else 0.0, K * w3[2] / n)


def _depth_terms(ld, dp, dt, dw, want_grad, grad_out=None):
    """DepthLoss `ld` of the contiguous fp32 prediction dp against targets / weights of its size: (float32 loss, d loss / d dp or
    None).  The gradient goes into `grad_out` where given.  Without `want_grad` nothing here waits for the device."""
    mode, w3 = DEPTH_MODES[ld.depth_act_mode], [float(v) for v in ld.weight]
    dt, dw = _f32(dt), _f32(dw)
    sums = depth_loss_sums(dp, dt, dw, mode)
    if not want_grad:
        return _depth_value_from_sums(sums, ld.loss_weight, w3).float(), None
    loss, coef = _depth_from_sums(sums, ld.loss_weight, w3)
    g = torch.empty_like(dp) if grad_out is None else grad_out
    depth_loss_grad(dp, dt, dw, mode, coef, g)
    return loss.float(), g


class DepthLoss(_Loss):
    """polyphonic/losses/depth_loss.py:36-65: forward(pred logits, target, mask_weight) -> loss_weight * mean(weight * (si, sq_rel, abs_rel))"""

    def __init__(self, loss_weight=1.0, depth_act_mode="monodepth", si_weight=1.0, sq_rel_weight=1.0, abs_rel_weight=1.0, **kw):
        super().__init__(False, loss_weight, "mean", **kw)
        self.depth_act_mode = depth_act_mode
        self.weight = torch.tensor([si_weight, sq_rel_weight, abs_rel_weight], dtype=torch.float32)

    def forward(self, pred, target, mask_weight, reduction_override="mean", **kwargs):
        if not torch.any(self.weight > 0):
            return (pred * 0).sum()
        _gpu(pred, "pred")
        s = depth_loss_sums(_f32(pred), _f32(target), _f32(mask_weight), DEPTH_MODES[self.depth_act_mode])
        loss = _depth_value_from_sums(s, self.loss_weight, [float(v) for v in self.weight])
        if reduction_override == "sum":
            loss = loss * 3.0
        return loss.float()


for _n, _c in (("FocalLoss", FocalLoss), ("CrossEntropyLoss", CrossEntropyLoss), ("DiceLoss", DiceLoss), ("DepthLoss", DepthLoss)):
    LOSSES.register_module(name=_n, module=_c, force=True)


def _mask_terms(head, mp, mask_targets, mask_weights, pos, B, N, H, W, losses, grad, keys, empty_keys):
    """The mask part both heads share (kernel_update_head.py:404-441, kernel_head.py:503-536): BCE mean over the selected
    pixels of the positive rows, the mean of the per-row dice losses, the rank cross-entropy.  mp [R, HW] fp32; `grad` (or
    None) [R, HW] receives d(sum of the three) / d(mask_pred).  `keys` / `empty_keys` name the entries with / without
    positives (the reference's names differ between the two cases)."""
    dev = mp.device
    R, HW = B * N, H * W
    ignore, lr = head.ignore_label, head.loss_rank
    num_pos = int(pos.sum())
    if not num_pos:
        z = torch.zeros((), device=dev)
        losses[empty_keys[0]], losses[empty_keys[1]] = z, z.clone()
        if lr is not None:
            losses[empty_keys[2]] = z.clone()
        if grad is not None:
            grad.zero_()
        return
    mt, mw = _f32(mask_targets).reshape(R, HW), _f32(mask_weights).reshape(R, HW)
    rows = pos.nonzero().flatten().to(torch.int32).contiguous()
    s = mask_loss_sums(mp, mt, mw, rows)                                                       # [P, 5] fp64
    ntot = s[:, 1].sum()
    lm, ldice = head.loss_mask, head.loss_dice
    losses[keys[0]] = (lm.loss_weight * s[:, 0].sum() / ntot).float()                          # BCE mean over the selected pixels
    bc = s[:, 3] + s[:, 4] + 2 * ldice.eps
    losses[keys[1]] = (ldice.loss_weight * (1 - 2 * s[:, 2] / bc).mean()).float()
    if lr is not None:
        rt = torch.empty((B, HW), dtype=torch.int32, device=dev)
        rank_target(mt, pos.to(torch.uint8).contiguous(), B, N, HW, ignore, rt)
        losses[keys[2]] = (lr.loss_weight * rank_loss_sum(mp.reshape(B, N, H, W), rt, ignore) / (B * HW)).float()
    if grad is not None:
        if lr is not None:
            rank_loss_grad(mp, rt, B, N, HW, ignore, lr.loss_weight / (B * HW), grad)
        else:
            grad.zero_()
        P = rows.numel()
        coef = torch.stack([torch.full((P,), lm.loss_weight, dtype=torch.float64, device=dev) / ntot,
                            -2.0 * ldice.loss_weight / (P * bc), 4.0 * ldice.loss_weight * s[:, 2] / (P * bc * bc)], 1)
        mask_loss_grad(mp, mt, mw, rows, coef.float().contiguous(), grad)


# ---- one stage -----------------------------------------------------------------------------------------------------------------
def stage_losses(head, cls_score, mask_pred, depth_pred, labels, label_weights, mask_targets, mask_weights, depth_targets,
                 depth_weights, with_grads=False):
    """KernelUpdateHead.loss (kernel_update_head.py:355-441).  cls_score [B, N, L], mask_pred / depth_pred [B, N, H, W] (at the
    assign stride), targets as `get_targets` returns them.  Returns the reference's dict of losses (+ 'pos_acc'); with
    `with_grads` also dict(mask_pred=, cls_score=, depth_pred=) = d(sum of the losses) / d(prediction)."""
    _gpu(mask_pred, "mask_pred")
    dev = mask_pred.device
    B, N, H, W = mask_pred.shape
    R, HW, L = B * N, H * W, head.num_classes
    mp, dp, cs = _f32(mask_pred).reshape(R, HW), _f32(depth_pred).reshape(R, HW), _f32(cls_score).reshape(R, -1)
    labels = labels.to(dev).long().contiguous()
    pos = (labels >= 0) & (labels < L)                                                        # :375
    num_pos = int(pos.sum())
    from .dist import reduce_mean
    avg = max(float(reduce_mean(pos.sum().float(), _REDUCE_GROUP[-1])), 1.0)                  # :376-377 (mean over ranks, clamp)
    losses = {}
    grads = dict(mask_pred=torch.empty_like(mp).view(B, N, H, W), cls_score=torch.empty_like(cs).view(B, N, -1),
                 depth_pred=torch.empty_like(dp).view(B, N, H, W)) if with_grads else None
    flat = lambda k: grads[k].view(R, -1) if with_grads else None             # the kernels write [R, .] rows
    # ---- depth (:383-391)
    losses["loss_depth"], _ = _depth_terms(head.loss_depth, dp, depth_targets, depth_weights, with_grads, flat("depth_pred"))
    # ---- classification (:393-402)
    lc = head.loss_cls
    lw = _f32(label_weights).reshape(R, -1)
    losses["loss_cls"] = (lc.loss_weight * focal_loss_sum(cs, labels, lw, lc.gamma, lc.alpha) / avg).float()
    if num_pos:
        losses["pos_acc"] = (cs[pos].argmax(1) == labels[pos]).float().sum() * (100.0 / num_pos)       # mmdet accuracy, top-1
    else:
        losses["pos_acc"] = torch.zeros((), device=dev)
    if with_grads:
        focal_loss_grad(cs, labels, lw, lc.gamma, lc.alpha, lc.loss_weight / avg, flat("cls_score"))
    # ---- masks (:404-437)
    _mask_terms(head, mp, mask_targets, mask_weights, pos, B, N, H, W, losses, flat("mask_pred"),
                ("loss_rpn_mask", "loss_rpn_dice", "loss_rank"), ("loss_mask", "loss_dice", "loss_rank"))
    return (losses, grads) if with_grads else losses


# ---- targets (kernel_update_head.py:443-591) ------------------------------------------------------------------------------------
def target_single(head, pos_inds, neg_inds, pos_mask, neg_mask, pos_gt_mask, pos_gt_labels, gt_sem_seg, gt_sem_cls, pos_depth,
                  neg_depth, gt_depth, gt_valid, cfg):
    """_get_target_single (:443-531): labels / weights / mask and depth targets of ONE image, tensors stay on their device"""
    dev = pos_mask.device
    num_pos, num_neg = pos_mask.shape[0], neg_mask.shape[0]
    R = num_pos + num_neg
    H, W = pos_mask.shape[-2:]
    L, ns, nt = head.num_classes, head.num_stuff_classes, head.num_thing_classes
    pw = 1.0 if cfg.pos_weight <= 0 else cfg.pos_weight
    valid = gt_valid.to(dev).float()
    labels = torch.full((R,), L, dtype=torch.long, device=dev)
    label_weights = torch.zeros((R, L), device=dev)
    mask_targets = torch.zeros((R, H, W), device=dev)
    mask_weights = valid[None].expand(R, H, W).clone()                    # 1 on the valid pixels of every row
    if num_pos:
        labels[pos_inds] = pos_gt_labels
        label_weights[pos_inds] = pw
        mask_targets[pos_inds] = pos_gt_mask.float()
    if num_neg:
        label_weights[neg_inds] = 1.0
    sem_rows = None
    if gt_sem_cls is not None and gt_sem_seg is not None:
        sem_labels = torch.full((ns,), L, dtype=torch.long, device=dev)
        sem_targets = torch.zeros((ns, H, W), device=dev)
        sem_weights = torch.zeros((ns, H, W), device=dev)
        sem_label_weights = torch.cat([torch.zeros((ns, nt), device=dev), torch.eye(ns, device=dev)], -1)
        if len(gt_sem_cls) > 0:
            sem_rows = (gt_sem_cls - nt).long()
            sem_labels[sem_rows] = gt_sem_cls.long()
            sem_targets[sem_rows] = gt_sem_seg.float()
            sem_weights[sem_rows] = 1
        sem_weights = sem_weights * valid
        label_weights[:, nt:] = 0
        labels = torch.cat([labels, sem_labels])
        label_weights = torch.cat([label_weights, sem_label_weights])
        mask_targets = torch.cat([mask_targets, sem_targets])
        mask_weights = torch.cat([mask_weights, sem_weights])
    depth_targets = depth_weights = None
    if pos_depth is not None:
        assert neg_depth is not None and gt_depth is not None
        Rd = R + ns
        gd = gt_depth.to(dev).float().reshape(H, W)           # [H, W] or [1, H, W] (the batched gt_depth of forward_train)
        depth_targets = torch.zeros((Rd, H, W), device=dev)
        depth_weights = torch.zeros((Rd, H, W), device=dev)
        if num_pos:
            depth_targets[pos_inds] = gd
            depth_weights[pos_inds] = pw * pos_gt_mask.float()
        if sem_rows is not None:
            depth_targets[sem_rows + R] = gd
            depth_weights[sem_rows + R] = gt_sem_seg.float() * pw
        depth_targets[-1] = gd                                            # the direct depth row (:525-528)
        depth_weights[-1] = 1.0
        depth_weights = depth_weights * (gd > 0.0).float()
    return labels, label_weights, mask_targets, mask_weights, depth_targets, depth_weights


def get_targets(head, sampling_results, gt_mask, gt_labels, rcnn_train_cfg, concat=True, gt_sem_seg=None, gt_sem_cls=None,
                gt_depth=None):
    """KernelUpdateHead.get_targets (:533-591)"""
    n = len(sampling_results)
    if gt_sem_seg is None:
        gt_sem_seg, gt_sem_cls = [None] * n, [None] * n
    has_depth = gt_depth is not None
    outs = []
    for i, res in enumerate(sampling_results):
        outs.append(target_single(head, res.pos_inds, res.neg_inds, res.pos_masks, res.neg_masks, res.pos_gt_masks, res.pos_gt_labels,
                                  gt_sem_seg[i], gt_sem_cls[i], res.pos_depth if has_depth else None,
                                  res.neg_depth if has_depth else None, gt_depth[i] if has_depth else None, res.valid_mask,
                                  rcnn_train_cfg))
    cols = list(zip(*outs))
    if concat:
        cols = [torch.cat(c, 0) if c[0] is not None else None for c in cols]
    return tuple(cols)


# ---- KernelHead (the rpn side): kernel_head.py:456-698 --------------------------------------------------------------------------
def rpn_losses(head, mask_pred, seg_preds, depth_pred, labels, label_weights, mask_targets, mask_weights, seg_targets,
               depth_targets, depth_weights, with_grads=False):
    """KernelHead.loss (kernel_head.py:456-569) for the shipped configuration (no cls_scores, no semantic_aspp): loss_depth on
    the direct depth map broadcast over the N rows, loss_rpn_mask / loss_rpn_dice / loss_rpn_rank on the positive rows,
    loss_rpn_seg = sigmoid focal loss of conv_seg's map over the labelled pixels.  mask_pred [B, N, H, W], seg_preds
    [B, L, H, W], depth_pred [B, 1 or N + stuff rows, H, W].  With `with_grads`: dict(mask_pred=, seg_preds=, depth_pred= [B, 1, H, W])."""
    _gpu(mask_pred, "mask_pred")
    dev = mask_pred.device
    B, N, H, W = mask_pred.shape
    R, HW, L = B * N, H * W, head.num_classes
    mp = _f32(mask_pred).reshape(R, HW)
    labels = labels.to(dev).long().contiguous()
    pos = (labels >= 0) & (labels < L)                                                        # :475
    losses = {}
    grads = dict(mask_pred=torch.empty_like(mp).view(B, N, H, W)) if with_grads else None
    if depth_pred is not None:                                                               # :478-486
        Rd = depth_targets.shape[0]               # B * (proposals + stuff rows): one broadcast map per image (:386,482)
        dp = _f32(depth_pred.expand(B, Rd // B, H, W)).reshape(Rd, HW)
        losses["loss_depth"], g = _depth_terms(head.loss_depth, dp, depth_targets, depth_weights, with_grads)
        if with_grads:
            grads["depth_pred"] = g.reshape(B, Rd // B, H, W).sum(1, keepdim=True)           # the rows are one broadcast map
    _mask_terms(head, mp, mask_targets, mask_weights, pos, B, N, H, W, losses, grads["mask_pred"].view(R, HW) if with_grads else None,
                ("loss_rpn_mask", "loss_rpn_dice", "loss_rpn_rank"), ("loss_rpn_mask", "loss_rpn_dice", "loss_rank"))
    if seg_preds is not None:                                                                 # :538-551
        ls = head.loss_seg
        if not ls.use_sigmoid:
            raise NotImplementedError("libpolyhead: loss_seg is the shipped sigmoid FocalLoss (polyphonic_former.py:73-78)")
        sp = _f32(seg_preds).reshape(B, seg_preds.shape[1], HW)
        st = seg_targets.to(dev).reshape(B, HW)
        nd = max(float(((st >= 0) & (st < L)).sum()), 1.0)                                    # num_dense_pos.clamp(min=1)
        st = st.to(torch.int32).contiguous()
        losses["loss_rpn_seg"] = (ls.loss_weight * seg_focal_sum(sp, st, ls.gamma, ls.alpha) / nd).float()
        if with_grads:
            g = torch.empty_like(sp)
            seg_focal_grad(sp, st, ls.gamma, ls.alpha, ls.loss_weight / nd, g)
            grads["seg_preds"] = g.reshape(seg_preds.shape)
    return (losses, grads) if with_grads else losses


def dense_depth_loss(head, depth_pred, gt_depth, with_grad=False):
    """losses['depth_dense'] (kernel_head.py:438-442): DepthLoss of the direct depth map against the ground truth, weight = gt > 0"""
    dp, gd = _f32(depth_pred).reshape(-1), _f32(gt_depth.to(depth_pred.device)).reshape(-1)
    if dp.numel() != gd.numel():
        raise ValueError(f"depth_dense: prediction {tuple(depth_pred.shape)} and gt_depth {tuple(gt_depth.shape)} differ in size")
    # without the gradient this is the logged value of a training step: nothing here waits for the device
    loss, g = _depth_terms(head.loss_depth, dp, gd, (gd > 0).float(), with_grad)
    return (loss, g.reshape(depth_pred.shape)) if with_grad else loss


def rpn_target_single(head, pos_inds, neg_inds, pos_mask, neg_mask, pos_gt_mask, pos_gt_labels, gt_sem_seg, gt_sem_cls, pos_depth,
                      neg_depth, gt_depth, gt_valid, cfg):
    """KernelHead._get_target_single (kernel_head.py:571-647): ONE image.  Unlike the update heads there are no stuff rows in
    labels / masks (label_weights is per row), a dense `seg_targets` map [H, W] (stuff classes first, then the assigned thing
    masks painted over them in order) and depth rows for the N proposals + the stuff rows, without a direct-depth row."""
    _gpu(pos_mask, "sampling result")
    dev = pos_mask.device
    num_pos, num_neg = pos_mask.shape[0], neg_mask.shape[0]
    R = num_pos + num_neg
    H, W = pos_mask.shape[-2:]
    L, ns, nt = head.num_classes, head.num_stuff_classes, head.num_thing_classes
    pw = 1.0 if cfg.pos_weight <= 0 else cfg.pos_weight
    valid = gt_valid.to(dev).float()
    labels = torch.full((R,), L, dtype=torch.long, device=dev)
    label_weights = torch.zeros((R,), device=dev)
    mask_targets = torch.zeros((R, H, W), device=dev)
    mask_weights = valid[None].expand(R, H, W).clone()
    has_sem = gt_sem_cls is not None and gt_sem_seg is not None
    S = len(gt_sem_cls) if has_sem else 0
    if num_pos:
        labels[pos_inds] = pos_gt_labels
        label_weights[pos_inds] = pw
        mask_targets[pos_inds] = pos_gt_mask.float()
    # the dense semantic target in one pass: stuff classes in order, then the assigned thing masks in order (:590-605)
    seg_targets = torch.empty((H, W), dtype=torch.long, device=dev)
    sem_f = gt_sem_seg.to(dev).float().contiguous() if S else None
    sem_c = gt_sem_cls.to(dev).long().contiguous() if S else None
    pgm = pos_gt_mask.float().contiguous() if num_pos else None
    pgl = pos_gt_labels.to(dev).long().contiguous() if num_pos else None
    seg_target(sem_f, sem_c, S, pgm, pgl, num_pos, L, seg_targets)
    if num_neg:
        label_weights[neg_inds] = 1.0
    depth_targets = depth_weights = None
    if pos_depth is not None:                                                                 # :610-640
        assert neg_depth is not None and gt_depth is not None
        gd = gt_depth.to(dev).float().reshape(H, W)
        depth_targets = torch.zeros((R + ns, H, W), device=dev)
        depth_weights = torch.zeros((R + ns, H, W), device=dev)
        if num_pos:
            depth_targets[pos_inds] = gd
            depth_weights[pos_inds] = pw * pos_gt_mask.float()
        if has_sem and len(gt_sem_cls) > 0:
            rows = (gt_sem_cls - nt).long() + R
            depth_targets[rows] = gd
            depth_weights[rows] = gt_sem_seg.float() * pw
        depth_weights = depth_weights * (gd > 0.0).float()
    return labels, label_weights, mask_targets, mask_weights, seg_targets, depth_targets, depth_weights


def rpn_get_targets(head, sampling_results, gt_mask, rpn_train_cfg, concat=True, gt_sem_seg=None, gt_sem_cls=None, gt_depth=None):
    """KernelHead.get_targets (kernel_head.py:649-698): per image, concatenated (seg_targets stacked)"""
    n = len(sampling_results)
    if gt_sem_seg is None:
        gt_sem_seg, gt_sem_cls = [None] * n, [None] * n
    has_depth = gt_depth is not None
    outs = []
    for i, res in enumerate(sampling_results):
        outs.append(rpn_target_single(head, res.pos_inds, res.neg_inds, res.pos_masks, res.neg_masks, res.pos_gt_masks,
                                      res.pos_gt_labels, gt_sem_seg[i], gt_sem_cls[i], res.pos_depth if has_depth else None,
                                      res.neg_depth if has_depth else None, gt_depth[i] if has_depth else None, res.valid_mask,
                                      rpn_train_cfg))
    cols = list(zip(*outs))
    if concat:
        cols = [None if c[0] is None else (torch.stack(c, 0) if k == 4 else torch.cat(c, 0)) for k, c in enumerate(cols)]
    return tuple(cols)


# =================================================================================================================================
# Round 5: the training path's targets + losses from DESCRIPTORS (csrc/ph_loss.hip `ph_train_losses`; include/polyhead.h).
# `get_targets` / `loss` above stay what the reference's API exposes (materialised [rows][H][W] targets, bit for bit); the
# heads' `forward_train` -- `train.rpn_forward_train` / `train.roi_forward_train` -- no longer goes through them: the Hungarian
# result lives on the host, every target row is a ground-truth row that already lies in HBM, so the host writes pointer tables
# (numpy, ~100 us), uploads them in one copy and ONE C call evaluates the head's or stage's losses and gradients.
# =================================================================================================================================
import copy  # noqa: E402
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402


LossCfg = _lib.LossCfg                 # ph_loss_cfg


class StepGT:
    """one training step's ground truth where the descriptors point: per image contiguous fp32 masks [G, H, W] (hardened when
    `hard_target`), stuff masks [S, H, W], the valid map (any mask set: kernel_head.py:415, kernel_update.py:238), the depth
    map; labels / stuff classes also on the host; the zero-padded stack [B, Gmax, H, W] the batched assignment reads"""

    def __init__(self, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_depth, hard_target):
        B = len(gt_masks)
        dev = gt_masks[0].device
        f = lambda t: t.detach().float().contiguous()
        self.masks = [f(m.bool()) if hard_target else f(m) for m in gt_masks]
        self.has_sem = gt_sem_seg is not None and gt_sem_cls is not None
        self.sem = [f(s) for s in gt_sem_seg] if self.has_sem else [self.masks[0][:0]] * B
        self.H, self.W = self.masks[0].shape[-2:]
        HW = self.HW = self.H * self.W
        self.G = [int(m.shape[0]) for m in self.masks]
        self.S = [int(s.shape[0]) for s in self.sem]
        valid = torch.zeros((B, self.H, self.W), dtype=torch.float32, device=dev)
        for i in range(B):
            for t in (self.masks[i], self.sem[i]):
                if t.shape[0]:
                    valid[i] += t.ne(0).any(dim=0)
        self.valid = (valid > 0).float()
        if isinstance(gt_depth, (list, tuple)):
            gt_depth = torch.stack([d.reshape(self.H, self.W) for d in gt_depth])
        self.depth = None if gt_depth is None else f(gt_depth.to(dev)).reshape(B, HW)
        # host copies of the small integer lists (ONE synchronising read per step)
        lab = torch.cat([l.reshape(-1).long() for l in gt_labels] + ([c.reshape(-1).long() for c in gt_sem_cls] if self.has_sem else []))
        lab = lab.cpu().numpy()
        o = np.cumsum([0] + self.G + (self.S if self.has_sem else []))
        self.labels_h = [lab[o[i]:o[i + 1]] for i in range(B)]
        self.sem_cls_h = [lab[o[B + i]:o[B + i + 1]] for i in range(B)] if self.has_sem else [np.zeros(0, np.int64)] * B
        self.labels_dev = [l.reshape(-1).long() for l in gt_labels]
        self.Gmax = max(self.G + [0])
        self.pad = torch.zeros((B, max(self.Gmax, 1), self.H, self.W), dtype=torch.float32, device=dev)
        for i in range(B):
            if self.G[i]:
                self.pad[i, :self.G[i]] = self.masks[i]
        self.mask_base = np.array([m.data_ptr() for m in self.masks], dtype=np.int64)
        self.sem_base = np.array([s.data_ptr() for s in self.sem], dtype=np.int64)
        self.valid_base = self.valid.data_ptr() + 4 * HW * np.arange(B, dtype=np.int64)
        self.depth_base = None if self.depth is None else self.depth.data_ptr() + 4 * HW * np.arange(B, dtype=np.int64)
        self.B = B
        self._table = None                  # `device_table`
        self.status_words = []              # one int64 [B] device tensor per device solve of the step (`assign_desc_device`)

    @classmethod
    def from_prepared(cls, things, G, labels_h, labels_dev, valid, stuff=None, S=None, sem_cls_h=None, depth=None):
        """the same object over buffers `ph_gt_prepare` wrote (gt.PreparedGT.step_gt): things [B, max(Gmax, 1), H, W] with zero rows
        beyond G[b] -- the soft or the hardened stack -- is `pad` as it stands and every image's masks are its leading rows; stuff
        [B, Smax, H, W] or None (no stuff targets, as `StepGT(m, l, None, None, None, h)`); valid [B, H, W]; depth [B, H, W] or None;
        labels_h / sem_cls_h the host lists, labels_dev their device copies.  No pass over the masks, no device -> host read."""
        self = cls.__new__(cls)
        B = self.B = len(G)
        self.H, self.W = things.shape[-2:]
        HW = self.HW = self.H * self.W
        self.G = [int(g) for g in G]
        self.Gmax = max(self.G + [0])
        if tuple(things.shape) != (B, max(self.Gmax, 1), self.H, self.W) or tuple(valid.shape) != (B, self.H, self.W):
            raise ValueError("StepGT.from_prepared: things must be [B, max(Gmax, 1), H, W] and valid [B, H, W]")
        self.pad = things
        self.masks = [things[b, :self.G[b]] for b in range(B)]
        self.has_sem = stuff is not None
        self.S = [int(s) for s in S] if self.has_sem else [0] * B
        self.sem = [stuff[b, :self.S[b]] for b in range(B)] if self.has_sem else [self.masks[0][:0]] * B
        self.valid = valid
        self.depth = None if depth is None else depth.reshape(B, HW)
        self.labels_h = [np.asarray(l, np.int64) for l in labels_h]
        self.sem_cls_h = [np.asarray(c, np.int64) for c in sem_cls_h] if self.has_sem else [np.zeros(0, np.int64)] * B
        self.labels_dev = list(labels_dev)
        rows = np.arange(B, dtype=np.int64)
        self.mask_base = things.data_ptr() + 4 * HW * things.shape[1] * rows
        self.sem_base = stuff.data_ptr() + 4 * HW * stuff.shape[1] * rows if self.has_sem else np.array([s.data_ptr() for s in self.sem], np.int64)
        self.valid_base = valid.data_ptr() + 4 * HW * rows
        self.depth_base = None if depth is None else depth.data_ptr() + 4 * HW * rows
        self._table = None
        self.status_words = []
        return self

    def device_table(self):
        """the ground-truth table `ph_assign_desc` reads (include/polyhead.h): per image the counts, the base addresses and where
        its labels and stuff classes lie, then those.  int64 on the device, built and uploaded on first use, once per step."""
        if self._table is None:
            B, W = self.B, _lib.PH_ASSIGN_GT_WORDS
            tab = np.zeros(B * W + sum(self.G) + sum(len(c) for c in self.sem_cls_h), np.int64)
            o = B * W
            for b in range(B):
                S = len(self.sem_cls_h[b])
                tab[b * W:(b + 1) * W] = [self.G[b], S, self.mask_base[b], self.sem_base[b], self.valid_base[b],
                                          0 if self.depth_base is None else self.depth_base[b], o, o + self.G[b]]
                tab[o:o + self.G[b]] = self.labels_h[b]
                tab[o + self.G[b]:o + self.G[b] + S] = self.sem_cls_h[b]
                o += self.G[b] + S
            self._table = torch.from_numpy(tab).to(self.pad.device, non_blocking=True)
        return self._table

    def all_pixels(self):
        """the same ground truth without its valid map, as an assigner that counts every pixel reads it (MaskHungarianAssigner,
        assigner.py:199-360): a shallow copy -- the tensors, the lists and `status_words` are this object's own"""
        v = copy.copy(self)
        v.valid = None
        return v


def _assign_cost(assigner, pred, cls_pred, gt):
    """the [B, Np, Gmax] matching cost of B images from ONE `ph_match_sums` pass (funcs/assigner.py:363-542 per image): class,
    mask and dice terms in this order, torch ops on the device.  Both assignment paths solve exactly this tensor."""
    from .assigner import MatchSums
    B, Np = pred.shape[:2]
    s = MatchSums(pred, gt.pad, gt.valid)
    cost = 0
    a = assigner
    if a.cls_cost.weight != 0 and cls_pred is not None:
        cc = a.cls_cost
        p = cls_pred.sigmoid()
        neg = -(1 - p + cc.eps).log() * (1 - cc.alpha) * p.pow(cc.gamma)
        pos = -(p + cc.eps).log() * cc.alpha * (1 - p).pow(cc.gamma)
        lab = torch.zeros((B, gt.Gmax), dtype=torch.long, device=pred.device)
        for i in range(B):
            if gt.G[i]:
                lab[i, :gt.G[i]] = gt.labels_dev[i]
        idx = lab[:, None, :].expand(B, Np, gt.Gmax)
        cost = cost + (pos.gather(2, idx) - neg.gather(2, idx)) * cc.weight
    if a.mask_cost.weight != 0:
        V = s.V[:, None, None]
        cost = cost + (-(s.A + (V - s.S[:, :, None] - s.T[:, None, :] + s.A)) / V * a.mask_cost.weight)
    if a.dice_cost.weight != 0:
        e = a.dice_cost.eps
        cost = cost + (-(2 * s.A) / ((s.Q + e)[:, :, None] + (s.C + e)[:, None, :]) * a.dice_cost.weight)
    return cost


def assign_batch(assigner, pred, cls_pred, gt):
    """the Hungarian assignment of B images from ONE `ph_match_sums` pass and ONE device -> host copy (funcs/assigner.py:363-542
    per image).  pred [B, Np, H, W] detached mask logits, cls_pred [B, Np, n_thing] or None.  -> per image (pred indices
    ascending, matched gt indices) as numpy arrays.  Configurations the batched algebra does not cover (DepthCost with a weight,
    topk > 1) are refused by the caller."""
    from .assigner import _hungarian
    B, Np = pred.shape[:2]
    out = [(np.zeros(0, np.int64), np.zeros(0, np.int64))] * B
    if gt.Gmax == 0:
        return out
    cost = _assign_cost(assigner, pred, cls_pred, gt)
    cost = cost.detach().cpu().numpy()
    for i in range(B):
        if gt.G[i]:
            r, c = _hungarian(torch.from_numpy(cost[i, :, :gt.G[i]]), 1)
            order = np.argsort(r, kind="stable")
            out[i] = (np.asarray(r)[order].astype(np.int64), np.asarray(c)[order].astype(np.int64))
    return out


def assign_match(assigner, pred, cls_pred, gt, device_assign=False):
    """the same assignment as a table on the device: `match` int32 [B, max(Gmax, 1)], the prediction row of every ground truth or
    -1.  Host path: `assign_batch` (one download, scipy) and one upload.  device_assign: the cost stays where `_assign_cost` forms
    it and `ph_assign_solve` solves it (its status words are appended to gt.status_words); beyond the kernel's limits, or with
    every cost weight zero, the host path runs."""
    B, Np = pred.shape[:2]
    ld, dev = max(gt.Gmax, 1), pred.device
    if gt.Gmax == 0:
        return torch.full((B, ld), -1, dtype=torch.int32, device=dev)
    if device_assign and max(Np, gt.Gmax) <= _lib.PH_ASSIGN_MAX:
        cost = _assign_cost(assigner, pred, cls_pred, gt)
        if torch.is_tensor(cost):
            cost = cost.detach().float().contiguous()
            match = torch.full((B, ld), -1, dtype=torch.int32, device=dev)
            status = torch.empty((B,), dtype=torch.int64, device=dev)
            counts = gt.device_table().view(torch.int32)                   # word 0 of every record: G_b (little endian int64)
            _lib.check(_lib.load().ph_assign_solve(_lib.ptr(cost), B, Np, ld, _lib.ptr(counts), 2 * _lib.PH_ASSIGN_GT_WORDS, _lib.ptr(match),
                                                   _lib.ptr(status), _lib.stream_ptr()), "ph_assign_solve")
            gt.status_words.append(status)
            return match
    rows = np.full((B, ld), -1, np.int32)
    for i, (r, c) in enumerate(assign_batch(assigner, pred, cls_pred, gt)):
        rows[i, c] = r
    return torch.from_numpy(rows).to(dev, non_blocking=True)


class LossDesc:
    """the pointer tables of one head / stage on the device + what the host knows about them: everything `fused_losses` reads.
    blob: the tables, uint8 on the device; offsets / n: per table its byte offset in the blob and its entry count; N rows per image,
    P of all rows positive; `gt` keeps the ground-truth tensors the pointers address alive"""

    def __init__(self, gt, N, P, depth_rows, roi, blob, offsets, n):
        self.blob, self.n = blob, n
        base = blob.data_ptr()
        self.ptr = {k: C.c_void_p(base + o) for k, o in offsets.items()}
        self.B, self.N, self.R, self.P, self.depth_rows, self.roi = gt.B, N, gt.B * N, P, depth_rows, roi
        self.has_depth = gt.depth_base is not None
        self.gt = gt


def _desc_rows(head, gt, cfg, num_proposals, roi):
    """(N, pos_weight) of a head's or stage's descriptor: the stuff rows follow the proposals where the roi head has stuff targets"""
    N = num_proposals + head.num_stuff_classes if (roi and gt.has_sem) else num_proposals
    return N, 1.0 if cfg.pos_weight <= 0 else float(cfg.pos_weight)


def build_desc(head, gt, assigns, num_proposals, cfg, roi):
    """roi=True : KernelUpdateHead._get_target_single (kernel_update_head.py:443-531) for B images: N = num_proposals + stuff rows
    roi=False: KernelHead._get_target_single (kernel_head.py:571-647): N = num_proposals rows, dense semantic target, the depth
    items of an image all on its ONE direct depth map.  The tables are packed on the host and uploaded once."""
    B, HW = gt.B, gt.HW
    L, ns, nt = head.num_classes, head.num_stuff_classes, head.num_thing_classes
    Np = num_proposals
    N, pw = _desc_rows(head, gt, cfg, Np, roi)
    R = B * N
    HW4 = 4 * HW
    tptr, wptr = np.zeros(R, np.int64), np.zeros(R, np.int64)
    labels = np.full(R, L, np.int64)
    pos_u8 = np.zeros(R, np.uint8)
    label_w = np.zeros((R, L), np.float32) if roi else None
    d_row, d_t, d_w, d_s = [], [], [], []
    s_cnt, s_m, s_l = [0], [], []
    for b in range(B):
        r0 = b * N
        pi, gi = assigns[b]
        rows = r0 + pi
        wptr[r0:r0 + Np] = gt.valid_base[b]
        tptr[rows] = gt.mask_base[b] + gi * HW4
        labels[rows] = gt.labels_h[b][gi]
        pos_u8[rows] = 1
        if roi:
            label_w[r0:r0 + Np, :(nt if gt.has_sem else L)] = 1.0
            label_w[rows, :(nt if gt.has_sem else L)] = pw
        sc = gt.sem_cls_h[b]
        srow = None
        if roi and gt.has_sem:
            label_w[r0 + Np + np.arange(ns), nt + np.arange(ns)] = 1.0
            if len(sc):
                srow = r0 + Np + (sc - nt)
                tptr[srow] = gt.sem_base[b] + np.arange(len(sc), dtype=np.int64) * HW4
                wptr[srow] = gt.valid_base[b]
                labels[srow] = sc
                pos_u8[srow] = 1
        if gt.depth_base is not None:
            dp = int(gt.depth_base[b])
            if roi:
                last = r0 + N - 1
                for r, w in zip(rows.tolist(), (gt.mask_base[b] + gi * HW4).tolist()):
                    if r != last:
                        d_row.append(r); d_t.append(dp); d_w.append(w); d_s.append(pw)
                if srow is not None:
                    for k, r in enumerate(srow.tolist()):
                        if r != last:
                            d_row.append(r); d_t.append(dp); d_w.append(int(gt.sem_base[b]) + k * HW4); d_s.append(pw)
                d_row.append(last); d_t.append(dp); d_w.append(1); d_s.append(1.0)          # the direct depth row (:525-528)
            else:
                for w in (gt.mask_base[b] + gi * HW4).tolist():
                    d_row.append(b); d_t.append(dp); d_w.append(w); d_s.append(pw)
                if gt.has_sem:
                    for k in range(len(sc)):
                        d_row.append(b); d_t.append(dp); d_w.append(int(gt.sem_base[b]) + k * HW4); d_s.append(pw)
        if not roi:         # dense semantic target: the stuff masks in order, then the assigned thing masks in order (:590-605)
            if gt.has_sem:
                for k in range(len(sc)):
                    s_m.append(int(gt.sem_base[b]) + k * HW4); s_l.append(int(sc[k]))
            for w, l in zip((gt.mask_base[b] + gi * HW4).tolist(), gt.labels_h[b][gi].tolist()):
                s_m.append(w); s_l.append(int(l))
            s_cnt.append(len(s_m))
    depth_rows = R if roi else B
    d_row = np.asarray(d_row, np.int64)
    order = np.argsort(d_row, kind="stable")
    dstart = np.zeros(depth_rows + 1, np.int32)
    if len(d_row):
        np.add.at(dstart, d_row + 1, 1)
    dstart = np.cumsum(dstart).astype(np.int32)
    pos_rows = np.nonzero(pos_u8)[0].astype(np.int32)
    sec = dict(tptr=tptr, wptr=wptr, labels=labels, pos_u8=pos_u8, pos_rows=pos_rows if len(pos_rows) else np.zeros(1, np.int32), dstart=dstart,
               dit_t=np.asarray(d_t, np.int64)[order] if len(d_row) else np.zeros(1, np.int64),
               dit_w=np.asarray(d_w, np.int64)[order] if len(d_row) else np.zeros(1, np.int64),
               dit_s=np.asarray(d_s, np.float32)[order] if len(d_row) else np.zeros(1, np.float32))
    if roi:
        sec["label_w"] = label_w.reshape(-1)
    else:
        sec.update(sstart=np.asarray(s_cnt, np.int32), sit_m=np.asarray(s_m if s_m else [0], np.int64), sit_l=np.asarray(s_l if s_l else [0], np.int32))
    off, total = {}, 0
    for k, a in sec.items():
        off[k] = total
        total += (a.nbytes + 15) // 16 * 16
    buf = np.zeros(max(total, 16), dtype=np.uint8)
    for k, a in sec.items():
        buf[off[k]:off[k] + a.nbytes] = a.view(np.uint8).reshape(-1)
    blob = torch.from_numpy(buf).to(gt.valid.device, non_blocking=True)
    return LossDesc(gt, N, int(len(pos_rows)), depth_rows, roi, blob, off, {k: a.size for k, a in sec.items()})


class DeviceDesc(LossDesc):
    """a `LossDesc` whose tables `ph_assign_desc` writes: the counts are the host's (they follow from the ground-truth counts), the
    contents never leave the device.  What a later stage needs to use the assignment again (`prev=`) stays with it: `match` int32
    [B, ldg] (prediction row per ground-truth column, -1 unmatched), `status` int64 [B], the kernel's cfg, counts and table."""

    def __init__(self, gt, N, roi, cfg, counts, lay, match, status, ldg):
        B, L = gt.B, cfg.L
        R, P, nd, nsit, depth_rows = B * N, int(lay.P), int(lay.depth_items), int(lay.seg_items), int(lay.depth_rows)
        n = dict(tptr=R, wptr=R, labels=R, pos_u8=R, pos_rows=max(P, 1), dstart=depth_rows + 1, dit_t=max(nd, 1), dit_w=max(nd, 1), dit_s=max(nd, 1))
        n.update(dict(label_w=R * L) if roi else dict(sstart=B + 1, sit_m=max(nsit, 1), sit_l=max(nsit, 1)))
        blob = torch.empty((lay.total_bytes,), dtype=torch.uint8, device=gt.valid.device)
        super().__init__(gt, N, P, depth_rows, roi, blob, {k: getattr(lay, k) for k in n}, n)
        self.cfg, self.counts, self.table = cfg, counts, gt.device_table()
        self.match, self.status, self.ldg = match, status, ldg

    def launch(self, cost):
        """`ph_assign_desc` into this descriptor's blob: solve `cost` [B, Np, ldg] (None: keep `match`), write the tables.
        Launches only.  -> the call's return code"""
        ip = lambda a: a.ctypes.data_as(C.c_void_p)
        G, S, last = self.counts
        return _lib.load().ph_assign_desc(C.byref(self.cfg), ip(G), ip(S), ip(last), _lib.ptr(cost), self.ldg, _lib.ptr(self.table),
                                          self.table.numel(), _lib.ptr(self.match), _lib.ptr(self.status), _lib.ptr(self.blob),
                                          self.blob.numel(), _lib.stream_ptr())


def _assign_counts(gt, head, roi):
    """host arrays of `ph_assign_desc` (G, S, last_pos) or None where the ground truth is outside the kernel's contract: stuff
    classes of an image must be distinct, and for the roi form lie in n_thing .. n_thing + n_stuff - 1"""
    key = ("_counts", bool(roi), head.num_thing_classes, head.num_stuff_classes)
    c = gt.__dict__.get(key, False)
    if c is False:
        nt, ns = head.num_thing_classes, head.num_stuff_classes
        ok = True
        last = np.zeros(gt.B, np.int32)
        for b, sc in enumerate(gt.sem_cls_h):
            if len(np.unique(sc)) != len(sc) or (roi and len(sc) and (sc.min() < nt or sc.max() >= nt + ns)):
                ok = False
            last[b] = int(roi and gt.has_sem and ns > 0 and (nt + ns - 1) in sc)
        c = (np.asarray(gt.G, np.int32), np.asarray([len(sc) for sc in gt.sem_cls_h], np.int32), last) if ok else None
        gt.__dict__[key] = c
    return c


def assign_desc_device(head, gt, assigner, pred, cls_pred, num_proposals, cfg, roi, prev=None):
    """`assign_batch` + `build_desc` without the host: the cost tensor stays where `_assign_cost` forms it, `ph_assign_desc` solves
    it per image as scipy would and writes the descriptor blob (csrc/ph_assign.hip).  Launches only.  `prev`: a DeviceDesc whose
    assignment is used again (a stage beyond `assign_stages`).  Returns a DeviceDesc, or None where the kernels' limits do not
    hold (more than 256 proposals or instances, more than 64 images, ...): the caller takes the host path."""
    lib = _lib.load()
    B, HW = gt.B, gt.HW
    L, ns, nt = head.num_classes, head.num_stuff_classes, head.num_thing_classes
    Np = num_proposals
    N, pw = _desc_rows(head, gt, cfg, Np, roi)
    has_depth = gt.depth_base is not None
    counts = _assign_counts(gt, head, roi)
    if (counts is None or B > _lib.PH_ASSIGN_MAX_B or max(Np, gt.Gmax, ns) > _lib.PH_ASSIGN_MAX or (roi and has_depth and N == Np)
            or pred.shape[1] != Np):
        return None
    G, S, last = counts
    dev = gt.valid.device
    c = _lib.AssignCfg(B=B, Np=Np, N=N, L=L, n_thing=nt, n_stuff=ns, roi=int(roi), has_sem=int(gt.has_sem), has_depth=int(has_depth),
                       pos_weight=pw, HW=HW)
    lay = _lib.AssignLayout()
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.ph_assign_desc_layout(C.byref(c), ip(G), ip(S), ip(last), C.byref(lay)), "ph_assign_desc_layout")
    cost = None
    if prev is not None:
        match, status, ldg = prev.match, prev.status, prev.ldg
    else:
        ldg = gt.Gmax
        if ldg:
            cost = _assign_cost(assigner, pred, cls_pred, gt)
            if not torch.is_tensor(cost):               # every cost weight is zero: nothing to solve on either path
                return None
            cost = cost.detach().float().contiguous()
            assert cost.shape == (B, Np, ldg)
        match = torch.empty((B, max(ldg, 1)), dtype=torch.int32, device=dev)
        status = torch.empty((B,), dtype=torch.int64, device=dev)
    d = DeviceDesc(gt, N, roi, c, counts, lay, match, status, ldg)
    rc = d.launch(cost)
    if rc == _lib.PH_EUNSUPPORTED:
        return None
    _lib.check(rc, "ph_assign_desc")
    if prev is None:
        gt.status_words.append(status)
    return d


_LOSS_SCRATCH = {}


def fused_losses(head, desc, mask_pred, cls_score, depth_pred, seg_pred, with_grads=True):
    """`ph_train_losses` for one head / stage: -> (dict of weighted losses as the reference names them, grads or None).
    mask_pred [B, N, H, W]; cls_score [B, N, L] (roi) / None; depth_pred [B, N, H, W] (roi) / [B, 1, H, W] (KernelHead's direct
    map) / None; seg_pred [B, L, H, W] (KernelHead) / None"""
    lib, dev = _lib.load(), mask_pred.device
    B, N, H, W = mask_pred.shape
    assert (B, N) == (desc.B, desc.N)
    HW, L = H * W, head.num_classes
    roi = desc.roi
    mp = _f32(mask_pred)
    cs = _f32(cls_score).reshape(B * N, L) if cls_score is not None else None
    have_depth = depth_pred is not None and desc.has_depth
    dp = _f32(depth_pred) if have_depth else mp                 # a valid pointer either way; without items nothing is read
    sp = _f32(seg_pred) if seg_pred is not None else None
    c = LossCfg()
    c.B, c.N, c.L, c.P, c.depth_rows, c.HW = B, N, L, desc.P, desc.depth_rows, HW
    c.seg_L = sp.shape[1] if sp is not None else 0
    lr = head.loss_rank
    c.has_rank, c.ignore = int(lr is not None), int(head.ignore_label)
    c.lw_mask, c.lw_dice, c.dice_eps = head.loss_mask.loss_weight, head.loss_dice.loss_weight, head.loss_dice.eps
    c.lw_rank = lr.loss_weight if lr is not None else 0.0
    ld = head.loss_depth
    if have_depth:
        c.depth_mode = DEPTH_MODES[ld.depth_act_mode]
        c.lw_depth = ld.loss_weight
        c.dw_si, c.dw_sq, c.dw_abs = [float(v) for v in ld.weight]
    if cs is not None:
        lc = head.loss_cls
        from .dist import reduce_mean
        import torch.distributed as tdist
        npos = float(desc.P)
        if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size(_REDUCE_GROUP[-1]) > 1:
            # gloo groups (the CPU tests) reduce host tensors, RCCL groups device tensors
            on = dev if tdist.get_backend(_REDUCE_GROUP[-1]) == "nccl" else "cpu"
            npos = float(reduce_mean(torch.tensor(npos, device=on), _REDUCE_GROUP[-1]))
        c.lw_cls, c.cls_gamma, c.cls_alpha, c.cls_avg = lc.loss_weight, lc.gamma, lc.alpha, max(npos, 1.0)
    else:
        c.cls_avg = 1.0
    if sp is not None:
        ls = head.loss_seg
        if not ls.use_sigmoid:
            raise NotImplementedError("libpolyhead: loss_seg is the shipped sigmoid FocalLoss (polyphonic_former.py:73-78)")
        c.lw_seg, c.seg_gamma, c.seg_alpha = ls.loss_weight, ls.gamma, ls.alpha
    nb = lib.ph_train_losses_scratch_bytes(C.byref(c))
    scratch = _LOSS_SCRATCH.get(dev)
    if scratch is None or scratch.numel() < nb:
        scratch = _LOSS_SCRATCH[dev] = torch.empty((nb,), dtype=torch.uint8, device=dev)
    out = torch.empty((8,), dtype=torch.float32, device=dev)
    g = None
    if with_grads:
        g = dict(mask_pred=torch.empty_like(mp), depth_pred=torch.empty_like(dp) if have_depth else None,
                 cls_score=torch.empty_like(cs) if cs is not None else None, seg_preds=torch.empty_like(sp) if sp is not None else None)
    P = desc.ptr
    gd = g["depth_pred"] if (g and have_depth) else (torch.empty_like(dp) if g else None)      # no depth items: dstart is all zero
    _lib.check(lib.ph_train_losses(C.byref(c), _lib.ptr(mp), _lib.ptr(cs), _lib.ptr(dp), _lib.ptr(sp), P["pos_rows"], P["pos_u8"], P["tptr"],
                                   P["wptr"], P["dstart"], P["dit_t"], P["dit_w"], P["dit_s"], P["labels"] if cs is not None else None,
                                   P.get("label_w") if cs is not None else None, P.get("sstart") if sp is not None else None,
                                   P.get("sit_m") if sp is not None else None, P.get("sit_l") if sp is not None else None, _lib.ptr(out),
                                   _lib.ptr(g["mask_pred"]) if g else None, _lib.ptr(g["cls_score"]) if (g and cs is not None) else None,
                                   _lib.ptr(gd), _lib.ptr(g["seg_preds"]) if (g and sp is not None) else None, _lib.ptr(scratch),
                                   scratch.numel(), _lib.stream_ptr()), "ph_train_losses")
    losses = {}
    if have_depth:
        losses["loss_depth"] = out[0]
    if roi:
        losses["loss_cls"], losses["pos_acc"] = out[1], out[6]
        keys = ("loss_rpn_mask", "loss_rpn_dice", "loss_rank") if desc.P else ("loss_mask", "loss_dice", "loss_rank")
    else:
        keys = ("loss_rpn_mask", "loss_rpn_dice", "loss_rpn_rank") if desc.P else ("loss_rpn_mask", "loss_rpn_dice", "loss_rank")
    losses[keys[0]], losses[keys[1]] = out[2], out[3]
    if lr is not None:
        losses[keys[2]] = out[4]
    if sp is not None:
        losses["loss_rpn_seg"] = out[5]
    if g is not None:
        g = dict(mask_pred=g["mask_pred"].reshape(B, N, H, W), cls_score=None if cs is None else g["cls_score"].reshape(B, N, L),
                 depth_pred=None if not have_depth else g["depth_pred"], seg_preds=g["seg_preds"])
    return losses, g
