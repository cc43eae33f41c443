"""The video training step on one GPU at cfg3's size: a 1024 x 2048 padded image, assign stride 4 (masks 256 x 512), FPN levels 256 x 512 ...
32 x 64, 2 images x 40 things per frame.

  (i)   `track_head.gt_mask_rois` (4 frames x 40 masks, selection included) against a torch restatement of
        polyphonic_former_video.py:283-305 + 413-415 (F.interpolate, sigmoid > 0.5, per mask nonzero, two means, two mean absolute
        deviations, four .item() calls, bboxlist2roi, clamp) on the same GPU, same process, alternating; median host wall time
        INCLUDING the final synchronisation;
  (ii)  `VideoTrainStep.forward_backward` with and without device_assign;
  (iii) the pieces by hand as they were before the step existed: neck_forward_train + TrainStep's two heads + the reference frame +
        `track_forward_train` with the torch boxes and the host assignment, one backward.

Prints one JSON line and writes it to --out.

    python tools/video_train_time.py --out profiles/video_train/time.json
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import helpers  # noqa: E402
from polyphonicformer_amd import losses as Lo, track_head as TH, train as T  # noqa: E402
from polyphonicformer_amd.registry import HEADS, NECKS  # noqa: E402
import polyphonicformer_amd.kernel_head, polyphonicformer_amd.kernel_update, polyphonicformer_amd.semantic_fpn  # noqa: F401,E401,E402
import polyphonicformer_amd.kernel_update_head, polyphonicformer_amd.kernel_updator, polyphonicformer_amd.track_head  # noqa: F401,E401,E402

NT, NS, NP = 8, 11, 100
H0, W0 = 256, 512                 # FPN level 0 = the assign resolution (stride 4 of 1024 x 2048)
PAD = (4 * H0, 4 * W0)
COST = dict(cls_cost=dict(type='FocalLossCost', weight=2.0), dice_cost=dict(type='DiceCost', weight=4.0, pred_act=True),
            mask_cost=dict(type='MaskCost', weight=1.0, pred_act=True))


def torch_boxes(masks_low, pos_gt, pad):
    """:283-291 + batch_mask2boxlist + bboxlist2roi + clamp for one frame, as the reference runs it"""
    m = F.interpolate(masks_low[pos_gt.long()].unsqueeze(0), size=pad, mode="bilinear", align_corners=False).squeeze(0)
    m = (m.sigmoid() > 0.5).float()
    boxes = []
    for mask in m:
        c = mask.nonzero().float()
        if c.numel() > 0:
            center = torch.mean(c, dim=0)
            dy = max(torch.mean((c[:, 0] - center[0]).abs(), dim=0), 1)
            dx = max(torch.mean((c[:, 1] - center[1]).abs(), dim=0), 1)
            box = torch.Tensor([(center[1] - dx * 2).item(), (center[0] - dy * 2).item(), (center[1] + dx * 2).item(), (center[0] + dy * 2).item()])
        else:
            box = torch.Tensor([0, 0, 0, 0])
        boxes.append(box.to(m.device).unsqueeze(0))
    b = torch.cat(boxes, 0)
    return torch.cat([b.new_zeros((b.shape[0], 1)), b], dim=-1).clamp(min=0.0)


def blobs(G, g):
    cy, cx = torch.rand(G, generator=g) * PAD[0], torch.rand(G, generator=g) * PAD[1]
    r = 30 + torch.rand(G, generator=g) * 160
    yy, xx = torch.arange(PAD[0])[None, :, None], torch.arange(PAD[1])[None, None, :]
    full = (((yy - cy[:, None, None]) ** 2 + (xx - cx[:, None, None]) ** 2) < r[:, None, None] ** 2).float()
    return F.interpolate(full[None], size=(H0, W0), mode="bilinear", align_corners=False)[0].contiguous()


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    return {"ms": round(statistics.median(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--things", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_train_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    B, G = 2, args.things
    tc = lambda kind, extra: dict(assigner=dict(type=kind, **copy.deepcopy(COST), **extra), sampler=dict(type='MaskPseudoSampler'), pos_weight=1.)
    torch.manual_seed(2)
    rpn = HEADS.build(dict(type="KernelHead", num_proposals=NP, num_classes=NT + NS, num_thing_classes=NT, num_stuff_classes=NS,
                           cat_stuff_mask=True, feat_downsample_stride=2, feat_refine=False, use_binary=True, proposal_feats_with_obj=True,
                           loss_rank=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.1),
                           loss_seg=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                           loss_mask=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_dice=dict(type="DiceLoss", loss_weight=4.0),
                           loss_depth=dict(type="DepthLoss", loss_weight=5.0, depth_act_mode="sigmoid"),
                           train_cfg=tc('MaskHungarianAssignerWithDepth', {})))
    roi = HEADS.build(dict(type="KernelUpdateIterHead", num_stages=3, assign_stages=3, stage_loss_weights=[1] * 3, num_proposals=NP,
                           num_thing_classes=NT, num_stuff_classes=NS, mask_head=helpers.stage_cfg(256, 2048, 8, NT + NS, NT, NS),
                           train_cfg=tc('MaskHungarianAssignerWithDepth', {})))
    neck = NECKS.build(dict(type="SemanticFPNWrapper", in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
                            upsample_times=2, positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                            cat_coors=False, cat_coors_level=3, fuse_by_cat=False, return_list=False, num_aux_convs=2,
                            norm_cfg=dict(type="GN", num_groups=32, requires_grad=True)))
    th = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32),
                          loss_track=dict(type="MultiPosCrossEntropyLoss", loss_weight=0.25),
                          loss_track_aux=dict(type="L2Loss", neg_pos_ub=3, pos_margin=0, neg_margin=0.1, hard_mining=True, loss_weight=1.0)))
    for m in (rpn, roi, neck, th):
        m.init_weights()
        m.to(dev).train()
    track_cfg = tc('MaskHungarianAssigner', {})
    x = [f.to(dev) for f in helpers.fpn_inputs(21, B, 256, H0, W0)]
    x_ref = [f.to(dev) for f in helpers.fpn_inputs(22, B, 256, H0, W0)]

    def frame_gt():
        out = []
        for _ in range(B):
            present = torch.randperm(NS, generator=g)[: NS // 2].sort()[0]
            sem = F.interpolate((torch.rand(1, len(present), H0 // 16, W0 // 16, generator=g) > 0.6).float(), size=(H0, W0), mode="nearest")[0]
            out.append(dict(masks=blobs(G, g).to(dev), labels=torch.randint(0, NT, (G,), generator=g).to(dev), sem_seg=sem.to(dev),
                            sem_cls=(present + NT).to(dev), depth=(torch.rand(H0, W0, generator=g) * 79.0 + 0.5).to(dev)))
        return out

    key, ref = frame_gt(), frame_gt()
    ids = [torch.arange(G).to(dev) + 100 * b for b in range(B)]
    rids = [torch.where(torch.arange(G) % 3 == 0, torch.arange(G) + 100 * b, torch.arange(G) + 5000).flip(0).to(dev) for b in range(B)]
    metas = [dict(img_shape=PAD + (3,), ori_shape=PAD + (3,), batch_input_shape=PAD)] * B
    gd = torch.stack([t["depth"][None] for t in key])
    img = (metas, [t["masks"] for t in key], [t["labels"] for t in key], [t["sem_seg"] for t in key], [t["sem_cls"] for t in key], gd)
    vid = (ids, [t["masks"] for t in ref], [t["labels"] for t in ref], rids, PAD)
    res = {"command": "python tools/video_train_time.py", "workload": f"1024 x 2048 padded, assign stride 4, {B} images x {G} things per frame",
           "reps": args.reps}

    # (i) the box step alone: 4 frames x G masks, an arbitrary one-to-one assignment
    masks = [t["masks"] for t in key + ref]
    match = [torch.randperm(NP, generator=g)[:G].to(torch.int32).to(dev) for _ in masks]
    pos = [torch.argsort(m_).to(torch.int32) for m_ in match]
    n = [G] * len(masks)
    ours = lambda: TH.gt_mask_rois(masks, match, n, PAD, num_proposals=NP)
    theirs = lambda: [torch_boxes(m_, p_, PAD) for m_, p_ in zip(masks, pos)]
    a, b = ours(), theirs()
    res["box_max_abs_diff"] = round(max(float((u - v).abs().max()) for u, v in zip(a[0], b)), 6)
    assert all(torch.equal(u, v) for u, v in zip(a[1], pos))
    t_ours, t_torch = [], []
    for _ in range(args.reps):
        t_ours += wall_ms(ours, 1)
        t_torch += wall_ms(theirs, 1)
    res["gt_mask_rois"], res["torch_boxes"] = summary(t_ours), summary(t_torch)

    # (ii) the step
    def run_step(device_assign):
        with T.VideoTrainStep(neck, rpn, roi, th, track_cfg, device_assign=device_assign) as step:
            def one():
                for p in step.parameters():
                    p.grad = None
                return step.forward_backward(x, x_ref, *img, *vid)
            one(); one()
            ms = wall_ms(one, args.reps)
            losses, total, _ = one()
        return ms, losses, total

    ms, losses, total = run_step(False)
    res["video_step_host_assign"] = summary(ms)
    res["losses"] = {k: round(float(v), 5) for k, v in losses.items() if "track" in k}
    res["objective"] = round(float(total), 4)
    ms, _, total_d = run_step(True)
    res["video_step_device_assign"] = summary(ms)
    res["device_assign_same_objective"] = bool(torch.equal(total, total_d))

    # (iii) the pieces by hand, as a user of the previous version had to write them
    helper = T.VideoTrainStep(neck, rpn, roi, th, track_cfg)
    helper.close()
    params = helper.parameters()

    def by_hand():
        for p in params:
            p.grad = None
        xl = [f.detach().requires_grad_(True) for f in x]
        with torch.enable_grad():
            feats = T.neck_forward_train(neck, xl)
            l24, last, cache = T._heads_forward_train(rpn, roi, feats, *img, False)
            ref_last = helper._reference_frame(x_ref, metas)
            gt, rgt = T._step_gt(cache, False, *img[1:]), Lo.StepGT(vid[1], vid[2], None, None, None, False)
            mk = T.track_sample(helper.track_assigner, last[3], last[1], gt, NP, NT)
            mr = T.track_sample(helper.track_assigner, ref_last[3], ref_last[1], rgt, NP, NT)
            order = lambda m_, Gi: torch.argsort(torch.where(m_[:Gi] >= 0, m_[:Gi], torch.full_like(m_[:Gi], 1 << 20)))[:min(Gi, NP)]
            kp = [order(mk[i], gt.G[i]) for i in range(B)]
            rp = [order(mr[i], rgt.G[i]) for i in range(B)]
            rois = [torch_boxes(gt.masks[i], kp[i], PAD) for i in range(B)]
            rrois = [torch_boxes(rgt.masks[i], rp[i], PAD) for i in range(B)]
            gmi = [T.gt_match_indices(ids[i], rids[i]) for i in range(B)]
            l24.update(T.track_forward_train(th, [[lv[i:i + 1] for lv in xl] for i in range(B)], [[lv[i:i + 1] for lv in x_ref] for i in range(B)],
                                             rois, rrois, kp, rp, gmi))
            T.parse_losses(l24).backward()

    by_hand(); by_hand()
    res["pieces_by_hand_torch_boxes"] = summary(wall_ms(by_hand, args.reps))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
