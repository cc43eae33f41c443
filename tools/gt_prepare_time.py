"""Building a video training step's ground truth on one GPU at cfg3's size: 2 key + 2 reference frames of 1024 x 2048, assign stride 4
(masks 256 x 512), 40 things + 11 stuff segments per frame, starting from what a loader hands over on the host.

  (i)  the ground-truth step alone, A and B alternating in one process, median host wall time INCLUDING the final synchronisation:
       A  the reference's operations in torch (polyphonic_former_video.py:114-138 and :159-183, restated in `torch_lists`: the fp32
          stack from host uint8 bitmasks, the upload, F.pad where the sizes differ, F.interpolate, the four splits, the nearest depth) followed
          by `losses.StepGT(lists, hard)` for both values of `hard` on the key frames and the soft one on the reference frames;
       B  `gt.prepare_gt(..., want_hard=True)` on the host index maps of the same frames followed by `step_gt` for both values.
       `index_map_from_bitmasks` (a loader worker's job, host numpy) is timed apart.
  (ii) the whole step from loader outputs both ways: A's lines + `VideoTrainStep.forward_backward`, B's call +
       `VideoTrainStep.forward_backward_prepared`, with and without device_assign.

Prints one JSON line and writes it to --out.

    python tools/gt_prepare_time.py --out profiles/gt_prepare/time.json
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "tools"))
import helpers  # noqa: E402
from video_train_time import COST, NP, NS, NT, summary, wall_ms  # noqa: E402
from polyphonicformer_amd import gt as GT, losses as Lo, train as T  # noqa: E402
from polyphonicformer_amd.registry import HEADS, NECKS  # noqa: E402

H0, W0 = 256, 512                 # FPN level 0 = the assign resolution (stride 4 of 1024 x 2048)
PAD = (4 * H0, 4 * W0)
STRIDE = 4


def loader_frame(rng, things, stuff):
    """one frame as a loader leaves it: disjoint uint8 bitmasks [things + stuff][1024][2048] that tile the image (stuff bands with
    discs of things painted over them), labels in loader order, instance ids (from a pool of twice the
    segment count, so that key and reference frames share some), the depth map"""
    H, W = PAD
    n = things + stuff
    order = rng.permutation(n)                                      # segment index of the i-th painted region
    lmap = np.empty(PAD, np.uint8)
    edges = np.linspace(0, W, stuff + 1).astype(int)
    for j in range(stuff):
        lmap[:, edges[j]:edges[j + 1]] = order[j]
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    for j in range(things):
        cy, cx, r = rng.random() * H, rng.random() * W, 30 + rng.random() * 160
        lmap[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = order[stuff + j]
    labels = np.empty(n, np.int64)
    labels[order[:stuff]] = NT + rng.permutation(NS)[:stuff]
    labels[order[stuff:]] = rng.integers(0, NT, things)
    masks = np.stack([lmap == i for i in range(n)]).astype(np.uint8)
    depth = (rng.random((1,) + PAD, dtype=np.float32) * 79.0 + 0.5).astype(np.float32)
    return dict(bitmasks=masks, labels=labels, ids=(rng.permutation(2 * n)[:n] + 1).astype(np.int64), depth=depth)


def torch_lists(frames, dev, nearest=False):
    """the torch way from host bitmasks to the lists a step takes, in the operations the reference uses
    (polyphonic_former_video.py:114-138) and in this project's words: per frame the whole [G][H][W] stack goes to fp32 on the host and
    over to the device (what `BitmapMasks.to_tensor(float32, device)` does), is zero-padded to PAD where it is smaller, resized to the
    assign resolution and split by label with boolean indexing; the depth maps are resized by nearest"""
    size = (PAD[0] // STRIDE, PAD[1] // STRIDE)
    resize = dict(mode="nearest") if nearest else dict(mode="bilinear", align_corners=False)
    things, thing_labels, stuff, stuff_labels, ids = [], [], [], [], []
    for f in frames:
        labels = torch.from_numpy(f["labels"]).to(dev)
        stack = torch.tensor(f["bitmasks"], dtype=torch.float32, device=dev)
        grow = (0, PAD[1] - stack.shape[2], 0, PAD[0] - stack.shape[1])
        if any(grow):
            stack = F.pad(stack, grow)
        low = F.interpolate(stack[None], size, **resize)[0]
        is_thing = labels < NT
        things.append(low[is_thing]); thing_labels.append(labels[is_thing])
        stuff.append(low[~is_thing]); stuff_labels.append(labels[~is_thing])
        ids.append(torch.from_numpy(f["ids"]).to(dev)[is_thing])
    depth = F.interpolate(torch.from_numpy(np.stack([f["depth"] for f in frames])).to(dev), size, mode="nearest")
    return things, thing_labels, stuff, stuff_labels, depth, ids


def prepared(frames, maps, dev):
    return GT.prepare_gt(maps, [f["labels"] for f in frames], PAD, NT, mask_assign_stride=STRIDE, gt_depth=np.stack([f["depth"] for f in frames]),
                         gt_instance_ids=[f["ids"] for f in frames], want_hard=True, device=dev)


def build_models(dev):
    tc = lambda kind: dict(assigner=dict(type=kind, **copy.deepcopy(COST)), sampler=dict(type='MaskPseudoSampler'), pos_weight=1.)
    torch.manual_seed(2)
    rpn = HEADS.build(dict(type="KernelHead", num_proposals=NP, num_classes=NT + NS, num_thing_classes=NT, num_stuff_classes=NS,
                           cat_stuff_mask=True, feat_downsample_stride=2, feat_refine=False, use_binary=True, proposal_feats_with_obj=True,
                           loss_rank=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.1),
                           loss_seg=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                           loss_mask=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_dice=dict(type="DiceLoss", loss_weight=4.0),
                           loss_depth=dict(type="DepthLoss", loss_weight=5.0, depth_act_mode="sigmoid"),
                           train_cfg=tc('MaskHungarianAssignerWithDepth')))
    roi = HEADS.build(dict(type="KernelUpdateIterHead", num_stages=3, assign_stages=3, stage_loss_weights=[1] * 3, num_proposals=NP,
                           num_thing_classes=NT, num_stuff_classes=NS, mask_head=helpers.stage_cfg(256, 2048, 8, NT + NS, NT, NS),
                           train_cfg=tc('MaskHungarianAssignerWithDepth')))
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
    return neck, rpn, roi, th, tc('MaskHungarianAssigner')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--things", type=int, default=40)
    ap.add_argument("--stuff", type=int, default=11)
    ap.add_argument("--no-step", action="store_true", help="measure (i) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_prepare_time.py measures on a GPU; none is visible")
    import polyphonicformer_amd.kernel_head, polyphonicformer_amd.kernel_update, polyphonicformer_amd.semantic_fpn  # noqa: F401,E401
    import polyphonicformer_amd.kernel_update_head, polyphonicformer_amd.kernel_updator, polyphonicformer_amd.track_head  # noqa: F401,E401
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    B = 2
    key = [loader_frame(rng, args.things, args.stuff) for _ in range(B)]
    ref = [loader_frame(rng, args.things, args.stuff) for _ in range(B)]
    res = {"command": "python tools/gt_prepare_time.py",
           "workload": f"{B} key + {B} reference frames of {PAD[0]} x {PAD[1]}, assign stride {STRIDE}, {args.things} things + {args.stuff} stuff segments each",
           "reps": args.reps, "upload_bytes_reference": int(sum(f["bitmasks"].size * 4 + f["depth"].nbytes for f in key + ref)),
           "upload_bytes_index_maps": int(sum(f["bitmasks"][0].size + f["depth"].nbytes for f in key + ref))}
    t0 = time.perf_counter()
    kmaps, rmaps = [GT.index_map_from_bitmasks(f["bitmasks"]) for f in key], [GT.index_map_from_bitmasks(f["bitmasks"]) for f in ref]
    res["index_map_from_bitmasks_host_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / (2 * B), 1)

    def gt_a():
        kl, rl = torch_lists(key, dev), torch_lists(ref, dev)
        return kl, rl, [Lo.StepGT(*kl[:5], h) for h in (False, True)], Lo.StepGT(rl[0], rl[1], None, None, None, False)

    def gt_b():
        kp, rp = prepared(key, kmaps, dev), prepared(ref, rmaps, dev)
        return kp, rp, [kp.step_gt(h) for h in (False, True)], rp.step_gt(False, with_stuff=False)

    a, b = gt_a(), gt_b()
    same = all(torch.equal(x, y) for x, y in zip(a[0][0] + a[0][2] + a[1][0], b[0].gt_masks + b[0].gt_sem_seg + b[1].gt_masks))
    same = same and torch.equal(a[0][4], b[0].gt_depth) and all(torch.equal(a[2][i].pad, b[2][i].pad) and torch.equal(a[2][i].valid, b[2][i].valid)
                                                                for i in range(2))
    res["prepared_equals_reference_lists"] = bool(same)
    del a, b
    t_a, t_b = [], []
    for _ in range(args.reps):
        t_a += wall_ms(gt_a, 1)
        t_b += wall_ms(gt_b, 1)
    res["gt_reference_lines_plus_StepGT"], res["gt_prepare_gt_plus_step_gt"] = summary(t_a), summary(t_b)
    res["gt_ratio"] = round(res["gt_reference_lines_plus_StepGT"]["ms"] / res["gt_prepare_gt_plus_step_gt"]["ms"], 1)

    if not args.no_step:
        neck, rpn, roi, th, track_cfg = build_models(dev)
        x = [f.to(dev) for f in helpers.fpn_inputs(21, B, 256, H0, W0)]
        x_ref = [f.to(dev) for f in helpers.fpn_inputs(22, B, 256, H0, W0)]
        metas = [dict(img_shape=PAD + (3,), ori_shape=PAD + (3,), batch_input_shape=PAD)] * B
        for device_assign in (False, True):
            with T.VideoTrainStep(neck, rpn, roi, th, track_cfg, device_assign=device_assign) as step:
                def clear():
                    for p in step.parameters():
                        p.grad = None

                def step_a():
                    clear()
                    kl, rl = torch_lists(key, dev), torch_lists(ref, dev)
                    return step.forward_backward(x, x_ref, metas, *kl, rl[0], rl[1], rl[5], PAD)

                def step_b():
                    clear()
                    return step.forward_backward_prepared(x, x_ref, metas, prepared(key, kmaps, dev), prepared(ref, rmaps, dev), PAD)

                ra, rb = step_a(), step_b()
                step_a(); step_b()
                t_a, t_b = [], []
                for _ in range(args.reps):
                    t_a += wall_ms(step_a, 1)
                    t_b += wall_ms(step_b, 1)
            tag = "device_assign" if device_assign else "host_assign"
            res[f"video_step_from_bitmasks_{tag}"], res[f"video_step_from_index_maps_{tag}"] = summary(t_a), summary(t_b)
            res[f"same_objective_{tag}"] = bool(torch.equal(ra[1], rb[1]))
            res[f"objective_{tag}"] = round(float(rb[1]), 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
