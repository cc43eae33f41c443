"""The training step's assignment on the device against the host path, on one GPU, at cfg2's training shape (bench.train_leg:
2 images, 100 proposals, 20 instances and half of the stuff classes per image, 256 x 512 at the assign stride).

  * `ph_assign_desc` alone -- the solve and the descriptor tables of one head or stage, cost tensor given -- for KernelHead's and
    the update head's form: HIP events around the one call, median of warm runs.
  * `TrainStep.forward_backward` with and without `device_assign`, alternating in one process: wall time around the step
    INCLUDING the final device synchronisation, median.

Prints one JSON line and writes it to --out.

    python tools/assign_time.py --out profiles/device_assign/assign_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from polyphonicformer_amd import losses as Lo, train as T  # noqa: E402
from polyphonicformer_amd.registry import HEADS  # noqa: E402
import polyphonicformer_amd.kernel_head, polyphonicformer_amd.kernel_update  # noqa: F401,E401,E402
import polyphonicformer_amd.kernel_update_head, polyphonicformer_amd.kernel_updator  # noqa: F401,E401,E402


def build(wl, dev, B):
    """the heads and the batch of bench.train_leg"""
    L, nt, ns, H, W = wl["n_thing"] + wl["n_stuff"], wl["n_thing"], wl["n_stuff"], wl["H"], wl["W"]
    cost = dict(cls_cost=dict(type='FocalLossCost', weight=2.0), dice_cost=dict(type='DiceCost', weight=4.0, pred_act=True),
                mask_cost=dict(type='MaskCost', weight=1.0, pred_act=True))
    tc = lambda extra: dict(assigner=dict(type='MaskHungarianAssignerWithDepth', **cost, **extra), sampler=dict(type='MaskPseudoSampler'),
                            pos_weight=1.)
    torch.manual_seed(2)
    losses = dict(loss_rank=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.1), loss_dice=dict(type="DiceLoss", loss_weight=4.0),
                  loss_depth=dict(type="DepthLoss", loss_weight=5.0, depth_act_mode="sigmoid"))
    rpn = HEADS.build(dict(type="KernelHead", num_proposals=wl["Nq"], num_classes=L, num_thing_classes=nt, num_stuff_classes=ns,
                           cat_stuff_mask=True, feat_downsample_stride=2, feat_refine=False, use_binary=True, proposal_feats_with_obj=True,
                           loss_seg=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                           loss_mask=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), train_cfg=tc({}), **losses))
    scfg = bench.stage_cfg(L, nt, ns, wl["F"])
    scfg.update(loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0), **losses)
    depth_cost = dict(depth_cost=dict(type='DepthCost', weight=0., loss_fn=dict(type='DepthMatchLoss', loss_weight=1.), depth_act_mode='sigmoid'))
    roi = HEADS.build(dict(type="KernelUpdateIterHead", num_stages=wl["S"], assign_stages=wl["S"], stage_loss_weights=[1] * wl["S"],
                           num_proposals=wl["Nq"], num_thing_classes=nt, num_stuff_classes=ns, mask_head=scfg, train_cfg=tc(depth_cost)))
    rpn.init_weights()
    roi.init_weights()
    rpn.to(dev)
    roi.to(dev)
    g = torch.Generator().manual_seed(11)
    feats = [torch.randn(B, 256, H, W, generator=g).relu().to(dev) for _ in range(3)]
    H2, W2 = 2 * H, 2 * W
    gts = []
    for b in range(B):
        G = 20
        cy, cx = torch.rand(G, generator=g) * H2, torch.rand(G, generator=g) * W2
        r = 8 + torch.rand(G, generator=g) * 40
        yy, xx = torch.arange(H2)[None, :, None], torch.arange(W2)[None, None, :]
        masks = (((yy - cy[:, None, None]) ** 2 + (xx - cx[:, None, None]) ** 2) < r[:, None, None] ** 2).float()
        present = torch.randperm(ns, generator=g)[: ns // 2].sort()[0]
        sem = (torch.rand(len(present), H2 // 16, W2 // 16, generator=g) > 0.6).float()
        sem = torch.nn.functional.interpolate(sem[None], size=(H2, W2), mode="nearest")[0]
        depth = torch.rand(H2, W2, generator=g) * 79.0 + 0.5
        gts.append(dict(masks=masks.to(dev), labels=torch.randint(0, nt, (G,), generator=g).to(dev), sem_seg=sem.to(dev),
                        sem_cls=(present + nt).to(dev), depth=depth.to(dev)))
    metas = [dict(img_shape=(H * 8, W * 8, 3), ori_shape=(H * 8, W * 8, 3), batch_input_shape=(H * 8, W * 8))] * B
    gd = torch.stack([x["depth"][None] for x in gts])
    return rpn, roi, (feats, metas, [x["masks"] for x in gts], [x["labels"] for x in gts], [x["sem_seg"] for x in gts],
                      [x["sem_cls"] for x in gts], gd)


def call_alone(head, assigner, cfg, gt, pred, cls, Np, roi, reps):
    """HIP-event time of `ph_assign_desc` on a fixed cost tensor, us: median, min, max of `reps` warm calls"""
    cost = Lo._assign_cost(assigner, pred, cls, gt).detach().float().contiguous()
    d = Lo.assign_desc_device(head, gt, assigner, pred, cls, Np, cfg, roi)
    assert d is not None, "the shape is outside the device path's limits"
    ts = []
    for it in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        rc = d.launch(cost)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0
        if it >= 5:
            ts.append(e0.elapsed_time(e1) * 1e3)
    assert int(d.status.abs().sum()) == 0
    return dict(us=round(statistics.median(ts), 2), us_min_max=[round(min(ts), 2), round(max(ts), 2)], blob_bytes=d.blob.numel(), positives=d.P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    wl, B = bench.WORKLOADS["cfg2"], 2
    rpn, roi, args = build(wl, dev, B)
    Np, nt = wl["Nq"], wl["n_thing"]
    res = dict(command="python tools/assign_time.py", workload="cfg2 training shape", images=B, proposals=Np, instances_per_image=20,
               assign_map=[2 * wl["H"], 2 * wl["W"]], reps=a.reps)
    with torch.no_grad():
        gt = Lo.StepGT(args[2], args[3], args[4], args[5], args[6], True)
        g = torch.Generator().manual_seed(3)
        pred = (torch.randn(B, Np, 2 * wl["H"], 2 * wl["W"], generator=g) * 2).to(dev)
        cls = torch.randn(B, Np, nt, generator=g).to(dev)
        res["ph_assign_desc_kernel_head"] = call_alone(rpn, rpn.assigner, rpn.train_cfg, gt, pred, None, Np, False, a.reps)
        res["ph_assign_desc_update_head"] = call_alone(roi.mask_head[0], roi.mask_assigner[0], roi.train_cfg[0], gt, pred, cls, Np, True, a.reps)
    step = T.TrainStep(rpn, roi)
    t = {False: [], True: []}
    for it in range(a.reps + 3):
        for on in (False, True):                          # alternating
            step.device_assign = on
            for p in step.parameters():
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, total, _ = step.forward_backward(*args)
            torch.cuda.synchronize()
            if it >= 3:
                t[on].append((time.perf_counter() - t0) * 1e3)
            res["objective_device" if on else "objective_host"] = float(total)
    status = step.assign_status()                         # of the last step, a device one
    res["solves_per_step"], res["status_all_zero"] = list(status.shape), bool((status == 0).all())
    for on, name in ((False, "step_host_assign_ms"), (True, "step_device_assign_ms")):
        res[name] = round(statistics.median(t[on]), 3)
        res[name + "_min_max"] = [round(min(t[on]), 3), round(max(t[on]), 3)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
