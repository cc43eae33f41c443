"""The optimizer step on the video model's real parameter set (neck, both heads, track head: what `VideoTrainStep.parameters()` lists):
`optim.AdamWStep.step()` against `clip_grad_norm_(..., foreach=True)` + `torch.optim.AdamW(fused=True).step()`, same process,
alternating, HIP events around the calls (so a side whose host work starves the GPU pays for it), median and min .. max after
warm-up.  Both with and without zeroing the gradients (`step(zero_grad=True)` against torch's `zero_grad(set_to_none=False)` behind
its step).  The host time of a call (launching only, no synchronisation inside) is recorded next to the event time.

Prints one JSON line and writes it to --out.

    python tools/optim_time.py --out profiles/optim/time.json
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import helpers  # noqa: E402
from polyphonicformer_amd import optim as O, train as T  # noqa: E402
from polyphonicformer_amd.registry import HEADS, NECKS  # noqa: E402
import polyphonicformer_amd.kernel_head, polyphonicformer_amd.kernel_update, polyphonicformer_amd.semantic_fpn  # noqa: F401,E401,E402
import polyphonicformer_amd.kernel_update_head, polyphonicformer_amd.kernel_updator, polyphonicformer_amd.track_head  # noqa: F401,E401,E402

NT, NS, NP = 8, 11, 100
COST = dict(cls_cost=dict(type='FocalLossCost', weight=2.0), dice_cost=dict(type='DiceCost', weight=4.0, pred_act=True),
            mask_cost=dict(type='MaskCost', weight=1.0, pred_act=True))
LR, WD, MAX_NORM = 2e-4, 0.05, 1.0            # schedule_1x.py / schedule_2x.py


def video_parameters(dev):
    """the video model's trained modules as tests/test_gpu_video_train.py builds them (only the shapes matter here)"""
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
    with T.VideoTrainStep(neck, rpn, roi, th, tc('MaskHungarianAssigner')) as step:
        return step.parameters()


def event_ms(fn):
    """(GPU milliseconds between events around fn(), host milliseconds fn() took to return)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def summary(samples):
    ev, host = [s[0] for s in samples], [s[1] for s in samples]
    return {"ms": round(statistics.median(ev), 4), "ms_min_max": [round(min(ev), 4), round(max(ev), 4)],
            "host_ms": round(statistics.median(host), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    ours_p = video_parameters(dev)
    torch_p = [torch.nn.Parameter(p.detach().clone()) for p in ours_p]
    gen = torch.Generator(device=dev).manual_seed(3)
    for p, q in zip(ours_p, torch_p):
        p.grad = 1e-2 * torch.randn(p.shape, device=dev, generator=gen)
        q.grad = p.grad.clone()
    refill = [p.grad.clone() for p in ours_p]
    ours = O.AdamWStep(ours_p, lr=LR, weight_decay=WD, max_norm=MAX_NORM)
    theirs = torch.optim.AdamW(torch_p, lr=LR, weight_decay=WD, fused=True)

    def torch_step(zero):
        torch.nn.utils.clip_grad_norm_(torch_p, MAX_NORM, foreach=True)
        theirs.step()
        if zero:
            theirs.zero_grad(set_to_none=False)

    def fill():                                                   # both sides start every repetition from the same gradients
        with torch.no_grad():
            torch._foreach_copy_([p.grad for p in ours_p], refill)
            torch._foreach_copy_([q.grad for q in torch_p], refill)

    runs = {"ours": lambda: ours.step(), "torch_clip_foreach_adamw_fused": lambda: torch_step(False),
            "ours_zero_grad": lambda: ours.step(zero_grad=True), "torch_clip_foreach_adamw_fused_zero_grad": lambda: torch_step(True)}
    samples = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():
            fill()
            s = event_ms(fn)
            if rep >= args.warmup:
                samples[k].append(s)
    info = ours.info()
    numel = sum(p.numel() for p in ours_p)
    res = {"command": "python tools/optim_time.py", "workload": f"the video model's {len(ours_p)} trained tensors, {numel} elements "
           f"({numel * 4 / 1e6:.1f} MB fp32), AdamW lr {LR} wd {WD}, max_norm {MAX_NORM}; HIP events around the calls, alternating",
           "tensors": len(ours_p), "elements": numel, "reps": args.reps, "warmup": args.warmup,
           "work_items": sum((p.numel() + O.CHUNK - 1) // O.CHUNK for p in ours_p)}
    res.update({k: summary(v) for k, v in samples.items()})
    res["ours_state"] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in info.items()}
    # how far the two sides drifted apart over all those steps (no yardstick here: tests/test_gpu_optim.py has torch in fp64)
    steps = 2 * (args.warmup + args.reps)
    with torch.no_grad():
        ulps = [float(((p - q).abs() / torch.ldexp(torch.ones_like(q), torch.frexp(q.abs().clamp_min(LR)).exponent - 24)).max())
                for p, q in zip(ours_p, torch_p)]
        res["steps_each"] = steps
        res["max_abs_param_diff_ours_vs_torch"] = max(float((p - q).abs().max()) for p, q in zip(ours_p, torch_p))
        res["max_abs_param"] = max(float(q.abs().max()) for q in torch_p)
        res["max_param_diff_in_ulp32_of_max_abs_param_and_lr"] = round(max(ulps), 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
