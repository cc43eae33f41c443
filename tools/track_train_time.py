"""Training the track head on one GPU: forward + backward of `train.track_forward_train` at cfg3's level sizes (a 1024 x 2048 image:
FPN levels 256 x 512 ... 32 x 64), 2 images x (40 key, 40 reference) RoIs, all 16 parameter gradients and the key frames' level
gradients.

  * the whole call + `backward()`: a host clock around the work INCLUDING the final device synchronisation, median of warm runs;
  * `ph_track_loss` alone (2 pairs of 40 x 40, and one pair of 100 x 100) and `ph_roi_align_fpn_bwd` alone (40 RoIs): HIP events
    around the one call, median of warm runs.

Prints one JSON line and writes it to --out; `readme_row` in it is the row for README.md's table.

    python tools/track_train_time.py --out profiles/track_train/time.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from polyphonicformer_amd import _lib, train as T  # noqa: E402
from polyphonicformer_amd.registry import HEADS  # noqa: E402
import polyphonicformer_amd.track_head  # noqa: F401,E402

LEVELS = [(256, 512), (128, 256), (64, 128), (32, 64)]
STRIDES = (4, 8, 16, 32)
IMAGE_STEP_MS = 13.0            # README: one image training step (2 images, TrainStep(device_assign=True))


def boxes(n, g, Hi=1024, Wi=2048):
    """n RoIs (0, x1, y1, x2, y2) with sides from 24 to 900 pixels: all four FPN levels are used"""
    side = torch.exp(torch.rand(n, 2, generator=g) * (torch.log(torch.tensor(900.0)) - torch.log(torch.tensor(24.0))) + torch.log(torch.tensor(24.0)))
    cx, cy = torch.rand(n, generator=g) * Wi, torch.rand(n, generator=g) * Hi
    b = torch.stack([torch.zeros(n), cx - side[:, 0] / 2, cy - side[:, 1] / 2, cx + side[:, 0] / 2, cy + side[:, 1] / 2], 1)
    return b.clamp(min=0)


def events_us(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return {"us": round(statistics.median(out), 2), "us_min_max": [round(min(out), 2), round(max(out), 2)]}


def loss_alone(dev, pairs, n, g, reps):
    lib = _lib.load()
    cfg = _lib.TrackLossCfg(pairs=pairs, E=256, lw_track=0.25, lw_aux=1.0, neg_pos_ub=3, pos_margin=0.0, neg_margin=0.1, hard_mining=1)
    shared = torch.randn(1, 256, generator=g)
    key = (0.65 * shared + torch.randn(pairs * n, 256, generator=g)).to(dev)
    ref = (0.65 * shared + torch.randn(pairs * n, 256, generator=g)).to(dev)
    gt = torch.arange(n, dtype=torch.int32).repeat(pairs).to(dev)
    match = torch.where(torch.arange(n) % 3 == 0, torch.arange(n), torch.full((n,), -1)).to(torch.int32).repeat(pairs).to(dev)
    st = (C.c_int32 * (pairs + 1))(*[p * n for p in range(pairs + 1)])
    losses, gk, gr = torch.empty(2, device=dev), torch.empty_like(key), torch.empty_like(ref)
    scratch = torch.empty((lib.ph_track_loss_scratch_bytes(C.byref(cfg), pairs * n, pairs * n),), dtype=torch.uint8, device=dev)
    call = lambda: _lib.check(lib.ph_track_loss(C.byref(cfg), _lib.ptr(key), _lib.ptr(ref), st, st, _lib.ptr(gt), _lib.ptr(gt), st, _lib.ptr(match),
                                                _lib.ptr(losses), _lib.ptr(gk), _lib.ptr(gr), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr()),
                              "ph_track_loss")
    r = events_us(call, reps)
    r["losses"] = [round(float(v), 6) for v in losses.cpu()]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rois", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_train_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    head = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32),
                            loss_track=dict(type="MultiPosCrossEntropyLoss", loss_weight=0.25),
                            loss_track_aux=dict(type="L2Loss", neg_pos_ub=3, pos_margin=0, neg_margin=0.1, hard_mining=True, loss_weight=1.0)))
    torch.manual_seed(3)
    head.init_weights()
    head.to(dev).train()
    B, n = 2, args.rois
    mk = lambda grad: [[torch.randn(1, 256, h, w, generator=g).to(dev).requires_grad_(grad) for h, w in LEVELS] for _ in range(B)]
    feats, ref_feats = mk(True), mk(False)
    rois, ref_rois = [boxes(n, g).to(dev) for _ in range(B)], [boxes(n, g).to(dev) for _ in range(B)]
    gt = [list(range(n)) for _ in range(B)]
    match = [[i if i % 3 == 0 else -1 for i in range(n)] for _ in range(B)]

    def step():
        for p in head.parameters():
            p.grad = None
        for lv in feats:
            for f in lv:
                f.grad = None
        losses = T.track_forward_train(head, feats, ref_feats, rois, ref_rois, gt, gt, match, strides=STRIDES)
        T.parse_losses(losses).backward()
        return losses

    for _ in range(5):
        losses = step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    res = {"command": "python tools/track_train_time.py", "workload": "cfg3 level sizes (1024 x 2048 image), forward + backward of track_forward_train",
           "images": B, "key_rois": n, "ref_rois": n, "levels": LEVELS, "reps": args.reps,
           "step_ms": round(statistics.median(ms), 3), "step_ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
           "losses": {k: round(float(v.detach()), 6) for k, v in losses.items()},
           "grads_finite": bool(all(torch.isfinite(p.grad).all() for p in head.parameters())),
           "image_training_step_ms": IMAGE_STEP_MS}
    res["ph_track_loss_2x40x40"] = loss_alone(dev, 2, n, g, args.reps)
    res["ph_track_loss_1x100x100"] = loss_alone(dev, 1, 100, g, args.reps)
    lib = _lib.load()
    g_roi = torch.randn(n, 256, 7, 7, generator=g).to(dev)
    outs = [torch.empty(1, 256, h, w, device=dev) for h, w in LEVELS]
    ptrs = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
    hw = (C.c_int32 * 8)(*[v for s in LEVELS for v in s])
    sc = (C.c_float * 4)(*[1.0 / s for s in STRIDES])
    res["ph_roi_align_fpn_bwd"] = events_us(lambda: _lib.check(lib.ph_roi_align_fpn_bwd(_lib.ptr(g_roi), hw, sc, 4, _lib.ptr(rois[0]), n, 56.0, ptrs,
                                                                                       _lib.stream_ptr()), "ph_roi_align_fpn_bwd"), args.reps)
    res["readme_row"] = (f"| the track head's training step ({B} images x ({n} key, {n} reference) RoIs, cfg3 levels: RoI features, the head, "
                         f"`ph_track_loss`, all gradients) | **{res['step_ms']:.1f} ms** beside the {IMAGE_STEP_MS} ms image step "
                         f"(`profiles/track_train/time.json`) |")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
