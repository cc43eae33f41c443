"""The FPN at the flagship size (1024 x 2048 image: levels 256x512 .. 32x64, 256 / 512 / 1024 / 2048 channels, fp32 NCHW stages),
B = 1 and B = 4, one process, alternating, HIP events around the calls, median and min .. max of --reps after warm-up:

  * `fpn.FPN.forward` in each grade ('bf16', 'fp16', 'fp32'),
  * the same arithmetic in torch on the same weights: fp32 NCHW `F.conv2d` / `F.interpolate`, and bf16 autocast on channels-last
    inputs and weights (the inputs converted before the timed window),
  * the lateral kernel alone per level and grade, with the bytes it must read (stage + coarse planes + weights) and write and the
    resulting TB/s.

Prints one JSON line and writes it to --out.

    python tools/fpn_time.py --out profiles/fpn/time.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import helpers  # noqa: E402
from polyphonicformer_amd import _lib, engine as E  # noqa: E402
from polyphonicformer_amd.fpn import FPN  # noqa: E402

CHANNELS = (256, 512, 1024, 2048)
SHAPES = ((256, 512), (128, 256), (64, 128), (32, 64))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def alternate(runs, reps, warmup):
    samples = {k: [] for k in runs}
    for rep in range(warmup + reps):
        for k, fn in runs.items():
            t = event_ms(fn)
            if rep >= warmup:
                samples[k].append(t)
    return {k: summary(v) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch forms")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fpn_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"command": "python tools/fpn_time.py", "workload": "FPN of a 1024 x 2048 image: fp32 NCHW stages 256x512x256 .. 32x64x2048 -> "
           "four fp32 NCHW 256-channel levels; HIP events around the calls, alternating in one process", "reps": args.reps,
           "warmup": args.warmup, "gflop_per_frame": round(sum(2 * 256 * (c + 9 * 256) * h * w for c, (h, w) in zip(CHANNELS, SHAPES)) / 1e9, 1)}

    def flush():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    mods = {}
    for grade in ("bf16", "fp16", "fp32"):
        m = FPN(list(CHANNELS), 256, 4)
        m.load_state_dict(helpers.seeded_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, 5))
        m.eval().to(dev)
        m.set_precision(grade)
        mods[grade] = m
    ref = mods["fp32"]
    ref_cl = FPN(list(CHANNELS), 256, 4)
    ref_cl.load_state_dict(ref.state_dict())
    ref_cl.eval().to(dev).to(memory_format=torch.channels_last)
    for B in (1, 4):
        g = torch.Generator().manual_seed(3)
        feats = [torch.randn(B, c, h, w, generator=g).relu().to(dev) for c, (h, w) in zip(CHANNELS, SHAPES)]
        runs = {f"ours_{grade}": (lambda m=m: m(feats)) for grade, m in mods.items()}
        if not args.no_torch:
            feats_cl = [f.contiguous(memory_format=torch.channels_last) for f in feats]

            def torch_fp32():
                with torch.no_grad():
                    ref._forward_torch(feats)

            def torch_bf16_cl():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    ref_cl._forward_torch(feats_cl)
            runs.update(torch_fp32_nchw=torch_fp32, torch_bf16_autocast_channels_last=torch_bf16_cl)
        print(f"B={B}: timing", list(runs), flush=True)
        res[f"B{B}"] = alternate(runs, args.reps, args.warmup)
        print(json.dumps(res[f"B{B}"]), flush=True)
        flush()
        # the lateral kernel alone: per level and grade, with the coarse planes where the level has one
        lat = {}
        for grade, m in mods.items():
            prec, pk = E.KHEAD_PREC[grade], m._pack(dev)
            P = 2 if prec == _lib.PH_PREC_SPLIT else 1
            planes = [torch.zeros((P, B, h * w, 256), dtype=torch.int16, device=dev) for h, w in SHAPES]
            runs = {}
            for lvl in range(4):
                c = pk["lateral"][lvl]
                runs[lvl] = (lambda lvl=lvl, c=c: E.fpn_lateral(feats[lvl], c["wp"], c["bias"], planes[lvl + 1] if lvl < 3 else None,
                                                                SHAPES[lvl + 1] if lvl < 3 else None, planes[lvl], prec))
            t = alternate(runs, args.reps, args.warmup)
            for lvl, (h, w) in enumerate(SHAPES):
                rd = B * CHANNELS[lvl] * h * w * 4 + P * 256 * CHANNELS[lvl] * 2 + (P * B * SHAPES[lvl + 1][0] * SHAPES[lvl + 1][1] * 512 if lvl < 3 else 0)
                wr = P * B * h * w * 512
                s = t[lvl]["ms"] * 1e-3
                lat[f"{grade}_level{lvl}"] = dict(t[lvl], bytes_read=rd, bytes_written=wr, tbps_read=round(rd / s / 1e12, 3),
                                                  tbps_read_and_written=round((rd + wr) / s / 1e12, 3),
                                                  tflops=round(2 * 256 * CHANNELS[lvl] * h * w * B * (3 if P == 2 else 1) / s / 1e12, 1))
        res[f"B{B}_lateral"] = lat
        print(json.dumps(lat), flush=True)
        flush()
        del feats
    print(flush())


if __name__ == "__main__":
    main()
