"""The FPN's direct hand-over to the neck at the flagship size (1024 x 2048 image: levels 256x512 .. 32x64, fp32 NCHW stages of
256 / 512 / 1024 / 2048 channels), B = 1 and B = 4, 'bf16' and 'fp16' grades; tools/fpn_time.py's method: one process,
alternating, HIP events around the calls, median and min .. max of --reps after warm-up:

  * `neck(fpn(stages))` -- the two-step path: every level written as fp32 NCHW (ph_fpn_output) and read back (ph_nhwc_ingest) --
    against `neck.forward_from_fpn(fpn, stages)` (ph_fpn_output_planes writes the neck's conv input planes) with and without the
    fp32 levels beside the planes,
  * the tail alone per level: ph_fpn_output + ph_nhwc_ingest against ph_fpn_output_planes (with and without the fp32 level), with
    the bytes each must move.

Prints one JSON line and writes it to --out.

    python tools/fpn_handoff_time.py --out profiles/fpn/handoff_time.json
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
from fpn_time import CHANNELS, SHAPES, alternate  # noqa: E402
from polyphonicformer_amd import _lib, engine as E  # noqa: E402
from polyphonicformer_amd.fpn import FPN  # noqa: E402
from polyphonicformer_amd.semantic_fpn import SemanticFPNWrapper  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fpn_handoff_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    res = {"command": "python tools/fpn_handoff_time.py", "workload": "FPN + SemanticFPNWrapper of a 1024 x 2048 image: fp32 NCHW stages "
           "256x512x256 .. 32x64x2048 -> the neck's three fp32 maps; HIP events around the calls, alternating in one process",
           "reps": args.reps, "warmup": args.warmup}

    def flush():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    mods = {}
    for grade in ("bf16", "fp16"):
        fpn = FPN(list(CHANNELS), 256, 4)
        fpn.load_state_dict(helpers.seeded_fill({k: tuple(v.shape) for k, v in fpn.state_dict().items()}, 5))
        neck = SemanticFPNWrapper(256, 256, 256, 0, 3, positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                                  upsample_times=2, num_aux_convs=2, norm_cfg=dict(type="GN", num_groups=32, requires_grad=True))
        neck.load_state_dict(helpers.seeded_fill({k: tuple(v.shape) for k, v in neck.state_dict().items()}, 6))
        for m in (fpn, neck):
            m.eval().to(dev)
            m.set_precision(grade)
        mods[grade] = (fpn, neck)
    for B in (1, 4):
        g = torch.Generator().manual_seed(3)
        stages = [torch.randn(B, c, h, w, generator=g).relu().to(dev) for c, (h, w) in zip(CHANNELS, SHAPES)]
        runs = {}
        for grade, (fpn, neck) in mods.items():
            a = [o.clone() for o in neck(list(fpn(stages)))]
            b = neck.forward_from_fpn(fpn, stages)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), "the two paths differ"
            runs[f"{grade}_two_step"] = lambda fpn=fpn, neck=neck: neck(list(fpn(stages)))
            runs[f"{grade}_direct"] = lambda fpn=fpn, neck=neck: neck.forward_from_fpn(fpn, stages)
            runs[f"{grade}_direct_with_levels"] = lambda fpn=fpn, neck=neck: neck.forward_from_fpn(fpn, stages, want_levels=True)
        print(f"B={B}: timing", list(runs), flush=True)
        res[f"B{B}"] = alternate(runs, args.reps, args.warmup)
        print(json.dumps(res[f"B{B}"]), flush=True)
        flush()
        # the tail alone, per level: the conv result is there; what follows it on either path
        tails = {}
        for grade in mods:
            prec = E.KHEAD_PREC[grade]
            for lvl, (h, w) in enumerate(SHAPES):
                HW = h * w
                y, bias = torch.randn(B, HW, 256, device=dev), torch.randn(256, device=dev)
                add = torch.randn(256, HW, device=dev) if lvl == 3 else None
                level = torch.empty(B, 256, 1, HW, device=dev)
                planes = torch.empty(1, B, HW, 256, dtype=torch.int16, device=dev)
                layout = prec | (_lib.PH_PLANES_C16 if lvl == 0 else 0)      # the neck's own layouts: chunk-major into level 0

                def two(y=y, bias=bias, add=add, level=level, planes=planes, HW=HW, layout=layout):
                    E.fpn_output(y, bias, level, B, HW)
                    E.nhwc_ingest(level, add, layout, planes)
                t = alternate({"two_step": two,
                               "direct": lambda y=y, bias=bias, add=add, planes=planes, HW=HW, layout=layout:
                               E.fpn_output_planes(y, bias, add, planes, None, B, HW, layout),
                               "direct_with_level": lambda y=y, bias=bias, add=add, level=level, planes=planes, HW=HW, layout=layout:
                               E.fpn_output_planes(y, bias, add, planes, level, B, HW, layout)}, args.reps, args.warmup)
                n = B * HW * 256
                tails[f"{grade}_level{lvl}"] = dict(t, bytes_two_step=n * (4 + 4 + 4 + 2), bytes_direct=n * (4 + 2), bytes_direct_with_level=n * (4 + 4 + 2))
                del y, level, planes
        res[f"B{B}_tail"] = tails
        print(json.dumps(tails), flush=True)
        flush()
        del stages
    print(flush())


if __name__ == "__main__":
    main()
