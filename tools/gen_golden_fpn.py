#!/usr/bin/env python
"""Golden for the FPN (polyphonicformer_amd/fpn.py), produced by the reference's own class on the CPU.

Loads mmdet/models/necks/fpn.py from the reference tree on top of oracle.ref_loader's stand-ins (plus `mmcv.runner.auto_fp16` as an
identity decorator and a package stub for `mmdet.models.necks`), builds the class from the `model.neck` dict of the reference's
resolved image config (resolved as oracle/gen_ref_cfg.py resolves it), fills it with helpers.seeded_fill(shapes, 5) and runs it on
relu(randn) inputs (generator seed 3) at level sizes (13, 19), (7, 10), (4, 5), (2, 3), B = 2, channels 256 / 512 / 1024 / 2048.

Writes
    tests/golden/fpn_cfg.json   the neck dict: settings only
    tests/golden/fpn.npz        out0..out3 (fp32), keys_json (state_dict key -> shape), emu_err_{bf16,fp16,fp32}

emu_err_*: this tool's torch emulation of the device arithmetic in float64 -- inputs, weights and the lateral sums rounded to the
grade (bf16, fp16, or bf16 hi + lo), everything else exact -- as helpers.rel_err against the reference output, maximum over levels.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fpn.py [--sizes 25,37]     (needs the reference tree)"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import helpers  # noqa: E402
from oracle import gen_ref_cfg, ref_loader  # noqa: E402

SIZES = ((13, 19), (7, 10), (4, 5), (2, 3))
B, WSEED, ISEED = 2, 5, 3


def load_reference_fpn():
    ref_loader.load_reference()
    sys.modules["mmcv.runner"].auto_fp16 = lambda *a, **k: (lambda f: f)
    if "mmdet.models.necks" not in sys.modules:
        ref_loader._mod("mmdet.models.necks")
    name = "mmdet.models.necks.fpn"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_loader.REF_ROOT, "mmdet/models/necks/fpn.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m.FPN


def neck_cfg():
    return gen_ref_cfg.jsonable(gen_ref_cfg.load_cfg(os.path.join(gen_ref_cfg.REF, "configs/polyphonic_image/poly_r50_cityscapes_2x.py"))
                                ["model"]["neck"])


def inputs(sizes, channels):
    g = torch.Generator().manual_seed(ISEED)
    return [torch.randn(B, c, h, w, generator=g).relu() for c, (h, w) in zip(channels, sizes)]


def rnd(t, grade):
    """float64 -> the grade's value, as float64"""
    f = t.float()
    if grade == "fp16":
        return f.half().double()
    hi = f.bfloat16().float()
    if grade == "bf16":
        return hi.double()
    return hi.double() + (f - hi).bfloat16().double()


def emulate(sd, feats, grade):
    w = lambda k: rnd(sd[k].double(), grade)
    lat = [None] * 4
    for i in (3, 2, 1, 0):
        s = F.conv2d(rnd(feats[i].double(), grade), w(f"lateral_convs.{i}.conv.weight"), sd[f"lateral_convs.{i}.conv.bias"].double())
        if i < 3:
            s = s + F.interpolate(lat[i + 1], size=s.shape[2:], mode="nearest")
        lat[i] = rnd(s, grade)
    return [F.conv2d(lat[i], w(f"fpn_convs.{i}.conv.weight"), sd[f"fpn_convs.{i}.conv.bias"].double(), padding=1) for i in range(4)]


def run(sizes):
    FPN = load_reference_fpn()
    cfg = neck_cfg()
    kw = {k: v for k, v in cfg.items() if k != "type"}
    m = FPN(**kw)
    sd = helpers.seeded_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, WSEED)
    m.load_state_dict(sd)
    m.eval()
    feats = inputs(sizes, cfg["in_channels"])
    with torch.no_grad():
        outs = m([f.clone() for f in feats])
        err = {g: max(helpers.rel_err(e, o) for e, o in zip(emulate(sd, feats, g), outs)) for g in ("bf16", "fp16", "fp32")}
    return cfg, m, outs, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=None, help="H,W of level 0 for an emulation-only run at another size (nothing is written)")
    a = ap.parse_args()
    if a.sizes:
        h, w = (int(v) for v in a.sizes.split(","))
        sizes = [(h, w)]
        for _ in range(3):
            sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
        print(sizes, run(sizes)[3])
        return
    cfg, m, outs, err = run(SIZES)
    gold = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(gold, "fpn_cfg.json"), "w") as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write("\n")
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    np.savez_compressed(os.path.join(gold, "fpn.npz"), keys_json=np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8),
                        **{f"out{i}": o.numpy() for i, o in enumerate(outs)},
                        **{f"emu_err_{g}": np.float64(e) for g, e in err.items()})
    print("fpn.npz", os.path.getsize(os.path.join(gold, "fpn.npz")), "bytes;", len(keys), "keys; emulation errors", err)


if __name__ == "__main__":
    main()
