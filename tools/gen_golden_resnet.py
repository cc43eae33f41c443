#!/usr/bin/env python
"""Golden for the backbone (polyphonicformer_amd/resnet.py), produced by the reference's own classes on the CPU.

Loads mmdet/models/utils/res_layer.py and mmdet/models/backbones/resnet.py from the reference tree on top of oracle.ref_loader's
stand-ins, plus the ones that only the backbone needs and that live here: `mmcv.cnn.build_conv_layer` (cfg None -> nn.Conv2d),
`mmcv.cnn.build_plugin_layer` (never reached: the config has no plugins), `mmcv.runner.Sequential` (nn.Sequential with an ignored
init_cfg) and torch's own `_BatchNorm`.  Builds the class from the `model.backbone` dict of the reference's resolved image config,
fills it by tests/resnet_cases.py and runs it on resnet_cases.inputs at 1 x 3 x 40 x 72 in fp32 and in float64.

Writes
    tests/golden/resnet_cfg.json   the backbone dict: settings only
    tests/golden/resnet.npz        out0..out3 (fp32), keys_json (state_dict key -> shape), f32_err, emu_err_{bf16,fp16}

f32_err: the fp32 run against the float64 run (helpers.rel_err, maximum over stages).
emu_err_*: this tool's float64 emulation of the device's rounding points -- the image as it is staged, the folded weights, every
layer output (the stem's after the pool), the residual read back as 16 bits and added before the rounding; b' kept in fp32 -- against
the reference's fp32 output, maximum over stages.

The tool asserts what keeps the golden from being dominated by biases or by a saturated value: every stage's float64 output stays
below 100, 50-90 % of each stage's entries are nonzero, and the generator's second input moves every stage by >= 0.1 max-normalised.

usage: PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_resnet.py     (needs the reference tree)"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import helpers  # noqa: E402
import resnet_cases  # noqa: E402
from oracle import gen_ref_cfg, ref_loader  # noqa: E402


def load_reference_resnet():
    ref_loader.load_reference()
    cnn, runner = sys.modules["mmcv.cnn"], sys.modules["mmcv.runner"]

    def build_conv_layer(cfg, *args, **kwargs):
        assert cfg is None or dict(cfg).get("type") in (None, "Conv2d", "Conv"), cfg
        return nn.Conv2d(*args, **kwargs)

    def build_plugin_layer(cfg, postfix="", **kwargs):
        raise NotImplementedError("plugins are not part of the shipped backbone")

    class Sequential(nn.Sequential):
        def __init__(self, *args, init_cfg=None):
            super().__init__(*args)

    cnn.build_conv_layer, cnn.build_plugin_layer, runner.Sequential = build_conv_layer, build_plugin_layer, Sequential

    def load(modname, relpath):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(ref_loader.REF_ROOT, relpath))
        m = importlib.util.module_from_spec(spec)
        sys.modules[modname] = m
        spec.loader.exec_module(m)
        return m

    utils = sys.modules.get("mmdet.models.utils") or ref_loader._mod("mmdet.models.utils")
    utils.ResLayer = load("mmdet.models.utils.res_layer", "mmdet/models/utils/res_layer.py").ResLayer
    if "mmdet.models.backbones" not in sys.modules:
        ref_loader._mod("mmdet.models.backbones")
    return load("mmdet.models.backbones.resnet", "mmdet/models/backbones/resnet.py").ResNet


def backbone_cfg():
    return gen_ref_cfg.jsonable(gen_ref_cfg.load_cfg(os.path.join(gen_ref_cfg.REF, "configs/polyphonic_image/poly_r50_cityscapes_2x.py"))
                                ["model"]["backbone"])


def rnd(t, grade):
    """float64 -> the grade's value, as float64"""
    return (t.float().half() if grade == "fp16" else t.float().bfloat16()).double()


def emulate(sd, x, grade, eps=1e-5):
    """the device path in float64 with its rounding points, from the reference's state_dict (depth read from the keys)"""
    def folded(conv, bn):
        s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + eps)
        return rnd(sd[conv + ".weight"].double() * s[:, None, None, None], grade), \
            (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).float().double()

    w, b = folded("conv1", "bn1")
    y = rnd(F.max_pool2d(F.conv2d(rnd(x.double(), grade), w, b, stride=2, padding=3).relu(), 3, 2, 1), grade)
    outs = []
    for i in range(1, 5):
        j = 0
        while f"layer{i}.{j}.conv1.weight" in sd:
            p = f"layer{i}.{j}."
            stride = 2 if (i > 1 and j == 0) else 1
            w, b = folded(p + "conv1", p + "bn1")
            t = rnd(F.conv2d(y, w, b).relu(), grade)
            w, b = folded(p + "conv2", p + "bn2")
            t = rnd(F.conv2d(t, w, b, stride=stride, padding=1).relu(), grade)
            idn = y
            if p + "downsample.0.weight" in sd:
                w, b = folded(p + "downsample.0", p + "downsample.1")
                idn = rnd(F.conv2d(y, w, b, stride=stride), grade)
            w, b = folded(p + "conv3", p + "bn3")
            y = rnd((F.conv2d(t, w, b) + idn).relu(), grade)
            j += 1
        outs.append(y)
    return outs


def run():
    ResNet = load_reference_resnet()
    cfg = backbone_cfg()
    m = ResNet(**{k: v for k, v in cfg.items() if k != "type"})
    sd = resnet_cases.fill(m.state_dict())
    m.load_state_dict(sd)
    m.eval()
    x, x2 = resnet_cases.inputs(2)
    with torch.no_grad():
        outs = m(x.clone())
        m.double()
        outs64, outs64b = m(x.double()), m(x2.double())
        m.float()
        for i, (o, o2) in enumerate(zip(outs64, outs64b)):
            peak, nz = float(o.abs().max()), float((o != 0).double().mean())
            moved = float((o - o2).abs().max() / o.abs().max())
            print(f"stage {i}: shape {tuple(o.shape)}  max |v| {peak:.2f}  nonzero {nz:.3f}  second input moves it by {moved:.3f}")
            assert peak < 100, (i, peak)
            assert 0.5 <= nz <= 0.9, (i, nz)
            assert moved >= 0.1, (i, moved)
        f32_err = max(helpers.rel_err(o, o64) for o, o64 in zip(outs, outs64))
        err = {g: max(helpers.rel_err(e, o) for e, o in zip(emulate(sd, x, g), outs)) for g in ("bf16", "fp16")}
    return cfg, m, outs, f32_err, err


def main():
    cfg, m, outs, f32_err, err = run()
    gold = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(gold, "resnet_cfg.json"), "w") as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write("\n")
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    np.savez_compressed(os.path.join(gold, "resnet.npz"), keys_json=np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8),
                        f32_err=np.float64(f32_err), **{f"out{i}": o.numpy() for i, o in enumerate(outs)},
                        **{f"emu_err_{g}": np.float64(e) for g, e in err.items()})
    print("resnet.npz", os.path.getsize(os.path.join(gold, "resnet.npz")), "bytes;", len(keys), "keys; f32_err", f32_err,
          "; emulation errors", err)


if __name__ == "__main__":
    main()
