"""CPU: polyphonicformer_amd/fpn.py -- the constructor contract against the reference's own config and key list, the training branch
(torch ops on the module's parameters) against the reference's statements with float64 autograd, and the integer nearest-index rule
ph_fpn_lateral relies on."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
from polyphonicformer_amd.registry import NECKS, wrap_fp16_model
import polyphonicformer_amd.fpn as FP


def _cfg():
    return json.load(open(os.path.join(Hh.GOLDEN, "fpn_cfg.json")))


def test_builds_from_the_reference_config_with_its_keys():
    m = NECKS.build(_cfg())
    assert isinstance(m, FP.FPN) and m.precision == "fp32"
    keys = json.loads(bytes(Hh.load_golden("fpn.npz")["keys_json"]).decode())
    sd = m.state_dict()
    assert list(sd) == list(keys) and len(keys) == 16
    assert {k: list(v.shape) for k, v in sd.items()} == keys
    assert wrap_fp16_model(torch.nn.Sequential(m)) == [m] and m.precision == "fp16"


@pytest.mark.parametrize("arg,value", [
    ("in_channels", [256, 512, 1024]), ("in_channels", [256, 512, 1024, 2048, 2048]), ("in_channels", [256, 512, 1024, 2000]),
    ("out_channels", 128), ("start_level", 1), ("num_outs", 5), ("end_level", 3), ("norm_cfg", dict(type="BN")),
    ("act_cfg", dict(type="ReLU")), ("conv_cfg", dict(type="ConvWS")), ("upsample_cfg", dict(mode="bilinear")),
    ("upsample_cfg", dict(mode="nearest", scale_factor=2)), ("add_extra_convs", "on_nothing")])
def test_unsupported_arguments_are_named(arg, value):
    cfg = dict(_cfg(), **{arg: value})
    with pytest.raises(NotImplementedError, match=arg):
        NECKS.build(cfg)


def test_training_branch_is_the_reference_statements_with_gradients():
    with torch.enable_grad():          # whatever grad mode an earlier test of the session left behind
        _training_branch()


def _training_branch():
    torch.manual_seed(0)
    m = NECKS.build(_cfg()).double().train()
    sd = {k: v.double() for k, v in Hh.seeded_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, 5).items()}
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(3)
    sizes = ((9, 11), (5, 6), (3, 3), (2, 2))
    feats = [torch.randn(2, c, h, w, generator=g, dtype=torch.float64).relu() for c, (h, w) in zip(m.in_channels, sizes)]
    outs = m(feats)
    assert isinstance(outs, tuple) and len(outs) == 4 and all(o.requires_grad for o in outs)
    # fpn.py:151-203 restated on leaf copies of the same values
    w = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    lat = [F.conv2d(feats[i], w[f"lateral_convs.{i}.conv.weight"], w[f"lateral_convs.{i}.conv.bias"]) for i in range(4)]
    for i in range(3, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    ref = [F.conv2d(lat[i], w[f"fpn_convs.{i}.conv.weight"], w[f"fpn_convs.{i}.conv.bias"], padding=1) for i in range(4)]
    cots = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in ref]
    for a, b in zip(outs, ref):
        assert a.shape == b.shape and Hh.rel_err(a.detach(), b.detach()) < 1e-12
    names = list(w)
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(names) and len(names) == 16
    got = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), [params[n] for n in names])
    want = torch.autograd.grad(sum((o * c).sum() for o, c in zip(ref, cots)), [w[n] for n in names])
    for n, a, b in zip(names, got, want):
        assert float(b.abs().max()) > 0 and Hh.rel_err(a, b) < 1e-12, n
    # without grad the module has no CPU path: the library is the only inference path
    with torch.no_grad(), pytest.raises(Exception, match="GPU"):
        m(feats)


def test_integer_nearest_index_is_torchs_on_a_stride2_pyramid():
    """the claim of include/polyhead.h (ph_fpn_lateral): for H in {2 Hc, 2 Hc - 1} the source row of F.interpolate(mode='nearest',
    size=H) is y * Hc // H"""
    for Hc in range(1, 601):
        src = torch.arange(Hc, dtype=torch.float32).reshape(1, 1, Hc, 1)
        for H in (2 * Hc, 2 * Hc - 1):
            got = F.interpolate(src, size=(H, 1), mode="nearest").reshape(-1).long()
            y = torch.arange(H)
            assert torch.equal(got, torch.clamp(y * Hc // H, max=Hc - 1)), (Hc, H)
