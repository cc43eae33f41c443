"""CPU: the FPN's training path on the library's kernels as far as it can be checked without a GPU -- the split rule of the wide
map x map^T product, the argument checks of csrc/ph_fpntrain.hip that come before any launch, the gather rule of the nearest add's
backward against torch's autograd, and the `train_on_device` switch of fpn.FPN."""
import ctypes as C
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
from polyphonicformer_amd import _lib
from polyphonicformer_amd.registry import NECKS
import polyphonicformer_amd.fpn as FP

NEW = ("ph_map_x_map_t_wide_nsplit", "ph_map_x_map_t_wide", "ph_nearest_up_add", "ph_nearest_up_add_bwd", "ph_nchw_bias_add",
       "ph_nchw_channel_sums_nsplit", "ph_nchw_channel_sums")
BUDGET = 1024           # workgroups the split rule aims at (ph_map_x_map_t_nsplit's)
ROWS_PER_PASS = 160     # G rows of one row pass (ph_train.hip MXM_RT * 16)


def test_header_and_bindings_declare_the_entry_points():
    hdr = open(os.path.join(Hh.REPO, "include", "polyhead.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES, name
    from polyphonicformer_amd import train
    for fn in (train.fpn_forward_train, train.map_x_mapT_wide, train.nearest_up_add, train.nearest_up_add_bwd, train.nchw_bias_add,
               train.nchw_channel_sums, train._Lateral, train._NearestUpAdd, train._Conv3x3Bias):
        assert callable(fn)


def test_wide_nsplit_bounds():
    """at least 1, at least 256 pixels per split, the workgroup budget divided by images, row passes AND K tiles"""
    lib = _lib.load()
    for B in (1, 2, 8):
        for M in (1, 37, 160, 161, 256, 321):
            passes = -(-M // ROWS_PER_PASS)
            for K in (1, 40, 256, 257, 264, 512, 1024, 2048, 4096):
                ktiles = -(-K // 256)
                for HW in (1, 255, 256, 257, 3337, 4100, 131072, 1 << 21):
                    ns = lib.ph_map_x_map_t_wide_nsplit(B, M, K, HW)
                    assert ns == max(1, min(BUDGET // (B * passes * ktiles), HW // 256)), (B, M, K, HW, ns)
                    assert ns >= 1 and (ns == 1 or HW // ns >= 256)
                    assert ns * B * passes * ktiles <= max(BUDGET, B * passes * ktiles)
                    if K <= 256:            # never more splits than the K <= 256 product takes (its rule rounds HW / 256 up)
                        assert ns <= lib.ph_map_x_map_t_nsplit(B, M, HW)
    # the four levels of a 1024 x 2048 frame pair: what DESIGN.md 7f7 quotes
    assert [lib.ph_map_x_map_t_wide_nsplit(2, 256, 256 << l, (256 >> l) * (512 >> l)) for l in range(4)] == [256, 128, 32, 8]


def test_argument_checks_without_a_device():
    """every refusal comes before the first launch, so none of these calls touches a device: the pointers are never read"""
    lib = _lib.load()
    p = C.c_void_p(4096)

    def wide(G=p, X=p, part=p, out=p, B=2, M=256, K=512, HW=4096, ns=4, rsp=None, rs=None):
        return lib.ph_map_x_map_t_wide(G, X, part, out, B, M, K, HW, ns, rsp, rs, 1, None)

    for kw in (dict(K=0), dict(K=4097), dict(K=-3), dict(G=None), dict(X=None), dict(part=None), dict(out=None), dict(B=0), dict(M=0),
               dict(HW=0), dict(ns=0), dict(rsp=p), dict(rs=p)):
        assert wide(**kw) == _lib.PH_EINVAL, kw
        assert Hh.last_error().startswith("ph_map_x_map_t_wide"), Hh.last_error()
    assert wide(K=4097) == _lib.PH_EINVAL and "4096" in Hh.last_error()
    # the K <= 256 product keeps its own limit and its own name
    assert lib.ph_map_x_map_t_ex(p, p, p, p, 2, 256, 257, 4096, 4, 0, None, None, 1, None) == _lib.PH_EINVAL
    assert Hh.last_error().startswith("ph_map_x_map_t_ex") and "K <= 256" in Hh.last_error()

    for fn, tail in ((lib.ph_nearest_up_add, ()), (lib.ph_nearest_up_add_bwd, (1,))):
        def call(a=p, b=p, planes=512, H=9, W=11, Hc=5, Wc=6):
            return fn(a, b, planes, H, W, Hc, Wc, *tail, None)
        for kw in (dict(a=None), dict(b=None), dict(planes=0), dict(H=0), dict(W=0),
                   dict(Hc=4), dict(Hc=6), dict(Wc=5), dict(Wc=7), dict(Hc=0), dict(Wc=0), dict(H=11), dict(H=8), dict(W=13), dict(W=10),
                   dict(H=5, W=6, Hc=9, Wc=11)):
            assert call(**kw) == _lib.PH_EINVAL, kw
        assert call(Hc=6) == _lib.PH_EINVAL and "2 Hc" in Hh.last_error()
    assert lib.ph_nchw_bias_add(None, p, 2, 256, 64, None) == _lib.PH_EINVAL and lib.ph_nchw_bias_add(p, None, 2, 256, 64, None) == _lib.PH_EINVAL
    assert lib.ph_nchw_bias_add(p, p, 0, 256, 64, None) == _lib.PH_EINVAL and lib.ph_nchw_bias_add(p, p, 2, 256, 0, None) == _lib.PH_EINVAL
    for args in ((None, p, p, 2, 256, 64), (p, None, p, 2, 256, 64), (p, p, None, 2, 256, 64), (p, p, p, 0, 256, 64), (p, p, p, 2, 0, 64),
                 (p, p, p, 2, 256, 0)):
        assert lib.ph_nchw_channel_sums(*args, None) == _lib.PH_EINVAL, args
    ns = [lib.ph_nchw_channel_sums_nsplit(hw) for hw in (1, 4096, 4097, 33828, 131072, 1 << 22)]
    assert ns == [1, 1, 2, 9, 32, 64]                      # a 256 x 512 plane is 32 workgroups' job, never one's


def test_gather_rule_of_the_backward_is_torchs_autograd():
    """under the size rule fine row y reads coarse row y >> 1, so coarse row Y gathers fine rows 2Y and 2Y + 1 where they exist:
    checked against the autograd of F.interpolate(mode='nearest', size=H) for every Hc <= 600 and both sizes"""
    for Hc in range(1, 601):
        for H in (2 * Hc, 2 * Hc - 1):
            c = torch.zeros(1, 1, Hc, 1, requires_grad=True)
            with torch.enable_grad():
                up = F.interpolate(c, size=(H, 1), mode="nearest")
            g = torch.arange(1, H + 1, dtype=torch.float32).reshape(1, 1, H, 1)          # integers: sums are exact in any order
            (want,) = torch.autograd.grad(up, c, g)
            Y = torch.arange(Hc)
            gf = g.reshape(-1)
            got = gf[2 * Y] + torch.where(2 * Y + 1 < H, gf[(2 * Y + 1).clamp(max=H - 1)], torch.zeros(()))
            assert torch.equal(got, want.reshape(-1)), (Hc, H)
            assert torch.equal(torch.arange(H) >> 1, torch.clamp(torch.arange(H) * Hc // H, max=Hc - 1)), (Hc, H)


def _fpn():
    return NECKS.build(json.load(open(os.path.join(Hh.GOLDEN, "fpn_cfg.json"))))


def test_train_on_device_is_off_by_default_and_names_a_cpu_input():
    m = _fpn().train()
    assert m.device_training is False
    sizes = ((9, 11), (5, 6), (3, 3), (2, 2))
    feats = [torch.randn(1, c, h, w) for c, (h, w) in zip(m.in_channels, sizes)]
    with torch.enable_grad():
        outs = m(feats)                                         # off: torch ops, on the CPU too
        assert len(outs) == 4 and all(o.requires_grad for o in outs)
        assert m.train_on_device() is m and m.device_training is True
        with pytest.raises(_lib.PolyheadError, match=r"inputs\[0\].*GPU"):
            m(feats)
        m.train_on_device(False)
        assert all(torch.equal(a, b) for a, b in zip(m(feats), outs))
    assert list(m.state_dict()) == list(_fpn().state_dict()) and len(m.state_dict()) == 16
