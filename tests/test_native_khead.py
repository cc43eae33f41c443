"""Host-side checks of the native KernelHead plan (include/polyhead.h ph_khead_cfg .. ph_khead_plan_timeouts): the parameter
table against KernelHead's own state_dict, the pack layout, the environment -> cfg mapping and argument validation (symbols, struct
layouts and the example programs' dependencies: tests/test_abi.py).  No GPU: nothing here
launches a kernel (the one-pass rule needs the device's CU count: tests/test_gpu_native_khead.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
from polyphonicformer_amd import build as BLD
from polyphonicformer_amd.registry import HEADS
import polyphonicformer_amd.kernel_head  # noqa: F401

FAKE_PTR = 1 << 40          # a 256-byte aligned address create() stores and never dereferences
def _cfg(**kw):
    base = dict(B=2, H=48, W=156, num_proposals=100, num_classes=19, num_thing_classes=8, cat_stuff=1, groups=32,
                mode=_lib.PH_MODE["fp16"], logit_dtype=_lib.PH_OUT_F32, emit_f32=1)
    return _lib.KheadCfg(**dict(base, **kw))


def _kernel_head(Nq=100, n_thing=8, n_stuff=11):
    return HEADS.build(dict(type="KernelHead", num_proposals=Nq, num_classes=n_thing + n_stuff, num_thing_classes=n_thing,
                            num_stuff_classes=n_stuff, in_channels=256, out_channels=256, cat_stuff_mask=True,
                            feat_downsample_stride=2, feat_refine_stride=1, feat_refine=False, use_binary=True,
                            conv_normal_init=True, proposal_feats_with_obj=True, xavier_init_kernel=False, kernel_init_std=1,
                            loss_seg=dict(type="FocalLoss", use_sigmoid=True), localization_fpn=None))


class _Recorder(dict):
    """a state_dict that records the keys read from it"""

    def __init__(self, d):
        super().__init__(d)
        self.read = []

    def __getitem__(self, k):
        self.read.append(k)
        return super().__getitem__(k)


def test_param_table_is_what_kernel_head_pack_reads():
    lib = _lib.load()
    h = _kernel_head(Nq=37, n_thing=5, n_stuff=9)
    sd = _Recorder(h.state_dict())
    E.KernelHeadPack(sd, _lib.PH_PREC_BF16, "cpu", 32)
    names = [lib.ph_khead_param_name(i).decode() for i in range(_lib.PH_KHEAD_NPARAMS)]
    assert lib.ph_khead_param_name(_lib.PH_KHEAD_NPARAMS) is None and lib.ph_khead_param_name(-1) is None
    assert set(names) == set(sd.read) and len(set(names)) == _lib.PH_KHEAD_NPARAMS
    cfg = _cfg(num_proposals=37, num_classes=14, num_thing_classes=5)
    assert [lib.ph_khead_param_numel(C.byref(cfg), i) for i in range(len(names))] == [sd[n].numel() for n in names]
    assert lib.ph_khead_param_numel(C.byref(cfg), len(names)) < 0


@pytest.mark.parametrize("mode", ["fp16", "bf16", "fp32", "mixed", "mixed16"])
def test_pack_layout(mode):
    """offsets 256-byte aligned, in order, non-overlapping, summing to ph_khead_pack_bytes; sizes those of KernelHeadPack's tensors"""
    lib = _lib.load()
    h = _kernel_head()
    prec = E.KHEAD_PREC[mode]
    ref = E.KernelHeadPack(h.state_dict(), prec, "cpu", 32)
    cfg = _cfg(mode=_lib.PH_MODE[mode])
    lay = _lib.KheadLayout()
    assert lib.ph_khead_pack_layout(C.byref(cfg), C.byref(lay)) == 0
    end = 0
    for i, name in enumerate(_lib.KPACK_PIECES):
        assert lay.offset[i] % 256 == 0 and lay.offset[i] == end, name
        t = getattr(ref, name)
        assert lay.bytes[i] == (0 if t is None else t.numel() * t.element_size()), name
        end = lay.offset[i] + (lay.bytes[i] + 255) // 256 * 256
    assert end == lib.ph_khead_pack_bytes(C.byref(cfg))
    assert (getattr(ref, "conv_frag") is None) == (prec == _lib.PH_PREC_SPLIT)


def test_native_khead_cfg_maps_the_environment(monkeypatch):
    """the switches KernelHeadPlan reads from the environment reach the native plan as cfg fields"""
    for k in ("PH_KHEAD_TWOPASS", "PH_POOL_NSPLIT"):
        monkeypatch.delenv(k, raising=False)
    args = (3, 48, 156, 100, 19, 8, True, 32)
    c = E.native_khead_cfg(*args, "fp16")
    assert (c.onepass, c.nsplit, c.mode, c.emit_f32, c.logit_dtype) == (_lib.PH_KNOB_AUTO, 0, _lib.PH_MODE["fp16"], 1, _lib.PH_OUT_F32)
    assert E.native_khead_cfg(*args, "fp16", onepass=False).onepass == _lib.PH_KNOB_OFF
    assert E.native_khead_cfg(*args, "fp16", onepass=True).onepass == _lib.PH_KNOB_ON
    assert E.native_khead_cfg(*args, _lib.PH_PREC_SPLIT).mode == _lib.PH_MODE["fp32"]
    assert E.native_khead_cfg(*args, "bf16", logit_dtype=torch.float16, want_f32=False, frame_invariant=True, nsplit=5).nsplit == 5
    monkeypatch.setenv("PH_KHEAD_TWOPASS", "1")
    monkeypatch.setenv("PH_POOL_NSPLIT", "3")
    c = E.native_khead_cfg(*args, "fp16")
    assert (c.onepass, c.nsplit) == (_lib.PH_KNOB_OFF, 3)
    assert E.native_khead_cfg(*args, "fp16", nsplit=7).nsplit == 7
    with pytest.raises(_lib.PolyheadError):
        E.native_khead_cfg(*args, "fp16", onepass=True)


def _create(cfg, nbytes=1 << 62):
    h = C.c_void_p()
    rc = _lib.load().ph_khead_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), nbytes, C.byref(h))
    return rc, h


# cfgs every entry point that takes one refuses: (fields, return code, a word of the message) and fields alone
BAD_WITH_WORD = [(dict(groups=24), -1, "groups"), (dict(mode=9), -1, "bad mode"),
                 (dict(logit_dtype=_lib.PH_OUT_F16, onepass=_lib.PH_KNOB_OFF), -2, "one-pass form")]
BAD = (dict(num_proposals=0), dict(num_proposals=300), dict(num_classes=300), dict(num_thing_classes=20), dict(B=0),
       dict(onepass=7), dict(nsplit=-1), dict(logit_dtype=_lib.PH_OUT_BF16), dict(num_proposals=250, num_classes=30),
       dict(nsplit=1000))
# the cfgs this file creates plans from on a machine without a device (two-pass: the one-pass rule is not asked)
TWO_PASS = (dict(onepass=_lib.PH_KNOB_OFF), dict(onepass=_lib.PH_KNOB_OFF, mode=_lib.PH_MODE["mixed"], cat_stuff=0, frame_invariant=1))


def test_errors_are_returned_before_anything_is_launched():
    lib = _lib.load()
    ws = lambda cfg: lib.ph_khead_plan_workspace_bytes(C.byref(cfg))
    cfg = _cfg(groups=24)
    assert ws(cfg) == 0 and "groups" in Hh.last_error()
    assert lib.ph_khead_pack_bytes(C.byref(cfg)) == 0 and "groups" in Hh.last_error()
    assert _create(cfg)[0] == -1 and "groups" in Hh.last_error()
    cfg = _cfg(mode=9)
    assert ws(cfg) == 0 and "bad mode" in Hh.last_error()
    assert _create(cfg)[0] == -1
    cfg = _cfg(logit_dtype=_lib.PH_OUT_F16, onepass=_lib.PH_KNOB_OFF)
    assert ws(cfg) == 0 and "one-pass form" in Hh.last_error()
    assert _create(cfg)[0] == -2 and "one-pass form" in Hh.last_error()
    for bad in BAD:
        assert ws(_cfg(**bad)) == 0 and Hh.last_error(), bad
        rc, h = _create(_cfg(**bad))
        assert rc < 0 and not h.value, bad
    # two-pass plans need no device: the size, a short workspace, a good one
    cfg = _cfg(onepass=_lib.PH_KNOB_OFF)
    need = ws(cfg)
    assert need > 0 and need % 256 == 0
    rc, h = _create(cfg, need - 256)
    assert rc == -4 and "workspace too small" in Hh.last_error() and not h.value
    rc, h = _create(cfg, need)
    assert rc == 0 and h.value
    g = _lib.KheadGeometry()
    assert lib.ph_khead_plan_info(h, C.byref(g)) == 0
    assert (g.onepass, g.N, g.Npad, g.HWp, g.P, g.prec, g.n_stuff) == (0, 111, 128, 7552, 1, _lib.PH_PREC_F16, 11)
    assert g.nsplit == E.default_nsplit(2, 48 * 156)
    lib.ph_khead_plan_destroy(h)
    rc, h = _create(_cfg(onepass=_lib.PH_KNOB_OFF, mode=_lib.PH_MODE["mixed"], cat_stuff=0, frame_invariant=1))
    assert rc == 0
    lib.ph_khead_plan_info(h, C.byref(g))
    assert (g.N, g.P, g.prec, g.n_stuff, g.nsplit) == (100, 2, _lib.PH_PREC_SPLIT, 0, E.default_nsplit(2, 48 * 156, True))
    lib.ph_khead_plan_destroy(h)
    # pack / run arguments, in a child process that sees no GPU: a check that ever stopped returning before the first launch would
    # fail on the host instead of launching on the fake addresses
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _RUN_CHECKS], cwd=os.path.dirname(BLD.HERE), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "run checks ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_geometry_of_is_what_a_plan_reports():
    """ph_khead_geometry_of(cfg) against ph_khead_plan_info of a plan created from the same cfg: the two structs byte for byte"""
    lib = _lib.load()
    for kw in TWO_PASS:
        cfg = _cfg(**kw)
        asked, told = _lib.KheadGeometry(), _lib.KheadGeometry()
        assert lib.ph_khead_geometry_of(C.byref(cfg), C.byref(asked)) == 0, Hh.last_error()
        rc, h = _create(cfg)
        assert rc == 0 and lib.ph_khead_plan_info(h, C.byref(told)) == 0
        lib.ph_khead_plan_destroy(h)
        assert bytes(asked) == bytes(told), kw
        assert asked.onepass == 0 and asked.nsplit > 0


def test_geometry_of_checks_its_arguments():
    """null cfg, null out and every cfg ph_khead_plan_workspace_bytes refuses: the same codes and messages, `out` untouched"""
    lib = _lib.load()
    g = _lib.KheadGeometry()
    assert lib.ph_khead_geometry_of(None, C.byref(g)) == -1 and "ph_khead_geometry_of: null cfg" in Hh.last_error()
    assert lib.ph_khead_geometry_of(C.byref(_cfg(onepass=_lib.PH_KNOB_OFF)), None) == -1 and "ph_khead_geometry_of: null out" in Hh.last_error()
    for kw, rc, word in BAD_WITH_WORD:
        assert lib.ph_khead_geometry_of(C.byref(_cfg(**kw)), C.byref(g)) == rc and word in Hh.last_error(), kw
    for kw in BAD:
        assert lib.ph_khead_geometry_of(C.byref(_cfg(**kw)), C.byref(g)) < 0 and "ph_khead_geometry_of" in Hh.last_error(), kw
    assert bytes(g) == bytes(_lib.KheadGeometry())


_RUN_CHECKS = r"""
import ctypes as C, sys
sys.path.insert(0, ".")
import torch
from polyphonicformer_amd import _lib
assert torch.cuda.device_count() == 0, "the run-time argument checks need a process without a visible GPU"
lib = _lib.load()
FAKE = 1 << 40
msg = lambda: lib.ph_last_error_string().decode()
cfg = _lib.KheadCfg(B=2, H=48, W=156, num_proposals=100, num_classes=19, num_thing_classes=8, cat_stuff=1, groups=32,
                    mode=_lib.PH_MODE["fp16"], logit_dtype=_lib.PH_OUT_F32, emit_f32=1)
# without a device the one-pass form cannot be chosen: AUTO gives a two-pass plan, ON is an error
assert lib.ph_khead_onepass_supported(2, 48 * 156, 32, _lib.PH_PREC_F16, _lib.PH_IN_F32_NCHW) == 0
cfg.onepass = _lib.PH_KNOB_ON
assert lib.ph_khead_plan_workspace_bytes(C.byref(cfg)) == 0 and "ph_khead_onepass cannot run" in msg()
geo = _lib.KheadGeometry()
assert lib.ph_khead_geometry_of(C.byref(cfg), C.byref(geo)) == -2 and "ph_khead_onepass cannot run" in msg()
cfg.onepass = _lib.PH_KNOB_AUTO
assert lib.ph_khead_geometry_of(C.byref(cfg), C.byref(geo)) == 0 and geo.onepass == 0
params = (C.c_void_p * _lib.PH_KHEAD_NPARAMS)(*([FAKE] * _lib.PH_KHEAD_NPARAMS))
assert lib.ph_khead_pack(C.byref(cfg), params, C.c_void_p(FAKE + 16), None) == -1 and "aligned" in msg()
params[11] = None
assert lib.ph_khead_pack(C.byref(cfg), params, C.c_void_p(FAKE), None) == -1 and "conv_seg.bias" in msg()
h = C.c_void_p()
assert lib.ph_khead_plan_create(C.byref(cfg), C.c_void_p(FAKE), C.c_void_p(FAKE), 1 << 62, C.byref(h)) == 0
ptrs = dict(f0=FAKE, f1=FAKE, f2=FAKE, xp=FAKE, dp=FAKE, bits=FAKE, x_f32=FAKE, dfe_f32=FAKE, mask_preds=FAKE, seg_preds=FAKE,
            depth_pred=FAKE, proposal=FAKE)
run = lambda **kw: lib.ph_khead_plan_run(h, C.byref(_lib.KheadIO(**dict(dict(ptrs, input_format=_lib.PH_IN_F32_NCHW), **kw))), None)
assert run(input_format=5) == -1 and "input_format" in msg()
assert run(f1=None) == -1 and "input map" in msg()
assert run(bits=None) == -1 and "output pointer" in msg()
assert run(x_f32=None) == -1 and "emit_f32" in msg()
assert run(depth_proposal=FAKE + 4) == -1 and "depth_proposal" in msg()
assert lib.ph_khead_plan_status(h, None) == 0 and lib.ph_khead_plan_timeouts(h, None) == 0      # two-pass plans: no device read
lib.ph_khead_plan_destroy(h)
cfg.emit_f32 = 0
assert lib.ph_khead_plan_create(C.byref(cfg), C.c_void_p(FAKE), C.c_void_p(FAKE), 1 << 62, C.byref(h)) == 0
assert run() == -1 and "emit_f32" in msg()
lib.ph_khead_plan_destroy(h)
print("run checks ok")
"""
