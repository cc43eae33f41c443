"""Host-side checks of the native decode plan (include/polyhead.h ph_decode_*): the workspace rule against engine.DecodePlan's
buffers, the launch geometry rule (one copy, in the library: ph_decode_geometry_of, which engine.DecodePlan asks too) against the
choices recorded in tests/golden/plan_geometry.json, the pack layout against pack.py's, and argument validation (symbols, struct
layouts and the example programs' dependencies: tests/test_abi.py).  No GPU: nothing here launches a kernel."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import bench
import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
from polyphonicformer_amd import build as BLD
from polyphonicformer_amd.pack import pack_stage

# (B, N, H, W, S, L): cfg1 (256x512 -> 32x64, N = 100, 1 stage), cfg2 / cfg3 (128x256, N = 153 / 111), cfg5 (48x156, N = 253)
SHAPES = {"cfg1": (100, 32, 64, 1, 19), "cfg2": (153, 128, 256, 3, 133), "cfg3": (111, 128, 256, 3, 19), "cfg5": (253, 48, 156, 3, 133)}
MODES = ["fp32", "mixed", "mixed16", "fp16", "bf16"]
FAKE_PTR = 1 << 40          # a 256-byte aligned address create() stores and never dereferences


def _lib_loaded():
    return _lib.load()


def test_param_table_is_the_stage_state_dict():
    lib = _lib_loaded()
    wl = dict(bench.WORKLOADS["tiny"], S=1)
    head = bench.build_head(wl, "fp32", torch.float32, "cpu")
    sd = head.mask_head[0].state_dict()
    names = [lib.ph_decode_param_name(i).decode() for i in range(_lib.PH_DECODE_NPARAMS)]
    assert lib.ph_decode_param_name(_lib.PH_DECODE_NPARAMS) is None
    assert names == list(sd.keys())
    cfg = _lib.DecodeCfg(B=1, N=100, H=16, W=32, S=1, L=wl["n_thing"] + wl["n_stuff"], F=wl["F"], mode=0)
    assert [lib.ph_decode_param_numel(C.byref(cfg), i) for i in range(len(names))] == [v.numel() for v in sd.values()]


class _FakePack:
    def __init__(self, prec, L, F=2048):
        self.prec, self.num_classes = prec, L
        self.lay = _lib.StageLayout(ffn_dim=F, num_classes=L)


def _al(n):
    return (n + 255) // 256 * 256


def _decode_plan_bytes(p):
    """the bytes of every buffer engine.DecodePlan allocates that the native plan keeps in its workspace: everything but the
    inputs (x, depth_feats, k0, q0, m0) and the caller's outputs (mask, mask_up, depth_up, the last stage's obj / dobj / cls);
    the low-resolution depth logits only where the final stage writes them (two-kernel form).  256-byte pieces."""
    nb = lambda t: _al(t.numel() * t.element_size())
    total = nb(p.xp) + nb(p.dp) + nb(p.bits) + nb(p.partial) + nb(p.pcount) + nb(p.ws)
    for s, o in enumerate(p.stage_out):
        total += nb(o["kern"]) + nb(o["kbias"])
        if s < p.S - 1:
            total += nb(o["obj"]) + nb(o["dobj"]) + nb(o["cls"])
    if not p.fused_up:
        total += nb(p.depth)
    if p.poolx:
        total += nb(p.partial_px) + nb(p.pcount_px)
    return total


def _create(cfg, S):
    lib = _lib_loaded()
    h = C.c_void_p()
    rc = lib.ph_decode_create(C.byref(cfg), (C.c_void_p * S)(*([FAKE_PTR] * S)), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h))
    return rc, h


# ---- the recorded choices of the launch geometry rule.  tests/golden/plan_geometry.json holds what engine.DecodePlan's own
# arithmetic chose at the commit named in the file, before that arithmetic was deleted in favour of the library's: the matrix of
# test_workspace_and_geometry_match_decode_plan, the environment cases, an explicit nsplit, and both sides of every threshold
ENV_KEYS = ("PH_POOL_NSPLIT", "PH_CONV_UP2", "PH_CONV_POOLX", "PH_POOLX_NSPLIT", "PH_UP2_SHARED_WGS", "PH_QUERY_FULL_SPLIT")
GEO_FIELDS = [n for n, _ in _lib.DecodeGeometry._fields_]


@functools.lru_cache(maxsize=None)
def _table():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_geometry.json")) as f:
        return json.load(f)


def _row_env(row, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)


def _row_args(row):
    return (row["B"], row["N"], row["H"], row["W"], row["S"], row["L"], E.MODES[row["mode"]], getattr(torch, row["out_dtype"]),
            row["frame_invariant"], row["nsplit_arg"])


def _geometry_of(cfg):
    g = _lib.DecodeGeometry()
    rc = _lib_loaded().ph_decode_geometry_of(C.byref(cfg), C.byref(g))
    assert rc == 0, _lib_loaded().ph_last_error_string()
    return g


def test_recorded_table_pins_both_branches():
    rows = _table()["decode_geometry"]
    assert len(rows) >= 216 and len(_table()["producing_commit"]) == 40
    for i in (2, 3):            # poolx, fused_up
        assert {r["expect"][i] for r in rows} == {False, True}
    assert {r["case"].split(":")[0] for r in rows} >= {"matrix", "env", "nsplit_arg", "thr"}


def test_geometry_of_equals_the_recorded_table(monkeypatch):
    """the library's rule (resolve() of ph_decode.hip through ph_decode_geometry_of: no plan, no device, no packs) chooses what the
    Python rule chose, row by row; and ph_decode_info on a plan created from the same cfg is the same fill, field by field"""
    lib = _lib_loaded()
    for row in _table()["decode_geometry"]:
        _row_env(row, monkeypatch)
        B, N, H, W, S, L, m, out_dtype, fi, nsplit = _row_args(row)
        for shares in (False, True):
            cfg = E.native_cfg(B, N, H, W, S, L, 2048, m, out_dtype, fi, shares, nsplit)
            g = _geometry_of(cfg)
            assert [g.nsplit, g.nsplit_px, bool(g.poolx), bool(g.fused_up)] == row["expect"], (row, shares)
            assert g.up2_workgroups == 0, row           # cfg.up2_wgs == 0: only ph_decode_create asks the device
            cfg.up2_wgs = 384                           # 1.5 per CU of a 256-CU device
            g = _geometry_of(cfg)
            assert g.up2_workgroups == (384 if (row["expect"][3] and shares and B * H >= 4 * 384) else 0), (row, shares)
            rc, h = _create(cfg, S)
            assert rc == 0, (row, lib.ph_last_error_string())
            gi = _lib.DecodeGeometry()
            assert lib.ph_decode_info(h, C.byref(gi)) == 0
            lib.ph_decode_destroy(h)
            assert [getattr(gi, f) for f in GEO_FIELDS] == [getattr(g, f) for f in GEO_FIELDS], (row, shares)


def test_decode_plan_attributes_equal_the_recorded_table(monkeypatch):
    """engine.DecodePlan (which now asks the library) still chooses what its own arithmetic chose"""
    for row in _table()["decode_geometry"]:
        _row_env(row, monkeypatch)
        B, N, H, W, S, L, m, out_dtype, fi, nsplit = _row_args(row)
        p = E.DecodePlan([_FakePack(m.query, L) for _ in range(S)], B, N, H, W, m, out_dtype, device="meta", nsplit=nsplit,
                         frame_invariant=fi)
        assert [p.nsplit, p.nsplit_px, p.poolx, p.fused_up] == row["expect"], row
        assert p.poolx == hasattr(p, "partial_px"), row


def test_default_nsplit_equals_the_recorded_table(monkeypatch):
    monkeypatch.delenv("PH_POOL_NSPLIT", raising=False)
    lib = _lib_loaded()
    rows = _table()["default_nsplit"]
    assert len(rows) == 8 * 4 * 2
    for r in rows:
        assert lib.ph_pool_default_nsplit(r["B"], r["HW"], int(r["frame_invariant"])) == r["expect"], r
        assert E.default_nsplit(r["B"], r["HW"], r["frame_invariant"]) == r["expect"], r
    monkeypatch.setenv("PH_POOL_NSPLIT", "7")           # the override stays the Python side's
    assert E.default_nsplit(1, 32768) == 7 and lib.ph_pool_default_nsplit(1, 32768, 0) == 32


def test_decode_plan_refuses_what_the_library_refuses():
    """a geometry the kernels cannot run is an error at construction (it used to surface at the first launch)"""
    m = E.MODES["fp16"]
    with pytest.raises(_lib.PolyheadError, match="at most 256 queries"):
        E.DecodePlan([_FakePack(m.query, 19)], 1, 300, 16, 32, m, torch.float16, device="meta")
    g = _lib.DecodeGeometry()
    assert _lib_loaded().ph_decode_geometry_of(None, C.byref(g)) == -1
    cfg = E.native_cfg(1, 111, 16, 32, 1, 19, 2048, m, torch.float16)
    assert _lib_loaded().ph_decode_geometry_of(C.byref(cfg), None) == -1 and "null out" in _lib_loaded().ph_last_error_string().decode()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("B", [1, 8, 32])
def test_workspace_and_geometry_match_decode_plan(shape, B, monkeypatch):
    for k in ("PH_POOL_NSPLIT", "PH_CONV_UP2", "PH_CONV_POOLX", "PH_POOLX_NSPLIT", "PH_UP2_SHARED_WGS", "PH_QUERY_FULL_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    lib = _lib_loaded()
    N, H, W, S, L = SHAPES[shape]
    recorded = {(r["B"], r["mode"], r["out_dtype"], r["frame_invariant"]): tuple(r["expect"])
                for r in _table()["decode_geometry"] if r["case"] == "matrix:" + shape}
    for mode in MODES:
        m = E.MODES[mode]
        for out_dtype in ((torch.float32, m.feat_dtype) if m.feat_dtype is not None else (torch.float32,)):
            for fi in (False, True):
                p = E.DecodePlan([_FakePack(m.query, L) for _ in range(S)], B, N, H, W, m, out_dtype, device="meta", frame_invariant=fi)
                for shares in (False, True):
                    cfg = E.native_cfg(B, N, H, W, S, L, 2048, m, out_dtype, fi, shares)
                    cfg.up2_wgs = 384           # the Python plan's 1.5 per CU of a 256-CU device (no device here)
                    what = (shape, B, mode, out_dtype, fi, shares)
                    assert lib.ph_decode_workspace_bytes(C.byref(cfg)) == _decode_plan_bytes(p), what
                    rc, h = _create(cfg, S)
                    assert rc == 0, (what, lib.ph_last_error_string())
                    g = _lib.DecodeGeometry()
                    assert lib.ph_decode_info(h, C.byref(g)) == 0
                    lib.ph_decode_destroy(h)
                    # the geometry against the recorded choices (the Python plan takes its own from the same library call now)
                    want = recorded[(B, mode, str(out_dtype).split(".")[1], fi)]
                    assert (g.nsplit, g.nsplit_px, bool(g.poolx), bool(g.fused_up)) == want == \
                        (p.nsplit, p.nsplit_px, p.poolx, p.fused_up), what
                    wg = 384 if (want[3] and shares and B * H >= 4 * 384) else 0
                    assert g.up2_workgroups == wg, what
                    assert (g.feat_prec, g.query_prec, g.conv_prec, g.kern_format, g.feat_planes) == \
                        (m.feat, m.query, m.conv, m.kern_fmt, m.FP), what


def test_environment_knobs_map_onto_the_cfg(monkeypatch):
    """the switches DecodePlan reads from the environment reach the native plan as cfg fields (the native side reads none)"""
    lib = _lib_loaded()
    monkeypatch.setenv("PH_CONV_UP2", "1")
    monkeypatch.setenv("PH_CONV_POOLX", "1")
    monkeypatch.setenv("PH_POOL_NSPLIT", "3")
    for mode in MODES:
        m = E.MODES[mode]
        out = {"bf16": torch.bfloat16, "mixed16": torch.float16, "fp16": torch.float16}.get(mode, torch.float32)
        p = E.DecodePlan([_FakePack(m.query, 19) for _ in range(2)], 1, 111, 16, 256, m, out, device="meta", frame_invariant=True)
        cfg = E.native_cfg(1, 111, 16, 256, 2, 19, 2048, m, out, True)
        cfg.up2_wgs = 384
        rc, h = _create(cfg, 2)
        assert rc == 0
        g = _lib.DecodeGeometry()
        lib.ph_decode_info(h, C.byref(g))
        lib.ph_decode_destroy(h)
        assert (g.nsplit, g.nsplit_px, bool(g.poolx), bool(g.fused_up)) == (p.nsplit, p.nsplit_px, p.poolx, p.fused_up) == \
            (3, 3, m.conv in (_lib.PH_PREC_BF16, _lib.PH_PREC_F16), m.KP == 1), mode


@pytest.mark.parametrize("mode", MODES)
def test_pack_layout_is_pack_py_layout(mode):
    lib = _lib_loaded()
    wl = dict(bench.WORKLOADS["tiny"], S=1)
    head = bench.build_head(wl, mode, torch.float32, "cpu")
    sd = {k: v.detach() for k, v in head.mask_head[0].state_dict().items()}
    L = wl["n_thing"] + wl["n_stuff"]
    m = E.MODES[mode]
    wb, wf, lay = pack_stage(sd, "", L, m.query)
    cfg = E.native_cfg(1, 100, 16, 32, 1, L, wl["F"], m)
    nlay, off = _lib.StageLayout(), C.c_size_t()
    assert lib.ph_decode_pack_layout(C.byref(cfg), C.byref(nlay), C.byref(off)) == 0
    assert bytes(nlay) == bytes(lay)
    assert off.value == _al(wb.numel() * 2)
    assert lib.ph_decode_pack_bytes(C.byref(cfg)) == off.value + _al(wf.numel() * 4)


def test_errors_are_returned_before_anything_is_launched():
    lib = _lib_loaded()
    base = dict(B=1, N=111, H=128, W=256, S=3, L=19, F=2048, mode=_lib.PH_MODE["fp16"], out_dtype=_lib.PH_OUT_F16, up2_wgs=384)
    # geometry the query / pooling kernels refuse
    cfg = _lib.DecodeCfg(**dict(base, N=300))
    assert lib.ph_decode_workspace_bytes(C.byref(cfg)) == 0 and "at most 256 queries" in Hh.last_error()
    assert _create(cfg, 3)[0] == -2
    cfg = _lib.DecodeCfg(**dict(base, F=1000))
    assert _create(cfg, 3)[0] == -1 and "multiple of 256" in Hh.last_error()
    # a fused form asked for where its kernel cannot run: PH_EUNSUPPORTED (the Python plan would fall back; the native one says so)
    cfg = _lib.DecodeCfg(**dict(base, W=200, fused_up=_lib.PH_KNOB_ON))
    assert _create(cfg, 3)[0] == -2 and "ph_dynconv_up2" in Hh.last_error()
    assert lib.ph_dynconv_up2_supported(111, 128, 200, _lib.PH_PREC_F16, _lib.PH_OUT_F16) == 0
    cfg = _lib.DecodeCfg(**dict(base, N=200, poolx=_lib.PH_KNOB_ON))
    assert _create(cfg, 3)[0] == -2 and "ph_dynconv_poolx" in Hh.last_error()
    assert lib.ph_dynconv_poolx_supported(200, _lib.PH_PREC_F16) == 0
    cfg = _lib.DecodeCfg(**dict(base, S=1, poolx=_lib.PH_KNOB_ON))
    assert _create(cfg, 1)[0] == -2
    # the same requests "where supported" are no error
    cfg = _lib.DecodeCfg(**dict(base, W=200, fused_up=_lib.PH_KNOB_WHERE_SUPPORTED))
    assert _create(cfg, 3)[0] == 0
    # too small a workspace
    cfg = _lib.DecodeCfg(**base)
    need = lib.ph_decode_workspace_bytes(C.byref(cfg))
    h = C.c_void_p()
    rc = lib.ph_decode_create(C.byref(cfg), (C.c_void_p * 3)(*([FAKE_PTR] * 3)), C.c_void_p(FAKE_PTR), need - 256, C.byref(h))
    assert rc == -4 and "workspace too small" in Hh.last_error() and not h.value
    # run-time arguments: in a child process that sees no GPU (_RUN_CHECKS), so that a validation that ever stopped returning
    # before the first launch fails on the host instead of launching a kernel on the fake addresses
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _RUN_CHECKS], cwd=os.path.dirname(BLD.HERE), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "run checks ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


_RUN_CHECKS = r"""
import ctypes as C, sys
sys.path.insert(0, ".")
import torch
from polyphonicformer_amd import _lib
assert torch.cuda.device_count() == 0, "the run-time argument checks need a process without a visible GPU"
lib = _lib.load()
FAKE = 1 << 40
def create(**kw):
    cfg = _lib.DecodeCfg(**dict(dict(B=1, N=111, H=128, W=256, S=3, L=19, F=2048, mode=_lib.PH_MODE["fp16"], out_dtype=_lib.PH_OUT_F16,
                                     up2_wgs=384), **kw))
    h = C.c_void_p()
    assert lib.ph_decode_create(C.byref(cfg), (C.c_void_p * 3)(*([FAKE] * 3)), C.c_void_p(FAKE), 1 << 62, C.byref(h)) == 0
    return h
msg = lambda: lib.ph_last_error_string().decode()
h = create()
io = _lib.DecodeIO(feat_format=_lib.PH_FEAT_F32, x=FAKE, depth_feats=FAKE, k0=FAKE, q0=FAKE, m0=FAKE, obj=FAKE, dobj=FAKE, cls=FAKE,
                   mask=FAKE, mask_up=FAKE, depth_up=None)
assert lib.ph_decode_run(h, C.byref(io), None) == -1 and "null input or output" in msg()
io.depth_up, io.feat_format = FAKE, 7
assert lib.ph_decode_run(h, C.byref(io), None) == -1 and "feat_format" in msg()
io.feat_format, io.bits = _lib.PH_FEAT_PLANES, None
assert lib.ph_decode_run(h, C.byref(io), None) == -1 and "bits" in msg()
io.feat_format, io.m0_dtype = _lib.PH_FEAT_F32, 9
assert lib.ph_decode_run(h, C.byref(io), None) == -1 and "m0_dtype" in msg()
lib.ph_decode_destroy(h)
h = create(mode=_lib.PH_MODE["fp32"], out_dtype=_lib.PH_OUT_F32)
io.feat_format, io.m0_dtype = _lib.PH_FEAT_16, _lib.PH_OUT_F32
assert lib.ph_decode_run(h, C.byref(io), None) == -1 and "16-bit feature inputs" in msg()
lib.ph_decode_destroy(h)
print("run checks ok")
"""


_LOSS_ARG_CHECKS = r"""
import ctypes as C, sys
sys.path.insert(0, ".")
import torch
from polyphonicformer_amd import _lib
from polyphonicformer_amd.losses import LossCfg
assert torch.cuda.device_count() == 0, "the argument checks need a process without a visible GPU"
lib = _lib.load()
FAKE = C.c_void_p(1 << 40)
msg = lambda: lib.ph_last_error_string().decode()
def call(**kw):
    c = LossCfg(**dict(dict(B=2, N=600, L=19, P=1100, depth_rows=1200, HW=493, has_rank=1, ignore=255, cls_avg=1.0), **kw))
    # scratch_bytes = 0: a cfg that passes every earlier check stops at "scratch too small", before anything is launched
    return lib.ph_train_losses(C.byref(c), FAKE, None, FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, None, None,
                               None, FAKE, None, None, None, None, FAKE, 0, None)
assert call() == -1 and "at most 512 positive rows per image" in msg(), msg()        # N and P both beyond what the rank target keeps
assert call(N=513, P=513) == -1 and "at most 512 positive rows per image" in msg(), msg()
for kw in (dict(N=512), dict(P=512, N=4000), dict(has_rank=0), dict(P=0)):           # an image cannot have more than min(N, P)
    assert call(**kw) == -1 and "scratch too small" in msg(), (kw, msg())
print("loss checks ok")
"""


def test_train_losses_refuses_more_rank_rows_than_it_keeps():
    """`k_rank_target_p` lists at most 512 positive rows per image: `ph_train_losses` returns PH_EINVAL for a cfg that could
    exceed that instead of dropping rows.  In a child process that sees no GPU, on fake addresses: nothing is launched."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _LOSS_ARG_CHECKS], cwd=os.path.dirname(BLD.HERE), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "loss checks ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
