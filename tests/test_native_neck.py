"""Host-side checks of the native neck plan (include/polyhead.h ph_neck_cfg .. ph_neck_plan_run_outputs): the parameter table against the reference's state_dict keys, the pack layout, the
workspace size, argument validation and the geometry rules (`fused_out`, `c16`, `tile_rows`).  No GPU: nothing here launches a
kernel (tests/test_gpu_native_neck.py does)."""
import ctypes as C
import json
import os

import pytest

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
from polyphonicformer_amd.registry import NECKS
import polyphonicformer_amd.semantic_fpn  # noqa: F401

FAKE_PTR = 1 << 40          # a 256-byte aligned address create() stores and never dereferences
S3 = ((32, 64), (16, 32), (8, 16), (4, 8))
# the issue's S1 and S2: stride-2 pyramids by the (n + 1) / 2 rule whose levels 2 / 3 do not reach level 1's size by x2 upsampling
# (3 x 4 -> 6 x 8, not 5 x 7; 2 x 18 -> 8 x 72, not 8 x 70).  The reference's level sum is undefined there and engine.NeckPlan raises in
# the middle of its run; the native plan must refuse them BEFORE any launch
S1_ISSUE = ((9, 13), (5, 7), (3, 4), (2, 2))
S2_ISSUE = ((16, 140), (8, 70), (4, 35), (2, 18))


def _cfg(shapes=S3, **kw):
    base = dict(B=2, groups=32, mode=_lib.PH_MODE["fp16"], num_outs=3, pos_level=3, emit_planes=1)
    base.update(kw)
    return _lib.NeckCfg(h=(C.c_int32 * 4)(*[s[0] for s in shapes]), w=(C.c_int32 * 4)(*[s[1] for s in shapes]), **base)


def _neck(num_aux_convs=2, groups=32):
    return NECKS.build(dict(type="SemanticFPNWrapper", in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
                            upsample_times=2, positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                            cat_coors=False, cat_coors_level=3, fuse_by_cat=False, return_list=False, num_aux_convs=num_aux_convs,
                            norm_cfg=dict(type="GN", num_groups=groups, requires_grad=True)))


def test_param_table_is_the_reference_state_dict():
    """ph_neck_param_name against tests/golden/neck_state_keys.json (the reference module's keys) and against this module's own
    state_dict: as a set, and per conv in (weight, gamma, beta) order; the element counts are the module's tensors'"""
    lib = _lib.load()
    with open(os.path.join(Hh.GOLDEN, "neck_state_keys.json")) as f:
        ref = json.load(f)["full"]
    names = [lib.ph_neck_param_name(i).decode() for i in range(_lib.PH_NECK_NPARAMS)]
    assert lib.ph_neck_param_name(_lib.PH_NECK_NPARAMS) is None and lib.ph_neck_param_name(-1) is None
    assert set(names) == set(ref) and len(set(names)) == _lib.PH_NECK_NPARAMS
    convs = ["convs_all_levels.0.conv0", "convs_all_levels.1.conv0", "convs_all_levels.2.conv0", "convs_all_levels.2.conv1",
             "convs_all_levels.3.conv0", "convs_all_levels.3.conv1", "convs_all_levels.3.conv2", "conv_pred", "aux_convs.0", "aux_convs.1"]
    assert names == [f"{c}.{leaf}" for c in convs for leaf in ("conv.weight", "gn.weight", "gn.bias")]
    sd = _neck().state_dict()
    assert set(sd) == set(names)
    cfg = _cfg()
    numel = [lib.ph_neck_param_numel(C.byref(cfg), i) for i in range(len(names))]
    assert numel == [sd[n].numel() for n in names]
    for n, k in zip(names, numel):
        shape = ref[n]
        assert k == int(__import__("math").prod(shape)), n
    assert lib.ph_neck_param_numel(C.byref(cfg), len(names)) < 0 and lib.ph_neck_param_numel(C.byref(cfg), -1) < 0


@pytest.mark.parametrize("mode,P", [("fp16", 1), ("bf16", 1), ("fp32", 2), ("mixed", 2)])
@pytest.mark.parametrize("num_outs", [1, 3])
def test_pack_layout(mode, P, num_outs):
    """offsets 256-byte aligned, in order, non-overlapping, ending at ph_neck_pack_bytes; sizes from the formulas of the header:
    wp = P planes of 256 x K 16-bit values (K = 2304 for 3x3, 256 for 1x1), gamma / beta 256 floats, outs_w [P][3][256][256]
    16-bit and outs_gn [3][2][256] floats with three outputs only"""
    lib = _lib.load()
    cfg = _cfg(mode=_lib.PH_MODE[mode], num_outs=num_outs)
    lay = _lib.NeckLayout()
    assert lib.ph_neck_pack_layout(C.byref(cfg), C.byref(lay)) == 0
    want = []
    for c in range(10):
        present = c < 7 + num_outs
        K = 2304 if c < 7 else 256
        want += [P * 256 * K * 2 if present else 0, 1024 if present else 0, 1024 if present else 0]
    want += [P * 3 * 256 * 256 * 2 if num_outs == 3 else 0, 3 * 2 * 256 * 4 if num_outs == 3 else 0]
    assert list(lay.bytes) == want
    end = 0
    for i in range(_lib.PH_NPACK_COUNT):
        assert lay.offset[i] % 256 == 0 and lay.offset[i] == end, i
        end = lay.offset[i] + (lay.bytes[i] + 255) // 256 * 256
    assert end == lib.ph_neck_pack_bytes(C.byref(cfg))
    last = max(i for i in range(_lib.PH_NPACK_COUNT) if lay.bytes[i])
    assert lib.ph_neck_pack_bytes(C.byref(cfg)) == (lay.offset[last] + lay.bytes[last] + 255) // 256 * 256


def test_workspace_bytes():
    lib = _lib.load()
    ws = lambda **kw: lib.ph_neck_plan_workspace_bytes(C.byref(_cfg(**kw)))
    for mode in ("fp16", "fp32"):
        for fo in (_lib.PH_KNOB_AUTO, _lib.PH_KNOB_OFF):
            sizes0 = [ws(B=B, mode=_lib.PH_MODE[mode], fused_out=fo, tower_buffers=0) for B in (1, 2, 3, 5, 8)]
            sizes1 = [ws(B=B, mode=_lib.PH_MODE[mode], fused_out=fo, tower_buffers=1) for B in (1, 2, 3, 5, 8)]
            assert all(s > 0 and s % 256 == 0 for s in sizes0 + sizes1)
            assert all(a > b for a, b in zip(sizes1, sizes0))                    # a set of buffers per level is larger
            assert sizes0 == sorted(sizes0) and sizes1 == sorted(sizes1)         # non-decreasing in B


# cfgs every entry point that takes one refuses, with a word of the message
BAD = [(dict(shapes=((9, 13), (5, 8), (3, 4), (2, 2))), "stride-2 pyramid"),
       (dict(shapes=S1_ISSUE), "stride-8 size"), (dict(shapes=S2_ISSUE), "stride-8 size"),
       (dict(groups=48), "groups"), (dict(B=0), "B > 0"), (dict(num_outs=4), "num_outs"), (dict(num_outs=0), "num_outs"),
       (dict(emit_planes=0, emit_f32=0), "emit_planes"), (dict(pos_level=4), "pos_level"), (dict(pos_level=-2), "pos_level"),
       (dict(fused_out=_lib.PH_KNOB_ON, num_outs=1), "ph_neck_out_convs"),
       (dict(fused_out=_lib.PH_KNOB_ON, groups=16), "ph_neck_out_convs"),
       (dict(fused_out=_lib.PH_KNOB_ON, mode=_lib.PH_MODE["fp32"]), "ph_neck_out_convs"),
       (dict(mode=9), "bad mode"), (dict(fused_out=7), "knob"), (dict(c16=_lib.PH_KNOB_ON), "knob"), (dict(tower_buffers=2), "knob"),
       (dict(eps=-1.0), "eps")]


def test_bad_cfgs_are_refused_with_a_message():
    lib = _lib.load()
    for kw, word in BAD:
        cfg = _cfg(**kw)
        assert lib.ph_neck_plan_workspace_bytes(C.byref(cfg)) == 0 and word in Hh.last_error(), (kw, Hh.last_error())
        assert lib.ph_neck_pack_bytes(C.byref(cfg)) == 0 and word in Hh.last_error(), kw
        h = C.c_void_p()
        rc = lib.ph_neck_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h))
        assert rc < 0 and not h.value and word in Hh.last_error(), kw
    # the two shape errors are "unsupported", like the over-asked fused form; the rest are invalid arguments
    h = C.c_void_p()
    for kw in (dict(shapes=S1_ISSUE), dict(shapes=((9, 13), (5, 8), (3, 4), (2, 2))), dict(fused_out=_lib.PH_KNOB_ON, num_outs=1)):
        assert lib.ph_neck_plan_create(C.byref(_cfg(**kw)), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h)) == -2, kw
    # a short workspace, a misaligned one, a good one
    cfg = _cfg()
    need = lib.ph_neck_plan_workspace_bytes(C.byref(cfg))
    assert lib.ph_neck_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), need - 256, C.byref(h)) == -4
    assert "workspace too small" in Hh.last_error() and not h.value
    assert lib.ph_neck_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR + 16), need, C.byref(h)) == -1 and "aligned" in Hh.last_error()
    assert lib.ph_neck_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), need, C.byref(h)) == 0 and h.value
    # run-time pointer checks come back before any launch (no GPU in this process' tests: a launch on the fake addresses would fault)
    run = lambda **kw: lib.ph_neck_plan_run(h, C.byref(_io(**kw)), None)
    assert run(feat2=None) == -1 and "level 2" in Hh.last_error()
    assert run(posenc=None) == -1 and "posenc" in Hh.last_error()
    assert run(plane1=None) == -1 and "out_planes[1]" in Hh.last_error()
    assert run(plane0=FAKE_PTR + 4) == -1 and "16-byte" in Hh.last_error()
    assert lib.ph_neck_plan_run_level(h, 4, C.byref(_io()), None) == -1 and "level" in Hh.last_error()
    assert lib.ph_neck_plan_run_level(h, 1, C.byref(_io(feat1=None)), None) == -1 and "level 1" in Hh.last_error()
    assert lib.ph_neck_plan_run_outputs(h, C.byref(_io(plane2=None)), None) == -1 and "out_planes[2]" in Hh.last_error()
    lib.ph_neck_plan_destroy(h)
    cfg = _cfg(pos_level=-1, emit_planes=0, emit_f32=1)
    assert lib.ph_neck_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h)) == 0
    assert run() == -1 and "posenc" in Hh.last_error()                                   # a table without a pos_level
    assert run(posenc=None) == -1 and "out_f32[0]" in Hh.last_error()
    lib.ph_neck_plan_destroy(h)
    # pack arguments
    params = (C.c_void_p * _lib.PH_NECK_NPARAMS)(*([FAKE_PTR] * _lib.PH_NECK_NPARAMS))
    cfg = _cfg(num_outs=2)
    assert lib.ph_neck_pack(C.byref(cfg), params, C.c_void_p(FAKE_PTR + 16), None) == -1 and "aligned" in Hh.last_error()
    params[25] = None
    assert lib.ph_neck_pack(C.byref(cfg), params, C.c_void_p(FAKE_PTR), None) == -1 and "aux_convs.0.gn.weight" in Hh.last_error()
    assert lib.ph_neck_posenc(0, 4, 128, 10000.0, 6.28, 1e-6, C.c_void_p(FAKE_PTR), None) == -1 and "bad size" in Hh.last_error()
    assert lib.ph_neck_posenc(2, 4, 128, 10000.0, 6.28, 1e-6, None, None) == -1 and "null out" in Hh.last_error()


def _io(**kw):
    io = _lib.NeckIO()
    for l in range(4):
        io.feats[l] = kw.get(f"feat{l}", FAKE_PTR)
    io.posenc = kw.get("posenc", FAKE_PTR)
    for i in range(3):
        io.out_planes[i] = kw.get(f"plane{i}", FAKE_PTR)
        io.out_f32[i] = kw.get(f"f32_{i}", None)
    return io


def _geo(cfg):
    """what a plan created from the cfg reports (ph_neck_plan_info) -- and what the query without a plan (ph_neck_geometry_of) says
    of the same cfg, which must be the same struct byte for byte"""
    lib = _lib.load()
    h, g, asked = C.c_void_p(), _lib.NeckGeometry(), _lib.NeckGeometry()
    assert lib.ph_neck_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h)) == 0, Hh.last_error()
    assert lib.ph_neck_plan_info(h, C.byref(g)) == 0
    lib.ph_neck_plan_destroy(h)
    assert lib.ph_neck_geometry_of(C.byref(cfg), C.byref(asked)) == 0, Hh.last_error()
    assert bytes(asked) == bytes(g)
    return g


def test_geometry_of_is_what_a_plan_reports():
    """the cfgs test_bad_cfgs_are_refused_with_a_message creates plans from (every other cfg of this file goes through `_geo`)"""
    for cfg in (_cfg(), _cfg(pos_level=-1, emit_planes=0, emit_f32=1)):
        g = _geo(cfg)
        assert (g.Ho, g.Wo, g.fused_out, g.c16, g.tower_buffers) == (16, 32, 1, 1, 0)


def test_geometry_of_checks_its_arguments():
    """null cfg, null out and every cfg ph_neck_plan_workspace_bytes refuses: the same messages, `out` untouched"""
    lib = _lib.load()
    g = _lib.NeckGeometry()
    assert lib.ph_neck_geometry_of(None, C.byref(g)) == -1 and "ph_neck_geometry_of: null cfg" in Hh.last_error()
    assert lib.ph_neck_geometry_of(C.byref(_cfg()), None) == -1 and "ph_neck_geometry_of: null out" in Hh.last_error()
    for kw, word in BAD:
        assert lib.ph_neck_geometry_of(C.byref(_cfg(**kw)), C.byref(g)) < 0 and word in Hh.last_error(), kw
        assert "ph_neck_geometry_of" in Hh.last_error()
    assert bytes(g) == bytes(_lib.NeckGeometry())


PYR = ((16, 32), (8, 16), (4, 8), (2, 4))


def _asked(B=1, prec="fp16", env=None, monkeypatch=None, **kw):
    """(fused_out, c16, tower_buffers) of ph_neck_geometry_of(native_neck_cfg(..)): what engine.NeckPlan takes as out2, c16, multi"""
    for k in ("PH_NECK_OUT2", "PH_NECK_C16", "PH_NECK_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    cfg = E.native_neck_cfg(B, PYR, kw.pop("groups", 32), prec, **kw)
    g = _lib.NeckGeometry()
    assert _lib.load().ph_neck_geometry_of(C.byref(cfg), C.byref(g)) == 0, Hh.last_error()
    return g.fused_out, g.c16, g.tower_buffers


def test_neck_plan_choices_table(monkeypatch):
    """the choices engine.NeckPlan takes from the library, against a literal table (each row confirmed once against the attributes
    of the Python rule this query replaced)"""
    ask = lambda *a, **kw: _asked(*a, monkeypatch=monkeypatch, **kw)
    for prec in ("fp16", "bf16"):
        for B in (1, 3):
            assert ask(B, prec) == (1, 1, 0), (prec, B)
        for B in (4, 5):
            assert ask(B, prec) == (1, 1, 1), (prec, B)
    for B in (1, 3, 4, 5):
        assert ask(B, "fp32") == (0, 0, int(B >= 4)), B
    for B in (1, 5):
        assert ask(B, num_outs=1)[0] == 0 and ask(B, groups=16)[0] == 0
        assert ask(B, tower_streams=False)[2] == 0 and ask(B, device_type="cpu")[2] == 0
    assert ask(2)[2] == 0 and ask(2, tower_streams="always")[2] == 1
    assert ask(5, env=dict(PH_NECK_OUT2="0")) == (0, 1, 1)
    assert ask(5, env=dict(PH_NECK_C16="0")) == (1, 0, 1)
    assert ask(5, env=dict(PH_NECK_STREAMS="0")) == (1, 1, 0)
    assert ask(2, env=dict(PH_NECK_STREAMS="2")) == (1, 1, 1)


def test_a_refused_pyramid_arrives_from_the_library(monkeypatch):
    """level sizes that are no stride-2 pyramid: native_neck_cfg builds the cfg, the library refuses it -- engine.NeckPlan has no
    check of its own any more"""
    for k in ("PH_NECK_OUT2", "PH_NECK_C16", "PH_NECK_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    cfg = E.native_neck_cfg(2, ((16, 32), (8, 16), (4, 8), (3, 4)), 32, "fp16")
    g = _lib.NeckGeometry()
    assert _lib.load().ph_neck_geometry_of(C.byref(cfg), C.byref(g)) == _lib.PH_EUNSUPPORTED
    assert "stride-2 pyramid" in Hh.last_error()
    with pytest.raises(_lib.PolyheadError, match="stride-2 pyramid"):
        E.NeckPlan(2, ((16, 32), (8, 16), (4, 8), (3, 4)), _lib.PH_PREC_F16, "cpu")


@pytest.mark.parametrize("mode", ["fp16", "bf16", "fp32", "mixed16"])
@pytest.mark.parametrize("groups", [32, 16])
@pytest.mark.parametrize("num_outs", [3, 1])
def test_geometry_rules(mode, groups, num_outs):
    """both sides of each rule: the fused output stage needs three outputs, 32 groups and a one-plane grade; chunk-major planes
    into level 0's conv need a one-plane grade; both can be switched off; ON where AUTO says no is an error"""
    one_plane = mode in ("fp16", "bf16")
    g = _geo(_cfg(mode=_lib.PH_MODE[mode], groups=groups, num_outs=num_outs, tower_buffers=1))
    assert g.fused_out == int(one_plane and groups == 32 and num_outs == 3)
    assert g.c16 == int(one_plane)
    assert (g.Ho, g.Wo, g.HWp, g.P, g.nconvs, g.tower_buffers) == (16, 32, 512, 1 if one_plane else 2, 7 + num_outs, 1)
    assert g.prec == E.KHEAD_PREC.get(mode, _lib.PH_PREC_SPLIT)
    off = _geo(_cfg(mode=_lib.PH_MODE[mode], groups=groups, num_outs=num_outs, fused_out=_lib.PH_KNOB_OFF, c16=_lib.PH_KNOB_OFF))
    assert (off.fused_out, off.c16, off.tower_buffers) == (0, 0, 0)
    if g.fused_out:
        assert _geo(_cfg(mode=_lib.PH_MODE[mode], groups=groups, num_outs=num_outs, fused_out=_lib.PH_KNOB_ON)).fused_out == 1
    else:
        assert _lib.load().ph_neck_plan_workspace_bytes(C.byref(_cfg(mode=_lib.PH_MODE[mode], groups=groups, num_outs=num_outs,
                                                                      fused_out=_lib.PH_KNOB_ON))) == 0


@pytest.mark.parametrize("shapes,B", [(S3, 5), (S3, 64), (((128, 512), (64, 256), (32, 128), (16, 64)), 5),
                                      (((128, 512), (64, 256), (32, 128), (16, 64)), 1), (((15, 287), (8, 144), (4, 72), (2, 36)), 40)])
def test_tile_rows_follow_the_launch_size(shapes, B):
    """tile_rows: 2 for every conv of a split-grade plan; in one-plane grades 4 exactly when the launch has at least 256 four-row
    tiles, B * ceil(Wo / 64) * ceil(Ho / 4) >= 256, with each conv's own output size; 0 beyond nconvs"""
    Ho, Wo = shapes[1]
    sizes = [(Ho, Wo), (Ho, Wo), shapes[2], (Ho, Wo), shapes[3], (2 * shapes[3][0], 2 * shapes[3][1]), (Ho, Wo)] + [(Ho, Wo)] * 3
    for num_outs in (1, 3):
        g = _geo(_cfg(shapes, B=B, mode=_lib.PH_MODE["fp32"], num_outs=num_outs))
        assert list(g.tile_rows) == [2] * (7 + num_outs) + [0] * (3 - num_outs)
        g = _geo(_cfg(shapes, B=B, mode=_lib.PH_MODE["bf16"], num_outs=num_outs))
        want = [4 if B * ((w + 63) // 64) * ((h + 3) // 4) >= 256 else 2 for h, w in sizes[:7 + num_outs]] + [0] * (3 - num_outs)
        assert list(g.tile_rows) == want


def test_native_neck_cfg_maps_the_environment(monkeypatch):
    """the switches NeckPlan reads from the environment reach the native plan as cfg fields"""
    for k in ("PH_NECK_OUT2", "PH_NECK_C16", "PH_NECK_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    c = E.native_neck_cfg(5, S3, 32, "fp16")
    assert (c.fused_out, c.c16, c.tower_buffers, c.mode, c.num_outs, c.pos_level, c.emit_planes, c.emit_f32) == \
        (_lib.PH_KNOB_AUTO, _lib.PH_KNOB_AUTO, 1, _lib.PH_MODE["fp16"], 3, 3, 0, 1)
    assert (list(c.h), list(c.w)) == ([32, 16, 8, 4], [64, 32, 16, 8])
    assert E.native_neck_cfg(2, S3, 32, "fp16").tower_buffers == 0                       # below 4 frames: one stream
    assert E.native_neck_cfg(2, S3, 32, "fp16", tower_streams="always").tower_buffers == 1
    assert E.native_neck_cfg(5, S3, 32, "fp16", tower_streams=False).tower_buffers == 0
    assert E.native_neck_cfg(5, S3, 32, "fp16", device_type="cpu").tower_buffers == 0
    assert E.native_neck_cfg(5, S3, 32, _lib.PH_PREC_SPLIT, to_planes=True, pos_level=None).pos_level == -1
    assert E.native_neck_cfg(5, S3, 32, "fp16", fused_out=False, c16=False).fused_out == _lib.PH_KNOB_OFF
    assert E.native_neck_cfg(5, S3, 32, "fp16", fused_out=True).fused_out == _lib.PH_KNOB_ON
    monkeypatch.setenv("PH_NECK_OUT2", "0")
    monkeypatch.setenv("PH_NECK_C16", "0")
    monkeypatch.setenv("PH_NECK_STREAMS", "0")
    c = E.native_neck_cfg(5, S3, 32, "fp16")
    assert (c.fused_out, c.c16, c.tower_buffers) == (_lib.PH_KNOB_OFF, _lib.PH_KNOB_OFF, 0)
    with pytest.raises(_lib.PolyheadError):
        E.native_neck_cfg(5, S3, 32, "fp16", fused_out=True)
    monkeypatch.setenv("PH_NECK_OUT2", "2")
    with pytest.raises(_lib.PolyheadError):
        E.native_neck_cfg(5, S3, 32, "fp16")
    monkeypatch.setenv("PH_NECK_STREAMS", "2")
    monkeypatch.delenv("PH_NECK_OUT2")
    assert E.native_neck_cfg(1, S3, 32, "fp16").tower_buffers == 1


def test_module_switch_refuses_borrowed_clips():
    m = _neck()
    assert m.native_plan is False and m.use_native_plan() is m and m.native_plan is True
    with pytest.raises(_lib.PolyheadError, match="native neck plan"):
        m.ingest_frames([])
    assert m.use_native_plan(False).native_plan is False
