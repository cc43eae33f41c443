"""Host-side checks of the native association plan (include/polyhead.h ph_track_cfg .. ph_assoc_plan_match): the track head's parameter table, the pack layout and the workspace size against a
Python computation of the same plan, and argument validation.  No GPU: nothing here launches a kernel
(tests/test_gpu_native_assoc.py does)."""
import ctypes as C

import pytest

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E

FAKE_PTR = 1 << 40          # a 256-byte aligned address create() stores and never dereferences
LEVELS = ((16, 32), (8, 16), (4, 8), (2, 4))


def _tcfg(**kw):
    base = dict(num_convs=4, fc_out_channels=1024, embed_channels=256, groups=32, prec=_lib.PH_PREC_SPLIT)
    base.update(kw)
    return _lib.TrackCfg(**base)


def _cfg(B=2, hw=(64, 128), K=24, cap=12, levels=LEVELS, track=None, **kw):
    c = E.native_assoc_cfg(B, hw, K, cap, 8, 11, levels[:4], track if track is not None else _tcfg())
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def al256(n):
    return (n + 255) // 256 * 256


def test_param_table_is_the_track_heads_state_dict():
    lib = _lib.load()
    cfg = _tcfg()
    names = [lib.ph_track_param_name(C.byref(cfg), i).decode() for i in range(16)]
    assert lib.ph_track_param_name(C.byref(cfg), 16) is None and lib.ph_track_param_name(C.byref(cfg), -1) is None
    want = [f"convs.{i}.{leaf}" for i in range(4) for leaf in ("conv.weight", "gn.weight", "gn.bias")] + \
        ["fcs.0.weight", "fcs.0.bias", "fc_embed.weight", "fc_embed.bias"]
    assert names == want
    shapes = {k[len("track_head."):]: v for k, v in Hh.TRACK_HEAD_SHAPES.items()}
    assert set(names) == set(shapes)
    for i, n in enumerate(names):
        assert lib.ph_track_param_numel(C.byref(cfg), i) == int(__import__("math").prod(shapes[n])), n
    assert lib.ph_track_param_numel(C.byref(cfg), 16) < 0
    c2 = _tcfg(num_convs=2, fc_out_channels=64)
    assert [lib.ph_track_param_name(C.byref(c2), i).decode() for i in (5, 6, 9)] == ["convs.1.gn.bias", "fcs.0.weight", "fc_embed.bias"]
    assert lib.ph_track_param_numel(C.byref(c2), 6) == 64 * 12544 and lib.ph_track_param_name(C.byref(c2), 10) is None


@pytest.mark.parametrize("prec,P", [(_lib.PH_PREC_BF16, 1), (_lib.PH_PREC_SPLIT, 2)])
@pytest.mark.parametrize("num_convs,F,Ech", [(4, 1024, 256), (2, 64, 32)])
def test_pack_layout(prec, P, num_convs, F, Ech):
    """offsets 256-byte aligned, in order, non-overlapping, ending at ph_track_pack_bytes; sizes = the tensors `_get_pack` builds"""
    lib = _lib.load()
    cfg = _tcfg(prec=prec, num_convs=num_convs, fc_out_channels=F, embed_channels=Ech)
    lay = _lib.TrackLayout()
    assert lib.ph_track_pack_layout(C.byref(cfg), C.byref(lay)) == 0
    want = [P * 256 * 2304 * 2 if i < num_convs else 0 for i in range(8)] + [1024 if i % 8 < num_convs else 0 for i in range(16)] + \
        [P * F * 12544 * 2, F * 4, P * Ech * F * 2, Ech * 4]
    assert list(lay.bytes) == want
    end = 0
    for i in range(_lib.PH_TPACK_COUNT):
        assert lay.offset[i] % 256 == 0 and lay.offset[i] == end, i
        end = lay.offset[i] + al256(lay.bytes[i])
    assert end == lib.ph_track_pack_bytes(C.byref(cfg))


def _gemm_ws(M, N, K):
    """ph_gemm_rows_splitk's split of (M, N, K), restated"""
    tiles = ((M + 31) // 32) * ((N // 16 + 3) // 4)
    KS, steps = K // 32, 8
    S = (KS + steps - 1) // steps
    while S > 1 and tiles * S > 2048:
        steps *= 2
        S = (KS + steps - 1) // steps
    return S, steps, S * M * N * 4


@pytest.mark.parametrize("B,hw,K,cap,prec", [(1, (64, 128), 24, 12, _lib.PH_PREC_SPLIT), (3, (37, 50), 24, 24, _lib.PH_PREC_BF16),
                                             (8, (128, 256), 120, 100, _lib.PH_PREC_BF16), (2, (64, 128), 24, 1, _lib.PH_PREC_SPLIT)])
def test_workspace_and_geometry_against_a_python_computation(B, hw, K, cap, prec):
    lib = _lib.load()
    F, P = 1024, 2 if prec == _lib.PH_PREC_SPLIT else 1
    cfg = _cfg(B, hw, K, cap, track=_tcfg(prec=prec))
    conv, fc, emb = _gemm_ws(49 * cap, 256, 2304), _gemm_ws(cap, F, 12544), _gemm_ws(cap, 256, F)
    for (M, N, Kk), w in (((49 * cap, 256, 2304), conv), ((cap, F, 12544), fc), ((cap, 256, F), emb)):
        assert lib.ph_gemm_rows_workspace_bytes(M, N, Kk) == w[2]
    planes = P * B * cap * 49 * 256 * 2
    pieces = [B * lib.ph_segment_boxes_workspace_bytes(K), B * K * 5 * 4, B * K * 4 * 4, B * (K + 1), B * (K + 1) * 8, planes, planes, planes,
              B * cap * 49 * 256 * 4, P * B * cap * F * 2, B * max(conv[2], fc[2], emb[2])]
    assert lib.ph_segment_boxes_workspace_bytes(K) == K * (3 * 8 + 4 * 4 + 2 * 8)
    assert lib.ph_assoc_plan_workspace_bytes(C.byref(cfg)) == sum(al256(p) for p in pieces)
    h, g = C.c_void_p(), _lib.AssocGeometry()
    assert lib.ph_assoc_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h)) == 0, Hh.last_error()
    assert lib.ph_assoc_plan_info(h, C.byref(g)) == 0
    lib.ph_assoc_plan_destroy(h)
    assert (g.things_words, g.P, g.vec8) == (2 + 7 * cap, P, int(hw[1] % 8 == 0))
    assert (g.conv_splits, g.conv_steps, g.fc_splits, g.fc_steps, g.emb_splits, g.emb_steps) == conv[:2] + fc[:2] + emb[:2]
    assert g.staging_bytes == al256(B * (2 + 7 * cap) * 4) + B * (K + 1) * 8


def test_the_split_does_not_depend_on_the_batch():
    lib = _lib.load()
    geos = []
    for B in (1, 3, 8):
        h, g = C.c_void_p(), _lib.AssocGeometry()
        assert lib.ph_assoc_plan_create(C.byref(_cfg(B=B)), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h)) == 0
        lib.ph_assoc_plan_info(h, C.byref(g))
        lib.ph_assoc_plan_destroy(h)
        geos.append((g.conv_splits, g.conv_steps, g.fc_splits, g.fc_steps, g.emb_splits, g.emb_steps))
    assert geos[0] == geos[1] == geos[2]


def test_bad_cfgs_are_refused_before_any_launch():
    lib = _lib.load()
    bad = [(dict(cap=25), "max_things", -1), (dict(cap=0), "max_things", -1), (dict(nlev=0), "nlev", -1), (dict(nlev=5), "nlev", -1),
           (dict(track=_tcfg(prec=_lib.PH_PREC_F16)), "prec", -1), (dict(track=_tcfg(prec=0)), "prec", -1),
           (dict(track=_tcfg(fc_out_channels=1000)), "fc_out_channels", -1), (dict(track=_tcfg(fc_out_channels=1040)), "fc_out_channels", -2),
           (dict(track=_tcfg(embed_channels=128)), "embed_channels", -2), (dict(track=_tcfg(num_convs=9)), "num_convs", -1),
           (dict(track=_tcfg(groups=48)), "groups", -1), (dict(B=0), "B, Ho, Wo, K", -1), (dict(K=2000, cap=10), "K must be", -2),
           (dict(num_stuff_classes=250), "void", -1), (dict(finest_scale=0.0), "finest_scale", -1)]
    for kw, word, code in bad:
        cfg = _cfg(**kw)
        assert lib.ph_assoc_plan_workspace_bytes(C.byref(cfg)) == 0 and word in Hh.last_error(), (kw, Hh.last_error())
        h = C.c_void_p()
        rc = lib.ph_assoc_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h))
        assert rc == code and not h.value and word in Hh.last_error(), (kw, rc, Hh.last_error())
    for kw in (dict(prec=_lib.PH_PREC_F16), dict(fc_out_channels=1000), dict(num_convs=0)):
        assert lib.ph_track_pack_bytes(C.byref(_tcfg(**kw))) == 0, kw
    # a short workspace, a misaligned one, a good one
    cfg, h = _cfg(), C.c_void_p()
    need = lib.ph_assoc_plan_workspace_bytes(C.byref(cfg))
    assert lib.ph_assoc_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), need - 256, C.byref(h)) == -4
    assert "workspace too small" in Hh.last_error() and not h.value
    assert lib.ph_assoc_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR + 16), need, C.byref(h)) == -1 and "aligned" in Hh.last_error()
    assert lib.ph_assoc_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), need, C.byref(h)) == 0 and h.value
    # run-time pointer checks come back before any launch (a launch on the fake addresses would fault)
    def io(**kw):
        o = _lib.AssocIO()
        for k in ("pan", "seg_records", "sem_out", "things_out", "embeds_out"):
            setattr(o, k, kw.get(k, FAKE_PTR))
        for l in range(4):
            o.levels[l] = kw.get(f"level{l}", FAKE_PTR)
            o.level_stride[l] = kw.get(f"stride{l}", 256 * LEVELS[l][0] * LEVELS[l][1])
        return o
    run = lambda **kw: lib.ph_assoc_plan_run(h, C.byref(io(**kw)), None)
    assert run(pan=None) == -1 and "pan" in Hh.last_error()
    assert run(embeds_out=None) == -1 and "embeds_out" in Hh.last_error()
    assert run(level2=None) == -1 and "level 2" in Hh.last_error()
    assert run(stride1=7) == -1 and "level_stride[1]" in Hh.last_error()
    assert run(pan=FAKE_PTR + 4) == -1 and "16-byte" in Hh.last_error()
    stage = C.create_string_buffer(64)
    m = lib.ph_assoc_plan_match(h, C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), stage, 64, 1,
                                C.c_void_p(FAKE_PTR), None, None)
    assert m == -4 and "staging" in Hh.last_error()
    assert lib.ph_assoc_plan_match(h, None, C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), stage, 1 << 30, 1,
                                   C.c_void_p(FAKE_PTR), None, None) == -1
    lib.ph_assoc_plan_destroy(h)
    # pack arguments
    params = (C.c_void_p * 16)(*([FAKE_PTR] * 16))
    assert lib.ph_track_pack(C.byref(_tcfg()), params, C.c_void_p(FAKE_PTR + 16), None) == -1 and "aligned" in Hh.last_error()
    params[13] = None
    assert lib.ph_track_pack(C.byref(_tcfg()), params, C.c_void_p(FAKE_PTR), None) == -1 and "fcs.0.bias" in Hh.last_error()


def test_module_switch_is_off_by_default():
    from polyphonicformer_amd import video as V
    a = V.VideoAssociator.__new__(V.VideoAssociator)
    assert a.native_plan is False
    with pytest.raises(_lib.PolyheadError, match="use_native_plan"):
        a.step_records(None, None, None)
    assert a.use_native_plan(True, max_things=12) is a and a.native_plan is True and a.max_things == 12
    assert a.use_native_plan(False).native_plan is False
