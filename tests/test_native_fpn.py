"""CPU: the host side of the native FPN plan (include/polyhead.h ph_fpn_cfg .. ph_fpn_geometry_of) and of the neck plan's level
inputs (ph_neck_plan_level_input): every cfg error before any device is touched, the pack layout against the header's formulas, the
parameter table against the reference's state_dict keys, and the level-input addresses of a plan created over memory it never
dereferences."""
import ctypes as C

import pytest

import helpers as Hh
from polyphonicformer_amd import _lib

FAKE_PTR = 1 << 40          # a 256-byte aligned address create() stores and never dereferences
PYR = ((16, 32), (8, 16), (4, 8), (2, 4))
ODD = ((15, 23), (8, 12), (4, 6), (2, 3))
CH = (64, 128, 256, 320)
# the reference's FPN.state_dict() keys, in its order (mmdet/models/necks/fpn.py: lateral_convs, then fpn_convs; ConvModule.conv)
KEYS = [f"{g}.{i}.conv.{p}" for g in ("lateral_convs", "fpn_convs") for i in range(4) for p in ("weight", "bias")]


def _cfg(B=2, shapes=PYR, k=CH, mode="bf16", x_dtype=_lib.PH_OUT_F32, emit_f32=1, emit_planes=0):
    i4 = lambda xs: (C.c_int32 * 4)(*xs)
    return _lib.FpnCfg(B=B, k=i4(k), h=i4([s[0] for s in shapes]), w=i4([s[1] for s in shapes]),
                       mode=mode if isinstance(mode, int) else _lib.PH_MODE[mode], x_dtype=x_dtype, emit_f32=emit_f32, emit_planes=emit_planes)


def _refused(cfg, code, word):
    lib = _lib.load()
    geo = _lib.FpnGeometry()
    assert lib.ph_fpn_geometry_of(C.byref(cfg), C.byref(geo)) == code
    assert "ph_fpn_geometry_of" in Hh.last_error() and word in Hh.last_error(), Hh.last_error()
    assert lib.ph_fpn_plan_workspace_bytes(C.byref(cfg)) == 0 and "ph_fpn_plan_workspace_bytes" in Hh.last_error()
    assert lib.ph_fpn_pack_bytes(C.byref(cfg)) == 0
    h = C.c_void_p()
    assert lib.ph_fpn_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h)) == code and not h.value


@pytest.mark.parametrize("k", [(32, 128, 256, 320), (64, 128, 224, 320), (64, 128, 256, 4160), (64, 0, 256, 320)])
def test_bad_stage_channels(k):
    _refused(_cfg(k=k), _lib.PH_EINVAL, "multiple of 64")


@pytest.mark.parametrize("shapes", [((16, 32), (8, 16), (4, 8), (1, 4)),        # H = 4 Hc
                                    ((16, 33), (8, 16), (4, 8), (2, 4)),        # W = 2 Wc + 1
                                    ((16, 32), (8, 16), (5, 8), (2, 4)),        # level 1 is 2 Hc - 2; level 2 is 2 Hc + 1
                                    ((14, 32), (8, 16), (4, 8), (2, 4))])       # H = 2 Hc - 2
def test_size_pairs_outside_the_nearest_rule(shapes):
    _refused(_cfg(shapes=shapes), _lib.PH_EUNSUPPORTED, "2 n")


def test_other_cfg_errors():
    _refused(_cfg(emit_f32=0, emit_planes=0), _lib.PH_EINVAL, "emit")
    _refused(_cfg(mode=17), _lib.PH_EINVAL, "mode")
    _refused(_cfg(mode=-1), _lib.PH_EINVAL, "mode")
    _refused(_cfg(x_dtype=3), _lib.PH_EINVAL, "x_dtype")
    _refused(_cfg(B=0), _lib.PH_EINVAL, "B")
    _refused(_cfg(B=4097), _lib.PH_EUNSUPPORTED, "4096")
    _refused(_cfg(shapes=((16, 32), (8, 16), (4, 8), (2, 0))), _lib.PH_EINVAL, "h, w")
    lib = _lib.load()
    assert lib.ph_fpn_geometry_of(None, C.byref(_lib.FpnGeometry())) == _lib.PH_EINVAL
    assert lib.ph_fpn_geometry_of(C.byref(_cfg()), None) == _lib.PH_EINVAL


@pytest.mark.parametrize("shapes", [PYR, ODD, ((1, 1), (1, 1), (1, 1), (1, 1))])
def test_every_stride_2_pyramid_is_accepted(shapes):
    lib = _lib.load()
    geo = _lib.FpnGeometry()
    for mode, P, prec in (("bf16", 1, _lib.PH_PREC_BF16), ("fp16", 1, _lib.PH_PREC_F16), ("fp32", 2, _lib.PH_PREC_SPLIT),
                          ("mixed", 2, _lib.PH_PREC_SPLIT), ("mixed16", 2, _lib.PH_PREC_SPLIT)):
        assert lib.ph_fpn_geometry_of(C.byref(_cfg(shapes=shapes, mode=mode)), C.byref(geo)) == 0, Hh.last_error()
        assert (geo.P, geo.prec) == (P, prec) and all(t in (2, 4) for t in geo.tile_rows)


@pytest.mark.parametrize("mode,P", [("bf16", 1), ("fp16", 1), ("fp32", 2)])
@pytest.mark.parametrize("k", [CH, (256, 512, 1024, 2048), (4096, 64, 64, 4096)])
def test_pack_layout(mode, P, k):
    """offsets 256-byte aligned, ascending, non-overlapping, ending at ph_fpn_pack_bytes; sizes from the formulas of the header"""
    lib = _lib.load()
    cfg = _cfg(k=k, mode=mode)
    lay = _lib.FpnLayout()
    assert lib.ph_fpn_pack_layout(C.byref(cfg), C.byref(lay)) == 0
    want = []
    for l in range(4):
        want += [P * 256 * k[l] * 2, 256 * 4]
    for l in range(4):
        want += [P * 256 * 2304 * 2, 256 * 4]
    assert list(lay.bytes) == want
    end = 0
    for i in range(_lib.PH_FPACK_COUNT):
        assert lay.offset[i] % 256 == 0 and lay.offset[i] == end, i
        end = lay.offset[i] + (lay.bytes[i] + 255) // 256 * 256
    assert end == lib.ph_fpn_pack_bytes(C.byref(cfg))
    assert lib.ph_fpn_pack_layout(C.byref(cfg), None) == _lib.PH_EINVAL
    # the pack call's own checks come before any launch: a NULL parameter, a misaligned pack
    params = (C.c_void_p * 16)(*([FAKE_PTR] * 16))
    assert lib.ph_fpn_pack(C.byref(cfg), params, C.c_void_p(FAKE_PTR + 16), None) == _lib.PH_EINVAL and "aligned" in Hh.last_error()
    params[9] = None
    assert lib.ph_fpn_pack(C.byref(cfg), params, C.c_void_p(FAKE_PTR), None) == _lib.PH_EINVAL and "fpn_convs.0.conv.bias" in Hh.last_error()


def test_parameter_table_is_the_reference_state_dict():
    lib = _lib.load()
    assert _lib.PH_FPN_NPARAMS == 16
    assert [lib.ph_fpn_param_name(i).decode() for i in range(16)] == KEYS
    assert lib.ph_fpn_param_name(-1) is None and lib.ph_fpn_param_name(16) is None
    cfg = _cfg()
    numel = [lib.ph_fpn_param_numel(C.byref(cfg), i) for i in range(16)]
    assert numel == [n for l in range(4) for n in (256 * CH[l], 256)] + [256 * 256 * 9, 256] * 4
    assert lib.ph_fpn_param_numel(C.byref(cfg), 16) < 0 and lib.ph_fpn_param_numel(None, 0) < 0
    assert lib.ph_fpn_param_numel(C.byref(_cfg(k=(96, 128, 256, 320))), 0) < 0
    # this package's module carries the same keys
    from polyphonicformer_amd.registry import NECKS
    import polyphonicformer_amd.fpn  # noqa: F401
    m = NECKS.build(dict(type="FPN", in_channels=list(CH), out_channels=256, num_outs=4))
    assert list(m.state_dict().keys()) == KEYS
    assert [v.numel() for v in m.state_dict().values()] == numel


def test_plan_create_checks_its_buffers():
    lib = _lib.load()
    cfg = _cfg(emit_planes=1)
    need = lib.ph_fpn_plan_workspace_bytes(C.byref(cfg))
    # four lateral sums (16-bit), one fp32 conv output of the largest level, the conv's partial sums
    B, hw = 2, [h * w for h, w in PYR]
    assert need == sum(B * n * 256 * 2 for n in hw) + B * hw[0] * 256 * 4 + 4 * max(lib.ph_conv_nhwc_partial_floats(B, h, w) for h, w in PYR)
    h = C.c_void_p()
    assert lib.ph_fpn_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), need - 256, C.byref(h)) == _lib.PH_EWORKSPACE
    assert not h.value
    assert lib.ph_fpn_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR + 16), need, C.byref(h)) == -1 and "aligned" in Hh.last_error()
    assert lib.ph_fpn_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR + 16), C.c_void_p(FAKE_PTR), need, C.byref(h)) == -1 and "aligned" in Hh.last_error()
    assert lib.ph_fpn_plan_create(C.byref(cfg), None, C.c_void_p(FAKE_PTR), need, C.byref(h)) == -1
    assert lib.ph_fpn_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), need, C.byref(h)) == 0 and h.value
    geo, geo2 = _lib.FpnGeometry(), _lib.FpnGeometry()
    assert lib.ph_fpn_plan_info(h, C.byref(geo)) == 0 and lib.ph_fpn_geometry_of(C.byref(cfg), C.byref(geo2)) == 0
    assert bytes(geo) == bytes(geo2)
    # the run calls refuse a bad io before any launch (nothing of these addresses is touched)
    io = _lib.FpnIO()
    assert lib.ph_fpn_plan_run(h, C.byref(io), None) == -1 and "stage 0" in Hh.last_error()
    assert lib.ph_fpn_plan_run_laterals(h, C.byref(io), None) == -1
    assert lib.ph_fpn_plan_run_output(h, 4, C.byref(io), None) == -1 and "level" in Hh.last_error()
    assert lib.ph_fpn_plan_run_output(h, 1, C.byref(io), None) == -1 and "out_f32[1]" in Hh.last_error()
    io.out_f32[1] = FAKE_PTR
    assert lib.ph_fpn_plan_run_output(h, 1, C.byref(io), None) == -1 and "out_planes[1]" in Hh.last_error()
    io.out_planes[1] = FAKE_PTR + 8
    assert lib.ph_fpn_plan_run_output(h, 1, C.byref(io), None) == -1 and "16-byte" in Hh.last_error()
    io.out_planes[1], io.planes_layout[1] = FAKE_PTR, 7
    assert lib.ph_fpn_plan_run_output(h, 1, C.byref(io), None) == -1 and "planes_layout[1]" in Hh.last_error()
    assert lib.ph_fpn_plan_run(None, C.byref(io), None) == -1 and lib.ph_fpn_plan_run(h, None, None) == -1
    lib.ph_fpn_plan_destroy(h)
    lib.ph_fpn_plan_destroy(None)
    # chunk-major planes need a one-plane grade
    cfg = _cfg(mode="fp32", emit_planes=1)
    assert lib.ph_fpn_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), 1 << 62, C.byref(h)) == 0
    io = _lib.FpnIO()
    io.out_f32[0], io.out_planes[0], io.planes_layout[0] = FAKE_PTR, FAKE_PTR, _lib.PH_PLANES_C16
    assert lib.ph_fpn_plan_run_output(h, 0, C.byref(io), None) == -1 and "one-plane" in Hh.last_error()
    lib.ph_fpn_plan_destroy(h)


@pytest.mark.parametrize("mode,tb", [("bf16", 0), ("fp16", 1), ("fp32", 0), ("fp32", 1)])
def test_neck_plan_level_inputs(mode, tb):
    """ph_neck_plan_create touches no device memory: a plan over an address it never dereferences answers where its level inputs
    lie -- one shared buffer, or four disjoint ones inside the workspace -- and which `prec` their writer passes"""
    lib = _lib.load()
    B = 2
    i4 = lambda xs: (C.c_int32 * 4)(*xs)
    cfg = _lib.NeckCfg(B=B, h=i4([s[0] for s in ODD]), w=i4([s[1] for s in ODD]), groups=32, mode=_lib.PH_MODE[mode], num_outs=3,
                       pos_level=3, emit_planes=1, tower_buffers=tb)
    need = lib.ph_neck_plan_workspace_bytes(C.byref(cfg))
    h = C.c_void_p()
    assert lib.ph_neck_plan_create(C.byref(cfg), C.c_void_p(FAKE_PTR), C.c_void_p(FAKE_PTR), need, C.byref(h)) == 0, Hh.last_error()
    geo = _lib.NeckGeometry()
    lib.ph_neck_plan_info(h, C.byref(geo))
    assert geo.tower_buffers == tb and geo.c16 == (0 if mode == "fp32" else 1)
    got = []
    for l in range(4):
        p, pl = C.c_void_p(), C.c_int32(-1)
        assert lib.ph_neck_plan_level_input(h, l, C.byref(p), C.byref(pl)) == 0
        assert pl.value == geo.prec | (_lib.PH_PLANES_C16 if (l == 0 and geo.c16) else 0)
        assert p.value % 256 == 0
        got.append((p.value - FAKE_PTR, geo.P * B * ODD[l][0] * ODD[l][1] * 256 * 2))
    if tb:
        spans = sorted(got)
        for (a, n), (b, _) in zip(spans, spans[1:]):
            assert a + n <= b
    else:
        assert len({a for a, _ in got}) == 1
    assert all(0 <= a and a + n <= need for a, n in got)
    p, pl = C.c_void_p(), C.c_int32()
    assert lib.ph_neck_plan_level_input(h, 4, C.byref(p), C.byref(pl)) == -1 and "level" in Hh.last_error()
    assert lib.ph_neck_plan_level_input(h, -1, C.byref(p), C.byref(pl)) == -1
    assert lib.ph_neck_plan_level_input(None, 0, C.byref(p), C.byref(pl)) == -1
    assert lib.ph_neck_plan_level_input(h, 0, None, C.byref(pl)) == -1
    assert lib.ph_neck_plan_run_level_planes(h, 4, None) == -1 and lib.ph_neck_plan_run_level_planes(None, 0, None) == -1
    lib.ph_neck_plan_destroy(h)
