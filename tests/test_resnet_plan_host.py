"""CPU: the native backbone plan's host side (include/polyhead.h ph_resnet_nparams .. ph_resnet_geometry_of): the parameter table
against resnet.ResNet's state_dict, the pack layout against the shapes of ResNet._pack's tensors, the geometry against
engine.ResNetPlan's block-table arithmetic and the library's own workgroup queries, and every refusal from every size query."""
import ctypes as C

import pytest

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
import polyphonicformer_amd.resnet as RN

NPARAMS = {50: 265, 101: 520, 152: 775}
SIZES = [(1, 40, 72), (2, 64, 128), (1, 1024, 2048)]


def _cfg(B=1, H=40, W=72, depth=50, prec="bf16", **kw):
    return E.native_resnet_cfg(B, H, W, depth, prec, **kw)


@pytest.mark.parametrize("depth", [50, 101, 152])
def test_parameter_table_is_the_state_dict(depth):
    lib, cfg = _lib.load(), _cfg(depth=depth)
    sd = RN.ResNet(depth).state_dict()
    keys = [k for k in sd if not k.endswith("num_batches_tracked")]
    n = lib.ph_resnet_nparams(C.byref(cfg))
    assert n == NPARAMS[depth] == len(keys)
    assert [lib.ph_resnet_param_name(C.byref(cfg), i).decode() for i in range(n)] == keys
    assert [lib.ph_resnet_param_numel(C.byref(cfg), i) for i in range(n)] == [sd[k].numel() for k in keys]
    for i in (-1, n):
        assert lib.ph_resnet_param_name(C.byref(cfg), i) is None and lib.ph_resnet_param_numel(C.byref(cfg), i) < 0
    bad = _cfg(depth=34)
    assert lib.ph_resnet_nparams(C.byref(bad)) < 0 and lib.ph_resnet_param_name(C.byref(bad), 0) is None
    assert lib.ph_resnet_param_numel(C.byref(bad), 0) < 0


def _convs(depth):
    """(cout, K of the packed matrix) per convolution in state_dict order, from the module's shapes alone"""
    m = RN.ResNet(depth)
    out = [(64, RN.STEM_K)]
    for name in m.res_layers:
        for b in getattr(m, name):
            for conv in (b.conv1, b.conv2, b.conv3) + ((b.downsample[0],) if b.downsample is not None else ()):
                co, ci, kh, kw = conv.weight.shape
                out.append((co, ci * kh * kw))
    return out


@pytest.mark.parametrize("depth", [50, 101, 152])
def test_pack_layout(depth):
    lib, cfg = _lib.load(), _cfg(depth=depth)
    lay = _lib.ResNetLayout()
    assert lib.ph_resnet_pack_layout(C.byref(cfg), C.byref(lay)) == 0
    convs = _convs(depth)
    assert lay.nconvs == len(convs) == NPARAMS[depth] // 5 <= _lib.PH_RESNET_MAX_CONVS
    end = 0
    for c, (cout, K) in enumerate(convs):
        assert cout % 32 == 0                                         # pack_b32 takes no other; the layout rule pads the rows to 32
        for piece, nbytes in ((2 * c, cout * K * 2), (2 * c + 1, cout * 4)):
            assert lay.offset[piece] % 256 == 0 and lay.offset[piece] >= end and lay.bytes[piece] == nbytes, (c, piece)
            end = lay.offset[piece] + lay.bytes[piece]
    assert all(v == 0 for v in list(lay.offset)[2 * lay.nconvs:] + list(lay.bytes)[2 * lay.nconvs:])
    assert lib.ph_resnet_pack_bytes(C.byref(cfg)) == (end + 255) // 256 * 256
    # the layout depends on the depth alone
    other = _lib.ResNetLayout()
    assert lib.ph_resnet_pack_layout(C.byref(_cfg(2, 64, 128, depth, "fp16")), C.byref(other)) == 0 and bytes(other) == bytes(lay)


def _expected(B, H, W, depth, out_indices):
    """(stage shapes, launches in order as (name, workgroups)) by engine.ResNetPlan's arithmetic and the library's workgroup queries"""
    lib = _lib.load()
    h, w = E.stem_out_size(H), E.stem_out_size(W)
    launches, shapes = [("stem", lib.ph_resnet_stem_workgroups(H, W, B))], []
    for si, stage in enumerate(RN.ResNet(depth).block_table()):
        run = si <= max(out_indices)
        for cin, planes, s, has_down in stage:
            ho, wo = E.conv_out_size(h, 3, s), E.conv_out_size(w, 3, s)
            order = [(1, 1, cin, planes, h, w), (3, s, planes, planes, h, w)] + ([(1, s, cin, 4 * planes, h, w)] if has_down else []) + \
                [(1, 1, planes, 4 * planes, ho, wo)]
            if run:
                launches += [("conv", lib.ph_conv_cl_workgroups(k, st, ci, co, hh, ww, B)) for k, st, ci, co, hh, ww in order]
            h, w = ho, wo
        shapes.append((4 * stage[-1][1], h, w))
        if si in out_indices:
            launches.append(("nchw", lib.ph_cl_to_nchw_workgroups(B, h * w, shapes[-1][0])))
    return shapes, launches


@pytest.mark.parametrize("B,H,W", SIZES)
@pytest.mark.parametrize("depth,out_indices", [(50, (0, 1, 2, 3)), (50, (0, 1)), (50, (1, 3)), (101, (0, 1, 2, 3))])
def test_geometry(B, H, W, depth, out_indices):
    lib = _lib.load()
    cfg = _cfg(B, H, W, depth, "fp16", out_indices=out_indices)
    geo = _lib.ResNetGeometry()
    assert lib.ph_resnet_geometry_of(C.byref(cfg), C.byref(geo)) == 0, Hh.last_error()
    shapes, launches = _expected(B, H, W, depth, out_indices)
    assert [(geo.c[i], geo.h[i], geo.w[i]) for i in range(4)] == shapes
    assert all(n > 0 for _, n in launches)
    assert geo.prec == _lib.PH_PREC_F16 and geo.launches == len(launches)
    assert geo.stem_workgroups == launches[0][1]
    convs = [n for kind, n in launches if kind == "conv"]
    assert geo.nconvs == len(convs) and list(geo.conv_workgroups)[:len(convs)] == convs
    assert not any(list(geo.conv_workgroups)[len(convs):])
    nchw = iter(n for kind, n in launches if kind == "nchw")
    assert list(geo.nchw_workgroups) == [next(nchw) if i in out_indices else 0 for i in range(4)]
    if depth == 50 and out_indices == (0, 1, 2, 3):
        assert geo.launches == 57 and geo.nconvs == 52
    if out_indices == (0, 1):                                           # the list stops after layer2
        assert geo.nconvs == 3 * 3 + 1 + 3 * 4 + 1 and geo.launches == 1 + geo.nconvs + 2
    # the workspace holds engine.ResNetPlan's six planes
    h0, w0 = E.stem_out_size(H), E.stem_out_size(W)
    io = inner = down = 0
    h, w = h0, w0
    for stage in RN.ResNet(depth).block_table():
        for cin, planes, s, has_down in stage:
            ho, wo = E.conv_out_size(h, 3, s), E.conv_out_size(w, 3, s)
            inner, io = max(inner, h * w * planes, ho * wo * planes), max(io, ho * wo * 4 * planes)
            down = max(down, ho * wo * 4 * planes) if has_down else down
            h, w = ho, wo
    al = lambda n: (B * n * 2 + 255) // 256 * 256
    assert lib.ph_resnet_plan_workspace_bytes(C.byref(cfg)) == al(h0 * w0 * 64) + 2 * al(io) + 2 * al(inner) + al(max(down, 8))


REFUSALS = [
    ("depth", dict(depth=34), _lib.PH_EUNSUPPORTED),
    ("mode", dict(prec="fp32"), _lib.PH_EUNSUPPORTED),
    ("out_mask", dict(out_mask=0), _lib.PH_EINVAL),
    ("out_mask", dict(out_mask=16), _lib.PH_EINVAL),
    ("x_dtype", dict(x_dtype=_lib.PH_OUT_F16), _lib.PH_EINVAL),
    ("out_dtype", dict(out_dtype=7), _lib.PH_EINVAL),
    ("B", dict(B=0), _lib.PH_EINVAL),
    ("B", dict(B=4097), _lib.PH_EUNSUPPORTED),
    ("H", dict(H=32769), _lib.PH_EINVAL),                               # ph_resnet_stem's limit
    ("W", dict(W=0), _lib.PH_EINVAL),
    ("eps", dict(eps=-1.0), _lib.PH_EINVAL),
]


@pytest.mark.parametrize("field,change,code", REFUSALS, ids=[f"{f}-{list(c.values())[0]}" for f, c, _ in REFUSALS])
def test_refusals_come_from_every_query(field, change, code):
    lib = _lib.load()
    change = dict(change)
    cfg = _cfg(depth=change.pop("depth", 50), prec=change.pop("prec", "bf16"))
    for k, v in change.items():
        setattr(cfg, k, v)
    geo, lay, h = _lib.ResNetGeometry(), _lib.ResNetLayout(), C.c_void_p()
    buf = (C.c_char * 1024)()
    aligned = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)         # host memory: a refused create touches nothing
    calls = [("ph_resnet_geometry_of", lambda: lib.ph_resnet_geometry_of(C.byref(cfg), C.byref(geo)), code),
             ("ph_resnet_pack_layout", lambda: lib.ph_resnet_pack_layout(C.byref(cfg), C.byref(lay)), code),
             ("ph_resnet_pack_bytes", lambda: lib.ph_resnet_pack_bytes(C.byref(cfg)), 0),
             ("ph_resnet_plan_workspace_bytes", lambda: lib.ph_resnet_plan_workspace_bytes(C.byref(cfg)), 0),
             ("ph_resnet_plan_create", lambda: lib.ph_resnet_plan_create(C.byref(cfg), aligned, aligned, 1 << 40, C.byref(h)), code),
             ("ph_resnet_pack", lambda: lib.ph_resnet_pack(C.byref(cfg), (C.c_void_p * 775)(), aligned, None), code)]
    for name, call, want in calls:
        assert call() == want, name
        msg = Hh.last_error()
        assert msg.startswith(name + ":") and field in msg, (name, msg)
    assert not h.value


def test_null_pointers_are_refused():
    lib, cfg = _lib.load(), _cfg()
    geo, lay, h = _lib.ResNetGeometry(), _lib.ResNetLayout(), C.c_void_p()
    buf = (C.c_char * 1024)()
    aligned = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)
    nws = lib.ph_resnet_plan_workspace_bytes(C.byref(cfg))
    assert nws > 0
    for name, call in [("ph_resnet_geometry_of", lambda: lib.ph_resnet_geometry_of(None, C.byref(geo))),
                       ("ph_resnet_geometry_of", lambda: lib.ph_resnet_geometry_of(C.byref(cfg), None)),
                       ("ph_resnet_pack_layout", lambda: lib.ph_resnet_pack_layout(C.byref(cfg), None)),
                       ("ph_resnet_plan_info", lambda: lib.ph_resnet_plan_info(None, C.byref(geo))),
                       ("ph_resnet_plan_create", lambda: lib.ph_resnet_plan_create(C.byref(cfg), None, aligned, nws, C.byref(h))),
                       ("ph_resnet_plan_create", lambda: lib.ph_resnet_plan_create(C.byref(cfg), aligned, None, nws, C.byref(h))),
                       ("ph_resnet_plan_create", lambda: lib.ph_resnet_plan_create(C.byref(cfg), aligned, aligned, nws, None)),
                       ("ph_resnet_pack", lambda: lib.ph_resnet_pack(C.byref(cfg), None, aligned, None)),
                       ("ph_resnet_pack", lambda: lib.ph_resnet_pack(C.byref(cfg), (C.c_void_p * 265)(), aligned, None)),
                       ("ph_resnet_plan_run", lambda: lib.ph_resnet_plan_run(None, C.byref(_lib.ResNetIO()), None))]:
        assert call() == _lib.PH_EINVAL, name
        assert Hh.last_error().startswith(name + ":") and ("null" in Hh.last_error() or "NULL" in Hh.last_error()), Hh.last_error()
    assert lib.ph_resnet_pack_bytes(None) == 0 and lib.ph_resnet_plan_workspace_bytes(None) == 0
    # a plan over host memory: create touches none of it, and the run calls check their pointers before the first launch
    assert lib.ph_resnet_plan_create(C.byref(cfg), aligned, aligned, nws - 1, C.byref(h)) == _lib.PH_EWORKSPACE and not h.value
    assert lib.ph_resnet_plan_create(C.byref(cfg), aligned, aligned, nws, C.byref(h)) == 0 and h.value
    assert bytes(buf) == bytes(1024)
    io = _lib.ResNetIO()
    assert lib.ph_resnet_plan_run(h, C.byref(io), None) == _lib.PH_EINVAL and "image" in Hh.last_error()
    assert lib.ph_resnet_plan_run_stem(h, C.byref(io), None) == _lib.PH_EINVAL and "image" in Hh.last_error()
    assert lib.ph_resnet_plan_run_stage(h, 2, C.byref(io), None) == _lib.PH_EINVAL and "stages[2]" in Hh.last_error()
    assert lib.ph_resnet_plan_run_stage(h, 4, C.byref(io), None) == _lib.PH_EINVAL
    io.image = 4096
    assert lib.ph_resnet_plan_run(h, C.byref(io), None) == _lib.PH_EINVAL and "stages[0]" in Hh.last_error()
    got = _lib.ResNetGeometry()
    assert lib.ph_resnet_plan_info(h, C.byref(got)) == 0 and lib.ph_resnet_geometry_of(C.byref(cfg), C.byref(geo)) == 0
    assert bytes(got) == bytes(geo)
    lib.ph_resnet_plan_destroy(h)
