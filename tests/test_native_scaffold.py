"""The host scaffold the native plan families share (csrc/ph_plan_inl.h; engine._NativePack / _NativePlan), family by family: what
every pack / workspace / create / geometry / info entry point answers to a NULL cfg and to NULL or misplaced buffers -- return codes,
`*out` and the entry point's own name at the start of the message -- and, on the Python side, that a refused cfg surfaces as a
PolyheadError with the library's words and that a dropped plan destroys each of its handles once.  No GPU: every call here returns
before its first launch (a launch on this file's fake addresses would answer PH_ELAUNCH, never the codes asserted), and create
stores pointers it never dereferences.  The one row that needs the device's CU count carries the gpu marker."""
import ctypes as C
import gc
import types

import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E

FAKE = 1 << 40              # a 256-byte aligned address nothing dereferences
I4 = lambda xs: (C.c_int32 * 4)(*xs)
PYR = ((8, 16), (4, 8), (2, 4), (1, 2))


def _track_cfg():
    return _lib.TrackCfg(num_convs=1, fc_out_channels=32, embed_channels=256, groups=32, prec=_lib.PH_PREC_BF16)


def _assoc_cfg():
    c = _lib.AssocCfg(B=1, Ho=8, Wo=8, K=2, max_things=1, num_thing_classes=1, num_stuff_classes=1, nlev=1, finest_scale=56.0)
    c.h[0], c.w[0], c.inv_stride[0] = 2, 2, 0.25
    c.track = _track_cfg()
    return c


class Fam(types.SimpleNamespace):
    """one family: its smallest valid cfg and the names of its entry points (None: the family has none of that kind)"""

    def __init__(self, name, cfg, **kw):
        base = dict(pack_bytes=None, pack_layout=None, layout_type=None, pack=None, nparams=0, param_name=None, workspace_bytes=None,
                    create=None, geometry_of=None, info=None, geometry_type=None, destroy=None, npacks=0, plan_cls=None)
        super().__init__(name=name, cfg=cfg, **dict(base, **kw))

    def __repr__(self):
        return self.name

    def fn(self, what):
        return getattr(_lib.load(), getattr(self, what))


FAMILIES = [
    Fam("decode", lambda: _lib.DecodeCfg(B=1, N=4, H=2, W=2, S=1, L=2, F=256, mode=_lib.PH_MODE["bf16"], out_dtype=_lib.PH_OUT_F32,
                                        up2_wgs=1),      # given: create needs no device to work it out
        pack_bytes="ph_decode_pack_bytes", pack_layout="ph_decode_pack_layout", layout_type=_lib.StageLayout, pack="ph_decode_pack_stage",
        nparams=_lib.PH_DECODE_NPARAMS, param_name=lambda cfg, i: _lib.load().ph_decode_param_name(i),
        workspace_bytes="ph_decode_workspace_bytes", create="ph_decode_create", geometry_of="ph_decode_geometry_of", info="ph_decode_info",
        geometry_type=_lib.DecodeGeometry, destroy="ph_decode_destroy", npacks=1, plan_cls=E.NativeDecodePlan),
    Fam("khead", lambda: _lib.KheadCfg(B=1, H=2, W=2, num_proposals=1, num_classes=1, num_thing_classes=1, cat_stuff=0, groups=32,
                                       mode=_lib.PH_MODE["bf16"], logit_dtype=_lib.PH_OUT_F32, emit_f32=1, onepass=_lib.PH_KNOB_OFF),
        pack_bytes="ph_khead_pack_bytes", pack_layout="ph_khead_pack_layout", layout_type=_lib.KheadLayout, pack="ph_khead_pack",
        nparams=_lib.PH_KHEAD_NPARAMS, param_name=lambda cfg, i: _lib.load().ph_khead_param_name(i),
        workspace_bytes="ph_khead_plan_workspace_bytes", create="ph_khead_plan_create", geometry_of="ph_khead_geometry_of",
        info="ph_khead_plan_info", geometry_type=_lib.KheadGeometry, destroy="ph_khead_plan_destroy", plan_cls=E.NativeKernelHeadPlan),
    Fam("neck", lambda: _lib.NeckCfg(B=1, h=I4([s[0] for s in PYR]), w=I4([s[1] for s in PYR]), groups=32, mode=_lib.PH_MODE["bf16"],
                                     num_outs=1, pos_level=-1, emit_f32=1),
        pack_bytes="ph_neck_pack_bytes", pack_layout="ph_neck_pack_layout", layout_type=_lib.NeckLayout, pack="ph_neck_pack",
        nparams=3 * 8, param_name=lambda cfg, i: _lib.load().ph_neck_param_name(i),
        workspace_bytes="ph_neck_plan_workspace_bytes", create="ph_neck_plan_create", geometry_of="ph_neck_geometry_of",
        info="ph_neck_plan_info", geometry_type=_lib.NeckGeometry, destroy="ph_neck_plan_destroy", plan_cls=E.NativeNeckPlan),
    Fam("fpn", lambda: _lib.FpnCfg(B=1, k=I4([64] * 4), h=I4([s[0] for s in PYR]), w=I4([s[1] for s in PYR]), mode=_lib.PH_MODE["bf16"],
                                   x_dtype=_lib.PH_OUT_F32, emit_f32=1),
        pack_bytes="ph_fpn_pack_bytes", pack_layout="ph_fpn_pack_layout", layout_type=_lib.FpnLayout, pack="ph_fpn_pack",
        nparams=_lib.PH_FPN_NPARAMS, param_name=lambda cfg, i: _lib.load().ph_fpn_param_name(i),
        workspace_bytes="ph_fpn_plan_workspace_bytes", create="ph_fpn_plan_create", geometry_of="ph_fpn_geometry_of",
        info="ph_fpn_plan_info", geometry_type=_lib.FpnGeometry, destroy="ph_fpn_plan_destroy", plan_cls=E.NativeFpnPlan),
    Fam("track", _track_cfg, pack_bytes="ph_track_pack_bytes", pack_layout="ph_track_pack_layout", layout_type=_lib.TrackLayout,
        pack="ph_track_pack", nparams=3 * 1 + 4, param_name=lambda cfg, i: _lib.load().ph_track_param_name(C.byref(cfg), i)),
    Fam("assoc", _assoc_cfg, workspace_bytes="ph_assoc_plan_workspace_bytes", create="ph_assoc_plan_create", info="ph_assoc_plan_info",
        geometry_type=_lib.AssocGeometry, destroy="ph_assoc_plan_destroy", plan_cls=E.NativeAssocPlan),
]
with_ = lambda *kinds: pytest.mark.parametrize("fam", [f for f in FAMILIES if all(getattr(f, k) for k in kinds)], ids=repr)


def _own_name(fam, what):
    """the last message starts with this entry point's own name"""
    name = getattr(fam, what)
    assert Hh.last_error().startswith(name + ": "), (name, Hh.last_error())
    return True


def _pack_arg(fam, value=FAKE):
    """create's pack argument: one pointer, or decode's array of S of them"""
    return (C.c_void_p * fam.npacks)(*([value] * fam.npacks)) if fam.npacks else C.c_void_p(value)


def _create(fam, cfg, pack, ws, nbytes, out=True):
    h = C.c_void_p(0xDEAD00)          # create must put NULL over this before it checks a buffer
    rc = fam.fn("create")(C.byref(cfg), pack, ws, nbytes, C.byref(h) if out else None)
    return rc, h


# ---- a NULL cfg ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES, ids=repr)
def test_null_cfg(fam):
    for what in ("pack_bytes", "workspace_bytes"):
        if getattr(fam, what):
            assert fam.fn(what)(None) == 0 and _own_name(fam, what) and "null cfg" in Hh.last_error()
    if fam.pack_layout:
        args = (None, C.byref(fam.layout_type())) + ((C.byref(C.c_size_t()),) if fam.name == "decode" else ())
        assert fam.fn("pack_layout")(*args) == _lib.PH_EINVAL and _own_name(fam, "pack_layout")
    if fam.pack:
        params = (C.c_void_p * fam.nparams)(*([FAKE] * fam.nparams))
        assert fam.fn("pack")(None, params, C.c_void_p(FAKE), None) == _lib.PH_EINVAL and _own_name(fam, "pack")
    if fam.create:
        h = C.c_void_p()
        assert fam.fn("create")(None, _pack_arg(fam), C.c_void_p(FAKE), 1 << 62, C.byref(h)) == _lib.PH_EINVAL and not h.value
        assert _own_name(fam, "create") and "null cfg" in Hh.last_error()
    if fam.geometry_of:
        assert fam.fn("geometry_of")(None, C.byref(fam.geometry_type())) == _lib.PH_EINVAL and _own_name(fam, "geometry_of")


# ---- the smallest valid cfg: NULL and misplaced buffers ------------------------------------------------------------------------------
@with_("pack_layout")
def test_pack_layout_and_bytes(fam):
    cfg, lay = fam.cfg(), fam.layout_type()
    nbytes = fam.fn("pack_bytes")(C.byref(cfg))
    assert nbytes > 0 and nbytes % 256 == 0, Hh.last_error()
    if fam.name == "decode":      # its own layout call: both outputs are optional
        off = C.c_size_t()
        assert fam.fn("pack_layout")(C.byref(cfg), None, None) == 0
        assert fam.fn("pack_layout")(C.byref(cfg), C.byref(lay), C.byref(off)) == 0 and 0 < off.value < nbytes and off.value % 256 == 0
        return
    assert fam.fn("pack_layout")(C.byref(cfg), None) == _lib.PH_EINVAL and _own_name(fam, "pack_layout") and "null layout" in Hh.last_error()
    assert fam.fn("pack_layout")(C.byref(cfg), C.byref(lay)) == 0
    ends = [int(o) + (int(b) + 255) // 256 * 256 for o, b in zip(lay.offset, lay.bytes)]
    assert all(int(o) % 256 == 0 for o in lay.offset) and max(ends) == nbytes


@with_("pack")
def test_pack_checks_come_before_the_launch(fam):
    cfg, pack = fam.cfg(), fam.fn("pack")
    full = lambda: (C.c_void_p * fam.nparams)(*([FAKE] * fam.nparams))
    assert pack(C.byref(cfg), None, C.c_void_p(FAKE), None) == _lib.PH_EINVAL and _own_name(fam, "pack")
    assert pack(C.byref(cfg), full(), None, None) == _lib.PH_EINVAL and _own_name(fam, "pack") and "null params or pack" in Hh.last_error()
    for i in (0, fam.nparams // 2, fam.nparams - 1):
        params = full()
        params[i] = None
        # a NULL parameter is named, and found before the pack's alignment is looked at
        assert pack(C.byref(cfg), params, C.c_void_p(FAKE + 16), None) == _lib.PH_EINVAL and _own_name(fam, "pack")
        assert f"parameter {i} ({fam.param_name(cfg, i).decode()}) is NULL" in Hh.last_error(), Hh.last_error()
    assert pack(C.byref(cfg), full(), C.c_void_p(FAKE + 128), None) == _lib.PH_EINVAL and _own_name(fam, "pack")
    assert "pack must be 256-byte aligned" in Hh.last_error()


@with_("create")
def test_create_checks_its_buffers(fam):
    cfg = fam.cfg()
    need = fam.fn("workspace_bytes")(C.byref(cfg))
    assert need > 0 and need % 256 == 0, Hh.last_error()
    ws = C.c_void_p(FAKE)
    # NULL pack, workspace or out: one check, before *out is touched
    rc, h = _create(fam, cfg, None, ws, need)
    assert rc == _lib.PH_EINVAL and h.value == 0xDEAD00 and _own_name(fam, "create") and "null pack" in Hh.last_error()
    rc, h = _create(fam, cfg, _pack_arg(fam), None, need)
    assert rc == _lib.PH_EINVAL and h.value == 0xDEAD00 and _own_name(fam, "create") and "workspace or out" in Hh.last_error()
    rc, _ = _create(fam, cfg, _pack_arg(fam), ws, need, out=False)
    assert rc == _lib.PH_EINVAL and _own_name(fam, "create") and "workspace or out" in Hh.last_error()
    # the buffers: *out is NULL from here on
    rc, h = _create(fam, cfg, _pack_arg(fam, FAKE + 128), ws, need)
    assert rc == _lib.PH_EINVAL and not h.value and _own_name(fam, "create") and "256-byte aligned" in Hh.last_error()
    if fam.npacks:
        rc, h = _create(fam, cfg, _pack_arg(fam, None), ws, need)
        assert rc == _lib.PH_EINVAL and not h.value and "pack 0 is NULL" in Hh.last_error()
    rc, h = _create(fam, cfg, _pack_arg(fam), ws, need - 1)
    assert rc == _lib.PH_EWORKSPACE and not h.value and _own_name(fam, "create") and f"workspace too small ({need - 1} < {need})" in Hh.last_error()
    rc, h = _create(fam, cfg, _pack_arg(fam), C.c_void_p(FAKE + 128), need)
    assert rc == _lib.PH_EINVAL and not h.value and _own_name(fam, "create") and "workspace must be 256-byte aligned" in Hh.last_error()
    # too small and misaligned: the size is looked at first
    assert _create(fam, cfg, _pack_arg(fam), C.c_void_p(FAKE + 128), need - 1)[0] == _lib.PH_EWORKSPACE
    rc, h = _create(fam, cfg, _pack_arg(fam), ws, need)
    assert rc == 0 and h.value not in (0, 0xDEAD00), Hh.last_error()
    # info: the plan's geometry; the same bytes geometry_of gives for the cfg
    geo = fam.geometry_type()
    assert fam.fn("info")(None, C.byref(geo)) == _lib.PH_EINVAL and _own_name(fam, "info") and "null plan or out" in Hh.last_error()
    assert fam.fn("info")(h, None) == _lib.PH_EINVAL and _own_name(fam, "info")
    assert fam.fn("info")(h, C.byref(geo)) == 0
    if fam.geometry_of:
        asked = fam.geometry_type()
        assert fam.fn("geometry_of")(C.byref(cfg), None) == _lib.PH_EINVAL and _own_name(fam, "geometry_of") and "null out" in Hh.last_error()
        assert fam.fn("geometry_of")(C.byref(cfg), C.byref(asked)) == 0 and bytes(asked) == bytes(geo)
    fam.fn("destroy")(h)
    fam.fn("destroy")(None)


@pytest.mark.gpu
def test_khead_plan_side_resolve_reads_the_device(gpu):
    """KernelHead's plan calls resolve with the device (the one-pass rule asks its CU count), its pack calls without: a cfg that
    leaves the choice open gives the one-pass form on the device at this size, in geometry_of and in a created plan alike"""
    fam = FAMILIES[1]
    lib, cfg = _lib.load(), fam.cfg()
    cfg.H, cfg.W, cfg.onepass = 4, 8, _lib.PH_KNOB_AUTO
    with torch.cuda.device(gpu):
        sup = lib.ph_khead_onepass_supported(1, 32, 32, _lib.PH_PREC_BF16, _lib.PH_IN_F32_NCHW)
        assert sup == 1
        asked, told = _lib.KheadGeometry(), _lib.KheadGeometry()
        assert lib.ph_khead_geometry_of(C.byref(cfg), C.byref(asked)) == 0 and asked.onepass == 1
        need = lib.ph_khead_plan_workspace_bytes(C.byref(cfg))
        rc, h = _create(fam, cfg, C.c_void_p(FAKE), C.c_void_p(FAKE), need)
        assert rc == 0 and lib.ph_khead_plan_info(h, C.byref(told)) == 0 and bytes(told) == bytes(asked)
        lib.ph_khead_plan_destroy(h)
        assert lib.ph_khead_pack_bytes(C.byref(cfg)) > 0


# ---- the Python bases -----------------------------------------------------------------------------------------------------------------
def _stub_pack(fam):
    """what a Native*Plan reads of its pack before it asks the library about the cfg"""
    return types.SimpleNamespace(blob=None, n_seg=1, n_init=1, groups=32, mode=_lib.PH_MODE["bf16"], num_outs=1, in_channels=(64,) * 4,
                                 cfg=_track_cfg())


def _plan(fam, cfg):
    pack = _stub_pack(fam)
    if fam.name == "decode":
        return E.NativeDecodePlan([None] * cfg.S, cfg.B, cfg.N, cfg.H, cfg.W, "bf16", device="cpu", num_classes=cfg.L, ffn_dim=cfg.F)
    if fam.name == "khead":
        return E.NativeKernelHeadPlan(pack, cfg.B, cfg.H, cfg.W, 1, 1, False, "cpu", cfg=cfg)
    if fam.name == "assoc":
        return E.NativeAssocPlan(pack, cfg, "cpu")
    return fam.plan_cls(pack, cfg.B, PYR, "cpu", cfg=cfg)


@with_("plan_cls")
def test_a_refused_cfg_raises_with_the_librarys_words(fam, monkeypatch):
    for k in ("PH_CONV_POOLX", "PH_CONV_UP2", "PH_POOL_NSPLIT", "PH_POOLX_NSPLIT", "PH_UP2_SHARED_WGS"):
        monkeypatch.delenv(k, raising=False)
    cfg = fam.cfg()
    cfg.B = 4097                       # every family: PH_EUNSUPPORTED, "at most 4096 frames per call"
    if fam.name == "decode":
        cfg.B, cfg.N = 1, 257          # decode's plan takes its sizes as arguments: "at most 256 queries"
    with pytest.raises(_lib.PolyheadError) as e:
        _plan(fam, cfg)
    words = "at most 256 queries" if fam.name == "decode" else "at most 4096 frames per call"
    assert f"{fam.workspace_bytes}: {fam.workspace_bytes}: {words}" in str(e.value), str(e.value)


class _Counting:
    """the loaded library with the calls of one symbol counted"""

    def __init__(self, lib, symbol):
        self._lib, self._symbol, self.calls = lib, symbol, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._symbol:
            return fn
        return lambda h: (self.calls.append(h.value), fn(h))[1]


@with_("plan_cls")
@pytest.mark.parametrize("nhandles", [1, 2])
def test_a_dropped_plan_destroys_each_handle_once(fam, nhandles, monkeypatch):
    lib, cfg = _lib.load(), fam.cfg()
    need = fam.fn("workspace_bytes")(C.byref(cfg))
    handles = []
    for _ in range(nhandles):
        rc, h = _create(fam, cfg, _pack_arg(fam), C.c_void_p(FAKE), need)
        assert rc == 0
        handles.append(h)
    assert fam.plan_cls._destroy_symbol == fam.destroy
    plan = object.__new__(fam.plan_cls)
    if nhandles == 1:
        plan._h = handles[0]
    else:
        plan._handles = dict(enumerate(handles))
    counting = _Counting(lib, fam.destroy)
    monkeypatch.setattr(_lib, "_lib", counting)
    want = sorted(h.value for h in handles)
    del plan
    gc.collect()
    assert sorted(counting.calls) == want
