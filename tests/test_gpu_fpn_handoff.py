"""GPU: the FPN's direct hand-over to the neck (csrc/ph_fpn.hip ph_fpn_output_planes; engine.FpnPlan.run(neck=...), engine.NeckHandoff;
SemanticFPNWrapper.forward_from_fpn).  Every comparison is between two paths that perform the same fp32 operations in the same order
-- the FPN's output tail writing the neck's conv input planes itself, against ph_fpn_output followed by ph_nhwc_ingest -- so every
equality is bit for bit and no tolerance appears.  Buffers are poisoned (NaN / 0x7FFF, neither a value these kernels write) before
each run, so an element that was not written shows."""
import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
from polyphonicformer_amd.registry import NECKS
from polyphonicformer_amd.semantic_fpn import sine_positional_encoding
import polyphonicformer_amd.fpn  # noqa: F401

pytestmark = pytest.mark.gpu

GRADES = {"bf16": _lib.PH_PREC_BF16, "fp16": _lib.PH_PREC_F16, "fp32": _lib.PH_PREC_SPLIT}
C16 = _lib.PH_PLANES_C16
P_EVEN = ((16, 32), (8, 16), (4, 8), (2, 4))
P_ODD = ((15, 23), (8, 12), (4, 6), (2, 3))          # level 0: 345 pixels (no multiple of 4, a partial tile); level 3: 6 pixels
P_WIDE = ((16, 143), (8, 72), (4, 36), (2, 18))      # crosses the 64-pixel tile
PYRAMIDS = {"even": P_EVEN, "odd": P_ODD, "wide": P_WIDE}
CH = (64, 128, 256, 320)
CH_FULL = (256, 512, 1024, 2048)
NECK_CFG = dict(type="SemanticFPNWrapper", in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
                upsample_times=2, positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                cat_coors=False, cat_coors_level=3, fuse_by_cat=False, return_list=False, num_aux_convs=2,
                norm_cfg=dict(type="GN", num_groups=32, requires_grad=True))


@pytest.fixture(autouse=True)
def _inference(monkeypatch):
    Hh.clear_plan_knobs(monkeypatch)
    with torch.no_grad():
        yield


def _poison(ts):
    for t in ts:
        t.fill_(0x7FFF if t.dtype == torch.int16 else float("nan"))


# ---- 1. the kernel against the two-step path --------------------------------------------------------------------------------------
_OPS = {}


def _operands(HW, gpu):
    """(y [3, HW, 256], bias [256], add [256, HW]) on the device, made once per size"""
    if HW not in _OPS:
        g = torch.Generator().manual_seed(100 + HW)
        _OPS[HW] = tuple(t.to(gpu) for t in (torch.randn(3, HW, 256, generator=g), torch.randn(256, generator=g),
                                            torch.randn(256, HW, generator=g)))
    return _OPS[HW]


def _two_step(y, bias, add, B, HW, prec):
    """nhwc_ingest(fpn_output(y, bias), add): (planes, the fp32 level)"""
    P = 2 if (prec & ~C16) == _lib.PH_PREC_SPLIT else 1
    level = torch.full((B, 256, 1, HW), float("nan"), device=y.device)
    planes = torch.full((P, B, HW, 256), 0x7FFF, dtype=torch.int16, device=y.device)
    E.fpn_output(y, bias, level, B, HW)
    E.nhwc_ingest(level, add, prec, planes)
    return planes, level


def _direct(y, bias, add, B, HW, prec, want_f32):
    P = 2 if (prec & ~C16) == _lib.PH_PREC_SPLIT else 1
    level = torch.full((B, 256, 1, HW), float("nan"), device=y.device) if want_f32 else None
    planes = torch.full((P, B, HW, 256), 0x7FFF, dtype=torch.int16, device=y.device)
    E.fpn_output_planes(y, bias, add, planes, level, B, HW, prec)
    return planes, level


LAYOUTS = [("bf16", 0), ("bf16", C16), ("fp16", 0), ("fp16", C16), ("fp32", 0)]


@pytest.mark.parametrize("HW", [6, 345, 2288])
@pytest.mark.parametrize("want_f32", [False, True], ids=["planes", "planes+f32"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("grade,layout", LAYOUTS, ids=[f"{g}-{'c16' if l else 'nhwc'}" for g, l in LAYOUTS])
def test_kernel_equals_the_two_step_path(gpu, grade, layout, with_add, want_f32, HW):
    B = 2
    y, bias, add = _operands(HW, gpu)
    y, add = y[:B].contiguous(), add if with_add else None
    prec = GRADES[grade] | layout
    want, level = _two_step(y, bias, add, B, HW, prec)
    got, got_level = _direct(y, bias, add, B, HW, prec, want_f32)
    torch.cuda.synchronize()
    assert not bool((want == 0x7FFF).any()) and not bool(level.isnan().any())      # the reference wrote every element
    assert torch.equal(got, want)
    if want_f32:
        assert torch.equal(got_level, level)


# ---- 2. batch invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grade,layout", LAYOUTS, ids=[f"{g}-{'c16' if l else 'nhwc'}" for g, l in LAYOUTS])
def test_a_frame_does_not_depend_on_the_batch(gpu, grade, layout):
    HW = 345
    y, bias, add = _operands(HW, gpu)
    prec = GRADES[grade] | layout
    p3, l3 = _direct(y, bias, add, 3, HW, prec, True)
    p1, l1 = _direct(y[:1].contiguous(), bias, add, 1, HW, prec, True)
    torch.cuda.synchronize()
    # frames are outermost inside a plane in both layouts ([P][B][HW][256]; chunk-major [B][16][HW][16], one plane)
    assert torch.equal(p3[:, :1], p1) and torch.equal(l3[:1], l1)


# ---- 3. bad arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(gpu):
    lib = _lib.load()
    HW, B = 345, 2
    y, bias, add = _operands(HW, gpu)
    planes = torch.full((2, B, HW, 256), 0x7FFF, dtype=torch.int16, device=gpu)
    level = torch.full((B, 256, HW), float("nan"), device=gpu)
    p = _lib.ptr

    def call(y_, bias_, planes_, prec, B_=B, HW_=HW):
        return lib.ph_fpn_output_planes(y_, bias_, p(add), planes_, p(level), B_, HW_, prec, _lib.stream_ptr())
    bf16, split = _lib.PH_PREC_BF16, _lib.PH_PREC_SPLIT
    for args in ((None, p(bias), p(planes), bf16),                     # a NULL pointer: y, bias, planes
                 (p(y), None, p(planes), bf16),
                 (p(y), p(bias), None, bf16),
                 (p(y), p(bias), p(planes), split | C16),              # chunk-major planes with the two-plane grade
                 (p(y), p(bias), p(planes), 0),                        # unknown grades
                 (p(y), p(bias), p(planes), _lib.PH_PREC_BF16_KSPLIT),
                 (p(y), p(bias), p(planes), 99 | C16),
                 (p(y), p(bias), p(planes), bf16, 0),                  # sizes
                 (p(y), p(bias), p(planes), bf16, B, 0)):
        assert call(*args) == _lib.PH_EINVAL, args
        assert "ph_fpn_output_planes" in Hh.last_error()
    torch.cuda.synchronize()
    assert bool((planes == 0x7FFF).all()) and bool(level.isnan().all())
    assert call(p(y), p(bias), p(planes), split) == 0
    torch.cuda.synchronize()
    assert not bool((planes == 0x7FFF).any()) and not bool(level.isnan().any())


# ---- 4. FpnPlan.run(neck=...) -------------------------------------------------------------------------------------------------------
_MODS = {}


def _fill(m, seed):
    """non-trivial parameters: default GroupNorm parameters and zero biases would hide a swapped or a dropped one"""
    g = torch.Generator().manual_seed(seed)
    for name, p in m.named_parameters():
        if name.endswith("conv.weight"):
            p.copy_(0.05 * torch.randn(p.shape, generator=g))
        elif name.endswith("gn.weight"):
            p.copy_(0.5 + torch.rand(p.shape, generator=g))
        else:
            p.copy_(0.2 * torch.randn(p.shape, generator=g))


def _fpn(grade, channels=CH):
    key = ("fpn", grade, channels)
    if key not in _MODS:
        m = NECKS.build(dict(type="FPN", in_channels=list(channels), out_channels=256, num_outs=4))
        _fill(m, 11)
        m.eval().to("cuda:0")
        m.set_precision(grade)
        _MODS[key] = m
    return _MODS[key]


def _neck(grade, num_aux=2, return_list=False):
    key = ("neck", grade, num_aux, return_list)
    if key not in _MODS:
        m = NECKS.build(dict(NECK_CFG, num_aux_convs=num_aux, return_list=return_list))
        _fill(m, 9 + num_aux)
        m.eval().to("cuda:0")
        m.set_precision(grade)
        _MODS[key] = m
    return _MODS[key]


def _stages(shapes, B, gpu, channels=CH, seed=3, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, h, w, generator=g).relu().to(dtype).to(gpu) for c, (h, w) in zip(channels, shapes)]


def _plans(grade, shapes, B, gpu, tower_streams, channels=CH):
    fpn, neck = _fpn(grade, channels), _neck(grade)
    fplan = E.FpnPlan(B, shapes, channels, GRADES[grade], gpu)
    nplan = E.NeckPlan(B, shapes, GRADES[grade], gpu, tower_streams=tower_streams)
    return fplan, fpn._pack(gpu), nplan, neck._pack(gpu), sine_positional_encoding(*shapes[3], 128).to(gpu)


def _check_handoff(gpu, grade, shapes, B, tower_streams, channels=CH):
    fplan, fpk, nplan, npk, posenc = _plans(grade, shapes, B, gpu, tower_streams, channels)
    assert nplan.multi == (tower_streams == "always")
    stages = _stages(shapes, B, gpu, channels)
    levels = [o.clone() for o in fplan.run(stages, fpk)]
    want = {tp: [o.clone() for o in nplan.run(levels, npk, 32, posenc, 3, to_planes=tp)] for tp in (False, True)}
    for tp in (False, True):
        _poison(fplan.outs + nplan.outs + nplan.pouts + [nplan.xa] + ([lv["xa"] for lv in nplan.lv] if nplan.multi else []))
        neck = E.NeckHandoff(nplan, npk, 32, posenc, 3, to_planes=tp)
        got_levels = fplan.run(stages, fpk, neck=neck)
        got = neck.finish()
        torch.cuda.synchronize()
        assert len(got) == 3
        for a, b in zip(got, want[tp]):
            assert torch.equal(a, b), (tp, grade)
        for a, b in zip(got_levels, levels):
            assert torch.equal(a, b)
    # without the fp32 levels: they stay untouched, the neck's outputs are the same
    _poison(fplan.outs + nplan.outs)
    neck = E.NeckHandoff(nplan, npk, 32, posenc, 3)
    fplan.run(stages, fpk, neck=neck, want_levels=False)
    got = neck.finish()
    torch.cuda.synchronize()
    assert all(bool(o.isnan().all()) for o in fplan.outs)
    for a, b in zip(got, want[False]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tower_streams", [False, "always"], ids=["shared", "towers"])
@pytest.mark.parametrize("grade", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("pyramid", ["even", "odd", "wide"])
def test_fpn_plan_writes_the_neck_plans_inputs(gpu, pyramid, grade, tower_streams):
    _check_handoff(gpu, grade, PYRAMIDS[pyramid], 2, tower_streams)


def test_fpn_plan_hand_over_at_the_shipped_stage_widths(gpu):
    _check_handoff(gpu, "fp16", P_ODD, 1, False, CH_FULL)


def test_hand_over_refuses_a_plan_of_another_geometry(gpu):
    fplan, fpk, nplan, npk, posenc = _plans("bf16", P_EVEN, 2, gpu, False)
    stages = _stages(P_EVEN, 2, gpu)
    other = E.NeckPlan(1, P_EVEN, GRADES["bf16"], gpu, tower_streams=False)
    with pytest.raises(_lib.PolyheadError, match="neck plan"):
        fplan.run(stages, fpk, neck=E.NeckHandoff(other, npk, 32, posenc, 3))
    other = E.NeckPlan(2, P_EVEN, GRADES["fp16"], gpu, tower_streams=False)
    with pytest.raises(_lib.PolyheadError, match="neck plan"):
        fplan.run(stages, fpk, neck=E.NeckHandoff(other, npk, 32, posenc, 3))
    with pytest.raises(_lib.PolyheadError, match="posenc"):
        E.NeckHandoff(nplan, npk, 32, posenc[:, :1].contiguous(), 3)


# ---- 5. the module API ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("native", [False, True], ids=["python-plan", "native-plan"])
@pytest.mark.parametrize("grade,pyramid,B", [("bf16", "odd", 2), ("fp16", "wide", 1), ("fp32", "even", 2), ("fp16", "even", 4)])
def test_forward_from_fpn(gpu, grade, pyramid, B, native):
    """B = 4: the tower-buffer form is the module's own choice from four frames"""
    shapes = PYRAMIDS[pyramid]
    fpn, neck = _fpn(grade), _neck(grade)
    stages = _stages(shapes, B, gpu, seed=5)
    neck.use_native_plan(native)
    try:
        levels = [o.clone() for o in fpn(stages)]
        want = [o.clone() for o in neck(levels)]
        want_planes = [o.clone() for o in neck.forward_planes(levels)]
        got = neck.forward_from_fpn(fpn, stages)
        assert isinstance(got, list) and len(got) == 3
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        for a, b in zip(neck.forward_from_fpn(fpn, stages, planes=True), want_planes):
            assert torch.equal(a, b)
        got, got_levels = neck.forward_from_fpn(fpn, stages, want_levels=True)
        assert isinstance(got_levels, tuple) and len(got_levels) == 4
        for a, b in zip(list(got) + list(got_levels), want + levels):
            assert torch.equal(a, b)
        got, got_levels = neck.forward_from_fpn(fpn, stages, planes=True, want_levels=True)
        for a, b in zip(list(got) + list(got_levels), want_planes + levels):
            assert torch.equal(a, b)
        # 16-bit stages go the same way
        st16 = [t.to(torch.bfloat16) for t in stages]
        want16 = [o.clone() for o in neck(list(fpn(st16)))]
        for a, b in zip(neck.forward_from_fpn(fpn, st16), want16):
            assert torch.equal(a, b)
    finally:
        neck.use_native_plan(False)


@pytest.mark.parametrize("native", [False, True], ids=["python-plan", "native-plan"])
def test_forward_from_fpn_returns_what_forward_returns(gpu, native):
    """one output map: a tensor, or a list of one with return_list"""
    fpn = _fpn("fp16")
    stages = _stages(P_EVEN, 1, gpu, seed=6)
    for return_list in (False, True):
        neck = _neck("fp16", num_aux=0, return_list=return_list)
        neck.use_native_plan(native)
        want = neck(list(fpn(stages)))
        want = [w.clone() for w in want] if return_list else want.clone()
        got = neck.forward_from_fpn(fpn, stages)
        assert type(got) is type(want)
        assert torch.equal(got[0], want[0]) if return_list else torch.equal(got, want)
        with pytest.raises(NotImplementedError):
            neck.forward_from_fpn(fpn, stages, planes=True)
        neck.use_native_plan(False)


def test_forward_from_fpn_is_inference_only(gpu):
    fpn, neck = _fpn("bf16"), _neck("bf16")
    stages = _stages(P_EVEN, 1, gpu)
    with torch.enable_grad():
        for m in (neck, fpn):
            m.train()
            try:
                with pytest.raises(_lib.PolyheadError, match=r"forward\(fpn\(stages\)\)"):
                    neck.forward_from_fpn(fpn, stages)
            finally:
                m.eval()
    other = _fpn("fp16")
    with pytest.raises(_lib.PolyheadError, match="precision"):
        neck.forward_from_fpn(other, stages)


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_whole_fpn_and_neck_run(gpu):
    """shared neck buffers, one stream: the FPN's laterals, then per level conv + tail + tower, then the neck's outputs"""
    B, shapes, grade = 2, P_ODD, "fp16"
    fplan, fpk, nplan, npk, posenc = _plans(grade, shapes, B, gpu, False)
    static = _stages(shapes, B, gpu, seed=20)
    neck = E.NeckHandoff(nplan, npk, 32, posenc, 3, to_planes=True)

    def run():
        fplan.run(static, fpk, neck=neck)
        return neck.finish()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                    # warm-up outside capture (lazy module load, the plane outputs' allocation)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for seed in (21, 22):
        for dst, src in zip(static, _stages(shapes, B, gpu, seed=seed)):
            dst.copy_(src)
        _poison(list(outs) + fplan.outs)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in list(outs) + fplan.outs]
        _poison(list(outs) + fplan.outs)
        eager = run()
        torch.cuda.synchronize()
        for a, b in zip(replayed, list(eager) + fplan.outs):
            assert torch.equal(a, b), seed
        levels = [o.clone() for o in fplan.run(static, fpk)]              # and both equal the two-step chain
        for a, b in zip(replayed, [o.clone() for o in nplan.run(levels, npk, 32, posenc, 3, to_planes=True)] + levels):
            assert torch.equal(a, b), seed
