"""GPU: the backbone's hand-over to the FPN on 16-bit channels-last stage planes (csrc/ph_fpn.hip ph_fpn_lateral_cl;
engine.ResNetPlan(stage_planes=True), engine.StagePlanes, engine.FpnPlan.run(StagePlanes); resnet.ResNet.forward_planes;
VideoFramePipeline.extract_feat and the runners' image calls).  Every comparison is between two paths that perform the same fp32
operations in the same order -- the lateral reading the backbone's plane, against ph_cl_to_nchw followed by ph_fpn_lateral on the fp32
tensor -- so every equality is bit for bit and no tolerance appears.  Buffers are poisoned (NaN / 0x7FFF, neither a value these
kernels write from these inputs) before each run, so an element that was not written shows."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import helpers as Hh
import resnet_cases
import test_gpu_video as GV
from polyphonicformer_amd import _lib, engine as E, registry, video as V
from polyphonicformer_amd.pack import pack_b32
import polyphonicformer_amd.fpn  # noqa: F401

pytestmark = pytest.mark.gpu

GRADES = {"bf16": _lib.PH_PREC_BF16, "fp16": _lib.PH_PREC_F16, "fp32": _lib.PH_PREC_SPLIT}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# (H, W) with its coarse level: less than a tile; 345 pixels (a partial tile, no multiple of 4); several tiles.  2 Hc - 1 and 2 Hc
# on the rows, 2 Wc - 1 and 2 Wc on the columns
SIZES = {(2, 3): (1, 2), (15, 23): (8, 12), (16, 143): (8, 72)}


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


def _weights(K, grade, gpu):
    """(pack_b32 fragments of W[256][K] in the grade [1, 256 K], bias [256]) on the device, made once"""
    key = ("w", K, grade)
    if key not in _OPS:
        g = torch.Generator().manual_seed(300 + K)
        w = torch.randn(256, K, generator=g, dtype=torch.float64) / K ** 0.5
        planes = E._planes_of(w, 1, grade == "fp16")
        _OPS[key] = (pack_b32(planes[0])[None].contiguous().to(gpu), torch.randn(256, generator=g).to(gpu))
    return _OPS[key]


def _plane(K, HW, x_grade, gpu):
    """X [3, HW, K]: randn rounded to `x_grade`, as the int16 plane"""
    key = ("x", K, HW, x_grade)
    if key not in _OPS:
        g = torch.Generator().manual_seed(500 + K + HW)
        _OPS[key] = torch.randn(3, HW, K, generator=g).to(DTYPES[x_grade]).view(torch.int16).to(gpu)
    return _OPS[key]


def _coarse(hw, grade, gpu):
    key = ("c", hw, grade)
    if key not in _OPS:
        g = torch.Generator().manual_seed(700 + hw[0] * hw[1])
        _OPS[key] = torch.randn(1, 3, hw[0] * hw[1], 256, generator=g).to(DTYPES[grade]).view(torch.int16).to(gpu)
    return _OPS[key]


def _two_step(x, x_grade, hw, wp, bias, coarse, chw, grade):
    """fpn_lateral(cl_to_nchw(X -> fp32), ...)"""
    B, HW, K = x.shape
    st = torch.full((B, K) + hw, float("nan"), device=x.device)
    E.cl_to_nchw(x, st, B, HW, K, GRADES[x_grade])
    out = torch.full((1, B, HW, 256), 0x7FFF, dtype=torch.int16, device=x.device)
    E.fpn_lateral(st, wp, bias, coarse, chw, out, GRADES[grade])
    return out, st


def _direct(x, x_grade, hw, wp, bias, coarse, chw, grade):
    out = torch.full((1, x.shape[0], x.shape[1], 256), 0x7FFF, dtype=torch.int16, device=x.device)
    return E.fpn_lateral_cl(x, GRADES[x_grade], hw, wp, bias, coarse, chw, out, GRADES[grade])


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
@pytest.mark.parametrize("x_grade", ["bf16", "fp16"])
@pytest.mark.parametrize("with_coarse", [False, True], ids=["top", "coarse"])
@pytest.mark.parametrize("hw", list(SIZES), ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("K", [64, 320, 2048])
def test_kernel_equals_the_two_step_path(gpu, K, hw, with_coarse, x_grade, grade):
    B, HW = 2, hw[0] * hw[1]
    wp, bias = _weights(K, grade, gpu)
    x = _plane(K, HW, x_grade, gpu)[:B].contiguous()
    chw = SIZES[hw] if with_coarse else None
    coarse = _coarse(chw, grade, gpu)[:, :B].contiguous() if with_coarse else None
    want, st = _two_step(x, x_grade, hw, wp, bias, coarse, chw, grade)
    got = _direct(x, x_grade, hw, wp, bias, coarse, chw, grade)
    torch.cuda.synchronize()
    assert not bool(st.isnan().any()) and not bool((want == 0x7FFF).any())        # the reference wrote every element
    assert torch.equal(st, x.view(DTYPES[x_grade]).float().permute(0, 2, 1).reshape(st.shape))
    assert torch.equal(got, want)


# ---- 2. batch invariance, an offset pointer -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_a_frame_does_not_depend_on_the_batch(gpu, grade):
    K, hw = 320, (15, 23)
    wp, bias = _weights(K, grade, gpu)
    x, coarse = _plane(K, 345, grade, gpu), _coarse(SIZES[hw], grade, gpu)
    o3 = _direct(x, grade, hw, wp, bias, coarse, SIZES[hw], grade)
    for b in range(3):
        o1 = _direct(x[b:b + 1].contiguous(), grade, hw, wp, bias, coarse[:, b:b + 1].contiguous(), SIZES[hw], grade)
        torch.cuda.synchronize()
        assert torch.equal(o3[:, b:b + 1], o1)


def test_a_plane_at_an_offset_of_64_elements(gpu):
    """128 bytes into an allocation: 16-byte aligned, not aligned to a row of the plane"""
    K, hw, grade = 320, (15, 23), "bf16"
    wp, bias = _weights(K, grade, gpu)
    x = _plane(K, 345, grade, gpu)[:2].contiguous()
    buf = torch.full((x.numel() + 64,), 0x7FFF, dtype=torch.int16, device=gpu)
    shifted = buf[64:].view(x.shape)
    shifted.copy_(x)
    assert shifted.data_ptr() == buf.data_ptr() + 128
    want = _direct(x, grade, hw, wp, bias, None, None, grade)
    got = _direct(shifted, grade, hw, wp, bias, None, None, grade)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- 3. bad arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(gpu):
    lib, p = _lib.load(), _lib.ptr
    K, hw, B = 320, (15, 23), 2
    wp, bias = _weights(K, "bf16", gpu)
    x = _plane(K, 345, "bf16", gpu)[:B].contiguous()
    coarse = _coarse(SIZES[hw], "bf16", gpu)[:, :B].contiguous()
    out = torch.full((2, B, 345, 256), 0x7FFF, dtype=torch.int16, device=gpu)
    bf16 = _lib.PH_PREC_BF16

    def call(x_=p(x), wp_=p(wp), bias_=p(bias), out_=p(out), K_=K, prec=bf16, x_prec=bf16, chw=SIZES[hw], wplane=None):
        return lib.ph_fpn_lateral_cl(x_, x_prec, wp_, 256 * K_ if wplane is None else wplane, bias_, p(coarse), chw[0], chw[1], out_,
                                     B, K_, hw[0], hw[1], prec, _lib.stream_ptr())
    misaligned = ctypes.c_void_p(x.data_ptr() + 2)
    for kw in (dict(x_=None), dict(wp_=None), dict(bias_=None), dict(out_=None),      # a NULL pointer
               dict(K_=96), dict(K_=0), dict(wplane=256 * K + 1),                   # K: a multiple of 64; the pack's size
               dict(x_=misaligned),                                                 # X off a 16-byte boundary
               dict(chw=(7, 12)), dict(chw=(8, 11)), dict(chw=(0, 12)),             # sizes outside the rule
               dict(prec=0), dict(prec=99), dict(x_prec=_lib.PH_PREC_SPLIT), dict(x_prec=0)):
        assert call(**kw) == _lib.PH_EINVAL, kw
        assert "ph_fpn_lateral_cl" in Hh.last_error()
    assert call(prec=_lib.PH_PREC_SPLIT) == _lib.PH_EUNSUPPORTED                    # the hi + lo grade keeps the NCHW path
    assert "ph_fpn_lateral_cl" in Hh.last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x7FFF).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out[0] == 0x7FFF).any()) and bool((out[1] == 0x7FFF).all())
    with pytest.raises(_lib.PolyheadError):
        E.fpn_lateral_cl(x, bf16, hw, wp, bias, None, None, out, _lib.PH_PREC_SPLIT)


# ---- 4. the plans -------------------------------------------------------------------------------------------------------------------
_MODS = {}


def _backbone(gpu, grade):
    if ("resnet", grade) not in _MODS:
        with open(os.path.join(Hh.GOLDEN, "resnet_cfg.json")) as f:
            m = registry.build_backbone(json.load(f))
        m.load_state_dict(resnet_cases.fill(m.state_dict()))
        m.eval().to(gpu)
        _MODS[("resnet", grade)] = m.set_precision(grade)
    return _MODS[("resnet", grade)]


def _fpn(gpu, grade):
    """the FPN and the fill of tests/test_gpu_resnet.py test_hand_off_to_the_fpn"""
    if ("fpn", grade) not in _MODS:
        with open(os.path.join(Hh.GOLDEN, "fpn_cfg.json")) as f:
            fpn = registry.NECKS.build(json.load(f))
        fpn.load_state_dict(Hh.seeded_fill({k: tuple(v.shape) for k, v in fpn.state_dict().items()}, 17))
        fpn.eval().to(gpu).set_precision(grade)
        _MODS[("fpn", grade)] = fpn
    return _MODS[("fpn", grade)]


IMAGES = [(2, 3, 64, 96), (1, 3, 40, 72)]             # the second: an odd size at every level


def _image(shape, gpu, n=0):
    return resnet_cases.inputs(n + 1, shape)[n].to(gpu)


def _plan_pair(gpu, grade, shape):
    m = _backbone(gpu, grade)
    args = (shape[0], shape[2], shape[3], m.block_table(), (0, 1, 2, 3), GRADES[grade], torch.float32, gpu)
    return m._pack(gpu), E.ResNetPlan(*args), E.ResNetPlan(*args, stage_planes=True)


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", IMAGES, ids=["64x96", "40x72"])
def test_resnet_plan_with_stage_planes(gpu, grade, shape):
    pk, default, planes = _plan_pair(gpu, grade, shape)
    assert default.planes is None and planes.workgroups == default.workgroups
    assert planes.outs is None                                       # the NCHW stages: allocated when first asked for
    x = _image(shape, gpu)
    want = [o.clone() for o in default.run(x, pk)]
    got = planes.run(x, pk)
    torch.cuda.synchronize()
    assert len(got) == 4
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b)
        p = planes.stage_plane(i)
        c, h, w = planes.stage_shapes[i]
        assert p.dtype == torch.int16 and tuple(p.shape) == (shape[0], h * w, c)
        assert torch.equal(p.view(DTYPES[grade]).float(), b.permute(0, 2, 3, 1).reshape(shape[0], h * w, c))
    # nchw=False: the planes are rewritten, the NCHW stages stay untouched; nothing is allocated
    x2 = _image(shape, gpu, 1)
    want2 = [o.clone() for o in default.run(x2, pk)]
    _poison(list(planes.outs.values()) + list(planes.planes.values()))
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(gpu)["allocation.all.allocated"]
    assert planes.run(x2, pk, nchw=False) is None
    planes.run(x2, pk, nchw=False)
    after = torch.cuda.memory_stats(gpu)["allocation.all.allocated"]
    torch.cuda.synchronize()
    assert after == before
    assert all(bool(o.isnan().all()) for o in planes.outs.values())
    for i, b in enumerate(want2):
        c, h, w = planes.stage_shapes[i]
        assert torch.equal(planes.stage_plane(i).view(DTYPES[grade]).float(), b.permute(0, 2, 3, 1).reshape(shape[0], h * w, c))
    before = torch.cuda.memory_stats(gpu)["allocation.all.allocated"]
    planes.run(x2, pk)                                               # with the NCHW stages too, once they exist
    assert torch.cuda.memory_stats(gpu)["allocation.all.allocated"] == before
    with pytest.raises(_lib.PolyheadError):
        default.run(x, pk, nchw=False)
    with pytest.raises(_lib.PolyheadError):
        default.stage_plane(0)


def _stage_planes(plan):
    return E.StagePlanes([plan.stage_plane(i) for i in range(4)], plan.stage_shapes, plan.prec)


def test_graph_of_the_backbone_and_the_fpn_on_planes(gpu):
    grade, shape = "fp16", IMAGES[1]
    pk, _, rplan = _plan_pair(gpu, grade, shape)
    fpn = _fpn(gpu, grade)
    fpk = fpn._pack(gpu)
    fplan = E.FpnPlan(shape[0], [s[1:] for s in rplan.stage_shapes], [s[0] for s in rplan.stage_shapes], GRADES[grade], gpu)
    static = _image(shape, gpu).clone()

    def run():
        rplan.run(static, pk, nchw=False)
        return fplan.run(_stage_planes(rplan), fpk)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                    # warm-up outside capture (lazy module load)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for n in (1, 2):
        static.copy_(_image(shape, gpu, n))
        _poison(list(outs) + list(rplan.planes.values()))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        _poison(list(outs) + list(rplan.planes.values()))
        eager = run()
        torch.cuda.synchronize()
        assert not any(bool(o.isnan().any()) for o in replayed)
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b), n


def test_fpn_plan_refuses_planes_of_another_geometry(gpu):
    pk, _, rplan = _plan_pair(gpu, "bf16", IMAGES[1])
    fpn = _fpn(gpu, "bf16")
    rplan.run(_image(IMAGES[1], gpu), pk, nchw=False)
    fplan = E.FpnPlan(2, [s[1:] for s in rplan.stage_shapes], [s[0] for s in rplan.stage_shapes], GRADES["bf16"], gpu)
    with pytest.raises(_lib.PolyheadError, match="StagePlanes"):
        fplan.run(_stage_planes(rplan), fpn._pack(gpu))


# ---- 5. the modules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", IMAGES, ids=["64x96", "40x72"])
@pytest.mark.parametrize("bgrade,fgrade", [("bf16", "bf16"), ("fp16", "fp16"), ("bf16", "fp16"), ("bf16", "fp32")])
def test_fpn_of_forward_planes_equals_fpn_of_forward(gpu, bgrade, fgrade, shape):
    """the fp32-grade FPN: the planes go through plan-owned fp32 NCHW stages and the hi + lo laterals"""
    m, fpn = _backbone(gpu, bgrade), _fpn(gpu, fgrade)
    img = _image(shape, gpu)
    want = [o.clone() for o in fpn(m(img))]
    plan = fpn._plan_of(m.forward_planes(img))[0]
    _poison(plan.outs + plan.lat)
    sp = m.forward_planes(img)
    assert isinstance(sp, E.StagePlanes) and len(sp) == 4 and sp.prec == GRADES[bgrade]
    got = fpn(sp)
    torch.cuda.synchronize()
    assert isinstance(got, tuple) and len(got) == 4
    for a, b in zip(got, want):
        assert not bool(b.isnan().any()) and torch.equal(a, b)
    assert (plan.stages_f32 is not None) == (fgrade == "fp32")


@pytest.mark.parametrize("native_neck", [False, True], ids=["python-plan", "native-plan"])
@pytest.mark.parametrize("shape", [IMAGES[0], (1, 3, 60, 92)], ids=["64x96", "60x92"])
def test_the_front_from_image_to_neck(gpu, shape, native_neck):
    """The neck takes pyramids whose levels 2 and 3 are exact halves of level 1 only, and refuses the 40x72 image's (10x18, 5x9, 3x5,
    2x3) on either path; 60x92 is the odd case it does take: stages 15x23, 8x12, 4x6, 2x3 -- 2 Hc - 1 on both axes at level 0."""
    from test_gpu_fpn_handoff import NECK_CFG, _fill
    m, fpn = _backbone(gpu, "bf16"), _fpn(gpu, "bf16")
    if "neck" not in _MODS:
        neck = registry.NECKS.build(dict(NECK_CFG))
        _fill(neck, 11)
        neck.eval().to(gpu)
        neck.set_precision("bf16")
        _MODS["neck"] = neck
    neck = _MODS["neck"]
    img = _image(shape, gpu)
    neck.use_native_plan(native_neck)
    try:
        want = [o.clone() for o in neck(list(fpn(m(img))))]
        got = neck.forward_from_fpn(fpn, m.forward_planes(img))
        torch.cuda.synchronize()
        assert len(got) == 3
        for a, b in zip(got, want):
            assert not bool(b.isnan().any()) and torch.equal(a, b)
    finally:
        neck.use_native_plan(False)


def test_forward_planes_is_the_inference_hand_over_of_the_python_plan(gpu):
    m, fpn = _backbone(gpu, "bf16"), _fpn(gpu, "bf16")
    img = _image(IMAGES[1], gpu)
    sp = m.forward_planes(img)
    with torch.enable_grad():
        m.train()
        try:
            with pytest.raises(_lib.PolyheadError, match="forward_planes"):
                m.forward_planes(img)
        finally:
            m.eval()
        fpn.train()
        try:
            with pytest.raises(_lib.PolyheadError, match="StagePlanes"):
                fpn(sp)
        finally:
            fpn.eval()
    m.use_native_plan(True)
    try:
        with pytest.raises(_lib.PolyheadError, match="native"):
            m.forward_planes(img)
    finally:
        m.use_native_plan(False)
    with pytest.raises(_lib.PolyheadError):
        m.forward_planes(img.cpu())


# ---- 6. the pipeline and the runners ------------------------------------------------------------------------------------------------
H8, W8 = 256, 512                                      # tests/test_gpu_video.py's smallest frame


def _image_pipeline(gpu):
    """test_gpu_video's fp16 cfg3 pipeline with the backbone and the FPN in front"""
    pipe = GV._cfg3_pipeline(gpu, precision="fp16")[0]
    pipe.backbone, pipe.fpn = _backbone(gpu, "fp16"), _fpn(gpu, "fp16")
    return pipe


def _frames(gpu, n, B=1):
    return [t.to(gpu) for t in resnet_cases.inputs(n, (B, 3, H8, W8))]


def _same_maps(got, want):
    assert len(got) == len(want) == 1
    for k in ("sem", "track", "depth"):
        assert got[0][k].dtype == want[0][k].dtype and np.array_equal(got[0][k], want[0][k]), k


def test_extract_feat_is_fpn_of_backbone(gpu):
    pipe = _image_pipeline(gpu)
    img = _frames(gpu, 1)[0]
    want = [o.clone() for o in pipe.fpn(pipe.backbone(img))]
    _poison(list(pipe.fpn(pipe.backbone.forward_planes(img))))
    with torch.enable_grad():                     # the pipeline's front is inference whatever the caller's grad mode
        got = pipe.extract_feat(img)
    torch.cuda.synchronize()
    assert len(got) == 4 and all(o.dtype == torch.float32 for o in got)
    for a, b in zip(got, want):
        assert not bool(b.isnan().any()) and torch.equal(a, b)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_stream_runner_takes_images(gpu, graph):
    pipe = _image_pipeline(gpu)
    frames, meta = _frames(gpu, 2), Hh.img_meta(H8, W8)
    pipe.init_tracker()
    runner = V.VideoStreamRunner(pipe, meta, graph=graph)
    want = [runner.run_one([o.clone() for o in pipe.fpn(pipe.backbone(img))]) for img in frames]
    assert all(np.isfinite(w[0]["depth"]).all() for w in want)
    pipe.init_tracker()
    runner.reset()
    for img, w in zip(frames, want):
        _same_maps(runner.run_one_image(img), w)
    # push_image: the same frames, each result one call late
    pipe.init_tracker()
    runner.reset()
    got = [runner.push_image(img) for img in frames]
    got = [g for g in got if g is not None] + runner.flush()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _same_maps(g, w)
    pipe.init_tracker()
    got = pipe.simple_test_image(frames[0], [meta])
    pipe.init_tracker()
    _same_maps(got, pipe.simple_test(pipe.extract_feat(frames[0]), [meta]))


def test_multi_stream_runner_takes_images(gpu):
    S = 2
    pipe = _image_pipeline(gpu)
    meta = Hh.img_meta(H8, W8)
    steps = _frames(gpu, 2, B=S)
    multi = V.MultiStreamRunner(pipe, meta, S)
    want = [multi.step([o.clone() for o in pipe.fpn(pipe.backbone(imgs))]) for imgs in steps]
    multi.init_tracker()
    for imgs, w in zip(steps, want):
        got = multi.step_images(imgs)
        assert len(got) == S
        for s in range(S):
            _same_maps(got[s], w[s])
    multi.init_tracker()
    got = multi.step_images(steps[0], active=[1, 0])
    assert got[1] is None
    _same_maps(got[0], want[0][0])
