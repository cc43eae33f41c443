"""The backbone on the device (polyphonicformer_amd/resnet.py, csrc/ph_resnet.hip): ph_conv_cl and ph_resnet_stem against float64 on
the 16-bit operands they read, ph_cl_to_nchw exactly, the module against the reference's golden outputs, batch invariance, graph
capture without allocation, re-packing on a changed running statistic, argument errors, and the hand-off to fpn.FPN.

Bound of the kernel tests (the rule of tests/test_gpu_qtrain_edges.py, plus the output's one rounding): every element within
u |ref| + max(4 e_ref, 1e-6) max|ref| of the float64 result, u = the unit round-off of the output format (2^-8 bf16, 2^-11 fp16: one rounding) and e_ref =
helpers.rel_err of torch's fp32 CPU run of the same operands against float64."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
import resnet_cases
from polyphonicformer_amd import _lib, engine as E, registry
from polyphonicformer_amd.pack import pack_b32
import polyphonicformer_amd.fpn as FP  # noqa: F401
import polyphonicformer_amd.resnet as RN

pytestmark = pytest.mark.gpu

GRADES = {"bf16": _lib.PH_PREC_BF16, "fp16": _lib.PH_PREC_F16}
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}     # half an ulp relative to the value: 8 and 11 significant bits
FACTOR, FLOOR = 4.0, 1e-6
GUARD = 4096                      # int16 words behind every output plane that no launch may touch


def _q(t, grade):
    """fp32 tensor -> (its value in the grade as float64, the int16 bits)"""
    r = t.float().half() if grade == "fp16" else t.float().bfloat16()
    return r.double(), r.view(torch.int16)


def _val(bits, grade):
    return bits.view(torch.float16 if grade == "fp16" else torch.bfloat16).double()


def _cl(t):
    """[B, C, H, W] -> channels-last plane [B, H*W, C]"""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous()


def _check(tag, got, ref, ref32, grade):
    e_ref = Hh.rel_err(ref32, ref)
    bound = max(FACTOR * e_ref, FLOOR)
    need = Hh.needed_atol(got, ref, rtol=UNIT[grade])
    print(tag, "needed atol", need, "bound", bound, "e_ref", e_ref, "rel_err", Hh.rel_err(got, ref))
    assert need <= bound, (tag, need, bound)


# ---- ph_conv_cl ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 64, 64), (1, 1, 64, 256), (1, 1, 2048, 512), (1, 1, 512, 2048), (1, 2, 256, 512), (1, 2, 1024, 2048), (3, 1, 64, 64),
          (3, 2, 128, 128), (3, 1, 512, 512), (3, 2, 512, 512)]
BIG = [(1, 1, 64, 256), (3, 1, 64, 64), (3, 2, 128, 128)]
CONV_CASES = [s + g for s in SHAPES for g in ((5, 9), (13, 19))] + [s + (33, 70) for s in BIG] + \
    [s + (6, 10) for s in SHAPES if s[1] == 2]          # stride 2 at an even H as well


# the wider tiles (csrc/ph_resnet.hip rc_geometry: 128 pixels x 64 or 128 channels once a frame has 256 such tiles) at the smallest sizes
# that select them, each with a 1x1, a 3x3 and a stride-2 form and a last pixel tile that is not full: (..., pixels, channels per workgroup)
WIDE_CASES = [(1, 1, 64, 2048, 33, 70, 128, 128), (3, 2, 64, 2048, 66, 141, 128, 128), (1, 2, 128, 2048, 65, 141, 128, 128),
              (3, 1, 64, 64, 128, 257, 128, 64), (3, 2, 128, 192, 160, 274, 128, 64), (1, 2, 64, 64, 257, 513, 128, 64)]


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
@pytest.mark.parametrize("k,s,cin,cout,H,W,tm,tn", [c + (64, 64) for c in CONV_CASES] + WIDE_CASES)
def test_conv_cl_against_float64(gpu, grade, k, s, cin, cout, H, W, tm, tn):
    B = 2
    npx = E.conv_out_size(H, k, s) * E.conv_out_size(W, k, s)
    assert _lib.load().ph_conv_cl_workgroups(k, s, cin, cout, H, W, B) == B * ((npx + tm - 1) // tm) * (cout // tn)    # the tile this case is about
    g = torch.Generator().manual_seed(1000 * k + 100 * s + cin + cout + H + W)
    xq, xb = _q(torch.randn(B, cin, H, W, generator=g), grade)
    wq, wb = _q(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5, grade)
    bias = torch.randn(cout, generator=g) * 0.3
    conv64 = F.conv2d(xq, wq, bias.double(), stride=s, padding=k // 2)
    conv32 = F.conv2d(xq.float(), wq.float(), bias, stride=s, padding=k // 2)
    Ho, Wo = conv64.shape[2:]
    assert (Ho, Wo) == ((H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1) == (E.conv_out_size(H, k, s), E.conv_out_size(W, k, s))
    rq, rb = _q(torch.randn(B, cout, Ho, Wo, generator=g), grade)
    wp = pack_b32(wb.permute(0, 2, 3, 1).reshape(cout, -1)).contiguous().to(gpu)          # k = tap * cin + c
    x_d, r_d, b_d = _cl(xb).to(gpu), _cl(rb).to(gpu), bias.to(gpu)
    assert _lib.load().ph_conv_cl_workgroups(k, s, cin, cout, H, W, B) > 0
    n = B * Ho * Wo * cout
    for with_r in (False, True):
        for relu in (False, True):
            out = torch.full((n + GUARD,), 0x7FFF, dtype=torch.int16, device=gpu)
            E.conv_cl(x_d, wp, b_d, r_d if with_r else None, out, k, s, relu, B, H, W, cin, cout, GRADES[grade])
            o = out.cpu()
            assert bool((o[n:] == 0x7FFF).all()), "the launch wrote behind the plane"
            got = _val(o[:n], grade).reshape(B, Ho, Wo, cout).permute(0, 3, 1, 2)
            ref, ref32 = conv64 + (rq if with_r else 0), conv32 + (rq.float() if with_r else 0)
            if relu:
                ref, ref32 = ref.relu(), ref32.relu()
            _check(f"conv_cl {grade} {(k, s, cin, cout, H, W)} R={with_r} relu={relu}", got, ref, ref32, grade)


def test_conv_cl_argument_errors_launch_nothing(gpu):
    lib = _lib.load()
    x = torch.zeros(1, 30, 128, dtype=torch.int16, device=gpu)
    wp = torch.zeros(128 * 9 * 128, dtype=torch.int16, device=gpu)
    bias = torch.zeros(128, device=gpu)
    out = torch.full((1, 30, 128), 0x1234, dtype=torch.int16, device=gpu)

    def call(k, cin, cout, y=out):
        return lib.ph_conv_cl(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(bias), None, _lib.ptr(y), k, 1, 1, 1, 5, 6, cin, cout, _lib.PH_PREC_BF16,
                              _lib.stream_ptr())
    for args in ((1, 96, 128), (1, 128, 96), (5, 128, 128), (1, 128, 128, None), (1, 32, 128), (1, 128, 4096)):
        assert call(*args) == _lib.PH_EINVAL, args
        assert "ph_conv_cl" in Hh.last_error()
    assert lib.ph_conv_cl_workgroups(5, 1, 128, 128, 5, 6, 1) == _lib.PH_EINVAL
    assert lib.ph_conv_cl_workgroups(3, 3, 128, 128, 5, 6, 1) == _lib.PH_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0x1234).all())
    assert call(1, 128, 128) == 0
    torch.cuda.synchronize()
    assert not bool((out == 0x1234).any())


# ---- ph_resnet_stem --------------------------------------------------------------------------------------------------------------
def _stem(gpu, grade, x, w, bias):
    """(device result as float64 NCHW, float64 reference, fp32 reference) of the stem on image x (fp32 or bf16) with folded w, bias"""
    B, _, H, W = x.shape
    xq, _ = _q(x.float(), grade)                                       # the image through fp32 to the grade, as the kernel stages it
    wq, _ = _q(w, grade)
    ref = F.max_pool2d(F.conv2d(xq, wq, bias.double(), stride=2, padding=3).relu(), 3, 2, 1)
    ref32 = F.max_pool2d(F.conv2d(xq.float(), wq.float(), bias, stride=2, padding=3).relu(), 3, 2, 1)
    Hq, Wq = ref.shape[2:]
    assert (Hq, Wq) == (E.stem_out_size(H), E.stem_out_size(W))
    wp = pack_b32(_q(RN.stem_matrix(wq).float(), grade)[1]).contiguous().to(gpu)      # exact: wq's values are the grade's already
    n = B * Hq * Wq * 64
    out = torch.full((n + GUARD,), 0x7FFF, dtype=torch.int16, device=gpu)
    assert _lib.load().ph_resnet_stem_workgroups(H, W, B) > 0
    E.resnet_stem(x.contiguous().to(gpu), wp, bias.to(gpu), out, GRADES[grade])
    o = out.cpu()
    assert bool((o[n:] == 0x7FFF).all()), "the launch wrote behind the plane"
    return _val(o[:n], grade).reshape(B, Hq, Wq, 64).permute(0, 3, 1, 2), ref, ref32


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(40, 72), (37, 75), (64, 130)])
def test_stem_against_float64(gpu, grade, dtype, H, W):
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(2, 3, H, W, generator=g).to(dtype)
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    bias = torch.randn(64, generator=g) * 0.3
    got, ref, ref32 = _stem(gpu, grade, x, w, bias)
    _check(f"stem {grade} {dtype} {(H, W)}", got, ref, ref32, grade)


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_stem_pool_takes_entries_inside_the_conv_map_only(gpu, grade):
    """MaxPool2d(3, 2, 1) has no window that lies wholly in the padding -- its centre is always inside the map -- so the case that tells
    padding from data is the border window, part in and part out.  The pool's border windows reach one row / column outside the conv map.  A conv value computed THERE from the zero-padded image is
    no entry of the window (MaxPool2d pads with -inf, and after the ReLU 0 is as good): output channel 0 has one tap, (6, 6) of image
    channel 0, so conv row -1 would read image row 1 and conv column -1 image column 1, which no conv pixel inside the map reads (those
    read odd rows and columns from 3 on); output channel 1 has tap (0, 0) of image channel 1, so conv row Hc would read image row
    2 Hc - 3, two rows below the last one a conv pixel inside the map reads.  Those rows and that column hold 50, the rest is small."""
    H, W = 37, 75
    Hc = (H - 1) // 2 + 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, H, W, generator=g) * 0.5
    x[:, 0, 1, :] = 50.0
    x[:, 0, :, 1] = 50.0
    x[:, 1, 2 * Hc - 3, :] = 50.0
    w = torch.zeros(64, 3, 7, 7)
    w[0, 0, 6, 6] = 1.0
    w[1, 1, 0, 0] = 1.0
    w[2:] = torch.randn(62, 3, 7, 7, generator=g) * 0.1
    bias = torch.full((64,), 0.25)
    got, ref, ref32 = _stem(gpu, grade, x, w, bias)
    assert float(ref[:, :2].max()) < 10          # the reference never sees the 50s in channels 0 and 1
    _check(f"stem border {grade}", got, ref, ref32, grade)
    assert float(got[:, :2].max()) < 10


def test_stem_argument_errors_launch_nothing(gpu):
    lib = _lib.load()
    x = torch.zeros(1, 3, 16, 16, device=gpu)
    wp = torch.zeros(64 * RN.STEM_K, dtype=torch.int16, device=gpu)
    bias = torch.zeros(64, device=gpu)
    out = torch.full((1, 16, 64), 0x1234, dtype=torch.int16, device=gpu)
    call = lambda y, dt, prec: lib.ph_resnet_stem(_lib.ptr(x), dt, _lib.ptr(wp), _lib.ptr(bias), y, 1, 16, 16, prec, _lib.stream_ptr())
    assert call(None, _lib.PH_OUT_F32, _lib.PH_PREC_BF16) == _lib.PH_EINVAL
    assert call(_lib.ptr(out), _lib.PH_OUT_F16, _lib.PH_PREC_BF16) == _lib.PH_EINVAL
    assert call(_lib.ptr(out), _lib.PH_OUT_F32, _lib.PH_PREC_SPLIT) == _lib.PH_EINVAL
    assert "ph_resnet_stem" in Hh.last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x1234).all())


# ---- ph_cl_to_nchw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grade", ["bf16", "fp16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C_", [256, 2048])
@pytest.mark.parametrize("HW", [6, 45, 4100])
def test_cl_to_nchw_is_exact(gpu, grade, dtype, C_, HW):
    B = 2
    g = torch.Generator().manual_seed(HW + C_)
    src = (torch.randn(B, HW, C_, generator=g) * 3).to(torch.float16 if grade == "fp16" else torch.bfloat16)
    ref = src.float().permute(0, 2, 1).to(dtype).contiguous()            # each value through fp32 to the hand-off dtype
    out = torch.full((B * C_ * HW + GUARD,), float("nan"), dtype=dtype, device=gpu)
    assert _lib.load().ph_cl_to_nchw_workgroups(B, HW, C_) == B * ((HW + 63) // 64) * (C_ // 64)
    E.cl_to_nchw(src.view(torch.int16).to(gpu), out, B, HW, C_, GRADES[grade])
    o = out.cpu()
    assert bool(o[B * C_ * HW:].isnan().all()), "the launch wrote behind the tensor"
    assert torch.equal(o[:B * C_ * HW].reshape(B, C_, HW), ref)


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _golden():
    return Hh.load_golden("resnet.npz")


def _module(gpu, grade, seed_shift=0.0):
    with open(os.path.join(Hh.GOLDEN, "resnet_cfg.json")) as f:
        m = registry.build_backbone(json.load(f))
    sd = resnet_cases.fill(m.state_dict())
    if seed_shift:
        sd["layer2.1.bn2.running_mean"] = sd["layer2.1.bn2.running_mean"] + seed_shift
    m.load_state_dict(sd)
    m.eval().to(gpu)
    return m.set_precision(grade)


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_module_against_reference_golden(gpu, grade):
    """Measured on an MI355X: see the figures beside the emulated ones in DESIGN.md 7f9."""
    g = _golden()
    m = _module(gpu, grade)
    with torch.no_grad():
        outs = m(resnet_cases.inputs(1)[0].to(gpu))
    bound = 2 * float(g[f"emu_err_{grade}"])
    assert len(outs) == 4
    for i, o in enumerate(outs):
        ref = torch.from_numpy(g[f"out{i}"])
        assert o.dtype == torch.float32 and tuple(o.shape) == tuple(ref.shape)
        e = Hh.rel_err(o.cpu(), ref)
        print("resnet", grade, "stage", i, e, "bound", bound)
        assert e <= bound, (i, e, bound)


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_batch_invariance(gpu, grade):
    m = _module(gpu, grade)
    x = resnet_cases.inputs(1, (3, 3, 64, 96))[0].to(gpu)
    with torch.no_grad():
        o3 = [o.clone() for o in m(x)]
        for b in range(3):
            o1 = m(x[b:b + 1].contiguous())
            for a, c in zip(o3, o1):
                assert torch.equal(a[b:b + 1], c)


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_launch_only(gpu, grade):
    m = _module(gpu, grade)
    x = resnet_cases.inputs(1, (2, 3, 40, 72))[0].to(gpu)
    with torch.no_grad():
        eager = [o.clone() for o in m(x)]
    plan, pk, xin = m._plan_of(x)
    assert all(n > 0 for _, n in plan.workgroups) and len(plan.workgroups) == 1 + 52 + 4
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    plan.run(xin, pk)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before, "run() allocated"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run(xin, pk)
    for o in plan.outs.values():
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for i, a in enumerate(eager):
        assert torch.equal(a, plan.outs[i])


def test_repack_on_a_changed_running_statistic(gpu):
    m = _module(gpu, "bf16")
    x = resnet_cases.inputs(1)[0].to(gpu)
    with torch.no_grad():
        first = [o.clone() for o in m(x)]
        m.layer2[1].bn2.running_mean.add_(0.5)
        second = [o.clone() for o in m(x)]
        want = _module(gpu, "bf16", seed_shift=0.5)(x)
    assert torch.equal(first[0], second[0])                              # stage 0 lies before the edited layer
    for i in (1, 2, 3):
        assert not torch.equal(first[i], second[i]) and torch.equal(second[i], want[i])


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_stage_dtypes_and_out_indices(gpu, grade):
    m = _module(gpu, grade)
    x = resnet_cases.inputs(1)[0].to(gpu)
    with torch.no_grad():
        f32 = [o.clone() for o in m(x)]
        own = torch.bfloat16 if grade == "bf16" else torch.float16
        m.set_stage_dtype(own)
        o16 = [o.clone() for o in m(x)]
        m.set_stage_dtype(torch.float32)
        m.out_indices = (1, 3)                                           # a live module: the plan follows
        sub = m(x)
    for a, b in zip(f32, o16):
        assert b.dtype == own and torch.equal(a, b.float())              # the plane's own format: the same values
    assert len(sub) == 2 and torch.equal(sub[0], f32[1]) and torch.equal(sub[1], f32[3])


def test_hand_off_to_the_fpn(gpu):
    """fpn.FPN in its bf16 grade rounds the stages to bf16 in the lateral either way: bf16 NCHW stages give the levels of the fp32 ones"""
    m = _module(gpu, "bf16")
    fpn = registry.NECKS.build(json.load(open(os.path.join(Hh.GOLDEN, "fpn_cfg.json"))))
    fpn.load_state_dict(Hh.seeded_fill({k: tuple(v.shape) for k, v in fpn.state_dict().items()}, 17))
    fpn.eval().to(gpu).set_precision("bf16")
    x = resnet_cases.inputs(1, (2, 3, 64, 96))[0].to(gpu)
    with torch.no_grad():
        lv32 = [o.clone() for o in fpn(m(x))]
        m.set_stage_dtype(torch.bfloat16)
        stages = m(x)
        assert all(s.dtype == torch.bfloat16 for s in stages)
        lv16 = fpn(stages)
    for a, b in zip(lv32, lv16):
        assert torch.equal(a, b)
