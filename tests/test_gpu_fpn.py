"""The FPN on the device (polyphonicformer_amd/fpn.py, csrc/ph_fpn.hip): the lateral kernel against float64 on the operands it
sees, the output tail against torch, the module against the reference's golden outputs, batch invariance, graph capture, and the
hand-over to SemanticFPNWrapper."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
from polyphonicformer_amd.pack import pack_b32
from polyphonicformer_amd.registry import NECKS
import polyphonicformer_amd.fpn as FP  # noqa: F401
import polyphonicformer_amd.semantic_fpn as SF  # noqa: F401

pytestmark = pytest.mark.gpu

GRADES = {"bf16": _lib.PH_PREC_BF16, "fp16": _lib.PH_PREC_F16, "fp32": _lib.PH_PREC_SPLIT}
# unit round-off of the output format; the bound of test_gpu_neck.py::test_conv_nhwc for fp32 accumulation of exact 16-bit products
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -16}
ACC = {"bf16": 1e-5, "fp16": 1e-5, "fp32": 5e-5}


def _decode(p, grade):
    """int16 planes [P, ...] -> float64"""
    if grade == "fp16":
        return p[0].view(torch.float16).double()
    return sum((p[i].to(torch.int32) << 16).view(torch.float32).double() for i in range(p.shape[0]))


def _planes(t64, grade):
    return E._planes_of(t64, 2 if grade == "fp32" else 1, grade == "fp16")


def _lateral_operands(K, H, W, B, coarse_hw, dtype, grade, gpu, seed=7):
    g = torch.Generator().manual_seed(seed + K + H + W)
    x = torch.randn(B, K, H, W, generator=g).to(dtype)
    w = torch.randn(256, K, generator=g) * 0.05
    bias = torch.randn(256, generator=g) * 0.1
    wpl = _planes(w.double(), grade)                                             # [P][256][K]
    wp = torch.stack([pack_b32(wpl[p]) for p in range(wpl.shape[0])], 0).contiguous().to(gpu)
    cpl = None
    if coarse_hw is not None:
        cpl = _planes(torch.randn(B, coarse_hw[0] * coarse_hw[1], 256, generator=g).double(), grade)   # [P][B][HcWc][256]
    # float64 on what the kernel sees: x through fp32 to the grade, the weight planes, the coarse planes
    xq = _decode(_planes(x.double(), grade), grade)
    ref = torch.einsum("nk,bkhw->bnhw", _decode(wpl, grade), xq) + bias.double()[None, :, None, None]
    if cpl is not None:
        cq = _decode(cpl, grade).reshape(B, coarse_hw[0], coarse_hw[1], 256).permute(0, 3, 1, 2)
        ref = ref + F.interpolate(cq, size=(H, W), mode="nearest")
    return x.to(gpu), wp, bias.to(gpu), (cpl.to(gpu) if cpl is not None else None), ref


LATERAL_CASES = [(2048, 2, 3, 2, None, torch.float32), (1024, 4, 5, 2, (2, 3), torch.float32), (512, 7, 10, 1, (4, 5), torch.float32),
                 (256, 13, 19, 2, (7, 10), torch.float32), (256, 6, 70, 2, (3, 35), torch.float32),
                 (512, 16, 80, 3, (8, 40), torch.bfloat16), (64, 5, 64, 1, None, torch.float16)]


# paths the cases above do not take: a K that ends in a partial chunk behind a full one (320 = 256 + 64), the largest K, and
# 16-bit stages whose H * W is no multiple of 4 (element loads instead of 8-byte ones)
LATERAL_MORE = [(320, 5, 7, 1, (3, 4), torch.bfloat16), (4096, 3, 3, 2, None, torch.float16), (448, 9, 8, 1, (5, 4), torch.float32)]


@pytest.mark.parametrize("grade", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("K,H,W,B,coarse_hw,dtype", LATERAL_CASES + LATERAL_MORE)
def test_lateral_against_float64(gpu, grade, K, H, W, B, coarse_hw, dtype):
    x, wp, bias, cpl, ref = _lateral_operands(K, H, W, B, coarse_hw, dtype, grade, gpu)
    P = 2 if grade == "fp32" else 1
    out = torch.full((P, B, H * W, 256), 0x7FFF, dtype=torch.int16, device=gpu)
    E.fpn_lateral(x, wp, bias, cpl, coarse_hw, out, GRADES[grade])
    got = _decode(out.cpu(), grade).reshape(B, H, W, 256).permute(0, 3, 1, 2)
    need = Hh.needed_atol(got, ref, rtol=UNIT[grade])
    print("lateral", grade, (K, H, W, B, coarse_hw, dtype), "needed atol", need, "rel_err", Hh.rel_err(got, ref))
    assert need < ACC[grade]


@pytest.mark.parametrize("grade", ["bf16", "fp32"])
def test_lateral_refuses_bad_arguments(gpu, grade):
    lib = _lib.load()
    P = 2 if grade == "fp32" else 1
    x, wp, bias, cpl, _ = _lateral_operands(256, 6, 10, 1, (3, 5), torch.float32, grade, gpu)
    out = torch.full((P, 1, 60, 256), 0x1234, dtype=torch.int16, device=gpu)

    def call(K, H, W, Hc, Wc, wplane):
        return lib.ph_fpn_lateral(_lib.ptr(x), _lib.PH_OUT_F32, _lib.ptr(wp), wplane, _lib.ptr(bias), _lib.ptr(cpl), Hc, Wc, _lib.ptr(out),
                                  1, K, H, W, GRADES[grade], _lib.stream_ptr())
    for args in ((256, 6, 10, 2, 5, 256 * 256),        # H = 3 Hc
                 (256, 6, 10, 3, 4, 256 * 256),        # W = 2 Wc + 2
                 (256, 6, 10, 4, 5, 256 * 256),        # H = 2 Hc - 2
                 (224, 6, 10, 3, 5, 256 * 224),        # K no multiple of 64
                 (32, 6, 10, 3, 5, 256 * 32)):         # K below 64
        assert call(*args) == _lib.PH_EINVAL, args
        assert "ph_fpn_lateral" in Hh.last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x1234).all())
    assert call(256, 6, 10, 3, 5, 256 * 256) == 0
    torch.cuda.synchronize()
    assert not bool((out == 0x1234).all())


@pytest.mark.parametrize("H,W", [(2, 3), (6, 70), (13, 19)])
def test_output_tail(gpu, H, W):
    g = torch.Generator().manual_seed(H * W)
    y = torch.randn(2, H * W, 256, generator=g)
    bias = torch.randn(256, generator=g)
    out = torch.full((2, 256, H, W), float("nan"), device=gpu)
    E.fpn_output(y.to(gpu), bias.to(gpu), out, 2, H * W)
    ref = (y + bias).reshape(2, H, W, 256).permute(0, 3, 1, 2)
    assert Hh.rel_err(out.cpu(), ref) < 1e-6


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _golden():
    g = Hh.load_golden("fpn.npz")
    keys = json.loads(bytes(g["keys_json"]).decode())
    return g, Hh.seeded_fill({k: tuple(v) for k, v in keys.items()}, 5)


def _module(gpu, grade, sd=None):
    cfg = json.load(open(os.path.join(Hh.GOLDEN, "fpn_cfg.json")))
    m = NECKS.build(cfg)
    if sd is None:
        m.load_state_dict(Hh.seeded_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, 17))
    else:
        m.load_state_dict(sd)
    m.eval().to(gpu)
    m.set_precision(grade)
    return m


def _inputs(sizes, B, seed=3, channels=(256, 512, 1024, 2048)):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, h, w, generator=g).relu() for c, (h, w) in zip(channels, sizes)]


@pytest.mark.parametrize("grade", ["bf16", "fp16", "fp32"])
def test_module_against_reference_golden(gpu, grade):
    g, sd = _golden()
    m = _module(gpu, grade, sd)
    feats = _inputs(((13, 19), (7, 10), (4, 5), (2, 3)), 2)
    outs = m([f.to(gpu) for f in feats])
    bound = 2 * float(g[f"emu_err_{grade}"])
    if grade == "fp32":
        bound = max(bound, 5e-5)
    assert len(outs) == 4
    for i, o in enumerate(outs):
        ref = torch.from_numpy(g[f"out{i}"])
        assert o.dtype == torch.float32 and tuple(o.shape) == tuple(ref.shape)
        e = Hh.rel_err(o.cpu(), ref)
        print("fpn", grade, "level", i, e, "bound", bound)
        assert e < bound, (i, e, bound)


@pytest.mark.parametrize("grade", ["bf16", "fp16", "fp32"])
def test_batch_invariance(gpu, grade):
    m = _module(gpu, grade)
    feats = [f.to(gpu) for f in _inputs(((16, 80), (8, 40), (4, 20), (2, 10)), 3, seed=9)]
    o3 = [o.clone() for o in m(feats)]
    o1 = m([f[:1].contiguous() for f in feats])
    for a, b in zip(o3, o1):
        assert torch.equal(a[:1], b)


@pytest.mark.parametrize("grade", ["bf16", "fp32"])
def test_launch_only(gpu, grade):
    m = _module(gpu, grade)
    sizes = ((13, 19), (7, 10), (4, 5), (2, 3))
    feats = [f.to(gpu) for f in _inputs(sizes, 2, seed=4)]
    eager = [o.clone() for o in m(feats)]
    again = [o.clone() for o in m(feats)]
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    plan, pk = next(iter(m._plans.values())), m._pack(gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run(feats, pk)
    for o in plan.outs:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, plan.outs):
        assert torch.equal(a, b)
    # other weights after a first forward: the pack follows the parameter versions
    other = _module(gpu, grade, _golden()[1])
    want = [o.clone() for o in other(feats)]
    m.load_state_dict(other.state_dict())
    got = m(feats)
    for a, b, c in zip(got, want, eager):
        assert torch.equal(a, b) and not torch.equal(a, c)


@pytest.mark.parametrize("grade", ["fp16", "fp32"])
def test_hand_over_to_the_neck(gpu, grade):
    """the neck's own contract (test_gpu_neck.py::test_neck_vs_reference_golden: 1e-3 in these grades) holds on the device FPN's levels.
    Measured on an MI355X: 8.8e-4 / 9.96e-4 / 8.8e-4 on the three maps in the fp16 grade (the FPN's own 5.5e-4 is the rounding of
    its inputs, weights and lateral sums to fp16, tools/gen_golden_fpn.py), 1.0e-5 / 1.2e-5 / 9.0e-6 in the fp32 grade."""
    keys = json.load(open(os.path.join(Hh.GOLDEN, "neck_state_keys.json")))["full"]
    neck = NECKS.build(dict(type="SemanticFPNWrapper", in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
                            upsample_times=2, positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                            cat_coors=False, cat_coors_level=3, fuse_by_cat=False, return_list=False, num_aux_convs=2,
                            norm_cfg=dict(type="GN", num_groups=32, requires_grad=True)))
    neck.load_state_dict(Hh.seeded_fill({k: tuple(v) for k, v in keys.items()}, 31))
    neck.eval().to(gpu)
    neck.set_precision(grade)
    sd = _golden()[1]
    m = _module(gpu, grade, sd)
    cpu = _inputs(((16, 32), (8, 16), (4, 8), (2, 4)), 1, seed=6)
    # the torch FPN (fpn.py:157-179) in float64, handed over as fp32: the same bits on every host
    d = {k: v.double() for k, v in sd.items()}
    lat = [F.conv2d(cpu[i].double(), d[f"lateral_convs.{i}.conv.weight"], d[f"lateral_convs.{i}.conv.bias"]) for i in range(4)]
    for i in (3, 2, 1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    ref_levels = [F.conv2d(lat[i], d[f"fpn_convs.{i}.conv.weight"], d[f"fpn_convs.{i}.conv.bias"], padding=1).float().to(gpu) for i in range(4)]
    want = [o.clone() for o in neck(ref_levels)]
    got = neck(list(m([f.to(gpu) for f in cpu])))
    for a, b in zip(got, want):
        e = Hh.rel_err(a.cpu(), b.cpu())
        print("hand-over", grade, e)
        assert e < 1e-3
