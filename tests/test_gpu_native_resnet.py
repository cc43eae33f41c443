"""GPU: the native backbone plan (include/polyhead.h ph_resnet_pack, ph_resnet_plan_*; engine.NativeResNetPlan; resnet.ResNet.
use_native_plan; examples/image_c).  The device fold-and-pack is compared byte for byte with resnet.ResNet._pack (host torch in float64),
the plan's stages bit for bit with engine.ResNetPlan, and the C++ program's files byte for byte with the Python chain on the same
native packs.  No tolerance appears: both sides issue the same launches.  The one bound is the golden's, restated from
tests/test_gpu_resnet.py: 2 x the emulated error per grade."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import bench
import helpers as Hh
import resnet_cases
from polyphonicformer_amd import _lib, engine as E, registry
from polyphonicformer_amd import build as BLD
from polyphonicformer_amd.pack import pack_b32
from polyphonicformer_amd.registry import ConfigDict
import polyphonicformer_amd.resnet as RN
import test_gpu_fpn_handoff as TH
import test_gpu_native_neck as TN

pytestmark = pytest.mark.gpu

GRADES = {"bf16": _lib.PH_PREC_BF16, "fp16": _lib.PH_PREC_F16}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SIZES = {"odd": (1, 3, 40, 72), "even": (2, 3, 64, 128)}      # stages 10x18, 5x9, 3x5, 2x3 (odd at every level) / 16x32 .. 2x4


@pytest.fixture(autouse=True)
def _inference(monkeypatch):
    Hh.clear_plan_knobs(monkeypatch)
    with torch.no_grad():
        yield



def _poison(ts):
    for t in ts:
        t.fill_(float("nan"))


# ---- modules and packs, built once ----------------------------------------------------------------------------------------------------
_MODS, _PACKS = {}, {}


def _wide(sd):
    """resnet_cases.fill with the fold away from the comfortable range: running_var log-uniform over [1e-6, 1e4] with both ends present,
    and one gamma in sixteen negative"""
    g = torch.Generator().manual_seed(29)
    for k in sorted(sd):
        if k.endswith("running_var"):
            v = 10.0 ** (torch.rand(sd[k].shape, generator=g) * 10.0 - 6.0)
            v[0], v[1] = 1e-6, 1e4
            sd[k] = v
        elif k.endswith(".weight") and sd[k].dim() == 1:               # a norm's gamma (the convolutions' weights are 4-D)
            sd[k] = torch.where(torch.rand(sd[k].shape, generator=g) < 1 / 16, -sd[k], sd[k])
    return sd


def _module(grade, depth=50, fill="golden", eps=1e-5):
    key = (grade, depth, fill, eps)
    if key not in _MODS:
        with open(os.path.join(Hh.GOLDEN, "resnet_cfg.json")) as f:
            m = registry.build_backbone(dict(json.load(f), depth=depth))
        sd = resnet_cases.fill(m.state_dict())
        if fill == "wide":
            sd = _wide(sd)
            assert any(bool((v < 0).any()) for k, v in sd.items() if v.dim() == 1 and k.endswith(".weight"))
        m.load_state_dict(sd)
        for b in m.modules():
            if isinstance(b, torch.nn.BatchNorm2d):
                b.eps = eps
        m.eval().to("cuda:0")
        _MODS[key] = m.set_precision(grade)
    return _MODS[key]


def _native_pack(grade, depth=50, fill="golden", eps=1e-5):
    key = (grade, depth, fill, eps)
    if key not in _PACKS:
        cfg = E.native_resnet_cfg(1, 40, 72, depth, grade, eps=eps)
        _PACKS[key] = E.native_resnet_pack(_module(*key), cfg, torch.device("cuda:0"))
    return _PACKS[key]


def _convs_of(pk):
    """[(name, (wp, bias))] of a pack dict in state_dict order"""
    out = [("stem", pk["stem"])]
    for si, stage in enumerate(pk["blocks"]):
        for j, blk in enumerate(stage):
            out += [(f"layer{si + 1}.{j}.{n}", blk[n]) for n in ("conv1", "conv2", "conv3", "downsample") if blk[n] is not None]
    return out


def _image(size, dtype, gpu, seed=0):
    x = resnet_cases.inputs(1 + seed, SIZES[size] if isinstance(size, str) else size)[seed]
    return x.to(dtype).to(gpu).contiguous()


# ---- 1. packing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill,eps", [("golden", 1e-5), ("golden", 1e-3), ("wide", 1e-5)])
@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_packing_is_the_module_pack_byte_for_byte(gpu, grade, fill, eps):
    """every piece of ph_resnet_pack's buffer against ResNet._pack's tensor: the weights as int16, the biases as their fp32 bits.  A
    packer that skipped the fold, or folded in fp32, differs in a large part of them (asserted for the wide fill)"""
    m = _module(grade, 50, fill, eps)
    pack = _native_pack(grade, 50, fill, eps)
    assert pack.eps == eps and pack.blob.numel() == _lib.load().ph_resnet_pack_bytes(C.byref(pack.cfg))
    again = E.native_resnet_pack(m.state_dict(), pack.cfg, gpu)      # a state_dict packs to the same bytes
    assert torch.equal(pack.blob, again.blob)
    ref = m._pack(gpu)
    got_c, ref_c = _convs_of(pack.pk), _convs_of(ref)
    assert [n for n, _ in got_c] == [n for n, _ in ref_c] and len(got_c) == 53 == pack.layout.nconvs
    covered = torch.zeros(pack.blob.numel(), dtype=torch.bool, device=gpu)
    for c, ((name, (gw, gb)), (_, (rw, rb))) in enumerate(zip(got_c, ref_c)):
        assert gw.dtype == rw.dtype == torch.int16 and gb.dtype == rb.dtype == torch.float32, name
        assert tuple(gw.shape) == tuple(rw.shape) and tuple(gb.shape) == tuple(rb.shape), name
        bad = int((gw != rw).sum())
        assert bad == 0, (name, "W", bad, gw.numel())
        assert torch.equal(gb.view(torch.int32), rb.view(torch.int32)), (name, "b")
        for piece in (2 * c, 2 * c + 1):
            off, nb = int(pack.layout.offset[piece]), int(pack.layout.bytes[piece])
            assert not bool(covered[off:off + nb].any())
            covered[off:off + nb] = True
    assert int(pack.blob[~covered].ne(0).sum()) == 0              # what lies between the pieces is zero
    if fill == "wide":
        convs = [(m.conv1, RN.stem_matrix)] + [(cv, None) for name in m.res_layers for b in getattr(m, name)
                                               for cv in (b.conv1, b.conv2, b.conv3) + ((b.downsample[0],) if b.downsample is not None else ())]
        differ = total = 0
        for (conv, matrix), (_, (gw, _)) in zip(convs, got_c):
            w = conv.weight.detach().cpu().double()
            w2 = matrix(w) if matrix else w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
            plain = pack_b32(E._planes_of(w2, 1, grade == "fp16")[0])
            differ, total = differ + int((plain != gw.cpu()).sum()), total + plain.numel()
        print("wide fill: 16-bit weights that the fold changes:", differ, "of", total)
        assert differ >= total // 4


def test_pack_writes_exactly_its_bytes(gpu):
    """every piece is a multiple of 256 bytes at the shipped widths, so the pack holds no padding of its own; a buffer full of ones
    holds exactly the pack afterwards, the guards on both sides untouched"""
    lib = _lib.load()
    want = _native_pack("bf16")
    cfg, n = want.cfg, want.blob.numel()
    assert sum(want.layout.bytes) == n
    nparams = lib.ph_resnet_nparams(C.byref(cfg))
    params, ptrs = E._gather_params(_module("bf16"), gpu, nparams, lambda i: lib.ph_resnet_param_name(C.byref(cfg), i),
                                    lambda i: lib.ph_resnet_param_numel(C.byref(cfg), i))
    G = 4096
    buf = torch.full((n + 2 * G,), 0xFF, dtype=torch.uint8, device=gpu)
    _lib.check(lib.ph_resnet_pack(C.byref(cfg), ptrs, C.c_void_p(buf.data_ptr() + G), _lib.stream_ptr()), "ph_resnet_pack")
    torch.cuda.synchronize()
    assert torch.equal(buf[G:G + n], want.blob) and bool((buf[:G] == 0xFF).all()) and bool((buf[G + n:] == 0xFF).all())
    assert lib.ph_resnet_pack(C.byref(cfg), ptrs, C.c_void_p(buf.data_ptr() + G + 16), _lib.stream_ptr()) == _lib.PH_EINVAL
    assert "256-byte aligned" in Hh.last_error()


# ---- 2. bit identity with engine.ResNetPlan -------------------------------------------------------------------------------------------
def _python_stages(m, x, pk, stage_dtype, out_indices=(0, 1, 2, 3)):
    B, _, H, W = x.shape
    plan = E.ResNetPlan(B, H, W, m.block_table(), out_indices, GRADES[m.precision], stage_dtype, x.device)
    return plan, [o.clone() for o in plan.run(x, pk)]


@pytest.mark.parametrize("grade", ["bf16", "fp16"])
@pytest.mark.parametrize("stage_dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("x_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("size", ["odd", "even"])
def test_stages_equal_the_python_plan(gpu, size, x_dtype, stage_dtype, grade):
    m, pack = _module(grade), _native_pack(grade)
    x = _image(size, DTYPES[x_dtype], gpu)
    B, _, H, W = x.shape
    pyplan, want = _python_stages(m, x, pack.pk, DTYPES[stage_dtype])           # the same pack under both plans
    plan = E.NativeResNetPlan(pack, B, H, W, gpu, DTYPES[stage_dtype])
    assert plan.geometry.prec == GRADES[grade] and plan.geometry.launches == len(pyplan.workgroups) == 57
    assert plan.stage_shapes == pyplan.stage_shapes
    got = plan.run(x)
    _poison(got)
    got = plan.run(x, pack.pk)
    torch.cuda.synchronize()
    assert len(got) == 4
    for a, b in zip(got, want):
        assert a.dtype == DTYPES[stage_dtype] and torch.equal(a, b)
    # and the module's own pack gives the Python plan the same stages: the two packs are interchangeable
    for a, b in zip(pyplan.run(x, m._pack(gpu)), want):
        assert torch.equal(a, b)
    with pytest.raises(_lib.PolyheadError, match="x must be"):
        plan.run(x.double())
    with pytest.raises(_lib.PolyheadError, match="the pack it was created with"):
        plan.run(x, m._pack(gpu))


@pytest.mark.parametrize("out_indices", [(1, 3), (0, 1)])
def test_out_mask_follows_out_indices(gpu, out_indices):
    m, pack = _module("bf16"), _native_pack("bf16")
    x = _image("odd", torch.float32, gpu)
    pyplan, want = _python_stages(m, x, pack.pk, torch.float32, out_indices)
    plan = E.NativeResNetPlan(pack, 1, 40, 72, gpu, out_indices=out_indices)
    assert plan.geometry.launches == 1 + plan.geometry.nconvs + 2
    assert plan.geometry.nconvs == (52 if 3 in out_indices else 23) and sorted(plan.outs) == list(out_indices)
    got = plan.run(x)
    torch.cuda.synchronize()
    assert len(got) == 2
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert Hh.graph_kernel_nodes(lambda: plan.run(x)) == Hh.graph_kernel_nodes(lambda: pyplan.run(x, pack.pk))


def test_depth_101(gpu):
    m, pack = _module("fp16", 101), _native_pack("fp16", 101)
    assert pack.layout.nconvs == 104 and [len(s) for s in pack.pk["blocks"]] == [3, 4, 23, 3]
    for (name, (gw, gb)), (_, (rw, rb)) in zip(_convs_of(pack.pk), _convs_of(m._pack(gpu))):
        assert torch.equal(gw, rw) and torch.equal(gb.view(torch.int32), rb.view(torch.int32)), name
    x = _image("odd", torch.float32, gpu)
    pyplan, want = _python_stages(m, x, pack.pk, torch.float32)
    plan = E.NativeResNetPlan(pack, 1, 40, 72, gpu)
    assert plan.geometry.launches == len(pyplan.workgroups) == 1 + 103 + 4
    got = plan.run(x)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_stem_and_stages_one_by_one(gpu):
    pack = _native_pack("fp16")
    x = _image("even", torch.bfloat16, gpu)
    whole = E.NativeResNetPlan(pack, 2, 64, 128, gpu, torch.float16)
    want = [o.clone() for o in whole.run(x)]
    plan = E.NativeResNetPlan(pack, 2, 64, 128, gpu, torch.float16)
    plan.workspace.fill_(0xFF)
    _poison(plan.outs.values())
    plan.run_stem(x, pack.pk)
    for si in range(4):
        plan.run_stage(si, pack.pk)
    torch.cuda.synchronize()
    for i, b in enumerate(want):
        assert torch.equal(plan.outs[i], b)


# ---- 3. the golden --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grade", ["bf16", "fp16"])
def test_native_plan_against_reference_golden(gpu, grade):
    g = Hh.load_golden("resnet.npz")
    x = resnet_cases.inputs(1)[0].to(gpu)
    outs = E.NativeResNetPlan(_native_pack(grade), 1, 40, 72, gpu).run(x)
    bound = 2 * float(g[f"emu_err_{grade}"])                    # tests/test_gpu_resnet.py's bound on the Python plan
    assert len(outs) == 4
    for i, o in enumerate(outs):
        ref = torch.from_numpy(g[f"out{i}"])
        assert o.dtype == torch.float32 and tuple(o.shape) == tuple(ref.shape)
        e = Hh.rel_err(o.cpu(), ref)
        print("native resnet", grade, "stage", i, e, "bound", bound)
        assert e <= bound, (i, e, bound)


# ---- 4. guarded buffers ---------------------------------------------------------------------------------------------------------------
def test_workspace_and_stages_stay_inside_their_bounds(gpu):
    """workspace and every stage between 4 KiB canaries: intact after a run; a workspace one byte short is refused, nothing launched"""
    lib = _lib.load()
    pack = _native_pack("bf16")
    B, H, W, G = 2, 40, 72, 4096
    cfg = E.native_resnet_cfg(B, H, W, 50, "bf16", torch.float32, torch.bfloat16)
    geo = _lib.ResNetGeometry()
    _lib.check(lib.ph_resnet_geometry_of(C.byref(cfg), C.byref(geo)), "ph_resnet_geometry_of")
    nws = lib.ph_resnet_plan_workspace_bytes(C.byref(cfg))
    guarded = lambda n: torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device=gpu)
    ws = guarded(nws)
    sizes = [B * geo.c[i] * geo.h[i] * geo.w[i] * 2 for i in range(4)]
    stages = [guarded(n) for n in sizes]
    h = C.c_void_p()
    ws_ptr = C.c_void_p(ws.data_ptr() + G)
    assert lib.ph_resnet_plan_create(C.byref(cfg), _lib.ptr(pack.blob), ws_ptr, nws - 1, C.byref(h)) == _lib.PH_EWORKSPACE and not h.value
    torch.cuda.synchronize()
    assert int(ws.ne(0x5A).sum()) == 0
    _lib.check(lib.ph_resnet_plan_create(C.byref(cfg), _lib.ptr(pack.blob), ws_ptr, nws, C.byref(h)), "ph_resnet_plan_create")
    torch.cuda.synchronize()
    assert int(ws.ne(0x5A).sum()) == 0                              # create touches no device memory
    x = _image((B, 3, H, W), torch.float32, gpu)
    io = _lib.ResNetIO(image=x.data_ptr())
    for i in range(4):
        io.stages[i] = stages[i].data_ptr() + G
    blob0 = pack.blob.clone()
    _lib.check(lib.ph_resnet_plan_run(h, C.byref(io), _lib.stream_ptr()), "ph_resnet_plan_run")
    torch.cuda.synchronize()
    lib.ph_resnet_plan_destroy(h)
    for buf, n in [(ws, nws)] + list(zip(stages, sizes)):
        assert int(buf[:G].ne(0x5A).sum()) == 0 and int(buf[G + n:].ne(0x5A).sum()) == 0
    assert torch.equal(pack.blob, blob0)
    _, want = _python_stages(_module("bf16"), x, pack.pk, torch.bfloat16)
    for buf, n, b in zip(stages, sizes, want):
        assert torch.equal(buf[G:G + n].view(torch.bfloat16).reshape(b.shape), b)


# ---- 5. the environment ---------------------------------------------------------------------------------------------------------------
def test_environment_does_not_reach_the_native_plan(gpu, monkeypatch):
    m = _module("fp16")
    x = _image("even", torch.float32, gpu)
    cfg = E.native_resnet_cfg(2, 64, 128, 50, "fp16")
    pack0 = E.native_resnet_pack(m, cfg, gpu)
    plan = E.NativeResNetPlan(pack0, 2, 64, 128, gpu)
    base = [o.clone() for o in plan.run(x)]
    geo0 = bytes(plan.geometry)
    nodes0 = Hh.graph_kernel_nodes(lambda: plan.run(x))
    for k, v in (("PH_NECK_OUT2", "0"), ("PH_NECK_C16", "0"), ("PH_NECK_STREAMS", "0"), ("PH_CONV_TH", "4")):
        assert k in Hh.PLAN_KNOBS
        monkeypatch.setenv(k, v)
    with _lib.switches(conv_tile_rows=4, gnsum_wgs=3, cplanes_tpw=2):     # the library's switches, by call
        pack1 = E.native_resnet_pack(m, E.native_resnet_cfg(2, 64, 128, 50, "fp16"), gpu)
        assert torch.equal(pack1.blob, pack0.blob)
        plan2 = E.NativeResNetPlan(pack1, 2, 64, 128, gpu)
        got = plan2.run(x)
        torch.cuda.synchronize()
        assert bytes(plan2.geometry) == geo0
        for a, b in zip(got, base):
            assert torch.equal(a, b)
        assert Hh.graph_kernel_nodes(lambda: plan2.run(x)) == nodes0          # the same launches, whatever the switches say


# ---- 6. graph capture -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_run(gpu):
    pack = _native_pack("bf16")
    plan = E.NativeResNetPlan(pack, 2, 64, 128, gpu)
    static = _image("even", torch.float32, gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.run(static)                        # warm-up outside capture (lazy module load)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    plan.run(static)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before, "run() allocated"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = plan.run(static)
    eager_plan = E.NativeResNetPlan(pack, 2, 64, 128, gpu)
    for seed in (1, 2):
        new = _image("even", torch.float32, gpu, seed=seed)
        static.copy_(new)
        _poison(outs)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager_plan.run(new)):
            assert torch.equal(a, b), seed


# ---- 7. the module's switch -----------------------------------------------------------------------------------------------------------
def test_module_switch(gpu):
    with open(os.path.join(Hh.GOLDEN, "resnet_cfg.json")) as f:
        m = registry.build_backbone(json.load(f))
    m.load_state_dict(resnet_cases.fill(m.state_dict()))
    m.eval().to(gpu)
    x = _image("odd", torch.float32, gpu)
    default = [o.clone() for o in m(x)]
    assert m.use_native_plan(True) is m
    native = [o.clone() for o in m(x)]
    assert m._native_plans and isinstance(next(iter(m._native_plans.values())), E.NativeResNetPlan)
    for a, b in zip(native, default):
        assert torch.equal(a, b)
    pack = next(iter(m._native_packs.values()))
    m(x)
    assert next(iter(m._native_packs.values())) is pack            # nothing changed: no repack
    m.layer2[1].bn2.running_var.mul_(1.5)                          # in place: the version key sees it
    native2 = [o.clone() for o in m(x)]
    assert next(iter(m._native_packs.values())) is not pack
    default2 = [o.clone() for o in m.use_native_plan(False)(x)]
    assert torch.equal(native2[0], native[0])                      # stage 0 lies before the edited layer
    for i in (1, 2, 3):
        assert not torch.equal(native2[i], native[i]) and torch.equal(native2[i], default2[i])
    m.use_native_plan(True).set_stage_dtype(torch.bfloat16)
    assert not m._native_plans
    for a, b in zip(m(x), default2):
        assert a.dtype == torch.bfloat16 and torch.equal(a.float(), b)
    m.set_precision("fp16")
    assert not m._native_packs and not m._native_plans
    f16 = [o.clone() for o in m(x)]
    for a, b in zip(f16, m.use_native_plan(False)(x)):
        assert torch.equal(a, b)


# ---- 8. the C++ program ---------------------------------------------------------------------------------------------------------------
def _raw(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


@pytest.mark.parametrize("case", ["even_B2_bf16", "odd_B1_fp16"])
def test_image_program(gpu, case, tmp_path):
    """examples/image_c: a fresh process with no Python in it goes from the image to the panoptic maps; every file it writes -- the
    four stages, then everything examples/fpn_c writes -- is byte-equal to the Python chain on the same native packs:
    NativeResNetPlan -> NativeFpnPlan into NativeNeckPlan's level inputs (planes out) -> KernelHeadPlan -> DecodePlan.run_from_planes
    -> upsample2x -> BatchMerge.  The bf16 case has fp32 stages and the shared-buffer interleaving, the fp16 case fp16 stages and
    tower buffers."""
    from polyphonicformer_amd.panoptic import BatchMerge, DEPTH_MODES
    from test_gpu_native_plan import _native_as_stagepack
    assert os.path.exists(BLD.IMAGE_EXAMPLE), "built by python -m polyphonicformer_amd.build"
    shapes, img, kmode, dmode, tb, sdt, xdt = dict(
        even_B2_bf16=(TH.P_EVEN, (2, 3, 64, 128), "bf16", "mixed16", 0, torch.float32, torch.float32),
        odd_B1_fp16=(TH.P_ODD, (1, 3, 60, 92), "fp16", "fp16", 1, torch.float16, torch.bfloat16))[case]
    B, CH = img[0], TH.CH_FULL
    NQ, L, N_THING, N_STUFF = TN.NQ, TN.L, TN.N_THING, TN.N_STUFF
    H, W = shapes[1]
    wl = dict(H=H, W=W, Nq=NQ, n_thing=N_THING, n_stuff=N_STUFF, S=2, F=2048)
    S, F, N = wl["S"], wl["F"], NQ + N_STUFF
    out_dtype = torch.float16
    mode = E.MODES[dmode]
    backbone, eps = _module(kmode), 1e-5
    fpn, neck = TH._fpn(kmode, CH), TH._neck(kmode)
    ksd = TN._small_head(kmode)
    ih = bench.build_head(wl, "fp32", torch.float32, gpu, seed=8)
    ih.test_cfg = ConfigDict(max_per_img=NQ, mask_thr=0.5, merge_stuff_thing=dict(overlap_thr=0.0, instance_score_thr=0.3))
    ih.mask_head[-1].fc_cls.bias.fill_(1.0)      # un-trained heads: let segments pass the score threshold
    depth_mode = DEPTH_MODES[ih.mask_head[-1].depth_act_mode]
    meta = dict(img_shape=(8 * H, 8 * W, 3), ori_shape=(8 * H, 8 * W, 3), batch_input_shape=(8 * H, 8 * W))
    x = _image(img, xdt, gpu)
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    d_out.mkdir()
    geom = [2 * H, 2 * W, 8 * H, 8 * W, 8 * H, 8 * W, 8 * H, 8 * W]
    vals = [B] + [v for s in shapes for v in s] + [32, _lib.PH_MODE[kmode], 3, 128, NQ, L, N_THING, S, F, _lib.PH_MODE[dmode],
                                                  E.OUT_CODE[out_dtype], 1, NQ, depth_mode] + geom + [0.3, 0.0] + list(CH) + \
        [E.OUT_CODE[sdt], tb, img[2], img[3], 50, E.OUT_CODE[xdt], repr(eps)]
    (d_in / "cfg.txt").write_text(" ".join(str(v) for v in vals) + "\n")
    lib = _lib.load()
    tofile = lambda ts, name: np.concatenate([t.detach().float().cpu().numpy().reshape(-1) for t in ts]).astype("<f4").tofile(d_in / name)
    rcfg = E.native_resnet_cfg(B, img[2], img[3], 50, kmode, xdt, sdt, eps=eps)
    bsd, fsd, nsd = backbone.state_dict(), fpn.state_dict(), neck.state_dict()
    tofile([bsd[lib.ph_resnet_param_name(C.byref(rcfg), i).decode()] for i in range(lib.ph_resnet_nparams(C.byref(rcfg)))], "resnet.bin")
    tofile([fsd[lib.ph_fpn_param_name(i).decode()] for i in range(_lib.PH_FPN_NPARAMS)], "fpn.bin")
    tofile([nsd[lib.ph_neck_param_name(i).decode()] for i in range(_lib.PH_NECK_NPARAMS)], "neck.bin")
    tofile([ksd[lib.ph_khead_param_name(i).decode()] for i in range(_lib.PH_KHEAD_NPARAMS)], "khead.bin")
    for s, st in enumerate(ih.mask_head):
        sd = st.state_dict()
        tofile([sd[lib.ph_decode_param_name(i).decode()] for i in range(_lib.PH_DECODE_NPARAMS)], f"stage{s}.bin")
    _raw(x).tofile(d_in / "image.bin")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "PYTHONHOME") and k not in Hh.PLAN_KNOBS}
    r = subprocess.run(["timeout", "-k", "10", "240", BLD.IMAGE_EXAMPLE, str(d_in), str(d_out)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout.strip())

    # the Python chain on the same native packs
    rplan = E.NativeResNetPlan(E.native_resnet_pack(backbone, rcfg, gpu), B, img[2], img[3], gpu, cfg=rcfg)
    stages = rplan.run(x)
    assert [tuple(s.shape[1:]) for s in stages] == [(c,) + tuple(s) for c, s in zip(CH, shapes)]
    assert all(s.dtype == sdt and bool(torch.isfinite(s).all()) for s in stages)
    table = E.native_neck_posenc(*shapes[3], 128, device=gpu)
    ncfg = TN._cfg(B, shapes, kmode, tb=tb)
    nplan = E.NativeNeckPlan(E.native_neck_pack(neck, ncfg, gpu), B, shapes, gpu, cfg=ncfg)
    fcfg = E.native_fpn_cfg(B, shapes, CH, kmode, sdt)
    nfpn = E.NativeFpnPlan(E.native_fpn_pack(fpn, fcfg, gpu), B, shapes, gpu, sdt)
    h = E.NeckHandoff(nplan, nplan.pack, 32, table, 3, to_planes=True)
    levels = nfpn.run(list(stages), neck=h)
    planes = h.finish()
    kcfg = E.native_khead_cfg(B, H, W, NQ, L, N_THING, True, 32, kmode, want_f32=False, frame_invariant=True)
    kpack = E.native_khead_pack(ksd, kcfg, gpu)
    kp = E.KernelHeadPlan(kpack, B, H, W, N_THING, L, True, gpu, want_f32=False, frame_invariant=True)
    kp.set_inputs(planes)
    kp.run()
    dcfg = E.native_cfg(B, N, H, W, S, L, F, mode, out_dtype, True)
    blobs = [E.native_pack_stage(st, dcfg, gpu) for st in ih.mask_head]
    dp = E.DecodePlan([_native_as_stagepack(b, dcfg, mode, L) for b in blobs], B, N, H, W, mode, out_dtype, gpu, frame_invariant=True)
    q0 = kpack.w_dd_f32.reshape(1, 1, 256).expand(B, N, 256).contiguous()
    dp.run_from_planes(kp.xp, kp.dp, kp.bits, kp.proposal, q0)
    d0 = E.upsample2x(kp.depth_pred)
    o = dp.outputs()
    bm = BatchMerge(ih, B, N, L, 2 * H, 2 * W, out_dtype, meta, gpu)
    bm.run(o["cls"], o["mask_up"], o["depth_up"], d0)
    torch.cuda.synchronize()
    assert kp.timeouts() == 0
    want = dict(s0=stages[0], s1=stages[1], s2=stages[2], s3=stages[3], p0=levels[0], p1=levels[1], p2=levels[2], p3=levels[3],
                posenc=table, n0=planes[0], n1=planes[1], n2=planes[2], xp=kp.xp, dp=kp.dp, bits=kp.bits, mask_preds=kp.mask_preds,
                seg_preds=kp.seg_preds, depth_pred=kp.depth_pred, proposal=kp.proposal, depth_proposal=q0, obj=o["obj"], dobj=o["dobj"],
                cls=o["cls"], mask=o["mask"], mask_up=o["mask_up"], depth_up=o["depth_up"], depth_init_up=d0, pan=bm.pan,
                depth_basic=bm.d_basic, depth_final=bm.d_final, seg_records=bm.records)
    written = sorted(p.name for p in d_out.iterdir())
    assert written == sorted([f"{k}.bin" for k in want] + ["geometry.txt"])
    for k in want:                                       # in the chain's order: the first difference names the step
        got = np.fromfile(d_out / f"{k}.bin", dtype="u1")
        w = _raw(want[k])
        assert got.shape == w.shape and np.array_equal(got, w), k
    # and the stages are the two-step path's: ResNetPlan on the module's own pack
    for a, b in zip(stages, _python_stages(backbone, x, backbone._pack(gpu), sdt)[1]):
        assert torch.equal(a, b)
    geo = dict(line.split() for line in (d_out / "geometry.txt").read_text().splitlines())
    assert (int(geo["resnet_prec"]), int(geo["resnet_launches"]), int(geo["resnet_nconvs"])) == (E.KHEAD_PREC[kmode], 57, 52)
    assert int(geo["resnet_stem_workgroups"]) == rplan.geometry.stem_workgroups
    assert (int(geo["fpn_P"]), int(geo["fpn_prec"]), int(geo["neck_tower_buffers"])) == (1, E.KHEAD_PREC[kmode], tb)
    assert (int(geo["khead_onepass"]), int(geo["fell_back"]), int(geo["timeouts"])) == (int(kp.onepass), 0, 0)
    assert int(geo["K"]) == bm.K
