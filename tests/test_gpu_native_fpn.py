"""GPU: the native FPN plan (include/polyhead.h ph_fpn_pack, ph_fpn_plan_*; engine.NativeFpnPlan; examples/fpn_c).  The packing is
compared byte for byte with fpn.FPN._pack, the plan's levels bit for bit with engine.FpnPlan, and -- written straight into a native
neck plan's level inputs -- the neck's outputs bit for bit with the Python chain FpnPlan -> NeckPlan.  No tolerance appears: both
sides issue the same launches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import bench
import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
from polyphonicformer_amd import build as BLD
from polyphonicformer_amd.registry import ConfigDict
import test_gpu_fpn_handoff as TH
import test_gpu_native_neck as TN

pytestmark = pytest.mark.gpu

GRADES, PYRAMIDS, CH = TH.GRADES, TH.PYRAMIDS, TH.CH
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(autouse=True)
def _inference(monkeypatch):
    Hh.clear_plan_knobs(monkeypatch)
    with torch.no_grad():
        yield


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


# ---- 1. packing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grade", ["bf16", "fp16", "fp32"])
def test_packing_is_the_module_pack_byte_for_byte(gpu, grade):
    m = TH._fpn(grade)
    cfg = E.native_fpn_cfg(2, TH.P_EVEN, CH, grade)
    lib = _lib.load()
    nbytes = lib.ph_fpn_pack_bytes(C.byref(cfg))
    pack = E.native_fpn_pack(m, cfg, gpu)
    again = E.native_fpn_pack(m.state_dict(), cfg, gpu)          # a state_dict packs to the same bytes
    torch.cuda.synchronize()
    assert pack.blob.numel() == nbytes and torch.equal(pack.blob, again.blob)
    ref = m._pack(gpu)
    covered = torch.zeros(nbytes, dtype=torch.bool, device=gpu)
    for kind, first in (("lateral", 0), ("output", 8)):
        for l in range(4):
            for j, name in enumerate(("wp", "bias")):
                i = first + 2 * l + j
                got, want = pack.pk[kind][l][name], ref[kind][l][name]
                assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (kind, l, name)
                assert torch.equal(_bytes(got), _bytes(want)), (kind, l, name)
                off, nb = int(pack.layout.offset[i]), int(pack.layout.bytes[i])
                assert nb == want.numel() * want.element_size() and not bool(covered[off:off + nb].any())
                covered[off:off + nb] = True
            assert (pack.pk[kind][l]["k"], pack.pk[kind][l]["s"]) == (ref[kind][l]["k"], ref[kind][l]["s"])
    assert int(pack.blob[~covered].ne(0).sum()) == 0              # what lies between the pieces is zero
    # either plan runs from the native pack's views
    stages = TH._stages(TH.P_EVEN, 2, gpu)
    plan = E.FpnPlan(2, TH.P_EVEN, CH, GRADES[grade], gpu)
    a = [o.clone() for o in plan.run(stages, ref)]
    for x, y in zip(a, plan.run(stages, pack.pk)):
        assert torch.equal(x, y)


def test_pack_writes_exactly_its_bytes(gpu):
    """the pieces of an FPN pack are multiples of 256 bytes, so ph_fpn_pack writes no padding of its own; a pack buffer that was full
    of ones holds exactly the pieces afterwards (every byte written, none beyond)"""
    lib = _lib.load()
    cfg = E.native_fpn_cfg(1, TH.P_EVEN, CH, "bf16")
    n = lib.ph_fpn_pack_bytes(C.byref(cfg))
    lay = _lib.FpnLayout()
    lib.ph_fpn_pack_layout(C.byref(cfg), C.byref(lay))
    assert sum(lay.bytes) == n
    want = E.native_fpn_pack(TH._fpn("bf16"), cfg, gpu).blob
    params, ptrs = E._gather_params(TH._fpn("bf16"), gpu, 16, lib.ph_fpn_param_name, lambda i: lib.ph_fpn_param_numel(C.byref(cfg), i))
    buf = torch.full((n + 512,), 0xFF, dtype=torch.uint8, device=gpu)
    _lib.check(lib.ph_fpn_pack(C.byref(cfg), ptrs, C.c_void_p(buf.data_ptr() + 256), _lib.stream_ptr()), "ph_fpn_pack")
    torch.cuda.synchronize()
    assert torch.equal(buf[256:256 + n], want) and bool((buf[:256] == 0xFF).all()) and bool((buf[256 + n:] == 0xFF).all())


# ---- 2. bit identity with engine.FpnPlan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("grade", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("pyramid", ["even", "odd", "wide"])
def test_levels_equal_the_python_plan(gpu, pyramid, grade, dtype):
    B, shapes = 2, PYRAMIDS[pyramid]
    m = TH._fpn(grade)
    stages = TH._stages(shapes, B, gpu, dtype=DTYPES[dtype])
    want = [o.clone() for o in E.FpnPlan(B, shapes, CH, GRADES[grade], gpu).run(stages, m._pack(gpu))]
    cfg = E.native_fpn_cfg(B, shapes, CH, grade, DTYPES[dtype])
    plan = E.NativeFpnPlan(E.native_fpn_pack(m, cfg, gpu), B, shapes, gpu, DTYPES[dtype])
    assert (plan.geometry.P, plan.geometry.prec) == (2 if grade == "fp32" else 1, GRADES[grade])
    plan.run(stages)                                            # allocates the levels
    TH._poison(plan.outs)
    got = plan.run(stages)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    with pytest.raises(_lib.PolyheadError, match="inputs\\[0\\]"):
        plan.run([t.double() for t in stages])


def test_levels_at_the_shipped_stage_widths(gpu):
    B, shapes, grade = 1, TH.P_ODD, "fp16"
    m = TH._fpn(grade, TH.CH_FULL)
    stages = TH._stages(shapes, B, gpu, TH.CH_FULL)
    want = [o.clone() for o in E.FpnPlan(B, shapes, TH.CH_FULL, GRADES[grade], gpu).run(stages, m._pack(gpu))]
    cfg = E.native_fpn_cfg(B, shapes, TH.CH_FULL, grade)
    got = E.NativeFpnPlan(E.native_fpn_pack(m, cfg, gpu), B, shapes, gpu).run(stages)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tb", [0, 1], ids=["shared", "towers"])
@pytest.mark.parametrize("grade", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("pyramid", ["even", "odd", "wide"])
def test_planes_into_a_native_neck_plan(gpu, pyramid, grade, tb):
    """ph_fpn_plan_run[_output] writes ph_neck_plan_level_input's planes; the native neck's outputs, fp32 and planes, equal the Python
    chain's (FpnPlan's levels through NeckPlan), and so do the fp32 levels written beside the planes"""
    B, shapes = 2, PYRAMIDS[pyramid]
    fpn, neck = TH._fpn(grade), TH._neck(grade)
    fplan, fpk, pyplan, npk, posenc = TH._plans(grade, shapes, B, gpu, "always" if tb else False)
    stages = TH._stages(shapes, B, gpu, seed=8)
    levels = [o.clone() for o in fplan.run(stages, fpk)]
    want = {tp: [o.clone() for o in pyplan.run(levels, npk, 32, posenc, 3, to_planes=tp)] for tp in (False, True)}
    ncfg = TN._cfg(B, shapes, grade, tb=tb)
    nplan = E.NativeNeckPlan(E.native_neck_pack(neck, ncfg, gpu), B, shapes, gpu, cfg=ncfg)
    assert nplan.multi == bool(tb)
    fcfg = E.native_fpn_cfg(B, shapes, CH, grade)
    nfpn = E.NativeFpnPlan(E.native_fpn_pack(fpn, fcfg, gpu), B, shapes, gpu)
    for tp in (False, True):
        for want_levels in (True, False):
            TH._poison(nplan.outputs(tp) + (nfpn.outs or []))
            nplan.workspace.fill_(0xFF)
            h = E.NeckHandoff(nplan, nplan.pack, 32, posenc, 3, to_planes=tp)
            got_levels = nfpn.run(stages, neck=h, want_levels=want_levels)
            got = h.finish()
            torch.cuda.synchronize()
            for a, b in zip(got, want[tp]):
                assert torch.equal(a, b), (tp, want_levels)
            if want_levels:
                for a, b in zip(got_levels, levels):
                    assert torch.equal(a, b)
            else:
                assert got_levels is None and all(bool(o.isnan().all()) for o in nfpn.outs)
    # the Python FPN plan writes the native neck plan's inputs as well
    TH._poison(nplan.outputs(True))
    h = E.NeckHandoff(nplan, nplan.pack, 32, posenc, 3, to_planes=True)
    fplan.run(stages, fpk, neck=h)
    for a, b in zip(h.finish(), want[True]):
        assert torch.equal(a, b)


# ---- 3. guarded buffers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grade,layout0", [("fp16", _lib.PH_PLANES_C16), ("fp32", 0), ("bf16", 0)])
def test_workspace_and_pack_stay_inside_their_bounds(gpu, grade, layout0):
    """pack, workspace and every output between 4 KiB canaries: intact after pack + run; a workspace 256 bytes short is refused,
    nothing launched"""
    lib = _lib.load()
    B, shapes, G = 3, TH.P_WIDE, 4096
    m = TH._fpn(grade)
    cfg = E.native_fpn_cfg(B, shapes, CH, grade, emit_f32=True, emit_planes=True)
    P = 2 if grade == "fp32" else 1
    nws, npk = lib.ph_fpn_plan_workspace_bytes(C.byref(cfg)), lib.ph_fpn_pack_bytes(C.byref(cfg))
    guarded = lambda n: torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device=gpu)
    ws, pk = guarded(nws), guarded(npk)
    hw = [h * w for h, w in shapes]
    maps, planes = [guarded(B * 256 * n * 4) for n in hw], [guarded(P * B * n * 256 * 2) for n in hw]
    params, ptrs = E._gather_params(m, gpu, 16, lib.ph_fpn_param_name, lambda i: lib.ph_fpn_param_numel(C.byref(cfg), i))
    pk_ptr, ws_ptr = C.c_void_p(pk.data_ptr() + G), C.c_void_p(ws.data_ptr() + G)
    h = C.c_void_p()
    assert lib.ph_fpn_plan_create(C.byref(cfg), pk_ptr, ws_ptr, nws - 256, C.byref(h)) == _lib.PH_EWORKSPACE and not h.value
    torch.cuda.synchronize()
    assert int(ws.ne(0x5A).sum()) == 0 and int(pk.ne(0x5A).sum()) == 0
    _lib.check(lib.ph_fpn_pack(C.byref(cfg), ptrs, pk_ptr, _lib.stream_ptr()), "ph_fpn_pack")
    _lib.check(lib.ph_fpn_plan_create(C.byref(cfg), pk_ptr, ws_ptr, nws, C.byref(h)), "ph_fpn_plan_create")
    stages = TH._stages(shapes, B, gpu, seed=13)
    add = torch.randn(256, *shapes[3], device=gpu)
    io = _lib.FpnIO()
    for l in range(4):
        io.stages[l], io.out_f32[l], io.out_planes[l] = stages[l].data_ptr(), maps[l].data_ptr() + G, planes[l].data_ptr() + G
    io.planes_layout[0], io.add[3] = layout0, add.data_ptr()
    _lib.check(lib.ph_fpn_plan_run(h, C.byref(io), _lib.stream_ptr()), "ph_fpn_plan_run")
    torch.cuda.synchronize()
    lib.ph_fpn_plan_destroy(h)
    for buf in [ws, pk] + maps + planes:
        n = buf.numel() - 2 * G
        assert int(buf[:G].ne(0x5A).sum()) == 0 and int(buf[G + n:].ne(0x5A).sum()) == 0
    # what lies between the canaries: FpnPlan's levels, and the planes ph_nhwc_ingest makes of them
    levels = E.FpnPlan(B, shapes, CH, GRADES[grade], gpu).run(stages, m._pack(gpu))
    for l in range(4):
        n = hw[l]
        assert torch.equal(maps[l][G:G + B * 256 * n * 4].view(torch.float32).reshape(levels[l].shape), levels[l]), l
        ref = torch.empty((P, B, n, 256), dtype=torch.int16, device=gpu)
        E.nhwc_ingest(levels[l], add if l == 3 else None, GRADES[grade] | (layout0 if l == 0 else 0), ref)
        assert torch.equal(planes[l][G:G + P * B * n * 256 * 2].view(torch.int16).reshape(ref.shape), ref), l


# ---- 4. the environment -----------------------------------------------------------------------------------------------------------------
def test_environment_does_not_reach_the_native_plan(gpu, monkeypatch):
    B, shapes, grade = 2, TH.P_WIDE, "fp16"         # every conv launch takes 2-row tiles here: conv_tile_rows=4 changes the public path's
    m = TH._fpn(grade)
    stages = TH._stages(shapes, B, gpu, seed=11)
    cfg = E.native_fpn_cfg(B, shapes, CH, grade)
    pack = E.native_fpn_pack(m, cfg, gpu)
    plan = E.NativeFpnPlan(pack, B, shapes, gpu)
    base = [o.clone() for o in plan.run(stages)]
    geo0 = bytes(plan.geometry)
    assert 4 not in list(plan.geometry.tile_rows)
    nodes0 = Hh.graph_kernel_nodes(lambda: plan.run(stages))
    for k, v in (("PH_NECK_OUT2", "0"), ("PH_NECK_C16", "0"), ("PH_NECK_STREAMS", "0")):
        assert k in Hh.PLAN_KNOBS
        monkeypatch.setenv(k, v)
    with _lib.switches(conv_tile_rows=4, gnsum_wgs=3, cplanes_tpw=2):            # the library's switches, by call
        plan2 = E.NativeFpnPlan(E.native_fpn_pack(m, E.native_fpn_cfg(B, shapes, CH, grade), gpu), B, shapes, gpu)
        got = plan2.run(stages)
        torch.cuda.synchronize()
        assert bytes(plan2.geometry) == geo0
        for a, b in zip(got, base):
            assert torch.equal(a, b)
        assert Hh.graph_kernel_nodes(lambda: plan2.run(stages)) == nodes0       # the same launches, whatever the switches say
        pyplan = E.FpnPlan(B, shapes, CH, GRADES[grade], gpu)                    # the public conv entry point listens
        assert Hh.graph_kernel_nodes(lambda: pyplan.run(stages, m._pack(gpu))) != nodes0


# ---- 5. graph capture -------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_run(gpu):
    B, shapes, grade = 2, TH.P_ODD, "bf16"
    m = TH._fpn(grade)
    cfg = E.native_fpn_cfg(B, shapes, CH, grade)
    pack = E.native_fpn_pack(m, cfg, gpu)
    plan = E.NativeFpnPlan(pack, B, shapes, gpu)
    static = TH._stages(shapes, B, gpu, seed=20)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.run(static)                        # warm-up outside capture (lazy module load)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = plan.run(static)
    eager_plan = E.NativeFpnPlan(pack, B, shapes, gpu)
    for seed in (21, 22):
        new = TH._stages(shapes, B, gpu, seed=seed)
        for dst, src in zip(static, new):
            dst.copy_(src)
        TH._poison(outs)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager_plan.run(new)):
            assert torch.equal(a, b), seed


# ---- 6. the C++ program -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["even_B2_bf16", "odd_B1_fp16"])
def test_fpn_program(gpu, case, tmp_path):
    """examples/fpn_c: a fresh process with no Python in it goes from the four backbone stages to the panoptic maps; every file it
    writes is byte-equal to the Python chain on the same native packs and the device-computed positional encoding: NativeFpnPlan
    into NativeNeckPlan's level inputs (planes out) -> KernelHeadPlan -> DecodePlan.run_from_planes -> upsample2x -> BatchMerge.
    The bf16 case runs the shared-buffer interleaving, the fp16 case the tower-buffer form."""
    from polyphonicformer_amd.panoptic import BatchMerge, DEPTH_MODES
    from test_gpu_native_plan import _native_as_stagepack
    assert os.path.exists(BLD.FPN_EXAMPLE), "built by python -m polyphonicformer_amd.build"
    shapes, B, kmode, dmode, tb = dict(even_B2_bf16=(TH.P_EVEN, 2, "bf16", "mixed16", 0), odd_B1_fp16=(TH.P_ODD, 1, "fp16", "fp16", 1))[case]
    NQ, L, N_THING, N_STUFF = TN.NQ, TN.L, TN.N_THING, TN.N_STUFF
    H, W = shapes[1]
    wl = dict(H=H, W=W, Nq=NQ, n_thing=N_THING, n_stuff=N_STUFF, S=2, F=2048)
    S, F, N = wl["S"], wl["F"], NQ + N_STUFF
    out_dtype = torch.float16
    mode = E.MODES[dmode]
    fpn, neck = TH._fpn(kmode), TH._neck(kmode)
    ksd = TN._small_head(kmode)
    ih = bench.build_head(wl, "fp32", torch.float32, gpu, seed=8)
    ih.test_cfg = ConfigDict(max_per_img=NQ, mask_thr=0.5, merge_stuff_thing=dict(overlap_thr=0.0, instance_score_thr=0.3))
    ih.mask_head[-1].fc_cls.bias.fill_(1.0)      # un-trained heads: let segments pass the score threshold
    depth_mode = DEPTH_MODES[ih.mask_head[-1].depth_act_mode]
    meta = dict(img_shape=(8 * H, 8 * W, 3), ori_shape=(8 * H, 8 * W, 3), batch_input_shape=(8 * H, 8 * W))
    stages = TH._stages(shapes, B, gpu, seed=17)
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    d_out.mkdir()
    geom = [2 * H, 2 * W, 8 * H, 8 * W, 8 * H, 8 * W, 8 * H, 8 * W]
    vals = [B] + [v for s in shapes for v in s] + [32, _lib.PH_MODE[kmode], 3, 128, NQ, L, N_THING, S, F, _lib.PH_MODE[dmode],
                                                  E.OUT_CODE[out_dtype], 1, NQ, depth_mode] + geom + [0.3, 0.0] + list(CH) + [_lib.PH_OUT_F32, tb]
    (d_in / "cfg.txt").write_text(" ".join(str(v) for v in vals) + "\n")
    lib = _lib.load()
    tofile = lambda ts, name: np.concatenate([t.detach().float().cpu().numpy().reshape(-1) for t in ts]).astype("<f4").tofile(d_in / name)
    fsd, nsd = fpn.state_dict(), neck.state_dict()
    tofile([fsd[lib.ph_fpn_param_name(i).decode()] for i in range(_lib.PH_FPN_NPARAMS)], "fpn.bin")
    tofile([nsd[lib.ph_neck_param_name(i).decode()] for i in range(_lib.PH_NECK_NPARAMS)], "neck.bin")
    tofile([ksd[lib.ph_khead_param_name(i).decode()] for i in range(_lib.PH_KHEAD_NPARAMS)], "khead.bin")
    for s, st in enumerate(ih.mask_head):
        sd = st.state_dict()
        tofile([sd[lib.ph_decode_param_name(i).decode()] for i in range(_lib.PH_DECODE_NPARAMS)], f"stage{s}.bin")
    for i, f in enumerate(stages):
        tofile([f], f"s{i}.bin")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "PYTHONHOME") and k not in Hh.PLAN_KNOBS}
    r = subprocess.run(["timeout", "-k", "10", "240", BLD.FPN_EXAMPLE, str(d_in), str(d_out)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout.strip())

    # the Python chain on the same native packs
    table = E.native_neck_posenc(*shapes[3], 128, device=gpu)
    ncfg = TN._cfg(B, shapes, kmode, tb=tb)
    nplan = E.NativeNeckPlan(E.native_neck_pack(neck, ncfg, gpu), B, shapes, gpu, cfg=ncfg)
    fcfg = E.native_fpn_cfg(B, shapes, CH, kmode)
    nfpn = E.NativeFpnPlan(E.native_fpn_pack(fpn, fcfg, gpu), B, shapes, gpu)
    h = E.NeckHandoff(nplan, nplan.pack, 32, table, 3, to_planes=True)
    levels = nfpn.run(stages, neck=h)
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
    want = dict(p0=levels[0], p1=levels[1], p2=levels[2], p3=levels[3],
                posenc=table, n0=planes[0], n1=planes[1], n2=planes[2], xp=kp.xp, dp=kp.dp, bits=kp.bits, mask_preds=kp.mask_preds,
                seg_preds=kp.seg_preds, depth_pred=kp.depth_pred, proposal=kp.proposal, depth_proposal=q0, obj=o["obj"], dobj=o["dobj"],
                cls=o["cls"], mask=o["mask"], mask_up=o["mask_up"], depth_up=o["depth_up"], depth_init_up=d0, pan=bm.pan,
                depth_basic=bm.d_basic, depth_final=bm.d_final, seg_records=bm.records)
    written = sorted(p.name for p in d_out.iterdir())
    assert written == sorted([f"{k}.bin" for k in want] + ["geometry.txt"])
    for k in ("p0", "p1", "p2", "p3", "n0", "n1", "n2", "pan") + tuple(k for k in want if k not in ("p0", "p1", "p2", "p3", "n0", "n1", "n2", "pan")):
        got = np.fromfile(d_out / f"{k}.bin", dtype="u1")
        w = TN._raw(want[k])
        assert got.shape == w.shape and np.array_equal(got, w), k
    # and the levels are the two-step chain's: FpnPlan on the module's own pack
    for a, b in zip(levels, E.FpnPlan(B, shapes, CH, E.KHEAD_PREC[kmode], gpu).run(stages, fpn._pack(gpu))):
        assert torch.equal(a, b)
    geo = dict(line.split() for line in (d_out / "geometry.txt").read_text().splitlines())
    assert (int(geo["fpn_P"]), int(geo["fpn_prec"]), int(geo["neck_tower_buffers"])) == (1, E.KHEAD_PREC[kmode], tb)
    assert [int(geo[f"fpn_tile_rows_{l}"]) for l in range(4)] == list(nfpn.geometry.tile_rows)
    assert (int(geo["neck_fused_out"]), int(geo["neck_c16"]), int(geo["neck_P"])) == (1, 1, 1)
    assert (int(geo["khead_onepass"]), int(geo["fell_back"]), int(geo["timeouts"])) == (int(kp.onepass), 0, 0)
    assert int(geo["K"]) == bm.K and int(bm.records[:, 0].min()) > 0          # the merge accepted segments in every frame
