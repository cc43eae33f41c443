"""The native decode plan on the device (include/polyhead.h ph_decode_*, engine.NativeDecodePlan): bit identity with
engine.DecodePlan in every mode and geometry the project runs, the packing kernel against pack.py, a decode from native packs
against the oracle, the module API switch, graph capture, and the Python-free example program."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import helpers as Hh
from oracle import poly_oracle as O
from polyphonicformer_amd import _lib, engine as E
from polyphonicformer_amd import build as BLD
from polyphonicformer_amd.pack import _bf16_planes, _pad_rows, pack_b_fragments

pytestmark = pytest.mark.gpu

MODES = ["fp32", "mixed", "mixed16", "fp16", "bf16"]
OUT16 = {"fp32": torch.float32, "mixed": torch.float32, "mixed16": torch.float16, "fp16": torch.float16, "bf16": torch.bfloat16}
TOL_IDENT = {"fp32": 1e-3, "mixed": 1e-3, "mixed16": 1e-3, "fp16": 1e-3, "bf16": 3e-2}      # tests/test_gpu_configs.py

# name -> (workload, B, shares_gpu): cfg1's exact shape (one frame 32 x 64, N = 100, one stage), cfg3 (N = 111, S = 3) at one and
# eight frames, cfg5 (48 x 156, N = 253), one 32-frame part of the headline step (cfg2 geometry, a part of a multi-stream step)
CASES = {
    "cfg1": (dict(H=32, W=64, Nq=89, n_thing=8, n_stuff=11, S=1, F=2048), 1, False),
    "cfg3_b1": (bench.WORKLOADS["cfg3"], 1, False),
    "cfg3_b8": (bench.WORKLOADS["cfg3"], 8, False),
    "cfg5": (bench.WORKLOADS["cfg5"], 1, False),
    "part32": (bench.WORKLOADS["cfg2"], 32, True),
}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    Hh.clear_plan_knobs(monkeypatch)


def _equal_outputs(a, b, what):
    for k in ("obj", "dobj", "cls", "mask", "mask_up", "depth_up", "depth"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k], b[k]), (what, k, (a[k].float() - b[k].float()).abs().max().item())


def _inputs(wl, B, gpu, seed=5):
    inp = bench.synth_inputs(wl, B, seed=seed)
    return {k: v.to(gpu) for k, v in inp.items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_identity_with_decode_plan(gpu, case):
    """the same StagePacks through DecodePlan and NativeDecodePlan: every output torch.equal, the same geometry chosen; every
    mode, both frame_invariant settings; fp32 feature inputs, and 16-bit ones in the 16-bit modes"""
    wl, B, shares = CASES[case]
    N = wl["Nq"] + wl["n_stuff"]
    head = bench.build_head(wl, "fp32", torch.float32, gpu, seed=3)
    g = _inputs(wl, B, gpu)
    for mode in MODES:
        packs = [h.stage_pack(gpu, mode) for h in head.mask_head]
        m = E.MODES[mode]
        feats = [(g["x"], g["dfe"])] + ([(g["x"].to(m.feat_dtype), g["dfe"].to(m.feat_dtype))] if m.feat_dtype is not None else [])
        for fi in (False, True):
            py = E.DecodePlan(packs, B, N, wl["H"], wl["W"], m, OUT16[mode], gpu, frame_invariant=fi)
            py.shares_gpu = shares
            nat = E.NativeDecodePlan(packs, B, N, wl["H"], wl["W"], m, OUT16[mode], gpu, frame_invariant=fi, shares_gpu=shares)
            assert (nat.nsplit, nat.nsplit_px, nat.poolx, nat.fused_up) == (py.nsplit, py.nsplit_px, py.poolx, py.fused_up), (case, mode, fi)
            if py.fused_up:
                wg = py.up2_shared_wgs if (shares and B * wl["H"] >= 4 * py.up2_shared_wgs) else 0
                assert nat.geometry.up2_workgroups == wg
            for x, dfe in feats:
                for p in (py, nat):
                    p.set_inputs(x, dfe, g["k0"], g["q0"], g["m0"])
                    p.run()
                torch.cuda.synchronize()
                _equal_outputs(py.outputs(), nat.outputs(), (case, mode, fi, x.dtype))
            print(f"{case} {mode} fi={fi}: nsplit {nat.nsplit} nsplit_px {nat.nsplit_px} poolx {nat.poolx} fused_up {nat.fused_up}: equal")
            del py, nat


def _split(w32, post16):
    """fp32 values -> (hi, lo) int16 planes as pack.py makes them (bf16 hi / lo, or one fp16 plane and a zero lo)"""
    if post16:
        h = w32.to(torch.float16).view(torch.int16)
        return h, torch.zeros_like(h)
    hi, lo = _bf16_planes(w32.double(), 2)
    return hi, lo


def _folds(sd, br):
    """pack.py's float64 folding of branch `br` (the same expressions): DYN [512][256], KERN [272][256], DYN_CNT [512], KERN_B [272]"""
    gd = lambda k: sd[k].detach().to("cpu", torch.float64)
    tr = ("feat_transform.conv.", "feat_depth_transform.conv.")[br]
    ku = ("kernel_update_conv.", "kernel_update_conv_depth.")[br]
    fc = ("fc_mask.", "fc_depth.")[br]
    Wx, bx = gd(tr + "weight").reshape(256, 256), gd(tr + "bias")
    Wdyn, Wk, bk = gd(ku + "dynamic_layer.weight"), gd(fc + "weight"), gd(fc + "bias")
    kern = _pad_rows(torch.cat([Wx.t() @ Wk, (bx @ Wk)[None]], 0))
    kb = torch.cat([torch.cat([Wx.t() @ bk, (bx @ bk)[None]], 0), torch.zeros(15, dtype=torch.float64)])
    return dict(DYN=Wdyn @ Wx, KERN=kern), dict(DYN_CNT=Wdyn @ bx, KERN_B=kb)


@pytest.mark.parametrize("mode", MODES)
def test_native_packing(gpu, mode):
    """ph_decode_pack_stage against pack.py (engine.StagePack): byte-equal on every non-folded block; on the folded ones
    (feat_transform into dynamic_layer / fc_mask / fc_depth) each entry is the split of pack.py's fp32 value or of one of its two
    fp32 neighbours -- the float64 sums run in another order (k ascending here, BLAS blocking there), so the fp32 rounding of a sum
    that lies within 2^-53-ish of a rounding boundary can land one ulp apart.  Two packings are byte-equal."""
    wl = dict(bench.WORKLOADS["cfg2"], S=1)
    head = bench.build_head(wl, "fp32", torch.float32, gpu, seed=4)
    stage = head.mask_head[0]
    L = wl["n_thing"] + wl["n_stuff"]
    m = E.MODES[mode]
    cfg = E.native_cfg(1, wl["Nq"] + wl["n_stuff"], wl["H"], wl["W"], 1, L, wl["F"], m)
    sp = E.StagePack({k: v.detach().cpu() for k, v in stage.state_dict().items()}, "", L, m.query, gpu)
    ref = E.native_pack_from(sp, cfg)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a = E.native_pack_stage(stage, cfg, gpu)
    start.record()
    b = E.native_pack_stage(stage, cfg, gpu)
    end.record()
    torch.cuda.synchronize()
    print(f"{mode}: ph_decode_pack_stage {start.elapsed_time(end) * 1e3:.0f} us for one cfg2 stage ({a.numel() / 1e6:.1f} MB)")
    assert torch.equal(a, b), "two packings of the same weights differ"
    lay, off = sp.lay, C.c_size_t()
    _lib.check(_lib.load().ph_decode_pack_layout(C.byref(cfg), None, C.byref(off)), "layout")
    P = sp.wb.shape[0]
    plane = lay.wb_plane_elems
    nat_wb = a[:P * plane * 2].view(torch.int16).reshape(P, plane).cpu()
    ref_wb = ref[:P * plane * 2].view(torch.int16).reshape(P, plane).cpu()
    nv = sp.wf.numel()
    nat_wf = a[off.value:off.value + nv * 4].view(torch.float32).cpu()
    ref_wf = ref[off.value:off.value + nv * 4].view(torch.float32).cpu()
    assert torch.equal(ref_wf, sp.wf.cpu()) and torch.equal(ref_wb, sp.wb.cpu())
    # block extents: the offsets in ascending order
    wstarts = sorted((int(lay.w[br][i]), br, n) for br in range(2) for i, n in enumerate(_lib.W_NAMES)
                     if not (br == 1 and n in ("H0B", "CLS")))
    vstarts = sorted((int(lay.v[br][i]), br, n) for br in range(2) for i, n in enumerate(_lib.V_NAMES)
                     if not (br == 1 and n in ("LN_H0B_G", "LN_H0B_B", "CLS_B")))
    hybrid = m.query == _lib.PH_PREC_QHYBRID
    POST = {"OUT", "FFN1", "FFN2", "H0A", "H0B", "CLS", "KERN", "QKV"}
    sd = {k: v.detach().cpu() for k, v in stage.state_dict().items()}
    off_ulp = 0
    for j, (o, br, n) in enumerate(wstarts):
        e = wstarts[j + 1][0] if j + 1 < len(wstarts) else plane
        if n not in ("DYN", "KERN"):
            assert torch.equal(nat_wb[:, o:e], ref_wb[:, o:e]), (br, n)
            continue
        w32 = pack_b_fragments(_folds(sd, br)[0][n]).to(torch.float32)
        assert w32.numel() == e - o
        post16 = hybrid and n in POST
        cands = [_split(c, post16) for c in (w32, torch.nextafter(w32, torch.tensor(float("inf"))),
                                              torch.nextafter(w32, torch.tensor(float("-inf"))))]
        hi, lo = nat_wb[0, o:e], (nat_wb[1, o:e] if P == 2 else None)
        ok = torch.zeros_like(hi, dtype=torch.bool)
        for ch, cl in cands:
            ok |= (hi == ch) & ((lo == cl) if lo is not None else True)
        assert bool(ok.all()), (br, n, int((~ok).sum()))
        off_ulp += int(((hi != cands[0][0]) | ((lo != cands[0][1]) if lo is not None else False)).sum())
    for j, (o, br, n) in enumerate(vstarts):
        e = vstarts[j + 1][0] if j + 1 < len(vstarts) else nv
        if n not in ("DYN_CNT", "KERN_B"):
            assert torch.equal(nat_wf[o:e], ref_wf[o:e]), (br, n)
            continue
        d = (nat_wf[o:e].view(torch.int32).long() - ref_wf[o:e].view(torch.int32).long()).abs()
        assert int(d.max()) <= 1, (br, n)
        off_ulp += int((d != 0).sum())
    print(f"{mode}: folded entries one fp32 ulp away from pack.py's: {off_ulp}")


def _native_as_stagepack(blob, cfg, m, L):
    """a native pack seen as a StagePack (pack.py's planes / vectors / layout), for DecodePlan"""
    lay, off = _lib.StageLayout(), C.c_size_t()
    _lib.check(_lib.load().ph_decode_pack_layout(C.byref(cfg), C.byref(lay), C.byref(off)), "layout")
    sp = E.StagePack.__new__(E.StagePack)
    P = 2 if m.query in (_lib.PH_PREC_SPLIT, _lib.PH_PREC_QHYBRID) else 1
    sp.wb = blob[:P * lay.wb_plane_elems * 2].view(torch.int16).reshape(P, lay.wb_plane_elems)
    nv = (_lib.load().ph_decode_pack_bytes(C.byref(cfg)) - off.value) // 4
    sp.wf = blob[off.value:].view(torch.float32)[:nv]
    sp.lay, sp.num_classes, sp.prec = lay, L, m.query
    return sp


@pytest.mark.parametrize("size", ["cfg2", "cfg5"])
def test_decode_from_native_packs_against_the_oracle(gpu, size, monkeypatch):
    """every stage packed by ph_decode_pack_stage, one frame decoded free running (NativeDecodePlan; the same run through
    DecodePlan on the same packs gives the hard masks every stage pooled with), against the oracle following those hard masks on
    the same 16-bit-rounded features: each mode's tolerance (tests/test_gpu_configs.py TOL_IDENT)"""
    wl = bench.WORKLOADS[size]
    N, L, S = wl["Nq"] + wl["n_stuff"], wl["n_thing"] + wl["n_stuff"], wl["S"]
    head = bench.build_head(wl, "fp32", torch.float32, gpu, seed=6)
    sd = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    inp = bench.synth_inputs(wl, 1, seed=15)
    HW = wl["H"] * wl["W"]
    for mode in MODES:
        m = E.MODES[mode]
        rd = m.feat_dtype
        i2 = dict(inp)
        if rd is not None:
            i2["x"], i2["dfe"] = inp["x"].to(rd).float(), inp["dfe"].to(rd).float()
        g = {k: v.to(gpu) for k, v in i2.items()}
        cfg = E.native_cfg(1, N, wl["H"], wl["W"], S, L, wl["F"], m, OUT16[mode], True)
        blobs = [E.native_pack_stage(h, cfg, gpu) for h in head.mask_head]
        nat = E.NativeDecodePlan(blobs, 1, N, wl["H"], wl["W"], m, OUT16[mode], gpu, frame_invariant=True, num_classes=L, ffn_dim=wl["F"])
        py = E.DecodePlan([_native_as_stagepack(b, cfg, m, L) for b in blobs], 1, N, wl["H"], wl["W"], m, OUT16[mode], gpu, frame_invariant=True)
        py.debug_bits = []
        x, dfe = (g["x"].to(rd), g["dfe"].to(rd)) if rd is not None else (g["x"], g["dfe"])
        for p in (nat, py):
            p.set_inputs(x, dfe, g["k0"], g["q0"], g["m0"])
            p.run()
        torch.cuda.synchronize()
        _equal_outputs(nat.outputs(), py.outputs(), (size, mode))
        hard = [torch.from_numpy(np.unpackbits(b.cpu().numpy().view("uint32").view("uint8"), axis=-1, bitorder="little")[:, :N, :HW]
                                 .astype("float32")).reshape(1, N, wl["H"], wl["W"]) for b in py.debug_bits]
        py.debug_bits = None
        with torch.no_grad():
            ref = O.iter_head_mask_preds(sd, S, i2["x"], i2["k0"], i2["m0"], i2["q0"], i2["dfe"], hard_masks=hard)
        o = nat.outputs()
        err = {n: Hh.rel_err(o[n].float().cpu(), ref[n]) for n in ("obj", "cls", "mask", "mask_up", "depth_up")}
        print(f"{size} {mode}: native packs, rel err vs the oracle on the device's hard masks", {k: f"{v:.1e}" for k, v in err.items()})
        assert max(err.values()) < TOL_IDENT[mode], (size, mode, err)
        del nat, py, blobs


def _same(a, b, path="r"):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, path


@pytest.mark.parametrize("which", ["image", "video"])
def test_module_api_switch(gpu, which):
    """`use_native_plan(True)` on the heads built from the reference's config: simple_test_mask_preds and simple_test equal the
    default path bit for bit (panoptic ids with np.array_equal), through the KernelHead hand-off and from given tensors"""
    from test_ref_configs import ref_cfg
    from polyphonicformer_amd.registry import build_heads_from_config
    import polyphonicformer_amd.kernel_head, polyphonicformer_amd.kernel_update, polyphonicformer_amd.semantic_fpn  # noqa: F401,E401
    torch.manual_seed(5)
    kh, ih = build_heads_from_config(ref_cfg(which))
    for mod in (kh, ih):
        mod.init_weights()
        mod.eval().to(gpu)
    with torch.no_grad():
        ih.mask_head[-1].fc_cls.bias.fill_(1.0)
    ih.test_cfg.merge_stuff_thing.overlap_thr = 0.0
    H8, W8 = 256, 512
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(1, 256, H8 // s, W8 // s, generator=gen).to(gpu) for s in (4, 8, 16, 32)]
    meta = [dict(img_shape=(H8, W8, 3), ori_shape=(H8, W8, 3), batch_input_shape=(H8, W8))]
    results = {}
    with torch.no_grad():
        for native in (False, True):
            ih.use_native_plan(native)
            pf, xf, mp, cs, seg, df, dp, dpr, aspp = kh.simple_test_rpn(feats, meta)
            mpreds = ih.simple_test_mask_preds(xf, pf, mp, cs, meta, depth_preds=dpr, depth_feats=df, depth_proposal=dp)
            plan = next(iter(ih._plans.values()))
            assert isinstance(plan, E.NativeDecodePlan) == native
            handoff = plan.handoff_runs
            # from given tensors (no hand-off: clones break the identity check)
            given = ih.simple_test_mask_preds(xf.clone(), pf.clone(), mp.clone(), cs, meta, depth_preds=dpr, depth_feats=df.clone(),
                                              depth_proposal=dp.clone())
            pf, xf, mp, cs, seg, df, dp, dpr, aspp = kh.simple_test_rpn(feats, meta)
            pan = ih.simple_test(xf, pf, mp, cs, meta, depth_preds=dpr, depth_feats=df, depth_proposal=dp, aspp_semantic=aspp)
            torch.cuda.synchronize()
            results[native] = (mpreds, given, pan, handoff)
    assert results[True][3] == results[False][3]
    print(f"{which}: KernelHead hand-off runs {results[True][3]}")
    _same(results[False][:3], results[True][:3])
    ih.use_native_plan(False)


def test_graph_capture_replays_the_eager_run(gpu):
    wl = bench.WORKLOADS["cfg3"]
    N = wl["Nq"] + wl["n_stuff"]
    head = bench.build_head(wl, "fp16", torch.float16, gpu, seed=3)
    packs = [h.stage_pack(gpu, "fp16") for h in head.mask_head]
    g = _inputs(wl, 2, gpu, seed=9)
    plan = E.NativeDecodePlan(packs, 2, N, wl["H"], wl["W"], "fp16", torch.float16, gpu, frame_invariant=True)
    plan.set_inputs(g["x"], g["dfe"], g["k0"], g["q0"], g["m0"])
    plan.run()
    torch.cuda.synchronize()
    eager = {k: (None if v is None else v.clone()) for k, v in plan.outputs().items()}
    plan.renew_outputs()
    plan.capture()
    for _ in range(3):
        for v in plan.outputs().values():
            if v is not None:
                v.zero_()
        plan.replay()
        torch.cuda.synchronize()
        _equal_outputs(eager, plan.outputs(), "replay")
    # new inputs reach the captured graph through set_inputs (copied into the tensors it reads)
    g2 = _inputs(wl, 2, gpu, seed=10)
    plan.set_inputs(g2["x"], g2["dfe"], g2["k0"], g2["q0"], g2["m0"])
    assert plan.graph is not None
    plan.replay()
    ref = E.DecodePlan(packs, 2, N, wl["H"], wl["W"], "fp16", torch.float16, gpu, frame_invariant=True)
    ref.set_inputs(g2["x"], g2["dfe"], g2["k0"], g2["q0"], g2["m0"])
    ref.run()
    torch.cuda.synchronize()
    _equal_outputs(ref.outputs(), plan.outputs(), "replay with new inputs")


@pytest.mark.parametrize("mode", ["fp16", "fp32"])
def test_example_program(gpu, mode, tmp_path):
    """examples/decode_c: a fresh process with no Python in it reads raw weights and inputs of a cfg3-shaped decode, packs,
    plans, runs once and writes the outputs: bit for bit DecodePlan's on the same (natively packed) weights"""
    assert os.path.exists(BLD.EXAMPLE), "built by python -m polyphonicformer_amd.build"
    wl = bench.WORKLOADS["cfg3"]
    B, N, L, S, H, W = 1, wl["Nq"] + wl["n_stuff"], wl["n_thing"] + wl["n_stuff"], wl["S"], wl["H"], wl["W"]
    m = E.MODES[mode]
    out_dtype = OUT16[mode]
    head = bench.build_head(wl, "fp32", torch.float32, gpu, seed=8)
    inp = bench.synth_inputs(wl, B, seed=21)
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    d_out.mkdir()
    (d_in / "cfg.txt").write_text(f"{B} {N} {H} {W} {S} {L} {wl['F']} {_lib.PH_MODE[mode]} {E.OUT_CODE[out_dtype]} 1\n")
    lib = _lib.load()
    for s, h in enumerate(head.mask_head):
        sd = h.state_dict()
        names = [lib.ph_decode_param_name(i).decode() for i in range(_lib.PH_DECODE_NPARAMS)]
        np.concatenate([sd[n].detach().float().cpu().numpy().reshape(-1) for n in names]).astype("<f4").tofile(d_in / f"stage{s}.bin")
    for k, f in (("x", "x"), ("dfe", "depth_feats"), ("k0", "k0"), ("q0", "q0"), ("m0", "m0")):
        inp[k].float().contiguous().numpy().astype("<f4").tofile(d_in / f"{f}.bin")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "PYTHONHOME")}
    r = subprocess.run(["timeout", "-k", "10", "240", BLD.EXAMPLE, str(d_in), str(d_out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout.strip())
    # the Python plan on the same packs
    cfg = E.native_cfg(B, N, H, W, S, L, wl["F"], m, out_dtype, True)
    blobs = [E.native_pack_stage(h, cfg, gpu) for h in head.mask_head]
    py = E.DecodePlan([_native_as_stagepack(b, cfg, m, L) for b in blobs], B, N, H, W, m, out_dtype, gpu, frame_invariant=True)
    g = {k: v.to(gpu) for k, v in inp.items()}
    py.set_inputs(g["x"], g["dfe"], g["k0"], g["q0"], g["m0"])
    py.run()
    torch.cuda.synchronize()
    o = py.outputs()
    npdt = {torch.float32: "<f4", torch.float16: "<f2", torch.bfloat16: "<u2"}
    for k in ("obj", "dobj", "cls", "mask", "mask_up", "depth_up"):
        t = o[k].cpu()
        want = (t.view(torch.int16).numpy().view("<u2") if t.dtype == torch.bfloat16 else t.numpy()).reshape(-1)
        got = np.fromfile(d_out / f"{k}.bin", dtype=npdt[t.dtype])
        assert got.shape == want.shape and np.array_equal(got.view("u1"), want.view("u1")), k
    geo = dict(line.split() for line in (d_out / "geometry.txt").read_text().splitlines())
    assert (int(geo["nsplit"]), int(geo["poolx"]), int(geo["fused_up"])) == (py.nsplit, int(py.poolx), int(py.fused_up))


# Child process of test_environment_does_not_reach_the_native_plan: captures one decode of a native plan and of the Python plan
# (same packs, the fused final stage) into graphs and prints the (grid, block, LDS) of every kernel node, as JSON.
_GRAPH_NODES = r"""
import json, sys
sys.path[:0] = [".", "tests"]
import torch
import bench
import helpers as Hh
from polyphonicformer_amd import engine as E

dev = torch.device("cuda:0")
wl = bench.WORKLOADS["cfg3"]
B, N = 4, wl["Nq"] + wl["n_stuff"]
head = bench.build_head(wl, "fp16", torch.float16, dev, seed=3)
packs = [h.stage_pack(dev, "fp16") for h in head.mask_head]
g = {k: v.to(dev) for k, v in bench.synth_inputs(wl, B, seed=5).items()}
res = {}
for name, cls in (("native", E.NativeDecodePlan), ("python", E.DecodePlan)):
    plan = cls(packs, B, N, wl["H"], wl["W"], "fp16", torch.float16, dev, frame_invariant=False)
    assert plan.fused_up
    plan.set_inputs(g["x"], g["dfe"], g["k0"], g["q0"], g["m0"])
    res[name] = Hh.graph_kernel_nodes(plan.run)
print(json.dumps(res))
"""


def test_environment_does_not_reach_the_native_plan(gpu):
    """the launch switches the public entry points take from the library's table, filled from the environment at first use
    (PH_UP2_WGS, PH_CONV_WGS, PH_QUERY_NRT), leave the native plan's launches as they are: the kernel nodes of a captured native decode
    (grid, block, LDS) are the same with and without them, while the Python plan's -- through the public entry points -- change.
    Without the variables both plans capture the same launches."""
    knobs = dict(PH_UP2_WGS="7", PH_CONV_WGS="5", PH_QUERY_NRT="1")
    base = {k: v for k, v in os.environ.items() if k not in knobs and k not in Hh.PLAN_KNOBS}
    out = {}
    for name, env in (("clean", base), ("knobs", dict(base, **knobs))):
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-c", _GRAPH_NODES], cwd=Hh.REPO, env=env, capture_output=True,
                           text=True, timeout=450)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["clean"]["native"] == out["clean"]["python"]            # the same kernel sequence and geometry
    assert out["knobs"]["native"] == out["clean"]["native"]            # the environment does not reach the native plan ...
    assert out["knobs"]["python"] != out["clean"]["python"]            # ... while it does steer the public entry points
    print("kernel nodes of one decode:", len(out["clean"]["native"]))
