"""The native KernelHead plan on the device (include/polyhead.h ph_khead_*, engine.NativeKernelHeadPlan): the packing kernel
byte for byte against engine.KernelHeadPack, bit identity with engine.KernelHeadPlan on every path, the in-call fallback, the
oracle, graph capture, the module API switch, the environment, and the Python-free program that runs the whole head."""
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
from polyphonicformer_amd.registry import HEADS, ConfigDict
import polyphonicformer_amd.kernel_head  # noqa: F401

pytestmark = pytest.mark.gpu

OUTS = ("xp", "dp", "bits", "x_f32", "dfe_f32", "mask_preds", "seg_preds", "depth_pred", "proposal")
NQ, N_THING, N_STUFF = 100, 8, 11          # num_proposals not a multiple of 32, 19 classes with 8 things
L = N_THING + N_STUFF


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    Hh.clear_plan_knobs(monkeypatch)


_HEADS = {}


def _head(precision, seed=5):
    """a KernelHead whose GroupNorm affine and biases are not trivial (shared per grade: built once), its fp32 state_dict"""
    if precision in _HEADS:
        return _HEADS[precision]
    torch.manual_seed(seed)
    h = HEADS.build(dict(type="KernelHead", num_proposals=NQ, num_classes=L, num_thing_classes=N_THING, num_stuff_classes=N_STUFF,
                         in_channels=256, out_channels=256, cat_stuff_mask=True, feat_downsample_stride=2, feat_refine_stride=1,
                         feat_refine=False, use_binary=True, conv_normal_init=True, proposal_feats_with_obj=True,
                         xavier_init_kernel=False, kernel_init_std=1, loss_seg=dict(type="FocalLoss", use_sigmoid=True),
                         localization_fpn=None))
    h.init_weights()
    with torch.no_grad():
        for n in ("loc", "seg", "depth"):
            m = getattr(h, f"{n}_convs")[0]
            m.gn.weight.add_(0.2 * torch.randn_like(m.gn.weight))
            m.gn.bias.add_(0.2 * torch.randn_like(m.gn.bias))
            m.conv.weight.mul_(8.0)
        h.conv_seg.weight.mul_(30.0)
        h.conv_seg.bias.copy_(0.5 * torch.randn_like(h.conv_seg.bias))
        h.conv_direct_depth.weight.mul_(30.0)
        h.conv_direct_depth.bias.fill_(0.37)
    sd = {k: v.detach().clone() for k, v in h.state_dict().items()}
    h.eval().to("cuda:0")
    h.set_precision(precision)
    _HEADS[precision] = (h, sd)
    return h, sd


def _native_pack(precision, gpu):
    h, sd = _head(precision)
    cfg = E.native_khead_cfg(1, 8, 16, NQ, L, N_THING, True, 32, precision)
    return E.native_khead_pack(sd, cfg, gpu), cfg


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_packing_is_kernel_head_pack_byte_for_byte(gpu, precision):
    """every piece ph_khead_pack writes against the tensor KernelHeadPack builds on the host from the same state_dict, pad rows
    included; the alignment padding is zero after packing into a poisoned buffer, so two packings are byte-equal"""
    lib = _lib.load()
    h, sd = _head(precision)
    ref = E.KernelHeadPack(sd, E.KHEAD_PREC[precision], gpu, 32)
    again, cfg = _native_pack(precision, gpu)
    params, ptrs = E._gather_params(sd, gpu, _lib.PH_KHEAD_NPARAMS, lib.ph_khead_param_name, lambda i: lib.ph_khead_param_numel(C.byref(cfg), i))
    blob = torch.full((lib.ph_khead_pack_bytes(C.byref(cfg)),), 0xA5, dtype=torch.uint8, device=gpu)
    _lib.check(lib.ph_khead_pack(C.byref(cfg), ptrs, _lib.ptr(blob), _lib.stream_ptr()), "ph_khead_pack")
    nat = E.NativeKernelHeadPack(blob, cfg)
    torch.cuda.synchronize()
    assert torch.equal(nat.blob, again.blob)
    assert (nat.prec, nat.n_init, nat.n_seg, nat.groups) == (ref.prec, ref.n_init, ref.n_seg, ref.groups)
    covered = torch.zeros_like(nat.blob, dtype=torch.bool)
    for i, name in enumerate(_lib.KPACK_PIECES):
        a, b = getattr(nat, name), getattr(ref, name)
        if b is None:
            assert a is None and nat.layout.bytes[i] == 0, name
            continue
        assert a.dtype == b.dtype and a.numel() == b.numel(), name
        assert torch.equal(_bytes(a), _bytes(b)), (name, int((_bytes(a) != _bytes(b)).sum()))
        covered[nat.layout.offset[i]:nat.layout.offset[i] + nat.layout.bytes[i]] = True
    assert bool((~covered).any()) and int(nat.blob[~covered].max()) == 0          # e.g. behind dd_bias (128 bytes)
    assert nat.init_planes.shape[1] == 128 and nat.seg_planes.shape[1] == 32          # rows zero-padded to 32
    print(f"{precision}: {nat.blob.numel()} bytes, {int((~covered).sum())} of padding")


def _pair(precision, gpu, B, H, W, cat_stuff=True, want_f32=True, logit_dtype=torch.float32, onepass=None, frame_invariant=False,
          dense=True):
    """the Python plan and the native plan on the SAME native pack"""
    pack, _ = _native_pack(precision, gpu)
    kw = dict(want_f32=want_f32, logit_dtype=logit_dtype, onepass=onepass, frame_invariant=frame_invariant)
    py = E.KernelHeadPlan(pack, B, H, W, N_THING, L, cat_stuff, gpu, **kw)
    nat = E.NativeKernelHeadPlan(pack, B, H, W, N_THING, L, cat_stuff, gpu, dense_depth_proposal=dense, **kw)
    return pack, py, nat


def _poison(p):
    for n in OUTS:
        t = getattr(p, n)
        if t is not None:
            t.fill_(float("nan")) if t.is_floating_point() else t.fill_(0x7E7E)


def _assert_equal(py, nat, what):
    for n in OUTS:
        a, b = getattr(py, n), getattr(nat, n)
        if a is None or b is None:
            assert a is None and b is None, (what, n)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, n)
        assert torch.equal(a, b), (what, n)
    assert (py.N, py.nsplit, py.onepass) == (nat.N, nat.nsplit, nat.onepass), what


def _planes_of(feats, dt, gpu):
    B, _, H, W = feats[0].shape
    HW, HWp = H * W, E.hw_padded(H * W)
    out = []
    for f in feats:
        p = torch.zeros((1, B, 256, HWp), dtype=dt, device=gpu)
        p[0, :, :, :HW] = f.reshape(B, 256, HW).to(dt)
        out.append(p.view(torch.int16))
    return out


# (H, W, B) = (8, 16, 3): one slice per frame; (48, 156, 5): H * W not a multiple of 128, more frames than frame slots
IDENT = {
    "fp16_small": ("fp16", 8, 16, 3, {}),
    "fp16_small_invariant": ("fp16", 8, 16, 3, dict(frame_invariant=True)),
    "bf16_small": ("bf16", 8, 16, 3, {}),
    "fp16_ragged": ("fp16", 48, 156, 5, {}),
    "fp16_ragged_invariant": ("fp16", 48, 156, 5, dict(frame_invariant=True)),
    "bf16_ragged": ("bf16", 48, 156, 5, {}),
    "fp32_small_twopass": ("fp32", 8, 16, 3, {}),
    "fp32_ragged_twopass": ("fp32", 48, 156, 5, {}),
    "bf16_ragged_twopass": ("bf16", 48, 156, 5, dict(onepass=False)),
    "fp16_ragged_planes": ("fp16", 48, 156, 5, dict(planes=True)),
    "bf16_small_twopass_planes": ("bf16", 8, 16, 3, dict(planes=True, onepass=False)),
    "fp16_small_no_stuff": ("fp16", 8, 16, 3, dict(cat_stuff=False)),
    "fp16_ragged_f16_logits_no_f32": ("fp16", 48, 156, 5, dict(logit_dtype=torch.float16, want_f32=False)),
}


@pytest.mark.parametrize("case", sorted(IDENT))
def test_bit_identity_with_kernel_head_plan(gpu, case):
    """the same pack bytes and the same inputs through KernelHeadPlan and NativeKernelHeadPlan: every output and hand-off buffer
    torch.equal, the same geometry chosen, and the one-pass launches themselves (no time-out) produced them"""
    precision, H, W, B, kw = IDENT[case]
    kw = dict(kw)
    planes = kw.pop("planes", False)
    pack, py, nat = _pair(precision, gpu, B, H, W, **kw)
    want_onepass = precision != "fp32" and kw.get("onepass") is not False
    assert py.onepass == nat.onepass == want_onepass, case
    feats = [f.to(gpu) for f in Hh.neck_inputs(31 + H, B, 256, H, W)]
    if planes:
        feats = _planes_of(feats, torch.float16 if precision == "fp16" else torch.bfloat16, gpu)
    for p in (py, nat):
        _poison(p)
        p.set_inputs(feats)
        p.run()
    torch.cuda.synchronize()
    assert py.timeouts() == 0 and nat.timeouts() == 0 and not nat.last_run_fell_back()
    _assert_equal(py, nat, case)
    cat = kw.get("cat_stuff", True)
    assert nat.N == NQ + (N_STUFF if cat else 0)
    assert torch.equal(nat.depth_proposal, pack.w_dd_f32.reshape(1, 1, 256).expand(B, nat.N, 256))
    if "ragged" in case and "invariant" in case:      # at B = 5 the one-frame split differs from the batch's
        assert nat.nsplit == E.default_nsplit(1, H * W) != E.default_nsplit(B, H * W)
    # a second run into renewed outputs gives the same bits
    first = {n: getattr(nat, n) for n in OUTS}
    nat.renew_outputs()
    nat.run()
    torch.cuda.synchronize()
    for n in OUTS:
        if first[n] is not None:
            assert first[n].data_ptr() != getattr(nat, n).data_ptr() and torch.equal(first[n], getattr(nat, n)), (case, n)
    print(f"{case}: onepass {nat.onepass} nsplit {nat.nsplit} N {nat.N}: equal")


def test_onepass_rule_and_forced_form(gpu):
    """AUTO is KernelHeadPlan's rule on this device; ON where the kernel cannot run is an error, not a silent two-pass plan"""
    pack, _ = _native_pack("fp16", gpu)
    lib = _lib.load()
    for H, W in ((8, 16), (48, 156), (7, 9)):       # 63 pixels: the fp32 input form needs H * W % 4 == 0
        sup = bool(lib.ph_khead_onepass_supported(2, H * W, 32, _lib.PH_PREC_F16, _lib.PH_IN_F32_NCHW))
        assert E.NativeKernelHeadPlan(pack, 2, H, W, N_THING, L, True, gpu).onepass == sup
        assert E.KernelHeadPlan(pack, 2, H, W, N_THING, L, True, gpu).onepass == sup
    assert not sup
    with pytest.raises(_lib.PolyheadError, match="ph_khead_onepass cannot run"):
        E.NativeKernelHeadPlan(pack, 2, 7, 9, N_THING, L, True, gpu, onepass=True)
    pack32, _ = _native_pack("fp32", gpu)
    with pytest.raises(_lib.PolyheadError):
        E.NativeKernelHeadPlan(pack32, 2, 8, 16, N_THING, L, True, gpu, logit_dtype=torch.float16)


def test_fallback_inside_the_native_call(gpu):
    """tests/test_gpu_khead1.py test_onepass_timeout_falls_back_inside_the_same_call's mechanism, once, at its smallest shape: a
    kernel on another stream holds 200 CUs' LDS (ph_selftest_hog), the hand-off bound is 0.5 ms, the one-pass launch of the native
    run gives up and the predicated two-pass kernels inside the SAME ph_khead_plan_run leave the two-pass plan's results."""
    import time
    lib = _lib.load()
    H, W, B = 48, 156, 5
    pack, _ = _native_pack("fp16", gpu)
    nat = E.NativeKernelHeadPlan(pack, B, H, W, N_THING, L, True, gpu, onepass=True)
    two = E.KernelHeadPlan(pack, B, H, W, N_THING, L, True, gpu, onepass=False)
    feats = [f.to(gpu) for f in Hh.neck_inputs(21, B, 256, H, W)]
    for p in (nat, two):
        p.set_inputs(feats)
    two.run()
    scratch = torch.zeros(4, dtype=torch.int32, device=gpu)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):     # first launch of the hog kernel (code-object load) outside the timed choreography
        _lib.check(lib.ph_selftest_hog(1, 1024, 1, _lib.ptr(scratch), _lib.stream_ptr()), "ph_selftest_hog")
    nat.run()                          # undisturbed: one pass
    torch.cuda.synchronize()
    assert nat.timeouts() == 0 and not nat.last_run_fell_back()
    try:
        lib.ph_khead_onepass_set_timeout_us(500)
        _poison(nat)
        scratch.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            _lib.check(lib.ph_selftest_hog(200, 100 * 1024, 40 * 1000, _lib.ptr(scratch), _lib.stream_ptr()), "ph_selftest_hog")
        t0 = time.perf_counter()
        while int(scratch[1]) < 190 and time.perf_counter() - t0 < 0.02:
            pass
        assert int(scratch[1]) >= 190, "the hog did not start in time"
        nat.run()
        torch.cuda.synchronize()
        fell_back, timeouts = nat.last_run_fell_back(), nat.timeouts()
        errs = {n: Hh.rel_err(getattr(nat, n).float().cpu(), getattr(two, n).float().cpu())
                for n in ("x_f32", "dfe_f32", "mask_preds", "seg_preds", "depth_pred", "proposal")}
        print(f"fell back {fell_back}, time-outs {timeouts}, rel err against the two-pass plan", {k: f"{v:.1e}" for k, v in errs.items()},
              "bit-identical" if all(torch.equal(getattr(nat, n), getattr(two, n)) for n in OUTS) else "")
        assert max(errs.values()) < 1e-3, errs                      # correct whichever form produced them
        want = (nat.mask_preds.reshape(B, nat.N, H * W) > 1.5 * 2.0 ** -24)
        got = torch.from_numpy(np.unpackbits(nat.bits.cpu().numpy().view("uint32").view("uint8"), axis=-1, bitorder="little")
                               .astype(bool))
        assert torch.equal(got[:, :nat.N, :H * W], want.cpu()) and not got[:, nat.N:].any()
        assert fell_back and timeouts > 0, "the hog did not run beside the launch: the fallback was not exercised"
        assert lib.ph_khead_plan_status(nat._h, _lib.stream_ptr()) == 1
    finally:
        lib.ph_khead_onepass_set_timeout_us(0)
        torch.cuda.synchronize()
    nat.run()                          # and the next undisturbed run is one pass again; the time-out count is sticky
    torch.cuda.synchronize()
    assert not nat.last_run_fell_back() and nat.timeouts() == timeouts


def test_native_pack_against_the_oracle(gpu):
    """fp16 grade at (6, 14, 2), weights packed by ph_khead_pack, against the CPU restatement of kernel_head.py:245-347: the
    tensors and the bound of tests/test_gpu_khead1.py test_onepass_vs_oracle (1e-3).  (proposal_feats is not among them: at 84
    pixels one hard-mask bit of a logit next to zero moves a pooled feature by 1e-2 of the largest entry; the identity tests
    compare it bit for bit with KernelHeadPlan's, the fallback test of test_gpu_khead1.py with the oracle at 7 488 pixels.)"""
    H, W, B = 6, 14, 2
    h, sd = _head("fp16")
    pack, _ = _native_pack("fp16", gpu)
    feats = Hh.neck_inputs(5, B, 256, H, W)
    ref = O.kernel_head_post_neck(sd, *feats, N_THING, L, 32)
    nat = E.NativeKernelHeadPlan(pack, B, H, W, N_THING, L, True, gpu, onepass=True)
    nat.set_inputs([f.to(gpu) for f in feats])
    nat.run()
    torch.cuda.synchronize()
    assert nat.onepass and nat.timeouts() == 0
    for name, t in (("x_feats", nat.x_f32), ("mask_preds", nat.mask_preds), ("seg_preds", nat.seg_preds),
                    ("depth_feats", nat.dfe_f32), ("depth_pred", nat.depth_pred)):
        e = Hh.rel_err(t.float().cpu().reshape(ref[name].shape), ref[name])
        print("native pack + plan, fp16 grade vs oracle", name, f"{e:.1e}")
        assert e < 1e-3, (name, e)


def test_graph_capture_replays_the_eager_run(gpu):
    H, W, B = 48, 156, 2
    pack, py, nat = _pair("fp16", gpu, B, H, W)
    feats = [f.to(gpu) for f in Hh.neck_inputs(7, B, 256, H, W)]
    nat.set_inputs(feats)              # contiguous fp32 device maps are read where they are: the graph keeps reading `feats`
    nat.run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nat.run()
    for seed in (8, 9):
        new = Hh.neck_inputs(seed, B, 256, H, W)
        for dst, src in zip(feats, new):
            dst.copy_(src)
        _poison(nat)
        g.replay()
        py.set_inputs([f.clone() for f in feats])
        py.run()
        torch.cuda.synchronize()
        _assert_equal(py, nat, f"replay, inputs of seed {seed}")
    assert nat.timeouts() == 0


def test_module_api_switch(gpu):
    """KernelHead.use_native_plan(True): the 9-tuple of simple_test_rpn is torch.equal to the default path's, again after an
    in-place weight change (the native pack is rebuilt), and the hand-off feeds KernelUpdateIterHead unchanged"""
    wl = dict(H=16, W=40, Nq=NQ, n_thing=N_THING, n_stuff=N_STUFF, S=2, F=2048)
    kh, _ = _head("fp16")
    ih = bench.build_head(wl, "fp16", torch.float16, gpu, seed=3)
    ih.frame_invariant = True
    B = 2
    feats = [f.to(gpu) for f in Hh.neck_inputs(13, B, 256, wl["H"], wl["W"])]
    meta = [dict(img_shape=(128, 320, 3), ori_shape=(128, 320, 3), batch_input_shape=(128, 320))] * B

    def both():
        res = {}
        for native in (False, True):
            kh.use_native_plan(native)
            with torch.no_grad():
                out = kh.simple_test_rpn(feats, meta)
                plan = next(iter(kh._plans.values()))
                assert isinstance(plan, E.NativeKernelHeadPlan) == native
                assert isinstance(kh._pack[1], E.NativeKernelHeadPack) == native
                pf, xf, mp, cs, seg, df, dp, dpr, aspp = out
                before = next(iter(ih._plans.values())).handoff_runs if ih._plans else 0
                dec = ih.simple_test_mask_preds(xf, pf, mp, cs, meta, depth_preds=dpr, depth_feats=df, depth_proposal=dp)
                assert next(iter(ih._plans.values())).handoff_runs == before + 1       # the planes and bits were adopted
            torch.cuda.synchronize()
            res[native] = (out, dec)
        return res

    def same(a, b, path="r"):
        if isinstance(a, torch.Tensor):
            assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f"{path}[{i}]")
        elif isinstance(a, dict):
            assert a.keys() == b.keys(), path
            for k in a:
                same(a[k], b[k], f"{path}.{k}")
        else:
            assert a == b, path

    try:
        r = both()
        assert len(r[True][0]) == 9
        same(r[False], r[True])
        ho_a, ho_b = r[False][0][1]._ph_handoff, r[True][0][1]._ph_handoff
        assert ho_a["prec"] == ho_b["prec"]
        for k in ("xp", "dp", "bits"):
            assert torch.equal(ho_a[k], ho_b[k]), k
        with torch.no_grad():          # in-place: the parameters' version counters move, both packs are rebuilt
            kh.init_kernels.weight.mul_(-1.5)
            kh.conv_seg.bias.add_(0.25)
            kh.seg_convs[0].gn.weight.mul_(1.1)
        r2 = both()
        same(r2[False], r2[True])
        assert not torch.equal(r[True][0][2], r2[True][0][2])
    finally:
        kh.use_native_plan(False)
        _HEADS.pop("fp16", None)       # the shared head's weights were changed


# Child process of test_environment_does_not_reach_the_native_plan: captures one a1 call of a native plan (an explicit, zero-
# initialised cfg: the module API's) and of the Python plan into graphs and prints the (grid, block, LDS) of every kernel node.
_GRAPH_NODES = r"""
import json, sys
sys.path[:0] = [".", "tests"]
import torch
import helpers as Hh
from polyphonicformer_amd import _lib, engine as E
import test_gpu_native_khead as T

dev = torch.device("cuda:0")
B, H, W = 2, 48, 156
h, sd = T._head("fp16")
cfg = _lib.KheadCfg(B=1, H=8, W=16, num_proposals=T.NQ, num_classes=T.L, num_thing_classes=T.N_THING, cat_stuff=1, groups=32,
                    mode=_lib.PH_MODE["fp16"], emit_f32=1)
pack = E.native_khead_pack(sd, cfg, dev)
cfg.B, cfg.H, cfg.W = B, H, W
feats = [f.to(dev) for f in Hh.neck_inputs(3, B, 256, H, W)]
res = {}
nat = E.NativeKernelHeadPlan(pack, B, H, W, T.N_THING, T.L, True, dev, cfg=cfg)
py = E.KernelHeadPlan(pack, B, H, W, T.N_THING, T.L, True, dev)
for name, plan in (("native", nat), ("python", py)):
    plan.set_inputs(feats)
    res[name] = Hh.graph_kernel_nodes(plan.run)
res["onepass"] = [bool(nat.onepass), bool(py.onepass)]
print(json.dumps(res))
"""


def test_environment_does_not_reach_the_native_plan(gpu):
    """PH_KHEAD_TWOPASS and PH_POOL_NSPLIT (read by the Python plan) and PH_KHEAD1_PAIR (a switch of the one-pass kernel that no
    longer exists: nothing reads it) leave the launches of a native plan built from an explicit cfg as they are -- the kernel nodes of a captured run (grid, block, LDS)
    are the same with and without them -- while the Python plan's change.  Without the variables both plans capture the same
    launches."""
    knobs = dict(PH_KHEAD1_PAIR="1", PH_KHEAD_TWOPASS="1", PH_POOL_NSPLIT="3")
    base = {k: v for k, v in os.environ.items() if k not in Hh.PLAN_KNOBS}
    out = {}
    for name, env in (("clean", base), ("knobs", dict(base, **knobs))):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _GRAPH_NODES], cwd=Hh.REPO, env=env, capture_output=True,
                           text=True, timeout=350)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["clean"]["onepass"] == [True, True] and out["knobs"]["onepass"] == [True, False]
    assert out["clean"]["native"] == out["clean"]["python"]            # the same kernel sequence and geometry
    assert out["knobs"]["native"] == out["clean"]["native"]            # the environment does not reach the native plan ...
    assert out["knobs"]["python"] != out["clean"]["python"]            # ... while it does steer the Python plan
    print("kernel nodes of one a1 call:", len(out["clean"]["native"]))


def _raw(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.numpy().reshape(-1).view("u1")


@pytest.mark.parametrize("case", ["cfg3_fp16", "ragged_bf16_mixed16"])
def test_head_program(gpu, case, tmp_path):
    """examples/head_c: a fresh process with no Python in it goes from the neck's three maps to the panoptic maps -- both heads
    packed natively, ph_khead_plan_run -> ph_decode_run -> ph_upsample2x -> ph_panoptic_merge -- and every file it writes is byte-
    equal to the Python chain on the same native packs: KernelHeadPlan -> DecodePlan.run_from_planes -> upsample2x -> BatchMerge"""
    from polyphonicformer_amd.panoptic import BatchMerge, DEPTH_MODES
    from test_gpu_native_plan import _native_as_stagepack
    assert os.path.exists(BLD.HEAD_EXAMPLE), "built by python -m polyphonicformer_amd.build"
    kmode, dmode, H, W, B = dict(cfg3_fp16=("fp16", "fp16", 128, 256, 1), ragged_bf16_mixed16=("bf16", "mixed16", 48, 156, 2))[case]
    wl = dict(H=H, W=W, Nq=NQ, n_thing=N_THING, n_stuff=N_STUFF, S=3, F=2048)
    S, F, N = wl["S"], wl["F"], NQ + N_STUFF
    out_dtype = torch.float16
    m = E.MODES[dmode]
    kh, ksd = _head(kmode)
    ih = bench.build_head(wl, "fp32", torch.float32, gpu, seed=8)
    ih.test_cfg = ConfigDict(max_per_img=NQ, mask_thr=0.5, merge_stuff_thing=dict(overlap_thr=0.0, instance_score_thr=0.3))
    with torch.no_grad():              # un-trained heads: let segments pass the score threshold and the overlap test
        ih.mask_head[-1].fc_cls.bias.fill_(1.0)
    depth_mode = DEPTH_MODES[ih.mask_head[-1].depth_act_mode]
    meta = dict(img_shape=(8 * H, 8 * W, 3), ori_shape=(8 * H, 8 * W, 3), batch_input_shape=(8 * H, 8 * W))
    feats = Hh.neck_inputs(17, B, 256, H, W)
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    d_out.mkdir()
    geom = [2 * H, 2 * W, 8 * H, 8 * W, 8 * H, 8 * W, 8 * H, 8 * W]
    (d_in / "cfg.txt").write_text(" ".join(str(v) for v in [B, H, W, NQ, L, N_THING, 32, _lib.PH_MODE[kmode], 1, S, F, _lib.PH_MODE[dmode],
                                                            E.OUT_CODE[out_dtype], 1, NQ, depth_mode] + geom + [0.3, 0.0]) + "\n")
    lib = _lib.load()
    tofile = lambda ts, name: np.concatenate([t.detach().float().cpu().numpy().reshape(-1) for t in ts]).astype("<f4").tofile(d_in / name)
    tofile([ksd[lib.ph_khead_param_name(i).decode()] for i in range(_lib.PH_KHEAD_NPARAMS)], "khead.bin")
    for s, st in enumerate(ih.mask_head):
        sd = st.state_dict()
        tofile([sd[lib.ph_decode_param_name(i).decode()] for i in range(_lib.PH_DECODE_NPARAMS)], f"stage{s}.bin")
    for i, f in enumerate(feats):
        tofile([f], f"f{i}.bin")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "PYTHONHOME") and k not in Hh.PLAN_KNOBS}
    r = subprocess.run(["timeout", "-k", "10", "240", BLD.HEAD_EXAMPLE, str(d_in), str(d_out)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(r.stdout.strip())

    # the Python chain on the same native packs
    kcfg = E.native_khead_cfg(B, H, W, NQ, L, N_THING, True, 32, kmode, frame_invariant=True)
    kpack = E.native_khead_pack(ksd, kcfg, gpu)
    kp = E.KernelHeadPlan(kpack, B, H, W, N_THING, L, True, gpu, want_f32=True, frame_invariant=True)
    kp.set_inputs([f.to(gpu) for f in feats])
    kp.run()
    dcfg = E.native_cfg(B, N, H, W, S, L, F, m, out_dtype, True)
    blobs = [E.native_pack_stage(st, dcfg, gpu) for st in ih.mask_head]
    dp = E.DecodePlan([_native_as_stagepack(b, dcfg, m, L) for b in blobs], B, N, H, W, m, out_dtype, gpu, frame_invariant=True)
    q0 = kpack.w_dd_f32.reshape(1, 1, 256).expand(B, N, 256).contiguous()
    dp.run_from_planes(kp.xp, kp.dp, kp.bits, kp.proposal, q0)
    d0 = E.upsample2x(kp.depth_pred)
    o = dp.outputs()
    bm = BatchMerge(ih, B, N, L, 2 * H, 2 * W, out_dtype, meta, gpu)
    bm.run(o["cls"], o["mask_up"], o["depth_up"], d0)
    torch.cuda.synchronize()
    assert kp.timeouts() == 0
    want = dict(xp=kp.xp, dp=kp.dp, bits=kp.bits, x_f32=kp.x_f32, dfe_f32=kp.dfe_f32, mask_preds=kp.mask_preds, seg_preds=kp.seg_preds,
                depth_pred=kp.depth_pred, proposal=kp.proposal, depth_proposal=q0, obj=o["obj"], dobj=o["dobj"], cls=o["cls"],
                mask=o["mask"], mask_up=o["mask_up"], depth_up=o["depth_up"], depth_init_up=d0, pan=bm.pan, depth_basic=bm.d_basic,
                depth_final=bm.d_final, seg_records=bm.records)
    written = sorted(p.name for p in d_out.iterdir())
    assert written == sorted([f"{k}.bin" for k in want] + ["geometry.txt"])
    for k, t in want.items():
        got = np.fromfile(d_out / f"{k}.bin", dtype="u1")
        w = _raw(t)
        assert got.shape == w.shape and np.array_equal(got, w), k
    geo = dict(line.split() for line in (d_out / "geometry.txt").read_text().splitlines())
    assert (int(geo["khead_onepass"]), int(geo["khead_nsplit"]), int(geo["N"]), int(geo["fell_back"]), int(geo["timeouts"])) == \
        (int(kp.onepass), kp.nsplit, kp.N, 0, 0)
    assert (int(geo["nsplit"]), int(geo["nsplit_px"]), int(geo["poolx"]), int(geo["fused_up"])) == \
        (dp.nsplit, dp.nsplit_px, int(dp.poolx), int(dp.fused_up))
    assert int(geo["K"]) == bm.K and int(bm.records[:, 0].min()) > 0          # the merge accepted segments in every frame


# ---- engine.KernelHeadPlan asks the library (ph_khead_geometry_of) ----------------------------------------------------------------
def _asked(plan):
    g = _lib.KheadGeometry()
    with torch.cuda.device(plan.xp.device):
        assert _lib.load().ph_khead_geometry_of(C.byref(plan.cfg), C.byref(g)) == 0, Hh.last_error()
    assert (plan.onepass, plan.nsplit) == (bool(g.onepass), g.nsplit)
    return g


def test_kernel_head_plan_takes_its_choices_from_the_library(gpu, monkeypatch):
    """one pass or two and the pooling split of a KernelHeadPlan are ph_khead_geometry_of's answer for the plan's own cfg, with and
    without the two environment switches; a cfg the library refuses is a PolyheadError with its message.
    PH_POOL_NSPLIT=3 is checked at 8 x 32, the smallest map of this height with three 64-pixel chunks: at 8 x 16 (128 pixels, two
    chunks) a split of 3 is out of the pooling kernel's range, which the library now says when the plan is built"""
    pack, _ = _native_pack("fp16", gpu)
    lib = _lib.load()
    plan = lambda H, W, **kw: E.KernelHeadPlan(pack, 2, H, W, N_THING, L, True, gpu, **kw)
    sup = bool(lib.ph_khead_onepass_supported(2, 8 * 16, 32, _lib.PH_PREC_F16, _lib.PH_IN_F32_NCHW))
    p = plan(8, 16)
    assert sup and p.onepass == bool(_asked(p).onepass) == sup
    monkeypatch.setenv("PH_KHEAD_TWOPASS", "1")
    p = plan(8, 16)
    assert not p.onepass and _asked(p).onepass == 0
    monkeypatch.delenv("PH_KHEAD_TWOPASS")
    monkeypatch.setenv("PH_POOL_NSPLIT", "3")
    p = plan(8, 32)
    assert p.nsplit == 3 and _asked(p).nsplit == 3 and p.partial.shape[1] == 3
    with pytest.raises(_lib.PolyheadError, match="nsplit out of range"):
        plan(8, 16)
    monkeypatch.delenv("PH_POOL_NSPLIT")
    p = plan(7, 9)                                   # 63 pixels: the fp32 input form needs H * W % 4 == 0
    assert not p.onepass and _asked(p).onepass == 0
    with pytest.raises(_lib.PolyheadError, match="ph_khead_onepass cannot run"):
        plan(7, 9, onepass=True)
    pack32, _ = _native_pack("fp32", gpu)
    with pytest.raises(_lib.PolyheadError, match="one-pass form"):
        E.KernelHeadPlan(pack32, 2, 8, 16, N_THING, L, True, gpu, logit_dtype=torch.float16)


def test_module_plan_cache_follows_the_environment(gpu, monkeypatch):
    """KernelHead's plan cache is keyed by the plan's cfg: PH_KHEAD_TWOPASS=1 set between two calls builds another plan"""
    kh, _ = _head("fp16")
    kh.use_native_plan(False)
    B, H, W = 2, 8, 16
    feats = [f.to(gpu) for f in Hh.neck_inputs(17, B, 256, H, W)]
    meta = [dict(img_shape=(64, 128, 3), ori_shape=(64, 128, 3), batch_input_shape=(64, 128))] * B
    with torch.no_grad():
        kh.simple_test_rpn(feats, meta)
        p1 = next(iter(kh._plans.values()))
        assert p1.onepass
        monkeypatch.setenv("PH_KHEAD_TWOPASS", "1")
        kh.simple_test_rpn(feats, meta)
        p2 = next(iter(kh._plans.values()))
    torch.cuda.synchronize()
    assert p2 is not p1 and not p2.onepass and len(kh._plans) == 1
    assert p1.timeouts() == 0
