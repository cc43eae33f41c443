"""The backbone's training path on the device (csrc/ph_resnet_train.hip, engine.ResNetTrainPlan, train.resnet_forward_train):
ph_conv_cl_bwd_data and ph_conv_cl_bwd_weight against float64 on the bf16 operands they read, the fold backward against the float64
formulas, the transposed pack and the gradient ingest exactly, and the module against float64 autograd of `_forward_torch` on the CPU
(which tests/test_resnet_train_host.py pins to the reference class through tests/golden/resnet_train.npz).

Bound of the kernel tests (the rule of tests/test_gpu_resnet.py): every element of a bf16 output within 2^-8 |ref| + max(4 e_ref, 1e-6)
max|ref| of the float64 result, every element of an fp32 output within max(4 e_ref, 1e-6) max|ref|; e_ref = helpers.rel_err of
torch's fp32 CPU run of the same operands against float64."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
import resnet_cases
import resnet_train_cases as TC
from polyphonicformer_amd import _lib, engine as E, registry, train as T
from polyphonicformer_amd.pack import pack_b32
import polyphonicformer_amd.resnet as RN  # noqa: F401

pytestmark = pytest.mark.gpu

FACTOR, FLOOR, U16 = 4.0, 1e-6, 2.0 ** -8
GUARD = 4096


def _q(t):
    r = t.float().bfloat16()
    return r.double(), r.view(torch.int16)


def _val(bits):
    return bits.view(torch.bfloat16).double()


def _cl(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).contiguous()


def _check(tag, got, ref, ref32, rtol):
    e_ref = Hh.rel_err(ref32, ref)
    bound = max(FACTOR * e_ref, FLOOR)
    need = Hh.needed_atol(got, ref, rtol=rtol)
    print(tag, "needed atol", need, "bound", bound, "e_ref", e_ref, "rel_err", Hh.rel_err(got, ref))
    assert need <= bound, (tag, need, bound)


# the (k, s, cin, cout) list and the sizes of tests/test_gpu_resnet.py
SHAPES = [(1, 1, 64, 64), (1, 1, 64, 256), (1, 1, 2048, 512), (1, 1, 512, 2048), (1, 2, 256, 512), (1, 2, 1024, 2048), (3, 1, 64, 64),
          (3, 2, 128, 128), (3, 1, 512, 512), (3, 2, 512, 512)]
BIG = [(1, 1, 64, 256), (3, 1, 64, 64), (3, 2, 128, 128)]
CONV_CASES = [s + g for s in SHAPES for g in ((5, 9), (13, 19))] + [s + (33, 70) for s in BIG] + \
    [s + (6, 10) for s in SHAPES if s[1] == 2]
# the data gradient's wider tiles (rc_geometry on the INPUT map and Cin): 128 x 128 once ceil(HW / 128) (Cin / 128) >= 256, 128 x 64
# once ceil(HW / 128) (Cin / 64) >= 256 -- the smallest maps that select each, a last pixel tile that is not full, stride 1 and 2
WIDE_DATA = [(1, 1, 2048, 64, 33, 70, 128, 128), (3, 2, 2048, 64, 33, 70, 128, 128), (3, 1, 64, 64, 128, 257, 128, 64),
             (1, 2, 64, 64, 129, 257, 128, 64)]


def _operands(k, s, cin, cout, H, W, B=2):
    g = torch.Generator().manual_seed(7000 * k + 300 * s + cin + 3 * cout + 5 * H + W)
    Ho, Wo = E.conv_out_size(H, k, s), E.conv_out_size(W, k, s)
    zq, zb = _q(torch.randn(B, cout, Ho, Wo, generator=g))
    xq, xb = _q(torch.randn(B, cin, H, W, generator=g))
    wq, wb = _q(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5)
    return g, Ho, Wo, zq, zb, xq, xb, wq, wb


def _wt_host(wb, k, cin, cout):
    """the data gradient's B operand from the bf16 weight bits [cout, cin, k, k]: WT[c][t * cout + n] = W[n][taps - 1 - t][c]"""
    w2 = wb.permute(0, 2, 3, 1).reshape(cout, k * k, cin).flip(1)
    return pack_b32(w2.permute(2, 1, 0).reshape(cin, k * k * cout).contiguous()).contiguous()


@pytest.mark.parametrize("k,s,cin,cout,H,W,tm,tn", [c + (64, 64) for c in CONV_CASES] + WIDE_DATA)
def test_conv_cl_bwd_data_against_float64(gpu, k, s, cin, cout, H, W, tm, tn):
    B = 2
    assert _lib.load().ph_conv_cl_bwd_data_workgroups(k, s, cin, cout, H, W, B) == B * ((H * W + tm - 1) // tm) * (cin // tn)
    g, Ho, Wo, zq, zb, _, _, wq, wb = _operands(k, s, cin, cout, H, W)
    ref0 = torch.nn.grad.conv2d_input((B, cin, H, W), wq, zq, stride=s, padding=k // 2)
    ref0_32 = torch.nn.grad.conv2d_input((B, cin, H, W), wq.float(), zq.float(), stride=s, padding=k // 2)
    rq, rb = _q(torch.randn(B, cin, H, W, generator=g))
    Hr, Wr = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    r2q, r2b = _q(torch.randn(B, cin, Hr, Wr, generator=g))
    spread = torch.zeros(B, cin, H, W, dtype=torch.float64)
    spread[:, :, ::2, ::2] = r2q
    m = torch.randn(B, cin, H, W, generator=g) + 0.52                 # about 70 % positive
    m.view(-1)[::7] = 0.0
    m.view(-1)[3::11] = -0.0
    mq, mb = _q(m)
    keep = (mq > 0).double()
    assert 0.5 < float(keep.mean()) < 0.8 and bool((mb == -32768).any()) and bool((mb == 0).any())       # -0 and +0 are there
    wt = _wt_host(wb, k, cin, cout).to(gpu)
    z_d, r_d, r2_d, m_d = _cl(zb).to(gpu), _cl(rb).to(gpu), _cl(r2b).to(gpu), _cl(mb).to(gpu)
    n = B * H * W * cin
    forms = [("plain", None, 1, None, ref0, ref0_32), ("M", None, 1, m_d, ref0 * keep, ref0_32 * keep.float()),
             ("R+M", r_d, 1, m_d, (ref0 + rq) * keep, (ref0_32 + rq.float()) * keep.float()),
             ("R2", r2_d, 2, None, ref0 + spread, ref0_32 + spread.float())]
    for name, r, rs, mm, ref, ref32 in forms:
        out = torch.full((n + GUARD,), 0x7FFF, dtype=torch.int16, device=gpu)
        E.conv_cl_bwd_data(z_d, wt, r, rs, mm, out, k, s, B, H, W, cin, cout)
        o = out.cpu()
        assert bool((o[n:] == 0x7FFF).all()), "the launch wrote behind the plane"
        got = _val(o[:n]).reshape(B, H, W, cin).permute(0, 3, 1, 2)
        _check(f"bwd_data {(k, s, cin, cout, H, W)} {name}", got, ref, ref32, U16)
        if mm is not None:
            assert bool((got[keep == 0] == 0).all())


def _nsplits(chunks):
    """0 (the rule), 1, one that leaves the last range short (where the chunk count has one), the largest legal one"""
    short = [n for n in range(2, chunks) if chunks % -(-chunks // n)]
    return sorted({0, 1, chunks} | set(short[:1]))


@pytest.mark.parametrize("k,s,cin,cout,H,W", CONV_CASES)
def test_conv_cl_bwd_weight_against_float64(gpu, k, s, cin, cout, H, W):
    B, lib = 2, _lib.load()
    g, Ho, Wo, zq, zb, xq, xb, _, _ = _operands(k, s, cin, cout, H, W)
    K = k * k * cin
    to2 = lambda t: t.permute(0, 2, 3, 1).reshape(cout, K)
    ref = to2(torch.nn.grad.conv2d_weight(xq, (cout, cin, k, k), zq, stride=s, padding=k // 2))
    ref32 = to2(torch.nn.grad.conv2d_weight(xq.float(), (cout, cin, k, k), zq.float(), stride=s, padding=k // 2))
    rb, rb32 = zq.sum((0, 2, 3)), zq.float().sum((0, 2, 3))
    z_d, x_d = _cl(zb).to(gpu), _cl(xb).to(gpu)
    chunks = B * ((Ho * Wo + 63) // 64)
    rule = lib.ph_conv_cl_bwd_weight_nsplit(k, s, cin, cout, H, W, B)
    assert 1 <= rule <= chunks
    runs = {}
    for ns in _nsplits(chunks):
        pf = lib.ph_conv_cl_bwd_weight_partial_floats(k, s, cin, cout, H, W, B, ns)
        eff = ns or rule
        assert pf == (0 if eff == 1 else eff * (cout * K + cout))
        partial = torch.empty((max(pf, 4),), device=gpu)
        for rep in range(2):
            dw = torch.full((cout * K + GUARD,), float("nan"), device=gpu)
            db = torch.full((cout + GUARD,), float("nan"), device=gpu)
            E.conv_cl_bwd_weight(z_d, x_d, dw, db, partial, ns, k, s, B, H, W, cin, cout)
            dwc, dbc = dw.cpu(), db.cpu()
            assert bool(dwc[cout * K:].isnan().all()) and bool(dbc[cout:].isnan().all()), "the launch wrote behind its outputs"
            runs.setdefault(ns, []).append((dwc[:cout * K].reshape(cout, K), dbc[:cout]))
        (a, ab), (b_, bb) = runs[ns]
        assert torch.equal(a, b_) and torch.equal(ab, bb), "two runs differ in bits"
        _check(f"bwd_weight {(k, s, cin, cout, H, W)} nsplit={ns} dW", a, ref, ref32, 0.0)
        _check(f"bwd_weight {(k, s, cin, cout, H, W)} nsplit={ns} db", ab, rb, rb32, 0.0)
    # one range too many: refused with nothing written
    dw = torch.full((cout * K,), float("nan"), device=gpu)
    db = torch.full((cout,), float("nan"), device=gpu)
    partial = torch.full((16,), float("nan"), device=gpu)
    rc = lib.ph_conv_cl_bwd_weight(_lib.ptr(z_d), _lib.ptr(x_d), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(partial), chunks + 1, k, s, B, H, W,
                                   cin, cout, _lib.stream_ptr())
    assert rc == _lib.PH_EINVAL and "ph_conv_cl_bwd_weight" in Hh.last_error()
    assert lib.ph_conv_cl_bwd_weight_partial_floats(k, s, cin, cout, H, W, B, chunks + 1) == _lib.PH_EINVAL
    torch.cuda.synchronize()
    assert bool(dw.isnan().all()) and bool(db.isnan().all()) and bool(partial.isnan().all())


def test_bwd_argument_errors_launch_nothing(gpu):
    lib = _lib.load()
    z = torch.zeros(1, 30, 128, dtype=torch.int16, device=gpu)
    wt = torch.zeros(128 * 9 * 128, dtype=torch.int16, device=gpu)
    out = torch.full((1, 30, 128), 0x1234, dtype=torch.int16, device=gpu)

    def call(k, cin, cout, dx=out, rs=1, r=None):
        return lib.ph_conv_cl_bwd_data(_lib.ptr(z), _lib.ptr(wt), _lib.ptr(r), rs, None, _lib.ptr(dx), k, 1, 1, 5, 6, cin, cout, _lib.stream_ptr())
    for args in ((1, 96, 128), (1, 128, 96), (5, 128, 128), (1, 128, 128, None), (1, 128, 4096), (1, 128, 128, out, 3, z)):
        assert call(*args) == _lib.PH_EINVAL, args
        assert "ph_conv_cl_bwd_data" in Hh.last_error()
    assert lib.ph_conv_cl_bwd_data_workgroups(5, 1, 128, 128, 5, 6, 1) == _lib.PH_EINVAL
    assert lib.ph_conv_cl_bwd_weight_nsplit(3, 3, 128, 128, 5, 6, 1) == _lib.PH_EINVAL
    g = torch.zeros(1, 128, 30, device=gpu)
    assert lib.ph_nchw_grad_to_cl(_lib.ptr(g), None, None, _lib.ptr(out), 1, 30, 96, _lib.stream_ptr()) == _lib.PH_EINVAL
    assert lib.ph_nchw_grad_to_cl(None, None, None, _lib.ptr(out), 1, 30, 128, _lib.stream_ptr()) == _lib.PH_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0x1234).all())
    assert call(1, 128, 128) == 0
    torch.cuda.synchronize()
    assert not bool((out == 0x1234).any())


# ---- the small kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("k,cin,cout", [(1, 64, 256), (3, 128, 128), (1, 1024, 2048)])
def test_fold_bwd_against_the_float64_formulas(gpu, eps, k, cin, cout):
    p = TC.fold_case(k, cin, cout, seed=k + cin + cout)
    dw64, dg64, db64 = TC.fold_bwd_formulas(p["dwp"].double(), p["db"].double(), p["w"].double(), p["gamma"].double(),
                                            p["mean"].double(), p["var"].double(), eps)
    dw32, dg32, db32 = TC.fold_bwd_formulas(p["dwp"], p["db"], p["w"], p["gamma"], p["mean"], p["var"], eps)
    d = {n: t.to(gpu) for n, t in p.items()}
    for want_bn in (True, False):
        dw = torch.full((cout * cin * k * k + GUARD,), float("nan"), device=gpu)
        dg, db = torch.full((cout + GUARD,), float("nan"), device=gpu), torch.full((cout + GUARD,), float("nan"), device=gpu)
        E.resnet_fold_bwd(d["dwp"], d["db"], d["w"], d["gamma"], d["mean"], d["var"], eps, dw, dg if want_bn else None,
                          db if want_bn else None, k, cin, cout)
        dwc, dgc, dbc = dw.cpu(), dg.cpu(), db.cpu()
        assert bool(dwc[cout * cin * k * k:].isnan().all()) and bool(dgc[cout:].isnan().all()) and bool(dbc[cout:].isnan().all())
        _check(f"fold_bwd {(k, cin, cout, eps)} dw", dwc[:cout * cin * k * k].reshape(cout, cin, k, k), dw64, dw32, 0.0)
        if want_bn:
            _check(f"fold_bwd {(k, cin, cout, eps)} dgamma", dgc[:cout], dg64, dg32, 0.0)
            assert torch.equal(dbc[:cout], p["db"])
        else:
            assert bool(dgc.isnan().all()) and bool(dbc.isnan().all())


@pytest.mark.parametrize("k,cin,cout", [(1, 64, 256), (3, 128, 64), (3, 512, 512), (1, 2048, 512)])
def test_pack_bwd_is_the_permutation(gpu, k, cin, cout):
    g = torch.Generator().manual_seed(k + cin + cout)
    wb = torch.randint(-32768, 32767, (cout, cin, k, k), generator=g, dtype=torch.int16)               # every value its own bits
    wp = pack_b32(wb.permute(0, 2, 3, 1).reshape(cout, -1)).contiguous().to(gpu)
    out = torch.full((cin * k * k * cout + GUARD,), 0x7FFF, dtype=torch.int16, device=gpu)
    E.conv_cl_pack_bwd(wp, out, k, cin, cout)
    o = out.cpu()
    assert bool((o[cin * k * k * cout:] == 0x7FFF).all())
    assert torch.equal(o[:cin * k * k * cout], _wt_host(wb, k, cin, cout).reshape(-1))


def test_resnet_pack_bwd_against_the_forward_pack(gpu):
    m = _module(gpu)
    cfg = E.native_resnet_cfg(1, 40, 72, 50, "bf16")
    pack = E.native_resnet_pack(m, cfg, gpu)
    wt = E.native_resnet_pack_bwd(pack)
    index = E.resnet_conv_index(m.block_table())
    want = {c for (si, j, name), c in index.items() if si >= 1 and not (si == 1 and j == 0 and name in ("conv1", "downsample"))}
    assert set(wt) == want and len(want) == 3 * 13 + 3 - 2
    lay = _lib.ResNetLayout()
    import ctypes
    _lib.check(_lib.load().ph_resnet_pack_bwd_layout(ctypes.byref(cfg), ctypes.byref(lay)), "ph_resnet_pack_bwd_layout")
    assert all(lay.bytes[2 * c + 1] == 0 for c in range(lay.nconvs)) and all(lay.offset[2 * c] % 256 == 0 for c in want)
    table = {(si, j): t for si, st in enumerate(m.block_table()) for j, t in enumerate(st)}
    for (si, j, name), c in index.items():
        if c not in want:
            continue
        cin_b, planes, s, _ = table[(si, j)]
        k, cin, cout = {"conv1": (1, cin_b, planes), "conv2": (3, planes, planes), "conv3": (1, planes, 4 * planes),
                        "downsample": (1, cin_b, 4 * planes)}[name]
        fwd = pack.pk["blocks"][si][j][name][0].cpu()                                      # fragments of W'[cout][taps * cin]
        rows = fwd.reshape(cout // 32, k * k * cin // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(cout, k * k, cin)      # pack_b32 undone
        wb = rows.permute(0, 2, 1).reshape(cout, cin, k, k)
        assert torch.equal(wt[c].cpu(), _wt_host(wb, k, cin, cout).reshape(-1)), (si, j, name)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("C_", [256, 2048])
@pytest.mark.parametrize("HW", [6, 45, 4100])
def test_nchw_grad_to_cl_is_exact(gpu, with_add, C_, HW):
    B = 2
    g = torch.Generator().manual_seed(HW + C_)
    grad = torch.randn(B, C_, HW, generator=g) * 3
    add = (torch.randn(B, HW, C_, generator=g) * 3).bfloat16()
    mask = (torch.randn(B, HW, C_, generator=g) + 0.52).bfloat16()
    mask.view(-1)[::7] = 0.0
    mask.view(-1)[3::11] = -0.0
    ref = ((add.float() if with_add else 0) + grad.permute(0, 2, 1)).bfloat16()
    ref = torch.where(mask.float() > 0, ref, torch.zeros_like(ref))
    out = torch.full((B * HW * C_ + GUARD,), 0x7FFF, dtype=torch.int16, device=gpu)
    E.nchw_grad_to_cl(grad.to(gpu), add.view(torch.int16).to(gpu) if with_add else None, mask.view(torch.int16).to(gpu), out, B, HW, C_)
    o = out.cpu()
    assert bool((o[B * HW * C_:] == 0x7FFF).all()), "the launch wrote behind the plane"
    assert torch.equal(o[:B * HW * C_].reshape(B, HW, C_), ref.view(torch.int16))
    out2 = torch.full((B * HW * C_,), 0x7FFF, dtype=torch.int16, device=gpu)             # no mask: the rounded sum alone
    E.nchw_grad_to_cl(grad.to(gpu), add.view(torch.int16).to(gpu) if with_add else None, None, out2, B, HW, C_)
    assert torch.equal(out2.cpu().reshape(B, HW, C_), ((add.float() if with_add else 0) + grad.permute(0, 2, 1)).bfloat16().view(torch.int16))


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _module(gpu, **cfg_changes):
    with open(os.path.join(Hh.GOLDEN, "resnet_cfg.json")) as f:
        cfg = json.load(f)
    cfg.update(cfg_changes)
    m = registry.build_backbone(cfg)
    m.load_state_dict(resnet_cases.fill(m.state_dict()))
    return m.to(gpu).train()


_CPU_REF = {}


def _cpu_reference(shape, frames=None):
    """float64 CPU autograd of `_forward_torch` with the golden's upstream gradients at `shape`: ({name: gradient}, stages), computed
    once per (shape, frames); frames: the batch entries that take part (None: all)"""
    key = (shape, frames)
    if key not in _CPU_REF:
        _CPU_REF[key] = TC.torch_reference(shape, frames)
    return _CPU_REF[key]


def _device_grads(m, x, ups):
    m.zero_grad(set_to_none=True)
    with torch.enable_grad():
        outs = m(x)
        torch.autograd.backward([outs[i] for i in ups], [ups[i] for i in ups])
    return outs, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _compare(tag, grads, ref, golden):
    """the issue's two assertions: per tensor rel_err <= 2 emu_gerr_bf16 and needed_atol(rtol 2^-8) <= 2 emu_gneed_bf16.  At the golden's
    weights the emulated error is 0.44 (a ReLU mask that the bf16 forward flips moves a gradient by tens of per cent), so this bound
    is 0.87: a zero gradient misses it, a gradient of half the batch would not.  Every test that calls this therefore also calls
    `_narrow`, whose bound is about 2e-2"""
    b_err, b_need = 2 * float(golden["emu_gerr_bf16"]), 2 * float(golden["emu_gneed_bf16"])
    worst = [0.0, 0.0]
    for n, r in ref.items():
        e, need = Hh.rel_err(grads[n].cpu(), r), Hh.needed_atol(grads[n].cpu(), r, rtol=U16)
        worst = [max(worst[0], e), max(worst[1], need)]
        assert e <= b_err, (tag, n, e, b_err)
        assert need <= b_need, (tag, n, need, b_need)
    print(tag, "max rel_err", worst[0], "bound", b_err, "max needed atol", worst[1], "bound", b_need)


def _narrow(tag, m, x, ups, grads, golden, case, per_frame=False):
    """The narrow check: the float64 chain rule WITHOUT any rounding, run on the CPU through the activation planes the device itself
    kept (so every ReLU mask is the device's), against the device's gradients.  What is left is the rounding of the gradient planes
    and the fp32 sums; the golden tool measured that on its own emulated activations at the same shape (emu_perr_bf16<case>,
    emu_pneed_bf16<case>, asserted there to stay below 5e-2), and the margin is the issue's factor 2.  per_frame: the reference is
    the float64 SUM of the chain rule run on each frame's planes and upstream gradients alone -- the batch sum, tightly."""
    plan, _, _, _ = T._resnet_train_state(m, x)
    B = x.shape[0]
    sd = {k_: v.detach().cpu() for k_, v in m.state_dict().items()}
    nchw = lambda plane, c, h, w: plane.cpu()[:B * c * h * w].view(torch.bfloat16).double().reshape(B, h, w, c).permute(0, 3, 1, 2)
    blocks = []
    for si, stage in enumerate(m.block_table()):
        for j, (cin, planes, s, has_down) in enumerate(stage):
            if si < plan.first_trained:
                continue
            (h, w, ho, wo), kp, p = plan.geo[(si, j)], plan.kept[(si, j)], f"layer{si + 1}.{j}."
            blk = dict(p=p, stride=s, stage=si, first=j == 0, x=nchw(plan.inputs[(si, j)], cin, h, w), a1=nchw(kp["a1"], planes, h, w),
                       a2=nchw(kp["a2"], planes, ho, wo), y=nchw(kp["y"], 4 * planes, ho, wo))
            for name, conv, bn in (("c1", "conv1", "bn1"), ("c2", "conv2", "bn2"), ("c3", "conv3", "bn3")) + \
                    ((("sc", "downsample.0", "downsample.1"),) if has_down else ()):
                blk[name] = TC.fold(sd, p + conv, p + bn, 1e-5, TC.bf16)
            blocks.append(blk)
    ups = {i: u.cpu() for i, u in ups.items()}
    if per_frame:
        ref = None
        for f in range(B):
            one = [{k_: (v[f:f + 1] if k_ in ("x", "a1", "a2", "y") else v) for k_, v in blk.items()} for blk in blocks]
            r = TC.backward_blocks(sd, one, {i: u[f:f + 1] for i, u in ups.items()}, TC.exact, plan.first_trained)
            ref = r if ref is None else {n: ref[n] + r[n] for n in r}
    else:
        ref = TC.backward_blocks(sd, blocks, ups, TC.exact, plan.first_trained)
    assert set(ref) == set(grads) and len(ref) == 126
    b_err, b_need = 2 * float(golden["emu_perr_bf16" + case]), 2 * float(golden["emu_pneed_bf16" + case])
    assert b_err < 0.1 and b_need < 0.1                                      # a bound that a wrong gradient cannot meet
    worst = [0.0, 0.0]
    for n, r in ref.items():
        assert float(r.abs().max()) > 0, n
        e, need = Hh.rel_err(grads[n].cpu(), r), Hh.needed_atol(grads[n].cpu(), r, rtol=U16)
        worst = [max(worst[0], e), max(worst[1], need)]
        assert e <= b_err and need <= b_need, (tag, n, e, b_err, need, b_need)
    print(tag, "on the device's activations: max rel_err", worst[0], "bound", b_err, "max needed atol", worst[1], "bound", b_need)


def test_module_gradients_against_float64_autograd(gpu):
    """Measured on an MI355X: see the figures beside the emulated ones in DESIGN.md 7f9."""
    golden = Hh.load_golden("resnet_train.npz")
    m = _module(gpu).train_on_device()
    x = resnet_cases.inputs(1)[0].to(gpu)
    ups = {i: u.to(gpu) for i, u in TC.upstream(resnet_cases.SHAPE).items()}
    outs, grads = _device_grads(m, x, ups)
    with torch.no_grad():
        m.eval()
        plain = m(x)
        m.train()
    assert len(outs) == 4 and all(torch.equal(a, b) for a, b in zip(outs, plain))
    ref, _ = _cpu_reference(resnet_cases.SHAPE)
    assert len(ref) == 126 and set(grads) == set(ref)
    _compare("resnet train 1x3x40x72", grads, ref, golden)
    outs, grads = _device_grads(m, x, ups)                                  # the plan's planes are this run's
    _narrow("resnet train 1x3x40x72", m, x, ups, grads, golden, "")


def test_batch_sum_and_run_to_run_bits(gpu):
    golden = Hh.load_golden("resnet_train.npz")
    shape = (2, 3, 64, 96)
    m = _module(gpu).train_on_device()
    x = resnet_cases.inputs(1, shape)[0].to(gpu)
    ups = {i: u.to(gpu) for i, u in TC.upstream(shape).items()}
    _, g1 = _device_grads(m, x, ups)
    _, g2 = _device_grads(m, x, ups)
    assert set(g1) == set(g2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    ra, _ = _cpu_reference(shape, (0,))
    rb, _ = _cpu_reference(shape, (1,))
    _compare("resnet train batch of 2 against the sum of the frames", g1, {n: ra[n] + rb[n] for n in ra}, golden)
    _narrow("resnet train 2x3x64x96, whole batch", m, x, ups, g2, golden, "_b2")
    _narrow("resnet train 2x3x64x96, sum of the frames", m, x, ups, g2, golden, "_b2", per_frame=True)


def test_a_missing_stage_gradient_is_zeros(gpu):
    m = _module(gpu).train_on_device()
    x = resnet_cases.inputs(1)[0].to(gpu)
    ups = {i: u.to(gpu) for i, u in TC.upstream(resnet_cases.SHAPE).items()}
    del ups[3]
    _, grads = _device_grads(m, x, ups)
    for n, g in grads.items():
        if n.startswith("layer4."):
            assert not bool(g.any()), n
        else:
            assert bool(g.any()), n
    assert any(n.startswith("layer2.") for n in grads) and any(n.startswith("layer3.") for n in grads)


def test_frozen_norms_return_no_norm_gradients(gpu):
    x = resnet_cases.inputs(1)[0].to(gpu)
    ups = {i: u.to(gpu) for i, u in TC.upstream(resnet_cases.SHAPE).items()}
    _, full = _device_grads(_module(gpu).train_on_device(), x, ups)
    _, conv_only = _device_grads(_module(gpu, norm_cfg=dict(type="BN", requires_grad=False)).train_on_device(), x, ups)
    assert len(conv_only) == 42 and all(n.endswith("conv1.weight") or n.endswith("conv2.weight") or n.endswith("conv3.weight")
                                        or n.endswith("downsample.0.weight") for n in conv_only)
    for n, g in conv_only.items():
        assert torch.equal(g, full[n]), n


@torch.enable_grad()
def test_refusals(gpu):
    x = resnet_cases.inputs(1)[0].to(gpu)
    for changes, arg in ((dict(frozen_stages=0), "frozen_stages"), (dict(frozen_stages=-1), "frozen_stages"), (dict(norm_eval=False), "norm_eval")):
        with pytest.raises(NotImplementedError, match=arg):
            _module(gpu, **changes).train_on_device()(x)
    with pytest.raises(NotImplementedError, match="precision"):
        _module(gpu).set_precision("fp16").train_on_device()(x)
    with pytest.raises(NotImplementedError, match="img"):
        _module(gpu).train_on_device()(x.clone().requires_grad_(True))


def test_plan_allocates_nothing_after_construction(gpu):
    m = _module(gpu).train_on_device()
    x = resnet_cases.inputs(1, (2, 3, 40, 72))[0].to(gpu)
    ups = {i: u.to(gpu) for i, u in TC.upstream((2, 3, 40, 72)).items()}
    _device_grads(m, x, ups)                                              # builds the packs and the plan
    plan, pk, wt, xin = T._resnet_train_state(m, x)
    assert plan.nbytes == sum(t.numel() * t.element_size() for t in plan._tensors) > 0
    f32 = lambda t: t.detach()
    params = {key: (f32(c.weight), f32(bn.weight), f32(bn.running_mean), f32(bn.running_var), bn.eps, True) for key, c, bn in T._resnet_trained(m)}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    plan.forward(xin, pk)
    plan.backward(ups, wt, params)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before, "forward() / backward() allocated"


def test_repack_after_an_in_place_update(gpu):
    m = _module(gpu).train_on_device()
    x = resnet_cases.inputs(1)[0].to(gpu)
    with torch.enable_grad():
        first = [o.detach().clone() for o in m(x)]
        assert "_ResNetStages" in type(m(x)[1].grad_fn).__name__                  # the device training path, not the inference plan
    with torch.no_grad():
        m.layer3[1].conv2.weight.mul_(1.5)
    with torch.enable_grad():
        second = [o.detach().clone() for o in m(x)]
    want = _module(gpu)
    with torch.no_grad():
        want.layer3[1].conv2.weight.mul_(1.5)
        want.eval()
        ref = want(x)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    for i in (2, 3):
        assert not torch.equal(first[i], second[i]) and torch.equal(second[i], ref[i])
