"""GPU: the optimizer step (csrc/ph_optim.hip, polyphonicformer_amd/optim.py) against torch itself.

Yardstick: `clip_grad_norm_(foreach=False)` + `torch.optim.AdamW(foreach=False)` on CPU copies in fp64.  The bounds for p, m, v are
measured from the reference, never from the code under test: the same torch pair on CPU in fp32 gives, per tensor,
e_ref = max |torch fp32 - torch fp64|, and the device result must lie within 4 e_ref + ulp32(max |value|) of the fp64 result (about
eight rounded fp32 operations per element, each moved by at most one rounding by another association; the added ulp because e_ref can
be exactly 0 on a 1-element tensor).  grad_norm and clip_coef are fp64 results rounded once to fp32 behind a few fp64 operations on
fp64 sums: 2^-22 relative.  Fixtures: parameters 0.05 N(0, 1), lr 1e-2 and 2e-2, so every element moves by a multiple of 1e-3 over the
three steps -- some 1e5 bounds: a wrong bias correction, a coupled weight decay or swapped betas cannot pass."""
import copy
import ctypes as C
import math

import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib
from polyphonicformer_amd import optim as O

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.999), 1e-8
LR_FACTORS = (1.0, 0.5, 0.75)
# element counts; "view": a view at storage offset 1 (the scalar path); "none": `.grad` stays None.  The last tensor ends in a
# float4 and a scalar tail behind two full items.
SPECS = [1, 3, 255, 4095, 4096, 0, 4097, "none", "view", (64, 33), 8197]
NONE, VIEW, LAST = SPECS.index("none"), SPECS.index("view"), len(SPECS) - 1
GROUP_OF = [0] * 6 + [1] * 5
GROUP_KW = [dict(lr=1e-2, weight_decay=0.05), dict(lr=2e-2, weight_decay=0.01)]


def _shape(spec):
    return (100,) if spec == "none" else (517,) if spec == "view" else (spec,) if isinstance(spec, int) else spec


def cpu_case(seed, steps=3, grad_scale=1.0):
    """(parameters, [per step the gradients]) on the CPU in fp32; entry NONE of every gradient list is None.  An element's gradient
    differs from step to step but keeps its sign and stays away from 0, sign (0.25 + |N(0, 1)|): its normalised update is then of order
    1 in every step and the steps add up, so EVERY element moves by about lr -- no element sits still by cancellation."""
    gen = torch.Generator().manual_seed(seed)
    ps = [0.05 * torch.randn(_shape(s), generator=gen) for s in SPECS]
    sign = [torch.where(torch.randn(_shape(s), generator=gen) < 0, -1.0, 1.0) for s in SPECS]
    gs = [[None if i == NONE else grad_scale * sg * (0.25 + torch.randn(_shape(s), generator=gen).abs()) for i, (s, sg) in enumerate(zip(SPECS, sign))]
          for _ in range(steps)]
    return ps, gs


def _groups(ps):
    return [dict(params=[p for p, g in zip(ps, GROUP_OF) if g == k], **GROUP_KW[k]) for k in range(2)]


def torch_run(ps, gs, dtype, max_norm, device="cpu", steps=None, opt=None):
    """the yardstick: clip_grad_norm_ + AdamW.step per step on copies of `ps` in `dtype` -> (params, optimizer, [norm per step])"""
    ps = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in ps] if opt is None else ps
    opt = opt or torch.optim.AdamW(_groups(ps), betas=BETAS, eps=EPS, foreach=False)
    norms = []
    for k in (range(len(gs)) if steps is None else steps):
        for p, g in zip(ps, gs[k]):
            p.grad = None if g is None else g.to(device=device, dtype=dtype).clone()
        for grp, kw in zip(opt.param_groups, GROUP_KW):
            grp["lr"] = kw["lr"] * LR_FACTORS[k]
        with_grad = [p for p in ps if p.grad is not None]
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(with_grad, max_norm, foreach=False).detach().cpu())
        else:
            norms.append(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in with_grad)).cpu())
        opt.step()
        for grp, kw in zip(opt.param_groups, GROUP_KW):                      # the groups keep their base rate, as an exported state must
            grp["lr"] = kw["lr"]
    return ps, opt, norms


def torch_state(ps, opt):
    """(p, m, v) lists of a torch optimizer on the CPU; zeros where torch keeps no state (the tensor never had a gradient)"""
    m = [opt.state[p]["exp_avg"] if p in opt.state else torch.zeros_like(p) for p in ps]
    v = [opt.state[p]["exp_avg_sq"] if p in opt.state else torch.zeros_like(p) for p in ps]
    return [[t.detach().cpu() for t in x] for x in (ps, m, v)]


def ulp32(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 2.0 ** -149


MAX_NORMS = {"clip_active": 1.0, "clip_inactive": 1e4}


@pytest.fixture(scope="module")
def reference():
    """computed once, shared, never modified: per clip case the fp64 yardstick after three steps, e_ref per tensor and quantity,
    and the fp64 norms of the three steps"""
    ps, gs = cpu_case(1234)
    out = {}
    for name, mn in MAX_NORMS.items():
        p64, o64, n64 = torch_run(ps, gs, torch.float64, mn)
        p32, o32, _ = torch_run(ps, gs, torch.float32, mn)
        s64, s32 = torch_state(p64, o64), torch_state(p32, o32)
        e_ref = [[float((a.double() - b).abs().max()) if a.numel() else 0.0 for a, b in zip(x32, x64)] for x32, x64 in zip(s32, s64)]
        out[name] = dict(state=s64, e_ref=e_ref, norms=[float(n) for n in n64])
    # the premise of the comparison: the clip does what its name says in either case
    assert min(out["clip_active"]["norms"]) > 100.0 and max(out["clip_inactive"]["norms"]) < 1e3
    return out


def device_params(ps, gpu):
    """the fixture's tensors on the GPU as leaves; VIEW sits one float into its storage"""
    out = []
    for i, p in enumerate(ps):
        if i == VIEW:
            base = torch.zeros(p.numel() + 1, device=gpu)
            t = base[1:].view(p.shape)
            t.copy_(p)
            assert t.data_ptr() % 16 == 4
        else:
            t = p.to(gpu).clone()
        out.append(t.requires_grad_())
    return out


def set_grads(ps, grads, gpu):
    """fresh gradient tensors; the first tensor of 4097 elements gets a gradient one float into ITS storage (p aligned, g not)"""
    for i, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
        elif SPECS[i] == 4097:
            base = torch.zeros(g.numel() + 1, device=gpu)
            base[1:].copy_(g)
            p.grad = base[1:].view(p.shape)
        else:
            p.grad = g.to(gpu).clone()


def make_opt(ps, max_norm, **kw):
    return O.AdamWStep(_groups(ps), betas=BETAS, eps=EPS, max_norm=max_norm, **kw)


def ordered(opt, ps):
    """the optimizer's per-parameter lists in the order of `ps` (the optimizer keeps group order)"""
    idx = {id(p): k for k, p in enumerate(opt.params)}
    return [opt.exp_avg[idx[id(p)]] for p in ps], [opt.exp_avg_sq[idx[id(p)]] for p in ps]


def run_ours(ps, gs, gpu, max_norm, steps=None, opt=None, dps=None, **kw):
    dps = dps if dps is not None else device_params(ps, gpu)
    opt = opt or make_opt(dps, max_norm, **kw)
    infos = []
    for k in (range(len(gs)) if steps is None else steps):
        set_grads(dps, gs[k], gpu)
        opt.step(lr_factor=LR_FACTORS[k])
        infos.append(opt.info())
    return dps, opt, infos


def snapshot(dps, opt):
    m, v = ordered(opt, dps)
    return [[t.detach().clone() for t in x] for x in (dps, m, v)] + [opt._state.clone()]


def same(a, b):
    return all(torch.equal(x, y) for la, lb in zip(a[:3], b[:3]) for x, y in zip(la, lb)) and torch.equal(a[3], b[3])


def check_bounds(state, ref, what, ratios=None):
    for q, name in enumerate("pmv"):
        for i, (got, want) in enumerate(zip(state[q], ref["state"][q])):
            if not want.numel():
                continue
            err = float((got.detach().cpu().double() - want).abs().max())
            bound = 4 * ref["e_ref"][q][i] + ulp32(float(want.abs().max()))
            if ratios is not None and ref["e_ref"][q][i] > 0:
                ratios.setdefault(name, []).append(err / ref["e_ref"][q][i])
            assert err <= bound, f"{what}: {name} of tensor {i} ({SPECS[i]}): error {err:.3e}, bound {bound:.3e}, e_ref {ref['e_ref'][q][i]:.3e}"


# ---- 1. three steps against torch fp64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MAX_NORMS))
def test_three_steps_against_torch_fp64(gpu, reference, case):
    ps, gs = cpu_case(1234)
    ref = reference[case]
    dps, opt, infos = run_ours(ps, gs, gpu, MAX_NORMS[case])
    m, v = ordered(opt, dps)
    ratios = {}
    check_bounds((dps, m, v), ref, case, ratios)
    print({k: (max(r), sum(r) / len(r)) for k, r in ratios.items()})          # device error / e_ref: max, mean
    assert [i["step"] for i in infos] == [1, 2, 3] and all(i["skipped"] == 0 and i["status"] == _lib.PH_OPTIM_OK for i in infos)
    for i, n64 in zip(infos, ref["norms"]):
        assert abs(i["grad_norm"] - n64) <= 2.0 ** -22 * n64, (i["grad_norm"], n64)
        c64 = min(1.0, MAX_NORMS[case] / (n64 + 1e-6))
        assert abs(i["clip_coef"] - c64) <= 2.0 ** -22 * c64, (i["clip_coef"], c64)
    assert float(opt.grad_norm) == infos[-1]["grad_norm"] and float(opt.clip_coef) == infos[-1]["clip_coef"]       # the device views
    # the tensor without a gradient keeps its bits; its moments stay zero
    assert torch.equal(dps[NONE].detach().cpu(), ps[NONE]) and not m[NONE].any() and not v[NONE].any()
    # every element moved by at least 1000 x its bound: the comparison above is sharp for the update
    for i, (a, b) in enumerate(zip(ref["state"][0], ps)):
        if i != NONE and b.numel():
            bound = 4 * ref["e_ref"][0][i] + ulp32(float(a.abs().max()))
            assert float((a - b.double()).abs().min()) > 1000 * bound, (i, float((a - b.double()).abs().min()), bound)
    if case == "clip_inactive":                                              # the coefficient is exactly 1: as without a clip
        assert all(i["clip_coef"] == 1.0 for i in infos)
        d2, o2, i2 = run_ours(ps, gs, gpu, None, skip_nonfinite=False)
        m2, v2 = ordered(o2, d2)
        assert all(torch.equal(x, y) for la, lb in ((dps, d2), (m, m2), (v, v2)) for x, y in zip(la, lb))
        assert all(i["grad_norm"] == -1.0 and i["clip_coef"] == 1.0 for i in i2)           # no norm was asked for


# ---- 2. the gradients are left alone ----------------------------------------------------------------------------------------------------
def test_gradients_untouched_or_zeroed_in_place(gpu):
    ps, gs = cpu_case(77, steps=1)
    dps = device_params(ps, gpu)
    opt = make_opt(dps, 1.0)
    set_grads(dps, gs[0], gpu)
    before = [None if p.grad is None else p.grad.clone() for p in dps]
    opt.step()
    assert opt.info()["clip_coef"] < 0.1                                     # the clip was active, on the fly
    for p, b in zip(dps, before):
        assert (p.grad is None) == (b is None) and (b is None or torch.equal(p.grad, b))
    addr = [None if p.grad is None else p.grad.data_ptr() for p in dps]
    opt.step(zero_grad=True)
    for p, a in zip(dps, addr):
        assert (p.grad is None) == (a is None) and (a is None or (p.grad.data_ptr() == a and not p.grad.any()))
    assert opt.info()["step"] == 2
    set_grads(dps, gs[0], gpu)
    addr = [None if p.grad is None else p.grad.data_ptr() for p in dps]
    snap = snapshot(dps, opt)
    opt.zero_grad()                                                          # the one-launch call: gradients only
    for p, a in zip(dps, addr):
        assert a is None or (p.grad.data_ptr() == a and not p.grad.any())
    assert same(snap, snapshot(dps, opt))


def test_group_values_written_between_steps_are_noticed(gpu):
    """mmcv's LR hook writes `group['lr']` directly: the next step re-uploads the table.  Halving every group's rate is the same
    product in fp64 as lr_factor = 0.5, so the two routes give the same bits; a changed weight_decay moves the result."""
    ps, gs = cpu_case(41, steps=2)
    runs = []
    for route in ("factor", "group", "decay"):
        dps = device_params(ps, gpu)
        opt = make_opt(dps, 1.0)
        set_grads(dps, gs[0], gpu)
        opt.step()
        set_grads(dps, gs[1], gpu)
        if route == "factor":
            opt.step(lr_factor=0.5)
        else:
            for g in opt.param_groups:
                g["lr"] *= 0.5
                g["weight_decay"] *= 1.0 if route == "group" else 2.0
            opt.step()
        runs.append(snapshot(dps, opt))
    assert same(runs[0], runs[1])
    assert not any(torch.equal(a, b) for i, (a, b) in enumerate(zip(runs[0][0], runs[2][0])) if i != NONE and a.numel())


# ---- 3. determinism, grid independence ---------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_grid(gpu):
    ps, gs = cpu_case(99, steps=2)
    runs = []
    for max_blocks in (0, 1, 3, 0):
        dps = device_params(ps, gpu)
        opt = make_opt(dps, 1.0)
        opt.max_blocks = max_blocks
        run_ours(ps, gs, gpu, 1.0, opt=opt, dps=dps)
        runs.append(snapshot(dps, opt))
    for r in runs[1:]:
        assert same(runs[0], r)


# ---- 4. non-finite gradients --------------------------------------------------------------------------------------------------------------
def _poison(gs, which):
    gs = [[None if g is None else g.clone() for g in step] for step in gs]
    if which == "nan_last":
        gs[0][LAST].view(-1)[-1] = float("nan")
    else:
        gs[0][0].view(-1)[0] = float("inf")
    return gs


@pytest.mark.parametrize("which", ["nan_last", "inf_first"])
def test_nonfinite_step_is_skipped(gpu, which):
    ps, gs = cpu_case(55, steps=2)
    bad = _poison(gs, which)
    dps = device_params(ps, gpu)
    opt = make_opt(dps, 1.0)
    run_ours(ps, gs, gpu, 1.0, steps=[1], opt=opt, dps=dps)                  # one clean step first: moments and counter are not zero
    snap = snapshot(dps, opt)
    set_grads(dps, bad[0], gpu)
    opt.step(zero_grad=True)
    info = opt.info()
    assert (info["step"], info["skipped"], info["status"]) == (1, 1, _lib.PH_OPTIM_ENONFINITE) and not math.isfinite(info["grad_norm"])
    now = snapshot(dps, opt)
    assert all(torch.equal(x, y) for la, lb in zip(snap[:3], now[:3]) for x, y in zip(la, lb))
    assert all(p.grad is None or not p.grad.any() for p in dps)              # the NaN does not stay to be accumulated
    # a fresh optimizer: the skipped call first, then a clean one == step 1 of an optimizer that never saw it, bit for bit
    d1 = device_params(ps, gpu)
    o1 = make_opt(d1, 1.0)
    set_grads(d1, bad[0], gpu)
    o1.step()
    assert torch.equal(d1[3].detach().cpu(), ps[3])
    run_ours(ps, gs, gpu, 1.0, steps=[0], opt=o1, dps=d1)
    d2, o2, _ = run_ours(ps, gs, gpu, 1.0, steps=[0])
    a, b = snapshot(d1, o1), snapshot(d2, o2)
    assert all(torch.equal(x, y) for la, lb in zip(a[:3], b[:3]) for x, y in zip(la, lb))
    i1, i2 = o1.info(), o2.info()
    assert (i1["step"], i1["skipped"], i1["status"]) == (1, 1, 0) and (i2["step"], i2["skipped"]) == (1, 0)
    assert (i1["grad_norm"], i1["clip_coef"]) == (i2["grad_norm"], i2["clip_coef"])


def test_nonfinite_without_the_skip_is_torchs(gpu):
    """skip_nonfinite=False: a NaN norm makes the coefficient NaN and with it every parameter that has a gradient, as torch's pair does"""
    ps, gs = cpu_case(55, steps=1)
    bad = _poison(gs, "nan_last")
    tp, _, _ = torch_run(ps, bad, torch.float32, 1.0)
    dps, opt, infos = run_ours(ps, bad, gpu, 1.0, skip_nonfinite=False)
    assert (infos[0]["step"], infos[0]["skipped"], infos[0]["status"]) == (1, 0, _lib.PH_OPTIM_ENONFINITE)
    for i, (d, t) in enumerate(zip(dps, tp)):
        assert torch.equal(torch.isnan(d.detach().cpu()), torch.isnan(t.detach())), i
        assert i == NONE or bool(torch.isnan(d).all())
    assert torch.equal(dps[NONE].detach().cpu(), ps[NONE])


def test_huge_finite_gradient_does_not_overflow_the_norm(gpu):
    """one element of 1e30: its square overflows fp32, the fp64 sum does not -- no skip, the norm to 2^-22, everything finite"""
    ps, gs = cpu_case(56, steps=1)
    gs[0][4].view(-1)[17] = 1e30
    assert not math.isfinite(float((gs[0][4] * gs[0][4]).sum()))             # the premise: fp32 squares overflow
    n64 = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs[0] if g is not None))
    dps, opt, infos = run_ours(ps, gs, gpu, 1.0)
    assert (infos[0]["step"], infos[0]["skipped"], infos[0]["status"]) == (1, 0, _lib.PH_OPTIM_OK)
    assert abs(infos[0]["grad_norm"] - n64) <= 2.0 ** -22 * n64
    m, v = ordered(opt, dps)
    assert all(bool(torch.isfinite(t).all()) for x in (dps, m, v) for t in x)


# ---- 5. device lr_factor, graph -------------------------------------------------------------------------------------------------------------
def test_captured_step_follows_a_device_lr_factor(gpu):
    """one eager step (it uploads the table), one captured, two replays with the factor and the gradients rewritten in place: the
    same bits as three eager steps.  The chain is linear: three kernels on one stream."""
    ps, gs = cpu_case(31)
    want_d, want_o, _ = run_ours(ps, gs, gpu, 1.0)
    want = snapshot(want_d, want_o)
    dps = device_params(ps, gpu)
    opt = make_opt(dps, 1.0)
    factor = torch.tensor([LR_FACTORS[0]], dtype=torch.float32, device=gpu)
    set_grads(dps, gs[0], gpu)
    opt.step(lr_factor=factor)
    versions = [p._version for p in dps]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(lr_factor=factor, zero_grad=False)
    for k in (1, 2):
        factor.fill_(LR_FACTORS[k])
        with torch.no_grad():
            for p, g in zip(dps, gs[k]):
                if g is not None:
                    p.grad.copy_(g.to(gpu).view(p.shape))
        graph.replay()
    torch.cuda.synchronize()
    assert same(want, snapshot(dps, opt)) and opt.info()["step"] == 3
    opt.mark_updated()
    assert all(p._version > v0 for i, (p, v0) in enumerate(zip(dps, versions)) if i != NONE)


def test_at_most_three_launches(gpu, monkeypatch):
    """the captured calls' kernel nodes: sums of squares, finalize, update -- two without a norm to take, one for zero_grad(); the
    grid is min(items, max_blocks), the finalize one workgroup; and a table that changed during a capture is refused"""
    ps, gs = cpu_case(32, steps=1)
    items = O.plan_items([p.numel() for p in ps], [True] * len(ps))[0]
    dps = device_params(ps, gpu)
    set_grads(dps, gs[0], gpu)
    opt = make_opt(dps, 1.0)
    assert Hh.graph_kernel_nodes(lambda: opt.step()) == [[1, 1, 1, 256, 0]] + [[items, 1, 1, 256, 0]] * 2
    opt.max_blocks = 3
    assert Hh.graph_kernel_nodes(lambda: opt.step(zero_grad=True)) == [[1, 1, 1, 256, 0]] + [[3, 1, 1, 256, 0]] * 2
    assert Hh.graph_kernel_nodes(lambda: opt.zero_grad()) == [[3, 1, 1, 256, 0]]
    set_grads(dps, gs[0], gpu)
    plain = make_opt(dps, None, skip_nonfinite=False)
    assert Hh.graph_kernel_nodes(lambda: plain.step()) == [[1, 1, 1, 256, 0], [items, 1, 1, 256, 0]]
    set_grads(dps, gs[0], gpu)                                               # the gradients moved: the table is stale
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)      # what step() asks; no capture is begun here
    with pytest.raises(_lib.PolyheadError, match="capture"):
        plain.step()
    monkeypatch.undo()
    plain.step()                                                             # and eagerly it is simply uploaded again
    assert plain.info()["step"] == 2                                         # the captured call above was never replayed


# ---- 6. state exchange with torch on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
def test_state_exchange_with_torch_on_the_device(gpu, reference, direction):
    ps, gs = cpu_case(1234)
    ref, mn = reference["clip_active"], MAX_NORMS["clip_active"]
    if direction == "ours_to_torch":
        dps, opt, _ = run_ours(ps, gs, gpu, mn, steps=[0, 1])
        tps = [torch.nn.Parameter(p.detach().clone()) for p in dps]
        topt = torch.optim.AdamW(_groups(tps), betas=BETAS, eps=EPS, foreach=False)
        topt.load_state_dict(opt.state_dict())
        assert all(float(topt.state[p]["step"]) == 2.0 for p in tps)
        torch_run(tps, gs, torch.float32, mn, device=gpu, steps=[2], opt=topt)
        state = torch_state(tps, topt)
    else:
        tps, topt, _ = torch_run(ps, gs, torch.float32, mn, device=gpu, steps=[0, 1])
        dps = device_params([p.detach().cpu() for p in tps], gpu)
        opt = make_opt(dps, mn)
        opt.load_state_dict(topt.state_dict())
        assert opt.info()["step"] == 2
        run_ours(ps, gs, gpu, mn, steps=[2], opt=opt, dps=dps)
        assert opt.info()["step"] == 3
        state = (dps,) + ordered(opt, dps)
    check_bounds(state, ref, direction)


# ---- 7. argument errors launch nothing -------------------------------------------------------------------------------------------------------
def _raw_call(gpu, mutate):
    """ph_optim_step on a two-tensor table with one thing wrong -> (rc, message, everything the call could have written: unchanged?)"""
    lib = _lib.load()
    n = [8, 4100]
    bufs = {k: [torch.full((m,), 0.5 + j, device=gpu) for m in n] for j, k in enumerate("pgmv")}
    table = (_lib.OptimTensor * 2)()
    for i in range(2):
        table[i].p, table[i].g, table[i].m, table[i].v = (bufs[k][i].data_ptr() for k in "pgmv")
        table[i].n, table[i].lr, table[i].weight_decay, table[i].first_item = n[i], 1e-2, 0.05, i
    need = lib.ph_optim_workspace_bytes(table, 2)
    assert need == 256 * ((3 * 8 + 255) // 256)
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(gpu)
    ws = torch.full((need + 256,), 7, dtype=torch.uint8, device=gpu)
    state = torch.full((5,), 3, dtype=torch.int64, device=gpu)
    a = dict(cfg=_lib.OptimCfg(0.9, 0.999, 1e-8, 1.0, _lib.PH_OPTIM_SKIP_NONFINITE | _lib.PH_OPTIM_ZERO_GRADS, 0), table=table, nt=2,
             ws_ptr=ws.data_ptr(), ws_bytes=need)
    mutate(a)
    before = [t.clone() for k in "pgmv" for t in bufs[k]] + [ws.clone(), state.clone()]
    rc = lib.ph_optim_step(C.byref(a["cfg"]), a["table"], _lib.ptr(table_dev), a["nt"], 1.0, None, _lib.ptr(state), C.c_void_p(a["ws_ptr"]),
                           a["ws_bytes"], _lib.stream_ptr())
    msg = Hh.last_error()
    torch.cuda.synchronize()
    after = [t for k in "pgmv" for t in bufs[k]] + [ws, state]
    return rc, msg, all(torch.equal(x, y) for x, y in zip(before, after))


def _cfg(field, value):
    return lambda a: setattr(a["cfg"], field, value)


def _entry(index, field, value):
    return lambda a: setattr(a["table"][index], field, value)


def _arg(field, value=None, plus=0):
    return lambda a: a.__setitem__(field, (a[field] if value is None else value) + plus)


BAD_ARGS = {
    "zero_tensors": (_arg("nt", 0), _lib.PH_EINVAL, "ntensors"),
    "negative_n": (_entry(1, "n", -1), _lib.PH_EINVAL, "negative n"),
    "null_p": (_entry(0, "p", None), _lib.PH_EINVAL, "null p / m / v"),
    "null_m": (_entry(1, "m", None), _lib.PH_EINVAL, "null p / m / v"),
    "null_v": (_entry(0, "v", None), _lib.PH_EINVAL, "null p / m / v"),
    "beta1_is_1": (_cfg("beta1", 1.0), _lib.PH_EINVAL, "beta1"),
    "beta2_negative": (_cfg("beta2", -0.1), _lib.PH_EINVAL, "beta2"),
    "eps_zero": (_cfg("eps", 0.0), _lib.PH_EINVAL, "eps"),
    "workspace_small": (_arg("ws_bytes", plus=-1), _lib.PH_EWORKSPACE, "workspace too small"),
    "workspace_misaligned": (_arg("ws_ptr", plus=8), _lib.PH_EINVAL, "workspace must be 256-byte aligned"),
    "first_item_wrong": (_entry(1, "first_item", 2), _lib.PH_EINVAL, "first_item"),
}


@pytest.mark.parametrize("case", list(BAD_ARGS))
def test_argument_errors_launch_nothing(gpu, case):
    mutate, code, word = BAD_ARGS[case]
    rc, msg, unchanged = _raw_call(gpu, mutate)
    assert rc == code and "ph_optim_step" in msg and word in msg, (rc, msg)
    assert unchanged


def test_the_raw_call_itself_runs(gpu):
    """the premise of the cases above: without a mutation the same call succeeds and writes"""
    rc, msg, unchanged = _raw_call(gpu, lambda a: None)
    assert rc == 0 and not unchanged


# ---- 8. in the loop ----------------------------------------------------------------------------------------------------------------------------
NT, NS = 8, 11


def _build_heads(gpu):
    from polyphonicformer_amd.registry import HEADS
    import polyphonicformer_amd.kernel_update  # noqa: F401
    from test_gpu_loss import _rpn_head
    rpn, sd = _rpn_head(gpu)
    roi = HEADS.build(dict(type="KernelUpdateIterHead", num_stages=3, assign_stages=3, stage_loss_weights=[1] * 3, num_proposals=100,
                           num_thing_classes=NT, num_stuff_classes=NS, do_panoptic=True, merge_joint=True,
                           mask_head=Hh.stage_cfg(256, 2048, 8, NT + NS, NT, NS),
                           train_cfg=dict(assigner=copy.deepcopy(Hh.ROI_ASSIGNER), sampler=dict(type='MaskPseudoSampler'), pos_weight=1.)))
    roi.load_state_dict({k[len("roi_head."):]: v for k, v in sd.items() if k.startswith("roi_head.")})
    return rpn, roi.to(gpu)


def _eval_outputs(rpn, roi, feats, metas):
    """the heads in eval form, from their packed weights (what `VideoTrainStep` runs its reference frame through)"""
    mods = [m for top in (rpn, roi) for m in top.modules()]
    flags = [m.training for m in mods]
    try:
        rpn.eval()
        roi.eval()
        with torch.no_grad():
            (pf, xf, mp, cs, _, df, dp, dpr, _) = rpn.simple_test_rpn([f.clone() for f in feats], metas)
            out = roi.simple_test_mask_preds(xf, pf, mp, cs, metas, depth_preds=dpr, depth_feats=df, depth_proposal=dp, imgs_whwh=None)
    finally:
        for m, f in zip(mods, flags):
            m.training = f
    flat = []

    def walk(o):
        if isinstance(o, torch.Tensor):
            flat.append(o.clone())
        elif isinstance(o, (list, tuple)):
            for x in o:
                walk(x)
        elif isinstance(o, dict):
            for k in sorted(o):
                walk(o[k])

    walk(out)
    assert flat
    return flat


def test_in_the_training_loop(gpu):
    """TrainStep.forward_backward -> step.optimizer().step(): every parameter with a gradient changes, the heads' packed inference
    weights follow (their cache key is `_lib.param_versions`), a second iteration with zero_grad=True runs"""
    from polyphonicformer_amd import train as T
    rpn, roi = _build_heads(gpu)
    B, H, W = 2, 8, 16
    feats = [f.to(gpu) for f in Hh.neck_inputs(77, B, 256, H, W)]
    gts = [{k: v.to(gpu) for k, v in g.items()} for g in Hh.train_gt(78, B, 2 * H, 2 * W, NT, NS, [4, 6])]
    metas = [Hh.img_meta(H * 8, W * 8)] * B
    args = (feats, metas, [g["masks"] for g in gts], [g["labels"] for g in gts], [g["sem_seg"] for g in gts], [g["sem_cls"] for g in gts],
            torch.stack([g["depth"][None] for g in gts]))
    stale = _eval_outputs(rpn, roi, feats, metas)                            # the packs exist before the step
    with T.TrainStep(rpn, roi) as step:
        opt = step.optimizer(lr=2e-4, weight_decay=0.05, max_norm=1.0)
        params = step.parameters()
        step.forward_backward(*args)
        before = [p.detach().clone() for p in params]
        versions = _lib.param_versions(rpn), _lib.param_versions(roi)
        opt.step()
        with_grad = [p.grad is not None for p in params]
        assert sum(with_grad) > 100
        for p, b, g in zip(params, before, with_grad):
            assert torch.equal(p.detach(), b) != g
        assert _lib.param_versions(rpn) != versions[0] and _lib.param_versions(roi) != versions[1]
        info = opt.info()
        assert (info["step"], info["skipped"], info["status"]) == (1, 0, 0) and info["grad_norm"] > 0
        got = _eval_outputs(rpn, roi, feats, metas)
        rpn2, roi2 = _build_heads(gpu)
        rpn2.load_state_dict(rpn.state_dict())
        roi2.load_state_dict(roi.state_dict())
        want = _eval_outputs(rpn2, roi2, feats, metas)
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
        assert not all(torch.equal(a, b) for a, b in zip(got, stale))       # and the step did move the outputs
        step.forward_backward(*args)                                         # accumulates onto the first iteration's gradients
        opt.step(zero_grad=True)
        assert opt.info()["step"] == 2
        assert all(p.grad is None or not p.grad.any() for p in params)
