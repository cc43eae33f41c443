"""GPU: the FPN in training on the library's kernels (csrc/ph_fpntrain.hip, train.fpn_forward_train, fpn.FPN.train_on_device,
VideoTrainStep(fpn=...)), against float64 torch on the CPU.

  1. the wide map x map^T product (`train.map_x_mapT_wide`) against float64 einsum, rel_err < 2e-5 (test_gpu_train_tiles.py's bound
     for the same arithmetic), row sums within the same bound, a second call the same bits; K = 40 and 256 additionally bit for bit
     `ph_map_x_map_t_ex` at the same split count; K = 264 (a ragged 8-column tile), 320, 2048; M = 256 (two row passes) and 37;
     HW = 47 x 71 (scalar path, ragged), 4100, 1028 (>= 3 splits per image at every K: asserted); B = 2 summed over the batch.
  2. the nearest add and its backward, exact: forward `torch.equal` to fp32 `F.interpolate` + add, backward to the documented
     summation order restated in torch, overwrite and accumulate forms.
  3. bias add exact; channel sums within max(4 e_ref, 1e-6), e_ref = the float32 CPU sum's distance from the float64 one.
  4. `fpn_forward_train` against the reference class's outputs (tests/golden/fpn.npz, tools/gen_golden_fpn.py's seeds), rel_err < 3e-5.
  5. `fpn_forward_train` against float64 autograd of fpn.py:151-203 as tests/test_fpn_host.py states them: the 16 parameter
     gradients and the four stage gradients, rel_err < 1e-3, every float64 gradient non-zero.
  6. `FPN.train().train_on_device()`: forward is `fpn_forward_train` bit for bit; switched off, the torch branch runs.
  7. `VideoTrainStep(fpn=...)` on test_gpu_video_train.py's fixture: the losses of the step without `fpn` fed with the detached
     levels, the stage gradients `autograd.grad` of `fpn_forward_train` under that step's level gradients, both bit for bit.

Measured on an MI355X (worst over the cases of a family):
  wide product   rel_err 6.4e-6 (K = 40, M = 37, 47 x 71), 5.1e-6 elsewhere; row sums 1.5e-7 (bound 2e-5)
  channel sums   5.4e-8 at both sizes against e_ref 1.0e-7 (HW = 4099) and 7.1e-8 (HW = 33828): the floor 1e-6 is the bound
  forward        7.8e-6 (level 2; bound 3e-5, the fp32 inference grade measures 8.6e-6)
  gradients      parameters 8.1e-6 (lateral_convs.3.conv.weight), stages 7.0e-6 (bound 1e-3)
"""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
from test_gpu_video_train import video_parts  # noqa: F401  (the module fixture of the video step's parts)

pytestmark = pytest.mark.gpu

SIZES = ((13, 19), (7, 10), (4, 5), (2, 3))       # tools/gen_golden_fpn.py
B, WSEED, ISEED = 2, 5, 3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# =================================================================================================================================
# 1. the wide product
# =================================================================================================================================
HWS = {"47x71": (47, 71), "4100": (50, 82), "1028": (4, 257)}


@functools.lru_cache(maxsize=None)
def _wide_inputs(K, hw):
    h, w = HWS[hw]
    g = _gen(1000 + K + h * w)
    return torch.randn(B, 256, h, w, generator=g), torch.randn(B, K, h, w, generator=g)


@functools.lru_cache(maxsize=None)
def _wide_reference(K, hw, M):
    G, X = _wide_inputs(K, hw)
    G = G[:, :M].double().flatten(2)
    return torch.einsum("bmp,bkp->mk", G, X.double().flatten(2)), G.sum((0, 2))


@pytest.mark.parametrize("hw", list(HWS))
@pytest.mark.parametrize("M", [256, 37])
@pytest.mark.parametrize("K", [40, 256, 264, 320, 2048])
def test_wide_product_vs_float64(gpu, K, M, hw):
    from polyphonicformer_amd import _lib, train as TR
    lib = _lib.load()
    G, X = _wide_inputs(K, hw)
    G, X = G[:, :M].contiguous().to(gpu), X.to(gpu)
    HW = G[0, 0].numel()
    ns = lib.ph_map_x_map_t_wide_nsplit(B, M, K, HW)
    assert ns >= 3, (K, M, hw, ns)                     # every case sums several splits per image; "1028": 4 at most, 4 at K = 2048 too
    want, want_rs = _wide_reference(K, hw, M)
    rs = torch.full((M,), float("nan"), device=gpu)
    out = TR.map_x_mapT_wide(G, X, rowsum=rs, sum_batch=True)
    assert out.shape == (M, K)
    e, e_rs = Hh.rel_err(out.cpu(), want), Hh.rel_err(rs.cpu(), want_rs)
    print(f"K={K} M={M} HW={hw} nsplit={ns}: rel_err {e:.3g}, row sums {e_rs:.3g}")
    assert e < 2e-5 and e_rs < 2e-5
    rs2 = torch.full((M,), float("nan"), device=gpu)
    out2 = TR.map_x_mapT_wide(G, X, rowsum=rs2, sum_batch=True)
    assert torch.equal(out, out2) and torch.equal(rs, rs2)
    if K <= 256:                                       # one K tile: the K <= 256 product's launch, bit for bit at the same split count
        part = torch.empty((B, ns, M, K), device=gpu)
        rsp = torch.empty((B, ns, M), device=gpu)
        o3, r3 = torch.full((M, K), float("nan"), device=gpu), torch.full((M,), float("nan"), device=gpu)
        _lib.check(lib.ph_map_x_map_t_ex(_lib.ptr(G), _lib.ptr(X), _lib.ptr(part), _lib.ptr(o3), B, M, K, HW, ns, 0, _lib.ptr(rsp),
                                         _lib.ptr(r3), 1, _lib.stream_ptr()), "ph_map_x_map_t_ex")
        assert torch.equal(out, o3) and torch.equal(rs, r3)


def test_wide_product_per_image_and_without_row_sums(gpu):
    """sum_batch = 0: one [M][K] record per image; no row sums asked for: none written"""
    from polyphonicformer_amd import train as TR
    K, M = 264, 37
    G, X = _wide_inputs(K, "47x71")
    G = G[:, :M].contiguous()
    want = torch.einsum("bmp,bkp->bmk", G.double().flatten(2), X.double().flatten(2))
    out = TR.map_x_mapT_wide(G.to(gpu), X.to(gpu))
    assert out.shape == (B, M, K) and Hh.rel_err(out.cpu(), want) < 2e-5
    summed = TR.map_x_mapT_wide(G.to(gpu), X.to(gpu), sum_batch=True)
    assert Hh.rel_err(summed.cpu(), want.sum(0)) < 2e-5


# =================================================================================================================================
# 2. the nearest add and its backward
# =================================================================================================================================
PAIRS = [((9, 11), (5, 6)), ((5, 6), (3, 3)), ((3, 3), (2, 2)), ((8, 6), (4, 3))]


def _gather(gf, start):
    """the documented order: start + g[2Y][2X] + g[2Y][2X+1] + g[2Y+1][2X] + g[2Y+1][2X+1], in-bounds terms only -- an out-of-bounds
    term is a +0 here, which changes no fp32 value"""
    Hc, Wc = start.shape[-2:]
    pad = torch.zeros(gf.shape[:-2] + (2 * Hc, 2 * Wc))
    pad[..., :gf.shape[-2], :gf.shape[-1]] = gf
    v = start.clone()
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        v = v + pad[..., dy::2, dx::2]
    return v


@pytest.mark.parametrize("fine,coarse", PAIRS)
def test_nearest_add_and_backward_are_exact(gpu, fine, coarse):
    from polyphonicformer_amd import train as TR
    g = _gen(7 + fine[0])
    for planes in ((2, 3), (2, 256)):
        f, c = torch.randn(planes + fine, generator=g), torch.randn(planes + coarse, generator=g)
        want = f + F.interpolate(c, size=fine, mode="nearest")
        fd = f.to(gpu)
        assert TR.nearest_up_add(fd, c.to(gpu)) is fd and torch.equal(fd.cpu(), want)
        gf, gc = torch.randn(planes + fine, generator=g), torch.randn(planes + coarse, generator=g)
        acc = TR.nearest_up_add_bwd(gf.to(gpu), gc.to(gpu), accumulate=True)
        assert torch.equal(acc.cpu(), _gather(gf, gc))
        over = TR.nearest_up_add_bwd(gf.to(gpu), torch.full(planes + coarse, float("nan"), device=gpu), accumulate=False)
        assert torch.equal(over.cpu(), _gather(gf, torch.zeros(planes + coarse)))
        # and the order restated is the transpose torch's autograd computes, to rounding
        cl = c.double().requires_grad_(True)
        with torch.enable_grad():
            (ag,) = torch.autograd.grad(F.interpolate(cl, size=fine, mode="nearest"), cl, gf.double())
        assert Hh.rel_err(over.cpu(), ag) < 1e-6


@pytest.mark.parametrize("planes,fine,coarse", [((1, 2), (130, 131), (65, 66)),          # rows wider than one wave's 64 lanes
                                                ((2, 256), (1025, 3), (513, 2))])         # more rows than one pass of the grid covers
def test_nearest_add_past_one_wave_and_one_grid_pass(gpu, planes, fine, coarse):
    from polyphonicformer_amd import train as TR
    g = _gen(fine[0])
    f, c = torch.randn(planes + fine, generator=g), torch.randn(planes + coarse, generator=g)
    assert planes[0] * planes[1] * coarse[0] > 65536 * 4 or fine[1] > 128
    assert torch.equal(TR.nearest_up_add(f.to(gpu), c.to(gpu)).cpu(), f + F.interpolate(c, size=fine, mode="nearest"))
    assert torch.equal(TR.nearest_up_add_bwd(f.to(gpu), c.to(gpu), accumulate=True).cpu(), _gather(f, c))


def test_nearest_add_refuses_sizes_outside_the_rule(gpu):
    from polyphonicformer_amd import _lib, train as TR
    f, c = torch.zeros(1, 2, 9, 11, device=gpu), torch.zeros(1, 2, 4, 6, device=gpu)
    with pytest.raises(_lib.PolyheadError, match="2 Hc"):
        TR.nearest_up_add(f, c)
    with pytest.raises(_lib.PolyheadError, match="2 Hc"):
        TR.nearest_up_add_bwd(f, c)


# =================================================================================================================================
# 3. bias add and channel sums
# =================================================================================================================================
@pytest.mark.parametrize("HW", [4099, 33828])
def test_bias_add_is_exact_and_channel_sums_follow_float64(gpu, HW):
    from polyphonicformer_amd import _lib, train as TR
    Cn = 6
    g = _gen(HW)
    y, bias = torch.randn(B, Cn, HW, generator=g) + 0.25, torch.randn(Cn, generator=g)
    yd = y.to(gpu)
    assert TR.nchw_bias_add(yd, bias.to(gpu)) is yd and torch.equal(yd.cpu(), y + bias[None, :, None])
    want = y.double().sum((0, 2))
    e_ref = Hh.rel_err(y.sum((0, 2)), want)
    got = TR.nchw_channel_sums(y.to(gpu))
    e = Hh.rel_err(got.cpu(), want)
    print(f"HW={HW}: channel sums err {e:.3g}, e_ref {e_ref:.3g}, splits {_lib.load().ph_nchw_channel_sums_nsplit(HW)}")
    assert got.shape == (Cn,) and e <= max(4 * e_ref, 1e-6)
    assert torch.equal(got, TR.nchw_channel_sums(y.to(gpu)))
    assert _lib.load().ph_nchw_channel_sums_nsplit(HW) == -(-HW // 4096)


# =================================================================================================================================
# 4 - 6. fpn_forward_train
# =================================================================================================================================
def _fpn(gpu):
    from polyphonicformer_amd.registry import NECKS
    import polyphonicformer_amd.fpn  # noqa: F401
    m = NECKS.build(json.load(open(os.path.join(Hh.GOLDEN, "fpn_cfg.json"))))
    m.load_state_dict(Hh.seeded_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, WSEED))
    return m.to(gpu).train()


def _stages(channels):
    g = _gen(ISEED)
    return [torch.randn(B, c, h, w, generator=g).relu() for c, (h, w) in zip(channels, SIZES)]


@functools.lru_cache(maxsize=None)
def _float64_reference():
    """fpn.py:151-203 as tests/test_fpn_host.py restates them, float64 autograd under random cotangents ->
    (cotangents, {name: parameter gradient}, [stage gradients])"""
    sd0 = json.loads(bytes(Hh.load_golden("fpn.npz")["keys_json"]).decode())
    sd = Hh.seeded_fill({k: tuple(v) for k, v in sd0.items()}, WSEED)
    w = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    feats = [t.double().requires_grad_(True) for t in _stages([256, 512, 1024, 2048])]
    with torch.enable_grad():
        lat = [F.conv2d(feats[i], w[f"lateral_convs.{i}.conv.weight"], w[f"lateral_convs.{i}.conv.bias"]) for i in range(4)]
        for i in range(3, 0, -1):
            lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
        ref = [F.conv2d(lat[i], w[f"fpn_convs.{i}.conv.weight"], w[f"fpn_convs.{i}.conv.bias"], padding=1) for i in range(4)]
        g = _gen(17)
        cots = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in ref]
        names = list(w)
        grads = torch.autograd.grad(sum((o * c).sum() for o, c in zip(ref, cots)), [w[n] for n in names] + feats)
    return cots, dict(zip(names, grads[:len(names)])), list(grads[len(names):])


def test_forward_vs_the_reference_class(gpu):
    from polyphonicformer_amd import train as TR
    m = _fpn(gpu)
    gold = Hh.load_golden("fpn.npz")
    with torch.enable_grad():
        outs = TR.fpn_forward_train(m, [t.to(gpu) for t in _stages(m.in_channels)])
    assert isinstance(outs, tuple) and len(outs) == 4 and all(o.requires_grad and o.dtype == torch.float32 for o in outs)
    errs = [Hh.rel_err(o.detach().cpu(), torch.from_numpy(gold[f"out{i}"])) for i, o in enumerate(outs)]
    print("fpn_forward_train vs the reference class, rel_err per level:", errs)
    assert [tuple(o.shape[2:]) for o in outs] == list(SIZES) and max(errs) < 3e-5


def test_gradients_vs_float64_autograd(gpu):
    from polyphonicformer_amd import train as TR
    cots, gp, gs = _float64_reference()
    m = _fpn(gpu)
    st = [t.to(gpu).requires_grad_(True) for t in _stages(m.in_channels)]
    with torch.enable_grad():
        outs = TR.fpn_forward_train(m, st)
        sum((o * c.float().to(gpu)).sum() for o, c in zip(outs, cots)).backward()
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(gp) and len(gp) == 16
    worst_p = worst_s = 0.0
    for n, want in gp.items():
        assert float(want.abs().max()) > 0, n
        e = Hh.rel_err(params[n].grad.cpu(), want)
        print(f"{n}: gradient rel_err {e:.3g}")
        worst_p = max(worst_p, e)
        assert params[n].grad.shape == want.shape and e < 1e-3, n
    for l, want in enumerate(gs):
        assert float(want.abs().max()) > 0, l
        e = Hh.rel_err(st[l].grad.cpu(), want)
        print(f"stage {l}: gradient rel_err {e:.3g}")
        worst_s = max(worst_s, e)
        assert st[l].grad.shape == want.shape and e < 1e-3, l
    print(f"worst parameter gradient {worst_p:.3g}, worst stage gradient {worst_s:.3g}")
    # the gradients are sums in a fixed order: a second backward gives the same bits
    first = [params[n].grad.clone() for n in gp] + [t.grad.clone() for t in st]
    for t in list(params.values()) + st:
        t.grad = None
    with torch.enable_grad():
        outs = TR.fpn_forward_train(m, st)
        sum((o * c.float().to(gpu)).sum() for o, c in zip(outs, cots)).backward()
    assert all(torch.equal(a, b) for a, b in zip(first, [params[n].grad for n in gp] + [t.grad for t in st]))
    # a stage that asks for no gradient gets none, the parameters still do
    for p in params.values():
        p.grad = None
    with torch.enable_grad():
        outs = TR.fpn_forward_train(m, [t.detach() for t in st])
        sum((o * c.float().to(gpu)).sum() for o, c in zip(outs, cots)).backward()
    assert all(torch.equal(params[n].grad, g) for n, g in zip(gp, first))


def test_module_switch_runs_the_device_path(gpu):
    from polyphonicformer_amd import _lib, train as TR
    m = _fpn(gpu)
    st = [t.to(gpu) for t in _stages(m.in_channels)]
    with torch.enable_grad():
        want = TR.fpn_forward_train(m, st)
        off = m(st)
        assert all("Convolution" in type(o.grad_fn).__name__ for o in off)             # the torch branch, as before
        on = m.train_on_device()(st)
        assert all("_Conv3x3Bias" in type(o.grad_fn).__name__ for o in on)
        assert all(torch.equal(a, b) for a, b in zip(on, want))
        with pytest.raises(_lib.PolyheadError, match=r"inputs\[2\]"):
            m([st[0], st[1], st[2].cpu(), st[3]])
        m.lateral_convs[1].conv.half()
        with pytest.raises(_lib.PolyheadError, match=r"lateral_convs\.1\.conv\.weight"):
            m(st)
        m.lateral_convs[1].conv.float()
        assert all("Convolution" in type(o.grad_fn).__name__ for o in m.train_on_device(False)(st))
    with torch.no_grad():                                                              # inference is the plan either way
        ev = m.train_on_device()(st)
    assert all(not o.requires_grad for o in ev)


# =================================================================================================================================
# 7. VideoTrainStep(fpn=...)
# =================================================================================================================================
def test_video_train_step_from_the_backbone_stages(gpu, video_parts):  # noqa: F811
    from polyphonicformer_amd import train as TR
    neck, rpn, roi, th, tcfg, _, _, img, vid = video_parts
    fpn = _fpn(gpu)
    mods = (fpn, neck, rpn, roi, th)
    st = [torch.randn(B, 256 << l, 16 >> l, 32 >> l, generator=_gen(41 + l)).relu().to(gpu) for l in range(4)]
    st_ref = [torch.randn(B, 256 << l, 16 >> l, 32 >> l, generator=_gen(51 + l)).relu().to(gpu) for l in range(4)]

    def clear():
        for top in mods:
            for p in top.parameters():
                p.grad = None

    with torch.enable_grad():
        levels = [t.detach().clone() for t in TR.fpn_forward_train(fpn, st)]
    with torch.no_grad():
        levels_ref = [t.clone() for t in fpn.eval()(st_ref)]
    fpn.train()
    clear()
    with TR.VideoTrainStep(neck, rpn, roi, th, tcfg) as step:
        assert not any(p is q for p in step.parameters() for q in fpn.parameters())
        want_losses, want_total, g_levels = step.forward_backward(levels, levels_ref, *img, *vid)
    clear()
    flags = [m.training for top in mods for m in top.modules()]
    with TR.VideoTrainStep(neck, rpn, roi, th, tcfg, fpn=fpn) as step:
        ps = step.parameters()
        assert len(ps) == len({id(p) for p in ps}) and all(a is b for a, b in zip(ps, fpn.parameters())) and len(list(fpn.parameters())) == 16
        losses, total, g_st = step.forward_backward(st, st_ref, *img, *vid)
    assert [m.training for top in mods for m in top.modules()] == flags
    assert set(losses) == set(want_losses) and len(losses) == 26
    for k, v in want_losses.items():
        assert torch.equal(losses[k], v), (k, float(losses[k]), float(v))
    assert torch.equal(total, want_total)
    for n, p in fpn.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    leaves = [t.detach().clone().requires_grad_(True) for t in st]
    with torch.enable_grad():
        want = torch.autograd.grad(TR.fpn_forward_train(fpn, leaves), leaves, grad_outputs=g_levels)
    assert len(g_st) == 4
    for l in range(4):
        assert g_st[l].shape == st[l].shape and torch.equal(g_st[l], want[l]), l
        assert float(g_st[l].abs().max()) > 0, l
