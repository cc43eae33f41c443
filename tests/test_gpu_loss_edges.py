"""GPU: the loss kernels (csrc/ph_loss.hip) against the loss oracle run in FLOAT64 with autograd (oracle/loss_oracle.py, proven
to be the reference's function by tests/test_loss_oracle.py), at the places the fixture-sized tests never reach: the second trip
of every capped grid-stride loop, the `monodepth` activation's derivative, gamma != 2, saturated logits, the scalar (V = 1) rank
path taken for alignment, a NULL rank target, every `nsplit` / `mask_ns` / `depth_ns` point, and the one-call descriptor form
(`ph_train_losses`) at training size.

Bounds (the suite's, now against float64): values |got - want| <= 2e-5 max(1, |want|), gradients `helpers.rel_err` < 1e-4, and for
the mask_pred / depth_pred gradients a PER-ROW figure (each prediction row normalised by its own float64 maximum, `row_err`),
because `rel_err`'s global maximum hides a row whose gradient is small.  The abs-rel depth term's gradient jumps at p == t: pixels
with float64 |p - t| / t < 1e-6 are left out of the element-wise depth comparisons, at most 1e-5 of a case's counted pixels.

Every "beyond the cap" size is derived from the `loss_grid(..., cap)` calls parsed out of ph_loss.hip, and each such test asserts
that its size really is beyond the cap it quotes.  `python tests/test_gpu_loss_edges.py` (no GPU needed) prints how far the fp32
oracle sits from the float64 one per row on the same inputs: the figure PER_ROW_BOUND is derived from."""
import ctypes as C
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers as Hh
from oracle import loss_oracle as LO
from oracle.poly_oracle import depth_act

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

VALUE_BOUND, GRAD_BOUND = 2e-5, 1e-4
# worst per-row distance of the fp32 CPU oracle from the float64 one over every per-row checked case of this file (measured on the
# CPU by `python tests/test_gpu_loss_edges.py`): 2.77e-5, depth "sigmoid-s12-w0" (a saturated logit under a target close to 0 owns
# its row's maximum: 1 - sigmoid carries fp32's absolute error).  The other families: depth <= 1.2e-6, rank <= 4.7e-7, mask
# <= 2.0e-7, the one-call form <= 1.2e-6.  8 x the worst, for `__expf` and fp32 `powf` in the kernels, kept inside [1e-6, 1e-4].
PER_ROW_FP32_ORACLE = 2.77e-5
PER_ROW_BOUND = min(max(8 * PER_ROW_FP32_ORACLE, 1e-6), 1e-4)
NEAR, NEAR_SHARE = 1e-6, 1e-5

# ---- the launch geometry, read from the source ----------------------------------------------------------------------------------
_SRC = open(os.path.join(Hh.REPO, "polyphonicformer_amd", "csrc", "ph_loss.hip")).read()
LOSS_T = int(re.search(r"constexpr int LOSS_T = (\d+);", _SRC).group(1))


def _cap_exprs(kernel):
    """the cap expression of every `hipLaunchKernelGGL(kernel, dim3(loss_grid(n, cap)...` in the source"""
    found = re.findall(r"hipLaunchKernelGGL\(\s*" + re.escape(kernel) + r"\s*,\s*dim3\(loss_grid\(([^,]+),\s*([^()]+?)\)", _SRC)
    assert found, f"no loss_grid launch of {kernel} in ph_loss.hip"
    return found


def cap(kernel):
    """the one block cap all launches of `kernel` use"""
    caps = {int(c) for _, c in _cap_exprs(kernel)}
    assert len(caps) == 1, (kernel, caps)
    return caps.pop()


def beyond(kernel, V=1, ragged=293):
    """(cap, a size whose grid-stride loop makes a second, partly filled trip): cap * LOSS_T * V + a ragged remainder"""
    c = cap(kernel)
    return c, c * LOSS_T * V + (ragged if V == 1 else 4 * (LOSS_T + 9))


def _csr_grad_cap(depth_rows):
    (_, expr), = _cap_exprs("k_depth_grad_csr")
    m = re.fullmatch(r"c\.depth_rows >= (\d+) \? (\d+) : (\d+)", expr.strip())
    assert m, expr
    return int(m.group(2)) if depth_rows >= int(m.group(1)) else int(m.group(3))


def _layout(P, depth_rows):
    """LossLayout's mask_ns and depth_ns for a descriptor, constants read from the source"""
    m = re.search(r"mask_ns = c\.P > 0 \? \(int\)\((\d+) / c\.P < 1 \? 1 : \(\1 / c\.P > (\d+) \? \2 : \1 / c\.P\)\) : 1;", _SRC)
    d = re.search(r"depth_ns = c\.depth_rows >= (\d+) \? (\d+) : (\d+);", _SRC)
    assert m and d, "LossLayout changed: re-derive the cases of this file"
    budget, top = int(m.group(1)), int(m.group(2))
    mask_ns = max(1, min(top, budget // P)) if P > 0 else 1
    return mask_ns, (int(d.group(2)) if depth_rows >= int(d.group(1)) else int(d.group(3))), budget, top


# ---- comparison helpers --------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def close(got, want, what):
    got, want = float(got), float(want)
    e = abs(got - want) / max(1.0, abs(want))
    print(f"  value {what}: got {got:.9g} want {want:.9g} err {e:.2e}")
    assert np.isfinite(got) and e <= VALUE_BOUND, (what, got, want)


def grad_close(got, want, what, keep=None):
    got = got.detach().double().cpu().reshape(want.shape)
    assert torch.isfinite(got).all(), what
    if keep is not None:
        got, want = got * keep, want * keep
    e = Hh.rel_err(got, want)
    print(f"  grad {what}: rel_err {e:.2e}")
    assert e < GRAD_BOUND, (what, e)


def row_err(got, want, keep=None):
    """max over the rows of max|got - want| / that row's float64 maximum; a row whose maximum is below 1e-12 of the global one
    is measured against 1e-12 of the global maximum instead, i.e. absolutely"""
    want = want.double().reshape(-1, want.shape[-1]) if want.dim() > 1 else want.double().reshape(1, -1)
    d = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    if keep is not None:
        d, want = d * keep.reshape(want.shape), want * keep.reshape(want.shape)
    rmax = want.abs().amax(1)
    norm = rmax.clamp_min(1e-12 * float(rmax.max())).clamp_min(1e-300)
    return float((d.amax(1) / norm).max())


def rows_close(got, want, what, keep=None):
    e = row_err(got, want, keep)
    print(f"  grad {what}: per-row err {e:.2e} (bound {PER_ROW_BOUND:.1e})")
    assert e < PER_ROW_BOUND, (what, e)


def near_mask(z64, tgt, wgt, mode):
    """(keep [like z] of 0 / 1, counted pixels, left out pixels): the pixels at the abs-rel term's sign jump"""
    p, t = depth_act(z64.double(), mode), tgt.double()
    counted = (t > 0) & (t < 80) & (wgt != 0)
    near = counted & ((p - t).abs() / t.clamp_min(1e-30) < NEAR)
    return counted, near


def assert_share(counted, near, what):
    n, k = int(counted.sum()), int(near.sum())
    print(f"  {what}: {k} of {n} counted pixels left out at the sign jump")
    assert k <= NEAR_SHARE * max(n, 1), (what, k, n)


def _lib():
    from polyphonicformer_amd import _lib as L
    return L


# =================================================================================================================================
# depth
# =================================================================================================================================
def depth_inputs(rows, px, scale, seed, kind="random"):
    g = _gen(seed)
    z = torch.randn(rows, px, generator=g) * scale
    t = torch.rand(rows, px, generator=g) * 90.0                      # > 80: not counted
    w = torch.rand(rows, px, generator=g) * (torch.rand(rows, px, generator=g) > 0.3).float() * 1.5      # non-binary, with zeros
    if rows * px >= 16:
        flat = t.view(-1)
        flat[torch.randperm(rows * px, generator=g)[: max(2, rows * px // 10)]] = 0.0          # exactly 0: unlabelled
        flat[torch.randperm(rows * px, generator=g)[: max(2, rows * px // 50)]] = 80.0         # exactly 80: not < 80
    if kind == "one":        # exactly one counted pixel
        w.zero_()
        k = rows * px // 2
        w.view(-1)[k], t.view(-1)[k] = 0.7, 33.25
    elif kind == "none":     # weights only where the target is not counted
        w = w * ((t <= 0) | (t >= 80)).float()
    elif rows * px == 1:
        t[0, 0], w[0, 0] = 12.5, 0.8
    return z, t, w


def depth_ref(z, t, w, mode, terms, dtype, loss_weight=5.0):
    with torch.enable_grad():
        zz = z.to(dtype).requires_grad_(True)
        v = LO.depth_loss(zz, t, w, mode, loss_weight=loss_weight, weights=terms)
        g = torch.autograd.grad(v, zz)[0] if v.requires_grad else torch.zeros_like(zz)      # no counted pixel: a constant
    return v.detach(), g


DEPTH_CASES = {}
for _mode in ("sigmoid", "monodepth"):
    for _scale in (1.0, 12.0):
        for _terms in ((1.0, 0.5, 2.0), (0.0, 1.0, 1.0)):
            DEPTH_CASES[f"{_mode}-s{_scale:g}-w{_terms[0]:g}"] = dict(rows=8, px=493, scale=_scale, mode=_mode, terms=_terms)
DEPTH_CASES.update({
    "size1": dict(rows=1, px=1, scale=1.0, mode="monodepth", terms=(1.0, 0.5, 2.0)),
    "size255": dict(rows=1, px=255, scale=12.0, mode="monodepth", terms=(1.0, 0.5, 2.0)),
    "size257": dict(rows=1, px=257, scale=1.0, mode="sigmoid", terms=(1.0, 0.5, 2.0)),
    "one-pixel": dict(rows=3, px=257, scale=1.0, mode="monodepth", terms=(1.0, 0.5, 2.0), kind="one"),
})


def _depth_on_gpu(gpu, z, t, w, mode, terms):
    from polyphonicformer_amd import losses as Lo
    L = _lib()
    zd, td, wd = z.to(gpu).contiguous(), t.to(gpu).contiguous(), w.to(gpu).contiguous()
    mod = Lo.DepthLoss(loss_weight=5.0, depth_act_mode=mode, si_weight=terms[0], sq_rel_weight=terms[1], abs_rel_weight=terms[2])
    value = mod(zd, td, wd)
    sums = Lo.depth_loss_sums(zd, td, wd, Lo.DEPTH_MODES[mode])
    v2, coef = Lo._depth_from_sums(sums, 5.0, list(terms))
    grad = torch.full_like(zd, float("nan"))                          # the kernel overwrites every element
    L.check(L.load().ph_depth_loss_grad(L.ptr(zd), L.ptr(td), L.ptr(wd), zd.numel(), Lo.DEPTH_MODES[mode], *coef, L.ptr(grad),
                                        L.stream_ptr()), "ph_depth_loss_grad")
    torch.cuda.synchronize()
    assert float(v2.float()) == float(value)
    return value, grad


def _check_depth(gpu, z, t, w, mode, terms, what):
    value, grad = _depth_on_gpu(gpu, z, t, w, mode, terms)
    want, wg = depth_ref(z, t, w, mode, terms, torch.float64)
    counted, near = near_mask(z, t, w, mode)
    assert_share(counted, near, what)
    keep = (~near).double()
    close(value, want, what)
    grad_close(grad, wg, what, keep)
    rows_close(grad, wg, what, keep)


@pytest.mark.parametrize("name", sorted(DEPTH_CASES))
def test_depth_vs_float64(gpu, name):
    c = DEPTH_CASES[name]
    z, t, w = depth_inputs(c["rows"], c["px"], c["scale"], 100 + sorted(DEPTH_CASES).index(name), c.get("kind", "random"))
    if c.get("kind") == "one":
        assert int(near_mask(z, t, w, c["mode"])[0].sum()) == 1
    _check_depth(gpu, z, t, w, c["mode"], c["terms"], name)


def test_depth_without_a_counted_pixel_is_exactly_zero(gpu):
    for mode in ("sigmoid", "monodepth"):
        z, t, w = depth_inputs(4, 493, 12.0, 140, "none")
        assert int(near_mask(z, t, w, mode)[0].sum()) == 0 and (w != 0).any()
        value, grad = _depth_on_gpu(gpu, z, t, w, mode, (1.0, 0.5, 2.0))
        assert float(value) == 0.0 and float(depth_ref(z, t, w, mode, (1.0, 0.5, 2.0), torch.float64)[0]) == 0.0
        assert torch.equal(grad, torch.zeros_like(grad))               # no NaN, no -0 + garbage: all bits zero or -0
        assert not torch.isnan(grad).any()


@pytest.mark.parametrize("kernel", ["k_depth_loss_sums", "k_depth_loss_grad"])
def test_depth_beyond_the_cap(gpu, kernel):
    c, total = beyond(kernel)
    assert total > c * LOSS_T, (kernel, c, total)
    z, t, w = depth_inputs(1, total, 4.0, 150)
    _check_depth(gpu, z, t, w, "monodepth", (1.0, 0.5, 2.0), f"{kernel} cap {c}, {total} pixels")


# =================================================================================================================================
# focal
# =================================================================================================================================
def focal_inputs(R, L, scale, seed):
    g = _gen(seed)
    z = torch.randn(R, L, generator=g) * scale
    labels = torch.randint(0, L + 1, (R,), generator=g)             # == L: background
    labels[: max(1, R // 4)] = L
    w = torch.rand(R, L, generator=g) * (torch.rand(R, L, generator=g) > 0.3).float()
    return z, labels, w


def focal_ref(z, labels, w, gamma, alpha, dtype, avg=7.0, lw=2.0):
    with torch.enable_grad():
        zz = z.to(dtype).requires_grad_(True)
        v = LO.focal_loss(zz, labels, w, avg, gamma=gamma, alpha=alpha, loss_weight=lw)
        g, = torch.autograd.grad(v, zz)
    return v.detach(), g


def _check_focal(gpu, R, L, gamma, alpha, scale, seed, what):
    from polyphonicformer_amd import losses as Lo
    Lb = _lib()
    z, labels, w = focal_inputs(R, L, scale, seed)
    assert (labels == L).any() and (w == 0).any()
    zd, ld, wd = z.to(gpu), labels.to(gpu), w.to(gpu).contiguous()
    value = Lo.FocalLoss(use_sigmoid=True, gamma=gamma, alpha=alpha, loss_weight=2.0)(zd, ld, wd, avg_factor=7.0)
    grad = torch.full_like(zd, float("nan"))
    Lb.check(Lb.load().ph_focal_loss_grad(Lb.ptr(zd), Lb.ptr(ld), Lb.ptr(wd), R, L, gamma, alpha, 2.0 / 7.0, Lb.ptr(grad), Lb.stream_ptr()),
             "ph_focal_loss_grad")
    want, wg = focal_ref(z, labels, w, gamma, alpha, torch.float64)
    close(value, want, what)
    grad_close(grad, wg, what)


@pytest.mark.parametrize("scale", [1.0, 10.0, 40.0])
@pytest.mark.parametrize("alpha", [0.25, 0.6])
@pytest.mark.parametrize("gamma", [2.0, 1.5])
@pytest.mark.parametrize("L", [19, 133])
def test_focal_vs_float64(gpu, L, gamma, alpha, scale):
    _check_focal(gpu, 75, L, gamma, alpha, scale, 200 + L, f"focal L={L} gamma={gamma} alpha={alpha} scale={scale}")


@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_focal_beyond_the_cap(gpu, gamma):
    c = cap("k_focal<true>")
    assert c == cap("k_focal<false>")
    L = 133
    R = c * LOSS_T // L + 37
    assert R * L > c * LOSS_T, (R, L, c)
    _check_focal(gpu, R, L, gamma, 0.25, 10.0, 260, f"focal R*L={R * L} over cap {c}")


# =================================================================================================================================
# focal over a class-major map (KernelHead's loss_rpn_seg)
# =================================================================================================================================
def seg_inputs(B, L, HW, scale, seed):
    g = _gen(seed)
    z = torch.randn(B, L, HW, generator=g) * scale
    t = torch.randint(0, L + 1, (B, HW), generator=g)               # == L: pixel not selected
    t[0, 0] = 3
    t[B - 1] = L                                                     # the last image has no selected pixel
    return z, t


def seg_ref(z, t, gamma, alpha, dtype, lw=1.0):
    """the seg part of LO.rpn_loss (kernel_head.py:539-551) on [B, L, HW]"""
    L = z.shape[1]
    with torch.enable_grad():
        zz = z.to(dtype).requires_grad_(True)
        sel = t != L
        flat = zz.permute(1, 0, 2)[..., sel].permute(1, 0)
        ft = t[sel]
        nd = ((ft >= 0) & (ft < L)).sum().float().clamp(min=1.0)
        v = LO.focal_loss(flat, ft, torch.ones(()), nd, gamma=gamma, alpha=alpha, loss_weight=lw)
        g, = torch.autograd.grad(v, zz)
    return v.detach(), g, float(nd)


def _check_seg(gpu, B, L, HW, gamma, scale, seed, what):
    from polyphonicformer_amd import losses as Lo
    Lb = _lib()
    z, t = seg_inputs(B, L, HW, scale, seed)
    want, wg, nd = seg_ref(z, t, gamma, 0.25, torch.float64)
    zd, td = z.to(gpu), t.to(torch.int32).to(gpu)
    value = Lo.seg_focal_sum(zd, td, gamma, 0.25) / nd
    grad = torch.full_like(zd, float("nan"))
    Lb.check(Lb.load().ph_seg_focal_grad(Lb.ptr(zd), Lb.ptr(td), B, L, HW, gamma, 0.25, 1.0 / nd, Lb.ptr(grad), Lb.stream_ptr()),
             "ph_seg_focal_grad")
    close(value, want, what)
    grad_close(grad, wg, what)
    assert torch.equal(grad[B - 1], torch.zeros_like(grad[B - 1])), "an image without a selected pixel has no gradient"


@pytest.mark.parametrize("scale", [2.0, 40.0])
@pytest.mark.parametrize("HW", [1, 493])
@pytest.mark.parametrize("L", [19, 133])
@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_seg_focal_vs_float64(gpu, gamma, L, HW, scale):
    _check_seg(gpu, 3, L, HW, gamma, scale, 300 + L + HW, f"seg focal gamma={gamma} L={L} HW={HW} scale={scale}")


@pytest.mark.parametrize("gamma", [2.0, 1.5])
def test_seg_focal_beyond_the_cap(gpu, gamma):
    c, HW = beyond("k_seg_focal<true>")
    assert c == cap("k_seg_focal<false>") and HW > c * LOSS_T
    _check_seg(gpu, 2, 19, HW, gamma, 2.0, 360, f"seg focal HW={HW} over cap {c}")


# =================================================================================================================================
# rank
# =================================================================================================================================
IGNORE = 255


def rank_inputs(B, N, HW, scale, seed):
    g = _gen(seed)
    z = torch.randn(B, N, HW, generator=g) * scale
    t = torch.randint(0, N, (B, HW), generator=g)
    t[torch.rand(B, HW, generator=g) < 0.2] = IGNORE
    if HW >= 16:
        t[:, 0:4] = IGNORE                                           # a vector of four pixels wholly ignored
        t[:, 4:6] = IGNORE                                           # one partly ignored
        t[:, 6:8] = N - 1
        t[:, HW - 1] = IGNORE
    else:
        t[0, 0] = 0
    return z, t


def rank_ref(z, t, dtype, lw=0.1):
    B, N, HW = z.shape
    with torch.enable_grad():
        zz = z.to(dtype).requires_grad_(True)
        v = LO.rank_loss(zz.reshape(B, N, HW, 1), t.reshape(B, HW, 1), IGNORE, loss_weight=lw)
        g, = torch.autograd.grad(v, zz)
    return v.detach(), g


def _rank_on_gpu(gpu, zd, td, lw=0.1):
    """zd [B, N, HW] on the device (possibly a view at a storage offset), td int32 [B, HW] or None"""
    from polyphonicformer_amd import losses as Lo
    Lb = _lib()
    B, N, HW = zd.shape
    assert zd.is_contiguous()
    value = None
    if td is not None:
        value = Lo.CrossEntropyLoss(use_sigmoid=False, loss_weight=lw, ignore_index=IGNORE)(zd.reshape(B, N, HW, 1), td.reshape(B, HW, 1))
    grad = torch.full((B, N, HW), float("nan"), device=gpu)
    Lb.check(Lb.load().ph_rank_loss_grad(Lb.ptr(zd), Lb.ptr(td), B, N, HW, IGNORE, lw / (B * HW), Lb.ptr(grad), Lb.stream_ptr()),
             "ph_rank_loss_grad")
    return value, grad


def _check_rank(gpu, B, N, HW, scale, seed, what):
    z, t = rank_inputs(B, N, HW, scale, seed)
    value, grad = _rank_on_gpu(gpu, z.to(gpu), t.to(torch.int32).to(gpu))
    want, wg = rank_ref(z, t, torch.float64)
    close(value, want, what)
    grad_close(grad, wg, what)
    rows_close(grad, wg, what)


@pytest.mark.parametrize("HW", [492, 493])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 153])
def test_rank_vs_float64(gpu, N, HW):
    for scale in (2.0, 40.0):
        _check_rank(gpu, 2, N, HW, scale, 400 + N, f"rank N={N} HW={HW} scale={scale}")


def test_rank_alignment_fallback_is_bit_identical(gpu):
    """HW % 4 == 0 but `pred` starts one float into its storage: the scalar kernels run, and give what the vector ones give"""
    B, N, HW = 2, 153, 492
    z, t = rank_inputs(B, N, HW, 2.0, 470)
    td = t.to(torch.int32).to(gpu)
    aligned = z.to(gpu)
    store = torch.zeros(B * N * HW + 8, device=gpu)
    store[1:1 + B * N * HW] = aligned.reshape(-1)
    off = store[1:1 + B * N * HW].view(B, N, HW)
    assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off.storage_offset() == 1 and HW % 4 == 0
    v0, g0 = _rank_on_gpu(gpu, aligned, td)
    v1, g1 = _rank_on_gpu(gpu, off, td)
    assert torch.equal(g0, g1) and float(v0) == float(v1)
    want, wg = rank_ref(z, t, torch.float64)
    close(v1, want, "rank, offset view")
    grad_close(g1, wg, "rank, offset view")


def test_rank_null_target_gives_zero_gradient(gpu):
    for HW in (492, 493):
        z, _ = rank_inputs(2, 5, HW, 2.0, 480)
        _, grad = _rank_on_gpu(gpu, z.to(gpu), None)
        assert torch.equal(grad, torch.zeros_like(grad)), HW


@pytest.mark.parametrize("kernel,V", [("k_rank_loss_sum<4>", 4), ("k_rank_loss_sum<1>", 1), ("k_rank_loss_grad<4>", 4), ("k_rank_loss_grad<1>", 1)])
def test_rank_beyond_the_cap(gpu, kernel, V):
    c, HW = beyond(kernel, V)
    assert HW > c * LOSS_T * V and (HW % 4 == 0) == (V == 4), (kernel, c, HW)
    _check_rank(gpu, 1, 2, HW, 2.0, 490, f"{kernel} cap {c}, HW={HW}")


# =================================================================================================================================
# mask BCE + dice
# =================================================================================================================================
def mask_inputs(R, HW, rows, seed):
    g = _gen(seed)
    z = torch.randn(R, HW, generator=g) * 2
    sat = rows[1]                                                    # a positive row of +-50 logits against soft targets
    z[sat] = (torch.randint(0, 2, (HW,), generator=g).float() * 2 - 1) * 50.0
    t = torch.randint(0, 5, (R, HW), generator=g).float() / 4        # soft: what the x4 bilinear downsample leaves (k / 4)
    w = (torch.rand(R, HW, generator=g) > 0.2).float()
    if HW >= 8:
        w[rows[-1]] = 0.0                                            # a positive row without a weighted pixel
    else:
        w[rows[0]] = 1.0
    return z, t, w


def mask_ref(z, t, w, rows, dtype, lw_mask=1.0, lw_dice=4.0, eps=1e-3):
    """the mask part of LO.stage_loss (kernel_update_head.py:408-419) on [R, HW] with explicit positive rows"""
    with torch.enable_grad():
        zz = z.to(dtype).requires_grad_(True)
        pm, pt, pw = zz[rows], t[rows], w[rows].bool()
        bce = LO.bce_mean(pm[pw], pt[pw], loss_weight=lw_mask)
        dice = torch.stack([LO.dice_one(pm[i][pw[i]], pt[i][pw[i]], eps=eps, loss_weight=lw_dice) for i in range(len(rows))]).mean()
        g, = torch.autograd.grad(bce + dice, zz)
    return bce.detach(), dice.detach(), g


def _mask_on_gpu(gpu, z, t, w, rows, nsplit, prefill=None, lw_mask=1.0, lw_dice=4.0, eps=1e-3):
    from polyphonicformer_amd import losses as Lo
    Lb = _lib()
    zd, td, wd = z.to(gpu), t.to(gpu), w.to(gpu)
    rd = torch.tensor(rows, dtype=torch.int32, device=gpu)
    P, HW = len(rows), z.shape[1]
    s = Lo.mask_loss_sums(zd, td, wd, rd, nsplit)                    # [P, 5] fp64: bce, count, a, b, c
    ntot = s[:, 1].sum()
    bc = s[:, 3] + s[:, 4] + 2 * eps
    bce, dice = lw_mask * s[:, 0].sum() / ntot, lw_dice * (1 - 2 * s[:, 2] / bc).mean()
    # the gradient kernel's contract: coef [P][3] = bce scale, dice A = -2 lw / (P (b + c)), dice B = 4 lw a / (P (b + c)^2)
    coef = torch.stack([lw_mask / ntot.expand(P), -2.0 * lw_dice / (P * bc), 4.0 * lw_dice * s[:, 2] / (P * bc * bc)], 1).float().contiguous()
    grad = torch.zeros_like(zd) if prefill is None else prefill.to(gpu).clone()
    Lb.check(Lb.load().ph_mask_loss_grad(Lb.ptr(zd), Lb.ptr(td), Lb.ptr(wd), Lb.ptr(rd), P, HW, Lb.ptr(coef), Lb.ptr(grad), Lb.stream_ptr()),
             "ph_mask_loss_grad")
    return bce, dice, grad, s


MASK_CASES = {"ns1": (493, 1), "ns3": (493, 3), "ns64": (493, 64), "hw17-ns64": (17, 64), "hw17-ns3": (17, 3), "hw1-ns3": (1, 3)}


@pytest.mark.parametrize("name", sorted(MASK_CASES))
def test_mask_vs_float64(gpu, name):
    HW, nsplit = MASK_CASES[name]
    rows = [5, 1, 6, 0, 3]                                           # not ascending; rows 2, 4, 7 are not positive
    assert rows != sorted(rows) and (HW % nsplit != 0 or HW < nsplit or nsplit == 1)
    z, t, w = mask_inputs(8, HW, rows, 500 + HW + nsplit)
    bce, dice, grad, s = _mask_on_gpu(gpu, z, t, w, rows, nsplit)
    wb, wd, wg = mask_ref(z, t, w, rows, torch.float64)
    close(bce, wb, f"mask bce {name}")
    close(dice, wd, f"dice {name}")
    assert torch.equal(s[:, 1].cpu(), w[rows].sum(1).double()), "every weighted pixel is counted once, whatever the split"
    grad_close(grad, wg, f"mask {name}")
    rows_close(grad, wg, f"mask {name}")
    # the kernel ADDS: a prefilled buffer keeps its values on the unweighted pixels and the other rows, and gains g elsewhere
    pre = torch.randn(z.shape, generator=_gen(7)) * float(wg.abs().max())
    _, _, grad2, _ = _mask_on_gpu(gpu, z, t, w, rows, nsplit, prefill=pre)
    touched = torch.zeros_like(w, dtype=torch.bool)
    touched[rows] = w[rows] != 0
    assert torch.equal(grad2.cpu()[~touched], pre[~touched]) and (~touched).any()
    assert torch.equal(grad2.cpu(), pre + grad.cpu())
    assert not grad.cpu()[~touched].any()


def test_mask_grad_beyond_the_cap(gpu):
    c, HW = beyond("k_mask_loss_grad")
    assert c == cap("k_mask_grad_p") and HW > c * LOSS_T
    rows = [2, 0, 3]
    z, t, w = mask_inputs(4, HW, rows, 560)
    for nsplit in (3, 64):
        bce, dice, grad, _ = _mask_on_gpu(gpu, z, t, w, rows, nsplit)
        wb, wd, wg = mask_ref(z, t, w, rows, torch.float64)
        close(bce, wb, f"mask bce HW={HW} nsplit={nsplit}")
        close(dice, wd, f"dice HW={HW} nsplit={nsplit}")
        grad_close(grad, wg, f"mask HW={HW} over cap {c}")
        rows_close(grad, wg, f"mask HW={HW} over cap {c}")


# =================================================================================================================================
# the one-call form: losses.build_desc + losses.fused_losses (ph_train_losses)
# =================================================================================================================================
FUSED_CASES = {
    # roi=True (KernelUpdateHead stage): N = Np + n_stuff rows, depth_rows = B * N
    "mini17x29": dict(B=2, H=17, W=29, nt=3, ns=2, Np=7, G=[3, 2]),                                       # P = 9: mask_ns 64; 18 depth rows
    "mid24x40": dict(B=2, H=24, W=40, nt=8, ns=11, Np=100, G=[40, 30], mode="monodepth", pw=2.0, terms=(1.0, 0.5, 2.0),
                     gamma=1.5, alpha=0.6),                                                                # P = 82: mask_ns 2048 / P
    "train128x256": dict(B=2, H=128, W=256, nt=8, ns=11, Np=153, G=[12, 9]),                               # training size
    "wide17x29": dict(B=5, H=17, W=29, nt=8, ns=11, Np=410, G=[7] * 5, all_rows=True, mode="monodepth"),   # P > 2048: mask_ns 1
    "no-instance-one": dict(B=2, H=24, W=40, nt=8, ns=11, Np=100, G=[5, 0], no_stuff=[1], terms=(0.0, 1.0, 1.0)),
    "nothing-at-all": dict(B=2, H=17, W=29, nt=8, ns=11, Np=20, G=[0, 0], no_stuff=[0, 1]),
    # roi=False (KernelHead): N = Np rows, a dense semantic target, depth_rows = B with several items per row
    "rpn-soft": dict(B=2, H=24, W=40, nt=8, ns=11, Np=100, G=[6, 4], roi=False, hard=False, gamma=1.5),
    "rpn-hard": dict(B=2, H=24, W=40, nt=8, ns=11, Np=100, G=[6, 4], roi=False, hard=True, mode="monodepth", pw=2.0, terms=(1.0, 0.5, 2.0)),
    "rpn-no-instance": dict(B=2, H=17, W=29, nt=8, ns=11, Np=20, G=[0, 0], roi=False, hard=False),
}


def _head(c):
    from polyphonicformer_amd import losses as Lo
    t = c.get("terms", (1.0, 1.0, 1.0))
    focal = dict(use_sigmoid=True, gamma=c.get("gamma", 2.0), alpha=c.get("alpha", 0.25))
    return SimpleNamespace(num_classes=c["nt"] + c["ns"], num_thing_classes=c["nt"], num_stuff_classes=c["ns"], ignore_label=IGNORE,
                           loss_rank=Lo.CrossEntropyLoss(use_sigmoid=False, loss_weight=0.1),
                           loss_mask=Lo.CrossEntropyLoss(use_sigmoid=True, loss_weight=1.0), loss_dice=Lo.DiceLoss(loss_weight=4.0),
                           loss_cls=Lo.FocalLoss(loss_weight=2.0, **focal), loss_seg=Lo.FocalLoss(loss_weight=1.0, **focal),
                           loss_depth=Lo.DepthLoss(loss_weight=5.0, depth_act_mode=c.get("mode", "sigmoid"), si_weight=t[0],
                                                   sq_rel_weight=t[1], abs_rel_weight=t[2]))


def _oracle_kw(c, roi):
    kw = dict(depth_terms=c.get("terms", (1.0, 1.0, 1.0)), depth_mode=c.get("mode", "sigmoid"))
    kw.update(dict(cls_gamma=c.get("gamma", 2.0), cls_alpha=c.get("alpha", 0.25)) if roi else
              dict(seg_gamma=c.get("gamma", 2.0), seg_alpha=c.get("alpha", 0.25)))
    return kw


@functools.lru_cache(maxsize=None)
def fused_inputs(name):
    """CPU: ground truth (helpers.train_gt, masks softened to k / 4), an assignment, predictions, the oracle's targets"""
    c = FUSED_CASES[name]
    B, H, W, nt, ns, Np = c["B"], c["H"], c["W"], c["nt"], c["ns"], c["Np"]
    roi, hard = c.get("roi", True), c.get("hard", False)
    L = nt + ns
    seed = 600 + sorted(FUSED_CASES).index(name)
    g = _gen(seed)
    gts = Hh.train_gt(seed, B, H, W, nt, ns, c["G"])
    assigns = []
    for b, gt in enumerate(gts):
        G = c["G"][b]
        gt["masks"] = gt["masks"] * torch.randint(1, 5, (G, H, W), generator=g).float() / 4
        if b in c.get("no_stuff", []):
            gt["sem_seg"], gt["sem_cls"] = torch.zeros(0, H, W), torch.zeros(0, dtype=torch.long)
        if c.get("all_rows"):
            pi, gi = np.arange(Np, dtype=np.int64), np.arange(Np, dtype=np.int64) % G
        else:
            pi = np.sort(torch.randperm(Np, generator=g)[:G].numpy()).astype(np.int64)
            gi = torch.randperm(G, generator=g).numpy().astype(np.int64)
        assigns.append((pi, gi))
    # the oracle's view of the same step: hardened masks where the head hardens them, gt_inds / assigned labels per prediction
    ogts, valids = [], []
    for gt, (pi, gi) in zip(gts, assigns):
        o = dict(gt)
        if hard:
            o["masks"] = (gt["masks"] != 0).float()
        o["gt_inds"] = torch.zeros(Np, dtype=torch.long)
        o["gt_inds"][torch.from_numpy(pi)] = torch.from_numpy(gi) + 1
        o["assigned_labels"] = torch.full((Np,), -1, dtype=torch.long)
        o["assigned_labels"][torch.from_numpy(pi)] = gt["labels"][torch.from_numpy(gi)]
        ogts.append(o)
        valids.append(torch.cat((o["masks"], o["sem_seg"]), 0).sum(0).bool().float())
    N = Np + ns if roi else Np
    preds = dict(mask_pred=torch.randn(B, N, H, W, generator=g) * 2)
    if roi:
        preds["cls_score"] = torch.randn(B, N, L, generator=g) * 2
        preds["depth_pred"] = torch.randn(B, N, H, W, generator=g) * 1.5
        tg = LO.get_targets(L, nt, ns, Np, H, W, ogts, valids, pos_weight=c.get("pw", 1.0))
    else:
        preds["seg_preds"] = torch.randn(B, L, H, W, generator=g) * 2
        preds["depth_pred"] = torch.randn(B, 1, H, W, generator=g) * 1.5
        tg = LO.rpn_get_targets(L, nt, ns, Np, H, W, ogts, valids, pos_weight=c.get("pw", 1.0))
    return c, gts, assigns, preds, tg


def fused_ref(name, dtype):
    """the oracle's losses and d(sum of the 'loss' entries) / d(predictions) in `dtype`, + the depth comparison's keep mask"""
    c, gts, assigns, preds, tg = fused_inputs(name)
    roi, L = c.get("roi", True), c["nt"] + c["ns"]
    with torch.enable_grad():
        p = {k: v.to(dtype).requires_grad_(True) for k, v in preds.items()}
        if roi:
            losses = LO.stage_loss(L, p["cls_score"], p["mask_pred"], p["depth_pred"], *tg, **_oracle_kw(c, roi))
        else:
            losses = LO.rpn_loss(L, p["mask_pred"], p["seg_preds"], p["depth_pred"], *tg, **_oracle_kw(c, roi))
        names = list(p)
        gr = torch.autograd.grad(sum(v for k, v in losses.items() if k.startswith("loss")), [p[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(p[k]) if g_ is None else g_).detach() for k, g_ in zip(names, gr)}
    # depth pixels at the abs-rel sign jump (any item of a prediction row)
    dt, dw = tg[-2], tg[-1]
    B, H, W = c["B"], c["H"], c["W"]
    dp = preds["depth_pred"].expand(B, dt.shape[0] // B, H, W).reshape(dt.shape)
    counted, near = near_mask(dp, dt, dw, c.get("mode", "sigmoid"))
    keep = (~near).reshape(B, -1, H, W)
    if not roi:
        keep = keep.all(1, keepdim=True)
    return {k: v.detach() for k, v in losses.items()}, grads, keep.double(), (counted, near)


@functools.lru_cache(maxsize=None)
def fused_ref64(name):
    return fused_ref(name, torch.float64)


_GPU_RUNS = {}


def fused_on_gpu(gpu, name):
    """(desc, fused losses / grads of two runs, unfused losses / grads), once per module"""
    if name in _GPU_RUNS:
        return _GPU_RUNS[name]
    from polyphonicformer_amd import losses as Lo
    c, gts, assigns, preds, tg = fused_inputs(name)
    roi = c.get("roi", True)
    head = _head(c)
    dg = [{k: v.to(gpu) for k, v in g.items()} for g in gts]
    gt = Lo.StepGT([g["masks"] for g in dg], [g["labels"] for g in dg], [g["sem_seg"] for g in dg], [g["sem_cls"] for g in dg],
                   [g["depth"] for g in dg], hard_target=c.get("hard", False))
    desc = Lo.build_desc(head, gt, assigns, c["Np"], SimpleNamespace(pos_weight=c.get("pw", 1.0)), roi=roi)
    p = {k: v.to(gpu) for k, v in preds.items()}
    runs = []
    for _ in range(2):
        losses, grads = Lo.fused_losses(head, desc, p["mask_pred"], p.get("cls_score"), p["depth_pred"], p.get("seg_preds"), with_grads=True)
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in losses.items()}, {k: v.clone() for k, v in grads.items() if v is not None}))
    dtg = [t.to(gpu) for t in tg]
    if roi:
        unfused = Lo.stage_losses(head, p["cls_score"], p["mask_pred"], p["depth_pred"], *dtg, with_grads=True)
    else:
        unfused = Lo.rpn_losses(head, p["mask_pred"], p["seg_preds"], p["depth_pred"], *dtg, with_grads=True)
    torch.cuda.synchronize()
    _GPU_RUNS[name] = (desc, runs, unfused)
    return _GPU_RUNS[name]


def test_fused_cases_cover_the_layout(gpu):
    """the cases land where this file says they do: all three mask_ns points, depth_rows on both sides of its threshold, second
    trips of k_mask_grad_p and k_depth_grad_csr at training size"""
    seen_ns, seen_dns = set(), set()
    for name in FUSED_CASES:
        c = FUSED_CASES[name]
        desc = fused_on_gpu(gpu, name)[0]
        mask_ns, depth_ns, budget, top = _layout(desc.P, desc.depth_rows)
        print(f"  {name}: P={desc.P} mask_ns={mask_ns} depth_rows={desc.depth_rows} depth_ns={depth_ns}")
        if desc.P:
            seen_ns.add("top" if mask_ns == top else ("one" if desc.P > budget else "budget / P"))
        seen_dns.add(depth_ns)
        if name == "wide17x29":
            assert desc.P > budget and mask_ns == 1
        if name == "train128x256":
            HW = c["H"] * c["W"]
            assert desc.N == 153 + c["ns"] and HW > cap("k_mask_grad_p") * LOSS_T and HW > _csr_grad_cap(desc.depth_rows) * LOSS_T
        if name == "nothing-at-all":
            assert desc.P == 0
    assert seen_ns == {"top", "budget / P", "one"} and len(seen_dns) == 2, (seen_ns, seen_dns)


@pytest.mark.parametrize("name", sorted(FUSED_CASES))
def test_fused_vs_float64(gpu, name):
    c = FUSED_CASES[name]
    _, runs, _ = fused_on_gpu(gpu, name)
    want, wg, keep, (counted, near) = fused_ref64(name)
    losses, grads = runs[0]
    assert set(losses) == set(want), (sorted(losses), sorted(want))       # the reference's key names, also without positives
    assert_share(counted, near, name)
    for k in sorted(want):
        close(losses[k], want[k], f"{name} {k}")
    for k in sorted(wg):
        kp = keep if k == "depth_pred" else None
        assert tuple(grads[k].shape) == tuple(wg[k].shape), k
        grad_close(grads[k], wg[k], f"{name} d/d{k}", kp)
        if k in ("mask_pred", "depth_pred"):
            HW = c["H"] * c["W"]
            rows_close(grads[k].reshape(-1, HW), wg[k].reshape(-1, HW), f"{name} d/d{k}", None if kp is None else kp.reshape(-1, HW))


@pytest.mark.parametrize("name", sorted(FUSED_CASES))
def test_fused_vs_unfused(gpu, name):
    """the descriptor form against `stage_losses` / `rpn_losses` on the oracle's materialised targets: same bounds"""
    _, runs, (ul, ug) = fused_on_gpu(gpu, name)
    _, _, keep, _ = fused_ref64(name)
    losses, grads = runs[0]
    assert set(losses) == set(ul), (sorted(losses), sorted(ul))
    for k in sorted(ul):
        close(losses[k], ul[k], f"{name} {k} (vs unfused)")
    for k in sorted(ug):
        grad_close(grads[k], ug[k].double().cpu(), f"{name} d/d{k} (vs unfused)", keep if k == "depth_pred" else None)


@pytest.mark.parametrize("name", sorted(FUSED_CASES))
def test_fused_is_bit_reproducible(gpu, name):
    _, runs, _ = fused_on_gpu(gpu, name)
    (l0, g0), (l1, g1) = runs
    assert all(torch.equal(l0[k], l1[k]) for k in l0) and set(g0) == set(g1)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


# =================================================================================================================================
# CPU only: how far the fp32 oracle sits from the float64 one per row, on the inputs of the per-row checks above
# =================================================================================================================================
def fp32_oracle_per_row_figures():
    out = {}
    for name in sorted(DEPTH_CASES):
        c = DEPTH_CASES[name]
        z, t, w = depth_inputs(c["rows"], c["px"], c["scale"], 100 + sorted(DEPTH_CASES).index(name), c.get("kind", "random"))
        counted, near = near_mask(z, t, w, c["mode"])
        out[f"depth {name}"] = (row_err(depth_ref(z, t, w, c["mode"], c["terms"], torch.float32)[1],
                                        depth_ref(z, t, w, c["mode"], c["terms"], torch.float64)[1], (~near).double()), int(near.sum()), int(counted.sum()))
    for kernel in ("k_depth_loss_sums", "k_depth_loss_grad"):
        z, t, w = depth_inputs(1, beyond(kernel)[1], 4.0, 150)
        counted, near = near_mask(z, t, w, "monodepth")
        out[f"depth {kernel}"] = (row_err(depth_ref(z, t, w, "monodepth", (1.0, 0.5, 2.0), torch.float32)[1],
                                          depth_ref(z, t, w, "monodepth", (1.0, 0.5, 2.0), torch.float64)[1], (~near).double()), int(near.sum()), int(counted.sum()))
    for N in (1, 2, 3, 4, 5, 153):
        for HW in (492, 493):
            for scale in (2.0, 40.0):
                z, t = rank_inputs(2, N, HW, scale, 400 + N)
                out[f"rank N={N} HW={HW} s={scale}"] = (row_err(rank_ref(z, t, torch.float32)[1], rank_ref(z, t, torch.float64)[1]), 0, 0)
    for name in sorted(MASK_CASES):
        HW, nsplit = MASK_CASES[name]
        rows = [5, 1, 6, 0, 3]
        z, t, w = mask_inputs(8, HW, rows, 500 + HW + nsplit)
        out[f"mask {name}"] = (row_err(mask_ref(z, t, w, rows, torch.float32)[2], mask_ref(z, t, w, rows, torch.float64)[2]), 0, 0)
    for name in sorted(FUSED_CASES):
        c = FUSED_CASES[name]
        HW = c["H"] * c["W"]
        _, g32, _, _ = fused_ref(name, torch.float32)
        _, g64, keep, (counted, near) = fused_ref64(name)
        for k in ("mask_pred", "depth_pred"):
            kp = keep.reshape(-1, HW) if k == "depth_pred" else None
            out[f"fused {name} {k}"] = (row_err(g32[k].reshape(-1, HW), g64[k].reshape(-1, HW), kp), int(near.sum()), int(counted.sum()))
    return out


if __name__ == "__main__":
    figs = fp32_oracle_per_row_figures()
    for k, (e, near, counted) in figs.items():
        print(f"{e:.3e}  left out {near} of {counted}  {k}")
    print("worst", max(e for e, _, _ in figs.values()))
