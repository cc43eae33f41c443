"""GPU: the map-sized training kernels past one tile, against float64 torch autograd on the CPU.

Every other GPU test of the training path runs on maps of 128 to 512 pixels: one 256-pixel tile of the 3x3 convolution, one split
of its weight gradient, one split and one slice of GroupNorm, at most two splits of a map x map^T product.  Here each kernel runs
where its launch geometry engages, and every case asserts -- through `ph_gn_train_nsplit`, `ph_gn_train_bwd_nsplit`,
`ph_map_x_map_t_nsplit` and the `slices` formula parsed out of ph_gntrain.hip -- that it reaches the count it is named for.

  1. GroupNorm + ReLU (csrc/ph_gntrain.hip: `train.gn_relu_fwd` / `train.gn_relu_bwd`) against `torch.native_group_norm(...)[0]
     .relu()`: out, out + add, the statistics (mean as |d| rstd, rstd relative), dx (global and per (image, channel) row), dgamma,
     dbeta; with / without `add`, `want_out`, `dyB`.  Bound per quantity: max(4 e_ref, 1e-6), e_ref = the distance of the float32 CPU
     `native_group_norm` path from the float64 one on the same inputs, computed in the test (`python tests/test_gpu_train_tiles.py`
     prints the table without a GPU).  A pre-activation within 5e-5 of 0 is a coin flip between device and float64: such elements
     of `y` are pushed away by 1e-3 and the test asserts that none remains.
  2. the 3x3 convolution node (`train._Conv3x3`) against float64 `F.conv2d` autograd, rel_err < 3e-5: tile boundaries in the middle
     of an image row, a short last split of the weight gradient, every parity of the stride-2 input gradient.
  3. `train.rows_x_map` / `train.map_x_mapT` against float64 einsum, rel_err < 2e-5, binarised row sums exact: ragged HW over two
     blocks, 14 splits (one 8-way unrolled body of `k_sum_splits` + a tail of 6), 42 records under `sum_batch`, two row passes.
  4. the neck in training (`train.neck_forward_train` through SemanticFPNWrapper) against `oracle/neck_oracle.semantic_fpn` in
     float64 under autograd, EVERY entry of the three outputs (1e-4), the 30 parameter gradients and the four input gradients
     (1e-3); the fixture's GroupNorm biases are nudged until no float64 GroupNorm output lies within 5e-5 of 0.

Measured on an MI355X (worst over the cases of a family):
  GroupNorm    worst device error 3.1e-7 (mean, offset 16: 0.35 e_ref) outside the two constant-2.3 cases, 6.9e-6 there (`out`,
               1.45 e_ref: the float32 x * scale + shift form itself); worst device / e_ref over all cases and quantities 1.91
               (dx at HW = 4100, 1.4e-7 against 7.2e-8), the statistics <= 1.0 e_ref; e_ref is at most 9e-7 but for dgamma / dbeta
               at HW >= 33828 (<= 6.0e-6), dgamma under the offset (8.9e-6) and the cases with the constant-2.3 group (out 4.7e-6,
               dx rows 2.1e-6, dgamma 3.5e-4).
               Before the statistics pass widened its elements to fp64 ahead of squaring, rstd and dx of the constant-2.3 cases
               were off by 8.9e-3 on both paths (bound 1e-6); every other case passed as it does now.
  conv 3x3     y 5.5e-6, dx 5.3e-6, dw 4.9e-6 (bound 3e-5); in-channels 40 needed the padded input-gradient form of `_Conv3x3`
  products     rows_x_map 8.8e-6 (47x71, M = 161, K = 40), map_x_mapT 3.6e-6 (bound 2e-5); binarised row sums exact
  neck         outputs 1.0e-5 (bound 1e-4), parameter gradients 1.6e-5, input gradients 1.1e-5 (bound 1e-3)
"""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
from oracle import neck_oracle as NO

pytestmark = pytest.mark.gpu

MARGIN = 5e-5               # test_gpu_qtrain.condition_relus' margin around a ReLU's 0
FACTOR, FLOOR = 4.0, 1e-6   # bound = max(FACTOR * e_ref, FLOOR): test_gpu_optim.py's factor, test_gpu_loss_edges.py's floor

# ---- the launch geometry of ph_gntrain.hip, read from the source ---------------------------------------------------------------
_SRC = open(os.path.join(Hh.REPO, "polyphonicformer_amd", "csrc", "ph_gntrain.hip")).read()


def _parse(pattern, what):
    m = re.search(pattern, _SRC)
    assert m, f"ph_gntrain.hip: {what} is gone -- re-derive the cases of tests/test_gpu_train_tiles.py"
    return m


GT_T = int(_parse(r"constexpr int GT_T = (\d+);", "GT_T").group(1))
_m = _parse(r"int64_t g = \(n \+ GT_T \* (\d+) \* (\d+) - 1\) / \(GT_T \* \1 \* \2\);\s*(?://[^\n]*)?\s*"
            r"return \(int\)\(g < 1 \? 1 : \(g > (\d+) \? \3 : g\)\);", "the slices() formula")
SLICE_PX, SLICE_CAP = GT_T * int(_m.group(1)) * int(_m.group(2)), int(_m.group(3))
FWD_CAP = int(_parse(r"ph_gn_train_nsplit\(int64_t HW, int cpg\) \{ return slices\(HW \* cpg\) > (\d+) \? \1 : slices\(HW \* cpg\); \}",
                     "the forward nsplit cap").group(1))
BWD_CAP = int(_parse(r"ph_gn_train_bwd_nsplit\(int64_t HW\) \{ return slices\(HW\) > (\d+) \? \1 : slices\(HW\); \}",
                     "the backward nsplit cap").group(1))


def uncapped(n):
    return max(1, -(-n // SLICE_PX))


def slices(n):
    return min(uncapped(n), SLICE_CAP)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _lib():
    from polyphonicformer_amd import _lib as L
    return L.load()


def row_err(got, want):
    """max over the rows of max|got - want| / that row's float64 maximum (rows: the last axis); a row whose maximum is below 1e-12
    of the global one is measured against 1e-12 of the global maximum -- test_gpu_loss_edges.row_err"""
    want = want.double().reshape(-1, want.shape[-1])
    d = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    rmax = want.abs().amax(1)
    norm = rmax.clamp_min(1e-12 * float(rmax.max())).clamp_min(1e-300)
    return float((d.amax(1) / norm).max())


# =================================================================================================================================
# 1. GroupNorm + ReLU
# =================================================================================================================================
# fwd / bwd: the split counts the library must report; fwd_raw / bwd_raw: slices before the cap; ap / ap_raw: apply slices
GN_CASES = {
    "hw1028": dict(B=2, C=16, G=2, HW=1028, fwd=3, bwd=1, ap=1),                       # split bounds 2741, 5482: no multiples of 4
    "hw4100": dict(B=2, C=16, G=2, HW=4100, fwd=9, bwd=2, ap=2, extras=0.0),          # bwd bound 2050 -> 2048
    "hw4100-offset16": dict(B=2, C=16, G=2, HW=4100, fwd=9, bwd=2, ap=2, offset=16.0),  # mean / std ~ 16: a 1x1 conv of a post-ReLU map
    "hw4099": dict(B=2, C=16, G=2, HW=4099, fwd=9, bwd=2, ap=2, extras=0.0),          # the same on the scalar path
    "hw4100-const2.3": dict(B=2, C=16, G=2, HW=4100, fwd=9, bwd=2, ap=2, extras=2.3),  # the constant group at a value whose square
    "hw4099-const2.3": dict(B=2, C=16, G=2, HW=4099, fwd=9, bwd=2, ap=2, extras=2.3),  # is no float32 number, both paths
    "hw4100-unaligned": dict(B=2, C=16, G=2, HW=4100, fwd=9, bwd=2, ap=2, shift=True),  # scalar path chosen by alignment
    "hw33828": dict(B=1, C=4, G=2, HW=33828, fwd=16, fwd_raw=17, bwd=8, bwd_raw=9, ap=9),
    "hw263204": dict(B=1, C=2, G=1, HW=263204, fwd=16, fwd_raw=129, bwd=8, bwd_raw=65, ap=64, ap_raw=65),
    "cpg1": dict(B=2, C=8, G=8, HW=4100, fwd=2, bwd=2, ap=2),                         # one channel per group
    "c264": dict(B=1, C=264, G=33, HW=36, fwd=1, bwd=1, ap=1),                        # two blocks of k_gnt_bwd_params
}


def _gn_autograd(y, gamma, beta, add, dyA, dyB, G, dtype):
    """native_group_norm + relu in `dtype`, the two backward forms (dy = dyA, dy = dyA + dyB), and the pre-activation"""
    B, C, HW = y.shape
    with torch.enable_grad():
        yy, gg, bb = (t.to(dtype).requires_grad_(True) for t in (y, gamma, beta))
        pre, mean, rstd = torch.native_group_norm(yy, gg, bb, B, C, HW, G, 1e-5)
        out = pre.relu()
        r = dict(pre=pre.detach(), out=out.detach(), osum=(out + add.to(dtype)).detach(), mean=mean.detach().reshape(B, G),
                 rstd=rstd.detach().reshape(B, G))
        for name, cot in (("A", dyA.to(dtype)), ("AB", dyA.to(dtype) + dyB.to(dtype))):
            r["dx" + name], r["dg" + name], r["db" + name] = [t.detach() for t in torch.autograd.grad(out, (yy, gg, bb), cot, retain_graph=True)]
    return r


@functools.lru_cache(maxsize=None)
def gn_fixture(name):
    """(inputs, the float64 reference, the float32 one), ReLU decisions conditioned.  CPU only; shared by the tests of a case."""
    c = GN_CASES[name]
    B, C, G, HW = c["B"], c["C"], c["G"], c["HW"]
    g = _gen(1000 + sorted(GN_CASES).index(name))
    y = torch.randn(B, C, HW, generator=g) + c.get("offset", 0.0)
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    add, dyA, dyB = torch.randn(B, C, HW, generator=g).relu(), torch.randn(B, C, HW, generator=g), torch.randn(B, C, HW, generator=g)
    if "extras" in c:
        gamma[2] = -0.8
        gamma[5], beta[5] = 0.0, 0.15                # gamma = 0: the pre-activation is beta everywhere
        gamma[11], beta[11] = 1e-2, 0.08             # a small-gamma channel: its dx row is what a global maximum hides
        # image 1, group 1: constant, variance 0.  0.0 (dead channels): every e_ref stays at rounding level.  2.3: x * scale + shift
        # cancels two products of 2.3 * rstd = 727 in float32, so xhat is 4e-5 instead of 0 there (e_ref of dgamma: 1e-4); and the
        # float32 square of float32(2.3) lies 1.8e-7 ABOVE the exact one: sums of squares rounded to float32 give var = 1.8e-7
        # against eps = 1e-5, an rstd that is 0.9 % low
        y[1, C // 2:] = c["extras"]
    for _ in range(2):                               # one pass suffices at these sizes (7, 8, 74 elements -> 0)
        pre = torch.native_group_norm(y.double(), gamma.double(), beta.double(), B, C, HW, G, 1e-5)[0]
        near = pre.abs() < MARGIN
        if not near.any():
            break
        # away from 0: d pre / d y has the sign of gamma
        sign = torch.where(pre >= 0, 1.0, -1.0) * torch.where(gamma >= 0, 1.0, -1.0)[None, :, None].double()
        y = torch.where(near, y + 1e-3 * sign.float(), y)
    pre = torch.native_group_norm(y.double(), gamma.double(), beta.double(), B, C, HW, G, 1e-5)[0]
    assert int((pre.abs() < MARGIN).sum()) == 0, (name, int((pre.abs() < MARGIN).sum()))
    inp = dict(y=y, gamma=gamma, beta=beta, add=add, dyA=dyA, dyB=dyB)
    r64 = _gn_autograd(y, gamma, beta, add, dyA, dyB, G, torch.float64)
    r32 = _gn_autograd(y, gamma, beta, add, dyA, dyB, G, torch.float32)
    return inp, r64, r32


def gn_errors(got, want):
    """the figure of every compared quantity; `got`: a dict like `_gn_autograd`'s (tensors of any float type, any device)"""
    e = {"out": Hh.rel_err(got["out"].cpu(), want["out"]), "out+add": Hh.rel_err(got["osum"].cpu(), want["osum"]),
         "mean": float(((got["mean"].cpu().double() - want["mean"]).abs() * want["rstd"]).max()),
         "rstd": float(((got["rstd"].cpu().double() - want["rstd"]).abs() / want["rstd"]).max())}
    for s in ("A", "AB"):
        sfx = "" if s == "A" else " (dyB)"
        e["dx" + sfx] = Hh.rel_err(got["dx" + s].cpu(), want["dx" + s])
        e["dx rows" + sfx] = row_err(got["dx" + s], want["dx" + s])
        e["dgamma" + sfx] = Hh.rel_err(got["dg" + s].cpu(), want["dg" + s])
        e["dbeta" + sfx] = Hh.rel_err(got["db" + s].cpu(), want["db" + s])
    return e


def _shifted(t, gpu):
    """a contiguous device copy of `t` that starts one float into its storage"""
    store = torch.zeros(t.numel() + 8, device=gpu)
    store[1:1 + t.numel()] = t.reshape(-1).to(gpu)
    v = store[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("name", sorted(GN_CASES))
def test_gn_relu_vs_float64(gpu, name):
    from polyphonicformer_amd import train as T
    c = GN_CASES[name]
    B, C, G, HW = c["B"], c["C"], c["G"], c["HW"]
    cpg = C // G
    lib = _lib()
    # the case is where its name says
    assert lib.ph_gn_train_nsplit(HW, cpg) == c["fwd"] == min(uncapped(HW * cpg), FWD_CAP), (lib.ph_gn_train_nsplit(HW, cpg), c)
    assert lib.ph_gn_train_bwd_nsplit(HW) == c["bwd"] == min(uncapped(HW), BWD_CAP), (lib.ph_gn_train_bwd_nsplit(HW), c)
    assert slices(HW) == c["ap"] and uncapped(HW * cpg) == c.get("fwd_raw", c["fwd"]) and uncapped(HW) == c.get("bwd_raw", c["bwd"])
    assert uncapped(HW) == c.get("ap_raw", c["ap"])
    if name == "hw1028":
        assert all((HW * cpg * s // c["fwd"]) % 4 for s in range(1, c["fwd"]))
    if name == "hw263204":
        assert HW % (SLICE_CAP * GT_T * 4) != 0 and HW > SLICE_CAP * GT_T * 4                 # further trips, the last partly filled
    if name == "c264":
        assert C > GT_T
    inp, r64, r32 = gn_fixture(name)
    vec = HW % 4 == 0 and not c.get("shift")
    put = (lambda t: _shifted(t, gpu)) if c.get("shift") else (lambda t: t.to(gpu).contiguous())
    y, dyA = put(inp["y"]), put(inp["dyA"])
    gamma, beta, add, dyB = (inp[k].to(gpu) for k in ("gamma", "beta", "add", "dyB"))
    if not c.get("shift"):
        assert (y.data_ptr() | dyA.data_ptr() | add.data_ptr() | dyB.data_ptr()) % 16 == 0
    print(f"  {name}: fwd nsplit {c['fwd']}, bwd nsplit {c['bwd']}, apply slices {c['ap']}, {'vector' if vec else 'scalar'} path")
    # forward: without add / with add / with add and the sum only
    out0, none0, st0 = T.gn_relu_fwd(y, gamma, beta, G)
    out1, osum1, st1 = T.gn_relu_fwd(y, gamma, beta, G, add=add)
    none2, osum2, st2 = T.gn_relu_fwd(y, gamma, beta, G, add=add, want_out=False)
    out3, none3, st3 = T.gn_relu_fwd(y, gamma, beta, G, want_out=False)             # nothing else to return: `out` all the same
    torch.cuda.synchronize()
    assert none0 is None and none2 is None and none3 is None
    assert torch.equal(out0, out1) and torch.equal(out0, out3) and torch.equal(osum1, osum2)
    assert torch.equal(st0, st1) and torch.equal(st0, st2) and torch.equal(st0, st3)
    got = dict(out=out0, osum=osum1, mean=st0[..., 0], rstd=st0[..., 1])
    # backward on the device's own statistics: dy = dyA, dy = dyA + dyB
    got["dxA"], got["dgA"], got["dbA"] = T.gn_relu_bwd(y, st0, gamma, beta, G, dyA)
    got["dxAB"], got["dgAB"], got["dbAB"] = T.gn_relu_bwd(y, st0, gamma, beta, G, dyA, dyB)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in got.values())
    e_dev, e_ref = gn_errors(got, r64), gn_errors(r32, r64)
    bad = []
    for k in e_dev:
        bound = max(FACTOR * e_ref[k], FLOOR)
        print(f"  {name} {k:>14}: device {e_dev[k]:.2e}  e_ref {e_ref[k]:.2e}  ratio {e_dev[k] / max(e_ref[k], 1e-300):8.2f}  bound {bound:.2e}")
        if not e_dev[k] <= bound:
            bad.append((k, e_dev[k], bound))
    assert not bad, (name, bad)


# =================================================================================================================================
# 2. the 3x3 convolution node
# =================================================================================================================================
CONV_TILE = 256             # pixels per workgroup of k_conv3x3_rows (64 * CT)
# stride, B, K, M, Hi, Wi, output tiles, input-gradient tiles, weight-gradient nsplit, its splits
CONV_CASES = {
    "s1-17x19": (1, 2, 40, 48, 17, 19, 2, 2, 2, (192, 131)),               # scalar path, tile boundary at pixel 256 = row 13, column 9
    "s1-20x28": (1, 1, 32, 176, 20, 28, 3, 3, 3, (192, 192, 176)),         # vector path, two m-passes in both kernels
    "s2-35x37": (2, 2, 40, 48, 35, 37, 2, 6, 2, (192, 150)),               # 18 x 19 out, odd x odd
    "s2-36x40": (2, 1, 32, 48, 36, 40, 2, 6, 2, (192, 168)),               # 18 x 20 out, even x even: last row / column by some taps only
    "s2-35x40": (2, 1, 32, 48, 35, 40, 2, 6, 2, (192, 168)),               # mixed parity
}


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv3x3_node_past_one_tile(gpu, name):
    from polyphonicformer_amd import train as T
    stride, B, K, M, Hi, Wi, tiles_out, tiles_in, nsplit, splits = CONV_CASES[name]
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    HWo = Ho * Wo
    assert -(-HWo // CONV_TILE) == tiles_out and -(-(Hi * Wi) // CONV_TILE) == tiles_in and tiles_out >= 2
    assert _lib().ph_map_x_map_t_nsplit(B, M, HWo) == nsplit
    chunk = (-(-HWo // nsplit) + 31) // 32 * 32                      # the split length, rounded up to the 32-pixel step
    assert tuple(min(chunk, HWo - s * chunk) for s in range(nsplit)) == splits
    if name == "s1-17x19":
        assert CONV_TILE % Wo != 0 and HWo % 4 != 0
    if name == "s1-20x28":
        assert HWo % 4 == 0 and M > 160 and M // 16 > 8
    g = _gen(Hi * Wi + stride)
    x, w = torch.randn(B, K, Hi, Wi, generator=g), torch.randn(M, K, 3, 3, generator=g) * 0.05
    with torch.enable_grad():
        xc, wc = x.double().requires_grad_(True), w.double().requires_grad_(True)
        yc = F.conv2d(xc, wc, None, stride=stride, padding=1)
        cot = torch.randn(yc.shape, generator=g)
        (yc * cot.double()).sum().backward()
        xd, wd = x.to(gpu).requires_grad_(True), w.to(gpu).requires_grad_(True)
        yd = T._Conv3x3.apply(xd, wd, stride)
        (yd * cot.to(gpu)).sum().backward()
    torch.cuda.synchronize()
    assert yd.shape == yc.shape and xd.grad.shape == x.shape and wd.grad.shape == w.shape
    e = (Hh.rel_err(yd.detach().cpu(), yc.detach()), Hh.rel_err(xd.grad.cpu(), xc.grad), Hh.rel_err(wd.grad.cpu(), wc.grad))
    print(f"  conv3x3 {name} (y, dx, dw) rel err: {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}")
    assert max(e) < 3e-5, e


# =================================================================================================================================
# 3. map products
# =================================================================================================================================
PROD_BOUND = 2e-5
PROD_HW = {"17x19": (17, 19, 2), "49x68": (49, 68, 14), "47x71": (47, 71, 14)}          # H, W, nsplit of map_x_mapT


def _prod_inputs(hw, M, K, B):
    H, W, _ = PROD_HW[hw]
    g = _gen(H * W + M + K)
    return (torch.randn(B, M, K, generator=g), torch.randn(B, K, H, W, generator=g) - 0.3, torch.randn(B, M, H, W, generator=g) - 0.3,
            torch.randn(B, M, generator=g), torch.randn(B, M, H, W, generator=g))


def _prod_close(got, want, what):
    e = Hh.rel_err(got.cpu(), want)
    print(f"  {what}: rel_err {e:.2e}")
    assert tuple(got.shape) == tuple(want.shape) and e < PROD_BOUND, (what, e)
    return e


@pytest.mark.parametrize("K", [256, 40])
@pytest.mark.parametrize("M", [161, 37])
@pytest.mark.parametrize("hw", sorted(PROD_HW))
def test_rows_x_map_past_one_block(gpu, hw, M, K):
    from polyphonicformer_amd import train as T
    H, W, _ = PROD_HW[hw]
    B, HW = 2, H * W
    assert HW > 256 and (HW % 4 == 0) == (hw == "49x68") and ((M + 15) // 16 > 10) == (M == 161)
    A, X, _, bias, add = _prod_inputs(hw, M, K, B)
    A64, X64 = A.double(), X.double()
    Xb = (X > T.BIN_THR).double()
    Ad, Xd = A.to(gpu), X.to(gpu)
    what = f"rows_x_map {hw} M={M} K={K}"
    _prod_close(T.rows_x_map(Ad, Xd), torch.einsum("bmk,bkhw->bmhw", A64, X64), what)
    _prod_close(T.rows_x_map(Ad, Xd, binarize_x=True), torch.einsum("bmk,bkhw->bmhw", A64, Xb), what + " binarize_x")
    want = torch.einsum("bmk,bkhw->bmhw", A64, X64) + bias.double()[:, :, None, None] + add.double()
    _prod_close(T.rows_x_map(Ad, Xd, bias=bias.to(gpu), add=add.to(gpu)), want, what + " bias + add")
    out = add.to(gpu).clone()
    res = T.rows_x_map(Ad, Xd, out=out, accumulate=True)
    assert res is out
    _prod_close(out, torch.einsum("bmk,bkhw->bmhw", A64, X64) + add.double(), what + " accumulate")
    shared = T.rows_x_map(Ad[:1], Xd)
    _prod_close(shared, torch.einsum("mk,bkhw->bmhw", A64[0], X64), what + " A shared")
    _prod_close(T.rows_x_map(Ad[:1], Xd, binarize_x=True), torch.einsum("mk,bkhw->bmhw", A64[0], Xb), what + " A shared, binarize_x")


@pytest.mark.parametrize("K", [256, 40])
@pytest.mark.parametrize("M", [161, 37])
@pytest.mark.parametrize("hw", sorted(PROD_HW))
def test_map_x_mapT_past_two_splits(gpu, hw, M, K):
    from polyphonicformer_amd import train as T
    H, W, nsplit = PROD_HW[hw]
    HW = H * W
    lib = _lib()
    # B = 1: `nsplit` records per output (14 = one unrolled body of k_sum_splits + a tail of 6); B = 3 + sum_batch: 3 nsplit records
    assert lib.ph_map_x_map_t_nsplit(1, M, HW) == nsplit and lib.ph_map_x_map_t_nsplit(3, M, HW) == nsplit
    assert nsplit == 2 or (nsplit >= 8 and nsplit % 8 == 6 and 3 * nsplit == 42)
    _, X, Gm, _, _ = _prod_inputs(hw, M, K, 3)
    X64, G64 = X.double(), Gm.double()
    Gb = (Gm > T.BIN_THR).double()
    Xd, Gd = X.to(gpu), Gm.to(gpu)
    what = f"map_x_mapT {hw} M={M} K={K}"
    _prod_close(T.map_x_mapT(Gd[:1], Xd[:1]), torch.einsum("bmhw,bkhw->bmk", G64[:1], X64[:1]), what)
    rs = torch.full((1, M), float("nan"), device=gpu)
    _prod_close(T.map_x_mapT(Gd[:1], Xd[:1], binarize_g=True, rowsum=rs), torch.einsum("bmhw,bkhw->bmk", Gb[:1], X64[:1]), what + " binarize_g")
    assert torch.equal(rs.cpu().double(), Gb[:1].sum((2, 3))), "the pixel count of every hard mask is exact"
    rs = torch.full((1, M), float("nan"), device=gpu)
    T.map_x_mapT(Gd[:1], Xd[:1], rowsum=rs)
    _prod_close(rs, G64[:1].sum((2, 3)), what + " rowsum")
    # the batch: per image, and summed over the images in the split reduction
    _prod_close(T.map_x_mapT(Gd, Xd), torch.einsum("bmhw,bkhw->bmk", G64, X64), what + " B=3")
    rs = torch.full((M,), float("nan"), device=gpu)
    _prod_close(T.map_x_mapT(Gd, Xd, rowsum=rs, sum_batch=True), torch.einsum("bmhw,bkhw->mk", G64, X64), what + " sum_batch")
    _prod_close(rs, G64.sum((0, 2, 3)), what + " sum_batch rowsum")
    rs = torch.full((M,), float("nan"), device=gpu)
    _prod_close(T.map_x_mapT(Gd, Xd, binarize_g=True, rowsum=rs, sum_batch=True), torch.einsum("bmhw,bkhw->mk", Gb, X64), what + " sum_batch binarize_g")
    assert torch.equal(rs.cpu().double(), Gb.sum((0, 2, 3))), "binarised row sums over the batch are exact"


# =================================================================================================================================
# 4. the neck in training, element-wise
# =================================================================================================================================
NECK_CASES = {
    # stride-8 map 24 x 28 = 672 px: 3 conv tiles, GroupNorm forward nsplit 2, weight-gradient nsplit 3
    "48x56": dict(B=1, H0=48, W0=56, wseed=33, iseed=34, cseed=35),
    # stride-8 map 20 x 36; the coarsest level is 5 x 9: no aligned rows
    "40x72": dict(B=2, H0=40, W0=72, wseed=36, iseed=37, cseed=38),
}
NECK_GROUPS, NECK_C = 32, 256


def _neck_condition(sd, feats, rounds=20):
    """test_gpu_qtrain.condition_relus for the neck: the offending channel's gn.bias is nudged by +2e-3 until no float64 GroupNorm
    output of the oracle's forward lies within MARGIN of 0 (52 -> 31 -> 19 -> 9 -> 0 of 1.3 M elements on the first case)"""
    real = F.group_norm
    f64 = [f.double() for f in feats]
    for _ in range(rounds):
        sd64 = {k: v.double() for k, v in sd.items()}
        key_of = {id(v): k for k, v in sd64.items()}
        seen = []

        def spy(x, groups, weight=None, bias=None, eps=1e-5):
            out = real(x, groups, weight, bias, eps)
            seen.append((key_of[id(bias)], out.detach()))
            return out

        F.group_norm = spy
        try:
            with torch.no_grad():
                NO.semantic_fpn(sd64, f64, groups=NECK_GROUPS)
        finally:
            F.group_norm = real
        assert len(seen) == 10 and len({k for k, _ in seen}) == 10, [k for k, _ in seen]
        near = 0
        for key, t in seen:
            close = (t.abs() < MARGIN).any(3).any(2).any(0)
            near += int((t.abs() < MARGIN).sum())
            if close.any():
                sd[key] = sd[key] + 2e-3 * close.float()
        if near == 0:
            return sd
    raise AssertionError("could not condition the neck fixture")


@functools.lru_cache(maxsize=None)
def neck_fixture(name):
    import json
    c = NECK_CASES[name]
    with open(Hh.GOLDEN + "/neck_state_keys.json") as f:
        shapes = json.load(f)["full"]
    sd = Hh.seeded_fill({k: tuple(v) for k, v in shapes.items()}, c["wseed"])
    feats = Hh.fpn_inputs(seed=c["iseed"], B=c["B"], C=NECK_C, H0=c["H0"], W0=c["W0"])
    sd = _neck_condition(sd, feats)
    g = _gen(c["cseed"])
    with torch.enable_grad():
        w = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        fi = [f.double().requires_grad_(True) for f in feats]
        outs = NO.semantic_fpn(w, fi, groups=NECK_GROUPS)
        cots = [torch.randn(o.shape, generator=g) for o in outs]
        sum((o * ct.double()).sum() for o, ct in zip(outs, cots)).backward()
    return sd, feats, cots, [o.detach() for o in outs], {k: v.grad for k, v in w.items()}, [f.grad for f in fi]


@pytest.mark.parametrize("name", sorted(NECK_CASES))
def test_neck_training_every_entry_vs_float64(gpu, name):
    from polyphonicformer_amd.registry import NECKS
    import polyphonicformer_amd.semantic_fpn  # noqa: F401
    c = NECK_CASES[name]
    lib = _lib()
    B, H8, W8 = c["B"], c["H0"] // 2, c["W0"] // 2
    if name == "48x56":
        assert H8 * W8 == 672 and -(-H8 * W8 // CONV_TILE) == 3 and lib.ph_gn_train_nsplit(H8 * W8, NECK_C // NECK_GROUPS) == 2
        assert lib.ph_map_x_map_t_nsplit(B, NECK_C, H8 * W8) == 3
    else:
        assert ((c["H0"] >> 3) * (c["W0"] >> 3)) % 4 != 0 and (c["W0"] >> 3) % 4 != 0 and -(-H8 * W8 // CONV_TILE) == 3
        assert lib.ph_gn_train_nsplit(H8 * W8, NECK_C // NECK_GROUPS) == 2
    sd, feats, cots, outs64, gw64, gin64 = neck_fixture(name)
    neck = NECKS.build(dict(type="SemanticFPNWrapper", in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
                            upsample_times=2, positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                            cat_coors=False, cat_coors_level=3, fuse_by_cat=False, return_list=False, num_aux_convs=2,
                            norm_cfg=dict(type="GN", num_groups=NECK_GROUPS, requires_grad=True)))
    neck.load_state_dict(sd)
    neck.to(gpu).train()
    fd = [f.to(gpu).requires_grad_(True) for f in feats]
    with torch.enable_grad():
        outs = neck(fd)
        sum((o * ct.to(gpu)).sum() for o, ct in zip(outs, cots)).backward()
    torch.cuda.synchronize()
    assert len(outs) == 3
    params = dict(neck.named_parameters())
    assert len(params) == 30 and set(params) == set(gw64)
    worst_out = max(Hh.rel_err(o.detach().cpu(), w) for o, w in zip(outs, outs64))
    eg = {n: Hh.rel_err(p.grad.cpu(), gw64[n]) for n, p in params.items()}
    ei = [Hh.rel_err(f.grad.cpu(), w) for f, w in zip(fd, gin64)]
    wn = max(eg, key=eg.get)
    print(f"  neck {name}: outputs {worst_out:.2e}; parameter gradients worst {eg[wn]:.2e} ({wn}); input gradients {['%.2e' % v for v in ei]}")
    for o, w in zip(outs, outs64):
        assert o.shape == w.shape
    assert worst_out < 1e-4, worst_out
    assert max(eg.values()) < 1e-3, sorted(eg.items(), key=lambda kv: -kv[1])[:3]
    assert max(ei) < 1e-3, ei


# =================================================================================================================================
# CPU only: how far the float32 native_group_norm path sits from the float64 one, per case and quantity
# =================================================================================================================================
if __name__ == "__main__":
    print(f"GT_T {GT_T}, {SLICE_PX} elements per slice, slice cap {SLICE_CAP}, nsplit caps {FWD_CAP} forward / {BWD_CAP} backward")
    for case in sorted(GN_CASES):
        _, ref64, ref32 = gn_fixture(case)
        print(case, "  ".join(f"{k} {v:.2e}" for k, v in gn_errors(ref32, ref64).items()))
