"""GPU: the track head's training path at real RoI counts, every entry against float64 on the CPU.

tests/test_gpu_track_train.py runs the branch on 3 + 4 RoIs and compares parameter gradients through 256 samples and a norm.  Here
each part runs where its tiling engages -- more than one 64-row tile of `ph_gemm32`, 130 images of 7 x 7 through `_Conv3x3` /
`_GNReLU` (130 records under `k_sum_splits`: sixteen 8-way bodies and a tail of 2), 128 x 128 in `ph_track_loss` with ties at the
hard-negative cut, more than 256 RoIs in the RoIAlign pair -- and every entry of every result is compared.  The inputs and their
float64 references come from tests/track_edge_cases.py (seeded, computed once per process); the conditions they rely on (mining
gaps and ties, ReLU margins, RoI sample coordinates) are asserted without a GPU in tests/test_track_oracle_host.py.

Bounds
  a, b  products: max(4 e_ref, 1e-6) per tensor, e_ref = the distance of the float32 CPU computation from the float64 one on the
        same inputs, computed in the test (the rule of tests/test_gpu_train_tiles.py)
  c, d, g  the stack's existing bounds, over every entry: 1e-4 outputs and losses, 1e-3 gradients through conv + GroupNorm
  e, f  3e-5, one fp32 node against float64 (tests/test_gpu_track_train.py)

Measured on an MI355X (worst over the cases of a family; device error, then its bound):
  gemm32 X W^T     4.8e-7 against 1.55e-6 (M = 130, N = 1024, K = 12544 in one pass), worst device / bound 0.35; one pass over
                   K = 12544 at M = 64, 65, 130: 3.5e-7 .. 4.8e-7 against 1.3e-6 .. 3.0e-6, 16 splits 1.5e-7 .. 2.8e-7.  Before
                   `k_gemm32` added every 128 k into a second accumulator those one-pass cases measured 3.5e-6 .. 4.6e-6, up to
                   2.95 x their bound (`test_gemm32_x_wT`).  Nothing outside [M][N] written in any call.
  gemm32 backward  (1,0) and (0,0) with K = n: 5.5e-7 against 1.9e-6, worst device / bound 0.29
  _FcEmbed         gW2 4.4e-7 against 1.33e-6 (n = 130), worst device / bound 0.35 (gW2, n = 65); out 2.6e-7, gx 2.8e-7, gW1 3.6e-7
  conv + GroupNorm y 4.7e-6 (1e-4); dx 5.5e-6, dw 4.7e-6, dgamma 3.7e-6, dbeta 4.4e-8 (1e-3), 65 and 130 records
  head             embeddings 1.1e-5 (1e-4); the 16 parameter gradients and dx <= 1.3e-5 (1e-3)
  track loss       losses 9.4e-7, gradients 1.0e-5 (113 x 97, g_key) (3e-5); the zero rows against their own maxima 2.9e-7; the
                   split pair of twins: g_ref 2.0e-6, twin sums 3.5e-6
  RoIAlign         forward 2.5e-6, backward 1.2e-6 (3e-5), 260 and 1024 RoIs
  whole chain      losses 4.1e-6 (1e-4), parameter and level gradients <= 5.2e-5 (1e-3)
Reverted one at a time in scratch builds of the library, each of these made a test of this file fail: the `m < J.M` store guard of
`k_gemm32` (floats behind C written), the tail loop of `k_sum_splits` (dw of the 65-map case off by 0.14), the `idx <= cut` term of
`kept()` in `k_track_loss` (113 x 97: g_key off by 1.2e-3), the `r += blockDim.x` stride of the RoI descriptor loop (260 RoIs).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
import track_edge_cases as TC
from oracle import track_loss_oracle as LO
from polyphonicformer_amd import _lib, track_head as T, train as TR
from polyphonicformer_amd.registry import HEADS

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 4.0, 1e-6            # products: bound = max(FACTOR * e_ref, FLOOR)
NODE, OUT, GRAD = 3e-5, 1e-4, 1e-3


def _bound(e_ref):
    return max(FACTOR * e_ref, FLOOR)


def _check(rows, what):
    """rows: (name, device error, bound) -- print every figure, then assert them all"""
    bad = []
    for name, e, b in rows:
        print(f"  {what} {name:>24}: {e:.2e}  (bound {b:.2e})")
        if not e <= b:
            bad.append((name, e, b))
    assert not bad, (what, bad)


# =================================================================================================================================
# a. ph_gemm32 alone
# =================================================================================================================================
def _gemm(gpu, A, kcA, B, kcB, M, N, K, ksplit=1, bias=None, ldc=None):
    """one ph_gemm32 call into a NaN-filled C with a whole 64-row tile of spare floats behind it -> the [ksplit, M, N] results on
    the CPU; asserts that nothing but [M][N] of every split was written"""
    ldc = N if ldc is None else ldc
    pad = 64 * ldc + 64                      # where a store without its row or column guard would land
    buf = torch.full((ksplit * M * ldc + pad,), float("nan"), device=gpu)
    Ad, Bd = A.to(gpu).contiguous(), B.to(gpu).contiguous()
    bd = None if bias is None else bias.to(gpu)
    _lib.check(_lib.load().ph_gemm32(_lib.ptr(Ad), Ad.shape[1], kcA, _lib.ptr(Bd), Bd.shape[1], kcB, _lib.ptr(buf), ldc, M, N, K, ksplit,
                                     _lib.ptr(bd), _lib.stream_ptr()), "ph_gemm32")
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.isnan(got[ksplit * M * ldc:]).all(), "floats behind C were written"
    Cm = got[:ksplit * M * ldc].view(ksplit, M, ldc)
    assert torch.isnan(Cm[:, :, N:]).all(), "columns N .. ldc of C were written"
    assert torch.isfinite(Cm[:, :, :N]).all(), "an entry of [M][N] was not written"
    return Cm[:, :, :N]


@pytest.fixture(scope="module")
def gemm_operands():
    g = TC.gen(7001)
    return torch.randn(130, 12544, generator=g), torch.randn(1024, 12544, generator=g), torch.randn(1024, generator=g)


@pytest.mark.parametrize("split", ["one", "split"])
@pytest.mark.parametrize("K", [32, 392, 12544])
@pytest.mark.parametrize("M", [1, 64, 65, 130])
def test_gemm32_x_wT(gpu, gemm_operands, M, K, split):
    """kcA, kcB = 1, 1 (X W^T, the forward's layout): N in {19, 64, 1024}, bias on and off, ldc > N once; `split`: ksplit =
    `_ksplit(K, 16)`, the forward's choice, against one pass over K.

    One pass over K = 12544 at M = 64, 65, 130 is the case that found something: with ONE float32 accumulation chain over all of K
    the kernel measured 3.5e-6 .. 4.6e-6 against bounds of 1.3e-6 .. 3.0e-6 (as far off as a float32 loop in index order on the
    CPU, 3.7e-6 .. 3.9e-6), while 16 splits of the same operands were within 6.3e-7.  `k_gemm32` now adds every 128 k into a
    second accumulator; the figures since are in the module docstring."""
    X, W, bias = gemm_operands
    ksplit = 1 if split == "one" else T._ksplit(K, 16)
    assert (ksplit > 1) == (split == "split" and K > 32), "K = 32 is one step: `split` is one pass there as well"
    if K == 392:
        assert (K % 32, K // 32) == (8, 12)                           # the ragged last K step: 12 steps + 8
    rows = []
    for N in (19, 64, 1024):
        A, B = X[:M, :K].contiguous(), W[:N, :K].contiguous()
        ref = A.double() @ B.double().t()
        r32 = A @ B.t()
        for bz in (None, bias[:N]):
            for ldc in ((N, N + 5) if (N, K) == (19, 392) else (N,)):
                want = ref if bz is None else ref + bz.double()
                w32 = r32 if bz is None else r32 + bz
                got = _gemm(gpu, A, 1, B, 1, M, N, K, ksplit, bz, ldc)
                if bz is not None and ksplit > 1:          # the bias lands in split 0 only: the other splits are pure partial products
                    steps, per = (K + 31) // 32, ((K + 31) // 32 + ksplit - 1) // ksplit
                    assert per * (ksplit - 1) < steps, "an empty split"
                    k1 = per * 32
                    tail = A[:, k1:].double() @ B[:, k1:].double().t()
                    e_tail = Hh.rel_err(got[1:].double().sum(0), tail)
                    assert e_tail <= _bound(Hh.rel_err(A[:, k1:] @ B[:, k1:].t(), tail)), ("splits 1.. carry more than their products", e_tail)
                rows.append((f"N={N} bias={bz is not None} ldc={ldc}", Hh.rel_err(got.double().sum(0), want), _bound(Hh.rel_err(w32, want))))
    _check(rows, f"gemm32 (1,1) M={M} K={K} ksplit={ksplit}")


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_gemm32_backward_layouts(gpu, gemm_operands, n):
    """1, 0 (dY W: n x 1024 x 256) and 0, 0 with K = n (dY^T X: 256 x 392 and 1024 x 12544), the layouts of `_FcEmbed.backward`"""
    X, W, _ = gemm_operands
    rows = []
    dY, Wm = X[:n, :256].contiguous(), W[:256, :1024].contiguous()              # A [n][256] k-contiguous, B [256 (k)][1024]
    want = dY.double() @ Wm.double()
    rows.append(("(1,0) n x 1024 x 256", Hh.rel_err(_gemm(gpu, dY, 1, Wm, 0, n, 1024, 256)[0], want), _bound(Hh.rel_err(dY @ Wm, want))))
    for M, N in ((256, 392), (1024, 12544)):
        A, B = W[:n, :M].contiguous(), X[:n, :N].contiguous()                  # A [n (k)][M], B [n (k)][N]
        want = A.double().t() @ B.double()
        rows.append((f"(0,0) {M} x {N}, K={n}", Hh.rel_err(_gemm(gpu, A, 0, B, 0, M, N, n)[0], want), _bound(Hh.rel_err(A.t() @ B, want))))
    _check(rows, f"gemm32 backward layouts n={n}")


# =================================================================================================================================
# b. the _FcEmbed node
# =================================================================================================================================
@pytest.mark.parametrize("n", [1, 65, 130])
def test_fc_embed_node_every_entry(gpu, n):
    x, W1, b1, W2, b2, cot = TC.fc_fixture()
    r64 = TC.fc_reference(n)
    r32 = TC.fc_autograd(x[:n], W1, b1, W2, b2, cot[:n], torch.float32)
    with torch.enable_grad():
        t = [v.to(gpu).requires_grad_(True) for v in (x[:n], W1, b1, W2, b2)]
        out = T._FcEmbed.apply(*t)
        grads = torch.autograd.grad(out, t, cot[:n].to(gpu))
    torch.cuda.synchronize()
    got = dict(zip(("out", "gx", "gW1", "gb1", "gW2", "gb2"), (out.detach(),) + tuple(grads)))
    for k, v in got.items():
        assert v.shape == r64[k].shape and torch.isfinite(v).all(), k
    _check([(k, Hh.rel_err(v.cpu(), r64[k]), _bound(Hh.rel_err(r32[k], r64[k]))) for k, v in got.items()], f"_FcEmbed n={n}")


# =================================================================================================================================
# c. _Conv3x3 + _GNReLU on n maps of 7 x 7
# =================================================================================================================================
@pytest.mark.parametrize("n", [65, 130])
def test_conv_gn_on_many_small_maps(gpu, n):
    lib = _lib.load()
    # the weight gradient: nine map x map^T products whose nsplit * B per-image records k_sum_splits adds up (ph_conv3x3_wgrad)
    records = lib.ph_map_x_map_t_nsplit(n, 256, 49) * n
    assert records >= n and 49 % 4 != 0
    if n == 130:
        assert records >= 130 and (records != 130 or (130 // 8, 130 % 8) == (16, 2))
    x, w, gamma, beta, cot = TC.conv_gn_fixture(n)
    r64 = TC.conv_gn_reference(n)
    with torch.enable_grad():
        t = [v.to(gpu).requires_grad_(True) for v in (x, w, gamma, beta)]
        y = TR._GNReLU.apply(TR._Conv3x3.apply(t[0], t[1], 1), t[2], t[3], 32, None)
        grads = torch.autograd.grad(y, t, cot.to(gpu))
    torch.cuda.synchronize()
    got = dict(zip(("y", "dx", "dw", "dgamma", "dbeta"), (y.detach(),) + tuple(grads)))
    for k, v in got.items():
        assert v.shape == r64[k].shape and torch.isfinite(v).all(), k
    _check([(k, Hh.rel_err(v.cpu(), r64[k]), OUT if k == "y" else GRAD) for k, v in got.items()], f"conv + GroupNorm n={n} ({records} records)")


# =================================================================================================================================
# d. the whole head in training form
# =================================================================================================================================
def _head(gpu, sd):
    head = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32), loss_track=dict(T.LOSS_TRACK_DEFAULT),
                            loss_track_aux=dict(T.LOSS_TRACK_AUX_DEFAULT)))
    head.load_state_dict(sd)
    return head.to(gpu).train()


@pytest.mark.parametrize("n", [64, 65, 130])
def test_head_training_every_entry(gpu, n):
    sd, x, cot = TC.head_fixture()
    emb64, gw64, gx64 = TC.head_reference(n)
    head = _head(gpu, sd)
    xd = x[:n].to(gpu).requires_grad_(True)
    with torch.enable_grad():
        emb = head(xd)
        assert emb.requires_grad
        emb.backward(cot[:n].to(gpu))
    torch.cuda.synchronize()
    params = dict(head.named_parameters())
    assert len(params) == 16 and set(params) == set(gw64)
    rows = [("embeddings", Hh.rel_err(emb.detach().cpu(), emb64), OUT), ("dx", Hh.rel_err(xd.grad.cpu(), gx64), GRAD)]
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == gw64[k].shape and torch.isfinite(p.grad).all(), k
        rows.append((k, Hh.rel_err(p.grad.cpu(), gw64[k]), GRAD))
    _check(rows, f"head n={n}")


# =================================================================================================================================
# e. ph_track_loss
# =================================================================================================================================
def _i32(a):
    return (C.c_int32 * len(a))(*[int(v) for v in a])


def _track_loss(gpu, pairs, cfg):
    """one ph_track_loss call on a list of pairs -> (losses [2], g_key, g_ref) on the CPU"""
    lib = _lib.load()
    E = pairs[0]["key"].shape[1]
    c = _lib.TrackLossCfg(pairs=len(pairs), E=E, lw_track=cfg["lw_track"], lw_aux=cfg["lw_aux"], neg_pos_ub=int(cfg["neg_pos_ub"]),
                          pos_margin=cfg["pos_margin"], neg_margin=cfg["neg_margin"], hard_mining=1)
    start = lambda k: np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])])
    i32 = lambda k: torch.tensor([v for p in pairs for v in p[k]], dtype=torch.int32, device=gpu)
    key, ref = torch.cat([p["key"] for p in pairs]).to(gpu).contiguous(), torch.cat([p["ref"] for p in pairs]).to(gpu).contiguous()
    kg, rg, gm = i32("key_gt"), i32("ref_gt"), i32("gt_match")
    losses = torch.full((2,), -7.0, device=gpu)
    gk, gr = torch.full_like(key, float("nan")), torch.full_like(ref, float("nan"))
    scratch = torch.empty((max(lib.ph_track_loss_scratch_bytes(C.byref(c), key.shape[0], ref.shape[0]), 256),), dtype=torch.uint8, device=gpu)
    _lib.check(lib.ph_track_loss(C.byref(c), _lib.ptr(key), _lib.ptr(ref), _i32(start("key_gt")), _i32(start("ref_gt")), _lib.ptr(kg), _lib.ptr(rg),
                                 _i32(start("gt_match")), _lib.ptr(gm), _lib.ptr(losses), _lib.ptr(gk), _lib.ptr(gr), _lib.ptr(scratch),
                                 scratch.numel(), _lib.stream_ptr()), "ph_track_loss")
    torch.cuda.synchronize()
    return losses.cpu(), gk.cpu(), gr.cpu()


def _loss_rows(losses, want):
    """the losses: max |difference| over the larger reference value, and exact zeros where the reference is 0"""
    assert all(float(l) == 0.0 for l, r in zip(losses, want) if float(r) == 0.0), (losses, want)
    return float((losses.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", sorted(TC.LOSS_CASES))
def test_track_loss_edges_vs_oracle(gpu, name):
    p, cfg, (l64, gk64, gr64) = TC.loss_case(name)
    losses, gk, gr = _track_loss(gpu, [p], cfg)
    assert torch.isfinite(losses).all() and torch.isfinite(gk).all() and torch.isfinite(gr).all()
    print(f"  {name}: losses {losses.tolist()} reference {l64.tolist()}")
    rows = [("losses", _loss_rows(losses, l64), NODE)]
    if name == "zero-rows":             # the matched zero rows carry 1 / eps: every row against its own maximum
        assert float(gk64.abs().max()) > 1e8
        rows += [("g_key rows", TC.row_err(gk, gk64), NODE), ("g_ref rows", TC.row_err(gr, gr64), NODE)]
    else:
        rows += [("g_key", Hh.rel_err(gk, gk64), NODE), ("g_ref", Hh.rel_err(gr, gr64), NODE)]
    if name == "split-tie":
        # g_ref above: every row under the oracle's tie rule.  The twins' sum, which no tie rule changes, as well; and the cut does
        # tell the twins apart.  (Against each row's OWN maximum -- row_err, not asserted -- the worst row measured 3.4e-5: a copy's
        # row has negatives only, its gradient is the softmax weight exp(d - max), and d is near 80 here, where one float32 step
        # of d is 7.6e-6.)
        h = p["twins"]
        rows += [("g_ref twin sums", Hh.rel_err(gr[:h] + gr[h:], gr64[:h] + gr64[h:]), NODE)]
        print(f"  track loss split-tie: g_ref against every row's own maximum {TC.row_err(gr, gr64):.2e}")
        assert not torch.equal(gr64[:h], gr64[h:]), "the cut does not tell the twins apart"
    _check(rows, f"track loss {name}")


def test_track_loss_three_edge_pairs_in_one_launch(gpu):
    """three of the pairs in one launch: against the oracle, and the single calls' rows times float(1 / 3) bit for bit"""
    cases = [TC.loss_case(n) for n in TC.JOINT]
    pairs = [c[0] for c in cases]
    losses, gk, gr = _track_loss(gpu, pairs, LO.SHIPPED)
    l64 = sum(c[2][0] for c in cases) / 3
    rows = [("losses", _loss_rows(losses, l64), NODE)]
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    ks, rs = np.cumsum([0] + [len(p["key_gt"]) for p in pairs]), np.cumsum([0] + [len(p["ref_gt"]) for p in pairs])
    singles = []
    for i, (n, c) in enumerate(zip(TC.JOINT, cases)):
        s = _track_loss(gpu, [c[0]], LO.SHIPPED)
        singles.append(s)
        assert torch.equal(gk[ks[i]:ks[i + 1]], s[1] * third) and torch.equal(gr[rs[i]:rs[i + 1]], s[2] * third), n
        rows += [(f"g_key {n}", Hh.rel_err(gk[ks[i]:ks[i + 1]] * 3, c[2][1]), NODE), (f"g_ref {n}", Hh.rel_err(gr[rs[i]:rs[i + 1]] * 3, c[2][2]), NODE)]
    # the losses leave the device as fp32 roundings of fp64 sums: the joint values are the mean of the single calls' to one rounding each
    assert Hh.rel_err(losses, sum(s[0].double() for s in singles) / 3) < 2e-7
    _check(rows, "track loss, three pairs")


# =================================================================================================================================
# f. RoIAlign forward and backward
# =================================================================================================================================
def _roi_fwd(gpu, feats, rois):
    return T.roi_extract([f.to(gpu) for f in feats], rois.to(gpu), _lib.PH_PREC_BF16, TC.STRIDES, float(TC.FINEST), want_f32=True)[1]


def _roi_bwd(gpu, g_roi, rois):
    outs = [torch.full((1, 256, h, w), float("nan"), device=gpu) for h, w in TC.LEVELS]
    ptrs = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
    hw = (C.c_int32 * 8)(*[v for s in TC.LEVELS for v in s])
    sc = (C.c_float * 4)(*[1.0 / s for s in TC.STRIDES])
    g, r = g_roi.to(gpu).contiguous(), rois.to(gpu).contiguous()
    _lib.check(_lib.load().ph_roi_align_fpn_bwd(_lib.ptr(g), hw, sc, 4, _lib.ptr(r), r.shape[0], float(TC.FINEST), ptrs, _lib.stream_ptr()),
               "ph_roi_align_fpn_bwd")
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("n", [260, 1024])
def test_roi_align_pair_past_256_rois(gpu, n):
    feats, rois, bad, cot, out64, grads64 = TC.roi_reference(n)
    assert rois.shape[0] == n and n > 256 and n <= 1024 and torch.isnan(rois[bad]).any()
    ok = torch.ones(n, dtype=torch.bool)
    ok[bad] = False
    out = _roi_fwd(gpu, feats, rois)
    torch.cuda.synchronize()
    assert out.shape == out64.shape and torch.isfinite(out[ok.to(gpu)]).all()
    rows = [("forward", Hh.rel_err(out.cpu()[ok], out64[ok]), NODE)]
    assert torch.equal(_roi_fwd(gpu, feats, rois)[ok.to(gpu)], out[ok.to(gpu)]), "a second forward differs"
    got = _roi_bwd(gpu, cot, rois)
    for l, (a, b) in enumerate(zip(got, grads64)):
        assert torch.isfinite(a).all(), ("the NaN box reached level", l)
        rows.append((f"backward level {l}", Hh.rel_err(a, b), NODE))
    poisoned = cot.clone()
    poisoned[bad] = float("nan")                     # the NaN box's cotangent is never read
    again = _roi_bwd(gpu, poisoned, rois)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "a second backward differs (or the NaN box's cotangent was read)"
    _check(rows, f"RoIAlign n={n}")


# =================================================================================================================================
# g. track_forward_train, two pairs
# =================================================================================================================================
def test_track_forward_train_every_entry(gpu):
    c = TC.chain_fixture()
    l64, gw64, gl64, _, _ = TC.chain_reference()
    head = _head(gpu, c["sd"])
    dev = lambda lv, grad: [f.to(gpu).requires_grad_(grad) for f in lv]
    feats, ref_feats = [dev(lv, True) for lv in c["feats"]], [dev(lv, True) for lv in c["ref_feats"]]
    with torch.enable_grad():
        losses = TR.track_forward_train(head, feats, ref_feats, [r.to(gpu) for r in c["rois"]], [r.to(gpu) for r in c["ref_rois"]],
                                        c["key_gt"], c["ref_gt"], c["gt_match"])
        assert set(losses) == {"loss_track", "loss_track_aux"}
        TR.parse_losses(losses).backward()
    torch.cuda.synchronize()
    got = torch.stack([losses["loss_track"].detach(), losses["loss_track_aux"].detach()]).cpu()
    print("  chain losses", got.tolist(), "reference", l64.tolist())
    rows = [("losses", _loss_rows(got, l64), OUT)]
    params = dict(head.named_parameters())
    assert len(params) == 16 and set(params) == set(gw64)
    for k, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        rows.append((k, Hh.rel_err(p.grad.cpu(), gw64[k]), GRAD))
    for i in range(2):
        for l in range(4):
            f = feats[i][l]
            assert f.grad is not None and f.grad.shape == f.shape and torch.isfinite(f.grad).all()
            rows.append((f"key level {l} of pair {i}", Hh.rel_err(f.grad.cpu(), gl64[i][l]), GRAD))
    assert all(f.grad is None for lv in ref_feats for f in lv)
    _check(rows, "track_forward_train")
