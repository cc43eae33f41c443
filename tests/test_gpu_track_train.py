"""GPU: training the track head.  `ph_track_loss` (targets, MultiPos + L2 losses with hard mining, gradients) against the reference's
own classes in fp64 (tests/golden/track_train.npz, tools/gen_golden_track_train.py); `ph_roi_align_fpn_bwd` against autograd of the
oracle's RoI extraction; the differentiable head against the reference's autograd; `track_forward_train` end to end.

Bounds: 3e-5 (max-normalised) for one fp32 node against fp64 -- the figure test_gpu_neck_train.py::test_conv3x3_node_vs_torch uses;
1e-4 on losses and 1e-3 on gradients through the conv + GroupNorm stack -- those of test_neck_training_vs_reference."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

import helpers as Hh
from oracle import video_oracle as VO
from polyphonicformer_amd import _lib, track_head as T, train as TR
from polyphonicformer_amd.registry import HEADS

pytestmark = pytest.mark.gpu

SHIPPED = dict(lw_track=0.25, lw_aux=1.0, neg_pos_ub=3, pos_margin=0.0, neg_margin=0.1, hard_mining=1)


def _fixture():
    z = Hh.load_golden("track_train.npz")
    return z, json.loads(bytes(z["meta_json"]).decode())


def _i32(a):
    return (C.c_int32 * len(a))(*[int(v) for v in a])


def _case(z, names):
    """the stored arrays of one case, or of several single-pair cases joined into one call"""
    cat = lambda k: np.concatenate([z[f"{n}.{k}"] for n in names])
    start = lambda k: np.concatenate([[0], np.cumsum(np.concatenate([np.diff(z[f"{n}.{k}"]) for n in names]))])
    return dict(key=cat("key"), ref=cat("ref"), key_gt=cat("key_gt"), ref_gt=cat("ref_gt"), gt_match=cat("gt_match"),
                key_start=start("key_start"), ref_start=start("ref_start"), match_start=start("match_start"))


def _run(gpu, c, grads=True, E=256, expect=0, **over):
    """one ph_track_loss call on the arrays of `c` -> (rc, losses [2], g_key, g_ref) as CPU tensors"""
    lib = _lib.load()
    pairs = len(c["key_start"]) - 1
    cfg = _lib.TrackLossCfg(pairs=pairs, E=E, **{**SHIPPED, **over})
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(gpu, dt)
    key, ref = dev(c["key"], torch.float32), dev(c["ref"], torch.float32)
    kg, rg, gm = dev(c["key_gt"], torch.int32), dev(c["ref_gt"], torch.int32), dev(c["gt_match"], torch.int32)
    losses = torch.full((2,), -7.0, device=gpu)
    gk, gr = (torch.full_like(key, -7.0), torch.full_like(ref, -7.0)) if grads else (None, None)
    scratch = torch.empty((max(lib.ph_track_loss_scratch_bytes(C.byref(cfg), key.shape[0], ref.shape[0]), 256),), dtype=torch.uint8, device=gpu)
    rc = lib.ph_track_loss(C.byref(cfg), _lib.ptr(key), _lib.ptr(ref), _i32(c["key_start"]), _i32(c["ref_start"]), _lib.ptr(kg), _lib.ptr(rg),
                           _i32(c["match_start"]), _lib.ptr(gm), _lib.ptr(losses), _lib.ptr(gk), _lib.ptr(gr), _lib.ptr(scratch), scratch.numel(),
                           _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (rc == 0) == (expect == 0), (rc, Hh.last_error())
    return rc, losses.cpu(), None if gk is None else gk.cpu(), None if gr is None else gr.cpu()


@pytest.mark.parametrize("name", ["a0", "a1", "a2", "e_one", "e_nomine", "e_twopos", "e_unmatched"])
def test_track_loss_vs_reference(gpu, name):
    z, _ = _fixture()
    _, losses, gk, gr = _run(gpu, _case(z, [name]))
    ref_l = torch.from_numpy(z[f"{name}.losses"])
    errs = (Hh.rel_err(losses, ref_l), Hh.rel_err(gk, z[f"{name}.g_key"]), Hh.rel_err(gr, z[f"{name}.g_ref"]))
    print(name, "losses", losses.tolist(), "ref", ref_l.tolist(), "rel err (losses, g_key, g_ref)", errs)
    assert (losses - ref_l).abs().max() <= 3e-5 * ref_l.abs().max(), (losses, ref_l)
    assert all(float(l) == 0.0 for l, r in zip(losses, ref_l) if float(r) == 0.0)
    assert max(errs[1:]) < 3e-5, errs
    # the loss values alone (no gradient buffers) are the same bits
    _, l2, _, _ = _run(gpu, _case(z, [name]), grads=False)
    assert torch.equal(l2, losses)


def test_three_pairs_in_one_launch(gpu):
    """pairs = 3 against the reference, and against the three single-pair calls bit for bit: a pair's numbers do not depend on its
    neighbours, and the mean over the pairs is one fp32 multiplication of the finished rows by float(1 / pairs)"""
    z, _ = _fixture()
    names = ["a0", "a1", "a2"]
    c = _case(z, names)
    _, losses, gk, gr = _run(gpu, c)
    ref_l = torch.from_numpy(z["a_all.losses"])
    print("a_all losses", losses.tolist(), "ref", ref_l.tolist())
    assert Hh.rel_err(losses, ref_l) < 3e-5
    ks, rs = c["key_start"], c["ref_start"]
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    singles = [_run(gpu, _case(z, [n])) for n in names]
    for p, (n, s) in enumerate(zip(names, singles)):
        assert Hh.rel_err(gk[ks[p]:ks[p + 1]] * 3, z[f"{n}.g_key"]) < 3e-5 and Hh.rel_err(gr[rs[p]:rs[p + 1]] * 3, z[f"{n}.g_ref"]) < 3e-5
        assert torch.equal(gk[ks[p]:ks[p + 1]], s[2] * third) and torch.equal(gr[rs[p]:rs[p + 1]], s[3] * third), n
    # the losses leave the device as fp32 roundings of fp64 sums: the joint values are the mean of the single calls' to one rounding each
    assert Hh.rel_err(losses, sum(s[1].double() for s in singles) / 3) < 2e-7


def test_second_call_is_bit_identical(gpu):
    z, _ = _fixture()
    for names in (["a0", "a1", "a2"], ["e_twopos"], ["e_pair_nan"]):
        a, b = _run(gpu, _case(z, names)), _run(gpu, _case(z, names))
        for x, y in zip(a[1:], b[1:]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), names


def test_nan_pair(gpu):
    z, _ = _fixture()
    _, losses, gk, gr = _run(gpu, _case(z, ["e_nan"]))
    assert torch.isnan(losses).all() and torch.isnan(gk).all() and torch.isnan(gr).all()
    assert np.array_equal(np.isnan(losses.numpy()), np.isnan(z["e_nan.losses"]))
    c = _case(z, ["e_pair_nan"])
    _, losses, gk, gr = _run(gpu, c)
    for got, want in ((losses, z["e_pair_nan.losses"]), (gk, z["e_pair_nan.g_key"]), (gr, z["e_pair_nan.g_ref"])):
        assert np.array_equal(np.isnan(got.numpy()), np.isnan(want))
    k1, r1 = c["key_start"][1], c["ref_start"][1]
    errs = Hh.rel_err(gk[:k1], z["e_pair_nan.g_key"][:k1]), Hh.rel_err(gr[:r1], z["e_pair_nan.g_ref"][:r1])
    print("finite pair beside the NaN pair: rel err", errs)
    assert max(errs) < 3e-5
    assert torch.allclose(gk, torch.from_numpy(z["e_pair_nan.g_key"]), rtol=0, atol=3e-5 * float(np.nanmax(np.abs(z["e_pair_nan.g_key"]))), equal_nan=True)


def test_argument_errors_launch_nothing(gpu):
    g = torch.Generator().manual_seed(5)

    def case(nk, nr):
        return dict(key=torch.randn(max(nk, 1), 256, generator=g).numpy(), ref=torch.randn(max(nr, 1), 256, generator=g).numpy(),
                    key_gt=np.zeros(max(nk, 1), np.int32), ref_gt=np.zeros(max(nr, 1), np.int32), gt_match=np.zeros(1, np.int32),
                    key_start=[0, nk], ref_start=[0, nr], match_start=[0, 1])

    for c, over, what in ((case(129, 4), {}, "129"), (case(4, 129), {}, "129"), (case(0, 3), {}, "empty"), (case(3, 0), {}, "empty"),
                          (case(5, 7), dict(hard_mining=0), "hard_mining")):
        rc, losses, gk, gr = _run(gpu, c, expect=_lib.PH_EUNSUPPORTED, **over)
        assert rc == -1, (what, rc)                                         # PH_EINVAL
        assert Hh.last_error().startswith("ph_track_loss"), Hh.last_error()
        assert (losses == -7).all() and (gk == -7).all() and (gr == -7).all(), what       # nothing ran
    # neg_pos_ub <= 0 never mines: accepted without hard_mining
    rc, losses, _, _ = _run(gpu, case(5, 7), hard_mining=0, neg_pos_ub=-1)
    assert rc == 0 and torch.isfinite(losses).all()
    # 128 on either side is inside the bound
    rc, losses, gk, gr = _run(gpu, case(128, 128))
    assert rc == 0 and torch.isfinite(gk).all() and torch.isfinite(gr).all()


# ---- RoIAlign backward -----------------------------------------------------------------------------------------------------------
ROIS = torch.tensor([[0, 10.0, 8.0, 50.0, 40.0],          # level 0
                     [0, 30.0, 20.0, 90.0, 60.0],         # level 0, overlapping the first
                     [0, 0.0, 0.0, 128.0, 120.0],         # level 1
                     [0, -40.0, -30.0, 200.0, 250.0],     # level 2
                     [0, -200.0, -200.0, 300.0, 320.0],   # level 3
                     [0, 100.0, 40.0, 150.0, 90.0],       # level 0, past the right and the lower edge of the 64 x 128 image
                     [0, 64.0, 10.0, 64.0, 50.0]])        # zero width -> level 0
LEVELS = [(16, 32), (8, 16), (4, 8), (2, 4)]


def _roi_bwd(gpu, g_roi, rois):
    outs = [torch.full((1, 256, h, w), float("nan"), device=gpu) for h, w in LEVELS]
    ptrs = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
    hw = (C.c_int32 * 8)(*[v for s in LEVELS for v in s])
    sc = (C.c_float * 4)(*[1.0 / s for s in (4, 8, 16, 32)])
    g, r = g_roi.to(gpu).contiguous(), rois.to(gpu).contiguous()
    _lib.check(_lib.load().ph_roi_align_fpn_bwd(_lib.ptr(g), hw, sc, 4, _lib.ptr(r), r.shape[0], 56.0, ptrs, _lib.stream_ptr()), "ph_roi_align_fpn_bwd")
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.fixture(scope="module")
def roi_reference():
    g = torch.Generator().manual_seed(11)
    feats = [torch.randn(1, 256, h, w, generator=g).requires_grad_(True) for h, w in LEVELS]
    cot = torch.randn(len(ROIS), 256, 7, 7, generator=g)
    assert VO.map_roi_levels(ROIS).tolist() == [0, 0, 1, 2, 3, 0, 0]
    with torch.enable_grad():
        out = VO.roi_extract(feats, ROIS)
        grads = torch.autograd.grad((out * cot).sum(), feats)
    return [f.detach() for f in feats], cot, out.detach(), [t.detach() for t in grads]


def test_roi_align_bwd_vs_oracle_autograd(gpu, roi_reference):
    feats, cot, out, grads = roi_reference
    got = _roi_bwd(gpu, cot, ROIS)
    for l, (a, b) in enumerate(zip(got, grads)):
        e = Hh.rel_err(a, b)
        print("level", l, "rel err", e, "max |grad|", float(b.abs().max()))
        assert torch.isfinite(a).all() and e < 3e-5, (l, e)
    again = _roi_bwd(gpu, cot, ROIS)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # only level-0 RoIs: the other levels are written as zeros (they held NaN)
    sub = _roi_bwd(gpu, cot[:2], ROIS[:2])
    assert all((t == 0).all() for t in sub[1:]) and torch.isfinite(sub[0]).all() and sub[0].abs().max() > 0


def test_roi_extract_node(gpu, roi_reference):
    feats, cot, out, grads = roi_reference
    fd = [f.to(gpu).requires_grad_(True) for f in feats]
    with torch.enable_grad():
        x = TR._RoIExtract.apply(ROIS.to(gpu), (4, 8, 16, 32), 56, *fd)
        (x * cot.to(gpu)).sum().backward()
    assert Hh.rel_err(x.detach().cpu(), out) < 1e-4
    assert all(Hh.rel_err(f.grad.cpu(), b) < 3e-5 for f, b in zip(fd, grads))


# ---- the differentiable head ----------------------------------------------------------------------------------------------------
def _sr(inds):
    return types.SimpleNamespace(pos_assigned_gt_inds=torch.as_tensor(inds))


def _digest(t, n=256):
    f = t.detach().double().reshape(-1).cpu()
    idx = torch.linspace(0, f.numel() - 1, n).long()
    return np.concatenate([[float(f.norm()), float(f.sum())], f[idx].numpy()])


def _seeded_head(meta, gpu):
    head = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32),
                            loss_track=meta["loss_track"], loss_track_aux=meta["loss_track_aux"]))
    shapes = {k: tuple(v) for k, v in meta["head"]["shapes"].items()}
    assert shapes == {k: tuple(v.shape) for k, v in head.state_dict().items()}
    head.load_state_dict(Hh.seeded_fill(shapes, meta["head"]["weight_seed"]))
    return head.to(gpu)


def test_head_training_vs_reference(gpu):
    z, meta = _fixture()
    hm = meta["head"]
    head = _seeded_head(meta, gpu).train()
    g = torch.Generator().manual_seed(hm["feat_seed"])
    xk = torch.randn(3, 256, 7, 7, generator=g).to(gpu).requires_grad_(True)
    xr = torch.randn(4, 256, 7, 7, generator=g).to(gpu)
    with torch.enable_grad():
        ke, re_ = head(xk), head(xr)
        assert ke.requires_grad and Hh.rel_err(ke.detach().cpu(), z["head.key_embeds"]) < 1e-4 and Hh.rel_err(re_.detach().cpu(), z["head.ref_embeds"]) < 1e-4
        losses = head.track_loss(ke, re_, [torch.tensor(hm["gt_match"])], [_sr(hm["key_gt"])], [_sr(hm["ref_gt"])])
        assert set(losses) == {"loss_track", "loss_track_aux"}
        TR.parse_losses(losses).backward()
    got = torch.stack([losses["loss_track"].detach(), losses["loss_track_aux"].detach()]).cpu()
    e_loss = Hh.rel_err(got, z["head.losses"])
    print("head losses", got.tolist(), "ref", z["head.losses"].tolist(), "rel err", e_loss)
    assert e_loss < 1e-4
    params = dict(head.named_parameters())
    assert list(params) == hm["params"]
    worst = 0.0
    for n, p in params.items():
        assert p.grad is not None, n
        ref = z[f"head.grad.{n}"]
        d = _digest(p.grad)
        e_norm = abs(d[0] - ref[0]) / max(ref[0], 1e-30)
        e_ent = float(np.abs(d[2:] - ref[2:]).max() / max(np.abs(ref[2:]).max(), 1e-30))
        print(n, "norm err", e_norm, "entry err", e_ent)
        worst = max(worst, e_norm, e_ent)
    e_x = Hh.rel_err(xk.grad.cpu(), z["head.g_key_feats"])
    print("d / d key RoI features: rel err", e_x)
    assert worst < 1e-3 and e_x < 1e-3


def test_inference_path_is_untouched(gpu):
    """eval mode, or training mode under no_grad: `forward` is `forward_planes` of the same input, bit for bit"""
    _, meta = _fixture()
    head = _seeded_head(meta, gpu)
    x = torch.randn(5, 256, 7, 7, generator=torch.Generator().manual_seed(3)).to(gpu)
    xc = x.permute(0, 2, 3, 1).reshape(5, 49, 256)
    hi = xc.to(torch.bfloat16)
    planes = torch.stack([hi.view(torch.int16), (xc - hi.float()).to(torch.bfloat16).view(torch.int16)], 0).contiguous()
    with torch.no_grad():
        want = head.eval().forward_planes(planes)
        assert torch.equal(head(x), want)
        assert torch.equal(head.train()(x), want)
    with torch.enable_grad():
        assert torch.equal(head.eval()(x), want) and not head(x).requires_grad
        assert head.train()(x).requires_grad


def test_track_forward_train_end_to_end(gpu):
    _, meta = _fixture()
    head = _seeded_head(meta, gpu).train()
    g = torch.Generator().manual_seed(21)
    mk = lambda: [torch.randn(1, 256, h, w, generator=g).to(gpu).requires_grad_(True) for h, w in LEVELS]
    feats, ref_feats = [mk(), mk()], [mk(), mk()]
    rois = [ROIS[[0, 2, 3]].to(gpu), ROIS[[1, 4, 5]].to(gpu)]
    ref_rois = [ROIS[[0, 1, 2, 3]].to(gpu), ROIS[[2, 3, 4, 5]].to(gpu)]
    with torch.enable_grad():                 # other test modules switch grad off for the process
        losses = TR.track_forward_train(head, feats, ref_feats, rois, ref_rois, [[0, 1, 2], [2, 0, 1]], [[0, 1, 2, 1], [0, 1, 2, 3]],
                                        [[1, -1, 0], [3, 0, -1]])
        vals = {k: float(v.detach()) for k, v in losses.items()}
        print(vals)
        assert set(vals) == {"loss_track", "loss_track_aux"} and all(np.isfinite(v) and v > 0 for v in vals.values())
        TR.parse_losses(losses).backward()
    for n, p in head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    assert len(list(head.parameters())) == 16
    for lv in feats:
        for f in lv:
            assert f.grad is not None and f.grad.shape == f.shape and torch.isfinite(f.grad).all()
        assert sum(float(f.grad.abs().sum()) for f in lv) > 0
    assert all(f.grad is None for lv in ref_feats for f in lv)
