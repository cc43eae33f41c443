"""GPU: the video training step.  `ph_gtmask_boxes` (the RoIs of the sampled ground-truth masks, csrc/ph_gtbox.hip) against the
reference's own lines and against exact arithmetic (tests/golden/video_train.npz, tools/gen_golden_video_train.py), `track_sample`
against the reference's assigner + sampler, `VideoTrainStep` against its parts.

Bounds.  RoIs against the reference: 1e-4 -- the reference takes its means in fp32 and lies `ref_gap` (about 1e-5) from exact
arithmetic; the test asserts ref_gap * 4 <= 1e-4 from the fixture, so the bound cannot hide an error of the kernel's own.  Against the
fixture's exact boxes: one fp32 ulp of the coordinate (means and deviations are fp64, rounded once).  Full width: 2.5e-4, one fp32 ulp
at 2048."""
import ctypes as C
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
from polyphonicformer_amd import _lib, assigner as A, losses as Lo, track_head as T, train as TR

sys.path.insert(0, os.path.join(Hh.REPO, "tools"))
import gen_golden_video_train as GV  # noqa: E402  (torch only at import; the reference is read by its main() alone)

pytestmark = pytest.mark.gpu

FILL = 0xFF


def _fixture():
    z = Hh.load_golden("video_train.npz")
    return z, json.loads(bytes(z["meta_json"]).decode())


def _i32(a):
    return (C.c_int32 * len(a))(*[int(v) for v in a])


def _call(gpu, frames, Np, hw, HW, mode=0, ws_bytes=None, n_override=None):
    """one raw ph_gtmask_boxes call.  frames: [(masks [G, h, w] tensor, match [G] int array)]; workspace and outputs are pre-filled
    with 0xFF bytes.  -> (rc, rois, pos_gt, count as CPU tensors over the concatenated rows, n per frame)"""
    lib = _lib.load()
    (h, w), (H, W) = hw, HW
    masks = [m.to(gpu).float().contiguous() for m, _ in frames]
    G = [int(m.shape[0]) for m in masks]
    n = [min(g, Np) for g in G] if n_override is None else list(n_override)
    ld = max(G + [1])
    mt = torch.full((len(frames), ld), -1, dtype=torch.int32)
    for b, (_, r) in enumerate(frames):
        mt[b, :G[b]] = torch.as_tensor(np.asarray(r), dtype=torch.int32)
    mt = mt.to(gpu)
    total = sum(n)
    rows = max(total, 1)
    rois = torch.full((rows, 5), 0, dtype=torch.float32, device=gpu).view(torch.uint8).fill_(FILL).view(torch.float32)
    pos_gt = torch.zeros(rows, dtype=torch.int32, device=gpu).view(torch.uint8).fill_(FILL).view(torch.int32)
    count = torch.zeros(rows, dtype=torch.int64, device=gpu).view(torch.uint8).fill_(FILL).view(torch.int64)
    need = lib.ph_gtmask_boxes_workspace_bytes(len(frames), _i32(G), max(H, 1), max(W, 1))
    ws = torch.full((max(need if ws_bytes is None else ws_bytes, 16),), FILL, dtype=torch.uint8, device=gpu)
    start = np.concatenate([[0], np.cumsum(n)])[:-1]
    ptrs = (C.c_void_p * len(frames))(*[m.data_ptr() if m.shape[0] else None for m in masks])
    rc = lib.ph_gtmask_boxes(ptrs, _i32(G), _i32(n), _i32(start), _lib.ptr(mt), ld, Np, len(frames), h, w, H, W, mode, _lib.ptr(rois),
                             _lib.ptr(pos_gt), _lib.ptr(count), _lib.ptr(ws), need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, rois.cpu(), pos_gt.cpu(), count.cpu(), n


def _untouched(*ts):
    return all(bool((t.contiguous().view(torch.uint8) == FILL).all()) for t in ts)


# ---- 1. boxes against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", ["identity", "perm", "few"])
@pytest.mark.parametrize("name", ["s4", "s4b", "frac", "one"])
def test_boxes_vs_reference(gpu, name, sel):
    z, meta = _fixture()
    assert meta["ref_gap"] * 4 <= 1e-4, meta["ref_gap"]
    h, w, H, W = meta["shapes"][name]
    masks = torch.from_numpy(z[f"a.{name}.masks"])
    match, Np = z[f"a.{name}.{sel}.match"], int(z[f"a.{name}.{sel}.Np"])
    rc, rois, pos_gt, count, n = _call(gpu, [(masks, match)], Np, (h, w), (H, W))
    assert rc == 0, Hh.last_error()
    want_pg = z[f"a.{name}.{sel}.pos_gt"]
    assert n[0] == len(want_pg) and np.array_equal(pos_gt.numpy(), want_pg)
    assert np.array_equal(count.numpy(), z[f"a.{name}.count"][want_pg])
    ref = torch.from_numpy(z[f"a.{name}.{sel}.ref_rois"])
    exact = z[f"a.{name}.exact"][want_pg]
    e_ref = float((rois - ref).abs().max())
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    e_ulp = float((np.abs(rois[:, 1:].numpy().astype(np.float64) - exact) / ulp).max())
    print(name, sel, "max |roi - reference|", e_ref, "max |roi - exact| in fp32 ulps", e_ulp)
    assert (rois[:, 0] == 0).all() and e_ref <= 1e-4
    assert e_ulp <= 1.0
    empty = count == 0
    assert (empty.any() or sel == "few") and (rois[empty] == 0).all()        # the empty mask: (0, 0, 0, 0)
    assert (rois[:, 1:] >= 0).all()                                          # the clamp at 0


# ---- 2. full width against torch on the device ------------------------------------------------------------------------------------
def test_full_width_vs_torch_on_device(gpu):
    h, w, H, W = 256, 512, 1024, 2048
    yy, xx = torch.meshgrid(torch.arange(H, device=gpu).float(), torch.arange(W, device=gpu).float(), indexing="ij")
    big = ((((yy - 500.0) / 420.0) ** 2 + ((xx - 900.0) / 800.0) ** 2) <= 1.0).float()
    low = F.interpolate(big[None, None], size=(h, w), mode="bilinear", align_corners=False)[0]
    few = torch.zeros(1, h, w, device=gpu)
    few[0, h - 1, w - 2:] = 1.0
    few[0, h - 2, w - 1] = 1.0
    masks = torch.cat([low, few]).contiguous()
    rc, rois, pos_gt, count, _ = _call(gpu, [(masks, [1, 0])], 4, (h, w), (H, W))
    assert rc == 0, Hh.last_error()
    hard = F.interpolate(masks[None], size=(H, W), mode="bilinear", align_corners=False)[0].sigmoid() > 0.5
    want = []
    for i in (1, 0):                                   # ascending prediction row: ground truth 1 first
        m = hard[i]
        r, c = m.sum(1).double(), m.sum(0).double()
        nn_ = r.sum()
        Y, X = torch.arange(H, device=gpu).double(), torch.arange(W, device=gpu).double()
        my, mx = (Y * r).sum() / nn_, (X * c).sum() / nn_
        dy, dx = ((r * (Y - my).abs()).sum() / nn_).clamp(min=1.0), ((c * (X - mx).abs()).sum() / nn_).clamp(min=1.0)
        want.append((int(nn_), torch.stack([mx - 2 * dx, my - 2 * dy, mx + 2 * dx, my + 2 * dy]).clamp(min=0).cpu()))
    print("full width: counts", count.tolist(), "want", [c_ for c_, _ in want], "rois", rois.tolist())
    assert pos_gt.tolist() == [1, 0]
    assert count.tolist() == [c_ for c_, _ in want] and count[0] < 200 < count[1]
    err = max(float((rois[i, 1:].double() - want[i][1]).abs().max()) for i in range(2))
    print("full width: max |roi - fp64 formula|", err)
    assert err <= 2.5e-4


# ---- 3. several frames in one call ----------------------------------------------------------------------------------------------------
def test_frames_in_one_call_equal_single_calls(gpu):
    z, meta = _fixture()
    h, w, H, W = meta["shapes"]["s4"]
    masks = torch.from_numpy(z["a.s4.masks"])
    G = masks.shape[0]
    Np = 7
    g = torch.Generator().manual_seed(4)
    f0 = (masks[:5], torch.randperm(Np, generator=g)[:5].numpy())                          # G = 5 = n
    m1 = np.full(G, -1, np.int64)
    m1[torch.randperm(G, generator=g)[:Np].numpy()] = torch.randperm(Np, generator=g).numpy()
    f1 = (masks, m1)                                                                       # G > Np: n = 7
    f2 = (masks[:0], np.zeros(0, np.int64))                                                # no ground truth: n = 0
    rc, rois, pos_gt, count, n = _call(gpu, [f0, f1, f2], Np, (h, w), (H, W))
    assert rc == 0 and n == [5, 7, 0], (rc, n, Hh.last_error())
    o = 0
    for f, nf in zip((f0, f1), n):
        rc1, r1, p1, c1, _ = _call(gpu, [f], Np, (h, w), (H, W))
        assert rc1 == 0
        assert torch.equal(rois[o:o + nf].view(torch.int32), r1.view(torch.int32)) and torch.equal(pos_gt[o:o + nf], p1) and torch.equal(count[o:o + nf], c1)
        o += nf
    # the binding: per-frame views of one allocation, the same numbers
    br, bp, bc = T.gt_mask_rois([f[0].to(gpu).contiguous() for f in (f0, f1, f2)],
                                [torch.as_tensor(np.asarray(f[1]), dtype=torch.int32).to(gpu) for f in (f0, f1, f2)], n, (H, W), num_proposals=Np)
    assert [t.shape[0] for t in br] == n and br[0].untyped_storage().data_ptr() == bc[1].untyped_storage().data_ptr()
    assert torch.equal(torch.cat(br).cpu(), rois) and torch.equal(torch.cat(bp).cpu(), pos_gt) and torch.equal(torch.cat(bc).cpu(), count)


# ---- 4. no zeroing contract, determinism, capture -------------------------------------------------------------------------------------
def test_second_call_and_graph_replay(gpu):
    z, meta = _fixture()
    h, w, H, W = meta["shapes"]["s4b"]
    masks = torch.from_numpy(z["a.s4b.masks"])
    match, Np = z["a.s4b.perm.match"], int(z["a.s4b.perm.Np"])
    a = _call(gpu, [(masks, match)], Np, (h, w), (H, W))            # buffers pre-filled with 0xFF
    b = _call(gpu, [(masks, match)], Np, (h, w), (H, W))
    assert a[0] == 0 and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a[1:4], b[1:4]))
    assert torch.isfinite(a[1]).all()
    # capture on one stream; a replay after the masks changed in place gives the new boxes
    lib = _lib.load()
    G = masks.shape[0]
    md = masks.to(gpu).contiguous()
    mt = torch.as_tensor(match, dtype=torch.int32).to(gpu)
    n = min(G, Np)
    rois = torch.empty((n, 5), dtype=torch.float32, device=gpu)
    pos_gt = torch.empty((n,), dtype=torch.int32, device=gpu)
    count = torch.empty((n,), dtype=torch.int64, device=gpu)
    need = lib.ph_gtmask_boxes_workspace_bytes(1, _i32([G]), H, W)
    ws = torch.empty((need,), dtype=torch.uint8, device=gpu)
    ptrs = (C.c_void_p * 1)(md.data_ptr())

    def launch():
        _lib.check(lib.ph_gtmask_boxes(ptrs, _i32([G]), _i32([n]), _i32([0]), _lib.ptr(mt), G, Np, 1, h, w, H, W, 0, _lib.ptr(rois), _lib.ptr(pos_gt),
                                       _lib.ptr(count), _lib.ptr(ws), need, _lib.stream_ptr()), "ph_gtmask_boxes")

    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        launch()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rois.cpu(), a[1]) and torch.equal(count.cpu(), a[3])
    flipped = torch.flip(masks, dims=(1, 2)).contiguous()
    md.copy_(flipped.to(gpu))
    graph.replay()
    torch.cuda.synchronize()
    want = _call(gpu, [(flipped, match)], Np, (h, w), (H, W))
    assert torch.equal(rois.cpu(), want[1]) and torch.equal(pos_gt.cpu(), want[2]) and torch.equal(count.cpu(), want[3])
    assert not torch.equal(want[1], a[1])


# ---- 5. argument errors launch nothing ------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(gpu):
    small = torch.ones(130, 4, 4)
    ident = lambda G: np.arange(G)
    ok_need = _lib.load().ph_gtmask_boxes_workspace_bytes(1, _i32([6]), 16, 16)
    cases = [("n > 128", dict(frames=[(small, ident(130))], Np=129, hw=(4, 4), HW=(8, 8)), _lib.PH_EINVAL),
             ("n != min(G, Np)", dict(frames=[(small[:6], ident(6))], Np=4, hw=(4, 4), HW=(16, 16), n_override=[6]), _lib.PH_EINVAL),
             ("short workspace", dict(frames=[(small[:6], ident(6))], Np=8, hw=(4, 4), HW=(16, 16), ws_bytes=ok_need - 256), _lib.PH_EWORKSPACE),
             ("H < h", dict(frames=[(small[:6], ident(6))], Np=8, hw=(4, 4), HW=(3, 16)), _lib.PH_EUNSUPPORTED),
             ("nearest", dict(frames=[(small[:6], ident(6))], Np=8, hw=(4, 4), HW=(16, 16), mode=_lib.PH_GTBOX_NEAREST), _lib.PH_EUNSUPPORTED)]
    for what, kw, code in cases:
        rc, rois, pos_gt, count, _ = _call(gpu, **kw)
        assert rc == code, (what, rc, Hh.last_error())
        assert Hh.last_error().startswith("ph_gtmask_boxes"), Hh.last_error()
        assert _untouched(rois, pos_gt, count), what
    rc, rois, _, count, _ = _call(gpu, frames=[(small[:6], ident(6))], Np=8, hw=(4, 4), HW=(16, 16))        # the same call without the fault
    assert rc == 0 and (count == 256).all() and torch.isfinite(rois).all()
    rc, rois, _, count, _ = _call(gpu, frames=[(small[:128], ident(128))], Np=128, hw=(4, 4), HW=(8, 8))    # 128 is inside the bound
    assert rc == 0 and (count == 64).all()


# ---- 6. track_sample -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_assign", [False, True])
@pytest.mark.parametrize("tag", ["g5", "g10"])
def test_track_sample_vs_reference_sampler(gpu, tag, device_assign):
    z, meta = _fixture()
    m = meta["sampling"][tag]
    assert m["margin"] >= 1e-2
    pred, cls, gt, labels = GV.sample_inputs(m["seed"], m["G"], m["Np"], m["nt"], m["h"], m["w"])
    sgt = Lo.StepGT([gt.to(gpu)], [labels.to(gpu)], None, None, None, False)
    assigner = A.build_assigner(dict(type="MaskHungarianAssigner", **copy.deepcopy(meta["track_assigner"])))
    match = TR.track_sample(assigner, pred[None].to(gpu), cls[None].to(gpu), sgt, m["Np"], m["nt"], device_assign=device_assign)
    assert match.dtype == torch.int32 and match.shape == (1, m["G"])
    if device_assign:
        assert len(sgt.status_words) == 1 and int(sgt.status_words[0][0]) == 0
    rows = match[0].cpu()
    assert sorted(rows[rows >= 0].tolist()) == z[f"b.{tag}.pos_inds"].tolist()
    n = min(m["G"], m["Np"])
    rois, pos_gt, count = T.gt_mask_rois(sgt.masks, match, [n], (4 * m["h"], 4 * m["w"]), num_proposals=m["Np"])
    print(tag, "device" if device_assign else "host", "match", rows.tolist(), "pos_gt", pos_gt[0].tolist())
    assert pos_gt[0].cpu().tolist() == z[f"b.{tag}.pos_gt"].tolist()
    hard = F.interpolate(sgt.masks[0][None], size=(4 * m["h"], 4 * m["w"]), mode="bilinear", align_corners=False)[0].sigmoid() > 0.5
    assert torch.equal(count[0].cpu(), hard.sum((1, 2)).cpu()[pos_gt[0].cpu().long()])      # RoI r is ground truth pos_gt[r]


# ---- 7. video_track_branch against the reference chain ---------------------------------------------------------------------------------
def _digest(t, n):
    f = t.detach().double().reshape(-1).cpu()
    idx = torch.linspace(0, f.numel() - 1, n).long()
    return np.concatenate([[float(f.norm()), float(f.sum())], f[idx].numpy()])


def _digest_err(d, ref):
    return max(abs(d[0] - ref[0]) / max(ref[0], 1e-30), float(np.abs(d[2:] - ref[2:]).max() / max(np.abs(ref[2:]).max(), 1e-30)))


@pytest.mark.parametrize("device_assign", [False, True])
def test_video_track_branch_vs_reference_chain(gpu, device_assign):
    """polyphonic_former_video.py:245-319 assembled from the reference's pieces in fp64 (fixture c).  Bounds: those of
    tests/test_gpu_track_train.py for the same quantities -- losses 3e-5 (max-normalised), gradients 1e-3.

    The fixture is decided: no GroupNorm output of the reference chain lies within 2e-5 of zero (the training products carry hi + lo
    bf16 operands, a product is good to 2^-16 = 1.5e-5 of its size).  A ReLU inside that band is decided either way, and one such
    unit moves its RoI's gradients by 1e-3 .. 3e-2 (measured on a 19-RoI fixture that did not keep the margin: convs.0-2 and their
    GroupNorms 1.4e-3 .. 1.7e-2 off, every layer above the flipped units and the losses at 2e-5): a coin, not arithmetic."""
    from polyphonicformer_amd.registry import HEADS
    z, meta = _fixture()
    c = meta["branch"]
    assert c["relu_margin"] >= c["relu_margin_min"] == 2e-5
    inp = GV.branch_inputs(c["seeds"])
    head = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32), loss_track=c["loss_track"],
                            loss_track_aux=c["loss_track_aux"]))
    head.load_state_dict(Hh.seeded_fill({k: tuple(v) for k, v in c["shapes"].items()}, c["weight_seed"]))
    head.to(gpu).train()
    x = [f.to(gpu).requires_grad_(True) for f in Hh.fpn_inputs(c["feat_seed"], c["B"], 256, c["H0"], c["W0"])]
    x_ref = [f.to(gpu).requires_grad_(True) for f in Hh.fpn_inputs(c["ref_feat_seed"], c["B"], 256, c["H0"], c["W0"])]
    last, gts = {}, {}
    for side in ("key", "ref"):
        pred = torch.stack([t[0] for t in inp[side]]).to(gpu)
        cls = torch.stack([t[1] for t in inp[side]]).to(gpu)
        last[side] = (None, cls, None, pred)
        gts[side] = Lo.StepGT([t[2].to(gpu) for t in inp[side]], [t[3].to(gpu) for t in inp[side]], None, None, None, False)
    assigner = A.build_assigner(dict(type="MaskHungarianAssigner", **copy.deepcopy(meta["track_assigner"])))
    ids = [torch.tensor(v).to(gpu) for v in c["gt_ids"]]
    rids = [torch.tensor(v).to(gpu) for v in c["ref_ids"]]
    assert torch.cat([TR.gt_match_indices(a, b) for a, b in zip(ids, rids)]).cpu().tolist() == z["c.gt_match"].tolist()
    for side in ("key", "ref"):                                  # the boxes and their order are the reference chain's
        mt = TR.track_sample(assigner, last[side][3], last[side][1], gts[side], c["Np"], c["nt"], device_assign=device_assign)
        rois, pos_gt, _ = T.gt_mask_rois(gts[side].masks, mt, [min(g_, c["Np"]) for g_ in gts[side].G], (4 * c["H0"], 4 * c["W0"]), num_proposals=c["Np"])
        assert torch.cat(pos_gt).cpu().tolist() == z[f"c.{side}_pos_gt"].tolist(), side
        assert float((torch.cat(rois).cpu()[:, 1:] - torch.from_numpy(z[f"c.{side}_rois"])[:, 1:]).abs().max()) <= 1e-4, side
    with torch.enable_grad():
        losses = TR.video_track_branch(head, assigner, x, x_ref, last["key"], last["ref"], gts["key"], gts["ref"], ids, rids,
                                       (4 * c["H0"], 4 * c["W0"]), c["Np"], c["nt"], device_assign=device_assign)
        TR.parse_losses(losses).backward()
    got = torch.stack([losses["loss_track"].detach(), losses["loss_track_aux"].detach()]).cpu().double()
    ref = torch.from_numpy(z["c.losses"])
    e_loss = float((got - ref).abs().max() / ref.abs().max())
    print("branch losses", got.tolist(), "ref", ref.tolist(), "err", e_loss)
    assert e_loss <= 3e-5
    params = dict(head.named_parameters())
    assert list(params) == c["params"]
    errs = {n: _digest_err(_digest(p.grad, 256), z[f"c.grad.{n}"]) for n, p in params.items()}
    for n, e in errs.items():
        print(n, "gradient err", e, "norm", float(params[n].grad.norm()), "ref norm", z[f"c.grad.{n}"][0])
    e_p = max(errs.values())
    e_x = max(_digest_err(_digest(f.grad, 4096), z[f"c.gx{l}"]) for l, f in enumerate(x) if np.abs(z[f"c.gx{l}"]).max() > 0)
    print("parameter gradients err", e_p, "level gradients err", e_x)
    assert e_p <= 1e-3 and e_x <= 1e-3
    for l, f in enumerate(x):
        if np.abs(z[f"c.gx{l}"]).max() == 0:
            assert f.grad is not None and (f.grad == 0).all(), l                    # a level no RoI maps to is written as zeros
    assert all(f.grad is None for f in x_ref)


# ---- 8. VideoTrainStep is the sum of its parts ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def video_parts(gpu):
    from polyphonicformer_amd.registry import HEADS, NECKS
    import polyphonicformer_amd.kernel_update  # noqa: F401
    import polyphonicformer_amd.semantic_fpn  # noqa: F401
    from test_gpu_device_assign import NT, NS, ROI_ASSIGNER
    from test_gpu_loss import _rpn_head
    rpn, sd = _rpn_head(gpu)
    roi = HEADS.build(dict(type="KernelUpdateIterHead", num_stages=3, assign_stages=3, stage_loss_weights=[1] * 3, num_proposals=100,
                           num_thing_classes=NT, num_stuff_classes=NS, do_panoptic=True, merge_joint=True,
                           mask_head=Hh.stage_cfg(256, 2048, 8, NT + NS, NT, NS),
                           train_cfg=dict(assigner=copy.deepcopy(ROI_ASSIGNER), sampler=dict(type='MaskPseudoSampler'), pos_weight=1.)))
    roi.load_state_dict({k[len("roi_head."):]: v for k, v in sd.items() if k.startswith("roi_head.")})
    roi.to(gpu)
    neck = NECKS.build(dict(type="SemanticFPNWrapper", in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
                            upsample_times=2, positional_encoding=dict(type="SinePositionalEncoding", num_feats=128, normalize=True),
                            cat_coors=False, cat_coors_level=3, fuse_by_cat=False, return_list=False, num_aux_convs=2,
                            norm_cfg=dict(type="GN", num_groups=32, requires_grad=True)))
    with open(Hh.GOLDEN + "/neck_state_keys.json") as f:
        shapes = json.load(f)["full"]
    neck.load_state_dict(Hh.seeded_fill({k: tuple(v) for k, v in shapes.items()}, 5))
    neck.to(gpu).train()
    tmeta = json.loads(bytes(Hh.load_golden("track_train.npz")["meta_json"]).decode())
    th = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32), loss_track=tmeta["loss_track"],
                          loss_track_aux=tmeta["loss_track_aux"]))
    th.load_state_dict(Hh.seeded_fill({k: tuple(v) for k, v in tmeta["head"]["shapes"].items()}, tmeta["head"]["weight_seed"]))
    th.to(gpu).train()
    B, H0, W0 = 2, 16, 32                                                     # 64 x 128 padded; the assign resolution is 16 x 32
    x = [f.to(gpu) for f in Hh.fpn_inputs(seed=31, B=B, C=256, H0=H0, W0=W0)]
    x_ref = [f.to(gpu) for f in Hh.fpn_inputs(seed=32, B=B, C=256, H0=H0, W0=W0)]
    gts = [{k: v.to(gpu) for k, v in g.items()} for g in Hh.train_gt(78, B, H0, W0, NT, NS, [4, 6])]
    rgts = [{k: v.to(gpu) for k, v in g.items()} for g in Hh.train_gt(79, B, H0, W0, NT, NS, [5, 4])]
    gd = torch.stack([g["depth"][None] for g in gts])
    ids = [torch.tensor([10, 11, 12, 13]).to(gpu), torch.tensor([20, 21, 22, 23, 24, 25]).to(gpu)]
    rids = [torch.tensor([12, 10, 99, 11, 50]).to(gpu), torch.tensor([25, 20, 21, 77]).to(gpu)]       # keys 13, 22, 23, 24 have no partner
    metas = [Hh.img_meta(4 * H0, 4 * W0)] * B
    img = (metas, [g["masks"] for g in gts], [g["labels"] for g in gts], [g["sem_seg"] for g in gts], [g["sem_cls"] for g in gts], gd)
    vid = (ids, [g["masks"] for g in rgts], [g["labels"] for g in rgts], rids, (4 * H0, 4 * W0))
    tcfg = dict(assigner=dict(type="MaskHungarianAssigner", **copy.deepcopy(GV.TRACK_ASSIGNER)), sampler=dict(type="MaskPseudoSampler"))
    return neck, rpn, roi, th, tcfg, x, x_ref, img, vid


def _all_params(*mods):
    return [p for m in mods for p in m.parameters()]


def _image_step(rpn, roi, feats, img):
    for p in _all_params(rpn, roi):
        p.grad = None
    with TR.TrainStep(rpn, roi) as step:
        losses, total, gf = step.forward_backward(feats, *img)
    return losses, total, gf, [None if p.grad is None else p.grad.clone() for p in _all_params(rpn, roi)]


def test_video_train_step_is_the_sum_of_its_parts(gpu, video_parts):
    neck, rpn, roi, th, tcfg, x, x_ref, img, vid = video_parts
    mods = (neck, rpn, roi, th)
    with torch.enable_grad():
        feats = [f.detach() for f in TR.neck_forward_train(neck, x)]
    before = _image_step(rpn, roi, feats, img)
    assert len(before[0]) == 24
    flags = [m.training for top in mods for m in top.modules()]
    for p in _all_params(*mods):
        p.grad = None
    with TR.VideoTrainStep(neck, rpn, roi, th, tcfg) as step:
        losses, total, gx = step.forward_backward(x, x_ref, *img, *vid)
        assert step.assign_status().numel() == 0
        assert [m.training for top in mods for m in top.modules()] == flags
        assert set(losses) == set(before[0]) | {"loss_track", "loss_track_aux"}
        for k, v in before[0].items():
            assert torch.equal(losses[k], v), (k, float(losses[k]), float(v))
        for top in mods:
            for nme, p in top.named_parameters():
                if nme.startswith("localization_fpn."):
                    continue
                assert p.grad is not None and torch.isfinite(p.grad).all(), nme
        assert len(gx) == 4 and all(g is not None and g.shape == f.shape and torch.isfinite(g).all() for g, f in zip(gx, x))
        print({k: float(v) for k, v in losses.items() if "track" in k}, "objective", float(total))
        assert all(np.isfinite(float(losses[k])) and float(losses[k]) > 0 for k in ("loss_track", "loss_track_aux"))

        # the parts by hand: the same functions on leaves of our own
        xl = [f.detach().float().contiguous().requires_grad_(True) for f in x]
        xr = [f.detach().float().contiguous().requires_grad_(True) for f in x_ref]
        with torch.enable_grad():
            f2 = TR.neck_forward_train(neck, xl)
            l24, last, cache = TR._heads_forward_train(rpn, roi, f2, *img, False)
            ref_last = step._reference_frame(xr, img[0])
            gt = TR._step_gt(cache, False, *img[1:])
            ref_gt = Lo.StepGT(vid[1], vid[2], None, None, None, False)
            lt = TR.video_track_branch(th, step.track_assigner, xl, xr, last, ref_last, gt, ref_gt, vid[0], vid[3], vid[4], roi.num_proposals,
                                       roi.num_thing_classes)
            for k in ("loss_track", "loss_track_aux"):
                assert torch.equal(lt[k].detach(), losses[k]), k
            g_neck = torch.autograd.grad(TR.parse_losses(l24), xl, retain_graph=True)
            g_roi = torch.autograd.grad(TR.parse_losses(lt), xl, allow_unused=True)
        for lvl in range(4):
            want = g_neck[lvl] if g_roi[lvl] is None else g_neck[lvl] + g_roi[lvl]
            assert torch.equal(gx[lvl], want), lvl
        assert sum(float(g.abs().sum()) for g in g_roi if g is not None) > 0
        assert all(f.grad is None for f in xr)

    # device_assign: the same losses bit for bit, nothing solved on the host
    with TR.VideoTrainStep(neck, rpn, roi, th, tcfg, device_assign=True) as dstep:
        dl, dt, dgx = dstep.forward_backward(x, x_ref, *img, *vid, backward=False)
        st = dstep.assign_status()
    assert st.shape == (6, 2) and (st == 0).all(), st
    assert torch.equal(dt, total) and all(torch.equal(dl[k], losses[k]) for k in losses)
    after = _image_step(rpn, roi, feats, img)
    assert torch.equal(before[1], after[1]) and all(torch.equal(before[0][k], after[0][k]) for k in before[0])
    assert all(torch.equal(a, b) for a, b in zip(before[2], after[2]))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(before[3], after[3]))
