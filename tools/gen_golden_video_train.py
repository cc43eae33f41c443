"""Fixtures for the video training step (tests/golden/video_train.npz), produced by the reference's own code on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_video_train.py

(a) box cases: low-resolution ground-truth masks made the way PolyphonicVideo.forward_train makes them (binary full-resolution blobs,
    bilinear down), a selection (`match`: the prediction row of every ground truth or -1), the reference's RoIs from
    polyphonic_former_video.py:283-291 + 413-415 verbatim (F.interpolate, sigmoid > 0.5, batch_mask2boxlist, bboxlist2roi, clamp), the
    on-pixel counts, and the same boxes in exact arithmetic (integer row / column histograms, fp64).  `ref_gap` is the largest
    |reference - exact| (the reference takes its means in fp32).  `box_cases()` needs torch only: tests/test_video_train_host.py runs
    it and compares the integer arrays with the committed file.
(b) sampling cases: the reference's MaskHungarianAssigner (FocalLossCost 2, DiceCost 4, MaskCost 1) + MaskPseudoSampler, Np = 8 against
    G = 5 and G = 10, 16 x 32; predictions are noisy copies of the ground truth and the seed is searched until every single change of
    the matching costs at least 1e-2 more.
(c) one whole track branch (:245-319) from the reference's pieces in fp64: assigner, sampler, interpolate, batch_mask2boxlist,
    bboxlist2roi, the oracle's RoIAlign, the head, match, get_track_targets, loss; losses, the 16 parameter gradients and the key-level
    gradients.  The FPN feature seed is searched until every ReLU of the head is decided (RELU_MARGIN below)."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = {"s4": (16, 32, 64, 128), "s4b": (12, 20, 48, 80), "frac": (10, 14, 25, 49), "one": (24, 40, 24, 40)}
BOX_SEED = 301
SWAP_MARGIN = 1e-2
TRACK_ASSIGNER = dict(cls_cost=dict(type="FocalLossCost", weight=2.0), dice_cost=dict(type="DiceCost", weight=4.0, pred_act=True),
                      mask_cost=dict(type="MaskCost", weight=1.0, pred_act=True))


def _blob(g, H, W, cy, cx, ry, rx):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).float()


def low_res_masks(name):
    """the ground-truth masks of one shape at the assign resolution [G, h, w] fp32 >= 0"""
    h, w, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(BOX_SEED + len(name))
    full = []
    full.append(_blob(g, H, W, H - 1 - H / 5, W - 1 - W / 6, H / 4, W / 5))                    # touches the right and the bottom edge
    full.append(torch.ones(H, W))                                                              # full
    far = torch.zeros(H, W)                                                                    # most of its mass in the first columns / rows, a
    far[:max(H // 8, 2), :max(W // 10, 2)] = 1                                                 # far piece: x1 and y1 would be negative
    far[H - max(H // 16, 1):, W - max(W // 20, 1):] = 1
    full.append(far)
    for _ in range(3):                                                                         # blobs somewhere inside
        cy, cx = (float(torch.rand((), generator=g)) * 0.6 + 0.2) * H, (float(torch.rand((), generator=g)) * 0.6 + 0.2) * W
        full.append(_blob(g, H, W, cy, cx, H * (0.06 + 0.15 * float(torch.rand((), generator=g))), W * (0.05 + 0.15 * float(torch.rand((), generator=g)))))
    full = torch.stack(full)
    low = F.interpolate(full[None], size=(h, w), mode="bilinear", align_corners=False)[0]      # the dataset pipeline's own step
    extra = [torch.zeros(h, w)]                                                                # empty
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):                              # one low-resolution pixel per corner
        m = torch.zeros(h, w)
        m[y, x] = 1.0
        extra.append(m)
    if (h, w) == (H, W):                                                                       # ratio 1: the max(., 1) clamp
        m = torch.zeros(h, w); m[h // 2, w // 3] = 1.0; extra.append(m)                        # a single pixel inside
        m = torch.zeros(h, w); m[3:h - 2, w // 2] = 1.0; extra.append(m)                       # one pixel wide
        m = torch.zeros(h, w); m[h // 3, 5:w - 7] = 1.0; extra.append(m)                       # one pixel high
    return torch.cat([torch.stack(extra), low]).contiguous()


def selections(name, G):
    """name -> (match int32 [G], Np): identity, a permutation (rows not monotone in g), G > n with -1 entries"""
    g = torch.Generator().manual_seed(BOX_SEED + 7 * len(name))
    perm_rows = torch.randperm(G + 9, generator=g)[:G]
    few = torch.full((G,), -1, dtype=torch.long)
    chosen = torch.randperm(G, generator=g)[:5]
    few[chosen] = torch.randperm(5, generator=g)
    return {"identity": (torch.arange(G), G + 3), "perm": (perm_rows, G + 9), "few": (few, 5)}


def upsampled_hard(low, H, W):
    up = F.interpolate(low[None], size=(H, W), mode="bilinear", align_corners=False)[0]        # :285-290
    pos = up[up > 0]
    assert pos.numel() == 0 or float(pos.min()) >= 2.0 ** -20, "input contract: no upsampled value in (0, 2^-20)"
    return (up.sigmoid() > 0.5).float()                                                        # :291


def exact_boxes(hard):
    """[n, H, W] 0 / 1 -> (count int64 [n], boxes fp64 [n, 4] (x1, y1, x2, y2) clamped at 0): integer histograms, fp64 means"""
    n = hard.shape[0]
    cnt, out = np.zeros(n, np.int64), np.zeros((n, 4), np.float64)
    for i in range(n):
        m = hard[i].numpy().astype(np.int64)
        r, c = m.sum(1), m.sum(0)
        cnt[i] = r.sum()
        if cnt[i] == 0:
            continue
        Y, X = np.arange(m.shape[0], dtype=np.float64), np.arange(m.shape[1], dtype=np.float64)
        my, mx = (Y * r).sum() / cnt[i], (X * c).sum() / cnt[i]
        dy, dx = max((r * np.abs(Y - my)).sum() / cnt[i], 1.0), max((c * np.abs(X - mx)).sum() / cnt[i], 1.0)
        out[i] = np.maximum([mx - 2 * dx, my - 2 * dy, mx + 2 * dx, my + 2 * dy], 0.0)
    return cnt, out


def box_cases(utils=None):
    """the arrays of part (a); `utils`: the reference's polyphonic/video/utils.py module, or None: everything but `ref_rois`"""
    out = {}
    for name, (h, w, H, W) in SHAPES.items():
        low = low_res_masks(name)
        G = low.shape[0]
        hard = upsampled_hard(low, H, W)
        cnt, ex = exact_boxes(hard)
        out[f"a.{name}.masks"] = low.numpy()
        out[f"a.{name}.count"], out[f"a.{name}.exact"] = cnt, ex
        for sel, (match, Np) in selections(name, G).items():
            order = sorted((int(r), g) for g, r in enumerate(match.tolist()) if r >= 0)        # pos_inds ascending (sampler.py:93-113)
            pos_gt = np.array([g for _, g in order], np.int32)
            assert len(pos_gt) == min(G, Np)
            out[f"a.{name}.{sel}.match"], out[f"a.{name}.{sel}.pos_gt"] = match.numpy().astype(np.int32), pos_gt
            out[f"a.{name}.{sel}.Np"] = np.array(Np, np.int32)
            if utils is not None:
                key_masks = upsampled_hard(low[torch.from_numpy(pos_gt).long()], H, W)         # res.pos_gt_masks -> :283-291
                rois = utils.bboxlist2roi(utils.batch_mask2boxlist([key_masks])).clamp(min=0.0)   # :413-415
                out[f"a.{name}.{sel}.ref_rois"] = rois.numpy().astype(np.float32)
    return out


def load_utils():
    from oracle import ref_loader
    spec = importlib.util.spec_from_file_location("_ref_video_utils", os.path.join(ref_loader.REF_ROOT, "polyphonic/video/utils.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def sample_inputs(seed, G, Np=8, nt=8, h=16, w=32):
    g = torch.Generator().manual_seed(seed)
    full = torch.stack([_blob(g, 4 * h, 4 * w, (0.15 + 0.7 * float(torch.rand((), generator=g))) * 4 * h, (0.1 + 0.8 * float(torch.rand((), generator=g))) * 4 * w,
                              4 * h * (0.08 + 0.1 * float(torch.rand((), generator=g))), 4 * w * (0.06 + 0.1 * float(torch.rand((), generator=g)))) for _ in range(G)])
    gt = F.interpolate(full[None], size=(h, w), mode="bilinear", align_corners=False)[0].contiguous()
    labels = torch.randint(0, nt, (G,), generator=g)
    rows = torch.randperm(max(Np, G), generator=g)
    pred = torch.randn(Np, h, w, generator=g) - 2.0
    for j in range(G):                                        # row rows[j] is a noisy copy of ground truth j (where that row exists)
        if rows[j] < Np:
            pred[rows[j]] = (gt[j] - 0.5) * 8 + 0.5 * torch.randn(h, w, generator=g)
    cls = torch.randn(Np, nt, generator=g)
    return pred.contiguous(), cls.contiguous(), gt, labels


def swap_margin(cost, rows_of_gt):
    """smallest increase of the total cost over all single changes of a matching: two ground truths exchanging rows, a matched one
    moving to a free row, an unmatched one taking a matched one's row.  cost [Np, G] fp64"""
    Np, G = cost.shape
    base = sum(cost[r, g] for g, r in enumerate(rows_of_gt) if r >= 0)
    free = set(range(Np)) - {r for r in rows_of_gt if r >= 0}
    best = float("inf")
    for g1, r1 in enumerate(rows_of_gt):
        for g2, r2 in enumerate(rows_of_gt):
            if g1 < g2 and r1 >= 0 and r2 >= 0:
                best = min(best, cost[r2, g1] + cost[r1, g2] - cost[r1, g1] - cost[r2, g2])
            if r1 >= 0 and r2 < 0:
                best = min(best, cost[r1, g2] - cost[r1, g1])
        if r1 >= 0:
            for r in free:
                best = min(best, cost[r, g1] - cost[r1, g1])
    return float(best), float(base)


def sampling_cases(ns, sampler):
    out, meta = {}, {}
    a = ns.AssignerNoDepth(**TRACK_ASSIGNER)
    for tag, G in (("g5", 5), ("g10", 10)):
        for seed in range(500, 900):
            pred, cls, gt, labels = sample_inputs(seed, G)
            r = a.assign(pred, cls, gt, labels, img_meta=None)
            sr = sampler.sample(r, pred, gt)
            cost = (a.cls_cost(cls, labels) + a.mask_cost(pred, gt) + a.dice_cost(pred, gt)).double().numpy()
            rows_of_gt = [-1] * G
            for p, gidx in zip(sr.pos_inds.tolist(), sr.pos_assigned_gt_inds.tolist()):
                rows_of_gt[gidx] = p
            margin, _ = swap_margin(cost, rows_of_gt)
            if margin >= SWAP_MARGIN:
                break
        else:
            raise RuntimeError(f"no seed gives a decided matching for {tag}")
        print("sampling", tag, "seed", seed, "margin", margin, "pos_inds", sr.pos_inds.tolist(), "gt", sr.pos_assigned_gt_inds.tolist())
        out[f"b.{tag}.pos_inds"] = sr.pos_inds.numpy().astype(np.int32)
        out[f"b.{tag}.pos_gt"] = sr.pos_assigned_gt_inds.numpy().astype(np.int32)
        out[f"b.{tag}.cost"] = cost.astype(np.float32)
        meta[tag] = dict(seed=seed, G=G, Np=8, nt=8, h=16, w=32, margin=margin)
    return out, meta


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
BRANCH = dict(B=2, H0=16, W0=32, Np=8, nt=8, key_G=[3, 2], ref_G=[2, 1], gt_ids=[[10, 11, 12], [20, 21]], ref_ids=[[12, 10], [21]])
# A ReLU whose pre-activation lies within the rounding of the training products of zero is decided either way, and one such unit moves
# a RoI's gradients by about 1 / sqrt(2304) of their size: the comparison would measure a coin, not arithmetic.  The products carry
# hi + lo bf16 operands, |x - hi - lo| <= 2^-17 |x|, so a product is good to 2^-16 = 1.5e-5 of its size; the FPN feature seeds are
# searched until no GroupNorm output of the reference chain lies closer to zero than that (as the mined pairs keep a gap at the cut).
RELU_MARGIN = 2e-5


def branch_inputs(seeds):
    """per frame set ('key', 'ref') and image: (pred [Np, h, w], cls [Np, nt], gt [G, h, w], labels [G]) from `sample_inputs`"""
    c = BRANCH
    return {side: [sample_inputs(seeds[side][i], G, c["Np"], c["nt"], c["H0"], c["W0"]) for i, G in enumerate(c[f"{side}_G"])]
            for side in ("key", "ref")}


def digest(t, n):
    f = t.detach().double().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, n).long()
    return np.concatenate([[float(f.norm()), float(f.sum())], f[idx].numpy()])


def branch_case(ns, sampler, utils):
    import helpers
    import gen_golden_track_train as GT
    from oracle import video_oracle as VO
    c = BRANCH
    a = ns.AssignerNoDepth(**TRACK_ASSIGNER)
    H, W = 4 * c["H0"], 4 * c["W0"]
    # seeds with a decided matching for every image of both frames
    seeds = {"key": [], "ref": []}
    for side in ("key", "ref"):
        for i, G in enumerate(c[f"{side}_G"]):
            for seed in range(600 + 100 * i + (50 if side == "ref" else 0), 1000):
                pred, cls, gt, labels = sample_inputs(seed, G, c["Np"], c["nt"], c["H0"], c["W0"])
                r = a.assign(pred, cls, gt, labels, img_meta=None)
                sr = sampler.sample(r, pred, gt)
                rows = [-1] * G
                for p_, g_ in zip(sr.pos_inds.tolist(), sr.pos_assigned_gt_inds.tolist()):
                    rows[g_] = p_
                cost = (a.cls_cost(cls, labels) + a.mask_cost(pred, gt) + a.dice_cost(pred, gt)).double().numpy()
                if swap_margin(cost, rows)[0] >= SWAP_MARGIN:
                    break
            else:
                raise RuntimeError("no decided matching")
            seeds[side].append(seed)
    inp = branch_inputs(seeds)
    srs, rois = {}, {}
    for side in ("key", "ref"):
        srs[side] = []
        for pred, cls, gt, labels in inp[side]:
            r = a.assign(pred, cls, gt, labels, img_meta=None)                                 # :256-260
            srs[side].append(sampler.sample(r, pred, gt))                                      # :261-265
        masks = [upsampled_hard(res.pos_gt_masks, H, W) for res in srs[side]]                  # :283-291
        rois[side] = utils.bboxlist2roi(utils.batch_mask2boxlist(masks)).clamp(min=0.0)        # :413-415
    gmi = []
    for i in range(c["B"]):                                                                    # :246-251
        ref_ids, gt_ids = c["ref_ids"][i], c["gt_ids"][i]
        gmi.append(torch.LongTensor([[ref_ids.index(j) if j in ref_ids else -1 for j in gt_ids]])[0])
    head = GT.build_head().double()
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    head.load_state_dict({k: v.double() for k, v in helpers.seeded_fill(shapes, GT.HEAD_SEED).items()})
    head.train()
    torch.set_default_dtype(torch.float64)                                                     # the oracle's RoIAlign allocates in the default
    try:
        def feats_of(levels, r):
            out = []
            for i in range(c["B"]):                                                            # SingleRoIExtractor, image by image
                ri = r[r[:, 0] == i].double().clone()
                ri[:, 0] = 0
                out.append(VO.roi_extract([lv[i:i + 1] for lv in levels], ri))
            return torch.cat(out)

        def relu_margin(t):
            """the smallest |GroupNorm output| over the head's four conv layers (track_heads.py:92-95) for the RoI features t"""
            sd, worst = head.state_dict(), float("inf")
            for i in range(4):
                t = F.group_norm(F.conv2d(t, sd[f"convs.{i}.conv.weight"], padding=1), 32, sd[f"convs.{i}.gn.weight"], sd[f"convs.{i}.gn.bias"], 1e-5)
                worst = min(worst, float(t.abs().min()))
                t = F.relu(t)
            return worst

        for feat_seed in range(41, 20000):
            torch.set_default_dtype(torch.float32)                                             # the fp32 draws the test repeats
            x = [f.double() for f in helpers.fpn_inputs(feat_seed, c["B"], 256, c["H0"], c["W0"])]
            x_ref = [f.double() for f in helpers.fpn_inputs(feat_seed + 5000, c["B"], 256, c["H0"], c["W0"])]
            torch.set_default_dtype(torch.float64)
            assert all(torch.equal(f, f.float().double()) for f in x + x_ref)
            with torch.no_grad():
                margin = relu_margin(torch.cat([feats_of(x, rois["key"]), feats_of(x_ref, rois["ref"])]))
            if margin >= RELU_MARGIN:
                break
        else:
            raise RuntimeError("no feature seed keeps every ReLU decided")
        print("feature seed", feat_seed, "smallest |pre-activation|", margin)
        for f in x:
            f.requires_grad_(True)
        key_feats = head(feats_of(x, rois["key"]))                                             # :293, 416-417
        with torch.no_grad():
            ref_in = feats_of(x_ref, rois["ref"])
        ref_feats = head(ref_in)                                                               # :305
        match_feats = head.match(key_feats, ref_feats, srs["key"], srs["ref"])                 # :307-312
        targets = head.get_track_targets(gmi, srs["key"], srs["ref"])                          # :314-318
        losses = head.loss(*match_feats, *targets)                                             # :319
        (losses["loss_track"] + losses["loss_track_aux"]).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    out = {"c.losses": np.array([float(losses["loss_track"].detach()), float(losses["loss_track_aux"].detach())])}
    for side in ("key", "ref"):
        out[f"c.{side}_rois"] = rois[side].numpy().astype(np.float32)
        out[f"c.{side}_pos_gt"] = np.concatenate([res.pos_assigned_gt_inds.numpy() for res in srs[side]]).astype(np.int32)
    out["c.gt_match"] = np.concatenate([g.numpy() for g in gmi]).astype(np.int32)
    names = [n for n, _ in head.named_parameters()]
    assert len(names) == 16
    for n, p in head.named_parameters():
        out[f"c.grad.{n}"] = digest(p.grad, 256)
    for l, f in enumerate(x):
        out[f"c.gx{l}"] = digest(torch.zeros_like(f) if f.grad is None else f.grad, 4096)       # a level no RoI maps to: zeros
    print("branch losses", out["c.losses"], "seeds", seeds, "gt_match", out["c.gt_match"].tolist())
    assert np.isfinite(out["c.losses"]).all() and (out["c.gt_match"] < 0).any() and (out["c.gt_match"] >= 0).any()
    meta = dict(BRANCH, feat_seed=feat_seed, ref_feat_seed=feat_seed + 5000, relu_margin=margin, relu_margin_min=RELU_MARGIN, seeds=seeds, weight_seed=GT.HEAD_SEED, params=names, loss_track=GT.LOSS_TRACK, loss_track_aux=GT.LOSS_AUX,
                shapes={k: list(v) for k, v in shapes.items()})
    return out, meta


def main():
    from oracle import ref_loader
    utils = load_utils()
    out = box_cases(utils)
    gap = 0.0
    for name in SHAPES:
        for sel in ("identity", "perm", "few"):
            pg = out[f"a.{name}.{sel}.pos_gt"]
            ref = out[f"a.{name}.{sel}.ref_rois"]
            assert ref.shape == (len(pg), 5) and (ref[:, 0] == 0).all()
            gap = max(gap, float(np.abs(ref[:, 1:].astype(np.float64) - out[f"a.{name}.exact"][pg]).max()))
    print("ref_gap", gap)
    assert gap * 4 <= 1e-4, gap
    meta = dict(shapes={k: list(v) for k, v in SHAPES.items()}, selections=["identity", "perm", "few"], ref_gap=gap, swap_margin_min=SWAP_MARGIN,
                track_assigner=TRACK_ASSIGNER)
    ns = ref_loader.load_reference_assigner()
    sampler = sys.modules["polyphonic.funcs.sampler"].MaskPseudoSampler()
    b, meta["sampling"] = sampling_cases(ns, sampler)
    out.update(b)
    cc, meta["branch"] = branch_case(ns, sampler, utils)
    out.update(cc)
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(REPO, "tests", "golden", "video_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
