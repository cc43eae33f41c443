"""Fixtures for the track head's training path (tests/golden/track_train.npz), produced by the reference's own classes in fp64 on the CPU:
QuasiDenseMaskEmbedHeadGTMask (match, get_track_targets, loss) with the reference's MultiPosCrossEntropyLoss and L2Loss behind it.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_track_train.py

(a) loss cases with hard negative mining, E = 256, one pair each and the three in one call; (b) edge cases; (c) the whole head: seeded
weights, RoI features through the reference class and its losses, autograd gradients.  Every case stores the embeddings, the index
vectors, both losses, both gradients (fp32 roundings of the fp64 results), the target matrices and row weights.  The generator
searches seeds until a mined case decides something: more negatives with a non-zero cost than are kept, and a gap of at least 1e-4
between the last kept and the first dropped cost (about 400 x the fp32-against-fp64 difference of a cost)."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import helpers  # noqa: E402
from oracle import ref_loader  # noqa: E402

E = 256
GAP = 1e-4
LOSS_TRACK = dict(type="MultiPosCrossEntropyLoss", loss_weight=0.25)
LOSS_AUX = dict(type="L2Loss", neg_pos_ub=3, pos_margin=0, neg_margin=0.1, hard_mining=True, loss_weight=1.0)
HEAD_SEED, FEAT_SEED = 71, 72


def load_losses():
    """the reference's two loss classes, loaded by path next to the vendored mmdet/models/losses/utils.py"""
    ref_loader.load_reference()
    reg = ref_loader.Registry("track_losses")
    mmcv = sys.modules["mmcv"]
    mmcv.jit = lambda **kw: (lambda f: f)

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_loader.REF_ROOT, rel))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    ut = load("_ref_loss_utils", "mmdet/models/losses/utils.py")
    mm = sys.modules["mmdet.models"]
    mm.LOSSES, mm.weighted_loss, mm.weight_reduce_loss = reg, ut.weighted_loss, ut.weight_reduce_loss
    mp = load("_ref_multipos", "polyphonic/video/qdtrack/losses/multipos_cross_entropy_loss.py")
    l2 = load("_ref_l2", "polyphonic/video/qdtrack/losses/l2_loss.py")
    return mp.MultiPosCrossEntropyLoss, l2.L2Loss


def build_head():
    th = ref_loader.load_reference_track_head()
    MultiPos, L2 = load_losses()
    head = th.Head(norm_cfg=dict(type="GN", num_groups=32), loss_track=dict(LOSS_TRACK), loss_track_aux=dict(LOSS_AUX))
    head.loss_track = MultiPos(**{k: v for k, v in LOSS_TRACK.items() if k != "type"})
    head.loss_track_aux = L2(**{k: v for k, v in LOSS_AUX.items() if k != "type"})
    return head


def sres(gt_inds):
    return types.SimpleNamespace(pos_masks=torch.zeros((len(gt_inds), 1, 1)), pos_assigned_gt_inds=torch.as_tensor(gt_inds, dtype=torch.long))


def run_reference(head, pairs):
    """pairs: list of dicts (key, ref fp32 embeddings, key_gt, ref_gt, gt_match) -> losses [2], per-pair gradients, targets, weights"""
    ks = [p["key"].double().requires_grad_(True) for p in pairs]
    rs = [p["ref"].double().requires_grad_(True) for p in pairs]
    ksr, rsr = [sres(p["key_gt"]) for p in pairs], [sres(p["ref_gt"]) for p in pairs]
    gm = [torch.as_tensor(p["gt_match"], dtype=torch.long) for p in pairs]
    dists, cos = head.match(torch.cat(ks), torch.cat(rs), ksr, rsr)
    targets, weights = head.get_track_targets(gm, ksr, rsr)
    keep = [t.clone() for t in targets]
    losses = head.loss(dists, cos, targets, weights)
    (losses["loss_track"] + losses["loss_track_aux"]).backward()
    return (torch.stack([losses["loss_track"].detach(), losses["loss_track_aux"].detach()]), [k.grad for k in ks], [r.grad for r in rs], keep,
            weights)


def mining_stats(p):
    """(negatives kept, negatives with a non-zero cost, gap between the last kept and the first dropped cost) of a mined pair"""
    k, r = p["key"].double(), p["ref"].double()
    c = torch.nn.functional.normalize(k, dim=1) @ torch.nn.functional.normalize(r, dim=1).t()
    gm = torch.as_tensor(p["gt_match"])
    tgt = gm[torch.as_tensor(p["key_gt"])][:, None] == torch.as_tensor(p["ref_gt"])[None]
    cost = ((c - LOSS_AUX["neg_margin"]).clamp(0, 1) ** 2)[~tgt]
    npos, nneg = int(tgt.sum()), int((~tgt).sum())
    if not nneg / (npos + 1) > LOSS_AUX["neg_pos_ub"]:
        return dict(mined=False, num_pos=npos, num_neg=nneg)
    keep = npos * LOSS_AUX["neg_pos_ub"]
    srt = cost.sort(descending=True)[0]
    gap = float(srt[keep - 1] - srt[keep]) if 0 < keep < nneg else float("inf")
    return dict(mined=True, num_pos=npos, num_neg=nneg, kept=keep, nonzero=int((cost > 0).sum()), gap=gap)


def make_pair(seed, nk, nr, npos, ref_gt=None, gt_match=None, key_gt=None):
    """embeddings 0.65 * shared + randn (cosines near 0.3: nearly every negative has a non-zero cost); by default every RoI has its own
    ground truth, `npos` key ground truths are matched to distinct reference ones, the rest to -1 or to a reference ground truth no RoI
    was assigned to"""
    g = torch.Generator().manual_seed(seed)
    shared = torch.randn(1, E, generator=g)
    key = (0.65 * shared + torch.randn(nk, E, generator=g)).float()
    ref = (0.65 * shared + torch.randn(nr, E, generator=g)).float()
    if key_gt is None:
        key_gt = torch.randperm(nk, generator=g).tolist()
    if ref_gt is None:
        ref_gt = torch.randperm(nr, generator=g).tolist()
    if gt_match is None:
        cols = torch.randperm(nr, generator=g)[:npos].tolist()
        gt_match = [cols[i] if i < npos else (-1 if i % 2 else nr + i) for i in range(nk)]
    return dict(key=key, ref=ref, key_gt=key_gt, ref_gt=ref_gt, gt_match=gt_match)


def store(out, meta, name, head, pairs, note):
    losses, gk, gr, targets, weights = run_reference(head, pairs)
    out[f"{name}.key"] = torch.cat([p["key"] for p in pairs]).numpy()
    out[f"{name}.ref"] = torch.cat([p["ref"] for p in pairs]).numpy()
    out[f"{name}.key_gt"] = np.concatenate([np.asarray(p["key_gt"], np.int32) for p in pairs])
    out[f"{name}.ref_gt"] = np.concatenate([np.asarray(p["ref_gt"], np.int32) for p in pairs])
    out[f"{name}.gt_match"] = np.concatenate([np.asarray(p["gt_match"], np.int32) for p in pairs])
    for k, f in (("key_start", lambda p: len(p["key_gt"])), ("ref_start", lambda p: len(p["ref_gt"])), ("match_start", lambda p: len(p["gt_match"]))):
        out[f"{name}.{k}"] = np.concatenate([[0], np.cumsum([f(p) for p in pairs])]).astype(np.int32)
    out[f"{name}.losses"] = losses.numpy()
    out[f"{name}.g_key"] = torch.cat(gk).float().numpy()
    out[f"{name}.g_ref"] = torch.cat(gr).float().numpy()
    out[f"{name}.targets"] = np.concatenate([t.numpy().astype(np.int8).reshape(-1) for t in targets])
    out[f"{name}.weights"] = np.concatenate([w.numpy().astype(np.float32) for w in weights])
    for st in (mining_stats(p) for p in pairs):
        assert not st["mined"] or (st["gap"] >= GAP and st["nonzero"] > st["kept"]), (name, st)
    meta["cases"][name] = dict(note=note, shapes=[[len(p["key_gt"]), len(p["ref_gt"])] for p in pairs], stats=[mining_stats(p) for p in pairs],
                               nan=[bool(torch.isnan(a).any()) for a in gk])
    return losses, gk, gr


def main():
    torch.manual_seed(0)
    head = build_head().double()
    out, meta = {}, dict(E=E, loss_track=LOSS_TRACK, loss_track_aux=LOSS_AUX, gap_min=GAP, cases={})

    # (a) mined cases: search seeds for a decisive cut
    mined = []
    for tag, (nk, nr, npos) in (("a0", (5, 7, 3)), ("a1", (17, 33, 6)), ("a2", (100, 100, 40))):
        for seed in range(1000, 1400):
            p = make_pair(seed, nk, nr, npos)
            st = mining_stats(p)
            if st["mined"] and st["num_pos"] == npos and st["nonzero"] > st["kept"] and st["gap"] >= GAP:
                break
        else:
            raise RuntimeError(f"no seed gives a decisive cut for {tag}")
        print(tag, "seed", seed, st)
        meta.setdefault("seeds", {})[tag] = seed
        mined.append((p, store(out, meta, tag, head, [p], f"one pair ({nk}, {nr}), {npos} positives, mined")))
    losses3, gk3, gr3, _, _ = run_reference(head, [p for p, _ in mined])
    for i, (_, (l1, gk1, gr1)) in enumerate(mined):       # the three in one call: the mean of the losses, a third of each gradient
        assert helpers.rel_err(gk3[i] * 3, gk1[0]) < 1e-12 and helpers.rel_err(gr3[i] * 3, gr1[0]) < 1e-12
    assert torch.allclose(losses3, sum(l for _, (l, _, _) in mined) / 3, rtol=1e-12)
    out["a_all.losses"] = losses3.numpy()
    meta["a_all"] = dict(parts=["a0", "a1", "a2"], note="the three pairs in one call: losses stored, gradients are the single calls' / 3")

    # (b) edge cases
    one = make_pair(2001, 1, 1, 1, key_gt=[0], ref_gt=[0], gt_match=[0])
    store(out, meta, "e_one", head, [one], "(1, 1) with its one positive: no negatives, loss_track = 0")
    nomine = make_pair(2002, 2, 3, 2, key_gt=[0, 1], ref_gt=[0, 1, 2], gt_match=[2, 0])
    store(out, meta, "e_nomine", head, [nomine], "(2, 3), 2 positives: 4 negatives <= 3 * 3, no mining")
    twopos = make_pair(2003, 4, 6, 0, key_gt=[0, 1, 2, 3], ref_gt=[0, 1, 1, 2, 3, 4], gt_match=[1, 0, -1, 4])
    store(out, meta, "e_twopos", head, [twopos], "(4, 6): key 0 has two positives (two reference RoIs of one ground truth), key 2 is unmatched")
    unm = make_pair(2004, 3, 5, 0, key_gt=[1, 0, 1], ref_gt=[0, 1, 2, 3, 4], gt_match=[3, -1])
    store(out, meta, "e_unmatched", head, [unm], "(3, 5): keys 0 and 2 share a ground truth whose gt_match is -1 (weight 0 rows), key 1 matches")
    nanp = make_pair(2005, 3, 4, 0, key_gt=[0, 1, 2], ref_gt=[0, 1, 2, 3], gt_match=[-1, -1, -1])
    l, gk, gr = store(out, meta, "e_nan", head, [nanp], "(3, 4) without any positive: 0 / 0, NaN losses and gradients")
    assert torch.isnan(l).all() and torch.isnan(gk[0]).all() and torch.isnan(gr[0]).all()
    l, gk, gr = store(out, meta, "e_pair_nan", head, [nomine, nanp], "two pairs, the pair without a positive second: its rows NaN, the first pair's finite")
    assert torch.isnan(l).all() and torch.isfinite(gk[0]).all() and torch.isfinite(gr[0]).all() and torch.isnan(gk[1]).all() and torch.isnan(gr[1]).all()
    for name in ("e_one", "e_nomine", "e_twopos", "e_unmatched"):
        assert not any(meta["cases"][name]["nan"]) and np.isfinite(out[f"{name}.losses"]).all(), name
    assert out["e_one.losses"][0] == 0.0

    # (c) the whole head: seeded weights, RoI features from a seed, the reference forward, losses and autograd
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    head.load_state_dict({k: v.double() for k, v in helpers.seeded_fill(shapes, HEAD_SEED).items()})
    head.train()
    g = torch.Generator().manual_seed(FEAT_SEED)
    xk = torch.randn(3, 256, 7, 7, generator=g).double().requires_grad_(True)
    xr = torch.randn(4, 256, 7, 7, generator=g).double().requires_grad_(True)
    key_gt, ref_gt, gt_match = [0, 1, 2], [0, 1, 2, 1], [1, -1, 0]
    ksr, rsr = [sres(key_gt)], [sres(ref_gt)]
    ke, re_ = head(xk), head(xr)
    dists, cos = head.match(ke, re_, ksr, rsr)
    targets, weights = head.get_track_targets([torch.as_tensor(gt_match)], ksr, rsr)
    losses = head.loss(dists, cos, targets, weights)
    (losses["loss_track"] + losses["loss_track_aux"]).backward()
    names = [n for n, _ in head.named_parameters()]
    assert len(names) == 16, names
    out["head.losses"] = np.array([float(losses["loss_track"].detach()), float(losses["loss_track_aux"].detach())])
    out["head.key_embeds"] = ke.detach().float().numpy()
    out["head.ref_embeds"] = re_.detach().float().numpy()
    out["head.g_key_feats"] = xk.grad.float().numpy()
    for n, p in head.named_parameters():
        out[f"head.grad.{n}"] = digest(p.grad)
    meta["head"] = dict(weight_seed=HEAD_SEED, feat_seed=FEAT_SEED, shapes={k: list(v) for k, v in shapes.items()}, params=names,
                        key_gt=key_gt, ref_gt=ref_gt, gt_match=gt_match,
                        note="weights: helpers.seeded_fill(shapes, weight_seed); features: randn [3,256,7,7] then [4,256,7,7] from ONE generator(feat_seed)")
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(REPO, "tests", "golden", "track_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


def digest(t, n=256):
    """(norm, sum, n strided entries) of a gradient -- the form tests/test_gpu_neck_train.py's _digest compares"""
    f = t.detach().double().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, n).long()
    return np.concatenate([[float(f.norm()), float(f.sum())], f[idx].numpy()])


if __name__ == "__main__":
    main()
