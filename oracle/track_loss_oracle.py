"""TEST INFRASTRUCTURE ONLY -- CPU restatement, in float64 under autograd, of the track head's losses
(polyphonic/video/track_heads.py:104-162: get_track_targets, match, loss) with the QDTrack loss classes behind it
(MultiPosCrossEntropyLoss, L2Loss with hard negative mining).  Same rules as oracle/poly_oracle.py: plain torch, no library call.

Pinning: tests/test_track_oracle_host.py compares `track_loss` with every case of tests/golden/track_train.npz, which the
reference's own classes produced (tools/gen_golden_track_train.py).

Two points the reference leaves open are fixed here as `ph_track_loss` (csrc/ph_trackloss.hip) documents them:
  * ties at the hard-negative cut go to the lowest row-major index i * Nr + j (the reference's `topk` does not say): a stable
    descending sort of the negatives in row-major order;
  * the products are formed without BLAS, so that identical embedding rows give bit-identical costs and really tie."""
import torch
import torch.nn.functional as F

SHIPPED = dict(lw_track=0.25, lw_aux=1.0, neg_pos_ub=3, pos_margin=0.0, neg_margin=0.1)


def targets(key_gt, ref_gt, gt_match):
    """get_track_targets for one pair: bool [Nk, Nr]; a key ground truth outside gt_match matches nothing"""
    key_gt, ref_gt, gt_match = (torch.as_tensor(t, dtype=torch.long).reshape(-1) for t in (key_gt, ref_gt, gt_match))
    inside = (key_gt >= 0) & (key_gt < gt_match.numel())
    m = torch.full_like(key_gt, torch.iinfo(torch.int32).min)
    m[inside] = gt_match[key_gt[inside]]
    return m[:, None] == ref_gt[None, :]


def _rows_dot(a, b):
    """[Na, E] x [Nb, E] -> [Na, Nb], every entry its own ascending sum (no BLAS blocking: equal rows give equal bits)"""
    return (a[:, None, :] * b[None, :, :]).sum(-1)


def mining_cut(cost_neg, keep):
    """the negatives (row-major order) that keep their weight: the `keep` largest costs, ties to the lowest index -> bool mask"""
    order = torch.sort(cost_neg, descending=True, stable=True)[1]
    kept = torch.zeros(cost_neg.numel(), dtype=torch.bool)
    kept[order[:keep]] = True
    return kept


def aux_weights(pred, tgt, neg_pos_ub):
    """L2Loss.update_weight after the clamp: (weight [Nk, Nr] of 0 / 1, mined?, negatives kept)"""
    num_pos, num_neg = int(tgt.sum()), int((~tgt).sum())
    w = torch.ones(tgt.shape, dtype=torch.float64)
    if not (neg_pos_ub > 0 and num_neg / (num_pos + 1) > neg_pos_ub):
        return w, False, num_neg
    keep = num_pos * int(neg_pos_ub)
    cost = ((pred.detach() - 0.0) ** 2)[~tgt]                       # row-major order of the negatives
    wn = torch.zeros(num_neg, dtype=torch.float64)
    wn[mining_cut(cost, keep)] = 1.0
    w[~tgt] = wn
    return w, True, keep


def track_loss_values(k, r, key_gt, ref_gt, gt_match, cfg=SHIPPED):
    """(loss_track, loss_track_aux) [2] of one pair as a function of the float64 embeddings k [Nk, E], r [Nr, E]: differentiable,
    so a caller may chain it behind an oracle that produced the embeddings"""
    tgt = targets(key_gt, ref_gt, gt_match)
    # ---- MultiPos: per row logsumexp over [0] and d_in - d_ip for every (negative n, positive p)
    d = _rows_dot(k, r)
    diff = d[:, :, None] - d[:, None, :]                                                      # [i, n, p]
    pair = (~tgt)[:, :, None] & tgt[:, None, :]
    x = torch.where(pair, diff, torch.full_like(diff, float("-inf"))).reshape(d.shape[0], -1)
    row = torch.logsumexp(torch.cat([torch.zeros(d.shape[0], 1, dtype=torch.float64), x], 1), 1)
    w = tgt.any(1).double()
    loss_track = cfg["lw_track"] * (row * w).sum() / w.sum()
    # ---- L2 on the clamped cosines
    cos = _rows_dot(F.normalize(k, p=2.0, dim=1, eps=1e-12), F.normalize(r, p=2.0, dim=1, eps=1e-12))
    margin = torch.full(tgt.shape, max(float(cfg["neg_margin"]), 0.0), dtype=torch.float64)           # a margin <= 0 is not applied
    margin[tgt] = max(float(cfg["pos_margin"]), 0.0)
    pred = (cos - margin).clamp(0.0, 1.0)
    wt, _, _ = aux_weights(pred, tgt, cfg["neg_pos_ub"])
    avg = (wt > 0).sum().double()
    loss_aux = cfg["lw_aux"] * (wt * (pred - tgt.double()) ** 2).sum() / avg
    return torch.stack([loss_track, loss_aux])


def track_loss(key, ref, key_gt, ref_gt, gt_match, cfg=SHIPPED):
    """one key / reference pair -> (losses [2] = (loss_track, loss_track_aux), d(sum of both) / d key, / d ref), float64"""
    with torch.enable_grad():
        k = torch.as_tensor(key).detach().double().clone().requires_grad_(True)
        r = torch.as_tensor(ref).detach().double().clone().requires_grad_(True)
        losses = track_loss_values(k, r, key_gt, ref_gt, gt_match, cfg)
        gk, gr = torch.autograd.grad(losses.sum(), (k, r))
    return losses.detach(), gk, gr


def track_loss_pairs(pairs, cfg=SHIPPED):
    """pairs: dicts (key, ref, key_gt, ref_gt, gt_match) -> (mean losses [2], g_key [sum Nk, E], g_ref [sum Nr, E]) of the mean"""
    res = [track_loss(p["key"], p["ref"], p["key_gt"], p["ref_gt"], p["gt_match"], cfg) for p in pairs]
    n = len(res)
    return sum(l for l, _, _ in res) / n, torch.cat([g for _, g, _ in res]) / n, torch.cat([g for _, _, g in res]) / n
