"""Seeded inputs of tests/test_gpu_track_train_edges.py and the conditions they must meet, CPU only.  The GPU tests build their
references from these; tests/test_track_oracle_host.py asserts every condition without a GPU, so that a seed change which breaks
one fails there.  Everything comes from seeded CPU generators; nothing is stored."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import helpers as Hh
from oracle import track_loss_oracle as LO, video_oracle as VO

MARGIN = 5e-5                    # a ReLU pre-activation this close to 0 is a coin flip between device and float64
NUDGE, ROUNDS = 2e-3, 20
GAP = 1e-5                       # the least distance between the last kept and the first dropped cost outside the tie cases
HEAD_SEED = 71                   # track_train.npz's head weights


def gen(seed):
    return torch.Generator().manual_seed(seed)


def row_err(got, want):
    """max over the rows of max|got - want| / that row's float64 maximum (rows: the last axis); a row whose maximum is below 1e-12
    of the global one is measured against 1e-12 of the global maximum -- test_gpu_loss_edges.row_err"""
    want = want.double().reshape(-1, want.shape[-1])
    d = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    rmax = want.abs().amax(1)
    norm = rmax.clamp_min(1e-12 * float(rmax.max())).clamp_min(1e-300)
    return float((d.amax(1) / norm).max())


# =================================================================================================================================
# ph_track_loss
# =================================================================================================================================
def make_pair(seed, nk, nr, npos, E=256, shared=0.65):
    """the recipe of tools/gen_golden_track_train.py::make_pair: embeddings `shared` * common + randn, every RoI its own ground
    truth, `npos` key ground truths matched to distinct reference ones, the rest to -1 or to one no RoI was assigned to"""
    g = gen(seed)
    common = torch.randn(1, E, generator=g)
    key = (shared * common + torch.randn(nk, E, generator=g)).float()
    ref = (shared * common + torch.randn(nr, E, generator=g)).float()
    key_gt = torch.randperm(nk, generator=g).tolist()
    ref_gt = torch.randperm(nr, generator=g).tolist()
    cols = torch.randperm(nr, generator=g)[:npos].tolist()
    gt_match = [cols[i] if i < npos else (-1 if i % 2 else nr + i) for i in range(nk)]
    return dict(key=key, ref=ref, key_gt=key_gt, ref_gt=ref_gt, gt_match=gt_match)


def _twin_refs(p):
    """the references twice, the copies under ground truths of their own: every negative cost of a column has a bit-equal twin"""
    nr = len(p["ref_gt"])
    return dict(p, ref=torch.cat([p["ref"], p["ref"]]), ref_gt=p["ref_gt"] + [1000 + v for v in p["ref_gt"]], twins=nr)


def _all_pos_row():
    """Nr = 5 RoIs of ONE ground truth: keys 0 and 1 (matched to it) have nothing but positives, keys 2..5 nothing but negatives"""
    p = make_pair(3107, 6, 5, 0)
    return dict(p, key_gt=[0, 0, 1, 2, 3, 4], ref_gt=[7, 7, 7, 7, 7], gt_match=[7, -1, 3, 9, -1])


def _zero_rows():
    """a matched key row and a matched reference row (of another key) are zero vectors: norms below the eps"""
    p = make_pair(3108, 12, 14, 4)
    tgt = LO.targets(p["key_gt"], p["ref_gt"], p["gt_match"])
    rows, cols = tgt.nonzero(as_tuple=True)
    kz, rz = int(rows[0]), int(cols[1])
    assert int(rows[1]) != kz
    key, ref = p["key"].clone(), p["ref"].clone()
    key[kz], ref[rz] = 0.0, 0.0
    return dict(p, key=key, ref=ref, zero=(kz, rz))


# name -> (builder, cfg overrides, kind); kind: "gap" (a decisive cut), "zeros" (the cut falls among zero costs), "twin" (the cut
# splits a bit-equal pair of positive costs), "free" (not mined).  Seeds: the first of the recipe that meets the case's condition.
LOSS_CASES = {
    "128x128": (lambda: make_pair(3001, 128, 128, 50), {}, "gap"),
    "128x1": (lambda: make_pair(3010, 128, 1, 1), {}, "gap"),
    "1x128": (lambda: make_pair(3020, 1, 128, 1), {}, "gap"),
    "113x97": (lambda: make_pair(3030, 113, 97, 30), {}, "gap"),
    "zeros-20x20": (lambda: make_pair(3040, 20, 20, 20, shared=0.0), {}, "zeros"),
    "zeros-40x60": (lambda: make_pair(3050, 40, 60, 30, shared=0.0), dict(neg_margin=0.3), "zeros"),
    "split-tie": (lambda: _twin_refs(make_pair(6, 9, 10, 5)), dict(neg_pos_ub=4), "twin"),
    "all-pos-row": (_all_pos_row, {}, "free"),
    "zero-rows": (_zero_rows, {}, "gap"),
    "E4": (lambda: make_pair(3060, 17, 33, 6, E=4), {}, "gap"),
    "E132": (lambda: make_pair(3070, 17, 33, 6, E=132), {}, "gap"),
    "ub-1": (lambda: make_pair(3080, 17, 33, 6), dict(neg_pos_ub=-1), "free"),
    "ub1": (lambda: make_pair(3080, 17, 33, 6), dict(neg_pos_ub=1), "gap"),
    "pos-margin": (lambda: make_pair(3080, 17, 33, 6), dict(pos_margin=0.2), "gap"),
}
JOINT = ("113x97", "zeros-20x20", "all-pos-row")        # three pairs of the shipped cfg and E = 256 in one launch


def loss_cfg(name):
    return {**LO.SHIPPED, **LOSS_CASES[name][1]}


def mining_stats(p, cfg):
    """of one pair in float64: positives, negatives, mined?, negatives kept, non-zero costs, the costs on either side of the cut,
    and the least distance of a negative's cosine from its clamp's lower end (where the cost leaves 0)"""
    k, r = p["key"].double(), p["ref"].double()
    cos = LO._rows_dot(F.normalize(k, dim=1), F.normalize(r, dim=1))
    tgt = LO.targets(p["key_gt"], p["ref_gt"], p["gt_match"])
    m = max(float(cfg["neg_margin"]), 0.0)
    cost = ((cos - m).clamp(0, 1) ** 2)[~tgt]
    npos, nneg = int(tgt.sum()), int((~tgt).sum())
    st = dict(num_pos=npos, num_neg=nneg, mined=bool(cfg["neg_pos_ub"] > 0 and nneg / (npos + 1) > cfg["neg_pos_ub"]),
              nonzero=int((cost > 0).sum()), edge=float((cos[~tgt] - m).abs().min()) if nneg else float("inf"))
    if st["mined"]:
        keep = npos * int(cfg["neg_pos_ub"])
        srt = cost.sort(descending=True)[0]
        st.update(kept=keep, last=float(srt[keep - 1]), first=float(srt[keep]))
    return st


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """(pair, cfg, float64 reference (losses, g_key, g_ref)) -- computed once, shared, never modified"""
    build, _, _ = LOSS_CASES[name]
    p, cfg = build(), loss_cfg(name)
    return p, cfg, LO.track_loss(p["key"], p["ref"], p["key_gt"], p["ref_gt"], p["gt_match"], cfg)


# =================================================================================================================================
# ReLU conditioning of the conv + GroupNorm stack and the linear layers
# =================================================================================================================================
def condition_bias(pre_of, bias, what):
    """nudge `bias` (float32 [C], changed in place) by NUDGE on every channel where pre_of(bias) -- the float64 pre-activation
    [n, C, ...] -- has an entry within MARGIN of 0, until none has; gives up after ROUNDS with an assertion.  -> rounds used"""
    for it in range(ROUNDS + 1):
        pre = pre_of(bias)
        near = pre.abs() < MARGIN
        if not near.any():
            return it
        assert it < ROUNDS, f"{what}: {int(near.sum())} pre-activations within {MARGIN} of 0 after {ROUNDS} rounds"
        ch = near.transpose(0, 1).reshape(pre.shape[1], -1).any(1)
        bias += NUDGE * ch.float()


def gn_pre(y, gamma, beta, groups=32):
    return F.group_norm(y, groups, gamma.double(), beta.double(), 1e-5)


def condition_head(sd, x, prefix=""):
    """layer by layer, in order: the GroupNorm biases of the four convs, then fcs.0.bias, of the float32 state dict `sd` (changed in
    place) on the RoI features x [n, 256, 7, 7]; -> the float64 pre-activations of the five layers under the final weights"""
    t, pres = x.double(), []
    for i in range(4):
        y = F.conv2d(t, sd[f"{prefix}convs.{i}.conv.weight"].double(), padding=1)
        gamma, beta = sd[f"{prefix}convs.{i}.gn.weight"], sd[f"{prefix}convs.{i}.gn.bias"]
        condition_bias(lambda b: gn_pre(y, gamma, b), beta, f"convs.{i}")
        pres.append(gn_pre(y, gamma, beta))
        t = pres[-1].relu()
    h = t.reshape(t.shape[0], -1) @ sd[prefix + "fcs.0.weight"].double().t()
    b1 = sd[prefix + "fcs.0.bias"]
    condition_bias(lambda b: h + b.double(), b1, "fcs.0")
    pres.append(h + b1.double())
    return pres


def head_state(seed=HEAD_SEED):
    shapes = {k[len("track_head."):]: v for k, v in Hh.TRACK_HEAD_SHAPES.items()}
    return Hh.seeded_fill(shapes, seed)


def head_autograd(sd, x, cot, dtype=torch.float64):
    """`video_oracle.track_embed_head` under autograd -> (embeddings, {parameter: gradient}, dx) for the cotangent `cot`"""
    with torch.enable_grad():
        w = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        xi = x.to(dtype).requires_grad_(True)
        out = VO.track_embed_head(w, xi, prefix="")
        grads = torch.autograd.grad(out, [xi] + [w[k] for k in sorted(w)], cot.to(dtype))
    return out.detach(), dict(zip(sorted(w), grads[1:])), grads[0]


HEAD_N = 130


@functools.lru_cache(maxsize=None)
def head_fixture():
    """(state dict, x [130, 256, 7, 7], cotangent [130, 256]) with every ReLU of the float64 forward decided; GroupNorm is per RoI
    and the linear layers per row, so the first n RoIs are conditioned for every n <= 130"""
    sd = head_state()
    g = gen(4101)
    x = torch.randn(HEAD_N, 256, 7, 7, generator=g)
    cot = torch.randn(HEAD_N, 256, generator=g)
    condition_head(sd, x)
    return sd, x, cot


@functools.lru_cache(maxsize=None)
def head_reference(n):
    sd, x, cot = head_fixture()
    return head_autograd(sd, x[:n], cot[:n])


# ---- one conv + GroupNorm + ReLU layer on n maps of 7 x 7 ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_gn_fixture(n):
    g = gen(4200 + n)
    x = torch.randn(n, 256, 7, 7, generator=g)
    w = torch.randn(256, 256, 3, 3, generator=g) * float(np.sqrt(2.0 / (2304 + 256)))
    gamma, beta = 1.0 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    cot = torch.randn(n, 256, 7, 7, generator=g)
    y = F.conv2d(x.double(), w.double(), padding=1)
    condition_bias(lambda b: gn_pre(y, gamma, b), beta, "conv + GroupNorm")
    return x, w, gamma, beta, cot


def conv_gn_autograd(x, w, gamma, beta, cot, dtype=torch.float64):
    """-> dict(y, dx, dw, dgamma, dbeta, pre) of relu(group_norm(conv2d(x, w)))"""
    n, HW = x.shape[0], x.shape[2] * x.shape[3]
    with torch.enable_grad():
        xi, wi, gi, bi = (t.to(dtype).requires_grad_(True) for t in (x, w, gamma, beta))
        conv = F.conv2d(xi, wi, padding=1)
        pre = torch.native_group_norm(conv, gi, bi, n, 256, HW, 32, 1e-5)[0]
        y = pre.relu()
        dx, dw, dg, db = torch.autograd.grad(y, (xi, wi, gi, bi), cot.to(dtype))
    return dict(y=y.detach(), dx=dx, dw=dw, dgamma=dg, dbeta=db, pre=pre.detach())


@functools.lru_cache(maxsize=None)
def conv_gn_reference(n):
    return conv_gn_autograd(*conv_gn_fixture(n))


# ---- fc_embed(relu(fcs.0(x))) ----------------------------------------------------------------------------------------------------
FC_N = 130


@functools.lru_cache(maxsize=None)
def fc_fixture():
    """(x [130, 12544], W1, b1, W2, b2, cotangent [130, 256]) at the shipped widths, fcs.0's ReLU decided for every row"""
    sd = head_state(4300)
    g = gen(4301)
    x = torch.randn(FC_N, 12544, generator=g).relu()                 # what follows a ReLU
    cot = torch.randn(FC_N, 256, generator=g)
    W1, b1, W2, b2 = sd["fcs.0.weight"], sd["fcs.0.bias"], sd["fc_embed.weight"], sd["fc_embed.bias"]
    h = x.double() @ W1.double().t()
    condition_bias(lambda b: h + b.double(), b1, "fcs.0")
    return x, W1, b1, W2, b2, cot


def fc_autograd(x, W1, b1, W2, b2, cot, dtype=torch.float64):
    with torch.enable_grad():
        t = [v.to(dtype).requires_grad_(True) for v in (x, W1, b1, W2, b2)]
        pre = F.linear(t[0], t[1], t[2])
        out = F.linear(pre.relu(), t[3], t[4])
        grads = torch.autograd.grad(out, t, cot.to(dtype))
    return dict(zip(("out", "gx", "gW1", "gb1", "gW2", "gb2", "pre"), (out.detach(),) + tuple(grads) + (pre.detach(),)))


@functools.lru_cache(maxsize=None)
def fc_reference(n):
    x, W1, b1, W2, b2, cot = fc_fixture()
    return fc_autograd(x[:n], W1, b1, W2, b2, cot[:n])


# =================================================================================================================================
# RoIAlign
# =================================================================================================================================
LEVELS = [(16, 32), (8, 16), (4, 8), (2, 4)]            # tests/test_gpu_track_train.py's: a 64 x 128 image
STRIDES, FINEST = (4, 8, 16, 32), 56
IMG_H, IMG_W = 64, 128
BOUNDARY = (56.0, 112.0, 224.0, 448.0)
ROI_SEED = {260: 5001, 1024: 5002}        # the first seeds from 5000 that meet the margins test_track_oracle_host.py asserts


def special_rois():
    """squares of exactly 56, 112, 224, 448 px and the same +- 0.01 (corners on integers, so that width and height are exact);
    boxes beyond every border; a zero-area box; -> (rois [k, 5], index of the first exact-boundary box)"""
    rows = []
    for s in BOUNDARY:
        rows += [[0.0, 3.0, 2.0, 3.0 + s, 2.0 + s], [0.0, 3.0, 2.0, 3.0 + s + 0.01, 2.0 + s + 0.01], [0.0, 3.0, 2.0, 3.0 + s - 0.01, 2.0 + s - 0.01]]
    rows += [[0.0, -300.0, -280.0, -200.0, -190.0],          # wholly left of / above the image: every sample dropped
             [0.0, 150.0, 90.0, 260.0, 170.0],               # wholly right of / below it
             [0.0, -20.0, -10.0, 30.0, 25.0],                # across the upper left corner
             [0.0, 100.0, 40.0, 170.0, 99.0],                # across the lower right corner
             [0.0, -500.0, -400.0, 700.0, 600.0],            # around the whole image
             [0.0, 40.0, 30.0, 40.0, 30.0],                  # zero area
             [0.0, 64.0, 10.0, 64.0, 50.0]]                  # zero width
    return torch.tensor(rows, dtype=torch.float32), 0


@functools.lru_cache(maxsize=None)
def roi_boxes(n):
    """n RoIs on the 64 x 128 image: the special boxes, one NaN box (the last but one), the rest with log-uniform sizes over all
    four levels and centres inside the image.  -> (rois [n, 5] float32, index of the NaN box)"""
    sp, _ = special_rois()
    g = gen(ROI_SEED[n])
    m = n - sp.shape[0] - 1
    size = 56.0 * 2.0 ** (torch.rand(m, generator=g) * 4.6 - 0.8)                  # sqrt(w h) from 32 to 760 px
    aspect = 2.0 ** (torch.rand(m, generator=g) * 2.0 - 1.0)
    w, h = size * aspect.sqrt(), size / aspect.sqrt()
    cx, cy = torch.rand(m, generator=g) * IMG_W, torch.rand(m, generator=g) * IMG_H
    rnd = torch.stack([torch.zeros(m), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).float()
    nan_box = torch.tensor([[0.0, float("nan"), 10.0, 50.0, 60.0]])
    perm = torch.randperm(m + sp.shape[0], generator=g)                            # the special boxes anywhere among the others
    rois = torch.cat([torch.cat([rnd, sp])[perm], nan_box])
    return rois.contiguous(), rois.shape[0] - 1


def roi_conditions(rois):
    """of the finite boxes of `rois`: (levels used, least distance of a sample coordinate from -1 and from H / W -- where the value
    jumps --, least relative distance of sqrt(w h) / 56 from a power of two over the boxes that are not boundary squares, the number
    of exact boundary squares, the same distance over the + - 0.01 squares -- 0.01 / 448 = 2.2e-5, some 180 float32 steps: the
    level of such a box does not depend on whose sqrt and log2 computed it -- and their number)"""
    fin = torch.isfinite(rois).all(1)
    r = rois[fin]
    lv = VO.map_roi_levels(r)
    ys, xs, Hn, Wn = VO.roi_sample_coords(r, lv, LEVELS, STRIDES)
    jump = min(float((ys + 1.0).abs().min()), float((ys - Hn[:, None].double()).abs().min()),
               float((xs + 1.0).abs().min()), float((xs - Wn[:, None].double()).abs().min()))
    wd, ht = (r[:, 3] - r[:, 1]).double(), (r[:, 4] - r[:, 2]).double()
    sc = (wd * ht).sqrt() / FINEST
    side = torch.tensor(BOUNDARY, dtype=torch.float64)
    exact = (wd == ht) & torch.isin(wd, side)
    beside = (wd == ht) & ~exact & ((wd[:, None] - side[None]).abs() < 0.011).any(1)       # the + - 0.01 squares

    def dist(sel):
        v = sc[sel & (sc > 0)]
        pw = 2.0 ** torch.log2(v).round()
        return float(((v - pw).abs() / pw).min()) if v.numel() else float("inf")

    return sorted(set(lv.tolist())), jump, dist(~exact & ~beside), int(exact.sum()), dist(beside), int(beside.sum())


@functools.lru_cache(maxsize=None)
def roi_reference(n):
    """(feats, rois, nan index, cotangent, float64 RoI features, float64 level gradients); the NaN box's cotangent rows reach nothing"""
    rois, bad = roi_boxes(n)
    g = gen(5100 + n)
    feats = [torch.randn(1, 256, h, w, generator=g) for h, w in LEVELS]
    cot = torch.randn(n, 256, 7, 7, generator=g)
    with torch.enable_grad():
        fi = [f.double().requires_grad_(True) for f in feats]
        out = VO.roi_extract_vec(fi, rois, STRIDES, FINEST)
        grads = torch.autograd.grad(out, fi, cot.double())
    return feats, rois, bad, cot, out.detach(), [t.detach() for t in grads]


# =================================================================================================================================
# the whole chain: two key / reference pairs
# =================================================================================================================================
CHAIN_NK, CHAIN_NR = (21, 17), (19, 23)


def _chain_boxes(g, n):
    size = 56.0 * 2.0 ** (torch.rand(n, generator=g) * 3.4 - 0.6)
    aspect = 2.0 ** (torch.rand(n, generator=g) * 1.6 - 0.8)
    w, h = size * aspect.sqrt(), size / aspect.sqrt()
    cx, cy = torch.rand(n, generator=g) * IMG_W, torch.rand(n, generator=g) * IMG_H
    return torch.stack([torch.zeros(n), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).float().contiguous()


@functools.lru_cache(maxsize=None)
def chain_fixture():
    """FPN levels, RoIs and ground-truth indices of two pairs, and the head's weights conditioned on the float64 RoI features"""
    g = gen(6001)
    mk = lambda: [torch.randn(1, 256, h, w, generator=g) for h, w in LEVELS]
    feats, ref_feats = [mk(), mk()], [mk(), mk()]
    rois = [_chain_boxes(g, n) for n in CHAIN_NK]
    ref_rois = [_chain_boxes(g, n) for n in CHAIN_NR]
    key_gt = [torch.randint(0, 12, (n,), generator=g).tolist() for n in CHAIN_NK]
    ref_gt = [torch.randint(0, 12, (n,), generator=g).tolist() for n in CHAIN_NR]
    gt_match = [[int(v) if v < 12 else -1 for v in torch.randint(0, 16, (12,), generator=g).tolist()] for _ in range(2)]
    sd = head_state()
    with torch.no_grad():
        x = torch.cat([VO.roi_extract_vec(f, r, STRIDES, FINEST) for f, r in zip(feats + ref_feats, rois + ref_rois)])
    condition_head(sd, x)
    return dict(feats=feats, ref_feats=ref_feats, rois=rois, ref_rois=ref_rois, key_gt=key_gt, ref_gt=ref_gt, gt_match=gt_match, sd=sd)


@functools.lru_cache(maxsize=None)
def chain_reference():
    """the three oracles in a row, float64 under autograd: RoI features of the key frames (gradients flow) and of the reference
    frames, the head on all of them, the mean of the pairs' losses -> (losses [2], {parameter: gradient}, key level gradients
    [pair][level], key embeddings, reference embeddings)"""
    c = chain_fixture()
    with torch.enable_grad():
        w = {k: v.double().requires_grad_(True) for k, v in c["sd"].items()}
        kf = [[f.double().requires_grad_(True) for f in lv] for lv in c["feats"]]
        key_x = [VO.roi_extract_vec(f, r, STRIDES, FINEST) for f, r in zip(kf, c["rois"])]
        with torch.no_grad():
            ref_x = [VO.roi_extract_vec(f, r, STRIDES, FINEST) for f, r in zip(c["ref_feats"], c["ref_rois"])]
        emb = VO.track_embed_head(w, torch.cat(key_x + ref_x), prefix="")
        ks, rs = np.cumsum((0,) + CHAIN_NK), sum(CHAIN_NK) + np.cumsum((0,) + CHAIN_NR)
        ke, re_ = [emb[ks[i]:ks[i + 1]] for i in range(2)], [emb[rs[i]:rs[i + 1]] for i in range(2)]
        losses = sum(LO.track_loss_values(ke[i], re_[i], c["key_gt"][i], c["ref_gt"][i], c["gt_match"][i]) for i in range(2)) / 2
        flat = [f for lv in kf for f in lv]
        leaves = [w[k] for k in sorted(w)] + flat
        grads = torch.autograd.grad(losses.sum(), leaves, allow_unused=True)           # a level without a RoI: zeros
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    nw = len(w)
    gl = [list(grads[nw + 4 * i:nw + 4 * i + 4]) for i in range(2)]
    return losses.detach(), dict(zip(sorted(w), grads[:nw])), gl, [t.detach() for t in ke], [t.detach() for t in re_]


def chain_mining_stats():
    c = chain_fixture()
    _, _, _, ke, re_ = chain_reference()
    return [mining_stats(dict(key=ke[i], ref=re_[i], key_gt=c["key_gt"][i], ref_gt=c["ref_gt"][i], gt_match=c["gt_match"][i]), LO.SHIPPED)
            for i in range(2)]
