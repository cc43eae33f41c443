"""No GPU: the float64 oracles that tests/test_gpu_track_train_edges.py compares the track head's training path with, pinned to
what is committed, and every condition that file's cases rely on, computed from the seeds (tests/track_edge_cases.py).

  * `oracle/track_loss_oracle.py` against every case of tests/golden/track_train.npz (the reference's own classes in float64):
    losses <= 1e-12 relative, gradients <= 1e-6 max-normalised (the fixture stores them in float32), the NaN patterns of the two
    cases without a positive, and the three pairs in one call;
  * `video_oracle.roi_extract_vec` against the loop form `roi_extract`, values and autograd gradients <= 1e-12;
  * the mining cuts (a decisive gap, zeros at the cut, a split bit-equal pair), the ReLU margins after conditioning, the RoI
    sample coordinates and level boundaries."""
import json

import numpy as np
import pytest
import torch

import helpers as Hh
import track_edge_cases as TC
from oracle import track_loss_oracle as LO, video_oracle as VO

FINITE = ["a0", "a1", "a2", "e_one", "e_nomine", "e_twopos", "e_unmatched"]


def _fixture():
    z = Hh.load_golden("track_train.npz")
    return z, json.loads(bytes(z["meta_json"]).decode())


def _pairs(z, name):
    ks, rs, ms = z[f"{name}.key_start"], z[f"{name}.ref_start"], z[f"{name}.match_start"]
    return [dict(key=torch.from_numpy(z[f"{name}.key"][ks[p]:ks[p + 1]]), ref=torch.from_numpy(z[f"{name}.ref"][rs[p]:rs[p + 1]]),
                 key_gt=z[f"{name}.key_gt"][ks[p]:ks[p + 1]].tolist(), ref_gt=z[f"{name}.ref_gt"][rs[p]:rs[p + 1]].tolist(),
                 gt_match=z[f"{name}.gt_match"][ms[p]:ms[p + 1]].tolist()) for p in range(len(ks) - 1)]


def _cfg(meta):
    aux = meta["loss_track_aux"]
    return dict(lw_track=meta["loss_track"]["loss_weight"], lw_aux=aux["loss_weight"], neg_pos_ub=aux["neg_pos_ub"],
                pos_margin=aux["pos_margin"], neg_margin=aux["neg_margin"])


@pytest.mark.parametrize("name", FINITE)
def test_loss_oracle_reproduces_the_reference(name):
    z, meta = _fixture()
    assert _cfg(meta) == LO.SHIPPED
    losses, gk, gr = LO.track_loss_pairs(_pairs(z, name), _cfg(meta))
    want = torch.from_numpy(z[f"{name}.losses"])
    e_l = float((losses - want).abs().max() / want.abs().max().clamp_min(1e-300))
    e_k, e_r = Hh.rel_err(gk, z[f"{name}.g_key"]), Hh.rel_err(gr, z[f"{name}.g_ref"])
    print(name, "losses", e_l, "g_key", e_k, "g_ref", e_r)
    assert e_l <= 1e-12 and e_k <= 1e-6 and e_r <= 1e-6
    assert all(float(l) == 0.0 for l, w in zip(losses, want) if float(w) == 0.0)
    tgt = torch.cat([LO.targets(p["key_gt"], p["ref_gt"], p["gt_match"]).reshape(-1) for p in _pairs(z, name)])
    assert np.array_equal(tgt.numpy().astype(np.int8), z[f"{name}.targets"])


def test_loss_oracle_three_pairs_and_nan_patterns():
    z, meta = _fixture()
    pairs = [p for n in ("a0", "a1", "a2") for p in _pairs(z, n)]
    losses, gk, gr = LO.track_loss_pairs(pairs)
    want = torch.from_numpy(z["a_all.losses"])
    assert float((losses - want).abs().max() / want.abs().max()) <= 1e-12
    assert Hh.rel_err(gk * 3, np.concatenate([z[f"{n}.g_key"] for n in ("a0", "a1", "a2")])) <= 1e-6
    for name in ("e_nan", "e_pair_nan"):
        losses, gk, gr = LO.track_loss_pairs(_pairs(z, name))
        for got, ref in ((losses, z[f"{name}.losses"]), (gk, z[f"{name}.g_key"]), (gr, z[f"{name}.g_ref"])):
            assert np.array_equal(np.isnan(got.numpy()), np.isnan(ref)), name
            ok = ~np.isnan(ref)
            if ok.any():
                assert np.abs(got.numpy()[ok] - ref[ok]).max() <= 1e-6 * np.abs(ref[ok]).max(), name


def test_tie_rule_of_the_oracle():
    """ties at the cut: the lowest row-major index keeps its weight"""
    cost = torch.tensor([0.5, 0.2, 0.5, 0.2, 0.0, 0.2], dtype=torch.float64)
    assert LO.mining_cut(cost, 3).tolist() == [True, True, True, False, False, False]
    assert LO.mining_cut(cost, 4).tolist() == [True, True, True, True, False, False]
    assert LO.mining_cut(torch.zeros(5, dtype=torch.float64), 2).tolist() == [True, True, False, False, False]
    assert LO.mining_cut(cost, 0).tolist() == [False] * 6


# ---- the loss cases of the GPU file -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TC.LOSS_CASES))
def test_loss_case_conditions(name):
    build, over, kind = TC.LOSS_CASES[name]
    p, cfg = build(), TC.loss_cfg(name)
    st = TC.mining_stats(p, cfg)
    print(name, st)
    nk, nr = len(p["key_gt"]), len(p["ref_gt"])
    assert 1 <= nk <= 128 and 1 <= nr <= 128 and st["num_pos"] >= 1 and p["key"].shape[1] % 4 == 0
    assert st["mined"] == (kind != "free")
    if kind == "gap":
        assert 0 < st["kept"] < st["nonzero"] and st["last"] - st["first"] >= TC.GAP, st
    if kind == "zeros":            # fewer non-zero costs than kept: the cut is decided by index alone, among hundreds of ties
        assert st["nonzero"] < st["kept"] < st["num_neg"] and st["last"] == st["first"] == 0.0 and st["num_neg"] - st["nonzero"] >= 100
        assert st["edge"] >= 1e-5, st          # no cosine so close to the margin that float32 could put it on the other side of 0
    if kind == "twin":             # the keep-th and the next cost are the same bits and positive: the cut splits a pair of twins
        assert st["kept"] % 2 == 0 and st["last"] == st["first"] > 0.0, st
        assert torch.equal(p["ref"][:p["twins"]], p["ref"][p["twins"]:])
    if name == "zeros-20x20":
        assert st["nonzero"] > 0          # some costs above the zeros, all of them kept
    if name == "128x128":
        assert (nk, nr, st["num_pos"]) == (128, 128, 50)
    if name == "all-pos-row":
        tgt = LO.targets(p["key_gt"], p["ref_gt"], p["gt_match"])
        assert nr == 5 and tgt.all(1).sum() == 2 and (~tgt.any(1)).sum() == 4
    if name == "zero-rows":
        kz, rz = p["zero"]
        tgt = LO.targets(p["key_gt"], p["ref_gt"], p["gt_match"])
        assert tgt[kz].any() and tgt[:, rz].any() and not tgt[kz, rz] and float(p["key"][kz].norm()) == 0 == float(p["ref"][rz].norm())
    if name in ("E4", "E132"):
        assert p["key"].shape[1] == int(name[1:]) and p["key"].shape[1] % 128 != 0
    _, _, (losses, gk, gr) = TC.loss_case(name)
    assert torch.isfinite(losses).all() and torch.isfinite(gk).all() and torch.isfinite(gr).all()
    if name == "zero-rows":
        assert float(gk[p["zero"][0]].abs().max()) > 1e8            # the matched zero row: 1 / eps in its gradient


def test_joint_cases_share_cfg_and_width():
    for n in TC.JOINT:
        assert TC.loss_cfg(n) == LO.SHIPPED and TC.LOSS_CASES[n][0]()["key"].shape[1] == 256


# ---- RoIAlign ---------------------------------------------------------------------------------------------------------------------
def test_roi_extract_vec_matches_the_loop_form():
    from test_gpu_track_train import ROIS, LEVELS
    assert LEVELS == TC.LEVELS
    g = TC.gen(17)
    extra = TC._chain_boxes(g, 20)
    rois = torch.cat([ROIS, extra])
    feats = [torch.randn(1, 256, h, w, generator=g, dtype=torch.float64) for h, w in LEVELS]
    cot = torch.randn(rois.shape[0], 256, 7, 7, generator=g, dtype=torch.float64)
    assert len(set(VO.map_roi_levels(rois).tolist())) == 4
    res = []
    for fn in (VO.roi_extract, VO.roi_extract_vec):
        with torch.enable_grad():
            fi = [f.clone().requires_grad_(True) for f in feats]
            out = fn(fi, rois)
            res.append((out.detach(), torch.autograd.grad(out, fi, cot.to(out.dtype))))
    assert res[0][0].dtype == torch.float64, "the loop form follows its input's type"
    e = [Hh.rel_err(res[1][0], res[0][0])] + [Hh.rel_err(a, b) for a, b in zip(res[1][1], res[0][1])]
    print("roi_extract_vec against roi_extract: values, level gradients", e)
    assert max(e) <= 1e-12, e


@pytest.mark.parametrize("n", [260, 1024])
def test_roi_case_conditions(n):
    rois, bad = TC.roi_boxes(n)
    assert rois.shape == (n, 5) and torch.isnan(rois[bad]).any() and int((~torch.isfinite(rois).all(1)).sum()) == 1
    levels, jump, pow2, exact, near, nnear = TC.roi_conditions(rois)
    print(n, "levels", levels, "least distance to a jump", jump, "to a level boundary (relative)", pow2, "boundary squares + - 0.01:", near)
    assert levels == [0, 1, 2, 3] and jump >= 1e-4 and pow2 >= 1e-4 and exact == 4 and nnear == 8 and near >= 2e-5
    fin = rois[torch.isfinite(rois).all(1)]
    lv = VO.map_roi_levels(fin)
    assert min(int((lv == l).sum()) for l in range(4)) >= 20
    # the exact squares go UP a level (the + 1e-6 rule), their 0.01-smaller neighbours stay below
    sp, _ = TC.special_rois()
    assert VO.map_roi_levels(sp[:12]).tolist() == [0, 0, 0, 1, 1, 0, 2, 2, 1, 3, 3, 2]
    w, h = fin[:, 3] - fin[:, 1], fin[:, 4] - fin[:, 2]
    assert int(((w == 0) & (h == 0)).sum()) == 1 and int((fin[:, 3] < 0).sum()) >= 1 and int((fin[:, 1] > TC.IMG_W).sum()) >= 1


# ---- ReLU margins -----------------------------------------------------------------------------------------------------------------
def _none_near(pre, what):
    near = int((pre.abs() < TC.MARGIN).sum())
    assert near == 0, f"{what}: {near} of {pre.numel()} pre-activations within {TC.MARGIN} of 0"


def test_head_fixture_is_conditioned():
    sd, x, cot = TC.head_fixture()
    seen = []
    real = torch.nn.functional.group_norm

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]

    torch.nn.functional.group_norm = spy
    try:
        with torch.no_grad():
            sd64 = {k: v.double() for k, v in sd.items()}
            VO.track_embed_head(sd64, x.double(), prefix="")
            t = seen[-1].relu().reshape(x.shape[0], -1)
            seen.append(torch.nn.functional.linear(t, sd64["fcs.0.weight"], sd64["fcs.0.bias"]))
    finally:
        torch.nn.functional.group_norm = real
    assert len(seen) == 5
    for i, pre in enumerate(seen):
        _none_near(pre, f"head layer {i}")


@pytest.mark.parametrize("n", [65, 130])
def test_conv_gn_fixture_is_conditioned(n):
    _none_near(TC.conv_gn_reference(n)["pre"], f"conv + GroupNorm, n = {n}")


def test_fc_fixture_is_conditioned():
    _none_near(TC.fc_reference(TC.FC_N)["pre"], "fcs.0")


def test_chain_fixture_is_conditioned():
    c = TC.chain_fixture()
    with torch.no_grad():
        x = torch.cat([VO.roi_extract_vec(f, r, TC.STRIDES, TC.FINEST) for f, r in zip(c["feats"] + c["ref_feats"], c["rois"] + c["ref_rois"])])
        sd = {k: v.clone() for k, v in c["sd"].items()}
        for i, pre in enumerate(TC.condition_head(sd, x)):
            _none_near(pre, f"chain, head layer {i}")
    assert all(torch.equal(sd[k], c["sd"][k]) for k in sd), "conditioning a conditioned fixture changes nothing"
    for rois in c["rois"] + c["ref_rois"]:
        levels, jump, pow2 = TC.roi_conditions(rois)[:3]
        assert jump >= 1e-4 and pow2 >= 1e-4
    st = TC.chain_mining_stats()
    print(st)
    for s in st:
        assert s["num_pos"] >= 2 and (not s["mined"] or (0 < s["kept"] < s["nonzero"] and s["last"] - s["first"] >= TC.GAP)), s
