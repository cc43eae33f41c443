"""CPU: the track head's training path as far as it can be checked without a GPU -- the C ABI declares the new entry points, the
targets `get_track_targets` builds from plain integer tensors equal the reference's (tests/golden/track_train.npz, written by
tools/gen_golden_track_train.py from the reference's own classes in fp64), the fixture keeps the conditions that make its mined cases
decisive, and the reference-named methods that take similarity matrices point at `track_loss`."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, track_head  # noqa: F401  (registers the head)
from polyphonicformer_amd.registry import HEADS


def _fixture():
    z = Hh.load_golden("track_train.npz")
    return z, json.loads(bytes(z["meta_json"]).decode())


def _head(**kw):
    return HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32), **kw))


def test_header_and_bindings_declare_the_entry_points():
    hdr = open(os.path.join(Hh.REPO, "include", "polyhead.h")).read()
    for name in ("ph_track_loss", "ph_track_loss_scratch_bytes", "ph_roi_align_fpn_bwd"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert "ph_track_loss_cfg" in _lib.STRUCTS
    assert [f for f, _ in _lib.TrackLossCfg._fields_] == ["pairs", "E", "lw_track", "lw_aux", "neg_pos_ub", "pos_margin", "neg_margin", "hard_mining"]


def test_get_track_targets_equals_the_reference():
    z, meta = _fixture()
    head = _head()
    assert len(meta["cases"]) >= 9
    for name, case in meta["cases"].items():
        ks, rs, ms = z[f"{name}.key_start"], z[f"{name}.ref_start"], z[f"{name}.match_start"]
        sr = lambda a, s, p: types.SimpleNamespace(pos_assigned_gt_inds=torch.from_numpy(a[s[p]:s[p + 1]].astype(np.int64)))
        P = len(case["shapes"])
        targets, weights = head.get_track_targets([torch.from_numpy(z[f"{name}.gt_match"][ms[p]:ms[p + 1]].astype(np.int64)) for p in range(P)],
                                                  [sr(z[f"{name}.key_gt"], ks, p) for p in range(P)],
                                                  [sr(z[f"{name}.ref_gt"], rs, p) for p in range(P)])
        assert [list(t.shape) for t in targets] == case["shapes"], name
        assert np.array_equal(np.concatenate([t.numpy().reshape(-1) for t in targets]), z[f"{name}.targets"]), name
        assert np.array_equal(np.concatenate([w.numpy() for w in weights]), z[f"{name}.weights"]), name
        assert all(t.dtype == torch.int32 for t in targets) and all(w.dtype == torch.float32 for w in weights)


def test_fixture_keeps_its_conditions():
    z, meta = _fixture()
    assert meta["E"] == 256 and meta["gap_min"] == 1e-4
    assert [meta["cases"][n]["shapes"] for n in ("a0", "a1", "a2")] == [[[5, 7]], [[17, 33]], [[100, 100]]]
    assert [meta["cases"][n]["stats"][0]["num_pos"] for n in ("a0", "a1", "a2")] == [3, 6, 40]
    for name, case in meta["cases"].items():
        for st in case["stats"]:
            if st["mined"]:                     # a cut that decides something, by a margin far above fp32 rounding
                assert st["gap"] >= 1e-4 and st["nonzero"] > st["kept"] and st["kept"] == 3 * st["num_pos"], (name, st)
            else:
                assert not st["num_neg"] / (st["num_pos"] + 1) > 3, (name, st)
    assert meta["cases"]["e_nan"]["nan"] == [True] and meta["cases"]["e_pair_nan"]["nan"] == [False, True]
    assert np.isnan(z["e_nan.losses"]).all() and np.isnan(z["e_nan.g_key"]).all() and np.isnan(z["e_nan.g_ref"]).all()
    ks, rs = z["e_pair_nan.key_start"], z["e_pair_nan.ref_start"]
    assert np.isfinite(z["e_pair_nan.g_key"][:ks[1]]).all() and np.isnan(z["e_pair_nan.g_key"][ks[1]:]).all()
    assert np.isfinite(z["e_pair_nan.g_ref"][:rs[1]]).all() and np.isnan(z["e_pair_nan.g_ref"][rs[1]:]).all()
    assert z["e_one.losses"][0] == 0.0 and not meta["cases"]["e_nomine"]["stats"][0]["mined"]
    assert z["e_twopos.targets"].reshape(4, 6).sum(1).max() == 2 and 0.0 in z["e_unmatched.weights"]
    assert np.allclose(z["a_all.losses"], (z["a0.losses"] + z["a1.losses"] + z["a2.losses"]) / 3, rtol=1e-12)
    assert len(meta["head"]["params"]) == 16 and all(f"head.grad.{n}" in z for n in meta["head"]["params"])
    assert os.path.getsize(os.path.join(Hh.REPO, "tests", "golden", "track_train.npz")) < (1 << 20)


def test_loss_and_match_point_at_track_loss():
    head = _head()
    for fn in (head.loss, head.match):
        with pytest.raises(NotImplementedError, match="track_loss"):
            fn(None, None, None, None)


def test_loss_configs_are_read_for_their_numbers():
    head = _head(loss_track=dict(type="MultiPosCrossEntropyLoss", loss_weight=0.5),
                 loss_track_aux=dict(type="L2Loss", neg_pos_ub=2, pos_margin=0, neg_margin=0.3, hard_mining=True, loss_weight=2.0))
    cfg = head._track_loss_cfg(3, 256)
    assert (cfg.pairs, cfg.E, cfg.lw_track, cfg.lw_aux, cfg.neg_pos_ub, cfg.hard_mining) == (3, 256, 0.5, 2.0, 2, 1)
    assert cfg.pos_margin == 0.0 and abs(cfg.neg_margin - 0.3) < 1e-7
    with pytest.raises(NotImplementedError):
        _head(loss_track=dict(type="CrossEntropyLoss"))._track_loss_cfg(1, 256)
    with pytest.raises(NotImplementedError):
        _head(loss_track_aux=dict(type="L2Loss", sample_ratio=3, margin=0.3))._track_loss_cfg(1, 256)
    with pytest.raises(NotImplementedError, match="softmax_temp"):
        _head(softmax_temp=0.1, loss_track_aux=dict(type="L2Loss"))._track_loss_cfg(1, 256)
