"""CPU: the host side of the ground-truth preparation (polyphonicformer_amd/gt.py) against tests/golden/gt_prepare.npz, which
tools/gen_golden_gt_prepare.py made with the reference's own statements (polyphonic_former_video.py:114-138), and an fp32 numpy
restatement of the arithmetic contract of `ph_gt_prepare` (include/polyhead.h) that tests/test_gpu_gt_prepare.py compares the
kernel with.

What the restatement owes the fixture: bit for bit at the ratios 4 and 1 and in nearest mode; within 2^-23 with identical zero sets
at the non-integer ratio -- torch's CPU kernel contracts one product there (one rounding of a value <= 1: 2^-24 over 40 seeds at
five shapes when the fixture was made).  A difference near 1e-4 would mean the source coordinate went into an FMA."""
import ctypes as C
import json

import numpy as np
import pytest

import helpers as Hh
from polyphonicformer_amd import _lib, gt as GT

CASES = ("s4", "frac", "one", "near")
F32 = np.float32


def fixture():
    z = Hh.load_golden("gt_prepare.npz")
    return z, json.loads(str(z["meta"]))


def frame(z, name, f):
    """one frame's loader outputs and the reference's lists: the bitmasks are cut from the stored label map"""
    pre = f"{name}.{f}."
    labels = z[pre + "labels"]
    lmap = z[pre + "label_map"]
    d = {k: z[pre + k] for k in ("labels", "instance_ids", "gt_masks", "gt_labels", "gt_sem_seg", "gt_sem_cls", "gt_instance_ids", "valid")}
    d["label_map"] = lmap
    d["bitmasks"] = np.stack([lmap == i for i in range(len(labels))]).astype(np.uint8)
    return d


def call_args(z, meta, name):
    """the arguments of one `ph_gt_prepare` call for a case: seg [F, Hs, Ws], row_of [F, 256], nseg, depth [F, Hp, Wp], sizes, mode"""
    c = meta["cases"][name]
    nt = meta["num_thing_classes"]
    frames = [frame(z, name, f) for f in range(c["frames"])]
    split = [GT.split_rows(fr["labels"], nt) for fr in frames]
    gmax, smax = max(max(len(t) for t, _ in split), 1), max(len(s) for _, s in split)
    Hp, Wp = c["pad_hw"]
    return dict(seg=np.stack([fr["label_map"] for fr in frames]), row_of=np.stack([GT.row_table(fr["labels"], nt, gmax) for fr in frames]),
                nseg=[len(fr["labels"]) for fr in frames], depth=np.ascontiguousarray(z[f"{name}.depth"][:, 0]), src_hw=tuple(c["src_hw"]),
                pad_hw=(Hp, Wp), assign_hw=(Hp // c["stride"], Wp // c["stride"]), gmax=gmax, smax=smax, nearest=c["nearest"],
                G=[len(t) for t, _ in split], S=[len(s) for _, s in split], frames=frames)


# ---- the arithmetic contract of ph_gt_prepare in fp32 numpy (no FMA: every numpy operation rounds once) ---------------------------
def _bilinear_src(n_in, n_out):
    scale = F32(n_in) / F32(n_out)
    r = scale * (np.arange(n_out, dtype=F32) + F32(0.5)) - F32(0.5)
    r = np.maximum(r, F32(0))
    i0 = np.minimum(r.astype(np.int32), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    l1 = r - i0.astype(F32)
    return i0, i1, F32(1) - l1, l1


def _nearest_src(n_in, n_out):
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int32), n_in - 1)


def np_gt_prepare(seg, row_of, nseg, depth, src_hw, pad_hw, assign_hw, gmax, smax, nearest=False, **_):
    """-> dict(things [F, gmax, aH, aW], stuff [F, smax, aH, aW], things_hard, stuff_hard, valid [F, aH, aW], depth [F, aH, aW])"""
    F_, (Hs, Ws), (Hp, Wp), (aH, aW) = len(nseg), src_hw, pad_hw, assign_hw
    out = dict(things=np.zeros((F_, gmax, aH, aW), F32), stuff=np.zeros((F_, smax, aH, aW), F32), valid=np.zeros((F_, aH, aW), F32),
               depth=np.zeros((F_, aH, aW), F32))
    if nearest:
        y0 = y1 = _nearest_src(Hp, aH)
        x0 = x1 = _nearest_src(Wp, aW)
        h0, h1, w0, w1 = np.ones(aH, F32), np.zeros(aH, F32), np.ones(aW, F32), np.zeros(aW, F32)
    else:
        y0, y1, h0, h1 = _bilinear_src(Hp, aH)
        x0, x1, w0, w1 = _bilinear_src(Wp, aW)
    yn, xn = _nearest_src(Hp, aH), _nearest_src(Wp, aW)
    h0, h1 = h0[:, None], h1[:, None]
    for f in range(F_):
        table = np.asarray(row_of[f], np.int64).copy()
        table[nseg[f]:] = -1
        table[255] = -1
        table[(table < 0) | (table >= gmax + smax)] = -1
        padded = np.full((Hp, Wp), 255, np.uint8)
        padded[:Hs, :Ws] = seg[f]
        rows = table[padded]
        a, b, c, d = rows[y0][:, x0], rows[y0][:, x1], rows[y1][:, x0], rows[y1][:, x1]
        for r in range(gmax + smax):
            v = h0 * (w0 * (a == r).astype(F32) + w1 * (b == r).astype(F32)) + h1 * (w0 * (c == r).astype(F32) + w1 * (d == r).astype(F32))
            assert v.dtype == F32
            if r < gmax:
                out["things"][f, r] = v
            else:
                out["stuff"][f, r - gmax] = v
        out["depth"][f] = depth[f][yn][:, xn]
        out["valid"][f] = ((out["things"][f] != 0).any(0) | (out["stuff"][f] != 0).any(0)).astype(F32)
    out["things_hard"], out["stuff_hard"] = (out["things"] != 0).astype(F32), (out["stuff"] != 0).astype(F32)
    return out


# ---- tests --------------------------------------------------------------------------------------------------------------------------
def test_index_map_round_trips_the_fixture_masks():
    z, meta = fixture()
    for name in CASES:
        for f in range(meta["cases"][name]["frames"]):
            fr = frame(z, name, f)
            m = GT.index_map_from_bitmasks(fr["bitmasks"])
            assert m.dtype == np.uint8 and m.shape == fr["bitmasks"].shape[1:]
            for i in range(len(fr["bitmasks"])):
                assert np.array_equal(m == i, fr["bitmasks"][i] != 0), (name, f, i)
            assert np.array_equal(m == 255, fr["bitmasks"].sum(0) == 0) and (m == 255).any()
            assert np.array_equal(m, fr["label_map"])

            class Bitmap:                                   # a BitmapMasks-like object
                masks = fr["bitmasks"].astype(bool)
            assert np.array_equal(GT.index_map_from_bitmasks(Bitmap()), m)
    assert GT.index_map_from_bitmasks(np.zeros((0, 5, 7), np.uint8)).tolist() == np.full((5, 7), 255).tolist()


def test_index_map_refuses_overlap_and_255_masks():
    m = np.zeros((2, 4, 6), np.uint8)
    m[0, :2], m[1, 1:3] = 1, 1
    with pytest.raises(ValueError, match="overlap"):
        GT.index_map_from_bitmasks(m)
    many = np.zeros((255, 16, 16), np.uint8)
    many.reshape(255, -1)[np.arange(255), np.arange(255)] = 1
    with pytest.raises(ValueError, match="254"):
        GT.index_map_from_bitmasks(many)
    assert np.array_equal(GT.index_map_from_bitmasks(many[:254]).reshape(-1)[:254], np.arange(254))


def test_row_table_and_splits_equal_the_reference_lists():
    z, meta = fixture()
    nt = meta["num_thing_classes"]
    seen_dropped = seen_no_things = seen_empty = False
    for name in CASES:
        for f in range(meta["cases"][name]["frames"]):
            fr = frame(z, name, f)
            lab = fr["labels"]
            th, st = GT.split_rows(lab, nt)
            assert np.array_equal(lab[th], fr["gt_labels"]) and np.array_equal(lab[st], fr["gt_sem_cls"])
            assert np.array_equal(fr["instance_ids"][th], fr["gt_instance_ids"])
            gmax = len(th) + 3
            row = GT.row_table(lab, nt, gmax)
            assert row.dtype == np.int32 and row.shape == (256,)
            assert np.array_equal(row[th], np.arange(len(th))) and np.array_equal(row[st], gmax + np.arange(len(st)))
            rest = np.setdiff1d(np.arange(256), np.concatenate([th, st]))
            assert (row[rest] == -1).all() and row[255] == -1
            # the rows are the reference's masks: row r of the things is the mask of the r-th thing in loader order
            seen_dropped |= bool((lab < 0).any())
            seen_no_things |= len(th) == 0
            seen_empty |= any(not fr["bitmasks"][i].any() for i in th)
    assert seen_dropped and seen_no_things and seen_empty
    with pytest.raises(ValueError, match="254"):
        GT.split_rows(np.zeros(255, np.int64), nt)


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_reproduces_the_fixture(name):
    z, meta = fixture()
    a = call_args(z, meta, name)
    got = np_gt_prepare(**a)
    exact = name != "frac"
    worst = 0.0
    for f, fr in enumerate(a["frames"]):
        G, S = a["G"][f], a["S"][f]
        for mine, ref in ((got["things"][f, :G], fr["gt_masks"]), (got["stuff"][f, :S], fr["gt_sem_seg"])):
            assert mine.shape == ref.shape and ref.dtype == F32
            worst = max(worst, float(np.abs(mine.astype(np.float64) - ref).max()) if ref.size else 0.0)
            if exact:
                assert np.array_equal(mine, ref), (name, f)
            else:
                assert np.abs(mine.astype(np.float64) - ref).max(initial=0.0) <= 2.0 ** -23, (name, f)
                assert np.array_equal(mine == 0, ref == 0), (name, f)
        assert not got["things"][f, G:].any() and not got["stuff"][f, S:].any()
        assert np.array_equal(got["valid"][f], fr["valid"])
        assert np.array_equal(got["depth"][f], z[f"{name}.gt_depth"][f, 0])
    print(name, "largest |restatement - reference|", worst)
    if name == "s4":
        vals = set(np.unique(np.concatenate([got["things"].ravel(), got["stuff"].ravel()])).tolist())
        assert vals == {0.0, 0.25, 0.5, 0.75, 1.0}


def test_argument_errors_come_back_before_any_launch():
    """the checks of `ph_gt_prepare` run on the host before the first launch, so they answer on a machine without a GPU"""
    lib = _lib.load()
    fake = C.c_void_p(256)

    def call(nseg=(8, 8), Hs=60, Ws=90, Hp=64, Wp=96, aH=16, aW=24, gmax=5, smax=3, mode=0):
        n = (C.c_int32 * len(nseg))(*nseg)
        return lib.ph_gt_prepare(fake, fake, n, None, len(nseg), Hs, Ws, Hp, Wp, aH, aW, gmax, smax, mode, fake, fake, None, None, fake, None, None)

    for kw, word in ((dict(nseg=(8, 255)), "segments"), (dict(Hs=65), "Hs <= Hp"), (dict(Ws=97), "Hs <= Hp"), (dict(aH=0), "positive"),
                     (dict(Hs=0), "positive"), (dict(gmax=_lib.PH_ASSIGN_MAX + 1), "rows per stack"), (dict(gmax=0, smax=0), "rows per stack"),
                     (dict(mode=2), "mode"), (dict(nseg=()), "frames"), (dict(nseg=(1,) * 65), "frames")):
        assert call(**kw) == _lib.PH_EINVAL, kw
        err = Hh.last_error()
        assert err.startswith("ph_gt_prepare") and word in err, (kw, err)
    assert _lib.PH_GTPREP_MAX_SEGMENTS == 254 and _lib.PH_GTPREP_MAX_FRAMES == 64
