"""DVPQ from per-frame tallies (dvps_eval.clip_tallies / depth_errors_from_tallies) against the metric on whole maps and the goldens
of the unmodified reference evaluator, and the host side of ph_dvpq_frames (include/polyhead.h): its refusals.
No GPU: nothing here launches a kernel (tests/test_gpu_dvpq.py does)."""
import ctypes as C
import json
import os

import numpy as np

import helpers as Hh
from polyphonicformer_amd import _lib
from polyphonicformer_amd import dvps_eval as D

THRS = (0.5, 0.25, 0.1)
FAKE_PTR = 1 << 40          # a 256-byte aligned address that a refused call never dereferences


def _records(frames):
    return [D.wire_record(f["pred"]) for f in frames], [D.wire_record(f["gt"]) for f in frames]


def test_clip_tallies_equal_evaluate_clip_bit_for_bit():
    """every window, threshold and clip of dvps_clip(seed=21): IoU sums and tp / fn / fp counts"""
    frames = Hh.dvps_clip(seed=21)
    pr, gr = _records(frames)
    tables = [D.frame_table(p, g, THRS) for p, g in zip(pr, gr)]
    assert all(t.dtype == np.uint32 and 10 < len(t) < 200 for t in tables)
    n = 0
    for k in (1, 2, 3, 4):
        for idx in range(len(frames) - k + 1):
            if frames[idx]["seq"] != frames[idx + k - 1]["seq"]:
                continue
            for thr in (0,) + THRS:
                want = D.evaluate_clip([{kk: np.array(v) for kk, v in r.items()} for r in pr[idx:idx + k]], gr[idx:idx + k], thr, 19)
                got = D.clip_tallies(tables[idx:idx + k], THRS.index(thr) if thr > 0 else None, 19)
                for a, b in zip(got, want):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (k, idx, thr)
                n += 1
    assert n == 4 * (10 + 8 + 6 + 4)


def test_dvpq_from_frames_equals_video_evaluate(tmp_path):
    frames = Hh.dvps_clip(seed=21)
    for fr in frames:
        D.save_record(str(tmp_path), fr["seq"], fr["img"], fr["pred"], "pred")
        D.save_record(str(tmp_path), fr["seq"], fr["img"], fr["gt"], "gt")
    want = D.video_evaluate(str(tmp_path), num_classes=19, num_things=8)
    pr, gr = _records(frames)
    rows = [(f["seq"], f["img"], D.frame_table(p, g, THRS)) for f, p, g in zip(frames, pr, gr)]
    assert D.dvpq_from_frames(rows[::-1], 19, 8) == want             # any order in, (seq, img) order scored


def test_vpq_eval_still_equals_the_golden():
    gold = Hh.load_golden("dvps_vpq.npz")
    for i, fr in enumerate(Hh.dvps_clip(seed=21)[:6]):
        p, g = D.wire_record(fr["pred"])["panseg"], D.wire_record(fr["gt"])["panseg"]
        assert np.array_equal(np.stack(D.vpq_eval(p, g, num_classes=19)), gold[f"frame{i}"]), i
        assert np.array_equal(np.stack(D.clip_tallies([D.frame_table(D.wire_record(fr["pred"]), D.wire_record(fr["gt"]))], None, 19)),
                              gold[f"frame{i}"]), i


def test_depth_errors_from_tallies():
    g = json.load(open(os.path.join(Hh.GOLDEN, "dvps_eval.json")))["depth_errors"]
    rows = [D.depth_tallies(f["pred"]["depth"], f["gt"]["depth"]) for f in Hh.dvps_clip(seed=21)]
    got = D.depth_errors_from_tallies(rows)
    assert sorted(got) == sorted(g)
    for k, v in g.items():
        print(k, float(got[k]), v, abs(float(got[k]) - v))
        assert abs(float(got[k]) - v) <= 1e-6 * max(1.0, abs(v)), k


def test_relabelling_and_the_zero_key():
    """one gt segment, two pred ids, one pixel over the threshold: the relabelled pixel leaves its segment; key (0, 0, 0) counts"""
    t = np.array([[0, 0, 0, 5], [0, 0, 1, 1], [0, 7, 0, 2]], dtype=np.uint32)
    a = D.clip_tallies([t], None, 19)
    b = D.vpq_eval(np.array([0] * 6 + [7] * 2), np.zeros(8, dtype=np.int64), num_classes=19)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    a = D.clip_tallies([t], 0, 19)
    b = D.vpq_eval(np.array([0] * 5 + [190000] + [7] * 2), np.zeros(8, dtype=np.int64), num_classes=19)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _cfg(**kw):
    base = dict(B=2, H=32, W=64, capacity=256, nthr=3)
    base.update(kw)
    c = _lib.DvpqCfg(**base)
    for j, t in enumerate(THRS):
        c.thr[j] = t
    return c


def test_refusals_come_before_any_launch():
    """every call below would fault on its fake addresses if it launched"""
    lib = _lib.load()
    msg = lambda: lib.ph_last_error_string().decode()
    need = lib.ph_dvpq_workspace_bytes(C.byref(_cfg()))
    assert need > 0 and need % 256 == 0
    assert lib.ph_dvpq_workspace_bytes(C.byref(_cfg(capacity=8192))) > need

    def io(**kw):
        o = _lib.DvpqIO()
        for k in ("pred_panseg", "pred_depth", "gt_panseg", "gt_depth", "table_out", "depth_out"):
            setattr(o, k, kw.get(k, FAKE_PTR))
        o.pred_sem, o.pred_track = kw.get("pred_sem"), kw.get("pred_track")
        return o

    for kw, word in ((dict(capacity=100), "capacity"), (dict(capacity=32), "capacity"), (dict(capacity=1 << 17), "capacity"),
                     (dict(nthr=9), "nthr"), (dict(nthr=-1), "nthr"), (dict(B=0), "B, H, W"), (dict(H=1 << 16, W=1 << 15), "2^31")):
        assert lib.ph_dvpq_workspace_bytes(C.byref(_cfg(**kw))) == 0 and word in msg(), (kw, msg())
        assert lib.ph_dvpq_frames(C.byref(_cfg(**kw)), C.byref(io()), C.c_void_p(FAKE_PTR), 1 << 40, None) == -1 and word in msg(), (kw, msg())
    run = lambda ws=FAKE_PTR, nbytes=need, **kw: lib.ph_dvpq_frames(C.byref(_cfg()), C.byref(io(**kw)), C.c_void_p(ws), nbytes, None)
    assert run(nbytes=need - 1) == -4 and "workspace too small" in msg()
    assert run(ws=FAKE_PTR + 16) == -1 and "256-byte" in msg()
    assert run(ws=None) == -1 and "workspace" in msg()
    assert run(gt_depth=None) == -1 and "gt_depth" in msg()
    assert run(pred_panseg=None) == -1 and "pred_sem" in msg()
    assert run(pred_panseg=None, pred_sem=FAKE_PTR) == -1 and "pred_track" in msg()
    assert run(pred_panseg=None, pred_sem=FAKE_PTR, pred_track=FAKE_PTR + 4) == -1 and "8-byte" in msg()
    assert run(gt_panseg=FAKE_PTR + 2) == -1 and "4-byte" in msg()
    assert run(table_out=FAKE_PTR + 4) == -1 and "16-byte" in msg()
    assert run(table_out=None) == -1 and "table_out" in msg()
