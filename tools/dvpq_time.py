"""DVPQ tallies on the device against the host evaluator, on one GPU: per-frame time of `ph_dvpq_frames` at 1024 x 2048 for B = 1 and
B = 8 (HIP events around the call, the maps already on the device), next to `dvps_eval.evaluate_clip` on the same frames (numpy, on
maps already in host memory: no download, no .pth round trip counted), and the achieved read rate at 16 B per pixel next to
`ph_selftest_readbw` on the same box.  The tables of the timed call are checked against the host metric before anything is timed.
Prints one JSON line and writes it to --out.

    python tools/dvpq_time.py --out profiles/dvpq/dvpq_time.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import helpers as Hh  # noqa: E402
from polyphonicformer_amd import _lib  # noqa: E402
from polyphonicformer_amd import dvps_eval as D  # noqa: E402

THRS = (0.5, 0.25, 0.1)


def events_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--capacity", type=int, default=8192)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    H, W = 1024, 2048
    frames = Hh.dvps_clip(seed=21, nseq=1, nframes=4, H=H, W=W)
    pr, gr = [D.wire_record(f["pred"]) for f in frames], [D.wire_record(f["gt"]) for f in frames]
    res = dict(command="python tools/dvpq_time.py", map=[H, W], capacity=a.capacity, thresholds=list(THRS), reps=a.reps, bytes_per_pixel=16)

    # the host evaluator on maps in memory: one window and threshold per call
    def host(k, thr, n=3):
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            D.evaluate_clip([{kk: np.array(v) for kk, v in r.items()} for r in pr[:k]], gr[:k], thr, 19)
            t.append(time.perf_counter() - t0)
        return round(statistics.median(t), 4)
    res["host_evaluate_clip_s"] = {"1_frame_thr0.5": host(1, 0.5), "4_frames_thr0.5": host(4, 0.5), "1_frame_no_thr": host(1, 0)}

    up = lambda recs, key, dtype, B: torch.from_numpy(np.stack([np.asarray(recs[b % 4][key]).astype(dtype) for b in range(B)])).to(dev)
    for B in (1, 8):
        cfg = _lib.DvpqCfg(B=B, H=H, W=W, capacity=a.capacity, nthr=len(THRS))
        for j, t in enumerate(THRS):
            cfg.thr[j] = t
        need = lib.ph_dvpq_workspace_bytes(C.byref(cfg))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        pp, gp = up(pr, "panseg", np.int64, B).to(torch.int32), up(gr, "panseg", np.int64, B).to(torch.int32)
        pd, gd = up(pr, "depth", np.float32, B), up(gr, "depth", np.float32, B)
        table = torch.empty(B, 4 + 4 * a.capacity, dtype=torch.int32, device=dev)
        drec = torch.empty(B, 8, dtype=torch.float64, device=dev)
        io = _lib.DvpqIO(pred_panseg=_lib.ptr(pp), pred_depth=_lib.ptr(pd), gt_panseg=_lib.ptr(gp), gt_depth=_lib.ptr(gd),
                         table_out=_lib.ptr(table), depth_out=_lib.ptr(drec))
        run = lambda: _lib.check(lib.ph_dvpq_frames(C.byref(cfg), C.byref(io), _lib.ptr(ws), need, _lib.stream_ptr()), "ph_dvpq_frames")
        run()
        torch.cuda.synchronize()
        t = table.cpu().numpy().view(np.uint32)
        assert not t[:, 1].any(), "overflow"
        tabs = [t[b, 4:4 + 4 * t[b, 0]].reshape(-1, 4) for b in range(B)]
        for thr in (0,) + THRS:            # the timed call computes what the host computes
            want = D.evaluate_clip([{kk: np.array(v) for kk, v in pr[0].items()}], gr[:1], thr, 19)
            got = D.clip_tallies(tabs[:1], THRS.index(thr) if thr > 0 else None, 19)
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), thr
        ms = events_ms(run, a.reps)
        med = statistics.median(ms)
        t0 = time.perf_counter()
        for thr in (0,) + THRS:
            for k in (1, 2, 3, 4):
                if k <= B:
                    D.clip_tallies(tabs[:k], THRS.index(thr) if thr > 0 else None, 19)
        host_tail = time.perf_counter() - t0
        res[f"B{B}"] = dict(rows_per_frame=[int(x) for x in t[:, 0]], call_ms=round(med, 4), call_ms_min_max=[round(min(ms), 4), round(max(ms), 4)],
                            per_frame_ms=round(med / B, 4), read_TBps=round(16.0 * H * W * B / (med * 1e-3) / 1e12, 3),
                            host_clip_tallies_all_windows_thresholds_s=round(host_tail, 5))
    buf = torch.randint(0, 2 ** 31 - 1, (16 * H * W * 8 // 4,), dtype=torch.int32, device=dev)          # the bytes of the B = 8 call
    out = torch.zeros(4, dtype=torch.int32, device=dev)
    ms = events_ms(lambda: lib.ph_selftest_readbw(_lib.ptr(buf), buf.numel() * 4, 4096, _lib.ptr(out), _lib.stream_ptr()), a.reps)
    res["selftest_readbw_TBps_same_bytes_as_B8"] = round(buf.numel() * 4 / (statistics.median(ms) * 1e-3) / 1e12, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
