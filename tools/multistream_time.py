"""S live video streams on one GPU: one launch sequence for the S current frames against the single-stream objects run S times.

(a) the tracker alone: one `NativeDeviceTrackerBank.step` of S streams against S sequential `NativeDeviceTracker.run` calls, S in
    --streams (default 1 4 16), 20 detections per frame against a memory of a few hundred columns (three warm-up frames of 100
    objects each per stream; every detection starts a tracklet that lives for the whole run: 300 rows growing to ~760), bisoftmax;
(b) the whole step at 1024 x 2048 (the fp16 cfg3 pipeline of tests/test_gpu_video.py): `MultiStreamRunner.step` of S streams against
    S `VideoStreamRunner.run_one` calls in turn (graph replay of the heads, one slot each) -- the parent's way of serving S cameras --,
    S in --step-streams (default 4).

Same process, alternating, HIP events around the calls, medians and min .. max after warm-up; the host time of the calls is recorded
next to the event time.  Both sides of (b) end with their downloads and a synchronisation, so event and host time nearly agree there.

Prints one JSON line and writes it to --out.

    python tools/multistream_time.py --out profiles/multistream/time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import helpers  # noqa: E402
from polyphonicformer_amd import tracker as TR, video as V  # noqa: E402

CAPACITY, MAX_DETS, WARM_OBJECTS, DETS = 1024, 128, 100, 20


def event_ms(fn):
    """(GPU milliseconds between events around fn(), host milliseconds fn() took to return)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def summary(samples, frames):
    ev, host = [s[0] for s in samples], [s[1] for s in samples]
    ms = statistics.median(ev)
    return {"ms_per_step": round(ms, 4), "ms_min_max": [round(min(ev), 4), round(max(ev), 4)], "host_ms": round(statistics.median(host), 4),
            "frames_per_s": round(frames / ms * 1e3, 1)}


def frame_tables(S, n, seed, dev):
    """S frames of n well separated detections with fresh identities: boxes [S, MAX_DETS, 5], labels, counts, embeds"""
    g = torch.Generator().manual_seed(seed)
    boxes, labels = torch.zeros(S, MAX_DETS, 5), torch.randint(0, 8, (S, MAX_DETS), generator=g, dtype=torch.int32)
    xy = torch.rand(S, n, 2, generator=g) * 40 + (torch.arange(n, dtype=torch.float32) * 300)[None, :, None]
    boxes[:, :n, :2], boxes[:, :n, 2:4], boxes[:, :n, 4] = xy, xy + 120, 0.5 + 0.5 * torch.rand(S, n, generator=g)
    embeds = torch.zeros(S, MAX_DETS, 256)
    embeds[:, :n] = torch.randn(S, n, 256, generator=g)
    return boxes.to(dev), labels.to(dev), torch.full((S,), n, dtype=torch.int32).to(dev), embeds.to(dev)


def tracker_alone(S, reps, warmup, dev):
    # every detection starts a tracklet (scores are 0.5 .. 1) and tracklets live for the whole run: 300 rows + 20 per timed frame
    cfg = TR.native_tracker_cfg(match_metric="bisoftmax", init_score_thr=0.35, obj_score_thr=0.3, memo_tracklet_frames=1000)
    bank = TR.NativeDeviceTrackerBank(cfg, dev, S, CAPACITY, MAX_DETS)
    solos = [TR.NativeDeviceTracker(cfg, dev, CAPACITY, MAX_DETS) for _ in range(S)]
    out_b = bank.step(*frame_tables(S, 1, 0, dev))
    out_s = [t.run(*(x[:1] for x in frame_tables(1, 1, 0, dev))) for t in solos]
    bank.reset()
    for t in solos:
        t.reset(1)
    for f in range(3):                                            # the memory: 3 x 100 tracklets per stream
        tabs = frame_tables(S, WARM_OBJECTS, 100 + f, dev)
        bank.step(*tabs, out=out_b)
        for s, t in enumerate(solos):
            t.run(*(x[s:s + 1] for x in tabs), out=out_s[s])
    samples = {"bank_step": [], "single_trackers_in_turn": []}
    for rep in range(warmup + reps):
        tabs = frame_tables(S, DETS, 1000 + rep, dev)
        per = [tuple(x[s:s + 1] for x in tabs) for s in range(S)]
        a = event_ms(lambda: bank.step(*tabs, out=out_b))
        b = event_ms(lambda: [t.run(*per[s], out=out_s[s]) for s, t in enumerate(solos)])
        if rep >= warmup:
            samples["bank_step"].append(a)
            samples["single_trackers_in_turn"].append(b)
    rows = [bank.status(s)["rows"] for s in range(S)]
    assert rows == [t.status()["rows"] for t in solos] and all(bank.status(s)["error"] == 0 for s in range(S))
    res = {k: summary(v, S) for k, v in samples.items()}
    res.update(streams=S, detections=DETS, memory_rows_at_the_end=rows[0])
    return res


def whole_step(S, reps, warmup, dev):
    import test_gpu_video as GV
    pipe, _, _, wl = GV._cfg3_pipeline(dev, precision="fp16")
    H8, W8 = wl["H"] * 8, wl["W"] * 8
    meta = helpers.img_meta(H8, W8)
    g = torch.Generator().manual_seed(5)
    base = [[torch.randn(1, 256, H8 // s, W8 // s, generator=g).to(dev) for s in (4, 8, 16, 32)] for _ in range(S)]
    frames = lambda f: [tuple(torch.roll(t, (f, 2 * f), dims=(2, 3)) for t in base[s]) for s in range(S)]
    multi = V.MultiStreamRunner(pipe, meta, S)
    singles = [V.VideoStreamRunner(pipe, meta, pipelined=False) for _ in range(S)]
    samples = {"multi_stream_step": [], "single_stream_runners_in_turn": []}
    for rep in range(warmup + reps):
        fr = frames(rep)
        x = tuple(torch.cat([fr[s][l] for s in range(S)], 0) for l in range(4))
        a = event_ms(lambda: multi.step(x))
        b = event_ms(lambda: [r.run_one(fr[s]) for s, r in enumerate(singles)])
        if rep >= warmup:
            samples["multi_stream_step"].append(a)
            samples["single_stream_runners_in_turn"].append(b)
    res = {k: summary(v, S) for k, v in samples.items()}
    res.update(streams=S, frame=[H8, W8], refused=[multi.device_status(s)["error"] for s in range(S)])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--step-streams", type=int, nargs="*", default=[4])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multistream_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    res = {"command": "python tools/multistream_time.py", "reps": args.reps, "warmup": args.warmup,
           "how": "same process, alternating, HIP events around the calls, medians",
           "tracker_alone": [tracker_alone(S, args.reps, args.warmup, dev) for S in args.streams],
           "whole_step_1024x2048_fp16": [whole_step(S, args.reps, args.warmup, dev) for S in args.step_streams]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
