"""Association step, launch-only form against the Python chain, on one GPU:
`VideoAssociator.step_records` (native association plan) vs `VideoAssociator.step_device` per frame, for one 1024 x 2048 frame with
about 20 things and for an 8-frame clip.  Same process, alternating runs, wall time around the calls with a device synchronisation
at the end of each (both forms leave their maps on the device).  Prints one JSON line and writes it to --out.

    python tools/native_assoc_time.py --out profiles/native_assoc/assoc_time.json
"""
import argparse
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
from polyphonicformer_amd import video as V  # noqa: E402
from polyphonicformer_amd.panoptic import segments_from_records  # noqa: E402
from polyphonicformer_amd.registry import HEADS  # noqa: E402
import polyphonicformer_amd.track_head  # noqa: E402,F401

K, N_THING, N_STUFF = 119, 8, 11
CFG = dict(init_score_thr=0.35, obj_score_thr=0.3, match_score_thr=0.5, memo_tracklet_frames=5, memo_backdrop_frames=1,
           memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True, match_metric="bisoftmax")


def frame(seed, H, W, nthing, nstuff):
    pan, _, feats, _ = Hh.video_case(seed=seed, H=H, W=W, nseg=nthing + nstuff)
    ids = [i for i in np.unique(pan) if i > 0]
    out = np.zeros_like(pan)
    row = np.zeros(1 + 5 * K, dtype=np.int32)
    scores = np.full(K, 0.1, dtype=np.float32)
    for new, old in enumerate(ids):
        out[pan == old] = new + 1
        label = new % N_THING if new < nthing else N_THING + new % N_STUFF
        row[1 + 4 * new:5 + 4 * new] = (new + 1, new, label, int((pan == old).sum()))
        scores[new] = 0.5 + 0.4 * ((new * 7) % 10) / 10
    row[0] = len(ids)
    row[1 + 4 * K:] = scores.view(np.int32)
    return out, row, feats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--precision", default="fp32")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    head = HEADS.build(dict(type="QuasiDenseMaskEmbedHeadGTMask", norm_cfg=dict(type="GN", num_groups=32)))
    sd = Hh.seeded_fill(Hh.TRACK_HEAD_SHAPES, 4321)
    head.load_state_dict({k[len("track_head."):]: v for k, v in sd.items()})
    head.to(dev).eval()
    head.precision = a.precision
    H, W = 1024, 2048
    res = dict(command="python tools/native_assoc_time.py", precision=a.precision, map=[H, W], K=K, reps=a.reps)
    for B in (1, 8):
        frames = [frame(100 + b, H, W, 20, 8) for b in range(B)]
        infos = [segments_from_records(f[1], K, N_THING) for f in frames]
        pans = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
        recs = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
        levels = [torch.cat([f[2][l] for f in frames], 0).to(dev).contiguous() for l in range(4)]
        per_frame = [[lv[b:b + 1] for lv in levels] for b in range(B)]
        py = V.VideoAssociator(head, CFG, N_THING, N_STUFF)
        nat = V.VideoAssociator(head, CFG, N_THING, N_STUFF).use_native_plan(True, max_things=32)

        def run_py():
            for b in range(B):
                py.step_device(per_frame[b], pans[b], infos[b])

        def run_nat():
            nat.step_records(levels, pans, recs)
        t = {"step_device": [], "step_records": []}
        for it in range(a.reps + 3):
            for name, fn in (("step_device", run_py), ("step_records", run_nat)):      # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= 3:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        res[f"B{B}"] = dict(things_per_frame=[sum(s["isthing"] for s in i) for i in infos],
                            step_device_ms=round(statistics.median(t["step_device"]), 4),
                            step_records_ms=round(statistics.median(t["step_records"]), 4),
                            step_device_ms_min_max=[round(min(t["step_device"]), 4), round(max(t["step_device"]), 4)],
                            step_records_ms_min_max=[round(min(t["step_records"]), 4), round(max(t["step_records"]), 4)])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
