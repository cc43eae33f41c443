"""Association step with the device tracker against the host tracker, on one GPU: `run + track` (ph_assoc_plan_run +
ph_assoc_plan_track: launches only) vs `run + match` (ph_assoc_plan_run + ph_assoc_plan_match: the host walk and its
synchronisations), for one 1024 x 2048 frame with 20 things and for an 8-frame call, plus the replay of `run + track` captured
into one graph.  Same process, alternating runs, median wall time around the calls INCLUDING the final device synchronisation.
The two trackers see the same stream, so their memories grow alike.  Prints one JSON line and writes it to --out.

    python tools/device_tracker_time.py --out profiles/device_tracker/track_time.json
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
from native_assoc_time import CFG, K, N_STUFF, N_THING, frame  # noqa: E402
from polyphonicformer_amd import engine as E, tracker as TR, video as V  # noqa: E402
from polyphonicformer_amd.registry import HEADS  # noqa: E402
import polyphonicformer_amd.track_head  # noqa: E402,F401


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
    pack = E.native_track_pack(head, E.native_track_cfg(head), dev)
    H, W, cap = 1024, 2048, 32
    res = dict(command="python tools/device_tracker_time.py", precision=a.precision, map=[H, W], K=K, max_things=cap, reps=a.reps)
    for B in (1, 8):
        frames = [frame(100 + b, H, W, 20, 8) for b in range(B)]
        pans = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
        recs = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
        levels = [torch.cat([f[2][l] for f in frames], 0).to(dev).contiguous() for l in range(4)]
        cfg = E.native_assoc_cfg(B, (H, W), K, cap, N_THING, N_STUFF, [tuple(f.shape[-2:]) for f in levels], pack.cfg)
        plans = [E.NativeAssocPlan(pack, cfg, dev) for _ in range(3)]                  # host path, device path, captured device path
        host = V.QuasiDenseEmbedTracker(**CFG)
        native = host.native_tracker(dev)
        dts = [TR.NativeDeviceTracker(TR.native_tracker_cfg(**CFG), dev, 4096, 128) for _ in range(2)]
        cnt = [1]

        def run_match():
            plans[0].run(pans, recs, levels)
            cnt[0] += plans[0].match(native, pans, cnt[0])[2]

        def run_track():
            plans[1].run(pans, recs, levels)
            plans[1].track(dts[0], pans)

        plans[2].run(pans, recs, levels)                                              # warm-up outside the capture
        plans[2].track(dts[1], pans)
        dts[1].reset(1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            plans[2].run(pans, recs, levels)
            plans[2].track(dts[1], pans)
        t = {"run_match": [], "run_track": [], "graph_replay": []}
        for it in range(a.reps + 3):
            for name, fn in (("run_match", run_match), ("run_track", run_track), ("graph_replay", g.replay)):      # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= 3:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        same = bool(torch.equal(plans[0].track_map, plans[1].track_map) and torch.equal(plans[1].track_map, plans[2].track_map))
        st = dts[0].status()
        res[f"B{B}"] = dict(things_per_frame=plans[1].things[:, 0].tolist(), same_maps=same, frames_matched=st["matched"], error=st["error"],
                            **{k + "_ms": round(statistics.median(v), 4) for k, v in t.items()},
                            **{k + "_ms_min_max": [round(min(v), 4), round(max(v), 4)] for k, v in t.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
