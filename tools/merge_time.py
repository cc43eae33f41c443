"""Times the panoptic merge of B frames at the cfg2 size (1024x2048, N = 153, one geometry): `get_panoptic` in a loop over the
frames (per-image host accept loop) against `get_panoptic_batch` (one launch-only native call, accept step on the device), for
B = 1, 4, 8, 16, in ONE process.  Inputs as bench.py's panoptic leg arranges them: the mask / depth logits an un-trained head
decodes from synthetic features, synthetic class scores (40 thing queries and every stuff class above instance_score_thr) and
overlap_thr 0, so that tens of segments are accepted.  Host wall time and GPU time (events), median of 30 runs after warm-up.

    python tools/merge_time.py [--loop-only] [--out FILE]

`--loop-only` times the per-image loop alone and touches nothing newer than `get_panoptic`: run from a checkout of an earlier
commit it gives that commit's figure (the baseline the batched form is compared with)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from polyphonicformer_amd import panoptic as Pn  # noqa: E402
from polyphonicformer_amd.registry import ConfigDict  # noqa: E402

BATCHES, RUNS, WARM = (1, 4, 8, 16), 30, 3


def inputs(wl, B, dev):
    head = bench.build_head(wl, "bf16", torch.bfloat16, dev, seed=0)
    head.test_cfg = ConfigDict(max_per_img=wl["Nq"], merge_stuff_thing=dict(overlap_thr=0.0, instance_score_thr=0.3))
    N, L, nt = wl["Nq"] + wl["n_stuff"], wl["n_thing"] + wl["n_stuff"], wl["n_thing"]
    inp = {k: v.to(dev) for k, v in bench.synth_inputs(wl, B, seed=1).items()}
    o = head._decode(inp["x"], inp["k0"].reshape(B, N, 256, 1, 1), inp["m0"], inp["dfe"], inp["q0"].reshape(B, N, 256, 1, 1))
    g = torch.Generator().manual_seed(17)
    cls = 0.01 + 0.01 * torch.arange(B * N * L, dtype=torch.float64).reshape(B, N, L) / (N * L) / B    # background: no exact ties, so
    cls = cls.float()                                                     # that topk's and the device selection's orders agree
    for b in range(B):
        hot = torch.randperm(wl["Nq"], generator=g)[:40]
        cls[b, hot, torch.randint(0, nt, (40,), generator=g)] = 0.35 + 0.6 * torch.rand(40, generator=g)
        sidx = torch.arange(wl["n_stuff"])
        cls[b, wl["Nq"] + sidx, nt + sidx] = 0.4 + 0.5 * torch.rand(wl["n_stuff"], generator=g)
    d0 = torch.randn(B, 1, 2 * wl["H"], 2 * wl["W"], generator=g).to(dev)
    torch.cuda.synchronize()
    return head, cls.to(dev), o["mask_up"].clone(), o["depth_up"].clone(), d0


def timed(fn):
    """median host wall ms and GPU ms of fn() (which ends synchronised)"""
    for _ in range(WARM):
        fn()
    wall, gpu = [], []
    for _ in range(RUNS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        gpu.append(s.elapsed_time(e))
    return round(statistics.median(wall), 3), round(statistics.median(gpu), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wl = bench.WORKLOADS["cfg2"]
    H, W = wl["H"] * 8, wl["W"] * 8
    meta = dict(img_shape=(H, W, 3), ori_shape=(H, W, 3), batch_input_shape=(H, W))
    head, cls, mm, dd, d0 = inputs(wl, max(BATCHES), dev)
    res = {"workload": f"cfg2 merge, {H}x{W}, N = {cls.shape[1]}, K = {wl['Nq'] + wl['n_stuff']} candidates, bf16 logits", "runs": RUNS,
           "device": torch.cuda.get_device_name(0), "rows": []}
    for B in BATCHES:
        out = {}

        def loop():
            out["loop"] = [Pn.get_panoptic(head, cls[b], mm[b], dd[b], d0[b], meta) for b in range(B)]

        row = {"B": B}
        row["loop_wall_ms"], row["loop_gpu_ms"] = timed(loop)
        row["segments_per_frame"] = [len(r[2][1]) for r in out["loop"]]
        if not args.loop_only:
            metas = [meta] * B

            def batch():
                out["batch"] = Pn.get_panoptic_batch(head, cls[:B], mm[:B], dd[:B], d0[:B], metas)

            row["batch_wall_ms"], row["batch_gpu_ms"] = timed(batch)
            row["same_id_maps"] = all((a[2][0] == b[2][0]).all() and a[2][1] == b[2][1] for a, b in zip(out["loop"], out["batch"]))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
