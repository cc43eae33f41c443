"""Host and GPU time of one eager module-API decode with and without the native plan (KernelUpdateIterHead.use_native_plan),
and the time of the native stage packing (ph_decode_pack_stage).

    python tools/native_plan_time.py [--calls 100] [--precision fp16]

One B = 1, cfg3-shaped call of `simple_test_mask_preds` (fp32 features in, as the video leg hands them over): `host_us` is
the wall time of the call itself (median; the launches are queued, the GPU is not waited for), `gpu_us` the time between two
events around it (median).  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import bench  # noqa: E402
from polyphonicformer_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--precision", default="fp16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    wl = bench.WORKLOADS["cfg3"]
    N = wl["Nq"] + wl["n_stuff"]
    out_dtype = torch.float16 if a.precision in ("fp16", "mixed16") else torch.float32
    head = bench.build_head(wl, a.precision, out_dtype, dev, seed=3)
    head.frame_invariant = True          # the module API's default
    g = {k: v.to(dev) for k, v in bench.synth_inputs(wl, 1, seed=5).items()}
    meta = [bench_meta(wl)]

    def call():
        return head.simple_test_mask_preds(g["x"], g["k0"].reshape(1, N, 256, 1, 1), g["m0"], None, meta, depth_feats=g["dfe"],
                                           depth_proposal=g["q0"].reshape(1, N, 256, 1, 1))

    for native in (False, True):
        head.use_native_plan(native)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        host, gpu = [], []
        for _ in range(a.calls):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            e.record()
            torch.cuda.synchronize()
            host.append((t1 - t0) * 1e6)
            gpu.append(s.elapsed_time(e) * 1e3)
        print(json.dumps({"what": "module API decode, B=1 cfg3", "precision": a.precision, "native_plan": native,
                          "calls": a.calls, "host_us_median": round(statistics.median(host), 1),
                          "gpu_us_median": round(statistics.median(gpu), 1)}), flush=True)
    head.use_native_plan(False)

    # the packing kernel: one cfg2 stage (L = 133), once per weight load
    wl2 = dict(bench.WORKLOADS["cfg2"], S=1)
    h2 = bench.build_head(wl2, "fp32", torch.float32, dev, seed=4)
    for mode in ("fp32", "fp16", "bf16"):
        cfg = E.native_cfg(1, wl2["Nq"] + wl2["n_stuff"], wl2["H"], wl2["W"], 1, wl2["n_thing"] + wl2["n_stuff"], wl2["F"], mode)
        E.native_pack_stage(h2.mask_head[0], cfg, dev)
        ts = []
        for _ in range(10):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            E.native_pack_stage(h2.mask_head[0], cfg, dev)
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) * 1e3)
        print(json.dumps({"what": "ph_decode_pack_stage, one cfg2 stage incl. the fp32 parameter copies", "mode": mode,
                          "gpu_us_median": round(statistics.median(ts), 1)}), flush=True)


def bench_meta(wl):
    return dict(img_shape=(wl["H"] * 8, wl["W"] * 8, 3), ori_shape=(wl["H"] * 8, wl["W"] * 8, 3),
                batch_input_shape=(wl["H"] * 8, wl["W"] * 8))


if __name__ == "__main__":
    main()
