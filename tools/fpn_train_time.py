"""GPU: forward + backward of the FPN in training, the library's nodes (`train.fpn_forward_train`) against torch's ops
(`FPN._forward_torch`) on the same fp32 stages: 2 images of 1024 x 2048 (stages 256 / 512 / 1024 / 2048 channels at strides 4 .. 32).
Both paths run in one process, alternating, HIP events around each forward + backward, the median of 25.  Also the wide
map x map^T product alone at the four levels' (K, HW), with the bytes per second it must move (one read of both operands).

usage: python tools/fpn_train_time.py [--out profiles/fpn/train_time.json] [--reps 25] [--height 1024 --width 2048]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphonicformer_amd import train as T  # noqa: E402
from polyphonicformer_amd.fpn import FPN  # noqa: E402

CH = (256, 512, 1024, 2048)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.images
    sizes = [(a.height >> (2 + l), a.width >> (2 + l)) for l in range(4)]
    g = torch.Generator().manual_seed(0)
    fpn = FPN(list(CH), 256, 4)
    fpn.init_weights()
    fpn.to(dev).train()
    stages = [torch.randn(B, c, h, w, generator=g).relu().to(dev).requires_grad_(True) for c, (h, w) in zip(CH, sizes)]
    cots = [torch.randn(B, 256, h, w, generator=g).to(dev) for h, w in sizes]

    def step(forward):
        for t in list(fpn.parameters()) + stages:
            t.grad = None
        with torch.enable_grad():
            torch.autograd.backward(forward(stages), cots)

    paths = {"device": lambda s: T.fpn_forward_train(fpn, s), "torch": fpn._forward_torch}
    for _ in range(2):
        for f in paths.values():
            step(f)
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(a.reps):
        for k, f in paths.items():
            ms[k].append(timed(lambda: step(f)))
    res = dict(images=B, image_size=[a.height, a.width], level_sizes=sizes, reps=a.reps, device=torch.cuda.get_device_name(0),
               fwd_bwd_ms={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in ms.items()})
    res["device_over_torch"] = round(res["fwd_bwd_ms"]["device"]["median"] / res["fwd_bwd_ms"]["torch"]["median"], 3)
    wide = []
    for c, (h, w) in zip(CH, sizes):
        G, X = torch.randn(B, 256, h, w, generator=g).to(dev), torch.randn(B, c, h, w, generator=g).to(dev)
        rs = torch.empty(256, device=dev)
        run = lambda: T.map_x_mapT_wide(G, X, rowsum=rs, sum_batch=True)
        run(); run()
        torch.cuda.synchronize()
        t = statistics.median(timed(run) for _ in range(a.reps))
        nbytes = B * (256 + c) * h * w * 4
        wide.append(dict(K=c, HW=h * w, ms=round(t, 4), bytes=nbytes, GBps=round(nbytes / t / 1e6, 1)))
    res["wide_product"] = wide
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
