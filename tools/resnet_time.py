"""The ResNet-50 backbone at the flagship size (1024 x 2048 image -> stages 256x512x256 .. 32x64x2048), B = 1 and B = 4, one process,
HIP events around the calls, median and min .. max of --reps after warm-up.  The two grades of
the device path and the two torch forms take turns inside every repetition; the per-group section follows them:

  * `resnet.ResNet.forward` (the module call) on the device in each grade ('bf16', 'fp16'), fp32 NCHW stages out,
  * the same module in torch: `_forward_torch` in fp32 NCHW, and under bf16 autocast with channels-last input and weights
    (the input converted before the timed window),
  * in a section of its own after those four have alternated, device path only: per layer group (stem, layer1..4) the time of that
    group's launches alone (`ResNetPlan.run_stem` / `run_stage`, without `forward`'s host work) and the achieved TFLOP/s from
    2 K Cout per output pixel -- twice the multiply-add count -- (the stem counted with K = 147; the NCHW conversion is inside its
    layer's window),
  * the whole backbone beside the FPN + neck's time (--fpn-neck-ms, DESIGN.md 7f7: 1.07 ms),
  * with --native-out, INSTEAD of the sections above: the native plan beside the Python plan, same method (HIP events, median of
    --reps after --warmup, alternating in one process): per B the GPU time and the host wall time per call (the time the call takes to
    return, the queue empty before it) of `NativeResNetPlan.run` (one native call) and `ResNetPlan.run` (57 ctypes calls) on the same
    pack; and the weight load from a resident fp32 state_dict, wall time to the finished pack: `ph_resnet_pack` (engine.
    native_resnet_pack) against `ResNet._pack` (host float64).

The result is written to --out after every section, so a run that is cut short leaves what it measured.

    python tools/resnet_time.py --out profiles/resnet/time.json
    python tools/resnet_time.py --native-out profiles/resnet/native_time.json
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import resnet_cases  # noqa: E402
from polyphonicformer_amd import engine as E  # noqa: E402
from polyphonicformer_amd.resnet import ResNet  # noqa: E402

H, W = 1024, 2048


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def alternate(runs, reps, warmup):
    samples = {k: [] for k in runs}
    for rep in range(warmup + reps):
        for k, fn in runs.items():
            t = event_ms(fn)
            if rep >= warmup:
                samples[k].append(t)
    return {k: summary(v) for k, v in samples.items()}


def alternate_host(runs, reps, warmup, sync_inside=False):
    """`alternate` with the host's wall time beside the GPU's: {name: {"gpu": summary, "host": summary}}.  The queue is empty when a
    call starts; `sync_inside`: the wall time runs to the end of the call's GPU work (a weight load), not to its return (a launch call)"""
    gpu, host = {k: [] for k in runs}, {k: [] for k in runs}
    for rep in range(warmup + reps):
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            if sync_inside:
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rep >= warmup:
                gpu[k].append(a.elapsed_time(b))
                host[k].append((t1 - t0) * 1e3)
    return {k: {"gpu": summary(gpu[k]), "host": summary(host[k])} for k in runs}


def native_section(m, dev, batches, reps, warmup, out):
    """the native plan beside the Python plan, and the two weight loads; written to `out` after every part"""
    res = {"command": "python tools/resnet_time.py --native-out OUT", "workload": "ResNet-50 of a 1024 x 2048 fp32 image -> four fp32 NCHW "
           "stages, grade bf16: NativeResNetPlan.run (one native call) and ResNetPlan.run (57 ctypes calls) on the same pack alternate in "
           "one process; gpu = HIP events around the call, host = wall time of the call itself with the queue empty before it.  pack: "
           "wall time from a resident fp32 state_dict to the finished device pack", "reps": reps, "warmup": warmup}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
    m = copy.deepcopy(m).set_precision("bf16")
    with torch.no_grad():
        cfg = E.native_resnet_cfg(1, H, W, 50, "bf16")
        pack = E.native_resnet_pack(m, cfg, dev)
        for B in batches:
            x = resnet_cases.inputs(1, (B, 3, H, W))[0].to(dev)
            native = E.NativeResNetPlan(pack, B, H, W, dev)
            python = E.ResNetPlan(B, H, W, m.block_table(), (0, 1, 2, 3), E.KHEAD_PREC["bf16"], torch.float32, dev)
            res[f"B{B}"] = alternate_host({"native_plan_run": lambda: native.run(x), "python_plan_run": lambda: python.run(x, pack.pk)},
                                          reps, warmup)
            del native, python
            torch.cuda.empty_cache()
            flush()
        sd = {k: v.detach().float().to(dev) for k, v in m.state_dict().items()}

        def python_pack():
            m._packs.clear()
            m._pack(dev)
        res["pack"] = alternate_host({"ph_resnet_pack": lambda: E.native_resnet_pack(sd, cfg, dev), "ResNet._pack": python_pack}, reps, warmup,
                                     sync_inside=True)
        flush()


def group_gflop(m):
    """GFLOP per frame of the stem and of each layer: 2 K Cout per output pixel"""
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = {"stem": 2 * 147 * 64 * h * w / 1e9}
    h, w = E.stem_out_size(H), E.stem_out_size(W)
    for si, stage in enumerate(m.block_table()):
        f = 0
        for cin, planes, s, down in stage:
            ho, wo = E.conv_out_size(h, 3, s), E.conv_out_size(w, 3, s)
            f += 2 * (cin * planes * h * w + 9 * planes * planes * ho * wo + planes * 4 * planes * ho * wo + (cin * 4 * planes * ho * wo if down else 0))
            h, w = ho, wo
        out[f"layer{si + 1}"] = f / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch forms")
    ap.add_argument("--native-out", default=None, help="measure the native plan beside the Python plan, and the two weight loads, instead")
    ap.add_argument("--fpn-neck-ms", type=float, default=1.07, help="the FPN + neck's time per frame to set the backbone beside")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    m = ResNet(50, frozen_stages=1, norm_eval=True)
    m.load_state_dict(resnet_cases.fill(m.state_dict()))
    m.eval().to(dev)
    if args.native_out:
        return native_section(m, dev, [int(b) for b in args.batches.split(",")], args.reps, args.warmup, args.native_out)
    gf = group_gflop(m)
    res = {"command": "python tools/resnet_time.py", "workload": "ResNet-50 of a 1024 x 2048 image: fp32 NCHW image -> four fp32 NCHW stages; "
           "HIP events around the calls; ResNet.forward in both grades and the two torch forms alternate in one process, the per-group times are a separate section on ResNetPlan's steps", "reps": args.reps, "warmup": args.warmup,
           "gflop_per_frame": {k: round(v, 2) for k, v in gf.items()}, "gflop_per_frame_total": round(sum(gf.values()), 1),
           "fpn_neck_ms_per_frame": args.fpn_neck_ms}

    def flush():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    batches = [int(b) for b in args.batches.split(",")]
    xs = {B: resnet_cases.inputs(1, (B, 3, H, W))[0].to(dev) for B in batches}
    mods = {grade: copy.deepcopy(m).set_precision(grade) for grade in ("bf16", "fp16")}
    mcl = copy.deepcopy(m).to(memory_format=torch.channels_last)
    with torch.no_grad():
        for B in batches:
            x = xs[B]
            xcl = x.contiguous(memory_format=torch.channels_last)

            def bf16_cl(xi=xcl):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return mcl._forward_torch(xi)
            # ONE alternation per B: the two grades of `forward` (the module call: version check, plan lookup and launches) and the two
            # torch forms take turns inside every repetition, so drift and other load fall on all four alike
            runs = {f"device_{grade}": (lambda mg=mg, xi=x: mg(xi)) for grade, mg in mods.items()}
            if not args.no_torch:
                runs["torch_fp32_nchw"] = (lambda xi=x: m._forward_torch(xi))
                runs["torch_bf16_autocast_channels_last"] = bf16_cl
            res[f"B{B}"] = alternate(runs, args.reps, args.warmup)
            for grade in mods:
                ms = res[f"B{B}"][f"device_{grade}"]["ms"]
                res[f"B{B}"][f"device_{grade}"]["tflops"] = round(sum(gf.values()) * B / ms, 1)
                res[f"B{B}"][f"device_{grade}"]["ms_per_frame_over_fpn_neck"] = round(ms / B / args.fpn_neck_ms, 2)
            print(flush(), flush=True)
            # a section of its own, device path only: the plan's steps (ResNetPlan.run_stem / run_stage, launches without forward's host
            # work), in order within a repetition -- each group runs on what the one before it left
            for grade, mg in mods.items():
                plan, pk, xin = mg._plan_of(x)
                groups = {"stem": (lambda p=plan, k=pk, xi=xin: p.run_stem(xi, k))}
                for si in range(4):
                    groups[f"layer{si + 1}"] = (lambda p=plan, k=pk, s=si: p.run_stage(s, k))
                t = alternate(groups, args.reps, args.warmup)
                for g, v in t.items():
                    v["tflops"] = round(gf[g] * B / v["ms"], 1)
                res[f"B{B}"][f"groups_{grade}"] = t
                mg._plans.clear()
            torch.cuda.empty_cache()
            print(flush(), flush=True)
    print(flush())


if __name__ == "__main__":
    main()
