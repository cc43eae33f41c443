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

  * with --train-out, INSTEAD of the sections above: forward + backward of the trained stages (frozen_stages=1, norm_eval=True) at
    B = 2 and B = 4 (--train-batches), gradients of randn on all four stages.  First, device path only, the weight-gradient kernel
    alone per layer group (every ph_conv_cl_bwd_weight launch of layer2 / layer3 / layer4 on the plan's own planes, the fold backward
    not included) with its TFLOP/s from 2 K Cout per output pixel, and the data gradient likewise (plus its three stride-2 3x3
    layers by themselves); then three sides alternating in one process: the device path
    (`train_on_device()`: module forward, `torch.autograd.backward`), torch fp32 NCHW, torch bf16 autocast on channels-last.

  * with --handoff-out, INSTEAD of the sections above: the backbone's hand-over to the FPN, the NCHW form (`fpn(backbone(img))`:
    ph_cl_to_nchw writes fp32 NCHW stages, ph_fpn_lateral reads them) beside the direct one (`fpn(backbone.forward_planes(img))`:
    ph_fpn_lateral_cl reads the backbone's planes), same method, grades 'bf16' and 'fp16', B = 1 and B = 4: backbone + FPN through
    the module calls (GPU time and the host's wall time per call); the four laterals alone in both forms and the four NCHW
    conversions alone, with the bytes each moves per second; the device memory of the backbone plan in both forms.

The result is written to --out after every section, so a run that is cut short leaves what it measured.

    python tools/resnet_time.py --out profiles/resnet/time.json
    python tools/resnet_time.py --native-out profiles/resnet/native_time.json
    python tools/resnet_time.py --train-out profiles/resnet/train_time.json
    python tools/resnet_time.py --handoff-out profiles/resnet/handoff_time.json
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


def train_section(dev, batches, reps, warmup, out):
    """forward + backward of the trained stages: the weight-gradient kernel per layer group, then the three sides; written to `out`
    after every part"""
    from polyphonicformer_amd import train as T
    res = {"command": "python tools/resnet_time.py --train-out OUT", "workload": "ResNet-50 (frozen_stages=1, norm_eval=True) of 1024 x 2048 "
           "fp32 images, forward + backward from randn gradients on the four fp32 NCHW stages to the 126 trained parameters' gradients; HIP "
           "events around forward + backward, the three sides alternate in one process; wgrad_groups / dgrad_groups: every "
           "ph_conv_cl_bwd_weight / ph_conv_cl_bwd_data launch of a layer group alone (2 K Cout per output pixel; the data gradient counts "
           "what it issues, stride2_conv2 = the three stride-2 3x3 layers, which issue 4 x their useful work)", "reps": reps, "warmup": warmup}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)

    def fresh():
        m = ResNet(50, frozen_stages=1, norm_eval=True)
        m.load_state_dict(resnet_cases.fill(m.state_dict()))
        return m.to(dev).train()
    m_dev, m_f32, m_cl = fresh().train_on_device(), fresh(), fresh().to(memory_format=torch.channels_last)

    def step(m, x, ups, autocast=False):
        for p in m.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            outs = m(x)
        pairs = [(o, u.to(o.dtype)) for o, u in zip(outs, ups) if o.requires_grad]           # torch: layer1's stage is frozen
        torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])

    for B in batches:
        x = resnet_cases.inputs(1, (B, 3, H, W))[0].to(dev)
        xcl = x.contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            shapes = [tuple(o.shape) for o in m_dev.eval()(x)]
        m_dev.train()
        g = torch.Generator().manual_seed(11)
        ups = [torch.randn(s, generator=g).to(dev) for s in shapes]
        step(m_dev, x, ups)                                        # builds the packs and the plan
        plan = T._resnet_train_state(m_dev, x)[0]
        res[f"B{B}"] = {"plan_bytes": plan.nbytes}
        groups, gflop = {}, {}
        for si in (1, 2, 3):
            calls = []
            for (s_, j, name, k, st, ci, co, hh, ww) in plan.sizes["layers"]:
                if s_ != si:
                    continue
                kp = plan.kept[(s_, j)]
                dz = {"conv1": kp["a1"], "conv2": kp["a2"], "conv3": kp["y"], "downsample": kp["y"]}[name]     # a plane of dZ's size
                xin = {"conv1": plan.inputs[(s_, j)], "conv2": kp["a1"], "conv3": kp["a2"], "downsample": plan.inputs[(s_, j)]}[name]
                calls.append((dz, xin, plan.nsplit[(s_, j, name)], k, st, hh, ww, ci, co))
                gflop[si] = gflop.get(si, 0.0) + 2.0 * k * k * ci * co * E.conv_out_size(hh, k, st) * E.conv_out_size(ww, k, st) * B / 1e9
            groups[f"layer{si + 1}"] = (lambda cs=calls: [E.conv_cl_bwd_weight(dz, xin, plan.dwp, plan.dbp, plan.partial, ns, k, st, B, hh, ww,
                                                                               ci, co) for dz, xin, ns, k, st, hh, ww, ci, co in cs])
        t = alternate(groups, reps, warmup)
        for si in (1, 2, 3):
            t[f"layer{si + 1}"]["tflops"] = round(gflop[si] / t[f"layer{si + 1}"]["ms"], 1)
            t[f"layer{si + 1}"]["gflop"] = round(gflop[si], 1)
        res[f"B{B}"]["wgrad_groups"] = t
        flush()
        # the data gradient alone: every ph_conv_cl_bwd_data launch of a layer group with the plan's own operands, and the three
        # stride-2 3x3 layers by themselves (their MFMAs run all nine taps: issued = 4 x useful)
        wt, ix = T._resnet_train_state(m_dev, x)[2], plan.index
        dgroups, dgf, s2_calls, s2_gf = {}, {}, [], 0.0
        for si in (1, 2, 3):
            calls = []
            for j, (cin, planes, st, has_down) in enumerate(plan.blocks[si]):
                (h, w, ho, wo), kp, xin = plan.geo[(si, j)], plan.kept[(si, j)], plan.inputs[(si, j)]
                calls.append((kp["y"], wt[ix[(si, j, "conv3")]], None, 1, kp["a2"], plan.d2, 1, 1, ho, wo, planes, 4 * planes))
                c2 = (kp["a2"], wt[ix[(si, j, "conv2")]], None, 1, kp["a1"], plan.d1, 3, st, h, w, planes, planes)
                calls.append(c2)
                if st == 2:
                    s2_calls.append(c2)
                    s2_gf += 2.0 * 9 * planes * planes * h * w * B / 1e9
                if (si, j) == (1, 0):
                    continue                                       # layer2.0: nothing trained in front of it
                if has_down:
                    calls.append((kp["y"], wt[ix[(si, j, "downsample")]], None, 1, None, plan.dt, 1, 1, ho, wo, cin, 4 * planes))
                    calls.append((kp["a1"], wt[ix[(si, j, "conv1")]], plan.dt, st, None, plan.ga, 1, 1, h, w, cin, planes))
                else:
                    calls.append((kp["a1"], wt[ix[(si, j, "conv1")]], kp["y"], 1, xin, plan.ga, 1, 1, h, w, cin, planes))
            dgf[si] = sum(2.0 * k * k * co * ci * hh * ww * B / 1e9 for (_, _, _, _, _, _, k, _, hh, ww, ci, co) in calls)
            dgroups[f"layer{si + 1}"] = calls
        dgroups["stride2_conv2"] = s2_calls
        run_d = lambda cs: [E.conv_cl_bwd_data(dz, w_, r, rs, mk, o, k, st, B, hh, ww, ci, co) for dz, w_, r, rs, mk, o, k, st, hh, ww, ci, co in cs]
        t = alternate({name: (lambda cs=cs: run_d(cs)) for name, cs in dgroups.items()}, reps, warmup)
        for si in (1, 2, 3):
            t[f"layer{si + 1}"]["gflop_issued"] = round(dgf[si], 1)
            t[f"layer{si + 1}"]["tflops_issued"] = round(dgf[si] / t[f"layer{si + 1}"]["ms"], 1)
        t["stride2_conv2"]["gflop_issued"], t["stride2_conv2"]["gflop_useful"] = round(s2_gf, 1), round(s2_gf / 4, 1)
        res[f"B{B}"]["dgrad_groups"] = t
        flush()
        runs = {"device_bf16": lambda: step(m_dev, x, ups), "torch_fp32_nchw": lambda: step(m_f32, x, ups),
                "torch_bf16_autocast_channels_last": lambda: step(m_cl, xcl, ups, autocast=True)}
        res[f"B{B}"].update(alternate(runs, reps, warmup))
        flush()
        m_dev.__dict__.pop("_train_state", None)
        torch.cuda.empty_cache()


def handoff_section(m, dev, batches, reps, warmup, out):
    """backbone + FPN and the laterals alone, NCHW hand-over beside the direct one; written to `out` after every part"""
    import helpers
    from polyphonicformer_amd.fpn import FPN
    res = {"command": "python tools/resnet_time.py --handoff-out OUT", "workload": "ResNet-50 + FPN of a 1024 x 2048 fp32 image -> four fp32 "
           "NCHW levels.  nchw: fpn(backbone(img)) -- fp32 NCHW stages between them; planes: fpn(backbone.forward_planes(img)) -- "
           "ph_fpn_lateral_cl on the backbone's 16-bit channels-last planes.  The sides alternate in one process; gpu = HIP events around "
           "the call, host = wall time of the call itself with the queue empty before it.  laterals: the four lateral launches alone "
           "(to_nchw: the four ph_cl_to_nchw launches the nchw form needs in front of them); gbytes = stage read + output planes written "
           "+ coarse planes read once + weights, gb_per_s from it.  plan_bytes: the backbone plan's device memory", "reps": reps, "warmup": warmup}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
    fpn = FPN([256, 512, 1024, 2048], 256, 4)
    fpn.load_state_dict(helpers.seeded_fill({k: tuple(v.shape) for k, v in fpn.state_dict().items()}, 17))
    fpn.eval().to(dev)
    with torch.no_grad():
        for grade in ("bf16", "fp16"):
            mg = copy.deepcopy(m).set_precision(grade)
            fpn.set_precision(grade)
            prec = E.KHEAD_PREC[grade]
            for B in batches:
                x = resnet_cases.inputs(1, (B, 3, H, W))[0].to(dev)
                r = res[f"{grade}_B{B}"] = {}
                r["backbone_fpn"] = alternate_host({"nchw": lambda: fpn(mg(x)), "planes": lambda: fpn(mg.forward_planes(x))}, reps, warmup)
                g = r["backbone_fpn"]
                g["planes_over_nchw_gpu"] = round(g["planes"]["gpu"]["ms"] / g["nchw"]["gpu"]["ms"], 4)
                flush()
                # the laterals alone, on the stages of one run in both forms and the FPN plan's own lateral planes
                pk, fpk = mg._pack(dev), fpn._pack(dev)
                rplan = mg._plan_of(x, stage_planes=True)[0]
                stages = rplan.run(x, pk)
                shapes = rplan.stage_shapes
                fplan = fpn._plan_of(stages)[0]
                r["plan_bytes"] = {"nchw": mg._plan_of(x)[0].bytes(), "planes_with_nchw_stages": rplan.bytes(),
                                   "planes": rplan.bytes() - sum(t.numel() * t.element_size() for t in rplan.outs.values())}

                def lateral(lvl, cl):
                    c = fpk["lateral"][lvl]
                    coarse, chw = (fplan.lat[lvl + 1], fplan.shapes[lvl + 1]) if lvl < 3 else (None, None)
                    if cl:
                        E.fpn_lateral_cl(rplan.stage_plane(lvl), prec, shapes[lvl][1:], c["wp"], c["bias"], coarse, chw, fplan.lat[lvl], prec)
                    else:
                        E.fpn_lateral(stages[lvl], c["wp"], c["bias"], coarse, chw, fplan.lat[lvl], prec)

                def to_nchw(lvl):
                    k, h, w = shapes[lvl]
                    E.cl_to_nchw(rplan.stage_plane(lvl), stages[lvl], B, h * w, k, prec)
                runs = {"to_nchw": lambda: [to_nchw(l) for l in (3, 2, 1, 0)],
                        "lateral_nchw": lambda: [lateral(l, False) for l in (3, 2, 1, 0)],
                        "lateral_cl": lambda: [lateral(l, True) for l in (3, 2, 1, 0)]}
                for l in range(4):
                    runs[f"lateral_nchw_level{l}"] = (lambda l=l: lateral(l, False))
                    runs[f"lateral_cl_level{l}"] = (lambda l=l: lateral(l, True))
                t = alternate(runs, reps, warmup)

                def gbytes(lvl, esz):
                    k, h, w = shapes[lvl]
                    coarse = B * fplan.shapes[lvl + 1][0] * fplan.shapes[lvl + 1][1] * 256 * 2 if lvl < 3 else 0
                    return (B * k * h * w * esz + B * h * w * 256 * 2 + coarse + 256 * k * 2) / 1e9
                for name, esz in (("lateral_nchw", 4), ("lateral_cl", 2)):
                    per = [gbytes(l, esz) for l in range(4)]
                    for key, gb in [(name, sum(per))] + [(f"{name}_level{l}", per[l]) for l in range(4)]:
                        t[key]["gbytes"] = round(gb, 4)
                        t[key]["gb_per_s"] = round(gb / t[key]["ms"] * 1e3, 1)
                gb = sum(B * k * h * w * (2 + 4) for k, h, w in shapes) / 1e9
                t["to_nchw"]["gbytes"], t["to_nchw"]["gb_per_s"] = round(gb, 4), round(gb / t["to_nchw"]["ms"] * 1e3, 1)
                r["laterals"] = t
                flush()
                mg._plans.clear(); fpn._plans.clear()
                del rplan, fplan, stages
                torch.cuda.empty_cache()


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
    ap.add_argument("--train-out", default=None, help="measure forward + backward of the trained stages instead")
    ap.add_argument("--train-batches", default="2,4")
    ap.add_argument("--handoff-out", default=None, help="measure the backbone -> FPN hand-over, NCHW stages beside stage planes, instead")
    ap.add_argument("--fpn-neck-ms", type=float, default=1.07, help="the FPN + neck's time per frame to set the backbone beside")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    if args.train_out:
        return train_section(dev, [int(b) for b in args.train_batches.split(",")], args.reps, args.warmup, args.train_out)
    m = ResNet(50, frozen_stages=1, norm_eval=True)
    m.load_state_dict(resnet_cases.fill(m.state_dict()))
    m.eval().to(dev)
    if args.handoff_out:
        return handoff_section(m, dev, [int(b) for b in args.batches.split(",")], args.reps, args.warmup, args.handoff_out)
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
