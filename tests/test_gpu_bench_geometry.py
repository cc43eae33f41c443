"""GPU: the launches bench.py times, against the oracle.

The benchmark runs `simple_test_mask_preds` as 16- to 48-frame parts on skewed streams inside one HIP graph
(engine.DualDecodePlan, every part `shares_gpu`).  At that size DecodePlan picks another launch geometry than the one- to
eight-frame plans of the other oracle tests: the widest query row tiling (PH_QUERY_WIDE), the fused conv + pooling between the
stages (ph_dynconv_poolx) with its own pixel split, a pooling split of 4 and the fused final stage at 1.5 workgroups per CU.
Each case below builds its runner exactly as bench.mode_leg / bench.main do, for every leg the default run and `--all-legs`
time, and
  * asserts the geometry every part chose (literals: a rule change that moves the timed geometry fails here on purpose);
  * runs the step once eagerly, recording the hard masks every stage pooled with (DecodePlan.debug_bits);
  * captures and replays the HIP graph and asserts that the replay reproduces the eager run bit for bit, so the oracle check
    below is a check of what the bench replays;
  * compares the first and last frame of the step and of the first part with the oracle on the same 16-bit-rounded inputs,
    following the device's hard masks (tests/test_gpu_configs.py: TOL_IDENT and the element-wise criterion); frames from
    different parts also check the slicing of the inputs into parts and the concatenation of the outputs."""
import pytest
import torch

import bench
import helpers as Hh
from oracle import poly_oracle as O
from polyphonicformer_amd import engine as E
from test_gpu_configs import ATOL_FRAC_FREE, TOL_IDENT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

OUT_DT = {"bf16": torch.bfloat16, "mixed": torch.float16, "mixed16": torch.float16, "fp16": torch.float16, "fp32": torch.float32}
# every part's geometry: pooling split, fused conv + pooling (and its split), fused final stage (and the workgroup count stages()
# gives it, in CUs * 3/2: 384 on a 256-CU MI355X), query rows per workgroup of the PH_QUERY_WIDE rule (ph_query.hip query_run)
_FUSED = dict(nsplit=4, nsplit_px=8, poolx=True, fused_up=True, up2_wgs_per_2cu=3, query_rows=80)
_TWO_PLANE = dict(nsplit=4, nsplit_px=8, poolx=False, fused_up=False, up2_wgs_per_2cu=None, query_rows=80)    # hi + lo kernels
CASES = [
    # id, workload, mode, frames per step, parts, fp32 features through ingest, mask_bias, geometry of every part
    ("cfg2-mixed16-headline", "cfg2", "mixed16", 128, 4, False, 0.0, _FUSED),
    ("cfg2-fp16", "cfg2", "fp16", 128, 4, False, 0.0, _FUSED),
    ("cfg2-bf16", "cfg2", "bf16", 128, 4, False, 0.0, _FUSED),
    ("cfg2-mixed", "cfg2", "mixed", 128, 4, False, 0.0, _TWO_PLANE),
    ("cfg2-fp32", "cfg2", "fp32", 32, 2, False, 0.0, dict(nsplit=8, nsplit_px=16, poolx=False, fused_up=False, up2_wgs_per_2cu=None,
                                                         query_rows=80)),
    # N = 253 > 192: no fused pooling; W = 156: no fused final stage; Npad = 256: 4 row tiles of 16
    ("cfg5-fp16", "cfg5", "fp16", 192, 4, False, 0.0, dict(nsplit=2, nsplit_px=5, poolx=False, fused_up=False, up2_wgs_per_2cu=None,
                                                          query_rows=64)),
    ("cfg5-fp16-fp32-features", "cfg5", "fp16", 192, 4, True, 0.0, dict(nsplit=2, nsplit_px=5, poolx=False, fused_up=False,
                                                                        up2_wgs_per_2cu=None, query_rows=64)),
    ("cfg2-mixed16-sparse-masks", "cfg2", "mixed16", 128, 4, False, -2.0, _FUSED),
]


def _final_stage_wgs(p):
    """the fused final stage's workgroup count as DecodePlan.stages() passes it to ph_dynconv_up2_wgs (0 = one per CU);
    None where the plan runs the two-kernel final stage"""
    if not p.fused_up:
        return None
    return p.up2_shared_wgs if (getattr(p, "shares_gpu", False) and p.B * p.H >= 4 * p.up2_shared_wgs) else 0


def _wide_query_rows(Npad):
    """rows per workgroup of a PH_QUERY_WIDE query launch: 16 x the largest of 5, 4, 3, 2 that divides Npad / 16"""
    t = Npad // 16
    return 16 * next((c for c in (5, 4, 3, 2) if t % c == 0), 1)


def _inputs(wl, mode, B, fp32_inputs, mask_bias, dev, seed):
    """bench.mode_leg's input formats, drawn on the device: 16-bit feature tensors in the mode's plane dtype (fp32 for the fp32
    mode or through ingest), the initial mask logits in the output dtype with 16-bit features"""
    N, H, W = wl["Nq"] + wl["n_stuff"], wl["H"], wl["W"]
    fdt = E.MODES[mode].feat_dtype
    sixteen = fdt is not None and not fp32_inputs
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn((B, 256, H, W), generator=g, device=dev, dtype=fdt if sixteen else torch.float32)
    dfe = torch.randn((B, 256, H, W), generator=g, device=dev, dtype=fdt if sixteen else torch.float32)
    k0 = torch.randn((B, N, 256), generator=g, device=dev)
    q0 = torch.randn((1, 1, 256), generator=g, device=dev).expand(B, N, 256)
    m0 = torch.randn((B, N, H, W), generator=g, device=dev) + mask_bias
    if sixteen and OUT_DT[mode] != torch.float32:
        m0 = m0.to(OUT_DT[mode])
    return x, dfe, k0, q0, m0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bench_step_geometry_and_oracle(gpu, monkeypatch, case):
    name, wln, mode, B, parts, fp32_inputs, mask_bias, geo = case
    for k in ("PH_POOL_NSPLIT", "PH_CONV_UP2", "PH_CONV_POOLX", "PH_POOLX_NSPLIT", "PH_UP2_SHARED_WGS"):
        monkeypatch.delenv(k, raising=False)           # the bench's geometry is the default one
    wl = bench.WORKLOADS[wln]
    N, H, W, S = wl["Nq"] + wl["n_stuff"], wl["H"], wl["W"], wl["S"]
    out_dtype = OUT_DT[mode]
    # -- the runner, as bench.mode_leg builds it
    head = bench.build_head(wl, mode, out_dtype, gpu)
    assert head.frame_invariant is False
    packs = head._plan(B // parts, N, H, W, gpu).packs
    head._plans.clear()                                # the single-stream plan is not part of the timed step
    runner = E.DualDecodePlan(packs, B, N, H, W, E.MODES[mode], out_dtype, gpu, parts=parts)
    sd = {k: v.detach().cpu() for k, v in head.state_dict().items()}
    del head
    # -- the geometry every part chose
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = B // parts
    assert runner.sizes == [n] * parts
    seen = []
    for p in runner.halves:
        got = dict(B=p.B, shares_gpu=getattr(p, "shares_gpu", False), nsplit=p.nsplit, nsplit_px=p.nsplit_px, poolx=p.poolx,
                   fused_up=p.fused_up, up2_wgs=_final_stage_wgs(p), query_rows=_wide_query_rows(E.n_padded(N)))
        want = dict(B=n, shares_gpu=True, nsplit=geo["nsplit"], nsplit_px=geo["nsplit_px"], poolx=geo["poolx"], fused_up=geo["fused_up"],
                    up2_wgs=None if geo["up2_wgs_per_2cu"] is None else geo["up2_wgs_per_2cu"] * cus // 2, query_rows=geo["query_rows"])
        assert got == want, (name, got, want)
        seen.append(got)
    if geo["fused_up"] and cus == 256:
        assert seen[0]["up2_wgs"] == 384
    print(f"\n{name}: {parts} parts x {n} frames, geometry of every part {seen[0]} ({cus} CUs)")
    # -- inputs as the bench hands them over
    x, dfe, k0, q0, m0 = _inputs(wl, mode, B, fp32_inputs, mask_bias, gpu, seed=99)
    runner.set_inputs(x, dfe, k0, q0, m0)
    # -- one eager step, recording the hard masks every stage of every part pooled with
    for p in runner.halves:
        p.debug_bits = []
    runner.run()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in runner.outputs().items() if v is not None}
    assert eager["mask_up"].shape == (B, N, 2 * H, 2 * W) and eager["mask"].dtype == out_dtype
    frames = sorted({0, n - 1, n, B - 1})
    hard = {}
    for f in frames:
        p, i = runner.halves[f // n], f % n
        assert len(p.debug_bits) == S
        hard[f] = Hh.unpack_hard_masks([b[i:i + 1] for b in p.debug_bits], N, H, W)
    for p in runner.halves:
        p.debug_bits = None
    # -- the graph the bench replays: poison the outputs, replay, the eager step's values bit for bit
    runner.capture()
    torch.cuda.synchronize()
    for p in runner.halves:
        bufs = [p.mask, p.mask_up, p.depth_up] + [p.stage_out[-1][k] for k in ("obj", "dobj", "cls")]
        if not p.fused_up:
            bufs.append(p.depth)
        for t in bufs:
            t.fill_(float("nan"))
    runner.replay()
    torch.cuda.synchronize()
    replayed = runner.outputs()
    for k, v in eager.items():
        assert torch.equal(replayed[k], v), (name, k)
    del replayed, runner
    # -- the checked frames against the oracle, on the inputs the device consumed and its hard masks
    rd = E.MODES[mode].feat_dtype              # fp32 features: the ingest kernel rounds them to this plane format (None: fp32 planes)
    tol = TOL_IDENT[mode]
    worst, worst_at, worst_flip = {}, {}, 0.0
    for f in frames:
        xo, do = x[f:f + 1].float().cpu(), dfe[f:f + 1].float().cpu()
        if rd is not None:
            xo, do = xo.to(rd).float(), do.to(rd).float()
        m0o = m0[f:f + 1].float().cpu()
        ref = O.iter_head_mask_preds(sd, S, xo, k0[f:f + 1].cpu(), m0o, q0[f:f + 1].cpu(), do, hard_masks=hard[f], return_stages=True)
        flips = [float((hard[f][0] != O.binarize(m0o)).float().mean())] + \
                [float((hard[f][s + 1] != O.binarize(ref["stages"][s]["mask"])).float().mean()) for s in range(S - 1)]
        assert flips[0] == 0.0, (name, f)                        # binarising the given logits is exact
        worst_flip = max(worst_flip, max(flips))
        for k in ("obj", "cls", "mask", "mask_up", "depth_up"):
            got = eager[k][f:f + 1].float().cpu()
            e, at = Hh.rel_err(got, ref[k]), Hh.needed_atol(got, ref[k], tol)
            worst[k], worst_at[k] = max(worst.get(k, 0.0), e), max(worst_at.get(k, 0.0), at)
            assert e < tol, (name, f, k, e)
            assert at < ATOL_FRAC_FREE * tol, (name, f, k, at)
    print(f"{name}: frames {frames} vs the oracle on the device's hard masks: largest rel err",
          {k: f"{v:.1e}" for k, v in worst.items()}, f"| needed atol / max|b| at rtol = {tol:g}",
          {k: f"{v:.1e}" for k, v in worst_at.items()}, f"| largest stage-input flip rate {worst_flip:.1e}")
    assert worst_flip < {"fp32": 1e-3, "mixed": 1e-3, "bf16": 5e-2}.get(mode, 5e-3), (name, worst_flip)
    del eager, x, dfe, k0, q0, m0
    torch.cuda.empty_cache()
