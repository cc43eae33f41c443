"""GPU: the paired depth pooling of DecodePlan's last two stages -- ph_pool_depth_pair (one read of depth_feats under two mask
sets), the query kernels' one-branch launches (PH_QUERY_MASK_ONLY / PH_QUERY_DEPTH_ONLY) and the plan that strings them together.
Nothing here has a tolerance: the pixel split, the chunk order and the MFMA order of every row are those of the unpaired
sequence, so every comparison is torch.equal."""
import pytest
import torch

import bench
from polyphonicformer_amd import _lib, engine as E

pytestmark = pytest.mark.gpu
SENTINEL = 7.5          # what the x halves (columns 0 .. 255) of the partial sums hold before the pooling: it must still be there


# ---- ph_pool_depth_pair against two ph_pool_counts launches on the depth plane -------------------------------------------------
def _mask_rows(B, N, HW, seed, gpu):
    """random mask bits for every padded row, with an all-zero and an all-one row inside the first and inside the last row tile"""
    g = torch.Generator().manual_seed(seed)
    Npad, words = E.n_padded(N), E.hw_padded(HW) // 32
    bits = torch.randint(-2 ** 31, 2 ** 31, (B, Npad, words), generator=g, dtype=torch.int64).to(torch.int32)
    bits[:, 0], bits[:, 1] = 0, -1
    bits[:, N - 1], bits[:, N - 2] = 0, -1
    return bits.to(gpu)


@pytest.mark.parametrize("prec,dt", [(_lib.PH_PREC_BF16, torch.bfloat16), (_lib.PH_PREC_F16, torch.float16)], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", [33, 111, 153, 160])
@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("HW", [512, 2048])
def test_pool_depth_pair_equals_two_depth_poolings(gpu, HW, nsplit, N, prec, dt):
    """N = 33 .. 160: 2 x 2 .. 2 x 5 row tiles (4 or 5 mask-word DMA instructions at 2 x 5: wave 0 carries two); pixel ranges of
    uneven chunk-pair counts (HW = 512: 8 chunks over 3 ranges), one range, ranges longer than the 4-deep ring (HW = 2048)"""
    assert _lib.load().ph_pool_depth_pair_supported(N, prec) == 1
    B, Npad = 2, E.n_padded(N)
    g = torch.Generator().manual_seed(HW + N)
    dp = torch.randn((B, 256, HW), generator=g).to(dt).view(torch.int16)[None].contiguous().to(gpu)
    bits = [_mask_rows(B, N, HW, 11 * N + s, gpu) for s in (0, 1)]
    bits[1][:, 2:4] = bits[0][:, 2:4]                       # and two rows the sets share
    new = lambda: (torch.full((B, nsplit, Npad, 512), SENTINEL, device=gpu), torch.full((B, nsplit, Npad), -1, dtype=torch.int32, device=gpu))
    ref, got = [new(), new()], [new(), new()]
    for (part, cnt), b in zip(ref, bits):
        E.pool_depth_only(dp, b, N, HW, prec, part, cnt)
    E.pool_depth_pair(dp, bits[0], bits[1], N, HW, prec, got[0][0], got[1][0], got[0][1], got[1][1])
    torch.cuda.synchronize()
    for s in (0, 1):
        assert torch.equal(got[s][0][..., 256:], ref[s][0][..., 256:]), f"set {s}: depth sums"
        assert torch.equal(got[s][1], ref[s][1]), f"set {s}: pixel counts"
        assert bool((got[s][0][..., :256] == SENTINEL).all()), f"set {s}: the x half was written"
        assert int(got[s][1][:, :, 1].sum()) == B * E.hw_padded(HW) and int(got[s][1][:, :, 0].sum()) == 0     # the all-one / all-zero rows
    assert not torch.equal(got[0][0][..., 256:], got[1][0][..., 256:])             # two different mask sets


def test_pool_depth_pair_refuses_what_it_does_not_support(gpu):
    lib = _lib.load()
    assert lib.ph_pool_depth_pair_supported(160, _lib.PH_PREC_BF16) == 1 and lib.ph_pool_depth_pair_supported(161, _lib.PH_PREC_BF16) == 0
    assert lib.ph_pool_depth_pair_supported(256, _lib.PH_PREC_F16) == 0
    assert lib.ph_pool_depth_pair_supported(153, _lib.PH_PREC_SPLIT) == 0           # two feature planes
    for N, prec, P in ((161, _lib.PH_PREC_BF16, 1), (153, _lib.PH_PREC_SPLIT, 2)):
        B, HW, Npad = 1, 512, E.n_padded(N)
        dp = torch.zeros((P, B, 256, HW), dtype=torch.int16, device=gpu)
        bits = torch.zeros((B, Npad, HW // 32), dtype=torch.int32, device=gpu)
        part = torch.full((B, 1, Npad, 512), SENTINEL, device=gpu)
        cnt = torch.full((B, 1, Npad), -1, dtype=torch.int32, device=gpu)
        with pytest.raises(_lib.PolyheadError, match="ph_pool_depth_pair"):
            E.pool_depth_pair(dp, bits, bits.clone(), N, HW, prec, part, part.clone(), cnt, cnt.clone())
        torch.cuda.synchronize()
        assert bool((part == SENTINEL).all()) and bool((cnt == -1).all())


# ---- the query kernels, one branch per launch -------------------------------------------------------------------------------------
_heads = {}


def _stage_pack(mode, gpu):
    if mode not in _heads:
        wl = dict(H=16, W=32, Nq=100, n_thing=80, n_stuff=53, S=1, F=2048)
        _heads[mode] = bench.build_head(wl, mode, torch.float32, gpu, seed=17)
    return _heads[mode].mask_head[0].stage_pack(gpu)


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
@pytest.mark.parametrize("N", [40, 153])
@pytest.mark.parametrize("mode", ["mixed16", "bf16"])
def test_query_one_branch_launches_equal_the_full_launch(gpu, mode, N, wide):
    """pre and post as launches of their own: [pre, post] of both branches against [pre, post] of the mask branch followed by
    [pre, post] of the depth branch, in one workspace.  The mask half once with the pooling's pixel counts and once counting the bit
    rows itself (what the plan's mask-only launch does: nothing has counted its masks yet)"""
    m, pack = E.MODES[mode], _stage_pack(mode, gpu)
    B, H, W, nsplit = 2, 16, 32, 3
    HW, Npad = H * W, E.n_padded(N)
    g = torch.Generator(device=gpu)
    g.manual_seed(300 + N)
    xp, dp = (E.ingest(torch.randn((B, 256, H, W), generator=g, device=gpu), m.feat) for _ in range(2))
    bits = E.binarize(torch.randn((B, N, H, W), generator=g, device=gpu))
    partial = torch.zeros((B, nsplit, Npad, 512), device=gpu)
    counts = torch.zeros((B, nsplit, Npad), dtype=torch.int32, device=gpu)
    E.pool(xp, dp, bits, N, HW, m.feat, nsplit, out=partial, counts=counts)
    k, q = (torch.randn((B, N, 256), generator=g, device=gpu) for _ in range(2))
    KP = 2 if m.kern_fmt != _lib.PH_KERN_F16 and pack.prec == _lib.PH_PREC_SPLIT else 1           # planes of `kern`
    ws = torch.zeros((_lib.load().ph_query_workspace_bytes(B, N, pack.prec),), dtype=torch.uint8, device=gpu)

    def run(launches):
        outs = dict(obj=torch.zeros((B, N, 256), device=gpu), dobj=torch.zeros((B, N, 256), device=gpu),
                    cls=torch.zeros((B, N, pack.num_classes), device=gpu), kern=torch.zeros((KP, 2, B, Npad, 256), dtype=torch.int16, device=gpu),
                    kbias=torch.zeros((2, B, Npad), device=gpu))
        ws.zero_()
        for branch, cnt in launches:
            for phase in (1, 2):                            # PH_QUERY_PRE, PH_QUERY_POST
                E.query_stage(partial, bits, k, q, pack, N, HW, cls_sigmoid=True, outs=outs, workspace=ws, kern_fmt=m.kern_fmt, counts=cnt,
                              phases=phase | (_lib.PH_QUERY_WIDE if wide else 0) | branch)
        torch.cuda.synchronize()
        return outs

    full = run([(0, counts)])
    halves = run([(_lib.PH_QUERY_MASK_ONLY, counts), (_lib.PH_QUERY_DEPTH_ONLY, counts)])
    swapped = run([(_lib.PH_QUERY_DEPTH_ONLY, counts), (_lib.PH_QUERY_MASK_ONLY, None)])
    for name in ("obj", "dobj", "cls", "kbias"):
        assert bool(torch.isfinite(full[name]).all()) and bool((full[name] != 0).any()), name
    for name in full:
        assert torch.equal(halves[name], full[name]), (mode, N, name)
        assert torch.equal(swapped[name], full[name]), (mode, N, name, "mask half counting the bit rows, depth half first")
    mask_only = run([(_lib.PH_QUERY_MASK_ONLY, None)])
    assert not bool(mask_only["dobj"].any()) and not bool(mask_only["kern"][:, 1].any()) and not bool(mask_only["kbias"][1].any())
    assert torch.equal(mask_only["obj"], full["obj"]) and torch.equal(mask_only["kern"][:, 0], full["kern"][:, 0])


def test_query_branch_flags_exclude_each_other(gpu):
    pack = _stage_pack("bf16", gpu)
    t = torch.zeros((1, 1, 64, 512), device=gpu)
    with pytest.raises(_lib.PolyheadError, match="phases"):
        E.query_stage(t, torch.zeros((1, 64, 16), dtype=torch.int32, device=gpu), torch.zeros((1, 40, 256), device=gpu),
                      torch.zeros((1, 40, 256), device=gpu), pack, 40, 512, phases=3 | _lib.PH_QUERY_MASK_ONLY | _lib.PH_QUERY_DEPTH_ONLY)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def _plan_inputs(wl, mode, B, out_dtype, gpu, seed):
    inp = bench.synth_inputs(wl, B, seed=seed)
    fdt = E.MODES[mode].feat_dtype
    return [inp["x"].to(gpu).to(fdt), inp["dfe"].to(gpu).to(fdt), inp["k0"].to(gpu), inp["q0"].to(gpu), inp["m0"].to(gpu).to(out_dtype)]


def _packs(wl, mode, gpu):
    head = bench.build_head(wl, mode, torch.float16, gpu, seed=4)
    return [h.stage_pack(gpu, mode) for h in head.mask_head]


@pytest.mark.parametrize("mode", ["mixed16", "fp16"])
@pytest.mark.parametrize("n_stuff", [53, 11], ids=["N153", "N111"])
def test_decode_plan_paired_equals_unpaired(gpu, monkeypatch, mode, n_stuff):
    """three stages on an 8 x 256 map, three frames: every output and every stage's hard masks, with the last two stages' depth
    poolings paired and as a launch each"""
    monkeypatch.setenv("PH_CONV_POOLX", "1")
    wl = dict(H=8, W=256, Nq=100, n_thing=8, n_stuff=n_stuff, S=3, F=2048)
    B, N, out_dtype = 3, 100 + n_stuff, torch.float16
    packs, gin = _packs(wl, mode, gpu), _plan_inputs(wl, mode, B, out_dtype, gpu, seed=21)
    res = {}
    for pair in (True, False):
        plan = E.DecodePlan(packs, B, N, wl["H"], wl["W"], E.MODES[mode], out_dtype, gpu, pair=pair)
        assert plan.poolx and plan.pair == pair
        plan.set_inputs(*gin)
        plan.debug_bits = []
        plan.run()
        torch.cuda.synchronize()
        res[pair] = ({k: v.clone() for k, v in plan.outputs().items() if v is not None}, plan.debug_bits)
    (out_p, bits_p), (out_u, bits_u) = res[True], res[False]
    assert len(bits_p) == len(bits_u) == 3 and set(out_p) == set(out_u) >= {"obj", "dobj", "cls", "mask", "mask_up", "depth_up"}
    for s in range(3):
        assert torch.equal(bits_p[s][:, :N], bits_u[s][:, :N]), f"hard masks of stage {s}"
    assert not torch.equal(bits_p[1], bits_p[2])
    for k in out_u:
        assert bool(torch.isfinite(out_u[k].float()).all()), k
        assert torch.equal(out_p[k], out_u[k]), k


def test_two_stage_plan_and_unsupported_plans_take_the_unpaired_path(gpu, monkeypatch):
    monkeypatch.setenv("PH_CONV_POOLX", "1")
    wl = dict(H=8, W=256, Nq=100, n_thing=8, n_stuff=11, S=2, F=2048)
    plan = E.DecodePlan(_packs(wl, "mixed16", gpu), 1, 111, 8, 256, E.MODES["mixed16"], torch.float16, gpu)
    assert plan.poolx and not plan.pair and not hasattr(plan, "bits_b")
    monkeypatch.setenv("PH_CONV_POOLX", "0")
    wl["S"] = 3
    plan = E.DecodePlan(_packs(wl, "mixed16", gpu), 1, 111, 8, 256, E.MODES["mixed16"], torch.float16, gpu, pair=True)
    assert not plan.poolx and not plan.pair


def test_multi_stream_graph_replay_equals_its_eager_run(gpu, monkeypatch):
    """two parts (2 + 1 frames) on their streams, as bench.py runs the step: the captured graph reproduces the eager run"""
    monkeypatch.setenv("PH_CONV_POOLX", "1")
    wl = dict(H=8, W=256, Nq=100, n_thing=80, n_stuff=53, S=3, F=2048)
    B, N, mode, out_dtype = 3, 153, "mixed16", torch.float16
    runner = E.DualDecodePlan(_packs(wl, mode, gpu), B, N, wl["H"], wl["W"], E.MODES[mode], out_dtype, gpu, parts=2)
    assert all(p.pair == E.POOL_PAIR and p.poolx for p in runner.halves) and E.POOL_PAIR
    runner.set_inputs(*_plan_inputs(wl, mode, B, out_dtype, gpu, seed=22))
    runner.run()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in runner.outputs().items() if v is not None}
    runner.capture()
    torch.cuda.synchronize()
    for p in runner.halves:
        for t in [p.mask, p.mask_up, p.depth_up] + [p.stage_out[-1][k] for k in ("obj", "dobj", "cls")]:
            t.fill_(float("nan"))
    runner.replay()
    torch.cuda.synchronize()
    replayed = runner.outputs()
    for k, v in eager.items():
        assert torch.equal(replayed[k], v), k
