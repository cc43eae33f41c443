"""GPU: `ph_gt_prepare` (csrc/ph_gtprep.hip) and what stands on it -- `gt.prepare_gt`, `gt.PreparedGT`, `StepGT.from_prepared`, the two
`forward_backward_prepared` -- against tests/golden/gt_prepare.npz (the reference's own statements, tools/gen_golden_gt_prepare.py)
and the fp32 numpy restatement of the arithmetic contract in tests/test_gt_prepare_host.py.

Bounds.  The kernel equals the restatement bit for bit in every case.  Against the fixture: equal at the ratios 4 and 1 and in
nearest mode; within 2^-23 at the non-integer ratio, where torch's CPU kernel contracts one product (2^-24 when the fixture was made).
The hardened masks, the valid map and the depth map are exact everywhere.  The training steps: the prepared ground truth equals the
reference's lists bit for bit at the ratio 4, so the prepared step may differ from the list step by no more than two list steps on
the same inputs differ from each other, which the test measures (zero: then `torch.equal`)."""
import numpy as np
import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, gt as GT, losses as Lo, train as TR
from test_gt_prepare_host import CASES, call_args, fixture, frame, np_gt_prepare
from test_gpu_video_train import video_parts  # noqa: F401  (the fixture: neck, the two heads, the track head as the step tests build them)

pytestmark = pytest.mark.gpu

OUTS = ("things", "stuff", "things_hard", "stuff_hard", "valid", "depth")


def _nan_outs(gpu, a, F_=None):
    F_ = len(a["nseg"]) if F_ is None else F_
    aH, aW = a["assign_hw"]
    shp = dict(things=(F_, a["gmax"], aH, aW), stuff=(F_, a["smax"], aH, aW), valid=(F_, aH, aW), depth=(F_, aH, aW))
    shp["things_hard"], shp["stuff_hard"] = shp["things"], shp["stuff"]
    return {k: torch.full(shp[k], float("nan"), dtype=torch.float32, device=gpu) for k in OUTS}


def _raw(gpu, a, frames=None, out=None, nseg=None, src_hw=None):
    """one raw call on the frames `frames` of a case's arguments; every output pre-filled with NaN"""
    idx = list(range(len(a["nseg"]))) if frames is None else list(frames)
    sub = dict(a, nseg=[a["nseg"][i] for i in idx])
    out = _nan_outs(gpu, sub) if out is None else out
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x[idx])).to(gpu)
    return GT.gt_prepare(up(a["seg"]), up(a["row_of"]), sub["nseg"] if nseg is None else nseg, up(a["depth"]), a["src_hw"] if src_hw is None else src_hw,
                         a["pad_hw"], a["assign_hw"], a["gmax"], a["smax"], nearest=a["nearest"], want_hard=(True, True), out=out)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _prepared(gpu, z, meta, name, want_hard=True):
    c = meta["cases"][name]
    frames = [frame(z, name, f) for f in range(c["frames"])]
    return GT.prepare_gt([GT.index_map_from_bitmasks(fr["bitmasks"]) for fr in frames], [fr["labels"] for fr in frames], c["pad_hw"],
                         meta["num_thing_classes"], mask_assign_stride=c["stride"], gt_depth=z[f"{name}.depth"],
                         gt_instance_ids=[fr["instance_ids"] for fr in frames], want_hard=want_hard, nearest=c["nearest"], device=gpu), frames


def _lists(gpu, z, name, frames):
    """the reference's lists of a case on the device, as `forward_backward` and `StepGT(...)` take them"""
    t = lambda k: [torch.from_numpy(fr[k]).to(gpu) for fr in frames]
    return t("gt_masks"), t("gt_labels"), t("gt_sem_seg"), t("gt_sem_cls"), torch.from_numpy(z[f"{name}.gt_depth"]).to(gpu), t("gt_instance_ids")


# ---- 1. the kernel against the fixture and the restatement; NaN-filled outputs come back fully written -------------------------------
@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_fixture_and_restatement(gpu, name):
    z, meta = fixture()
    a = call_args(z, meta, name)
    want = np_gt_prepare(**a)
    got = {k: v.cpu() for k, v in _raw(gpu, a).items()}
    for k in OUTS:
        assert not torch.isnan(got[k]).any(), k                       # rows beyond a frame's count, the frame without things, the padded border
        assert torch.equal(got[k], torch.from_numpy(want[k])), (name, k)
    for f, fr in enumerate(a["frames"]):
        G, S = a["G"][f], a["S"][f]
        for stack, n, key in (("things", G, "gt_masks"), ("stuff", S, "gt_sem_seg")):
            mine, ref = got[stack][f, :n], torch.from_numpy(fr[key])
            diff = float((mine.double() - ref.double()).abs().max()) if n else 0.0
            print(name, f, stack, "largest |kernel - reference|", diff)
            if name == "frac":
                assert diff <= 2.0 ** -23 and torch.equal(mine == 0, ref == 0)
            else:
                assert torch.equal(mine, ref), (name, f, stack)
            assert torch.equal(got[stack + "_hard"][f, :n], ref.bool().float())                       # kernel_head.py:400-403
            assert not got[stack][f, n:].any() and not got[stack + "_hard"][f, n:].any()
        ref_valid = torch.cat((torch.from_numpy(fr["gt_masks"]), torch.from_numpy(fr["gt_sem_seg"]))).sum(0).bool().float()
        assert torch.equal(got["valid"][f], ref_valid) and np.array_equal(fr["valid"], ref_valid.numpy())
        assert torch.equal(got["depth"][f], torch.from_numpy(z[f"{name}.gt_depth"][f, 0]))


# ---- 2. same bits twice; a frame does not depend on its neighbours --------------------------------------------------------------------
@pytest.mark.parametrize("name", ("s4", "frac"))
def test_two_calls_equal_bits_and_frames_are_independent(gpu, name):
    z, meta = fixture()
    a = call_args(z, meta, name)
    one, two = _raw(gpu, a), _raw(gpu, a)
    for k in OUTS:
        assert torch.equal(_bits(one[k]), _bits(two[k])), k
    for order in ([0], [1], [1, 0, 1]):
        sub = _raw(gpu, a, frames=order)
        for k in OUTS:
            for j, f in enumerate(order):
                assert torch.equal(_bits(sub[k][j]), _bits(one[k][f])), (k, order)


def test_frames_of_different_sizes_are_padded_with_no_segment(gpu):
    z, meta = fixture()
    full, frames = _prepared(gpu, z, meta, "s4")
    maps = [GT.index_map_from_bitmasks(fr["bitmasks"]) for fr in frames]
    cut = maps[1].copy()
    cut[40:], cut[:, 70:] = 255, 255
    kw = dict(gt_depth=z["s4.depth"], device=gpu)
    small = GT.prepare_gt([maps[0], np.ascontiguousarray(maps[1][:40, :70])], [fr["labels"] for fr in frames], (64, 96), 8, **kw)
    wide = GT.prepare_gt([maps[0], cut], [fr["labels"] for fr in frames], (64, 96), 8, **kw)
    for k in ("things", "stuff", "valid", "depth"):
        assert torch.equal(getattr(small, k), getattr(wide, k)), k
    assert torch.equal(small.things[0], full.things[0]) and not torch.equal(small.things[1], full.things[1])


# ---- 3. argument errors launch nothing ------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(gpu):
    z, meta = fixture()
    a = call_args(z, meta, "s4")
    for what, kw in (("255 segments", dict(nseg=[a["nseg"][0], 255])), ("Hs > Hp", dict(src_hw=(65, 90)))):
        out = _nan_outs(gpu, a)
        if "src_hw" in kw:                                             # a map of the refused size, so that the wrapper's shape check passes
            b = dict(a, seg=np.full((2,) + kw["src_hw"], 255, np.uint8), src_hw=kw["src_hw"])
            with pytest.raises(_lib.PolyheadError, match="ph_gt_prepare"):
                _raw(gpu, b, out=out)
        else:
            with pytest.raises(_lib.PolyheadError, match="ph_gt_prepare"):
                _raw(gpu, a, out=out, **kw)
        torch.cuda.synchronize()
        assert all(torch.isnan(t).all() for t in out.values()), what
    assert not any(torch.isnan(t).any() for t in _raw(gpu, a).values())          # the same call without the fault


# ---- 4. PreparedGT.step_gt against StepGT on the reference's lists ----------------------------------------------------------------------
@pytest.mark.parametrize("hard", (False, True))
def test_step_gt_equals_stepgt_of_the_lists(gpu, hard):
    z, meta = fixture()
    prep, frames = _prepared(gpu, z, meta, "s4")
    gm, gl, ss, sc, gd, ids = _lists(gpu, z, "s4", frames)
    for k, mine in (("gt_masks", prep.gt_masks), ("gt_labels", prep.gt_labels), ("gt_sem_seg", prep.gt_sem_seg), ("gt_sem_cls", prep.gt_sem_cls),
                    ("gt_instance_ids", prep.gt_instance_ids)):
        want = dict(gt_masks=gm, gt_labels=gl, gt_sem_seg=ss, gt_sem_cls=sc, gt_instance_ids=ids)[k]
        assert all(torch.equal(m, w) and m.dtype == w.dtype for m, w in zip(mine, want)), k
    assert torch.equal(prep.gt_depth, gd)
    assert prep.gt_masks[0].data_ptr() == prep.things.data_ptr()                                     # views: nothing is copied
    ref = Lo.StepGT(gm, gl, ss, sc, gd, hard)
    got = prep.step_gt(hard)
    assert (got.B, got.G, got.S, got.Gmax, got.H, got.W, got.HW, got.has_sem) == (ref.B, ref.G, ref.S, ref.Gmax, ref.H, ref.W, ref.HW, ref.has_sem)
    for b in range(ref.B):
        assert torch.equal(_bits(got.masks[b]), _bits(ref.masks[b])) and torch.equal(_bits(got.sem[b]), _bits(ref.sem[b])), b
        assert np.array_equal(got.labels_h[b], ref.labels_h[b]) and np.array_equal(got.sem_cls_h[b], ref.sem_cls_h[b])
        assert torch.equal(got.labels_dev[b], ref.labels_dev[b])
    for k in ("valid", "depth", "pad"):
        assert torch.equal(_bits(getattr(got, k)), _bits(getattr(ref, k))), k
    W = _lib.PH_ASSIGN_GT_WORDS
    tg, tr = got.device_table().cpu().numpy(), ref.device_table().cpu().numpy()
    assert tg.shape == tr.shape and np.array_equal(tg[ref.B * W:], tr[ref.B * W:])                   # labels and stuff classes
    stack = prep.things_hard if hard else prep.things
    HW4 = 4 * ref.HW
    for b in range(ref.B):
        rg, rr = tg[b * W:(b + 1) * W], tr[b * W:(b + 1) * W]
        assert np.array_equal(rg[[0, 1, 6, 7]], rr[[0, 1, 6, 7]])                                    # counts and label offsets
        assert rg[2] == stack.data_ptr() + b * stack.shape[1] * HW4 and rg[3] == prep.stuff.data_ptr() + b * prep.stuff.shape[1] * HW4
        assert rg[4] == prep.valid.data_ptr() + b * HW4 and rg[5] == prep.depth.data_ptr() + b * HW4
    # the reference frames' form: the things alone
    ref_t, got_t = Lo.StepGT(gm, gl, None, None, None, False), prep.step_gt(False, with_stuff=False)
    assert (got_t.has_sem, got_t.S, got_t.depth, got_t.G) == (ref_t.has_sem, ref_t.S, ref_t.depth, ref_t.G)
    assert torch.equal(_bits(got_t.pad), _bits(ref_t.pad)) and all(s.numel() == 0 for s in got_t.sem)
    for b in range(ref_t.B):
        assert torch.equal(_bits(got_t.masks[b]), _bits(ref_t.masks[b])) and torch.equal(got_t.labels_dev[b], ref_t.labels_dev[b])
    # the one field that differs, as `step_gt` documents: the prepared valid map marks things OR stuff, the list form the things alone
    assert got_t.valid.data_ptr() == prep.valid.data_ptr() and torch.equal(got_t.valid, ref.valid)
    assert torch.equal(ref_t.valid, torch.stack([m.ne(0).any(0) for m in gm]).float())
    assert bool((ref_t.valid <= got_t.valid).all()) and not torch.equal(ref_t.valid, got_t.valid)
    soft_only, _ = _prepared(gpu, z, meta, "s4", want_hard=False)
    assert soft_only.things_hard is None and torch.equal(soft_only.things, prep.things)
    with pytest.raises(ValueError, match="want_hard"):
        soft_only.step_gt(True)


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(gpu):
    z, meta = fixture()
    a = call_args(z, meta, "s4")
    eager = _raw(gpu, a)
    out = _nan_outs(gpu, a)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    seg, rows, depth = up(a["seg"]), up(a["row_of"]), up(a["depth"])
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):                                      # one stream, one branch
        GT.gt_prepare(seg, rows, a["nseg"], depth, a["src_hw"], a["pad_hw"], a["assign_hw"], a["gmax"], a["smax"], want_hard=(True, True), out=out)
    graph.replay()
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.equal(_bits(out[k]), _bits(eager[k])), k


# ---- 6. the two training steps on prepared ground truth ---------------------------------------------------------------------------------
def _grads(mods):
    return [None if p.grad is None else p.grad.clone() for m in mods for p in m.parameters()]


def _clear(mods):
    for m in mods:
        for p in m.parameters():
            p.grad = None


def _gap(a, b):
    """largest absolute difference between two step results (losses, objective, input gradients, parameter gradients)"""
    worst = max(float((a[0][k].double() - b[0][k].double()).abs()) for k in a[0])
    worst = max(worst, float((a[1].double() - b[1].double()).abs()))
    for x, y in zip(list(a[2]) + a[3], list(b[2]) + b[3]):
        assert (x is None) == (y is None)
        if x is not None:
            worst = max(worst, float((x.double() - y.double()).abs().max()))
    return worst


def _same(a, b):
    ok = set(a[0]) == set(b[0]) and all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and torch.equal(a[1], b[1])
    return ok and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(list(a[2]) + a[3], list(b[2]) + b[3]))


@pytest.mark.parametrize("device_assign", (False, True))
def test_steps_on_prepared_ground_truth_equal_the_list_steps(gpu, video_parts, device_assign):  # noqa: F811
    neck, rpn, roi, th, tcfg = video_parts[:5]
    mods = (neck, rpn, roi, th)
    z, meta = fixture()
    key, kframes = _prepared(gpu, z, meta, "s4")
    ref, rframes = _prepared(gpu, z, meta, "near")                     # the reference frames: the same padded size, nearest masks
    gm, gl, ss, sc, gd, ids = _lists(gpu, z, "s4", kframes)
    rgm, rgl, _, _, _, rids = _lists(gpu, z, "near", rframes)
    B, H0, W0 = 2, 16, 24                                              # 64 x 96 padded; the assign resolution is 16 x 24
    pad_hw = (4 * H0, 4 * W0)
    x = [f.to(gpu) for f in Hh.fpn_inputs(seed=41, B=B, C=256, H0=H0, W0=W0)]
    x_ref = [f.to(gpu) for f in Hh.fpn_inputs(seed=42, B=B, C=256, H0=H0, W0=W0)]
    metas = [Hh.img_meta(60, 90, pad_to=pad_hw)] * B

    def run(fn):
        _clear(mods)
        losses, total, gx = fn()
        return losses, total, gx, _grads(mods)

    with TR.VideoTrainStep(neck, rpn, roi, th, tcfg, device_assign=device_assign) as step:
        lists = lambda: step.forward_backward(x, x_ref, metas, gm, gl, ss, sc, gd, ids, rgm, rgl, rids, pad_hw)
        a1, a2 = run(lists), run(lists)
        if device_assign:
            st = step.assign_status()
            assert st.shape == (6, 2) and (st == 0).all(), st
        p = run(lambda: step.forward_backward_prepared(x, x_ref, metas, key, ref, pad_hw))
        if device_assign:
            st = step.assign_status()
            assert st.shape == (6, 2) and (st == 0).all(), st
    assert all(np.isfinite(float(v)) for v in a1[0].values()), a1[0]   # a pair without a positive gives NaN, as in the reference
    noise = _gap(a1, a2)
    print("video step: two list steps differ by", noise, "; prepared - list", _gap(a1, p))
    assert len(p[0]) == 26 and all(np.isfinite(float(v)) for v in p[0].values())
    assert _same(a1, p) if noise == 0 else _gap(a1, p) <= noise
    assert any(g is not None and float(g.abs().sum()) > 0 for g in p[3])

    with torch.enable_grad():
        feats = [f.detach() for f in TR.neck_forward_train(neck, x)]
    with TR.TrainStep(rpn, roi, device_assign=device_assign) as istep:
        lists = lambda: istep.forward_backward(feats, metas, gm, gl, ss, sc, gd)
        b1, b2 = run(lists), run(lists)
        q = run(lambda: istep.forward_backward_prepared(feats, metas, key))
    noise = _gap(b1, b2)
    print("image step: two list steps differ by", noise, "; prepared - list", _gap(b1, q))
    assert len(q[0]) == 24
    assert _same(b1, q) if noise == 0 else _gap(b1, q) <= noise
    _clear(mods)


@pytest.mark.parametrize("device_assign", (False, True))
def test_hardened_rpn_targets_on_prepared_ground_truth(gpu, video_parts, device_assign):  # noqa: F811
    """rpn.hard_target = True, roi.hard_target = False: the step holds two `StepGT`s, the rpn side's on the hardened prepared stack
    (kernel_head.py:400-403), the roi side's on the soft one.  Same bound as above: what two list steps differ by."""
    neck, rpn, roi = video_parts[:3]
    z, meta = fixture()
    key, kframes = _prepared(gpu, z, meta, "s4")
    gm, gl, ss, sc, gd, _ = _lists(gpu, z, "s4", kframes)
    B, H0, W0 = 2, 16, 24
    x = [f.to(gpu) for f in Hh.fpn_inputs(seed=41, B=B, C=256, H0=H0, W0=W0)]
    with torch.enable_grad():
        feats = [f.detach() for f in TR.neck_forward_train(neck, x)]
    metas = [Hh.img_meta(60, 90, pad_to=(4 * H0, 4 * W0))] * B

    def run(fn):
        _clear((rpn, roi))
        losses, total, gx = fn()
        return losses, total, gx, _grads((rpn, roi))

    assert any(bool(((m > 0) & (m < 1)).any()) for m in gm)            # hardening changes the targets
    with TR.TrainStep(rpn, roi, device_assign=device_assign) as step:
        soft = run(lambda: step.forward_backward(feats, metas, gm, gl, ss, sc, gd))
        assert rpn.hard_target is False
        rpn.hard_target = True
        try:
            assert set(TR._prepared_cache(key, (rpn.hard_target, roi.hard_target))) == {False, True}
            lists = lambda: step.forward_backward(feats, metas, gm, gl, ss, sc, gd)
            h1, h2 = run(lists), run(lists)
            p = run(lambda: step.forward_backward_prepared(feats, metas, key))
        finally:
            rpn.hard_target = False
    noise = _gap(h1, h2)
    print("image step, hardened rpn targets: two list steps differ by", noise, "; prepared - list", _gap(h1, p), "; hard - soft", _gap(h1, soft))
    assert len(p[0]) == 24 and all(np.isfinite(float(v)) for v in p[0].values())
    assert not _same(h1, soft)                                         # the hardened stack was read
    assert _same(h1, p) if noise == 0 else _gap(h1, p) <= noise
    _clear((rpn, roi))
