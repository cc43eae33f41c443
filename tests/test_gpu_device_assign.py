"""GPU: the training step's Hungarian assignment and target descriptors on the device (csrc/ph_assign.hip) -- `ph_assign_solve`
against the installed scipy, ties included; `ph_assign_desc`'s blob against `losses.build_desc` fed by `losses.assign_batch`, byte
for byte; a whole `TrainStep` with the switch on against the host path, with scipy made to raise."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import helpers as Hh
from polyphonicformer_amd import _lib
from polyphonicformer_amd import assigner as A
from polyphonicformer_amd import losses as Lo
from test_device_assign import KINDS, cost_matrix

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (3, 5), (64, 64), (65, 33), (100, 57), (129, 127), (256, 256)]


def device_solve(gpu, cost, counts):
    """cost [B, Np, ldg] numpy fp32, counts [B] -> (rc, match [B, ldg], status [B]) as numpy"""
    B, Np, ldg = cost.shape
    c = torch.from_numpy(np.ascontiguousarray(cost)).to(gpu)
    cnt = torch.tensor(counts, dtype=torch.int32, device=gpu)
    match = torch.full((B, ldg), -7, dtype=torch.int32, device=gpu)
    status = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    rc = _lib.load().ph_assign_solve(_lib.ptr(c), B, Np, ldg, _lib.ptr(cnt), 1, _lib.ptr(match), _lib.ptr(status), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, match.cpu().numpy(), status.cpu().numpy()


def as_scipy(match_row, Np):
    """(rows ascending, cols) of the pairs a match row (prediction per ground-truth column) holds"""
    g = np.nonzero(match_row >= 0)[0]
    order = np.argsort(match_row[g], kind="stable")
    return match_row[g][order].astype(np.int64), g[order].astype(np.int64)


@pytest.mark.parametrize("kind", KINDS)
def test_solver_equals_scipy(gpu, kind):
    for n, (Np, G) in enumerate(SHAPES):
        c = cost_matrix(kind, Np, G, 500 + 10 * KINDS.index(kind) + n)
        rc, match, status = device_solve(gpu, c[None], [G])
        assert rc == 0 and status[0] == _lib.PH_ASSIGN_OK, (Np, G, rc, status)
        r, col = linear_sum_assignment(c)
        r1, c1 = as_scipy(match[0], Np)
        assert np.array_equal(r, r1) and np.array_equal(col, c1), (kind, Np, G)


def test_solver_mixed_counts_in_one_launch(gpu):
    """G_b = 0, 1 and ldg in one launch: nothing to solve, the transposed and the not transposed orientation"""
    Np, ldg = 5, 7
    cost = np.stack([cost_matrix("ints", Np, ldg, 900 + b) for b in range(3)])
    rc, match, status = device_solve(gpu, cost, [0, 1, ldg])
    assert rc == 0 and (status == 0).all()
    assert (match[0] == -7).all() and (match[1, 1:] == -7).all()          # entries at or beyond G_b are not written
    for b, G in ((1, 1), (2, ldg)):
        r, col = linear_sum_assignment(cost[b, :, :G])
        r1, c1 = as_scipy(match[b, :G], Np)
        assert np.array_equal(r, r1) and np.array_equal(col, c1), b


def test_non_finite_cost_sets_the_status_word(gpu):
    """a data check, no fault: the image with the NaN gets the trivial matching and its status word, the others are solved"""
    Np, G = 6, 4
    cost = np.stack([cost_matrix("normal", Np, G, 910 + b) for b in range(3)])
    cost[1, 3, 2] = np.nan
    rc, match, status = device_solve(gpu, cost, [G] * 3)
    assert rc == 0
    assert status.tolist() == [_lib.PH_ASSIGN_OK, _lib.PH_ASSIGN_ENONFINITE, _lib.PH_ASSIGN_OK]
    assert match[1].tolist() == list(range(G))
    for b in (0, 2):
        r, col = linear_sum_assignment(cost[b])
        r1, c1 = as_scipy(match[b], Np)
        assert np.array_equal(r, r1) and np.array_equal(col, c1), b


def test_oversize_is_refused_before_any_launch(gpu):
    cost = np.zeros((1, 4, 257), np.float32)
    rc, match, status = device_solve(gpu, cost, [257])
    assert rc == _lib.PH_EUNSUPPORTED and "256" in Hh.last_error()
    assert (match == -7).all() and (status == -7).all()


# ---- the descriptor blob ---------------------------------------------------------------------------------------------------------
NT, NS = 8, 11
ROI_ASSIGNER = Hh.ROI_ASSIGNER


def _tie_gt(H, W):
    """two identical instance masks of different class, two all-zero masks (instances that vanish at the assign stride), one more"""
    g = Hh.train_gt(61, 1, H, W, NT, NS, [5])[0]
    g["masks"][1] = g["masks"][0]
    g["masks"][2] = 0
    g["masks"][3] = 0
    g["labels"] = torch.tensor([1, 4, 2, 2, 6])
    return [g]


BLOB_CASES = {"two_images": lambda: (Hh.train_gt(78, 2, 16, 32, NT, NS, [4, 6]), 16, 32),
              "ragged_one_empty": lambda: (Hh.train_gt(52, 3, 14, 22, NT, NS, [4, 0, 7]), 14, 22),
              "ties": lambda: (_tie_gt(16, 32), 16, 32)}


@pytest.mark.parametrize("roi", [True, False], ids=["roi", "khead"])
@pytest.mark.parametrize("case", list(BLOB_CASES))
def test_blob_equals_build_desc(gpu, case, roi):
    gts, H, W = BLOB_CASES[case]()
    gts = [{k: v.to(gpu) for k, v in g.items()} for g in gts]
    B, Np = len(gts), 100
    gt = Lo.StepGT([g["masks"] for g in gts], [g["labels"] for g in gts], [g["sem_seg"] for g in gts], [g["sem_cls"] for g in gts],
                   torch.stack([g["depth"][None] for g in gts]), True)
    gen = torch.Generator().manual_seed(7)
    pred = torch.randn(B, Np, H, W, generator=gen) * 2
    for b in range(B):                                   # every third prediction is a noisy copy of an instance, some of them twice
        for n in range(0, Np, 3):
            if gt.G[b]:
                pred[b, n] = (gts[b]["masks"][(n // 3) % gt.G[b]].cpu() - 0.5) * 6 + torch.randn(H, W, generator=gen)
    pred = pred.to(gpu)
    cls = torch.randn(B, Np, NT, generator=gen).to(gpu) if roi else None
    assigner = A.build_assigner(copy.deepcopy(ROI_ASSIGNER))
    head = SimpleNamespace(num_classes=NT + NS, num_thing_classes=NT, num_stuff_classes=NS)
    cfg = SimpleNamespace(pos_weight=1.0)
    want = Lo.build_desc(head, gt, Lo.assign_batch(assigner, pred, cls, gt), Np, cfg, roi)
    got = Lo.assign_desc_device(head, gt, assigner, pred, cls, Np, cfg, roi)
    assert got is not None
    torch.cuda.synchronize()
    assert torch.stack(gt.status_words).eq(0).all()
    assert got.blob.numel() == want.blob.numel()
    diff = (got.blob != want.blob).nonzero().flatten().tolist()
    off = {k: p.value - want.blob.data_ptr() for k, p in want.ptr.items()}
    assert torch.equal(got.blob, want.blob), (len(diff), diff[:8], off)
    assert {k: p.value - got.blob.data_ptr() for k, p in got.ptr.items()} == off and got.n == want.n
    assert (got.B, got.N, got.R, got.P, got.depth_rows, got.roi, got.has_depth) == \
        (want.B, want.N, want.R, want.P, want.depth_rows, want.roi, want.has_depth)
    if roi:                                              # a later stage with the same assignment: no solve, the same tables
        again = Lo.assign_desc_device(head, gt, None, pred, None, Np, cfg, roi, prev=got)
        assert torch.equal(again.blob, want.blob) and len(gt.status_words) == 1


# ---- the whole step ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def heads(gpu):
    from polyphonicformer_amd.registry import HEADS
    import polyphonicformer_amd.kernel_update  # noqa: F401
    from test_gpu_loss import _rpn_head
    rpn, sd = _rpn_head(gpu)
    roi = HEADS.build(dict(type="KernelUpdateIterHead", num_stages=3, assign_stages=3, stage_loss_weights=[1] * 3, num_proposals=100,
                           num_thing_classes=NT, num_stuff_classes=NS, do_panoptic=True, merge_joint=True,
                           mask_head=Hh.stage_cfg(256, 2048, 8, NT + NS, NT, NS),
                           train_cfg=dict(assigner=copy.deepcopy(ROI_ASSIGNER), sampler=dict(type='MaskPseudoSampler'), pos_weight=1.)))
    roi.load_state_dict({k[len("roi_head."):]: v for k, v in sd.items() if k.startswith("roi_head.")})
    roi.to(gpu)
    B, H, W = 2, 8, 16
    feats = [f.to(gpu) for f in Hh.neck_inputs(77, B, 256, H, W)]
    gts = [{k: v.to(gpu) for k, v in g.items()} for g in Hh.train_gt(78, B, 2 * H, 2 * W, NT, NS, [4, 6])]
    gd = torch.stack([g["depth"][None] for g in gts])
    args = (feats, [Hh.img_meta(H * 8, W * 8)] * B, [g["masks"] for g in gts], [g["labels"] for g in gts], [g["sem_seg"] for g in gts],
            [g["sem_cls"] for g in gts], gd)
    return rpn, roi, args


def _raise(*a, **k):
    raise AssertionError("the host Hungarian solver was called on the device path")


def _run_step(T, rpn, roi, args, **kw):
    params = list(rpn.parameters()) + list(roi.parameters())
    for p in params:
        p.grad = None
    with T.TrainStep(rpn, roi, **kw) as step:
        losses, total, gfeat = step.forward_backward(*args)
        status = step.assign_status()
    return losses, total, gfeat, [None if p.grad is None else p.grad.clone() for p in params], status


def _same(a, b):
    la, ta, fa, ga, _ = a
    lb, tb, fb, gb, _ = b
    if set(la) != set(lb) or not torch.equal(ta, tb):
        return False
    return (all(torch.equal(la[k], lb[k]) for k in la) and all(torch.equal(x, y) for x, y in zip(fa, fb)) and
            all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(ga, gb)))


def test_whole_step_without_the_host_solver(gpu, heads, monkeypatch):
    """`TrainStep(device_assign=True)` never reaches scipy, reports status 0 for its four solves and returns the host path's 24
    losses, objective and gradients bit for bit.  The training kernels use no float atomics, so two host-path runs are equal:
    asserted first, as the premise of the comparison."""
    import scipy.optimize
    from polyphonicformer_amd import train as T
    rpn, roi, args = heads
    host = _run_step(T, rpn, roi, args)
    assert len(host[0]) == 24 and host[4].numel() == 0
    assert _same(host, _run_step(T, rpn, roi, args)), "two runs of the host path differ: the step is not deterministic"
    monkeypatch.setattr(scipy.optimize, "linear_sum_assignment", _raise)
    monkeypatch.setattr(A, "linear_sum_assignment", _raise)
    monkeypatch.setattr(A, "_hungarian", _raise)
    dev = _run_step(T, rpn, roi, args, device_assign=True)
    assert dev[4].shape == (4, 2) and (dev[4] == 0).all(), dev[4]
    for k in host[0]:
        assert torch.equal(host[0][k], dev[0][k]), (k, float(host[0][k]), float(dev[0][k]))
    assert _same(host, dev)


def test_whole_step_on_materialised_targets(gpu, heads, monkeypatch):
    """the other path of the training forward -- per-image `assign` / `sample`, `get_targets`, `stage_losses` / `rpn_losses`: what a
    configuration outside `train._fast_assign_ok` (topk > 1, a weighted DepthCost, another sampler) runs -- forced on the shipped
    configuration: the descriptor path's 24 keys, the objective and every value within `test_gpu_loss_edges.VALUE_BOUND` of the
    descriptor path's (the forward does not depend on the targets, so both paths see the same predictions in every stage: what
    differs is what `test_fused_vs_unfused` compares under that bound), every parameter and map gradient present and finite.
    Gradients are not compared across the two paths: the abs-rel depth term's gradient jumps at p == t, and two fp32 kernels may
    sit on different sides of it at single pixels."""
    from polyphonicformer_amd import train as T
    from test_gpu_loss_edges import close
    rpn, roi, args = heads
    desc = _run_step(T, rpn, roi, args)
    monkeypatch.setattr(T, "_fast_assign_ok", lambda a, s: False)

    def no_descriptors(*a, **k):
        raise AssertionError("the descriptor path ran although _fast_assign_ok refuses it")

    monkeypatch.setattr(Lo, "fused_losses", no_descriptors)
    mat = _run_step(T, rpn, roi, args)
    assert set(mat[0]) == set(desc[0]) and len(mat[0]) == 24
    close(mat[1], desc[1], "objective")
    for k in sorted(desc[0]):
        close(mat[0][k], desc[0][k], k)
    for g in mat[2] + mat[3]:
        assert g is not None and torch.isfinite(g).all()
    assert len(mat[2]) == 3 and mat[4].numel() == 0


def test_device_step_does_not_wait_for_the_host(gpu, heads, monkeypatch):
    """with the switch on nothing between the construction of the step's ground truth (its one label read) and the end of backward
    synchronises with the device: torch raises on any such operation here"""
    from polyphonicformer_amd import train as T
    rpn, roi, args = heads
    real = Lo.StepGT

    def step_gt(*a, **k):
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("default")
        try:
            gt = real(*a, **k)
            gt.device_table()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        return gt

    monkeypatch.setattr(Lo, "StepGT", step_gt)
    with T.TrainStep(rpn, roi, device_assign=True) as step:
        step.forward_backward(*args)                      # warm: scratch buffers, cached tables
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            step.forward_backward(*args)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert (step.assign_status() == 0).all()


def test_module_api_switch(gpu, heads, monkeypatch):
    """`device_assign = True` on the two heads: their `forward_train` returns the default's loss dict without the host solver"""
    rpn, roi, (feats, metas, gm, gl, gs, gc, gd) = heads

    def run():
        (rl, pf, xf, mp, cs, df, dp, dpr, _) = rpn.forward_train([f.clone() for f in feats], metas, gm, gl, gs, gc, gd)
        losses = roi.forward_train(xf, pf, mp, cs, metas, gm, gl, gt_depth=gd, depth_preds=dpr, depth_feats=df, depth_proposal=dp, gt_sem_seg=gs,
                                   gt_sem_cls=gc, imgs_whwh=None)
        losses.update(rl)
        return {k: v.detach() for k, v in losses.items()}

    want = run()
    monkeypatch.setattr(A, "_hungarian", _raise)
    try:
        rpn.device_assign = roi.device_assign = True
        got = run()
    finally:
        del rpn.device_assign, roi.device_assign
    assert set(got) == set(want) and len(want) == 24
    for k in want:
        assert torch.equal(got[k], want[k]), k
