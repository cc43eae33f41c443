"""CPU: the specification of the device Hungarian solver (csrc/ph_assign.hip k_assign_solve) and the descriptor layout.

`solve` restates scipy's shortest-augmenting-path solver (scipy/optimize/rectangular_lsap) operation for operation; the kernel
restates `solve`.  The first test holds it against the installed scipy on matrices full of ties, so that a scipy with another tie
order shows up here and not as a puzzling GPU failure; the second holds the kernel's selection rule -- positions dealt to 64 lanes,
a butterfly under a total order -- against the sequential scan.  `ph_assign_desc_layout` (a pure host function) is compared with
the blob `losses.build_desc` lays out."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from polyphonicformer_amd import _lib
from polyphonicformer_amd import losses as Lo

KINDS = ("normal", "ints", "blocks", "equal")


def _select_sequential(remaining, sp, row4col):
    index, lowest = -1, np.inf
    for it, j in enumerate(remaining):
        if sp[j] < lowest or (sp[j] == lowest and row4col[j] == -1):
            lowest, index = sp[j], it
    return index, lowest


def _better(a, b):
    """the kernel's total order on (sp, unassigned, position); position < 0: no candidate"""
    if a[2] < 0 or b[2] < 0:
        return b[2] < 0 <= a[2]
    if a[0] != b[0]:
        return a[0] < b[0]
    if a[1] != b[1]:
        return a[1] > b[1]
    return a[2] > b[2] if a[1] else a[2] < b[2]


def _select_parallel(remaining, sp, row4col):
    """the parallel form: among the positions that hold the minimum the LARGEST unassigned one, else the SMALLEST -- as the kernel
    evaluates it: lane l folds positions l, l + 64, ..., then a 64-lane xor butterfly"""
    lanes = []
    for lane in range(64):
        best = (np.inf, 0, -1)
        for it in range(lane, len(remaining), 64):
            j = remaining[it]
            cand = (sp[j], int(row4col[j] == -1), it)
            if _better(cand, best):
                best = cand
        lanes.append(best)
    m = 1
    while m < 64:
        lanes = [lanes[l ^ m] if _better(lanes[l ^ m], lanes[l]) else lanes[l] for l in range(64)]
        m <<= 1
    assert all(x == lanes[0] for x in lanes)
    return lanes[0][2], lanes[0][0]


def solve(cost, select=_select_sequential):
    """scipy.optimize.linear_sum_assignment restated; cost [nr0, nc0]; scipy transposes iff nc0 < nr0 (strictly)"""
    cost = np.asarray(cost, np.float64)
    nr, nc = cost.shape
    tr = nc < nr
    if tr:
        cost = cost.T.copy()
        nr, nc = nc, nr
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = -np.ones(nr, int), -np.ones(nc, int)
    for cur in range(nr):
        sp, path = np.full(nc, np.inf), -np.ones(nc, int)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        remaining = [nc - it - 1 for it in range(nc)]
        minv, i, sink = 0.0, cur, -1
        while sink == -1:
            SR[i] = True
            for j in remaining:
                r = minv + cost[i, j] - u[i] - v[j]                 # left to right, no fused multiply-add
                if r < sp[j]:
                    path[j], sp[j] = i, r
            index, minv = select(remaining, sp, row4col)
            assert minv != np.inf
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            remaining[index] = remaining[-1]                        # swap-remove: positions matter
            remaining.pop()
        u[cur] += minv
        for i2 in range(nr):
            if SR[i2] and i2 != cur:
                u[i2] += minv - sp[col4row[i2]]
        for j in range(nc):
            if SC[j]:
                v[j] -= minv - sp[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if tr:
        order = np.argsort(col4row)
        return col4row[order], order
    return np.arange(nr), col4row


def cost_matrix(kind, N, G, seed):
    """fp32 [N, G]: normal entries | integers 0..2 | a block of identical columns (duplicated instances) | every column equal
    (ground-truth masks that vanish at the assign stride)"""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((N, G)).astype(np.float32)
    if kind == "ints":
        return rng.integers(0, 3, (N, G)).astype(np.float32)
    if kind == "blocks":
        c = rng.standard_normal((N, G)).astype(np.float32)
        k = int(rng.integers(0, G))
        c[:, k:] = c[:, k:k + 1]
        return c
    assert kind == "equal"
    return np.repeat(rng.standard_normal((N, 1)).astype(np.float32), G, 1)


SIZES = [(1, 1), (1, 40), (40, 1), (2, 2), (5, 3), (3, 5), (7, 7), (13, 29), (29, 13), (16, 17), (17, 16), (24, 24), (31, 40), (40, 31),
         (40, 40), (33, 8), (8, 33), (39, 39), (12, 12), (20, 35)]


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_scipy(kind):
    for n, (N, G) in enumerate(SIZES):
        c = cost_matrix(kind, N, G, 1000 * KINDS.index(kind) + n)
        r0, c0 = linear_sum_assignment(c)
        r1, c1 = solve(c)
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (kind, N, G)


@pytest.mark.parametrize("kind", KINDS)
def test_parallel_selection_equals_sequential(kind):
    for n, (N, G) in enumerate([(5, 3), (3, 5), (24, 24), (70, 66), (66, 70), (9, 130)]):
        c = cost_matrix(kind, N, G, 77 + 10 * KINDS.index(kind) + n)
        r0, c0 = solve(c)
        r1, c1 = solve(c, _select_parallel)
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (kind, N, G)


# ---- the layout ----------------------------------------------------------------------------------------------------------------
def hand_assignments(seed, G, Np):
    """per image (prediction indices ascending, ground-truth indices): min(G, Np) pairs"""
    rng = np.random.default_rng(seed)
    out = []
    for g in G:
        m = min(g, Np)
        out.append((np.sort(rng.permutation(Np)[:m]).astype(np.int64), rng.permutation(g)[:m].astype(np.int64)))
    return out


def step_gt(seed, G, H, W, nt, ns, stuff, depth, dev="cpu"):
    import helpers as Hh
    gts = [{k: v.to(dev) for k, v in g.items()} for g in Hh.train_gt(seed, len(G), H, W, nt, ns, list(G))]
    return Lo.StepGT([g["masks"] for g in gts], [g["labels"] for g in gts], [g["sem_seg"] for g in gts] if stuff else None,
                     [g["sem_cls"] for g in gts] if stuff else None, torch.stack([g["depth"][None] for g in gts]) if depth else None, True)


def layout_call(head, gt, Np, roi, last):
    lib = _lib.load()
    N = Np + head.num_stuff_classes if (roi and gt.has_sem) else Np
    c = _lib.AssignCfg(B=gt.B, Np=Np, N=N, L=head.num_classes, n_thing=head.num_thing_classes, n_stuff=head.num_stuff_classes, roi=int(roi),
                       has_sem=int(gt.has_sem), has_depth=int(gt.depth_base is not None), pos_weight=1.0, HW=gt.HW)
    G, S = np.asarray(gt.G, np.int32), np.asarray([len(s) for s in gt.sem_cls_h], np.int32)
    last = np.asarray(last, np.int32)
    lay = _lib.AssignLayout()
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.ph_assign_desc_layout(C.byref(c), ip(G), ip(S), ip(last), C.byref(lay))
    assert rc == 0, lib.ph_last_error_string()
    return lay


@pytest.mark.parametrize("G", [(3, 0, 5), (0, 0), (9, 2), (1,)])
@pytest.mark.parametrize("depth", [True, False])
@pytest.mark.parametrize("stuff", [True, False])
@pytest.mark.parametrize("roi", [True, False])
def test_layout_equals_build_desc(roi, stuff, depth, G):
    nt, ns, Np, H, W = 4, 5, 7, 3, 5
    head = SimpleNamespace(num_classes=nt + ns, num_thing_classes=nt, num_stuff_classes=ns)
    gt = step_gt(3 + len(G), G, H, W, nt, ns, stuff, depth)
    assigns = hand_assignments(5, G, Np)
    desc = Lo.build_desc(head, gt, assigns, Np, SimpleNamespace(pos_weight=1.0), roi)
    # is the image's last row a positive (roi form: its depth item gives way to the direct-depth item)
    if roi and stuff:
        last = [int(nt + ns - 1 in sc) for sc in gt.sem_cls_h]
    else:
        last = [int(roi and Np - 1 in pi) for pi, _ in assigns]
    lay = layout_call(head, gt, Np, roi, last)
    base = desc.blob.data_ptr()
    for k, p in desc.ptr.items():
        assert getattr(lay, k) == p.value - base, (k, getattr(lay, k), p.value - base)
    assert lay.total_bytes == desc.blob.numel()
    assert (lay.P, lay.depth_rows) == (desc.P, desc.depth_rows)
    nd = int(np.frombuffer(desc.blob.numpy().tobytes(), np.int32, desc.depth_rows + 1, desc.ptr["dstart"].value - base)[-1])
    assert lay.depth_items == nd
    if not roi:
        assert lay.seg_items == int(np.frombuffer(desc.blob.numpy().tobytes(), np.int32, gt.B + 1, desc.ptr["sstart"].value - base)[-1])
