"""Fixture for the ground-truth preparation (tests/golden/gt_prepare.npz), produced on the CPU by the reference's own statements, which the
generator reads from the reference tree (oracle/ref_loader.REF_ROOT) when it runs:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_gt_prepare.py

Inputs per frame, as a loader hands them over: disjoint bitmasks `uint8 [n][Hs][Ws]` cut from a blocky random label map (block size
3, so that segment edges do not sit on multiples of the assign stride), labels (things < NUM_THINGS <= stuff), instance ids, a depth
map at the padded size (a ramp).  Pixels of label-map value 255 belong to no mask; one segment per frame carries label -1: the loader dropped
it from its list, its index stays in the index map (`gt.prepare_gt` maps it to no row); one things mask is empty (cropped away) and
stays in the list, as the reference keeps it; one frame has no things at all.

Outputs per frame: what PolyphonicVideo.forward_train holds at polyphonic_former_video.py:185, from its statements :103-138 (the sizes
:103-105, the loop over the frames :114-133, the nearest depth :135-138).  They are named below by line number only: the generator
parses the reference's file, takes those statements out of forward_train and runs them on the kept masks, so the file holds what the
reference computes and follows it when it changes -- gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_instance_ids, gt_depth -- and
the valid map of kernel_head.py:415.

Cases (the smallest at which the kernel can still go wrong):
    s4    pad 64 x 96, source 60 x 90, stride 4 -> 16 x 24, bilinear; 5 things + 3 stuff per frame
    frac  pad 50 x 70, source 47 x 66, stride 4 -> 12 x 17 (a non-integer ratio, as pad // stride gives), bilinear; the frame
          without things
    one   pad 37 x 53, source 35 x 50, stride 1, bilinear
    near  pad 64 x 96, source 60 x 90, stride 4, nearest (the semantic_kitti configuration); its frames share instance ids with
          s4's, so the two make the key and reference frames of a video step"""
import ast
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "gt_prepare.npz")
NUM_THINGS, NUM_STUFF = 8, 11
SEED = 1907
BLOCK = 3
ID_POOL = 10                       # instance ids are drawn from 1 .. ID_POOL, so that frames of two cases share some (a video pair)
# name: (pad_hw, src_hw, stride, nearest, per frame (things, stuff))
CASES = {"s4": ((64, 96), (60, 90), 4, False, ((5, 3), (5, 3))),
         "frac": ((50, 70), (47, 66), 4, False, ((4, 2), (0, 3))),
         "one": ((37, 53), (35, 50), 1, False, ((3, 2), (2, 2))),
         "near": ((64, 96), (60, 90), 4, True, ((5, 3), (3, 3)))}


class BitmapMasks:
    """what the statements below use of mmdet.core.mask.structures.BitmapMasks: masks, height, width, to_tensor"""

    def __init__(self, masks, height, width):
        self.masks, self.height, self.width = masks, height, width

    def to_tensor(self, dtype, device):
        return torch.tensor(self.masks, dtype=dtype, device=device)


def frame_inputs(rng, src_hw, n_things, n_stuff):
    """-> bitmasks uint8 [n][Hs][Ws] (disjoint), labels int64 [n] (-1: dropped by the loader), instance ids int64 [n], the label map
    the bitmasks were cut from (bitmasks[i] = label_map == i; the file stores this, a ninth of the bitmasks' bytes)"""
    Hs, Ws = src_hw
    n = n_things + n_stuff + 1                                     # + the dropped segment
    labels = np.concatenate([rng.integers(0, NUM_THINGS, n_things), rng.choice(np.arange(NUM_THINGS, NUM_THINGS + NUM_STUFF), n_stuff, replace=False), [-1]])   # stuff classes of a frame are distinct
    labels = labels[rng.permutation(n)]                            # loader order: things, stuff and the dropped one interleaved
    empty = int(np.flatnonzero((labels >= 0) & (labels < NUM_THINGS))[0]) if n_things else -1
    values = np.array([i for i in range(n) if i != empty] + [255])
    coarse = values[rng.integers(0, len(values), (-(-Hs // BLOCK), -(-Ws // BLOCK)))]
    label_map = np.kron(coarse, np.ones((BLOCK, BLOCK), np.int64))[:Hs, :Ws]
    masks = np.stack([(label_map == i) for i in range(n)]).astype(np.uint8)
    assert masks.sum(0).max() == 1 and (label_map == 255).any() and (empty < 0 or masks[empty].sum() == 0)
    assert all(masks[i].any() for i in range(n) if i != empty)
    return masks, labels.astype(np.int64), (rng.permutation(ID_POOL)[:n] + 1).astype(np.int64), label_map.astype(np.uint8)


REF_FILE, REF_METHOD = "polyphonic/polyphonic_former_video.py", "forward_train"
REF_FIRST, REF_LAST = 103, 138     # the statements between the asserts on the arguments and the reference frame's squeezes


def reference_statements():
    """the statements REF_FIRST .. REF_LAST of the reference's file, read from the reference tree when the generator runs and compiled
    under the file's own name and line numbers; nothing of them is kept in this repository.  The line range has to be whole statements
    of PolyphonicVideo.forward_train's body, or this raises."""
    from oracle import ref_loader
    path = os.path.join(ref_loader.REF_ROOT, REF_FILE)
    with open(path) as f:
        source = f.read()
    body = next(n for n in ast.walk(ast.parse(source)) if isinstance(n, ast.FunctionDef) and n.name == REF_METHOD).body
    stmts = [s for s in body if REF_FIRST <= s.lineno and s.end_lineno <= REF_LAST]
    inside = [s for s in body if s.lineno <= REF_LAST and s.end_lineno >= REF_FIRST]
    if not stmts or stmts != inside or stmts[0].lineno != REF_FIRST or stmts[-1].end_lineno != REF_LAST:
        raise RuntimeError(f"{path}:{REF_FIRST}-{REF_LAST} is not a run of whole statements of {REF_METHOD}: the reference has moved")
    return compile(ast.Module(body=stmts, type_ignores=[]), path, "exec")


def reference_lists(code, gt_masks, gt_labels, gt_instance_ids, gt_depth, pad_hw, mask_assign_stride, semantic_kitti):
    """runs the reference's statements on one set of frames: the names they read are bound here (`self` to the three attributes they use,
    `img_metas` to the padded size), the names they leave are read back"""
    scope = dict(torch=torch, F=F, img_metas=[dict(batch_input_shape=pad_hw)], gt_masks=gt_masks, gt_labels=gt_labels,
                 gt_instance_ids=gt_instance_ids, gt_depth=gt_depth,
                 self=types.SimpleNamespace(mask_assign_stride=mask_assign_stride, semantic_kitti=semantic_kitti, num_thing_classes=NUM_THINGS))
    exec(code, scope)
    return tuple(scope[k] for k in ("gt_masks", "gt_labels", "gt_sem_seg", "gt_sem_cls", "gt_instance_ids", "gt_depth"))


def main():
    torch.set_num_threads(1)
    rng = np.random.default_rng(SEED)
    code = reference_statements()
    out, meta = {}, {"num_thing_classes": NUM_THINGS, "cases": {}}
    for name, (pad_hw, src_hw, stride, nearest, counts) in CASES.items():
        frames = [frame_inputs(rng, src_hw, nt, ns) for nt, ns in counts]
        # a ramp: every source pixel has its own value, so a depth output names the pixel it was read from
        depth = (np.arange(len(frames) * pad_hw[0] * pad_hw[1], dtype=np.float32) * 0.0078125 + 0.5).reshape((len(frames), 1) + pad_hw)
        keep = [lab >= 0 for _, lab, _, _ in frames]                  # the loader's list: the dropped segment is not in it
        lists = reference_lists(code, [BitmapMasks(m[k], *src_hw) for (m, _, _, _), k in zip(frames, keep)],
                                [torch.from_numpy(lab[k]) for (_, lab, _, _), k in zip(frames, keep)],
                                [torch.from_numpy(ids[k]) for (_, _, ids, _), k in zip(frames, keep)],
                                torch.from_numpy(depth), pad_hw, stride, nearest)
        gm, gl, ss, sc, ids, gd = lists
        assert tuple(gd.shape[-2:]) == (pad_hw[0] // stride, pad_hw[1] // stride)
        out[f"{name}.depth"] = depth
        out[f"{name}.gt_depth"] = gd.numpy()
        for f, (m, lab, iid, lmap) in enumerate(frames):
            assert (gm[f].shape[0], ss[f].shape[0]) == counts[f]
            out[f"{name}.{f}.label_map"] = lmap
            out[f"{name}.{f}.labels"] = lab
            out[f"{name}.{f}.instance_ids"] = iid
            out[f"{name}.{f}.gt_masks"] = gm[f].numpy()
            out[f"{name}.{f}.gt_labels"] = gl[f].numpy()
            out[f"{name}.{f}.gt_sem_seg"] = ss[f].numpy()
            out[f"{name}.{f}.gt_sem_cls"] = sc[f].numpy()
            out[f"{name}.{f}.gt_instance_ids"] = ids[f].numpy()
            out[f"{name}.{f}.valid"] = torch.cat((gm[f], ss[f])).sum(0).bool().float().numpy()          # kernel_head.py:415
        if stride == 4 and not nearest and pad_hw[0] % 4 == 0 and pad_hw[1] % 4 == 0:
            vals = set(np.unique(np.concatenate([g.numpy().ravel() for g in gm + ss])).tolist())
            assert {0.0, 0.25, 0.5, 0.75, 1.0} == vals, vals       # every partial coverage of the 2 x 2 taps occurs
        if nearest:
            assert all(set(np.unique(g.numpy()).tolist()) <= {0.0, 1.0} for g in gm + ss)
        meta["cases"][name] = dict(pad_hw=pad_hw, src_hw=src_hw, stride=stride, nearest=nearest, frames=len(frames))
    for f in range(2):                                             # s4 (key) and near (reference) make a video pair: some things have a partner
        k, r = out[f"s4.{f}.gt_instance_ids"], out[f"near.{f}.gt_instance_ids"]
        assert 0 < len(np.intersect1d(k, r)) < len(k), (f, k, r)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
