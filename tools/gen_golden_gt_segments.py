"""Fixture for the ground truth from panoptic id maps (tests/golden/gt_segments.npz), produced on the CPU by the reference's own
statements, which the generator reads from the reference tree (oracle/ref_loader.REF_ROOT) when it runs:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_gt_segments.py

Per frame the file records the inputs -- a small crafted raw id map (class * 1000 + instance, as Cityscapes-DVPS stores it), a raw
uint16 depth map, the augmentation -- and what the reference's loader holds after each of its steps.  The statements that are numpy only
are taken out of the reference's files by name or line range, compiled under the file's own name and run; nothing of them is kept here:

    datasets/cityscapes_dvps.py     the class tuples and constants, `to_coco`                          -> the mapped id map, the class map
    datasets/pipelines/loading.py   :201-220 of LoadAnnotationsDirect.__call__, `bitmasks2bboxes`      -> ids, labels, masks, boxes
    mmdet/datasets/pipelines/transforms.py   Resize._resize_bboxes, RandomFlip.bbox_flip               -> boxes after resize and flip
    datasets/pipelines/transforms.py   :233-268 of SeqRandomCropWithDepth.random_crop                  -> boxes, valid, kept lists, cropped
                                                                                                          masks and depth

NOT executed: the nearest resize of the masks and the depth map, which is cv2's.  For that step the generator gathers with the tables of
`gt.nearest_tables`, and the fixture records those tables: what the tests pin for a ratio other than 1 is that restatement of OpenCV's
documented rule, not OpenCV.  The depth decode (uint16 / 256, values >= 80 become 80: loading.py:171-173 around an image read), the
horizontal flip of the maps and the zero pad are one numpy expression each and are written out below.

The masks after the last step are stored as one index map per frame (the index of the kept mask that covers the pixel, 255 for none).

Cases, 3 frames each (the smallest maps at which the kernels can still go wrong):
    a   37 x 53: 13 segments (two ids that share their low ten bits, two in one bitmap word, a one-pixel segment, a segment one pixel
        wide, segments on every border, no-object pixels) | all no-object | one stuff segment
    b   64 x 128: 254 segments | 13 segments | three stuff segments, no things
Augmentations: identity, a crop with an offset, a flip with a crop, ratio 1.37 with flip and crop, ratio 2.0."""
import ast
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "gt_segments.npz")
SEED = 2309
DIVISOR = 10000
# name: (resize ratio, flip, crop offset (y, x) or None, crop size (h, w)); the crop of "crop" runs past the image's bottom edge in case a
AUGS = {"ident": (1.0, False, None, None), "crop": (1.0, False, (9, 14), (30, 32)), "flip": (1.0, True, (2, 5), (32, 48)),
        "r137": (1.37, True, (6, 3), (40, 64)), "r2": (2.0, False, None, None)}


class NumpyWithInt:
    """numpy as the reference's statements were written against it: `np.int` was an alias of `int` until numpy 1.24"""
    int = int

    def __getattr__(self, name):
        return getattr(np, name)


NP = NumpyWithInt()


class BitmapMasks:
    """what the statements below use of mmdet.core.mask.structures.BitmapMasks: the stacked masks, height, width, indexing by an index
    array, crop by (x1, y1, x2, y2)"""

    def __init__(self, masks, height, width):
        self.height, self.width = height, width
        self.masks = np.stack(masks).reshape(-1, height, width) if len(masks) else np.empty((0, height, width), dtype=np.uint8)

    def __getitem__(self, index):
        m = self.masks[index].reshape(-1, self.height, self.width)
        return BitmapMasks(m, self.height, self.width)

    def crop(self, bbox):
        x1, y1, x2, y2 = (int(v) for v in bbox)
        x1, x2 = np.clip([x1, x2], 0, self.width)
        y1, y2 = np.clip([y1, y2], 0, self.height)
        w, h = max(x2 - x1, 1), max(y2 - y1, 1)
        return BitmapMasks(self.masks[:, y1:y1 + h, x1:x1 + w], h, w)


def _source(relpath):
    from oracle import ref_loader
    path = os.path.join(ref_loader.REF_ROOT, relpath)
    with open(path) as f:
        return path, ast.parse(f.read())


def _compile(stmts, path):
    return compile(ast.fix_missing_locations(ast.Module(body=stmts, type_ignores=[])), path, "exec")


def _function(tree, name, cls=None):
    """the module-level function `name`, or the method `name` of class `cls`"""
    scope = tree.body if cls is None else next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    return next(n for n in scope if isinstance(n, ast.FunctionDef) and n.name == name)


def _statements(tree, path, cls, func, first, last):
    """the statements first .. last of the method's body; the range has to be whole statements of it, or this raises"""
    body = _function(tree, func, cls).body
    stmts = [s for s in body if first <= s.lineno and s.end_lineno <= last]
    inside = [s for s in body if s.lineno <= last and s.end_lineno >= first]
    if not stmts or stmts != inside or stmts[0].lineno != first or stmts[-1].end_lineno != last:
        raise RuntimeError(f"{path}:{first}-{last} is not a run of whole statements of {func}: the reference has moved")
    return stmts


def reference_code():
    """-> namespace with to_coco, the dataset's constants, bitmasks2bboxes, resize_bboxes(self, results), bbox_flip(self, ...),
    `loading` (code of loading.py:201-220) and crop(self, results, ...) (transforms.py:233-268 as a function: they hold a return)"""
    ns = dict(np=NP, BitmapMasks=BitmapMasks)
    path, tree = _source("datasets/cityscapes_dvps.py")
    names = {"CLASSES", "THING_CLASSES", "STUFF_CLASSES", "NO_OBJ", "NO_OBJ_HB", "DIVISOR_PAN", "NUM_THING", "NUM_STUFF"}
    consts = [s for s in tree.body if isinstance(s, ast.Assign) and all(isinstance(t, ast.Name) and t.id in names for t in s.targets)]
    assert {t.id for s in consts for t in s.targets} == names
    exec(_compile(consts + [_function(tree, "to_coco")], path), ns)
    path, tree = _source("datasets/pipelines/loading.py")
    exec(_compile([_function(tree, "bitmasks2bboxes")], path), ns)
    ns["loading"] = _compile(_statements(tree, path, "LoadAnnotationsDirect", "__call__", 201, 220), path)
    path, tree = _source("mmdet/datasets/pipelines/transforms.py")
    exec(_compile([_function(tree, "_resize_bboxes", "Resize"), _function(tree, "bbox_flip", "RandomFlip")], path), ns)
    path, tree = _source("datasets/pipelines/transforms.py")
    shell = ast.parse("def crop(self, results, offset_h, offset_w, img_shape, crop_y1, crop_y2, crop_x1, crop_x2):\n    pass\n"
                      "    return results, valid_inds\n").body[0]
    shell.body = _statements(tree, path, "SeqRandomCropWithDepth", "random_crop", 233, 268) + shell.body[1:]
    exec(_compile([shell], path), ns)
    return types.SimpleNamespace(**ns)


def class_map(ref):
    """raw class -> training class as to_coco maps it, read off to_coco itself: one pixel per raw class"""
    cm = np.full(ref.NO_OBJ + 1, -1, np.int32)
    for c in range(ref.NO_OBJ + 1):
        try:
            cm[c] = int(ref.to_coco(np.array([[c * ref.DIVISOR_PAN]], np.float32), DIVISOR)[0, 0]) // DIVISOR
        except KeyError:
            pass
    assert cm[ref.NO_OBJ] == ref.NO_OBJ_HB and (cm >= 0).sum() == len(ref.CLASSES) + 1
    return cm


def blocky(rng, hw, block, values):
    """[H][W] map of `values`, constant on blocks, every value at least once"""
    H, W = hw
    gh, gw = -(-H // block[0]), -(-W // block[1])
    assert gh * gw >= len(values)
    cells = np.concatenate([np.arange(len(values)), rng.integers(0, len(values), gh * gw - len(values))])
    coarse = np.asarray(values)[rng.permutation(cells)].reshape(gh, gw)
    return np.kron(coarse, np.ones(block, np.int64))[:H, :W].astype(np.int32)


def frames_of(rng, ref, case):
    raw_cls = lambda name: ref.CLASSES.index(name)
    no = ref.NO_OBJ * ref.DIVISOR_PAN
    car, person, bike = raw_cls("car") * 1000, raw_cls("person") * 1000, raw_cls("bicycle") * 1000
    stuff = [raw_cls(n) * 1000 for n in ("road", "sidewalk", "building", "sky", "vegetation", "pole")]
    if case == "a":
        hw = (37, 53)
        twin = (car + 8 - person) % 1024                        # person + twin and car + 8 share their low ten bits
        assert 0 < twin < 1000
        ids11 = stuff[:4] + [car + 8, person + twin, car + 1, car + 2, car + 33, bike + 999, person + 1]   # car 1, car 2: one bitmap word
        f0 = blocky(rng, hw, (5, 6), ids11 + [no])
        f0[17, 29] = bike + 7                                   # a one-pixel segment
        f0[3:20, 41] = car + 77                                 # one pixel wide
        f1 = np.full(hw, no, np.int32)
        f2 = np.full(hw, stuff[0], np.int32)
        f2[30:, 40:] = no
        return [f0, f1, f2]
    hw = (64, 128)
    ids254 = [c + i for c in (car, person, bike) for i in range(1, 82)] + stuff + [raw_cls("truck") * 1000 + i for i in (5, 517, 1 + 512, 999, 0)]
    assert len(set(ids254)) == 254
    f0 = blocky(rng, hw, (4, 8), ids254 + [no])
    f1 = blocky(rng, hw, (7, 9), stuff[:5] + [car + i for i in (3, 4, 900)] + [person + i for i in (3, 4, 5, 6)] + [bike + 2, no])
    f2 = blocky(rng, hw, (16, 32), stuff[:3])
    return [f0, f1, f2]


def depth_of(rng, hw):
    d = rng.integers(0, 65536, hw).astype(np.uint16)
    d[0, :6] = [20477, 20479, 20480, 20481, 65535, 0]           # 79.99, just below 80, 80.0, just above, 255.996, 0
    d[-1, -3:] = [20480, 65535, 1]
    return d


def run_frame(ref, raw, raw_depth, aug, pad_hw):
    """one frame through the loader -> dict of recorded arrays"""
    from polyphonicformer_amd import gt as GT
    ratio, flip, off, chw = aug
    H, W = raw.shape
    out = {}
    # 1. loading
    ps_id = ref.to_coco(raw.astype(np.float32), DIVISOR)
    scope = dict(np=NP, BitmapMasks=BitmapMasks, ps_id=ps_id, self=types.SimpleNamespace(divisor=DIVISOR),
                 results=dict(no_obj_class=ref.NO_OBJ_HB, img_shape=(H, W, 3)))
    exec(ref.loading, scope)
    gt_labels, gt_ids, gt_masks = scope["gt_labels"], scope["gt_instance_ids"], scope["gt_masks"]
    boxes = ref.bitmasks2bboxes(gt_masks)
    depth = raw_depth.astype(np.float32) / 256.
    depth[depth >= 80.] = 80.
    out.update(ids=gt_ids.astype(np.int64), labels=gt_labels.astype(np.int64), boxes=boxes,
               areas=gt_masks.masks.reshape(len(gt_ids), H * W).sum(1).astype(np.int64))
    # 2. resize: the boxes by the reference, the maps by the tables (cv2's step)
    nh, nw = int(H * ratio + 0.5), int(W * ratio + 0.5)          # mmcv.rescale_size
    ry, rx, scale, _ = GT.nearest_tables((H, W), (nh, nw), flip, None, None)
    sy, sx, scale2, out_hw = GT.nearest_tables((H, W), (nh, nw), flip, off, chw)
    assert (scale == scale2).all()
    rself = types.SimpleNamespace(bbox_clip_border=True, allow_negative_crop=True,
                                  bbox2label={'gt_bboxes': ['gt_labels', 'gt_instance_ids']}, bbox2mask={'gt_bboxes': 'gt_masks'})
    results = dict(bbox_fields=['gt_bboxes'], gt_bboxes=boxes, scale_factor=scale, img_shape=(nh, nw, 3), gt_labels=gt_labels,
                   gt_instance_ids=gt_ids, depth_fields=['gt_depth'], seg_fields=[])
    ref._resize_bboxes(rself, results)
    masks = gt_masks.masks[:, ry][:, :, rx] if len(gt_ids) else np.empty((0, nh, nw), gt_masks.masks.dtype)   # resized AND flipped
    depth = depth[ry][:, rx].copy()
    depth /= scale.mean()
    # 3. flip
    if flip:
        results['gt_bboxes'] = ref.bbox_flip(rself, results['gt_bboxes'], (nh, nw, 3), 'horizontal')
    results['gt_masks'], results['gt_depth'] = BitmapMasks(masks, nh, nw), depth
    valid = np.ones(len(gt_ids), bool)
    # 4. crop
    if off is not None:
        oy, ox = off
        img_shape = np.empty((nh, nw, 3), np.uint8)[oy:oy + chw[0], ox:ox + chw[1]].shape
        results, valid = ref.crop(rself, results, oy, ox, img_shape, oy, oy + chw[0], ox, ox + chw[1])
    m, d = results['gt_masks'].masks, results['gt_depth']
    assert m.shape[1:] == out_hw == d.shape, (m.shape, out_hw, d.shape)
    # 5. pad
    index = np.full(out_hw, 255, np.uint8)
    assert m.shape[0] <= 254 and (m.sum(0) <= 1).all()
    for i in range(m.shape[0]):
        index[m[i] != 0] = i
    dpad = np.zeros(pad_hw, np.float32)
    dpad[:out_hw[0], :out_hw[1]] = d
    out.update(src_y=sy, src_x=sx, scale_factor=scale, aug_boxes=results['gt_bboxes'], valid=np.asarray(valid, bool),
               kept_ids=np.asarray(results['gt_instance_ids'], np.int64), kept_labels=np.asarray(results['gt_labels'], np.int64),
               index_map=index, depth=dpad, resized_hw=np.array([nh, nw]))
    return out


def main():
    rng = np.random.default_rng(SEED)
    ref = reference_code()
    cm = class_map(ref)
    out = {"class_map": cm}
    meta = dict(raw_divisor=int(ref.DIVISOR_PAN), divisor=DIVISOR, no_obj_class=int(ref.NO_OBJ_HB), num_thing_classes=int(ref.NUM_THING),
                cases={}, augs={k: dict(ratio=r, flip=f, crop_offset=o, crop_hw=c) for k, (r, f, o, c) in AUGS.items()})
    for case in ("a", "b"):
        raws = frames_of(rng, ref, case)
        hw = raws[0].shape
        depths = [depth_of(rng, hw) for _ in raws]
        out[f"{case}.raw"], out[f"{case}.raw_depth"] = np.stack(raws), np.stack(depths)
        meta["cases"][case] = dict(hw=hw, frames=len(raws), pad={})
        for an, aug in AUGS.items():
            recs = []
            for f, (raw, dep) in enumerate(zip(raws, depths)):
                nh, nw = int(hw[0] * aug[0] + 0.5), int(hw[1] * aug[0] + 0.5)
                o_hw = (nh, nw) if aug[2] is None else (min(aug[3][0], nh - aug[2][0]), min(aug[3][1], nw - aug[2][1]))
                pad_hw = (-(-o_hw[0] // 8) * 8 + 8, -(-o_hw[1] // 8) * 8)            # a pad on both sides of a multiple of 4
                recs.append(run_frame(ref, raw, dep, aug, pad_hw))
                meta["cases"][case]["pad"][an] = pad_hw
            for f, rec in enumerate(recs):
                for k, v in rec.items():
                    if an == "ident" or k not in ("ids", "labels", "boxes", "areas"):
                        out[f"{case}.{an}.{f}.{k}"] = v
        counts = [len(out[f"{case}.ident.{f}.ids"]) for f in range(len(raws))]
        assert counts == ([13, 0, 1] if case == "a" else [254, 13, 3]), counts
    a0 = out["a.ident.0.boxes"]
    assert ((a0[:, 0] == a0[:, 2]) | (a0[:, 1] == a0[:, 3])).sum() >= 2                          # the one-pixel and the one-wide segment
    assert a0[:, 0].min() == 0 and a0[:, 1].min() == 0 and a0[:, 2].max() == 52 and a0[:, 3].max() == 36
    for an in ("crop", "flip", "r137"):                                                        # dropped, and kept without a pixel
        v = out[f"a.{an}.0.valid"]
        assert not v.all() and v.any(), an
    assert any(set(range(len(out[f"{c}.{an}.{f}.kept_ids"]))) - set(np.unique(out[f"{c}.{an}.{f}.index_map"]).tolist())
               for c in "ab" for an in AUGS for f in range(3)), "no kept segment without a pixel: move a crop"
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
