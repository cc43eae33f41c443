"""CPU: the host side of the ground truth from panoptic id maps (polyphonicformer_amd/gt.py: `nearest_tables`, `transform_boxes`) and
an integer / fp32 numpy restatement of the contracts of `ph_gt_segments` and `ph_gt_index_maps` (include/polyhead.h), against
tests/golden/gt_segments.npz, which tools/gen_golden_gt_segments.py made with the reference's own statements (to_coco,
loading.py:201-220, bitmasks2bboxes, mmdet's _resize_bboxes and bbox_flip, transforms.py:233-268).  tests/test_gpu_gt_segments.py compares
the kernels with the restatement and the fixture.

Everything here is exact: ids, boxes, areas, kept sets and index maps are integers, the depth is two correctly rounded fp32 divisions.

What the fixture does NOT hold is OpenCV: the reference resizes its masks with cv2, which the generator cannot run, so for that step it
gathers with the tables of `gt.nearest_tables` and records them.  The tests of a ratio other than 1 therefore pin that restatement of
OpenCV's documented INTER_NEAREST rule, not the library."""
import ctypes as C
import json

import numpy as np
import pytest

import helpers as Hh
from polyphonicformer_amd import _lib, gt as GT

CASES = ("a", "b")
AUGS = ("ident", "crop", "flip", "r137", "r2")
ROW = _lib.PH_GTSEG_ROW_WORDS


def fixture():
    z = Hh.load_golden("gt_segments.npz")
    return z, json.loads(str(z["meta"]))


def mapping(z, meta):
    return dict(class_map=z["class_map"], raw_divisor=meta["raw_divisor"], divisor=meta["divisor"], no_obj_class=meta["no_obj_class"])


def aug_of(meta, case, an):
    """-> (resized_hw, flip, crop_offset, crop_hw) as `gt.nearest_tables` takes them, and the padded size the fixture used"""
    a, (H, W) = meta["augs"][an], meta["cases"][case]["hw"]
    resized = (int(H * a["ratio"] + 0.5), int(W * a["ratio"] + 0.5))
    off = None if a["crop_offset"] is None else tuple(a["crop_offset"])
    return (resized, a["flip"], off, None if off is None else tuple(a["crop_hw"])), tuple(meta["cases"][case]["pad"][an])


# ---- the contract of ph_gt_segments in numpy ---------------------------------------------------------------------------------------
def np_mapped(raw, class_map, raw_divisor, divisor, no_obj_class):
    """per pixel the mapped id (int64; -1 where the pixel belongs to no segment: no-object, unmapped, outside) and the frame's status"""
    key = np.asarray(raw).astype(np.int64)
    cm = np.asarray(class_map).astype(np.int64)
    inside = (key >= 0) & (key < cm.size * raw_divisor)
    cls = np.where(inside, key // raw_divisor, 0)
    m = np.where(inside, cm[cls], -1)
    status = (_lib.PH_GTSEG_EOUTSIDE if (~inside).any() else 0) | (_lib.PH_GTSEG_EUNMAPPED if (inside & (m < 0)).any() else 0)
    seg = inside & (m >= 0) & (m != no_obj_class)
    return np.where(seg, m * divisor + key % raw_divisor, -1), status


def np_gt_segments(raw, class_map, raw_divisor, divisor, no_obj_class, fill=0):
    """raw [F][Hs][Ws] -> (tables int32 [F][PH_GTSEG_TABLE_WORDS], status int32 [F]); the table of a frame with a status stays `fill`"""
    F_ = len(raw)
    tables = np.full((F_, _lib.PH_GTSEG_TABLE_WORDS), fill, np.int32)
    status = np.zeros(F_, np.int32)
    for f in range(F_):
        mapped, st = np_mapped(raw[f], class_map, raw_divisor, divisor, no_obj_class)
        ids = np.unique(mapped[mapped >= 0])
        if ids.size > _lib.PH_GTPREP_MAX_SEGMENTS:
            st |= _lib.PH_GTSEG_ETOOMANY
        status[f] = st
        if st:
            continue
        tables[f] = 0
        tables[f, 0] = ids.size
        for r, i in enumerate(ids):
            ys, xs = np.nonzero(mapped == i)
            tables[f, 1 + r * ROW:1 + (r + 1) * ROW] = (i, xs.min(), ys.min(), xs.max(), ys.max(), ys.size)
    return tables, status


def table_rows(table):
    """one frame's table -> (ids int64 [n], boxes fp32 [n][4], areas int64 [n]), as gt.segment_tables unpacks it"""
    t = table[1:1 + int(table[0]) * ROW].reshape(-1, ROW)
    return t[:, 0].astype(np.int64), t[:, 1:5].astype(np.float32), t[:, 5].astype(np.int64)


# ---- the contract of ph_gt_index_maps in numpy (every numpy operation rounds once) --------------------------------------------------
def np_gt_index_maps(raw, raw_depth, class_map, raw_divisor, divisor, no_obj_class, kept_ids, src_y, src_x, pad_hw, scale_mean,
                     depth_div=256.0, depth_max=80.0):
    """raw [F][Hs][Ws], kept_ids per frame ascending, src_y [F][Hc], src_x [F][Wc] (-1: none) -> (seg uint8 [F][Hc][Wc], depth fp32
    [F][Hp][Wp] or None)"""
    F_, (Hc, Wc), (Hp, Wp) = len(raw), (len(src_y[0]), len(src_x[0])), pad_hw
    seg = np.full((F_, Hc, Wc), 255, np.uint8)
    depth = None if raw_depth is None else np.zeros((F_, Hp, Wp), np.float32)
    for f in range(F_):
        sy, sx = np.asarray(src_y[f]), np.asarray(src_x[f])
        ok = (sy >= 0)[:, None] & (sx >= 0)[None, :]
        mapped, _ = np_mapped(raw[f], class_map, raw_divisor, divisor, no_obj_class)
        g = mapped[np.maximum(sy, 0)][:, np.maximum(sx, 0)]
        kept = np.asarray(kept_ids[f], np.int64)
        at = np.searchsorted(kept, g)
        hit = ok & (g >= 0) & (at < kept.size)
        hit[hit] = kept[at[hit]] == g[hit]
        seg[f][hit] = at[hit]
        if depth is not None:
            d = raw_depth[f][np.maximum(sy, 0)][:, np.maximum(sx, 0)].astype(np.float32) / np.float32(depth_div)
            d = np.where(d >= np.float32(depth_max), np.float32(depth_max), d) / np.float32(scale_mean[f])
            depth[f, :Hc, :Wc] = np.where(ok, d, np.float32(0))
    return seg, depth


# ---- the loader's bitmask path in numpy: what the device path replaces (also side A of tools/gt_segments_time.py) ----------------------
def np_bitmask_loader(raw, raw_depth, aug, pad_hw, class_map, raw_divisor, divisor, no_obj_class):
    """one frame the reference's way, in its order: the mapped id map, np.unique and one full-frame compare per segment, the boxes of the
    stack, then resize, flip and crop applied to the whole [G][H][W] stack (the resize as a gather with `gt.nearest_tables`), the
    crop's box filter, the depth map alongside -> dict(bitmasks uint8 [n][Hc][Wc], labels, ids, depth fp32 [Hp][Wp])"""
    resized, flip, off, chw = aug
    mapped, status = np_mapped(raw, class_map, raw_divisor, divisor, no_obj_class)
    assert status == 0
    ids = np.unique(mapped)
    ids = ids[ids >= 0]
    masks = np.stack([(mapped == i).astype(np.int64) for i in ids]) if ids.size else np.zeros((0,) + mapped.shape, np.int64)
    boxes = np.zeros((ids.size, 4), np.float32)
    for i, m in enumerate(masks):
        xs, ys = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
        boxes[i] = (xs[0], ys[0], xs[-1], ys[-1])
    ry, rx, scale, _ = GT.nearest_tables(raw.shape, resized, flip, None, None)
    masks = masks[:, ry][:, :, rx]
    depth = raw_depth.astype(np.float32) / np.float32(256)
    depth[depth >= 80] = 80
    depth = depth[ry][:, rx] / scale.mean()
    _, valid = GT.transform_boxes(boxes, scale, resized, flip, off, chw)
    if off is not None:
        masks = masks[valid, off[0]:off[0] + chw[0], off[1]:off[1] + chw[1]]
        depth = depth[off[0]:off[0] + chw[0], off[1]:off[1] + chw[1]]
    dpad = np.zeros(pad_hw, np.float32)
    dpad[:depth.shape[0], :depth.shape[1]] = depth
    return dict(bitmasks=masks.astype(np.uint8), labels=ids[valid] // divisor, ids=ids[valid], depth=dpad)


def kept_of(z, meta, case, an, f):
    """the kept ids of a frame from the FILE's table and `gt.transform_boxes`, as prepare_gt_from_panoptic derives them"""
    (resized, flip, off, chw), _ = aug_of(meta, case, an)
    pre = f"{case}.ident.{f}."
    boxes, valid = GT.transform_boxes(z[pre + "boxes"], z[f"{case}.{an}.{f}.scale_factor"], resized, flip, off, chw)
    return z[pre + "ids"][valid], boxes, valid


@pytest.mark.parametrize("case", CASES)
def test_segment_restatement_equals_the_reference_lists(case):
    z, meta = fixture()
    tables, status = np_gt_segments(z[f"{case}.raw"], **mapping(z, meta))
    assert not status.any()
    for f in range(meta["cases"][case]["frames"]):
        ids, boxes, areas = table_rows(tables[f])
        pre = f"{case}.ident.{f}."
        assert np.array_equal(ids, z[pre + "ids"]) and np.array_equal(ids // meta["divisor"], z[pre + "labels"])
        assert boxes.dtype == z[pre + "boxes"].dtype and np.array_equal(boxes, z[pre + "boxes"])
        assert np.array_equal(areas, z[pre + "areas"])
        assert not tables[f, 1 + ids.size * ROW:].any()
    assert [int(t[0]) for t in tables] == ([13, 0, 1] if case == "a" else [254, 13, 3])


def test_segment_restatement_reports_status():
    z, meta = fixture()
    m = mapping(z, meta)
    raw = z["a.raw"].copy()
    raw[0, 0, 0] = 19 * 1000                                   # a class the map sends to -1
    raw[1, 5, 5] = 40 * 1000                                   # a class beyond the map
    raw[2, 1, 1] = -3
    tables, status = np_gt_segments(raw, fill=-7, **m)
    assert status.tolist() == [_lib.PH_GTSEG_EUNMAPPED, _lib.PH_GTSEG_EOUTSIDE, _lib.PH_GTSEG_EOUTSIDE] and (tables == -7).all()
    raw = z["b.raw"].copy()
    raw[0, 0, 0] = 13 * 1000 + 998                             # a 255th segment
    raw[1, 0, 0] = 0 * 1000 + 5                                # a stuff id with an instance part is a segment like any other
    tables, status = np_gt_segments(raw, fill=-7, **m)
    assert status.tolist() == [_lib.PH_GTSEG_ETOOMANY, 0, 0] and (tables[0] == -7).all() and tables[1, 0] == 14


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("an", AUGS)
def test_transform_boxes_equals_the_reference(case, an):
    z, meta = fixture()
    for f in range(meta["cases"][case]["frames"]):
        kept, boxes, valid = kept_of(z, meta, case, an, f)
        pre = f"{case}.{an}.{f}."
        assert np.array_equal(valid, z[pre + "valid"])
        assert boxes.dtype == np.float32 and np.array_equal(boxes[valid], z[pre + "aug_boxes"])
        assert np.array_equal(kept, z[pre + "kept_ids"]) and np.array_equal(kept // meta["divisor"], z[pre + "kept_labels"])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("an", AUGS)
def test_index_map_restatement_equals_the_reference(case, an):
    """the id map gathered through the tables and looked up in the kept list IS the reference's stack of resized, flipped, cropped
    masks; the depth has numpy's bits"""
    z, meta = fixture()
    (resized, flip, off, chw), pad_hw = aug_of(meta, case, an)
    F_ = meta["cases"][case]["frames"]
    tabs = [GT.nearest_tables(meta["cases"][case]["hw"], resized, flip, off, chw) for _ in range(F_)]
    kept = [kept_of(z, meta, case, an, f)[0] for f in range(F_)]
    seg, depth = np_gt_index_maps(z[f"{case}.raw"], z[f"{case}.raw_depth"], kept_ids=kept, src_y=[t[0] for t in tabs], src_x=[t[1] for t in tabs],
                                  pad_hw=pad_hw, scale_mean=[t[2].mean() for t in tabs], **mapping(z, meta))
    for f in range(F_):
        pre = f"{case}.{an}.{f}."
        assert np.array_equal(tabs[f][0], z[pre + "src_y"]) and np.array_equal(tabs[f][1], z[pre + "src_x"])
        assert np.array_equal(tabs[f][2], z[pre + "scale_factor"]) and tabs[f][2].dtype == np.float32
        assert np.array_equal(seg[f], z[pre + "index_map"])
        assert np.array_equal(depth[f].view(np.uint32), z[pre + "depth"].view(np.uint32))
    if (case, an) == ("a", "ident"):                           # 79.99, 80.0 and 255.996 of the raw depth
        assert depth[0, 0, :6].tolist() == [np.float32(20477 / 256), np.float32(20479 / 256), 80.0, 80.0, 80.0, 0.0]


@pytest.mark.parametrize("an", ("crop", "r137"))
def test_bitmask_loader_equals_the_reference(an):
    """the numpy loader the GPU end-to-end test and the timing tool compare the device path with gives the reference's lists"""
    z, meta = fixture()
    aug, pad_hw = aug_of(meta, "b", an)
    for f in range(3):
        got = np_bitmask_loader(z["b.raw"][f], z["b.raw_depth"][f], aug, pad_hw, **mapping(z, meta))
        pre = f"b.{an}.{f}."
        assert np.array_equal(got["ids"], z[pre + "kept_ids"]) and np.array_equal(got["labels"], z[pre + "kept_labels"])
        assert np.array_equal(GT.index_map_from_bitmasks(got["bitmasks"]), z[pre + "index_map"])
        assert np.array_equal(got["depth"].view(np.uint32), z[pre + "depth"].view(np.uint32))


def test_a_kept_segment_without_a_pixel_and_a_dropped_thin_one():
    """the crop's test is on the box: the fixture holds a kept segment that has no pixel in the crop (its index does not occur) and a
    segment one pixel wide that is dropped although the crop holds pixels of it (they read 255)"""
    z, meta = fixture()
    unused = thin = 0
    for case in CASES:
        for an in ("crop", "flip", "r137"):
            for f in range(3):
                pre = f"{case}.{an}.{f}."
                kept, valid, imap = z[pre + "kept_ids"], z[pre + "valid"], z[pre + "index_map"]
                unused += len(set(range(len(kept))) - set(np.unique(imap).tolist()))
                ids, boxes = z[f"{case}.ident.{f}.ids"], z[f"{case}.ident.{f}.boxes"]
                mapped, _ = np_mapped(z[f"{case}.raw"][f], **mapping(z, meta))
                g = mapped[z[pre + "src_y"]][:, z[pre + "src_x"]]
                for i in ids[~valid & ((boxes[:, 0] == boxes[:, 2]) | (boxes[:, 1] == boxes[:, 3]))]:
                    if (g == i).any():
                        thin += 1
                        assert (imap[g == i] == 255).all()
    assert unused and thin


@pytest.mark.parametrize("ratio", (1.0, 2.0, 1.37))
@pytest.mark.parametrize("flip", (False, True))
def test_nearest_tables_are_monotone_and_in_range(ratio, flip):
    H, W = 37, 53
    nh, nw = int(H * ratio + 0.5), int(W * ratio + 0.5)
    off, chw = (3, 5), (nh - 5, nw - 9)
    sy, sx, scale, out_hw = GT.nearest_tables((H, W), (nh, nw), flip, off, chw)
    assert sy.dtype == sx.dtype == np.int32 and out_hw == chw == (sy.size, sx.size)
    assert sy.min() >= 0 and sy.max() < H and sx.min() >= 0 and sx.max() < W
    assert (np.diff(sy) >= 0).all() and (np.diff(sx) <= 0 if flip else np.diff(sx) >= 0).all()
    assert scale.dtype == np.float32 and scale.tolist() == [np.float32(nw / W), np.float32(nh / H)] * 2
    fy, fx, _, full = GT.nearest_tables((H, W), (nh, nw), flip, None, None)
    assert full == (nh, nw) and set(fy.tolist()) == set(range(H)) and set(fx.tolist()) == set(range(W))      # an upscale loses no pixel
    if ratio == 1.0 and not flip:
        assert np.array_equal(sy, np.arange(3, 3 + chw[0])) and np.array_equal(sx, np.arange(5, 5 + chw[1]))
    if ratio == 1.0 and flip:
        assert np.array_equal(sx, (W - 1 - np.arange(W))[5:5 + chw[1]])
    if ratio == 2.0:
        assert np.array_equal(fy, np.arange(nh) // 2) and np.array_equal(fx, (np.arange(nw) // 2)[::-1] if flip else np.arange(nw) // 2)
    # a crop that runs past the resized image is clipped as the reference's slice is
    assert GT.nearest_tables((H, W), (nh, nw), flip, (nh - 4, nw - 6), (10, 10))[3] == (4, 6)


def test_argument_errors_come_back_before_any_launch():
    """the checks of both calls run on the host before the first launch, so they answer on a machine without a GPU"""
    lib = _lib.load()
    fake = C.c_void_p(256)
    cm = (C.c_int32 * 33)(*([-1] * 33))
    for c, m in ((11, 0), (13, 2), (0, 8), (32, 255)):
        cm[c] = m

    def seg(dtype=0, frames=2, Hs=37, Ws=53, class_map=cm, n_map=33, raw_divisor=1000, divisor=10000, no_obj=255, tables=fake, ws=fake,
            ws_bytes=1 << 30):
        return lib.ph_gt_segments(fake, dtype, frames, Hs, Ws, class_map, n_map, raw_divisor, divisor, no_obj, tables, fake, ws, ws_bytes, None)

    twice = (C.c_int32 * 33)(*cm)
    twice[12] = 2
    bad = (C.c_int32 * 33)(*cm)
    bad[3] = 256
    for kw, rc, word in ((dict(Hs=0), _lib.PH_EINVAL, "sizes"), (dict(Ws=-1), _lib.PH_EINVAL, "sizes"), (dict(frames=0), _lib.PH_EINVAL, "frames"),
                         (dict(frames=65), _lib.PH_EINVAL, "frames"), (dict(dtype=2), _lib.PH_EINVAL, "dtype"),
                         (dict(n_map=257), _lib.PH_EINVAL, "raw classes"), (dict(divisor=999), _lib.PH_EINVAL, "raw_divisor <= divisor"),
                         (dict(class_map=twice), _lib.PH_EINVAL, "two raw classes"), (dict(class_map=bad), _lib.PH_EINVAL, "training class"),
                         (dict(n_map=33, raw_divisor=8000, divisor=10000), -2, "presence bitmap"), (dict(tables=None), _lib.PH_EINVAL, "null"),
                         (dict(ws_bytes=64), _lib.PH_EWORKSPACE, "workspace"), (dict(ws=None), _lib.PH_EINVAL, "workspace")):
        assert seg(**kw) == rc, kw
        err = Hh.last_error()
        assert err.startswith("ph_gt_segments") and word in err, (kw, err)
    assert lib.ph_gt_segments_workspace_bytes(2, 33, 8000) == 0 and lib.ph_gt_segments_workspace_bytes(0, 33, 1000) == 0
    assert lib.ph_gt_segments_workspace_bytes(3, 33, 1000) >= 3 * (33000 // 8 + 2 * 254 * 4)
    assert _lib.PH_GTSEG_MAX_KEYS == 262144 and _lib.PH_GTSEG_TABLE_WORDS == 1 + 254 * 6

    def idx(Hs=37, Ws=53, Hc=4, Wc=5, Hp=8, Wp=8, kept_n=(3, 254), sy=None, sx=None, depth=False, scale=(1.0, 1.37)):
        n = (C.c_int32 * len(kept_n))(*kept_n)
        hy = (C.c_int32 * (len(kept_n) * max(Hc, 1)))(*(sy if sy is not None else [0, 1, 36, -1] * len(kept_n)))
        hx = (C.c_int32 * (len(kept_n) * max(Wc, 1)))(*(sx if sx is not None else [52, 0, -1, 3, 3] * len(kept_n)))
        sm = (C.c_float * len(kept_n))(*scale)
        return lib.ph_gt_index_maps(fake, 1, fake if depth else None, len(kept_n), Hs, Ws, cm, 33, 1000, 10000, 255, fake, n, hy, hx, fake, fake,
                                    Hc, Wc, Hp, Wp, 256.0, 80.0, sm, fake, fake if depth else None, None)

    for kw, word in ((dict(sy=[0, 1, 37, 0] * 2), "src_y[0][2] = 37"), (dict(sy=[0, 1, 2, 3, 0, 0, -2, 0]), "src_y[1][2] = -2"),
                     (dict(sx=[0, 0, 0, 0, 53] * 2), "src_x[0][4] = 53"), (dict(kept_n=(3, 255)), "kept segments"), (dict(Hs=0), "sizes"),
                     (dict(Hp=3), "Hc <= Hp"), (dict(Wp=4), "Wc <= Wp"), (dict(depth=True, scale=(1.0, 0.0)), "scale_mean[1]")):
        assert idx(**kw) == _lib.PH_EINVAL, kw
        err = Hh.last_error()
        assert err.startswith("ph_gt_index_maps") and word in err, (kw, err)
