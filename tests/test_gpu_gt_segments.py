"""GPU: `ph_gt_segments` and `ph_gt_index_maps` (csrc/ph_gtseg.hip) and what stands on them -- `gt.segment_tables`,
`gt.prepare_gt_from_panoptic` -- against tests/golden/gt_segments.npz (the reference's own statements,
tools/gen_golden_gt_segments.py) and the numpy restatement of the two contracts in tests/test_gt_segments_host.py.

Bounds: none, everything is exact.  Tables, status words and index maps are integers; the depth is two correctly rounded fp32 divisions
and is compared by its bits.  The maps are 37 x 53 (Wc = 53: byte stores) and 64 x 128 (Wc = 128, 48, 32: 16-byte stores), three frames
a call with 13 / 0 / 1 and 254 / 13 / 3 segments.  For a ratio other than 1 the fixture pins the restatement of OpenCV's nearest rule in
`gt.nearest_tables`, not OpenCV (see the host file).

Status bits are found on the device, so a call that reports one HAS launched; what the tests hold it to is that the refused frame's
table stays as the caller left it and the other frames of the call are served.  The argument errors launch nothing at all."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, gt as GT, train as TR
from test_gt_segments_host import (AUGS, CASES, aug_of, fixture, kept_of, mapping, np_bitmask_loader, np_gt_index_maps, np_gt_segments,
                                   table_rows)
from test_gpu_video_train import video_parts  # noqa: F401  (the fixture: neck and the two heads as the step tests build them)

pytestmark = pytest.mark.gpu

FILL = 0x7F7F7F7F
DTYPES = (np.int32, np.uint16)


def _dev(gpu, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _segments(gpu, raw, m, dtype=np.int32, tables=None, status=None, workspace=None):
    """one call on host maps `raw`; tables and status pre-filled with FILL -> (tables, status) as numpy"""
    r = _dev(gpu, raw.astype(dtype))
    tables = torch.full((len(raw), _lib.PH_GTSEG_TABLE_WORDS), FILL, dtype=torch.int32, device=gpu) if tables is None else tables
    status = torch.full((len(raw),), FILL, dtype=torch.int32, device=gpu) if status is None else status
    GT.gt_segments(r, _lib.PH_GTSEG_I32 if dtype == np.int32 else _lib.PH_GTSEG_U16, m["class_map"], m["raw_divisor"], m["divisor"],
                   m["no_obj_class"], tables=tables, status=status, workspace=workspace)
    return tables.cpu().numpy(), status.cpu().numpy()


def _index_args(z, meta, case, an):
    """the arguments of one `ph_gt_index_maps` call for a case and an augmentation, all frames"""
    (resized, flip, off, chw), pad_hw = aug_of(meta, case, an)
    F_ = meta["cases"][case]["frames"]
    tabs = [GT.nearest_tables(meta["cases"][case]["hw"], resized, flip, off, chw) for _ in range(F_)]
    return dict(kept_ids=[kept_of(z, meta, case, an, f)[0] for f in range(F_)], src_y=np.stack([t[0] for t in tabs]),
                src_x=np.stack([t[1] for t in tabs]), pad_hw=pad_hw, scale_mean=np.array([t[2].mean() for t in tabs], np.float32))


def _filled_outs(gpu, F_, out_hw, pad_hw, offset=0):
    """seg filled with 0xFF starting `offset` bytes into its allocation, depth filled with NaN"""
    n = F_ * out_hw[0] * out_hw[1]
    seg = torch.full((n + 16,), 0xFF, dtype=torch.uint8, device=gpu)[offset:offset + n].view(F_, *out_hw)
    return seg, torch.full((F_,) + tuple(pad_hw), float("nan"), dtype=torch.float32, device=gpu)


def _index_maps(gpu, raw, raw_depth, m, a, dtype=np.int32, offset=0, frames=None):
    idx = list(range(len(raw))) if frames is None else list(frames)
    pick = lambda x: [x[i] for i in idx] if isinstance(x, list) else x[idx]
    out = _filled_outs(gpu, len(idx), (a["src_y"].shape[1], a["src_x"].shape[1]), a["pad_hw"], offset)
    assert out[0].data_ptr() % 16 == offset
    seg, depth = GT.gt_index_maps(_dev(gpu, raw[idx].astype(dtype)), _lib.PH_GTSEG_I32 if dtype == np.int32 else _lib.PH_GTSEG_U16,
                                  None if raw_depth is None else _dev(gpu, raw_depth[idx]), m["class_map"], m["raw_divisor"], m["divisor"],
                                  m["no_obj_class"], pick(a["kept_ids"]), pick(a["src_y"]), pick(a["src_x"]), a["pad_hw"],
                                  scale_mean=pick(a["scale_mean"]), out=out)
    return seg, depth


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. ph_gt_segments against the fixture and the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_segments_equal_the_reference_lists(gpu, case):
    """ids that share their low bits and their bitmap word, segments on every border, a one-pixel segment, a frame that is all
    no-object, 254 segments; int32 and uint16 maps give the same table; FILL-ed tables come back fully written"""
    z, meta = fixture()
    m = mapping(z, meta)
    raw = z[f"{case}.raw"]
    want, _ = np_gt_segments(raw, **m)
    for dtype in DTYPES:
        tables, status = _segments(gpu, raw, m, dtype)
        assert not status.any() and np.array_equal(tables, want), dtype
    for f in range(len(raw)):
        ids, boxes, areas = table_rows(tables[f])
        pre = f"{case}.ident.{f}."
        assert np.array_equal(ids, z[pre + "ids"]) and np.array_equal(boxes, z[pre + "boxes"]) and np.array_equal(areas, z[pre + "areas"])
    assert tables[:, 0].tolist() == ([13, 0, 1] if case == "a" else [254, 13, 3])
    tabs = GT.segment_tables(raw, device=gpu, **m)
    for f, t in enumerate(tabs):
        pre = f"{case}.ident.{f}."
        assert np.array_equal(t.ids, z[pre + "ids"]) and t.boxes.dtype == np.float32 and np.array_equal(t.boxes, z[pre + "boxes"])
        assert np.array_equal(t.ids // m["divisor"], z[pre + "labels"]) and np.array_equal(t.areas, z[pre + "areas"])


# ---- 2. status words: the refused frame's table stays as it was, its neighbours are served ----------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_status_words(gpu, dtype):
    z, meta = fixture()
    m = mapping(z, meta)
    raw = z["b.raw"].copy()
    raw[0, 0, 0] = 13 * 1000 + 998                             # a 255th segment
    raw[1, 0, 0] = 0 * 1000 + 5                                # a stuff id with an instance part: no error
    raw[2, 63, 127] = 19 * 1000                                # a class the map sends to -1
    more = z["b.raw"].copy()
    more[0, 5, 5] = 40 * 1000                                  # a class beyond the map
    more[2, 0, 0], more[2, 9, 9] = 19 * 1000 + 1, 33 * 1000    # both
    for r, st in ((raw, [_lib.PH_GTSEG_ETOOMANY, 0, _lib.PH_GTSEG_EUNMAPPED]),
                  (more, [_lib.PH_GTSEG_EOUTSIDE, 0, _lib.PH_GTSEG_EUNMAPPED | _lib.PH_GTSEG_EOUTSIDE])):
        want, want_st = np_gt_segments(r, fill=FILL, **m)
        assert want_st.tolist() == st
        tables, status = _segments(gpu, r, m, dtype)
        assert status.tolist() == st and np.array_equal(tables, want)
        assert (tables[0] == FILL).all() and (tables[2] == FILL).all() and tables[1, 0] in (13, 14)
    with pytest.raises(ValueError, match=r"frame 0: more than 254 segments"):
        GT.segment_tables(raw[:1].astype(dtype), device=gpu, **m)
    with pytest.raises(ValueError, match=r"frame 1: .*sends to -1.*outside the class map"):
        GT.segment_tables(more[1:].astype(dtype), device=gpu, **m)
    if dtype == np.int32:
        neg = z["a.raw"].copy()
        neg[1, 3, 3] = -1
        assert _segments(gpu, neg, m)[1].tolist() == [0, _lib.PH_GTSEG_EOUTSIDE, 0]


# ---- 3. argument errors launch nothing --------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(gpu):
    z, meta = fixture()
    m = mapping(z, meta)
    lib = _lib.load()
    raw = _dev(gpu, z["a.raw"])
    cm = np.ascontiguousarray(m["class_map"], np.int32)
    cmp_ = cm.ctypes.data_as(C.POINTER(C.c_int32))
    tables = torch.full((3, _lib.PH_GTSEG_TABLE_WORDS), FILL, dtype=torch.int32, device=gpu)
    status = torch.full((3,), FILL, dtype=torch.int32, device=gpu)
    ws = torch.empty(lib.ph_gt_segments_workspace_bytes(3, cm.size, 1000), dtype=torch.uint8, device=gpu)

    def seg(Hs=37, raw_divisor=1000, ws_bytes=ws.numel(), n_map=cm.size):
        return lib.ph_gt_segments(_lib.ptr(raw), _lib.PH_GTSEG_I32, 3, Hs, 53, cmp_, n_map, raw_divisor, 10000, 255, _lib.ptr(tables),
                                  _lib.ptr(status), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())

    for kw, rc in ((dict(Hs=0), _lib.PH_EINVAL), (dict(Hs=-37), _lib.PH_EINVAL), (dict(raw_divisor=8000), -2),
                   (dict(ws_bytes=ws.numel() - 256), _lib.PH_EWORKSPACE), (dict(n_map=0), _lib.PH_EINVAL)):
        assert seg(**kw) == rc, kw
        torch.cuda.synchronize()
        assert bool((tables == FILL).all()) and bool((status == FILL).all()), kw
    assert seg() == 0 and not bool((tables == FILL).any()) and not status.any()          # the same call without the fault

    a = _index_args(z, meta, "a", "crop")
    for what, kw in (("src_y", dict(src_y=np.where(a["src_y"] == a["src_y"].max(), 37, a["src_y"]))),
                     ("src_x", dict(src_x=np.where(a["src_x"] == a["src_x"].min(), -2, a["src_x"]))),
                     ("kept", dict(kept_ids=[np.arange(255)] * 3)), ("pad", dict(pad_hw=(a["src_y"].shape[1] - 1, 64)))):
        out = _filled_outs(gpu, 3, (a["src_y"].shape[1], a["src_x"].shape[1]), dict(a, **kw)["pad_hw"])
        with pytest.raises((ValueError, _lib.PolyheadError), match="ph_gt_index_maps|at most 254"):
            b = dict(a, **kw)
            GT.gt_index_maps(raw, _lib.PH_GTSEG_I32, _dev(gpu, z["a.raw_depth"]), cm, 1000, 10000, 255, b["kept_ids"], b["src_y"], b["src_x"],
                             b["pad_hw"], scale_mean=b["scale_mean"], out=out)
        torch.cuda.synchronize()
        assert bool((out[0] == 0xFF).all()) and bool(torch.isnan(out[1]).all()), what


# ---- 4. ph_gt_index_maps against the fixture: identity, crop with offset, flip, ratio 1.37, ratio 2 -------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("an", AUGS)
def test_index_maps_equal_the_reference(gpu, case, an):
    """0xFF / NaN filled outputs come back fully written, the depth pad included; a kept segment without a pixel keeps its index unused
    and a dropped thin segment reads 255 because the fixture says so (test_gt_segments_host pins that the fixture holds both)"""
    z, meta = fixture()
    m = mapping(z, meta)
    a = _index_args(z, meta, case, an)
    raw, raw_depth = z[f"{case}.raw"], z[f"{case}.raw_depth"]
    want_seg, want_depth = np_gt_index_maps(raw, raw_depth, **a, **m)
    Wc = a["src_x"].shape[1]
    for dtype, offset in ((np.int32, 0), (np.uint16, 0), (np.int32, 1)):                  # offset 1: byte stores whatever Wc is
        seg, depth = _index_maps(gpu, raw, raw_depth, m, a, dtype, offset)
        assert not torch.isnan(depth).any()
        assert np.array_equal(seg.cpu().numpy(), want_seg) and np.array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
    for f in range(len(raw)):
        pre = f"{case}.{an}.{f}."
        assert np.array_equal(want_seg[f], z[pre + "index_map"]) and np.array_equal(want_depth[f].view(np.uint32), z[pre + "depth"].view(np.uint32))
    assert (case, an, Wc % 16 == 0) in {("a", "ident", False), ("a", "crop", True), ("a", "flip", True), ("a", "r137", True), ("a", "r2", False),
                                        ("b", "ident", True), ("b", "crop", True), ("b", "flip", True), ("b", "r137", True), ("b", "r2", True)}


def test_depth_bits_and_frames_smaller_than_the_call(gpu):
    """79.99, 80.0 and 255.996 of the raw depth under scale_mean 1, 1.37 and 2; rows and columns of -1 read as no segment, depth 0;
    without a depth map the call writes the index maps alone"""
    z, meta = fixture()
    m = mapping(z, meta)
    a = _index_args(z, meta, "a", "ident")
    a["scale_mean"] = np.array([1.0, 1.37, 2.0], np.float32)
    a["src_y"], a["src_x"] = a["src_y"].copy(), a["src_x"].copy()
    a["src_y"][1, 30:], a["src_x"][1, 41:], a["src_x"][2, :3] = -1, -1, -1
    raw, raw_depth = z["a.raw"], z["a.raw_depth"].copy()
    raw_depth[1:, 0, 3:9] = [20477, 20479, 20480, 20481, 65535, 0]
    want_seg, want_depth = np_gt_index_maps(raw, raw_depth, **a, **m)
    seg, depth = _index_maps(gpu, raw, raw_depth, m, a)
    assert np.array_equal(seg.cpu().numpy(), want_seg) and np.array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
    f32 = np.float32
    assert want_depth[1, 0, 3:9].tolist() == [f32(20477 / 256) / f32(1.37), f32(20479 / 256) / f32(1.37), f32(80) / f32(1.37)] + \
        [f32(80) / f32(1.37)] * 2 + [0.0]
    assert (want_seg[1, 30:] == 255).all() and (want_seg[1, :, 41:] == 255).all() and not want_depth[1, 30:].any() and not want_depth[2, :, :3].any()
    seg2, none = _index_maps(gpu, raw, None, m, a)
    assert none is None and torch.equal(seg2, seg)


# ---- 5. same bits twice and from a graph; a frame does not depend on its neighbours ---------------------------------------------------------
def test_two_calls_a_graph_replay_and_single_frames(gpu):
    z, meta = fixture()
    m = mapping(z, meta)
    raw, raw_depth = z["b.raw"], z["b.raw_depth"]
    a = _index_args(z, meta, "b", "r137")
    t1, t2 = _segments(gpu, raw, m), _segments(gpu, raw, m)
    assert np.array_equal(t1[0], t2[0]) and np.array_equal(t1[1], t2[1])
    s1, s2 = _index_maps(gpu, raw, raw_depth, m, a), _index_maps(gpu, raw, raw_depth, m, a)
    assert torch.equal(s1[0], s2[0]) and torch.equal(_bits(s1[1]), _bits(s2[1]))
    for order in ([1], [2, 1, 0]):
        sub_t = _segments(gpu, raw[order], m)
        sub_s = _index_maps(gpu, raw, raw_depth, m, a, frames=order)
        for j, f in enumerate(order):
            assert np.array_equal(sub_t[0][j], t1[0][f]) and sub_t[1][j] == t1[1][f]
            assert torch.equal(sub_s[0][j], s1[0][f]) and torch.equal(_bits(sub_s[1][j]), _bits(s1[1][f]))

    # one capture of both calls on buffers uploaded beforehand (the Python wrapper of the second uploads its tables: not capturable)
    lib = _lib.load()
    cm = np.ascontiguousarray(m["class_map"], np.int32)
    cmp_ = cm.ctypes.data_as(C.POINTER(C.c_int32))
    r, d = _dev(gpu, raw), _dev(gpu, raw_depth)
    F_, (Hs, Ws), (Hc, Wc), (Hp, Wp) = 3, raw.shape[1:], (a["src_y"].shape[1], a["src_x"].shape[1]), a["pad_hw"]
    kept = np.zeros((F_, 256), np.int32)
    for f, k in enumerate(a["kept_ids"]):
        kept[f, :len(k)] = k
    kept_n = np.array([len(k) for k in a["kept_ids"]], np.int32)
    sy, sx = np.ascontiguousarray(a["src_y"], np.int32), np.ascontiguousarray(a["src_x"], np.int32)
    kept_d, sy_d, sx_d = _dev(gpu, kept), _dev(gpu, sy), _dev(gpu, sx)
    tables = torch.full((F_, _lib.PH_GTSEG_TABLE_WORDS), FILL, dtype=torch.int32, device=gpu)
    status = torch.full((F_,), FILL, dtype=torch.int32, device=gpu)
    ws = torch.empty(lib.ph_gt_segments_workspace_bytes(F_, cm.size, 1000), dtype=torch.uint8, device=gpu)
    seg, depth = _filled_outs(gpu, F_, (Hc, Wc), (Hp, Wp))
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):                                      # one stream, one branch
        st = _lib.stream_ptr()
        _lib.check(lib.ph_gt_segments(_lib.ptr(r), _lib.PH_GTSEG_I32, F_, Hs, Ws, cmp_, cm.size, 1000, 10000, 255, _lib.ptr(tables), _lib.ptr(status),
                                      _lib.ptr(ws), ws.numel(), st), "ph_gt_segments")
        _lib.check(lib.ph_gt_index_maps(_lib.ptr(r), _lib.PH_GTSEG_I32, _lib.ptr(d), F_, Hs, Ws, cmp_, cm.size, 1000, 10000, 255, _lib.ptr(kept_d),
                                        kept_n.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(sy.ctypes.data), C.c_void_p(sx.ctypes.data),
                                        _lib.ptr(sy_d), _lib.ptr(sx_d), Hc, Wc, Hp, Wp, 256.0, 80.0,
                                        a["scale_mean"].ctypes.data_as(C.POINTER(C.c_float)), _lib.ptr(seg), _lib.ptr(depth), st), "ph_gt_index_maps")
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(tables.cpu().numpy(), t1[0]) and not status.any()
    assert torch.equal(seg, s1[0]) and torch.equal(_bits(depth), _bits(s1[1]))


# ---- 6. end to end: the PreparedGT of the device path equals the bitmask path's, and so does a training step on it --------------------------
def test_prepared_from_panoptic_equals_the_bitmask_path(gpu, video_parts):  # noqa: F811
    z, meta = fixture()
    m = mapping(z, meta)
    nt = meta["num_thing_classes"]
    raw = np.stack([z["b.raw"][1], np.roll(z["b.raw"][1], 37, axis=1)])                  # 13 segments each, 64 x 128
    raw_depth = z["b.raw_depth"][:2]
    pad_hw = (64, 96)
    aug = [((64, 128), False, (2, 10), (60, 90)), ((88, 175), True, (20, 31), (60, 90))]  # crop; ratio 1.37, flip, crop
    host = [np_bitmask_loader(raw[f], raw_depth[f], aug[f], pad_hw, **m) for f in range(2)]
    assert all(h["ids"].size > 0 for h in host) and all((h["labels"] < nt).any() and (h["labels"] >= nt).any() for h in host)
    want = GT.prepare_gt([GT.index_map_from_bitmasks(h["bitmasks"]) for h in host], [h["labels"] for h in host], pad_hw, nt, mask_assign_stride=4,
                         gt_depth=np.stack([h["depth"] for h in host]), gt_instance_ids=[h["ids"] for h in host], want_hard=True, device=gpu)
    kw = dict(mask_assign_stride=4, want_hard=True, device=gpu, **m)
    got = GT.prepare_gt_from_panoptic(raw, raw_depth, aug, nt, pad_hw, **kw)
    cached = GT.prepare_gt_from_panoptic(_dev(gpu, raw), _dev(gpu, raw_depth), aug, nt, pad_hw, tables=GT.segment_tables(raw, device=gpu, **m), **kw)
    for p in (got, cached):
        for k in ("things", "stuff", "things_hard", "valid", "depth"):
            assert torch.equal(_bits(getattr(p, k)), _bits(getattr(want, k))), k
        assert (p.G, p.S) == (want.G, want.S) and want.G[0] > 0 and want.S[0] > 0
        for k in ("labels_h", "sem_cls_h", "ids_h"):
            assert all(np.array_equal(x, y) for x, y in zip(getattr(p, k), getattr(want, k))), k
        for k in ("gt_labels", "gt_sem_cls", "gt_instance_ids"):
            assert all(torch.equal(x, y) for x, y in zip(getattr(p, k), getattr(want, k))), k

    neck, rpn, roi = video_parts[:3]
    B, H0, W0 = 2, 16, 24                                              # 64 x 96 padded; the assign resolution is 16 x 24
    x = [f.to(gpu) for f in Hh.fpn_inputs(seed=41, B=B, C=256, H0=H0, W0=W0)]
    with torch.enable_grad():
        feats = [f.detach() for f in TR.neck_forward_train(neck, x)]
    metas = [Hh.img_meta(60, 90, pad_to=pad_hw)] * B
    totals = []
    with TR.TrainStep(rpn, roi, device_assign=False) as step:
        for p in (want, got):
            for mod in (rpn, roi):
                for q in mod.parameters():
                    q.grad = None
            losses, total, _ = step.forward_backward_prepared(feats, metas, p)
            assert np.isfinite(float(total))
            totals.append(total.detach().clone())
    for mod in (rpn, roi):
        for q in mod.parameters():
            q.grad = None
    assert torch.equal(totals[0], totals[1])
