"""GPU: `ph_image_prepare` (csrc/ph_imgprep.hip) and what stands on it -- `image.prepare_images`, `image.prepare_step_inputs`,
`image.prepare_test_images` -- against the numpy restatements of tests/test_image_prepare_host.py: the reference's whole-image pipeline
(`np_pipeline`) and the call's contract (`np_image_prepare`).

Bounds: none, everything is exact.  The resize is integer arithmetic and the normalisation one fp32 subtract and one fp32 multiply, so
outputs are compared by their bits (as int32 / int16 views); the bf16 outputs against `torch.from_numpy(ref).to(torch.bfloat16)`.  The
files are 2 x 2, 5 x 8 and 37 x 53; one output of 70 x 300 spans several workgroups and several 16-byte runs of a lane.  Every case runs
with padded widths that are and are not multiples of the 16-byte store (4 fp32, 8 bf16 columns) and with the output pointer one element
off, which takes the element-store path whatever the width.  For a ratio other than 1 the tests pin the restatement of OpenCV's rule in
`image.linear_taps`, not OpenCV (see the host file)."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
from polyphonicformer_amd import _lib, gt as GT, image as IM
from test_gt_segments_host import fixture, mapping
from test_image_prepare_host import AUGS, CASES, FILES, MEAN, STD, aug_of, bits, image_of, np_image_prepare, np_pipeline, tables_of

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0                       # what an output holds before a call that must launch nothing
DTYPES = (torch.float32, torch.bfloat16)


def _filled(gpu, shape, dtype, channels_last, offset=0):
    """an output [F, 3, Hp, Wp] filled with NaN, starting `offset` elements into a 16-byte aligned allocation"""
    F_, _, Hp, Wp = shape
    n = F_ * 3 * Hp * Wp
    flat = torch.full((n + 16,), float("nan"), dtype=dtype, device=gpu)[offset:offset + n]
    assert flat.data_ptr() % 16 == offset * flat.element_size()
    return flat.view(F_, Hp, Wp, 3).permute(0, 3, 1, 2) if channels_last else flat.view(shape)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(out, ref):
    """out: a device tensor; ref: fp32 numpy of the same logical shape.  Bit equality in out's dtype."""
    want = torch.from_numpy(ref).to(out.dtype)
    return torch.equal(_bits(out.cpu()), _bits(want))


def _run(gpu, raw, ty, tx, pad, dtype=torch.float32, channels_last=False, to_rgb=False, offset=0):
    mean, stdinv = IM.norm_constants(MEAN, STD)
    out = _filled(gpu, (raw.shape[0], 3) + tuple(pad), dtype, channels_last, offset)
    got = IM.image_prepare(torch.from_numpy(raw).to(gpu), ty, tx, pad, mean, stdinv, to_rgb=to_rgb, dtype=dtype, channels_last=channels_last, out=out)
    assert got is out
    return out


def _pads(Hc, Wc, pad):
    """the case's own pad, the bare frame, a width that is a multiple of 8 (16-byte stores in both dtypes), one that is a multiple of 4
    and not of 8 (16-byte stores in fp32, element stores in bf16) and one that is odd"""
    up8 = -(-Wc // 8) * 8
    return (pad, (Hc, Wc), (Hc, up8), (Hc + 1, up8 + 4), (Hc + 2, up8 + 7))


# ---- 1. bits: every case and augmentation, both dtypes, both layouts, to_rgb, ragged widths, the pointer one element off ---------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("an", tuple(AUGS))
def test_bits_equal_the_reference_pipeline(gpu, case, an):
    raw = image_of(case, frames=2)
    ty, tx, aug, pad0 = tables_of(case, an, frames=2)
    Hc, Wc = ty.shape[1], tx.shape[1]
    mean, stdinv = IM.norm_constants(MEAN, STD)
    widths = set()
    for pad in _pads(Hc, Wc, pad0):
        widths.add((pad[1] % 4 == 0, pad[1] % 8 == 0))
        for to_rgb in (False, True):
            ref = np.stack([np_pipeline(raw[f], aug, pad, to_rgb=to_rgb) for f in range(2)])
            assert np.array_equal(ref.view(np.int32), np_image_prepare(raw, ty, tx, pad, mean, stdinv, to_rgb).view(np.int32))
            for dtype in DTYPES:
                for cl in (False, True):
                    for offset in (0, 1):
                        out = _run(gpu, raw, ty, tx, pad, dtype, cl, to_rgb, offset)
                        assert out.shape == (2, 3) + tuple(pad)
                        assert out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
                        assert _same(out, ref), (pad, to_rgb, dtype, cl, offset)
    assert widths >= {(True, True), (True, False), (False, False)}       # multiples of 8, of 4 alone, of neither


def test_an_output_of_several_workgroups(gpu):
    """37 x 53 -> 75 x 311, flipped, cropped to 70 x 300 at (3, 7): 72 x 304 padded is 18 workgroups a frame with 38 live lanes a row, every
    lane with two (fp32) 16-byte stores per plane; 71 x 301 takes the element stores; 70 x 1100 has three row pieces a row"""
    raw = image_of("m", seed=3, frames=2)
    aug = ((75, 311), True, (3, 7), (70, 300))
    ty, tx, _, chw = IM.bilinear_tables(FILES["m"], *aug)
    assert chw == (70, 300)
    ty, tx = np.stack([ty] * 2), np.stack([tx] * 2)
    for pad in ((72, 304), (71, 301), (70, 1100)):
        ref = np.stack([np_pipeline(raw[f], aug, pad) for f in range(2)])
        for dtype in DTYPES:
            for cl in (False, True):
                assert _same(_run(gpu, raw, ty, tx, pad, dtype, cl), ref), (pad, dtype, cl)


def test_tables_of_the_callers_own(gpu):
    """taps no resize rule gives -- far apart, in any order, both weighted (the gather's byte loads), beside neighbouring ones (its
    8-byte loads), entries of -1, and the last pixel of the call's images, where an 8-byte load would pass their end -- against the contract"""
    rng = np.random.default_rng(17)
    raw = image_of("m", seed=17, frames=2)
    (Hs, Ws), (Hc, Wc) = FILES["m"], (19, 45)

    def table(n, limit):
        i0, i1, w1 = rng.integers(0, limit, (2, n)), rng.integers(0, limit, (2, n)), rng.integers(0, 2049, (2, n))
        near = rng.random((2, n)) < 0.5
        i1 = np.where(near, np.minimum(i0 + 1, limit - 1), i1)
        return np.stack([IM.pack_taps(i0[f], i1[f], 2048 - w1[f], w1[f]) for f in range(2)])

    ty, tx = table(Hc, Hs), table(Wc, Ws)
    ty[1, 3, 0], tx[0, 5, 0] = -1, -1
    ty[1, -1], tx[1, -1] = IM.pack_taps([Hs - 1], [Hs - 2], [1024], [1024])[0], IM.pack_taps([Ws - 1], [Ws - 1], [2048], [0])[0]
    mean, stdinv = IM.norm_constants(MEAN, STD)
    for pad in ((Hc, Wc), (Hc + 1, 48)):
        for to_rgb in (False, True):
            ref = np_image_prepare(raw, ty, tx, pad, mean, stdinv, to_rgb)
            assert ref[1, :, Hc - 1, Wc - 1].tolist() != [0.0] * 3 and not ref[1, :, 3].any() and not ref[0, :, :, 5].any()
            for dtype in DTYPES:
                for cl in (False, True):
                    assert _same(_run(gpu, raw, ty, tx, pad, dtype, cl, to_rgb), ref), (pad, to_rgb, dtype, cl)


# ---- 2. the pad: exactly +0.0, and no word of the output keeps what it held --------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cl", (False, True))
def test_pad_is_plus_zero_and_every_word_is_written(gpu, dtype, cl):
    raw = image_of("m")
    ty, tx, aug, pad = tables_of("m", "small")
    Hc, Wc = ty.shape[1], tx.shape[1]
    for p in (pad, (pad[0], pad[1] + 1)):
        out = _run(gpu, raw, ty, tx, p, dtype, cl)
        assert not torch.isnan(out).any()
        for piece in (out[:, :, Hc:], out[:, :, :, Wc:]):
            assert piece.numel() and not _bits(piece).any()                      # +0.0: all bits clear
        assert bool((out[:, :, :Hc, :Wc] != 0).any())


# ---- 3. frames in one call -----------------------------------------------------------------------------------------------------------------
def test_frames_of_different_sizes_and_single_frames(gpu):
    """four frames of one file size under four augmentations: rows and columns of -1 beyond the smaller ones; a frame's bits are those
    it gets alone in a call"""
    raw = image_of("m", seed=5, frames=4)
    augs = [aug_of("m", an)[0] for an in ("crop0", "down", "ident", "small")]
    tabs = [IM.bilinear_tables(FILES["m"], *a) for a in augs]
    Hc, Wc = max(t[3][0] for t in tabs), max(t[3][1] for t in tabs)
    pad = (Hc + 3, -(-Wc // 8) * 8)
    ty, tx = IM._stack_tables([t[0] for t in tabs], Hc), IM._stack_tables([t[1] for t in tabs], Wc)
    assert (ty[:, :, 0] == -1).any() and (tx[:, :, 0] == -1).any() and len({t[3] for t in tabs}) == 4
    ref = np.stack([np_pipeline(raw[f], augs[f], pad) for f in range(4)])
    for dtype in DTYPES:
        for cl in (False, True):
            out = _run(gpu, raw, ty, tx, pad, dtype, cl)
            assert _same(out, ref)
            for f in (3, 1):
                alone = _run(gpu, raw[f:f + 1], ty[f:f + 1], tx[f:f + 1], pad, dtype, cl)
                assert torch.equal(_bits(alone[0]), _bits(out[f]))
            via = IM.prepare_images(raw, augs, pad, MEAN, STD, dtype=dtype, channels_last=cl, device=gpu)
            assert via.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format) and torch.equal(_bits(via), _bits(out))


def test_66_frames_are_chunked(gpu):
    """more frames than one call takes: `prepare_images` chunks them, and every frame equals its own call"""
    n = 66
    assert n > _lib.PH_IMGPREP_MAX_FRAMES
    raw = image_of("s", seed=9, frames=n)
    names = tuple(AUGS)
    augs = [aug_of("s", names[f % len(names)])[0] for f in range(n)]
    pad = (16, 24)
    out = IM.prepare_images(raw, augs, pad, MEAN, STD, to_rgb=True, device=gpu)
    assert out.shape == (n, 3, 16, 24)
    ref = np.stack([np_pipeline(raw[f], augs[f], pad, to_rgb=True) for f in range(n)])
    assert _same(out, ref)
    for f in (0, 63, 64, 65):
        alone = IM.prepare_images(raw[f:f + 1], augs[f:f + 1], pad, MEAN, STD, to_rgb=True, device=gpu)
        assert torch.equal(_bits(alone[0]), _bits(out[f]))


# ---- 4. the same bits twice and from a graph -------------------------------------------------------------------------------------------------
def test_two_calls_and_a_graph_replay(gpu):
    raw = image_of("m", seed=11, frames=2)
    ty, tx, aug, pad = tables_of("m", "r137", frames=2)
    a, b = _run(gpu, raw, ty, tx, pad), _run(gpu, raw, ty, tx, pad)
    assert torch.equal(_bits(a), _bits(b))

    lib = _lib.load()
    mean, stdinv = IM.norm_constants(MEAN, STD)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    ty, tx = np.ascontiguousarray(ty), np.ascontiguousarray(tx)
    r, ty_d, tx_d = torch.from_numpy(raw).to(gpu), torch.from_numpy(ty).to(gpu), torch.from_numpy(tx).to(gpu)
    out = _filled(gpu, (2, 3) + tuple(pad), torch.float32, False)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):                                      # one stream, one launch
        _lib.check(lib.ph_image_prepare(_lib.ptr(r), 2, raw.shape[1], raw.shape[2], C.c_void_p(ty.ctypes.data), C.c_void_p(tx.ctypes.data),
                                        _lib.ptr(ty_d), _lib.ptr(tx_d), ty.shape[1], tx.shape[1], pad[0], pad[1], fp(mean), fp(stdinv), 0,
                                        _lib.PH_OUT_F32, _lib.PH_IMG_NCHW, _lib.ptr(out), _lib.stream_ptr()), "ph_image_prepare")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(a))
    other = image_of("m", seed=12, frames=2)
    r.copy_(torch.from_numpy(other))                                   # the file's bytes change, the capture stays
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(_run(gpu, other, ty, tx, pad))) and not torch.equal(_bits(out), _bits(a))


# ---- 5. argument errors launch nothing -------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(gpu):
    lib = _lib.load()
    raw = image_of("m", frames=2)
    ty, tx, aug, pad = tables_of("m", "ident", frames=2)
    ty, tx = np.ascontiguousarray(ty), np.ascontiguousarray(tx)
    Hs, Ws = FILES["m"]
    mean, stdinv = IM.norm_constants(MEAN, STD)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    r, ty_d, tx_d = torch.from_numpy(raw).to(gpu), torch.from_numpy(ty).to(gpu), torch.from_numpy(tx).to(gpu)
    out = torch.full((2, 3) + tuple(pad), SENTINEL, dtype=torch.float32, device=gpu)

    def call(frames=2, Hs=Hs, Ws=Ws, hy=ty, hx=tx, Hp=pad[0], Wp=pad[1], dtype=_lib.PH_OUT_F32, layout=_lib.PH_IMG_NCHW, rawp=_lib.ptr(r),
             outp=_lib.ptr(out)):
        hy, hx = np.ascontiguousarray(hy), np.ascontiguousarray(hx)
        return lib.ph_image_prepare(rawp, frames, Hs, Ws, C.c_void_p(hy.ctypes.data), C.c_void_p(hx.ctypes.data), _lib.ptr(ty_d), _lib.ptr(tx_d),
                                    ty.shape[1], tx.shape[1], Hp, Wp, fp(mean), fp(stdinv), 0, dtype, layout, outp, _lib.stream_ptr())

    bad_y, bad_x = ty.copy(), tx.copy()
    bad_y[1, 5, 0] = (Hs - 1) | (Hs << 16)                               # a second tap at Hs
    bad_x[0, 7, 0] = Ws | (Ws << 16)                                     # both taps at Ws
    for kw, rc, word in ((dict(hy=bad_y), _lib.PH_EINVAL, "tab_y[1][5]"), (dict(hx=bad_x), _lib.PH_EINVAL, "tab_x[0][7]"),
                         (dict(Hp=ty.shape[1] - 1), _lib.PH_EINVAL, "Hc <= Hp"), (dict(frames=0), _lib.PH_EINVAL, "frames"),
                         (dict(frames=_lib.PH_IMGPREP_MAX_FRAMES + 1), _lib.PH_EINVAL, "frames"), (dict(dtype=_lib.PH_OUT_F16), _lib.PH_EINVAL, "out_dtype"),
                         (dict(dtype=7), _lib.PH_EINVAL, "out_dtype"), (dict(layout=2), _lib.PH_EINVAL, "layout"),
                         (dict(rawp=None), _lib.PH_EINVAL, "null"), (dict(outp=None), _lib.PH_EINVAL, "null"),
                         (dict(Hs=32768), _lib.PH_EUNSUPPORTED, "32767")):
        assert call(**kw) == rc, kw
        err = Hh.last_error()
        assert err.startswith("ph_image_prepare") and word in err, (kw, err)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), kw
    assert call() == 0                                                   # the same call without the fault
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())
    with pytest.raises(ValueError, match="above pad_hw"):
        IM.prepare_images(raw, [aug] * 2, (pad[0], FILES["m"][1] - 1), MEAN, STD, device=gpu)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        IM.prepare_images(raw, [aug] * 2, pad, MEAN, STD, dtype=torch.float16, device=gpu)


# ---- 6. the step's image and ground truth from one set of augmentation parameters -------------------------------------------------------------
def test_step_inputs_agree_pixel_for_pixel(gpu):
    """a frame of the ground-truth fixture painted one colour per segment, ratio 1 with flip and crop: wherever the index map names a
    segment, the image holds that segment's normalised colour"""
    z, meta = fixture()
    m = mapping(z, meta)
    nt = meta["num_thing_classes"]
    raw_maps = np.stack([z["b.raw"][1], np.roll(z["b.raw"][1], 37, axis=1)])             # 13 segments each, 64 x 128
    raw_depth = z["b.raw_depth"][:2]
    ids = np.unique(raw_maps)
    colour = np.random.default_rng(3).permutation(256 ** 2)[:ids.size]                   # distinct colours
    lut = np.stack([colour & 255, colour >> 8, (np.arange(ids.size) * 37 + 11) & 255], 1).astype(np.uint8)
    images = lut[np.searchsorted(ids, raw_maps)]                                         # [2][64][128][3]
    aug = [((64, 128), True, (2, 10), (60, 90)), ((64, 128), True, (0, 38), (60, 90))]
    pad_hw = (64, 96)
    kw = dict(mask_assign_stride=4, want_hard=True, **m)
    img, prepared = IM.prepare_step_inputs(images, raw_maps, raw_depth, aug, nt, pad_hw, mean=MEAN, std=STD, device=gpu, **kw)
    alone = IM.prepare_images(images, aug, pad_hw, MEAN, STD, device=gpu)
    want = GT.prepare_gt_from_panoptic(raw_maps, raw_depth, aug, nt, pad_hw, device=gpu, **kw)
    assert img.shape == (2, 3, 64, 96) and torch.equal(_bits(img), _bits(alone))
    for k in ("things", "stuff", "things_hard", "valid", "depth"):
        assert torch.equal(_bits(getattr(prepared, k)), _bits(getattr(want, k))), k
    assert (prepared.G, prepared.S) == (want.G, want.S) and all(torch.equal(x, y) for x, y in zip(prepared.gt_instance_ids, want.gt_instance_ids))

    # the index maps of the same augmentation, as prepare_gt_from_panoptic makes them
    tables = GT.segment_tables(raw_maps, device=gpu, **m)
    raw_d, dtype = GT._raw_maps(raw_maps, gpu, "test")
    kept, sys_, sxs = [], [], []
    for tab, a in zip(tables, aug):
        sy, sx, scale, _ = GT.nearest_tables((64, 128), *a)
        kept.append(tab.ids[GT.transform_boxes(tab.boxes, scale, *a)[1]])
        sys_.append(sy); sxs.append(sx)
    seg, _ = GT.gt_index_maps(raw_d, dtype, None, m["class_map"], m["raw_divisor"], m["divisor"], m["no_obj_class"], kept, np.stack(sys_),
                              np.stack(sxs), pad_hw)
    seg, got = seg.cpu().numpy(), img.cpu().numpy()
    mean, stdinv = IM.norm_constants(MEAN, STD)
    # to_coco on one raw id: class_map[raw // raw_divisor] * divisor + raw % raw_divisor
    row_of = {int(m["class_map"][int(r) // m["raw_divisor"]]) * m["divisor"] + int(r) % m["raw_divisor"]: j for j, r in enumerate(ids)}
    named = 0
    for f in range(2):
        assert seg[f].shape == (60, 90)
        for i, mapped in enumerate(kept[f]):
            want_px = (lut[row_of[int(mapped)]].astype(np.float32) - mean) * stdinv
            where = seg[f] == i
            named += int(where.sum())
            assert np.array_equal(bits(got[f][:, :60, :90][:, where]), bits(np.broadcast_to(want_px[:, None], (3, int(where.sum())))))
    assert named > 2 * 60 * 90 // 2


# ---- 7. the test pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", ((64, 128), (37, 53)))
def test_test_images_equal_normalize_pad_transpose(gpu, hw):
    frames = np.random.default_rng(21).integers(0, 256, (3,) + hw + (3,), dtype=np.uint8)
    mean, stdinv = IM.norm_constants(MEAN, STD)
    Hp, Wp = -(-hw[0] // 32) * 32, -(-hw[1] // 32) * 32
    for to_rgb in (False, True):
        x = torch.from_numpy(frames).to(gpu)
        if to_rgb:
            x = x.flip(-1)
        want = torch.nn.functional.pad(((x.float() - torch.from_numpy(mean).to(gpu)) * torch.from_numpy(stdinv).to(gpu)).permute(0, 3, 1, 2),
                                       (0, Wp - hw[1], 0, Hp - hw[0]))
        for src in (frames, torch.from_numpy(frames).to(gpu), [f for f in frames]):
            img, metas = IM.prepare_test_images(src, MEAN, STD, to_rgb=to_rgb, device=gpu)
            assert img.shape == (3, 3, Hp, Wp) and torch.equal(_bits(img), _bits(want))
        assert all(m["img_shape"] == hw + (3,) and m["pad_shape"] == (Hp, Wp, 3) and m["batch_input_shape"] == (Hp, Wp) for m in metas)
        assert len(metas) == 3 and metas[0]["img_norm_cfg"]["to_rgb"] is to_rgb
        bf, _ = IM.prepare_test_images(frames, MEAN, STD, to_rgb=to_rgb, dtype=torch.bfloat16, channels_last=True, device=gpu)
        assert bf.is_contiguous(memory_format=torch.channels_last) and torch.equal(_bits(bf), _bits(want.to(torch.bfloat16)))
    # frames of two sizes in one batch: padded to the largest, each with its own shapes
    two = [frames[0], frames[1][:hw[0] - 3, :hw[1] - 5]]
    img, metas = IM.prepare_test_images(two, MEAN, STD, device=gpu)
    assert [m["img_shape"] for m in metas] == [hw + (3,), (hw[0] - 3, hw[1] - 5, 3)]
    one, _ = IM.prepare_test_images(two[1][None], MEAN, STD, device=gpu)
    assert not _bits(img[1, :, hw[0] - 3:]).any() and not _bits(img[1, :, :, hw[1] - 5:]).any()
    assert torch.equal(_bits(img[1, :, :hw[0] - 3, :hw[1] - 5]), _bits(one[0, :, :hw[0] - 3, :hw[1] - 5]))
