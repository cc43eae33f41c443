"""CPU: the host side of the images on the device (polyphonicformer_amd/image.py: `linear_taps`, `bilinear_tables`, the test metas) and two
numpy restatements that tests/test_gpu_image_prepare.py compares `ph_image_prepare` with:

  np_pipeline        the reference's train_pipeline on ONE image, whole-image steps in its order (configs/_base_/datasets/
                     cityscapes_dvps.py:11-20): the uint8 bilinear resize by OpenCV's fixed-point formula, mmcv.imflip, the crop slice of
                     datasets/pipelines/transforms.py:227, mmcv.imnormalize in fp32, the zero pad, the transpose.  Its taps come from
                     `cv_taps`, a scalar restatement of OpenCV's rule written out index by index, not from `image.linear_taps`.
  np_image_prepare   the contract of `ph_image_prepare` (include/polyhead.h): the composed tables applied per output pixel

Everything is exact: the resize is integer arithmetic, the normalisation one fp32 subtract and one fp32 multiply; values are compared by
their bits.  What is NOT pinned is OpenCV itself: cv2 is not available here, so the resize rule is the restatement in `image.linear_taps`
(see its docstring), held to float64 bilinear interpolation at the same taps within one grey level."""
import math

import numpy as np
import pytest

from polyphonicformer_amd import gt as GT, image as IM

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]          # img_norm_cfg, cityscapes_dvps.py:4-6

# file sizes (h, w); "m" has the odd width the flips run on
FILES = {"t": (2, 2), "s": (5, 8), "m": (37, 53)}
# name -> (ratio, flip, crop as fractions of the resized image (offset y, x, size h, w) or None, frame smaller than pad_hw)
AUGS = {
    "ident": (1.0, False, None, False),
    "r137": (1.37, False, None, False),
    "r2flip": (2.0, True, None, False),
    "down": (0.6, True, None, False),
    "crop0": (1.37, True, (0.0, 0.0, 0.6, 0.7), False),                  # crop at offset 0
    "cropend": (2.0, False, (0.45, 0.35, 0.55, 0.65), False),            # crop reaching the resized image's last row and column
    "small": (1.0, True, (0.3, 0.2, 0.5, 0.5), True),                    # pad_hw well above the augmented frame
}
CASES = tuple(FILES)


def aug_of(case, an):
    """-> ((resized_hw, flip, crop_offset, crop_hw) as `image.bilinear_tables` takes them, (Hc, Wc), pad_hw)"""
    (H, W), (ratio, flip, crop, small) = FILES[case], AUGS[an]
    nh, nw = max(1, int(H * ratio + 0.5)), max(1, int(W * ratio + 0.5))
    off = chw = None
    Hc, Wc = nh, nw
    if crop is not None:
        Hc, Wc = max(1, int(math.ceil(nh * crop[2]))), max(1, int(math.ceil(nw * crop[3])))
        off = (nh - Hc, nw - Wc) if an == "cropend" else (min(int(nh * crop[0]), nh - Hc), min(int(nw * crop[1]), nw - Wc))
        chw = (Hc, Wc)
    pad = (Hc + 9, Wc + 11) if small else (-(-Hc // 32) * 32, -(-Wc // 32) * 32)                   # SeqPadWithDepth(size_divisor=32)
    return ((nh, nw), flip, off, chw), (Hc, Wc), pad


def image_of(case, seed=0, frames=1):
    H, W = FILES[case]
    return np.random.default_rng(1000 + seed).integers(0, 256, (frames, H, W, 3), dtype=np.uint8)


# ---- OpenCV's rule, index by index (resize.cpp, the INTER_LINEAR branch of the table set-up and the 8-bit fixed-point kernels) ---------------
def cv_taps(old, new, axis):
    """-> per destination index (i0, i1, w0, w1, fraction): python scalars, the statements of the rule one after another"""
    scale = 1.0 / (float(new) / old)
    out = []
    for d in range(new):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if axis == "x":
            if s < 0:
                s, f = 0, np.float32(0)
            if s >= old - 1:
                s, f = old - 1, np.float32(0)
            i0, i1 = s, min(s + 1, old - 1)
        else:
            i0, i1 = min(max(s, 0), old - 1), min(max(s + 1, 0), old - 1)
        w0 = int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048)))
        w1 = int(np.rint(f * np.float32(2048)))
        out.append((i0, i1, w0, w1, float(f)))
    return out


def np_resize(img, new_hw):
    """uint8 [H][W][3] -> uint8 [nh][nw][3]: the WHOLE image through the horizontal pass (int32 rows, 11 coefficient bits) and the
    vertical pass ((b (H >> 4)) >> 16 per row, + 2, >> 2)"""
    (H, W), (nh, nw) = img.shape[:2], new_hw
    ty, tx = cv_taps(H, nh, "y"), cv_taps(W, nw, "x")
    S = img.astype(np.int32)
    rows = np.stack([S[:, x0] * a0 + S[:, x1] * a1 for x0, x1, a0, a1, _ in tx], axis=1)          # [H][nw][3]
    out = np.stack([(((b0 * (rows[y0] >> 4)) >> 16) + ((b1 * (rows[y1] >> 4)) >> 16) + 2) >> 2 for y0, y1, b0, b1, _ in ty])
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def np_pipeline(img, aug, pad_hw, mean=MEAN, std=STD, to_rgb=False):
    """one uint8 [H][W][3] image the reference's way -> fp32 [3][Hp][Wp]"""
    resized, flip, off, chw = aug
    x = np_resize(img, resized)                                         # SeqResizeWithDepth: mmcv.imrescale, bilinear, on uint8
    if flip:
        x = x[:, ::-1]                                                  # SeqFlipWithDepth: mmcv.imflip, horizontal
    if off is not None:
        x = x[off[0]:off[0] + chw[0], off[1]:off[1] + chw[1]]           # SeqRandomCropWithDepth, transforms.py:227
    x = x.astype(np.float32)                                            # SeqNormalizeWithDepth: mmcv.imnormalize
    if to_rgb:
        x = x[..., ::-1]
    x = (x - np.asarray(mean, np.float64).astype(np.float32)) * (1 / np.asarray(std, np.float64)).astype(np.float32)
    assert x.dtype == np.float32
    out = np.zeros(tuple(pad_hw) + (3,), np.float32)                    # SeqPadWithDepth: mmcv.impad, pad_val 0, after Normalize
    out[:x.shape[0], :x.shape[1]] = x
    return np.ascontiguousarray(out.transpose(2, 0, 1))                 # SeqDefaultFormatBundle


# ---- the contract of ph_image_prepare in numpy ---------------------------------------------------------------------------------------
def np_image_prepare(raw, tab_y, tab_x, pad_hw, mean, stdinv, to_rgb=False):
    """raw uint8 [F][Hs][Ws][3], tab_y int32 [F][Hc][2], tab_x int32 [F][Wc][2] -> fp32 [F][3][Hp][Wp] (the logical NCHW values of
    either layout)"""
    F_, Hs, Ws, _ = raw.shape
    (Hc, Wc), (Hp, Wp) = (tab_y.shape[1], tab_x.shape[1]), pad_hw
    out = np.zeros((F_, 3, Hp, Wp), np.float32)
    mean, stdinv = np.asarray(mean, np.float32), np.asarray(stdinv, np.float32)
    for f in range(F_):
        y0, y1, b0, b1 = IM.unpack_taps(tab_y[f])
        x0, x1, a0, a1 = IM.unpack_taps(tab_x[f])
        oky, okx = (tab_y[f, :, 0] >= 0) & (y0 < Hs) & (y1 < Hs), (tab_x[f, :, 0] >= 0) & (x0 < Ws) & (x1 < Ws)
        y0, y1, x0, x1 = np.where(oky, y0, 0), np.where(oky, y1, 0), np.where(okx, x0, 0), np.where(okx, x1, 0)
        S = raw[f].astype(np.int32)
        if to_rgb:
            S = S[..., ::-1]
        a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[:, None, None], b1[:, None, None]
        h0 = S[y0][:, x0] * a0 + S[y0][:, x1] * a1
        h1 = S[y1][:, x0] * a0 + S[y1][:, x1] * a1
        v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
        val = (v.astype(np.float32) - mean) * stdinv
        ok = oky[:, None] & okx[None, :]
        out[f, :, :Hc, :Wc] = np.where(ok[None], val.transpose(2, 0, 1), np.float32(0))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def tables_of(case, an, frames=1):
    aug, chw, pad = aug_of(case, an)
    ty, tx, scale, got_chw = IM.bilinear_tables(FILES[case], *aug)
    assert got_chw == chw
    return np.stack([ty] * frames), np.stack([tx] * frames), aug, pad


# ---- 1. the composed tables, applied per output pixel, are the reference's whole-image pipeline ------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("an", tuple(AUGS))
@pytest.mark.parametrize("to_rgb", (False, True))
def test_tables_equal_the_reference_pipeline(case, an, to_rgb):
    raw = image_of(case)
    ty, tx, aug, pad = tables_of(case, an)
    mean, stdinv = IM.norm_constants(MEAN, STD)
    got = np_image_prepare(raw, ty, tx, pad, mean, stdinv, to_rgb)[0]
    want = np_pipeline(raw[0], aug, pad, to_rgb=to_rgb)
    assert got.shape == want.shape == (3,) + pad and np.array_equal(bits(got), bits(want))
    Hc, Wc = ty.shape[1], tx.shape[1]
    assert not bits(got[:, Hc:]).any() and not bits(got[:, :, Wc:]).any()          # the pad is +0.0
    if AUGS[an][3]:
        assert pad[0] > Hc + 8 and pad[1] > Wc + 8


def test_the_augmentations_cover_what_they_claim():
    (_, _, off, chw), _, _ = aug_of("m", "crop0")
    assert off == (0, 0)
    (resized, _, off, chw), _, _ = aug_of("m", "cropend")
    assert (off[0] + chw[0], off[1] + chw[1]) == resized and off[0] > 0 and off[1] > 0
    assert FILES["m"][1] % 2 == 1 and AUGS["down"][1] and AUGS["small"][1]         # flips on an odd width
    assert aug_of("m", "down")[0][0] == (22, 32) and aug_of("m", "r137")[0][0] == (51, 73)


def test_linear_taps_equal_the_scalar_rule():
    for old, new in ((2, 2), (2, 4), (2, 5), (53, 73), (53, 32), (37, 74), (37, 22), (7, 1), (1, 6), (640, 1333)):
        for axis in "xy":
            i0, i1, w0, w1 = IM.linear_taps(old, new, axis)
            want = cv_taps(old, new, axis)
            assert all(a.dtype == np.int32 and a.shape == (new,) for a in (i0, i1, w0, w1))
            assert [tuple(int(v) for v in t) for t in zip(i0, i1, w0, w1)] == [t[:4] for t in want], (old, new, axis)
            assert i0.min() >= 0 and max(i0.max(), i1.max()) <= old - 1
    # an upscale by 2 along y: the first row keeps its fraction on a clipped index, along x it does not
    assert [int(a[0]) for a in IM.linear_taps(4, 8, "y")] == [0, 0, 512, 1536] and [int(a[0]) for a in IM.linear_taps(4, 8, "x")] == [0, 1, 2048, 0]


# ---- 2. the integer rule against float64 bilinear interpolation at the same taps ---------------------------------------------------------------
def _float_cases():
    rng = np.random.default_rng(7)
    for i in range(300):
        H, W = int(rng.integers(2, 41)), int(rng.integers(2, 41))
        ry, rx = rng.uniform(0.4, 3.0, 2)
        kind = ("random", "checker", "white")[i % 3]
        if kind == "random":
            img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif kind == "checker":
            img = np.broadcast_to(((np.add.outer(np.arange(H), np.arange(W)) & 1) * 255).astype(np.uint8)[..., None], (H, W, 3)).copy()
        else:
            img = np.full((H, W, 3), 255, np.uint8)
        yield kind, img, (max(1, int(H * ry + 0.5)), max(1, int(W * rx + 0.5)))


def test_integer_rule_stays_within_a_grey_level_of_float64():
    """bound: 1.0 grey level.  The horizontal pass is exact (integers), the two >> 4 lose below 2^-7 of a grey level each, the two >> 16
    at most 2^-2 each (the sums carry 2 fraction bits), the final + 2 >> 2 rounds to half a level, and a weight is its fraction within
    2^-12: under one level in all."""
    worst = 0.0
    for kind, img, new_hw in _float_cases():
        got = np_resize(img, new_hw).astype(np.float64)
        ty, tx = cv_taps(img.shape[0], new_hw[0], "y"), cv_taps(img.shape[1], new_hw[1], "x")
        S = img.astype(np.float64)
        rows = np.stack([S[:, x0] * (1.0 - f) + S[:, x1] * f for x0, x1, _, _, f in tx], axis=1)
        want = np.stack([rows[y0] * (1.0 - f) + rows[y1] * f for y0, y1, _, _, f in ty])
        assert got.min() >= 0 and got.max() <= 255
        worst = max(worst, float(np.abs(got - want).max()))
        if kind == "white":
            assert (got == 255).all()
        assert all(w0 + w1 == 2048 for t in (ty, tx) for _, _, w0, w1, _ in t), (img.shape, new_hw)
    assert worst <= 1.0, worst


# ---- 3. weights and identity -------------------------------------------------------------------------------------------------------------
def test_weights_sum_to_one_and_identity_returns_the_source():
    for case in CASES:
        for an in AUGS:
            ty, tx, _, _ = tables_of(case, an)
            for t in (ty[0], tx[0]):
                _, _, w0, w1 = IM.unpack_taps(t)
                assert ((w0 + w1) == 2048).all() and w0.min() >= 0 and w1.min() >= 0
    raw = image_of("m")
    H, W = FILES["m"]
    ty, tx, _, chw = IM.bilinear_tables((H, W), (H, W), False, None, None)
    for t, n in ((ty, H), (tx, W)):                                     # ratio 1: tap i at full weight; the second tap, at weight 0, is i + 1
        i0, _, w0, w1 = IM.unpack_taps(t)
        assert np.array_equal(i0, np.arange(n)) and (w0 == 2048).all() and (w1 == 0).all()
        assert np.array_equal(IM.unpack_taps(IM.identity_table(n))[0], i0) and np.array_equal(IM.identity_table(n)[:, 1], t[:, 1])
    assert chw == (H, W)
    got = np_image_prepare(raw, ty[None], tx[None], (H, W), np.zeros(3, np.float32), np.ones(3, np.float32))
    assert np.array_equal(got[0], raw[0].transpose(2, 0, 1).astype(np.float32))
    assert np.array_equal(np_resize(raw[0], (H, W)), raw[0])


# ---- 4. the same geometry as the ground truth ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("an", tuple(AUGS))
def test_same_geometry_as_the_ground_truth(case, an):
    aug, chw, _ = aug_of(case, an)
    ty, tx, scale, got = IM.bilinear_tables(FILES[case], *aug)
    sy, sx, gscale, ghw = GT.nearest_tables(FILES[case], *aug)
    assert got == ghw == chw == (ty.shape[0], tx.shape[0]) == (sy.size, sx.size)
    assert scale.dtype == gscale.dtype == np.float32 and np.array_equal(scale, gscale)
    # a crop that runs past the resized image is clipped alike
    (nh, nw), flip = aug[0], aug[1]
    past = ((nh, nw), flip, (max(nh - 1, 0), max(nw - 1, 0)), (10, 10))
    assert IM.bilinear_tables(FILES[case], *past)[3] == GT.nearest_tables(FILES[case], *past)[3] == (1, 1)
    if AUGS[an][0] == 1.0:                                                                     # ratio 1: the taps ARE the nearest tables
        i0, i1, w0, w1 = IM.unpack_taps(ty)
        assert np.array_equal(i0, sy) and (w0 == 2048).all() and (w1 == 0).all()
        assert np.array_equal(IM.unpack_taps(tx)[0], sx)


# ---- 5. the test pipeline's metas -----------------------------------------------------------------------------------------------------------
def test_test_metas():
    keys = {"ori_shape", "img_shape", "pad_shape", "batch_input_shape", "scale_factor", "flip", "flip_direction", "img_norm_cfg"}
    for sizes, batch in (([(64, 128)] * 2, (64, 128)), ([(37, 53)], (64, 64)), ([(37, 53), (70, 33)], (96, 64)), ([(1024, 2048)], (1024, 2048))):
        metas = IM.frame_metas(sizes, batch, MEAN, STD, False, 32)
        assert len(metas) == len(sizes)
        for (h, w), m in zip(sizes, metas):
            assert set(m) == keys
            assert m["ori_shape"] == m["img_shape"] == (h, w, 3)
            assert m["pad_shape"] == (-(-h // 32) * 32, -(-w // 32) * 32, 3) and m["batch_input_shape"] == batch
            assert m["pad_shape"][0] % 32 == 0 and m["pad_shape"][1] % 32 == 0 and m["pad_shape"][0] - h < 32 and m["pad_shape"][1] - w < 32
            assert m["scale_factor"].dtype == np.float32 and m["scale_factor"].tolist() == [1.0] * 4
            assert m["flip"] is False and m["flip_direction"] is None
            cfg = m["img_norm_cfg"]
            assert cfg["to_rgb"] is False and cfg["mean"].dtype == np.float32 and np.allclose(cfg["mean"], MEAN) and np.allclose(cfg["std"], STD)
    assert IM.frame_metas([(5, 5)], (8, 8), MEAN, STD, True, 8)[0]["img_norm_cfg"]["to_rgb"] is True


def test_norm_constants_and_argument_errors():
    mean, stdinv = IM.norm_constants(MEAN, STD)
    assert mean.dtype == stdinv.dtype == np.float32
    assert np.array_equal(stdinv, (1 / np.asarray(STD, np.float64)).astype(np.float32)) and np.array_equal(mean, np.asarray(MEAN, np.float32))
    with pytest.raises(ValueError):
        IM.norm_constants(MEAN, [1.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        IM.linear_taps(4, 8, "z")
    with pytest.raises(ValueError):
        IM.bilinear_tables((40000, 8), (8, 8), False, None, None)


def test_argument_errors_come_back_before_any_launch():
    """the checks of `ph_image_prepare` run on the host before the launch, so they answer on a machine without a GPU"""
    import ctypes as C

    import helpers as Hh
    from polyphonicformer_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(256)
    mean, stdinv = IM.norm_constants(MEAN, STD)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def call(frames=2, Hs=37, Ws=53, ty=None, tx=None, Hc=4, Wc=5, Hp=8, Wp=8, dtype=_lib.PH_OUT_F32, layout=_lib.PH_IMG_NCHW, raw=fake, out=fake,
             dev_tab=fake, to_rgb=0, m=mean):
        hy = np.ascontiguousarray(np.stack([IM.identity_table(37)[-Hc:]] * max(frames, 1)) if ty is None else ty, np.int32)
        hx = np.ascontiguousarray(np.stack([IM.identity_table(53)[-Wc:]] * max(frames, 1)) if tx is None else tx, np.int32)
        return lib.ph_image_prepare(raw, frames, Hs, Ws, C.c_void_p(hy.ctypes.data), C.c_void_p(hx.ctypes.data), dev_tab, dev_tab, Hc, Wc, Hp, Wp,
                                    fp(m), fp(stdinv), to_rgb, dtype, layout, out, None)

    row = np.stack([IM.identity_table(37)[-4:]] * 2)
    col = np.stack([IM.identity_table(53)[-5:]] * 2)
    bad_y, bad_x, bad_w, neg = row.copy(), col.copy(), col.copy(), row.copy()
    bad_y[1, 2, 0] = 36 | (37 << 16)
    bad_x[0, 4, 0] = 53 | (52 << 16)
    bad_w[1, 0, 1] = 2049
    neg[0, 1, 0] = -2
    for kw, rc, word in ((dict(ty=bad_y), _lib.PH_EINVAL, "tab_y[1][2]"), (dict(tx=bad_x), _lib.PH_EINVAL, "tab_x[0][4]"),
                         (dict(tx=bad_w), _lib.PH_EINVAL, "weights"), (dict(ty=neg), _lib.PH_EINVAL, "tab_y[0][1]"),
                         (dict(Hp=3), _lib.PH_EINVAL, "Hc <= Hp"), (dict(Wp=4), _lib.PH_EINVAL, "Wc <= Wp"),
                         (dict(frames=0), _lib.PH_EINVAL, "frames"), (dict(frames=65), _lib.PH_EINVAL, "frames"),
                         (dict(dtype=_lib.PH_OUT_F16), _lib.PH_EINVAL, "out_dtype"), (dict(layout=2), _lib.PH_EINVAL, "layout"),
                         (dict(raw=None), _lib.PH_EINVAL, "null"), (dict(out=None), _lib.PH_EINVAL, "null"),
                         (dict(dev_tab=C.c_void_p(260)), _lib.PH_EINVAL, "8-byte"), (dict(out=C.c_void_p(258)), _lib.PH_EINVAL, "aligned"),
                         (dict(to_rgb=2), _lib.PH_EINVAL, "to_rgb"), (dict(m=np.array([0, np.nan, 0], np.float32)), _lib.PH_EINVAL, "finite"),
                         (dict(Hs=32768), _lib.PH_EUNSUPPORTED, "32767"), (dict(Ws=40000), _lib.PH_EUNSUPPORTED, "32767"),
                         (dict(Hs=0), _lib.PH_EINVAL, "sizes")):
        assert call(**kw) == rc, kw
        err = Hh.last_error()
        assert err.startswith("ph_image_prepare") and word in err, (kw, err)
    assert _lib.PH_IMGPREP_MAX_FRAMES == _lib.PH_GTPREP_MAX_FRAMES == 64
