"""A frame's image from the file's bytes to the tensor the backbone takes, on the device (csrc/ph_imgprep.hip, `ph_image_prepare`).

The reference's train_pipeline (configs/_base_/datasets/cityscapes_dvps.py:8-21, datasets/pipelines/transforms.py) takes the image
through SeqResizeWithDepth (a bilinear resize on uint8 by a ratio of 1 .. 2), SeqFlipWithDepth, SeqRandomCropWithDepth (:227),
SeqNormalizeWithDepth, SeqPadWithDepth(size_divisor=32) and SeqDefaultFormatBundle (the transpose to CHW) on the host and uploads an
fp32 NCHW batch, 25 MB per 1024 x 2048 frame against 6 MB of file bytes.  Resize, flip and crop are separable two-tap gathers, so the
host composes them into one table per axis and frame (`bilinear_tables`) and one launch does the rest.  The tables are made of the
augmentation parameters `gt.prepare_gt_from_panoptic` takes, so a step's image and ground truth cannot disagree on geometry:

    img, prepared = image.prepare_step_inputs(raw_images, raw_maps, raw_depth, aug, num_thing_classes, pad_hw, class_map, mean, std)

The test_pipeline (:23-41: Normalize, Pad(size_divisor=32), ImageToTensor) is the same call with identity tables:

    img, img_metas = image.prepare_test_images(frames, mean, std)          # uint8 HWC camera frames -> what VideoStreamRunner takes
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import gt as GT

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS              # OpenCV's INTER_RESIZE_COEF_SCALE: a tap weight is 0 .. 2048


def linear_taps(old, new, axis):
    """host: the two taps of every destination index of a bilinear resize old -> new along `axis` ("x" or "y") -> (i0, i1, w0, w1), int32
    [new] each: source indices and weights of 11 bits, w0 + w1 = 2048.  OpenCV's INTER_LINEAR rule for 8-bit images:
        scale = 1.0 / (double(new) / old);  f = float32((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s
        x:  s < 0 -> s = 0, f = 0;  s >= old - 1 -> s = old - 1, f = 0;  i0 = s, i1 = min(s + 1, old - 1)
        y:  i0 = clip(s, 0, old - 1), i1 = clip(s + 1, 0, old - 1), the fraction is kept
        w1 = rint(f * 2048), w0 = rint((1 - f) * 2048): round half to even, the products in fp32
    The rule is RESTATED here, not checked against the library: cv2 and mmcv are not available where this package is built and tested,
    and an OpenCV built with IPP may differ from its own generic path by a grey level.  A loader that needs its library's exact taps
    supplies its own tables; `ph_image_prepare` takes the tables and not the rule for that reason."""
    if axis not in ("x", "y"):
        raise ValueError(f"linear_taps: axis is 'x' or 'y', got {axis!r}")
    old, new = int(old), int(new)
    if old < 1 or new < 1:
        raise ValueError(f"linear_taps: sizes of at least 1, got {old} -> {new}")
    scale = 1.0 / (float(new) / float(old))
    f = ((np.arange(new, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    if axis == "x":
        low, high = s < 0, s >= old - 1
        s = np.where(low, 0, np.where(high, old - 1, s)).astype(np.int32)
        f = np.where(low | high, np.float32(0), f).astype(np.float32)
        i0, i1 = s, np.minimum(s + 1, old - 1)
    else:
        i0, i1 = np.clip(s, 0, old - 1), np.clip(s + 1, 0, old - 1)
    w1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int32)
    w0 = np.rint((np.float32(1) - f) * np.float32(COEF_ONE)).astype(np.int32)
    return i0.astype(np.int32), i1.astype(np.int32), w0, w1


def pack_taps(i0, i1, w0, w1):
    """(i0, i1, w0, w1) [n] each -> int32 [n][2], the table words of `ph_image_prepare`: i0 | i1 << 16, w0 | w1 << 16"""
    t = np.empty((len(i0), 2), np.int32)
    t[:, 0] = np.asarray(i0, np.int32) | (np.asarray(i1, np.int32) << 16)
    t[:, 1] = np.asarray(w0, np.int32) | (np.asarray(w1, np.int32) << 16)
    return t


def unpack_taps(tab):
    """int32 [..][2] table words -> (i0, i1, w0, w1); the entries of a word -1 (none) come back as they are packed"""
    tab = np.asarray(tab)
    return tab[..., 0] & 0xFFFF, (tab[..., 0] >> 16) & 0xFFFF, tab[..., 1] & 0xFFFF, (tab[..., 1] >> 16) & 0xFFFF


def identity_table(n):
    """the table of an axis that is not resized: tap i with weight 2048, the second tap (weight 0) on the same index"""
    i = np.arange(n, dtype=np.int32)
    return pack_taps(i, i, np.full(n, COEF_ONE, np.int32), np.zeros(n, np.int32))


def bilinear_tables(src_hw, resized_hw, flip, crop_offset, crop_hw):
    """host: the resize to resized_hw, the horizontal flip (bool) and the crop (offset (y, x), size (h, w), clipped by the resized image
    as the reference's slice is; crop_offset = None: no crop) of one frame composed into two tap tables -- the arguments and the
    composition of `gt.nearest_tables` -> (tab_y int32 [Hc][2], tab_x int32 [Wc][2], scale_factor fp32 (w, h, w, h), (Hc, Wc)).
    scale_factor and (Hc, Wc) equal `gt.nearest_tables`' for every input.  The taps are `linear_taps`': a restatement, see there."""
    (H, W), (nh, nw) = src_hw, resized_hw
    if H > 32767 or W > 32767:
        raise ValueError(f"bilinear_tables: a file of {H} x {W}; a table word holds two indices of 15 bits")
    ty, tx = pack_taps(*linear_taps(H, nh, "y")), pack_taps(*linear_taps(W, nw, "x"))
    if flip:
        tx = tx[::-1]
    if crop_offset is not None:
        (oy, ox), (ch, cw) = crop_offset, crop_hw
        ty, tx = ty[oy:oy + ch], tx[ox:ox + cw]
    scale = np.array([nw / W, nh / H, nw / W, nh / H], dtype=np.float32)
    return np.ascontiguousarray(ty), np.ascontiguousarray(tx), scale, (int(ty.shape[0]), int(tx.shape[0]))


def norm_constants(mean, std):
    """-> (mean fp32 [3], stdinv fp32 [3]) as mmcv.imnormalize forms them: float32(float64(mean)), float32(1 / float64(std))"""
    mean = np.asarray(mean, np.float64).reshape(-1)
    std = np.asarray(std, np.float64).reshape(-1)
    if mean.size != 3 or std.size != 3 or not (std != 0).all():
        raise ValueError("image: mean and std have three entries, and no std is zero")
    return mean.astype(np.float32), (1.0 / std).astype(np.float32)


def _out_strides(shape, channels_last):
    B, _, Hp, Wp = shape
    return (3 * Hp * Wp, 1, Wp * 3, 3) if channels_last else (3 * Hp * Wp, Hp * Wp, Wp, 1)


def image_prepare(raw, tab_y, tab_x, pad_hw, mean, stdinv, to_rgb=False, dtype=torch.float32, channels_last=False, out=None):
    """one raw `ph_image_prepare` call per 64 frames.  raw: contiguous uint8 [F, Hs, Ws, 3] on the device; tab_y int32 [F, Hc, 2] and tab_x
    int32 [F, Wc, 2] on the host (word 0 == -1: none); mean, stdinv fp32 [3].  Uploads both tables in one copy -> [F, 3, Hp, Wp] of
    `dtype` (fp32 or bf16), channels-last memory when asked; `out` supplies the buffer."""
    if not raw.is_cuda:
        raise _lib.PolyheadError("image_prepare: the images must live on the GPU: libpolyhead has no CPU path")
    if raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[3] != 3 or raw.shape[0] == 0 or not raw.is_contiguous():
        raise ValueError(f"image_prepare: raw must be contiguous uint8 [frames, Hs, Ws, 3] with at least one frame, got {tuple(raw.shape)}")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"image_prepare: dtype is torch.float32 or torch.bfloat16, got {dtype}")
    F_, Hs, Ws, _ = raw.shape
    dev = raw.device
    tab_y, tab_x = np.ascontiguousarray(tab_y, dtype=np.int32), np.ascontiguousarray(tab_x, dtype=np.int32)
    if tab_y.ndim != 3 or tab_x.ndim != 3 or tab_y.shape[0] != F_ or tab_x.shape[0] != F_ or tab_y.shape[2] != 2 or tab_x.shape[2] != 2:
        raise ValueError("image_prepare: one tab_y [Hc][2] and one tab_x [Wc][2] per frame")
    (Hc, Wc), (Hp, Wp) = (tab_y.shape[1], tab_x.shape[1]), (int(pad_hw[0]), int(pad_hw[1]))
    shape = (F_, 3, Hp, Wp)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    else:
        want = _out_strides(shape, channels_last)
        if tuple(out.shape) != shape or out.dtype != dtype or out.device != dev or \
                any(s != w for s, w, n in zip(out.stride(), want, shape) if n > 1):
            raise ValueError(f"image_prepare: out must be {dtype} {shape} on {dev} with strides {want}")
    d = GT._up(np.concatenate((tab_y.ravel(), tab_x.ravel())), dev)
    ty_d, tx_d = d[:tab_y.size], d[tab_y.size:]
    mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(3)
    stdinv = np.ascontiguousarray(stdinv, dtype=np.float32).reshape(3)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    lib = _lib.load()
    frame_bytes = 3 * Hp * Wp * out.element_size()
    for f0 in range(0, F_, _lib.PH_IMGPREP_MAX_FRAMES):
        n = min(F_, f0 + _lib.PH_IMGPREP_MAX_FRAMES) - f0
        hy, hx = tab_y[f0:f0 + n], tab_x[f0:f0 + n]
        _lib.check(lib.ph_image_prepare(
            _lib.ptr(raw[f0:f0 + n]), n, Hs, Ws, C.c_void_p(hy.ctypes.data), C.c_void_p(hx.ctypes.data), _lib.ptr(ty_d[f0 * Hc * 2:]),
            _lib.ptr(tx_d[f0 * Wc * 2:]), Hc, Wc, Hp, Wp, fp(mean), fp(stdinv), int(bool(to_rgb)),
            _lib.PH_OUT_BF16 if dtype == torch.bfloat16 else _lib.PH_OUT_F32, _lib.PH_IMG_NHWC if channels_last else _lib.PH_IMG_NCHW,
            C.c_void_p(out.data_ptr() + f0 * frame_bytes), _lib.stream_ptr()), "ph_image_prepare")
    return out


def _raw_images(raw, dev, what):
    """host or device images -> contiguous uint8 device tensor [B, Hs, Ws, 3]"""
    if not torch.is_tensor(raw):
        raw = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(r) for r in raw]) if isinstance(raw, (list, tuple)) else np.asarray(raw)))
    if raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[3] != 3 or raw.shape[0] == 0:
        raise ValueError(f"{what}: uint8 [frames][Hs][Ws][3] with at least one frame, got {raw.dtype} {tuple(raw.shape)}")
    return raw.to(dev, non_blocking=True).contiguous()


def _stack_tables(tabs, n):
    """per-frame tables of different lengths -> int32 [B][n][2], the word -1 (none) beyond each"""
    out = np.full((len(tabs), n, 2), -1, np.int32)
    for b, t in enumerate(tabs):
        out[b, :t.shape[0]] = t
    return out


def prepare_images(raw, aug, pad_hw, mean, std, to_rgb=False, dtype=torch.float32, channels_last=False, out=None, device="cuda"):
    """The step's images from what the files hold.  raw: uint8 [B, Hs, Ws, 3] on host or device, the images as decoded (the channel order of
    the file reader; to_rgb reverses it as mmcv.imnormalize does); aug: per frame (resized_hw, flip, crop_offset, crop_hw), exactly what
    `gt.prepare_gt_from_panoptic` takes; pad_hw: the batch's padded size; mean, std: the img_norm_cfg.  Builds the tap tables on the host,
    uploads them in one copy and makes one `ph_image_prepare` call per 64 frames -> [B, 3, Hp, Wp] of `dtype` (torch.float32 or
    torch.bfloat16), in channels-last memory when asked; zero (in normalised units) beyond each frame's augmented size."""
    raw = _raw_images(raw, torch.device(device), "prepare_images")
    B, Hs, Ws, _ = raw.shape
    if len(aug) != B:
        raise ValueError("prepare_images: one augmentation per frame")
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    tabs = [bilinear_tables((Hs, Ws), *a) for a in aug]
    Hc, Wc = max(t[3][0] for t in tabs), max(t[3][1] for t in tabs)
    if Hc > Hp or Wc > Wp:
        raise ValueError(f"prepare_images: the augmented frames are {Hc} x {Wc}, above pad_hw {Hp} x {Wp}")
    m, si = norm_constants(mean, std)
    return image_prepare(raw, _stack_tables([t[0] for t in tabs], Hc), _stack_tables([t[1] for t in tabs], Wc), (Hp, Wp), m, si, to_rgb=to_rgb,
                         dtype=dtype, channels_last=channels_last, out=out)


def prepare_step_inputs(raw_images, raw_maps, raw_depth, aug, num_thing_classes, pad_hw, class_map, mean, std, to_rgb=False,
                        dtype=torch.float32, channels_last=False, device="cuda", **gt_kwargs):
    """a training step's inputs from the files' bytes and ONE set of augmentation parameters: `prepare_images` and
    `gt.prepare_gt_from_panoptic` (which takes gt_kwargs: raw_divisor, divisor, no_obj_class, mask_assign_stride, want_hard, nearest,
    tables, depth_div, depth_max) on one `aug` and one `pad_hw` -> (img [B, 3, Hp, Wp], PreparedGT)"""
    img = prepare_images(raw_images, aug, pad_hw, mean, std, to_rgb=to_rgb, dtype=dtype, channels_last=channels_last, device=device)
    return img, GT.prepare_gt_from_panoptic(raw_maps, raw_depth, aug, num_thing_classes, pad_hw, class_map, device=device, **gt_kwargs)


def frame_metas(sizes, batch_hw, mean, std, to_rgb, size_divisor):
    """host: per frame the meta the test_pipeline's Collect step and the detector's forward_test leave (cityscapes_dvps.py:34-39), for
    frames of `sizes` (h, w) in a batch padded to batch_hw"""
    up = lambda v: -(-v // size_divisor) * size_divisor
    cfg = dict(mean=np.asarray(mean, np.float32), std=np.asarray(std, np.float32), to_rgb=bool(to_rgb))
    return [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(up(h), up(w), 3), batch_input_shape=tuple(batch_hw),
                 scale_factor=np.ones(4, np.float32), flip=False, flip_direction=None, img_norm_cfg=cfg) for h, w in sizes]



def prepare_test_images(frames, mean, std, to_rgb=False, size_divisor=32, dtype=torch.float32, channels_last=False, device="cuda"):
    """the test_pipeline on uint8 HWC camera frames: Normalize, Pad up to the divisor, ImageToTensor -- identity tables through
    `ph_image_prepare`.  frames: uint8 [B, H, W, 3] on host or device, or a list of host [h, w, 3] frames (of different sizes: the batch
    is padded to the largest) -> (img [B, 3, Hp, Wp], img_metas), one meta per frame with ori_shape, img_shape, pad_shape,
    batch_input_shape, scale_factor (ones), flip=False, flip_direction=None and img_norm_cfg."""
    dev = torch.device(device)
    if isinstance(frames, (list, tuple)) and len({tuple(np.shape(f)) for f in frames}) > 1:
        fr = [np.asarray(f) for f in frames]
        if any(f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8 for f in fr):
            raise ValueError("prepare_test_images: a frame is uint8 [h][w][3]")
        sizes = [f.shape[:2] for f in fr]
        host = np.zeros((len(fr), max(h for h, _ in sizes), max(w for _, w in sizes), 3), np.uint8)
        for b, f in enumerate(fr):
            host[b, :f.shape[0], :f.shape[1]] = f
        raw = _raw_images(host, dev, "prepare_test_images")
    else:
        raw = _raw_images(frames, dev, "prepare_test_images")
        sizes = [tuple(raw.shape[1:3])] * raw.shape[0]
    Hs, Ws = raw.shape[1:3]
    up = lambda v: -(-v // size_divisor) * size_divisor
    Hp, Wp = up(Hs), up(Ws)
    m, si = norm_constants(mean, std)
    tab_y = _stack_tables([identity_table(h) for h, _ in sizes], Hs)
    tab_x = _stack_tables([identity_table(w) for _, w in sizes], Ws)
    img = image_prepare(raw, tab_y, tab_x, (Hp, Wp), m, si, to_rgb=to_rgb, dtype=dtype, channels_last=channels_last)
    return img, frame_metas(sizes, (Hp, Wp), mean, std, to_rgb, size_divisor)

