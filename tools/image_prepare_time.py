"""The loader's image work on the device, timed on one GPU at the training size: `ph_image_prepare` against the same steps in torch's own
device ops.  Uint8 HWC frames resident on the device in both sides (their upload, 6 MB a frame, is outside both).

  train   4 frames, 1024 x 2048 file -> ratio 1.5 (1536 x 3072) -> horizontal flip -> crop 1024 x 2048 at (200, 500) -> normalise -> pad
          (none left at this size) -> [4, 3, 1024, 2048], each of fp32 / bf16 x NCHW / channels-last
  test    the test pipeline (identity tables: normalise, pad to a multiple of 32, transpose) at 1 and 8 frames of 1024 x 2048, fp32 NCHW

  A  one `ph_image_prepare` launch on tables uploaded beforehand
  B  torch: uint8 -> float, F.interpolate(bilinear, align_corners=False), flip, crop, normalise, F.pad, the memory format, the cast.  The
     same WORK, not the same bits: torch interpolates in fp32 where the kernel follows OpenCV's 8-bit fixed-point rule (the largest
     difference of the two outputs is reported in grey levels of the normalised image times std).

A and B alternate in one process; per call two HIP events; median of --reps (25).  TB/s = (bytes written + source bytes touched) over A's
time; the source bytes touched are the rows x columns the frame's tables name, 3 bytes each.  Also the wall time of
`image.prepare_images` (host tables, their upload and the launch, synchronised).  Prints one JSON line and writes it to --out.

    python tools/image_prepare_time.py --out profiles/image_prepare/time.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
from polyphonicformer_amd import _lib, image as IM  # noqa: E402

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
FILE = (1024, 2048)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def summary(ms):
    a = np.asarray(ms)
    return {"us": round(float(np.median(a)) * 1e3, 1), "min_us": round(float(a.min()) * 1e3, 1), "max_us": round(float(a.max()) * 1e3, 1)}


def kernel_call(raw, ty, tx, pad, dtype, channels_last):
    """-> (a closure that makes one raw launch on resident tables, its output tensor)"""
    lib = _lib.load()
    B, Hs, Ws, _ = raw.shape
    ty, tx = np.ascontiguousarray(ty), np.ascontiguousarray(tx)
    ty_d, tx_d = torch.from_numpy(ty).to(raw.device), torch.from_numpy(tx).to(raw.device)
    mean, stdinv = IM.norm_constants(MEAN, STD)
    out = torch.empty((B, 3) + tuple(pad), dtype=dtype, device=raw.device,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    keep = (ty, tx, ty_d, tx_d, mean, stdinv)

    def run():
        _lib.check(lib.ph_image_prepare(_lib.ptr(raw), B, Hs, Ws, C.c_void_p(ty.ctypes.data), C.c_void_p(tx.ctypes.data), _lib.ptr(ty_d),
                                        _lib.ptr(tx_d), ty.shape[1], tx.shape[1], pad[0], pad[1], fp(mean), fp(stdinv), 0,
                                        _lib.PH_OUT_BF16 if dtype == torch.bfloat16 else _lib.PH_OUT_F32,
                                        _lib.PH_IMG_NHWC if channels_last else _lib.PH_IMG_NCHW, _lib.ptr(out), _lib.stream_ptr()), "ph_image_prepare")
        return out
    run.keep = keep
    return run


def torch_call(raw, aug, pad, dtype, channels_last):
    mean, stdinv = (torch.from_numpy(a).to(raw.device)[None, :, None, None] for a in IM.norm_constants(MEAN, STD))
    resized, flip, off, chw = aug

    def run():
        x = raw.permute(0, 3, 1, 2).float()
        if tuple(resized) != tuple(raw.shape[1:3]):
            x = F.interpolate(x, size=resized, mode="bilinear", align_corners=False)
        if flip:
            x = x.flip(-1)
        if off is not None:
            x = x[:, :, off[0]:off[0] + chw[0], off[1]:off[1] + chw[1]]
        x = (x - mean) * stdinv
        x = F.pad(x, (0, pad[1] - x.shape[3], 0, pad[0] - x.shape[2]))
        return x.contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format).to(dtype)
    return run


def touched_bytes(ty, tx):
    """source bytes the tables name: per frame (distinct rows) x (distinct columns) x 3"""
    total = 0
    for f in range(ty.shape[0]):
        y0, y1, _, b1 = IM.unpack_taps(ty[f])
        x0, x1, _, a1 = IM.unpack_taps(tx[f])
        rows = set(y0.tolist()) | set(y1[b1 > 0].tolist())
        cols = set(x0.tolist()) | set(x1[a1 > 0].tolist())
        total += len(rows) * len(cols) * 3
    return total


def measure(raw, aug, pad, dtype, channels_last, reps):
    B = raw.shape[0]
    tabs = [IM.bilinear_tables(tuple(raw.shape[1:3]), *aug) for _ in range(B)]
    ty, tx = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    a, b = kernel_call(raw, ty, tx, pad, dtype, channels_last), torch_call(raw, aug, pad, dtype, channels_last)
    for _ in range(3):
        oa, ob = a(), b()
    torch.cuda.synchronize()
    diff = float(((oa.float() - ob.float()).abs() * torch.tensor(STD, device=raw.device)[None, :, None, None]).max())
    del ob
    ta, tb = [], []
    for _ in range(reps):
        ta.append(event_ms(a)[0])
        ms, ob = event_ms(b)
        del ob
        tb.append(ms)
    moved = oa.numel() * oa.element_size() + touched_bytes(ty, tx)
    ra, rb = summary(ta), summary(tb)
    return {"kernel": ra, "torch": rb, "torch_over_kernel": round(rb["us"] / ra["us"], 2), "bytes_written": oa.numel() * oa.element_size(),
            "source_bytes_touched": touched_bytes(ty, tx), "kernel_TB_per_s": round(moved / (ra["us"] * 1e-6) / 1e12, 3),
            "max_abs_diff_grey_levels": round(diff, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_prepare_time.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.integers(0, 256, (8,) + FILE + (3,), dtype=np.uint8)).to(dev)
    train_aug = ((1536, 3072), True, (200, 500), FILE)
    test_aug = (FILE, False, None, None)
    res = {"command": "python tools/image_prepare_time.py", "reps": args.reps,
           "workload": {"train": "4 frames, 1024 x 2048 file, ratio 1.5, flip, crop 1024 x 2048 at (200, 500), pad 1024 x 2048",
                        "test": "identity tables, 1024 x 2048, pad to a multiple of 32 (none left), 1 and 8 frames, fp32 NCHW"},
           "not_measured": "other sizes, graph replay, more than one box or run, the uint8 upload"}
    res["train"] = {}
    for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for cl, ln in ((False, "nchw"), (True, "channels_last")):
            res["train"][f"{dn}_{ln}"] = measure(frames[:4], train_aug, FILE, dtype, cl, args.reps)
    res["test"] = {f"{n}_frames": measure(frames[:n], test_aug, FILE, torch.float32, False, args.reps) for n in (1, 8)}

    # the Python entry: host tables, one upload, the launch
    aug4 = [train_aug] * 4
    IM.prepare_images(frames[:4], aug4, FILE, MEAN, STD, device=dev)
    torch.cuda.synchronize()
    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        IM.prepare_images(frames[:4], aug4, FILE, MEAN, STD, device=dev)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["prepare_images_wall_fp32_nchw_4_frames"] = summary(wall)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
