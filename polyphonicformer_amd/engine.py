"""Host orchestration of the decode hot path on one GPU: owns the device buffers (torch tensors are
used for allocation and streams only) and issues the libpolyhead kernels on the current stream.

Per frame-batch the launch sequence is

    ingest(x), ingest(depth_feats), binarize(mask_preds)
    for s in 0..S-1:   pool -> query_stage(pre, post) -> dynconv (bits for s < S-1, logits for s = S-1)
    upsample2x(mask) ; dynconv(depth) ; upsample2x(depth)

No step synchronises or allocates once a `DecodePlan` exists, so the whole sequence can be captured
into a HIP graph (`DecodePlan.capture`)."""
import contextlib
import ctypes as C
import math

import torch

from . import _lib, knobs
from .pack import pack_stage

import collections

# Precision modes of the decode path.  One row = the arithmetic of every operator of a stage:
#   feat  : element format / planes of the feature maps (ingest, pool)        query : the query-side GEMMs
#   conv  : the dynamic 1x1 conv (feature planes x kernel planes)             kern_fmt : what the query kernel emits for it
Mode = collections.namedtuple("Mode", "name feat query conv kern_fmt FP KP feat_dtype")
# query side of the modes that emit fp16 dynamic kernels: hybrid grade (updator half hi/lo bf16, attention / FFN / tower half one
# fp16 plane, include/polyhead.h PH_PREC_QHYBRID) unless PH_QUERY_FULL_SPLIT=1 asks for hi/lo bf16 throughout (read here, at
# import: MODES is a module constant)
_QH = _lib.PH_PREC_SPLIT if knobs.get("PH_QUERY_FULL_SPLIT") else _lib.PH_PREC_QHYBRID
MODES = {
    # fast: bf16 everywhere, one plane (6e-3 per stage against fp32)
    "bf16": Mode("bf16", _lib.PH_PREC_BF16, _lib.PH_PREC_BF16, _lib.PH_PREC_BF16, _lib.PH_KERN_BF16_PLANES, 1, 1, torch.bfloat16),
    # bf16 feature planes as they are (cfg2's input dtype), everything computed FROM them at fp32 grade: exact 0/1 x bf16
    # pooling, hi/lo split query GEMMs, hi/lo dynamic kernels x one feature plane (<= 1e-3 on identical inputs)
    "mixed": Mode("mixed", _lib.PH_PREC_BF16, _lib.PH_PREC_SPLIT, _lib.PH_PREC_BF16_KSPLIT, _lib.PH_KERN_BF16_PLANES, 1, 2, torch.bfloat16),
    # as `mixed`, but the dynamic kernels as ONE fp16 plane: the conv converts its bf16 feature fragments to fp16 in registers
    # (exact) and runs one f16 MFMA -- the single-plane conv speed (kernel rounding 2^-12: 2.5e-4 per stage on its own)
    "mixed16": Mode("mixed16", _lib.PH_PREC_BF16, _QH, _lib.PH_PREC_BF16_KF16, _lib.PH_KERN_F16, 1, 1, torch.bfloat16),
    # fp16 feature planes / kernels / outputs (cfg5), fp32-grade query side
    "fp16": Mode("fp16", _lib.PH_PREC_F16, _QH, _lib.PH_PREC_F16, _lib.PH_KERN_F16, 1, 1, torch.float16),
    # parity grade: every operand hi + lo (1.6e-5 per stage)
    "fp32": Mode("fp32", _lib.PH_PREC_SPLIT, _lib.PH_PREC_SPLIT, _lib.PH_PREC_SPLIT, _lib.PH_KERN_BF16_PLANES, 2, 2, None),
}
MODES["split"] = MODES["fp32"]
# arithmetic of the kernels that know two grades only (KernelHead, the neck, the track head): fast or fp32 grade
PREC = {"bf16": _lib.PH_PREC_BF16, "split": _lib.PH_PREC_SPLIT, "fp32": _lib.PH_PREC_SPLIT,
        "mixed": _lib.PH_PREC_SPLIT, "mixed16": _lib.PH_PREC_SPLIT, "fp16": _lib.PH_PREC_SPLIT}
# KernelHead's post-neck part (a1) and the neck have a third grade: "fp16" = ONE fp16 plane of the maps and weights (2^-12 per operand, one
# MFMA per product), whose planes and mask bits the decode's `fp16` mode adopts as they are
KHEAD_PREC = dict(PREC, fp16=_lib.PH_PREC_F16)
OUT_CODE = {torch.float32: _lib.PH_OUT_F32, torch.bfloat16: _lib.PH_OUT_BF16, torch.float16: _lib.PH_OUT_F16}


def mode_of(p):
    """Mode from a Mode, a mode name, or a legacy precision code (PH_PREC_BF16 / PH_PREC_SPLIT)"""
    if isinstance(p, Mode):
        return p
    if isinstance(p, str):
        return MODES[p]
    return {_lib.PH_PREC_BF16: MODES["bf16"], _lib.PH_PREC_SPLIT: MODES["fp32"], _lib.PH_PREC_F16: MODES["fp16"]}[p]


def hw_padded(hw):
    return (hw + 127) // 128 * 128


def n_padded(n):
    return (n + 31) // 32 * 32


def _require_gpu(t, name):
    if not t.is_cuda:
        raise _lib.PolyheadError(f"{name} must live on the GPU: libpolyhead has no CPU path")


class StagePack:
    """device-resident packed weights of one KernelUpdateHead stage"""

    def __init__(self, sd, prefix, num_classes, prec, device):
        wb, wf, lay = pack_stage(sd, prefix, num_classes, prec)
        self.wb = wb.to(device)
        self.wf = wf.to(device)
        self.lay = lay
        self.num_classes = num_classes
        self.prec = prec


def default_nsplit(B, HW, frame_invariant=False):
    """pixel ranges per frame for the split-K pooling: PH_POOL_NSPLIT when set, else the library's rule (ph_pool_default_nsplit,
    csrc/ph_pool.hip, which also says what `frame_invariant` -- the split of a ONE-frame launch whatever B is -- buys)"""
    n = knobs.get("PH_POOL_NSPLIT")
    if n is not None:                   # a set 0 included (knobs.py: the known oddity against the cfg builders' "0 = the rule")
        return n
    return int(_lib.load().ph_pool_default_nsplit(B, HW, int(bool(frame_invariant))))


# ---- thin op wrappers (each = one C-ABI call) ---------------------------------------------------
def ingest(x, prec, out=None):
    """fp32 [B,256,H,W] -> bf16 planes int16 [P,B,256,HWp]"""
    _require_gpu(x, "x")
    B, Cc, H, W = x.shape
    if Cc != 256:
        raise _lib.PolyheadError("libpolyhead supports 256 channels (the shipped configs)")
    x = x.contiguous().float()
    P = 2 if prec == _lib.PH_PREC_SPLIT else 1          # PH_PREC_BF16 / PH_PREC_F16: one plane
    if out is None:
        out = torch.empty((P, B, 256, hw_padded(H * W)), dtype=torch.int16, device=x.device)
    lib = _lib.load()
    _lib.check(lib.ph_ingest_features(_lib.ptr(x), _lib.ptr(out), B, H * W, prec, _lib.stream_ptr()), "ph_ingest_features")
    return out


def binarize(m, out=None):
    """mask logits [B,N,H,W] (fp32, or fp16 / bf16 as a 16-bit KernelHead grade hands them over) -> mask bits int32 [B,Npad,HWp/32]"""
    _require_gpu(m, "mask_preds")
    B, N, H, W = m.shape
    m = m.contiguous() if m.dtype in OUT_CODE else m.contiguous().float()
    if out is None:
        out = torch.empty((B, n_padded(N), hw_padded(H * W) // 32), dtype=torch.int32, device=m.device)
    lib = _lib.load()
    _lib.check(lib.ph_binarize_if(_lib.ptr(m), OUT_CODE[m.dtype], 0, _lib.ptr(out), B, N, H * W, None, _lib.stream_ptr()), "ph_binarize")
    return out


def pool(xp, dp, bits, N, HW, prec, nsplit=None, out=None, counts=None):
    """`counts`: optional int32 [B, nsplit, Npad] that receives the masks' pixel counts per pixel range (ph_pool_counts)"""
    B = xp.shape[1]
    if nsplit is None:
        nsplit = default_nsplit(B, HW)
    if out is None:
        out = torch.empty((B, nsplit, n_padded(N), 512), dtype=torch.float32, device=xp.device)
    lib = _lib.load()
    if counts is not None:
        _lib.check(lib.ph_pool_counts(_lib.ptr(xp), _lib.ptr(dp), _lib.ptr(bits), _lib.ptr(out), _lib.ptr(counts), B, N, HW, nsplit, prec,
                                      _lib.stream_ptr()), "ph_pool_counts")
    else:
        _lib.check(lib.ph_pool(_lib.ptr(xp), _lib.ptr(dp), _lib.ptr(bits), _lib.ptr(out), B, N, HW, nsplit, prec,
                               _lib.stream_ptr()), "ph_pool")
    return out


def query_stage(partial, bits, k_in, q_in, pack, N, HW, cls_sigmoid=False, outs=None, workspace=None, phases=3,
                kern_fmt=_lib.PH_KERN_BF16_PLANES, counts=None):
    B, nsplit = partial.shape[0], partial.shape[1]
    dev = partial.device
    prec = pack.prec
    P = 1 if kern_fmt == _lib.PH_KERN_F16 else (2 if prec == _lib.PH_PREC_SPLIT else 1)     # planes of `kern`
    Npad = n_padded(N)
    lib = _lib.load()
    if outs is None:
        outs = dict(obj=torch.empty((B, N, 256), dtype=torch.float32, device=dev),
                    dobj=torch.empty((B, N, 256), dtype=torch.float32, device=dev),
                    cls=torch.empty((B, N, pack.num_classes), dtype=torch.float32, device=dev),
                    kern=torch.empty((P, 2, B, Npad, 256), dtype=torch.int16, device=dev),
                    kbias=torch.empty((2, B, Npad), dtype=torch.float32, device=dev))
    if workspace is None:
        workspace = torch.empty((lib.ph_query_workspace_bytes(B, N, prec),), dtype=torch.uint8, device=dev)
    tail = (_lib.ptr(k_in), _lib.ptr(q_in), _lib.ptr(pack.wb), _lib.ptr(pack.wf), C.byref(pack.lay),
            _lib.ptr(outs["obj"]), _lib.ptr(outs["dobj"]), _lib.ptr(outs["cls"]), 1 if cls_sigmoid else 0, _lib.ptr(outs["kern"]),
            _lib.ptr(outs["kbias"]), _lib.ptr(workspace), workspace.numel(), B, N, HW, prec, kern_fmt, phases, _lib.stream_ptr())
    if counts is not None:
        _lib.check(lib.ph_query_stage_counts(_lib.ptr(partial), nsplit, _lib.ptr(bits), _lib.ptr(counts), *tail), "ph_query_stage_counts")
    else:
        _lib.check(lib.ph_query_stage(_lib.ptr(partial), nsplit, _lib.ptr(bits), *tail), "ph_query_stage")
    return outs


def dynconv(planes, kern, kbias, branch, N, HW, prec, bits_out=None, logits_out=None, out_dtype=_lib.PH_OUT_F32):
    """per-frame dynamic kernels: kern [P,2,B,Npad,256], kbias [2,B,Npad]; `branch` = mask (0) / depth (1)."""
    B, Npad = kern.shape[2], kern.shape[3]
    lib = _lib.load()
    kptr = C.c_void_p(kern.data_ptr() + branch * B * Npad * 256 * 2)
    bptr = C.c_void_p(kbias.data_ptr() + branch * B * Npad * 4)
    _lib.check(lib.ph_dynconv(_lib.ptr(planes), kptr, 2 * B * Npad * 256, Npad * 256, bptr, Npad, _lib.ptr(bits_out),
                              _lib.ptr(logits_out), out_dtype, N * HW, B, N, HW, prec, _lib.stream_ptr()), "ph_dynconv")
    return bits_out if bits_out is not None else logits_out


def dynconv_poolx(planes, kern, kbias, N, HW, prec, bits_out, partial):
    """non-final stage's mask conv (branch 0) -> mask bits, AND the next stage's pooling of the x map (columns 0 .. 255 of
    `partial` [B, nsplit, Npad, 512]) from one read of the plane (ph_dynconv_poolx); kern [1,2,B,Npad,256], kbias [2,B,Npad]"""
    B, Npad = kern.shape[2], kern.shape[3]
    lib = _lib.load()
    _lib.check(lib.ph_dynconv_poolx(_lib.ptr(planes), _lib.ptr(kern), Npad * 256, _lib.ptr(kbias), Npad, _lib.ptr(bits_out), _lib.ptr(partial),
                                    partial.shape[1], B, N, HW, prec, _lib.stream_ptr()), "ph_dynconv_poolx")
    return bits_out


def pool_depth_only(dp, bits, N, HW, prec, partial, counts):
    """the depth_feats half of a pooling whose x half ph_dynconv_poolx has written: columns 256 .. 511 of `partial` and the pixel counts"""
    B, nsplit = partial.shape[0], partial.shape[1]
    lib = _lib.load()
    _lib.check(lib.ph_pool_counts(_lib.ptr(dp), None, _lib.ptr(bits), C.c_void_p(partial.data_ptr() + 256 * 4), _lib.ptr(counts), B, N, HW, nsplit, prec,
                                  _lib.stream_ptr()), "ph_pool_counts(depth)")


def pool_depth_pair(dp, bits_a, bits_b, N, HW, prec, partial_a, partial_b, counts_a, counts_b):
    """pool_depth_only under two mask sets from ONE read of depth_feats (ph_pool_depth_pair): the same bits as two calls"""
    B, nsplit = partial_a.shape[0], partial_a.shape[1]
    _lib.check(_lib.load().ph_pool_depth_pair(_lib.ptr(dp), _lib.ptr(bits_a), _lib.ptr(bits_b), _lib.ptr(partial_a), _lib.ptr(partial_b),
                                              _lib.ptr(counts_a), _lib.ptr(counts_b), B, N, HW, nsplit, prec, _lib.stream_ptr()),
               "ph_pool_depth_pair")


def dynconv_up2(planes, kern, kbias, branch, N, H, W, prec, up_out, logits_out=None, out_dtype=_lib.PH_OUT_F16, workgroups=0):
    """final-stage dynamic conv + x2 bilinear upsample in one kernel (ph_dynconv_up2): kern [1,2,B,Npad,256] (one 16-bit
    plane), kbias [2,B,Npad]; writes up_out [B,N,2H,2W] and, when given, the low-resolution logits [B,N,H,W].
    `workgroups`: 0 = one per CU; a launch that shares the GPU ends sooner with 1.5 per CU (ph_dynconv_up2_wgs; same values)"""
    B, Npad = kern.shape[2], kern.shape[3]
    lib = _lib.load()
    kptr = C.c_void_p(kern.data_ptr() + branch * B * Npad * 256 * 2)
    bptr = C.c_void_p(kbias.data_ptr() + branch * B * Npad * 4)
    _lib.check(lib.ph_dynconv_up2_wgs(_lib.ptr(planes), kptr, Npad * 256, bptr, Npad, _lib.ptr(logits_out), _lib.ptr(up_out), out_dtype,
                                      B, N, H, W, prec, int(workgroups), _lib.stream_ptr()), "ph_dynconv_up2")
    return up_out


def static_conv(planes, wplanes, bias, N, HW, prec, logits_out, out_rows):
    """the same 1x1 conv weights for every frame: wplanes [P,Npad,256] bf16 planes, bias fp32 [Npad];
    writes fp32 logits into rows [0, N) of each frame of `logits_out` ([B, out_rows, H, W] view)."""
    B = planes.shape[1]
    Npad = wplanes.shape[1]
    lib = _lib.load()
    _lib.check(lib.ph_dynconv(_lib.ptr(planes), _lib.ptr(wplanes), Npad * 256, 0, _lib.ptr(bias), 0, None,
                              _lib.ptr(logits_out), _lib.PH_OUT_F32, out_rows * HW, B, N, HW, prec, _lib.stream_ptr()),
               "ph_dynconv(static)")
    return logits_out


def upsample2x(src, out=None):
    """[..., H, W] fp32 or bf16 -> [..., 2H, 2W] (bilinear, align_corners=False)"""
    _require_gpu(src, "src")
    src = src.contiguous()
    H, W = src.shape[-2:]
    planes = src.numel() // (H * W)
    if out is None:
        out = torch.empty(tuple(src.shape[:-2]) + (2 * H, 2 * W), dtype=src.dtype, device=src.device)
    if src.dtype not in OUT_CODE:
        raise _lib.PolyheadError("upsample2x: fp32, bf16 or fp16 only")
    dt = OUT_CODE[src.dtype]
    lib = _lib.load()
    _lib.check(lib.ph_upsample2x(_lib.ptr(src), _lib.ptr(out), dt, planes, H, W, _lib.stream_ptr()), "ph_upsample2x")
    return out


# ---- the S-stage plan ------------------------------------------------------------------------------
POOL_PAIR = knobs.get("PH_POOL_PAIR") != "0"       # A/B: DecodePlan's paired depth pooling of the last two stages (read once, here)


def _knob_code(off, on, on_code):
    """a cfg's off / on / auto field (include/polyhead.h PH_KNOB_*): PH_KNOB_OFF if `off`, else `on_code` if `on`, else
    PH_KNOB_AUTO.  `on_code` says what "on" asks of the library: PH_KNOB_WHERE_SUPPORTED (the decode's fields: the fused form
    wherever it exists, the plain one elsewhere) or PH_KNOB_ON (KernelHead's and the neck's: an error where AUTO says no)"""
    return _lib.PH_KNOB_OFF if off else (on_code if on else _lib.PH_KNOB_AUTO)


def native_cfg(B, N, H, W, S, L, F, prec, out_dtype=torch.float32, frame_invariant=False, shares_gpu=False, nsplit=None):
    """the ph_decode_cfg of a decode plan, Python or native.  The decode's variables (knobs.py: PH_CONV_POOLX, PH_CONV_UP2,
    PH_POOL_NSPLIT, PH_POOLX_NSPLIT, PH_UP2_SHARED_WGS) are read here, through knobs.get, at every call, and become the cfg's
    explicit fields -- the library itself never reads them.  DecodePlan asks the library for its launch geometry with it
    (ph_decode_geometry_of), NativeDecodePlan creates its plan from it, so the two agree by construction"""
    mode = mode_of(prec)
    poolx, up2 = knobs.get("PH_CONV_POOLX"), knobs.get("PH_CONV_UP2")
    return _lib.DecodeCfg(B=B, N=N, H=H, W=W, S=S, L=L, F=F, mode=_lib.PH_MODE[mode.name], out_dtype=OUT_CODE[out_dtype],
                          frame_invariant=int(bool(frame_invariant)),
                          query_full_split=int(mode.name in ("mixed16", "fp16") and mode.query == _lib.PH_PREC_SPLIT),
                          shares_gpu=int(bool(shares_gpu)),
                          poolx=_knob_code(poolx == "0", poolx == "1", _lib.PH_KNOB_WHERE_SUPPORTED),
                          fused_up=_knob_code(up2 == "0", up2 == "1", _lib.PH_KNOB_WHERE_SUPPORTED),
                          nsplit=int(nsplit or knobs.get("PH_POOL_NSPLIT") or 0),
                          nsplit_px=0 if frame_invariant else knobs.get("PH_POOLX_NSPLIT") or 0,
                          up2_wgs=knobs.get("PH_UP2_SHARED_WGS") or 0)


def _cfg_error(what):
    msg = _lib.load().ph_last_error_string()
    return _lib.PolyheadError(f"{what}: {msg.decode() if msg else ''}")


class DecodePlan:
    """All buffers for `simple_test_mask_preds` at one (B, N, H, W, precision, output dtype)."""

    def __init__(self, packs, B, N, H, W, prec, out_dtype=torch.float32, device="cuda:0", nsplit=None, frame_invariant=False,
                 shares_gpu=False, pair=None):
        """`pair`: the last two stages pool depth_feats in one launch (None: POOL_PAIR; only where the plan can, see `self.pair`).
        `frame_invariant` (round 6): every choice that touches a frame's arithmetic -- the pooling's pixel split, the fused / two-
        kernel final stage -- is the ONE-frame launch's at any B, so a frame's outputs do not depend on its batch (the module API's
        default; a clip's frames through one launch equal the per-frame loop bit for bit).
        `shares_gpu`: the plan is one part of a multi-stream step (DualDecodePlan): query launches with the most rows per workgroup
        (PH_QUERY_WIDE), the fused final stage with `up2_shared_wgs` workgroups -- the other parts' kernels run beside them"""
        self.packs, self.S = packs, len(packs)
        self.frame_invariant, self.shares_gpu = frame_invariant, shares_gpu
        self.feat_is_bf16 = False      # set_inputs: the features came as 16-bit planes, no ingest pass
        self.debug_bits = None         # tests: a list that receives the hard masks every stage pools with (eager runs only)
        self.on_first_pool = None      # multi-part callers skew their parts by one phase: called behind the first stage's pooling
        self.B, self.N, self.H, self.W, self.HW = B, N, H, W, H * W
        self.mode = mode_of(prec)
        self.prec, self.out_dtype = self.mode.feat, out_dtype           # `prec`: the feature planes' code (ingest / pool)
        if any(p.prec != self.mode.query for p in packs):
            raise _lib.PolyheadError(f"stage packs are not packed for mode '{self.mode.name}'")
        # the launch geometry -- the pooling's pixel split, whether the stage-boundary conv also pools (ph_dynconv_poolx) and
        # whether the final stage is conv + x2 upsample in one kernel (ph_dynconv_up2) -- is the library's choice: the rule and the
        # measurements behind its thresholds live in resolve() of csrc/ph_decode.hip, the same call a native plan is built from
        L = packs[0].num_classes
        self.cfg = native_cfg(B, N, H, W, self.S, L, packs[0].lay.ffn_dim, self.mode, out_dtype, frame_invariant, shares_gpu, nsplit)
        geo = _lib.DecodeGeometry()
        if _lib.load().ph_decode_geometry_of(C.byref(self.cfg), C.byref(geo)) != 0:
            raise _cfg_error("ph_decode_geometry_of")
        self.nsplit, self.nsplit_px, self.poolx, self.fused_up = geo.nsplit, geo.nsplit_px, bool(geo.poolx), bool(geo.fused_up)
        dev = torch.device(device)
        P, KP = self.mode.FP, self.mode.KP
        Npad, HWp = n_padded(N), hw_padded(self.HW)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        # static inputs (graph-capturable)
        self.x = e((B, 256, H, W), torch.float32)
        self.dfe = e((B, 256, H, W), torch.float32)
        self.k0 = e((B, N, 256), torch.float32)
        self.q0 = e((B, N, 256), torch.float32)
        self.m0 = e((B, N, H, W), torch.float32)
        # internals
        # (zero-filled when the planes carry pixel padding: 16-bit inputs are copied into them row by row and the kernels read whole
        # 128-pixel chunks -- a NaN bit pattern in the padding would survive the multiplication with a zero mask bit)
        z = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if HWp != self.HW else e
        self.xp = z((P, B, 256, HWp), torch.int16)
        self.dp = z((P, B, 256, HWp), torch.int16)
        self.bits = e((B, Npad, HWp // 32), torch.int32)
        self.partial = e((B, self.nsplit, Npad, 512), torch.float32)
        self.pcount = e((B, self.nsplit, Npad), torch.int32)      # the masks' pixel counts per pixel range, pool -> query kernel
        self.ws = e((_lib.load().ph_query_workspace_bytes(B, N, self.mode.query),), torch.uint8)
        self.stage_out = [dict(obj=e((B, N, 256), torch.float32), dobj=e((B, N, 256), torch.float32),
                               cls=e((B, N, L), torch.float32), kern=e((KP, 2, B, Npad, 256), torch.int16),
                               kbias=e((2, B, Npad), torch.float32)) for _ in range(self.S)]
        # outputs
        self.mask = e((B, N, H, W), out_dtype)
        self.depth = e((B, N, H, W), out_dtype)
        self.mask_up = e((B, N, 2 * H, 2 * W), out_dtype)
        self.depth_up = e((B, N, 2 * H, 2 * W), out_dtype)
        self.graph = None
        self.handoff_runs = 0          # runs that started from another kernel's planes (tests observe the path taken)
        self.want_depth_lowres = False     # the fused final stage writes the depth branch's low-resolution logits only on request
        # workgroups of the fused final stage when the plan is one part of a multi-stream step: 1.5 per CU (cfg.up2_wgs = n; stages())
        self.up2_shared_wgs = self.cfg.up2_wgs or \
            (3 * torch.cuda.get_device_properties(device).multi_processor_count // 2 if dev.type == "cuda" else 0)
        if self.poolx:
            self.partial_px = e((B, self.nsplit_px, Npad, 512), torch.float32)
            self.pcount_px = e((B, self.nsplit_px, Npad), torch.int32)
        # the depth halves of the last two stages' poolings from ONE read of depth_feats (ph_pool_depth_pair): the last stage's mask
        # bits, partial sums and counts get buffers of their own (the B set; the names above stay the A set).  Same bits either way
        self.pair = bool((POOL_PAIR if pair is None else pair) and self.poolx and self.S >= 3 and
                         _lib.load().ph_pool_depth_pair_supported(N, self.prec))
        if self.pair:
            self.bits_b, self.partial_px_b, self.pcount_px_b = (torch.empty_like(t) for t in (self.bits, self.partial_px, self.pcount_px))

    @property
    def out_code(self):
        return OUT_CODE[self.out_dtype]

    def renew_outputs(self):
        """Give the next `run` fresh output tensors (allocation only, no copy).  The reference's methods return tensors the
        caller owns (SURVEY 8b "Threading / ownership"): the module API calls this before every run, so that results kept
        from an earlier call -- e.g. the key frame's while the reference frame is decoded,
        polyphonic_former_video.py:208-242 -- are never overwritten.  Captured plans (bench) keep their fixed buffers."""
        if self.graph is not None:
            raise _lib.PolyheadError("renew_outputs on a captured plan")
        e = lambda t: torch.empty_like(t)
        self.mask, self.depth, self.mask_up, self.depth_up = e(self.mask), e(self.depth), e(self.mask_up), e(self.depth_up)
        last = self.stage_out[-1]
        for k in ("obj", "dobj", "cls"):
            last[k] = e(last[k])

    def set_inputs(self, x, dfe, k0, q0, m0):
        """x / dfe: fp32 NCHW (converted to planes by the ingest kernel inside `run`), or 16-bit NCHW tensors of the
        mode's own plane format (bf16 for 'bf16' / 'mixed', fp16 for 'fp16'), which ARE the plane format when H*W is
        a multiple of 128: they are adopted as they are and no ingest pass runs.  Other sizes (cfg5: 48 x 156): the rows are copied
        into the planes' first H*W pixels, the padding up to the next multiple of 128 stays zero (round 6)."""
        self.feat_is_bf16 = x.dtype in (torch.bfloat16, torch.float16) and dfe.dtype == x.dtype     # 16-bit plane inputs
        if self.feat_is_bf16:
            if self.mode.feat_dtype != x.dtype:
                raise _lib.PolyheadError(f"{x.dtype} feature inputs need a mode with that plane format (bf16: 'bf16' / "
                                         f"'mixed' / 'mixed16', fp16: 'fp16'; this plan: '{self.mode.name}')")
            self.xp.view(x.dtype)[0, :, :, :self.HW].copy_(x.reshape(self.B, 256, self.HW))
            self.dp.view(x.dtype)[0, :, :, :self.HW].copy_(dfe.reshape(self.B, 256, self.HW))
        else:
            self.x.copy_(x)
            self.dfe.copy_(dfe)
        self.k0.copy_(k0.reshape(self.B, self.N, 256))
        self.q0.copy_(q0.reshape(self.B, self.N, 256))   # materialises the stride-0 expand view
        if m0.dtype in OUT_CODE and self.m0.dtype != m0.dtype:
            # mask logits are binarised from the format they arrive in (16-bit: what a 16-bit KernelHead grade hands over and what
            # cfg2's bf16 inputs mean -- half the bytes; never a rounding of fp32 logits).  A captured graph holds the old buffer:
            # it is dropped, the owner captures again
            self.m0 = torch.empty_like(self.m0, dtype=m0.dtype)
            self.graph = None
        self.m0.copy_(m0)

    def ingest(self):
        if not self.feat_is_bf16:
            ingest(self.x, self.prec, out=self.xp)
            ingest(self.dfe, self.prec, out=self.dp)
        binarize(self.m0, out=self.bits)

    def stages(self, xp=None, dp=None):
        """the S stages on the plan's own planes, or on read-only planes another kernel produced; the mask bits are
        always the plan's own (they are rewritten by every non-final stage)"""
        xp = self.xp if xp is None else xp
        dp = self.dp if dp is None else dp
        k, q = self.k0, self.q0
        cv = self.mode.conv

        def query(s, part, bits, cnt, branches=0):
            return query_stage(part, bits, k, q, self.packs[s], self.N, self.HW, cls_sigmoid=s == self.S - 1,
                               outs=self.stage_out[s], workspace=self.ws, kern_fmt=self.mode.kern_fmt, counts=cnt,
                               phases=3 | (_lib.PH_QUERY_WIDE if self.shares_gpu else 0) | branches)

        for s in range(self.S):
            last = s == self.S - 1
            bits = self.bits_b if self.pair and last else self.bits
            if self.debug_bits is not None:      # tests: the hard masks stage s pools with (eager runs only)
                self.debug_bits.append(bits.clone())
            if self.pair and s == self.S - 2:
                # the depth branch never feeds the mask branch (kernel_update_head.py:250-288), so this stage's depth half waits until
                # its mask half and the conv behind it have written the LAST stage's masks: depth_feats is then read once for both
                # stages.  The mask half runs before anything has counted its masks' pixels: it counts the bit rows (same integers)
                o = query(s, self.partial_px, bits, None, _lib.PH_QUERY_MASK_ONLY)
                dynconv_poolx(xp, o["kern"], o["kbias"], self.N, self.HW, cv, self.bits_b, self.partial_px_b)
                pool_depth_pair(dp, bits, self.bits_b, self.N, self.HW, self.prec, self.partial_px, self.partial_px_b,
                                self.pcount_px, self.pcount_px_b)
                query(s, self.partial_px, bits, self.pcount_px, _lib.PH_QUERY_DEPTH_ONLY)
                k, q = o["obj"], o["dobj"]
                continue
            if self.pair and last:
                part, cnt = self.partial_px_b, self.pcount_px_b      # both halves are there
            elif s > 0 and self.poolx:
                # the x map's sums came with the previous stage's conv (same read of the plane): depth_feats alone here
                pool_depth_only(dp, bits, self.N, self.HW, self.prec, self.partial_px, self.pcount_px)
                part, cnt = self.partial_px, self.pcount_px
            else:
                pool(xp, dp, bits, self.N, self.HW, self.prec, self.nsplit, out=self.partial, counts=self.pcount)
                part, cnt = self.partial, self.pcount
            if s == 0 and self.on_first_pool is not None:
                self.on_first_pool()       # multi-part callers skew their parts by one phase (an event recorded here)
            o = query(s, part, bits, cnt)
            if not last:
                if self.poolx:
                    dynconv_poolx(xp, o["kern"], o["kbias"], self.N, self.HW, cv, self.bits, self.partial_px)
                else:
                    dynconv(xp, o["kern"], o["kbias"], 0, self.N, self.HW, cv, bits_out=self.bits)
            else:
                # each x2 upsample directly behind the conv that wrote its source (240 MB of logits at cfg2, 24 frames): on
                # its own a part's four launches take 659 us in this order against 823 us as conv, conv, up, up; inside the
                # four-stream step the other parts' streams evict the logits either way (same-box A/B: no difference)
                if self.fused_up:
                    # a part of a multi-stream step (`shares_gpu`): 1.5 workgroups per CU -- the other parts' query kernels hold CUs when
                    # this launch starts, and what cannot start at once leaves a shorter tail (+0.9 % on the step, profiles/r06/knob_sweep.txt)
                    wg = self.up2_shared_wgs if (self.shares_gpu and self.B * self.H >= 4 * self.up2_shared_wgs) else 0
                    dynconv_up2(xp, o["kern"], o["kbias"], 0, self.N, self.H, self.W, cv, self.mask_up, logits_out=self.mask,
                                out_dtype=self.out_code, workgroups=wg)
                    dynconv_up2(dp, o["kern"], o["kbias"], 1, self.N, self.H, self.W, cv, self.depth_up,
                                logits_out=self.depth if self.want_depth_lowres else None, out_dtype=self.out_code, workgroups=wg)
                else:
                    dynconv(xp, o["kern"], o["kbias"], 0, self.N, self.HW, cv, logits_out=self.mask, out_dtype=self.out_code)
                    upsample2x(self.mask, out=self.mask_up)
                    dynconv(dp, o["kern"], o["kbias"], 1, self.N, self.HW, cv, logits_out=self.depth, out_dtype=self.out_code)
                    upsample2x(self.depth, out=self.depth_up)
            k, q = o["obj"], o["dobj"]

    def run(self):
        """one pass: ingest + S stages + final upsample, on the current stream"""
        self.ingest()
        self.stages()

    def run_from_planes(self, xp, dp, bits, k0, q0):
        """same, starting from feature planes / mask bits another kernel already produced (KernelHead hand-off): no
        ingest pass.  The planes are only read; the bits are copied (0.6 MB per frame at cfg2) because the stages
        rewrite them, so the producer's tensors stay valid for its caller."""
        self.handoff_runs += 1
        self.bits.copy_(bits)
        self.k0.copy_(k0.reshape(self.B, self.N, 256))
        self.q0.copy_(q0.reshape(self.B, self.N, 256))
        self.stages(xp, dp)

    def capture(self):
        """record `run` into a HIP graph (replay with `replay`)"""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.run()      # warm-up outside capture (lazy module load, attribute setup)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.run()
        return self.graph

    def replay(self):
        self.graph.replay()

    def outputs(self):
        last = self.stage_out[-1]
        depth = self.depth if (not self.fused_up or self.want_depth_lowres) else None      # fused final stage: never written
        return dict(obj=last["obj"], dobj=last["dobj"], cls=last["cls"], mask=self.mask, depth=depth,
                    mask_up=self.mask_up, depth_up=self.depth_up)


# ---- the S-stage plan as a native object (include/polyhead.h ph_decode_*) -----------------------------------
def _gather_params(module, device, count, name_of, numel_of, slots=None):
    """the `count` parameters a device packer reads, by the names of its table (`name_of(i)`), as fp32 device tensors of
    `numel_of(i)` elements -> (the tensors, kept alive by the caller until the launch is queued; the host array of their pointers,
    `slots` long with NULL behind the parameters when the table has more entries than this cfg reads)"""
    sd = module.state_dict() if hasattr(module, "state_dict") else module
    params = []
    for i in range(count):
        name = name_of(i).decode()
        t = sd[name].detach().to(device=device, dtype=torch.float32).contiguous()
        if t.numel() != numel_of(i):
            raise _lib.PolyheadError(f"{name}: {t.numel()} elements, the cfg needs {numel_of(i)}")
        params.append(t)
    return params, (C.c_void_p * (slots or count))(*[t.data_ptr() for t in params])


def _pack_on_device(params_from, cfg, device, symbols, nparams, slots=None, name_takes_cfg=False):
    """the body of every native_*_pack* function: the `nparams` parameters of `params_from` (a module or a state_dict) packed on the
    current stream of `device` -> a new uint8 tensor.  `symbols`: the library's (pack bytes, parameter name, parameter numel, pack)"""
    lib, ref = _lib.load(), C.byref(cfg)
    bytes_fn, name_fn, numel_fn, pack_fn = (getattr(lib, s) for s in symbols)
    nbytes = bytes_fn(ref)
    if nbytes == 0:
        raise _cfg_error(symbols[0])
    name_of = (lambda i: name_fn(ref, i)) if name_takes_cfg else name_fn
    params, ptrs = _gather_params(params_from, device, nparams, name_of, lambda i: numel_fn(ref, i), slots)
    blob = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(pack_fn(ref, ptrs, _lib.ptr(blob), _lib.stream_ptr()), symbols[3])
    return blob


def _pack_piece(blob, layout, i, dtype, shape):
    """piece `i` of a pack layout as a view of the pack; None for an empty piece"""
    off, nb = int(layout.offset[i]), int(layout.bytes[i])
    return blob[off:off + nb].view(dtype).reshape(shape) if nb else None


# a1's / the neck's grade of a cfg's mode code (as KHEAD_PREC maps the names), and the mode's name
_GRADE_OF_MODE = {code: KHEAD_PREC[name] for name, code in _lib.PH_MODE.items()}
_MODE_NAME = {code: name for name, code in _lib.PH_MODE.items() if name != "split"}


class _NativePack:
    """the base of the four native packs: one device buffer packed by the library, its layout asked from the library,
    a copy of its cfg, `mode` / `prec` / `P`, and the views a family cuts from it in `_pieces(cfg)` with `piece`.  Per family:
    `_symbols`, the library's (pack bytes, parameter name, parameter numel, pack, pack layout); `_layout_type`; `_nparams(cfg)`;
    `_slots`, the length of the pointer table when it is longer than that"""
    _symbols, _layout_type, _slots, _name_takes_cfg = (), None, None, False

    def __init__(self, blob, cfg):
        lay = self._layout_type()
        _lib.check(getattr(_lib.load(), self._symbols[4])(C.byref(cfg), C.byref(lay)), self._symbols[4])
        self.blob, self.layout, self.cfg = blob, lay, type(cfg).from_buffer_copy(bytes(cfg))
        self.mode = getattr(cfg, "mode", None)                       # the track head's cfg carries its grade itself
        self.prec = cfg.prec if self.mode is None else _GRADE_OF_MODE[self.mode]
        self.P = 2 if self.prec == _lib.PH_PREC_SPLIT else 1
        self._pieces(cfg)

    def piece(self, i, dtype, shape):
        return _pack_piece(self.blob, self.layout, i, dtype, shape)

    @classmethod
    def pack_on_device(cls, module, cfg, device):
        """`module`'s parameters (a module or its state_dict) packed on the device by the family's packer -> the pack"""
        return cls(_pack_on_device(module, cfg, device, cls._symbols[:4], cls._nparams(cfg), cls._slots, cls._name_takes_cfg), cfg)


class _OwnsHandles:
    """the Python owner of native plans: its handle `_h`, or the values of `_handles`, are destroyed by the library's
    `_destroy_symbol` when the object goes -- if the library is still loaded"""
    _destroy_symbol = None

    def _destroy(self):
        for h in list(getattr(self, "_handles", {}).values()) + [getattr(self, "_h", None)]:
            if h is not None and h.value and _lib._lib is not None:
                getattr(_lib._lib, self._destroy_symbol)(h)
        self._handles, self._h = {}, None

    __del__ = _destroy


def _on(dev):
    """the device context of a plan's library calls (the CU count the library asks for is the current device's); none off the GPU"""
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


class _NativePlan(_OwnsHandles):
    """the base of the native plans over `self.cfg`, `self.device` and `self.workspace`.  Per family: `_symbols`, the
    library's (workspace bytes, create, info); `_geometry_type`; `_destroy_symbol`; `_zeroed`, the workspace's contract"""
    _symbols, _geometry_type, _zeroed = (), None, False

    def _alloc_workspace(self):
        """the workspace of `self.cfg`, or the library's words about the cfg"""
        with _on(self.device):
            nbytes = getattr(_lib.load(), self._symbols[0])(C.byref(self.cfg))
            if nbytes == 0:
                raise _cfg_error(self._symbols[0])
            self.workspace = (torch.zeros if self._zeroed else torch.empty)((nbytes,), dtype=torch.uint8, device=self.device)

    def _create(self, pack, **fields):
        """a native plan of `self.cfg`, these fields replaced, over `pack` (a pointer, or an array of them) and the workspace"""
        cfg = type(self.cfg).from_buffer_copy(bytes(self.cfg))
        for k, v in fields.items():
            setattr(cfg, k, int(v))
        h = C.c_void_p()
        with _on(self.device):
            _lib.check(getattr(_lib.load(), self._symbols[1])(C.byref(cfg), pack, _lib.ptr(self.workspace), self.workspace.numel(),
                                                             C.byref(h)), self._symbols[1])
        return h

    def _handle_of(self, **fields):
        """the plan of these cfg fields, created on first use: the plans of one object share its workspace -- a run uses one of them"""
        key = tuple(fields.values())
        if key not in self._handles:
            self._handles[key] = self._create(_lib.ptr(self.pack.blob), **fields)
        return self._handles[key]

    def _info(self, h):
        geo = self._geometry_type()
        _lib.check(getattr(_lib.load(), self._symbols[2])(h, C.byref(geo)), self._symbols[2])
        return geo


def _fan_out_towers(streams, device, tower):
    """the four level towers side by side: streams[l] (made here on first use) waits for the current stream and runs `tower(l)`,
    the longest chains first, and the current stream waits for all four.  -> the streams"""
    if streams is None:
        streams = [torch.cuda.Stream(device=device) for _ in range(4)]
    cur = torch.cuda.current_stream()
    for lvl in (0, 3, 2, 1):
        streams[lvl].wait_stream(cur)
        with torch.cuda.stream(streams[lvl]):
            tower(lvl)
    for st in streams:
        cur.wait_stream(st)
    return streams


def native_pack_stage(module, cfg, device):
    """one KernelUpdateHead stage's parameters packed on the device by ph_decode_pack_stage -> uint8 tensor (one pack)"""
    return _pack_on_device(module, cfg, device, ("ph_decode_pack_bytes", "ph_decode_param_name", "ph_decode_param_numel",
                                                 "ph_decode_pack_stage"), _lib.PH_DECODE_NPARAMS)


def native_pack_from(pack, cfg):
    """a StagePack (pack.py's planes + vectors) laid out as one native pack; its layout must be the native one"""
    lib = _lib.load()
    lay, off = _lib.StageLayout(), C.c_size_t()
    _lib.check(lib.ph_decode_pack_layout(C.byref(cfg), C.byref(lay), C.byref(off)), "ph_decode_pack_layout")
    if bytes(lay) != bytes(pack.lay):
        raise _lib.PolyheadError("the StagePack's layout differs from the native pack layout of this cfg")
    blob = torch.zeros((lib.ph_decode_pack_bytes(C.byref(cfg)),), dtype=torch.uint8, device=pack.wb.device)
    wb = pack.wb.contiguous().view(torch.uint8).reshape(-1)
    wf = pack.wf.contiguous().view(torch.uint8).reshape(-1)
    blob[:wb.numel()].copy_(wb)
    blob[off.value:off.value + wf.numel()].copy_(wf)
    return blob


class NativeDecodePlan(_NativePlan):
    """DecodePlan's surface (set_inputs, run, run_from_planes, renew_outputs, outputs, capture / replay) over ONE native call per
    decode (ph_decode_run): the same launch sequence and geometry as the DecodePlan of the same arguments, so the same bits.
    `packs`: StagePacks (re-laid out as native packs once) or native packs (`native_pack_stage`)."""
    _symbols, _geometry_type, _destroy_symbol = ("ph_decode_workspace_bytes", "ph_decode_create", "ph_decode_info"), _lib.DecodeGeometry, \
        "ph_decode_destroy"

    def __init__(self, packs, B, N, H, W, prec, out_dtype=torch.float32, device="cuda:0", nsplit=None, frame_invariant=False,
                 shares_gpu=False, num_classes=None, ffn_dim=None):
        self.S, self.B, self.N, self.H, self.W, self.HW = len(packs), B, N, H, W, H * W
        self.mode = mode_of(prec)
        self.prec, self.out_dtype, self.frame_invariant, self.shares_gpu = self.mode.feat, out_dtype, frame_invariant, shares_gpu
        dev = torch.device(device)
        self.device = dev
        if all(isinstance(p, StagePack) for p in packs):
            if any(p.prec != self.mode.query for p in packs):
                raise _lib.PolyheadError(f"stage packs are not packed for mode '{self.mode.name}'")
            L, F = packs[0].num_classes, packs[0].lay.ffn_dim
        else:
            L, F = num_classes, ffn_dim
        self.cfg = native_cfg(B, N, H, W, self.S, L, F, self.mode, out_dtype, frame_invariant, shares_gpu, nsplit)
        self._alloc_workspace()
        self.packs = [native_pack_from(p, self.cfg) if isinstance(p, StagePack) else p for p in packs]
        self._h = self._create((C.c_void_p * self.S)(*[p.data_ptr() for p in self.packs]))
        self.geometry = geo = self._info(self._h)
        self.nsplit, self.nsplit_px, self.poolx, self.fused_up = geo.nsplit, geo.nsplit_px, bool(geo.poolx), bool(geo.fused_up)
        Npad, HWp = n_padded(N), hw_padded(self.HW)
        # shapes of the plan's planes and bits (they live in the workspace): what the module API compares a KernelHead hand-off with
        self.xp = torch.empty((self.mode.FP, B, 256, HWp), dtype=torch.int16, device="meta")
        self.bits = torch.empty((B, Npad, HWp // 32), dtype=torch.int32, device="meta")
        self.want_depth_lowres = False
        self.graph = None
        self.handoff_runs = 0
        self._in = None
        self.io = _lib.DecodeIO()
        self._alloc_outputs()

    @property
    def out_code(self):
        return OUT_CODE[self.out_dtype]

    def _alloc_outputs(self):
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        B, N, H, W = self.B, self.N, self.H, self.W
        self.obj, self.dobj = e((B, N, 256), torch.float32), e((B, N, 256), torch.float32)
        self.cls = e((B, N, self.cfg.L), torch.float32)
        self.mask, self.mask_up, self.depth_up = e((B, N, H, W), self.out_dtype), e((B, N, 2 * H, 2 * W), self.out_dtype), \
            e((B, N, 2 * H, 2 * W), self.out_dtype)
        self.depth = e((B, N, H, W), self.out_dtype) if (not self.fused_up or self.want_depth_lowres) else None
        io = self.io
        io.obj, io.dobj, io.cls = self.obj.data_ptr(), self.dobj.data_ptr(), self.cls.data_ptr()
        io.mask, io.mask_up, io.depth_up = self.mask.data_ptr(), self.mask_up.data_ptr(), self.depth_up.data_ptr()

    def renew_outputs(self):
        """fresh output tensors for the next `run` (DecodePlan.renew_outputs)"""
        if self.graph is not None:
            raise _lib.PolyheadError("renew_outputs on a captured plan")
        self._alloc_outputs()

    def set_inputs(self, x, dfe, k0, q0, m0):
        """as DecodePlan.set_inputs: fp32 NCHW features, or 16-bit NCHW in the mode's plane format.  Eager plans read the given
        tensors in place (no copy); a captured plan copies them into the tensors its graph reads."""
        B, N = self.B, self.N
        f16 = x.dtype in (torch.bfloat16, torch.float16) and dfe.dtype == x.dtype
        if f16 and self.mode.feat_dtype != x.dtype:
            raise _lib.PolyheadError(f"{x.dtype} feature inputs need a mode with that plane format (bf16: 'bf16' / "
                                     f"'mixed' / 'mixed16', fp16: 'fp16'; this plan: '{self.mode.name}')")
        for t, nm, numel in ((x, "x", B * 256 * self.HW), (dfe, "depth_feats", B * 256 * self.HW), (k0, "proposal_feats", B * N * 256),
                             (q0, "depth_proposal", None), (m0, "mask_preds", B * N * self.HW)):
            _require_gpu(t, nm)
            if numel is not None and t.numel() != numel:
                raise _lib.PolyheadError(f"{nm}: {tuple(t.shape)} does not fit the plan (B={B}, N={N}, H={self.H}, W={self.W})")
        cast = (lambda t: t.contiguous()) if f16 else (lambda t: t.float().contiguous())
        new = dict(x=cast(x), dfe=cast(dfe), k0=k0.reshape(B, N, 256).float().contiguous(),
                   q0=q0.reshape(B, N, 256).float().contiguous(),      # materialises the stride-0 expand view
                   m0=m0.contiguous() if m0.dtype in OUT_CODE else m0.float().contiguous())
        if self.graph is not None and self._in is not None and self._in.get("feat") == 1 and all(
                self._in[k].dtype == v.dtype for k, v in new.items()):
            for k, v in new.items():
                self._in[k].copy_(v)
            return
        self.graph = None           # a captured graph read other tensors: the owner captures again
        self._in = dict(new, feat=1)
        self._point_inputs(_lib.PH_FEAT_16 if f16 else _lib.PH_FEAT_F32)

    def _point_inputs(self, feat_format, bits=None):
        i, io = self._in, self.io
        io.feat_format = feat_format
        io.x, io.depth_feats, io.k0, io.q0 = i["x"].data_ptr(), i["dfe"].data_ptr(), i["k0"].data_ptr(), i["q0"].data_ptr()
        io.m0 = None if bits is not None else i["m0"].data_ptr()
        io.m0_dtype = OUT_CODE.get(i["m0"].dtype, _lib.PH_OUT_F32) if bits is None else _lib.PH_OUT_F32
        io.bits = None if bits is None else bits.data_ptr()

    def run(self):
        """one pass: ingest + S stages + final stage, ONE native call on the current stream"""
        io = self.io
        if (not self.fused_up or self.want_depth_lowres) and self.depth is None:
            self.depth = torch.empty((self.B, self.N, self.H, self.W), dtype=self.out_dtype, device=self.device)
        io.depth = self.depth.data_ptr() if (not self.fused_up or self.want_depth_lowres) else None
        _lib.check(_lib.load().ph_decode_run(self._h, C.byref(io), _lib.stream_ptr()), "ph_decode_run")

    def run_from_planes(self, xp, dp, bits, k0, q0):
        """DecodePlan.run_from_planes: planes and mask bits another kernel produced (read only; the bits are copied)"""
        if tuple(xp.shape) != tuple(self.xp.shape) or tuple(dp.shape) != tuple(self.xp.shape) or tuple(bits.shape) != tuple(self.bits.shape):
            raise _lib.PolyheadError("run_from_planes: planes / bits of another geometry")
        self.handoff_runs += 1
        B, N = self.B, self.N
        self.graph = None
        self._in = dict(x=xp.contiguous(), dfe=dp.contiguous(), k0=k0.reshape(B, N, 256).float().contiguous(),
                        q0=q0.reshape(B, N, 256).float().contiguous(), m0=None, bits=bits.contiguous())
        self._point_inputs(_lib.PH_FEAT_PLANES, bits=self._in["bits"])
        self.run()

    def capture(self):
        """record `run` into a HIP graph (replay with `replay`); the inputs of the last `set_inputs` become plan-owned copies"""
        if self._in is None or self._in.get("feat") != 1:
            raise _lib.PolyheadError("capture needs set_inputs first")
        ff = self.io.feat_format
        self._in = dict({k: v.clone() for k, v in self._in.items() if k != "feat"}, feat=1)
        self._point_inputs(ff)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.run()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.run()
        self.graph = g
        return g

    def replay(self):
        self.graph.replay()

    def outputs(self):
        depth = self.depth if (not self.fused_up or self.want_depth_lowres) else None
        return dict(obj=self.obj, dobj=self.dobj, cls=self.cls, mask=self.mask, depth=depth, mask_up=self.mask_up,
                    depth_up=self.depth_up)


# ---- KernelHead (a1) ---------------------------------------------------------------------------------
def _planes_of(w64, P, fp16=False):
    """float64 [..] -> int16 [P, ...] bf16 hi(/lo) planes, or ONE fp16 plane"""
    w = w64.to(torch.float32)
    if fp16:
        return w.to(torch.float16).view(torch.int16)[None].contiguous()
    hi = w.to(torch.bfloat16)
    out = [hi.view(torch.int16)]
    if P == 2:
        out.append((w - hi.float()).to(torch.bfloat16).view(torch.int16))
    return torch.stack(out, 0).contiguous()


def _pad_rows32(w):
    r = (-w.shape[0]) % 32
    return torch.cat([w, w.new_zeros((r,) + tuple(w.shape[1:]))], 0) if r else w


class KernelHeadPack:
    """device-resident packed parameters of KernelHead's post-neck part (kernel_head.py:142-211)"""

    def __init__(self, sd, prec, device, groups):
        P = 2 if prec == _lib.PH_PREC_SPLIT else 1
        h = prec == _lib.PH_PREC_F16                                         # one fp16 plane of every weight
        g = lambda k: sd[k].detach().to("cpu", torch.float64)
        convs = torch.stack([g(f"{n}_convs.0.conv.weight").reshape(256, 256) for n in ("loc", "seg", "depth")], 0)
        self.wplanes = _planes_of(convs, P, h).to(device)                    # [P,3,256,256]
        self.gn = torch.stack([torch.stack([g(f"{n}_convs.0.gn.weight"), g(f"{n}_convs.0.gn.bias")], 0)
                               for n in ("loc", "seg", "depth")], 0).float().contiguous().to(device)   # [3,2,256]
        w_init = g("init_kernels.weight").reshape(-1, 256)
        w_seg = g("conv_seg.weight").reshape(-1, 256)
        w_dd = g("conv_direct_depth.weight").reshape(1, 256)
        self.n_init, self.n_seg = w_init.shape[0], w_seg.shape[0]
        self.init_planes = _planes_of(_pad_rows32(w_init), P, h).to(device)
        self.seg_planes = _planes_of(_pad_rows32(w_seg), P, h).to(device)
        self.dd_planes = _planes_of(_pad_rows32(w_dd), P, h).to(device)
        z = lambda n: torch.zeros(n, dtype=torch.float32)
        sb = z(self.seg_planes.shape[1]); sb[:self.n_seg] = g("conv_seg.bias").float()
        self.seg_bias = sb.to(device)
        db = z(32); db[0] = float(g("conv_direct_depth.bias")[0])
        self.dd_bias = db.to(device)
        # the same three weights as MFMA A fragments for the fused second GEMM of ph_khead_fused
        from .pack import pack_b32
        frag = lambda pl: torch.stack([pack_b32(pl[p].cpu()) for p in range(P)], 0).contiguous().to(device)
        self.init_frag, self.seg_frag, self.dd_frag = frag(self.init_planes), frag(self.seg_planes), frag(self.dd_planes)
        # the three conv weights in the same fragment form: the A operand of ph_khead_onepass (one-plane grades)
        self.conv_frag = torch.stack([pack_b32(self.wplanes[0, m].cpu()) for m in range(3)], 0).contiguous().to(device) if P == 1 else None
        self.w_init_f32 = w_init.float().contiguous().to(device)
        self.w_seg_f32 = w_seg.float().contiguous().to(device)
        self.w_dd_f32 = sd["conv_direct_depth.weight"].detach().float().contiguous().to(device)   # [1,256,1,1]
        self.prec, self.groups = prec, groups


class _KernelHeadPlanBase:
    """what the two KernelHead plans share: everything `KernelHead.simple_test_rpn` hands to its caller (the 9-tuple and the plane /
    bit hand-off to KernelUpdateIterHead), and the three input maps.  A subclass sets B, H, W, HW and N, then calls `_alloc_io`."""

    def _alloc_io(self, P, n_seg, want_f32, logit_dtype, device, dense_depth_proposal=False):
        B, H, W, N, HWp = self.B, self.H, self.W, self.N, hw_padded(self.HW)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        self.f = [None, None, None]        # set_inputs: borrowed from the caller or allocated on first copy
        self._borrowed = set()
        self.in_planes = False
        self.xp, self.dp = e((P, B, 256, HWp), torch.int16), e((P, B, 256, HWp), torch.int16)
        self.x_f32 = e((B, 256, H, W), torch.float32) if want_f32 else None
        self.dfe_f32 = e((B, 256, H, W), torch.float32) if want_f32 else None
        self.mask_preds = e((B, N, H, W), logit_dtype)
        self.seg_preds = e((B, n_seg, H, W), logit_dtype)
        self.depth_pred = e((B, 1, H, W), logit_dtype)
        self.bits = e((B, n_padded(N), HWp // 32), torch.int32)
        self.proposal = e((B, N, 256), torch.float32)
        self.depth_proposal = e((B, N, 256), torch.float32) if dense_depth_proposal else None

    def renew_outputs(self):
        """fresh tensors for everything `KernelHead.simple_test_rpn` hands to its caller (the 9-tuple and the plane / bit
        hand-off to KernelUpdateIterHead), see DecodePlan.renew_outputs"""
        e = lambda t: None if t is None else torch.empty_like(t)
        self.xp, self.dp, self.bits = e(self.xp), e(self.dp), e(self.bits)
        self.x_f32, self.dfe_f32 = e(self.x_f32), e(self.dfe_f32)
        self.mask_preds, self.seg_preds, self.depth_pred = e(self.mask_preds), e(self.seg_preds), e(self.depth_pred)
        self.proposal, self.depth_proposal = e(self.proposal), e(self.depth_proposal)

    def set_inputs(self, feats):
        """the three post-neck maps: contiguous fp32 device tensors of the plan's shape are used where they are (the
        kernels only read them; a captured graph keeps pointing at them, so they stay referenced here), anything
        else is copied into the plan's own buffers"""
        self.in_planes = feats[0].dtype == torch.int16
        if self.in_planes:          # bf16 planes [P][B][256][HWp] from the neck (SemanticFPNWrapper.forward_planes)
            for i, src in enumerate(feats):
                if tuple(src.shape) != tuple(self.xp.shape) or not src.is_contiguous():
                    raise _lib.PolyheadError("plane inputs must be contiguous int16 [P][B][256][HWp]")
                self.f[i] = src
            self._borrowed = {t.data_ptr() for t in self.f}
            return
        for i, src in enumerate(feats):
            if (src.dtype == torch.float32 and src.is_contiguous() and src.device == self.xp.device
                    and tuple(src.shape) == (self.B, 256, self.H, self.W)):
                self.f[i] = src.detach()
            else:
                if self.f[i] is None or self.f[i].data_ptr() in self._borrowed:
                    self.f[i] = torch.empty((self.B, 256, self.H, self.W), dtype=torch.float32, device=self.xp.device)
                self.f[i].copy_(src)
        self._borrowed = {t.data_ptr() for t, src in zip(self.f, feats) if t.data_ptr() == src.data_ptr()}

    def check_status(self):
        """kept for callers of round 3's API: returns `timeouts()`; nothing to raise any more, results are valid either way"""
        return self.timeouts()


class KernelHeadPlan(_KernelHeadPlanBase):
    """buffers + launch sequence of KernelHead's post-neck part for one (B, H, W)."""

    def __init__(self, pack, B, H, W, num_thing_classes, num_classes, cat_stuff, device, want_f32=True, nsplit=None,
                 logit_dtype=torch.float32, onepass=None, frame_invariant=False):
        """`onepass`: None = ph_khead_onepass whenever the geometry / grade allows it (and native_khead_cfg's switch is unset),
        True = the same, an error where it cannot run, False = always the two-pass ph_khead_fused.  `logit_dtype`: fp32 (the
        reference API) or fp16 (one-pass form only) for mask_preds / seg_preds / depth_pred."""
        self.pack, self.B, self.H, self.W, self.HW = pack, B, H, W, H * W
        self.n_thing_cls, self.n_cls, self.cat_stuff = num_thing_classes, num_classes, cat_stuff
        self.Nq = pack.n_init
        self.n_stuff = (num_classes - num_thing_classes) if cat_stuff else 0
        self.N = self.Nq + self.n_stuff
        prec = pack.prec
        dev = torch.device(device)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        lib = _lib.load()
        # one pass or two and the pooling's pixel split are the library's choice: the rule lives in resolve() of
        # csrc/ph_kheadplan.hip, the same call a native plan is built from (it asks the current device for its CU count)
        self.cfg = native_khead_cfg(B, H, W, pack.n_init, pack.n_seg, num_thing_classes, cat_stuff, pack.groups, prec, logit_dtype,
                                    want_f32, frame_invariant, onepass, nsplit)
        geo = _lib.KheadGeometry()
        with torch.cuda.device(dev):
            if lib.ph_khead_geometry_of(C.byref(self.cfg), C.byref(geo)) != 0:
                raise _cfg_error("ph_khead_geometry_of")
        self.onepass, self.nsplit = bool(geo.onepass), geo.nsplit
        if self.onepass and pack.conv_frag is None:
            raise _lib.PolyheadError("ph_khead_onepass needs the pack's conv fragments (a one-plane grade)")
        self.logit_dtype = logit_dtype
        self.ws1 = None
        if self.onepass:
            # hand-off state of the persistent launch; zeroed ONCE (its last 256 bytes are the sticky time-out words, which the
            # calls never clear)
            self.ws1 = torch.zeros((lib.ph_khead_onepass_workspace_bytes(B, self.HW),), dtype=torch.uint8, device=dev)
        self._alloc_io(2 if prec == _lib.PH_PREC_SPLIT else 1, pack.n_seg, want_f32, logit_dtype, dev)
        self.partial = e((B, self.nsplit, n_padded(self.Nq), 512), torch.float32)
        # the two-pass kernels' workspace: the path itself, or the in-call fallback of a one-pass launch that gave up
        self.ws = e((lib.ph_khead_workspace_bytes(B, self.HW, pack.groups),), torch.uint8)
        self.w_stuff = pack.w_seg_f32[num_thing_classes:num_classes].contiguous() if self.n_stuff else None

    def run(self):
        lib, pk, s = _lib.load(), self.pack, _lib.stream_ptr
        B, HW, prec = self.B, self.HW, pk.prec
        fmt = _lib.PH_IN_PLANES if self.in_planes else _lib.PH_IN_F32_NCHW
        if self.onepass:
            # one read of the three maps: conv1x1+GN+ReLU x3, x = sem + loc, the static 1x1 convs AND the mask bits
            # (kernel_head.py:250-331, :314-317) in one persistent launch; the object pooling reads the thing rows of
            # the full bit tensor in place
            _lib.check(lib.ph_khead_onepass(_lib.ptr(self.f[0]), _lib.ptr(self.f[1]), _lib.ptr(self.f[2]), _lib.ptr(pk.conv_frag),
                                            _lib.ptr(pk.gn), pk.groups, 1e-5, _lib.ptr(pk.init_frag), self.Nq,
                                            _lib.ptr(pk.seg_frag), _lib.ptr(pk.seg_bias), pk.n_seg, _lib.ptr(pk.dd_frag),
                                            _lib.ptr(pk.dd_bias), self.n_thing_cls, self.n_stuff, _lib.ptr(self.xp), _lib.ptr(self.dp),
                                            _lib.ptr(self.x_f32), _lib.ptr(self.dfe_f32), _lib.ptr(self.mask_preds),
                                            _lib.ptr(self.seg_preds), _lib.ptr(self.depth_pred), OUT_CODE[self.logit_dtype],
                                            _lib.ptr(self.bits), self.bits.shape[1], _lib.ptr(self.ws1), self.ws1.numel(),
                                            B, HW, prec, fmt, s()), "ph_khead_onepass")
            # the in-call fallback: the two-pass kernels and the binarisation, PREDICATED on the one-pass launch's status word
            # (first word of ws1).  The persistent grid needs a workgroup resident on every CU; when another kernel holds CUs
            # beyond the hand-off bound the launch gives up, raises that word, and these launches -- which otherwise return at
            # once -- rewrite every output of the call.  No host round trip, valid under graph capture and replay.
            _lib.check(lib.ph_khead_fused_if(_lib.ptr(self.f[0]), _lib.ptr(self.f[1]), _lib.ptr(self.f[2]), _lib.ptr(pk.wplanes),
                                             _lib.ptr(pk.gn), pk.groups, 1e-5, _lib.ptr(pk.init_frag), self.Nq,
                                             _lib.ptr(pk.seg_frag), _lib.ptr(pk.seg_bias), pk.n_seg, _lib.ptr(pk.dd_frag),
                                             _lib.ptr(pk.dd_bias), self.n_thing_cls, self.n_stuff, _lib.ptr(self.xp), _lib.ptr(self.dp),
                                             _lib.ptr(self.x_f32), _lib.ptr(self.dfe_f32), _lib.ptr(self.mask_preds),
                                             _lib.ptr(self.seg_preds), _lib.ptr(self.depth_pred), OUT_CODE[self.logit_dtype],
                                             _lib.ptr(self.ws1), _lib.ptr(self.ws), self.ws.numel(), B, HW, prec, fmt, s()),
                       "ph_khead_fused_if")
            _lib.check(lib.ph_binarize_if(_lib.ptr(self.mask_preds), OUT_CODE[self.logit_dtype], 0, _lib.ptr(self.bits), B, self.N, HW,
                                          _lib.ptr(self.ws1), s()), "ph_binarize_if")
        else:
            # conv1x1+GN+ReLU x3, x = sem + loc, and the static 1x1 convs on the normalised tiles (kernel_head.py:250-331):
            # init_kernels(loc) -> thing rows of mask_preds (:256), conv_seg(sem) -> seg_preds (:295) and its stuff rows ->
            # the remaining rows of mask_preds (:329-331), conv_direct_depth(dfe) -> depth_pred (:285)
            _lib.check(lib.ph_khead_fused(_lib.ptr(self.f[0]), _lib.ptr(self.f[1]), _lib.ptr(self.f[2]), _lib.ptr(pk.wplanes),
                                          _lib.ptr(pk.gn), pk.groups, 1e-5, _lib.ptr(pk.init_frag), self.Nq,
                                          _lib.ptr(pk.seg_frag), _lib.ptr(pk.seg_bias), pk.n_seg, _lib.ptr(pk.dd_frag),
                                          _lib.ptr(pk.dd_bias), self.n_thing_cls, self.n_stuff, _lib.ptr(self.xp), _lib.ptr(self.dp),
                                          _lib.ptr(self.x_f32), _lib.ptr(self.dfe_f32), _lib.ptr(self.mask_preds),
                                          _lib.ptr(self.seg_preds), _lib.ptr(self.depth_pred), _lib.ptr(self.ws), self.ws.numel(),
                                          B, HW, prec, fmt, s()), "ph_khead_fused")
            # object features: binarise the logits once (all rows: the decode stages start from these bits), pool x over the
            # THING rows (:314-320)
            _lib.check(lib.ph_binarize(_lib.ptr(self.mask_preds), 0, _lib.ptr(self.bits), B, self.N, HW, s()), "ph_binarize")
        self._finish_run(lib, pk, s, B, HW, prec)

    def _finish_run(self, lib, pk, s, B, HW, prec):
        # object features: pool x over the THING rows of the bit tensor (:314-320), add them to the kernels (:324-326)
        _lib.check(lib.ph_pool_rows(_lib.ptr(self.xp), None, _lib.ptr(self.bits), self.bits.shape[1], _lib.ptr(self.partial),
                                    B, self.Nq, HW, self.nsplit, prec, s()), "ph_pool_rows")
        _lib.check(lib.ph_khead_proposals(_lib.ptr(self.partial), self.nsplit, _lib.ptr(pk.w_init_f32),
                                          _lib.ptr(self.w_stuff),
                                          _lib.ptr(self.proposal), B, self.Nq, self.n_stuff, s()), "ph_khead_proposals")

    def timeouts(self):
        """one-pass form: number of workgroup time-outs since the plan was built (sticky across calls and graph replays;
        synchronises the stream).  A time-out costs the affected call its one-pass speed -- the predicated two-pass fallback
        inside `run` produces its results -- never the results."""
        if not self.onepass:
            return 0
        return int(_lib.load().ph_khead_onepass_timeouts(_lib.ptr(self.ws1), self.B, self.HW, _lib.stream_ptr()))

    def last_run_fell_back(self):
        """one-pass form: True if the most recent run gave up and was redone by the two-pass kernels (synchronises)"""
        return bool(self.onepass and _lib.load().ph_khead_onepass_status(_lib.ptr(self.ws1), self.B, _lib.stream_ptr()) != 0)


# ---- KernelHead's post-neck part as a native object (include/polyhead.h ph_khead_cfg .. ph_khead_plan_timeouts) ------------
_KHEAD_MODE_OF_PREC = {_lib.PH_PREC_F16: "fp16", _lib.PH_PREC_BF16: "bf16", _lib.PH_PREC_SPLIT: "fp32"}


def native_khead_cfg(B, H, W, num_proposals, num_classes, num_thing_classes, cat_stuff, groups, prec, logit_dtype=torch.float32,
                     want_f32=True, frame_invariant=False, onepass=None, nsplit=None):
    """the ph_khead_cfg of an a1 plan, Python or native.  KernelHead's variables (knobs.py: PH_KHEAD_TWOPASS, PH_POOL_NSPLIT) are
    read here, through knobs.get, at every call, and become the cfg's explicit fields.  KernelHeadPlan asks the library for its
    geometry with it (ph_khead_geometry_of), NativeKernelHeadPlan creates its plan from it, so the two agree by construction.
    `prec`: a precision name (engine.KHEAD_PREC's keys) or a1's grade code; `num_classes`: the rows of conv_seg"""
    name = prec if isinstance(prec, str) else _KHEAD_MODE_OF_PREC[prec]
    twopass = knobs.get("PH_KHEAD_TWOPASS")
    if onepass and twopass:
        raise _lib.PolyheadError("ph_khead_onepass asked for while PH_KHEAD_TWOPASS is set")
    if logit_dtype not in (torch.float32, torch.float16):
        raise _lib.PolyheadError("KernelHead logits are fp32 or fp16")
    return _lib.KheadCfg(B=B, H=H, W=W, num_proposals=num_proposals, num_classes=num_classes, num_thing_classes=num_thing_classes,
                         cat_stuff=int(bool(cat_stuff)), groups=groups, mode=_lib.PH_MODE[name], logit_dtype=OUT_CODE[logit_dtype],
                         emit_f32=int(bool(want_f32)), frame_invariant=int(bool(frame_invariant)),
                         onepass=_knob_code(onepass is False or twopass, onepass, _lib.PH_KNOB_ON),
                         nsplit=int(nsplit or knobs.get("PH_POOL_NSPLIT") or 0))


class NativeKernelHeadPack(_NativePack):
    """one device buffer packed by ph_khead_pack, and its pieces as views under KernelHeadPack's attribute names (so either plan
    -- KernelHeadPlan or NativeKernelHeadPlan -- runs from it)"""
    _symbols = ("ph_khead_pack_bytes", "ph_khead_param_name", "ph_khead_param_numel", "ph_khead_pack", "ph_khead_pack_layout")
    _layout_type, _nparams = _lib.KheadLayout, staticmethod(lambda cfg: _lib.PH_KHEAD_NPARAMS)

    def _pieces(self, cfg):
        self.groups, self.n_init, self.n_seg = cfg.groups, cfg.num_proposals, cfg.num_classes
        P = self.P
        dt = dict(wplanes=(torch.int16, (P, 3, 256, 256)), gn=(torch.float32, (3, 2, 256)),
                  init_planes=(torch.int16, (P, n_padded(self.n_init), 256)), seg_planes=(torch.int16, (P, n_padded(self.n_seg), 256)),
                  dd_planes=(torch.int16, (P, 32, 256)), seg_bias=(torch.float32, (n_padded(self.n_seg),)), dd_bias=(torch.float32, (32,)),
                  init_frag=(torch.int16, (P, n_padded(self.n_init) * 256)), seg_frag=(torch.int16, (P, n_padded(self.n_seg) * 256)),
                  dd_frag=(torch.int16, (P, 32 * 256)), conv_frag=(torch.int16, (3, 256 * 256)),
                  w_init_f32=(torch.float32, (self.n_init, 256)), w_seg_f32=(torch.float32, (self.n_seg, 256)),
                  w_dd_f32=(torch.float32, (1, 256, 1, 1)))
        for i, name in enumerate(_lib.KPACK_PIECES):
            setattr(self, name, self.piece(i, *dt[name]))


def native_khead_pack(module, cfg, device):
    """KernelHead's own parameters (a module, or a state_dict without the neck's entries) packed on the device by ph_khead_pack"""
    return NativeKernelHeadPack.pack_on_device(module, cfg, device)


class NativeKernelHeadPlan(_KernelHeadPlanBase, _NativePlan):
    """KernelHeadPlan's surface (_KernelHeadPlanBase, run, timeouts, last_run_fell_back and the output attributes) over ONE
    native call per a1 (ph_khead_plan_run): the same launch sequence and geometry as the KernelHeadPlan of the same arguments, so
    the same bits.  `pack`: a NativeKernelHeadPack.  `dense_depth_proposal`: also write depth_proposal [B, N, 256] (what a C caller
    hands to ph_decode_io.q0; the module API keeps the reference's stride-0 view of the weight and needs no launch for it)."""
    _symbols, _geometry_type, _destroy_symbol = ("ph_khead_plan_workspace_bytes", "ph_khead_plan_create", "ph_khead_plan_info"), \
        _lib.KheadGeometry, "ph_khead_plan_destroy"
    _zeroed = True      # ONCE: the one-pass launch's hand-off state ends in the sticky time-out words, which no call clears

    def __init__(self, pack, B, H, W, num_thing_classes, num_classes, cat_stuff, device, want_f32=True, nsplit=None,
                 logit_dtype=torch.float32, onepass=None, frame_invariant=False, dense_depth_proposal=False, cfg=None):
        """`cfg`: a ph_khead_cfg to use as it is (no PH_* variable is then consulted) instead of `native_khead_cfg`'s"""
        if num_classes != pack.n_seg:
            raise _lib.PolyheadError("the native KernelHead plan needs num_classes == rows of conv_seg (a sigmoid loss_seg)")
        self.pack, self.B, self.H, self.W, self.HW = pack, B, H, W, H * W
        dev = torch.device(device)
        self.device, self.logit_dtype, self.want_f32 = dev, logit_dtype, want_f32
        self.cfg = cfg if cfg is not None else native_khead_cfg(B, H, W, pack.n_init, pack.n_seg, num_thing_classes, cat_stuff,
                                                                pack.groups, _MODE_NAME[pack.mode], logit_dtype, want_f32, frame_invariant, onepass, nsplit)
        self._alloc_workspace()
        self._h = self._create(_lib.ptr(pack.blob))
        self.geometry = geo = self._info(self._h)
        self.onepass, self.nsplit, self.N, self.n_stuff = bool(geo.onepass), geo.nsplit, geo.N, geo.n_stuff
        self.Nq = pack.n_init
        self.dense_depth_proposal = dense_depth_proposal
        self.io = _lib.KheadIO()
        self._alloc_io(geo.P, pack.n_seg, want_f32, logit_dtype, dev, dense_depth_proposal)

    def run(self):
        """one a1 call on the current stream: ONE native call"""
        io, dp = self.io, lambda t: None if t is None else t.data_ptr()
        io.input_format = _lib.PH_IN_PLANES if self.in_planes else _lib.PH_IN_F32_NCHW
        io.f0, io.f1, io.f2 = self.f[0].data_ptr(), self.f[1].data_ptr(), self.f[2].data_ptr()
        io.xp, io.dp, io.bits, io.x_f32, io.dfe_f32 = dp(self.xp), dp(self.dp), dp(self.bits), dp(self.x_f32), dp(self.dfe_f32)
        io.mask_preds, io.seg_preds, io.depth_pred = dp(self.mask_preds), dp(self.seg_preds), dp(self.depth_pred)
        io.proposal, io.depth_proposal = dp(self.proposal), dp(self.depth_proposal)
        _lib.check(_lib.load().ph_khead_plan_run(self._h, C.byref(io), _lib.stream_ptr()), "ph_khead_plan_run")

    def timeouts(self):
        """workgroup time-outs of the one-pass launches since the plan was built (KernelHeadPlan.timeouts; synchronises)"""
        return int(_lib.load().ph_khead_plan_timeouts(self._h, _lib.stream_ptr()))

    def last_run_fell_back(self):
        """True if the most recent run gave up its one-pass launch and was redone by the two-pass kernels (synchronises)"""
        return bool(_lib.load().ph_khead_plan_status(self._h, _lib.stream_ptr()) != 0)


# ---- SemanticFPNWrapper (N3) -------------------------------------------------------------------------------
def nhwc_ingest(x, add, prec, out):
    B, Cc, H, W = x.shape
    lib = _lib.load()
    _lib.check(lib.ph_nhwc_ingest(_lib.ptr(x), _lib.ptr(add), _lib.ptr(out), B, H * W, prec, _lib.stream_ptr()), "ph_nhwc_ingest")
    return out


def conv_nhwc(xp, pk, y, partial, B, H, W, prec):
    lib = _lib.load()
    _lib.check(lib.ph_conv_nhwc(_lib.ptr(xp), _lib.ptr(pk["wp"]), pk["wp"].shape[1], _lib.ptr(y), _lib.ptr(partial), pk["k"],
                                pk["s"], B, H, W, prec, _lib.stream_ptr()), "ph_conv_nhwc")


def gn_finalize(partial, stats, nwg, groups, HW, B, eps=1e-5):
    lib = _lib.load()
    _lib.check(lib.ph_gn_finalize(_lib.ptr(partial), _lib.ptr(stats), nwg, groups, HW, eps, B, _lib.stream_ptr()), "ph_gn_finalize")


def gn_apply(y, stats, pk, groups, mode, B, H, W, prec, planes=None, outf=None, accumulate=False):
    lib = _lib.load()
    _lib.check(lib.ph_gn_apply(_lib.ptr(y), _lib.ptr(stats), _lib.ptr(pk["gamma"]) if pk else None,
                               _lib.ptr(pk["beta"]) if pk else None, groups, mode, 1 if accumulate else 0, _lib.ptr(planes),
                               _lib.ptr(outf), B, H, W, prec, _lib.stream_ptr()), "ph_gn_apply")


def gn_sum_planes(ys, stats, pks, groups, planes, B, HW, prec):
    lib = _lib.load()
    n = len(ys)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    _lib.check(lib.ph_gn_sum_planes(arr(ys), arr(stats), arr([p["gamma"] for p in pks]), arr([p["beta"] for p in pks]), n, groups,
                                    _lib.ptr(planes), B, HW, prec, _lib.stream_ptr()), "ph_gn_sum_planes")


def neck_out_convs(planes, channels_last, wplanes, gn_affine, groups, out_planes, out_f32, ws, B, HW, prec, eps=1e-5):
    """conv_pred + 2 aux convs (1x1 conv + GN + ReLU each) of the level sum `planes` ([P,B,HW,256] when channels_last, else channel
    planes [P,B,256,HWp]); out_planes / out_f32: lists of 3 (None: not wanted)"""
    lib = _lib.load()
    op = out_planes if out_planes is not None else [None] * 3
    of = out_f32 if out_f32 is not None else [None] * 3
    _lib.check(lib.ph_neck_out_convs(_lib.ptr(planes), 1 if channels_last else 0, _lib.ptr(wplanes), _lib.ptr(gn_affine), groups, eps,
                                     _lib.ptr(op[0]), _lib.ptr(op[1]), _lib.ptr(op[2]), _lib.ptr(of[0]), _lib.ptr(of[1]), _lib.ptr(of[2]),
                                     _lib.ptr(ws), ws.numel() * ws.element_size(), B, HW, prec, _lib.stream_ptr()), "ph_neck_out_convs")


class NeckPlan:
    """buffers + launch sequence of SemanticFPNWrapper.forward for one (B, level shapes): channels-last bf16 planes
    between the convs, fp32 channels-last conv outputs (one per level for the fused level sum), three fp32 NCHW outputs"""

    def __init__(self, B, shapes, prec, device, tower_streams=True, groups=32, num_outs=3):
        self.B, self.shapes, self.prec, self.groups, self.num_outs = B, shapes, prec, groups, num_outs
        P = 2 if prec == _lib.PH_PREC_SPLIT else 1
        dev = torch.device(device)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        lib = _lib.load()
        # the tower-stream form, the fused output stage and level 0's plane layout are the library's choice, and so is the check of
        # the level sizes (a stride-2 pyramid whose levels 2 and 3 reach the stride-8 size by x2 upsampling): the rule lives in
        # resolve() of csrc/ph_neckplan.hip, the same call a native plan is built from
        self.cfg = native_neck_cfg(B, shapes, groups, prec, num_outs, tower_streams=tower_streams, device_type=dev.type)
        geo = _lib.NeckGeometry()
        if lib.ph_neck_geometry_of(C.byref(self.cfg), C.byref(geo)) != 0:
            raise _cfg_error("ph_neck_geometry_of")
        self.Ho, self.Wo = geo.Ho, geo.Wo                          # stride-8 output size
        big = max(h * w for h, w in shapes)
        self.xa = e((P, B, big, 256), torch.int16)                 # conv input planes (ping)
        self.xb = e((P, B, self.Ho * self.Wo, 256), torch.int16)   # conv input planes (pong, <= output size)
        self.ys = [e((B, self.Ho * self.Wo, 256), torch.float32) for _ in range(4)]   # last conv output of each level
        self.y = e((B, self.Ho * self.Wo, 256), torch.float32)     # other conv outputs (pre-norm)
        self.partial = e((lib.ph_conv_nhwc_partial_floats(B, self.Ho, self.Wo),), torch.float32)
        self.lstats = [e((B, 256, 2), torch.float32) for _ in range(4)]
        self.stats = e((B, 256, 2), torch.float32)
        self.outs = [e((B, 256, self.Ho, self.Wo), torch.float32) for _ in range(3)]
        self.pouts = None                                          # plane outputs, allocated on first use
        # Round 3: the four level towers are independent until the level sum and the small ones leave most of the chip idle
        # (a 3x3 conv at 16 x 32 x 16 frames is 32 workgroups): each tower gets its own buffers and its own HIP stream, the
        # small launches run beside the stride-4 level's ingest + stride-2 conv (native_neck_cfg says when)
        self.multi = bool(geo.tower_buffers)
        self.lv = None
        if self.multi:
            self.lv = []
            for lvl, (h, w) in enumerate(shapes):
                # the towers of levels 2 and 3 upsample up to the output size between their convs; levels 0 and 1 are a single conv
                n_small = self.Ho * self.Wo if lvl >= 2 else 1
                self.lv.append(dict(xa=e((P, B, max(h * w, n_small), 256), torch.int16), xb=e((P, B, n_small, 256), torch.int16),   # ping / pong
                                    y=e((B, n_small, 256), torch.float32), stats=e((B, 256, 2), torch.float32),
                                    partial=e((lib.ph_conv_nhwc_partial_floats(B, self.Ho, self.Wo),), torch.float32)))
        self._streams = None                                       # created on first use; not part of a copy of the plan
        self.skip_ingest = False                                   # set around a capture whose replays follow `ingest_frames`
        # Round 4: the three output convs (conv_pred + 2 aux convs) as stats / apply passes over the level sum in channel planes
        # (ph_neck_out_convs) instead of conv -> fp32 NHWC -> finalize -> apply per map.  Three maps, 32 groups and one-plane grades
        # only: with hi / lo planes the recompute pass is three MFMAs per product and costs more than the fp32 round trip it removes
        # (whole head 19.1 -> 20.4 ms per 16 frames at the parity grade, same box)
        self.out2 = bool(geo.fused_out)
        self.ws2 = e((lib.ph_neck_out_convs_workspace_bytes(B, self.Ho * self.Wo, 32) // 4 + 64,), torch.float32) if self.out2 else None
        # a level that starts with the stride-2 conv (level 0) hands it chunk-major planes (PH_PLANES_C16: the kernel's 16-channel
        # stages then read whole lines; else channels-last); one-plane grades
        self.c16 = _lib.PH_PLANES_C16 if geo.c16 else 0

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_streams"] = None               # HIP streams cannot be copied / pickled (copy.deepcopy of a module that holds a plan)
        return d

    def _conv_gn(self, xp, pk, H, W, groups, y, stats, partial=None, layout=0):
        """conv + statistics; returns the conv output size"""
        B, prec = self.B, self.prec | layout
        partial = self.partial if partial is None else partial
        k, s = pk["k"], pk["s"]
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        conv_nhwc(xp, pk, y, partial, B, H, W, prec)
        nwg = _lib.load().ph_conv_nhwc_workgroups_b(k, s, Ho, Wo, prec, B)
        gn_finalize(partial, stats, nwg, groups, Ho * Wo, B)
        return Ho, Wo

    def _tower(self, lvl, feat, pk, groups, posenc, bufs):
        """one level: ingest -> (conv + GN + ReLU + x2 upsample)* -> last conv (its GroupNorm is applied by the level sum)"""
        B, prec = self.B, self.prec
        H, W = self.shapes[lvl]
        xa, xb, y, stats, partial = bufs["xa"], bufs["xb"], bufs["y"], bufs["stats"], bufs["partial"]
        convs = pk["levels"][lvl]
        c16 = self.c16 if (convs[0]["s"] == 2 and convs[0]["k"] == 3) else 0      # the plan's layout into a stride-2 3x3 first conv
        if not self.skip_ingest:
            nhwc_ingest(feat, posenc, prec | c16, xa)
        src = xa
        for j, c in enumerate(convs):
            lay = c16 if j == 0 else 0
            if j + 1 < len(convs):      # every non-final conv of levels 2 and 3 is followed by an x2 upsample
                H, W = self._conv_gn(src, c, H, W, groups, y, stats, partial, lay)
                dst = xb if src is xa else xa
                gn_apply(y, stats, c, groups, _lib.PH_GN_UP2_PLANES, B, H, W, prec, planes=dst)
                H, W, src = 2 * H, 2 * W, dst
            else:
                H, W = self._conv_gn(src, c, H, W, groups, self.ys[lvl], self.lstats[lvl], partial, lay)
                if (H, W) != (self.Ho, self.Wo):
                    raise _lib.PolyheadError("level does not end at the stride-8 size")

    def can_ingest_frames(self):
        """True when the levels' conv input planes can be filled frame by frame AHEAD of `run` (`ingest_frames`): every level owns its
        buffers (the tower-stream form) and the grade has one plane"""
        return bool(self.multi) and self.prec != _lib.PH_PREC_SPLIT

    def ingest_frames(self, frames, pk, posenc, pos_level):
        """round 6 (video clips without the staging copy): the ingest step of `run` for `frames` = B one-frame level tuples (fp32
        [1, 256, h, w], contiguous), each written straight from the caller's tensor into its slice of the level's conv input planes -- on the
        CURRENT stream, outside any graph.  A `run(..)` with `skip_ingest` set (the captured graph) continues from those planes."""
        if not self.can_ingest_frames() or len(frames) != self.B:
            raise _lib.PolyheadError("NeckPlan.ingest_frames: needs the tower-stream form, a one-plane grade and B frames")
        lib, st = _lib.load(), _lib.stream_ptr()
        for lvl, (h, w) in enumerate(self.shapes):
            convs = pk["levels"][lvl]
            c16 = self.c16 if (convs[0]["s"] == 2 and convs[0]["k"] == 3) else 0
            xa = self.lv[lvl]["xa"]
            add = _lib.ptr(posenc) if lvl == pos_level and posenc is not None else None
            for b, f in enumerate(frames):
                t = f[lvl]
                if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (1, 256, h, w) or t.device != xa.device:
                    raise _lib.PolyheadError("NeckPlan.ingest_frames: fp32 contiguous [1, 256, h, w] device tensors")
                _lib.check(lib.ph_nhwc_ingest(_lib.ptr(t), add, C.c_void_p(xa.data_ptr() + b * h * w * 256 * 2), 1, h * w, self.prec | c16, st),
                           "ph_nhwc_ingest(frame)")

    def _check_pk(self, pk, groups):
        if len(pk["outs"]) != self.num_outs or groups != self.groups:
            raise _lib.PolyheadError(f"NeckPlan.run: the plan was built for {self.num_outs} output convs and {self.groups} groups, "
                                     f"not {len(pk['outs'])} and {groups}")

    # ---- a level started from planes (FpnPlan.run's `neck`): the producer writes `level_input` -- positional encoding included --
    # and the tower runs without its ingest.  Shared buffers (`multi` False): the four levels share `xa`, so a level's planes are
    # written and its `run_level_planes` issued before the next level's are written; `multi`: every level owns its `xa` and
    # `run_towers_planes` runs the four towers on their streams
    def level_input(self, lvl, pk, to_planes=False):
        """(the level's conv input planes, the `prec` value -- grade | layout -- their writer uses)"""
        c0 = pk["levels"][lvl][0]
        c16 = self.c16 if (c0["s"] == 2 and c0["k"] == 3) else 0
        return (self.lv[lvl]["xa"] if self.multi else self.xa), self.prec | c16

    def _from_planes(self, fn):
        saved, self.skip_ingest = self.skip_ingest, True
        try:
            fn()
        finally:
            self.skip_ingest = saved

    def run_level_planes(self, lvl, pk, groups, to_planes=False):
        self._check_pk(pk, groups)
        bufs = self.lv[lvl] if self.multi else dict(xa=self.xa, xb=self.xb, y=self.y, stats=self.stats, partial=self.partial)
        self._from_planes(lambda: self._tower(lvl, None, pk, groups, None, bufs))

    def run_towers_planes(self, pk, groups, to_planes=False):
        self._check_pk(pk, groups)
        self._from_planes(lambda: self._towers([None] * 4, pk, groups, None, -1))

    def run(self, feats, pk, groups, posenc, pos_level, to_planes=False):
        self._check_pk(pk, groups)
        self._towers(feats, pk, groups, posenc, pos_level)
        return self.run_outputs(pk, groups, to_planes)

    def _towers(self, feats, pk, groups, posenc, pos_level):
        if self.multi:
            self._streams = _fan_out_towers(self._streams, self.xa.device, lambda lvl: self._tower(
                lvl, feats[lvl], pk, groups, posenc if lvl == pos_level else None, self.lv[lvl]))
        else:
            shared = dict(xa=self.xa, xb=self.xb, y=self.y, stats=self.stats, partial=self.partial)
            for lvl in range(4):
                self._tower(lvl, feats[lvl], pk, groups, posenc if lvl == pos_level else None, shared)

    def run_outputs(self, pk, groups, to_planes=False, posenc=None):
        """the level sum and conv_pred / the aux convs, behind the four towers"""
        B, prec = self.B, self.prec
        if to_planes and self.pouts is None:
            P = 2 if prec == _lib.PH_PREC_SPLIT else 1
            self.pouts = [torch.empty((P, B, 256, hw_padded(self.Ho * self.Wo)), dtype=torch.int16, device=self.xa.device)
                          for _ in range(3)]
        # sum over levels of ReLU(GN(.)) straight to conv input planes (channels-last)
        gn_sum_planes(self.ys, self.lstats, [pk["levels"][l][-1] for l in range(4)], groups, self.xb, B, self.Ho * self.Wo, prec)
        if self.out2:
            # statistics pass (three maps in one launch) + finalize + one apply launch per map
            neck_out_convs(self.xb, True, pk["outs_w"], pk["outs_gn"], groups,
                           self.pouts if to_planes else None, None if to_planes else self.outs, self.ws2, B, self.Ho * self.Wo, prec)
            return self.pouts if to_planes else self.outs
        # conv_pred / aux convs -> fp32 NCHW
        for i, c in enumerate(pk["outs"]):
            self._conv_gn(self.xb, c, self.Ho, self.Wo, groups, self.y, self.stats)
            if to_planes:       # bf16 channel planes, the decode path's feature format (KernelHead hand-off)
                gn_apply(self.y, self.stats, c, groups, _lib.PH_GN_TO_CPLANES, B, self.Ho, self.Wo, prec, planes=self.pouts[i])
            else:
                gn_apply(self.y, self.stats, c, groups, _lib.PH_GN_TO_NCHW, B, self.Ho, self.Wo, prec, outf=self.outs[i])
        return (self.pouts if to_planes else self.outs)[:len(pk["outs"])]


# ---- FPN (mmdet/models/necks/fpn.py:151-203): backbone stages -> the four pyramid levels ------------------------------------
def fpn_lateral(x, wp, bias, coarse, coarse_hw, out, prec):
    """one level's 1x1 lateral conv + nearest top-down add: x [B, K, H, W] (fp32 / bf16 / fp16, contiguous) -> 16-bit NHWC planes
    `out` [P, B, H*W, 256]; coarse: the next coarser level's planes [P, B, Hc*Wc, 256] with coarse_hw = (Hc, Wc), or None"""
    B, K, H, W = x.shape
    Hc, Wc = coarse_hw if coarse is not None else (0, 0)
    lib = _lib.load()
    _lib.check(lib.ph_fpn_lateral(_lib.ptr(x), OUT_CODE[x.dtype], _lib.ptr(wp), wp.shape[1], _lib.ptr(bias), _lib.ptr(coarse), Hc, Wc,
                                  _lib.ptr(out), B, K, H, W, prec, _lib.stream_ptr()), "ph_fpn_lateral")
    return out


def fpn_lateral_cl(x, x_prec, hw, wp, bias, coarse, coarse_hw, out, prec):
    """`fpn_lateral` for a stage that is a channels-last 16-bit plane: x int16 [B, H*W, K] of grade `x_prec` with hw = (H, W); the
    other arguments are fpn_lateral's, `prec` PH_PREC_BF16 / PH_PREC_F16.  The bits of fpn_lateral on cl_to_nchw's tensor of x"""
    B, HW, K = x.shape
    H, W = hw
    if H * W != HW:
        raise _lib.PolyheadError("fpn_lateral_cl: x must be [B, H*W, K]")
    Hc, Wc = coarse_hw if coarse is not None else (0, 0)
    _lib.check(_lib.load().ph_fpn_lateral_cl(_lib.ptr(x), x_prec, _lib.ptr(wp), wp.shape[1], _lib.ptr(bias), _lib.ptr(coarse), Hc, Wc,
                                             _lib.ptr(out), B, K, H, W, prec, _lib.stream_ptr()), "ph_fpn_lateral_cl")
    return out


def fpn_output(y, bias, out, B, HW):
    """fp32 NHWC conv result [B, HW, 256] + bias -> fp32 NCHW `out`"""
    _lib.check(_lib.load().ph_fpn_output(_lib.ptr(y), _lib.ptr(bias), _lib.ptr(out), B, HW, _lib.stream_ptr()), "ph_fpn_output")
    return out


def fpn_output_planes(y, bias, add, planes, out_f32, B, HW, prec):
    """fp32 NHWC conv result [B, HW, 256] + bias (+ add [256, HW], or None) -> the neck's conv input `planes` (a tensor or a device
    address; `prec`: the grade, | PH_PLANES_C16 for chunk-major planes) and, `out_f32` given, the fp32 NCHW level as well"""
    pp = planes if isinstance(planes, C.c_void_p) else _lib.ptr(planes)
    _lib.check(_lib.load().ph_fpn_output_planes(_lib.ptr(y), _lib.ptr(bias), _lib.ptr(add), pp, _lib.ptr(out_f32), B, HW, prec,
                                                _lib.stream_ptr()), "ph_fpn_output_planes")


class NeckHandoff:
    """FpnPlan.run's `neck`: a neck plan (NeckPlan or NativeNeckPlan) with the arguments of its run.  `FpnPlan.run(.., neck=this)`
    writes the levels into the plan's conv input planes (and, shared buffers, runs each level's tower); `finish()` runs what is left
    -- the four towers of the tower-buffer form, the level sum and the output convs -- and returns the neck's outputs"""

    def __init__(self, plan, pk, groups, posenc, pos_level, to_planes=False):
        self.plan, self.pk, self.groups, self.to_planes = plan, pk, groups, to_planes
        self.posenc = posenc
        self.pos_level = -1 if (posenc is None or pos_level is None) else pos_level
        if posenc is not None and (posenc.dtype != torch.float32 or not posenc.is_contiguous() or
                                   tuple(posenc.shape) != (256,) + tuple(plan.shapes[self.pos_level])):
            raise _lib.PolyheadError("NeckHandoff: posenc must be fp32 contiguous [256, h, w] of pos_level")

    def finish(self):
        if self.plan.multi:
            self.plan.run_towers_planes(self.pk, self.groups, self.to_planes)
        return self.plan.run_outputs(self.pk, self.groups, self.to_planes, posenc=self.posenc)


class FpnPlan:
    """buffers + launch sequence of fpn.FPN.forward for one (B, level shapes, input channels): the four lateral sums as 16-bit
    channels-last planes, one fp32 channels-last conv output, the four fp32 NCHW levels.  `run` issues everything on the current
    stream -- one stream only, so a captured graph of it has no parallel branches -- and neither allocates nor synchronises; the
    outputs are the plan's buffers and are overwritten by the next call, as NeckPlan's are."""

    def __init__(self, B, shapes, in_channels, prec, device):
        if len(shapes) != 4 or len(in_channels) != 4:
            raise _lib.PolyheadError("FpnPlan: four levels")
        self.B, self.shapes, self.in_channels, self.prec = B, tuple(tuple(s) for s in shapes), tuple(in_channels), prec
        P = 2 if prec == _lib.PH_PREC_SPLIT else 1
        dev = torch.device(device)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        lib = _lib.load()
        self.lat = [e((P, B, h * w, 256), torch.int16) for h, w in self.shapes]
        big = max(h * w for h, w in self.shapes)
        self.y = e((B, big, 256), torch.float32)
        self.partial = e((max(lib.ph_conv_nhwc_partial_floats(B, h, w) for h, w in self.shapes),), torch.float32)   # the conv's GN sums: unused
        self.outs = [e((B, 256, h, w), torch.float32) for h, w in self.shapes]
        self.stages_f32 = None                    # the hi + lo grade's NCHW stages of a StagePlanes input, allocated when first needed

    def _laterals_cl(self, sp, pk):
        """the four laterals from a StagePlanes: ph_fpn_lateral_cl in the one-plane grades; the hi + lo grade converts each plane to a
        plan-owned fp32 NCHW stage (ph_cl_to_nchw: exact) and runs ph_fpn_lateral on it"""
        B, prec = self.B, self.prec
        if len(sp) != 4 or sp.B != B or sp.device != self.y.device or \
                tuple(sp.shapes) != tuple((k,) + hw for k, hw in zip(self.in_channels, self.shapes)):
            raise _lib.PolyheadError(f"FpnPlan.run: the StagePlanes must hold {B} frames of the plan's four stages "
                                     f"{[(k,) + hw for k, hw in zip(self.in_channels, self.shapes)]} on its device")
        split = prec == _lib.PH_PREC_SPLIT
        if split and self.stages_f32 is None:
            self.stages_f32 = [torch.empty((B, k) + hw, dtype=torch.float32, device=self.y.device)
                               for k, hw in zip(self.in_channels, self.shapes)]
        for lvl in (3, 2, 1, 0):
            c, (h, w) = pk["lateral"][lvl], self.shapes[lvl]
            coarse, chw = (self.lat[lvl + 1], self.shapes[lvl + 1]) if lvl < 3 else (None, None)
            if split:
                cl_to_nchw(sp.planes[lvl], self.stages_f32[lvl], B, h * w, self.in_channels[lvl], sp.prec)
                fpn_lateral(self.stages_f32[lvl], c["wp"], c["bias"], coarse, chw, self.lat[lvl], prec)
            else:
                fpn_lateral_cl(sp.planes[lvl], sp.prec, (h, w), c["wp"], c["bias"], coarse, chw, self.lat[lvl], prec)

    def run(self, feats, pk, neck=None, want_levels=True):
        """feats: the four backbone stages [B, K_l, H_l, W_l], or a StagePlanes (the backbone's own channels-last planes: the laterals
        read them directly, everything behind the laterals is the same); pk: fpn.FPN's pack (lateral / output: lists of dicts).
        neck: a NeckHandoff -- the direct hand-over: each output conv's tail (ph_fpn_output_planes) writes the neck plan's conv input
        planes of that level, positional encoding included, instead of the fp32 level that the neck would ingest; the fp32 levels are
        written as well when `want_levels`.  Shared neck buffers: the level's tower runs before the next level is written; tower
        buffers: the four inputs are written and `neck.finish()` runs the towers.  Either way `neck.finish()` returns the neck's
        outputs, bit for bit those of the neck plan's `run` on this plan's levels."""
        B, prec = self.B, self.prec
        if neck is not None and (neck.plan.B != B or tuple(tuple(x) for x in neck.plan.shapes) != self.shapes or neck.plan.prec != prec):
            raise _lib.PolyheadError("FpnPlan.run: the neck plan's frames, level sizes or grade differ from this plan's")
        if isinstance(feats, StagePlanes):
            self._laterals_cl(feats, pk)
        else:
            for lvl, t in enumerate(feats):
                if tuple(t.shape) != (B, self.in_channels[lvl]) + self.shapes[lvl] or t.dtype not in OUT_CODE or not t.is_contiguous() \
                        or t.device != self.y.device:
                    raise _lib.PolyheadError(f"FpnPlan.run: inputs[{lvl}] must be a contiguous fp32 / bf16 / fp16 device tensor of shape "
                                             f"{(B, self.in_channels[lvl]) + self.shapes[lvl]}")
            for lvl in (3, 2, 1, 0):                  # coarse to fine: each lateral adds the finished one above it
                c = pk["lateral"][lvl]
                fpn_lateral(feats[lvl], c["wp"], c["bias"], self.lat[lvl + 1] if lvl < 3 else None,
                            self.shapes[lvl + 1] if lvl < 3 else None, self.lat[lvl], prec)
        for lvl, (h, w) in enumerate(self.shapes):
            c = pk["output"][lvl]
            conv_nhwc(self.lat[lvl], c, self.y, self.partial, B, h, w, prec)
            if neck is None:
                fpn_output(self.y, c["bias"], self.outs[lvl], B, h * w)
                continue
            xa, layout = neck.plan.level_input(lvl, neck.pk, neck.to_planes)
            fpn_output_planes(self.y, c["bias"], neck.posenc if lvl == neck.pos_level else None, xa,
                              self.outs[lvl] if want_levels else None, B, h * w, layout)
            if not neck.plan.multi:
                neck.plan.run_level_planes(lvl, neck.pk, neck.groups, neck.to_planes)
        return self.outs


# ---- the neck as a native object (include/polyhead.h ph_neck_cfg .. ph_neck_plan_run_outputs) ------------------------------
def native_neck_cfg(B, shapes, groups, prec, num_outs=3, pos_level=3, to_planes=False, tower_streams=True, fused_out=None, c16=None,
                    device_type="cuda"):
    """the ph_neck_cfg of a neck plan, Python or native.  The neck's variables (knobs.py: PH_NECK_OUT2=0, PH_NECK_C16=0,
    PH_NECK_STREAMS) are read here, through knobs.get, at every call, and become the cfg's explicit fields.  NeckPlan asks the
    library for its geometry with it (ph_neck_geometry_of), NativeNeckPlan creates its plan from it, so the two agree by construction.
    `prec`: a precision name (engine.KHEAD_PREC's keys) or the grade code; `shapes`: the four level sizes; `pos_level`: None / -1 for
    no positional encoding; `fused_out` / `c16`: None = the variable's choice, else True (fused_out only) / False"""
    name = prec if isinstance(prec, str) else _KHEAD_MODE_OF_PREC[prec]
    out2 = knobs.get("PH_NECK_OUT2")
    if out2 in ("2", "3"):
        raise _lib.PolyheadError("PH_NECK_OUT2=2 / 3: these measurement forms of the neck's output stage were removed (both were slower)")
    if fused_out and out2 == "0":
        raise _lib.PolyheadError("ph_neck_out_convs asked for while PH_NECK_OUT2=0 is set")
    fo = _knob_code(fused_out is False or out2 == "0", fused_out, _lib.PH_KNOB_ON)
    cc = _lib.PH_KNOB_OFF if (c16 is False or knobs.get("PH_NECK_C16") == "0") else _lib.PH_KNOB_AUTO      # a field without an "on"
    # the four level towers with their own buffers, each on its own stream (NeckPlan.__init__): from 4 frames per call -- one frame
    # at a time (the video loop) is bound by the host's launch rate, where the stream switches cost more than the overlap returns
    # (cfg4 7.95 -> 9.08 ms per two frames with tower streams).  PH_NECK_STREAMS=0 or the module attribute `tower_streams = False`:
    # one stream, shared buffers (needed when TWO pipelines are captured into one HIP graph: the nested fork / join of 2 x 4 streams
    # made hipStreamEndCapture segfault on ROCm 7.2); PH_NECK_STREAMS=2 or tower_streams = "always": at any B
    ns = knobs.get("PH_NECK_STREAMS")
    multi = bool(tower_streams) and (B >= 4 or ns == "2" or tower_streams == "always") and ns != "0" and device_type == "cuda"
    if len(shapes) != 4:
        raise _lib.PolyheadError("the neck takes four FPN levels")
    return _lib.NeckCfg(B=B, h=(C.c_int32 * 4)(*[int(x[0]) for x in shapes]), w=(C.c_int32 * 4)(*[int(x[1]) for x in shapes]),
                        groups=groups, mode=_lib.PH_MODE[name], num_outs=num_outs, pos_level=-1 if pos_level is None else pos_level,
                        emit_planes=int(bool(to_planes)), emit_f32=int(not to_planes), fused_out=fo, c16=cc, tower_buffers=int(multi))


class NativeNeckPack(_NativePack):
    """one device buffer packed by ph_neck_pack, and its pieces as views in the form of SemanticFPNWrapper._pack's dict (`pk`: so
    either plan -- NeckPlan or NativeNeckPlan -- runs from it)"""
    _symbols = ("ph_neck_pack_bytes", "ph_neck_param_name", "ph_neck_param_numel", "ph_neck_pack", "ph_neck_pack_layout")
    _layout_type, _nparams = _lib.NeckLayout, staticmethod(lambda cfg: 3 * (7 + cfg.num_outs))
    _slots = _lib.PH_NECK_NPARAMS                                  # absent aux convs: NULL

    def _pieces(self, cfg):
        self.groups, self.num_outs = cfg.groups, cfg.num_outs
        P, piece = self.P, self.piece

        def one(c):
            k = 3 if c < 7 else 1
            return dict(wp=piece(3 * c, torch.int16, (P, 256 * k * k * 256)), gamma=piece(3 * c + 1, torch.float32, (256,)),
                        beta=piece(3 * c + 2, torch.float32, (256,)), k=k, s=2 if c == 0 else 1)
        self.pk = dict(levels=[[one(0)], [one(1)], [one(2), one(3)], [one(4), one(5), one(6)]],
                       outs=[one(7 + i) for i in range(cfg.num_outs)])
        if cfg.num_outs == 3:
            self.pk["outs_w"] = piece(_lib.PH_NPACK_OUTS_W, torch.int16, (P, 3, 256, 256))
            self.pk["outs_gn"] = piece(_lib.PH_NPACK_OUTS_GN, torch.float32, (3, 2, 256))


def native_neck_pack(module, cfg, device):
    """the neck's parameters (a SemanticFPNWrapper, or its state_dict) packed on the device by ph_neck_pack"""
    return NativeNeckPack.pack_on_device(module, cfg, device)


def native_neck_posenc(H, W, num_feats, temperature=10000, scale=2 * math.pi, eps=1e-6, device="cuda:0"):
    """ph_neck_posenc: the sine positional encoding evaluated in fp64 on the device -> fp32 [2 * num_feats, H, W]"""
    out = torch.empty((2 * num_feats, H, W), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().ph_neck_posenc(H, W, num_feats, float(temperature), float(scale), float(eps), _lib.ptr(out),
                                              _lib.stream_ptr()), "ph_neck_posenc")
    return out


class NativeNeckPlan(_NativePlan):
    """NeckPlan's `run` surface over the native plan: ONE native call per forward (ph_neck_plan_run), or -- where NeckPlan would put
    the four level towers on their own streams -- ph_neck_plan_run_level on the same four streams and ph_neck_plan_run_outputs
    behind them; the same launch sequence and geometry as the NeckPlan of the same arguments, so the same bits.  `pack`: a
    NativeNeckPack.  `cfg`: a ph_neck_cfg to use as it is (no PH_* variable is then consulted; its emit flags follow
    each run's `to_planes`) instead of `native_neck_cfg`'s."""
    _symbols, _geometry_type, _destroy_symbol = ("ph_neck_plan_workspace_bytes", "ph_neck_plan_create", "ph_neck_plan_info"), \
        _lib.NeckGeometry, "ph_neck_plan_destroy"

    def __init__(self, pack, B, shapes, device, pos_level=3, tower_streams=True, cfg=None):
        dev = torch.device(device)
        self.pack, self.B, self.shapes, self.device = pack, B, tuple(tuple(x) for x in shapes), dev
        base = cfg if cfg is not None else native_neck_cfg(B, self.shapes, pack.groups, _MODE_NAME[pack.mode], pack.num_outs, pos_level, False,
                                                           tower_streams, device_type=dev.type)
        self.cfg = _lib.NeckCfg.from_buffer_copy(bytes(base))
        self.pos_level, self.groups = self.cfg.pos_level, self.cfg.groups
        self._alloc_workspace()
        self._handles, self._outs = {}, {}
        self.geometry = self._info(self._handle(bool(self.cfg.emit_planes) and not self.cfg.emit_f32))
        self.Ho, self.Wo, self.multi = self.geometry.Ho, self.geometry.Wo, bool(self.geometry.tower_buffers)
        self._streams = None
        self.io = _lib.NeckIO()

    def _handle(self, to_planes):
        """the native plan that writes planes / fp32 maps"""
        return self._handle_of(emit_planes=bool(to_planes), emit_f32=not to_planes)

    def outputs(self, to_planes):
        """the output tensors of the planes / fp32 form (allocated on first use)"""
        if to_planes not in self._outs:
            g, n = self.geometry, self.cfg.num_outs
            shape, dt = ((g.P, self.B, 256, g.HWp), torch.int16) if to_planes else ((self.B, 256, g.Ho, g.Wo), torch.float32)
            self._outs[to_planes] = [torch.empty(shape, dtype=dt, device=self.device) for _ in range(n)]
        return self._outs[to_planes]

    def _fill_io(self, feats, posenc, outs, to_planes):
        io = self.io
        for l in range(4):
            f = feats[l]
            if f.dtype != torch.float32 or not f.is_contiguous() or tuple(f.shape) != (self.B, 256) + self.shapes[l] or f.device != self.device:
                raise _lib.PolyheadError(f"NativeNeckPlan.run: level {l} must be fp32 contiguous {(self.B, 256) + self.shapes[l]} on {self.device}")
            io.feats[l] = f.data_ptr()
        if self.pos_level >= 0:
            if posenc is None or posenc.dtype != torch.float32 or not posenc.is_contiguous() or \
                    tuple(posenc.shape) != (256,) + self.shapes[self.pos_level] or posenc.device != self.device:
                raise _lib.PolyheadError("NativeNeckPlan.run: posenc must be fp32 contiguous [256, h, w] of the cfg's pos_level")
            io.posenc = posenc.data_ptr()
        else:
            io.posenc = None
        return self._point_outputs(outs, to_planes)

    def _point_outputs(self, outs, to_planes):
        io = self.io
        for i in range(3):
            t = outs[i] if i < len(outs) else None
            io.out_planes[i] = t.data_ptr() if (to_planes and t is not None) else None
            io.out_f32[i] = t.data_ptr() if (not to_planes and t is not None) else None
        return io

    def run(self, feats, pk=None, groups=None, posenc=None, pos_level=None, to_planes=False):
        """NeckPlan.run's arguments; `pk`: the NativeNeckPack to run from (a new one -- re-packed weights -- replaces the plan's),
        `groups` / `pos_level`: must be the cfg's when given"""
        if pk is not None and pk is not self.pack:
            if (pk.mode, pk.groups, pk.num_outs) != (self.pack.mode, self.pack.groups, self.pack.num_outs):
                raise _lib.PolyheadError("NativeNeckPlan.run: the pack's mode, groups or outputs differ from the plan's")
            self._destroy()
            self.pack = pk
        if groups is not None and groups != self.groups:
            raise _lib.PolyheadError("NativeNeckPlan.run: groups differ from the plan's cfg")
        if posenc is None and self.pos_level >= 0 and pos_level is not None:
            raise _lib.PolyheadError("NativeNeckPlan.run: the plan's cfg has a positional encoding, the call has none")
        if posenc is not None and pos_level is not None and pos_level != self.pos_level:
            raise _lib.PolyheadError("NativeNeckPlan.run: pos_level differs from the plan's cfg")
        lib, h = _lib.load(), self._handle(to_planes)
        outs = self.outputs(to_planes)
        io = self._fill_io(feats, posenc if self.pos_level >= 0 else None, outs, to_planes)
        if self.multi:
            self._streams = _fan_out_towers(self._streams, self.device, lambda lvl: _lib.check(
                lib.ph_neck_plan_run_level(h, lvl, C.byref(io), _lib.stream_ptr()), "ph_neck_plan_run_level"))
            _lib.check(lib.ph_neck_plan_run_outputs(h, C.byref(io), _lib.stream_ptr()), "ph_neck_plan_run_outputs")
        else:
            _lib.check(lib.ph_neck_plan_run(h, C.byref(io), _lib.stream_ptr()), "ph_neck_plan_run")
        return outs

    # ---- a level started from planes (NeckPlan's surface of the same names; `pk` / `groups` are the plan's own)
    prec = property(lambda self: self.geometry.prec)

    def level_input(self, lvl, pk=None, to_planes=False):
        p, layout = C.c_void_p(), C.c_int32()
        _lib.check(_lib.load().ph_neck_plan_level_input(self._handle(to_planes), lvl, C.byref(p), C.byref(layout)), "ph_neck_plan_level_input")
        return p, layout.value

    def run_level_planes(self, lvl, pk=None, groups=None, to_planes=False):
        _lib.check(_lib.load().ph_neck_plan_run_level_planes(self._handle(to_planes), lvl, _lib.stream_ptr()), "ph_neck_plan_run_level_planes")

    def run_towers_planes(self, pk=None, groups=None, to_planes=False):
        self._streams = _fan_out_towers(self._streams, self.device, lambda lvl: self.run_level_planes(lvl, to_planes=to_planes))

    def run_outputs(self, pk=None, groups=None, to_planes=False, posenc=None):
        outs = self.outputs(to_planes)
        io = self._point_outputs(outs, to_planes)
        io.posenc = posenc.data_ptr() if (self.pos_level >= 0 and posenc is not None) else None
        _lib.check(_lib.load().ph_neck_plan_run_outputs(self._handle(to_planes), C.byref(io), _lib.stream_ptr()), "ph_neck_plan_run_outputs")
        return outs


# ---- the FPN as a native object (include/polyhead.h ph_fpn_cfg .. ph_fpn_plan_run) -------------------------------------------
def native_fpn_cfg(B, shapes, in_channels, prec, x_dtype=torch.float32, emit_f32=True, emit_planes=False):
    """the ph_fpn_cfg of a native FPN plan.  `prec`: a precision name (engine.KHEAD_PREC's keys) or the grade code; `shapes`: the four
    level sizes; `in_channels`: the four stage widths; `x_dtype`: the stages' torch dtype.  The FPN has no PH_* variable"""
    name = prec if isinstance(prec, str) else _KHEAD_MODE_OF_PREC[prec]
    if len(shapes) != 4 or len(in_channels) != 4:
        raise _lib.PolyheadError("the FPN takes four stages")
    if x_dtype not in OUT_CODE:
        raise _lib.PolyheadError("the FPN's stages are fp32, bf16 or fp16")
    i4 = lambda xs: (C.c_int32 * 4)(*[int(x) for x in xs])
    return _lib.FpnCfg(B=B, k=i4(in_channels), h=i4([x[0] for x in shapes]), w=i4([x[1] for x in shapes]), mode=_lib.PH_MODE[name],
                       x_dtype=OUT_CODE[x_dtype], emit_f32=int(bool(emit_f32)), emit_planes=int(bool(emit_planes)))


class NativeFpnPack(_NativePack):
    """one device buffer packed by ph_fpn_pack, and its pieces as views in the form of fpn.FPN._pack's dict (`pk`: so either plan --
    FpnPlan or NativeFpnPlan -- runs from it)"""
    _symbols = ("ph_fpn_pack_bytes", "ph_fpn_param_name", "ph_fpn_param_numel", "ph_fpn_pack", "ph_fpn_pack_layout")
    _layout_type, _nparams = _lib.FpnLayout, staticmethod(lambda cfg: _lib.PH_FPN_NPARAMS)

    def _pieces(self, cfg):
        self.in_channels = tuple(cfg.k)
        one = lambda i, kk, k: dict(wp=self.piece(i, torch.int16, (self.P, 256 * kk)), bias=self.piece(i + 1, torch.float32, (256,)), k=k, s=1)
        self.pk = dict(lateral=[one(2 * l, cfg.k[l], 1) for l in range(4)], output=[one(8 + 2 * l, 9 * 256, 3) for l in range(4)])


def native_fpn_pack(module, cfg, device):
    """the FPN's parameters (a fpn.FPN, or its state_dict) packed on the device by ph_fpn_pack"""
    return NativeFpnPack.pack_on_device(module, cfg, device)


class NativeFpnPlan(_NativePlan):
    """FpnPlan's `run` surface over the native plan: ONE native call per forward (ph_fpn_plan_run), or -- handing over to a neck plan
    with shared buffers -- ph_fpn_plan_run_laterals and then ph_fpn_plan_run_output level by level with the level's tower behind it;
    the same launch sequence as the FpnPlan of the same arguments, so the same bits.  `pack`: a NativeFpnPack; `cfg`: a ph_fpn_cfg to
    use as it is (its emit flags follow each run) instead of `native_fpn_cfg`'s."""
    _symbols, _geometry_type, _destroy_symbol = ("ph_fpn_plan_workspace_bytes", "ph_fpn_plan_create", "ph_fpn_plan_info"), \
        _lib.FpnGeometry, "ph_fpn_plan_destroy"

    def __init__(self, pack, B, shapes, device, x_dtype=torch.float32, cfg=None):
        dev = torch.device(device)
        self.pack, self.B, self.shapes, self.device = pack, B, tuple(tuple(x) for x in shapes), dev
        base = cfg if cfg is not None else native_fpn_cfg(B, self.shapes, pack.in_channels, _MODE_NAME[pack.mode], x_dtype)
        self.cfg = _lib.FpnCfg.from_buffer_copy(bytes(base))
        self.in_channels, self.x_dtype = tuple(self.cfg.k), {v: k for k, v in OUT_CODE.items()}[self.cfg.x_dtype]
        self._alloc_workspace()
        self._handles = {}
        self.geometry = self._info(self._handle(True, False))
        self.prec = self.geometry.prec
        self.outs = None                                                            # the fp32 levels, allocated on first use
        self.io = _lib.FpnIO()

    def _handle(self, emit_f32, emit_planes):
        """the native plan of these emit flags"""
        return self._handle_of(emit_f32=bool(emit_f32), emit_planes=bool(emit_planes))

    def run(self, feats, pk=None, neck=None, want_levels=True):
        """FpnPlan.run's arguments (`pk`: the plan's own pack, when given)"""
        if pk is not None and pk is not self.pack and pk is not self.pack.pk:
            raise _lib.PolyheadError("NativeFpnPlan.run: the plan runs from the pack it was created with")
        B, io, lib = self.B, self.io, _lib.load()
        for l, t in enumerate(feats):
            if tuple(t.shape) != (B, self.in_channels[l]) + self.shapes[l] or t.dtype != self.x_dtype or not t.is_contiguous() \
                    or t.device != self.device:
                raise _lib.PolyheadError(f"NativeFpnPlan.run: inputs[{l}] must be a contiguous {self.x_dtype} tensor of shape "
                                         f"{(B, self.in_channels[l]) + self.shapes[l]} on {self.device}")
            io.stages[l] = t.data_ptr()
        if neck is not None and (neck.plan.B != B or tuple(tuple(x) for x in neck.plan.shapes) != self.shapes or neck.plan.prec != self.prec):
            raise _lib.PolyheadError("NativeFpnPlan.run: the neck plan's frames, level sizes or grade differ from this plan's")
        want_f32 = neck is None or want_levels
        if want_f32 and self.outs is None:
            self.outs = [torch.empty((B, 256, h, w), dtype=torch.float32, device=self.device) for h, w in self.shapes]
        for l in range(4):
            io.out_f32[l] = self.outs[l].data_ptr() if want_f32 else None
            io.out_planes[l], io.planes_layout[l], io.add[l] = None, 0, None
            if neck is not None:
                xa, layout = neck.plan.level_input(l, neck.pk, neck.to_planes)
                io.out_planes[l] = xa.value if isinstance(xa, C.c_void_p) else xa.data_ptr()
                io.planes_layout[l] = layout & _lib.PH_PLANES_C16
                io.add[l] = neck.posenc.data_ptr() if l == neck.pos_level else None
        h, st = self._handle(want_f32, neck is not None), _lib.stream_ptr()
        if neck is None or neck.plan.multi:
            _lib.check(lib.ph_fpn_plan_run(h, C.byref(io), st), "ph_fpn_plan_run")
        else:
            _lib.check(lib.ph_fpn_plan_run_laterals(h, C.byref(io), st), "ph_fpn_plan_run_laterals")
            for l in range(4):
                _lib.check(lib.ph_fpn_plan_run_output(h, l, C.byref(io), st), "ph_fpn_plan_run_output")
                neck.plan.run_level_planes(l, neck.pk, neck.groups, neck.to_planes)
        return self.outs if want_f32 else None


class DualDecodePlan:
    """`parts` part-batches (two by default) on as many HIP streams, each one phase behind the previous: the query
    kernels of a stage are a short, latency-bound chain on ~1 workgroup per CU, the pooling / conv / upsample kernels are
    HBM-bound; running one part's HBM phases underneath another's query phase (and vice versa) fills both.  Frames are
    independent, so the split changes nothing numerically.  Captured as ONE HIP graph with fork/join edges.  Measured on
    one box at 24 frames per part: 2 parts 13.1-13.3 k frames/s, 4 parts 13.4-13.8 k (the fill / drain of the skew is
    amortised over more parts), 6 or 8 parts no further gain."""

    def __init__(self, packs, B, N, H, W, prec, out_dtype=torch.float32, device="cuda:0", parts=2):
        assert B >= parts >= 2
        self.B, self.parts = B, parts
        base, rem = divmod(B, parts)
        self.sizes = [base + (1 if i < rem else 0) for i in range(parts)]
        self.halves = [DecodePlan(packs, n, N, H, W, prec, out_dtype, device, shares_gpu=True) for n in self.sizes]
        self.graph = None

    def set_inputs(self, x, dfe, k0, q0, m0):
        o = 0
        before = [p.m0.dtype for p in self.halves]
        for p, n in zip(self.halves, self.sizes):
            p.set_inputs(x[o:o + n], dfe[o:o + n], k0[o:o + n], q0[o:o + n], m0[o:o + n])
            o += n
        if before != [p.m0.dtype for p in self.halves]:
            self.graph = None            # the parts re-allocated their mask-logit buffers: the captured graph is stale (capture again)

    def _issue(self, *streams):
        cur = torch.cuda.current_stream()
        prev = None
        for p, st in zip(self.halves, streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                if prev is not None:
                    st.wait_event(prev)      # a part starts once the previous one's ingest is done: a phase apart from then on
                p.ingest()
                prev = torch.cuda.Event()
                prev.record(st)
                p.stages()
        for st in streams:
            cur.wait_stream(st)

    def run(self):
        if not hasattr(self, "_streams"):
            self._streams = tuple(torch.cuda.Stream() for _ in range(self.parts))
        self._issue(*self._streams)

    def capture(self):
        self.run()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._issue(*self._streams)
        return self.graph

    def replay(self):
        self.graph.replay()

    def outputs(self):
        o = [h.outputs() for h in self.halves]
        return {k: (None if o[0][k] is None else torch.cat([oi[k] for oi in o], 0)) for k in o[0]}


# ---- the native association plan (include/polyhead.h ph_track_cfg .. ph_assoc_plan_match; csrc/ph_assocplan.hip) -------------------
def native_track_cfg(head, prec=None):
    """a ph_track_cfg of a QuasiDenseMaskEmbedHeadGTMask (or of a dict with its sizes); `prec`: a precision name or PH_PREC_* code,
    default the head's own"""
    get = (lambda k, d=None: head.get(k, d)) if isinstance(head, dict) else (lambda k, d=None: getattr(head, k, d))
    if prec is None:
        prec = get("precision", "fp32")
    return _lib.TrackCfg(num_convs=int(get("num_convs", 4)), fc_out_channels=int(get("fc_out_channels", 1024)),
                         embed_channels=int(get("embed_channels", 256)), groups=int(get("groups", 32)),
                         prec=PREC[prec] if isinstance(prec, str) else int(prec), eps=0.0)


def native_assoc_cfg(B, out_hw, K, max_things, num_thing_classes, num_stuff_classes, level_shapes, track, strides=(4, 8, 16, 32),
                     finest_scale=56.0):
    """a ph_assoc_cfg: B frames of an (Ho, Wo) id map with K record rows and `max_things` RoIs per frame; `level_shapes`: (h, w) of
    the FPN levels RoIAlign reads, finest first; `track`: a ph_track_cfg (`native_track_cfg`).  Reads no PH_* variable."""
    L = len(level_shapes)
    if not 1 <= L <= 4:
        raise _lib.PolyheadError("native_assoc_cfg: 1 .. 4 FPN levels")
    c = _lib.AssocCfg(B=B, Ho=out_hw[0], Wo=out_hw[1], K=K, max_things=max_things, num_thing_classes=num_thing_classes,
                      num_stuff_classes=num_stuff_classes, nlev=L, finest_scale=finest_scale)
    for l, (h, w) in enumerate(level_shapes):
        c.h[l], c.w[l], c.inv_stride[l] = int(h), int(w), 1.0 / strides[l]
    c.track = _lib.TrackCfg.from_buffer_copy(bytes(track))
    return c


class NativeTrackPack(_NativePack):
    """one device buffer packed by ph_track_pack + views of its pieces under `_get_pack`'s names (the views share the buffer)"""
    _symbols = ("ph_track_pack_bytes", "ph_track_param_name", "ph_track_param_numel", "ph_track_pack", "ph_track_pack_layout")
    _layout_type, _nparams, _name_takes_cfg = _lib.TrackLayout, staticmethod(lambda cfg: 3 * cfg.num_convs + 4), True

    def _pieces(self, cfg):
        piece, P, F, E, n = self.piece, self.P, cfg.fc_out_channels, cfg.embed_channels, cfg.num_convs
        self.pk = dict(convs=[piece(i, torch.int16, (P, 256 * 2304)) for i in range(n)],
                       gn=[(piece(_lib.PH_TRACK_MAX_CONVS + i, torch.float32, (256,)),
                            piece(2 * _lib.PH_TRACK_MAX_CONVS + i, torch.float32, (256,))) for i in range(n)],
                       fc=piece(_lib.PH_TPACK_FC, torch.int16, (P, F * 49 * 256)), fc_b=piece(_lib.PH_TPACK_FC_B, torch.float32, (F,)),
                       emb=piece(_lib.PH_TPACK_EMB, torch.int16, (P, E * F)), emb_b=piece(_lib.PH_TPACK_EMB_B, torch.float32, (E,)),
                       prec=self.prec, P=P)


def native_track_pack(module, cfg, device):
    """the track head's parameters (a QuasiDenseMaskEmbedHeadGTMask, or its state_dict) packed on the device by ph_track_pack"""
    return NativeTrackPack.pack_on_device(module, cfg, device)


class NativeAssocPlan(_NativePlan):
    """The association step of B frames over ph_panoptic_merge's device outputs: `run` is ONE launch-only native call
    (ph_assoc_plan_run: things tables, `sem`, boxes, RoIAlign, track embeddings -- capturable with torch.cuda.graph), `match` the one
    synchronising call behind it (ph_assoc_plan_match: the tracker and the `track` maps), `track` that call's launch-only counterpart
    over a tracker.NativeDeviceTracker (ph_assoc_plan_track).  `pack`: a NativeTrackPack; `cfg`: a
    ph_assoc_cfg (`native_assoc_cfg`).  The outputs are this object's static tensors: the next call overwrites them."""
    _symbols, _geometry_type, _destroy_symbol = ("ph_assoc_plan_workspace_bytes", "ph_assoc_plan_create", "ph_assoc_plan_info"), \
        _lib.AssocGeometry, "ph_assoc_plan_destroy"

    def __init__(self, pack, cfg, device):
        dev = torch.device(device)
        self.pack, self.device = pack, dev
        self.cfg = _lib.AssocCfg.from_buffer_copy(bytes(cfg))
        if bytes(self.cfg.track) != bytes(pack.cfg):
            raise _lib.PolyheadError("NativeAssocPlan: the pack was made for another track head cfg")
        self._alloc_workspace()
        self._h = self._create(_lib.ptr(pack.blob))
        self.geometry = self._info(self._h)
        c = self.cfg
        self.B, self.K, self.cap, self.words = c.B, c.K, c.max_things, self.geometry.things_words
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        self.sem, self.track_map = e((c.B, c.Ho, c.Wo), torch.uint8), e((c.B, c.Ho, c.Wo), torch.float64)
        self.things, self.embeds = e((c.B, self.words), torch.int32), e((c.B, self.cap, 256), torch.float32)
        self.staging = torch.empty((int(self.geometry.staging_bytes),), dtype=torch.uint8, pin_memory=dev.type == "cuda")
        self.ids = torch.zeros((c.B, self.cap), dtype=torch.int64)
        self.ids_dev = e((c.B, self.cap), torch.int64)                              # `track`'s painted ids
        self.io = _lib.AssocIO()
        self._keep = None

    def rois(self):
        """the RoIs of the last run, fp32 [B, K, 5] (a view of the workspace; inspection)"""
        o = int(self.geometry.rois_offset)
        return self.workspace[o:o + self.B * self.K * 20].view(torch.float32).reshape(self.B, self.K, 5)

    def roi_planes(self):
        """RoIAlign's output of the last run, bf16 planes as int16 [P, B, cap, 49, 256] (a view of the workspace; inspection)"""
        o, P = int(self.geometry.roi_planes_offset), self.geometry.P
        return self.workspace[o:o + P * self.B * self.cap * 49 * 256 * 2].view(torch.int16).reshape(P, self.B, self.cap, 49, 256)

    def run(self, pan, seg_records, levels, roi_planes=None):
        """pan int32 [B, Ho, Wo], seg_records int32 [B, 1 + 5 K], levels: fp32 [B, 256, h_l, w_l] per level, all contiguous on the
        device -> (sem uint8 [B, Ho, Wo], things tables int32 [B, 2 + 7 cap], embeddings fp32 [B, cap, 256]); launches only.
        `roi_planes`: the caller's RoI features, int16 [P, B, cap, 49, 256], instead of RoIAlign's"""
        if roi_planes is not None and (roi_planes.dtype != torch.int16 or not roi_planes.is_contiguous() or
                                       tuple(roi_planes.shape) != (self.geometry.P, self.B, self.cap, 49, 256)):
            raise _lib.PolyheadError("NativeAssocPlan.run: roi_planes must be int16 contiguous [P, B, cap, 49, 256]")
        self.io.roi_planes = None if roi_planes is None else roi_planes.data_ptr()
        c, io = self.cfg, self.io
        if pan.dtype != torch.int32 or tuple(pan.shape) != (c.B, c.Ho, c.Wo) or not pan.is_contiguous() or pan.device != self.device:
            raise _lib.PolyheadError(f"NativeAssocPlan.run: pan must be int32 contiguous {(c.B, c.Ho, c.Wo)} on {self.device}")
        if seg_records.dtype != torch.int32 or tuple(seg_records.shape) != (c.B, 1 + 5 * c.K) or not seg_records.is_contiguous():
            raise _lib.PolyheadError(f"NativeAssocPlan.run: seg_records must be int32 contiguous {(c.B, 1 + 5 * c.K)}")
        if len(levels) != c.nlev:
            raise _lib.PolyheadError(f"NativeAssocPlan.run: {c.nlev} FPN levels expected")
        for l, f in enumerate(levels):
            if f.dtype != torch.float32 or not f.is_contiguous() or tuple(f.shape) != (c.B, 256, c.h[l], c.w[l]) or f.device != self.device:
                raise _lib.PolyheadError(f"NativeAssocPlan.run: level {l} must be fp32 contiguous {(c.B, 256, c.h[l], c.w[l])} on {self.device}")
            io.levels[l], io.level_stride[l] = f.data_ptr(), 256 * c.h[l] * c.w[l]
        io.pan, io.seg_records = pan.data_ptr(), seg_records.data_ptr()
        io.sem_out, io.things_out, io.embeds_out = self.sem.data_ptr(), self.things.data_ptr(), self.embeds.data_ptr()
        self._keep = (pan, seg_records, tuple(levels), roi_planes)      # alive until the launches have run (static under graph capture)
        _lib.check(_lib.load().ph_assoc_plan_run(self._h, C.byref(io), _lib.stream_ptr()), "ph_assoc_plan_run")
        return self.sem, self.things, self.embeds

    def match(self, tracker, pan, first_frame_id):
        """the host tracker (a tracker.NativeHostTracker) and the track-id maps behind `run` on the current stream: synchronises.
        Returns (track float64 [B, Ho, Wo] on the device, painted ids int64 [B, cap] on the host, frames matched)"""
        m = _lib.load().ph_assoc_plan_match(self._h, tracker.handle, _lib.ptr(pan), _lib.ptr(self.things), _lib.ptr(self.embeds),
                                            C.c_void_p(self.staging.data_ptr()), self.staging.numel(), int(first_frame_id),
                                            _lib.ptr(self.track_map), C.c_void_p(self.ids.data_ptr()), _lib.stream_ptr())
        if m < 0:
            _lib.check(m, "ph_assoc_plan_match")
        return self.track_map, self.ids, int(m)

    def track(self, dtracker, pan):
        """the device tracker (a tracker.NativeDeviceTracker) and the track-id maps behind `run` on the current stream: launches only, no
        synchronisation, capturable.  Returns (track float64 [B, Ho, Wo], painted ids int64 [B, cap]), both on the device; the frames
        matched are `dtracker.status()["matched"]`"""
        _lib.check(_lib.load().ph_assoc_plan_track(self._h, dtracker._h, _lib.ptr(pan), _lib.ptr(self.things), _lib.ptr(self.embeds),
                                                   _lib.ptr(self.track_map), _lib.ptr(self.ids_dev), _lib.stream_ptr()), "ph_assoc_plan_track")
        return self.track_map, self.ids_dev

    def track_streams(self, bank, pan, active=None):
        """`track` with frame b going to stream b of a tracker.NativeDeviceTrackerBank of B streams (ph_assoc_plan_track_streams): one
        tracker step for the B frames.  `active`: int32 [B] on the device or None; a zero word is an idle stream -- its tracker is
        untouched and its track map all zero.  Launches only, capturable; same returns as `track`"""
        active = bank._active(active)
        self._keep_active = active
        _lib.check(_lib.load().ph_assoc_plan_track_streams(self._h, bank._h, _lib.ptr(pan), _lib.ptr(self.things), _lib.ptr(self.embeds),
                                                           None if active is None else _lib.ptr(active), _lib.ptr(self.track_map),
                                                           _lib.ptr(self.ids_dev), _lib.stream_ptr()), "ph_assoc_plan_track_streams")
        return self.track_map, self.ids_dev


# ---- ResNet backbone at inference (mmdet/models/backbones/resnet.py; csrc/ph_resnet.hip): the image tensor -> the FPN's stages ----
def conv_out_size(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def conv_cl(x, wp, bias, res, y, k, s, relu, B, H, W, cin, cout, prec):
    """channels-last 16-bit plane x [B, H*W, cin] -> y [B, Ho*Wo, cout]: conv k x k stride s with the folded BN (wp: pack_b32 fragments
    of W'[cout][k*k*cin], bias: b'), + res (y's form, or None), ReLU if `relu`, one rounding"""
    _lib.check(_lib.load().ph_conv_cl(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(res), _lib.ptr(y), k, s, int(bool(relu)), B, H, W,
                                      cin, cout, prec, _lib.stream_ptr()), "ph_conv_cl")
    return y


def resnet_stem(x, wp, bias, y, prec):
    """x [B, 3, H, W] fp32 / bf16 contiguous -> y [B, Hq*Wq, 64]: conv 7x7 s2 + folded BN + ReLU + MaxPool2d(3, 2, 1)"""
    B, _, H, W = x.shape
    _lib.check(_lib.load().ph_resnet_stem(_lib.ptr(x), OUT_CODE[x.dtype], _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(y), B, H, W, prec,
                                          _lib.stream_ptr()), "ph_resnet_stem")
    return y


def stem_out_size(n):
    return ((n - 1) // 2 + 1 - 1) // 2 + 1


def cl_to_nchw(x, out, B, HW, C_, prec):
    """channels-last 16-bit plane x [B, HW, C] of grade `prec` -> out [B, C, h, w] fp32 / bf16 / fp16"""
    _lib.check(_lib.load().ph_cl_to_nchw(_lib.ptr(x), _lib.ptr(out), OUT_CODE[out.dtype], B, HW, C_, prec, _lib.stream_ptr()), "ph_cl_to_nchw")
    return out


class ResNetPlan:
    """buffers + launch sequence of resnet.ResNet.forward for one (B, H, W, block structure, grade, hand-off dtype): the stem's plane, two
    ping-pong block planes, the two inner planes of a bottleneck, the downsample plane and the NCHW stages, all sized here.  `run`
    issues everything on the current stream -- one stream, so a captured graph of it has no parallel branches -- and neither
    allocates nor synchronises; the outputs are the plan's buffers and are overwritten by the next call, as FpnPlan's are.
    blocks: per stage a list of (cin, planes, stride, has_downsample).
    stage_planes=True: the last bottleneck of every output stage writes a plane the plan owns for that stage (`stage_plane(i)`) instead
    of a ping-pong plane, which the next stage overwrites -- the same launches and values, so the stage outlives the run as the 16-bit
    channels-last plane `fpn_lateral_cl` reads; `run(.., nchw=False)` then skips the NCHW conversions, and the NCHW tensors are
    allocated at the first run that asks for them."""

    def __init__(self, B, H, W, blocks, out_indices, prec, stage_dtype, device, stage_planes=False):
        if prec not in (_lib.PH_PREC_BF16, _lib.PH_PREC_F16):
            raise _lib.PolyheadError("ResNetPlan: the grade must be bf16 or fp16 (one 16-bit plane)")
        if stage_dtype not in OUT_CODE:
            raise _lib.PolyheadError("ResNetPlan: the hand-off dtype must be torch.float32, torch.bfloat16 or torch.float16")
        self.B, self.H, self.W, self.prec, self.stage_dtype = B, H, W, prec, stage_dtype
        self.blocks, self.out_indices = [list(s) for s in blocks], tuple(out_indices)
        lib, dev = _lib.load(), torch.device(device)
        self.device = dev

        def wg(n, what):
            if n <= 0:
                _lib.check(n if n < 0 else _lib.PH_EINVAL, what)
            return n
        h, w = stem_out_size(H), stem_out_size(W)
        self.stem_hw = (h, w)
        self.workgroups = [("stem", wg(lib.ph_resnet_stem_workgroups(H, W, B), "ph_resnet_stem_workgroups"))]
        io = inner = down = 0
        self.stage_shapes = []
        for si, stage in enumerate(self.blocks):
            for j, (cin, planes, s, has_down) in enumerate(stage):
                ho, wo = conv_out_size(h, 3, s), conv_out_size(w, 3, s)
                for name, k, st, ci, co, hh, ww in (("conv1", 1, 1, cin, planes, h, w), ("conv2", 3, s, planes, planes, h, w),
                                                    ("conv3", 1, 1, planes, 4 * planes, ho, wo)) + \
                        ((("downsample", 1, s, cin, 4 * planes, h, w),) if has_down else ()):
                    self.workgroups.append((f"layer{si + 1}.{j}.{name}", wg(lib.ph_conv_cl_workgroups(k, st, ci, co, hh, ww, B),
                                                                          "ph_conv_cl_workgroups")))
                inner = max(inner, h * w * planes, ho * wo * planes)
                io = max(io, ho * wo * 4 * planes)
                if has_down:
                    down = max(down, ho * wo * 4 * planes)
                elif (cin, s) != (4 * planes, 1):
                    raise _lib.PolyheadError("ResNetPlan: a block without downsample must keep its shape")
                h, w = ho, wo
            self.stage_shapes.append((4 * stage[-1][1], h, w))
            self.workgroups.append((f"layer{si + 1}.to_nchw", wg(lib.ph_cl_to_nchw_workgroups(B, h * w, 4 * stage[-1][1]),
                                                               "ph_cl_to_nchw_workgroups")))
        e = lambda n: torch.empty((B * n,), dtype=torch.int16, device=dev)
        self.p0 = e(self.stem_hw[0] * self.stem_hw[1] * 64)
        self.pa, self.pb, self.t1, self.t2, self.pd = e(io), e(io), e(inner), e(inner), e(max(down, 8))
        self.planes = {i: e(math.prod(self.stage_shapes[i])).view(B, -1, self.stage_shapes[i][0]) for i in self.out_indices} \
            if stage_planes else None
        self.outs = None if stage_planes else self._nchw()

    def _nchw(self):
        return {i: torch.empty((self.B,) + self.stage_shapes[i], dtype=self.stage_dtype, device=self.device) for i in self.out_indices}

    def stage_plane(self, i):
        """output stage i as the last run left it: int16 [B, h*w, C] holding the grade's 16-bit values (stage_planes=True only)"""
        if self.planes is None:
            raise _lib.PolyheadError("ResNetPlan.stage_plane: the plan was built without stage_planes=True")
        return self.planes[i]

    def bytes(self):
        """device memory the plan holds at this moment"""
        ts = [self.p0, self.pa, self.pb, self.t1, self.t2, self.pd] + list((self.planes or {}).values()) + list((self.outs or {}).values())
        return sum(t.numel() * t.element_size() for t in ts)

    def run_stem(self, x, pk):
        """the stem's launch; x: [B, 3, H, W] fp32 / bf16 contiguous on the plan's device"""
        B = self.B
        if tuple(x.shape) != (B, 3, self.H, self.W) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous() \
                or x.device != self.device:
            raise _lib.PolyheadError(f"ResNetPlan.run: x must be a contiguous fp32 / bf16 device tensor of shape {(B, 3, self.H, self.W)}")
        resnet_stem(x, pk["stem"][0], pk["stem"][1], self.p0, self.prec)
        self._at = (self.stem_hw, self.p0, self.pa)                 # (size, the plane that holds the activation, the one to write next)

    def run_stage(self, si, pk, nchw=True):
        """stage si's launches (its bottlenecks and, if it is an output and `nchw`, the NCHW conversion) on what the previous step left"""
        B, prec, stage = self.B, self.prec, self.blocks[si]
        (h, w), cur, nxt = self._at
        for j, (cin, planes, s, has_down) in enumerate(stage):
            if self.planes is not None and si in self.planes and j == len(stage) - 1:
                nxt = self.planes[si]                            # both ping-pong planes are free behind it
            c = pk["blocks"][si][j]
            ho, wo = conv_out_size(h, 3, s), conv_out_size(w, 3, s)
            conv_cl(cur, c["conv1"][0], c["conv1"][1], None, self.t1, 1, 1, True, B, h, w, cin, planes, prec)
            conv_cl(self.t1, c["conv2"][0], c["conv2"][1], None, self.t2, 3, s, True, B, h, w, planes, planes, prec)
            idn = cur
            if has_down:
                idn = conv_cl(cur, c["downsample"][0], c["downsample"][1], None, self.pd, 1, s, False, B, h, w, cin, 4 * planes, prec)
            conv_cl(self.t2, c["conv3"][0], c["conv3"][1], idn, nxt, 1, 1, True, B, ho, wo, planes, 4 * planes, prec)
            cur, nxt = nxt, (self.pb if nxt is self.pa else self.pa)
            h, w = ho, wo
        if nchw and si in self.out_indices:
            if self.outs is None:
                self.outs = self._nchw()
            cl_to_nchw(cur, self.outs[si], B, h * w, 4 * stage[-1][1], prec)
        self._at = ((h, w), cur, nxt)

    def run(self, x, pk, nchw=True):
        """x: [B, 3, H, W] fp32 / bf16 contiguous on the plan's device; pk: resnet.ResNet's pack.  Returns the NCHW stages of
        out_indices; nchw=False (a stage_planes plan): the launches without the NCHW conversions, returns None -- `stage_plane(i)`"""
        if not nchw and self.planes is None:
            raise _lib.PolyheadError("ResNetPlan.run: nchw=False needs a plan built with stage_planes=True")
        self.run_stem(x, pk)
        for si in range(max(self.out_indices) + 1):              # a stage behind the last output has no reader
            self.run_stage(si, pk, nchw)
        return tuple(self.outs[i] for i in self.out_indices) if nchw else None


class StagePlanes:
    """the backbone's output stages as it holds them: `planes[l]` int16 [B, h*w, C] (16-bit channels-last values of grade `prec`,
    PH_PREC_BF16 / PH_PREC_F16), `shapes[l]` = (C, h, w).  What resnet.ResNet.forward_planes returns and FpnPlan.run, fpn.FPN and
    SemanticFPNWrapper.forward_from_fpn take in place of the NCHW tensors.  The planes are the backbone plan's buffers: the next
    forward of the same size overwrites them."""

    def __init__(self, planes, shapes, prec):
        if prec not in (_lib.PH_PREC_BF16, _lib.PH_PREC_F16):
            raise _lib.PolyheadError("StagePlanes: the grade must be PH_PREC_BF16 or PH_PREC_F16")
        self.planes, self.shapes, self.prec = tuple(planes), tuple(tuple(int(v) for v in s) for s in shapes), prec
        if len(self.planes) != len(self.shapes):
            raise _lib.PolyheadError("StagePlanes: one (C, h, w) per plane")
        for t, (c, h, w) in zip(self.planes, self.shapes):
            if t.dtype != torch.int16 or not t.is_contiguous() or t.dim() != 3 or tuple(t.shape[1:]) != (h * w, c):
                raise _lib.PolyheadError(f"StagePlanes: a plane must be contiguous int16 [B, {h * w}, {c}]")

    B = property(lambda self: self.planes[0].shape[0])
    device = property(lambda self: self.planes[0].device)

    def __len__(self):
        return len(self.planes)


# ---- the backbone as a native object (include/polyhead.h ph_resnet_cfg .. ph_resnet_plan_run) --------------------------------
RESNET_ARCH = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}       # Bottleneck blocks per stage


def native_resnet_cfg(B, H, W, depth, prec, x_dtype=torch.float32, stage_dtype=torch.float32, out_indices=(0, 1, 2, 3), eps=1e-5):
    """the ph_resnet_cfg of a native backbone plan.  `prec`: a precision name (engine.KHEAD_PREC's keys) or the grade code; `x_dtype`:
    the image's torch dtype; `stage_dtype`: the stages'; `out_indices`: the stages written.  The backbone has no PH_* variable"""
    name = prec if isinstance(prec, str) else _KHEAD_MODE_OF_PREC[prec]
    if x_dtype not in OUT_CODE or stage_dtype not in OUT_CODE:
        raise _lib.PolyheadError("the backbone's image is fp32 or bf16, its stages fp32, bf16 or fp16")
    if not out_indices or min(out_indices) < 0 or max(out_indices) > 3:
        raise _lib.PolyheadError("out_indices must lie in [0, 4)")
    mask = 0
    for i in out_indices:
        mask |= 1 << int(i)
    return _lib.ResNetCfg(B=B, H=H, W=W, depth=depth, mode=_lib.PH_MODE[name], x_dtype=OUT_CODE[x_dtype], out_dtype=OUT_CODE[stage_dtype],
                          out_mask=mask, eps=float(eps))


class NativeResNetPack(_NativePack):
    """one device buffer packed by ph_resnet_pack (the BatchNorm fold in float64 on the device), and its pieces as views in the form
    of resnet.ResNet._pack's dict (`pk`: so either plan -- ResNetPlan or NativeResNetPlan -- runs from it)"""
    _symbols = ("ph_resnet_pack_bytes", "ph_resnet_param_name", "ph_resnet_param_numel", "ph_resnet_pack", "ph_resnet_pack_layout")
    _layout_type, _name_takes_cfg = _lib.ResNetLayout, True
    _nparams = staticmethod(lambda cfg: _lib.load().ph_resnet_nparams(C.byref(cfg)))

    def _pieces(self, cfg):
        self.depth, self.eps = cfg.depth, cfg.eps
        convs = iter(range(self.layout.nconvs))                 # state_dict order: a block's conv1, conv2, conv3, downsample

        def one():
            c = next(convs)
            return self.piece(2 * c, torch.int16, (-1,)), self.piece(2 * c + 1, torch.float32, (-1,))
        stem = one()
        self.pk = dict(stem=stem, blocks=[[dict(conv1=one(), conv2=one(), conv3=one(), downsample=one() if j == 0 else None)
                                           for j in range(nb)] for nb in RESNET_ARCH[cfg.depth]])


def native_resnet_pack(module, cfg, device):
    """the backbone's parameters and running statistics (a resnet.ResNet, or its state_dict) folded and packed on the device by
    ph_resnet_pack"""
    return NativeResNetPack.pack_on_device(module, cfg, device)


class NativeResNetPlan(_NativePlan):
    """ResNetPlan's `run` / `run_stem` / `run_stage` surface over the native plan: ONE native call per forward (ph_resnet_plan_run)
    instead of 57 at depth 50; the same launch sequence and arguments as the ResNetPlan of the same shape, so the same bits.  The
    plan owns the stage tensors as ResNetPlan does.  `pack`: a NativeResNetPack; `cfg`: a ph_resnet_cfg to use as it is (its x_dtype
    follows each run's image) instead of `native_resnet_cfg`'s."""
    _symbols, _geometry_type, _destroy_symbol = ("ph_resnet_plan_workspace_bytes", "ph_resnet_plan_create", "ph_resnet_plan_info"), \
        _lib.ResNetGeometry, "ph_resnet_plan_destroy"

    def __init__(self, pack, B, H, W, device, stage_dtype=torch.float32, out_indices=(0, 1, 2, 3), cfg=None):
        dev = torch.device(device)
        self.pack, self.B, self.H, self.W, self.device = pack, B, H, W, dev
        base = cfg if cfg is not None else native_resnet_cfg(B, H, W, pack.depth, _MODE_NAME[pack.mode], torch.float32, stage_dtype,
                                                             out_indices, pack.eps)
        self.cfg = _lib.ResNetCfg.from_buffer_copy(bytes(base))
        self.out_indices = tuple(i for i in range(4) if self.cfg.out_mask >> i & 1)
        self.stage_dtype = {v: k for k, v in OUT_CODE.items()}[self.cfg.out_dtype]
        self._alloc_workspace()
        self._handles = {}
        self.geometry = geo = self._info(self._handle(torch.float32))
        self.prec = geo.prec
        self.stage_shapes = [(geo.c[i], geo.h[i], geo.w[i]) for i in range(4)]
        self.outs = {i: torch.empty((B,) + self.stage_shapes[i], dtype=self.stage_dtype, device=dev) for i in self.out_indices}
        self.io = _lib.ResNetIO()
        for i, t in self.outs.items():
            self.io.stages[i] = t.data_ptr()

    def _handle(self, x_dtype):
        """the native plan of this image dtype"""
        return self._handle_of(x_dtype=OUT_CODE[x_dtype])

    def _own(self, pk, what):
        if pk is not None and pk is not self.pack and pk is not self.pack.pk:
            raise _lib.PolyheadError(f"NativeResNetPlan.{what}: the plan runs from the pack it was created with")

    def _image(self, x):
        if tuple(x.shape) != (self.B, 3, self.H, self.W) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous() \
                or x.device != self.device:
            raise _lib.PolyheadError(f"NativeResNetPlan.run: x must be a contiguous fp32 / bf16 device tensor of shape "
                                     f"{(self.B, 3, self.H, self.W)}")
        self.io.image = x.data_ptr()
        self._h_run = self._handle(x.dtype)

    def run_stem(self, x, pk=None):
        """the stem's launch; x: [B, 3, H, W] fp32 / bf16 contiguous on the plan's device"""
        self._own(pk, "run_stem")
        self._image(x)
        _lib.check(_lib.load().ph_resnet_plan_run_stem(self._h_run, C.byref(self.io), _lib.stream_ptr()), "ph_resnet_plan_run_stem")

    def run_stage(self, si, pk=None):
        """stage si's launches on what the previous step left (ResNetPlan.run_stage)"""
        self._own(pk, "run_stage")
        _lib.check(_lib.load().ph_resnet_plan_run_stage(self._h_run, si, C.byref(self.io), _lib.stream_ptr()), "ph_resnet_plan_run_stage")

    def run(self, x, pk=None):
        """ResNetPlan.run's arguments (`pk`: the plan's own pack, when given).  Returns the NCHW stages of out_indices"""
        self._own(pk, "run")
        self._image(x)
        _lib.check(_lib.load().ph_resnet_plan_run(self._h_run, C.byref(self.io), _lib.stream_ptr()), "ph_resnet_plan_run")
        return tuple(self.outs[i] for i in self.out_indices)


# ---- the backbone in training (csrc/ph_resnet_train.hip): data and weight gradients of the stages behind the frozen ones -----------
def conv_cl_bwd_data(dz, wt, r, r_stride, m, dx, k, s, B, H, W, cin, cout):
    """gradient at a convolution's input plane dx [B, H*W, cin] from the gradient dz [B, Ho*Wo, cout] at its output; wt: the transposed
    pack (ph_conv_cl_pack_bwd); r (bf16 plane or None, r_stride 1: dx's size, 2: the half-resolution plane spread to the even pixels) is
    added in fp32, the result is zero where the plane m (or None) is <= 0; k, s, H, W, cin, cout: the FORWARD layer's"""
    _lib.check(_lib.load().ph_conv_cl_bwd_data(_lib.ptr(dz), _lib.ptr(wt), _lib.ptr(r), r_stride, _lib.ptr(m), _lib.ptr(dx), k, s, B, H, W,
                                               cin, cout, _lib.stream_ptr()), "ph_conv_cl_bwd_data")
    return dx


def conv_cl_bwd_weight(dz, x, dw, db, partial, nsplit, k, s, B, H, W, cin, cout):
    """dw fp32 [cout, k*k*cin] (k = tap * cin + c) and db fp32 [cout] of a convolution from dz [B, Ho*Wo, cout] and its input plane x
    [B, H*W, cin]; nsplit 0: the library's rule; partial: fp32 scratch of ph_conv_cl_bwd_weight_partial_floats (None for one range)"""
    _lib.check(_lib.load().ph_conv_cl_bwd_weight(_lib.ptr(dz), _lib.ptr(x), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(partial), nsplit, k, s, B,
                                                 H, W, cin, cout, _lib.stream_ptr()), "ph_conv_cl_bwd_weight")
    return dw, db


def resnet_fold_bwd(dwp, db, w, gamma, mean, var, eps, dw, dgamma, dbeta, k, cin, cout):
    """(dW', db) of a folded convolution -> dw (w's shape), dgamma, dbeta (either None: not wanted)"""
    _lib.check(_lib.load().ph_resnet_fold_bwd(_lib.ptr(dwp), _lib.ptr(db), _lib.ptr(w), _lib.ptr(gamma), _lib.ptr(mean), _lib.ptr(var),
                                              float(eps), _lib.ptr(dw), _lib.ptr(dgamma), _lib.ptr(dbeta), k, cin, cout, _lib.stream_ptr()),
               "ph_resnet_fold_bwd")


def conv_cl_pack_bwd(wp, wt, k, cin, cout):
    """a convolution's forward pack wp -> the data gradient's operand wt (int16, the same number of elements)"""
    _lib.check(_lib.load().ph_conv_cl_pack_bwd(_lib.ptr(wp), _lib.ptr(wt), k, cin, cout, _lib.stream_ptr()), "ph_conv_cl_pack_bwd")
    return wt


def nchw_grad_to_cl(g, add, mask, out, B, HW, C_):
    """a stage's fp32 NCHW gradient g (+ the bf16 plane add) -> the bf16 channels-last plane out, zero where the plane mask is <= 0"""
    _lib.check(_lib.load().ph_nchw_grad_to_cl(_lib.ptr(g), _lib.ptr(add), _lib.ptr(mask), _lib.ptr(out), B, HW, C_, _lib.stream_ptr()),
               "ph_nchw_grad_to_cl")
    return out


def native_resnet_pack_bwd(pack):
    """the data-gradient operands of a NativeResNetPack (bf16), packed on the device by ph_resnet_pack_bwd -> {convolution index in
    state_dict order: its int16 view}"""
    lib, ref = _lib.load(), C.byref(pack.cfg)
    nbytes = lib.ph_resnet_pack_bwd_bytes(ref)
    if nbytes == 0:
        raise _cfg_error("ph_resnet_pack_bwd_bytes")
    lay = _lib.ResNetLayout()
    _lib.check(lib.ph_resnet_pack_bwd_layout(ref, C.byref(lay)), "ph_resnet_pack_bwd_layout")
    blob = torch.empty((nbytes,), dtype=torch.uint8, device=pack.blob.device)
    with torch.cuda.device(blob.device):
        _lib.check(lib.ph_resnet_pack_bwd(ref, _lib.ptr(pack.blob), _lib.ptr(blob), _lib.stream_ptr()), "ph_resnet_pack_bwd")
    return {c: _pack_piece(blob, lay, 2 * c, torch.int16, (-1,)) for c in range(lay.nconvs) if lay.bytes[2 * c]}


def resnet_conv_index(blocks):
    """{(stage, block, name): index of the convolution in state_dict order} (the stem is 0) of a block table"""
    out, n = {}, 1
    for si, stage in enumerate(blocks):
        for j, (_, _, _, has_down) in enumerate(stage):
            for name in ("conv1", "conv2", "conv3") + (("downsample",) if has_down else ()):
                out[(si, j, name)] = n
                n += 1
    return out


def resnet_train_sizes(B, H, W, blocks, first_trained):
    """the element counts engine.ResNetTrainPlan allocates, from the sizes alone (no device): dict(frozen_io, frozen_inner, frozen_down:
    the shared planes of the stages in front of `first_trained`; kept: the a1 + a2 + y (+ downsample) planes of every trained block;
    grad_io / grad_inner / grad_down: the backward's planes; wmax: floats of the largest dW'; layers: per trained convolution
    (stage, block, name, k, s, cin, cout, h, w) in forward order), all per plan, B included"""
    h, w = stem_out_size(H), stem_out_size(W)
    z = dict(stem=B * h * w * 64, frozen_io=0, frozen_inner=0, frozen_down=0, kept=0, grad_io=0, grad_inner=0, grad_down=0, wmax=0, layers=[])
    for si, stage in enumerate(blocks):
        for j, (cin, planes, s, has_down) in enumerate(stage):
            ho, wo = conv_out_size(h, 3, s), conv_out_size(w, 3, s)
            a1, a2, y = B * h * w * planes, B * ho * wo * planes, B * ho * wo * 4 * planes
            if si < first_trained:
                z["frozen_inner"] = max(z["frozen_inner"], a1, a2)
                z["frozen_io"] = max(z["frozen_io"], y)
                z["frozen_down"] = max(z["frozen_down"], y if has_down else 0)
            else:
                z["kept"] += a1 + a2 + y + (y if has_down else 0)
                z["grad_inner"] = max(z["grad_inner"], a1, a2)
                z["grad_io"] = max(z["grad_io"], y, B * h * w * cin if (si, j) != (first_trained, 0) else 0)
                if has_down and si > first_trained:
                    z["grad_down"] = max(z["grad_down"], B * ho * wo * cin)
                for name, k, st, ci, co, hh, ww in (("conv1", 1, 1, cin, planes, h, w), ("conv2", 3, s, planes, planes, h, w),
                                                    ("conv3", 1, 1, planes, 4 * planes, ho, wo)) + \
                        ((("downsample", 1, s, cin, 4 * planes, h, w),) if has_down else ()):
                    z["layers"].append((si, j, name, k, st, ci, co, hh, ww))
                    z["wmax"] = max(z["wmax"], co * k * k * ci)
            h, w = ho, wo
    return z


class ResNetTrainPlan:
    """forward + backward of resnet.ResNet's trained stages for one (B, H, W, block structure), grade bf16: the forward is ResNetPlan's
    launch sequence with the a1, a2 and y planes (and the downsample plane) of every block of a trained stage kept in planes of their
    own -- the frozen stages in front share ResNetPlan's ping-pong planes --; the backward runs from the last block down to the first
    block of stage `first_trained` on gradient planes of its own (two block-gradient planes, two inner ones, one for a downsample's
    low-resolution input gradient), with one dW' / db buffer and one partial-sum scratch for every weight gradient, and writes the
    parameter gradients into `self.grads`.  Everything is sized here; `forward` and `backward` issue launches on the current stream and
    neither allocate nor synchronise.  `nbytes`: the device memory the plan holds."""

    def __init__(self, B, H, W, blocks, out_indices, first_trained, device, stage_dtype=torch.float32):
        if not 1 <= first_trained <= 3:
            raise _lib.PolyheadError("ResNetTrainPlan: first_trained must lie in [1, 3] (the stem and layer1 have no backward)")
        lib, dev = _lib.load(), torch.device(device)
        self.B, self.H, self.W, self.first_trained, self.device, self.prec = B, H, W, first_trained, dev, _lib.PH_PREC_BF16
        self.blocks, self.out_indices = [list(s) for s in blocks], tuple(out_indices)
        self.index = resnet_conv_index(self.blocks)
        z = self.sizes = resnet_train_sizes(B, H, W, self.blocks, first_trained)
        self._tensors = []

        def e(n, dtype=torch.int16):
            t = torch.empty((max(int(n), 8),), dtype=dtype, device=dev)
            self._tensors.append(t)
            return t
        self.p0, self.pa, self.pb = e(z["stem"]), e(z["frozen_io"]), e(z["frozen_io"])
        self.t1, self.t2, self.pd = e(z["frozen_inner"]), e(z["frozen_inner"]), e(z["frozen_down"])
        h, w = stem_out_size(H), stem_out_size(W)
        self.kept, self.stage_shapes, self.geo = {}, [], {}
        for si, stage in enumerate(self.blocks):
            for j, (cin, planes, s, has_down) in enumerate(stage):
                ho, wo = conv_out_size(h, 3, s), conv_out_size(w, 3, s)
                self.geo[(si, j)] = (h, w, ho, wo)
                if si >= first_trained:
                    self.kept[(si, j)] = dict(a1=e(B * h * w * planes), a2=e(B * ho * wo * planes), y=e(B * ho * wo * 4 * planes),
                                              d=e(B * ho * wo * 4 * planes) if has_down else None)
                if not has_down and (cin, s) != (4 * planes, 1):
                    raise _lib.PolyheadError("ResNetTrainPlan: a block without downsample must keep its shape")
                h, w = ho, wo
            self.stage_shapes.append((4 * stage[-1][1], h, w))
        self.outs = {i: e(B * self.stage_shapes[i][0] * self.stage_shapes[i][1] * self.stage_shapes[i][2], stage_dtype)
                     .view((B,) + self.stage_shapes[i]) for i in self.out_indices}
        # backward
        self.ga, self.gb, self.d1, self.d2, self.dt = e(z["grad_io"]), e(z["grad_io"]), e(z["grad_inner"]), e(z["grad_inner"]), e(z["grad_down"])
        self.dwp, self.dbp = e(z["wmax"], torch.float32), e(2048, torch.float32)
        self.nsplit, pmax = {}, 0
        for (si, j, name, k, s, ci, co, hh, ww) in z["layers"]:
            n = lib.ph_conv_cl_bwd_weight_nsplit(k, s, ci, co, hh, ww, B)
            if n <= 0:
                _lib.check(n if n < 0 else _lib.PH_EINVAL, "ph_conv_cl_bwd_weight_nsplit")
            self.nsplit[(si, j, name)] = n
            pmax = max(pmax, lib.ph_conv_cl_bwd_weight_partial_floats(k, s, ci, co, hh, ww, B, n))
        self.partial = e(pmax, torch.float32)
        self.zero_grads = {si: e(B * c * hh * ww, torch.float32).zero_().view(B, c, hh, ww)
                           for si, (c, hh, ww) in enumerate(self.stage_shapes) if si >= first_trained}
        self.grads = {}
        for (si, j, name, k, s, ci, co, hh, ww) in z["layers"]:
            self.grads[(si, j, name)] = (e(co * ci * k * k, torch.float32).view(co, ci, k, k), e(co, torch.float32)[:co], e(co, torch.float32)[:co])
        self.nbytes = sum(t.numel() * t.element_size() for t in self._tensors)
        self.generation = 0

    def forward(self, x, pk):
        """x: [B, 3, H, W] fp32 / bf16 contiguous on the plan's device; pk: the forward pack (resnet.ResNet._pack's dict).  Returns the
        NCHW stages of out_indices: the plan's buffers, and the bits of ResNetPlan.run"""
        B, prec = self.B, self.prec
        if tuple(x.shape) != (B, 3, self.H, self.W) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous() \
                or x.device != self.device:
            raise _lib.PolyheadError(f"ResNetTrainPlan.forward: x must be a contiguous fp32 / bf16 device tensor of shape {(B, 3, self.H, self.W)}")
        self.generation += 1
        resnet_stem(x, pk["stem"][0], pk["stem"][1], self.p0, prec)
        cur, nxt = self.p0, self.pa
        self.inputs = {}
        for si, stage in enumerate(self.blocks):
            for j, (cin, planes, s, has_down) in enumerate(stage):
                c, (h, w, ho, wo) = pk["blocks"][si][j], self.geo[(si, j)]
                kp = self.kept.get((si, j))
                t1, t2, pd, y = (kp["a1"], kp["a2"], kp["d"], kp["y"]) if kp else (self.t1, self.t2, self.pd, nxt)
                self.inputs[(si, j)] = cur
                conv_cl(cur, c["conv1"][0], c["conv1"][1], None, t1, 1, 1, True, B, h, w, cin, planes, prec)
                conv_cl(t1, c["conv2"][0], c["conv2"][1], None, t2, 3, s, True, B, h, w, planes, planes, prec)
                idn = cur
                if has_down:
                    idn = conv_cl(cur, c["downsample"][0], c["downsample"][1], None, pd, 1, s, False, B, h, w, cin, 4 * planes, prec)
                conv_cl(t2, c["conv3"][0], c["conv3"][1], idn, y, 1, 1, True, B, ho, wo, planes, 4 * planes, prec)
                cur, nxt = y, (self.pb if nxt is self.pa else self.pa)
            if si in self.outs:
                c_, hh, ww = self.stage_shapes[si]
                cl_to_nchw(cur, self.outs[si], B, hh * ww, c_, prec)
        return tuple(self.outs[i] for i in self.out_indices)

    def backward(self, stage_grads, wt, params):
        """stage_grads: {stage: fp32 contiguous [B, C, h, w] gradient} for the trained stages (a missing one is zeros); wt: the transposed
        packs by convolution index (native_resnet_pack_bwd); params: {(stage, block, name): (w, gamma, mean, var, eps, want_bn)} fp32
        device tensors of every trained convolution.  Fills and returns self.grads: {(stage, block, name): (dw, dgamma, dbeta)}"""
        B, ft = self.B, self.first_trained
        cur, nxt = self.ga, self.gb

        def ingest(si, add):
            c_, hh, ww = self.stage_shapes[si]
            g = stage_grads.get(si)
            g = self.zero_grads[si] if g is None else g
            if tuple(g.shape) != (B, c_, hh, ww) or g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device:
                raise _lib.PolyheadError(f"ResNetTrainPlan.backward: stage {si}'s gradient must be a contiguous fp32 tensor of shape {(B, c_, hh, ww)}")
            return nchw_grad_to_cl(g, add, self.kept[(si, len(self.blocks[si]) - 1)]["y"], cur, B, hh * ww, c_)

        def wgrad(key, dz, x, k, s, h, w, ci, co):
            conv_cl_bwd_weight(dz, x, self.dwp, self.dbp, self.partial, self.nsplit[key], k, s, B, h, w, ci, co)
            wp, gamma, mean, var, eps, want_bn = params[key]
            dw, dg, dbt = self.grads[key]
            resnet_fold_bwd(self.dwp, self.dbp, wp, gamma, mean, var, eps, dw, dg if want_bn else None, dbt if want_bn else None, k, ci, co)

        top = len(self.blocks) - 1
        ingest(top, None)
        for si in range(top, ft - 1, -1):
            for j in range(len(self.blocks[si]) - 1, -1, -1):
                cin, planes, s, has_down = self.blocks[si][j]
                (h, w, ho, wo), kp, x, ix = self.geo[(si, j)], self.kept[(si, j)], self.inputs[(si, j)], self.index
                need_dx = (si, j) != (ft, 0)
                g = cur
                conv_cl_bwd_data(g, wt[ix[(si, j, "conv3")]], None, 1, kp["a2"], self.d2, 1, 1, B, ho, wo, planes, 4 * planes)
                wgrad((si, j, "conv3"), g, kp["a2"], 1, 1, ho, wo, planes, 4 * planes)
                if has_down:
                    wgrad((si, j, "downsample"), g, x, 1, s, h, w, cin, 4 * planes)
                    if need_dx:                                   # the 1x1 layer on the pixels it sampled: a stride-1 layer at ho x wo
                        conv_cl_bwd_data(g, wt[ix[(si, j, "downsample")]], None, 1, None, self.dt, 1, 1, B, ho, wo, cin, 4 * planes)
                conv_cl_bwd_data(self.d2, wt[ix[(si, j, "conv2")]], None, 1, kp["a1"], self.d1, 3, s, B, h, w, planes, planes)
                wgrad((si, j, "conv2"), self.d2, kp["a1"], 3, s, h, w, planes, planes)
                wgrad((si, j, "conv1"), self.d1, x, 1, 1, h, w, cin, planes)
                if not need_dx:
                    continue
                if has_down:                                      # the stage's first block: dL/dx unmasked, then the stage in front
                    conv_cl_bwd_data(self.d1, wt[ix[(si, j, "conv1")]], self.dt, s, None, nxt, 1, 1, B, h, w, cin, planes)
                    ingest(si - 1, nxt)
                else:
                    conv_cl_bwd_data(self.d1, wt[ix[(si, j, "conv1")]], g, 1, x, nxt, 1, 1, B, h, w, cin, planes)
                    cur, nxt = nxt, cur
        return self.grads
