"""ctypes binding of libpolyhead.so (include/polyhead.h).  The library is the ONLY compute path:
if it is missing or fails to load this module raises -- there is no CPU or PyTorch fallback."""
import contextlib
import ctypes as C
import os

import torch  # noqa: F401  -- MUST precede dlopen: libpolyhead has to bind to the HIP runtime torch loaded

from . import knobs

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpolyhead.so")
if knobs.get("PH_ALT_LIB"):           # measurement aid: a variant build (tools/build_variant.py) for same-box A/B timing
    LIB_PATH = os.path.abspath(knobs.get("PH_ALT_LIB"))

PH_PREC_BF16, PH_PREC_BF16_KSPLIT, PH_PREC_SPLIT, PH_PREC_F16, PH_PREC_BF16_KF16, PH_PREC_QHYBRID = 1, 2, 3, 5, 6, 7
PH_PLANES_C16 = 0x100            # flag on `prec` of ph_nhwc_ingest / ph_conv_nhwc: chunk-major planes [B][16][HW][16] (polyhead.h)
PH_QUERY_WIDE = 0x100            # ph_query_stage phases flag: most rows per workgroup (launches that share the GPU)
PH_QUERY_MASK_ONLY, PH_QUERY_DEPTH_ONLY = 0x200, 0x400      # ... one branch's half of the launch
PH_OUT_F32, PH_OUT_BF16, PH_OUT_F16 = 0, 1, 2
PH_KERN_BF16_PLANES, PH_KERN_F16 = 0, 1
PH_GN_TO_PLANES, PH_GN_UP2_PLANES, PH_GN_ACCUM, PH_GN_TO_NCHW, PH_GN_TO_CPLANES = 0, 1, 2, 3, 4
PH_IN_F32_NCHW, PH_IN_PLANES = 0, 1

# the library's switches (polyhead.h PH_SWITCH_*): position = id; `switches` below sets them by these names
SWITCHES = ("conv_wgs", "up2_wgs", "query_nrt", "query_timeline", "conv_tile_rows", "gnsum_wgs", "cplanes_tpw", "pan_generic")

W_NAMES = ["DYN", "INP", "IG", "UG", "FC", "QKV", "OUT", "FFN1", "FFN2", "H0A", "H0B", "CLS", "KERN"]
V_NAMES = ["DYN_CNT", "DYN_B", "INP_B", "IG_B", "UG_B", "LN_IG_G", "LN_IG_B", "LN_UG_G", "LN_UG_B",
           "LN_PO_G", "LN_PO_B", "LN_IO_G", "LN_IO_B", "FC_B", "LN_FC_G", "LN_FC_B", "QKV_B", "OUT_B",
           "LN_ATT_G", "LN_ATT_B", "FFN1_B", "FFN2_B", "LN_FFN_G", "LN_FFN_B", "LN_H0A_G", "LN_H0A_B",
           "LN_H0B_G", "LN_H0B_B", "CLS_B", "KERN_B"]
W_IDX = {n: i for i, n in enumerate(W_NAMES)}
V_IDX = {n: i for i, n in enumerate(V_NAMES)}


class StageLayout(C.Structure):
    _fields_ = [("w", (C.c_int64 * len(W_NAMES)) * 2), ("v", (C.c_int64 * len(V_NAMES)) * 2),
                ("wb_plane_elems", C.c_int64), ("ffn_dim", C.c_int32), ("num_classes", C.c_int32)]


# the native decode plan (polyhead.h ph_decode_*)
PH_MODE = {"fp32": 0, "split": 0, "mixed": 1, "mixed16": 2, "fp16": 3, "bf16": 4}
PH_KNOB_AUTO, PH_KNOB_ON, PH_KNOB_OFF, PH_KNOB_WHERE_SUPPORTED = 0, 1, 2, 3
PH_FEAT_F32, PH_FEAT_16, PH_FEAT_PLANES = 0, 1, 2
PH_DECODE_NPARAMS = 83


class DecodeCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "N", "H", "W", "S", "L", "F", "mode", "out_dtype", "frame_invariant", "query_full_split",
                                          "shares_gpu", "poolx", "fused_up", "nsplit", "nsplit_px", "up2_wgs")]


class DecodeGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nsplit", "nsplit_px", "poolx", "fused_up", "up2_workgroups", "feat_prec", "query_prec",
                                          "conv_prec", "kern_format", "feat_planes")]


class DecodeIO(C.Structure):
    _fields_ = [("feat_format", C.c_int32), ("m0_dtype", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("x", "depth_feats", "k0", "q0", "m0", "bits", "obj", "dobj", "cls", "mask", "mask_up", "depth_up",
                                   "depth")]


# the native KernelHead plan (polyhead.h ph_khead_cfg .. ph_khead_plan_timeouts)
PH_KHEAD_NPARAMS = 14
KPACK_PIECES = ("wplanes", "gn", "init_planes", "seg_planes", "dd_planes", "seg_bias", "dd_bias", "init_frag", "seg_frag", "dd_frag",
                "conv_frag", "w_init_f32", "w_seg_f32", "w_dd_f32")        # PH_KPACK_*; engine.KernelHeadPack's attribute names
PH_KPACK_COUNT = len(KPACK_PIECES)


class KheadCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "num_proposals", "num_classes", "num_thing_classes", "cat_stuff", "groups",
                                          "mode", "logit_dtype", "emit_f32", "frame_invariant", "onepass", "nsplit")]


class KheadLayout(C.Structure):
    _fields_ = [("offset", C.c_uint64 * PH_KPACK_COUNT), ("bytes", C.c_uint64 * PH_KPACK_COUNT)]


class KheadGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("onepass", "nsplit", "N", "Npad", "HWp", "P", "prec", "n_stuff")]


class KheadIO(C.Structure):
    _fields_ = [("input_format", C.c_int32), ("reserved", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("f0", "f1", "f2", "xp", "dp", "bits", "x_f32", "dfe_f32", "mask_preds", "seg_preds", "depth_pred",
                                   "proposal", "depth_proposal")]


# the native neck plan (polyhead.h ph_neck_cfg .. ph_neck_plan_run_outputs)
PH_NECK_NPARAMS = 30
PH_NECK_NCONVS = 10
PH_NPACK_OUTS_W, PH_NPACK_OUTS_GN, PH_NPACK_COUNT = 30, 31, 32      # pieces 3 c, 3 c + 1, 3 c + 2: wp, gamma, beta of conv c


class NeckCfg(C.Structure):
    _fields_ = [("B", C.c_int32), ("h", C.c_int32 * 4), ("w", C.c_int32 * 4)] + \
        [(n, C.c_int32) for n in ("groups", "mode", "num_outs", "pos_level", "emit_planes", "emit_f32", "fused_out", "c16",
                                  "tower_buffers")] + [("eps", C.c_float)]


class NeckLayout(C.Structure):
    _fields_ = [("offset", C.c_uint64 * PH_NPACK_COUNT), ("bytes", C.c_uint64 * PH_NPACK_COUNT)]


class NeckGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("Ho", "Wo", "HWp", "P", "prec", "fused_out", "c16", "tower_buffers", "nconvs")] + \
        [("tile_rows", C.c_int32 * PH_NECK_NCONVS)]


class NeckIO(C.Structure):
    _fields_ = [("feats", C.c_void_p * 4), ("posenc", C.c_void_p), ("out_planes", C.c_void_p * 3), ("out_f32", C.c_void_p * 3)]


# the native FPN plan (polyhead.h ph_fpn_cfg .. ph_fpn_plan_run); piece i of the pack is parameter i: lateral l weight 2 l, bias 2 l + 1,
# output conv l weight 8 + 2 l, bias 9 + 2 l
PH_FPN_NPARAMS = PH_FPACK_COUNT = 16


class FpnCfg(C.Structure):
    _fields_ = [("B", C.c_int32), ("k", C.c_int32 * 4), ("h", C.c_int32 * 4), ("w", C.c_int32 * 4)] + \
        [(n, C.c_int32) for n in ("mode", "x_dtype", "emit_f32", "emit_planes")]


class FpnLayout(C.Structure):
    _fields_ = [("offset", C.c_uint64 * PH_FPACK_COUNT), ("bytes", C.c_uint64 * PH_FPACK_COUNT)]


class FpnGeometry(C.Structure):
    _fields_ = [("P", C.c_int32), ("prec", C.c_int32), ("tile_rows", C.c_int32 * 4)]


class FpnIO(C.Structure):
    _fields_ = [("stages", C.c_void_p * 4), ("out_f32", C.c_void_p * 4), ("out_planes", C.c_void_p * 4), ("planes_layout", C.c_int32 * 4),
                ("add", C.c_void_p * 4)]


# the native backbone plan (polyhead.h ph_resnet_cfg .. ph_resnet_plan_run); convolution c of the depth's table owns parameters
# 5 c .. 5 c + 4 and pack pieces 2 c (W) and 2 c + 1 (b)
PH_RESNET_MAX_CONVS = 155


class ResNetCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "depth", "mode", "x_dtype", "out_dtype", "out_mask")] + [("eps", C.c_double)]


class ResNetLayout(C.Structure):
    _fields_ = [("offset", C.c_uint64 * (2 * PH_RESNET_MAX_CONVS)), ("bytes", C.c_uint64 * (2 * PH_RESNET_MAX_CONVS)),
                ("nconvs", C.c_int32), ("reserved", C.c_int32)]


class ResNetGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("prec", "launches", "nconvs", "stem_workgroups")] + \
        [(n, C.c_int32 * 4) for n in ("c", "h", "w", "nchw_workgroups")] + [("conv_workgroups", C.c_int32 * PH_RESNET_MAX_CONVS)]


class ResNetIO(C.Structure):
    _fields_ = [("image", C.c_void_p), ("stages", C.c_void_p * 4)]


# the native association plan (polyhead.h ph_track_cfg .. ph_assoc_plan_match)
PH_TRACK_MAX_CONVS = 8
PH_TPACK_FC, PH_TPACK_FC_B, PH_TPACK_EMB, PH_TPACK_EMB_B, PH_TPACK_COUNT = 24, 25, 26, 27, 28     # conv i, gamma 8 + i, beta 16 + i


class TrackCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_convs", "fc_out_channels", "embed_channels", "groups", "prec")] + [("eps", C.c_float)]


class TrackLayout(C.Structure):
    _fields_ = [("offset", C.c_uint64 * PH_TPACK_COUNT), ("bytes", C.c_uint64 * PH_TPACK_COUNT)]


class AssocCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "Ho", "Wo", "K", "max_things", "num_thing_classes", "num_stuff_classes", "nlev")] + \
        [("h", C.c_int32 * 4), ("w", C.c_int32 * 4), ("inv_stride", C.c_float * 4), ("finest_scale", C.c_float), ("track", TrackCfg)]


class AssocGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("things_words", "P", "conv_splits", "conv_steps", "fc_splits", "fc_steps", "emb_splits",
                                          "emb_steps", "vec8", "reserved")] + [(n, C.c_uint64) for n in ("staging_bytes", "rois_offset", "roi_planes_offset")]


class AssocIO(C.Structure):
    _fields_ = [("pan", C.c_void_p), ("seg_records", C.c_void_p), ("levels", C.c_void_p * 4), ("level_stride", C.c_int64 * 4),
                ("sem_out", C.c_void_p), ("things_out", C.c_void_p), ("embeds_out", C.c_void_p), ("roi_planes", C.c_void_p)]


# the device tracker (polyhead.h ph_dtracker_* .. ph_assoc_plan_track); ph_tracker_cfg is the host tracker's too
PH_DTRK_OK, PH_DTRK_EPOOL, PH_DTRK_EREFUSED, PH_DTRK_ECOUNT = 0, 1, 2, 3
DTRK_STATUS = ("matched", "num_tracklets", "rows", "error", "refused_frame", "frame_id", "free", "frames_seen")     # PH_DTRK_ST_*
PH_DTRK_ST_WORDS = len(DTRK_STATUS)


class TrackerCfg(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("init_score_thr", "obj_score_thr", "match_score_thr", "memo_momentum", "one_minus_momentum",
                                         "nms_conf_thr", "nms_backdrop_iou_thr", "nms_class_iou_thr")] + \
        [(n, C.c_int32) for n in ("memo_tracklet_frames", "memo_backdrop_frames", "with_cats", "metric")]


class DtrackerLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("pool", "trk_id", "trk_seen", "trk_label", "trk_slot", "trk_box", "bd_count", "bd_label", "bd_slot",
                                          "bd_box", "free_stack", "status", "workspace", "total_bytes")] + \
        [(n, C.c_int32) for n in ("capacity", "max_dets", "generations", "reserved")]


class DtrackerIO(C.Structure):
    _fields_ = [("boxes", C.c_void_p), ("box_stride", C.c_int64), ("labels", C.c_void_p), ("label_stride", C.c_int64),
                ("counts", C.c_void_p), ("count_stride", C.c_int64), ("refuse", C.c_void_p), ("refuse_stride", C.c_int64),
                ("embeds", C.c_void_p), ("embed_stride", C.c_int64), ("kept_out", C.c_void_p), ("ids_out", C.c_void_p),
                ("kept_counts", C.c_void_p)]


# DVPQ tallies on the device (polyhead.h ph_dvpq_cfg .. ph_dvpq_frames)
PH_DVPQ_MAX_THR = 8


class DvpqCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "capacity", "nthr")] + [("thr", C.c_float * PH_DVPQ_MAX_THR)]


class DvpqIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pred_panseg", "pred_sem", "pred_track", "pred_depth", "gt_panseg", "gt_depth", "table_out",
                                          "depth_out")]


# the training step's assignment + descriptors on the device (polyhead.h ph_assign_cfg .. ph_assign_desc)
PH_ASSIGN_MAX, PH_ASSIGN_MAX_B, PH_ASSIGN_GT_WORDS = 256, 64, 8
PH_ASSIGN_OK, PH_ASSIGN_ENONFINITE, PH_ASSIGN_ESOLVE = 0, 1, 2
PH_EUNSUPPORTED = -2
ASSIGN_SECTIONS = ("tptr", "wptr", "labels", "pos_u8", "pos_rows", "dstart", "dit_t", "dit_w", "dit_s", "label_w", "sstart", "sit_m", "sit_l")


class AssignCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "Np", "N", "L", "n_thing", "n_stuff", "roi", "has_sem", "has_depth")] + \
        [("pos_weight", C.c_float), ("HW", C.c_int64)]


class AssignLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ASSIGN_SECTIONS + ("total_bytes",)] + \
        [(n, C.c_int64) for n in ("P", "depth_items", "seg_items", "depth_rows")]


# the training path's losses from descriptors (polyhead.h ph_loss_cfg, ph_train_losses)
class LossCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "N", "L", "P", "depth_rows", "seg_L", "has_rank", "ignore", "depth_mode")] + \
        [("HW", C.c_int64)] + \
        [(n, C.c_float) for n in ("lw_mask", "lw_dice", "dice_eps", "lw_rank", "lw_depth", "dw_si", "dw_sq", "dw_abs", "lw_cls",
                                  "cls_gamma", "cls_alpha", "cls_avg", "lw_seg", "seg_gamma", "seg_alpha")]


# the track head's training losses (polyhead.h ph_track_loss_cfg, ph_track_loss)
PH_TRACK_LOSS_MAX_ROIS, PH_TRACK_LOSS_MAX_PAIRS = 128, 64


# the RoIs of the sampled ground-truth masks (polyhead.h ph_gtmask_boxes)
PH_GTBOX_MAX_FRAMES, PH_GTBOX_BILINEAR, PH_GTBOX_NEAREST = 64, 0, 1
# the step's ground truth from segment-index maps (polyhead.h ph_gt_prepare)
PH_GTPREP_MAX_FRAMES, PH_GTPREP_MAX_SEGMENTS = 64, 254
# the index maps from the dataset's panoptic id maps (polyhead.h ph_gt_segments, ph_gt_index_maps)
PH_GTSEG_MAX_KEYS, PH_GTSEG_ROW_WORDS, PH_GTSEG_TABLE_WORDS = 262144, 6, 1 + 254 * 6
PH_GTSEG_I32, PH_GTSEG_U16 = 0, 1
PH_GTSEG_ETOOMANY, PH_GTSEG_EUNMAPPED, PH_GTSEG_EOUTSIDE = 1, 2, 4
PH_EINVAL, PH_EWORKSPACE = -1, -4
# the image of the frame from the file's bytes (polyhead.h ph_image_prepare); its out_dtype is PH_OUT_F32 / PH_OUT_BF16
PH_IMGPREP_MAX_FRAMES = 64
PH_IMG_NCHW, PH_IMG_NHWC = 0, 1


class TrackLossCfg(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("E", C.c_int32), ("lw_track", C.c_float), ("lw_aux", C.c_float), ("neg_pos_ub", C.c_int32),
                ("pos_margin", C.c_float), ("neg_margin", C.c_float), ("hard_mining", C.c_int32)]


# the optimizer step (polyhead.h ph_optim_tensor .. ph_optim_zero_grads)
PH_OPTIM_CHUNK, PH_OPTIM_MAX_TENSORS = 4096, 4096
PH_OPTIM_SKIP_NONFINITE, PH_OPTIM_ZERO_GRADS = 1, 2
PH_OPTIM_OK, PH_OPTIM_ENONFINITE = 0, 1


class OptimTensor(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("p", "g", "m", "v")] + [("n", C.c_int64), ("lr", C.c_double), ("weight_decay", C.c_double),
                                                                  ("first_item", C.c_int64)]


class OptimCfg(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("beta1", "beta2", "eps", "max_norm")] + [("flags", C.c_int32), ("max_blocks", C.c_int32)]


class OptimState(C.Structure):
    _fields_ = [("step", C.c_int64), ("skipped", C.c_int64), ("status", C.c_int32), ("skip", C.c_int32)] + \
        [(n, C.c_float) for n in ("grad_norm", "clip_coef", "bias1", "bias2_sqrt")]


# C typedef name -> its mirror above: every Structure of this module (tests/test_abi.py compares each layout with the header's)
STRUCTS = {"ph_stage_layout": StageLayout, "ph_decode_cfg": DecodeCfg, "ph_decode_geometry": DecodeGeometry, "ph_decode_io": DecodeIO,
           "ph_khead_cfg": KheadCfg, "ph_khead_layout": KheadLayout, "ph_khead_geometry": KheadGeometry, "ph_khead_io": KheadIO,
           "ph_neck_cfg": NeckCfg, "ph_neck_layout": NeckLayout, "ph_neck_geometry": NeckGeometry, "ph_neck_io": NeckIO,
           "ph_fpn_cfg": FpnCfg, "ph_fpn_layout": FpnLayout, "ph_fpn_geometry": FpnGeometry, "ph_fpn_io": FpnIO,
           "ph_resnet_cfg": ResNetCfg, "ph_resnet_layout": ResNetLayout, "ph_resnet_geometry": ResNetGeometry, "ph_resnet_io": ResNetIO,
           "ph_track_cfg": TrackCfg, "ph_track_layout": TrackLayout, "ph_assoc_cfg": AssocCfg, "ph_assoc_geometry": AssocGeometry,
           "ph_assoc_io": AssocIO, "ph_tracker_cfg": TrackerCfg, "ph_dtracker_layout": DtrackerLayout, "ph_dtracker_io": DtrackerIO,
           "ph_dvpq_cfg": DvpqCfg, "ph_dvpq_io": DvpqIO, "ph_assign_cfg": AssignCfg, "ph_assign_layout": AssignLayout,
           "ph_loss_cfg": LossCfg, "ph_track_loss_cfg": TrackLossCfg, "ph_optim_tensor": OptimTensor, "ph_optim_cfg": OptimCfg,
           "ph_optim_state": OptimState}

# name -> (restype, argtypes); every symbol include/polyhead.h declares
_P, _I, _L, _Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
SIGNATURES = {
    "ph_version": (C.c_int, []),
    "ph_last_error_string": (C.c_char_p, []),
    "ph_set_switch": (C.c_int, [_I, _I]),
    "ph_get_switch": (C.c_int, [_I, C.POINTER(C.c_int)]),
    "ph_ingest_features": (C.c_int, [_P, _P, _I, _L, _I, _P]),
    "ph_binarize": (C.c_int, [_P, _L, _P, _I, _I, _L, _P]),
    "ph_pool": (C.c_int, [_P, _P, _P, _P, _I, _I, _L, _I, _I, _P]),
    "ph_pool_rows": (C.c_int, [_P, _P, _P, _I, _P, _I, _I, _L, _I, _I, _P]),
    "ph_pool_counts": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _L, _I, _I, _P]),
    "ph_pool_default_nsplit": (C.c_int, [_I, _L, _I]),
    "ph_query_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "ph_query_stage": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, C.POINTER(StageLayout), _P, _P, _P, _I, _P, _P,
                                 _P, _Z, _I, _I, _L, _I, _I, _I, _P]),
    "ph_query_stage_counts": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, C.POINTER(StageLayout), _P, _P, _P, _I, _P, _P,
                                        _P, _Z, _I, _I, _L, _I, _I, _I, _P]),
    "ph_query_workspace_updator_offset": (C.c_size_t, [_I, _I, _I]),
    "ph_dynconv": (C.c_int, [_P, _P, _L, _L, _P, _L, _P, _P, _I, _L, _I, _I, _L, _I, _P]),
    "ph_khead_workspace_bytes": (C.c_size_t, [_I, _L, _I]),
    "ph_khead_conv_gn": (C.c_int, [_P, _P, _P, _P, _P, _I, C.c_float, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _L, _I, _P]),
    "ph_khead_fused": (C.c_int, [_P, _P, _P, _P, _P, _I, C.c_float, _P, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P,
                                 _P, _P, _P, _P, _Z, _I, _L, _I, _I, _P]),
    "ph_khead_onepass_supported": (C.c_int, [_I, _L, _I, _I, _I]),
    "ph_khead_onepass_workspace_bytes": (C.c_size_t, [_I, _L]),
    "ph_khead_onepass": (C.c_int, [_P, _P, _P, _P, _P, _I, C.c_float, _P, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P,
                                   _P, _P, _P, _I, _P, _I, _P, _Z, _I, _L, _I, _I, _P]),
    "ph_khead_onepass_status": (C.c_int, [_P, _I, _P]),
    "ph_khead_onepass_timeouts": (C.c_int, [_P, _I, _L, _P]),
    "ph_khead_onepass_set_timeout_us": (None, [_I]),
    "ph_khead_fused_if": (C.c_int, [_P, _P, _P, _P, _P, _I, C.c_float, _P, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P,
                                    _P, _P, _P, _I, _P, _P, _Z, _I, _L, _I, _I, _P]),
    "ph_binarize_if": (C.c_int, [_P, _I, _L, _P, _I, _I, _L, _P, _P]),
    "ph_selftest_hog": (C.c_int, [_I, _I, _I, _P, _P]),
    "ph_khead_onepass_set_timeline": (None, [_P]),
    "ph_khead_proposals": (C.c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "ph_match_record_floats": (C.c_int64, [_I, _I]),
    "ph_match_nsplit": (C.c_int, [_L, _I]),
    "ph_match_sums": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _P]),
    "ph_upsample2x": (C.c_int, [_P, _P, _I, _L, _I, _I, _P]),
    "ph_dynconv_poolx_supported": (C.c_int, [_I, _I]),
    "ph_pool_depth_pair_supported": (C.c_int, [_I, _I]),
    "ph_pool_depth_pair": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _L, _I, _I, _P]),
    "ph_dynconv_poolx": (C.c_int, [_P, _P, _L, _P, _L, _P, _P, _I, _I, _I, _L, _I, _P]),
    "ph_dynconv_up2_supported": (C.c_int, [_I, _I, _I, _I, _I]),
    "ph_dynconv_up2": (C.c_int, [_P, _P, _L, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ph_dynconv_up2_wgs": (C.c_int, [_P, _P, _L, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ph_mask_loss_sums": (C.c_int, [_P, _P, _P, _P, _I, _L, _I, _P, _P]),
    "ph_mask_loss_grad": (C.c_int, [_P, _P, _P, _P, _I, _L, _P, _P, _P]),
    "ph_rank_loss_blocks": (C.c_int, [_L]),
    "ph_rank_loss_sum": (C.c_int, [_P, _P, _I, _I, _L, _I, _P, _P]),
    "ph_rank_loss_grad": (C.c_int, [_P, _P, _I, _I, _L, _I, C.c_float, _P, _P]),
    "ph_depth_loss_blocks": (C.c_int, [_L]),
    "ph_depth_loss_sums": (C.c_int, [_P, _P, _P, _L, _I, _P, _P]),
    "ph_depth_loss_grad": (C.c_int, [_P, _P, _P, _L, _I, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P]),
    "ph_focal_loss_blocks": (C.c_int, [_L]),
    "ph_focal_loss_sum": (C.c_int, [_P, _P, _P, _L, _I, C.c_float, C.c_float, _P, _P]),
    "ph_focal_loss_grad": (C.c_int, [_P, _P, _P, _L, _I, C.c_float, C.c_float, C.c_float, _P, _P]),
    "ph_seg_focal_sum": (C.c_int, [_P, _P, _I, _I, _L, C.c_float, C.c_float, _P, _P]),
    "ph_seg_focal_grad": (C.c_int, [_P, _P, _I, _I, _L, C.c_float, C.c_float, C.c_float, _P, _P]),
    "ph_rank_target": (C.c_int, [_P, _P, _I, _I, _L, _I, _P, _P]),
    "ph_seg_target": (C.c_int, [_P, _P, _I, _P, _P, _I, _I, _L, _P, _P]),
    "ph_depth_cost_sums": (C.c_int, [_P, _P, _P, _I, _I, _L, _I, C.c_float, _P, _P, _P]),
    "ph_rows_x_map": (C.c_int, [_P, _L, _I, _I, _I, _I, _P, _P, _I, _L, _I, _P]),
    "ph_map_x_map_t_nsplit": (C.c_int, [_I, _I, _L]),
    "ph_map_x_map_t": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _I, _I, _P]),
    "ph_upsample2x_bwd": (C.c_int, [_P, _P, _L, _I, _I, _P]),
    "ph_rows_x_map_ex": (C.c_int, [_P, _L, _I, _I, _I, _I, _P, _P, _I, _L, _I, _P, _P, _P]),
    "ph_map_x_map_t_ex": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _I, _I, _P, _P, _I, _P]),
    "ph_conv3x3_taps": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "ph_conv3x3_train": (C.c_int, [_P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ph_conv3x3_wgrad": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ph_gn_train_nsplit": (C.c_int, [_L, _I]),
    "ph_gn_train_bwd_nsplit": (C.c_int, [_L]),
    "ph_gn_train_fwd": (C.c_int, [_P, _P, _P, _I, C.c_float, _P, _P, _P, _P, _P, _I, _I, _L, _P]),
    "ph_gn_train_bwd": (C.c_int, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _L, _P]),
    "ph_hard_count": (C.c_int, [_P, _P, _L, _L, _P]),
    "ph_map_x_map_t_wide_nsplit": (C.c_int, [_I, _I, _I, _L]),
    "ph_map_x_map_t_wide": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _I, _P, _P, _I, _P]),
    "ph_nearest_up_add": (C.c_int, [_P, _P, _L, _I, _I, _I, _I, _P]),
    "ph_nearest_up_add_bwd": (C.c_int, [_P, _P, _L, _I, _I, _I, _I, _I, _P]),
    "ph_nchw_bias_add": (C.c_int, [_P, _P, _I, _I, _L, _P]),
    "ph_nchw_channel_sums_nsplit": (C.c_int, [_L]),
    "ph_nchw_channel_sums": (C.c_int, [_P, _P, _P, _I, _I, _L, _P]),
    "ph_train_losses_scratch_bytes": (C.c_size_t, [_P]),
    "ph_train_losses": (C.c_int, [_P] * 24 + [_Z, _P]),
    "ph_gemm32": (C.c_int, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    "ph_qtrain_saved_floats": (C.c_size_t, [_I, _I, _I, _I]),
    "ph_qtrain_scratch_floats": (C.c_size_t, [_I, _I, _I, _I]),
    "ph_qtrain_forward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ph_qtrain_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ph_panoptic_select": (C.c_int, [_P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
    "ph_panoptic_activate": (C.c_int, [_P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "ph_panoptic_argmax": (C.c_int, [_P, _P, _I, C.POINTER(C.c_int32), _I, _P, _P, _P]),
    "ph_panoptic_paste": (C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_int32), _I, _P, _P, _P, _P]),
    "ph_panoptic_accept": (C.c_int, [_P, _P, _P, _L, _I, _I, _I, C.c_double, C.c_double, _P, _L, _P, _P, _L, _P]),
    "ph_panoptic_activate_batch": (C.c_int, [_P, _P, _I, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "ph_panoptic_argmax_batch": (C.c_int, [_P, _P, _L, _I, _I, C.POINTER(C.c_int32), _I, _I, _P, _P, _L, _P]),
    "ph_panoptic_paste_batch": (C.c_int, [_P, _P, _L, _P, _P, _I, _I, C.POINTER(C.c_int32), _I, _P, _P, _P, _P]),
    "ph_panoptic_merge_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "ph_panoptic_merge": (C.c_int, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32), _I, C.c_double,
                                    C.c_double, _P, _Z, _P, _P, _P, _P, _P]),
    "ph_segment_boxes_workspace_bytes": (C.c_size_t, [_I]),
    "ph_segment_boxes": (C.c_int, [_P, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "ph_roi_align_fpn": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_float), _I, _P, _I, C.c_float,
                                   _P, _P, _I, _P]),
    "ph_gemm_rows": (C.c_int, [_P, _P, _L, _P, _I, _P, _P, _I, _I, _I, _I, _P]),
    "ph_track_affinity_workspace_bytes": (C.c_size_t, [_I, _I]),
    "ph_track_affinity": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "ph_im2col7": (C.c_int, [_P, _P, _I, _I, _P]),
    "ph_gemm_rows_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "ph_gemm_rows_splitk": (C.c_int, [_P, _I, _P, _L, _P, _I, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "ph_gn_relu_cl": (C.c_int, [_P, _P, _P, _I, C.c_float, _P, _I, _I, _P]),
    "ph_nhwc_ingest": (C.c_int, [_P, _P, _P, _I, _L, _I, _P]),
    "ph_conv_nhwc_partial_floats": (C.c_size_t, [_I, _I, _I]),
    "ph_conv_nhwc_workgroups_b": (C.c_int, [_I, _I, _I, _I, _I, _I]),
    "ph_conv_nhwc": (C.c_int, [_P, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ph_gn_finalize": (C.c_int, [_P, _P, _I, _I, _L, C.c_float, _I, _P]),
    "ph_gn_sum_planes": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                   _I, _I, _P, _I, _L, _I, _P]),
    "ph_neck_out_convs_workspace_bytes": (C.c_size_t, [_I, _L, _I]),
    "ph_neck_out_convs": (C.c_int, [_P, _I, _P, _P, _I, C.c_float, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _L, _I, _P]),
    "ph_gn_apply": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P]),
    "ph_fpn_lateral": (C.c_int, [_P, _I, _P, _L, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "ph_fpn_lateral_cl": (C.c_int, [_P, _I, _P, _L, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "ph_fpn_output": (C.c_int, [_P, _P, _P, _I, _L, _P]),
    "ph_fpn_output_planes": (C.c_int, [_P, _P, _P, _P, _P, _I, _L, _I, _P]),
    "ph_conv_cl_workgroups": (C.c_int, [_I, _I, _I, _I, _I, _I, _I]),
    "ph_conv_cl": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ph_resnet_stem_workgroups": (C.c_int, [_I, _I, _I]),
    "ph_resnet_stem": (C.c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ph_cl_to_nchw_workgroups": (C.c_int, [_I, _L, _I]),
    "ph_cl_to_nchw": (C.c_int, [_P, _P, _I, _I, _L, _I, _I, _P]),
    "ph_conv_cl_bwd_data_workgroups": (C.c_int, [_I, _I, _I, _I, _I, _I, _I]),
    "ph_conv_cl_bwd_data": (C.c_int, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ph_conv_cl_bwd_weight_nsplit": (C.c_int, [_I, _I, _I, _I, _I, _I, _I]),
    "ph_conv_cl_bwd_weight_partial_floats": (C.c_int64, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "ph_conv_cl_bwd_weight": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ph_resnet_fold_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_double, _P, _P, _P, _I, _I, _I, _P]),
    "ph_conv_cl_pack_bwd": (C.c_int, [_P, _P, _I, _I, _I, _P]),
    "ph_nchw_grad_to_cl": (C.c_int, [_P, _P, _P, _P, _I, _L, _I, _P]),
    "ph_tracker_device_bytes": (C.c_size_t, [_I, _I]),
    "ph_tracker_create": (C.c_void_p, [_P, _P, _Z, _I, _I]),
    "ph_tracker_destroy": (None, [_P]),
    "ph_tracker_reset": (None, [_P]),
    "ph_tracker_num_tracklets": (C.c_int64, [_P]),
    "ph_tracker_rows": (C.c_int, [_P]),
    "ph_tracker_debug_times": (None, [_P, _P]),
    "ph_tracker_match": (C.c_int, [_P, _P, _P, _P, _I, _L, _P, _P, _P]),
    "ph_tracker_match_frames": (C.c_int, [_P, _P, _P, _P, _P, _I, _L, _P, _P, _P, _P]),
    "ph_decode_param_name": (C.c_char_p, [_I]),
    "ph_decode_param_numel": (C.c_int64, [C.POINTER(DecodeCfg), _I]),
    "ph_decode_pack_bytes": (C.c_size_t, [C.POINTER(DecodeCfg)]),
    "ph_decode_pack_layout": (C.c_int, [C.POINTER(DecodeCfg), C.POINTER(StageLayout), C.POINTER(C.c_size_t)]),
    "ph_decode_pack_stage": (C.c_int, [C.POINTER(DecodeCfg), C.POINTER(C.c_void_p), _P, _P]),
    "ph_decode_workspace_bytes": (C.c_size_t, [C.POINTER(DecodeCfg)]),
    "ph_decode_create": (C.c_int, [C.POINTER(DecodeCfg), C.POINTER(C.c_void_p), _P, _Z, C.POINTER(C.c_void_p)]),
    "ph_decode_info": (C.c_int, [_P, C.POINTER(DecodeGeometry)]),
    "ph_decode_geometry_of": (C.c_int, [C.POINTER(DecodeCfg), C.POINTER(DecodeGeometry)]),
    "ph_decode_destroy": (None, [_P]),
    "ph_decode_run": (C.c_int, [_P, C.POINTER(DecodeIO), _P]),
    "ph_khead_param_name": (C.c_char_p, [_I]),
    "ph_khead_param_numel": (C.c_int64, [C.POINTER(KheadCfg), _I]),
    "ph_khead_pack_bytes": (C.c_size_t, [C.POINTER(KheadCfg)]),
    "ph_khead_pack_layout": (C.c_int, [C.POINTER(KheadCfg), C.POINTER(KheadLayout)]),
    "ph_khead_pack": (C.c_int, [C.POINTER(KheadCfg), C.POINTER(C.c_void_p), _P, _P]),
    "ph_khead_plan_workspace_bytes": (C.c_size_t, [C.POINTER(KheadCfg)]),
    "ph_khead_plan_create": (C.c_int, [C.POINTER(KheadCfg), _P, _P, _Z, C.POINTER(C.c_void_p)]),
    "ph_khead_plan_info": (C.c_int, [_P, C.POINTER(KheadGeometry)]),
    "ph_khead_geometry_of": (C.c_int, [C.POINTER(KheadCfg), C.POINTER(KheadGeometry)]),
    "ph_khead_plan_destroy": (None, [_P]),
    "ph_khead_plan_run": (C.c_int, [_P, C.POINTER(KheadIO), _P]),
    "ph_khead_plan_status": (C.c_int, [_P, _P]),
    "ph_khead_plan_timeouts": (C.c_int, [_P, _P]),
    "ph_neck_param_name": (C.c_char_p, [_I]),
    "ph_neck_param_numel": (C.c_int64, [C.POINTER(NeckCfg), _I]),
    "ph_neck_pack_bytes": (C.c_size_t, [C.POINTER(NeckCfg)]),
    "ph_neck_pack_layout": (C.c_int, [C.POINTER(NeckCfg), C.POINTER(NeckLayout)]),
    "ph_neck_pack": (C.c_int, [C.POINTER(NeckCfg), C.POINTER(C.c_void_p), _P, _P]),
    "ph_neck_posenc": (C.c_int, [_I, _I, _I, C.c_double, C.c_double, C.c_double, _P, _P]),
    "ph_neck_plan_workspace_bytes": (C.c_size_t, [C.POINTER(NeckCfg)]),
    "ph_neck_plan_create": (C.c_int, [C.POINTER(NeckCfg), _P, _P, _Z, C.POINTER(C.c_void_p)]),
    "ph_neck_plan_info": (C.c_int, [_P, C.POINTER(NeckGeometry)]),
    "ph_neck_geometry_of": (C.c_int, [C.POINTER(NeckCfg), C.POINTER(NeckGeometry)]),
    "ph_neck_plan_destroy": (None, [_P]),
    "ph_neck_plan_run": (C.c_int, [_P, C.POINTER(NeckIO), _P]),
    "ph_neck_plan_run_level": (C.c_int, [_P, _I, C.POINTER(NeckIO), _P]),
    "ph_neck_plan_run_outputs": (C.c_int, [_P, C.POINTER(NeckIO), _P]),
    "ph_neck_plan_level_input": (C.c_int, [_P, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "ph_neck_plan_run_level_planes": (C.c_int, [_P, _I, _P]),
    "ph_fpn_param_name": (C.c_char_p, [_I]),
    "ph_fpn_param_numel": (C.c_int64, [C.POINTER(FpnCfg), _I]),
    "ph_fpn_pack_bytes": (C.c_size_t, [C.POINTER(FpnCfg)]),
    "ph_fpn_pack_layout": (C.c_int, [C.POINTER(FpnCfg), C.POINTER(FpnLayout)]),
    "ph_fpn_pack": (C.c_int, [C.POINTER(FpnCfg), C.POINTER(C.c_void_p), _P, _P]),
    "ph_fpn_plan_workspace_bytes": (C.c_size_t, [C.POINTER(FpnCfg)]),
    "ph_fpn_plan_create": (C.c_int, [C.POINTER(FpnCfg), _P, _P, _Z, C.POINTER(C.c_void_p)]),
    "ph_fpn_plan_info": (C.c_int, [_P, C.POINTER(FpnGeometry)]),
    "ph_fpn_geometry_of": (C.c_int, [C.POINTER(FpnCfg), C.POINTER(FpnGeometry)]),
    "ph_fpn_plan_destroy": (None, [_P]),
    "ph_fpn_plan_run_laterals": (C.c_int, [_P, C.POINTER(FpnIO), _P]),
    "ph_fpn_plan_run_output": (C.c_int, [_P, _I, C.POINTER(FpnIO), _P]),
    "ph_fpn_plan_run": (C.c_int, [_P, C.POINTER(FpnIO), _P]),
    "ph_resnet_nparams": (C.c_int, [C.POINTER(ResNetCfg)]),
    "ph_resnet_param_name": (C.c_char_p, [C.POINTER(ResNetCfg), _I]),
    "ph_resnet_param_numel": (C.c_int64, [C.POINTER(ResNetCfg), _I]),
    "ph_resnet_pack_bytes": (C.c_size_t, [C.POINTER(ResNetCfg)]),
    "ph_resnet_pack_layout": (C.c_int, [C.POINTER(ResNetCfg), C.POINTER(ResNetLayout)]),
    "ph_resnet_pack": (C.c_int, [C.POINTER(ResNetCfg), C.POINTER(C.c_void_p), _P, _P]),
    "ph_resnet_pack_bwd_bytes": (C.c_size_t, [C.POINTER(ResNetCfg)]),
    "ph_resnet_pack_bwd_layout": (C.c_int, [C.POINTER(ResNetCfg), C.POINTER(ResNetLayout)]),
    "ph_resnet_pack_bwd": (C.c_int, [C.POINTER(ResNetCfg), _P, _P, _P]),
    "ph_resnet_plan_workspace_bytes": (C.c_size_t, [C.POINTER(ResNetCfg)]),
    "ph_resnet_plan_create": (C.c_int, [C.POINTER(ResNetCfg), _P, _P, _Z, C.POINTER(C.c_void_p)]),
    "ph_resnet_plan_info": (C.c_int, [_P, C.POINTER(ResNetGeometry)]),
    "ph_resnet_geometry_of": (C.c_int, [C.POINTER(ResNetCfg), C.POINTER(ResNetGeometry)]),
    "ph_resnet_plan_destroy": (None, [_P]),
    "ph_resnet_plan_run_stem": (C.c_int, [_P, C.POINTER(ResNetIO), _P]),
    "ph_resnet_plan_run_stage": (C.c_int, [_P, _I, C.POINTER(ResNetIO), _P]),
    "ph_resnet_plan_run": (C.c_int, [_P, C.POINTER(ResNetIO), _P]),
    "ph_track_param_name": (C.c_char_p, [C.POINTER(TrackCfg), _I]),
    "ph_track_param_numel": (C.c_int64, [C.POINTER(TrackCfg), _I]),
    "ph_track_pack_bytes": (C.c_size_t, [C.POINTER(TrackCfg)]),
    "ph_track_pack_layout": (C.c_int, [C.POINTER(TrackCfg), C.POINTER(TrackLayout)]),
    "ph_track_pack": (C.c_int, [C.POINTER(TrackCfg), C.POINTER(C.c_void_p), _P, _P]),
    "ph_assoc_plan_workspace_bytes": (C.c_size_t, [C.POINTER(AssocCfg)]),
    "ph_assoc_plan_create": (C.c_int, [C.POINTER(AssocCfg), _P, _P, _Z, C.POINTER(C.c_void_p)]),
    "ph_assoc_plan_info": (C.c_int, [_P, C.POINTER(AssocGeometry)]),
    "ph_assoc_plan_destroy": (None, [_P]),
    "ph_assoc_plan_run": (C.c_int, [_P, C.POINTER(AssocIO), _P]),
    "ph_assoc_plan_match": (C.c_int, [_P, _P, _P, _P, _P, _P, _Z, _L, _P, _P, _P]),
    "ph_dtracker_device_bytes": (C.c_size_t, [C.POINTER(TrackerCfg), _I, _I]),
    "ph_dtracker_create": (C.c_int, [C.POINTER(TrackerCfg), _P, _Z, _I, _I, C.POINTER(C.c_void_p)]),
    "ph_dtracker_destroy": (None, [_P]),
    "ph_dtracker_reset": (C.c_int, [_P, _L, _P]),
    "ph_dtracker_get_layout": (C.c_int, [_P, C.POINTER(DtrackerLayout)]),
    "ph_dtracker_run": (C.c_int, [_P, C.POINTER(DtrackerIO), _I, _P]),
    "ph_assoc_plan_track": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "ph_dtracker_bank_bytes": (C.c_size_t, [C.POINTER(TrackerCfg), _I, _I, _I]),
    "ph_dtracker_bank_create": (C.c_int, [C.POINTER(TrackerCfg), _P, _Z, _I, _I, _I, C.POINTER(C.c_void_p)]),
    "ph_dtracker_get_streams": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "ph_dtracker_reset_streams": (C.c_int, [_P, _L, _L, _P]),
    "ph_dtracker_step": (C.c_int, [_P, C.POINTER(DtrackerIO), _P, _P]),
    "ph_assoc_plan_track_streams": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ph_dvpq_workspace_bytes": (C.c_size_t, [C.POINTER(DvpqCfg)]),
    "ph_dvpq_frames": (C.c_int, [C.POINTER(DvpqCfg), C.POINTER(DvpqIO), _P, _Z, _P]),
    "ph_assign_desc_layout": (C.c_int, [C.POINTER(AssignCfg), _P, _P, _P, C.POINTER(AssignLayout)]),
    "ph_assign_solve": (C.c_int, [_P, _I, _I, _I, _P, _L, _P, _P, _P]),
    "ph_assign_desc": (C.c_int, [C.POINTER(AssignCfg), _P, _P, _P, _P, _I, _P, _L, _P, _P, _P, _Z, _P]),
    "ph_track_loss_scratch_bytes": (C.c_size_t, [C.POINTER(TrackLossCfg), _I, _I]),
    "ph_track_loss": (C.c_int, [C.POINTER(TrackLossCfg), _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, C.POINTER(C.c_int32),
                                _P, _P, _P, _P, _P, _Z, _P]),
    "ph_roi_align_fpn_bwd": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float), _I, _P, _I, C.c_float, C.POINTER(C.c_void_p), _P]),
    "ph_gtmask_boxes_workspace_bytes": (C.c_size_t, [_I, C.POINTER(C.c_int32), _I, _I]),
    "ph_gtmask_boxes": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _L, _I, _I,
                                  _I, _I, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "ph_gt_prepare": (C.c_int, [_P, _P, C.POINTER(C.c_int32), _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "ph_gt_segments_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "ph_gt_segments": (C.c_int, [_P, _I, _I, _I, _I, C.POINTER(C.c_int32), _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "ph_gt_index_maps": (C.c_int, [_P, _I, _P, _I, _I, _I, C.POINTER(C.c_int32), _I, _I, _I, _I, _P, C.POINTER(C.c_int32), _P, _P, _P, _P,
                                   _I, _I, _I, _I, C.c_float, C.c_float, C.POINTER(C.c_float), _P, _P, _P]),
    "ph_image_prepare": (C.c_int, [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _I, _I, _I,
                                   _P, _P]),
    "ph_optim_workspace_bytes": (C.c_size_t, [_P, _I]),
    "ph_optim_step": (C.c_int, [C.POINTER(OptimCfg), _P, _P, _I, C.c_float, _P, _P, _P, _Z, _P]),
    "ph_optim_zero_grads": (C.c_int, [_P, _P, _I, _I, _P]),
    "ph_selftest_mfma16": (C.c_int, [_P, _P, _P, _P]),
    "ph_selftest_mfma32": (C.c_int, [_P, _P, _P, _P]),
    "ph_selftest_readbw": (C.c_int, [_P, _L, _I, _P, _P]),
    "ph_selftest_trread": (C.c_int, [_P, _P, _P]),
}

_lib = None


class PolyheadError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PolyheadError(
            f"{LIB_PATH} is missing: build it with `python -m polyphonicformer_amd.build` "
            "(needs hipcc, gfx950). There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().ph_last_error_string()
        raise PolyheadError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


@contextlib.contextmanager
def switches(**values):
    """sets library switches by name (SWITCHES) for the block and puts the values it found back afterwards:
    `with _lib.switches(up2_wgs=7): ...`.  The table lives in the library alone (ph_get_switch reads it)"""
    lib, old = load(), {}
    try:
        for name, v in values.items():
            i, cur = SWITCHES.index(name), C.c_int()
            check(lib.ph_get_switch(i, cur), "ph_get_switch")
            check(lib.ph_set_switch(i, v), f"ph_set_switch({name}, {v})")
            old[i] = cur.value
        yield
    finally:
        for i, v in old.items():
            check(lib.ph_set_switch(i, v), "ph_set_switch")


def ptr(t):
    """raw device (or host) pointer of a torch tensor; None -> NULL"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    """raw hipStream_t of torch's current stream on the current device.  One C call: `torch.cuda.current_stream()` builds a
    Stream object per call (~9 us) and every kernel launch of a frame asks -- 0.7 ms per video frame (round 4 host profile)"""
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _tree(module):
    """cached [(prefix, sub-module)] of `module`, re-discovered when the tree changed: the signature is the identity of every
    cached module's direct children (a replaced / added / removed sub-module -- `head.fc_cls = nn.Linear(...)`,
    `rpn_head.localization_fpn = None` -- changes it).  ~100 dict reads per call instead of a generator walk."""
    c = module.__dict__.get("_ph_tree")
    if c is not None:
        sig = tuple(id(ch) for _, m in c[1] for ch in m._modules.values())
        if sig == c[0]:
            return c[1]
    mods = [(n + "." if n else "", m) for n, m in module.named_modules()]
    module.__dict__["_ph_tree"] = (tuple(id(ch) for _, m in mods for ch in m._modules.values()), mods)
    return mods


def param_versions(module):
    """the `_version` counters of every parameter of `module` -- the cache key of the packed device weights (an in-place
    update such as load_state_dict / an optimizer step bumps them; a replaced Parameter or sub-module is seen through the
    live `_parameters` dicts / `_tree`'s signature; the id of each Parameter is part of the key for that reason).
    `module.parameters()` re-discovers the module tree on every call, 0.8 ms per video frame."""
    return tuple((id(p), p._version) for _, m in _tree(module) for p in m._parameters.values() if p is not None)


def named_params(module):
    """dict(module.named_parameters()) without re-discovering the module tree on every call (`_tree`); like
    `named_parameters`, a Parameter shared by two modules appears once, under its first name.  The training forward asks once
    per stage and head: 1 641 `named_parameters` generator steps, 1.3 ms per step (round 4 host profile)."""
    out, seen = {}, set()
    for pre, m in _tree(module):
        for k, p in m._parameters.items():
            if p is not None and id(p) not in seen:
                seen.add(id(p))
                out[pre + k] = p
    return out
