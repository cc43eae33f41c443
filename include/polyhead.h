/*
 * polyhead.h -- C ABI of libpolyhead.so: the MI355X (gfx950) implementation of PolyphonicFormer's
 * unified-query decode hot path.  Plain pointers, sizes and a hipStream_t (passed as void*); no
 * torch types.  Every entry point
 *   - returns 0 on success or a negative PH_E* code (never throws, see ph_last_error_string),
 *   - never allocates and never synchronises: the caller owns every buffer and passes the stream,
 *   - is thread-compatible (no mutable globals besides a thread-local error string and the atomic switch table below).
 *
 * The reference is 100 % Python: there is no FFI in it to mirror.  Each function
 * below therefore cites the reference *Python* lines whose device work it replaces; the Python
 * classes in polyphonicformer_amd/ keep the reference's registry names / kwargs / state_dict keys
 * and call these through ctypes (INTEGRATION.md shows the binding).
 *
 * Internal device formats:
 *   feature planes  : uint16 (bf16 bits) [P][B][256][HWp], HWp = HW rounded up to 128, zero padded.
 *                     P = 1 for PH_PREC_BF16; P = 2 (hi, lo with x ~= hi + lo to 2^-17) for
 *                     PH_PREC_SPLIT, the fp32-grade mode used for the 1e-3 parity runs.
 *   mask bits       : uint32 [B][Npad][HWp/32], bit j of word w = 1[logit(pixel 32w+j) > 0];
 *                     Npad = N rounded up to 32; rows >= N and pixels >= HW are 0.
 *   query matrices  : fp32 [B][N][256] row major at the API; bf16 planes [P][...][Npad][256] inside.
 */
#ifndef POLYHEAD_H_
#define POLYHEAD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PH_VERSION 100

enum { PH_OK = 0, PH_EINVAL = -1, PH_EUNSUPPORTED = -2, PH_ELAUNCH = -3, PH_EWORKSPACE = -4 };
/* Arithmetic of an operator = element format of its 16-bit operands x planes per operand:
 *   PH_PREC_BF16         bf16, one plane each                          (1 MFMA per product, ~2^-9 per operand)
 *   PH_PREC_BF16_KSPLIT  ph_dynconv only: bf16 features in ONE plane, the dynamic kernels as hi + lo planes (2 MFMAs):
 *                        exact for features that ARE bf16 values, kernels to 2^-17
 *   PH_PREC_SPLIT        bf16, hi + lo planes of both operands, a.b ~= ah.bh + ah.bl + al.bh (3 MFMAs, ~2^-16)
 *   PH_PREC_F16          IEEE fp16, one plane each (1 MFMA, ~2^-12 per operand; |values| < 65504)
 *   PH_PREC_BF16_KF16    ph_dynconv only: bf16 features in ONE plane, the dynamic kernels as ONE fp16 plane (PH_KERN_F16); the
 *                        feature fragments are converted to fp16 in registers (exact inside fp16's normal range) and the
 *                        product is one f16 MFMA: ~2^-12 on the kernels only -- 2.5e-4 per stage, single-plane speed.
 *   PH_PREC_QHYBRID      ph_query_stage only: the updator half (pooled sums, gate products: unbounded operands) as
 *                        PH_PREC_SPLIT, the attention / FFN / fc-tower half -- every product there has a LayerNorm- or softmax-
 *                        bounded operand -- as ONE fp16 plane of weights and activations (1 MFMA, 2^-12 per operand, half the
 *                        weight stream); weights packed accordingly (pack.py), dynamic kernels out as PH_KERN_F16. */
enum { PH_PREC_BF16 = 1, PH_PREC_BF16_KSPLIT = 2, PH_PREC_SPLIT = 3, PH_PREC_F16 = 5, PH_PREC_BF16_KF16 = 6, PH_PREC_QHYBRID = 7 };
/* flag OR-ed into `prec` of ph_nhwc_ingest (output) and ph_conv_nhwc (input, 3x3 stride 2, one-plane formats): the planes are
   chunk-major [frame][256 / 16][HW][16] instead of channels-last [frame][HW][256].  The stride-2 kernel stages 16 channels of
   a 9 x 129 pixel patch at a time; from channels-last planes that is 32 bytes of every 512, i.e. a quarter of each 128-byte
   line per stage and (the lines do not survive in L2 between stages) four times the plane's bytes from HBM. */
enum { PH_PLANES_C16 = 0x100 };
enum { PH_OUT_F32 = 0, PH_OUT_BF16 = 1, PH_OUT_F16 = 2 };
enum { PH_KERN_BF16_PLANES = 0, PH_KERN_F16 = 1 };   /* ph_query_stage: format of the dynamic conv kernels it emits */
enum { PH_GN_TO_PLANES = 0, PH_GN_UP2_PLANES = 1, PH_GN_ACCUM = 2, PH_GN_TO_NCHW = 3, PH_GN_TO_CPLANES = 4 };   /* ph_gn_apply modes */
enum { PH_IN_F32_NCHW = 0, PH_IN_PLANES = 1 };   /* ph_khead_fused input_format */

#define PH_C 256          /* channels: in_channels == out_channels == feat_channels == 256 */
#define PH_HEADS 8        /* num_heads (head dim 32) */

int         ph_version(void);
const char* ph_last_error_string(void);

/* ---- the library's switches -----------------------------------------------------------------
 * Measurement and test switches of the public launch entry points: ONE process-wide table of integers, 0 = the
 * built-in rule.  The table is filled from the environment exactly once, on the first use of any of them (a launch through one of
 * the entry points named below, ph_get_switch or ph_set_switch), from the variable named with each id; after that the
 * environment is never read again and a switch changes by ph_set_switch only.  PH_CONV_TH_NOW, the retired per-call spelling of
 * PH_SWITCH_CONV_TILE_ROWS, is still honoured at that one read and, as before, wins over PH_CONV_TH when both are set.  A variable
 * whose value ph_set_switch would refuse is ignored.
 * Every entry is a relaxed atomic: a launch concurrent with a ph_set_switch sees the old or the new value, never a mix; a
 * captured graph keeps the geometry it was captured with, whatever is set before its replay.  No native plan function
 * (ph_decode_*, ph_khead_plan_*, ph_neck_plan_*, ph_fpn_plan_*, ph_assoc_plan_*, ...) consults the table: their choices are their
 * cfg's fields.  ph_set_switch allocates nothing and launches nothing. */
enum {
    PH_SWITCH_CONV_WGS = 0,        /* PH_CONV_WGS: workgroups of ph_dynconv; >= 0 */
    PH_SWITCH_UP2_WGS = 1,         /* PH_UP2_WGS: workgroups of ph_dynconv_up2[_wgs], over the caller's count; >= 0 */
    PH_SWITCH_QUERY_NRT = 2,       /* PH_QUERY_NRT: 16-row blocks per workgroup of ph_query_stage[_counts]; >= 0 */
    PH_SWITCH_QUERY_TIMELINE = 3,  /* PH_QUERY_TIMELINE: 1 = ph_query_stage[_counts] prints one workgroup's phase times (debug:
                                      synchronises; the first such launch allocates the 128-byte stamp buffer); 0 or 1 */
    PH_SWITCH_CONV_TILE_ROWS = 4,  /* PH_CONV_TH: output rows per tile of ph_conv_nhwc in the one-plane grades; 0, 2 or 4 */
    PH_SWITCH_GNSUM_WGS = 5,       /* PH_GNSUM_WGS: workgroups per frame of ph_gn_sum_planes; >= 0 */
    PH_SWITCH_CPLANES_TPW = 6,     /* PH_CPLANES_TPW: 64-pixel tiles per workgroup of ph_gn_apply's PH_GN_TO_CPLANES mode; >= 0 */
    PH_SWITCH_PAN_GENERIC = 7,     /* PH_PAN_GENERIC (set to anything): 1 = ph_panoptic_argmax takes the generic kernel on the x4
                                      geometry too; 0 or 1 */
    PH_SWITCH_COUNT = 8
};
/* PH_EINVAL, with a message and nothing changed, on an id outside the enum or a value outside the id's range above */
int ph_set_switch(int id, int value);
int ph_get_switch(int id, int* value);

/* ---- geometry helpers ------------------------------------------------------------------- */
static inline int64_t ph_hw_padded(int64_t hw) { return (hw + 127) / 128 * 128; }
static inline int     ph_n_padded(int n) { return (n + 31) / 32 * 32; }

/* ---- feature-map ingest ------------------------------------------------------------------
 * fp32 NCHW [B][256][HW] (what KernelHead hands over, kernel_head.py:347 x_feats/depth_feats)
 * -> bf16 planes [P][B][256][HWp].  Replaces nothing arithmetic in the reference; it is the
 * format change at the boundary. */
int ph_ingest_features(const float* src, uint16_t* planes, int B, int64_t HW, int prec, void* stream);

/* fp32 mask logits [B][N][HW] -> mask bits.  kernel_update_head.py:236-238
 * (sigmoid -> > hard_mask_thr(0.5) -> float), stated as logit > 0. */
int ph_binarize(const float* logits, int64_t logits_batch_stride /* elements; 0 = N*HW (contiguous) */, uint32_t* bits,
                int B, int N, int64_t HW, void* stream);
/* the same for fp32 or fp16 logits (dtype PH_OUT_F32 / PH_OUT_F16), optionally predicated on a device word: when run_if is
 * non-NULL and *run_if == 0 at execution time the launch returns at once (see ph_khead_fused_if) */
int ph_binarize_if(const void* logits, int dtype, int64_t logits_batch_stride, uint32_t* bits, int B, int N, int64_t HW,
                   const uint32_t* run_if /* nullable */, void* stream);

/* ---- A7: masked pooling -------------------------------------------------------------------
 * kernel_update_head.py:241-242  einsum('bnhw,bchw->bnc') for x and depth_feats in one pass
 * (and kernel_head.py:320 with only `xplanes`).  Split over `nsplit` pixel ranges; the
 * deterministic partial sums land in partial[B][nsplit][Npad][512] (cols 0..255 = x,
 * 256..511 = depth_feats) and are summed in fixed order by the consumer. `dplanes` may be NULL. */
int ph_pool(const uint16_t* xplanes, const uint16_t* dplanes, const uint32_t* bits, float* partial,
            int B, int N, int64_t HW, int nsplit, int prec, void* stream);
/* the same over the first ph_n_padded(N) rows of a bits tensor that has `bits_rows` (>= that) rows per frame:
 * kernel_head.py:314-320 pools over the THING rows of the full mask tensor */
int ph_pool_rows(const uint16_t* xplanes, const uint16_t* dplanes, const uint32_t* bits, int bits_rows, float* partial,
                 int B, int N, int64_t HW, int nsplit, int prec, void* stream);
/* ph_pool that also writes pcount[B][nsplit][ph_n_padded(N)] (int32): the set bits of every mask row in every pixel range -- the
 * `count(M)` of the folded feat_transform bias (kernel_update_head.py:225,241), handed to ph_query_stage_counts */
int ph_pool_counts(const uint16_t* xplanes, const uint16_t* dplanes, const uint32_t* bits, float* partial, int32_t* pcount,
                   int B, int N, int64_t HW, int nsplit, int prec, void* stream);
/* ONE read of depth_feats pooled under TWO mask sets (the depth halves of two consecutive stages' poolings, behind two
 * ph_dynconv_poolx launches): columns 256 .. 511 of partialA / partialB ([B][nsplit][Npad][512]; columns 0 .. 255 are not touched)
 * and pcountA / pcountB ([B][nsplit][Npad]) are, bit for bit, what ph_pool_counts(dplanes, NULL, bitsX, partialX + 256, pcountX, ...)
 * leaves for X = A and X = B at the same nsplit: the pixel split, the chunk order and the MFMA order of every row are the same.
 * ph_pool_depth_pair_supported: one feature plane (PH_PREC_BF16 / PH_PREC_F16) and N <= 160; elsewhere PH_EUNSUPPORTED. */
int ph_pool_depth_pair_supported(int N, int prec);
int ph_pool_depth_pair(const uint16_t* dplanes, const uint32_t* bitsA, const uint32_t* bitsB, float* partialA, float* partialB,
                       int32_t* pcountA, int32_t* pcountB, int B, int N, int64_t HW, int nsplit, int prec, void* stream);
/* the `nsplit` every plan of this library pools with when its caller names none (the cfgs' nsplit = 0, engine.default_nsplit):
 * 4 * B * nsplit workgroups fill the chip once, at most 32 ranges and one per 128-pixel chunk; frame_invariant != 0: the split
 * of a one-frame launch at any B (a frame's partial sums are then added in the same order whatever shares its launch) */
int ph_pool_default_nsplit(int B, int64_t HW, int frame_invariant);

/* ---- packed per-stage weights -------------------------------------------------------------
 * One KernelUpdateHead stage (kernel_update_head.py:21-191 parameters) packed by the host into
 *   wb : uint16 [P][wb_plane_elems]   bf16 MFMA B-fragments, tile-major
 *   wf : float  [..]                  biases, LayerNorm affine, folded vectors
 * with offsets (in elements) indexed by the enums below; branch 0 = mask, 1 = depth. */
enum {
    PH_W_DYN = 0,   /* dynamic_layer folded with feat_transform: [512][256]   kernel_updator.py:58, kernel_update_head.py:225 */
    PH_W_INP,       /* input_layer [512][256]                                  kernel_updator.py:64 */
    PH_W_IG,        /* input_gate  [256][256]                                  :73 */
    PH_W_UG,        /* update_gate [256][256]                                  :74 */
    PH_W_FC,        /* fc_layer    [256][256]                                  :89 */
    PH_W_QKV,       /* attn.in_proj_weight [768][256]                          kernel_update_head.py:112-115 */
    PH_W_OUT,       /* attn.out_proj [256][256] */
    PH_W_FFN1,      /* ffn.layers.0.0 [F][256]                                 :146-151 */
    PH_W_FFN2,      /* ffn.layers.1   [256][F] */
    PH_W_H0A,       /* cls_fcs.0 (mask branch) / depth_regs.0 (depth branch)   :161-187 */
    PH_W_H0B,       /* mask_fcs.0 (mask branch only) */
    PH_W_CLS,       /* fc_cls [Lpad][256] (mask branch only)                   :169-172 */
    PH_W_KERN,      /* fc_mask / fc_depth folded with feat_(depth_)transform: [272][256]; row 256 = bias dot  :189-190,225-226 */
    PH_W_COUNT
};
enum {
    PH_V_DYN_CNT = 0, /* [512] dynamic_layer.weight @ feat_transform.bias (multiplies the pixel count) */
    PH_V_DYN_B, PH_V_INP_B, PH_V_IG_B, PH_V_UG_B,
    PH_V_LN_IG_G, PH_V_LN_IG_B,   /* input_norm_in   kernel_updator.py:73 */
    PH_V_LN_UG_G, PH_V_LN_UG_B,   /* norm_in         :74 */
    PH_V_LN_PO_G, PH_V_LN_PO_B,   /* norm_out        :78 */
    PH_V_LN_IO_G, PH_V_LN_IO_B,   /* input_norm_out  :79 */
    PH_V_FC_B, PH_V_LN_FC_G, PH_V_LN_FC_B,
    PH_V_QKV_B, PH_V_OUT_B, PH_V_LN_ATT_G, PH_V_LN_ATT_B,
    PH_V_FFN1_B, PH_V_FFN2_B, PH_V_LN_FFN_G, PH_V_LN_FFN_B,
    PH_V_LN_H0A_G, PH_V_LN_H0A_B, PH_V_LN_H0B_G, PH_V_LN_H0B_B,
    PH_V_CLS_B, PH_V_KERN_B,       /* [272] folded fc_mask/fc_depth bias (entry 256 = bias . transform bias) */
    PH_V_COUNT
};
typedef struct {
    int64_t w[2][PH_W_COUNT];   /* element offsets into one plane of wb */
    int64_t v[2][PH_V_COUNT];   /* element offsets into wf */
    int64_t wb_plane_elems;     /* distance between the hi and lo plane */
    int32_t ffn_dim;            /* F, multiple of 256 */
    int32_t num_classes;        /* L */
} ph_stage_layout;

/* ---- A8-A12: the query side of one stage ---------------------------------------------------
 * kernel_update_head.py:245-288 + funcs/kernel_updator.py:55-93 for both branches:
 *   pre : partial-sum reduce, KernelUpdator x2, attention in-projection
 *   post: self-attention per branch, out-proj + LN, FFN + LN, cls / mask-kernel / depth-kernel heads
 * Inputs  k_in, q_in fp32 [B][N][256] (proposal_feat, depth_proposal); bits for the pixel counts.
 * Outputs obj, dobj fp32 [B][N][256]; cls fp32 [B][N][L]; kern planes [P][2][B][Npad][256] and
 *         kbias fp32 [2][B][Npad]: the dynamic 1x1 conv kernels already folded with
 *         feat_transform, i.e. new_mask_logits = kern[0] . x + kbias[0]  (kernel_update_head.py:317-329).
 * Workspace (ph_query_workspace_bytes): q/k/v planes + residual.
 * phases: PH_QUERY_PRE | PH_QUERY_POST, optionally | PH_QUERY_WIDE: as many rows per workgroup as divide the padded row
 *         count (fewest CU-seconds; for launches that share the GPU with other streams).  Without it the launch is shaped
 *         to fill the chip by itself (lowest latency of a single launch).
 *         | PH_QUERY_MASK_ONLY or | PH_QUERY_DEPTH_ONLY: one branch's half of the launch (grid.y = 1).  The branches share no data
 *         inside a stage, so the two halves, in either order, leave exactly what the full launch leaves: the mask half writes obj,
 *         cls, kern[0], kbias[0] from columns 0 .. 255 of `partial`, the depth half dobj, kern[1], kbias[1] from columns 256 .. 511.
 *         The pixel counts are the same integers from the bit rows (ph_query_stage) as from ph_pool_counts. */
enum { PH_QUERY_PRE = 1, PH_QUERY_POST = 2, PH_QUERY_BOTH = 3, PH_QUERY_WIDE = 0x100, PH_QUERY_MASK_ONLY = 0x200, PH_QUERY_DEPTH_ONLY = 0x400 };
size_t ph_query_workspace_bytes(int B, int N, int prec);
/* byte offset, inside the workspace, of the fp32 [B][2][Npad][256] KernelUpdator outputs
 * (funcs/kernel_updator.py:93) that the PRE phase leaves behind for the POST phase. */
size_t ph_query_workspace_updator_offset(int B, int N, int prec);
int ph_query_stage(const float* partial, int nsplit, const uint32_t* bits,
                   const float* k_in, const float* q_in,
                   const uint16_t* wb, const float* wf, const ph_stage_layout* layout,
                   float* obj, float* dobj, float* cls, int cls_sigmoid /* kernel_update.py:396-397 */,
                   uint16_t* kern, float* kbias,
                   void* workspace, size_t workspace_bytes,
                   int B, int N, int64_t HW, int prec /* PH_PREC_BF16 | PH_PREC_SPLIT */,
                   int kern_format /* PH_KERN_BF16_PLANES: [P][2][B][Npad][256]; PH_KERN_F16: one fp16 plane */,
                   int phases, void* stream);
/* the same, taking the hard masks' pixel counts from ph_pool_counts instead of counting the bit rows again; prec may also
 * be PH_PREC_QHYBRID (with PH_KERN_F16) in both entry points */
int ph_query_stage_counts(const float* partial, int nsplit, const uint32_t* bits, const int32_t* pcount, const float* k_in,
                          const float* q_in, const uint16_t* wb, const float* wf, const ph_stage_layout* layout,
                          float* obj, float* dobj, float* cls, int cls_sigmoid, uint16_t* kern, float* kbias,
                          void* workspace, size_t workspace_bytes, int B, int N, int64_t HW, int prec, int kern_format,
                          int phases, void* stream);

/* ---- A13: dynamic 1x1 convolution -----------------------------------------------------------
 * kernel_update_head.py:317-329: logits[b][n][hw] = sum_c kern[b][n][c] * feat[b][c][hw] + kbias[b][n].
 * Either writes the mask bits the next stage pools with (bits_out != NULL; the logits of a
 * non-final stage are consumed only through `> 0`, kernel_update_head.py:236-238) or the logits
 * themselves (logits_out, dtype out_dtype = PH_OUT_F32 / BF16 / F16).  `prec` = PH_PREC_BF16 (1 feature plane, 1 kernel
 * plane), PH_PREC_BF16_KSPLIT (1, 2), PH_PREC_SPLIT (2, 2), PH_PREC_F16 (fp16 planes, 1, 1) or PH_PREC_BF16_KF16 (bf16 plane, one fp16 kernel plane).
 * `kern` is planes [P][..][Npad][256] (plane stride
 * given), `kern_batch_stride` / `kbias_batch_stride` / `out_batch_stride` are the element distances
 * between frames: Npad*256 / Npad / N*HW for per-frame dynamic kernels; 0 / 0 / rows*HW when the
 * same static 1x1 conv weights serve every frame (kernel_head.py:256,285,295 init_kernels,
 * conv_direct_depth, conv_seg), which also lets the output be a row slice of a larger tensor. */
int ph_dynconv(const uint16_t* planes, const uint16_t* kern, int64_t kern_plane_stride, int64_t kern_batch_stride,
               const float* kbias, int64_t kbias_batch_stride, uint32_t* bits_out, void* logits_out, int out_dtype,
               int64_t out_batch_stride, int B, int N, int64_t HW, int prec, void* stream);

/* ---- A14: x2 bilinear upsample, align_corners=False (kernel_update.py:131-143); dtype PH_OUT_* ------------- */
int ph_upsample2x(const void* src, void* dst, int dtype, int64_t planes /* B*N */, int H, int W, void* stream);

/* ---- A13 of the final stage + A14 fused (round 4): up_out[b][n] = bilinear x2 (align_corners=False) of the 16-bit logits
 * kern[b][n] . feat[b] + kbias[b][n], from ONE read of the feature plane; logits_out (nullable) additionally receives the
 * low-resolution logits [B][N][H][W] themselves (kernel_update.py:131-143 returns both for the mask branch; the depth
 * branch's low-resolution logits are never returned: kernel_update.py:338-345,401).  Same values as ph_dynconv followed by
 * ph_upsample2x up to fp32 rounding inside the interpolation.  `kern`: ONE 16-bit plane [B][Npad][256] (frame stride given),
 * prec PH_PREC_BF16 (out_dtype PH_OUT_BF16), PH_PREC_F16 or PH_PREC_BF16_KF16 (out_dtype PH_OUT_F16).
 * ph_dynconv_up2_supported: W == 256 (tiles of 64 pixels must not straddle image rows; 2048 / 8), H * W % 128 == 0,
 * 65 <= N <= 224; otherwise callers use the two-kernel form. */
int ph_dynconv_up2_supported(int N, int H, int W, int prec, int out_dtype);
int ph_dynconv_up2(const uint16_t* planes, const uint16_t* kern, int64_t kern_batch_stride, const float* kbias,
                   int64_t kbias_batch_stride, void* logits_out /* nullable */, void* up_out, int out_dtype, int B, int N, int H,
                   int W, int prec, void* stream);
/* the same with the launch geometry chosen by the caller (round 6): `workgroups` contiguous ranges of image rows, 0 = one per CU.  A
 * launch that shares the GPU with other streams' kernels ends sooner with 1.5 per CU (engine.DecodePlan: plans marked `shares_gpu`);
 * the values do not depend on it. */
int ph_dynconv_up2_wgs(const uint16_t* planes, const uint16_t* kern, int64_t kern_batch_stride, const float* kbias,
                       int64_t kbias_batch_stride, void* logits_out /* nullable */, void* up_out, int out_dtype, int B, int N, int H,
                       int W, int prec, int workgroups, void* stream);

/* ---- A13 of a NON-final stage fused with the x half of the next stage's A7 (round 6): the mask bits of ph_dynconv AND
 * partial[b][split][n][0 .. 255] = sum over the pixels of range `split` of bits[n][px] * x[c][px] -- ph_pool's output for the x map
 * (kernel_update_head.py:317-329, :236-241) -- from ONE read of the x plane.  The caller pools depth_feats alone afterwards
 * (ph_pool_counts with xplanes = the depth plane, dplanes = NULL, partial + 256: columns 256 .. 511 and the pixel counts).
 * `kern`: ONE 16-bit plane [B][Npad][256]; prec PH_PREC_BF16, PH_PREC_F16 or PH_PREC_BF16_KF16; 33 <= N <= 192
 * (ph_dynconv_poolx_supported); grid = nsplit x B workgroups, one per CU when nsplit * B is about the CU count.  The bits are
 * ph_dynconv's bit for bit.  The pixel ranges are ph_pool's for the same nsplit (whole pairs of 64-pixel chunks; an empty range
 * writes zeros), and in the PH_PREC_BF16 / PH_PREC_F16 grades every range's sums are ph_pool's BIT FOR BIT (same operands, same
 * order); in the PH_PREC_BF16_KF16 grade the tile is pooled after its conversion to fp16 (exact for every bf16 value inside
 * fp16's normal range: 1e-6 apart on N(0, 1) data).  Replaces: kernel_update_head.py:317-329 + the x half of :241. */
int ph_dynconv_poolx_supported(int N, int prec);
int ph_dynconv_poolx(const uint16_t* planes, const uint16_t* kern, int64_t kern_batch_stride, const float* kbias,
                     int64_t kbias_batch_stride, uint32_t* bits_out, float* partial, int nsplit, int B, int N, int64_t HW, int prec,
                     void* stream);

/* ---- A1-A5: KernelHead after localization_fpn (kernel_head.py:245-347) ------------------------
 * ph_khead_conv_gn: loc/sem/dfe = ReLU(GN(conv1x1(f0/f1/f2))) and x = sem + loc, from the three fp32
 *   post-neck maps [B][256][HW] to bf16 planes (+ optional fp32 NCHW x_feats / depth_feats).
 *   wplanes: bf16 planes [P][3][256][256] of {loc,seg,depth}_convs.0.conv.weight;
 *   gn_affine: fp32 [3][2][256] (gamma, beta) of the three GroupNorms; eps 1e-5.
 * The remaining 1x1 convs (init_kernels :256, conv_seg :295, conv_direct_depth :285) are ph_dynconv
 * calls with static weights, the object pooling (:314-320) is ph_pool, and
 * ph_khead_proposals forms proposal_feats = [init_kernels.weight + pooled ; conv_seg.weight[stuff]]
 * (:299-300,324-335) as fp32 [B][n_thing_queries + n_stuff][256]. */
size_t ph_khead_workspace_bytes(int B, int64_t HW, int groups);
int ph_khead_conv_gn(const float* f0, const float* f1, const float* f2, const uint16_t* wplanes,
                     const float* gn_affine, int groups, float eps,
                     uint16_t* loc_planes, uint16_t* sem_planes, uint16_t* x_planes, uint16_t* dfe_planes,
                     float* x_f32 /* nullable */, float* dfe_f32 /* nullable */,
                     void* workspace, size_t workspace_bytes, int B, int64_t HW, int prec, void* stream);
/* ph_khead_fused: the same two passes with the three static 1x1 convs applied to the normalised tile while it is
 * still in LDS (second GEMM of the apply pass): loc and sem never reach HBM, and the mask / seg / depth logits leave
 * the kernel directly.  Replaces ph_khead_conv_gn + 3 x ph_dynconv + the stuff-row copy (kernel_head.py:250-331).
 *   w2_init / w2_seg / w2_dd: bf16 planes [P][rows32/32][16][64][8] = MFMA 32x32x16 A fragments of
 *     init_kernels.weight [n_init][256], conv_seg.weight [n_seg][256], conv_direct_depth.weight [1][256], rows zero
 *     padded to a multiple of 32 (block (row tile, k-step): lane l holds row (l & 31), k = 16*step + 8*(l >> 5) .. +8);
 *   bias_seg [rows32(n_seg)], bias_dd [32] fp32 (init_kernels has no bias);
 *   mask_preds fp32 [B][n_init + n_stuff][HW]: rows [0, n_init) = init_kernels(loc), rows [n_init, ..) = seg rows
 *     [stuff_lo, stuff_lo + n_stuff) (cat_stuff_mask, :329-331; n_stuff = 0: none);
 *   seg_preds fp32 [B][n_seg][HW]; depth_pred fp32 [B][1][HW]; x_planes / dfe_planes / x_f32 / dfe_f32 as above
 *   (dfe_planes doubles as the scratch that carries loc from the first to the second apply launch).
 *   input_format: PH_IN_F32_NCHW -- f0/f1/f2 are the fp32 maps [B][256][HW] of the reference boundary;
 *     PH_IN_PLANES -- they are bf16 planes [P][B][256][HWp], zero in [HW, HWp) (what ph_gn_apply PH_GN_TO_CPLANES
 *     writes: the neck hands its outputs over at 2 bytes per element; in bf16 precision the results are bit-identical
 *     to feeding the fp32 maps, whose first use is the same rounding).
 *   The mask bits of these logits (use_binary, :310-314) are ph_binarize's: emitting them from this epilogue (ballot per
 *   accumulator register) measured slower than that separate pass. */
int ph_khead_fused(const void* f0, const void* f1, const void* f2, const uint16_t* wplanes,
                   const float* gn_affine, int groups, float eps,
                   const uint16_t* w2_init, int n_init, const uint16_t* w2_seg, const float* bias_seg, int n_seg,
                   const uint16_t* w2_dd, const float* bias_dd, int stuff_lo, int n_stuff,
                   uint16_t* x_planes, uint16_t* dfe_planes, float* x_f32 /* nullable */, float* dfe_f32 /* nullable */,
                   float* mask_preds, float* seg_preds, float* depth_pred,
                   void* workspace, size_t workspace_bytes, int B, int64_t HW, int prec, int input_format, void* stream);
/* ph_khead_fused with the logit dtype as an argument (PH_OUT_F32 / PH_OUT_F16) and a device predicate: when run_if is non-NULL
 * and *run_if == 0 at execution time every launch of the call returns at once.  Issued behind ph_khead_onepass with run_if =
 * that call's status word (the first 4 bytes of its workspace) it is the in-call fallback of a one-pass launch that gave up:
 * same buffers, same results to the two forms' summation-order difference, no host round trip, capturable in a HIP graph. */
int ph_khead_fused_if(const void* f0, const void* f1, const void* f2, const uint16_t* wplanes,
                      const float* gn_affine, int groups, float eps,
                      const uint16_t* w2_init, int n_init, const uint16_t* w2_seg, const float* bias_seg, int n_seg,
                      const uint16_t* w2_dd, const float* bias_dd, int stuff_lo, int n_stuff,
                      uint16_t* x_planes, uint16_t* dfe_planes, float* x_f32 /* nullable */, float* dfe_f32 /* nullable */,
                      void* mask_preds, void* seg_preds, void* depth_pred, int logits_dtype, const uint32_t* run_if /* nullable */,
                      void* workspace, size_t workspace_bytes, int B, int64_t HW, int prec, int input_format, void* stream);
/* ph_khead_onepass (round 3): ph_khead_fused's results from ONE read of the three maps.  The conv output of a 128-pixel
 * slice stays in the accumulator registers of one workgroup per CU while the GroupNorm sums of the whole (frame, map)
 * are exchanged between the workgroups inside the launch (persistent grid, bounded spins); loc waits in LDS for
 * x = sem + loc; the mask bits of `mask_preds` (kernel_head.py:314-317; what ph_binarize would write) come from the
 * second GEMM's accumulators.  Same arithmetic as ph_khead_fused's PH_PREC_BF16 / PH_PREC_F16 grades.
 *   conv_frags: {loc,seg,depth}_convs.0.conv.weight as MFMA 32x32x16 A fragments [3][8][16][64][8] (one 16-bit plane);
 *   mask_preds / seg_preds / depth_pred: fp32 or fp16 (`out_dtype` PH_OUT_F32 / PH_OUT_F16), shapes as ph_khead_fused;
 *   bits: nullable, uint32 [B][bits_rows][HWp/32], rows >= n_init + n_stuff are cleared;
 *   workspace: ph_khead_onepass_workspace_bytes(B, HW) bytes; the caller zeroes it ONCE after allocation, every call clears all
 *     of it but the last 256 bytes (a memset node ahead of the kernel): those hold the sticky time-out words.
 * ph_khead_onepass_supported: 1 when the geometry fits (HWp / 128 <= #CUs, 32 groups, one-plane grade, HW % 4 == 0 for
 * fp32 inputs); otherwise callers use ph_khead_fused.
 * The persistent grid needs one workgroup resident on every CU it uses.  When that does not happen within the hand-off bound
 * (ph_khead_onepass_set_timeout_us, default 20 ms: another kernel holds CUs that long, or two one-pass launches starve each
 * other) the launch GIVES UP: it raises the per-call status word (first 4 bytes of the workspace), its workgroups leave, and
 * the tensors it was writing are incomplete.  Round 4: the caller issues ph_khead_fused_if + ph_binarize_if predicated on that
 * word directly behind the call (engine.KernelHeadPlan.run does), so the SAME call still ends with the right results -- there
 * is no undefined-result mode, no host synchronisation, and it holds inside HIP graphs.  ph_khead_onepass_status: 1 if the last
 * call gave up; ph_khead_onepass_timeouts: workgroup time-outs since the workspace was zeroed (both synchronise the stream). */
int ph_khead_onepass_supported(int B, int64_t HW, int groups, int prec, int input_format);
size_t ph_khead_onepass_workspace_bytes(int B, int64_t HW);
int ph_khead_onepass(const void* f0, const void* f1, const void* f2, const uint16_t* conv_frags,
                     const float* gn_affine, int groups, float eps,
                     const uint16_t* w2_init, int n_init, const uint16_t* w2_seg, const float* bias_seg, int n_seg,
                     const uint16_t* w2_dd, const float* bias_dd, int stuff_lo, int n_stuff,
                     uint16_t* x_planes, uint16_t* dfe_planes, float* x_f32 /* nullable */, float* dfe_f32 /* nullable */,
                     void* mask_preds, void* seg_preds, void* depth_pred, int out_dtype,
                     uint32_t* bits /* nullable */, int bits_rows,
                     void* workspace, size_t workspace_bytes, int B, int64_t HW, int prec, int input_format, void* stream);
int ph_khead_onepass_status(const void* workspace, int B, void* stream);
int ph_khead_onepass_timeouts(const void* workspace, int B, int64_t HW, void* stream);
void ph_khead_onepass_set_timeout_us(int microseconds /* <= 0: the default */);
/* debugging aid: device buffer [grid][2][3 * rounds][16] uint64 filled with s_memtime stamps by the following launches (NULL: off) */
void ph_khead_onepass_set_timeline(void* buf);
int ph_khead_proposals(const float* partial, int nsplit, const float* w_init /*[Nq][256]*/,
                       const float* w_stuff /*[n_stuff][256]*/, float* proposal_feats,
                       int B, int n_thing_queries, int n_stuff, void* stream);

/* ---- N4 (first part): matching costs of the mask Hungarian assigner (polyphonic/funcs/assigner.py:113-129 DiceCost,
 * :164-194 MaskCost with pred_act = sigmoid, gt_valid as MaskHungarianAssignerWithDepth.assign :478-498 passes it) --
 * every pixel sum of B images in one pass: logits fp32 [B][N][HW] (mask logits, sigmoid applied inside), gt fp32
 * [B][G][HW] (soft masks; pad unused rows with zeros), valid fp32 [B][HW] of 0/1 or NULL.  N <= 256, G <= 127.
 * partial: fp32 [B][ph_match_nsplit(HW, B)][ph_match_record_floats(N, G)]; the caller adds the records of one image in
 * order.  Record (Npad = ph_n_padded(N), Gpad = ph_n_padded(G + 1)):
 *   A[Npad][Gpad] (A[n][g] = sum p t v; column G = S[n] = sum p v) | Q[Npad] = sum p^2 v | C[Gpad] = sum t^2 v |
 *   T[Gpad] = sum t v | V = sum v. */
int64_t ph_match_record_floats(int N, int G);
int ph_match_nsplit(int64_t HW, int B);
int ph_match_sums(const float* logits, const float* gt, const float* valid, float* partial, int B, int N, int G,
                  int64_t HW, void* stream);

/* ---- N4 (training path): the pixel passes of one stage's losses, kernel_update_head.py:355-441 ------------------------------
 * Every *_sums entry writes fixed-order partial records (doubles, one per workgroup) that the caller adds up in index
 * order; every *_grad entry writes d loss / d logits given the coefficients the caller derives from those sums.
 *  mask : positive prediction rows `pos_rows[P]` of pred / target / weight [rows][HW]; out [P][nsplit][5] = sum BCE-with-logits,
 *         pixel count, a = sum sig t, b = sum sig^2, c = sum t^2 over the pixels with weight != 0 (loss_mask: mmdet
 *         cross_entropy_loss.py:74-113, loss_dice: dice_loss.py:9-46).  grad += coef[p][0] (sig - t) + (coef[p][1] t + coef[p][2] sig)
 *         sig (1 - sig) on those pixels.
 *  rank : softmax cross entropy over the N mask channels of each pixel against rank_target [B][HW] (int32, ignore_index),
 *         cross_entropy_loss.py:9-47; out [B * ph_rank_loss_blocks(HW)]; grad (overwritten, all N channels) = scale (softmax - onehot).
 *  depth: DepthLoss (polyphonic/losses/depth_loss.py:9-65) over 0 < target < 80, weight != 0; out [blocks][5] = n, sum lm^2, sum lm,
 *         sum r^2, sum |r| with lm = (log p - log t) w, r = (p - t) w / t, p = depth_act(pred); grad (overwritten) =
 *         ((c0 lm + c1) w / p + (c2 r + c3 sign r) w / t) depth_act'(pred).
 *  focal: py_sigmoid_focal_loss (focal_loss.py:12-60) on pred [R][L], labels [R] (>= L: background), weight [R][L]. */
int ph_mask_loss_sums(const float* pred, const float* target, const float* weight, const int32_t* pos_rows, int P, int64_t HW,
                      int nsplit, double* out, void* stream);
int ph_mask_loss_grad(const float* pred, const float* target, const float* weight, const int32_t* pos_rows, int P, int64_t HW,
                      const float* coef, float* grad, void* stream);
int ph_rank_loss_blocks(int64_t HW);
int ph_rank_loss_sum(const float* pred, const int32_t* rank_target, int B, int N, int64_t HW, int ignore_index, double* out,
                     void* stream);
int ph_rank_loss_grad(const float* pred, const int32_t* rank_target, int B, int N, int64_t HW, int ignore_index, float scale,
                      float* grad, void* stream);
int ph_depth_loss_blocks(int64_t total);
int ph_depth_loss_sums(const float* pred, const float* target, const float* weight, int64_t total, int depth_mode, double* out,
                       void* stream);
int ph_depth_loss_grad(const float* pred, const float* target, const float* weight, int64_t total, int depth_mode, float c0,
                       float c1, float c2, float c3, float* grad, void* stream);
int ph_focal_loss_blocks(int64_t total);
int ph_focal_loss_sum(const float* pred, const int64_t* labels, const float* weight, int64_t R, int L, float gamma, float alpha,
                      double* out, void* stream);
int ph_focal_loss_grad(const float* pred, const int64_t* labels, const float* weight, int64_t R, int L, float gamma, float alpha,
                       float scale, float* grad, void* stream);
/* the same focal loss over a class-major map: pred [B][L][HW], target int32 [B][HW] (== L: pixel not selected) -- KernelHead's
 * loss_rpn_seg, kernel_head.py:538-551; out [B * ph_rank_loss_blocks(HW)], grad [B][L][HW] (overwritten) */
int ph_seg_focal_sum(const float* pred, const int32_t* target, int B, int L, int64_t HW, float gamma, float alpha, double* out,
                     void* stream);
int ph_seg_focal_grad(const float* pred, const int32_t* target, int B, int L, int64_t HW, float gamma, float alpha, float scale,
                      float* grad, void* stream);

/* target assembly of the losses above.  rank_target: out[b][p] = the last j with pos[b*N + j] and mask_targets[b*N + j][p] != 0,
 * else ignore_index (kernel_update_head.py:420-432).  seg_target (one image): L, then sem_cls[s] where sem_seg[s] != 0 in order,
 * then pos_labels[i] where pos_masks[i] != 0 in order (kernel_head.py:590-605). */
int ph_rank_target(const float* mask_targets, const uint8_t* pos, int B, int N, int64_t HW, int ignore_index, int32_t* out,
                   void* stream);
int ph_seg_target(const float* sem_seg, const int64_t* sem_cls, int S, const float* pos_masks, const int64_t* pos_labels, int P,
                  int L, int64_t HW, int64_t* out, void* stream);

/* DepthCost (funcs/assigner.py:17-80): out[n][g] = { sum lm^2, sum lm, sum r^2, sum |r| } over the pixels with
 * gt_depth * gt_masks[g] > 0, lm = log(depth_act(z_n) + eps) - log(gt_depth * gt_masks[g] + eps), r = (d - t) / t;
 * nvalid[g] = number of those pixels.  depth_mode: 0 'sigmoid', 1 'monodepth' (funcs/depth_utils.py). */
int ph_depth_cost_sums(const float* depth_logits, const float* gt_depth, const float* gt_masks, int N, int G, int64_t HW,
                       int depth_mode, float eps, float* out, float* nvalid, void* stream);

/* ---- N4, backward: the map-sized products on fp32 NCHW maps (csrc/ph_train.hip); hi+lo bf16 MFMA, fp32 grade ----------------
 * rows_x_map : Y[b][m][p] = sum_k A[b][m][k] X[b][k][p].  A [B or 1][Mpad][lda] zero padded (Mpad % 16 == 0, lda % 8 == 0),
 *              a_batch_stride in elements (0: one A for every image).  binarize_x: X is used as (X > 1.5 * 2^-24) ? 1 : 0.
 *              Replaces F.conv2d with 1x1 static / dynamic kernels (kernel_head.py:250-295, kernel_update_head.py:317-329)
 *              and autograd's grad_input of those and of the einsum pooling (kernel_update_head.py:241-242).
 * map_x_mapT : O[b][m][k] = sum_p G[b][m][p] X[b][k][p], K <= 256.  nsplit from ph_map_x_map_t_nsplit; partial holds
 *              B * nsplit * M * K floats, summed in a fixed order.  binarize_g as above (the hard-mask pooling forward).
 * upsample2x_bwd : transpose of ph_upsample2x (F.interpolate x2 bilinear, align_corners=False). */
int ph_rows_x_map(const float* A, int64_t a_batch_stride, int lda, int Mpad, int M, int K, const float* X, float* Y, int B, int64_t HW,
                  int binarize_x, void* stream);
int ph_map_x_map_t_nsplit(int B, int M, int64_t HW);
int ph_map_x_map_t(const float* G, const float* X, float* partial, float* out, int B, int M, int K, int64_t HW, int nsplit,
                  int binarize_g, void* stream);
int ph_upsample2x_bwd(const float* grad_out, float* grad_in, int64_t planes, int H, int W, void* stream);
/* round 5: _ex forms.  rows_x_map: bias [B][M] (nullable) added to every pixel of row m -- the scalar bias of a folded dynamic
 * kernel, kernel_update_head.py:317-329 --, add [B][M][HW] (nullable, may be Y itself): Y = A X + add (a second gradient
 * contribution lands where the first one lies).
 * map_x_mapT: rowsum [B][M] = sum_p G[b][m][p] (binarised: the pixel count of each hard mask; otherwise the gradient of a dynamic
 * kernel's scalar bias), rs_partial [B][nsplit][M] its per-split scratch; both null or both given.
 * hard_count: out[r] = #{p : sigmoid(logits[r][p]) > 0.5}. */
int ph_rows_x_map_ex(const float* A, int64_t a_batch_stride, int lda, int Mpad, int M, int K, const float* X, float* Y, int B,
                     int64_t HW, int binarize_x, const float* bias, const float* add, void* stream);
int ph_map_x_map_t_ex(const float* G, const float* X, float* partial, float* out, int B, int M, int K, int64_t HW, int nsplit,
                      int binarize_g, float* rs_partial, float* rowsum, int sum_batch, void* stream);
/* GroupNorm + ReLU of a ConvModule in training mode, fp32 NCHW (csrc/ph_gntrain.hip; kernel_head.py:250-278, semantic_fpn.py:75-178).
 * fwd: out = relu(GN(y)) (nullable when out_sum is given); out_sum = out + add (both null or both given: KernelHead's
 *      x_feats = sem + loc, the neck's sum over its towers); stats [B][groups][2]
 *      (mean, rstd) kept for the backward; partial: B * groups * ph_gn_train_nsplit(HW, C / groups) * 2 doubles of scratch.
 * bwd: dy = dyA (+ dyB) masked by out > 0 (recomputed from y); dx, dgamma [C], dbeta [C] are overwritten;
 *      partial: B * C * ph_gn_train_bwd_nsplit(HW) * 2 doubles of scratch.  sum_batch != 0 in ph_map_x_map_t_ex: out [M][K] and
 *      rowsum [M] are summed over the images as well (the gradient of a static 1x1 kernel and of its bias). */
/* 3x3 convolutions of SemanticFPNWrapper's towers in training (fp32 NCHW, csrc/ph_train.hip; semantic_fpn.py:75-150):
 * conv3x3_taps : W [M][K][3][3] <-> tap-major [9][M][K] (transpose: [9][K][M]; flip: tap 8 - t -- together the operand of the input
 *                gradient of a stride-1 conv); to_weight != 0 runs the inverse (a tap-major weight gradient back to [M][K][3][3]).
 * conv3x3_train: Y [B][M][Ho][Wo] = sum_tap taps[tap] X[.., src_tap(.)], X [B][K][Hi][Wi]; mode 0: forward with `stride` (also the
 *                input gradient of a stride-1 conv with flipped / transposed taps), mode 1: input gradient of the stride-2 conv
 *                (X = dL/dY [Hi][Wi], Y = dL/dX [Ho][Wo], taps transposed, NOT flipped).
 * conv3x3_wgrad: tap-major dW [9][M][K] summed over the batch; partial: B * nsplit * M * K floats (nsplit: ph_map_x_map_t_nsplit). */
int ph_conv3x3_taps(const float* W, float* taps, int M, int K, int transpose, int flip, int to_weight, void* stream);
int ph_conv3x3_train(const float* taps, int M, int K, const float* X, float* Y, int B, int Hi, int Wi, int Ho, int Wo, int stride,
                     int mode, void* stream);
int ph_conv3x3_wgrad(const float* dY, const float* X, float* partial, float* taps_out, int B, int M, int K, int Hi, int Wi, int Ho,
                     int Wo, int stride, int nsplit, void* stream);
int ph_gn_train_nsplit(int64_t HW, int cpg);
int ph_gn_train_bwd_nsplit(int64_t HW);
int ph_gn_train_fwd(const float* y, const float* gamma, const float* beta, int groups, float eps, const float* add, float* out,
                    float* out_sum, float* stats, double* partial, int B, int C, int64_t HW, void* stream);
int ph_gn_train_bwd(const float* y, const float* stats, const float* gamma, const float* beta, int groups, const float* dyA,
                    const float* dyB, float* dx, float* dgamma, float* dbeta, double* partial, int B, int C, int64_t HW, void* stream);
int ph_hard_count(const float* logits, float* out, int64_t rows, int64_t HW, void* stream);
/* FPN in training (fp32 NCHW, csrc/ph_fpntrain.hip; mmdet/models/necks/fpn.py:151-203): what the lateral 1x1 convolutions, the
 * top-down pathway and the biased 3x3 output convolutions need beyond the calls above.  Launch-only, no atomics, fixed-order sums.
 * map_x_map_t_wide : ph_map_x_map_t_ex without binarize_g for any K in 1 .. 4096 (K tiles of 256 columns; for K <= 256 and the
 *                same nsplit the same bits): O[b][m][k] = sum_p G[b][m][p] X[b][k][p], rowsum [B][M] = sum_p G (both null or both given with rs_partial
 *                [B][nsplit][M]), sum_batch != 0: out [M][K] and rowsum [M] summed over the images too -- the weight and bias
 *                gradients of a lateral convolution.  nsplit from ph_map_x_map_t_wide_nsplit (the workgroup budget divided by row
 *                passes and K tiles, at least 256 pixels per split); partial holds B * nsplit * M * K floats.
 * nearest_up_add : in place fine[pl][y][x] += coarse[pl][y * Hc / H][x * Wc / W] (F.interpolate nearest to the finer size + add);
 *                H must be 2 Hc or 2 Hc - 1 and W must be 2 Wc or 2 Wc - 1 (ph_fpn_lateral's rule: there the source index is y >> 1).
 * nearest_up_add_bwd : its transpose as a gather: g_coarse[pl][Y][X] (accumulate != 0: the value already there, else 0) + g_fine[2Y][2X]
 *                + g_fine[2Y][2X+1] + g_fine[2Y+1][2X] + g_fine[2Y+1][2X+1], in-bounds terms only, added in that order.
 * nchw_bias_add : in place y[b][c][p] += bias[c].   nchw_channel_sums : out[c] = sum_b sum_p g[b][c][p], accumulated in fp64 in a
 *                fixed order; partial: C * B * ph_nchw_channel_sums_nsplit(HW) doubles of scratch. */
int ph_map_x_map_t_wide_nsplit(int B, int M, int K, int64_t HW);
int ph_map_x_map_t_wide(const float* G, const float* X, float* partial, float* out, int B, int M, int K, int64_t HW, int nsplit,
                        float* rs_partial, float* rowsum, int sum_batch, void* stream);
int ph_nearest_up_add(float* fine, const float* coarse, int64_t planes, int H, int W, int Hc, int Wc, void* stream);
int ph_nearest_up_add_bwd(const float* g_fine, float* g_coarse, int64_t planes, int H, int W, int Hc, int Wc, int accumulate,
                          void* stream);
int ph_nchw_bias_add(float* y, const float* bias, int B, int C, int64_t HW, void* stream);
int ph_nchw_channel_sums_nsplit(int64_t HW);
int ph_nchw_channel_sums(const float* g, double* partial, float* out, int B, int C, int64_t HW, void* stream);

/* ---- N4: targets + losses + d(losses)/d(predictions) of one head / stage in ONE call, from DESCRIPTORS (csrc/ph_loss.hip) ------
 * Replaces `get_targets` + `loss` of both heads on the training path (kernel_update_head.py:355-591, kernel_head.py:456-698): every
 * target / weight row the reference materialises is a ground-truth mask, the image's valid map, its depth map, ones or zeros,
 * so rows are described by device POINTERS (int64 addresses of fp32 rows of HW pixels):
 *   pos_rows int32 [P] (rows with a label in [0, L)), pos_u8 [B*N]; tptr / wptr int64 [B*N]: mask target / weight row (0 = zeros);
 *   depth items grouped per prediction row: dstart int32 [depth_rows + 1], dit_t (target row), dit_w (weight row; 1 = ones),
 *   dit_s (scale; the weight is scale * row, and the reference's `* (gt_depth > 0)` is the kernel's own `0 < target < 80`);
 *   labels int64 [B*N], label_w fp32 [B*N][L] (nullable together with cls_score: KernelHead has no classification);
 *   KernelHead only: seg_pred [B][seg_L][HW] with the paint lists of the dense semantic target (kernel_head.py:590-605):
 *   sstart int32 [B + 1], sit_m (mask row), sit_l (class), painted in order over background = seg_L.
 * mask_pred [B][N][HW]; depth_pred [depth_rows][HW] (KernelHead: the ONE direct depth map per image, all its items summed).
 * losses [8] (device): loss_depth, loss_cls, mask BCE, dice, rank, seg focal, pos_acc, number of labelled seg pixels -- weighted as
 * the reference's loss modules weight them.  g_* nullable all together: d(sum of the losses)/d(prediction), overwritten.
 * Loss values and gradient coefficients are formed on the device (fp64, fixed order): no host round trip inside the call. */
typedef struct {
    int32_t B, N, L, P, depth_rows, seg_L, has_rank, ignore, depth_mode;
    int64_t HW;
    float lw_mask, lw_dice, dice_eps, lw_rank, lw_depth, dw_si, dw_sq, dw_abs, lw_cls, cls_gamma, cls_alpha, cls_avg, lw_seg, seg_gamma,
        seg_alpha;
} ph_loss_cfg;
size_t ph_train_losses_scratch_bytes(const ph_loss_cfg* cfg);
int ph_train_losses(const ph_loss_cfg* cfg, const float* mask_pred, const float* cls_score, const float* depth_pred,
                    const float* seg_pred, const int32_t* pos_rows, const uint8_t* pos_u8, const int64_t* tptr, const int64_t* wptr,
                    const int32_t* dstart, const int64_t* dit_t, const int64_t* dit_w, const float* dit_s, const int64_t* labels,
                    const float* label_w, const int32_t* sstart, const int64_t* sit_m, const int32_t* sit_l, float* losses,
                    float* g_mask, float* g_cls, float* g_depth, float* g_seg, void* scratch, size_t scratch_bytes, void* stream);

/* ---- N4, device half: the QUERY SIDE of one KernelUpdateHead stage in TRAINING mode (csrc/ph_qtrain.hip) -------------------
 * Replaces what autograd records for kernel_update_head.py:245-288 (KernelUpdator x2, funcs/kernel_updator.py:55-93; mmcv
 * MultiheadAttention + LayerNorm x2; FFN + LayerNorm x2; cls_fcs / mask_fcs / depth_regs + fc_cls / fc_mask / fc_depth) and its
 * backward.  Rows r = b * N + n of 256 features; two branches (0 mask, 1 depth).  fp32 in, fp32 out, fp32 MFMA products.
 * params: HOST array [2][PH_QTRAIN_NPARAM] of DEVICE pointers to the fp32 parameters as nn.Parameter stores them ([out][in]
 * weights), per branch in this order (mask-branch names; the depth branch: *_depth, depth_regs / fc_depth for 34-38, 39-43 null):
 *   0 feat_transform.conv.weight  1 .bias | kernel_update_conv: 2 dynamic_layer.weight 3 .bias 4 input_layer.weight 5 .bias
 *   6 input_gate.weight 7 .bias 8 update_gate.weight 9 .bias 10 input_norm_in.weight 11 .bias 12 norm_in.weight 13 .bias
 *   14 norm_out.weight 15 .bias 16 input_norm_out.weight 17 .bias 18 fc_layer.weight 19 .bias 20 fc_norm.weight 21 .bias |
 *   22 attention.attn.in_proj_weight 23 in_proj_bias 24 out_proj.weight 25 out_proj.bias 26 attention_norm.weight 27 .bias |
 *   28 ffn.layers.0.0.weight 29 .bias 30 ffn.layers.1.weight 31 .bias 32 ffn_norm.weight 33 .bias |
 *   34 mask_fcs.0.weight 35 mask_fcs.1.weight 36 mask_fcs.1.bias 37 fc_mask.weight 38 fc_mask.bias |
 *   39 cls_fcs.0.weight 40 cls_fcs.1.weight 41 cls_fcs.1.bias 42 fc_cls.weight 43 fc_cls.bias
 * forward : pooled [2][R][256] = the hard-mask pooling of x / depth_feats BEFORE feat_transform (folded: pooling is linear in it),
 *           cnt [R] = pixels of each hard mask, k [R][256] kernels, q [R][256] depth kernels (the kernel k.detach() is added inside,
 *           :250).  Writes cls [R][L], kern [2][R][256] = fc_mask / fc_depth outputs folded with feat_transform's weight,
 *           kbias [2][R] = their product with its bias, obj [2][R][256] = the updated kernels; `saved` (ph_qtrain_saved_floats)
 *           keeps the pre-normalisation rows, activations and attention probabilities the backward needs.
 * backward: gradients w.r.t. cls, kern, kbias, obj in; writes grads [2][PH_QTRAIN_NPARAM] (HOST array of device pointers, each
 *           the size of its parameter; every one is overwritten, none accumulated), g_pooled [2][R][256], g_k, g_q [R][256].
 *           `scratch`: ph_qtrain_scratch_floats.  Fixed summation orders throughout (no atomics). */
/* ph_gemm32: one product of the training side's fp32-MFMA tile GEMM on its own (tests, timing): C [M][N] = A(m,k) B(k,n) (+ bias[n]);
 * kcA / kcB != 0: the operand is k-contiguous (X [row][k] / W [out][in]), else row-contiguous ([k][row]); ksplit > 1: C [ksplit][M][ldc] */
int ph_gemm32(const float* A, int lda, int kcA, const float* B, int ldb, int kcB, float* C, int ldc, int M, int N, int K, int ksplit,
              const float* bias, void* stream);
#define PH_QTRAIN_NPARAM 44
size_t ph_qtrain_saved_floats(int B, int N, int L, int F);
size_t ph_qtrain_scratch_floats(int B, int N, int L, int F);
int ph_qtrain_forward(const float* const* params, const float* pooled, const float* cnt, const float* k, const float* q, float* cls,
                      float* kern, float* kbias, float* obj, float* saved, int B, int N, int L, int F, void* stream);
int ph_qtrain_backward(const float* const* params, const float* pooled, const float* cnt, const float* k, const float* q,
                       const float* saved, const float* g_cls, const float* g_kern, const float* g_kbias, const float* g_obj,
                       float* const* grads, float* g_pooled, float* g_k, float* g_q, float* scratch, int B, int N, int L, int F,
                       void* stream);

/* ---- A16-A18: panoptic merge (kernel_update.py:421-535, kernel_update_head.py:593-626) -------
 * geom = {sh, sw, Hb, Wb, h, w, Ho, Wo}: stride-4 source size, batch_input_shape, img_shape, ori_shape.
 * activate: act_mask[k] = sigmoid(mask_up[q_idx[k]]), act_depth[k] = depth_act(depth_up[q_idx[k]]),
 *           act_depth0 = depth_act(depth_init_up); logits fp32 or bf16 ([N][sh][sw]), outputs fp32.
 * argmax  : ids[px] = first argmax_k scores[k] * rescale(act_mask[k])(px); counts[0][k] = #{ids == k},
 *           counts[1][k] = #{rescale(act_mask[k]) >= 0.5} (counts zeroed by the call).
 * paste   : pan = newid[ids]; depth_final = newid[ids] > 0 ? rescale(act_depth[ids]) : rescale(act_depth0).
 * from_probs != 0: act_* are already full-resolution [K][Ho][Wo] maps (no resampling) -- the integer
 * semantics in isolation. The accept loop between argmax and paste (:500-533) is host logic here; ph_panoptic_accept below
 * is the same step on the device. */
/* select  : the segment candidates of kernel_update.py:428-434 / :448-459 on the device, for B frames: the top max_per_img
 *           (query, thing class) pairs of cls_scores [B][N][L] (post-sigmoid) in descending order, then the stuff queries'
 *           own-class scores (the diagonal of the [N - num_proposals] x [L - num_thing_classes] block) in descending order;
 *           q_idx / labels / scores [B][out_batch_stride], K = max_per_img + stuff entries each.  Ties: ascending index. */
int ph_panoptic_select(const float* cls_scores, int64_t cls_batch_stride, int B, int N, int L, int num_proposals,
                       int num_thing_classes, int max_per_img, int32_t* q_idx, int32_t* labels, float* scores,
                       int64_t out_batch_stride, void* stream);
int ph_panoptic_activate(const void* mask_up, const void* depth_up, int dtype, const float* depth_init_up,
                         const int32_t* q_idx, int K, int h2, int w2, int depth_mode /*0 sigmoid, 1 monodepth*/,
                         float* act_mask, float* act_depth, float* act_depth0, void* stream);
int ph_panoptic_argmax(const float* act_mask, const float* scores, int K, const int32_t* geom, int from_probs,
                       int32_t* ids, int32_t* counts /*[2][K]*/, void* stream);
int ph_panoptic_paste(const int32_t* ids, const int32_t* newid, const float* act_depth, const float* act_depth0,
                      const int32_t* geom, int from_probs, int32_t* pan, float* depth_basic, float* depth_final,
                      void* stream);

/* ---- the merge as launches only, for B frames of ONE geometry -------------------------------
 * accept  : the accept step (kernel_update.py:497-533) on the device, one workgroup per frame.  Per frame it reads labels[K],
 *           scores[K] and counts[2][K] as select and argmax leave them (the three pointers advance by in_batch_stride elements
 *           per frame) and writes newid[K] (0 = rejected), nseg, and the record table seg[K][4] = {new id, candidate index k,
 *           label, area} with rows in id order and the unused rows zero (nseg and seg advance by rec_batch_stride int32 per
 *           frame).  A thing is rejected when score < (float)instance_score_thr, evaluated in fp32; every candidate needs
 *           area > 0 && orig > 0 and !((double)area / (double)orig < overlap_thr), one IEEE fp64 division.  Kept candidates are
 *           numbered 1.. in the order of a stable descending sort of the scores: ties by ascending index, NaN last
 *           (torch.argsort(-scores, stable=True)).  K <= 4096.
 * *_batch : ph_panoptic_activate / _argmax / _paste for B frames in one launch each -- the same kernels with the frame in the
 *           grid; the single-frame calls are their B = 1 case.  Logits [B][N][h2][w2]; act_mask / act_depth [B][K][..],
 *           act_depth0 [B][..], ids / pan / depths [B][Ho][Wo] dense; q_idx, scores, counts and newid advance by the given
 *           stride (in elements) per frame.  generic_only != 0: never the x4 form of the argmax (tests); no environment is read.
 * merge   : select -> activate -> clear + argmax -> accept -> paste from the decode's outputs (ph_decode_io cls, mask_up, depth_up
 *           and ph_upsample2x of KernelHead's direct depth) to the id and depth maps.  Enqueue only: no allocation, no
 *           synchronisation, no environment variable; capturable in a HIP graph.  K = max_per_img + min(N - num_proposals,
 *           L - num_thing_classes).  The workspace (256-byte aligned, ph_panoptic_merge_workspace_bytes) holds the candidate pack
 *           [B][5K], act_mask, act_depth, act_depth0, ids and newid.  seg_records [B][1 + 5K] int32 per frame:
 *           nseg | seg[K][4] | scores[K] as fp32 bits -- all a host needs for the reference's segments_info.
 *           PH_EINVAL / PH_EUNSUPPORTED / PH_EWORKSPACE are returned before the first launch (message: ph_last_error_string);
 *           the size query returns 0 for a bad size, with a message.  Candidate order among exactly equal scores is
 *           ph_panoptic_select's: ascending index. */
int ph_panoptic_accept(const int32_t* labels, const float* scores, const int32_t* counts /*[2][K]*/, int64_t in_batch_stride, int B,
                       int K, int num_thing_classes, double instance_score_thr, double overlap_thr, int32_t* newid,
                       int64_t newid_batch_stride, int32_t* nseg, int32_t* seg /*[K][4]*/, int64_t rec_batch_stride, void* stream);
int ph_panoptic_activate_batch(const void* mask_up, const void* depth_up, int dtype, const float* depth_init_up,
                               const int32_t* q_idx, int64_t q_batch_stride, int B, int N, int K, int h2, int w2, int depth_mode,
                               float* act_mask, float* act_depth, float* act_depth0, void* stream);
int ph_panoptic_argmax_batch(const float* act_mask, const float* scores, int64_t scores_batch_stride, int B, int K,
                             const int32_t* geom, int from_probs, int generic_only, int32_t* ids, int32_t* counts,
                             int64_t counts_batch_stride, void* stream);
int ph_panoptic_paste_batch(const int32_t* ids, const int32_t* newid, int64_t newid_batch_stride, const float* act_depth,
                            const float* act_depth0, int B, int K, const int32_t* geom, int from_probs, int32_t* pan,
                            float* depth_basic, float* depth_final, void* stream);
size_t ph_panoptic_merge_workspace_bytes(int B, int K, int h2, int w2, const int32_t* geom);
int ph_panoptic_merge(const float* cls /*[B][N][L]*/, const void* mask_up, const void* depth_up, int dtype,
                      const float* depth_init_up /*[B][h2][w2]*/, int B, int N, int L, int num_proposals, int num_thing_classes,
                      int max_per_img, int h2, int w2, const int32_t* geom /*one for the batch*/, int depth_mode,
                      double instance_score_thr, double overlap_thr, void* workspace, size_t workspace_bytes,
                      int32_t* pan /*[B][Ho][Wo]*/, float* depth_basic, float* depth_final,
                      int32_t* seg_records /*[B][1 + 5K]: nseg | seg[K][4] | scores[K] as fp32 bits*/, void* stream);

/* ---- device side of the video association step (polyphonic_former_video.py:359-396) ----------
 * ph_segment_boxes : int32 panoptic id map [H][W], segment ids 1..nseg -> rois [nseg][5] = (0, x1, y1, x2, y2)
 *                    (centre +- 2 * mean |deviation| per axis, clamped at 0: polyphonic/video/utils.py:39-83,
 *                    polyphonic_former_video.py:413-415) and tight extent boxes [nseg][4] (funcs/utils.py:4-22).
 * ph_roi_align_fpn : mmdet SingleRoIExtractor (level = floor(log2(sqrt(area)/56 + 1e-6))) + mmcv RoIAlign(7,
 *                    sampling_ratio 2, avg, aligned) over `nlev` fp32 maps [1][256][H_l][W_l] (feats = host array of
 *                    device pointers, hw = {H_0, W_0, H_1, ...}, scales = 1/stride) -> channels-last bf16 planes
 *                    [P][n][49][256] (+ optional fp32 [n][256][7][7]).
 * ph_gemm_rows     : Y[M][N] = act(X[M][K] W^T + b), X bf16 planes [P][M][K], W packed B fragments (plane stride
 *                    given), Y fp32 and/or bf16 planes; the track head's conv3x3-as-GEMM, fc and fc_embed
 *                    (polyphonic/video/track_heads.py:92-102).
 * ph_im2col7       : channels-last [P][n][49][256] -> 3x3/pad-1 patches [P][n*49][2304], K order (tap, channel).
 * ph_gn_relu_cl    : per-RoI GroupNorm + ReLU of fp32 [n*49][256] -> channels-last bf16 planes. */
size_t ph_segment_boxes_workspace_bytes(int nseg);
int ph_segment_boxes(const int32_t* pan, int H, int W, int nseg, float* rois, float* ext_boxes,
                     void* workspace, size_t workspace_bytes, void* stream);
int ph_roi_align_fpn(const float* const* feats, const int32_t* hw, const float* scales, int nlev, const float* rois,
                     int n, float finest_scale, uint16_t* out_cl, float* out_f32 /* nullable */, int prec, void* stream);
int ph_gemm_rows(const uint16_t* X, const uint16_t* Wp, int64_t w_plane_elems, const float* bias /* nullable */, int relu,
                 float* Yf /* nullable */, uint16_t* Yp /* nullable */, int M, int N, int K, int prec, void* stream);
int ph_im2col7(const uint16_t* in, uint16_t* out, int n, int prec, void* stream);
/* ph_gemm_rows for the association step's small M (a dozen RoIs): K split over several hundred workgroups, partial sums in
 * `workspace`, added in a fixed order (deterministic; the split depends on M, N, K only).  im2col7 = 1: X is the channels-last
 * [P][M / 49][49][256] maps and the 3x3 / pad-1 patches are gathered by the operand loads (K = 2304; what ph_im2col7 +
 * ph_gemm_rows compute through a materialised matrix). */
size_t ph_gemm_rows_workspace_bytes(int M, int N, int K);
int ph_gemm_rows_splitk(const uint16_t* X, int im2col7, const uint16_t* Wp, int64_t w_plane_elems, const float* bias /* nullable */,
                        int relu, float* Yf /* nullable */, uint16_t* Yp /* nullable */, int M, int N, int K, int prec,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Tracker affinity (quasi_dense_embed_tracker.py:165-182) on the device, next to the embeddings: score[n][m] between the n
 * detections (emb fp32 [n][256], labels int32 [n]) and the m memory columns (memo_emb fp32 [m][256], memo_labels int32 [m]);
 * metric 0 = bisoftmax, 1 = softmax, 2 = cosine; with_cats: zero where the labels differ.  n <= 128, m <= 4096.  The greedy
 * assignment that consumes the matrix is host logic (video.QuasiDenseEmbedTracker). */
size_t ph_track_affinity_workspace_bytes(int n, int m);
int ph_track_affinity(const float* emb, const int32_t* labels, const float* memo_emb, const int32_t* memo_labels, int n, int m,
                      int metric, int with_cats, float* score, void* workspace, size_t workspace_bytes, void* stream);
int ph_gn_relu_cl(const float* y, const float* gamma, const float* beta, int groups, float eps, uint16_t* out, int n,
                  int prec, void* stream);

/* ---- the step before the path, SemanticFPNWrapper.forward (polyphonic/funcs/semantic_fpn.py:198-235,
 * configs/_base_/models/polyphonic_former.py:78-96).  Inside the neck every map is channels-last (NHWC):
 * ph_nhwc_ingest : fp32 NCHW [B][256][HW] (+ add[256][HW], nullable: SinePositionalEncoding on level 3, :202-208)
 *                  -> bf16 NHWC planes [P][B][HW][256].
 * ph_conv_nhwc   : ConvModule's conv (no bias): KSxKS, pad KS/2, stride 1 or 2 (3x3) / 1 (1x1), 256 -> 256 channels;
 *                  X bf16 NHWC planes, Wp = pack.pack_b32 fragments of W[n][tap * 256 + c], Y fp32 NHWC [B][Ho][Wo][256];
 *                  partial = per-channel (sum, sum of squares) of every (row pair, column tile) [B][nwg][256][2]
 *                  (ph_conv_nhwc_partial_floats) for the GroupNorm that follows.
 * ph_gn_finalize : partial -> stats [B][groups][2] = (mean, rstd), fp64 combine (also used by ph_khead_conv_gn).
 * ph_gn_apply    : GroupNorm affine + ReLU on fp32 NHWC (stats == NULL: plain copy/convert), then per `mode`:
 *                  bf16 NHWC planes | x2 bilinear (align_corners=False, nn.Upsample :131-134) bf16 NHWC planes |
 *                  fp32 NHWC accumulate | fp32 NCHW (what KernelHead takes; LDS transpose).
 * ph_gn_sum_planes: sum over `nlev` <= 4 levels of ReLU(GroupNorm(y_l)) -> bf16 NHWC planes (the sum over levels, :221,
 *                  without an fp32 sum buffer); ys / stats / gammas / betas are HOST arrays of `nlev` device pointers. */
int ph_nhwc_ingest(const float* src, const float* add /* nullable */, uint16_t* dst, int B, int64_t HW, int prec, void* stream);
size_t ph_conv_nhwc_partial_floats(int B, int Ho, int Wo);                     /* upper bound, any instantiation */
/* `nwg` for ph_gn_finalize = entries per frame of ph_conv_nhwc's `partial` output: one per (pair of output rows, 64-pixel column
   tile) whatever tile form the launch takes (round 6: batch-invariant partial sums; rounds 3-5 it was the workgroups of the
   chosen form, hence the arguments) */
int ph_conv_nhwc_workgroups_b(int ksize, int stride, int Ho, int Wo, int prec, int B);
int ph_conv_nhwc(const uint16_t* X, const uint16_t* Wp, int64_t w_plane_elems, float* Y, float* partial, int ksize, int stride,
                 int B, int H, int W, int prec, void* stream);
int ph_gn_finalize(const float* partial, float* stats, int nwg, int groups, int64_t HW, float eps, int B, void* stream);
int ph_gn_sum_planes(const float* const* ys, const float* const* stats, const float* const* gammas, const float* const* betas,
                     int nlev, int groups, uint16_t* planes, int B, int64_t HW, int prec, void* stream);
/* ph_neck_out_convs: conv_pred + the two aux convs (semantic_fpn.py:156-178,223-231; each 1x1 conv + GN + ReLU of the level sum)
 * in two passes over that sum -- statistics by recomputation, then normalise + ReLU + store -- without an fp32 conv output in
 * memory.  in_channels_last == 0: the sum as CHANNEL planes [P][B][256][HWp] (zero in [HW, HWp)); != 0: ph_gn_sum_planes'
 * [P][B][HW][256] instead (a 64-pixel tile is 32 KiB of consecutive
 * bytes and its B fragments are plain 16-byte LDS reads: no transposition anywhere -- the form NeckPlan uses).
 * wplanes: 16-bit planes [P][3][256][256] (out, in) of the three conv weights; gn_affine fp32 [3][2][256];
 * out_planes_m: 16-bit planes [P][B][256][HWp] and / or out_f32_m: fp32 NCHW [B][256][HW], at least one per map;
 * workspace: ph_neck_out_convs_workspace_bytes(B, HW, groups).  Up to 3 frames per launch a frame's outputs are bit-identical to
 * those of a one-frame launch (tile runs and summation order do not depend on B). */
size_t ph_neck_out_convs_workspace_bytes(int B, int64_t HW, int groups);
int ph_neck_out_convs(const uint16_t* in_planes, int in_channels_last, const uint16_t* wplanes, const float* gn_affine, int groups,
                      float eps, uint16_t* out_planes0, uint16_t* out_planes1, uint16_t* out_planes2, float* out_f32_0,
                      float* out_f32_1, float* out_f32_2, void* workspace, size_t workspace_bytes, int B, int64_t HW, int prec,
                      void* stream);
int ph_gn_apply(const float* y, const float* stats /* nullable */, const float* gamma, const float* beta, int groups, int mode,
                int accumulate, uint16_t* planes /* nullable */, float* outf /* nullable */, int B, int H, int W, int prec,
                void* stream);

/* ---- FPN: the step before the neck (mmdet/models/necks/fpn.py:151-203 as configs/_base_/models/polyphonic_former.py:22-29 builds
 * it: four 1x1 lateral convs K -> 256 and four 3x3 output convs 256 -> 256, each with bias, no norm, no activation, nearest top-down
 * add).  Every call launches only: no allocation, no synchronisation, no environment variable.
 * ph_fpn_lateral : one level's lateral conv + top-down add (fpn.py:157-173).  x: the backbone stage, NCHW-contiguous [B][K][H * W] of
 *                  x_dtype PH_OUT_F32 / PH_OUT_BF16 / PH_OUT_F16, K a multiple of 64 in [64, 4096]; every element is read once and
 *                  converted through fp32 to the grade's 16-bit format inside the kernel.  Wp: pack.pack_b32 fragments of W[256][K],
 *                  one blob per plane (w_plane_elems = 256 K); bias fp32 [256].  coarse (nullable): the finished lateral of the next
 *                  coarser level, planes [P][B][Hc * Wc][256] of the same grade; its value at (min(y Hc / H, Hc - 1),
 *                  min(x Wc / W, Wc - 1)) -- integer division -- is added in fp32 before the one rounding.  That index is
 *                  F.interpolate(mode='nearest', size=(H, W))'s whenever H is 2 Hc or 2 Hc - 1 and W is 2 Wc or 2 Wc - 1 (every
 *                  stride-2 pyramid); any other size pair is PH_EINVAL with a message, never an approximate gather.
 *                  out: 16-bit NHWC planes [P][B][H * W][256], what ph_conv_nhwc reads.  prec PH_PREC_BF16 / PH_PREC_F16: one plane;
 *                  PH_PREC_SPLIT: hi + lo planes of both operands, hi.hi + hi.lo + lo.hi.  fp32 accumulation.  A frame's result
 *                  does not depend on B.  A bad argument leaves `out` untouched.
 * ph_fpn_lateral_cl : ph_fpn_lateral for a stage that is a channels-last 16-bit plane X [B][H * W][K] of grade x_prec (PH_PREC_BF16 /
 *                  PH_PREC_F16: the backbone's plane as ph_conv_cl writes it), 16-byte aligned; every other argument, the K range and
 *                  the size rule are ph_fpn_lateral's.  prec PH_PREC_BF16 / PH_PREC_F16; with x_prec != prec each value goes through
 *                  fp32 to the grade while it is staged.  The same MFMA, B fragments, accumulation order and epilogue: the bits of
 *                  ph_fpn_lateral on ph_cl_to_nchw's tensor of X, without that tensor crossing memory.  PH_PREC_SPLIT is
 *                  PH_EUNSUPPORTED before any launch (the hi + lo grade keeps the NCHW path).
 * ph_fpn_output  : the tail of an output conv (fpn.py:177-179): y = ph_conv_nhwc's fp32 NHWC [B][HW][256] result (ksize 3, stride 1,
 *                  on the lateral planes) + bias[256] -> fp32 NCHW [B][256][HW], the level as the module returns it. */
int ph_fpn_lateral(const void* x, int x_dtype, const uint16_t* Wp, int64_t w_plane_elems, const float* bias,
                   const uint16_t* coarse /* nullable */, int Hc, int Wc, uint16_t* out, int B, int K, int H, int W, int prec,
                   void* stream);
int ph_fpn_lateral_cl(const uint16_t* X, int x_prec, const uint16_t* Wp, int64_t w_plane_elems, const float* bias,
                      const uint16_t* coarse /* nullable */, int Hc, int Wc, uint16_t* out, int B, int K, int H, int W, int prec,
                      void* stream);
int ph_fpn_output(const float* y, const float* bias, float* out, int B, int64_t HW, void* stream);
/* ph_fpn_output_planes : the same tail, handing the level to the neck directly: y (as above, read once) + bias -> the 16-bit planes
 *                  the neck's first convolution of that level reads, and -- out_f32 given -- the fp32 NCHW level as well (ph_fpn_output's
 *                  bits: y + bias, without `add`; the track head's RoIAlign and the module API take it).  planes: channels-last
 *                  [P][B][HW][256] for PH_PREC_BF16 / PH_PREC_F16 / PH_PREC_SPLIT (hi + lo), or with PH_PLANES_C16 OR-ed into `prec`
 *                  (one-plane grades) chunk-major [B][16][HW][16]: ph_nhwc_ingest's two layouts.  add (nullable): fp32 [256][HW], the
 *                  positional encoding of the neck's pos_level as ph_nhwc_ingest takes it.  Order: v = y + bias rounded to fp32,
 *                  v + add rounded to fp32, one rounding to 16 bits (lo = bf16 of v - hi), no contraction: the planes are bit for bit
 *                  what ph_nhwc_ingest writes from ph_fpn_output's level and the same `add`.  Any HW; a frame's bits do not depend
 *                  on B.  A NULL y / bias / planes, PH_PLANES_C16 with PH_PREC_SPLIT or an unknown grade is PH_EINVAL with a message
 *                  before any launch: the outputs stay untouched. */
int ph_fpn_output_planes(const float* y, const float* bias, const float* add /* nullable */, uint16_t* planes,
                         float* out_f32 /* nullable */, int B, int64_t HW, int prec /* may carry PH_PLANES_C16 */, void* stream);

/* ---- ResNet backbone at inference: the step before the FPN (mmdet/models/backbones/resnet.py as configs/_base_/models/
 * polyphonic_former.py:12-21 builds it; csrc/ph_resnet.hip).  norm_eval=True makes every BatchNorm an affine map, folded by the
 * caller in float64: w' = w g / sqrt(var + eps) rounded once to the grade, b' = beta - mu g / sqrt(var + eps) in fp32.  Activations
 * are ONE 16-bit channels-last plane [B][H * W][C]; prec is PH_PREC_BF16 or PH_PREC_F16 (the FPN's one-plane grades); accumulation
 * is fp32 and each layer output is rounded once.  All three calls launch only: no allocation, no synchronisation, no environment
 * variable; a frame's bits do not depend on B; a bad argument is PH_EINVAL with a message before any launch, the output untouched.
 * The *_workgroups functions return the workgroups of the launch the same arguments take (negative: the error code).
 * ph_conv_cl     : Y[b][p][n] = act(sum_{tap, c} X[b][s p + tap][c] W'[n][tap][c] + b'[n] + R[b][p][n]).  ksize 1 or 3 (pad ksize / 2),
 *                  stride 1 or 2 (a 1x1 stride-2 conv reads the sampled pixels only), Cin and Cout multiples of 64 in [64, 2048];
 *                  output size floor((H + 2 pad - ksize) / stride) + 1 per axis, any H, W.  X: [B][H * W][Cin]; Wp: pack.pack_b32
 *                  fragments of W'[Cout][ksize^2 * Cin] with k = tap * Cin + c, tap = 3 kh + kw; bias: b', fp32 [Cout]; R (nullable):
 *                  the residual, Y's layout and format, added in fp32 before the one rounding; relu != 0: ReLU, else identity.
 * ph_resnet_stem : conv 7x7 stride 2 pad 3 (3 -> 64) + b' + ReLU + MaxPool2d(3, 2, 1) in one kernel (the half-resolution map stays
 *                  in LDS).  x: NCHW [B][3][H][W] of x_dtype PH_OUT_F32 or PH_OUT_BF16 (what ph_image_prepare writes), rounded to the
 *                  grade as it is staged; Wp: pack.pack_b32 fragments of W'[64][176] with k = 24 kh + 3 kw + c (kw < 7; zero
 *                  elsewhere); Y: [B][Hq * Wq][64], Hc = (H - 1) / 2 + 1, Hq = (Hc - 1) / 2 + 1 and likewise for W.  The maximum
 *                  is over the window's entries inside the conv map only.
 * ph_cl_to_nchw  : a plane X [B][HW][C] of grade prec (C a multiple of 64 in [64, 4096]) -> NCHW [B][C][HW] of out_dtype PH_OUT_F32 /
 *                  PH_OUT_BF16 / PH_OUT_F16, each value through fp32 (exact unless out_dtype is the other 16-bit format). */
int ph_conv_cl_workgroups(int ksize, int stride, int Cin, int Cout, int H, int W, int B);
int ph_conv_cl(const uint16_t* X, const uint16_t* Wp, const float* bias, const uint16_t* R /* nullable */, uint16_t* Y, int ksize,
               int stride, int relu, int B, int H, int W, int Cin, int Cout, int prec, void* stream);
int ph_resnet_stem_workgroups(int H, int W, int B);
int ph_resnet_stem(const void* x, int x_dtype, const uint16_t* Wp, const float* bias, uint16_t* Y, int B, int H, int W, int prec,
                   void* stream);
int ph_cl_to_nchw_workgroups(int B, int64_t HW, int C);
int ph_cl_to_nchw(const uint16_t* X, void* out, int out_dtype, int B, int64_t HW, int C, int prec, void* stream);

/* ---- ResNet backbone in training: data and weight gradients of ph_conv_cl's layers (csrc/ph_resnet_train.hip).  The forward of one
 * convolution + BatchNorm (norm_eval=True) is z = W' * x + b' with s = gamma / sqrt(var + eps), W' = w s rounded to bf16, b' = beta - mu s.
 * With dZ the gradient at z (behind the ReLU mask): dW'[n][tap][c] = sum_{b, p} dZ[b][p][n] X[b][stride p + tap - pad][c], db[n] =
 * sum_{b, p} dZ[b][p][n]; dw = dW' s, dbeta = db, dgamma = (sum_k dW'[n][k] w[n][k] - mu[n] db[n]) / sqrt(var[n] + eps) (the rounding of W'
 * passed straight through).  Planes are bf16 channels-last [B][H * W][C], accumulation is fp32.  All calls launch only: no allocation,
 * no synchronisation, no atomics, sums in a fixed order (the same bits from run to run); a bad argument is PH_EINVAL with a message
 * before any launch, the outputs untouched.  ksize, stride, Cin, Cout, H, W, B are the FORWARD layer's (ph_conv_cl's limits); H, W its
 * input size, Ho, Wo = floor((H + 2 pad - ksize) / stride) + 1.
 * ph_conv_cl_bwd_data   : dX[b][q][c] = mask(sum_{tap, n} dZ[b][(q + pad - tap) / stride][n] W'[n][tap][c] + R), over the taps whose
 *                         quotient is whole on both axes and inside Ho x Wo.  dZ: [B][Ho * Wo][Cout]; Wt: the transposed pack of the
 *                         same rounded W' (ph_conv_cl_pack_bwd); R (nullable): a bf16 plane added in fp32 before the one rounding --
 *                         r_stride 1: dX's size; r_stride 2: [B][Hr * Wr][Cin] with Hr = (H - 1) / 2 + 1, read at (qy / 2, qx / 2) where
 *                         qy and qx are even and zero elsewhere (a stride-2 1x1 layer's gradient spread to the pixels it sampled);
 *                         M (nullable): dX's size, the output is zero where M <= 0 (-0 included).  A stride-2 layer runs the MFMAs
 *                         of every tap and zeroes the operands the parity rule excludes.
 * ph_conv_cl_bwd_weight : dW fp32 [Cout][ksize^2 * Cin] in ph_conv_cl's K order (k = tap * Cin + c) and db fp32 [Cout], from dZ
 *                         [B][Ho * Wo][Cout] and X [B][H * W][Cin].  The (frame, pixel) axis is cut into 64-pixel chunks per frame and
 *                         those into nsplit ranges (0: ph_conv_cl_bwd_weight_nsplit, the library's rule); with more than one range the
 *                         partial sums go to `partial` (ph_conv_cl_bwd_weight_partial_floats floats, 16-byte aligned; nullable for
 *                         one range) and are added in range order.  nsplit above the number of chunks B ceil(Ho Wo / 64): PH_EINVAL.
 * ph_resnet_fold_bwd    : (dW', db) and the fp32 w [Cout][Cin][kh][kw], gamma, mean, var -> dw in w's order, dgamma, dbeta (both
 *                         nullable: a norm whose parameters do not require grad); s and the dgamma sum in float64, outputs fp32.
 * ph_conv_cl_pack_bwd   : Wt = pack.pack_b32 fragments of WT[Cin][ksize^2 * Cout], WT[c][t * Cout + n] = W'[n][ksize^2 - 1 - t][c]: a
 *                         permutation of the 16-bit values of ph_conv_cl's Wp.
 * ph_resnet_pack_bwd    : ph_conv_cl_pack_bwd over a ph_resnet_pack buffer, for the convolutions whose input gradient a backward from
 *                         layer4 down to layer2.0 needs: layer2 .. layer4 without layer2.0's conv1 and downsample.  The layout is a
 *                         ph_resnet_layout whose piece PH_RPACK_W(c) is convolution c's Wt (its bytes the forward piece's) and whose
 *                         other pieces are empty; cfg.mode must be PH_MODE_BF16.
 * ph_nchw_grad_to_cl    : out[b][p][c] = bf16((add ? add[b][p][c] : 0) + g[b][c][p]), zero where mask[b][p][c] <= 0; g: a stage's fp32
 *                         NCHW gradient, add / mask (nullable): bf16 planes; C a multiple of 64 in [64, 4096], any HW. */
int ph_conv_cl_bwd_data_workgroups(int ksize, int stride, int Cin, int Cout, int H, int W, int B);
int ph_conv_cl_bwd_data(const uint16_t* dZ, const uint16_t* Wt, const uint16_t* R /* nullable */, int r_stride,
                        const uint16_t* M /* nullable */, uint16_t* dX, int ksize, int stride, int B, int H, int W, int Cin, int Cout,
                        void* stream);
int ph_conv_cl_bwd_weight_nsplit(int ksize, int stride, int Cin, int Cout, int H, int W, int B);
int64_t ph_conv_cl_bwd_weight_partial_floats(int ksize, int stride, int Cin, int Cout, int H, int W, int B, int nsplit);
int ph_conv_cl_bwd_weight(const uint16_t* dZ, const uint16_t* X, float* dW, float* db, float* partial /* nullable */, int nsplit, int ksize,
                          int stride, int B, int H, int W, int Cin, int Cout, void* stream);
int ph_resnet_fold_bwd(const float* dWp, const float* db, const float* w, const float* gamma, const float* mean, const float* var,
                       double eps, float* dw, float* dgamma /* nullable */, float* dbeta /* nullable */, int ksize, int Cin, int Cout,
                       void* stream);
int ph_conv_cl_pack_bwd(const uint16_t* Wp, uint16_t* Wt, int ksize, int Cin, int Cout, void* stream);
int ph_nchw_grad_to_cl(const float* g, const uint16_t* add /* nullable */, const uint16_t* mask /* nullable */, uint16_t* out, int B,
                       int64_t HW, int C, void* stream);

/* ---- N1: the quasi-dense embedding tracker as a native object (csrc/ph_tracker.hip; polyphonic/video/qdtrack/trackers/
 * quasi_dense_embed_tracker.py:47-207).  Host bookkeeping in C++ (boxes, labels, ids, ages), embeddings in a device POOL of
 * `capacity` rows of 256 floats inside `device_mem` (ph_tracker_device_bytes; owned by the caller, alive as long as the tracker).
 * match: boxes [n][5] (x1, y1, x2, y2, score) and labels [n] on the HOST, embeds [n][256] on the DEVICE; writes the kept detections
 * in descending-score order -- kept_out [k] (indices into the input), ids_out [k] (>= 0 track id, -1 unmatched, -2 suppressed) -- and
 * updates the memory.  Returns k >= 0 or a negative error.  One stream synchronisation inside (the [n x m] score download).
 * thresholds are compared in fp32 like the reference's tensors; memo_momentum / one_minus_momentum: fp32(m) and fp32(1 - m) with
 * 1 - m evaluated in double (what `(1 - momentum) * tensor` does). */
typedef struct {
    float init_score_thr, obj_score_thr, match_score_thr, memo_momentum, one_minus_momentum, nms_conf_thr, nms_backdrop_iou_thr,
        nms_class_iou_thr;
    int32_t memo_tracklet_frames, memo_backdrop_frames, with_cats, metric;   /* metric: 0 bisoftmax, 1 softmax, 2 cosine */
} ph_tracker_cfg;
typedef struct ph_tracker ph_tracker;
size_t ph_tracker_device_bytes(int capacity, int max_dets);
ph_tracker* ph_tracker_create(const ph_tracker_cfg* cfg, void* device_mem, size_t device_bytes, int capacity, int max_dets);
void ph_tracker_destroy(ph_tracker* t);
void ph_tracker_reset(ph_tracker* t);
int64_t ph_tracker_num_tracklets(const ph_tracker* t);
int ph_tracker_rows(const ph_tracker* t);
void ph_tracker_debug_times(const ph_tracker* t, double* out6);   /* accumulated host seconds per phase of `match` (csrc/ph_tracker.hip) */
int ph_tracker_match(ph_tracker* t, const float* boxes, const int64_t* labels, const float* embeds_dev, int n, int64_t frame_id,
                     int32_t* kept_out, int64_t* ids_out, void* stream);
/* a whole step's frames in one call (`video.replay_tracking` after the all-gather): frame f's rows of boxes / labels / kept_out /
   ids_out start at sum(counts[0..f-1]); embeds_dev[f]: that frame's [counts[f]][256] device rows; frames without detections are
   skipped and do not advance the frame counter (polyphonic_former_video.py:391-402).  Returns the number of frames matched. */
int ph_tracker_match_frames(ph_tracker* t, const float* boxes, const int64_t* labels, const float* const* embeds_dev, const int32_t* counts,
                            int nframes, int64_t first_frame_id, int32_t* kept_out, int64_t* ids_out, int32_t* kept_counts, void* stream);

/* ---- N2: the S-stage decode as a native object (csrc/ph_decode.hip): what engine.DecodePlan does from Python --
 * kernel_update.py:356-401 (simple_test_mask_preds) for a C / C++ caller.  The plan owns no memory: the caller packs every
 * stage's weights into device memory it owns (ph_decode_pack_bytes / ph_decode_pack_stage, once per weight load), hands a
 * workspace of ph_decode_workspace_bytes and supplies inputs and outputs per call.  ph_decode_run launches exactly the kernel
 * sequence engine.DecodePlan.stages launches for the same geometry on the one given stream, with no host synchronisation,
 * allocation or read of device data: it can be captured into a hipGraph (the captured pointers must then stay valid).
 * No ph_decode_* function reads the environment: the knobs engine.DecodePlan reads from it are fields of ph_decode_cfg, and
 * the plan's launches go through internal forms of ph_dynconv / ph_dynconv_up2_wgs / ph_query_stage_counts that take their
 * launch knobs as arguments (the public entry points keep reading PH_CONV_* / PH_UP2_* / PH_QUERY_*), so setting
 * those variables changes nothing in a plan.  Errors: every argument and geometry error (sizes, modes, limits of the query,
 * pooling and fused kernels, a fused form forced where it cannot run, a short workspace, bad pointers or formats) is returned
 * by ph_decode_create / ph_decode_run before the first launch; only a launch the runtime itself refuses (PH_ELAUNCH) can
 * come back after earlier kernels of the sequence were queued.
 * A zero-initialised ph_decode_cfg plus the sizes and the mode is the module API's configuration: every knob on "auto"
 * (= the rule of resolve() in csrc/ph_decode.hip, which engine.DecodePlan follows too, with no environment variable set). */
enum { PH_MODE_FP32 = 0, PH_MODE_MIXED = 1, PH_MODE_MIXED16 = 2, PH_MODE_FP16 = 3, PH_MODE_BF16 = 4 };   /* engine.MODES */
/* poolx / fused_up: AUTO = the library's rule (ask ph_decode_geometry_of what it picks); ON = the fused form, an error
 * (PH_EUNSUPPORTED) where it cannot run this geometry; OFF = never; WHERE_SUPPORTED = wherever it can run (what PH_CONV_POOLX=1 / PH_CONV_UP2=1 do for the Python plan) */
enum { PH_KNOB_AUTO = 0, PH_KNOB_ON = 1, PH_KNOB_OFF = 2, PH_KNOB_WHERE_SUPPORTED = 3 };
typedef struct {
    int32_t B, N, H, W;         /* frames, queries (things + stuff), feature map (stride 8) */
    int32_t S;                  /* update stages, 1 .. 16 */
    int32_t L;                  /* classes (fc_cls rows), 1 .. 1024 */
    int32_t F;                  /* feedforward_channels, multiple of 256 */
    int32_t mode;               /* PH_MODE_* */
    int32_t out_dtype;          /* PH_OUT_* of mask / mask_up / depth / depth_up (obj, dobj, cls are fp32) */
    int32_t frame_invariant;    /* 1: a frame's outputs do not depend on B (the module API's default; engine.DecodePlan) */
    int32_t query_full_split;   /* mixed16 / fp16: 1 = query side hi + lo bf16 (PH_PREC_SPLIT) instead of PH_PREC_QHYBRID */
    int32_t shares_gpu;         /* 1: one part of a multi-stream step (PH_QUERY_WIDE, the final stage's shared workgroup count) */
    int32_t poolx;              /* PH_KNOB_*: ph_dynconv_poolx between the stages              (env PH_CONV_POOLX of the Python plan) */
    int32_t fused_up;           /* PH_KNOB_*: ph_dynconv_up2 for the final stage                (PH_CONV_UP2) */
    int32_t nsplit;             /* 0 = auto, else pixel ranges of ph_pool_counts                (PH_POOL_NSPLIT) */
    int32_t nsplit_px;          /* 0 = auto, else pixel ranges of ph_dynconv_poolx; frame_invariant plans use nsplit (PH_POOLX_NSPLIT) */
    int32_t up2_wgs;            /* 0 = auto (1.5 per CU), else the final stage's workgroups of shares_gpu plans (PH_UP2_SHARED_WGS) */
} ph_decode_cfg;

/* the geometry a plan chose (ph_decode_info), or would choose (ph_decode_geometry_of) */
typedef struct {
    int32_t nsplit, nsplit_px, poolx, fused_up;
    int32_t up2_workgroups;     /* workgroups of the fused final stage's launches: 0 = one per CU; follows cfg.up2_wgs, which
                                   only ph_decode_create fills from the device: ph_decode_geometry_of reports 0 when it is 0 */
    int32_t feat_prec, query_prec, conv_prec, kern_format;   /* PH_PREC_* / PH_KERN_* of ingest + pool, query, dynamic conv */
    int32_t feat_planes;        /* P of the feature planes [P][B][256][HWp] */
} ph_decode_geometry;

/* ph_decode_run's inputs and outputs.  feat_format:
 *   PH_FEAT_F32     x / depth_feats fp32 NCHW [B][256][H][W]       (ingested to planes inside the call)
 *   PH_FEAT_16      16-bit NCHW of the mode's plane format: bf16 for bf16 / mixed / mixed16, fp16 for fp16 (copied into the planes)
 *   PH_FEAT_PLANES  feature planes [P][B][256][HWp] another kernel produced (ph_khead_*), read only, and `bits` [B][Npad][HWp/32]
 *                   instead of m0 (copied: the stages rewrite them) */
enum { PH_FEAT_F32 = 0, PH_FEAT_16 = 1, PH_FEAT_PLANES = 2 };
typedef struct {
    int32_t feat_format;        /* PH_FEAT_* */
    int32_t m0_dtype;           /* PH_OUT_* of m0 */
    const void* x;
    const void* depth_feats;
    const float* k0;            /* proposal_feats [B][N][256] */
    const float* q0;            /* depth_proposal [B][N][256] */
    const void* m0;             /* mask logits [B][N][H][W] (unused with PH_FEAT_PLANES) */
    const uint32_t* bits;       /* PH_FEAT_PLANES only */
    float* obj;                 /* [B][N][256]  last stage's object_feats */
    float* dobj;                /* [B][N][256]  last stage's depth_proposal */
    float* cls;                 /* [B][N][L]    sigmoid class scores */
    void* mask;                 /* [B][N][H][W]     out_dtype */
    void* mask_up;              /* [B][N][2H][2W]   out_dtype */
    void* depth_up;             /* [B][N][2H][2W]   out_dtype */
    void* depth;                /* nullable: [B][N][H][W] low-resolution depth logits */
} ph_decode_io;

/* ---- stage packing: the one stage's parameters below, fp32 device tensors in this order (the reference's state_dict names,
 * SURVEY.md 8b; KernelUpdateHead with num_cls_fcs = num_mask_fcs = 1, num_ffn_fcs = 2), packed into the layout pack.py
 * describes: the Linear weights as MFMA B-fragments in one or two 16-bit planes, feat_transform / feat_depth_transform folded
 * into dynamic_layer and fc_mask / fc_depth in float64 (k ascending: deterministic), then rounded to fp32 and split.
 *    0 attention.attn.in_proj_weight [768][256]    1 attention.attn.in_proj_bias [768]
 *    2 attention.attn.out_proj.weight [256][256]   3 attention.attn.out_proj.bias
 *    4 .. 7   attention_depth.attn.* in the same order
 *    8 attention_norm.weight         9 attention_norm.bias      10 attention_norm_depth.weight   11 attention_norm_depth.bias
 *   12 kernel_update_conv.dynamic_layer.weight [512][256]      13 .dynamic_layer.bias [512]
 *   14 kernel_update_conv.input_layer.weight [512][256]        15 .input_layer.bias [512]
 *   16 .input_gate.weight [256][256]   17 .input_gate.bias     18 .update_gate.weight          19 .update_gate.bias
 *   20 .norm_in.weight        21 .norm_in.bias                 22 .norm_out.weight             23 .norm_out.bias
 *   24 .input_norm_in.weight  25 .input_norm_in.bias           26 .input_norm_out.weight       27 .input_norm_out.bias
 *   28 .fc_layer.weight       29 .fc_layer.bias                30 .fc_norm.weight              31 .fc_norm.bias
 *   32 .. 51 kernel_update_conv_depth.* in the same order
 *   52 feat_transform.conv.weight [256][256][1][1]        53 feat_transform.conv.bias
 *   54 feat_depth_transform.conv.weight                   55 feat_depth_transform.conv.bias
 *   56 ffn.layers.0.0.weight [F][256]   57 .bias [F]      58 ffn.layers.1.weight [256][F]   59 .bias
 *   60 ffn_norm.weight                  61 ffn_norm.bias
 *   62 .. 67 ffn_depth.layers.0.0.{weight, bias}, ffn_depth.layers.1.{weight, bias}, ffn_norm_depth.{weight, bias}
 *   68 cls_fcs.0.weight    69 cls_fcs.1.weight    70 cls_fcs.1.bias    71 fc_cls.weight [L][256]    72 fc_cls.bias [L]
 *   73 mask_fcs.0.weight   74 mask_fcs.1.weight   75 mask_fcs.1.bias
 *   76 depth_regs.0.weight 77 depth_regs.1.weight 78 depth_regs.1.bias
 *   79 fc_mask.weight      80 fc_mask.bias        81 fc_depth.weight   82 fc_depth.bias
 * (ph_decode_param_name / ph_decode_param_numel state the same table.)  Vectors are [256] unless noted.
 * One pack = uint16 planes [P][wb_plane_elems] followed, at the next 256-byte boundary, by the fp32 vectors.  Packs made
 * by pack.py (engine.StagePack: wb, wf) in the same layout serve a plan as well. */
#define PH_DECODE_NPARAMS 83
const char* ph_decode_param_name(int index);                        /* NULL out of range */
int64_t ph_decode_param_numel(const ph_decode_cfg* cfg, int index); /* elements; < 0 out of range */
size_t ph_decode_pack_bytes(const ph_decode_cfg* cfg);              /* 0 on a bad cfg (see ph_last_error_string) */
/* the layout of a pack (pack.py's StageLayout; offsets in elements; wb at byte 0, wf at wf_byte_offset) */
int ph_decode_pack_layout(const ph_decode_cfg* cfg, ph_stage_layout* layout, size_t* wf_byte_offset);
/* one launch; `params`: host array of PH_DECODE_NPARAMS device pointers */
int ph_decode_pack_stage(const ph_decode_cfg* cfg, const float* const* params, void* pack, void* stream);

/* ---- plan lifetime.  workspace: feature planes, mask bits, pooled partial sums and pixel counts, the query workspace,
 * every stage's outputs but the last stage's obj / dobj / cls, the low-resolution depth logits of the two-kernel final
 * stage; 256-byte aligned pieces.  The caller keeps the packs and the workspace alive as long as the plan. */
typedef struct ph_decode ph_decode;
size_t ph_decode_workspace_bytes(const ph_decode_cfg* cfg);         /* 0 on a bad cfg */
int ph_decode_create(const ph_decode_cfg* cfg, const void* const* packs /* S device pointers */, void* workspace,
                     size_t workspace_bytes, ph_decode** out);
int ph_decode_info(const ph_decode* plan, ph_decode_geometry* out);
/* the same answer without a plan: the launch geometry rule applied to a cfg (it is the only copy of that rule: engine.DecodePlan
 * takes nsplit, nsplit_px, poolx and fused_up from here).  Needs no device, no packs and no workspace; every cfg error of
 * ph_decode_create comes back from here too.  up2_workgroups: see ph_decode_geometry */
int ph_decode_geometry_of(const ph_decode_cfg* cfg, ph_decode_geometry* out);
void ph_decode_destroy(ph_decode* plan);
int ph_decode_run(ph_decode* plan, const ph_decode_io* io, void* stream);

/* ---- A1 as a native object (csrc/ph_kheadplan.hip): what engine.KernelHeadPack + engine.KernelHeadPlan do from Python --
 * kernel_head.py:245-347 (_decode_init_proposals after localization_fpn) for a C / C++ caller: from the neck's three maps to
 * the feature planes, the mask bits, the mask / seg / depth logits and proposal_feats, i.e. to every input of ph_decode_run
 * (PH_FEAT_PLANES: x = xp, depth_feats = dp, bits = bits, k0 = proposal, q0 = depth_proposal).  Conventions are ph_decode_*'s:
 * status codes + ph_last_error_string, caller-owned memory, no allocation of device memory, no synchronisation and no host read
 * of device data in pack / create / run, every argument or geometry error returned before the first launch.  No ph_khead_plan_*
 * / ph_khead_pack* function reads the environment: the plan's launches are the public ph_khead_onepass / ph_khead_fused_if,
 * which read none either, and what engine.KernelHeadPlan reads from PH_KHEAD_TWOPASS / PH_POOL_NSPLIT are the cfg's
 * `onepass` / `nsplit` fields.  The only process-wide setting a plan honours is ph_khead_onepass_set_timeout_us.
 * A zero-initialised ph_khead_cfg plus the sizes and the mode is the module API's configuration.
 *   mode         PH_MODE_*, mapped to a1's grade as engine.KHEAD_PREC maps the precision names: PH_MODE_FP16 -> PH_PREC_F16 (one
 *                fp16 plane; pairs with a PH_MODE_FP16 decode plan), PH_MODE_BF16 -> PH_PREC_BF16 (one bf16 plane; pairs with
 *                PH_MODE_BF16 / _MIXED / _MIXED16 decode plans), every other mode -> PH_PREC_SPLIT (hi + lo bf16 planes; pairs
 *                with PH_MODE_FP32)
 *   logit_dtype  PH_OUT_F32 or PH_OUT_F16 (one-pass form only) of mask_preds / seg_preds / depth_pred
 *   emit_f32     1: the fp32 NCHW x_feats / depth_feats of the reference API are written too (ph_khead_io x_f32 / dfe_f32)
 *   onepass      PH_KNOB_AUTO: ph_khead_onepass wherever ph_khead_onepass_supported(B, H*W, groups, grade, PH_IN_F32_NCHW) says so
 *                (engine.KernelHeadPlan's rule with no environment variable set); PH_KNOB_ON: the same, PH_EUNSUPPORTED where
 *                it says no; PH_KNOB_OFF: always the two-pass ph_khead_fused (PH_KHEAD_TWOPASS of the Python plan)
 *   nsplit       0 = ph_pool_default_nsplit(B, H*W, frame_invariant), else the pixel ranges of the object pooling (PH_POOL_NSPLIT) */
typedef struct {
    int32_t B, H, W;            /* frames, feature map (stride 8) */
    int32_t num_proposals;      /* rows of init_kernels (thing queries), 1 .. 256 */
    int32_t num_classes;        /* rows of conv_seg, 1 .. 256 */
    int32_t num_thing_classes;  /* <= num_classes; the stuff rows of conv_seg are [num_thing_classes, num_classes) */
    int32_t cat_stuff;          /* 1: the stuff rows are appended to mask_preds / proposal (cat_stuff_mask, inference) */
    int32_t groups;             /* GroupNorm groups (divides 256) */
    int32_t mode;               /* PH_MODE_* */
    int32_t logit_dtype;        /* PH_OUT_F32 / PH_OUT_F16 */
    int32_t emit_f32;
    int32_t frame_invariant;    /* 1: the pooling split of a one-frame launch at any B (the module API's default) */
    int32_t onepass;            /* PH_KNOB_AUTO / _ON / _OFF */
    int32_t nsplit;
} ph_khead_cfg;

/* ---- the parameter table: the 14 fp32 tensors of KernelHead's own state_dict (reference names) that the pack is made of
 *    0 loc_convs.0.conv.weight [256][256][1][1]   1 loc_convs.0.gn.weight [256]   2 loc_convs.0.gn.bias [256]
 *    3 .. 5 seg_convs.0.*  and  6 .. 8 depth_convs.0.*  in the same order
 *    9 init_kernels.weight [num_proposals][256][1][1]
 *   10 conv_seg.weight [num_classes][256][1][1]   11 conv_seg.bias [num_classes]
 *   12 conv_direct_depth.weight [1][256][1][1]    13 conv_direct_depth.bias [1] */
#define PH_KHEAD_NPARAMS 14
const char* ph_khead_param_name(int index);                        /* NULL out of range */
int64_t ph_khead_param_numel(const ph_khead_cfg* cfg, int index);  /* elements; < 0 out of range */

/* ---- packing (k_pack_pieces: one launch, once per weight load).  The pieces are engine.KernelHeadPack's tensors, byte for byte
 * (nothing is folded: fp32 -> bf16 / fp16 round to nearest even, lo = bf16(w - float(hi)) in fp32), each at a 256-byte aligned
 * offset of one device buffer; the alignment padding is written as zeros.  P = planes of the grade (2 for PH_PREC_SPLIT),
 * rows32(n) = n rounded up to 32 (pad rows zero):
 *   WPLANES      uint16 [P][3][256][256]            {loc,seg,depth}_convs.0.conv.weight
 *   GN           float  [3][2][256]                 (gamma, beta) of the three GroupNorms
 *   INIT_PLANES  uint16 [P][rows32(num_proposals)][256]     SEG_PLANES [P][rows32(num_classes)][256]     DD_PLANES [P][32][256]
 *   SEG_BIAS     float  [rows32(num_classes)]               DD_BIAS float [32]
 *   INIT_FRAG / SEG_FRAG / DD_FRAG   the three planes as MFMA 32x32x16 A fragments (ph_khead_fused's w2_*)
 *   CONV_FRAG    uint16 [3][8][16][64][8], one-plane grades only (0 bytes for PH_PREC_SPLIT): ph_khead_onepass's conv_frags
 *   W_INIT_F32 [num_proposals][256], W_SEG_F32 [num_classes][256], W_DD_F32 [256]   fp32 copies (ph_khead_proposals) */
enum { PH_KPACK_WPLANES = 0, PH_KPACK_GN, PH_KPACK_INIT_PLANES, PH_KPACK_SEG_PLANES, PH_KPACK_DD_PLANES, PH_KPACK_SEG_BIAS,
       PH_KPACK_DD_BIAS, PH_KPACK_INIT_FRAG, PH_KPACK_SEG_FRAG, PH_KPACK_DD_FRAG, PH_KPACK_CONV_FRAG, PH_KPACK_W_INIT_F32,
       PH_KPACK_W_SEG_F32, PH_KPACK_W_DD_F32, PH_KPACK_COUNT };
typedef struct {
    uint64_t offset[PH_KPACK_COUNT];   /* bytes from the start of the pack, multiples of 256 */
    uint64_t bytes[PH_KPACK_COUNT];    /* size of the piece; the next piece starts at offset + bytes rounded up to 256 */
} ph_khead_layout;
size_t ph_khead_pack_bytes(const ph_khead_cfg* cfg);               /* 0 on a bad cfg (see ph_last_error_string) */
int ph_khead_pack_layout(const ph_khead_cfg* cfg, ph_khead_layout* layout);
/* `params`: host array of PH_KHEAD_NPARAMS device pointers; `pack`: 256-byte aligned device buffer of ph_khead_pack_bytes */
int ph_khead_pack(const ph_khead_cfg* cfg, const float* const* params, void* pack, void* stream);

/* ---- plan lifetime.  The workspace holds the one-pass launch's hand-off state (one-pass plans), the two-pass kernels'
 * workspace (the path itself, or the in-call fallback of a one-pass launch that gave up) and the pooled partial sums.
 * ZEROING CONTRACT: the caller zeroes the whole workspace ONCE (hipMemset) before ph_khead_plan_create and never again --
 * ph_khead_onepass clears its hand-off state on every call except the sticky time-out words, which count from that one
 * zeroing on.  ph_khead_plan_create itself touches no device memory.  The caller keeps pack and workspace alive as long as
 * the plan; both 256-byte aligned. */
typedef struct ph_khead_plan ph_khead_plan;
typedef struct {
    int32_t onepass;            /* 1: ph_khead_onepass + the predicated fallback; 0: ph_khead_fused + ph_binarize */
    int32_t nsplit;             /* pixel ranges of the object pooling */
    int32_t N;                  /* num_proposals + stuff rows: rows of mask_preds / proposal */
    int32_t Npad;               /* N rounded up to 32: rows of bits */
    int32_t HWp;                /* H * W rounded up to 128 */
    int32_t P;                  /* planes of xp / dp */
    int32_t prec;               /* the grade, PH_PREC_* */
    int32_t n_stuff;
} ph_khead_geometry;
size_t ph_khead_plan_workspace_bytes(const ph_khead_cfg* cfg);     /* 0 on a bad cfg */
int ph_khead_plan_create(const ph_khead_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes, ph_khead_plan** out);
int ph_khead_plan_info(const ph_khead_plan* plan, ph_khead_geometry* out);
/* the same answer without a plan: the geometry rule applied to a cfg (the only copy of that rule: engine.KernelHeadPlan takes
 * onepass and nsplit from here).  Needs no pack and no workspace, but -- like ph_khead_plan_create -- the CURRENT DEVICE: the
 * one-pass rule asks it for its CU count.  Every cfg error of ph_khead_plan_create comes back from here too. */
int ph_khead_geometry_of(const ph_khead_cfg* cfg, ph_khead_geometry* out);
void ph_khead_plan_destroy(ph_khead_plan* plan);

/* ---- one a1 call.  Inputs f0 / f1 / f2: the neck's three maps, fp32 NCHW [B][256][H][W] (PH_IN_F32_NCHW) or 16-bit planes
 * [P][B][256][HWp] of the grade's format, zero in [H*W, HWp) (PH_IN_PLANES).  Outputs are the caller's, per call:
 *   xp, dp          uint16 [P][B][256][HWp]      x and depth_feats planes      -> ph_decode_io.x / .depth_feats (PH_FEAT_PLANES)
 *   bits            uint32 [B][Npad][HWp/32]     hard masks of mask_preds      -> ph_decode_io.bits
 *   x_f32, dfe_f32  float [B][256][H][W]         non-NULL exactly when cfg.emit_f32
 *   mask_preds [B][N][H][W], seg_preds [B][num_classes][H][W], depth_pred [B][1][H][W]   logit_dtype
 *                   (ph_upsample2x of depth_pred is ph_panoptic_merge's depth_init_up)
 *   proposal        float [B][N][256]            proposal_feats                -> ph_decode_io.k0
 *   depth_proposal  float [B][N][256], nullable  conv_direct_depth.weight in every row (the reference hands it on as a
 *                   stride-0 view, kernel_head.py:286-289; ph_decode_io.q0 wants it dense)   -> ph_decode_io.q0
 * The launch sequence is engine.KernelHeadPlan.run's: one-pass plans ph_khead_onepass, ph_khead_fused_if and ph_binarize_if
 * predicated on its status word, two-pass plans ph_khead_fused and ph_binarize; then ph_pool_rows and ph_khead_proposals (and
 * the depth_proposal broadcast).  Capturable into a hipGraph.
 * ph_khead_plan_status: 1 if the last run of a one-pass plan gave up and was redone by the two-pass kernels inside the same
 * call; ph_khead_plan_timeouts: workgroup time-outs since the workspace was zeroed; both 0 for two-pass plans, negative on a
 * runtime error, and both SYNCHRONISE the stream (they read device words). */
typedef struct {
    int32_t input_format;       /* PH_IN_F32_NCHW / PH_IN_PLANES */
    int32_t reserved;           /* 0 */
    const void* f0;
    const void* f1;
    const void* f2;
    uint16_t* xp;
    uint16_t* dp;
    uint32_t* bits;
    float* x_f32;
    float* dfe_f32;
    void* mask_preds;
    void* seg_preds;
    void* depth_pred;
    float* proposal;
    float* depth_proposal;
} ph_khead_io;
int ph_khead_plan_run(ph_khead_plan* plan, const ph_khead_io* io, void* stream);
int ph_khead_plan_status(const ph_khead_plan* plan, void* stream);
int ph_khead_plan_timeouts(const ph_khead_plan* plan, void* stream);

/* ---- N3 as a native object (csrc/ph_neckplan.hip): what SemanticFPNWrapper._pack + sine_positional_encoding + engine.NeckPlan
 * do from Python -- semantic_fpn.py:198-235 for a C / C++ caller: from the four FPN levels to the neck's maps, as fp32 NCHW and / or
 * as the 16-bit planes that ph_khead_io takes (PH_IN_PLANES: f0 / f1 / f2 = out_planes[0 .. 2]).  Conventions are ph_decode_*'s and
 * ph_khead_*'s: status codes + ph_last_error_string, caller-owned 256-byte aligned memory, no allocation of device memory, no
 * synchronisation and no host read of device data in pack / posenc / create / run, every argument or geometry error returned
 * before the first launch.  No ph_neck_plan_* / ph_neck_pack* / ph_neck_posenc function reads the environment: the plan's
 * launches go through internal forms of ph_conv_nhwc / ph_gn_sum_planes / ph_gn_apply that take their launch knobs as arguments
 * (the public entry points take theirs from the switch table: PH_SWITCH_CONV_TILE_ROWS / PH_SWITCH_GNSUM_WGS /
 * PH_SWITCH_CPLANES_TPW; ph_neck_out_convs has no knobs), and the Python side's PH_NECK_OUT2 / PH_NECK_C16 / PH_NECK_STREAMS arrive as the cfg's `fused_out` / `c16` /
 * `tower_buffers` fields: engine.native_neck_cfg is the one place that reads them (PH_NECK_OUT2=0 -> fused_out PH_KNOB_OFF,
 * PH_NECK_C16=0 -> c16 PH_KNOB_OFF, PH_NECK_STREAMS=0 -> tower_buffers 0), and engine.NeckPlan takes its choices from
 * ph_neck_geometry_of of that cfg, so the Python plan and the native plan agree by construction.
 * A zero-initialised ph_neck_cfg plus the sizes, the mode, num_outs, pos_level and an emit flag is the module API's configuration.
 *   h, w         the four FPN level sizes, level 0 (stride 4) first: each level (n + 1) / 2 of the one before, and levels 2 and 3
 *                exactly 1/2 and 1/4 of level 1 (they reach it by x2 upsampling); otherwise PH_EUNSUPPORTED
 *   groups       GroupNorm groups, divides 256
 *   mode         PH_MODE_*, mapped to the grade as ph_khead_cfg.mode / engine.KHEAD_PREC: PH_MODE_FP16 -> PH_PREC_F16, PH_MODE_BF16 ->
 *                PH_PREC_BF16, every other mode -> PH_PREC_SPLIT (hi + lo bf16 planes)
 *   num_outs     1 .. 3: conv_pred + 0 .. 2 aux convs
 *   pos_level    the level the positional encoding is added to (the module's cat_coors_level), 0 .. 3; -1: none
 *   emit_planes  1: ph_neck_io.out_planes are written;  emit_f32  1: ph_neck_io.out_f32 are written; at least one
 *   fused_out    PH_KNOB_AUTO: conv_pred + the aux convs as ONE ph_neck_out_convs when num_outs == 3, groups == 32 and the grade has
 *                one plane; PH_KNOB_ON: the same, PH_EUNSUPPORTED where
 *                that says no; PH_KNOB_OFF: conv -> finalize -> apply per map (PH_NECK_OUT2=0 of the Python plan)
 *   c16          PH_KNOB_AUTO: chunk-major planes (PH_PLANES_C16) into level 0's stride-2 conv in one-plane grades;
 *                PH_KNOB_OFF: channels-last (PH_NECK_C16=0)
 *   tower_buffers  1: every level owns its ping / pong planes, conv output, statistics and partial sums (engine.NeckPlan's `multi`
 *                layout), so the four ph_neck_plan_run_level calls may run concurrently; 0: one shared set, a smaller workspace
 *   eps          GroupNorm epsilon; 0 = 1e-5 */
typedef struct {
    int32_t B;
    int32_t h[4], w[4];
    int32_t groups;
    int32_t mode;               /* PH_MODE_* */
    int32_t num_outs;
    int32_t pos_level;
    int32_t emit_planes, emit_f32;
    int32_t fused_out;          /* PH_KNOB_AUTO / _ON / _OFF */
    int32_t c16;                /* PH_KNOB_AUTO / _OFF */
    int32_t tower_buffers;
    float eps;
} ph_neck_cfg;

/* ---- the parameter table: (conv.weight [256][256][k][k], gn.weight [256], gn.bias [256]) of the ten convs, fp32 device tensors
 * under the reference's state_dict names, in this order:
 *    0 .. 2   convs_all_levels.0.conv0 (3x3, stride 2)      3 .. 5   convs_all_levels.1.conv0
 *    6 .. 11  convs_all_levels.2.conv0, .conv1              12 .. 20 convs_all_levels.3.conv0, .conv1, .conv2      (3x3)
 *   21 .. 23  conv_pred     24 .. 26  aux_convs.0     27 .. 29  aux_convs.1                                        (1x1)
 * the entries of aux convs beyond num_outs - 1 are ignored and may be NULL */
#define PH_NECK_NPARAMS 30
const char* ph_neck_param_name(int index);                         /* NULL out of range */
int64_t ph_neck_param_numel(const ph_neck_cfg* cfg, int index);    /* elements; < 0 out of range */

/* ---- packing (k_pack_pieces: one launch, once per weight load).  The pieces are SemanticFPNWrapper._pack's tensors, byte for byte
 * (fp32 -> bf16 / fp16 round to nearest even, lo = bf16(w - float(hi)) in fp32), each at a 256-byte aligned offset of one device
 * buffer; the alignment padding is written as zeros.  P = planes of the grade (2 for PH_PREC_SPLIT), conv c = parameter 3 c:
 *   WP(c)        uint16 [P][256 * K]   pack.pack_b32 fragments of W[n][tap * 256 + c'] -- the (kh, kw, in) K order, K = 2304 (3x3)
 *                or 256 (1x1): ph_conv_nhwc's Wp
 *   GAMMA(c), BETA(c)   float [256]
 *   OUTS_W       uint16 [P][3][256][256] (out, in) of conv_pred + the two aux convs, OUTS_GN float [3][2][256] (gamma, beta):
 *                ph_neck_out_convs' operands; only with num_outs == 3 (0 bytes otherwise, as are the pieces of an absent aux conv) */
#define PH_NPACK_WP(c) (3 * (c))
#define PH_NPACK_GAMMA(c) (3 * (c) + 1)
#define PH_NPACK_BETA(c) (3 * (c) + 2)
enum { PH_NPACK_OUTS_W = 30, PH_NPACK_OUTS_GN = 31, PH_NPACK_COUNT = 32 };
typedef struct {
    uint64_t offset[PH_NPACK_COUNT];   /* bytes from the start of the pack, multiples of 256 */
    uint64_t bytes[PH_NPACK_COUNT];    /* size of the piece; the next piece starts at offset + bytes rounded up to 256 */
} ph_neck_layout;
size_t ph_neck_pack_bytes(const ph_neck_cfg* cfg);                 /* 0 on a bad cfg (see ph_last_error_string) */
int ph_neck_pack_layout(const ph_neck_cfg* cfg, ph_neck_layout* layout);
/* `params`: host array of PH_NECK_NPARAMS device pointers; `pack`: 256-byte aligned device buffer of ph_neck_pack_bytes */
int ph_neck_pack(const ph_neck_cfg* cfg, const float* const* params, void* pack, void* stream);

/* ---- the positional encoding (k_neck_posenc: one launch, once per map size): mmdet's SinePositionalEncoding(normalize=True) for an
 * empty ignore mask (semantic_fpn.py:202-208), out float [2 * num_feats][H][W] -- the y block first, then x; sin on even and cos on
 * odd indices of  embed / temperature^(2 (i / 2) / num_feats),  embed = (row or column + 1) / (H or W + eps) * scale.  Evaluated
 * in fp64 and rounded once to fp32 (the reference evaluates in fp32: the two differ in the last bits; a caller that wants the
 * Python path's bits hands ph_neck_io.posenc the host-computed table instead).  The shipped model: num_feats 128,
 * temperature 10000, scale 2 pi, eps 1e-6. */
int ph_neck_posenc(int H, int W, int num_feats, double temperature, double scale, double eps, float* out, void* stream);

/* ---- plan lifetime.  The workspace holds the towers' ping / pong planes, conv outputs, GroupNorm statistics and partial sums, the
 * level sum and the output stage's buffers.  ZEROING CONTRACT: none -- every word a launch reads was written by an earlier launch
 * of the same run.  ph_neck_plan_create touches no device memory.  The caller keeps pack and workspace alive as long as the plan;
 * both 256-byte aligned. */
typedef struct ph_neck_plan ph_neck_plan;
typedef struct {
    int32_t Ho, Wo;             /* the output (stride-8) size = level 1's */
    int32_t HWp;                /* Ho * Wo rounded up to 128 */
    int32_t P;                  /* planes of out_planes */
    int32_t prec;               /* the grade, PH_PREC_* */
    int32_t fused_out;          /* 1: ph_neck_out_convs; 0: conv -> finalize -> apply per map */
    int32_t c16;                /* 1: chunk-major planes into level 0's stride-2 conv */
    int32_t tower_buffers;
    int32_t nconvs;             /* 7 + num_outs */
    int32_t tile_rows[10];      /* per conv (parameter-table order): output rows per tile its ph_conv_nhwc launch takes at this B (2 or
                                   4; for the output convs of a fused_out plan: what the per-map form would take); 0 beyond nconvs */
} ph_neck_geometry;
size_t ph_neck_plan_workspace_bytes(const ph_neck_cfg* cfg);       /* 0 on a bad cfg */
int ph_neck_plan_create(const ph_neck_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes, ph_neck_plan** out);
int ph_neck_plan_info(const ph_neck_plan* plan, ph_neck_geometry* out);
/* the same answer without a plan: the geometry rule applied to a cfg (the only copy of that rule: engine.NeckPlan takes
 * fused_out, c16 and tower_buffers from here).  Needs no device, no pack and no workspace; every cfg error of ph_neck_plan_create
 * comes back from here too. */
int ph_neck_geometry_of(const ph_neck_cfg* cfg, ph_neck_geometry* out);
void ph_neck_plan_destroy(ph_neck_plan* plan);

/* ---- one neck call.
 *   feats[l]       float [B][256][h_l][w_l], fp32 NCHW, the four FPN levels
 *   posenc         float [256][h][w] of level pos_level (ph_neck_posenc, or the caller's own table); NULL exactly when pos_level < 0
 *   out_planes[i]  uint16 [P][B][256][HWp] of the grade's format: ph_khead_io's PH_IN_PLANES input, zero in [Ho*Wo, HWp) whatever
 *                  the buffer held before (cfg.emit_planes)
 *   out_f32[i]     float [B][256][Ho][Wo] (cfg.emit_f32);   entries >= num_outs are ignored; outputs 16-byte aligned
 * ph_neck_plan_run: the whole neck on one stream, in engine.NeckPlan.run's launch sequence -- per level ph_nhwc_ingest, then
 * (ph_conv_nhwc, ph_gn_finalize, ph_gn_apply x2 upsample)* and the last conv + finalize; then ph_gn_sum_planes and ph_neck_out_convs
 * (fused_out) or ph_conv_nhwc, ph_gn_finalize, ph_gn_apply per map.  It is ph_neck_plan_run_level for levels 0 .. 3 and
 * ph_neck_plan_run_outputs in one call.  With tower_buffers == 1 the four level calls may run on four streams concurrently; the
 * caller orders them before ph_neck_plan_run_outputs with events.  With tower_buffers == 0 they share buffers and are valid back to
 * back on one stream only.  All three are capturable into a hipGraph. */
typedef struct {
    const float* feats[4];
    const float* posenc;
    uint16_t* out_planes[3];
    float* out_f32[3];
} ph_neck_io;
int ph_neck_plan_run(ph_neck_plan* plan, const ph_neck_io* io, void* stream);
int ph_neck_plan_run_level(ph_neck_plan* plan, int level, const ph_neck_io* io, void* stream);
int ph_neck_plan_run_outputs(ph_neck_plan* plan, const ph_neck_io* io, void* stream);
/* ---- a level started from planes: the producer of a level (ph_fpn_output_planes, ph_fpn_plan_run_output) writes the level's
 * conv-input planes itself and the tower runs without its ph_nhwc_ingest; ph_neck_io.feats is then not read at all.
 * ph_neck_plan_level_input: the device address of level `level`'s conv-input planes inside the plan's workspace (P planes of
 *   B * h_l * w_l * 256 elements) and the value a writer passes as `prec`: the grade, with PH_PLANES_C16 OR-ed in where the level's
 *   first convolution reads chunk-major planes (level 0 of a c16 plan).  The writer adds the positional encoding of pos_level.
 * ph_neck_plan_run_level_planes: ph_neck_plan_run_level without the ingest, from what the caller wrote there.
 * ORDERING.  tower_buffers == 0: the four levels share ONE input buffer (ph_neck_plan_level_input returns the same address for
 *   each), so a level's planes are written and its ph_neck_plan_run_level_planes is enqueued -- same stream -- before the next
 *   level's planes are written.  tower_buffers == 1: every level owns its buffer; the four may be written in any order and their
 *   towers run concurrently, each ordered behind its own writer.  ph_neck_plan_run_outputs follows the four towers as before. */
int ph_neck_plan_level_input(const ph_neck_plan* plan, int level, uint16_t** planes, int32_t* prec_layout);
int ph_neck_plan_run_level_planes(ph_neck_plan* plan, int level, void* stream);

/* ---- the FPN as a native object (csrc/ph_fpnplan.hip): what fpn.FPN._pack + engine.FpnPlan do from Python -- fpn.py:151-203 for a
 * C / C++ caller: from the four backbone stages to the four pyramid levels, as fp32 NCHW maps and / or as the conv-input planes of a
 * neck plan (ph_neck_plan_level_input).  Conventions are ph_neck_plan_*'s: status codes + ph_last_error_string, caller-owned
 * 256-byte aligned pack and workspace, no allocation of device memory, no synchronisation, no host read of device data and no
 * environment variable in pack / create / run (the 3x3 convolutions go through the internal form of ph_conv_nhwc that takes its
 * launch knobs as arguments), every cfg or pointer error returned before the first launch, every run call capturable into a hipGraph.
 *   B            frames per call, 1 .. 4096
 *   k            channels of the four backbone stages, each a multiple of 64 in [64, 4096] (PH_EINVAL otherwise)
 *   h, w         the four stage = level sizes, level 0 (the finest) first; each level 2 n or 2 n - 1 of the next coarser one in both
 *                directions -- ph_fpn_lateral's rule, at which the integer nearest index is torch's -- otherwise PH_EUNSUPPORTED
 *   mode         PH_MODE_*, mapped to the grade as ph_neck_cfg.mode
 *   x_dtype      element type of the stages: PH_OUT_F32 / PH_OUT_BF16 / PH_OUT_F16
 *   emit_f32     1: ph_fpn_io.out_f32 are written;  emit_planes  1: ph_fpn_io.out_planes are written; at least one */
typedef struct {
    int32_t B;
    int32_t k[4];
    int32_t h[4], w[4];
    int32_t mode;               /* PH_MODE_* */
    int32_t x_dtype;            /* PH_OUT_* */
    int32_t emit_f32, emit_planes;
} ph_fpn_cfg;

/* ---- the parameter table: fp32 device tensors under the reference's 16 state_dict keys, in state_dict order:
 *    2 l, 2 l + 1       lateral_convs.l.conv.weight [256][k_l][1][1], .bias [256]     (l = 0 .. 3)
 *    8 + 2 l, 9 + 2 l   fpn_convs.l.conv.weight [256][256][3][3], .bias [256] */
#define PH_FPN_NPARAMS 16
const char* ph_fpn_param_name(int index);                          /* NULL out of range */
int64_t ph_fpn_param_numel(const ph_fpn_cfg* cfg, int index);      /* elements; < 0 out of range or on a bad k */

/* ---- packing (k_pack_pieces: one launch, once per weight load).  Piece i is parameter i; the pieces are fpn.FPN._pack's tensors,
 * byte for byte, each at a 256-byte aligned offset of one device buffer, the alignment padding written as zeros:
 *   LAT_W(l)   uint16 [P][256 * k_l]    pack.pack_b32 fragments of W[n][c]: ph_fpn_lateral's Wp
 *   OUT_W(l)   uint16 [P][256 * 2304]   pack.pack_b32 fragments of W[n][tap * 256 + c]: ph_conv_nhwc's Wp
 *   LAT_B(l), OUT_B(l)   float [256] */
#define PH_FPACK_LAT_W(l) (2 * (l))
#define PH_FPACK_LAT_B(l) (2 * (l) + 1)
#define PH_FPACK_OUT_W(l) (8 + 2 * (l))
#define PH_FPACK_OUT_B(l) (9 + 2 * (l))
enum { PH_FPACK_COUNT = 16 };
typedef struct {
    uint64_t offset[PH_FPACK_COUNT];   /* bytes from the start of the pack, multiples of 256 */
    uint64_t bytes[PH_FPACK_COUNT];    /* size of the piece; the next piece starts at offset + bytes rounded up to 256 */
} ph_fpn_layout;
size_t ph_fpn_pack_bytes(const ph_fpn_cfg* cfg);                   /* 0 on a bad cfg (see ph_last_error_string) */
int ph_fpn_pack_layout(const ph_fpn_cfg* cfg, ph_fpn_layout* layout);
/* `params`: host array of PH_FPN_NPARAMS device pointers; `pack`: 256-byte aligned device buffer of ph_fpn_pack_bytes */
int ph_fpn_pack(const ph_fpn_cfg* cfg, const float* const* params, void* pack, void* stream);

/* ---- plan lifetime.  The workspace holds the four lateral sums as 16-bit channels-last planes, ONE fp32 channels-last conv output
 * (the largest level's) and the conv's per-workgroup GroupNorm sums, which nothing reads.  ZEROING CONTRACT: none.
 * ph_fpn_plan_create touches no device memory.  The caller keeps pack and workspace alive as long as the plan. */
typedef struct ph_fpn_plan ph_fpn_plan;
typedef struct {
    int32_t P;                  /* planes of the grade */
    int32_t prec;               /* the grade, PH_PREC_* */
    int32_t tile_rows[4];       /* per level: output rows per tile its ph_conv_nhwc launch takes at this B (2 or 4) */
} ph_fpn_geometry;
size_t ph_fpn_plan_workspace_bytes(const ph_fpn_cfg* cfg);         /* 0 on a bad cfg */
int ph_fpn_plan_create(const ph_fpn_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes, ph_fpn_plan** out);
int ph_fpn_plan_info(const ph_fpn_plan* plan, ph_fpn_geometry* out);
/* the same answer without a plan; needs no device, no pack and no workspace; every cfg error of ph_fpn_plan_create comes back
 * from here too */
int ph_fpn_geometry_of(const ph_fpn_cfg* cfg, ph_fpn_geometry* out);
void ph_fpn_plan_destroy(ph_fpn_plan* plan);

/* ---- one FPN call.
 *   stages[l]         the backbone stage [B][k_l][h_l][w_l] of cfg.x_dtype, NCHW-contiguous
 *   out_f32[l]        float [B][256][h_l][w_l], the level as the module returns it (cfg.emit_f32)
 *   out_planes[l]     the level as conv-input planes of the grade (cfg.emit_planes): channels-last [P][B][h_l * w_l][256] when
 *                     planes_layout[l] == 0, chunk-major [B][16][h_l * w_l][16] when it is PH_PLANES_C16 (one-plane grades) --
 *                     the address and the layout ph_neck_plan_level_input returns; 16-byte aligned
 *   add[l]            nullable: float [256][h_l][w_l] added to the planes (never to out_f32): the neck's positional encoding on its
 *                     pos_level; ignored without cfg.emit_planes
 * ph_fpn_plan_run_laterals: the four ph_fpn_lateral launches, coarse to fine (reads `stages` only).
 * ph_fpn_plan_run_output: level `level`'s 3x3 convolution on its lateral sum, then ONE tail launch: ph_fpn_output_planes when planes
 *   are emitted (with out_f32 when that is emitted too), else ph_fpn_output (reads that level's output entries only).
 * ph_fpn_plan_run: the laterals, then the outputs of levels 0 .. 3, all on `stream`: a captured graph of it has no parallel branches.
 * A neck plan with tower_buffers == 0 takes ph_fpn_plan_run_laterals once and then, level by level, ph_fpn_plan_run_output followed
 * by ph_neck_plan_run_level_planes (ph_neck_plan_level_input's ordering rule); the results equal ph_fpn_plan_run's. */
typedef struct {
    const void* stages[4];
    float* out_f32[4];
    uint16_t* out_planes[4];
    int32_t planes_layout[4];   /* 0 or PH_PLANES_C16 */
    const float* add[4];
} ph_fpn_io;
int ph_fpn_plan_run_laterals(ph_fpn_plan* plan, const ph_fpn_io* io, void* stream);
int ph_fpn_plan_run_output(ph_fpn_plan* plan, int level, const ph_fpn_io* io, void* stream);
int ph_fpn_plan_run(ph_fpn_plan* plan, const ph_fpn_io* io, void* stream);

/* ---- the backbone as a native object (csrc/ph_resnetplan.hip): what resnet.ResNet._pack + engine.ResNetPlan do from Python --
 * mmdet/models/backbones/resnet.py:631-646 at inference for a C / C++ caller: from the image tensor to the four stages ph_fpn_io.stages
 * takes.  Conventions are ph_fpn_plan_*'s: status codes + ph_last_error_string, caller-owned 256-byte aligned pack and workspace, no
 * allocation of device memory, no synchronisation, no host read of device data and no environment variable in pack / create / run,
 * every cfg or pointer error returned before the first launch, every run call capturable into a hipGraph (one stream, no parallel
 * branches).  The launches are ph_resnet_stem, ph_conv_cl and ph_cl_to_nchw with engine.ResNetPlan's arguments, so the bits of every
 * stage are the Python plan's.
 *   B            frames per call, 1 .. 4096
 *   H, W         image size; a size at which ph_resnet_stem, ph_conv_cl or ph_cl_to_nchw would refuse its launch is refused with its words
 *   depth        50, 101 or 152 (Bottleneck blocks (3, 4, 6, 3) / (3, 4, 23, 3) / (3, 8, 36, 3)); anything else is PH_EUNSUPPORTED
 *   mode         PH_MODE_*, mapped to the grade as ph_fpn_cfg.mode; the backbone has one-plane grades only (PH_MODE_BF16, PH_MODE_FP16):
 *                a mode whose grade is hi + lo is PH_EUNSUPPORTED
 *   x_dtype      element type of the image: PH_OUT_F32 / PH_OUT_BF16 (ph_resnet_stem's)
 *   out_dtype    element type of the stages: PH_OUT_F32 / PH_OUT_BF16 / PH_OUT_F16 (ph_cl_to_nchw's)
 *   out_mask     bit i set: stage i is written; non-zero, within the low 4 bits.  Stages behind the highest set bit are not run
 *   eps          the BatchNorm eps of the fold (finite, >= 0) */
typedef struct {
    int32_t B, H, W;
    int32_t depth;
    int32_t mode;               /* PH_MODE_* */
    int32_t x_dtype, out_dtype; /* PH_OUT_* */
    int32_t out_mask;
    double eps;
} ph_resnet_cfg;

/* ---- the parameter table: fp32 device tensors under the reference's state_dict keys, in state_dict order without the
 * num_batches_tracked entries.  Convolution c owns entries 5 c .. 5 c + 4: its weight [Cout][Cin][k][k], then its norm's weight, bias,
 * running_mean, running_var [Cout].  Convolution 0 is conv1 / bn1; then per block conv1 / bn1, conv2 / bn2, conv3 / bn3 and, where the
 * block has one, downsample.0 / downsample.1.  53 / 104 / 155 convolutions, 265 / 520 / 775 parameters at depth 50 / 101 / 152. */
#define PH_RESNET_MAX_CONVS 155
int ph_resnet_nparams(const ph_resnet_cfg* cfg);                            /* reads cfg.depth only; < 0 on a bad depth */
const char* ph_resnet_param_name(const ph_resnet_cfg* cfg, int index);      /* NULL out of range or on a bad depth */
int64_t ph_resnet_param_numel(const ph_resnet_cfg* cfg, int index);         /* elements; < 0 out of range or on a bad depth */

/* ---- packing (k_resnet_pack: the float64 BatchNorm fold and the fragment order in one kernel, one launch per convolution, once per
 * weight load).  Convolution c has two pieces, 2 c (W) and 2 c + 1 (b), each at a 256-byte aligned offset of one device buffer, the
 * alignment padding written as zeros; they are resnet.ResNet._pack's tensors, byte for byte:
 *   W   uint16 [rows * K]   pack.pack_b32 fragments of the folded W'[n][tap * Cin + c] = fp32(w[n][c][tap] * s[n]) rounded to the grade,
 *                           s = gamma / sqrt(var + eps) in float64; K = k * k * Cin; rows = Cout rounded up to a multiple of 32, the
 *                           rows at or above Cout zero.  The stem's matrix is [64][176] in resnet.stem_matrix's K order
 *                           (24 kh + 3 kw + c, zero where 3 kw + c >= 21 or K >= 168): ph_resnet_stem's Wp
 *   b   float [Cout]        b' = fp32(beta - mean * s), in float64 */
#define PH_RPACK_W(c) (2 * (c))
#define PH_RPACK_B(c) (2 * (c) + 1)
typedef struct {
    uint64_t offset[2 * PH_RESNET_MAX_CONVS];   /* bytes from the start of the pack, multiples of 256 */
    uint64_t bytes[2 * PH_RESNET_MAX_CONVS];    /* size of the piece; the next piece starts at offset + bytes rounded up to 256 */
    int32_t nconvs;                             /* convolutions in use: pieces 0 .. 2 nconvs - 1 */
    int32_t reserved;
} ph_resnet_layout;
size_t ph_resnet_pack_bytes(const ph_resnet_cfg* cfg);                      /* 0 on a bad cfg (see ph_last_error_string) */
int ph_resnet_pack_layout(const ph_resnet_cfg* cfg, ph_resnet_layout* layout);
/* `params`: host array of ph_resnet_nparams device pointers; `pack`: 256-byte aligned device buffer of ph_resnet_pack_bytes */
int ph_resnet_pack(const ph_resnet_cfg* cfg, const float* const* params, void* pack, void* stream);
/* the data gradient's operands from a packed buffer (ph_resnet_pack_bwd in the training block above); `pack_bwd`: 256-byte aligned
   device buffer of ph_resnet_pack_bwd_bytes (0 on a bad cfg) */
size_t ph_resnet_pack_bwd_bytes(const ph_resnet_cfg* cfg);
int ph_resnet_pack_bwd_layout(const ph_resnet_cfg* cfg, ph_resnet_layout* layout);
int ph_resnet_pack_bwd(const ph_resnet_cfg* cfg, const void* pack, void* pack_bwd, void* stream);

/* ---- plan lifetime.  The workspace holds engine.ResNetPlan's planes (16-bit channels-last): the stem's, two ping-pong block planes,
 * a bottleneck's two inner planes and the downsample plane.  The stages are the caller's.  ZEROING CONTRACT: none.
 * ph_resnet_plan_create touches no device memory.  The caller keeps pack and workspace alive as long as the plan. */
typedef struct ph_resnet_plan ph_resnet_plan;
typedef struct {
    int32_t prec;               /* the grade, PH_PREC_BF16 or PH_PREC_F16 */
    int32_t launches;           /* launches of ph_resnet_plan_run: 1 + convolutions of the stages run + stages written */
    int32_t nconvs;             /* ph_conv_cl launches of a run */
    int32_t stem_workgroups;    /* ph_resnet_stem_workgroups */
    int32_t c[4], h[4], w[4];   /* the four stages: [B][c][h][w] */
    int32_t nchw_workgroups[4]; /* ph_cl_to_nchw_workgroups of a stage that is written, 0 otherwise */
    int32_t conv_workgroups[PH_RESNET_MAX_CONVS];  /* ph_conv_cl_workgroups per convolution in launch order (per block: conv1, conv2,
                                                      downsample where the block has one, conv3); 0 behind nconvs */
} ph_resnet_geometry;
size_t ph_resnet_plan_workspace_bytes(const ph_resnet_cfg* cfg);            /* 0 on a bad cfg */
int ph_resnet_plan_create(const ph_resnet_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes, ph_resnet_plan** out);
int ph_resnet_plan_info(const ph_resnet_plan* plan, ph_resnet_geometry* out);
/* the same answer without a plan; needs no device, no pack and no workspace; every cfg error of ph_resnet_plan_create comes back
 * from here too */
int ph_resnet_geometry_of(const ph_resnet_cfg* cfg, ph_resnet_geometry* out);
void ph_resnet_plan_destroy(ph_resnet_plan* plan);

/* ---- one backbone call.
 *   image          [B][3][H][W] of cfg.x_dtype, NCHW-contiguous
 *   stages[i]      [B][c_i][h_i][w_i] of cfg.out_dtype, NCHW-contiguous, for every bit i of cfg.out_mask; the others are not read
 * ph_resnet_plan_run_stem: the stem's launch (reads `image`).
 * ph_resnet_plan_run_stage: stage `stage`'s bottlenecks on what the previous piece left in the workspace and, if the stage is written,
 *   its ph_cl_to_nchw launch (reads stages[stage] only).  Stage 0 follows the stem, stage i stage i - 1.
 * ph_resnet_plan_run: the stem, then stages 0 .. the highest bit of out_mask, all on `stream`. */
typedef struct {
    const void* image;
    void* stages[4];
} ph_resnet_io;
int ph_resnet_plan_run_stem(ph_resnet_plan* plan, const ph_resnet_io* io, void* stream);
int ph_resnet_plan_run_stage(ph_resnet_plan* plan, int stage, const ph_resnet_io* io, void* stream);
int ph_resnet_plan_run(ph_resnet_plan* plan, const ph_resnet_io* io, void* stream);

/* ---- N1 as a native object (csrc/ph_assocplan.hip): the association step of PolyphonicVideo.simple_test
 * (polyphonic_former_video.py:359-405) behind ph_panoptic_merge, for a C / C++ caller -- what video.VideoAssociator and
 * track_head.QuasiDenseMaskEmbedHeadGTMask string together from Python: things for tracking -> segment boxes -> FPN RoIAlign ->
 * track embedding head -> tracker -> `sem` and `track` maps.  Conventions are ph_khead_plan_* / ph_neck_plan_*'s: status codes +
 * ph_last_error_string, caller-owned 256-byte aligned memory, size queries that return 0 with a message on a bad cfg,
 * PH_EINVAL / PH_EUNSUPPORTED / PH_EWORKSPACE before the first launch, no environment variable read, no memset node (buffers are
 * zeroed by kernels).  Everything except ph_assoc_plan_match is enqueue-only and capturable into a hipGraph.
 *
 * The track head (track_heads.py:12-102): num_convs x (conv3x3 256 -> 256 without bias, GroupNorm, ReLU) on the 7 x 7 x 256 RoI
 * features, fcs.0 (256 * 49 -> fc_out_channels, ReLU), fc_embed (fc_out_channels -> embed_channels).
 *   num_convs        1 .. PH_TRACK_MAX_CONVS
 *   fc_out_channels  a multiple of 16 (PH_EINVAL otherwise) and of 32 (fc_embed's k-steps; PH_EUNSUPPORTED otherwise)
 *   embed_channels   a multiple of 16; the association plan and the tracker need 256
 *   groups           GroupNorm groups, divides 256;   eps: 0 = 1e-5
 *   prec             PH_PREC_BF16 (one bf16 plane) or PH_PREC_SPLIT (hi + lo planes) */
#define PH_TRACK_MAX_CONVS 8
typedef struct {
    int32_t num_convs, fc_out_channels, embed_channels, groups, prec;
    float eps;
} ph_track_cfg;

/* ---- the parameter table, fp32 device tensors under the reference's state_dict names, 3 num_convs + 4 entries:
 *    3 i .. 3 i + 2      convs.{i}.conv.weight [256][256][3][3], convs.{i}.gn.weight [256], convs.{i}.gn.bias [256]
 *    3 num_convs + 0..3  fcs.0.weight [F][256 * 49], fcs.0.bias [F], fc_embed.weight [E][F], fc_embed.bias [E] */
const char* ph_track_param_name(const ph_track_cfg* cfg, int index);      /* NULL out of range or on a bad cfg */
int64_t ph_track_param_numel(const ph_track_cfg* cfg, int index);         /* elements; < 0 out of range */

/* ---- packing (k_pack_pieces: one launch, once per weight load).  The pieces are QuasiDenseMaskEmbedHeadGTMask._get_pack's tensors,
 * byte for byte (hi = bf16(w) round to nearest even, lo = bf16(w - float(hi)) in fp32), each at a 256-byte aligned offset of one
 * device buffer; the alignment padding is written as zeros.  P = planes of the grade (2 for PH_PREC_SPLIT):
 *   CONV(i)          uint16 [P][256 * 2304]  pack.pack_b_fragments of W[n][tap * 256 + c] -- the (kh, kw, in) K order
 *   GAMMA(i), BETA(i)  float [256]
 *   FC               uint16 [P][F * 12544]   fragments of fcs.0.weight with its K axis permuted from ci * 49 + pos to pos * 256 + ci
 *   FC_B             float [F]
 *   EMB              uint16 [P][E * F]       fragments of fc_embed.weight;   EMB_B  float [E]
 * pieces of convs beyond num_convs are empty (0 bytes) */
#define PH_TPACK_CONV(i) (i)
#define PH_TPACK_GAMMA(i) (PH_TRACK_MAX_CONVS + (i))
#define PH_TPACK_BETA(i) (2 * PH_TRACK_MAX_CONVS + (i))
enum { PH_TPACK_FC = 24, PH_TPACK_FC_B = 25, PH_TPACK_EMB = 26, PH_TPACK_EMB_B = 27, PH_TPACK_COUNT = 28 };
typedef struct {
    uint64_t offset[PH_TPACK_COUNT];   /* bytes from the start of the pack, multiples of 256 */
    uint64_t bytes[PH_TPACK_COUNT];    /* size of the piece; the next piece starts at offset + bytes rounded up to 256 */
} ph_track_layout;
size_t ph_track_pack_bytes(const ph_track_cfg* cfg);                      /* 0 on a bad cfg (see ph_last_error_string) */
int ph_track_pack_layout(const ph_track_cfg* cfg, ph_track_layout* layout);
/* `params`: host array of 3 num_convs + 4 device pointers; `pack`: 256-byte aligned device buffer of ph_track_pack_bytes */
int ph_track_pack(const ph_track_cfg* cfg, const float* const* params, void* pack, void* stream);

/* ---- the plan's cfg.
 *   B                 frames per call
 *   Ho, Wo            size of the panoptic id map (ph_panoptic_merge's `pan`)
 *   K                 record capacity of ph_panoptic_merge (seg_records rows are 1 + 5 K words), 1 .. 1024
 *   max_things        `cap`: rows of a frame's things table = RoIs per frame the launches are sized for, 1 <= cap <= K
 *   num_thing_classes, num_stuff_classes   labels < num_thing_classes are things; void = num_thing_classes + num_stuff_classes (< 256)
 *   nlev              FPN levels RoIAlign reads, 1 .. 4, level 0 (the finest) first: h[l], w[l] and inv_stride[l] = 1 / stride
 *   finest_scale      SingleRoIExtractor's finest_scale (the shipped model: 56)
 *   track             the track head; embed_channels must be 256 */
typedef struct {
    int32_t B, Ho, Wo, K, max_things, num_thing_classes, num_stuff_classes, nlev;
    int32_t h[4], w[4];
    float inv_stride[4];
    float finest_scale;
    ph_track_cfg track;
} ph_assoc_cfg;

/* ---- plan lifetime.  ph_assoc_plan_create touches no device memory; the caller keeps pack (ph_track_pack's) and workspace alive as
 * long as the plan, both 256-byte aligned.  ZEROING CONTRACT: none -- every word a launch reads was written by an earlier launch of
 * the same run.
 * The split-K rule of the track head's GEMMs is fixed at create time: ph_gemm_rows_splitk's split of (49 cap, 256, 2304) for the
 * convs, of (cap, F, 12544) for fcs.0 and of (cap, 256, F) for fc_embed -- it depends neither on the device counts nor on B.  So (1)
 * with cap == n a frame's embeddings are bit-identical to the Python head's forward_planes on its n RoIs, and (2) for a fixed cap an
 * embedding does not depend on how many other things or frames share the launch. */
typedef struct ph_assoc_plan ph_assoc_plan;
typedef struct {
    int32_t things_words;       /* int32 words of one frame's things table: 2 + 7 cap */
    int32_t P;                  /* planes of the grade */
    int32_t conv_splits, conv_steps, fc_splits, fc_steps, emb_splits, emb_steps;   /* the three GEMMs' split-K geometry */
    int32_t vec8;               /* 1: the box kernels read 8 pixels per thread (Wo % 8 == 0; needs a 16-byte aligned pan) */
    int32_t reserved;
    uint64_t staging_bytes;     /* host staging ph_assoc_plan_match needs: B things tables + B track tables of K + 1 doubles */
    uint64_t rois_offset;       /* for inspection, bytes into the workspace: the RoIs float [B][K][5] = (0, x1, y1, x2, y2) of every id */
    uint64_t roi_planes_offset; /* ... and RoIAlign's output, uint16 bf16 planes [P][B][cap][49][256] (channels last) */
} ph_assoc_geometry;
size_t ph_assoc_plan_workspace_bytes(const ph_assoc_cfg* cfg);      /* 0 on a bad cfg */
int ph_assoc_plan_create(const ph_assoc_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes, ph_assoc_plan** out);
int ph_assoc_plan_info(const ph_assoc_plan* plan, ph_assoc_geometry* out);
void ph_assoc_plan_destroy(ph_assoc_plan* plan);

/* ---- one call for B frames, launches only.
 *   pan            int32 [B][Ho][Wo]         ph_panoptic_merge's id maps (ids 0 .. K)
 *   seg_records    int32 [B][1 + 5 K]        ph_panoptic_merge's records: nseg | seg[K][4] | scores[K]
 *   levels[l]      float [B][256][h_l][w_l]  the FPN levels, frame b at levels[l] + b * level_stride[l] (elements)
 *   sem_out        uint8 [B][Ho][Wo]         get_semantic_seg: the label of every pixel's segment, void outside
 *   things_out     int32 [B][2 + 7 cap]      per frame: nthing | seg_id[cap] | label[cap] | box[cap][5] (fp32 bits: the extent box
 *                                            x1, y1, x2, y2 and the score) | overflow -- the thing segments in the records' order
 *                                            (panoptic.segments_from_records, then video.things_for_tracking); unused rows are zero;
 *                                            a frame with more than cap things keeps the first cap and sets overflow = 1
 *   embeds_out     float [B][cap][256]       the track embeddings of rows < nthing; the other rows are not written
 * Sequence: k_assoc_things (the tables and the semantic look-up tables), k_assoc_paint (sem_out: it needs nothing from the tracker,
 * so a caller can start its download at once), the four box kernels of ph_segment_boxes with the frame in blockIdx.y and nseg = K, a
 * gather of the things' extent boxes, then RoIAlign, the split-K GEMMs and the GroupNorm kernel in their device-count forms: grids
 * sized for cap RoIs per frame, every workgroup reading its frame's nthing and returning when it lies beyond it. */
typedef struct {
    const int32_t* pan;
    const int32_t* seg_records;
    const float* levels[4];
    int64_t level_stride[4];
    uint8_t* sem_out;
    int32_t* things_out;
    float* embeds_out;
    const uint16_t* roi_planes; /* NULL, or the caller's own RoI features as bf16 planes [P][B][cap][49][256]: RoIAlign is skipped and
                                   the track head reads these (rows < nthing of every frame) */
} ph_assoc_io;
int ph_assoc_plan_run(ph_assoc_plan* plan, const ph_assoc_io* io, void* stream);

/* ---- the ONE stateful, synchronising call of the plan: the tracker and the track-id maps behind ph_assoc_plan_run on the same stream.
 * It copies the B things tables to `host_staging` (pinned host memory of ph_assoc_geometry.staging_bytes), SYNCHRONISES the stream
 * once, refuses a frame whose overflow word is set (PH_EUNSUPPORTED), calls ph_tracker_match_frames with the device embedding rows
 * (which synchronises per non-empty frame itself; frames without things are skipped and do not advance the frame counter), forms
 * each frame's track look-up table as VideoAssociator.step_device does -- ids + 1, negatives to 0, painted in segment order onto the
 * ids in the order the tracker returns them (the reference's quirk, polyphonic_former_video.py:403) -- uploads the tables and
 * launches k_assoc_paint's float64 form.  It does not wait for that launch.
 *   track_out      double [B][Ho][Wo] on the device
 *   ids_host_out   int64 [B][cap] on the host, nullable: the value painted onto thing j of frame b (0 beyond nthing)
 * Returns the number of frames matched (the caller advances its frame counter by it), or a negative error. */
int ph_assoc_plan_match(ph_assoc_plan* plan, ph_tracker* tracker, const int32_t* pan, const int32_t* things_dev, const float* embeds_dev,
                        void* host_staging, size_t staging_bytes, int64_t first_frame_id, double* track_out, int64_t* ids_host_out,
                        void* stream);

/* ---- N1: the tracker with its state ON THE DEVICE (csrc/ph_dtracker.hip).  The semantics are ph_tracker_match /
 * ph_tracker_match_frames' (quasi_dense_embed_tracker.py:47-207), decision for decision and id for id; what differs is where the
 * state lives and who walks it.  Everything -- the embedding pool, the tracklet table, the backdrop generations, the free-slot stack,
 * num_tracklets, the frame counter and a status record -- lies in ONE caller-owned 256-byte aligned device buffer; the host object
 * holds the cfg, the pointers and the sizes: no host mirror, no pinned buffer, no event.  ph_dtracker_run is launches only and
 * capturable into a hipGraph; the state carries across replays.  Conventions are the ph_*_plan_* family's: status codes +
 * ph_last_error_string, a size query that returns 0 with a message on a bad cfg, argument errors before the first launch, no
 * environment variable read, no memset node.  ZEROING CONTRACT: none, but ph_dtracker_reset must run before the first ph_dtracker_run.
 *
 * Per frame of a call, in order (a frame depends on the one before): k_dtrk_prepare (one workgroup: stable descending-score order by
 * counting, de-duplication, the memory columns), the gather of the kept rows and the pool rows, ph_track_affinity's three kernels, and
 * k_trk_update's EMA, all in device-count forms (grids sized for max_dets / capacity, the counts read from the frame record on the
 * device), with k_dtrk_assign (one workgroup: the greedy walk, new ids, the slot reservation, update_memo, expiry, status) in between.
 *
 * ERRORS are status words, not return codes: a frame is REFUSED when it needs more pool slots than are free (PH_DTRK_EPOOL), when
 * its `refuse` word is non-zero (PH_DTRK_EREFUSED) or when its count is negative or above max_dets (PH_DTRK_ECOUNT).  The reservation
 * is checked before the first mutation, so a refused frame leaves the state as the previous frame left it; its kept_counts entry is 0.
 * The error is sticky: every later frame is skipped the same way (kept_counts 0) until ph_dtracker_reset.
 *
 * The status record: PH_DTRK_ST_WORDS int64 words at ph_dtracker_layout.status. */
enum { PH_DTRK_OK = 0, PH_DTRK_EPOOL = 1, PH_DTRK_EREFUSED = 2, PH_DTRK_ECOUNT = 3 };
enum {
    PH_DTRK_ST_MATCHED = 0,        /* frames matched since the reset */
    PH_DTRK_ST_NUM_TRACKLETS = 1,  /* ids handed out (the next new id) */
    PH_DTRK_ST_ROWS = 2,           /* live tracklet rows */
    PH_DTRK_ST_ERROR = 3,          /* PH_DTRK_OK or the code of the first refusal */
    PH_DTRK_ST_REFUSED_FRAME = 4,  /* index of the first refused frame, counting every frame handed to ph_dtracker_run since the reset
                                      (empty ones included) from 0; -1: none */
    PH_DTRK_ST_FRAME_ID = 5,       /* the frame id the next matched frame gets: first_frame_id + frames matched */
    PH_DTRK_ST_FREE = 6,           /* free pool slots */
    PH_DTRK_ST_FRAMES_SEEN = 7,    /* frames handed to ph_dtracker_run since the reset */
    PH_DTRK_ST_WORDS = 8
};
typedef struct ph_dtracker ph_dtracker;
/* byte offsets into the device buffer, multiples of 256.  Tracklet rows 0 .. rows - 1 are live, in creation order; generation g of
 * the backdrops (0 = the newest frame's) has bd_count[g] rows at [g][0 .. max_dets) of its tables. */
typedef struct {
    uint64_t pool;        /* float [capacity][256] */
    uint64_t trk_id;      /* int64 [capacity] */
    uint64_t trk_seen;    /* int64 [capacity]: the frame id a row was last matched in */
    uint64_t trk_label;   /* int32 [capacity] */
    uint64_t trk_slot;    /* int32 [capacity]: the row's pool slot */
    uint64_t trk_box;     /* float [capacity][5] */
    uint64_t bd_count;    /* int32 [generations] */
    uint64_t bd_label;    /* int32 [generations][max_dets] */
    uint64_t bd_slot;     /* int32 [generations][max_dets] */
    uint64_t bd_box;      /* float [generations][max_dets][5] */
    uint64_t free_stack;  /* int32 [capacity]: entries 0 .. free - 1, the top is taken first */
    uint64_t status;      /* int64 [PH_DTRK_ST_WORDS] */
    uint64_t workspace;   /* per-frame scratch (frame record, tables, gathered rows, scores); overwritten by every frame */
    uint64_t total_bytes; /* ph_dtracker_device_bytes */
    int32_t capacity, max_dets, generations /* memo_backdrop_frames */, reserved;
} ph_dtracker_layout;
/* capacity 16 .. 4096 rows, max_dets 1 .. 128, as ph_tracker_create; cfg->metric 0 .. 2, memo_tracklet_frames >= 0,
   memo_backdrop_frames 0 .. 16.  0 with a message otherwise. */
size_t ph_dtracker_device_bytes(const ph_tracker_cfg* cfg, int capacity, int max_dets);
/* touches no device memory; the caller keeps device_mem (256-byte aligned, ph_dtracker_device_bytes) alive as long as the tracker */
int ph_dtracker_create(const ph_tracker_cfg* cfg, void* device_mem, size_t device_bytes, int capacity, int max_dets, ph_dtracker** out);
void ph_dtracker_destroy(ph_dtracker* t);
/* one launch: empty tables, full free stack, frame counter = first_frame_id, status 0 (refused frame -1) */
int ph_dtracker_reset(ph_dtracker* t, int64_t first_frame_id, void* stream);
/* for inspection and checkpointing (a C typedef and a function cannot share a name, hence get_) */
int ph_dtracker_get_layout(const ph_dtracker* t, ph_dtracker_layout* out);
/* all DEVICE pointers; frame b at base + b * stride (elements) */
typedef struct {
    const float* boxes;    int64_t box_stride;      /* [n][5]: x1, y1, x2, y2, score */
    const int32_t* labels; int64_t label_stride;
    const int32_t* counts; int64_t count_stride;    /* n of the frame; 0: the frame is skipped and does not advance the frame counter */
    const int32_t* refuse; int64_t refuse_stride;   /* nullable: a non-zero word (the things table's overflow word) refuses the frame */
    const float* embeds;   int64_t embed_stride;    /* [n][256] */
    int32_t* kept_out;     /* [B][max_dets] indices into the frame's input, descending score; entries < kept_counts[b] are written */
    int64_t* ids_out;      /* [B][max_dets]: >= 0 track id, -1 unmatched, -2 suppressed */
    int32_t* kept_counts;  /* [B] */
} ph_dtracker_io;
/* B frames in order, launches only, capturable.  The caller learns what happened from the status record whenever it next
   synchronises. */
int ph_dtracker_run(ph_dtracker* t, const ph_dtracker_io* io, int B, void* stream);

/* ---- a BANK of device trackers: `streams` independent states (1 .. 64 cameras) advanced by one frame each in ONE launch sequence.
 * Stream s's block -- its whole state and per-frame scratch, ph_dtracker_layout's layout -- lies at s * total_bytes of one caller-owned
 * buffer of ph_dtracker_bank_bytes; ph_dtracker_get_layout keeps answering for stream 0.  The kernels are ph_dtracker_run's with one
 * more grid dimension of size `streams`: a step of S streams is the seven launches of one frame, and the tracker of ph_dtracker_create
 * is the bank of one.  Streams share nothing (no atomics, no hand-off between workgroups).  Same conventions as above. */
/* 0 with a message on a bad cfg, capacity, max_dets or streams outside 1 .. 64 */
size_t ph_dtracker_bank_bytes(const ph_tracker_cfg* cfg, int capacity, int max_dets, int streams);
/* ph_dtracker_create for `streams` states; device_mem: ph_dtracker_bank_bytes, 256-byte aligned.  Destroyed by ph_dtracker_destroy */
int ph_dtracker_bank_create(const ph_tracker_cfg* cfg, void* device_mem, size_t device_bytes, int capacity, int max_dets, int streams,
                            ph_dtracker** out);
/* the stream count and the bytes between two streams' blocks (ph_dtracker_layout.total_bytes) */
int ph_dtracker_get_streams(const ph_dtracker* t, int* streams_out, uint64_t* stride_bytes_out);
/* one launch: the streams whose bit is set in `mask` (bit s = stream s; the 64 bits of the word, stream 63 being its sign bit) are
   reset as ph_dtracker_reset does -- a camera starts a new sequence --, the others are untouched.  A bit beyond the tracker's streams:
   PH_EINVAL.  ph_dtracker_reset resets every stream. */
int ph_dtracker_reset_streams(ph_dtracker* t, int64_t mask, int64_t first_frame_id, void* stream);
/* one frame of every stream: io's strides index STREAMS (frame s is stream s's next frame; kept_out / ids_out [streams][max_dets],
   kept_counts [streams]).  active: nullable DEVICE int32 [streams]; a zero word means the stream has no frame in this step -- its
   workgroups return before they read or write anything of the stream, so its state, frame counter and status keep their bits, and its
   kept_counts entry is 0.  Count 0, `refuse`, PH_DTRK_ECOUNT, PH_DTRK_EPOOL and the sticky error mean per stream what they mean for
   ph_dtracker_run; a refused or sticky stream does not affect any other.  Launches only; capturable.  ph_dtracker_run on a tracker of
   more than one stream is PH_EINVAL: its frames are in order, a bank's are side by side. */
int ph_dtracker_step(ph_dtracker* t, const ph_dtracker_io* io, const int32_t* active, void* stream);

/* ---- the launch-only counterpart of ph_assoc_plan_match: the device tracker and the track-id maps behind ph_assoc_plan_run on the
 * same stream, with no host staging and no synchronisation; capturable.  It points a ph_dtracker_io at the things tables (counts at
 * word 0, labels, boxes and the overflow word at their offsets, embeddings [B][cap][256]) one frame at a time -- the tracker's
 * per-frame outputs live in the tracker's own buffer, so the plan's workspace is what it was --, forms each frame's track look-up
 * table on the device exactly as ph_assoc_plan_match documents (ids + 1, negatives to 0, painted in segment order onto the ids in
 * the order the tracker returns them; all zero for a skipped or refused frame) and launches k_assoc_paint's float64 form.
 * Needs max_things <= the tracker's max_dets (PH_EINVAL).  A frame with more than max_things things is a refused frame
 * (PH_DTRK_EREFUSED in the status record).  The frames matched are PH_DTRK_ST_MATCHED of the status record.
 *   track_out      double [B][Ho][Wo] on the device
 *   ids_dev_out    int64 [B][cap] on the DEVICE, nullable: the value painted onto thing j of frame b (0 beyond nthing) */
int ph_assoc_plan_track(ph_assoc_plan* plan, ph_dtracker* tracker, const int32_t* pan, const int32_t* things_dev, const float* embeds_dev,
                        double* track_out, int64_t* ids_dev_out, void* stream);
/* ph_assoc_plan_track with frame b of the plan going to STREAM b of a tracker bank: one ph_dtracker_step over the things tables, one
 * k_assoc_trklut launch over the B frames, the paint.  Needs plan B == the tracker's streams and max_things <= max_dets (PH_EINVAL).
 * active: as ph_dtracker_step's; an idle stream's track map is all zero. */
int ph_assoc_plan_track_streams(ph_assoc_plan* plan, ph_dtracker* tracker, const int32_t* pan, const int32_t* things_dev,
                                const float* embeds_dev, const int32_t* active, double* track_out, int64_t* ids_dev_out, void* stream);

/* ================================================================================================================================
 * DVPQ tallies on the device (ph_dvpq.hip): what dvps_eval.video_evaluate needs from a frame, computed from the maps where they lie.
 *
 * The metric compares (gt id, pred id) intersection counts; a clip is its frames side by side, so a clip's counts are the sums of
 * its frames' counts, and a depth threshold only relabels the pred id of the pixels that violate it.  One pass over a frame
 * therefore yields a small integer table -- rows (gt id, pred id, mask of violated thresholds, pixel count) -- from which every
 * window and every threshold follows on the host (dvps_eval.clip_tallies), and the ingredients of dvps_eval.compute_errors.
 *
 * Conventions of the ph_*_plan_* family: status codes plus ph_last_error_string, a caller-owned 256-byte aligned workspace, a size
 * query that returns 0 with a message on a bad cfg, PH_EINVAL / PH_EWORKSPACE before the first launch, no environment variable
 * read, no memset node, enqueue-only and capturable into a hipGraph.  ZEROING CONTRACT: none -- the first launch clears what the
 * others read, and every word of table_out / depth_out up to the sizes below is written.
 *
 *   B, H, W      frames per call and the map size, H * W < 2^31, B <= 65535
 *   capacity     rows of a frame's table, a power of two in 64 .. 65536
 *   nthr, thr    0 .. PH_DVPQ_MAX_THR depth thresholds (not NaN).  Bit j of a pixel's mask is set iff gt_depth > 0 and
 *                |pred_depth - gt_depth| / gt_depth > thr[j], evaluated in fp32 with one correctly rounded division -- what numpy
 *                computes in dvps_eval.evaluate_clip for fp32 maps and the threshold rounded to fp32
 *
 * Per pixel g = gt_panseg, p = pred_panseg, or, with pred_panseg == NULL, (uint32)(pred_sem * 10000 + (int64)pred_track): the
 * association plan's own outputs, packed as dvps_eval.wire_record packs them.  Any uint32 is a legal id, (0, 0, 0) is a legal key.
 *
 *   table_out    uint32 [B][4 + 4 capacity]: n | overflow | 0 | 0 | n rows (g, p, mask, count) ascending in (g, p, mask) | zeros.
 *                Canonical: the same inputs give the same bytes.  A frame with more than `capacity` distinct keys sets overflow = 1
 *                and keeps n <= capacity rows of its true table (ascending, counts exact); which ones is not specified.
 *   depth_out    double [B][8] over the pixels with gt_depth > 0: their count | sum |g - p| / g | sum (g - p)^2 / g | sum (g - p)^2 |
 *                sum (ln g - ln p)^2, the terms in fp64 from the fp32 maps | the counts of max(g / p, p / g) < 1.25, 1.5625,
 *                1.953125, compared in fp32.  *_sums convention: one fixed-order partial record per workgroup, added in index order.
 *
 * Launches: k_dvpq_clear, k_dvpq_frames (grid (workgroups per frame, B): equal keys are combined inside a wave, then in a
 * per-workgroup LDS table, then in the frame's table in the workspace with 64-bit compare-and-swap and add), k_dvpq_finish (one
 * workgroup per frame: compaction, ranking, the depth partials).  Pointers: maps naturally aligned (a 16-byte aligned frame is read
 * with 16-byte loads), table_out 16-byte, depth_out 8-byte, workspace 256-byte aligned. */
#define PH_DVPQ_MAX_THR 8
typedef struct {
    int32_t B, H, W;
    int32_t capacity;                     /* power of two, 64 .. 65536 */
    int32_t nthr;                         /* 0 .. PH_DVPQ_MAX_THR */
    float thr[PH_DVPQ_MAX_THR];
} ph_dvpq_cfg;
typedef struct {
    const uint32_t* pred_panseg;          /* [B][H][W], or NULL: then pred_sem + pred_track */
    const uint8_t* pred_sem;              /* ph_assoc_plan_run's sem_out */
    const double* pred_track;             /* ph_assoc_plan_match's track_out (integral, >= 0) */
    const float* pred_depth;              /* [B][H][W] */
    const uint32_t* gt_panseg;
    const float* gt_depth;
    uint32_t* table_out;                  /* [B][4 + 4 capacity] */
    double* depth_out;                    /* [B][8] */
} ph_dvpq_io;
size_t ph_dvpq_workspace_bytes(const ph_dvpq_cfg* cfg);            /* 0 on a bad cfg (see ph_last_error_string) */
int ph_dvpq_frames(const ph_dvpq_cfg* cfg, const ph_dvpq_io* io, void* workspace, size_t workspace_bytes, void* stream);

/* ================================================================================================================================
 * The training step's Hungarian assignment and target descriptors on the device (ph_assign.hip): what losses.assign_batch (cost
 * download + scipy.optimize.linear_sum_assignment per image) and losses.build_desc (numpy pointer tables + one upload) do on the
 * host, as launches that no host code waits for.  With one-to-one matching every SIZE of the descriptor follows from the
 * ground-truth counts (ph_assign_desc_layout, a pure host function); only the contents depend on the solve.
 *
 * ph_assign_solve: cost fp32 [B][Np][ldg] on the device; counts[b * count_stride] = G_b columns of image b (clamped to 0 .. ldg),
 * read on the device.  One workgroup of one wave per image restates scipy's shortest-augmenting-path solver in fp64 -- operation
 * order, scan order of `remaining`, swap-remove and tie rule -- so the matching is the installed scipy's, ties included (transposed
 * iff G_b < Np, as scipy does).  match int32 [B][ldg]: the prediction row of ground-truth column g < G_b, -1 when G_b > Np leaves it
 * unmatched; entries at or beyond G_b are not written.  status int64 [B]: PH_ASSIGN_OK; PH_ASSIGN_ENONFINITE: a cost entry is NaN
 * or infinite (scipy raises) -- the image gets the trivial matching, column g <- row g; PH_ASSIGN_ESOLVE: a loop bound was hit
 * (cannot happen on finite costs), trivial matching likewise.  max(Np, ldg) <= PH_ASSIGN_MAX, PH_EUNSUPPORTED beyond, before any
 * launch.  Every loop of the kernel is bounded by the matrix size.
 *
 * ph_assign_desc: the one call of a head or stage.  Solves (cost != NULL and ldg > 0; with cost == NULL `match` is taken as it is: a
 * stage that re-uses the previous assignment) and writes into `blob` every section losses.build_desc produces, byte for byte, the
 * 16-byte section alignment and the one-element placeholders of empty sections included; every byte up to total_bytes is written.
 *   cfg        B <= PH_ASSIGN_MAX_B images, Np proposals, N rows per image (Np, + n_stuff for the roi form with stuff), L classes,
 *              roi: KernelUpdateHead's form (label_w, one depth row per row), else KernelHead's (sstart / sit_m / sit_l, one depth
 *              row per image); pos_weight as build_desc resolves it (<= 0 there: 1)
 *   G, S       HOST int32 [B]: instances and stuff masks per image (S nullable without has_sem); last_pos HOST int32 [B], nullable:
 *              1 where the image's last row is a positive (roi form: its depth item gives way to the direct-depth item)
 *   gt_table   DEVICE int64 [gt_words]: B records of PH_ASSIGN_GT_WORDS words -- G_b | S_b | address of the masks fp32 [G][HW] |
 *              of the stuff masks [S][HW] | of the valid map [HW] | of the depth map [HW] | word index of the G_b labels | of the
 *              S_b stuff classes (distinct within an image, n_thing .. n_thing + n_stuff - 1) -- then the labels and classes
 *   match, status   DEVICE int32 [B][max(ldg, 1)], int64 [B]
 * PH_EUNSUPPORTED (before any launch) beyond the limits and for the roi form with depth but without stuff rows. */
#define PH_ASSIGN_MAX 256
#define PH_ASSIGN_MAX_B 64
#define PH_ASSIGN_GT_WORDS 8
enum { PH_ASSIGN_OK = 0, PH_ASSIGN_ENONFINITE = 1, PH_ASSIGN_ESOLVE = 2 };
typedef struct {
    int32_t B, Np, N, L, n_thing, n_stuff;
    int32_t roi, has_sem, has_depth;
    float pos_weight;
    int64_t HW;
} ph_assign_cfg;
typedef struct {
    uint64_t tptr, wptr, labels, pos_u8, pos_rows, dstart, dit_t, dit_w, dit_s, label_w, sstart, sit_m, sit_l;   /* byte offsets */
    uint64_t total_bytes;
    int64_t P;             /* positives: LossCfg.P and the focal normaliser */
    int64_t depth_items, seg_items, depth_rows;
} ph_assign_layout;
int ph_assign_desc_layout(const ph_assign_cfg* cfg, const int32_t* G, const int32_t* S, const int32_t* last_pos, ph_assign_layout* out);
int ph_assign_solve(const float* cost, int B, int Np, int ldg, const int32_t* counts, int64_t count_stride, int32_t* match, int64_t* status,
                    void* stream);
int ph_assign_desc(const ph_assign_cfg* cfg, const int32_t* G, const int32_t* S, const int32_t* last_pos, const float* cost, int ldg,
                   const int64_t* gt_table, int64_t gt_words, int32_t* match, int64_t* status, void* blob, size_t blob_bytes, void* stream);

/* ---- training the track head: QDTrack targets, both losses and their gradients in ONE call (csrc/ph_trackloss.hip) -------------
 * Replaces, for `pairs` key / reference image pairs, get_track_targets + match + loss of QuasiDenseMaskEmbedHeadGTMask
 * (polyphonic/video/track_heads.py:104-162) with cal_similarity, MultiPosCrossEntropyLoss and L2Loss (hard mining) behind them, for
 * softmax_temp <= 0.  One workgroup per pair; launches only: no allocation, no synchronisation, no atomics, fixed summation orders
 * (fp32 products, fp64 loss sums), so two calls on the same inputs give the same bits and a pair's numbers do not depend on the
 * other pairs of the call.
 *   cfg        pairs <= PH_TRACK_LOSS_MAX_PAIRS, E (embedding width, a multiple of 4), the two loss weights, L2Loss's neg_pos_ub
 *              (<= 0: no mining), pos_margin / neg_margin (applied when > 0) and hard_mining.  hard_mining == 0 with neg_pos_ub > 0
 *              is PH_EINVAL: whether a pair exceeds the bound is known on the device only, and the reference's random choice is not
 *              implemented.
 *   key_start, ref_start, match_start   HOST int32 [pairs + 1]: row offsets of each pair's RoIs in key_emb / ref_emb (and key_gt /
 *              ref_gt) and of its ground truths in gt_match.  1 .. PH_TRACK_LOSS_MAX_ROIS RoIs per side and pair, PH_EINVAL
 *              otherwise (the reference asserts on an empty side); checked before anything is launched.
 *   key_emb [sum Nk][E], ref_emb [sum Nr][E]   DEVICE fp32, 16-byte aligned
 *   key_gt [sum Nk], ref_gt [sum Nr]   DEVICE int32: pos_assigned_gt_inds of every RoI; a key index outside the pair's gt_match
 *              range matches nothing
 *   gt_match   DEVICE int32: per key-frame ground truth its index among the reference frame's, or -1
 *   target[i][j] = (gt_match[key_gt[i]] == ref_gt[j]); row weight = any_j target.
 *   losses [2] DEVICE: loss_track, loss_track_aux, weighted and divided by `pairs`
 *   g_key, g_ref   DEVICE, nullable together: d(loss_track + loss_track_aux) / d(embedding), overwritten
 *   scratch    DEVICE, 16-byte aligned, the bytes the size query returns (PH_EWORKSPACE when smaller)
 * Hard mining: when num_neg > neg_pos_ub * (num_pos + 1), the num_pos * neg_pos_ub negatives of largest squared clamped cost keep
 * weight 1, found by a bitwise select on the costs' bit patterns in LDS; TIES at the cut go to the lowest row-major index i * Nr + j
 * (torch.topk leaves its tie order unspecified; ties at cost 0 change neither loss nor gradient).  The clamp's gradient is 1 on the
 * closed interval.  A pair without any positive gives 0 / 0 as in the reference: NaN in both losses and in every gradient row of
 * that pair, the other pairs' rows unaffected. */
#define PH_TRACK_LOSS_MAX_ROIS 128
#define PH_TRACK_LOSS_MAX_PAIRS 64
typedef struct {
    int32_t pairs, E;
    float lw_track, lw_aux;
    int32_t neg_pos_ub;
    float pos_margin, neg_margin;
    int32_t hard_mining;
} ph_track_loss_cfg;
size_t ph_track_loss_scratch_bytes(const ph_track_loss_cfg* cfg, int total_key, int total_ref);
int ph_track_loss(const ph_track_loss_cfg* cfg, const float* key_emb, const float* ref_emb, const int32_t* key_start,
                  const int32_t* ref_start, const int32_t* key_gt, const int32_t* ref_gt, const int32_t* match_start,
                  const int32_t* gt_match, float* losses, float* g_key, float* g_ref, void* scratch, size_t scratch_bytes, void* stream);
/* Gradient of ph_roi_align_fpn's fp32 output into the FPN levels: g_roi [n][256][7][7] -> g_feats[l] [1][256][H_l][W_l] (HOST array
 * of DEVICE pointers), every level overwritten in full, zeros included.  The forward's level map and sampling.  A gather: one thread
 * per pixel and 16 channels walks the RoIs in index order (the weight of bin (ph, pw) on pixel (y, x) is Wy[ph](y) Wx[pw](x) / 4), so
 * there are no atomics and two calls give the same bits.  n <= 1024. */
int ph_roi_align_fpn_bwd(const float* g_roi, const int32_t* hw, const float* scales, int nlev, const float* rois, int n,
                         float finest_scale, float* const* g_feats, void* stream);

/* ---- the RoIs of a training step's sampled ground-truth masks, from the masks at the assign resolution (csrc/ph_gtbox.hip) -------
 * Replaces, for `frames` key / reference frames, what PolyphonicVideo.forward_train does per sampled mask on the host
 * (polyphonic_former_video.py:283-305, 413-415; video/utils.py:39-83): F.interpolate(size = (H, W), bilinear, align_corners = False)
 * of the mask [h][w], sigmoid > 0.5, nonzero, centre +- 2 max(mean |deviation|, 1) per axis, (0, 0, 0, 0) for an empty mask,
 * bboxlist2roi and clamp(min = 0).  No [n][H][W] tensor is formed: a box needs the row and column pixel counts r[Y], c[X] only,
 *     n = sum r,  mean_y = sum Y r[Y] / n,  MAD_y = sum r[Y] |Y - mean_y| / n  (likewise in x),
 * counts and coordinate sums are integers, means and deviations fp64, each coordinate rounded once to fp32.
 *
 * The selection happens in the same call.  match: DEVICE int32, row b * match_stride of frame b as ph_assign_solve leaves it -- the
 * prediction row of ground truth g < G[b], or -1.  The frame's RoIs come out in ascending prediction row (MaskPseudoSampler's
 * pos_inds): RoI r is the ground truth whose row has rank r among the matched ones, and pos_gt[r] is that ground truth (the
 * reference's pos_assigned_gt_inds, the form ph_track_loss takes as key_gt / ref_gt).  n[b] = min(G[b], Np) is the number of matched
 * ground truths: the host knows it from the counts, so no size depends on a download.  A match row with more entries >= 0 than n[b]
 * has the surplus ranks dropped, one with fewer leaves the last rows of the frame unwritten; nothing is written out of bounds.
 *
 * The per-pixel predicate is ATen's bilinear form in fp32 without contraction -- source index scale (dst + 0.5) - 0.5 clamped at 0,
 * scale = float(in) / out, h0 (w0 a + w1 b) + h1 (w0 c + w1 d), the + 1 tap falling on the same pixel at the last row / column --
 * followed by the fp32 sigmoid test (value > 1.5 * 2^-24).  INPUT CONTRACT: the masks are non-negative (ground-truth masks), and no
 * upsampled value lies in (0, 2^-20); then a pixel is on exactly when a tap with a non-zero weight is positive, whatever the rounding
 * of the evaluation.  (A binary mask downsampled bilinearly by 4 and upsampled again has no positive value below 2^-8.)
 *
 *   masks      HOST [frames] of DEVICE fp32 [G[b]][h][w] (NULL allowed where G[b] == 0)
 *   G, n, roi_start   HOST int32 [frames]: ground truths (0 .. PH_ASSIGN_MAX), matched count (<= PH_TRACK_LOSS_MAX_ROIS), first row of
 *              the frame in rois / pos_gt / count.  A frame with n == 0 writes nothing.
 *   h, w, H, W one size for the call; H >= h and W >= w, any ratio, at most 65536.  mode: PH_GTBOX_BILINEAR; the nearest mode of the
 *              semantic_kitti configuration is PH_EUNSUPPORTED, as is a downsample
 *   rois [sum n][5] fp32 (0, x1, y1, x2, y2) | pos_gt [sum n] int32 | count [sum n] int64: the on pixels of the upsampled mask
 *   workspace  DEVICE, 16-byte aligned, ph_gtmask_boxes_workspace_bytes = al256(S H 4) + al256(S ceil(H / 64) W 2) bytes with
 *              S = sum G and al256 rounding up to 256: the row histograms and, per band of 64 rows, the column partials
 * Launches only (two): no allocation, no synchronisation, no atomics, no memset node, capturable.  ZEROING CONTRACT: none -- every
 * word the second launch reads is written by the first.  Integer sums: two calls give the same bits and a frame's rows do not depend
 * on the other frames of the call.  PH_EINVAL (n > 128, n != min(G, Np), ...) / PH_EUNSUPPORTED / PH_EWORKSPACE are returned
 * before anything is launched. */
#define PH_GTBOX_MAX_FRAMES 64
enum { PH_GTBOX_BILINEAR = 0, PH_GTBOX_NEAREST = 1 };
size_t ph_gtmask_boxes_workspace_bytes(int frames, const int32_t* G, int H, int W);   /* 0 on a bad argument (ph_last_error_string) */
int ph_gtmask_boxes(const float* const* masks, const int32_t* G, const int32_t* n, const int32_t* roi_start, const int32_t* match,
                    int64_t match_stride, int Np, int frames, int h, int w, int H, int W, int mode, float* rois, int32_t* pos_gt,
                    int64_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a training step's ground truth from one segment-index map per frame (csrc/ph_gtprep.hip).  A loader's masks of a frame are
 * disjoint (they tile the image), so the [G][Hp][Wp] stack polyphonic_former_video.py:115 uploads as fp32 is one byte per pixel: the
 * index of the pixel's segment in the loader's list, 255 where there is none.  This call turns `frames` such maps into everything
 * the step reads at the assign resolution (:114-138 and what losses.StepGT derives from it):
 *   seg        DEVICE uint8 [frames][Hs][Ws], the loader's un-padded size.  Pixels at y >= Hs or x >= Ws up to the padded size
 *              Hp x Wp read as "no segment" (the F.pad(..., value=0) of :116-118).
 *   row_of     DEVICE int32 [frames][256]: segment index -> output row.  0 .. Gmax-1 a row of `things`, Gmax .. Gmax+Smax-1 row
 *              (value - Gmax) of `stuff`, anything else (-1) dropped.  Entry 255 and the entries from nseg[b] on count as -1 whatever they hold.
 *   nseg       HOST int32 [frames]: segments in the frame's list, 0 .. PH_GTPREP_MAX_SEGMENTS
 *   depth      DEVICE fp32 [frames][Hp][Wp] or NULL (then depth_out is NULL too)
 *   things [frames][Gmax][aH][aW] | stuff [frames][Smax][aH][aW] fp32: the soft masks; rows no segment maps to are zero, so
 *              `things` is the zero-padded stack the batched assignment reads.  NULL allowed for a stack without rows.
 *   things_hard, stuff_hard   the same shapes or NULL: value != 0 ? 1 : 0 (kernel_head.py:400-403)
 *   valid [frames][aH][aW] fp32: 1 where any row of either stack is non-zero | depth_out [frames][aH][aW] fp32
 * Arithmetic, fp32 without contraction.  PH_GTBOX_BILINEAR: ATen's bilinear form (align_corners = False), scale = float(in) / out
 * with in the PADDED size, source index max(scale (dst + 0.5) - 0.5, 0), the + 1 tap falling on the same pixel at the last row /
 * column, value h0 (w0 a + w1 b) + h1 (w0 c + w1 d) with a .. d = 1.0 where the tap's segment maps to the row, else 0.0.
 * PH_GTBOX_NEAREST: the tap at min(floor(dst scale), in - 1).  The depth map is always nearest (:135-138).
 * One launch: no allocation, no synchronisation, no atomics, no workspace, capturable.  ZEROING CONTRACT: none -- every word of
 * every output is written, zeros included.  Two calls give the same bits; a frame's outputs do not depend on the other frames.
 * PH_EINVAL (more than 254 segments in a frame, Gmax or Smax above PH_ASSIGN_MAX, Hs > Hp, Ws > Wp, a size <= 0, ...) is returned
 * before anything is launched. */
#define PH_GTPREP_MAX_FRAMES 64
#define PH_GTPREP_MAX_SEGMENTS 254
int ph_gt_prepare(const uint8_t* seg, const int32_t* row_of, const int32_t* nseg, const float* depth, int frames, int Hs, int Ws, int Hp,
                  int Wp, int aH, int aW, int Gmax, int Smax, int mode, float* things, float* stuff, float* things_hard,
                  float* stuff_hard, float* valid, float* depth_out, void* stream);

/* ---- the segment-index maps themselves from the dataset's panoptic id maps (csrc/ph_gtseg.hip).  In the file a frame's ground truth
 * is one raw id per pixel, class * raw_divisor + instance, and it stays one id per pixel through every transform of the shipped
 * train_pipeline (nearest resize, flip, crop, pad: separable nearest gathers).  The two calls replace the loader's numpy work in front
 * of ph_gt_prepare: to_coco (datasets/cityscapes_dvps.py:89-109), np.unique and a full-frame compare per segment
 * (datasets/pipelines/loading.py:201-220), bitmasks2bboxes (:11-21), and the resize / flip / crop / pad of the [G][H][W] stack and of
 * the depth map (datasets/pipelines/transforms.py).  The loader keeps the id map and the augmentation's parameters.
 *
 * Shared arguments:
 *   raw        DEVICE [frames][Hs][Ws], int32 (PH_GTSEG_I32) or uint16 (PH_GTSEG_U16), the ids as the file holds them; fewer than
 *              2^31 pixels a frame
 *   class_map  HOST int32 [n_map], raw class -> training class 0 .. 255; -1: not a class of this dataset; the no-object class maps
 *              to no_obj_class.  Two raw classes must not map to one training class other than no_obj_class (PH_EINVAL: their segments
 *              would share ids).  It travels as a kernel argument; n_map <= 256.
 *   raw_divisor, divisor   1 <= raw_divisor <= divisor <= 2^23.  mapped id = class_map[raw / raw_divisor] * divisor + raw % raw_divisor
 *              (to_coco; a pixel whose mapped class is no_obj_class belongs to no segment, whatever its instance part)
 * THE LIMIT: n_map * raw_divisor <= PH_GTSEG_MAX_KEYS (262144 raw ids: a presence bitmap of 32 KB, one workgroup's LDS), beyond it
 * PH_EUNSUPPORTED before any launch.  Cityscapes-DVPS has 33 * 1000.
 *
 * ph_gt_segments: one segment table per frame, what loading.py:201-220 and bitmasks2bboxes leave at file resolution.
 *   tables     DEVICE int32 [frames][PH_GTSEG_TABLE_WORDS]: word 0 the count n of segments (no-object excluded), then
 *              PH_GTPREP_MAX_SEGMENTS rows of (mapped id, xmin, ymin, xmax, ymax, area), ascending by mapped id -- np.unique's order --
 *              boxes inclusive in pixels, rows from n on zero
 *   status     DEVICE int32 [frames]: 0, or an OR of PH_GTSEG_ETOOMANY (more than 254 segments), PH_GTSEG_EUNMAPPED (an id whose
 *              class maps to -1), PH_GTSEG_EOUTSIDE (an id below 0 or at or above n_map * raw_divisor).  A stuff id with a non-zero
 *              instance part is no error (the reference only asserts it).  Always written.  A frame with a non-zero status keeps
 *              its table as the caller left it; the other frames of the call are not affected.
 *   workspace  DEVICE, 256-byte aligned, ph_gt_segments_workspace_bytes: per frame the presence bitmap, the keys present and their rows
 * Four launches, nothing else: no allocation, no synchronisation, no host read, no memset node, capturable.  ZEROING CONTRACT: none --
 * the first launch clears what the others accumulate into, and every word of the table of a frame with status 0 is written.  Integer
 * atomics only (or, min, max, add): the order and every number are exact, two calls give the same bits, a frame's outputs do not
 * depend on the other frames of the call.
 *
 * ph_gt_index_maps: the raw maps through the augmentation, a pure gather; it takes no position on any resize rule.
 *   kept_id    DEVICE int32 [frames][256]: the mapped ids of the segments the crop kept, ascending; a pixel's output is its
 *              segment's index in this list (the index in the loader's list).  kept_n HOST int32 [frames]: 0 .. 254 entries
 *   src_y, src_x   DEVICE int32 [frames][Hc] and [frames][Wc]: the file row / column of every output row / column; -1: none (the
 *              pixel has no segment and depth 0 -- a frame smaller than the call's Hc x Wc).  src_y_host, src_x_host: the same words
 *              on the HOST, bounds-checked before anything is launched (PH_EINVAL); the caller keeps the two copies equal, and an
 *              index the kernels find outside the file reads as -1
 *   raw_depth  DEVICE uint16 [frames][Hs][Ws] or NULL (then depth is NULL too); depth_div (256), depth_max (80); scale_mean HOST fp32
 *              [frames], the mean of the frame's resize factors
 *   seg        uint8 [frames][Hc][Wc], any alignment: the index in kept_id, 255 where the mapped id is not in it (dropped, no-object,
 *              unmapped, outside).  One 16-byte store per 16 pixels where Wc is a multiple of 16 and seg 16-byte aligned, bytes otherwise
 *   depth      fp32 [frames][Hp][Wp], Hp >= Hc, Wp >= Wc: min(float(u) / depth_div, depth_max) / scale_mean in fp32 with IEEE
 *              divisions (numpy's bits), zero outside Hc x Wc
 * Two launches (one without depth): no allocation, no synchronisation, no atomics, no workspace, capturable.  ZEROING CONTRACT:
 * none -- every word of both outputs is written, the pad included.  Two calls give the same bits; a frame's outputs do not depend on
 * the other frames.  The output is what ph_gt_prepare takes as seg (Hs, Ws there = Hc, Wc here) and depth. */
#define PH_GTSEG_MAX_KEYS 262144
#define PH_GTSEG_ROW_WORDS 6
#define PH_GTSEG_TABLE_WORDS (1 + PH_GTPREP_MAX_SEGMENTS * PH_GTSEG_ROW_WORDS)
enum { PH_GTSEG_I32 = 0, PH_GTSEG_U16 = 1 };
enum { PH_GTSEG_ETOOMANY = 1, PH_GTSEG_EUNMAPPED = 2, PH_GTSEG_EOUTSIDE = 4 };
size_t ph_gt_segments_workspace_bytes(int frames, int n_map, int raw_divisor);   /* 0 on a bad argument (ph_last_error_string) */
int ph_gt_segments(const void* raw, int dtype, int frames, int Hs, int Ws, const int32_t* class_map, int n_map, int raw_divisor,
                   int divisor, int no_obj_class, int32_t* tables, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int ph_gt_index_maps(const void* raw, int dtype, const uint16_t* raw_depth, int frames, int Hs, int Ws, const int32_t* class_map, int n_map,
                     int raw_divisor, int divisor, int no_obj_class, const int32_t* kept_id, const int32_t* kept_n,
                     const int32_t* src_y_host, const int32_t* src_x_host, const int32_t* src_y, const int32_t* src_x, int Hc, int Wc, int Hp,
                     int Wp, float depth_div, float depth_max, const float* scale_mean, uint8_t* seg, float* depth, void* stream);

/* ---- the image of the same frame from the file's bytes (csrc/ph_imgprep.hip): the reference's train_pipeline on the image
 * (configs/_base_/datasets/cityscapes_dvps.py:8-21: bilinear resize on uint8, horizontal flip, crop, Normalize, Pad(size_divisor = 32),
 * the transpose to CHW) and its test_pipeline (:23-41: Normalize, Pad, ImageToTensor) in one launch, ending at the tensor the backbone
 * takes.  Like ph_gt_index_maps it takes TABLES, not a resize rule: the host composes resize, flip and crop into one two-tap table per
 * axis and frame (image.bilinear_tables), with the augmentation parameters ph_gt_index_maps' tables are made of, so the image and the
 * ground truth of a frame cannot disagree on geometry.
 *   raw        DEVICE uint8 [frames][Hs][Ws][3], the image as decoded from the file, interleaved channels, any alignment.
 *              Hs, Ws <= 32767, beyond it PH_EUNSUPPORTED
 *   tab_y, tab_x   DEVICE int32 [frames][Hc][2] and [frames][Wc][2], 8-byte aligned.  Word 0 = i0 | i1 << 16: the two source rows /
 *              columns of the output row / column; word 0 == -1: none, the pixel is pad (a frame smaller than the call's Hc x Wc).
 *              Word 1 = w0 | w1 << 16: the two tap weights, each 0 .. 2048 (11 coefficient bits).  Both indices and both weights
 *              travel: OpenCV's rule does not make i1 = i0 + 1 or w0 = 2048 - w1 in every case.  tab_y_host, tab_x_host: the same
 *              words on the HOST, checked before anything is launched (PH_EINVAL: an index at or above Hs / Ws, a weight above 2048);
 *              the caller keeps the two copies equal, and an index the kernel finds outside the file reads as none
 *   mean, stdinv   HOST fp32 [3], finite; to_rgb 0 or 1.  With to_rgb = 1 output channel c reads input channel 2 - c, and mean /
 *              stdinv index the OUTPUT channel, as mmcv.imnormalize does after its colour conversion
 *   out        out_dtype PH_OUT_F32 or PH_OUT_BF16 (round to nearest even), aligned to its element; layout PH_IMG_NCHW
 *              [frames][3][Hp][Wp] or PH_IMG_NHWC [frames][Hp][Wp][3] (the memory of a channels-last tensor of shape
 *              [frames, 3, Hp, Wp]); Hp >= Hc, Wp >= Wc
 * ARITHMETIC, exact by definition (S a source byte, a / b the weights of tab_x / tab_y; OpenCV's generic fixed-point INTER_LINEAR path
 * for 8-bit images):
 *     H0 = S[y0][x0][c] a0 + S[y0][x1][c] a1                                        (int32; H1 the same on row y1)
 *     v  = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2               (0 .. 255 where a0 + a1 = b0 + b1 = 2048)
 *     out = (float(v) - mean[c]) stdinv[c]                                          (fp32: one subtract, one multiply)
 * and exactly +0.0 outside Hc x Wc and where a table word is -1: the reference pads AFTER Normalize, so the pad is zero in normalised
 * units.  Identity tables (w0 = 2048, w1 = 0) return S itself, so the test pipeline, which does not resize, is the same code path.
 * One launch: no allocation, no synchronisation, no atomics, no workspace, capturable.  ZEROING CONTRACT: none -- every word of the
 * output is written, the pad included.  Two calls give the same bits; a frame's output does not depend on the other frames.  A wave
 * writes 512 adjacent columns of one row, a lane 8 of them: 16-byte stores, contiguous from lane to lane in either layout, where Wp is a
 * multiple of 16 bytes of elements (4 fp32, 8 bf16) and out is 16-byte aligned, element stores otherwise.  The source is read with
 * unaligned 8-byte loads that stay inside [raw, raw + frames Hs Ws 3).  A bad argument returns its code before anything is launched,
 * with ph_last_error_string naming it. */
#define PH_IMGPREP_MAX_FRAMES 64
enum { PH_IMG_NCHW = 0, PH_IMG_NHWC = 1 };
int ph_image_prepare(const uint8_t* raw, int frames, int Hs, int Ws, const int32_t* tab_y_host, const int32_t* tab_x_host,
                     const int32_t* tab_y, const int32_t* tab_x, int Hc, int Wc, int Hp, int Wp, const float* mean, const float* stdinv,
                     int to_rgb, int out_dtype, int layout, void* out, void* stream);

/* ---- the optimizer step: gradient clipping by the global L2 norm + AdamW over every tensor in ONE call (csrc/ph_optim.hip) ------
 * Replaces torch.nn.utils.clip_grad_norm_(max_norm, norm_type = 2) + torch.optim.AdamW.step (the schedule of every shipped config:
 * AdamW(lr = 2e-4, weight_decay = 0.05) behind grad_clip = dict(max_norm = 1, norm_type = 2)) without rewriting a gradient.
 *
 * THE TABLE.  One ph_optim_tensor per tensor, the same bytes on the host (table_host: read by the argument checks) and on the device
 * (table_dev: read by the kernels; the caller uploads it and keeps the two equal).  p, g, m, v: DEVICE fp32 [n], any 4-byte
 * alignment; g == NULL: the tensor takes no part in the call (torch's `.grad is None`).  lr: the tensor's base rate, multiplied by
 * the call's lr_factor; weight_decay: decoupled, as AdamW's.
 *
 * WORK ITEMS.  An item is one chunk of PH_OPTIM_CHUNK elements of ONE tensor, the last chunk of a tensor short; the items are numbered
 * tensor by tensor and first_item is the number of the tensor's first one (a tensor of n == 0 has none and shares its number with its
 * successor; n > 0 with g == NULL keeps its items, which do nothing).  The call checks the column.  A workgroup of 256 threads takes
 * items in a grid-stride loop (at most max_blocks workgroups; 0: the library's choice), finds an item's tensor by a search over the
 * column in LDS, and moves 16 bytes per lane where p, g, m, v of the tensor are all 16-byte aligned, 4 bytes otherwise and on the
 * last n % 4 elements.  Everything a launch reduces is stored per item and summed in index order: no float atomics, and the results
 * do not depend on the grid.
 *
 * AT MOST THREE LAUNCHES, nothing else: no allocation, no synchronisation, no memset node, capturable.
 *   1. k_optim_sumsq     partial[item] = sum g^2, squared and summed in fp64 from the element up (a finite |g| > 1.8e19 does not
 *                        overflow).  Omitted when neither max_norm > 0 nor PH_OPTIM_SKIP_NONFINITE asks for the norm.
 *   2. k_optim_finalize  one workgroup: the partials in a fixed tree in fp64, norm = sqrt(sum), coef = max_norm / (norm + 1e-6) clamped
 *                        at 1 as torch does (a NaN stays a NaN; max_norm <= 0: coef = 1), skip = norm not finite and
 *                        PH_OPTIM_SKIP_NONFINITE; when not skipping the step counter t advances; 1 - beta1^t and sqrt(1 - beta2^t) in
 *                        fp64, each rounded once to fp32; the state record.
 *   3. k_optim_update    torch's _single_tensor_adamw in fp32 without contraction, g' = g coef on the fly, lr = tensor lr * lr_factor:
 *                            p *= 1 - lr wd;  m += (g' - m)(1 - beta1);  v = beta2 v + ((1 - beta2) g') g';
 *                            p += (-(lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps)
 *                        (1 - lr wd and lr / bc1 formed in fp64 and rounded once, as torch's Python scalars are).  g is NOT modified
 *                        unless PH_OPTIM_ZERO_GRADS is set: then zeros are stored over every gradient read.  On a skipped call p, m,
 *                        v and the step counter keep their bits; the gradients are still zeroed if asked.
 * lr_factor_dev != NULL: the factor is read from that DEVICE fp32 by the kernel (a captured graph follows a schedule); else the
 * host value lr_factor is used.
 *
 * state      DEVICE, 8-byte aligned, zeroed by the caller before the first call (step 0): see ph_optim_state
 * workspace  DEVICE, 256-byte aligned, ph_optim_workspace_bytes: the fp64 partials.  ZEROING CONTRACT: none.
 * PH_EINVAL (ntensors <= 0, n < 0, a null p / m / v with n > 0, a first_item that is not the running item count, beta1 / beta2
 * outside [0, 1), eps <= 0, a misaligned state or workspace), PH_EUNSUPPORTED (more than PH_OPTIM_MAX_TENSORS tensors, 2^31 items)
 * and PH_EWORKSPACE are returned before anything is launched, with ph_last_error_string naming the argument. */
#define PH_OPTIM_CHUNK 4096
#define PH_OPTIM_MAX_TENSORS 4096
enum { PH_OPTIM_SKIP_NONFINITE = 1, PH_OPTIM_ZERO_GRADS = 2 };      /* ph_optim_cfg.flags */
enum { PH_OPTIM_OK = 0, PH_OPTIM_ENONFINITE = 1 };                  /* ph_optim_state.status */
typedef struct {
    float* p;
    float* g;
    float* m;
    float* v;
    int64_t n;
    double lr, weight_decay;
    int64_t first_item;
} ph_optim_tensor;
typedef struct {
    double beta1, beta2, eps;
    double max_norm;         /* <= 0: no clipping */
    int32_t flags;
    int32_t max_blocks;      /* workgroups per launch at most; 0: the library's choice.  The results do not depend on it */
} ph_optim_cfg;
typedef struct {
    int64_t step;            /* calls applied so far: AdamW's t, ONE count for every tensor */
    int64_t skipped;         /* calls skipped so far */
    int32_t status;          /* of the last call: PH_OPTIM_OK, or PH_OPTIM_ENONFINITE: its norm was not finite */
    int32_t skip;            /* 1: the last call was skipped (p, m, v, step untouched) */
    float grad_norm;         /* of the last call, before clipping; -1 where the call did not ask for it */
    float clip_coef;         /* g' = g clip_coef */
    float bias1, bias2_sqrt; /* 1 - beta1^step, sqrt(1 - beta2^step) */
} ph_optim_state;
size_t ph_optim_workspace_bytes(const ph_optim_tensor* table_host, int ntensors);   /* 0 on a bad table (ph_last_error_string) */
int ph_optim_step(const ph_optim_cfg* cfg, const ph_optim_tensor* table_host, const ph_optim_tensor* table_dev, int ntensors,
                  float lr_factor, const float* lr_factor_dev, ph_optim_state* state, void* workspace, size_t workspace_bytes,
                  void* stream);
/* zeros over every gradient of the table, in place: ONE launch, the same items (the table checks of ph_optim_step apply) */
int ph_optim_zero_grads(const ph_optim_tensor* table_host, const ph_optim_tensor* table_dev, int ntensors, int max_blocks, void* stream);

/* ---- self tests of the gfx950 fragment layouts the kernels rely on (tests/test_gpu_selftest.py) */
int ph_selftest_mfma16(const uint16_t* a /*[16][32]*/, const uint16_t* bt /*[16][32]*/, float* d /*[16][16]*/, void* stream);
int ph_selftest_mfma32(const uint16_t* a /*[32][16]*/, const uint16_t* bt /*[32][16]*/, float* d /*[32][32]*/, void* stream);
int ph_selftest_readbw(const void* p, int64_t bytes, int blocks, void* out /*4 B*/, void* stream);   /* streaming-read yardstick */
int ph_selftest_trread(const uint16_t* src /*[16][16]*/, uint16_t* out /*[64][4]*/, void* stream);
/* holds `blocks` workgroup slots with `lds_bytes` of LDS each for `microseconds` (a CU-hogging neighbour for the time-out tests) */
int ph_selftest_hog(int blocks, int lds_bytes, int microseconds, void* scratch4, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POLYHEAD_H_ */
