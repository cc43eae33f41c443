// Shared device helpers for libpolyhead (gfx950 / CDNA4 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/polyhead.h"

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8_t;
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4_t;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4_t;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float f32x16_t;

#define PH_LDS __attribute__((address_space(3)))

void ph_set_error(const char* fmt, ...);

#define PH_CHECK_ARG(cond, msg)                                        \
    do {                                                               \
        if (!(cond)) {                                                 \
            ph_set_error("%s: %s", __func__, msg);                     \
            return PH_EINVAL;                                          \
        }                                                              \
    } while (0)

// the same under the public entry point's name, for its internal *_k form
#define PH_CHECK_ARG_AS(fn, cond, msg)                                 \
    do {                                                               \
        if (!(cond)) {                                                 \
            ph_set_error("%s: %s", fn, msg);                           \
            return PH_EINVAL;                                          \
        }                                                              \
    } while (0)

#define PH_CHECK_LAUNCH()                                                          \
    do {                                                                           \
        hipError_t e_ = hipGetLastError();                                         \
        if (e_ != hipSuccess) {                                                    \
            ph_set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_)); \
            return PH_ELAUNCH;                                                     \
        }                                                                          \
    } while (0)

// run-or-return for host code that chains other entry points of this library (the native plans' launch sequences)
#define PH_RUN(call)                   \
    do {                               \
        const int rc_ = (call);        \
        if (rc_ != PH_OK) return rc_;  \
    } while (0)

// the pieces of a caller-owned workspace or pack start at 256-byte boundaries
static inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// a cfg's mode (PH_MODE_*) -> the grade of the KernelHead / neck / FPN kernels (engine.KHEAD_PREC); -1: no such mode
static inline int ph_mode_grade(int mode) {
    switch (mode) {
        case PH_MODE_FP16: return PH_PREC_F16;
        case PH_MODE_BF16: return PH_PREC_BF16;
        case PH_MODE_FP32: case PH_MODE_MIXED: case PH_MODE_MIXED16: return PH_PREC_SPLIT;
        default: return -1;
    }
}

// the FPN's top-down size rule: a level is 2 n or 2 n - 1 of the coarser one's n (the sizes at which the integer nearest index is torch's)
static inline bool ph_fpn_size_rule(int fine, int coarse) { return fine == 2 * coarse || fine == 2 * coarse - 1; }

// every buffer check of a native plan's create / run call, in this order: pack alignment (pack_or_null: none to check), workspace
// NULL, workspace size (PH_EWORKSPACE), workspace alignment; the messages carry the public function's name (ph_api.hip)
int ph_check_buffers(const char* fn, const void* pack_or_null, const void* workspace, size_t workspace_bytes, size_t need);

// compute units of the current device, asked once per process (the first device's answer stays); 0 when the query fails
int ph_num_cus();

// ---- the weight packs of the native KernelHead / neck / association plans: one kernel (ph_wpack.hip) writes a pack from a table of
// its pieces.  A piece is a run of 16-byte units of one kind; what lies between its data and the next piece is padding (zeros).
enum {
    PH_PIECE_PLANES = 0,     // 16-bit [P][nmat][rows][K] as stored; rows at or above rows_valid are zero
    PH_PIECE_FRAG32 = 1,     // 16-bit [P][nmat] x pack.pack_b32 fragments of W2 [rows][K]; rows_valid likewise
    PH_PIECE_FRAG16 = 2,     // 16-bit [P] x pack.pack_b_fragments fragments of W2 [rows][K]
    PH_PIECE_F32 = 3,        // fp32 copy of parameter `first`
    PH_PIECE_GN = 4,         // fp32 [3][2][256]: (gamma, beta) of three convs, parameters first + 3 m + 1, + 2
    PH_PIECE_BIAS = 5        // fp32 parameter `first`, zero at or beyond entry rows_valid
};
struct PhPackPiece {
    uint32_t u0;             // first unit of the piece (ascending over the pieces)
    uint32_t nvalid;         // units that carry data; the rest up to the next piece is padding
    uint32_t rows, K;        // 16-bit kinds: W2 is [rows][K] (rows as padded in the pack)
    uint32_t rows_valid;
    uint8_t kind, first, pstep, nmat;   // first parameter; 16-bit kinds: distance between the matrices' parameters, matrices per plane
    uint8_t taps;            // 16-bit kinds: > 0: K = taps * 256 of a parameter stored [row][256][taps]; 0: the parameter is [row][K]
};
enum { PH_PACK_MAX_PARAMS = 30, PH_PACK_MAX_PIECES = 32 };
struct PhPackTable {
    const float* p[PH_PACK_MAX_PARAMS];
    PhPackPiece pc[PH_PACK_MAX_PIECES];
    uint32_t total_u;        // units of the whole pack
    int32_t npieces;
    int32_t f16;             // 16-bit values are fp16 (one plane); else bf16 hi (+ lo) planes
};
static_assert(sizeof(PhPackTable) <= 2048, "the pack table travels as a kernel argument");
static_assert(PH_KHEAD_NPARAMS <= PH_PACK_MAX_PARAMS && PH_NECK_NPARAMS <= PH_PACK_MAX_PARAMS && 3 * PH_TRACK_MAX_CONVS + 4 <= PH_PACK_MAX_PARAMS &&
              PH_FPN_NPARAMS <= PH_PACK_MAX_PARAMS && PH_FPACK_COUNT <= PH_PACK_MAX_PIECES &&
              PH_KPACK_COUNT <= PH_PACK_MAX_PIECES && PH_NPACK_COUNT <= PH_PACK_MAX_PIECES && PH_TPACK_COUNT <= PH_PACK_MAX_PIECES,
              "include/polyhead.h: a pack's parameters and pieces fit the table");
// piece `i` of a pack layout (include/polyhead.h: offset[] / bytes[] of the pieces) into the table
static inline void ph_pack_piece(PhPackTable& t, const uint64_t* offset, const uint64_t* bytes, int i, int kind, int first, int taps = 0,
                                 uint32_t rows = 0, uint32_t K = 0, uint32_t rows_valid = 0, int nmat = 1, int pstep = 0) {
    t.pc[i] = PhPackPiece{(uint32_t)(offset[i] / 16), (uint32_t)(bytes[i] / 16), rows, K, rows_valid,
                          (uint8_t)kind, (uint8_t)first, (uint8_t)pstep, (uint8_t)nmat, (uint8_t)taps};
}
// launches the packer on `stream` with at most `max_blocks` workgroups; `fn`: the public entry point, for the message
int ph_pack_pieces(const char* fn, const PhPackTable& t, void* pack, unsigned max_blocks, void* stream);

// ---- the hard mask threshold (kernel_update_head.py:236-238, kernel_head.py:314-317): `sigmoid(z) > 0.5` in fp32.
// Evaluated as the reference does -- 1 / (1 + exp(-z)), every operation rounded to fp32 -- the comparison is true exactly
// for z > 1.5 * 2^-24: below that 1 - z rounds to 1 - 2^-24 or 1, 2 - 2^-24 rounds to 2, and 1 / 2 = 0.5.  (Probe on
// torch's CPU sigmoid: smallest z with sigmoid(z) > 0.5 is 97 * 2^-30.)  `z > 0` would differ on 0 < z <= 1.5 * 2^-24:
// 3.6e-8 of N(0, 1) logits, i.e. about one pixel in four full-size frames -- enough to move a pooled feature by 1e-3.
#define PH_BIN_THR 0x1.8p-24f

// ---- launch knobs of the decode kernels.  The public entry points (ph_dynconv, ph_dynconv_up2[_wgs], ph_query_stage[_counts])
// fill them, by value and once per call, from the library's switch table (ph_api.hip, include/polyhead.h PH_SWITCH_*: read from
// the environment once at first use, set by ph_set_switch after that) and call the *_k forms below; the native decode
// plan (ph_decode.hip) passes the defaults explicitly and so consults neither.  KernelHead's post-neck kernels (ph_khead.hip,
// ph_khead1.hip) have no knobs: their public entry points are what the native plans call.
int ph_switch(int id);           // the current value of switch PH_SWITCH_<id>
struct PhConvKnobs {
    int wgs = 0;                 // PH_SWITCH_CONV_WGS: workgroups (0 = one per CU)
};
struct PhUp2Knobs {
    int wgs = 0;                 // PH_SWITCH_UP2_WGS: overrides the caller's workgroup count (0 = keep it)
};
struct PhQueryKnobs {
    int nrt = 0;                             // PH_SWITCH_QUERY_NRT: row blocks per workgroup (0 = the launch's own choice)
    unsigned long long* timeline = nullptr;  // PH_SWITCH_QUERY_TIMELINE: phase times of one workgroup (debug; synchronises)
};
int ph_dynconv_k(const PhConvKnobs& kn, const uint16_t* planes, const uint16_t* kern, int64_t kern_plane_stride,
                 int64_t kern_batch_stride, const float* kbias, int64_t kbias_batch_stride, uint32_t* bits_out, void* logits_out,
                 int out_dtype, int64_t out_batch_stride, int B, int N, int64_t HW, int prec, void* stream);
int ph_dynconv_up2_k(const PhUp2Knobs& kn, const uint16_t* planes, const uint16_t* kern, int64_t kern_batch_stride, const float* kbias,
                     int64_t kbias_batch_stride, void* logits_out, void* up_out, int out_dtype, int B, int N, int H, int W, int prec,
                     int workgroups, void* stream);
int ph_query_stage_counts_k(const PhQueryKnobs& kn, const float* partial, int nsplit, const uint32_t* bits, const int32_t* pcount,
                            const float* k_in, const float* q_in, const uint16_t* wb, const float* wf, const ph_stage_layout* layout,
                            float* obj, float* dobj, float* cls, int cls_sigmoid, uint16_t* kern, float* kbias, void* workspace,
                            size_t workspace_bytes, int B, int N, int64_t HW, int prec, int kern_format, int phases, void* stream);

// launch knobs of the neck's kernels (ph_neck.hip), in the same way: the public ph_conv_nhwc / ph_gn_sum_planes /
// ph_gn_apply fill them from the switch table; the native neck and FPN plans (ph_neckplan.hip, ph_fpnplan.hip) pass the
// defaults.  0 = the built-in rule
struct PhNeckKnobs {
    int conv_th = 0;             // PH_SWITCH_CONV_TILE_ROWS: forced output rows per conv tile (2 or 4; one-plane grades)
    int gnsum_wgs = 0;           // PH_SWITCH_GNSUM_WGS: workgroups per frame of ph_gn_sum_planes
    int cplanes_tpw = 0;         // PH_SWITCH_CPLANES_TPW: 64-pixel tiles per workgroup of ph_gn_apply's PH_GN_TO_CPLANES mode
};
// rows per tile of a ph_conv_nhwc launch of this output size, grade and batch (2 or 4)
int ph_conv_nhwc_tile_rows_k(const PhNeckKnobs& kn, int Ho, int Wo, int prec, int B);
int ph_conv_nhwc_k(const PhNeckKnobs& kn, const uint16_t* X, const uint16_t* Wp, int64_t w_plane_elems, float* Y, float* partial,
                   int ksize, int stride, int B, int H, int W, int prec, void* stream);
int ph_gn_sum_planes_k(const PhNeckKnobs& kn, const float* const* ys, const float* const* stats, const float* const* gammas,
                       const float* const* betas, int nlev, int groups, uint16_t* planes, int B, int64_t HW, int prec, void* stream);
int ph_gn_apply_k(const PhNeckKnobs& kn, const float* y, const float* stats, const float* gamma, const float* beta, int groups, int mode,
                  int accumulate, uint16_t* planes, float* outf, int B, int H, int W, int prec, void* stream);

// the map x map^T product of the training path (ph_train.hip) under its public names: ph_map_x_map_t_ex (wide = 0: K <= 256) and
// ph_map_x_map_t_wide (ph_fpntrain.hip; wide != 0: K <= 4096 in tiles of 256 columns); row passes of M rows per image and split
int ph_map_x_map_t_k(const char* fn, int wide, const float* G, const float* X, float* partial, float* out, int B, int M, int K, int64_t HW,
                     int nsplit, int binarize_g, float* rs_partial, float* rowsum, int sum_batch, void* stream);
int ph_map_x_map_t_passes(int M);

// device-count forms of the association step's kernels (ph_track.hip) for the native association plan (ph_assocplan.hip): B frames per
// launch, the grids sized for `cap` RoIs per frame, every workgroup reading its frame's count from the things tables on the device
// (int32 [B][words], word 0 = the count, words 1 .. cap = the segment ids) and returning when it lies beyond it.  The public entry
// points are the same kernels without the count.
struct PhThings { const int32_t* tab = nullptr; int words = 0; int cap = 0; };
void ph_gemm_split(int M, int N, int K, int& S, int& steps);      // ph_gemm_rows_splitk's split of (M, N, K)
int ph_segment_boxes_b(const char* fn, const int32_t* pan, int B, int H, int W, int nseg, float* rois, float* ext_boxes, void* workspace,
                       size_t workspace_bytes, void* stream);
int ph_roi_align_fpn_cnt(const float* const* feats, const int32_t* hw, const float* scales, const int64_t* frame_strides, int nlev,
                         const float* rois, int nseg, PhThings th, int B, float finest_scale, uint16_t* out_cl, int prec, void* stream);
int ph_gemm_rows_splitk_cnt(const uint16_t* X, int im2col7, const uint16_t* Wp, int64_t w_plane_elems, const float* bias, int relu, float* Yf,
                            uint16_t* Yp, int M, int N, int K, int prec, PhThings th, int rows_per, int B, void* workspace, void* stream);
int ph_gn_relu_cl_cnt(const float* y, const float* gamma, const float* beta, int groups, float eps, uint16_t* out, PhThings th, int B,
                      int prec, void* stream);

// device-count form of ph_track_affinity (ph_track.hip) for the device tracker (ph_dtracker.hip): grids sized for (max_n, max_m), every
// workgroup reading cnt = (n, m, need) on the device -- need == 0: nothing runs.  workspace: ph_track_affinity_workspace_bytes(max_n,
// max_m).  Launches only; the caller checks the launch.  `streams` trackers side by side: every pointer (cnt and workspace included)
// is stream 0's and stream s's lies s * stride_bytes behind it; one more grid dimension of size `streams`; `active` (nullable, int32
// [streams]): a zero word's workgroups return before they read anything of their stream.
void ph_track_affinity_cnt(const float* emb, const int32_t* labels, const float* memo_emb, const int32_t* memo_labels, int max_n, int max_m,
                           const int32_t* cnt, int metric, int with_cats, float* score, void* workspace, int streams, size_t stride_bytes,
                           const int32_t* active, void* stream);
// the device tracker's per-frame outputs inside its own buffer, for ph_assoc_plan_track (one frame at a time) and
// ph_assoc_plan_track_streams (one frame per stream): kept [max_dets], ids [max_dets], kept_count [1] of stream 0; stream s's lie
// s * the strides (elements) behind them
struct PhDtrkScratch {
    int32_t* kept = nullptr; int64_t* ids = nullptr; int32_t* kept_count = nullptr; int max_dets = 0;
    int streams = 1; int64_t kept_stride = 0, ids_stride = 0, kc_stride = 0;
};
PhDtrkScratch ph_dtracker_scratch(const ph_dtracker* t);
// ph_dtracker_step with these pieces as its outputs; `in`: the input pointers and strides of a ph_dtracker_io (checked by the caller)
int ph_dtracker_step_scratch(ph_dtracker* t, const ph_dtracker_io* in, const int32_t* active, void* stream);

// ---- bf16 bit helpers (round to nearest even; inputs are finite in this code base) ----------
// gfx950 has a hardware round-to-nearest-even conversion (v_cvt_pk_bf16_f32); the compiler selects
// it for fp32 -> __bf16 conversions.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t f2bf(float x) { return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)x); }
// two conversions in one instruction: low half = a, high half = b
__device__ __forceinline__ uint32_t f2bf_pk(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{a, b}, bf16x2_t));
}
__device__ __forceinline__ float bf2f(uint32_t h) { return __uint_as_float(h << 16); }
// x ~= hi + lo, |x - hi - lo| <= 2^-17 |x|
__device__ __forceinline__ void f2bf_split(float x, uint32_t& hi, uint32_t& lo) {
    hi = f2bf(x);
    lo = f2bf(x - bf2f(hi));
}
__device__ __forceinline__ uint32_t pack2(uint32_t a, uint32_t b) { return a | (b << 16); }

// ---- 16-bit element formats of feature planes / dynamic kernels / outputs: bf16 (8-bit mantissa, fp32 range) or IEEE
// fp16 (11-bit mantissa, |x| < 65504).  A bf16 value is exactly representable in fp16 when it is inside fp16's normal
// range, so an fp16 plane carries bf16-rounded inputs unchanged and fp32 inputs with 8x finer rounding.
enum { PH_E_BF16 = 0, PH_E_F16 = 1, PH_E_F16_FROM_BF16 = 2 /* conv only: bf16 feature tile converted to fp16 in LDS */ };
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t f2h(float x) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x); }
__device__ __forceinline__ float h2f(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
__device__ __forceinline__ uint32_t f2h_pk(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{a, b}, f16x2_t));
}
template <int E> __device__ __forceinline__ uint32_t f2e(float x) { return E == PH_E_F16 ? f2h(x) : f2bf(x); }
template <int E> __device__ __forceinline__ float e2f(uint32_t h) { return E == PH_E_F16 ? h2f(h) : bf2f(h); }
// x -> (hi, lo) planes of format E: bf16 hi + lo (lo unused by one-plane callers), or ONE fp16 value (lo = 0)
template <int E> __device__ __forceinline__ void f2e_split(float x, uint32_t& hi, uint32_t& lo) {
    if constexpr (E == PH_E_F16) { hi = f2h(x); lo = 0; }
    else f2bf_split(x, hi, lo);
}
template <int E> __device__ __forceinline__ uint32_t f2e_pk(float a, float b) { return E == PH_E_F16 ? f2h_pk(a, b) : f2bf_pk(a, b); }

// ---- streaming (non-temporal) 16-byte accesses for data that is written or read exactly once per kernel: the x2
// upsample's 965 MB of output per launch went from 5.4 to 6.9 TB/s with them (stores no longer allocate in L2 / MALL)
// cache policy of the LDS-DMA feature streams (aux operand of global_load_lds on gfx950: 1 = sc0, 2 = nt, 16 = sc1):
// nt | sc1 measured pool 197 -> 181 us, dynconv bits 102 -> 94 us against the default policy; sc1 alone is slower
#ifndef PH_CPOL_STREAM      // -DPH_CPOL_STREAM=0: default policy (tools/mall_probe.py)
#define PH_CPOL_STREAM 18
#endif
typedef unsigned ph_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_nt16(void* p, uint4 v) { __builtin_nontemporal_store(ph_u32x4{v.x, v.y, v.z, v.w}, (ph_u32x4*)p); }
__device__ __forceinline__ void st_nt16(void* p, float4 v) {
    __builtin_nontemporal_store(ph_u32x4{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}, (ph_u32x4*)p);
}
typedef unsigned ph_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 ld_nt8(const void* p) {
    const ph_u32x2 v = __builtin_nontemporal_load((const ph_u32x2*)p);
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint4 ld_nt16(const void* p) {
    const ph_u32x4 v = __builtin_nontemporal_load((const ph_u32x4*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// ---- MFMA wrappers.  Fragment maps (verified on hardware by ph_selftest_*):
//  16x16x32: A lane l: row l&15, k = (l>>4)*8 + e;  B lane l: col l&15, k = (l>>4)*8 + e;
//            D lane l, reg r: row (l>>4)*4 + r, col l&15.
//  32x32x16: A lane l: row l&31, k = (l>>5)*8 + e;  B lane l: col l&31, k = (l>>5)*8 + e;
//            D lane l, reg r: row (r&3) + 8*(r>>2) + 4*(l>>5), col l&31.
__device__ __forceinline__ f32x4_t mfma16(uint4 a, uint4 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                   __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16_t mfma32(uint4 a, uint4 b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                   __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// two bf16 in a dword -> two fp16 (exact whenever the value is inside fp16's normal range; bf16 has 8 significand bits)
__device__ __forceinline__ uint32_t bf2h_pk(uint32_t w) { return f2h_pk(__uint_as_float(w << 16), __uint_as_float(w & 0xFFFF0000u)); }
__device__ __forceinline__ uint4 bf2h_x8(uint4 v) { return make_uint4(bf2h_pk(v.x), bf2h_pk(v.y), bf2h_pk(v.z), bf2h_pk(v.w)); }

template <int E> __device__ __forceinline__ f32x4_t mfma16e(uint4 a, uint4 b, f32x4_t c) {
    if constexpr (E == PH_E_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    else
        return mfma16(a, b, c);
}
template <int E> __device__ __forceinline__ f32x16_t mfma32e(uint4 a, uint4 b, f32x16_t c) {
    if constexpr (E == PH_E_F16 || E == PH_E_F16_FROM_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    else
        return mfma32(a, b, c);
}

// Transposing LDS read: within each 16-lane group the lanes point at 16 8-byte chunks forming a
// [4 rows][16 cols] bf16 block (lane i -> row i>>2, cols (i&3)*4..+3); lane i receives column i,
// i.e. element j = block[j][i].
__device__ __forceinline__ uint2 lds_read_tr16(const uint16_t* p) {
    bf16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((PH_LDS bf16x4_t*)(p));
    return __builtin_bit_cast(uint2, v);
}

// 16-lane butterflies on the DPP crossbar (no LDS traffic): quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror.  Every lane of a 16-lane row ends with the same value, and the pairing
// (hence the fp result) is that of an xor-1/2/4/8 butterfly.
template <int CTRL> __device__ __forceinline__ float dpp_mov(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_group16_sum(float t) {
    t += dpp_mov<0xB1>(t);
    t += dpp_mov<0x4E>(t);
    t += dpp_mov<0x141>(t);
    t += dpp_mov<0x140>(t);
    return t;
}
__device__ __forceinline__ float wave_group16_max(float t) {
    t = fmaxf(t, dpp_mov<0xB1>(t));
    t = fmaxf(t, dpp_mov<0x4E>(t));
    t = fmaxf(t, dpp_mov<0x141>(t));
    t = fmaxf(t, dpp_mov<0x140>(t));
    return t;
}
// 1 ulp hardware transcendentals (v_exp_f32 / v_rcp_f32 / v_rsq_f32): ~2e-7 relative, far inside both
// precision modes' budgets, and an order of magnitude fewer VALU slots than the IEEE-exact library forms.
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fast_sigmoid(float x) { return fast_rcp(1.f + fast_exp(-x)); }
