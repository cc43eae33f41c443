// ph_image_prepare: the loader's image work on the device (include/polyhead.h) -- bilinear resize on uint8, horizontal flip, crop,
// normalise, zero pad and the transpose to CHW of the reference's train_pipeline (configs/_base_/datasets/cityscapes_dvps.py:8-21:
// SeqResizeWithDepth, SeqFlipWithDepth, SeqRandomCropWithDepth, SeqNormalizeWithDepth, SeqPadWithDepth, SeqDefaultFormatBundle) and the
// Normalize + Pad + ImageToTensor of its test_pipeline (:23-41), in one launch.  Resize, flip and crop are separable two-tap gathers,
// so they travel as one table per axis and frame; the kernel takes no position on how the taps were chosen.
//
//   k_image_prepare   grid (row pieces, frames).  A WAVE owns 512 adjacent columns of one row of the PADDED output, so the row's tab_y
//                     entry, the two source row bases and the vertical weights are wave-uniform (scalar loads).  A lane owns 8 of the
//                     columns, in groups of one 16-byte store (4 fp32, 8 bf16) that lie 64 groups apart, so that every store
//                     instruction of the wave covers one contiguous kilobyte of a plane.
//                       gather: the 8 tab_x word pairs first, then the source bytes, all issued before the first is used.  Where the
//                     two taps are neighbours (i1 = i0 + 1, every interior column of a resize) or the second has weight zero, the six
//                     bytes of both pixels come in ONE unaligned 8-byte load per source row; a row of weight zero is not loaded at all
//                     (identity tables: one load per pixel).  Any other pair of taps, and the last two bytes of the call's images
//                     (an 8-byte load would pass their end), take byte loads.
//                       arithmetic: OpenCV's 8-bit fixed-point formula, then (v - mean) * stdinv in fp32.
//                       stores: NCHW 16-byte stores per channel plane.  NHWC: the wave's run of 512 x 3 elements is put
//                     together in LDS and leaves as 16-byte stores that are contiguous from lane to lane (a lane's own run
//                     is 48 or 96 bytes long: stored directly, every instruction would touch a sixth or a third of each line).  Element
//                     stores where Wp or the output pointer do not allow 16-byte ones.
// Per pixel 12 bytes are written (fp32) against at most 12 bytes gathered from a source that fits the caches.
#include <cmath>
#include <type_traits>

#include "ph_common.h"

namespace {

constexpr int IP_T = 256;                  // threads per workgroup: four waves, four row pieces
constexpr int IP_PX = 8;                   // output columns per lane
constexpr int IP_WAVE_PX = 64 * IP_PX;     // output columns per wave

struct IpNorm {
    float mean[3], stdinv[3];
};

// one table word pair -> the two indices and weights; false: the entry is none (-1) or names a row / column outside the file
__device__ __forceinline__ bool ip_taps(int2 t, int limit, int& i0, int& i1, int& w0, int& w1) {
    i0 = t.x & 0xFFFF;
    i1 = (t.x >> 16) & 0xFFFF;
    w0 = t.y & 0xFFFF;
    w1 = (t.y >> 16) & 0xFFFF;
    return t.x >= 0 && i0 < limit && i1 < limit;
}

// eight bytes from any address: one global_load_dwordx2 (the target runs in unaligned access mode)
__device__ __forceinline__ uint2 ip_ld8(const uint8_t* p) {
    uint2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
// byte k (0 .. 5, a constant after unrolling) of such a load: the three channels of the first pixel, then of its right neighbour
__device__ __forceinline__ int ip_byte(uint2 q, int k) { return (int)(((k < 4 ? q.x >> (8 * k) : q.y >> (8 * (k - 4)))) & 255u); }

// plain stores: the streaming form measured the same (59.6 against 59.8 us at four 1024 x 2048 frames), and the backbone reads the
// output next
__device__ __forceinline__ void ip_st16(void* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }

// BF16: bf16 output (round to nearest even), else fp32.  NHWC: [frames][Hp][Wp][3], else [frames][3][Hp][Wp].
// VEC: Wp is a multiple of 16 bytes of elements and the output base 16-byte aligned, so every 16-byte piece of a row is aligned
template <bool BF16, bool NHWC, bool VEC>
__global__ __launch_bounds__(IP_T) void k_image_prepare(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ raw_end,
                                                         const int2* __restrict__ tab_y, const int2* __restrict__ tab_x, IpNorm nm, int to_rgb,
                                                         int Hs, int Ws, int Hc, int Wc, int Hp, int Wp, int npiece, void* __restrict__ out) {
#pragma clang fp contract(off)
    using E = typename std::conditional<BF16, uint16_t, float>::type;
    constexpr int U = 16 / (int)sizeof(E);                           // columns per group: one 16-byte store of a plane
    constexpr int G = IP_PX / U;                                     // groups per lane
    constexpr int VPW = IP_WAVE_PX * 3 / U;                          // 16-byte vectors of a wave's NHWC run
    constexpr bool STAGE = NHWC && VEC;
    __shared__ uint4 stage[STAGE ? (IP_T / 64) * VPW : 1];

    const int f = blockIdx.y, lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int item = (int)blockIdx.x * (IP_T / 64) + wave;
    const bool live = item < Hp * npiece;                            // wave-uniform; nobody returns early: the NHWC form has a barrier
    const int y = live ? item / npiece : 0;
    const int px0 = live ? (item - y * npiece) * IP_WAVE_PX : 0;     // the first column of the wave's piece
    // column u of the lane's group g
    auto col_of = [&](int g, int u) { return px0 + (g * 64 + lane) * U + u; };

    int y0 = 0, y1 = 0, b0 = 0, b1 = 0;
    bool row_in = false;
    if (live && y < Hc) row_in = ip_taps(tab_y[(int64_t)f * Hc + y], Hs, y0, y1, b0, b1);
    const int64_t row_bytes = (int64_t)Ws * 3;
    const uint8_t* __restrict__ r0 = raw + ((int64_t)f * Hs + y0) * row_bytes;
    const uint8_t* __restrict__ r1 = raw + ((int64_t)f * Hs + y1) * row_bytes;

    // the taps of the lane's columns; a column beyond Wc reads the last entry and is masked
    int2 t[IP_PX];
#pragma unroll
    for (int j = 0; j < IP_PX; ++j) t[j] = tab_x[(int64_t)f * Wc + min(col_of(j / U, j % U), Wc - 1)];

    int x0[IP_PX], x1[IP_PX], a0[IP_PX], a1[IP_PX];
    bool ok[IP_PX], fast[IP_PX];
    bool slow = false;                                               // a column of this lane needs byte loads
#pragma unroll
    for (int j = 0; j < IP_PX; ++j) {
        ok[j] = ip_taps(t[j], Ws, x0[j], x1[j], a0[j], a1[j]) && row_in && col_of(j / U, j % U) < Wc;
        fast[j] = ok[j] && (a1[j] == 0 || x1[j] == x0[j] + 1) && r0 + x0[j] * 3 + 8 <= raw_end && r1 + x0[j] * 3 + 8 <= raw_end;
        slow = slow || (ok[j] && !fast[j]);
    }
    // the gathers, one masked load a column and row; a row of weight zero (wave-uniform) adds nothing whatever it holds and is not loaded
    uint2 q0[IP_PX], q1[IP_PX];
#pragma unroll
    for (int j = 0; j < IP_PX; ++j) {
        q0[j] = q1[j] = make_uint2(0u, 0u);
        if (fast[j]) q0[j] = ip_ld8(r0 + x0[j] * 3);
    }
    if (b1) {
#pragma unroll
        for (int j = 0; j < IP_PX; ++j)
            if (fast[j]) q1[j] = ip_ld8(r1 + x0[j] * 3);
    }

    // every multiplication has factors below 2^24 (a byte x a weight of 16 bits; a weight x 21 bits): v_mul_u32_u24 / v_mad_u32_u24.
    // Straight-line for every lane; a column that is pad or takes byte loads computes on zeros here
    int val[IP_PX][3];                                               // by the FILE's channel
#pragma unroll
    for (int j = 0; j < IP_PX; ++j)
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const int h0 = __mul24(ip_byte(q0[j], ci), a0[j]) + __mul24(ip_byte(q0[j], 3 + ci), a1[j]);
            const int h1 = __mul24(ip_byte(q1[j], ci), a0[j]) + __mul24(ip_byte(q1[j], 3 + ci), a1[j]);
            val[j][ci] = ((__mul24(b0, h0 >> 4) >> 16) + (__mul24(b1, h1 >> 4) >> 16) + 2) >> 2;
        }
    if (slow) {                                                      // skipped by the whole wave where no lane needs it: every resize's tables
#pragma unroll
        for (int j = 0; j < IP_PX; ++j)
            if (ok[j] && !fast[j]) {
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const int o0 = x0[j] * 3 + ci, o1 = x1[j] * 3 + ci;
                    const int h0 = (int)r0[o0] * a0[j] + (int)r0[o1] * a1[j];
                    const int h1 = (int)r1[o0] * a0[j] + (int)r1[o1] * a1[j];
                    val[j][ci] = ((__mul24(b0, h0 >> 4) >> 16) + (__mul24(b1, h1 >> 4) >> 16) + 2) >> 2;
                }
            }
    }
    float v[3][IP_PX];
#pragma unroll
    for (int j = 0; j < IP_PX; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // mmcv.imnormalize: the colour conversion first, then mean / std per OUTPUT channel.  The pad is zero in normalised units:
            // the reference pads after Normalize
            const int vc = to_rgb ? val[j][2 - c] : val[j][c];
            v[c][j] = ok[j] ? ((float)vc - nm.mean[c]) * nm.stdinv[c] : 0.f;
        }

    E* __restrict__ o = static_cast<E*>(out);
    const int64_t plane = (int64_t)Hp * Wp;
    if constexpr (!VEC) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < IP_PX; ++j) {
                const int x = col_of(j / U, j % U);
                if (!live || x >= Wp) continue;
                const int64_t at = NHWC ? (((int64_t)f * Hp + y) * Wp + x) * 3 + c : ((int64_t)f * 3 + c) * plane + (int64_t)y * Wp + x;
                if constexpr (BF16) o[at] = (uint16_t)f2bf(v[c][j]);
                else o[at] = v[c][j];
            }
    } else if constexpr (!NHWC) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int x = col_of(g, 0);                          // Wp is a multiple of U: a group is inside the row or outside it
                if (!live || x >= Wp) continue;
                uint4 w;
                if constexpr (BF16) w = make_uint4(f2bf_pk(v[c][0], v[c][1]), f2bf_pk(v[c][2], v[c][3]), f2bf_pk(v[c][4], v[c][5]), f2bf_pk(v[c][6], v[c][7]));
                else w = make_uint4(__float_as_uint(v[c][4 * g]), __float_as_uint(v[c][4 * g + 1]), __float_as_uint(v[c][4 * g + 2]),
                                    __float_as_uint(v[c][4 * g + 3]));
                ip_st16(o + ((int64_t)f * 3 + c) * plane + (int64_t)y * Wp + x, w);
            }
    } else {
        // the group's U columns x 3 channels in memory order, three vectors at (g * 64 + lane) * 3 of the wave's run
        uint4* __restrict__ mine = stage + wave * VPW;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            uint32_t w[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                if constexpr (BF16) {
                    const int e0 = 2 * k, e1 = 2 * k + 1;
                    w[k] = f2bf_pk(v[e0 % 3][g * U + e0 / 3], v[e1 % 3][g * U + e1 / 3]);
                } else {
                    w[k] = __float_as_uint(v[k % 3][g * U + k / 3]);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) mine[(g * 64 + lane) * 3 + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        }
        __syncthreads();
        const int nvec = live ? max(0, min(IP_WAVE_PX, Wp - px0)) * 3 / U : 0;
        E* __restrict__ p = o + (((int64_t)f * Hp + y) * Wp + px0) * 3;
#pragma unroll
        for (int k = 0; k < VPW / 64; ++k) {
            const int m = k * 64 + lane;
            if (m < nvec) ip_st16(p + (int64_t)m * U, mine[m]);
        }
    }
}

// every word of one axis' host tables: an index pair inside the file or -1, weights of 0 .. 2048
int ip_check_table(const int32_t* tab, int frames, int n, int limit, const char* name, const char* what) {
    for (int b = 0; b < frames; ++b)
        for (int i = 0; i < n; ++i) {
            const int32_t w0 = tab[((size_t)b * n + i) * 2], w1 = tab[((size_t)b * n + i) * 2 + 1];
            if (w0 == -1) continue;
            const int i0 = w0 & 0xFFFF, i1 = (w0 >> 16) & 0xFFFF;
            if (w0 < 0 || i0 >= limit || i1 >= limit) {
                ph_set_error("ph_image_prepare: %s[%d][%d] names %s %d and %d (word 0x%08x); a file %s is 0 .. %d, the word -1 means none", name,
                             b, i, what, i0, i1, (unsigned)w0, what, limit - 1);
                return PH_EINVAL;
            }
            const int a0 = w1 & 0xFFFF, a1 = (w1 >> 16) & 0xFFFF;
            if (w1 < 0 || a0 > 2048 || a1 > 2048) {
                ph_set_error("ph_image_prepare: %s[%d][%d] has the weights %d and %d (word 0x%08x); a tap weight is 0 .. 2048", name, b, i, a0,
                             a1, (unsigned)w1);
                return PH_EINVAL;
            }
        }
    return PH_OK;
}

}  // namespace

extern "C" int ph_image_prepare(const uint8_t* raw, int frames, int Hs, int Ws, const int32_t* tab_y_host, const int32_t* tab_x_host,
                                const int32_t* tab_y, const int32_t* tab_x, int Hc, int Wc, int Hp, int Wp, const float* mean,
                                const float* stdinv, int to_rgb, int out_dtype, int layout, void* out, void* stream) {
    PH_CHECK_ARG(raw && tab_y_host && tab_x_host && tab_y && tab_x && mean && stdinv && out, "null argument");
    PH_CHECK_ARG(frames >= 1 && frames <= PH_IMGPREP_MAX_FRAMES, "1 .. 64 frames per call");
    PH_CHECK_ARG(Hs >= 1 && Ws >= 1, "image sizes of at least 1");
    if (Hs > 32767 || Ws > 32767) {
        ph_set_error("ph_image_prepare: a file of %d x %d; a table word holds two indices of 15 bits, so Hs, Ws <= 32767", Hs, Ws);
        return PH_EUNSUPPORTED;
    }
    PH_CHECK_ARG(Hc >= 1 && Wc >= 1 && Hp >= Hc && Wp >= Wc && Hp <= 65536 && Wp <= 65536, "1 <= Hc <= Hp <= 65536 and 1 <= Wc <= Wp <= 65536");
    PH_CHECK_ARG(out_dtype == PH_OUT_F32 || out_dtype == PH_OUT_BF16, "out_dtype is PH_OUT_F32 or PH_OUT_BF16");
    PH_CHECK_ARG(layout == PH_IMG_NCHW || layout == PH_IMG_NHWC, "layout is PH_IMG_NCHW or PH_IMG_NHWC");
    PH_CHECK_ARG(to_rgb == 0 || to_rgb == 1, "to_rgb is 0 or 1");
    PH_CHECK_ARG(((uintptr_t)tab_y & 7) == 0 && ((uintptr_t)tab_x & 7) == 0, "tab_y and tab_x are pairs of int32, 8-byte aligned");
    const int esize = out_dtype == PH_OUT_BF16 ? 2 : 4;
    PH_CHECK_ARG(((uintptr_t)out & (esize - 1)) == 0, "the output is aligned to its element");
    IpNorm nm;
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(stdinv[c])) {
            ph_set_error("ph_image_prepare: mean[%d] = %g, stdinv[%d] = %g; both are finite", c, (double)mean[c], c, (double)stdinv[c]);
            return PH_EINVAL;
        }
        nm.mean[c] = mean[c];
        nm.stdinv[c] = stdinv[c];
    }
    PH_RUN(ip_check_table(tab_y_host, frames, Hc, Hs, "tab_y", "row"));
    PH_RUN(ip_check_table(tab_x_host, frames, Wc, Ws, "tab_x", "column"));

    const int npiece = (Wp + IP_WAVE_PX - 1) / IP_WAVE_PX;
    const dim3 grid((unsigned)(((int64_t)Hp * npiece + IP_T / 64 - 1) / (IP_T / 64)), frames), block(IP_T);
    const bool vec = Wp % (16 / esize) == 0 && ((uintptr_t)out & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const int2* ty = reinterpret_cast<const int2*>(tab_y);
    const int2* tx = reinterpret_cast<const int2*>(tab_x);
    const uint8_t* raw_end = raw + (size_t)frames * Hs * Ws * 3;      // an 8-byte gather stays below it
#define IP_LAUNCH(B, N, V) \
    hipLaunchKernelGGL((k_image_prepare<B, N, V>), grid, block, 0, st, raw, raw_end, ty, tx, nm, to_rgb, Hs, Ws, Hc, Wc, Hp, Wp, npiece, out)
#define IP_LAUNCH_V(B, N)         \
    do {                          \
        if (vec) IP_LAUNCH(B, N, true); \
        else IP_LAUNCH(B, N, false);    \
    } while (0)
    if (out_dtype == PH_OUT_BF16) {
        if (layout == PH_IMG_NHWC) IP_LAUNCH_V(true, true);
        else IP_LAUNCH_V(true, false);
    } else {
        if (layout == PH_IMG_NHWC) IP_LAUNCH_V(false, true);
        else IP_LAUNCH_V(false, false);
    }
#undef IP_LAUNCH_V
#undef IP_LAUNCH
    PH_CHECK_LAUNCH();
    return PH_OK;
}
