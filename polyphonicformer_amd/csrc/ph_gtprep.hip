// ph_gt_prepare: a training step's ground truth at the assign resolution from one segment-index map per frame (include/polyhead.h).
// Replaces, per frame, polyphonic_former_video.py:114-138 -- BitmapMasks.to_tensor (a [G][Hp][Wp] fp32 upload), F.pad, F.interpolate
// down by the assign stride, the four boolean-index splits, the nearest F.interpolate of the depth map -- and the passes losses.StepGT
// runs over their results (contiguous copy, hardened copy, valid map, zero-padded stack).
//
// The masks of a frame are disjoint, so the stack is one byte per source pixel, and an output pixel touches at most four rows of it.
// The pass is bound by its writes ((Gmax + Smax) planes per frame against one byte map), hence:
//   k_gtprep  grid (tiles of 256 threads over aH * ceil(aW / 4), frames): a thread owns four adjacent output columns of one output
//             row, resolves their 4 x 4 taps once (byte loads, the frame's 256-entry row table in LDS) and walks the rows of both
//             stacks storing 16 bytes a row; the rows no tap maps to get their zeros from the same loop, so no memset precedes the
//             launch.  The valid map is the OR of the values stored, the depth map one nearest load per column.
// No atomics, no workspace; every output word is written by exactly one thread.
#include "ph_common.h"

namespace {

constexpr int GP_T = 256;            // threads per workgroup = entries of the row table
constexpr int GP_C = 4;              // output columns per thread: one 16-byte store per row

struct GpSeg {
    int32_t n[PH_GTPREP_MAX_FRAMES];           // segments of the frame: table entries from n on read as dropped
};

// ATen's bilinear source index of a destination pixel (area_pixel_compute_source_index, align_corners = False), fp32, as
// ph_gtbox.hip has it; `in` is the padded size
__device__ __forceinline__ void gp_src(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    float r = scale * ((float)dst + 0.5f) - 0.5f;
    r = r < 0.f ? 0.f : r;
    i0 = (int)r;
    i0 = i0 > in - 1 ? in - 1 : i0;
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    l1 = r - (float)i0;
    l0 = 1.f - l1;
}

// ATen's nearest source index (nearest_neighbor_compute_source_index): min(floor(dst * scale), in - 1)
__device__ __forceinline__ int gp_near(float scale, int dst, int in) {
#pragma clang fp contract(off)
    const int i = (int)floorf((float)dst * scale);
    return i < in - 1 ? (i < 0 ? 0 : i) : in - 1;
}

template <bool VEC>
__device__ __forceinline__ void gp_store(float* __restrict__ p, const float (&v)[GP_C], int live) {
    if (VEC) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < GP_C; ++c)
            if (c < live) p[c] = v[c];
    }
}

// VEC: aW is a multiple of 4 and every output base is 16-byte aligned, so each thread's four columns are one aligned float4
template <bool VEC>
__global__ __launch_bounds__(GP_T) void k_gtprep(const uint8_t* __restrict__ seg, const int32_t* __restrict__ row_of,
                                                  const float* __restrict__ depth, GpSeg ns, int Hs, int Ws, int Hp, int Wp, int aH, int aW,
                                                  int Gmax, int Smax, int nearest, float scale_h, float scale_w, float* __restrict__ things,
                                                  float* __restrict__ stuff, float* __restrict__ things_hard, float* __restrict__ stuff_hard,
                                                  float* __restrict__ valid, float* __restrict__ depth_out) {
#pragma clang fp contract(off)
    __shared__ int16_t srow[256];
    const int f = blockIdx.y, t = threadIdx.x;
    {
        // 255 is "no segment"; an entry outside the two stacks is dropped like -1, so no table content reaches an address
        const int r = row_of[(int64_t)f * 256 + t];
        srow[t] = (int16_t)((t < ns.n[f] && t < 255 && r >= 0 && r < Gmax + Smax) ? r : -1);
    }
    __syncthreads();
    const int nx = (aW + GP_C - 1) / GP_C;
    const int idx = blockIdx.x * GP_T + t;
    if (idx >= aH * nx) return;
    const int y = idx / nx, x = (idx - y * nx) * GP_C;
    const int live = min(GP_C, aW - x);
    const uint8_t* __restrict__ sf = seg + (int64_t)f * Hs * Ws;

    int y0, y1;
    float h0, h1;
    if (nearest) {
        y0 = y1 = gp_near(scale_h, y, Hp);
        h0 = 1.f;
        h1 = 0.f;
    } else {
        gp_src(scale_h, y, Hp, y0, y1, h0, h1);
    }
    // the four taps of every column as output rows (-1: none) and the two horizontal weights
    int ra[GP_C], rb[GP_C], rc[GP_C], rd[GP_C];
    float w0[GP_C], w1[GP_C];
#pragma unroll
    for (int c = 0; c < GP_C; ++c) {
        const int X = x + (c < live ? c : 0);          // a dead column repeats the first one: in bounds, never stored
        int x0, x1;
        if (nearest) {
            x0 = x1 = gp_near(scale_w, X, Wp);
            w0[c] = 1.f;
            w1[c] = 0.f;
        } else {
            gp_src(scale_w, X, Wp, x0, x1, w0[c], w1[c]);
        }
        // the pad of :116-118: beyond the loader's size there is no segment
        const bool iy0 = y0 < Hs, iy1 = y1 < Hs, ix0 = x0 < Ws, ix1 = x1 < Ws;
        const int sa = iy0 && ix0 ? sf[(int64_t)y0 * Ws + x0] : 255;
        const int sb = iy0 && ix1 ? sf[(int64_t)y0 * Ws + x1] : 255;
        const int sc = iy1 && ix0 ? sf[(int64_t)y1 * Ws + x0] : 255;
        const int sd = iy1 && ix1 ? sf[(int64_t)y1 * Ws + x1] : 255;
        ra[c] = srow[sa];
        rb[c] = srow[sb];
        rc[c] = srow[sc];
        rd[c] = srow[sd];
    }

    const int64_t plane = (int64_t)aH * aW, pix = (int64_t)y * aW + x;
    bool any[GP_C] = {false, false, false, false};
    auto walk = [&](int first, int count, float* __restrict__ soft, float* __restrict__ hard) {
#pragma clang fp contract(off)
        float* __restrict__ ps = soft + ((int64_t)f * count) * plane + pix;
        float* __restrict__ ph = hard ? hard + ((int64_t)f * count) * plane + pix : nullptr;
        for (int r = 0; r < count; ++r) {
            const int row = first + r;
            float v[GP_C], hv[GP_C];
#pragma unroll
            for (int c = 0; c < GP_C; ++c) {
                const float a = ra[c] == row ? 1.f : 0.f, b = rb[c] == row ? 1.f : 0.f;
                const float cc = rc[c] == row ? 1.f : 0.f, d = rd[c] == row ? 1.f : 0.f;
                v[c] = h0 * (w0[c] * a + w1[c] * b) + h1 * (w0[c] * cc + w1[c] * d);
                hv[c] = v[c] != 0.f ? 1.f : 0.f;
                any[c] = any[c] || v[c] != 0.f;
            }
            gp_store<VEC>(ps + r * plane, v, live);
            if (ph) gp_store<VEC>(ph + r * plane, hv, live);
        }
    };
    walk(0, Gmax, things, things_hard);
    walk(Gmax, Smax, stuff, stuff_hard);

    float va[GP_C];
#pragma unroll
    for (int c = 0; c < GP_C; ++c) va[c] = any[c] ? 1.f : 0.f;
    gp_store<VEC>(valid + (int64_t)f * plane + pix, va, live);
    if (depth) {
        const float* __restrict__ dr = depth + ((int64_t)f * Hp + gp_near(scale_h, y, Hp)) * Wp;
        float dv[GP_C];
#pragma unroll
        for (int c = 0; c < GP_C; ++c) dv[c] = dr[gp_near(scale_w, x + (c < live ? c : 0), Wp)];
        gp_store<VEC>(depth_out + (int64_t)f * plane + pix, dv, live);
    }
}

}  // namespace

extern "C" int ph_gt_prepare(const uint8_t* seg, const int32_t* row_of, const int32_t* nseg, const float* depth, int frames, int Hs, int Ws,
                             int Hp, int Wp, int aH, int aW, int Gmax, int Smax, int mode, float* things, float* stuff, float* things_hard,
                             float* stuff_hard, float* valid, float* depth_out, void* stream) {
    PH_CHECK_ARG(seg && row_of && nseg && valid, "null argument");
    PH_CHECK_ARG(frames >= 1 && frames <= PH_GTPREP_MAX_FRAMES, "1 .. 64 frames per call");
    PH_CHECK_ARG(mode == PH_GTBOX_BILINEAR || mode == PH_GTBOX_NEAREST, "mode is PH_GTBOX_BILINEAR or PH_GTBOX_NEAREST");
    PH_CHECK_ARG(Hs >= 1 && Ws >= 1 && Hp >= 1 && Wp >= 1 && aH >= 1 && aW >= 1, "sizes must be positive");
    PH_CHECK_ARG(Hp <= 65536 && Wp <= 65536 && aH <= 65536 && aW <= 65536, "sizes of at most 65536");
    if (Hs > Hp || Ws > Wp) {
        ph_set_error("ph_gt_prepare: Hs <= Hp and Ws <= Wp (the padded size holds the loader's); got %d x %d in %d x %d", Hs, Ws, Hp, Wp);
        return PH_EINVAL;
    }
    if (Gmax < 0 || Smax < 0 || Gmax + Smax < 1 || Gmax > PH_ASSIGN_MAX || Smax > PH_ASSIGN_MAX) {
        ph_set_error("ph_gt_prepare: 0 .. %d rows per stack and at least one row; got Gmax %d, Smax %d", PH_ASSIGN_MAX, Gmax, Smax);
        return PH_EINVAL;
    }
    PH_CHECK_ARG((Gmax == 0 || things) && (Smax == 0 || stuff), "a stack with rows needs its output");
    PH_CHECK_ARG(!depth == !depth_out, "depth and depth_out come together");
    GpSeg ns;
    for (int b = 0; b < PH_GTPREP_MAX_FRAMES; ++b) ns.n[b] = 0;
    for (int b = 0; b < frames; ++b) {
        if (nseg[b] < 0 || nseg[b] > PH_GTPREP_MAX_SEGMENTS) {
            ph_set_error("ph_gt_prepare: 0 .. %d segments per frame (index 255 means none); frame %d has %d", PH_GTPREP_MAX_SEGMENTS, b,
                         nseg[b]);
            return PH_EINVAL;
        }
        ns.n[b] = nseg[b];
    }
    const float* outs[6] = {things, stuff, things_hard, stuff_hard, valid, depth_out};
    for (const float* p : outs) PH_CHECK_ARG(((uintptr_t)p & 3) == 0, "outputs are fp32");
    PH_CHECK_ARG(((uintptr_t)row_of & 3) == 0 && ((uintptr_t)depth & 3) == 0, "row_of is int32, depth fp32");
    bool vec = aW % GP_C == 0;
    for (const float* p : outs) vec = vec && ((uintptr_t)p & 15) == 0;
    const int nx = (aW + GP_C - 1) / GP_C;
    const int64_t tiles = ((int64_t)aH * nx + GP_T - 1) / GP_T;
    const float sh = (float)Hp / (float)aH, sw = (float)Wp / (float)aW;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, frames), block(GP_T);
    if (vec)
        hipLaunchKernelGGL(k_gtprep<true>, grid, block, 0, st, seg, row_of, depth, ns, Hs, Ws, Hp, Wp, aH, aW, Gmax, Smax,
                           mode == PH_GTBOX_NEAREST, sh, sw, things, stuff, things_hard, stuff_hard, valid, depth_out);
    else
        hipLaunchKernelGGL(k_gtprep<false>, grid, block, 0, st, seg, row_of, depth, ns, Hs, Ws, Hp, Wp, aH, aW, Gmax, Smax,
                           mode == PH_GTBOX_NEAREST, sh, sw, things, stuff, things_hard, stuff_hard, valid, depth_out);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
