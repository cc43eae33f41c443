// ph_gtmask_boxes: the RoIs of the sampled ground-truth masks of a training step (include/polyhead.h), straight from the masks at the
// assign resolution.  Replaces, per key / reference frame, polyphonic_former_video.py:283-305 (bilinear upsample to the padded image,
// sigmoid > 0.5) + video/utils.py:39-83 (nonzero, two means, two mean absolute deviations, four .item() calls per mask) + :413-415.
//
// A mask's box needs its row and column pixel counts only, so no [n][H][W] tensor is formed:
//   k_gtbox_counts  grid (row bands of 64 output rows, ground truths, frames): a thread owns output columns X = t, t + 256, ... and walks
//                   down the band with the two horizontally interpolated source rows in registers (reloaded when the source row
//                   changes: 2 / ratio loads per pixel); the band's row counts are one disjoint slice of the mask's row histogram, its
//                   column counts one partial row.  No atomics, every word the second launch reads is written here.
//   k_gtbox_finish  grid (ground truths, frames): rank of the mask's prediction row among the matched ones, integer sums of the
//                   histograms (order-free, hence the same bits in every call), means and deviations in fp64, one rounding to fp32.
#include "ph_common.h"

namespace {

constexpr int GB_T = 256;            // threads per workgroup (both kernels)
constexpr int GB_ROWS = 64;          // output rows per band = lanes per wave: lane i keeps the count of the band's row i

struct GbFrames {
    const float* m[PH_GTBOX_MAX_FRAMES];       // DEVICE [G][h][w]
    int32_t G[PH_GTBOX_MAX_FRAMES];
    int32_t n[PH_GTBOX_MAX_FRAMES];
    int32_t roi0[PH_GTBOX_MAX_FRAMES];         // first row of the frame in rois / pos_gt / count
    int32_t slot0[PH_GTBOX_MAX_FRAMES];        // first workspace slot of the frame (one per ground truth)
};
static_assert(sizeof(GbFrames) <= 2048, "the frame table travels as a kernel argument");

// ATen's source index of a destination pixel (area_pixel_compute_source_index, align_corners = False), fp32
__device__ __forceinline__ void gb_src(float scale, int dst, int in, int& i0, int& step, float& l0, float& l1) {
#pragma clang fp contract(off)
    float r = scale * ((float)dst + 0.5f) - 0.5f;
    r = r < 0.f ? 0.f : r;
    i0 = (int)r;
    i0 = i0 > in - 1 ? in - 1 : i0;           // never taken for H >= h (r < in - 0.5); keeps every address inside the mask regardless
    step = i0 < in - 1 ? 1 : 0;
    l1 = r - (float)i0;
    l0 = 1.f - l1;
}

__global__ __launch_bounds__(GB_T) void k_gtbox_counts(GbFrames fr, const int32_t* __restrict__ match, int64_t match_stride, int h, int w,
                                                        int H, int W, float scale_h, float scale_w, int nb, int32_t* __restrict__ rowcnt,
                                                        uint16_t* __restrict__ colpart) {
#pragma clang fp contract(off)
    const int f = blockIdx.z, g = blockIdx.y, band = blockIdx.x;
    if (g >= fr.G[f] || match[f * match_stride + g] < 0) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t slot = fr.slot0[f] + g;
    const float* __restrict__ m = fr.m[f] + (int64_t)g * h * w;
    const int Y0 = band * GB_ROWS;
    const int rows = min(GB_ROWS, H - Y0);
    uint16_t* __restrict__ cp = colpart + (slot * nb + band) * (int64_t)W;
    int rowacc = 0;
    for (int X0 = 0; X0 < W; X0 += GB_T) {            // uniform trip count: the ballots below see whole waves
        const int X = X0 + t;
        const bool live = X < W;
        int x0, xs;
        float wl0, wl1;
        gb_src(scale_w, live ? X : W - 1, w, x0, xs, wl0, wl1);
        int cached = -1, colc = 0;
        float top = 0.f, bot = 0.f;
        for (int yi = 0; yi < rows; ++yi) {
            int y0, ys;
            float hl0, hl1;
            gb_src(scale_h, Y0 + yi, h, y0, ys, hl0, hl1);
            if (y0 != cached) {                       // uniform
                const float* r0 = m + (int64_t)y0 * w;
                const float* r1 = r0 + (int64_t)ys * w;
                top = wl0 * r0[x0] + wl1 * r0[x0 + xs];
                bot = wl0 * r1[x0] + wl1 * r1[x0 + xs];
                cached = y0;
            }
            const float v = hl0 * top + hl1 * bot;
            const bool on = live && v > PH_BIN_THR;
            colc += on ? 1 : 0;
            const int pc = __popcll(__ballot(on));
            rowacc += lane == yi ? pc : 0;
        }
        if (live) cp[X] = (uint16_t)colc;
    }
    __shared__ int srow[GB_T / 64][GB_ROWS];
    srow[wave][lane] = rowacc;
    __syncthreads();
    if (t < rows) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < GB_T / 64; ++k) s += srow[k][t];
        rowcnt[slot * H + Y0 + t] = s;
    }
}

// sums of two int64 per thread over the workgroup, every thread gets both; integer sums are the same in any order
__device__ __forceinline__ void gb_sum2(long long& a, long long& b, long long (*s)[2]) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t][0] = a;
    s[t][1] = b;
    __syncthreads();
    for (int k = GB_T / 2; k > 0; k >>= 1) {
        if (t < k) {
            s[t][0] += s[t + k][0];
            s[t][1] += s[t + k][1];
        }
        __syncthreads();
    }
    a = s[0][0];
    b = s[0][1];
}

// (count, sum of index * count) over the entries selected by `below` (index < mean; all of them when mean < 0 is not needed: pass +inf)
__device__ __forceinline__ void gb_axis(const int32_t* rows, const uint16_t* cols, int nb, int len, double below, long long& cnt,
                                        long long& sum) {
    cnt = sum = 0;
    for (int i = threadIdx.x; i < len; i += GB_T) {
        long long c = 0;
        if (rows) c = rows[i];
        else
            for (int b = 0; b < nb; ++b) c += cols[(int64_t)b * len + i];
        if ((double)i < below) {
            cnt += c;
            sum += c * i;
        }
    }
}

__global__ __launch_bounds__(GB_T) void k_gtbox_finish(GbFrames fr, const int32_t* __restrict__ match, int64_t match_stride, int H, int W,
                                                        int nb, const int32_t* __restrict__ rowcnt, const uint16_t* __restrict__ colpart,
                                                        float* __restrict__ rois, int32_t* __restrict__ pos_gt,
                                                        int64_t* __restrict__ count) {
    const int f = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
    const int G = fr.G[f];
    if (g >= G) return;
    const int32_t* mt = match + f * match_stride;
    const int mg = mt[g];
    if (mg < 0) return;
    // rank of this mask's prediction row among the matched ones (G <= PH_ASSIGN_MAX = GB_T); equal rows, which a matching never
    // holds, are ordered by g so that the ranks stay distinct
    int before = 0;
    if (t < G) {
        const int mo = mt[t];
        before = mo >= 0 && (mo < mg || (mo == mg && t < g));
    }
    const int rank = __syncthreads_count(before);
    if (rank >= fr.n[f]) return;                      // more matched entries than the caller sized the outputs for: dropped, not written
    __shared__ long long s[GB_T][2];
    const int64_t slot = fr.slot0[f] + g;
    const int32_t* rows = rowcnt + slot * H;
    const uint16_t* cols = colpart + slot * nb * (int64_t)W;
    const double inf = __builtin_huge_val();
    long long n, sy, nx, sx;
    gb_axis(rows, nullptr, 0, H, inf, n, sy);
    gb_sum2(n, sy, s);
    gb_axis(nullptr, cols, nb, W, inf, nx, sx);
    gb_sum2(nx, sx, s);
    float box[4] = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) {                                      // uniform
        const double my = (double)sy / (double)n, mx = (double)sx / (double)n;
        long long nly, sly, nlx, slx;
        gb_axis(rows, nullptr, 0, H, my, nly, sly);
        gb_sum2(nly, sly, s);
        gb_axis(nullptr, cols, nb, W, mx, nlx, slx);
        gb_sum2(nlx, slx, s);
        // sum c |i - mean| = mean (n_lo - n_hi) + (S_hi - S_lo); an index equal to the mean adds 0 on either side
        const double dy = (my * (double)(2 * nly - n) + (double)(sy - 2 * sly)) / (double)n;
        const double dx = (mx * (double)(2 * nlx - n) + (double)(sx - 2 * slx)) / (double)n;
        const double ey = 2.0 * (dy > 1.0 ? dy : 1.0), ex = 2.0 * (dx > 1.0 ? dx : 1.0);
        box[0] = (float)(mx - ex);
        box[1] = (float)(my - ey);
        box[2] = (float)(mx + ex);
        box[3] = (float)(my + ey);
    }
    if (t == 0) {
        const int64_t r = fr.roi0[f] + rank;
        rois[r * 5] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) rois[r * 5 + 1 + k] = box[k] < 0.f ? 0.f : box[k];       // :415 clamp(min=0)
        pos_gt[r] = g;
        count[r] = n;
    }
}

size_t gb_workspace(int64_t slots, int H, int W, size_t* col_off) {
    const int64_t nb = (H + GB_ROWS - 1) / GB_ROWS;
    const size_t rows = al256((size_t)slots * H * sizeof(int32_t));
    if (col_off) *col_off = rows;
    return rows + al256((size_t)slots * nb * W * sizeof(uint16_t));
}

}  // namespace

extern "C" size_t ph_gtmask_boxes_workspace_bytes(int frames, const int32_t* G, int H, int W) {
    if (frames < 1 || frames > PH_GTBOX_MAX_FRAMES || !G || H < 1 || W < 1 || H > 65536 || W > 65536) {
        ph_set_error("ph_gtmask_boxes_workspace_bytes: 1 .. %d frames, G, 1 <= H, W <= 65536", PH_GTBOX_MAX_FRAMES);
        return 0;
    }
    int64_t slots = 0;
    for (int b = 0; b < frames; ++b) {
        if (G[b] < 0 || G[b] > PH_ASSIGN_MAX) {
            ph_set_error("ph_gtmask_boxes_workspace_bytes: 0 .. %d ground truths per frame", PH_ASSIGN_MAX);
            return 0;
        }
        slots += G[b];
    }
    return gb_workspace(slots, H, W, nullptr);
}

extern "C" int ph_gtmask_boxes(const float* const* masks, const int32_t* G, const int32_t* n, const int32_t* roi_start, const int32_t* match,
                               int64_t match_stride, int Np, int frames, int h, int w, int H, int W, int mode, float* rois, int32_t* pos_gt,
                               int64_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(GB_T >= PH_ASSIGN_MAX, "k_gtbox_finish ranks a frame's ground truths with one thread each");
    PH_CHECK_ARG(masks && G && n && roi_start && match && rois && pos_gt && count, "null argument");
    PH_CHECK_ARG(frames >= 1 && frames <= PH_GTBOX_MAX_FRAMES, "1 .. 64 frames per call");
    if (mode != PH_GTBOX_BILINEAR) {
        ph_set_error("ph_gtmask_boxes: only the bilinear upsample (align_corners = False) is implemented, not the nearest mode");
        return PH_EUNSUPPORTED;
    }
    PH_CHECK_ARG(h >= 1 && w >= 1 && H >= 1 && W >= 1 && H <= 65536 && W <= 65536 && Np >= 0, "1 <= h, w, H, W <= 65536, Np >= 0");
    if (H < h || W < w) {
        ph_set_error("ph_gtmask_boxes: H >= h and W >= w (an upsample); got %d x %d -> %d x %d", h, w, H, W);
        return PH_EUNSUPPORTED;
    }
    GbFrames fr;
    int64_t slots = 0;
    int gmax = 0, total = 0;
    for (int b = 0; b < PH_GTBOX_MAX_FRAMES; ++b) {
        fr.m[b] = nullptr;
        fr.G[b] = fr.n[b] = fr.roi0[b] = fr.slot0[b] = 0;
    }
    for (int b = 0; b < frames; ++b) {
        PH_CHECK_ARG(G[b] >= 0 && G[b] <= PH_ASSIGN_MAX, "0 .. 256 ground truths per frame");
        PH_CHECK_ARG(n[b] <= PH_TRACK_LOSS_MAX_ROIS, "at most 128 RoIs per frame");
        PH_CHECK_ARG(n[b] == (G[b] < Np ? G[b] : Np), "n must be the matched count min(G, Np)");
        PH_CHECK_ARG(G[b] == 0 || (masks[b] && ((uintptr_t)masks[b] & 3) == 0), "a frame with ground truths needs its masks (fp32)");
        PH_CHECK_ARG(roi_start[b] >= 0, "negative row offset");
        PH_CHECK_ARG(frames == 1 || match_stride >= G[b], "match_stride below a frame's ground-truth count");
        fr.m[b] = masks[b];
        fr.G[b] = G[b];
        fr.n[b] = n[b];
        fr.roi0[b] = roi_start[b];
        fr.slot0[b] = (int32_t)slots;
        slots += G[b];
        gmax = G[b] > gmax ? G[b] : gmax;
        total += n[b];
    }
    size_t col_off = 0;
    const size_t need = gb_workspace(slots, H, W, &col_off);
    if (need > 0) {
        if (!workspace || workspace_bytes < need) {
            ph_set_error("ph_gtmask_boxes: workspace too small (%zu bytes, %zu needed)", workspace ? workspace_bytes : (size_t)0, need);
            return PH_EWORKSPACE;
        }
        PH_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "the workspace must be 16-byte aligned");
    }
    if (total == 0) return PH_OK;                     // nothing matched anywhere: no RoI to write
    const int nb = (H + GB_ROWS - 1) / GB_ROWS;
    int32_t* rowcnt = (int32_t*)workspace;
    uint16_t* colpart = (uint16_t*)((char*)workspace + col_off);
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_gtbox_counts, dim3(nb, gmax, frames), dim3(GB_T), 0, st, fr, match, match_stride, h, w, H, W, sh, sw, nb, rowcnt,
                       colpart);
    PH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gtbox_finish, dim3(gmax, frames), dim3(GB_T), 0, st, fr, match, match_stride, H, W, nb, rowcnt, colpart, rois, pos_gt,
                       count);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
