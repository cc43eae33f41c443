// libpolyhead, training side: what the FPN (mmdet/models/necks/fpn.py:151-203) needs beyond the neck's and the heads' training
// kernels, on fp32 NCHW maps as autograd hands them over.
//
//   ph_map_x_map_t_wide : O[m][k] = sum_b sum_p G[b][m][p] X[b][k][p] for K up to 4096 -- the weight gradient of a lateral 1x1
//                         convolution (G = dL/dlateral, 256 rows; X = the backbone stage, 256 .. 2048 rows) and, from the same pass,
//                         the bias gradient (row sums of G).  The kernel is ph_train.hip's k_map_x_mapT with K tiles of 256 columns
//                         as one more grid dimension: this file adds the split rule and the public name.
//   ph_nearest_up_add[_bwd] : the top-down pathway (fpn.py:164-175, nearest to the finer level's size) in place, and its transpose
//                         as a gather: every coarse pixel is written once, its (up to) four sources added in a fixed order.
//   ph_nchw_bias_add, ph_nchw_channel_sums : the bias of the 3x3 output convolutions and its gradient (fp64 sums, fixed order).
//
// Launch-only: no allocation, no synchronisation, no atomics; argument errors are PH_EINVAL before anything is launched.
#include "ph_common.h"

namespace {

// ---- top-down add ------------------------------------------------------------------------------------------------------------
// Sizes: H in {2 Hc, 2 Hc - 1}, likewise W (ph_fpn_lateral's rule).  There floor(y * Hc / H) = y >> 1 for every y < H: with
// H = 2 Hc - 1, y Hc / H = y / 2 + y / (2 H) and y / (2 H) < 1 / 2.  So fine pixel (y, x) reads coarse (y >> 1, x >> 1), and coarse
// pixel (Y, X) is read by (2Y, 2X), (2Y, 2X + 1), (2Y + 1, 2X), (2Y + 1, 2X + 1) where those exist.
// One wave per map row, four rows per workgroup, grid-stride over the rows.
__global__ __launch_bounds__(256) void k_nearest_up_add(float* __restrict__ fine, const float* __restrict__ coarse, int64_t rows, int H, int W,
                                                        int Hc, int Wc) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t pl = r / H;
        const int y = (int)(r - pl * H);
        float* f = fine + r * W;
        const float* c = coarse + (pl * Hc + min(y >> 1, Hc - 1)) * Wc;
        for (int x = lane; x < W; x += 64) f[x] += c[min(x >> 1, Wc - 1)];
    }
}

template <bool ACC>
__global__ __launch_bounds__(256) void k_nearest_up_add_bwd(const float* __restrict__ gf, float* __restrict__ gc, int64_t rows, int H, int W,
                                                            int Hc, int Wc) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t pl = r / Hc;
        const int Y = (int)(r - pl * Hc);
        const float* a = gf + (pl * H + 2 * Y) * W;          // 2 Y < H under the size rule
        const bool two = 2 * Y + 1 < H;
        float* o = gc + r * Wc;
        for (int X = lane; X < Wc; X += 64) {
            const bool right = 2 * X + 1 < W;
            float v = ACC ? o[X] : 0.f;
            v += a[2 * X];
            if (right) v += a[2 * X + 1];
            if (two) {
                v += a[W + 2 * X];
                if (right) v += a[W + 2 * X + 1];
            }
            o[X] = v;
        }
    }
}

// ---- bias of an NCHW map and its gradient -----------------------------------------------------------------------------------------
constexpr int BIAS_CHUNK = 4096;        // pixels of one plane per workgroup
__global__ __launch_bounds__(256) void k_nchw_bias_add(float* __restrict__ y, const float* __restrict__ bias, int C, int64_t HW) {
    const int64_t pl = blockIdx.x;
    const float bv = bias[pl % C];
    float* p = y + pl * HW;
    const int64_t pa = (int64_t)blockIdx.y * BIAS_CHUNK, pe = min(HW, pa + BIAS_CHUNK);
    for (int64_t i = pa + threadIdx.x; i < pe; i += 256) p[i] += bv;
}

// partial [C][B][nsplit] doubles: thread t of a workgroup adds pixels pa + t, pa + t + 256, .. in that order, the 256 threads are
// folded by an xor butterfly inside each wave and the four waves in order
__global__ __launch_bounds__(256) void k_nchw_channel_partial(const float* __restrict__ g, double* __restrict__ partial, int B, int C, int64_t HW,
                                                              int64_t chunk) {
    __shared__ double red[4];
    const int64_t pl = blockIdx.x;
    const int b = (int)(pl / C), c = (int)(pl % C);
    const int s = blockIdx.y, nsplit = gridDim.y;
    const float* p = g + pl * HW;
    const int64_t pa = s * chunk, pe = min(HW, pa + chunk);
    double acc = 0.0;
    for (int64_t i = pa + threadIdx.x; i < pe; i += 256) acc += (double)p[i];
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[((int64_t)c * B + b) * nsplit + s] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_nchw_channel_final(const double* __restrict__ partial, float* __restrict__ out, int C, int n) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double* p = partial + (int64_t)c * n;
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += p[i];
    out[c] = (float)acc;
}

unsigned row_blocks(int64_t rows) {
    const int64_t blocks = (rows + 3) / 4;
    return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

}  // namespace

// ---- the wide map x map^T product ------------------------------------------------------------------------------------------------
extern "C" int ph_map_x_map_t_wide_nsplit(int B, int M, int K, int64_t HW) {
    const int passes = M > 0 ? ph_map_x_map_t_passes(M) : 1;
    const int ktiles = K > 256 ? (K + 255) / 256 : 1;
    int64_t want = 1024 / ((int64_t)(B > 0 ? B : 1) * passes * ktiles);      // the workgroup budget, shared by the K tiles too
    const int64_t most = HW / 256;                                           // at least 256 pixels per split: HW / nsplit >= 256
    if (want > most) want = most;
    if (want < 1) want = 1;
    return (int)want;
}

extern "C" int ph_map_x_map_t_wide(const float* G, const float* X, float* partial /* [B][nsplit][M][K] */, float* out, int B, int M, int K,
                                   int64_t HW, int nsplit, float* rs_partial /* [B][nsplit][M] or null */, float* rowsum, int sum_batch,
                                   void* stream) {
    return ph_map_x_map_t_k("ph_map_x_map_t_wide", 1, G, X, partial, out, B, M, K, HW, nsplit, 0, rs_partial, rowsum, sum_batch, stream);
}

// ---- top-down add ------------------------------------------------------------------------------------------------------------------
extern "C" int ph_nearest_up_add(float* fine /* [planes][H][W], in place */, const float* coarse /* [planes][Hc][Wc] */, int64_t planes, int H,
                                 int W, int Hc, int Wc, void* stream) {
    PH_CHECK_ARG(fine && coarse && planes > 0 && H > 0 && W > 0, "bad pointer or size");
    PH_CHECK_ARG(Hc > 0 && Wc > 0 && ph_fpn_size_rule(H, Hc) && ph_fpn_size_rule(W, Wc), "coarse size: H must be 2 Hc or 2 Hc - 1 and W must be 2 Wc or 2 Wc - 1");
    const int64_t rows = planes * H;
    hipLaunchKernelGGL(k_nearest_up_add, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, fine, coarse, rows, H, W, Hc, Wc);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

extern "C" int ph_nearest_up_add_bwd(const float* g_fine /* [planes][H][W] */, float* g_coarse /* [planes][Hc][Wc] */, int64_t planes, int H,
                                     int W, int Hc, int Wc, int accumulate, void* stream) {
    PH_CHECK_ARG(g_fine && g_coarse && planes > 0 && H > 0 && W > 0, "bad pointer or size");
    PH_CHECK_ARG(Hc > 0 && Wc > 0 && ph_fpn_size_rule(H, Hc) && ph_fpn_size_rule(W, Wc), "coarse size: H must be 2 Hc or 2 Hc - 1 and W must be 2 Wc or 2 Wc - 1");
    const int64_t rows = planes * Hc;
    if (accumulate)
        hipLaunchKernelGGL(k_nearest_up_add_bwd<true>, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, g_fine, g_coarse, rows, H, W, Hc, Wc);
    else
        hipLaunchKernelGGL(k_nearest_up_add_bwd<false>, dim3(row_blocks(rows)), dim3(256), 0, (hipStream_t)stream, g_fine, g_coarse, rows, H, W, Hc, Wc);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// ---- bias and channel sums ---------------------------------------------------------------------------------------------------------
extern "C" int ph_nchw_bias_add(float* y /* [B][C][HW], in place */, const float* bias /* [C] */, int B, int C, int64_t HW, void* stream) {
    PH_CHECK_ARG(y && bias && B > 0 && C > 0 && HW > 0, "bad pointer or size");
    const int64_t chunks = (HW + BIAS_CHUNK - 1) / BIAS_CHUNK;
    PH_CHECK_ARG((int64_t)B * C <= 0x7FFFFFFF && chunks <= 65535, "B * C or HW out of range");
    hipLaunchKernelGGL(k_nchw_bias_add, dim3((unsigned)((int64_t)B * C), (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, y, bias, C, HW);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

extern "C" int ph_nchw_channel_sums_nsplit(int64_t HW) {
    int64_t n = (HW + BIAS_CHUNK - 1) / BIAS_CHUNK;     // at least 4096 pixels per split, at most 64 splits of a plane
    if (n > 64) n = 64;
    if (n < 1) n = 1;
    return (int)n;
}

extern "C" int ph_nchw_channel_sums(const float* g /* [B][C][HW] */, double* partial /* [C][B][nsplit] */, float* out /* [C] */, int B, int C,
                                    int64_t HW, void* stream) {
    PH_CHECK_ARG(g && partial && out && B > 0 && C > 0 && HW > 0, "bad pointer or size");
    PH_CHECK_ARG((int64_t)B * C <= 0x7FFFFFFF, "B * C out of range");
    const int ns = ph_nchw_channel_sums_nsplit(HW);
    int64_t chunk = (HW + ns - 1) / ns;
    chunk = (chunk + 255) / 256 * 256;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nchw_channel_partial, dim3((unsigned)((int64_t)B * C), ns), dim3(256), 0, s, g, partial, B, C, HW, chunk);
    PH_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_nchw_channel_final, dim3((C + 255) / 256), dim3(256), 0, s, partial, out, C, B * ns);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
