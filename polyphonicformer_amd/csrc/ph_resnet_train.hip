// ResNet backbone in training (norm_eval=True: every BatchNorm is the affine map ph_resnet_pack folds; grade bf16).  The forward is
// ph_resnet.hip's, z = W' * x + b' with W' = w s rounded to bf16, s = gamma / sqrt(var + eps), b' = beta - mu s.  With dZ the gradient
// at z (behind the ReLU mask):
//   dW'[n][tap][c] = sum_{b, p} dZ[b][p][n] X[b][stride p + tap - pad][c]        db[n] = sum_{b, p} dZ[b][p][n]
//   dX[q][c]       = sum_{tap, n} dZ[(q + pad - tap) / stride][n] W'[n][tap][c]   over the taps where the quotient is whole and inside
//   dw = dW' s,  dbeta = db,  dgamma = (sum_k dW'[n][k] w[n][k] - mu[n] db[n]) / sqrt(var[n] + eps)   (the rounding of W' passed through)
//
//   k_conv_cl_bwd_data   : k_conv_cl's GEMM core (ph_resnet.hip) on dZ and the transposed, tap-flipped pack of the same rounded W'
//                          (ph_resnet_pack_bwd): with the taps flipped the gather of a stride-1 layer is the forward's, a stride-2 layer
//                          adds the parity predicate.  Epilogue: + R (same size, or the half-resolution plane spread to the even / even
//                          pixels), zero where the mask plane is <= 0, one rounding.
//   k_conv_cl_bwd_weight : the reduction over (frame, pixel).  Both MFMA operands are [pixels][channels] tiles consumed along their slow
//                          axis: staged once in LDS as they lie in memory, read through ds_read_b64_tr_b16.  The pixel axis is split
//                          into nsplit ranges of whole 64-pixel chunks; partial sums go to the caller's scratch and are added in range
//                          order by k_bwd_weight_reduce, so the bits are the same from run to run.
//   k_resnet_fold_bwd    : (dW', db) -> (dw, dgamma, dbeta), s and the dgamma sum in float64.
//   k_resnet_pack_bwd    : the data gradient's B operand as a permutation of the 16-bit values of the forward pack.
//   k_nchw_grad_to_cl    : a stage's fp32 NCHW gradient (+ a bf16 plane) -> the masked bf16 channels-last plane, through an LDS transpose.
// All entry points launch only: no allocation, no synchronisation, no atomics.
#include <algorithm>

#include "ph_resnet_inl.h"

#pragma clang fp contract(off)

// ---- data gradient ------------------------------------------------------------------------------------------------------------
struct RDArgs {
    const uint16_t* dz;      // [B][Ho * Wo][Cout]
    const uint16_t* w;       // pack_b32 fragments of WT[Cin][taps * Cout], WT[c][t * Cout + n] = W'[n][taps - 1 - t][c]
    const uint16_t* r;       // [B][Hr * Wr][Cin] or null
    const uint16_t* m;       // [B][H * W][Cin] or null
    uint16_t* dx;            // [B][H * W][Cin]
    int H, W, Ho, Wo, Cin, Cout, ks, stride, rstride, Hr, Wr;
};

template <int MI, int NI>
__global__ __launch_bounds__(RC_THREADS) void k_conv_cl_bwd_data(const RDArgs a) {
    constexpr int E = PH_E_BF16;
    constexpr int TM = 64 * MI, TN = 64 * NI, EPW = 32 * NI + 4;
    constexpr int NU = TM * 8 / RC_THREADS;                       // 16-byte units of the chunk per thread
    constexpr size_t LDS_A = (size_t)TM * RC_LDA * 2, LDS_E = (size_t)4 * 32 * EPW * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_A > LDS_E ? LDS_A : LDS_E];
    uint16_t* la = (uint16_t*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.z, n0 = blockIdx.y * TN;
    const int64_t HW = (int64_t)a.H * a.W, m0 = (int64_t)blockIdx.x * TM;
    const int pad = a.ks >> 1, taps = a.ks * a.ks, cpt = a.Cout / RC_KC, nch = taps * cpt, KS16 = taps * a.Cout / 16;
    const uint16_t* zb = a.dz + (int64_t)b * a.Ho * a.Wo * a.Cout;

    // the rows this thread stages: unit u = tid + 256 i -> row u >> 3, channels 8 (u & 7) ..
    const int c8 = (tid & 7) * 8;
    int ty0[NU], tx0[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int64_t p = m0 + (tid >> 3) + 32 * i;
        if (p < HW) {
            const int qy = (int)(p / a.W), qx = (int)(p - (int64_t)qy * a.W);
            ty0[i] = qy - pad; tx0[i] = qx - pad;
        } else {
            ty0[i] = -0x40000000; tx0[i] = 0;                       // never inside the map
        }
    }
    const int odd = a.stride - 1, sh = a.stride >> 1;               // stride 1: no parity rule, quotient = the value; stride 2: even only
    auto load = [&](uint4 (&v)[NU], int q) {
        const int tap = q / cpt, c0 = (q - tap * cpt) * RC_KC;
        const int ky = tap / a.ks, kx = tap - ky * a.ks;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int ty = ty0[i] + ky, tx = tx0[i] + kx;
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            if (ty >= 0 && tx >= 0 && !((ty | tx) & odd)) {
                const int oy = ty >> sh, ox = tx >> sh;
                if (oy < a.Ho && ox < a.Wo) v[i] = *(const uint4*)(zb + ((int64_t)oy * a.Wo + ox) * a.Cout + c0 + c8);
            }
        }
    };

    f32x16_t acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const uint16_t* wrow[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) wrow[ni] = a.w + ((int64_t)(n0 / 32 + wn * NI + ni) * KS16 * 64 + lane) * 8;

    uint4 wf[4][NI];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) wf[kk][ni] = *(const uint4*)(wrow[ni] + (int64_t)kk * 512);
    uint4 v[NU];
    load(v, 0);
    for (int q = 0; q < nch; ++q) {
        __syncthreads();                                           // the previous chunk's fragment reads are done
#pragma unroll
        for (int i = 0; i < NU; ++i) *(uint4*)(la + ((tid >> 3) + 32 * i) * RC_LDA + c8) = v[i];
        __syncthreads();
        const bool more = q + 1 < nch;                             // uniform
        if (more) load(v, q + 1);                                  // in flight during the MFMAs
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            uint4 xf[MI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) xf[mi] = *(const uint4*)(la + (wm * 32 * MI + mi * 32 + l32) * RC_LDA + kk * 16 + g * 8);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = mfma32e<E>(xf[mi], wf[kk][ni], acc[mi][ni]);
            if (more) {
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) wf[kk][ni] = *(const uint4*)(wrow[ni] + (int64_t)((q + 1) * 4 + kk) * 512);
            }
        }
    }

    // ---- epilogue.  D layout: row = pixel (r & 3) + 8 (r >> 2) + 4 g, column = channel lane & 31 of sub-tile (mi, ni)
    __syncthreads();                                               // the last chunk's reads are done: the LDS is free
    float* ep = (float*)smem + wave * 32 * EPW;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * g) * EPW + ni * 32 + l32] = acc[mi][ni][r];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2 * NI; ++it) {                      // 32 pixels x 4 NI units of 8 channels, 64 lanes
            const int idx = lane + 64 * it, row = idx / (4 * NI), u = idx - row * (4 * NI);
            const int64_t p = m0 + wm * 32 * MI + mi * 32 + row;
            if (p < HW) {
                const float4 s0 = *(const float4*)(ep + row * EPW + u * 8), s1 = *(const float4*)(ep + row * EPW + u * 8 + 4);
                float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const int ch = n0 + wn * 32 * NI + u * 8;
                const int64_t o = ((int64_t)b * HW + p) * a.Cin + ch;
                if (a.r) {
                    int64_t ro = o;
                    bool have = true;
                    if (a.rstride == 2) {
                        const int qy = (int)(p / a.W), qx = (int)(p - (int64_t)qy * a.W);
                        have = !((qy | qx) & 1);
                        ro = (((int64_t)b * a.Hr + (qy >> 1)) * a.Wr + (qx >> 1)) * a.Cin + ch;
                    }
                    if (have) {
                        const uint4 t = *(const uint4*)(a.r + ro);
                        const uint32_t wds[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            s[2 * e] += e2f<E>(wds[e] & 0xFFFFu);
                            s[2 * e + 1] += e2f<E>(wds[e] >> 16);
                        }
                    }
                }
                if (a.m) {
                    const uint4 t = *(const uint4*)(a.m + o);
                    const uint32_t wds[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (!(e2f<E>(wds[e] & 0xFFFFu) > 0.f)) s[2 * e] = 0.f;
                        if (!(e2f<E>(wds[e] >> 16) > 0.f)) s[2 * e + 1] = 0.f;
                    }
                }
                uint32_t h[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) h[e] = f2e<E>(s[e]);
                *(uint4*)(a.dx + o) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
            }
        }
        __syncthreads();
    }
}

extern "C" int ph_conv_cl_bwd_data_workgroups(int ksize, int stride, int Cin, int Cout, int H, int W, int B) {
    const int rc = rc_check("ph_conv_cl_bwd_data_workgroups", ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    const int64_t HW = (int64_t)H * W;
    const int geo = rc_geometry(HW, Cin);
    const int64_t n = ((HW + (geo ? 127 : 63)) / (geo ? 128 : 64)) * (Cin / (geo == 2 ? 128 : 64)) * B;
    return n > 0x7FFFFFFF ? PH_EINVAL : (int)n;
}

extern "C" int ph_conv_cl_bwd_data(const uint16_t* dZ, const uint16_t* Wt, const uint16_t* R, int r_stride, const uint16_t* M, uint16_t* dX,
                                   int ksize, int stride, int B, int H, int W, int Cin, int Cout, void* stream) {
    PH_CHECK_ARG(dZ && Wt && dX, "null pointer (dZ, Wt, dX)");
    const int rc = rc_check("ph_conv_cl_bwd_data", ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    PH_CHECK_ARG(!R || r_stride == 1 || r_stride == 2, "r_stride must be 1 or 2");
    PH_CHECK_ARG(((uintptr_t)dZ & 15) == 0 && ((uintptr_t)Wt & 15) == 0 && ((uintptr_t)dX & 15) == 0 && ((uintptr_t)R & 15) == 0 &&
                     ((uintptr_t)M & 15) == 0,
                 "dZ, Wt, R, M and dX must be 16-byte aligned");
    const int pad = ksize / 2, Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const int64_t HW = (int64_t)H * W;
    const int geo = rc_geometry(HW, Cin);
    const int64_t mt = (HW + (geo ? 127 : 63)) / (geo ? 128 : 64);
    PH_CHECK_ARG(mt <= 0x7FFFFFFF, "too many pixels");
    RDArgs a{dZ, Wt, R, M, dX, H, W, Ho, Wo, Cin, Cout, ksize, stride, R ? r_stride : 1, (H - 1) / 2 + 1, (W - 1) / 2 + 1};
    const dim3 grid((unsigned)mt, (unsigned)(Cin / (geo == 2 ? 128 : 64)), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (geo == 2) hipLaunchKernelGGL((k_conv_cl_bwd_data<2, 2>), grid, dim3(RC_THREADS), 0, s, a);
    else if (geo == 1) hipLaunchKernelGGL((k_conv_cl_bwd_data<2, 1>), grid, dim3(RC_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_conv_cl_bwd_data<1, 1>), grid, dim3(RC_THREADS), 0, s, a);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// One workgroup = one 64 (Cout) x 64 (Cin) tile of one tap and one range of 64-pixel chunks (chunk q = frame q / cpf, pixels
// 64 (q % cpf) ..: a chunk never crosses a frame).  Per chunk the dZ tile [64 pixels][64 n] and the gathered X tile [64 pixels][64 c]
// are staged as they lie in memory, row pitch 96 elements (192 bytes: the four rows of a transposed read land 16 banks apart, so the
// 32 lanes of a half cover 64 distinct banks; 8-byte aligned units), and each of the 2 x 2 waves reads its 32-channel halves of both
// through ds_read_b64_tr_b16: lane (l32, g) gets pixels 8 g .. 8 g + 7 of channel l32, the MFMA's A / B fragment.  The next chunk's
// loads are in flight during a chunk's MFMAs.  db: the workgroups of tap 0 / Cin tile 0 also sum the dZ tile's columns, per chunk 16
// rows per thread first, then into the running sum.
constexpr int RW_LD = 96;

struct RWArgs {
    const uint16_t* dz;      // [B][Ho * Wo][Cout]
    const uint16_t* x;       // [B][H * W][Cin]
    float* dw;               // [nsplit][Cout][taps * Cin] (nsplit 1: the result)
    float* db;               // [nsplit][Cout]
    int H, W, Ho, Wo, Cin, Cout, ks, stride, cpf, nchunks, cps;
};

typedef short s16x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 rw_frag(const uint16_t* p) {          // rows r .. r + 3 and r + 4 .. r + 7 of the lane's block
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((PH_LDS s16x4_t*)p);
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((PH_LDS s16x4_t*)(p + 4 * RW_LD));
    const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
    return make_uint4(l.x, l.y, h.x, h.y);
}

__global__ __launch_bounds__(256) void k_conv_cl_bwd_weight(const RWArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lz[64 * RW_LD];
    __shared__ __attribute__((aligned(16))) uint16_t lx[64 * RW_LD];
    __shared__ float lsum[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, l32 = lane & 31;
    const int ctiles = a.Cin / 64, tap = blockIdx.x / ctiles, c0 = (blockIdx.x - tap * ctiles) * 64, n0 = blockIdx.y * 64, z = blockIdx.z;
    const int pad = a.ks >> 1, ky = tap / a.ks, kx = tap - ky * a.ks;
    const int HoWo = a.Ho * a.Wo;
    const int64_t HW = (int64_t)a.H * a.W;
    const bool with_db = blockIdx.x == 0;                          // uniform
    const int q0 = z * a.cps, q1 = min(q0 + a.cps, a.nchunks);

    const int c8 = (tid & 7) * 8, row = tid >> 3;                  // units tid and tid + 256: rows row and row + 32
    auto load = [&](uint4 (&vz)[2], uint4 (&vx)[2], int q) {
        const int b = q / a.cpf, p0 = (q - b * a.cpf) * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = p0 + row + 32 * i;
            vz[i] = make_uint4(0u, 0u, 0u, 0u); vx[i] = make_uint4(0u, 0u, 0u, 0u);
            if (p < HoWo) {
                vz[i] = *(const uint4*)(a.dz + ((int64_t)b * HoWo + p) * a.Cout + n0 + c8);
                const int oy = p / a.Wo, ox = p - oy * a.Wo, iy = oy * a.stride + ky - pad, ix = ox * a.stride + kx - pad;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    vx[i] = *(const uint4*)(a.x + ((int64_t)b * HW + (int64_t)iy * a.W + ix) * a.Cin + c0 + c8);
            }
        }
    };

    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float dbsum = 0.f;

    // the lane's transposed-read address inside a 16-pixel k-step: row 8 g + (i16 >> 2), column 32 w + 16 gi + 4 (i16 & 3)
    const int i16 = lane & 15, gi = (lane >> 4) & 1;
    const int fo = (8 * g + (i16 >> 2)) * RW_LD + 16 * gi + 4 * (i16 & 3);
    const uint16_t* fz = lz + fo + 32 * wm;
    const uint16_t* fx = lx + fo + 32 * wn;

    uint4 vz[2], vx[2];
    if (q0 < q1) load(vz, vx, q0);
    for (int q = q0; q < q1; ++q) {
        __syncthreads();                                           // the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *(uint4*)(lz + (row + 32 * i) * RW_LD + c8) = vz[i];
            *(uint4*)(lx + (row + 32 * i) * RW_LD + c8) = vx[i];
        }
        __syncthreads();
        if (q + 1 < q1) load(vz, vx, q + 1);                       // uniform; in flight during the MFMAs
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const uint4 za = rw_frag(fz + kk * 16 * RW_LD), xb = rw_frag(fx + kk * 16 * RW_LD);
            acc = mfma32e<PH_E_BF16>(za, xb, acc);
        }
        if (with_db) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) s += bf2f(lz[(wave * 16 + r) * RW_LD + lane]);
            dbsum += s;
        }
    }

    // D layout: row = output channel (r & 3) + 8 (r >> 2) + 4 g of the wave's 32, column = input channel l32
    const int K = a.ks * a.ks * a.Cin;
    float* out = a.dw + (int64_t)z * a.Cout * K + (int64_t)(n0 + wm * 32) * K + tap * a.Cin + c0 + wn * 32 + l32;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * g) * K] = acc[r];
    if (with_db) {
        lsum[wave][lane] = dbsum;
        __syncthreads();
        if (tid < 64) a.db[(int64_t)z * a.Cout + n0 + tid] = ((lsum[0][tid] + lsum[1][tid]) + lsum[2][tid]) + lsum[3][tid];
    }
}

// out[i] = ((p[0][i] + p[1][i]) + p[2][i]) + ...: the ranges in order, four floats per thread; n4 = floats / 4 of one range
__global__ __launch_bounds__(256) void k_bwd_weight_reduce(const float4* __restrict__ p, float4* __restrict__ out, int64_t n4, int nsplit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 s = p[i];
    for (int z = 1; z < nsplit; ++z) {
        const float4 t = p[(int64_t)z * n4 + i];
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    out[i] = s;
}

static int64_t rw_chunks(int ksize, int stride, int H, int W, int B) {
    const int pad = ksize / 2, Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    return (((int64_t)Ho * Wo + 63) / 64) * B;
}

static int rw_check(const char* fn, int ksize, int stride, int Cin, int Cout, int H, int W, int B) {
    const int rc = rc_check(fn, ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    PH_CHECK_ARG_AS(fn, rw_chunks(ksize, stride, H, W, B) <= 0x3FFFFFFF, "too many pixels");
    return PH_OK;
}

// The library's one rule.  tiles = workgroups of one range; the ranges multiply them until the 256 CUs have about four workgroups
// each, while a range keeps at least four chunks (below that the partial planes cost more than the parallelism gives) and there are
// at most 64 of them.
extern "C" int ph_conv_cl_bwd_weight_nsplit(int ksize, int stride, int Cin, int Cout, int H, int W, int B) {
    const int rc = rw_check("ph_conv_cl_bwd_weight_nsplit", ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    const int64_t chunks = rw_chunks(ksize, stride, H, W, B), tiles = (int64_t)ksize * ksize * (Cin / 64) * (Cout / 64);
    int64_t n = (1024 + tiles - 1) / tiles;
    n = std::min(n, std::max<int64_t>(chunks / 4, 1));
    n = std::min<int64_t>(n, 64);
    // every range non-empty: ranges of cps = ceil(chunks / n) chunks, the count that such ranges fill
    const int64_t cps = (chunks + n - 1) / n;
    return (int)((chunks + cps - 1) / cps);
}

extern "C" int64_t ph_conv_cl_bwd_weight_partial_floats(int ksize, int stride, int Cin, int Cout, int H, int W, int B, int nsplit) {
    const int rc = rw_check("ph_conv_cl_bwd_weight_partial_floats", ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    if (nsplit == 0) nsplit = ph_conv_cl_bwd_weight_nsplit(ksize, stride, Cin, Cout, H, W, B);
    if (nsplit < 1 || nsplit > rw_chunks(ksize, stride, H, W, B)) {
        ph_set_error("ph_conv_cl_bwd_weight_partial_floats: nsplit must lie in [1, the number of 64-pixel chunks]");
        return PH_EINVAL;
    }
    return nsplit == 1 ? 0 : (int64_t)nsplit * ((int64_t)Cout * ksize * ksize * Cin + Cout);
}

extern "C" int ph_conv_cl_bwd_weight(const uint16_t* dZ, const uint16_t* X, float* dW, float* db, float* partial, int nsplit, int ksize,
                                     int stride, int B, int H, int W, int Cin, int Cout, void* stream) {
    PH_CHECK_ARG(dZ && X && dW && db, "null pointer (dZ, X, dW, db)");
    const int rc = rw_check("ph_conv_cl_bwd_weight", ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    const int64_t chunks = rw_chunks(ksize, stride, H, W, B);
    if (nsplit == 0) nsplit = ph_conv_cl_bwd_weight_nsplit(ksize, stride, Cin, Cout, H, W, B);
    PH_CHECK_ARG(nsplit >= 1 && nsplit <= chunks, "nsplit must lie in [1, the number of 64-pixel chunks]");
    PH_CHECK_ARG(nsplit <= 65535, "nsplit: at most 65535 ranges");
    PH_CHECK_ARG(nsplit == 1 || partial, "null partial with more than one range");
    PH_CHECK_ARG(((uintptr_t)dZ & 15) == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)dW & 15) == 0 && ((uintptr_t)db & 15) == 0 &&
                     ((uintptr_t)partial & 15) == 0,
                 "dZ, X, dW, db and partial must be 16-byte aligned");
    const int pad = ksize / 2, Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const int taps = ksize * ksize;
    const int64_t nw = (int64_t)Cout * taps * Cin;
    const int cpf = (int)(chunks / B), cps = (int)((chunks + nsplit - 1) / nsplit);
    hipStream_t s = (hipStream_t)stream;
    RWArgs a{dZ, X, nsplit == 1 ? dW : partial, nsplit == 1 ? db : partial + (int64_t)nsplit * nw, H, W, Ho, Wo, Cin, Cout, ksize, stride,
             cpf, (int)chunks, cps};
    hipLaunchKernelGGL(k_conv_cl_bwd_weight, dim3((unsigned)(taps * (Cin / 64)), (unsigned)(Cout / 64), (unsigned)nsplit), dim3(256), 0, s, a);
    PH_CHECK_LAUNCH();
    if (nsplit > 1) {
        hipLaunchKernelGGL(k_bwd_weight_reduce, dim3((unsigned)((nw / 4 + 255) / 256)), dim3(256), 0, s, (const float4*)partial, (float4*)dW,
                           nw / 4, nsplit);
        PH_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_bwd_weight_reduce, dim3((unsigned)((Cout / 4 + 255) / 256)), dim3(256), 0, s,
                           (const float4*)(partial + (int64_t)nsplit * nw), (float4*)db, (int64_t)(Cout / 4), nsplit);
        PH_CHECK_LAUNCH();
    }
    return PH_OK;
}

// ---- fold backward ------------------------------------------------------------------------------------------------------------
// one workgroup per output channel n.  dw[n][c][tap] = fp32(dW'[n][tap * Cin + c] s) with s = gamma / sqrt(var + eps) in float64;
// dgamma = (sum_k dW'[n][k] w[n][k] - mu db) / sqrt(var + eps): each thread adds its k = tid, tid + 256, .. in order, the 256 sums are
// folded pairwise in LDS -- a fixed order.
struct RFArgs {
    const float *dwp, *db, *w, *gamma, *mean, *var;
    float *dw, *dgamma, *dbeta;
    double eps;
    int Cin, taps;
};

__global__ __launch_bounds__(256) void k_resnet_fold_bwd(const RFArgs a) {
    __shared__ double red[256];
    const int n = blockIdx.x, tid = threadIdx.x, K = a.taps * a.Cin;
    const double rstd = 1.0 / sqrt((double)a.var[n] + a.eps), s = (double)a.gamma[n] / sqrt((double)a.var[n] + a.eps);
    const float* src = a.dwp + (int64_t)n * K;
    const float* wn = a.w + (int64_t)n * K;
    float* dst = a.dw + (int64_t)n * K;
    double sum = 0.0;
    for (int k = tid; k < K; k += 256) {
        const int tap = k / a.Cin, c = k - tap * a.Cin, j = c * a.taps + tap;
        const double d = (double)src[k];
        dst[j] = (float)(d * s);
        sum += d * (double)wn[j];
    }
    red[tid] = sum;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        const double dbn = (double)a.db[n];
        if (a.dgamma) a.dgamma[n] = (float)((red[0] - (double)a.mean[n] * dbn) * rstd);
        if (a.dbeta) a.dbeta[n] = a.db[n];
    }
}

extern "C" int ph_resnet_fold_bwd(const float* dWp, const float* db, const float* w, const float* gamma, const float* mean, const float* var,
                                  double eps, float* dw, float* dgamma, float* dbeta, int ksize, int Cin, int Cout, void* stream) {
    PH_CHECK_ARG(dWp && db && w && gamma && mean && var && dw, "null pointer (dWp, db, w, gamma, mean, var, dw)");
    PH_CHECK_ARG(ksize == 1 || ksize == 3, "ksize must be 1 or 3");
    PH_CHECK_ARG(Cin >= 1 && Cin <= 4096 && Cout >= 1 && Cout <= 65535, "Cin, Cout out of range");
    PH_CHECK_ARG(eps >= 0 && eps < 1e300, "eps must be finite and >= 0");
    RFArgs a{dWp, db, w, gamma, mean, var, dw, dgamma, dbeta, eps, Cin, ksize * ksize};
    hipLaunchKernelGGL(k_resnet_fold_bwd, dim3((unsigned)Cout), dim3(256), 0, (hipStream_t)stream, a);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// ---- transposed pack ----------------------------------------------------------------------------------------------------------
// one thread per 16-byte unit of the output: 8 consecutive k = t * Cout + n of one row c of WT, from 8 rows n of the forward pack
// (fragment order [ct][ks][g][n][e] holds W2[32 ct + n][16 ks + 8 g + e])
__global__ __launch_bounds__(256) void k_resnet_pack_bwd(const uint16_t* __restrict__ fwd, uint4* __restrict__ out, uint32_t units, int Cin,
                                                         int Cout, int taps) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const uint32_t i = u * 8u, KSo = (uint32_t)(taps * Cout) / 16u, KSi = (uint32_t)(taps * Cin) / 16u;
    const uint32_t nn = (i >> 3) & 31u, gq = (i >> 8) & 1u, r = i >> 9;
    const int c = (int)(32u * (r / KSo) + nn), k = (int)(16u * (r % KSo) + 8u * gq);      // row of WT, its first k
    const int t = k / Cout, n_first = k - t * Cout, kin = (taps - 1 - t) * Cin + c;      // a unit lies in one tap: Cout % 8 == 0
    uint32_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t n = (uint32_t)(n_first + e);
        const size_t src = ((((size_t)(n >> 5) * KSi + (uint32_t)kin / 16u) * 2u + (((uint32_t)kin >> 3) & 1u)) * 32u + (n & 31u)) * 8u +
                           ((uint32_t)kin & 7u);
        v[e] = fwd[src];
    }
    out[u] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
}

extern "C" int ph_conv_cl_pack_bwd(const uint16_t* Wp, uint16_t* Wt, int ksize, int Cin, int Cout, void* stream) {
    PH_CHECK_ARG(Wp && Wt, "null pointer (Wp, Wt)");
    const int rc = rc_check("ph_conv_cl_pack_bwd", ksize, 1, Cin, Cout, 1, 1, 1);
    if (rc != PH_OK) return rc;
    PH_CHECK_ARG(((uintptr_t)Wp & 1) == 0 && ((uintptr_t)Wt & 15) == 0, "Wt must be 16-byte aligned");
    const uint32_t units = (uint32_t)((int64_t)Cin * ksize * ksize * Cout / 8);
    hipLaunchKernelGGL(k_resnet_pack_bwd, dim3((units + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, Wp, (uint4*)Wt, units, Cin, Cout,
                       ksize * ksize);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// the convolutions whose input gradient the backward needs: stages 1 .. 3 (layer2 .. layer4) without layer2.0's conv1 and downsample,
// behind which everything is frozen.  Piece PH_RPACK_W(i) of the layout is convolution i's transposed pack (i: the forward's index in
// state_dict order; the bytes are the forward W piece's), every other piece is empty.
struct RTConv { int ks, cin, cout, wanted; };

static int rt_layouts(const ph_resnet_cfg* cfg, ph_resnet_layout* fwd, ph_resnet_layout* bwd, RTConv* cv, uint64_t* total, const char* fn) {
    PH_CHECK_ARG_AS(fn, cfg != nullptr, "null cfg");
    PH_CHECK_ARG_AS(fn, ph_mode_grade(cfg->mode) == PH_PREC_BF16, "mode: the backbone trains in its bf16 grade (PH_MODE_BF16)");
    PH_RUN(ph_resnet_pack_layout(cfg, fwd));                        // refuses every other cfg error, the depth among them
    static const int a50[4] = {3, 4, 6, 3}, a101[4] = {3, 4, 23, 3}, a152[4] = {3, 8, 36, 3};
    const int* arch = cfg->depth == 50 ? a50 : cfg->depth == 101 ? a101 : a152;
    *bwd = ph_resnet_layout{};
    bwd->nconvs = fwd->nconvs;
    cv[0] = RTConv{7, 3, 64, 0};
    uint64_t o = 0;
    int i = 1, inpl = 64;
    for (int si = 0; si < 4; ++si) {
        const int planes = 64 << si;
        for (int j = 0; j < arch[si]; ++j) {
            const int cin = j == 0 ? inpl : 4 * planes, frozen_behind = si == 1 && j == 0;
            cv[i++] = RTConv{1, cin, planes, si >= 1 && !frozen_behind};
            cv[i++] = RTConv{3, planes, planes, si >= 1};
            cv[i++] = RTConv{1, planes, 4 * planes, si >= 1};
            if (j == 0) cv[i++] = RTConv{1, cin, 4 * planes, si >= 1 && !frozen_behind};
        }
        inpl = 4 * planes;
    }
    for (int c = 1; c < i; ++c) {
        if (!cv[c].wanted) continue;
        bwd->offset[PH_RPACK_W(c)] = o;
        bwd->bytes[PH_RPACK_W(c)] = fwd->bytes[PH_RPACK_W(c)];
        o += al256(fwd->bytes[PH_RPACK_W(c)]);
    }
    *total = o;
    return PH_OK;
}

extern "C" size_t ph_resnet_pack_bwd_bytes(const ph_resnet_cfg* cfg) {
    ph_resnet_layout f, b;
    RTConv cv[PH_RESNET_MAX_CONVS];
    uint64_t total = 0;
    return rt_layouts(cfg, &f, &b, cv, &total, __func__) == PH_OK ? (size_t)total : 0;
}

extern "C" int ph_resnet_pack_bwd_layout(const ph_resnet_cfg* cfg, ph_resnet_layout* layout) {
    PH_CHECK_ARG(layout != nullptr, "null layout");
    ph_resnet_layout f;
    RTConv cv[PH_RESNET_MAX_CONVS];
    uint64_t total = 0;
    return rt_layouts(cfg, &f, layout, cv, &total, __func__);
}

extern "C" int ph_resnet_pack_bwd(const ph_resnet_cfg* cfg, const void* pack, void* pack_bwd, void* stream) {
    ph_resnet_layout f, b;
    RTConv cv[PH_RESNET_MAX_CONVS];
    uint64_t total = 0;
    PH_RUN(rt_layouts(cfg, &f, &b, cv, &total, __func__));
    PH_CHECK_ARG(pack && pack_bwd, "null pack or pack_bwd");
    PH_CHECK_ARG(((uintptr_t)pack & 255) == 0 && ((uintptr_t)pack_bwd & 255) == 0, "pack and pack_bwd must be 256-byte aligned");
    for (int c = 1; c < b.nconvs; ++c)
        if (cv[c].wanted)
            PH_RUN(ph_conv_cl_pack_bwd((const uint16_t*)((const char*)pack + f.offset[PH_RPACK_W(c)]),
                                       (uint16_t*)((char*)pack_bwd + b.offset[PH_RPACK_W(c)]), cv[c].ks, cv[c].cin, cv[c].cout, stream));
    return PH_OK;
}

// ---- gradient ingest ----------------------------------------------------------------------------------------------------------
// the mirror of k_cl_to_nchw: a block takes 64 pixels x 64 channels, per channel row a run of 64 consecutive pixels in, through fp32
// in LDS, whole 16-byte channel runs out
__global__ __launch_bounds__(256) void k_nchw_grad_to_cl(const float* __restrict__ gsrc, const uint16_t* __restrict__ add,
                                                         const uint16_t* __restrict__ mask, uint16_t* __restrict__ out, int64_t HW, int C) {
    __shared__ float t[64][65];
    const int tid = threadIdx.x, b = blockIdx.z, c0 = blockIdx.y * 64;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int idx = tid + 256 * it, ch = idx >> 6, pl = idx & 63;
        if (p0 + pl < HW) t[pl][ch] = gsrc[((int64_t)b * C + c0 + ch) * HW + p0 + pl];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + 256 * it, pl = idx >> 3, u = idx & 7;
        if (p0 + pl >= HW) continue;
        const int64_t o = ((int64_t)b * HW + p0 + pl) * C + c0 + u * 8;
        float s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = t[pl][u * 8 + e];
        if (add) {
            const uint4 q = *(const uint4*)(add + o);
            const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[2 * e] = bf2f(wds[e] & 0xFFFFu) + s[2 * e];
                s[2 * e + 1] = bf2f(wds[e] >> 16) + s[2 * e + 1];
            }
        }
        uint32_t h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = f2bf(s[e]);
        if (mask) {
            const uint4 q = *(const uint4*)(mask + o);
            const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!(bf2f(wds[e] & 0xFFFFu) > 0.f)) h[2 * e] = 0u;
                if (!(bf2f(wds[e] >> 16) > 0.f)) h[2 * e + 1] = 0u;
            }
        }
        *(uint4*)(out + o) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
    }
}

extern "C" int ph_nchw_grad_to_cl(const float* g, const uint16_t* add, const uint16_t* mask, uint16_t* out, int B, int64_t HW, int C,
                                  void* stream) {
    PH_CHECK_ARG(g && out, "null pointer (g, out)");
    PH_CHECK_ARG(B > 0 && B <= 65535 && HW > 0 && HW <= (int64_t)64 * 0x7FFFFFFF, "B, HW out of range");
    PH_CHECK_ARG(C >= 64 && C <= 4096 && C % 64 == 0, "C must be a multiple of 64 in [64, 4096]");
    PH_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)add & 15) == 0 && ((uintptr_t)mask & 15) == 0 && ((uintptr_t)out & 15) == 0,
                 "add, mask and out must be 16-byte aligned, g element-aligned");
    const dim3 grid((unsigned)((HW + 63) / 64), (unsigned)(C / 64), (unsigned)B);
    hipLaunchKernelGGL(k_nchw_grad_to_cl, grid, dim3(256), 0, (hipStream_t)stream, g, add, mask, out, HW, C);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
