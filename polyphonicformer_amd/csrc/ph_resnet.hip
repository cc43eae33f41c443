// ResNet backbone at inference (mmdet/models/backbones/resnet.py as configs/_base_/models/polyphonic_former.py:12-21 builds it;
// norm_eval=True, so every BatchNorm is an affine map that the host folds into the convolution in float64: w' = w g / sqrt(var + eps)
// rounded once to the grade, b' = beta - mu g / sqrt(var + eps) in fp32).  Activations are ONE 16-bit channels-last plane
// [B][H * W][C] (bf16 or fp16), accumulation is fp32, each layer output is rounded once.
//
//   k_conv_cl     : Y[b][p][n] = act(sum_{tap, c} X[b][s p + tap][c] W'[n][tap][c] + b'[n] + R[b][p][n]); 1x1 / 3x3, stride 1 / 2,
//                   Cin and Cout multiples of 64, R nullable, act = ReLU or identity.  Implicit GEMM on the 32x32x16 MFMA.
//   k_resnet_stem : conv 7x7 stride 2 pad 3 (3 -> 64) + folded BN + ReLU + MaxPool2d(3, 2, 1) from the NCHW image to the channels-last
//                   plane; the half-resolution conv map lives in LDS only.
//   k_cl_to_nchw  : a stage's channels-last plane -> NCHW fp32 / bf16 / fp16 through an LDS transpose.
//
// GEMM core of k_conv_cl.  M = a run of TM = 64 MI consecutive output pixels of one frame, N = TN = 64 NI output channels, K in
// chunks of 64 input channels of one tap.  One workgroup = 4 waves as 2 x 2; a wave owns 32 MI pixels x 32 NI channels, MI x NI
// accumulators of the 32x32x16 MFMA.  Channels-last makes the A fragment of a pixel 8 consecutive channels, so the chunk is staged
// [TM][64] (row pitch 72) with one 16-byte load per thread and unit -- a tap outside the map or a pixel past the frame is a zero
// unit, a 1x1 stride-2 conv loads the sampled pixels only -- and read back with plain 16-byte LDS reads.  The B operand
// (pack.pack_b32 fragments of W'[Cout][taps * Cin], k = tap * Cin + c: one 1 KiB block per 32 channels and k-step) streams from
// memory (L2 resident) one chunk ahead, in registers.  The next chunk's A loads are in flight during a chunk's MFMAs as well.
// Every output element is the same chain of MFMA accumulations in every geometry, so the bits depend on neither the geometry nor B.
// Epilogue: accumulators + b' as fp32 through a wave-private LDS tile, then whole 16-byte channel runs: R in, + , act, one rounding, Y out.
#include "ph_resnet_inl.h"

#pragma clang fp contract(off)

struct RCArgs {
    const uint16_t* x;       // [B][H * W][Cin]
    const uint16_t* w;       // pack_b32 fragments of W'[Cout][taps * Cin]
    const float* bias;       // [Cout]
    const uint16_t* r;       // [B][Ho * Wo][Cout] or null
    uint16_t* y;             // [B][Ho * Wo][Cout]
    int H, W, Ho, Wo, Cin, Cout, ks, stride, relu;
};

template <int MI, int NI, int E>
__global__ __launch_bounds__(RC_THREADS) void k_conv_cl(const RCArgs a) {
    constexpr int TM = 64 * MI, TN = 64 * NI, EPW = 32 * NI + 4;
    constexpr int NU = TM * 8 / RC_THREADS;                       // 16-byte units of the chunk per thread
    constexpr size_t LDS_A = (size_t)TM * RC_LDA * 2, LDS_E = (size_t)4 * 32 * EPW * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_A > LDS_E ? LDS_A : LDS_E];
    uint16_t* la = (uint16_t*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.z, n0 = blockIdx.y * TN;
    const int64_t HoWo = (int64_t)a.Ho * a.Wo, m0 = (int64_t)blockIdx.x * TM;
    const int pad = a.ks >> 1, taps = a.ks * a.ks, cpt = a.Cin / RC_KC, nch = taps * cpt, KS16 = taps * a.Cin / 16;
    const uint16_t* xb = a.x + (int64_t)b * a.H * a.W * a.Cin;

    // the rows this thread stages: unit u = tid + 256 i -> row u >> 3, channels 8 (u & 7) ..
    const int c8 = (tid & 7) * 8;
    int iy0[NU], ix0[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int64_t p = m0 + (tid >> 3) + 32 * i;
        if (p < HoWo) {
            const int oy = (int)(p / a.Wo), ox = (int)(p - (int64_t)oy * a.Wo);
            iy0[i] = oy * a.stride - pad; ix0[i] = ox * a.stride - pad;
        } else {
            iy0[i] = -0x40000000; ix0[i] = 0;                       // never inside the map
        }
    }
    auto load = [&](uint4 (&v)[NU], int q) {
        const int tap = q / cpt, c0 = (q - tap * cpt) * RC_KC;
        const int ky = tap / a.ks, kx = tap - ky * a.ks;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int iy = iy0[i] + ky, ix = ix0[i] + kx;
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v[i] = *(const uint4*)(xb + ((int64_t)iy * a.W + ix) * a.Cin + c0 + c8);
        }
    };

    f32x16_t acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // this wave's B fragments: block (ct, ks) of the pack, 64 lanes x 8 elements
    const uint16_t* wrow[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) wrow[ni] = a.w + ((int64_t)(n0 / 32 + wn * NI + ni) * KS16 * 64 + lane) * 8;

    // B fragments of a whole chunk live in registers and run one chunk ahead: fragment kk of chunk q + 1 is requested right after the
    // MFMAs that consumed fragment kk of chunk q, so its latency has a chunk of MFMAs, two barriers and the staging to hide behind
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
    float bv[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) bv[ni] = a.bias[n0 + (wn * NI + ni) * 32 + l32];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) ep[((r & 3) + 8 * (r >> 2) + 4 * g) * EPW + ni * 32 + l32] = acc[mi][ni][r] + bv[ni];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2 * NI; ++it) {                      // 32 pixels x 4 NI units of 8 channels, 64 lanes
            const int idx = lane + 64 * it, row = idx / (4 * NI), u = idx - row * (4 * NI);
            const int64_t p = m0 + wm * 32 * MI + mi * 32 + row;
            if (p < HoWo) {
                const float4 s0 = *(const float4*)(ep + row * EPW + u * 8), s1 = *(const float4*)(ep + row * EPW + u * 8 + 4);
                float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const int64_t o = ((int64_t)b * HoWo + p) * a.Cout + n0 + wn * 32 * NI + u * 8;
                if (a.r) {
                    const uint4 t = *(const uint4*)(a.r + o);
                    const uint32_t wds[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s[2 * e] += e2f<E>(wds[e] & 0xFFFFu);
                        s[2 * e + 1] += e2f<E>(wds[e] >> 16);
                    }
                }
                uint32_t h[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) h[e] = f2e<E>(a.relu ? fmaxf(s[e], 0.f) : s[e]);
                *(uint4*)(a.y + o) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
            }
        }
        __syncthreads();
    }
}

extern "C" int ph_conv_cl_workgroups(int ksize, int stride, int Cin, int Cout, int H, int W, int B) {
    const int rc = rc_check("ph_conv_cl_workgroups", ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    const int pad = ksize / 2, Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const int64_t HoWo = (int64_t)Ho * Wo;
    const int geo = rc_geometry(HoWo, Cout);
    const int64_t n = ((HoWo + (geo ? 127 : 63)) / (geo ? 128 : 64)) * (Cout / (geo == 2 ? 128 : 64)) * B;
    return n > 0x7FFFFFFF ? PH_EINVAL : (int)n;
}

extern "C" int ph_conv_cl(const uint16_t* X, const uint16_t* Wp, const float* bias, const uint16_t* R, uint16_t* Y, int ksize,
                          int stride, int relu, int B, int H, int W, int Cin, int Cout, int prec, void* stream) {
    PH_CHECK_ARG(X && Wp && bias && Y, "null pointer (X, Wp, bias, Y)");
    const int rc = rc_check("ph_conv_cl", ksize, stride, Cin, Cout, H, W, B);
    if (rc != PH_OK) return rc;
    PH_CHECK_ARG(prec == PH_PREC_BF16 || prec == PH_PREC_F16, "prec must be PH_PREC_BF16 or PH_PREC_F16");
    PH_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Wp & 15) == 0 && ((uintptr_t)Y & 15) == 0 && ((uintptr_t)R & 15) == 0,
                 "X, Wp, R and Y must be 16-byte aligned");
    const int pad = ksize / 2, Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const int64_t HoWo = (int64_t)Ho * Wo;
    const int geo = rc_geometry(HoWo, Cout);
    const int64_t mt = (HoWo + (geo ? 127 : 63)) / (geo ? 128 : 64);
    PH_CHECK_ARG(mt <= 0x7FFFFFFF, "too many pixels");
    RCArgs a{X, Wp, bias, R, Y, H, W, Ho, Wo, Cin, Cout, ksize, stride, relu != 0};
    const dim3 grid((unsigned)mt, (unsigned)(Cout / (geo == 2 ? 128 : 64)), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
#define PH_RC(MI_, NI_)                                                                                                  \
    do {                                                                                                                 \
        if (prec == PH_PREC_F16) hipLaunchKernelGGL((k_conv_cl<MI_, NI_, PH_E_F16>), grid, dim3(RC_THREADS), 0, s, a);   \
        else hipLaunchKernelGGL((k_conv_cl<MI_, NI_, PH_E_BF16>), grid, dim3(RC_THREADS), 0, s, a);                      \
    } while (0)
    if (geo == 2) PH_RC(2, 2);
    else if (geo == 1) PH_RC(2, 1);
    else PH_RC(1, 1);
#undef PH_RC
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// ---- stem ---------------------------------------------------------------------------------------------------------------------
// One workgroup = an 8 x 8 tile of pooled pixels x 64 channels.  It needs the 17 x 17 conv pixels (2 py0 - 1 .., the pool's one-row
// and one-column halo recomputed: (17 / 16)^2 = 1.13 of the conv work) and for those the 39 x 39 x 3 image patch, staged in LDS as
// 16-bit [row][col][c] so that the 21 values (kx, c) of one kernel row are consecutive.  K order: k = 24 ky + 3 kx + c, each kernel
// row padded from 21 to 24 (zero weights), K = 168 padded to 176 = 11 k-steps; an 8-value A group never crosses a kernel row.  The
// conv map (+ b', ReLU, rounded -- rounding is monotone, so pooling the rounded values is pooling then rounding) is written to LDS
// [320][64] and pooled from there; conv pixels outside the conv map take no part in the max (not zeros, not relu(b')).
constexpr int ST_PT = 8, ST_CT = 2 * ST_PT + 1, ST_IN = 2 * ST_CT + 5;       // pooled tile, conv tile 17, image patch 39
constexpr int ST_NM = (ST_CT * ST_CT + 31) / 32;                             // 10 M tiles of 32 conv pixels
constexpr int ST_K = 176, ST_LDC = 64 + 8;
constexpr int ST_PATCH = ST_IN * ST_IN * 3, ST_PATCH_PAD = (ST_PATCH + 16 + 7) / 8 * 8;

struct STArgs {
    const void* x;           // [B][3][H][W] fp32 or bf16
    const uint16_t* w;       // pack_b32 fragments of W'[64][176]
    const float* bias;       // [64]
    uint16_t* y;             // [B][Hq * Wq][64]
    int H, W, Hc, Wc, Hq, Wq;
};

template <int E, int INDT>
__global__ __launch_bounds__(256) void k_resnet_stem(const STArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lin[ST_PATCH_PAD];
    __shared__ __attribute__((aligned(16))) uint16_t lc[ST_NM * 32 * ST_LDC];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.z, py0 = blockIdx.y * ST_PT, px0 = blockIdx.x * ST_PT;
    const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1, iy00 = 2 * cy0 - 3, ix00 = 2 * cx0 - 3;
    const int64_t HW = (int64_t)a.H * a.W;

    // image patch -> LDS, converted through fp32 to the grade; outside the image (the conv's zero padding) and the slack: zero
    for (int i = tid; i < ST_PATCH_PAD; i += 256) {
        uint32_t h = 0;
        if (i < ST_PATCH) {
            const int c = i / (ST_IN * ST_IN), rem = i - c * (ST_IN * ST_IN), r = rem / ST_IN, col = rem - r * ST_IN;
            const int iy = iy00 + r, ix = ix00 + col;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                const int64_t idx = ((int64_t)b * 3 + c) * HW + (int64_t)iy * a.W + ix;
                const float f = INDT == PH_OUT_F32 ? ((const float*)a.x)[idx] : bf2f(((const uint16_t*)a.x)[idx]);
                h = f2e<E>(f);
            }
            lin[(r * ST_IN + col) * 3 + c] = (uint16_t)h;
        } else {
            lin[i] = 0;                                             // i in [ST_PATCH, ST_PATCH_PAD): the slack behind the patch
        }
    }
    __syncthreads();

    const float bv0 = a.bias[l32], bv1 = a.bias[32 + l32];
    for (int mt = wave; mt < ST_NM; mt += 4) {                      // wave-uniform
        int m = mt * 32 + l32;
        if (m > ST_CT * ST_CT - 1) m = ST_CT * ST_CT - 1;           // rows past the conv tile: computed, never used
        const int ly = m / ST_CT, lx = m - ly * ST_CT;
        f32x16_t acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < ST_K / 16; ++ks) {
            int j = ks * 2 + g;                                     // 8-value group: kernel row j / 3, values 8 (j % 3) .. of its 24
            const bool kpad = j > 20;                               // k in [168, 176): zero weights
            if (kpad) j = 20;
            const int ky = j / 3, o8 = (j - ky * 3) * 8;
            const uint16_t* src = lin + ((2 * ly + ky) * ST_IN + 2 * lx) * 3 + o8;
            uint32_t e[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) e[t] = (kpad || o8 + t >= 21) ? 0u : (uint32_t)src[t];
            const uint4 xf = make_uint4(pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7]));
            const uint4 w0 = *(const uint4*)(a.w + ((int64_t)ks * 64 + lane) * 8);
            const uint4 w1 = *(const uint4*)(a.w + ((int64_t)(ST_K / 16 + ks) * 64 + lane) * 8);
            acc0 = mfma32e<E>(xf, w0, acc0);
            acc1 = mfma32e<E>(xf, w1, acc1);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
            lc[row * ST_LDC + l32] = (uint16_t)f2e<E>(fmaxf(acc0[r] + bv0, 0.f));
            lc[row * ST_LDC + 32 + l32] = (uint16_t)f2e<E>(fmaxf(acc1[r] + bv1, 0.f));
        }
    }
    __syncthreads();

    // pool: 64 pooled pixels x 8 units of 8 channels, two per thread
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + 256 * it, pl = idx >> 3, u = idx & 7;
        const int ty = pl / ST_PT, tx = pl - ty * ST_PT, py = py0 + ty, px = px0 + tx;
        if (py >= a.Hq || px >= a.Wq) continue;
        float m[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ly = 2 * ty + dy, lx = 2 * tx + dx, cy = cy0 + ly, cx = cx0 + lx;
                if (cy < 0 || cy >= a.Hc || cx < 0 || cx >= a.Wc) continue;
                const uint4 t = *(const uint4*)(lc + (ly * ST_CT + lx) * ST_LDC + u * 8);
                const uint32_t wds[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    m[2 * e] = fmaxf(m[2 * e], e2f<E>(wds[e] & 0xFFFFu));
                    m[2 * e + 1] = fmaxf(m[2 * e + 1], e2f<E>(wds[e] >> 16));
                }
            }
        uint32_t h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = f2e<E>(m[e]);
        *(uint4*)(a.y + (((int64_t)b * a.Hq + py) * a.Wq + px) * 64 + u * 8) =
            make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
    }
}

static int st_check(const char* fn, int H, int W, int B) {
    PH_CHECK_ARG_AS(fn, B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 32768 && W <= 32768, "B, H, W out of range");
    return PH_OK;
}

extern "C" int ph_resnet_stem_workgroups(int H, int W, int B) {
    const int rc = st_check("ph_resnet_stem_workgroups", H, W, B);
    if (rc != PH_OK) return rc;
    const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1, Hq = (Hc - 1) / 2 + 1, Wq = (Wc - 1) / 2 + 1;
    const int64_t n = (int64_t)((Hq + ST_PT - 1) / ST_PT) * ((Wq + ST_PT - 1) / ST_PT) * B;
    return n > 0x7FFFFFFF ? PH_EINVAL : (int)n;
}

extern "C" int ph_resnet_stem(const void* x, int x_dtype, const uint16_t* Wp, const float* bias, uint16_t* Y, int B, int H, int W,
                              int prec, void* stream) {
    PH_CHECK_ARG(x && Wp && bias && Y, "null pointer (x, Wp, bias, Y)");
    const int rc = st_check("ph_resnet_stem", H, W, B);
    if (rc != PH_OK) return rc;
    PH_CHECK_ARG(x_dtype == PH_OUT_F32 || x_dtype == PH_OUT_BF16, "x_dtype must be PH_OUT_F32 or PH_OUT_BF16");
    PH_CHECK_ARG(prec == PH_PREC_BF16 || prec == PH_PREC_F16, "prec must be PH_PREC_BF16 or PH_PREC_F16");
    PH_CHECK_ARG(((uintptr_t)Wp & 15) == 0 && ((uintptr_t)Y & 15) == 0, "Wp and Y must be 16-byte aligned");
    const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1, Hq = (Hc - 1) / 2 + 1, Wq = (Wc - 1) / 2 + 1;
    PH_CHECK_ARG((Hq + ST_PT - 1) / ST_PT <= 65535, "H out of range");
    STArgs a{x, Wp, bias, Y, H, W, Hc, Wc, Hq, Wq};
    const dim3 grid((unsigned)((Wq + ST_PT - 1) / ST_PT), (unsigned)((Hq + ST_PT - 1) / ST_PT), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (prec == PH_PREC_F16) {
        if (x_dtype == PH_OUT_F32) hipLaunchKernelGGL((k_resnet_stem<PH_E_F16, PH_OUT_F32>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_resnet_stem<PH_E_F16, PH_OUT_BF16>), grid, dim3(256), 0, s, a);
    } else {
        if (x_dtype == PH_OUT_F32) hipLaunchKernelGGL((k_resnet_stem<PH_E_BF16, PH_OUT_F32>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_resnet_stem<PH_E_BF16, PH_OUT_BF16>), grid, dim3(256), 0, s, a);
    }
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// ---- channels-last plane -> NCHW ------------------------------------------------------------------------------------------------
// a block takes 64 pixels x 64 channels: whole 128-byte channel runs in, through fp32 in LDS, and per channel row a run of 64
// consecutive pixels out (one wave instruction = 64 consecutive elements: whole 128- or 256-byte lines wherever the run is aligned)
template <int E, int ODT>
__global__ __launch_bounds__(256) void k_cl_to_nchw(const uint16_t* __restrict__ x, void* __restrict__ out, int64_t HW, int C) {
    __shared__ float t[64][65];
    const int tid = threadIdx.x, b = blockIdx.z, c0 = blockIdx.y * 64;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + 256 * it, pl = idx >> 3, u = idx & 7;
        if (p0 + pl < HW) {
            const uint4 q = *(const uint4*)(x + ((int64_t)b * HW + p0 + pl) * C + c0 + u * 8);
            const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                t[pl][u * 8 + 2 * e] = e2f<E>(wds[e] & 0xFFFFu);
                t[pl][u * 8 + 2 * e + 1] = e2f<E>(wds[e] >> 16);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int idx = tid + 256 * it, ch = idx >> 6, pl = idx & 63;
        if (p0 + pl >= HW) continue;
        const float f = t[pl][ch];
        const int64_t o = ((int64_t)b * C + c0 + ch) * HW + p0 + pl;
        if constexpr (ODT == PH_OUT_F32) ((float*)out)[o] = f;
        else if constexpr (ODT == PH_OUT_BF16) ((uint16_t*)out)[o] = (uint16_t)f2bf(f);
        else ((uint16_t*)out)[o] = (uint16_t)f2h(f);
    }
}

static int cn_check(const char* fn, int B, int64_t HW, int C) {
    PH_CHECK_ARG_AS(fn, B > 0 && B <= 65535 && HW > 0 && HW <= (int64_t)64 * 0x7FFFFFFF, "B, HW out of range");
    PH_CHECK_ARG_AS(fn, C >= 64 && C <= 4096 && C % 64 == 0, "C must be a multiple of 64 in [64, 4096]");
    return PH_OK;
}

extern "C" int ph_cl_to_nchw_workgroups(int B, int64_t HW, int C) {
    const int rc = cn_check("ph_cl_to_nchw_workgroups", B, HW, C);
    if (rc != PH_OK) return rc;
    const int64_t n = ((HW + 63) / 64) * (C / 64) * B;
    return n > 0x7FFFFFFF ? PH_EINVAL : (int)n;
}

extern "C" int ph_cl_to_nchw(const uint16_t* X, void* out, int out_dtype, int B, int64_t HW, int C, int prec, void* stream) {
    PH_CHECK_ARG(X && out, "null pointer (X, out)");
    const int rc = cn_check("ph_cl_to_nchw", B, HW, C);
    if (rc != PH_OK) return rc;
    PH_CHECK_ARG(out_dtype == PH_OUT_F32 || out_dtype == PH_OUT_BF16 || out_dtype == PH_OUT_F16,
                 "out_dtype must be PH_OUT_F32, PH_OUT_BF16 or PH_OUT_F16");
    PH_CHECK_ARG(prec == PH_PREC_BF16 || prec == PH_PREC_F16, "prec must be PH_PREC_BF16 or PH_PREC_F16");
    PH_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)out & 3) == 0, "X must be 16-byte aligned, out element-aligned");
    const dim3 grid((unsigned)((HW + 63) / 64), (unsigned)(C / 64), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
#define PH_CN(E_)                                                                                                               \
    do {                                                                                                                        \
        if (out_dtype == PH_OUT_F32) hipLaunchKernelGGL((k_cl_to_nchw<E_, PH_OUT_F32>), grid, dim3(256), 0, s, X, out, HW, C);  \
        else if (out_dtype == PH_OUT_BF16) hipLaunchKernelGGL((k_cl_to_nchw<E_, PH_OUT_BF16>), grid, dim3(256), 0, s, X, out, HW, C); \
        else hipLaunchKernelGGL((k_cl_to_nchw<E_, PH_OUT_F16>), grid, dim3(256), 0, s, X, out, HW, C);                          \
    } while (0)
    if (prec == PH_PREC_F16) PH_CN(PH_E_F16); else PH_CN(PH_E_BF16);
#undef PH_CN
    PH_CHECK_LAUNCH();
    return PH_OK;
}
