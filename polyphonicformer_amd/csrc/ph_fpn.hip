// FPN (mmdet/models/necks/fpn.py:151-203 as configured in configs/_base_/models/polyphonic_former.py:22-29): four 1x1 lateral
// convolutions K -> 256 with bias, joined top-down by a nearest-neighbour add, then four 3x3 convolutions 256 -> 256 with bias; no
// norm, no activation.  The 3x3 convolutions are ph_conv_nhwc as it is; this file adds what stands around them:
//
//   k_fpn_lateral : one level's lateral.  out[b][px][n] = round16(sum_k W[n][k] x[b][k][px] + bias[n] + coarse[b][nearest(px)][n])
//                   straight from the backbone's NCHW map (fp32 / bf16 / fp16; every element crosses HBM once, converted through
//                   fp32 to the grade's 16-bit format while it is staged) to the channels-last 16-bit planes the 3x3 kernel reads.
//   k_fpn_lateral_cl : the same lateral from the backbone's channels-last 16-bit plane, which then never becomes an NCHW tensor.
//   k_fpn_output  : fp32 NHWC conv result + bias -> fp32 NCHW, the level the module hands out.
//
// GEMM core of the lateral (the recipe of ph_khead.hip with the operands swapped): M = 64-pixel tile, N = 256 output channels, K in
// chunks of 256 input channels.  One workgroup = 8 waves; wave w owns output channels 32 w .. 32 w + 31 and streams its B operand
// (pack.pack_b32 fragments of W: one 1 KiB block per k-step, L2 resident) from memory; the A operand is the pixel tile, staged into
// LDS as [256 c][64 px] and read back with ds_read_b64_tr_b16.  The next chunk's loads are in flight during a chunk's MFMAs.
// Epilogue: accumulators + bias as fp32 [64 px][256] in LDS, then whole 16-byte channel runs: coarse planes in, output planes out.
#include "ph_common.h"

constexpr int FL_T = 64;                 // pixels per tile
constexpr int FL_KC = 256;               // input channels per chunk
constexpr int FL_LDT = FL_T + 32;        // row stride 48 dwords: the transposing reads are bank-conflict free (ph_khead.hip)
constexpr int FL_THREADS = 512;
constexpr int FL_EP = 256 + 4;           // fp32 row pitch of the epilogue tile

struct FLArgs {
    const void* x;                // [B][K][HW], element type INDT
    const uint16_t* w;            // [P] x pack_b32 fragments of W[256][K]
    int64_t w_plane;
    const float* bias;            // [256]
    const uint16_t* coarse;       // [P][B][Hc * Wc][256] or null
    uint16_t* out;                // [P][B][H * W][256]
    int B, K, H, W, Hc, Wc;
};

template <int INDT> __device__ __forceinline__ float fl_ld(const void* base, int64_t idx) {
    if constexpr (INDT == PH_OUT_F32) return __builtin_nontemporal_load((const float*)base + idx);
    else if constexpr (INDT == PH_OUT_BF16) return bf2f(__builtin_nontemporal_load((const uint16_t*)base + idx));
    else return h2f(__builtin_nontemporal_load((const uint16_t*)base + idx));
}
template <int INDT> __device__ __forceinline__ float fl_cv(uint32_t h) { return INDT == PH_OUT_BF16 ? bf2f(h) : h2f(h); }

// chunk [256 c][64 px] of frame `src` ([K][HW]) from channel k0: 16 threads per channel row, 4 px each, 32 rows per pass.  Every
// load is unconditional and inside the map: the pixel column is clamped (and zeroed when it is staged), a channel row past K
// -- the last chunk of a K that is no multiple of 256 -- is clamped to K - 1 (the k-loop never reads it).
// AL4: HW % 4 == 0 and an aligned base (one 16- or 8-byte load per pass), else four element loads.
template <int INDT, bool AL4>
__device__ __forceinline__ void fl_load(float (&v)[8][4], const void* src, int K, int64_t HW, int k0, int64_t px0, int tid) {
    const int row_in = tid >> 4, p4 = (tid & 15) * 4;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        int c = k0 + q * 32 + row_in;
        if (c > K - 1) c = K - 1;
        if constexpr (AL4) {
            int64_t col = px0 + p4;
            if (col > HW - 4) col = HW - 4;
            const int64_t idx = (int64_t)c * HW + col;
            if constexpr (INDT == PH_OUT_F32) {
                const uint4 t = ld_nt16((const float*)src + idx);
                v[q][0] = __uint_as_float(t.x); v[q][1] = __uint_as_float(t.y); v[q][2] = __uint_as_float(t.z); v[q][3] = __uint_as_float(t.w);
            } else {
                const uint2 t = ld_nt8((const uint16_t*)src + idx);
                v[q][0] = fl_cv<INDT>(t.x & 0xFFFFu); v[q][1] = fl_cv<INDT>(t.x >> 16);
                v[q][2] = fl_cv<INDT>(t.y & 0xFFFFu); v[q][3] = fl_cv<INDT>(t.y >> 16);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int64_t col = px0 + p4 + e;
                if (col > HW - 1) col = HW - 1;
                v[q][e] = fl_ld<INDT>(src, (int64_t)c * HW + col);
            }
        }
    }
}

// fp32 -> the grade's plane(s) in LDS; columns past the map are zero
template <int PA, int E>
__device__ __forceinline__ void fl_store(const float (&v)[8][4], uint16_t* lds, int tid, int64_t HW, int64_t px0) {
    const int row_in = tid >> 4, p4 = (tid & 15) * 4;
    bool ok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ok[e] = px0 + p4 + e < HW;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int row = q * 32 + row_in;
        uint32_t hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) f2e_split<E>(ok[e] ? v[q][e] : 0.f, hi[e], lo[e]);
        *(uint2*)(lds + row * FL_LDT + p4) = make_uint2(pack2(hi[0], hi[1]), pack2(hi[2], hi[3]));
        if (PA == 2) *(uint2*)(lds + FL_KC * FL_LDT + row * FL_LDT + p4) = make_uint2(pack2(lo[0], lo[1]), pack2(lo[2], lo[3]));
    }
}

// the epilogue of both lateral kernels, called by all 512 threads behind the last chunk: accumulators + bias as fp32 [64 px][256]
// through LDS, then whole 16-byte channel runs -- the coarse level's value in, one rounding, the output planes out
template <int PA, int E>
__device__ __forceinline__ void fl_epilogue(const FLArgs& a, const f32x16_t (&acc)[2], uint16_t* lds, int b, int64_t HW, int64_t px0,
                                            int tid, int lane, int wave, int g) {
    // D layout: row = pixel (r & 3) + 8 (r >> 2) + 4 g of sub-tile ct, column = channel 32 wave + (lane & 31)
    __syncthreads();                                     // the last chunk's fragment reads are done: the LDS is free
    float* tf = (float*)lds;
    {
        const int ch = wave * 32 + (lane & 31);
        const float bv = a.bias[ch];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int px = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
                tf[px * FL_EP + ch] = acc[ct][r] + bv;
            }
    }
    __syncthreads();
    const int64_t oplane = (int64_t)a.B * HW * 256;
    const int64_t HWc = (int64_t)a.Hc * a.Wc, cplane = (int64_t)a.B * HWc * 256;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int idx = tid + it * FL_THREADS;
        const int pl = idx >> 5, c8 = (idx & 31) * 8;
        const int64_t px = px0 + pl;
        if (px >= HW) continue;
        const float4 s0 = *(const float4*)(tf + pl * FL_EP + c8), s1 = *(const float4*)(tf + pl * FL_EP + c8 + 4);
        float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        if (a.coarse) {
            // F.interpolate(mode='nearest', size=(H, W)) for H in {2 Hc, 2 Hc - 1}: source index y Hc / H in integers (host-checked)
            const int y = (int)(px / a.W), x = (int)(px - (int64_t)y * a.W);
            int cy = y * a.Hc / a.H, cx = x * a.Wc / a.W;
            if (cy > a.Hc - 1) cy = a.Hc - 1;
            if (cx > a.Wc - 1) cx = a.Wc - 1;
            const uint16_t* cp = a.coarse + ((int64_t)b * HWc + (int64_t)cy * a.Wc + cx) * 256 + c8;
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                const uint4 q = *(const uint4*)(cp + p * cplane);
                const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[2 * e] += e2f<E>(wds[e] & 0xFFFFu);
                    s[2 * e + 1] += e2f<E>(wds[e] >> 16);
                }
            }
        }
        uint32_t hi[8], lo[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f2e_split<E>(s[e], hi[e], lo[e]);
        uint16_t* op = a.out + ((int64_t)b * HW + px) * 256 + c8;
        *(uint4*)op = make_uint4(pack2(hi[0], hi[1]), pack2(hi[2], hi[3]), pack2(hi[4], hi[5]), pack2(hi[6], hi[7]));
        if (PA == 2) *(uint4*)(op + oplane) = make_uint4(pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(lo[4], lo[5]), pack2(lo[6], lo[7]));
    }
}

template <int PA, int E, int INDT, bool AL4>
__global__ __launch_bounds__(FL_THREADS) void k_fpn_lateral(const FLArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, i16 = lane & 15, gi = (lane >> 4) & 1;
    const int b = blockIdx.y, K = a.K;
    const int64_t HW = (int64_t)a.H * a.W, px0 = (int64_t)blockIdx.x * FL_T;
    const size_t esz = INDT == PH_OUT_F32 ? 4 : 2;
    const void* src = (const char*)a.x + (size_t)b * K * HW * esz;
    // this wave's B fragments: block (ct = wave, ks) of the pack, 64 lanes x 8 elements
    const uint16_t* wrow = a.w + ((int64_t)wave * (K / 16) * 64 + lane) * 8;

    f32x16_t acc[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

    float v[8][4];
    fl_load<INDT, AL4>(v, src, K, HW, 0, px0, tid);
    for (int k0 = 0; k0 < K; k0 += FL_KC) {
        __syncthreads();
        fl_store<PA, E>(v, lds, tid, HW, px0);
        __syncthreads();
        if (k0 + FL_KC < K) fl_load<INDT, AL4>(v, src, K, HW, k0 + FL_KC, px0, tid);     // in flight during the MFMAs (uniform branch)
        const int nks = (K - k0 < FL_KC ? K - k0 : FL_KC) / 16;                          // K % 64 == 0: a multiple of 4
        const uint16_t* wk = wrow + (int64_t)(k0 / 16) * 512;
        for (int ks4 = 0; ks4 < nks; ks4 += 4) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ks = ks4 + kk;
                uint4 wf[PA];
#pragma unroll
                for (int p = 0; p < PA; ++p) wf[p] = *(const uint4*)(wk + p * a.w_plane + (int64_t)ks * 512);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    uint4 xf[PA];
#pragma unroll
                    for (int p = 0; p < PA; ++p) {
                        // every lane's address lies inside the [256][FL_LDT] image (pad, don't mask); all 64 lanes are active here
                        const uint16_t* a0 = lds + p * FL_KC * FL_LDT + (ks * 16 + g * 8 + (i16 >> 2)) * FL_LDT + ct * 32 + gi * 16 + (i16 & 3) * 4;
                        const uint2 lo = lds_read_tr16(a0);
                        const uint2 hi = lds_read_tr16(a0 + 4 * FL_LDT);
                        xf[p] = make_uint4(lo.x, lo.y, hi.x, hi.y);
                    }
                    acc[ct] = mfma32e<E>(xf[0], wf[0], acc[ct]);
                    if (PA == 2) {
                        acc[ct] = mfma32e<E>(xf[0], wf[PA - 1], acc[ct]);
                        acc[ct] = mfma32e<E>(xf[PA - 1], wf[0], acc[ct]);
                    }
                }
            }
        }
    }

    fl_epilogue<PA, E>(a, acc, lds, b, HW, px0, tid, lane, wave, g);
}

extern "C" int ph_fpn_lateral(const void* x, int x_dtype, const uint16_t* Wp, int64_t w_plane_elems, const float* bias,
                              const uint16_t* coarse, int Hc, int Wc, uint16_t* out, int B, int K, int H, int W, int prec,
                              void* stream) {
    PH_CHECK_ARG(x && Wp && bias && out, "null pointer (x, Wp, bias, out)");
    PH_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= (int64_t)FL_T * 0x7FFFFFFF, "B, H, W out of range");
    PH_CHECK_ARG(K >= 64 && K <= 4096 && K % 64 == 0, "K must be a multiple of 64 in [64, 4096]");
    PH_CHECK_ARG(w_plane_elems == (int64_t)256 * K, "w_plane_elems must be 256 * K (pack_b32 fragments of W[256][K])");
    PH_CHECK_ARG(x_dtype == PH_OUT_F32 || x_dtype == PH_OUT_BF16 || x_dtype == PH_OUT_F16, "x_dtype must be PH_OUT_F32, PH_OUT_BF16 or PH_OUT_F16");
    PH_CHECK_ARG(prec == PH_PREC_BF16 || prec == PH_PREC_SPLIT || prec == PH_PREC_F16, "prec must be PH_PREC_BF16, PH_PREC_SPLIT or PH_PREC_F16");
    if (coarse) {
        PH_CHECK_ARG(Hc > 0 && Wc > 0 && ph_fpn_size_rule(H, Hc) && ph_fpn_size_rule(W, Wc),
                     "coarse size: H must be 2 Hc or 2 Hc - 1 and W must be 2 Wc or 2 Wc - 1 (the sizes at which the integer nearest index is torch's)");
        PH_CHECK_ARG(((uintptr_t)coarse & 15) == 0, "coarse must be 16-byte aligned");
    }
    PH_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)Wp & 15) == 0, "out and Wp must be 16-byte aligned");
    const int64_t HW = (int64_t)H * W;
    const int PA = prec == PH_PREC_SPLIT ? 2 : 1;
    const size_t esz = x_dtype == PH_OUT_F32 ? 4 : 2;
    const bool al4 = HW % 4 == 0 && ((uintptr_t)x % (4 * esz)) == 0;
    FLArgs a{x, Wp, w_plane_elems, bias, coarse, out, B, K, H, W, coarse ? Hc : 1, coarse ? Wc : 1};
    const dim3 grid((unsigned)((HW + FL_T - 1) / FL_T), (unsigned)B);
    size_t lds = (size_t)PA * FL_KC * FL_LDT * sizeof(uint16_t);
    const size_t ep = (size_t)FL_T * FL_EP * sizeof(float);
    if (lds < ep) lds = ep;
    hipStream_t s = (hipStream_t)stream;
#define PH_FL(PA_, E_, D_, A_)                                                                                                    \
    do {                                                                                                                          \
        static const bool once = [&] {                                                                                            \
            (void)hipFuncSetAttribute((const void*)k_fpn_lateral<PA_, E_, D_, A_>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                      (int)((size_t)PA_ * FL_KC * FL_LDT * sizeof(uint16_t) < ep ? ep                            \
                                                                                                 : (size_t)PA_ * FL_KC * FL_LDT * sizeof(uint16_t))); \
            return true;                                                                                                          \
        }();                                                                                                                      \
        (void)once;                                                                                                               \
        hipLaunchKernelGGL((k_fpn_lateral<PA_, E_, D_, A_>), grid, dim3(FL_THREADS), lds, s, a);                                  \
    } while (0)
#define PH_FL_A(PA_, E_, D_)                                                                                                      \
    do {                                                                                                                          \
        if (al4) PH_FL(PA_, E_, D_, true); else PH_FL(PA_, E_, D_, false);                                                        \
    } while (0)
#define PH_FL_D(PA_, E_)                                                                                                          \
    do {                                                                                                                          \
        if (x_dtype == PH_OUT_F32) PH_FL_A(PA_, E_, PH_OUT_F32);                                                                  \
        else if (x_dtype == PH_OUT_BF16) PH_FL_A(PA_, E_, PH_OUT_BF16);                                                           \
        else PH_FL_A(PA_, E_, PH_OUT_F16);                                                                                        \
    } while (0)
    if (prec == PH_PREC_BF16) PH_FL_D(1, PH_E_BF16);
    else if (prec == PH_PREC_F16) PH_FL_D(1, PH_E_F16);
    else PH_FL_D(2, PH_E_BF16);
#undef PH_FL_D
#undef PH_FL_A
#undef PH_FL
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// ---- the lateral of a stage that is a channels-last 16-bit plane [B][HW][K] (the backbone's own, as ph_conv_cl writes it): the same
// GEMM -- tile, MFMA, B fragments, one accumulator chain per output element over ascending k, fl_epilogue -- so ph_fpn_lateral's
// bits on the NCHW form of the same values.  Channels-last makes the A fragment of a pixel 8 consecutive channels, so the chunk is
// staged [64 px][256 c] (k_conv_cl's staging at this tile) and read back with plain 16-byte LDS reads.  Row pitch 264 elements =
// 132 dwords: the 16 rows of each lane group of a 16-byte read start 4 banks apart, every group covers the 64 banks once.
constexpr int FC_LDA = FL_KC + 8;

// the four 16-byte units of this thread: rows tid / 32 + 16 q, channels 8 (tid % 32) ..; every load is unconditional and inside the
// plane: a row past HW is clamped to the last pixel (its output is never written, and no other row's output reads it), a unit past
// K -- the last chunk of a K that is no multiple of 256 -- to the row's last unit (the k-loop never reads it)
__device__ __forceinline__ void fc_load(uint4 (&v)[4], const uint16_t* src, int K, int64_t HW, int k0, int64_t px0, int tid) {
    int c = k0 + (tid & 31) * 8;
    if (c > K - 8) c = K - 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int64_t px = px0 + (tid >> 5) + 16 * q;
        if (px > HW - 1) px = HW - 1;
        v[q] = ld_nt16(src + px * K + c);
    }
}

// format XE -> fp32 -> format E (fl_store's conversion of the fp32 stage); the same format passes through
template <int XE, int E> __device__ __forceinline__ uint32_t fc_cv2(uint32_t w) {
    if constexpr (XE == E) return w;
    else return pack2(f2e<E>(e2f<XE>(w & 0xFFFFu)), f2e<E>(e2f<XE>(w >> 16)));
}

template <int XE, int E>
__global__ __launch_bounds__(FL_THREADS) void k_fpn_lateral_cl(const FLArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.y, K = a.K;
    const int64_t HW = (int64_t)a.H * a.W, px0 = (int64_t)blockIdx.x * FL_T;
    const uint16_t* src = (const uint16_t*)a.x + (int64_t)b * HW * K;
    const uint16_t* wrow = a.w + ((int64_t)wave * (K / 16) * 64 + lane) * 8;

    f32x16_t acc[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;

    uint4 v[4];
    fc_load(v, src, K, HW, 0, px0, tid);
    for (int k0 = 0; k0 < K; k0 += FL_KC) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(uint4*)(lds + ((tid >> 5) + 16 * q) * FC_LDA + (tid & 31) * 8) =
                make_uint4(fc_cv2<XE, E>(v[q].x), fc_cv2<XE, E>(v[q].y), fc_cv2<XE, E>(v[q].z), fc_cv2<XE, E>(v[q].w));
        __syncthreads();
        if (k0 + FL_KC < K) fc_load(v, src, K, HW, k0 + FL_KC, px0, tid);                // in flight during the MFMAs (uniform branch)
        const int nks = (K - k0 < FL_KC ? K - k0 : FL_KC) / 16;                          // K % 64 == 0: a multiple of 4
        const uint16_t* wk = wrow + (int64_t)(k0 / 16) * 512;
        for (int ks4 = 0; ks4 < nks; ks4 += 4) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ks = ks4 + kk;
                const uint4 wf = *(const uint4*)(wk + (int64_t)ks * 512);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const uint4 xf = *(const uint4*)(lds + (ct * 32 + l32) * FC_LDA + ks * 16 + g * 8);
                    acc[ct] = mfma32e<E>(xf, wf, acc[ct]);
                }
            }
        }
    }

    fl_epilogue<1, E>(a, acc, lds, b, HW, px0, tid, lane, wave, g);
}

extern "C" int ph_fpn_lateral_cl(const uint16_t* X, int x_prec, const uint16_t* Wp, int64_t w_plane_elems, const float* bias,
                                 const uint16_t* coarse, int Hc, int Wc, uint16_t* out, int B, int K, int H, int W, int prec,
                                 void* stream) {
    PH_CHECK_ARG(X && Wp && bias && out, "null pointer (X, Wp, bias, out)");
    PH_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= (int64_t)FL_T * 0x7FFFFFFF, "B, H, W out of range");
    PH_CHECK_ARG(K >= 64 && K <= 4096 && K % 64 == 0, "K must be a multiple of 64 in [64, 4096]");
    PH_CHECK_ARG(w_plane_elems == (int64_t)256 * K, "w_plane_elems must be 256 * K (pack_b32 fragments of W[256][K])");
    PH_CHECK_ARG(x_prec == PH_PREC_BF16 || x_prec == PH_PREC_F16, "x_prec must be PH_PREC_BF16 or PH_PREC_F16");
    if (prec == PH_PREC_SPLIT) {
        ph_set_error("%s: %s", __func__, "PH_PREC_SPLIT: the hi + lo grade takes the NCHW stage (ph_cl_to_nchw, then ph_fpn_lateral)");
        return PH_EUNSUPPORTED;
    }
    PH_CHECK_ARG(prec == PH_PREC_BF16 || prec == PH_PREC_F16, "prec must be PH_PREC_BF16 or PH_PREC_F16");
    if (coarse) {
        PH_CHECK_ARG(Hc > 0 && Wc > 0 && ph_fpn_size_rule(H, Hc) && ph_fpn_size_rule(W, Wc),
                     "coarse size: H must be 2 Hc or 2 Hc - 1 and W must be 2 Wc or 2 Wc - 1 (the sizes at which the integer nearest index is torch's)");
        PH_CHECK_ARG(((uintptr_t)coarse & 15) == 0, "coarse must be 16-byte aligned");
    }
    PH_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)Wp & 15) == 0, "X, out and Wp must be 16-byte aligned");
    FLArgs a{X, Wp, w_plane_elems, bias, coarse, out, B, K, H, W, coarse ? Hc : 1, coarse ? Wc : 1};
    const dim3 grid((unsigned)(((int64_t)H * W + FL_T - 1) / FL_T), (unsigned)B);
    constexpr size_t lds = (size_t)FL_T * FL_EP * sizeof(float);             // the epilogue tile; the staged chunk is smaller
    static_assert((size_t)FL_T * FC_LDA * sizeof(uint16_t) <= lds, "the staged chunk must fit the epilogue tile");
    hipStream_t s = (hipStream_t)stream;
#define PH_FC(XE_, E_)                                                                                                            \
    do {                                                                                                                          \
        static const bool once = [&] {                                                                                            \
            (void)hipFuncSetAttribute((const void*)k_fpn_lateral_cl<XE_, E_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            return true;                                                                                                          \
        }();                                                                                                                      \
        (void)once;                                                                                                               \
        hipLaunchKernelGGL((k_fpn_lateral_cl<XE_, E_>), grid, dim3(FL_THREADS), lds, s, a);                                       \
    } while (0)
    if (prec == PH_PREC_BF16) { if (x_prec == PH_PREC_BF16) PH_FC(PH_E_BF16, PH_E_BF16); else PH_FC(PH_E_F16, PH_E_BF16); }
    else { if (x_prec == PH_PREC_BF16) PH_FC(PH_E_BF16, PH_E_F16); else PH_FC(PH_E_F16, PH_E_F16); }
#undef PH_FC
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// fp32 NHWC [B][HW][256] + bias[256] -> fp32 NCHW [B][256][HW] through an LDS transpose (k_gn_to_nchw's shape, ph_neck.hip): a
// block takes 32 pixels x 256 channels, reads whole 1 KiB pixel vectors and writes 128-byte runs of 32 pixels per channel row
__global__ __launch_bounds__(256) void k_fpn_output(const float* __restrict__ y, const float* __restrict__ bias, float* __restrict__ out,
                                                    int64_t HW) {
    __shared__ float t[256][33];
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * 32;
    const int c4 = (threadIdx.x & 63) * 4, pq = threadIdx.x >> 6;
    const float4 bv = *(const float4*)(bias + c4);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int pl = k * 4 + pq;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p0 + pl < HW) {
            const uint4 q = ld_nt16(y + ((int64_t)b * HW + p0 + pl) * 256 + c4);
            v = make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
        }
        t[c4][pl] = v.x + bv.x; t[c4 + 1][pl] = v.y + bv.y; t[c4 + 2][pl] = v.z + bv.z; t[c4 + 3][pl] = v.w + bv.w;
    }
    __syncthreads();
    const int pl = threadIdx.x & 31, cr = threadIdx.x >> 5;       // 8 channel rows per pass
    if (p0 + pl < HW) {
#pragma unroll 4
        for (int c = cr; c < 256; c += 8) out[((int64_t)b * 256 + c) * HW + p0 + pl] = t[c][pl];
    }
}

extern "C" int ph_fpn_output(const float* y, const float* bias, float* out, int B, int64_t HW, void* stream) {
    PH_CHECK_ARG(y && bias && out, "null pointer (y, bias, out)");
    PH_CHECK_ARG(B > 0 && B <= 65535 && HW > 0 && HW <= (int64_t)32 * 0x7FFFFFFF, "B, HW out of range");
    PH_CHECK_ARG(((uintptr_t)y & 15) == 0 && ((uintptr_t)bias & 15) == 0, "y and bias must be 16-byte aligned");
    hipLaunchKernelGGL(k_fpn_output, dim3((unsigned)((HW + 31) / 32), (unsigned)B), dim3(256), 0, (hipStream_t)stream, y, bias, out, HW);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

// ---- the direct hand-over to the neck: the tail of an output conv that writes the neck's conv-input planes itself, so the fp32 NCHW
// level does not cross memory twice on its way there (ph_fpn_output writes it, ph_nhwc_ingest reads it back).  One block = 32 pixels
// x 256 channels, k_fpn_output's tile: y is read once as whole 1 KiB pixel vectors, v = y + bias goes to LDS as [channel][pixel];
// a channel-row pass then writes the fp32 NCHW level (128-byte runs of 32 pixels, k_fpn_output's stores and bits) and / or adds the
// positional encoding ([256][HW], the same runs) in place; the last pass rounds once and writes whole 128-byte lines of planes:
//   channels-last [P][B][HW][256]: 8 lanes x 16 bytes = 64 channels of a pixel (k_nhwc_ingest_v4's stores), a wave = 8 pixels
//   PH_PLANES_C16 [B][16][HW][16]: a wave = the 32 pixels of one 16-channel chunk, 1 KiB of consecutive bytes
// The arithmetic is ph_nhwc_ingest's on ph_fpn_output's value: (y + bias) rounded to fp32, + add, one rounding to 16 bits.
// `zadd`: ph_nhwc_ingest's 16-byte form (HW % 4 == 0) adds a zero where there is no table, which turns -0 into +0; the same here.
#pragma clang fp contract(off)
template <int PA, int E, bool C16>
__global__ __launch_bounds__(256) void k_fpn_output_planes(const float* __restrict__ y, const float* __restrict__ bias,
                                                           const float* __restrict__ add, uint16_t* __restrict__ planes,
                                                           float* __restrict__ outf, int B, int64_t HW, int zadd) {
    __shared__ float t[256][33];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 32;
    {
        const int c4 = (tid & 63) * 4, pq = tid >> 6;
        const float4 bv = *(const float4*)(bias + c4);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int pl = k * 4 + pq;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p0 + pl < HW) {
                const uint4 q = ld_nt16(y + ((int64_t)b * HW + p0 + pl) * 256 + c4);
                v = make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
            }
            t[c4][pl] = v.x + bv.x; t[c4 + 1][pl] = v.y + bv.y; t[c4 + 2][pl] = v.z + bv.z; t[c4 + 3][pl] = v.w + bv.w;
        }
    }
    __syncthreads();
    if (outf || add) {                                            // uniform: kernel arguments
        const int pl = tid & 31, cr = tid >> 5;                   // 8 channel rows per pass; a thread rewrites its own elements only
        if (p0 + pl < HW) {
#pragma unroll 4
            for (int c = cr; c < 256; c += 8) {
                const float v = t[c][pl];
                if (outf) outf[((int64_t)b * 256 + c) * HW + p0 + pl] = v;
                if (add) t[c][pl] = v + add[(int64_t)c * HW + p0 + pl];
            }
        }
        __syncthreads();
    }
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t plane = (int64_t)B * HW * 256;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // channels-last: 64 channels of wave `wave`, pixels 8 k .. 8 k + 7;  C16: chunk 4 k + wave, all 32 pixels
        const int px = C16 ? lane >> 1 : k * 8 + (lane >> 3);
        const int c0 = C16 ? (k * 4 + wave) * 16 + (lane & 1) * 8 : wave * 64 + (lane & 7) * 8;
        if (p0 + px >= HW) continue;
        uint32_t hi[8], lo[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float s = t[c0 + e][px];
            if (zadd) s += 0.f;
            f2e_split<E>(s, hi[e], lo[e]);
        }
        uint16_t* d = C16 ? planes + (((int64_t)b * 16 + (c0 >> 4)) * HW + p0 + px) * 16 + (c0 & 15)
                          : planes + ((int64_t)b * HW + p0 + px) * 256 + c0;
        *(uint4*)d = make_uint4(pack2(hi[0], hi[1]), pack2(hi[2], hi[3]), pack2(hi[4], hi[5]), pack2(hi[6], hi[7]));
        if (PA == 2) *(uint4*)(d + plane) = make_uint4(pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(lo[4], lo[5]), pack2(lo[6], lo[7]));
    }
}

extern "C" int ph_fpn_output_planes(const float* y, const float* bias, const float* add, uint16_t* planes, float* out_f32, int B,
                                    int64_t HW, int prec, void* stream) {
    PH_CHECK_ARG(y && bias && planes, "null pointer (y, bias, planes)");
    const bool c16 = (prec & PH_PLANES_C16) != 0;
    prec &= ~PH_PLANES_C16;
    PH_CHECK_ARG(prec == PH_PREC_BF16 || prec == PH_PREC_SPLIT || prec == PH_PREC_F16, "prec must be PH_PREC_BF16, PH_PREC_SPLIT or PH_PREC_F16");
    PH_CHECK_ARG(!c16 || prec != PH_PREC_SPLIT, "PH_PLANES_C16 output: one-plane formats only");
    PH_CHECK_ARG(B > 0 && B <= 65535 && HW > 0 && HW <= (int64_t)32 * 0x7FFFFFFF, "B, HW out of range");
    PH_CHECK_ARG(((uintptr_t)y & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)planes & 15) == 0,
                 "y, bias and planes must be 16-byte aligned");
    PH_CHECK_ARG(((uintptr_t)add & 3) == 0 && ((uintptr_t)out_f32 & 3) == 0, "add and out_f32 must be 4-byte aligned");
    const dim3 grid((unsigned)((HW + 31) / 32), (unsigned)B);
    const int zadd = !add && (HW & 3) == 0;
    hipStream_t s = (hipStream_t)stream;
#define PH_FOP(PA_, E_, C_) hipLaunchKernelGGL((k_fpn_output_planes<PA_, E_, C_>), grid, dim3(256), 0, s, y, bias, add, planes, out_f32, B, HW, zadd)
    if (prec == PH_PREC_SPLIT) PH_FOP(2, PH_E_BF16, false);
    else if (prec == PH_PREC_F16) { if (c16) PH_FOP(1, PH_E_F16, true); else PH_FOP(1, PH_E_F16, false); }
    else { if (c16) PH_FOP(1, PH_E_BF16, true); else PH_FOP(1, PH_E_BF16, false); }
#undef PH_FOP
    PH_CHECK_LAUNCH();
    return PH_OK;
}
