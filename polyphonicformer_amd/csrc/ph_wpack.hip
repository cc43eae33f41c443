// The weight packs of the native KernelHead, neck and association plans (ph_khead_pack, ph_neck_pack, ph_track_pack) are written by
// ONE kernel from a table of pieces (ph_common.h PhPackTable).  The decode plan's packer (ph_decode.hip k_decode_pack) folds
// matrices in fp64 and is a different algorithm.
#include "ph_common.h"

#pragma clang fp contract(off)

// one 16-bit value of plane `lo` (0 = hi): fp16 has one plane, the bf16 form splits w into hi + lo
__device__ __forceinline__ uint32_t wp_cvt(float w, bool f16, bool lo) {
    if (f16) return f2h(w);
    uint32_t h, l;
    f2bf_split(w, h, l);
    return lo ? l : h;
}

__device__ __forceinline__ uint4 wp_copy4(const float* src) {
    return make_uint4(__float_as_uint(src[0]), __float_as_uint(src[1]), __float_as_uint(src[2]), __float_as_uint(src[3]));
}

// k_pack_pieces: every 16-byte unit of the pack is written by one thread (one 16-byte store; the alignment padding as zeros, so two
// packings of the same weights are byte-equal).  A unit is 8 consecutive 16-bit values or 4 floats, and in every piece those come
// from ONE parameter row: `step` floats apart in a tap-permuted fragment (the parameter is [row][c][tap]), consecutive otherwise.
// The stores are whole 128-byte lines per 8 lanes; the gather is not coalesced, which a once-per-weight-load kernel can afford.
__global__ __launch_bounds__(256) void k_pack_pieces(const PhPackTable t, uint4* __restrict__ pack) {
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < t.total_u; u += gridDim.x * 256u) {
        int k = 0;
        for (int i = 1; i < t.npieces; ++i)
            if (u >= t.pc[i].u0) k = i;          // an empty piece shares its start with its successor, which wins
        const PhPackPiece pc = t.pc[k];
        const uint32_t lu = u - pc.u0;
        uint4 out = make_uint4(0u, 0u, 0u, 0u);
        if (lu < pc.nvalid) {
            if (pc.kind == PH_PIECE_F32) {
                out = wp_copy4(t.p[pc.first] + (size_t)lu * 4u);
            } else if (pc.kind == PH_PIECE_GN) {     // [3][2][256]: (gamma, beta) of map m = parameters first + 3 m + 1, + 2
                const uint32_t i = lu * 4u, m = i >> 9, wb = (i >> 8) & 1u, c = i & 255u;
                out = wp_copy4(t.p[pc.first + 3u * m + 1u + wb] + c);
            } else if (pc.kind == PH_PIECE_BIAS) {   // a bias vector, zero beyond its valid entries
                uint32_t v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t i = lu * 4u + e;
                    v[e] = i < pc.rows_valid ? __float_as_uint(t.p[pc.first][i]) : 0u;
                }
                out = make_uint4(v[0], v[1], v[2], v[3]);
            } else {                                 // 16-bit planes: [P][nmat] matrices of rows x K, W2[row][k] of each in `kind`'s order
                const uint32_t mat = pc.rows * pc.K, per = mat * pc.nmat;
                const uint32_t e0 = lu * 8u, pl = e0 / per, r0 = e0 % per, m = r0 / mat, i = r0 % mat;
                uint32_t row, kk;
                if (pc.kind == PH_PIECE_PLANES) { row = i / pc.K; kk = i % pc.K; }
                else if (pc.kind == PH_PIECE_FRAG32) {   // pack.pack_b32: [ct][ks][g][n][e] holds W2[32 ct + n][16 ks + 8 g + e]
                    const uint32_t KS = pc.K / 16u, n = (i >> 3) & 31u, gq = (i >> 8) & 1u, r = i >> 9;
                    row = 32u * (r / KS) + n; kk = 16u * (r % KS) + 8u * gq;
                } else {                                 // pack.pack_b_fragments: [ct][ks][g][j][e] holds W2[16 ct + j][32 ks + 8 g + e]
                    const uint32_t KS = pc.K / 32u, j = (i >> 3) & 15u, gq = (i >> 7) & 3u, r = i >> 9;
                    row = 16u * (r / KS) + j; kk = 32u * (r % KS) + 8u * gq;
                }
                if (row < pc.rows_valid) {
                    // taps > 0: k = tap * 256 + c of a parameter stored [row][c][tap] (1x1 and 3x3 convs, tap = kh * 3 + kw; fcs.0,
                    // taps = 49: its K axis permuted from ci * 49 + pos to pos * 256 + ci); taps == 0: k as stored, [row][K]
                    const float* src = t.p[pc.first + m * pc.pstep];
                    const size_t step = pc.taps ? pc.taps : 1u;
                    src += pc.taps ? ((size_t)row * 256u + (kk & 255u)) * step + (kk >> 8) : (size_t)row * pc.K + kk;
                    uint32_t v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = wp_cvt(src[(size_t)e * step], t.f16 != 0, pl != 0);
                    out = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
                }
            }
        }
        pack[u] = out;
    }
}

int ph_pack_pieces(const char* fn, const PhPackTable& t, void* pack, unsigned max_blocks, void* stream) {
    const unsigned blocks = (t.total_u + 255u) / 256u;
    hipLaunchKernelGGL(k_pack_pieces, dim3(blocks < max_blocks ? blocks : max_blocks), dim3(256), 0, (hipStream_t)stream, t, (uint4*)pack);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ph_set_error("%s: launch failed: %s", fn, hipGetErrorString(e)); return PH_ELAUNCH; }
    return PH_OK;
}
