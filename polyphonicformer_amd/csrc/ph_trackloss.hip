// Training the track head (polyphonic/video/track_heads.py:104-162): for every key / reference image pair the QDTrack targets, the
// dot-product and cosine similarities (qdtrack/track/similarity.py), MultiPosCrossEntropyLoss (losses/multipos_cross_entropy_loss.py)
// and L2Loss with hard negative mining (losses/l2_loss.py), and d(loss_track + loss_track_aux) / d(embeddings) -- ONE workgroup per pair,
// the whole [Nk][Nr] matrix in LDS (<= 128 x 128), one tiny kernel that adds the pairs up.
//
//   d = K R^T (fp32, ascending e), a_i = max(|k_i|, 1e-12), b_j likewise, c_ij = d_ij / (a_i b_j)
//   target_ij = (gt_match[key_gt[i]] == ref_gt[j]),  w_i = any_j target_ij
//   loss_track = lw_track * sum_i w_i log(1 + sum_{neg j} sum_{pos p} exp(d_ij - d_ip)) / sum_i w_i
//   loss_aux   = lw_aux * sum_ij wt_ij (clamp(c_ij - margin_ij, 0, 1) - target_ij)^2 / #{wt > 0};  wt = 1, but when
//                num_neg > neg_pos_ub (num_pos + 1) only the num_pos * neg_pos_ub negatives of largest cost keep it
// Everything the two losses' gradients need is a gradient with respect to d plus two diagonal corrections for the normalisations:
//   T_ij = dL/dd_ij (MultiPos) + gc_ij / (a_i b_j),   gc = dL/dc (L2),   u_i = sum_j gc_ij c_ij,   v_j = sum_i gc_ij c_ij
//   g_key = T R - diag(u / a^2) K,    g_ref = T^T K - diag(v / b^2) R      (no correction for a row whose norm is below the eps)
// T overwrites d in place.  Sums that end in a loss are fp64 in a fixed order (a row per thread ascending j, then the rows ascending);
// the products are register tiled fp32 in ascending k; counts are integers.  No atomics anywhere: a second call gives the same bits,
// and a pair's numbers do not depend on which other pairs share the launch.
//
// The hard-negative cut: the k-th largest cost among the negatives by a bitwise search on the costs' bit patterns (non-negative floats
// order as their bits): 31 counting passes over the key matrix in LDS.  Ties at the cut go to the lowest row-major index i * Nr + j.
// A pair without a positive has sum w = 0 (and, when it is mined, no weight left): the divisions give inf, 0 * inf = NaN as in the
// reference, for both losses and every gradient element of the pair.
#include "ph_common.h"

namespace {

constexpr int TL_MAX = PH_TRACK_LOSS_MAX_ROIS;       // RoIs per side
constexpr int TL_T = 256;
constexpr int TL_EC = 32, TL_EP = 33;                // k per staged chunk of the d product, its LDS pitch
constexpr int TL_CB = 128;                           // embedding columns per pass of the gradient products

struct TlOffsets { int32_t key[PH_TRACK_LOSS_MAX_PAIRS + 1], ref[PH_TRACK_LOSS_MAX_PAIRS + 1], match[PH_TRACK_LOSS_MAX_PAIRS + 1]; };

struct TlSmall {                                     // the per-row / per-column records
    int kmatch[TL_MAX], rgt[TL_MAX];
    float inva[TL_MAX], invb[TL_MAX];                // 1 / max(norm, eps)
    float na2[TL_MAX], nb2[TL_MAX];                  // 1 / norm^2 where the norm is above the eps, else 0 (the normalisation's own gradient)
    float mn[TL_MAX], mp[TL_MAX], sa[TL_MAX], sb[TL_MAX];      // MultiPos row: max over negatives of d, over positives of -d, sigma / A', sigma / B'
    float wrow[TL_MAX];
    double rowd[TL_MAX];                             // a per-row fp64 partial
    float u[TL_MAX], v[TL_MAX];
    int npos[TL_MAX];
    int cnt[2][4];
    int chunk_eq[TL_T];
    // scalars (thread 0 writes, a barrier publishes)
    int num_pos, mining, kkeep, cut_idx;
    unsigned thr;
    double sumw, track_sum;
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// block-wide integer sum (exact, order free); `slot` alternates so that one barrier per call is enough
__device__ __forceinline__ int block_count(int v, TlSmall& S, int slot) {
    v = wave_sum_i(v);
    if ((threadIdx.x & 63) == 0) S.cnt[slot][threadIdx.x >> 6] = v;
    __syncthreads();
    return S.cnt[slot][0] + S.cnt[slot][1] + S.cnt[slot][2] + S.cnt[slot][3];
}

// the L2 loss's prediction of one entry: (clamped value, inside the closed clamp interval)
__device__ __forceinline__ float tl_pred(float c, bool pos, float pos_margin, float neg_margin, bool& inside) {
    const float m = pos ? (pos_margin > 0.f ? pos_margin : 0.f) : (neg_margin > 0.f ? neg_margin : 0.f);
    const float x = c - m;
    inside = x >= 0.f && x <= 1.f;
    return fminf(fmaxf(x, 0.f), 1.f);
}

// O[rows][E] = (T(^T) X - diag(corr) Y) * scale for one pair.  TR == false: O = g_key [Nk][E], T as stored [Nk][pitch], X = R [Nr][E], Y = K;
// TR == true: O = g_ref [Nr][E], T transposed, X = K [Nk][E], Y = R.  Thread (ti, tj) owns rows ti + 16 r, columns tj + 16 c of a
// 128 x 128 block; the inner index runs ascending in staged chunks of 32.
template <bool TR>
__device__ __forceinline__ void tl_grad_product(const float* Tm, int pitch, int Nk, int Nr, const float* __restrict__ X, const float* __restrict__ Y,
                                                const float* corr, float scale, float* __restrict__ O, int E, float* stage /* [32][TL_CB] */) {
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const int rows = TR ? Nr : Nk, inner = TR ? Nk : Nr;
    for (int cb = 0; cb < E; cb += TL_CB) {
        float acc[8][8];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
        for (int j0 = 0; j0 < inner; j0 += 32) {
            __syncthreads();                              // the previous chunk's reads are done
#pragma unroll
            for (int q = t; q < 32 * (TL_CB / 4); q += TL_T) {
                const int jj = q / (TL_CB / 4), c4 = q - jj * (TL_CB / 4);
                const int j = j0 + jj, e = cb + c4 * 4;
                float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j < inner && e < E) vv = *(const float4*)(X + (int64_t)j * E + e);
                *(float4*)(stage + jj * TL_CB + c4 * 4) = vv;
            }
            __syncthreads();
            const int jn = inner - j0 < 32 ? inner - j0 : 32;
            for (int jj = 0; jj < jn; ++jj) {
                float av[8], bv[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int row = ti + 16 * r;
                    av[r] = row < rows ? (TR ? Tm[(j0 + jj) * pitch + row] : Tm[row * pitch + j0 + jj]) : 0.f;
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) bv[c] = stage[jj * TL_CB + tj + 16 * c];
#pragma unroll
                for (int r = 0; r < 8; ++r)
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[r][c] += av[r] * bv[c];
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int row = ti + 16 * r;
            if (row >= rows) continue;
            const float cr = corr[row];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int e = cb + tj + 16 * c;
                if (e < E) O[(int64_t)row * E + e] = (cr != 0.f ? acc[r][c] - cr * Y[(int64_t)row * E + e] : acc[r][c]) * scale;
            }
        }
    }
}

__global__ __launch_bounds__(TL_T) void k_track_loss(ph_track_loss_cfg cfg, TlOffsets off, const float* __restrict__ key_emb,
                                                     const float* __restrict__ ref_emb, const int32_t* __restrict__ key_gt,
                                                     const int32_t* __restrict__ ref_gt, const int32_t* __restrict__ gt_match,
                                                     float* __restrict__ g_key, float* __restrict__ g_ref, double* __restrict__ rec,
                                                     int dmat_floats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tl_lds[];
    TlSmall& S = *(TlSmall*)tl_lds;
    float* D = (float*)(tl_lds + ((sizeof(TlSmall) + 15) / 16) * 16);       // [Nk][pitch]
    float* stage = D + dmat_floats;                                          // staging of the products | the key matrix of the select
    unsigned* keys = (unsigned*)stage;

    const int p = blockIdx.x, t = threadIdx.x, E = cfg.E;
    const int k0 = off.key[p], Nk = off.key[p + 1] - k0, r0 = off.ref[p], Nr = off.ref[p + 1] - r0;
    const int m0 = off.match[p], nm = off.match[p + 1] - m0;
    const int pitch = Nr | 1, total = Nk * Nr;
    const float* K = key_emb + (int64_t)k0 * E;
    const float* R = ref_emb + (int64_t)r0 * E;

    // ---- rows: matched reference ground truth of every key RoI, norms (fp64, ascending e)
    if (t < TL_MAX) {
        if (t < Nk) {
            const int g = key_gt[k0 + t];
            S.kmatch[t] = (g >= 0 && g < nm) ? gt_match[m0 + g] : INT32_MIN;
            double s = 0.0;
            for (int e = 0; e < E; e += 4) {
                const float4 q = *(const float4*)(K + (int64_t)t * E + e);
                s += (double)q.x * q.x; s += (double)q.y * q.y; s += (double)q.z * q.z; s += (double)q.w * q.w;
            }
            const float nrm = (float)sqrt(s);
            S.inva[t] = 1.f / fmaxf(nrm, 1e-12f);
            S.na2[t] = nrm > 1e-12f ? (float)(1.0 / s) : 0.f;
        }
    } else {
        const int j = t - TL_MAX;
        if (j < Nr) {
            S.rgt[j] = ref_gt[r0 + j];
            double s = 0.0;
            for (int e = 0; e < E; e += 4) {
                const float4 q = *(const float4*)(R + (int64_t)j * E + e);
                s += (double)q.x * q.x; s += (double)q.y * q.y; s += (double)q.z * q.z; s += (double)q.w * q.w;
            }
            const float nrm = (float)sqrt(s);
            S.invb[j] = 1.f / fmaxf(nrm, 1e-12f);
            S.nb2[j] = nrm > 1e-12f ? (float)(1.0 / s) : 0.f;
        }
    }

    // ---- d = K R^T: thread (ti, tj) owns rows ti + 16 r, columns tj + 16 c; chunks of 32 k staged [row][33]
    {
        const int ti = t >> 4, tj = t & 15;
        float* Ks = stage;
        float* Rs = stage + TL_MAX * TL_EP;
        float acc[8][8];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
        for (int e0 = 0; e0 < E; e0 += TL_EC) {
            __syncthreads();
#pragma unroll
            for (int q = t; q < TL_MAX * (TL_EC / 4); q += TL_T) {
                const int row = q >> 3, c4 = q & 7, e = e0 + c4 * 4;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (e < E) {
                    if (row < Nk) a = *(const float4*)(K + (int64_t)row * E + e);
                    if (row < Nr) b = *(const float4*)(R + (int64_t)row * E + e);
                }
                float* ka = Ks + row * TL_EP + c4 * 4;
                float* rb = Rs + row * TL_EP + c4 * 4;
                ka[0] = a.x; ka[1] = a.y; ka[2] = a.z; ka[3] = a.w;
                rb[0] = b.x; rb[1] = b.y; rb[2] = b.z; rb[3] = b.w;
            }
            __syncthreads();
#pragma unroll 4
            for (int e = 0; e < TL_EC; ++e) {
                float av[8], bv[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) av[r] = Ks[(ti + 16 * r) * TL_EP + e];
#pragma unroll
                for (int c = 0; c < 8; ++c) bv[c] = Rs[(tj + 16 * c) * TL_EP + e];
#pragma unroll
                for (int r = 0; r < 8; ++r)
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[r][c] += av[r] * bv[c];
            }
        }
        __syncthreads();                                  // the staging buffer becomes the key matrix below
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int row = ti + 16 * r, col = tj + 16 * c;
                if (row < Nk && col < Nr) D[row * pitch + col] = acc[r][c];
            }
    }
    __syncthreads();

    // ---- the select's keys: bits of the squared clamped cost + 1 for a negative, 0 for a positive
    for (int idx = t; idx < total; idx += TL_T) {
        const int i = idx / Nr, j = idx - i * Nr;
        const bool pos = S.kmatch[i] == S.rgt[j];
        bool in;
        const float pr = tl_pred(D[i * pitch + j] * S.inva[i] * S.invb[j], pos, cfg.pos_margin, cfg.neg_margin, in);
        keys[idx] = pos ? 0u : __float_as_uint(pr * pr) + 1u;
    }
    // ---- MultiPos rows (a row per thread, fp64): L_i = softplus(m_n + m_p + log(A' B'))
    if (t < Nk) {
        const int i = t;
        const float* d = D + i * pitch;
        const int km = S.kmatch[i];
        int np = 0;
        float mn = -INFINITY, mp = -INFINITY;
        for (int j = 0; j < Nr; ++j) {
            if (km == S.rgt[j]) { ++np; mp = fmaxf(mp, -d[j]); } else mn = fmaxf(mn, d[j]);
        }
        double L = 0.0;
        float sa = 0.f, sb = 0.f;
        if (np > 0 && np < Nr) {
            double A = 0.0, B = 0.0;
            for (int j = 0; j < Nr; ++j) {
                if (km == S.rgt[j]) B += exp((double)(-d[j]) - (double)mp); else A += exp((double)d[j] - (double)mn);
            }
            const double tt = (double)mn + (double)mp + log(A * B);
            L = tt > 0.0 ? tt + log1p(exp(-tt)) : log1p(exp(tt));
            const double sg = 1.0 / (1.0 + exp(-tt));
            sa = (float)(sg / A); sb = (float)(sg / B);
        }
        S.npos[i] = np;
        S.wrow[i] = np > 0 ? 1.f : 0.f;
        S.rowd[i] = np > 0 ? L : 0.0;
        S.mn[i] = mn; S.mp[i] = mp; S.sa[i] = sa; S.sb[i] = sb;
    }
    __syncthreads();
    if (t == 0) {
        int npos = 0;
        double sumw = 0.0, track_sum = 0.0;
        for (int i = 0; i < Nk; ++i) { npos += S.npos[i]; sumw += (double)S.wrow[i]; track_sum += S.rowd[i]; }
        S.sumw = sumw; S.track_sum = track_sum;
        const int nneg = total - npos;
        S.num_pos = npos;
        S.mining = cfg.neg_pos_ub > 0 && (int64_t)nneg > (int64_t)cfg.neg_pos_ub * (npos + 1);      // num_neg / (num_pos + 1) > neg_pos_ub
        S.kkeep = S.mining ? npos * cfg.neg_pos_ub : nneg;
        S.cut_idx = INT32_MAX;
        S.thr = 1u;                                       // no mining: every negative (key >= 1)
    }
    __syncthreads();

    // ---- hard negatives: the kkeep-th largest key, bit by bit; ties at the cut to the lowest row-major index
    if (S.mining) {                                       // uniform
        const int kk = S.kkeep;
        unsigned thr = 0xFFFFFFFFu;                       // kk == 0: nothing is kept
        if (kk > 0) {
            thr = 0u;
            int slot = 0;
            for (int bit = 30; bit >= 0; --bit) {         // keys <= bits(1.0f) + 1 < 2^30 + 2^29
                const unsigned cand = thr | (1u << bit);
                int c = 0;
                for (int idx = t; idx < total; idx += TL_T) c += keys[idx] >= cand;
                if (block_count(c, S, slot) >= kk) thr = cand;
                slot ^= 1;
            }
            int cg = 0, ce = 0;
            const int chunk = (total + TL_T - 1) / TL_T, i0 = t * chunk, i1 = i0 + chunk < total ? i0 + chunk : total;
            for (int idx = i0; idx < i1; ++idx) { cg += keys[idx] > thr; ce += keys[idx] == thr; }
            S.chunk_eq[t] = ce;
            const int gt_total = block_count(cg, S, slot);          // its barrier publishes chunk_eq too
            const int need = kk - gt_total;                         // >= 1 ties to keep
            int before = 0;
            for (int q = 0; q < t; ++q) before += S.chunk_eq[q];
            if (before < need && before + ce >= need) {             // exactly one thread: the need-th tie lies in its chunk
                int seen = before;
                for (int idx = i0; idx < i1; ++idx)
                    if (keys[idx] == thr && ++seen == need) { S.cut_idx = idx; break; }
            }
        }
        if (t == 0) S.thr = thr;
        __syncthreads();
    }
    const unsigned thr = S.thr;
    const int cut = S.cut_idx;
    const double avg = (double)S.num_pos + (double)S.kkeep;        // #{weight > 0}
    // d loss / d (row loss) and d loss / d (weighted squared error): inf for an empty normaliser, and 0 * inf = NaN below, as in the reference
    // (the 1 / pairs of the mean over the pairs is ONE fp32 multiplication of the finished gradient rows, so a pair's rows in a joint
    // call are its single-pair call's rows times float(1 / pairs), bit for bit)
    const float coefT = (float)((double)cfg.lw_track / S.sumw);
    const float coefA = (float)((double)cfg.lw_aux / avg);
    const float inv_pairs = (float)(1.0 / (double)cfg.pairs);
    auto kept = [&](int idx, unsigned key) { return key > thr || (key == thr && idx <= cut); };

    // ---- L2 rows (thread i) and columns (thread 128 + j): the loss's row sums (fp64), u_i and v_j
    if (t < TL_MAX) {
        if (t < Nk) {
            const int i = t;
            double ls = 0.0, us = 0.0;
            for (int j = 0; j < Nr; ++j) {
                const bool pos = S.kmatch[i] == S.rgt[j];
                const float c = D[i * pitch + j] * S.inva[i] * S.invb[j];
                bool in;
                const float pr = tl_pred(c, pos, cfg.pos_margin, cfg.neg_margin, in);
                const float wt = (pos || kept(i * Nr + j, keys[i * Nr + j])) ? 1.f : 0.f;
                const float df = pr - (pos ? 1.f : 0.f);
                ls += (double)wt * ((double)df * (double)df);
                const float gc = coefA * (wt * 2.f * df * (in ? 1.f : 0.f));
                us += (double)gc * (double)c;
            }
            S.rowd[i] = ls;
            S.u[i] = (float)us * S.na2[i];
        }
    } else {
        const int j = t - TL_MAX;
        if (j < Nr) {
            double vs = 0.0;
            for (int i = 0; i < Nk; ++i) {
                const bool pos = S.kmatch[i] == S.rgt[j];
                const float c = D[i * pitch + j] * S.inva[i] * S.invb[j];
                bool in;
                const float pr = tl_pred(c, pos, cfg.pos_margin, cfg.neg_margin, in);
                const float wt = (pos || kept(i * Nr + j, keys[i * Nr + j])) ? 1.f : 0.f;
                const float gc = coefA * (wt * 2.f * (pr - (pos ? 1.f : 0.f)) * (in ? 1.f : 0.f));
                vs += (double)gc * (double)c;
            }
            S.v[j] = (float)vs * S.nb2[j];
        }
    }
    __syncthreads();
    if (t == 0) {
        double aux = 0.0;
        for (int i = 0; i < Nk; ++i) aux += S.rowd[i];
        double* o = rec + (int64_t)p * 4;
        o[0] = S.track_sum; o[1] = S.sumw; o[2] = aux; o[3] = avg;
    }
    if (!g_key) return;                                   // uniform

    // ---- T over d, in place
    for (int idx = t; idx < total; idx += TL_T) {
        const int i = idx / Nr, j = idx - i * Nr;
        const bool pos = S.kmatch[i] == S.rgt[j];
        const float d = D[i * pitch + j];
        const float c = d * S.inva[i] * S.invb[j];
        bool in;
        const float pr = tl_pred(c, pos, cfg.pos_margin, cfg.neg_margin, in);
        const float wt = (pos || kept(idx, keys[idx])) ? 1.f : 0.f;
        const float gc = coefA * (wt * 2.f * (pr - (pos ? 1.f : 0.f)) * (in ? 1.f : 0.f));
        const float sm = pos ? -expf(-d - S.mp[i]) * S.sb[i] : expf(d - S.mn[i]) * S.sa[i];       // sa = sb = 0: a row without a pair
        const float gm = coefT * (S.wrow[i] * ((S.sa[i] != 0.f || S.sb[i] != 0.f) ? sm : 0.f));
        D[i * pitch + j] = gm + gc * S.inva[i] * S.invb[j];
    }
    // ---- g_key = T R - diag(u) K, g_ref = T^T K - diag(v) R (the products' first barrier orders T and ends the key matrix's life)
    tl_grad_product<false>(D, pitch, Nk, Nr, R, K, S.u, inv_pairs, g_key + (int64_t)k0 * E, E, stage);
    tl_grad_product<true>(D, pitch, Nk, Nr, K, R, S.v, inv_pairs, g_ref + (int64_t)r0 * E, E, stage);
}

// the pairs in index order: both losses, weighted and divided by the number of pairs
__global__ void k_track_loss_finish(ph_track_loss_cfg cfg, const double* __restrict__ rec, float* __restrict__ losses) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double lt = 0.0, la = 0.0;
    for (int p = 0; p < cfg.pairs; ++p) {
        lt += (double)cfg.lw_track * (rec[p * 4 + 0] / rec[p * 4 + 1]);
        la += (double)cfg.lw_aux * (rec[p * 4 + 2] / rec[p * 4 + 3]);
    }
    losses[0] = (float)(lt / (double)cfg.pairs);
    losses[1] = (float)(la / (double)cfg.pairs);
}

size_t tl_lds_bytes(int max_nk, int max_nr, int* dmat_floats) {
    const int dm = (max_nk * (max_nr | 1) + 3) / 4 * 4;
    const size_t stage = (size_t)2 * TL_MAX * TL_EP;                       // the d product's staging (>= 32 * TL_CB, the gradients')
    const size_t keys = (size_t)max_nk * max_nr;
    *dmat_floats = dm;
    return ((sizeof(TlSmall) + 15) / 16) * 16 + ((size_t)dm + (stage > keys ? stage : keys)) * sizeof(float);
}

}  // namespace

extern "C" size_t ph_track_loss_scratch_bytes(const ph_track_loss_cfg* cfg, int total_key, int total_ref) {
    if (!cfg || cfg->pairs <= 0 || cfg->pairs > PH_TRACK_LOSS_MAX_PAIRS || total_key < 0 || total_ref < 0) {
        ph_set_error("ph_track_loss_scratch_bytes: 1 .. %d pairs", PH_TRACK_LOSS_MAX_PAIRS);
        return 0;
    }
    return al256((size_t)cfg->pairs * 4 * sizeof(double));
}

extern "C" int ph_track_loss(const ph_track_loss_cfg* cfg, const float* key_emb, const float* ref_emb, const int32_t* key_start,
                             const int32_t* ref_start, const int32_t* key_gt, const int32_t* ref_gt, const int32_t* match_start,
                             const int32_t* gt_match, float* losses, float* g_key, float* g_ref, void* scratch, size_t scratch_bytes,
                             void* stream) {
    PH_CHECK_ARG(cfg && key_emb && ref_emb && key_start && ref_start && key_gt && ref_gt && match_start && gt_match && losses && scratch,
                 "null pointer");
    PH_CHECK_ARG((g_key == nullptr) == (g_ref == nullptr), "g_key and g_ref are nullable together");
    PH_CHECK_ARG(cfg->pairs > 0 && cfg->pairs <= PH_TRACK_LOSS_MAX_PAIRS, "1 .. 64 pairs per call");
    PH_CHECK_ARG(cfg->E > 0 && cfg->E % 4 == 0, "the embedding width must be a multiple of 4");
    PH_CHECK_ARG((((uintptr_t)key_emb | (uintptr_t)ref_emb | (uintptr_t)scratch) & 15) == 0, "embeddings and scratch must be 16-byte aligned");
    PH_CHECK_ARG(cfg->hard_mining != 0 || cfg->neg_pos_ub <= 0, "neg_pos_ub > 0 needs hard_mining (the random choice of negatives is not implemented)");
    TlOffsets off;
    int max_nk = 0, max_nr = 0;
    for (int p = 0; p <= cfg->pairs; ++p) { off.key[p] = key_start[p]; off.ref[p] = ref_start[p]; off.match[p] = match_start[p]; }
    PH_CHECK_ARG(off.key[0] >= 0 && off.ref[0] >= 0 && off.match[0] >= 0, "negative offset");
    for (int p = 0; p < cfg->pairs; ++p) {
        const int nk = off.key[p + 1] - off.key[p], nr = off.ref[p + 1] - off.ref[p];
        PH_CHECK_ARG(nk >= 1 && nr >= 1, "a pair needs at least one RoI on either side");
        PH_CHECK_ARG(nk <= TL_MAX && nr <= TL_MAX, "at most 128 RoIs per side and pair");
        PH_CHECK_ARG(off.match[p + 1] >= off.match[p], "match_start must not decrease");
        max_nk = nk > max_nk ? nk : max_nk;
        max_nr = nr > max_nr ? nr : max_nr;
    }
    if (scratch_bytes < ph_track_loss_scratch_bytes(cfg, off.key[cfg->pairs], off.ref[cfg->pairs])) {
        ph_set_error("ph_track_loss: scratch too small");
        return PH_EWORKSPACE;
    }
    int dm;
    const size_t lds = tl_lds_bytes(max_nk, max_nr, &dm);
    static const hipError_t attr = hipFuncSetAttribute((const void*)k_track_loss, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (attr != hipSuccess || lds > 160 * 1024) { ph_set_error("ph_track_loss: %zu bytes of LDS are not available", lds); return PH_EUNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    double* rec = (double*)scratch;
    hipLaunchKernelGGL(k_track_loss, dim3(cfg->pairs), dim3(TL_T), lds, s, *cfg, off, key_emb, ref_emb, key_gt, ref_gt, gt_match, g_key, g_ref,
                       rec, dm);
    hipLaunchKernelGGL(k_track_loss_finish, dim3(1), dim3(64), 0, s, *cfg, (const double*)rec, losses);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
