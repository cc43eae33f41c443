// libpolyhead: the training step's Hungarian assignment and its target descriptors ON THE DEVICE (include/polyhead.h ph_assign_*).
// The host path is losses.assign_batch (a synchronising cost download + scipy.optimize.linear_sum_assignment per image) followed by
// losses.build_desc (numpy pointer tables, one upload).  Here k_assign_solve restates scipy's shortest-augmenting-path solver
// (scipy/optimize/rectangular_lsap/rectangular_lsap.cpp) in fp64 with its operation order, its left-to-right scan of `remaining` and
// its swap-remove, so that ties fall as they do there, and k_assign_desc writes the blob build_desc would have written, byte for
// byte.  Everything the host has to know -- section sizes, the positive count -- follows from the ground-truth counts alone
// (ph_assign_desc_layout), so nothing is downloaded.
//
// k_assign_solve: one workgroup of ONE wave per image (latency-bound by design, like k_dtrk_assign).  Position `it` of `remaining`
// belongs to lane it % 64; a row scan is one pass of the lanes over their positions and a 64-lane butterfly that takes the minimum
// under scipy's tie rule: among the positions that hold the minimum, the LARGEST unassigned one, else the SMALLEST.  Every loop is
// bounded by the matrix size.  k_assign_desc: one workgroup per image; every byte of the blob has exactly one writer.
#include "ph_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AS_MAX = 256;                              // max(Np, G_b)
constexpr int AS_TILE = 12288;                           // cost entries kept in LDS (48 KB); larger matrices are read from global memory
constexpr int NSEC = 13;
enum { GT_G = 0, GT_S = 1, GT_MASK = 2, GT_SEM = 3, GT_VALID = 4, GT_DEPTH = 5, GT_LAB = 6, GT_CLS = 7 };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// scipy's choice between two candidates of one scan: (sp, unassigned, position in `remaining`); pos < 0: no candidate
__device__ __forceinline__ bool better(double as, int au, int ap, double bs, int bu, int bp) {
    if (ap < 0) return false;
    if (bp < 0) return true;
    if (as < bs) return true;
    if (bs < as) return false;
    if (au != bu) return au > bu;
    return au ? ap > bp : ap < bp;
}

__global__ __launch_bounds__(64) void k_assign_solve(const float* __restrict__ cost, int Np, int ldg, const int32_t* __restrict__ counts,
                                                     int64_t count_stride, int32_t* __restrict__ match, int64_t* __restrict__ status) {
    __shared__ double u[AS_MAX], v[AS_MAX], sp[AS_MAX];
    __shared__ int path[AS_MAX], row4col[AS_MAX], col4row[AS_MAX], remaining[AS_MAX];
    __shared__ unsigned char SR[AS_MAX], SC[AS_MAX];
    __shared__ float tile[AS_TILE];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int G = clampi(counts[b * count_stride], 0, ldg);
    const float* c = cost + (size_t)b * Np * ldg;
    int32_t* mt = match + (size_t)b * ldg;
    if (G == 0) {
        if (lane == 0) status[b] = PH_ASSIGN_OK;
        return;
    }
    const bool tr = G < Np;                              // scipy transposes iff there are strictly fewer columns than rows
    const int nr = tr ? G : Np, nc = tr ? Np : G;
    const bool in_lds = nr * nc <= AS_TILE;
    // a non-finite entry (scipy raises): the status word and the trivial matching, so that the tables behind stay well formed
    int bad = 0;
    for (int e = lane; e < Np * G; e += 64) {
        const int p = e / G, g = e - p * G;
        const float x = c[(size_t)p * ldg + g];
        bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1 : 0;
        if (in_lds) tile[tr ? g * nc + p : p * nc + g] = x;      // tile[i][j]: row i of the (transposed) problem contiguous
    }
    if (__ballot(bad) != 0ull) {
        for (int g = lane; g < G; g += 64) mt[g] = g < Np ? g : -1;
        if (lane == 0) status[b] = PH_ASSIGN_ENONFINITE;
        return;
    }
    for (int i = lane; i < nr; i += 64) { u[i] = 0.0; col4row[i] = -1; }
    for (int j = lane; j < nc; j += 64) { v[j] = 0.0; row4col[j] = -1; }
    __syncthreads();
    int failed = 0;
    for (int cur = 0; cur < nr && !failed; ++cur) {
        for (int j = lane; j < nc; j += 64) { sp[j] = INFINITY; path[j] = -1; SC[j] = 0; remaining[j] = nc - j - 1; }
        for (int i = lane; i < nr; i += 64) SR[i] = 0;
        __syncthreads();
        int nrem = nc, i = cur, sink = -1;
        double minv = 0.0;
        for (int step = 0; step < nc && sink < 0; ++step) {          // at most nc selections per row
            if (lane == 0) SR[i] = 1;
            const double ui = u[i];
            double bs = INFINITY;
            int bu = 0, bp = -1;
            for (int it = lane; it < nrem; it += 64) {
                const int j = remaining[it];
                const float cf = in_lds ? tile[i * nc + j] : (tr ? c[(size_t)j * ldg + i] : c[(size_t)i * ldg + j]);
                double r = minv + (double)cf;                        // left to right, every result rounded on its own
                r = r - ui;
                r = r - v[j];
                double s = sp[j];
                if (r < s) { path[j] = i; sp[j] = r; s = r; }
                const int un = row4col[j] == -1 ? 1 : 0;
                if (better(s, un, it, bs, bu, bp)) { bs = s; bu = un; bp = it; }
            }
            for (int m = 1; m < 64; m <<= 1) {
                const double os = __shfl_xor(bs, m, 64);
                const int ou = __shfl_xor(bu, m, 64), op = __shfl_xor(bp, m, 64);
                if (better(os, ou, op, bs, bu, bp)) { bs = os; bu = ou; bp = op; }
            }
            if (bp < 0 || bp >= nrem) { failed = 1; break; }         // uniform; cannot happen while nrem >= 1
            minv = bs;
            const int j = remaining[bp];
            const int r4 = row4col[j];
            const int tail = remaining[nrem - 1];
            __syncthreads();
            if (lane == 0) { SC[j] = 1; remaining[bp] = tail; }      // scipy's swap-remove: the positions of the others stay
            --nrem;
            if (r4 == -1) sink = j; else i = r4;
            __syncthreads();
        }
        if (sink < 0) { failed = 1; break; }
        if (lane == 0) u[cur] = u[cur] + minv;
        for (int i2 = lane; i2 < nr; i2 += 64) {
            const int cj = col4row[i2];
            if (SR[i2] && i2 != cur && cj >= 0) u[i2] = u[i2] + (minv - sp[cj]);
        }
        for (int j = lane; j < nc; j += 64)
            if (SC[j]) v[j] = v[j] - (minv - sp[j]);
        __syncthreads();
        if (lane == 0) {                                             // augment: at most nr steps back along the path
            int j = sink;
            for (int k = 0; k <= nr; ++k) {
                const int pi = clampi(path[j], 0, nr - 1);
                row4col[j] = pi;
                const int t = col4row[pi];
                col4row[pi] = j;
                j = t;
                if (pi == cur || j < 0) break;
            }
        }
        __syncthreads();
    }
    if (failed) {
        for (int g = lane; g < G; g += 64) mt[g] = g < Np ? g : -1;
        if (lane == 0) status[b] = PH_ASSIGN_ESOLVE;
        return;
    }
    for (int g = lane; g < G; g += 64) mt[g] = tr ? col4row[g] : row4col[g];
    if (lane == 0) status[b] = PH_ASSIGN_OK;
}

struct DescArgs {
    ph_assign_cfg c;
    uint64_t off[NSEC];                                  // section offsets, ph_assign_layout's order
    uint64_t real[NSEC];                                 // bytes of a section that carry content (a placeholder carries none)
    uint64_t end[NSEC];                                  // offset of the next section (or the total): what lies between is zeros
    const int64_t* gt; int64_t gt_words;
    int32_t pos_off[PH_ASSIGN_MAX_B + 1], dit_off[PH_ASSIGN_MAX_B + 1], sit_off[PH_ASSIGN_MAX_B + 1];      // prefix sums over the images
    int16_t G[PH_ASSIGN_MAX_B], S[PH_ASSIGN_MAX_B];     // the host's counts: every bound of the writer follows from them
    const int32_t* match; int ldg;
    int64_t* status; int clear_status;
    unsigned char* blob;
};
enum { S_TPTR = 0, S_WPTR, S_LABELS, S_POS_U8, S_POS_ROWS, S_DSTART, S_DIT_T, S_DIT_W, S_DIT_S, S_LABEL_W, S_SSTART, S_SIT_M, S_SIT_L };

__global__ __launch_bounds__(256) void k_assign_desc(DescArgs a) {
    __shared__ int g_of[AS_MAX];                         // prediction row -> its ground-truth column, -1 unmatched
    __shared__ int before[AS_MAX];                       // matched prediction rows below this one
    __shared__ int64_t scls[AS_MAX];                     // the image's stuff classes
    const ph_assign_cfg& c = a.c;
    const int b = blockIdx.x, t = threadIdx.x;
    const int Np = c.Np, N = c.N, L = c.L, nt = c.n_thing, ns = c.n_stuff;
    const bool roi = c.roi != 0, sem = c.has_sem != 0, dep = c.has_depth != 0;
    const int64_t HW4 = 4 * c.HW;
    const int64_t* T = a.gt + (int64_t)b * PH_ASSIGN_GT_WORDS;
    const int G = clampi(a.G[b], 0, a.ldg), S = clampi(a.S[b], 0, min(ns, AS_MAX));
    const int m = min(G, Np);
    const int64_t mask_base = T[GT_MASK], sem_base = T[GT_SEM], valid_base = T[GT_VALID], depth_base = T[GT_DEPTH];
    const int64_t lab_off = T[GT_LAB], cls_off = T[GT_CLS];
    const bool lab_ok = lab_off >= 0 && lab_off + G <= a.gt_words, cls_ok = cls_off >= 0 && cls_off + S <= a.gt_words;
    // items in front of this image and its own: prefix sums of counts the host knows (layout_of)
    const int64_t pos_off = a.pos_off[b], dit_off = a.dit_off[b], sit_off = a.sit_off[b];
    const int64_t pos_n = a.pos_off[b + 1] - pos_off, ditems = a.dit_off[b + 1] - dit_off;
    for (int p = t; p < Np; p += 256) g_of[p] = -1;
    for (int k = t; k < S; k += 256) scls[k] = cls_ok ? a.gt[cls_off + k] : (int64_t)nt + k;
    __syncthreads();
    for (int g = t; g < G; g += 256) {
        const int p = a.match[(size_t)b * a.ldg + g];
        if (p >= 0 && p < Np) g_of[p] = g;
    }
    __syncthreads();
    if (t < Np) {
        int n = 0;
        for (int j = 0; j < t; ++j) n += g_of[j] >= 0 ? 1 : 0;
        before[t] = n;
    }
    __syncthreads();
    unsigned char* B0 = a.blob;
    int64_t* tptr = (int64_t*)(B0 + a.off[S_TPTR]);
    int64_t* wptr = (int64_t*)(B0 + a.off[S_WPTR]);
    int64_t* labels = (int64_t*)(B0 + a.off[S_LABELS]);
    unsigned char* pos_u8 = B0 + a.off[S_POS_U8];
    int32_t* pos_rows = (int32_t*)(B0 + a.off[S_POS_ROWS]);
    int32_t* dstart = (int32_t*)(B0 + a.off[S_DSTART]);
    int64_t* dit_t = (int64_t*)(B0 + a.off[S_DIT_T]);
    int64_t* dit_w = (int64_t*)(B0 + a.off[S_DIT_W]);
    float* dit_s = (float*)(B0 + a.off[S_DIT_S]);
    float* label_w = (float*)(B0 + a.off[S_LABEL_W]);
    int32_t* sstart = (int32_t*)(B0 + a.off[S_SSTART]);
    int64_t* sit_m = (int64_t*)(B0 + a.off[S_SIT_M]);
    int32_t* sit_l = (int32_t*)(B0 + a.off[S_SIT_L]);
    const int64_t r0 = (int64_t)b * N;
    const float pw = c.pos_weight;
    const int ncol = sem ? nt : L;                       // label-weight columns of a proposal row
    // the roi form's depth items of an image: its positives except one on the last row, then the direct-depth item on the last row
    const int last = N - 1;
    // ---- the rows
    for (int r = t; r < N; r += 256) {
        int64_t tp = 0, wp = 0, lab = L;
        int ps = 0, items_le = 0;                        // depth items of the image on rows <= r (roi form)
        if (r < Np) {
            const int g = g_of[r];
            wp = valid_base;
            if (g >= 0) {
                tp = mask_base + g * HW4;
                lab = lab_ok ? a.gt[lab_off + g] : L;
                ps = 1;
                const int k = before[r];
                if (k < m) pos_rows[pos_off + k] = (int32_t)(r0 + r);
                if (dep && k < m) {
                    if (roi) {
                        if (r != last) { dit_t[dit_off + k] = depth_base; dit_w[dit_off + k] = tp; dit_s[dit_off + k] = pw; }
                    } else {
                        dit_t[dit_off + k] = depth_base; dit_w[dit_off + k] = tp; dit_s[dit_off + k] = pw;
                    }
                }
                if (!roi && k < m) { sit_m[sit_off + S + k] = tp; sit_l[sit_off + S + k] = (int32_t)lab; }
            }
            items_le = before[r] + ps;
        } else {                                         // a stuff row of the roi form: class nt + (r - Np)
            const int k = r - Np;
            int j = -1, rank = 0;
            for (int q = 0; q < S; ++q) {
                const int64_t kq = scls[q] - nt;
                if (kq == k) j = q;
                rank += kq <= k ? 1 : 0;                  // the classes of an image are distinct (the caller checks)
            }
            if (j >= 0) {
                tp = sem_base + j * HW4; wp = valid_base; lab = scls[j]; ps = 1;
                const int at = m + rank - 1;
                if (at < pos_n) pos_rows[pos_off + at] = (int32_t)(r0 + r);
                if (dep && r != last && at < ditems - 1) { dit_t[dit_off + at] = depth_base; dit_w[dit_off + at] = tp; dit_s[dit_off + at] = pw; }
            }
            items_le = m + rank;
        }
        tptr[r0 + r] = tp; wptr[r0 + r] = wp; labels[r0 + r] = lab; pos_u8[r0 + r] = (unsigned char)ps;
        if (roi) dstart[r0 + r + 1] = dep ? (int32_t)(dit_off + (r == last ? ditems : items_le)) : 0;
    }
    if (roi) {
        for (int e = t; e < N * L; e += 256) {
            const int r = e / L, col = e - r * L;
            float w = 0.f;
            if (r < Np) w = col < ncol ? (g_of[r] >= 0 ? pw : 1.f) : 0.f;
            else w = col == nt + (r - Np) ? 1.f : 0.f;
            label_w[r0 * L + e] = w;
        }
        if (dep && t == 0 && ditems > 0) { dit_t[dit_off + ditems - 1] = depth_base; dit_w[dit_off + ditems - 1] = 1; dit_s[dit_off + ditems - 1] = 1.f; }
    } else {
        // KernelHead: the stuff masks in order (depth items behind the things, dense-target items in front of them)
        for (int k = t; k < S; k += 256) {
            const int64_t w = sem_base + k * HW4;
            if (dep && m + k < ditems) { dit_t[dit_off + m + k] = depth_base; dit_w[dit_off + m + k] = w; dit_s[dit_off + m + k] = pw; }
            sit_m[sit_off + k] = w; sit_l[sit_off + k] = (int32_t)scls[k];
        }
        if (t == 0) {
            dstart[b + 1] = dep ? (int32_t)(dit_off + ditems) : 0;
            sstart[b + 1] = a.sit_off[b + 1];
        }
    }
    if (t == 0 && a.clear_status) a.status[b] = PH_ASSIGN_OK;
    // ---- workgroup 0: the first words of the start tables, the placeholders of empty sections and the padding between sections
    if (b == 0) {
        if (t == 0) { dstart[0] = 0; if (!roi) sstart[0] = 0; }
        for (int s = 0; s < NSEC; ++s)
            for (uint64_t e = a.off[s] + a.real[s] + t; e < a.end[s]; e += 256) B0[e] = 0;
    }
}

// sizes of the sections from the counts alone; `real`: bytes that carry content; pre: [3][B + 1] prefix sums (positives, depth items,
// dense-target items) when B <= PH_ASSIGN_MAX_B
int layout_of(const ph_assign_cfg* c, const int32_t* G, const int32_t* S, const int32_t* last_pos, ph_assign_layout* out, uint64_t* real,
              uint64_t* end, int32_t (*pre)[PH_ASSIGN_MAX_B + 1], const char* fn) {
    if (!c || !G || !out) { ph_set_error("%s: null cfg, counts or out", fn); return PH_EINVAL; }
    if (c->B < 1 || c->B > 4096 || c->Np < 1 || c->Np > 65536 || c->L < 1 || c->L > 65536 || c->HW < 1 || c->n_thing < 0 || c->n_stuff < 0 ||
        c->n_stuff > 65536) {
        ph_set_error("%s: B must be 1 .. 4096, Np, L 1 .. 65536, HW positive, class counts 0 .. 65536", fn);
        return PH_EINVAL;
    }
    const bool roi = c->roi != 0, sem = c->has_sem != 0;
    if (c->N != c->Np + ((roi && sem) ? c->n_stuff : 0)) { ph_set_error("%s: N must be Np (+ n_stuff for the roi form with stuff)", fn); return PH_EINVAL; }
    if (sem && !S) { ph_set_error("%s: has_sem without stuff counts", fn); return PH_EINVAL; }
    uint64_t P = 0, nd = 0, nsit = 0;
    for (int b = 0; b < c->B; ++b) {
        const int Sb = sem ? S[b] : 0;
        if (G[b] < 0 || G[b] > 65536 || Sb < 0 || Sb > c->n_stuff) { ph_set_error("%s: image %d: counts out of range", fn, b); return PH_EINVAL; }
        const uint64_t m = G[b] < c->Np ? G[b] : c->Np;
        // the roi form drops the depth item of a positive on the image's last row: the direct-depth item takes its place
        const uint64_t lp = (roi && last_pos && last_pos[b]) ? 1 : 0;
        if (lp > m + Sb) { ph_set_error("%s: image %d: last_pos without a positive", fn, b); return PH_EINVAL; }
        if (pre && b < PH_ASSIGN_MAX_B) { pre[0][b] = (int32_t)P; pre[1][b] = (int32_t)nd; pre[2][b] = (int32_t)nsit; }
        P += m + (roi ? Sb : 0);
        nsit += m + Sb;
        nd += c->has_depth ? (roi ? m + Sb + 1 - lp : m + Sb) : 0;
    }
    if (pre && c->B <= PH_ASSIGN_MAX_B) { pre[0][c->B] = (int32_t)P; pre[1][c->B] = (int32_t)nd; pre[2][c->B] = (int32_t)nsit; }
    const uint64_t R = (uint64_t)c->B * c->N, depth_rows = roi ? R : (uint64_t)c->B;
    const uint64_t bytes[NSEC] = {R * 8, R * 8, R * 8, R, P * 4, (depth_rows + 1) * 4, nd * 8, nd * 8, nd * 4,
                                  roi ? R * c->L * 4 : 0, roi ? 0 : ((uint64_t)c->B + 1) * 4, roi ? 0 : nsit * 8, roi ? 0 : nsit * 4};
    const uint64_t unit[NSEC] = {8, 8, 8, 1, 4, 4, 8, 8, 4, 4, 4, 8, 4};
    const bool present[NSEC] = {true, true, true, true, true, true, true, true, true, roi, !roi, !roi, !roi};
    uint64_t* offs[NSEC] = {&out->tptr, &out->wptr, &out->labels, &out->pos_u8, &out->pos_rows, &out->dstart, &out->dit_t, &out->dit_w, &out->dit_s,
                            &out->label_w, &out->sstart, &out->sit_m, &out->sit_l};
    uint64_t o = 0;
    for (int s = 0; s < NSEC; ++s) {
        *offs[s] = o;
        const uint64_t nb = present[s] ? (bytes[s] ? bytes[s] : unit[s]) : 0;     // an empty section is one zero element
        if (real) real[s] = present[s] ? bytes[s] : 0;
        o += (nb + 15) / 16 * 16;
        if (end) end[s] = o;
    }
    out->total_bytes = o < 16 ? 16 : o;
    out->P = (int64_t)P; out->depth_items = (int64_t)nd; out->seg_items = roi ? 0 : (int64_t)nsit;
    out->depth_rows = (int64_t)depth_rows;
    return PH_OK;
}

}  // namespace

extern "C" int ph_assign_desc_layout(const ph_assign_cfg* cfg, const int32_t* G, const int32_t* S, const int32_t* last_pos, ph_assign_layout* out) {
    return layout_of(cfg, G, S, last_pos, out, nullptr, nullptr, nullptr, "ph_assign_desc_layout");
}

extern "C" int ph_assign_solve(const float* cost, int B, int Np, int ldg, const int32_t* counts, int64_t count_stride, int32_t* match,
                               int64_t* status, void* stream) {
    PH_CHECK_ARG(cost && counts && match && status, "null cost, counts, match or status");
    PH_CHECK_ARG(B >= 1 && B <= 65535 && Np >= 1 && ldg >= 1 && count_stride >= 0, "B must be 1 .. 65535, Np and ldg positive");
    if (Np > AS_MAX || ldg > AS_MAX) {
        ph_set_error("ph_assign_solve: max(Np, ldg) must be <= %d, got Np %d, ldg %d", AS_MAX, Np, ldg);
        return PH_EUNSUPPORTED;
    }
    hipLaunchKernelGGL(k_assign_solve, dim3(B), dim3(64), 0, (hipStream_t)stream, cost, Np, ldg, counts, count_stride, match, status);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

extern "C" int ph_assign_desc(const ph_assign_cfg* cfg, const int32_t* G, const int32_t* S, const int32_t* last_pos, const float* cost, int ldg,
                              const int64_t* gt_table, int64_t gt_words, int32_t* match, int64_t* status, void* blob, size_t blob_bytes,
                              void* stream) {
    DescArgs a{};
    ph_assign_layout lay;
    int32_t pre[3][PH_ASSIGN_MAX_B + 1] = {};
    PH_RUN(layout_of(cfg, G, S, last_pos, &lay, a.real, a.end, pre, "ph_assign_desc"));
    PH_CHECK_ARG(gt_table && match && status && blob, "null gt_table, match, status or blob");
    PH_CHECK_ARG(ldg >= 0 && gt_words >= (int64_t)cfg->B * PH_ASSIGN_GT_WORDS, "ldg must be >= 0 and gt_table hold B records");
    PH_CHECK_ARG(((uintptr_t)blob & 15) == 0, "blob must be 16-byte aligned");
    if (blob_bytes < lay.total_bytes) {
        ph_set_error("ph_assign_desc: blob of %zu bytes, %llu needed", blob_bytes, (unsigned long long)lay.total_bytes);
        return PH_EWORKSPACE;
    }
    if (cfg->B > PH_ASSIGN_MAX_B || cfg->Np > AS_MAX || ldg > AS_MAX || cfg->n_stuff > AS_MAX) {
        ph_set_error("ph_assign_desc: B must be <= %d, Np, ldg and n_stuff <= %d, got %d, %d, %d, %d", PH_ASSIGN_MAX_B, AS_MAX, cfg->B, cfg->Np, ldg,
                     cfg->n_stuff);
        return PH_EUNSUPPORTED;
    }
    if (cfg->roi && cfg->has_depth && cfg->N == cfg->Np) {
        ph_set_error("ph_assign_desc: the roi form with depth needs stuff rows (its direct-depth row would be a proposal row)");
        return PH_EUNSUPPORTED;
    }
    for (int b = 0; b < cfg->B; ++b) {
        if (G[b] > ldg) { ph_set_error("ph_assign_desc: image %d has %d columns, ldg is %d", b, G[b], ldg); return PH_EINVAL; }
        a.G[b] = (int16_t)G[b];
        a.S[b] = (int16_t)(cfg->has_sem ? S[b] : 0);
    }
    hipStream_t s = (hipStream_t)stream;
    if (cost != nullptr && ldg > 0)
        hipLaunchKernelGGL(k_assign_solve, dim3(cfg->B), dim3(64), 0, s, cost, cfg->Np, ldg, (const int32_t*)gt_table,
                           (int64_t)(2 * PH_ASSIGN_GT_WORDS), match, status);
    a.c = *cfg;
    const uint64_t offs[NSEC] = {lay.tptr, lay.wptr, lay.labels, lay.pos_u8, lay.pos_rows, lay.dstart, lay.dit_t, lay.dit_w, lay.dit_s, lay.label_w,
                                 lay.sstart, lay.sit_m, lay.sit_l};
    for (int i = 0; i < NSEC; ++i) a.off[i] = offs[i];
    for (int b = 0; b <= cfg->B; ++b) { a.pos_off[b] = pre[0][b]; a.dit_off[b] = pre[1][b]; a.sit_off[b] = pre[2][b]; }
    a.gt = gt_table; a.gt_words = gt_words; a.match = match; a.ldg = ldg; a.status = status;
    a.clear_status = ldg == 0 ? 1 : 0;                   // no column anywhere: nothing was solved and nothing can have gone wrong
    a.blob = (unsigned char*)blob;
    hipLaunchKernelGGL(k_assign_desc, dim3(cfg->B), dim3(256), 0, s, a);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
