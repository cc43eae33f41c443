// DVPQ tallies on the device (include/polyhead.h ph_dvpq_cfg .. ph_dvpq_frames): per frame the table of (gt id, pred id, mask of
// violated depth thresholds) -> pixel count that dvps_eval.clip_tallies turns into every window and threshold of the metric, and the
// ingredients of dvps_eval.compute_errors.  Three launches, no synchronisation, no environment variable, no memset node:
//   k_dvpq_clear   the frames' hash tables and flags in the workspace
//   k_dvpq_frames  grid (workgroups per frame, B).  A lane reads 4 pixels (16-byte loads when the frame is 16-byte aligned); equal keys
//                  are combined inside the wave (neighbouring pixels nearly always share a key, so this leaves one add per distinct key
//                  per wave and step), then in an open-addressing table in LDS, which is added to the frame's table in the workspace
//                  at the end; a key that finds no room in LDS within DQ_LDS_PROBES slots goes to the frame's table directly
//   k_dvpq_finish  one workgroup per frame: compaction, ranking by counting (rows ascending in (g, p, mask)), the depth partials
//
// The tables.  A key has 72 bits (any uint32 is a legal id), more than one compare-and-swap covers, so a slot is claimed in two
// steps, each a 64-bit compare-and-swap from 0 of a word that cannot be 0:  A = 1 << 63 | mask << 32 | p,  B = 1 << 32 | g.  A slot
// belongs to the key whose A AND B it holds; an inserter that finds another A, or its own A and another B, moves to the next slot.
// Both words are immutable once set and every inserter that sets A goes on to B, so nobody waits for anybody, a slot is never
// half-claimed after the kernel, and a key's first matching slot is the same for every inserter: no key is counted in two slots.
// The count is a third word (atomic add).  The all-zero key (0, 0, 0) is an ordinary key: A = 1 << 63, B = 1 << 32.
//
// Overflow.  A frame's table has T = 2 capacity slots, probed linearly from the key's hash over all T: with at most `capacity`
// distinct keys an insert cannot fail.  An insert that finds all T slots taken sets the frame's `full` flag and drops its pixels;
// from then on inserters give up after DQ_CHECK probes (a frame of noise must not cost T probes per pixel).  k_dvpq_finish then keeps
// only the keys that lie less than DQ_CHECK slots from their hash: those were reached by every one of their inserts, so their counts
// are exact.  overflow = full, or more keys than capacity.
#include <math.h>

#include "ph_common.h"

#pragma clang fp contract(off)

enum {
    DQ_THREADS = 256,
    DQ_QUADS = 1024,            // 4-pixel quads per workgroup at least: 4096 pixels
    DQ_MAX_WGS = 1024,          // workgroups per frame at most
    DQ_LDS_SLOTS = 512,         // 10 KB of LDS
    DQ_LDS_PROBES = 16,
    DQ_CHECK = 64,
    DQ_REC = 8,                 // doubles of a depth record
    DQ_FIN_THREADS = 1024
};

struct DGeo {
    int B, H, W, cap, nthr, T, nq, qpw, wgs;
    int64_t HW;
    float thr[PH_DVPQ_MAX_THR];
    size_t o_a, o_b, o_c, o_flags, o_dense, o_part, clear_bytes, total;
};

static int resolve(const ph_dvpq_cfg* c, DGeo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = DGeo{};
    g.B = c->B; g.H = c->H; g.W = c->W; g.cap = c->capacity; g.nthr = c->nthr;
    if (!(g.B > 0 && g.H > 0 && g.W > 0)) { ph_set_error("%s: bad size (B, H, W > 0)", fn); return PH_EINVAL; }
    if (g.B > 65535) { ph_set_error("%s: at most 65535 frames per call", fn); return PH_EINVAL; }
    g.HW = (int64_t)g.H * g.W;
    if (g.HW >= (1ll << 31)) { ph_set_error("%s: H * W must be below 2^31", fn); return PH_EINVAL; }
    if (!(g.cap >= 64 && g.cap <= 65536 && (g.cap & (g.cap - 1)) == 0)) {
        ph_set_error("%s: capacity must be a power of two in 64 .. 65536, got %d", fn, g.cap);
        return PH_EINVAL;
    }
    if (!(g.nthr >= 0 && g.nthr <= PH_DVPQ_MAX_THR)) { ph_set_error("%s: nthr must be 0 .. %d, got %d", fn, PH_DVPQ_MAX_THR, g.nthr); return PH_EINVAL; }
    for (int j = 0; j < PH_DVPQ_MAX_THR; ++j) {
        g.thr[j] = j < g.nthr ? c->thr[j] : 0.f;
        if (g.thr[j] != g.thr[j]) { ph_set_error("%s: thr[%d] is NaN", fn, j); return PH_EINVAL; }
    }
    g.T = 2 * g.cap;
    g.nq = (int)((g.HW + 3) / 4);
    g.wgs = (g.nq + DQ_QUADS - 1) / DQ_QUADS;
    if (g.wgs > DQ_MAX_WGS) g.wgs = DQ_MAX_WGS;
    g.qpw = ((g.nq + g.wgs - 1) / g.wgs + DQ_THREADS - 1) / DQ_THREADS * DQ_THREADS;
    const size_t slots = (size_t)g.B * g.T;
    size_t o = 0;
    g.o_a = o; o += al256(slots * 8);
    g.o_b = o; o += al256(slots * 8);
    g.o_c = o; o += al256(slots * 4);
    g.o_flags = o; o += al256((size_t)g.B * 4 * 4);
    g.clear_bytes = o;
    g.o_dense = o; o += al256((size_t)g.B * g.cap * 16);
    g.o_part = o; o += al256((size_t)g.B * g.wgs * DQ_REC * 8);
    g.total = o;
    return PH_OK;
}

// ---------------------------------------------------------------------------------------------
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t dq_hash(uint32_t g, uint32_t p, uint32_t m) {
    uint32_t h = g * 0x9E3779B1u ^ (p + 0x7F4A7C15u) * 0x85EBCA6Bu ^ (m + 1u) * 0xC2B2AE35u;
    h ^= h >> 15; h *= 0x2C1B3C6Du;
    h ^= h >> 12; h *= 0x297A2D39u;
    h ^= h >> 15;
    return h;
}
__device__ __forceinline__ u64 dq_word_a(uint32_t p, uint32_t m) { return (1ull << 63) | ((u64)m << 32) | p; }
__device__ __forceinline__ u64 dq_word_b(uint32_t g) { return (1ull << 32) | g; }

// adds n to the slot of the key (ka, kb), claiming one if need be; false: no slot within max_probes (or the frame is full)
template <int SCOPE>
__device__ __forceinline__ bool dq_insert(u64* A, u64* Bk, uint32_t* C, uint32_t mask, uint32_t h, u64 ka, u64 kb, uint32_t n, int max_probes,
                                          const uint32_t* full) {
#pragma unroll 1
    for (int i = 0; i < max_probes; ++i) {
        if (full != nullptr && i != 0 && i % DQ_CHECK == 0 && __hip_atomic_load(full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
        const uint32_t s = (h + (uint32_t)i) & mask;
        u64 a = __hip_atomic_load(A + s, __ATOMIC_RELAXED, SCOPE);
        if (a == 0) {
            a = atomicCAS(A + s, 0ull, ka);
            if (a == 0) a = ka;
        }
        if (a != ka) continue;
        u64 b = __hip_atomic_load(Bk + s, __ATOMIC_RELAXED, SCOPE);
        if (b == 0) {
            b = atomicCAS(Bk + s, 0ull, kb);
            if (b == 0) b = kb;
        }
        if (b != kb) continue;
        atomicAdd(C + s, n);
        return true;
    }
    return false;
}

struct DqFrameTable { u64* A; u64* Bk; uint32_t* C; uint32_t* flags; uint32_t mask; };

__device__ __forceinline__ void dq_global_add(const DqFrameTable& t, uint32_t g, uint32_t p, uint32_t m, uint32_t n) {
    if (!dq_insert<__HIP_MEMORY_SCOPE_AGENT>(t.A, t.Bk, t.C, t.mask, dq_hash(g, p, m), dq_word_a(p, m), dq_word_b(g), n, (int)t.mask + 1, t.flags))
        atomicOr(t.flags, 1u);
}

__global__ __launch_bounds__(256) void k_dvpq_clear(uint4* __restrict__ ws, int64_t n16) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) ws[i] = make_uint4(0u, 0u, 0u, 0u);
}

struct DqArgs {
    const uint32_t* pp; const uint8_t* ps; const double* pt; const float* pd; const uint32_t* gp; const float* gd;
    int64_t HW;
    int nq, qpw, wgs, nthr, T;
    float thr[PH_DVPQ_MAX_THR];
    u64* A; u64* Bk; uint32_t* C; uint32_t* flags; double* part;
};

template <bool PANSEG>
__global__ __launch_bounds__(DQ_THREADS) void k_dvpq_frames(const DqArgs a) {
    __shared__ u64 lA[DQ_LDS_SLOTS], lB[DQ_LDS_SLOTS];
    __shared__ uint32_t lC[DQ_LDS_SLOTS];
    __shared__ double red[DQ_THREADS / 64][DQ_REC];
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
    for (int i = tid; i < DQ_LDS_SLOTS; i += DQ_THREADS) { lA[i] = 0; lB[i] = 0; lC[i] = 0; }
    __syncthreads();
    const int64_t base = (int64_t)b * a.HW;
    const uint32_t* gp = a.gp + base;
    const float* gd = a.gd + base;
    const float* pd = a.pd + base;
    const uint32_t* pp = PANSEG ? a.pp + base : nullptr;
    const uint8_t* ps = PANSEG ? nullptr : a.ps + base;
    const double* pt = PANSEG ? nullptr : a.pt + base;
    // 16-byte loads need the frame's first pixel at a 16-byte boundary in every map (a quad of sem bytes: 4)
    const bool vec = PANSEG ? ((((uintptr_t)gp | (uintptr_t)gd | (uintptr_t)pd | (uintptr_t)pp) & 15) == 0)
                            : ((((uintptr_t)gp | (uintptr_t)gd | (uintptr_t)pd | (uintptr_t)pt) & 15) == 0 && ((uintptr_t)ps & 3) == 0);
    DqFrameTable tab{a.A + (size_t)b * a.T, a.Bk + (size_t)b * a.T, a.C + (size_t)b * a.T, a.flags + (size_t)b * 4, (uint32_t)a.T - 1u};

    uint32_t n_pos = 0, n1 = 0, n2 = 0, n3 = 0;
    double s_abs = 0., s_sq = 0., s_d2 = 0., s_log = 0.;
    const int q0 = blockIdx.x * a.qpw;
    const int q1 = q0 + a.qpw < a.nq ? q0 + a.qpw : a.nq;
    for (int it = q0; it < q1; it += DQ_THREADS) {         // uniform trip count: every lane takes part in the ballots
        const int q = it + tid;
        const int64_t idx = 4ll * q;
        uint32_t g[4], p[4], m[4];
        float fg[4], fp[4];
        bool v[4];
        if (q < q1 && vec && idx + 3 < a.HW) {
            const uint4 x = *(const uint4*)(gp + idx);
            const float4 y = *(const float4*)(gd + idx), z = *(const float4*)(pd + idx);
            g[0] = x.x; g[1] = x.y; g[2] = x.z; g[3] = x.w;
            fg[0] = y.x; fg[1] = y.y; fg[2] = y.z; fg[3] = y.w;
            fp[0] = z.x; fp[1] = z.y; fp[2] = z.z; fp[3] = z.w;
            if (PANSEG) {
                const uint4 w = *(const uint4*)(pp + idx);
                p[0] = w.x; p[1] = w.y; p[2] = w.z; p[3] = w.w;
            } else {
                const uint32_t s4 = *(const uint32_t*)(ps + idx);
                const double2 t0 = *(const double2*)(pt + idx), t1 = *(const double2*)(pt + idx + 2);
                p[0] = (uint32_t)((long long)(s4 & 255u) * 10000ll + (long long)t0.x);
                p[1] = (uint32_t)((long long)((s4 >> 8) & 255u) * 10000ll + (long long)t0.y);
                p[2] = (uint32_t)((long long)((s4 >> 16) & 255u) * 10000ll + (long long)t1.x);
                p[3] = (uint32_t)((long long)(s4 >> 24) * 10000ll + (long long)t1.y);
            }
            v[0] = v[1] = v[2] = v[3] = true;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = q < q1 && idx + j < a.HW;
                g[j] = p[j] = 0u;
                fg[j] = fp[j] = 0.f;
                if (v[j]) {
                    g[j] = gp[idx + j]; fg[j] = gd[idx + j]; fp[j] = pd[idx + j];
                    p[j] = PANSEG ? pp[idx + j] : (uint32_t)((long long)ps[idx + j] * 10000ll + (long long)pt[idx + j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = 0u;
            if (v[j] && fg[j] > 0.f) {
                const float rel = __fdiv_rn(fabsf(fp[j] - fg[j]), fg[j]);
#pragma unroll
                for (int k = 0; k < PH_DVPQ_MAX_THR; ++k)
                    if (k < a.nthr && rel > a.thr[k]) m[j] |= 1u << k;
                const float r0 = __fdiv_rn(fg[j], fp[j]), r1 = __fdiv_rn(fp[j], fg[j]);       // max(r0, r1) < c, false on a NaN as numpy's
                n_pos += 1u;
                n1 += (r0 < 1.25f && r1 < 1.25f) ? 1u : 0u;
                n2 += (r0 < 1.5625f && r1 < 1.5625f) ? 1u : 0u;
                n3 += (r0 < 1.953125f && r1 < 1.953125f) ? 1u : 0u;
                const double dg = (double)fg[j], dp = (double)fp[j], d = dg - dp, d2 = d * d, dl = log(dg) - log(dp);
                s_abs += fabs(d) / dg;
                s_sq += d2 / dg;
                s_d2 += d2;
                s_log += dl * dl;
            }
        }
        // a lane's own pixels first, then the wave's
        uint32_t c[4] = {v[0] ? 1u : 0u, 1u, 1u, 1u};
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (v[j] && v[0] && g[j] == g[0] && p[j] == p[0] && m[j] == m[0]) { c[0] += 1u; v[j] = false; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u64 todo = __ballot(v[j]);
            while (todo) {
                const int leader = __builtin_ctzll(todo);
                const uint32_t kg = __builtin_amdgcn_readlane(g[j], leader), kp = __builtin_amdgcn_readlane(p[j], leader),
                               km = __builtin_amdgcn_readlane(m[j], leader);
                const bool match = v[j] && g[j] == kg && p[j] == kp && m[j] == km;
                const u64 mm = __ballot(match);
                const uint32_t n = __popcll(__ballot(match && (c[j] & 1u))) + 2u * __popcll(__ballot(match && (c[j] & 2u))) +
                                   4u * __popcll(__ballot(match && (c[j] & 4u)));
                if (lane == leader) {
                    const uint32_t h = dq_hash(kg, kp, km);
                    if (!dq_insert<__HIP_MEMORY_SCOPE_WORKGROUP>(lA, lB, lC, DQ_LDS_SLOTS - 1, h >> 16, dq_word_a(kp, km), dq_word_b(kg), n,
                                                                 DQ_LDS_PROBES, nullptr))
                        dq_global_add(tab, kg, kp, km, n);
                }
                todo &= ~mm;
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < DQ_LDS_SLOTS; s += DQ_THREADS) {
        const u64 wa = lA[s], wb = lB[s];
        const uint32_t n = lC[s];
        if (wa != 0 && wb != 0 && n != 0) dq_global_add(tab, (uint32_t)wb, (uint32_t)wa, (uint32_t)(wa >> 32) & 255u, n);
    }
    // the depth record of this workgroup: a fixed tree inside the wave, the waves in order
    double r[DQ_REC] = {(double)n_pos, s_abs, s_sq, s_d2, s_log, (double)n1, (double)n2, (double)n3};
#pragma unroll
    for (int k = 0; k < DQ_REC; ++k)
        for (int off = 32; off > 0; off >>= 1) r[k] += __shfl_down(r[k], off, 64);
    if (lane == 0)
        for (int k = 0; k < DQ_REC; ++k) red[tid >> 6][k] = r[k];
    __syncthreads();
    if (tid < DQ_REC) {
        double s = red[0][tid];
        for (int w = 1; w < DQ_THREADS / 64; ++w) s += red[w][tid];
        a.part[((size_t)b * a.wgs + blockIdx.x) * DQ_REC + tid] = s;
    }
}

__global__ __launch_bounds__(DQ_FIN_THREADS) void k_dvpq_finish(const u64* __restrict__ A, const u64* __restrict__ Bk, const uint32_t* __restrict__ C,
                                                                const uint32_t* __restrict__ flags, uint4* dense, const double* __restrict__ part,
                                                                int wgs, int T, int cap, uint32_t* table_out, double* __restrict__ depth_out) {
    __shared__ uint32_t total_s;
    __shared__ uint32_t tg[DQ_FIN_THREADS], tp[DQ_FIN_THREADS], tm[DQ_FIN_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    A += (size_t)b * T; Bk += (size_t)b * T; C += (size_t)b * T;
    dense += (size_t)b * cap;
    uint4* out = (uint4*)(table_out + (size_t)b * (4 + 4 * (size_t)cap));
    const bool full = flags[(size_t)b * 4] != 0;
    if (tid == 0) total_s = 0;
    __syncthreads();
    for (int s = tid; s < T; s += DQ_FIN_THREADS) {
        const u64 wa = A[s], wb = Bk[s];
        if (wa == 0 || wb == 0) continue;
        const uint32_t g = (uint32_t)wb, p = (uint32_t)wa, m = (uint32_t)(wa >> 32) & 255u;
        if (full && (((uint32_t)s - dq_hash(g, p, m)) & (uint32_t)(T - 1)) >= (uint32_t)DQ_CHECK) continue;      // its count may be short
        const uint32_t i = atomicAdd(&total_s, 1u);
        if (i < (uint32_t)cap) dense[i] = make_uint4(g, p, m, C[s]);
    }
    __syncthreads();
    const uint32_t total = total_s;
    const int n = total < (uint32_t)cap ? (int)total : cap;
    if (tid == 0) out[0] = make_uint4((uint32_t)n, (full || total > (uint32_t)cap) ? 1u : 0u, 0u, 0u);
    // keys are distinct: the number of smaller keys is the row
    for (int i0 = 0; i0 < n; i0 += DQ_FIN_THREADS) {
        const int i = i0 + tid;
        const uint4 mine = i < n ? dense[i] : make_uint4(0u, 0u, 0u, 0u);
        const u64 k = ((u64)mine.x << 32) | mine.y;
        uint32_t rank = 0;
        for (int t0 = 0; t0 < n; t0 += DQ_FIN_THREADS) {
            __syncthreads();
            if (t0 + tid < n) {
                const uint4 e = dense[t0 + tid];
                tg[tid] = e.x; tp[tid] = e.y; tm[tid] = e.z;
            }
            __syncthreads();
            const int lim = n - t0 < DQ_FIN_THREADS ? n - t0 : DQ_FIN_THREADS;
            if (i < n)
                for (int j = 0; j < lim; ++j) {
                    const u64 kj = ((u64)tg[j] << 32) | tp[j];
                    rank += (kj < k || (kj == k && tm[j] < mine.z)) ? 1u : 0u;
                }
        }
        if (i < n) out[1 + rank] = mine;
    }
    for (int i = n + tid; i < cap; i += DQ_FIN_THREADS) out[1 + i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid < DQ_REC) {
        double s = 0.;
        for (int w = 0; w < wgs; ++w) s += part[((size_t)b * wgs + w) * DQ_REC + tid];
        depth_out[(size_t)b * DQ_REC + tid] = s;
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" size_t ph_dvpq_workspace_bytes(const ph_dvpq_cfg* cfg) {
    DGeo g;
    if (resolve(cfg, g, "ph_dvpq_workspace_bytes")) return 0;
    return g.total;
}

extern "C" int ph_dvpq_frames(const ph_dvpq_cfg* cfg, const ph_dvpq_io* io, void* workspace, size_t workspace_bytes, void* stream) {
    DGeo g;
    const int rc = resolve(cfg, g, "ph_dvpq_frames");
    if (rc) return rc;
    PH_CHECK_ARG(io != nullptr, "null io");
    PH_CHECK_ARG(io->pred_panseg || (io->pred_sem && io->pred_track), "null prediction: pred_panseg, or pred_sem and pred_track");
    PH_CHECK_ARG(io->pred_depth && io->gt_panseg && io->gt_depth, "null pred_depth, gt_panseg or gt_depth");
    PH_CHECK_ARG(io->table_out && io->depth_out, "null table_out or depth_out");
    PH_RUN(ph_check_buffers("ph_dvpq_frames", nullptr, workspace, workspace_bytes, g.total));
    PH_CHECK_ARG((((uintptr_t)io->pred_panseg | (uintptr_t)io->pred_depth | (uintptr_t)io->gt_panseg | (uintptr_t)io->gt_depth) & 3) == 0,
                 "the uint32 / float maps must be 4-byte aligned");
    PH_CHECK_ARG(io->pred_panseg || ((uintptr_t)io->pred_track & 7) == 0, "pred_track must be 8-byte aligned");
    PH_CHECK_ARG(((uintptr_t)io->table_out & 15) == 0, "table_out must be 16-byte aligned");
    PH_CHECK_ARG(((uintptr_t)io->depth_out & 7) == 0, "depth_out must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int64_t n16 = (int64_t)(g.clear_bytes / 16);
    const int64_t cb = (n16 + 255) / 256;
    hipLaunchKernelGGL(k_dvpq_clear, dim3((unsigned)(cb < 1024 ? cb : 1024)), dim3(256), 0, s, (uint4*)ws, n16);
    DqArgs a;
    a.pp = io->pred_panseg; a.ps = io->pred_sem; a.pt = io->pred_track; a.pd = io->pred_depth; a.gp = io->gt_panseg; a.gd = io->gt_depth;
    a.HW = g.HW; a.nq = g.nq; a.qpw = g.qpw; a.wgs = g.wgs; a.nthr = g.nthr; a.T = g.T;
    for (int j = 0; j < PH_DVPQ_MAX_THR; ++j) a.thr[j] = g.thr[j];
    a.A = (u64*)(ws + g.o_a); a.Bk = (u64*)(ws + g.o_b); a.C = (uint32_t*)(ws + g.o_c); a.flags = (uint32_t*)(ws + g.o_flags);
    a.part = (double*)(ws + g.o_part);
    if (io->pred_panseg)
        hipLaunchKernelGGL(k_dvpq_frames<true>, dim3(g.wgs, g.B), dim3(DQ_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(k_dvpq_frames<false>, dim3(g.wgs, g.B), dim3(DQ_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_dvpq_finish, dim3(g.B), dim3(DQ_FIN_THREADS), 0, s, a.A, a.Bk, a.C, a.flags, (uint4*)(ws + g.o_dense), a.part, g.wgs, g.T,
                       g.cap, io->table_out, io->depth_out);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
