// The optimizer step (include/polyhead.h ph_optim_*): clip_grad_norm_(max_norm, 2) + AdamW over every tensor of a table in at most
// three launches -- per-item sums of squares in fp64, one workgroup that turns them into the call's state record, the update.  A work
// item is PH_OPTIM_CHUNK elements of one tensor; whatever is reduced is stored per item and summed in index order, so the grid decides
// nothing.  fp32 without contraction: the update is torch's _single_tensor_adamw operation by operation.
#include "ph_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int OPT_T = 256;                                   // threads per workgroup
constexpr int OPT_V4 = PH_OPTIM_CHUNK / (4 * OPT_T);         // float4 per thread and full item
static_assert(OPT_V4 * 4 * OPT_T == PH_OPTIM_CHUNK, "an item is a whole number of float4 per thread");
static_assert(sizeof(ph_optim_tensor) == 64 && sizeof(ph_optim_state) == 40, "include/polyhead.h: the table entry and the state record");

// the first_item column in LDS (the video model has 341 tensors)
__device__ __forceinline__ void opt_load_column(const ph_optim_tensor* __restrict__ tab, int nt, int32_t* first) {
    for (int i = threadIdx.x; i < nt; i += OPT_T) first[i] = (int32_t)tab[i].first_item;
    __syncthreads();
}

// the tensor of an item: the LAST entry whose first item is not above it (a tensor without items shares its number with its successor,
// which wins; first[0] == 0)
__device__ __forceinline__ int opt_find(const int32_t* first, int nt, int item) {
    int lo = 0, hi = nt;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

// 16 bytes per lane where all four streams of the tensor allow it (an item starts a multiple of 16 KB into each)
__device__ __forceinline__ bool opt_vec(const ph_optim_tensor& e) {
    return (((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v) & 15) == 0;
}

__device__ __forceinline__ double opt_sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(OPT_T) void k_optim_sumsq(const ph_optim_tensor* __restrict__ tab, int nt, int nitems, double* __restrict__ partial) {
    __shared__ int32_t first[PH_OPTIM_MAX_TENSORS];
    __shared__ double red[OPT_T / 64];
    const int tid = threadIdx.x;
    opt_load_column(tab, nt, first);
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int t = opt_find(first, nt, item);
        const ph_optim_tensor e = tab[t];
        const int64_t off = (int64_t)(item - first[t]) * PH_OPTIM_CHUNK;
        const int64_t left = e.n - off;
        const int cnt = left < PH_OPTIM_CHUNK ? (int)left : PH_OPTIM_CHUNK;
        double s = 0.0;
        if (e.g != nullptr) {
            const float* g = e.g + off;
            int done = 0;
            if (opt_vec(e)) {
                const int n4 = cnt >> 2;
#pragma unroll
                for (int k = 0; k < OPT_V4; ++k) {
                    const int i = tid + k * OPT_T;
                    if (i < n4) {
                        const float4 x = ((const float4*)g)[i];
                        s += (opt_sq(x.x) + opt_sq(x.y)) + (opt_sq(x.z) + opt_sq(x.w));
                    }
                }
                done = n4 << 2;
            }
            for (int i = done + tid; i < cnt; i += OPT_T) s += opt_sq(g[i]);
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) partial[item] = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
    }
}

// ONE workgroup: the partials in index order (a fixed tree), the norm, the coefficient, the skip decision, the step counter and the
// bias corrections.  nitems == 0: the call did not ask for the norm.
__global__ __launch_bounds__(OPT_T) void k_optim_finalize(const double* __restrict__ partial, int nitems, ph_optim_cfg cfg, ph_optim_state* st) {
    __shared__ double red[OPT_T];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < nitems; i += OPT_T) s += partial[i];
    red[tid] = s;
    __syncthreads();
    for (int o = OPT_T / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid != 0) return;
    double norm = -1.0, coef = 1.0;
    bool finite = true;
    if (nitems > 0) {
        norm = sqrt(red[0]);
        finite = isfinite(norm);
        if (cfg.max_norm > 0.0) {
            const double c = cfg.max_norm / (norm + 1e-6);
            coef = c > 1.0 ? 1.0 : c;                        // torch's clamp(max = 1): a NaN stays a NaN
        }
    }
    const bool skip = !finite && (cfg.flags & PH_OPTIM_SKIP_NONFINITE) != 0;
    int64_t step = st->step, skipped = st->skipped;
    if (skip) ++skipped; else ++step;
    st->step = step;
    st->skipped = skipped;
    st->status = finite ? PH_OPTIM_OK : PH_OPTIM_ENONFINITE;
    st->skip = skip ? 1 : 0;
    st->grad_norm = (float)norm;
    st->clip_coef = (float)coef;
    st->bias1 = (float)(1.0 - pow(cfg.beta1, (double)step));
    st->bias2_sqrt = (float)sqrt(1.0 - pow(cfg.beta2, (double)step));
}

struct OptScalars { float coef, decay, omb1, beta2, omb2, bias2_sqrt, eps, nstep; };

// torch/optim/adam.py _single_tensor_adam with decoupled weight decay, one element: mul_, lerp_ (weight < 0.5: m + w (g - m)),
// mul_ + addcmul_ ((value g) g), sqrt / bias2_sqrt + eps, addcdiv_ ((value m) / denom)
__device__ __forceinline__ void opt_element(float& p, float g, float& m, float& v, const OptScalars& s) {
    g = g * s.coef;
    p = p * s.decay;
    m = m + s.omb1 * (g - m);
    v = v * s.beta2 + (s.omb2 * g) * g;
    const float denom = sqrtf(v) / s.bias2_sqrt + s.eps;
    p = p + (s.nstep * m) / denom;
}

__device__ __forceinline__ void opt_element4(float4& p, const float4& g, float4& m, float4& v, const OptScalars& s) {
    opt_element(p.x, g.x, m.x, v.x, s);
    opt_element(p.y, g.y, m.y, v.y, s);
    opt_element(p.z, g.z, m.z, v.z, s);
    opt_element(p.w, g.w, m.w, v.w, s);
}

__global__ __launch_bounds__(OPT_T) void k_optim_update(const ph_optim_tensor* __restrict__ tab, int nt, int nitems,
                                                         const ph_optim_state* __restrict__ st, float beta2, float omb1, float omb2,
                                                         float eps, int zero_grads, float lr_factor, const float* __restrict__ lr_factor_dev) {
    __shared__ int32_t first[PH_OPTIM_MAX_TENSORS];
    const int tid = threadIdx.x;
    const bool skip = st->skip != 0;
    if (skip && !zero_grads) return;
    opt_load_column(tab, nt, first);
    OptScalars s;
    s.coef = st->clip_coef;
    s.omb1 = omb1;
    s.beta2 = beta2;
    s.omb2 = omb2;
    s.bias2_sqrt = st->bias2_sqrt;
    s.eps = eps;
    const double bias1 = (double)st->bias1;
    const double lf = (double)(lr_factor_dev != nullptr ? *lr_factor_dev : lr_factor);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int t = opt_find(first, nt, item);
        const ph_optim_tensor e = tab[t];
        if (e.g == nullptr) continue;
        const int64_t off = (int64_t)(item - first[t]) * PH_OPTIM_CHUNK;
        const int64_t left = e.n - off;
        const int cnt = left < PH_OPTIM_CHUNK ? (int)left : PH_OPTIM_CHUNK;
        const double lr = e.lr * lf;
        s.decay = (float)(1.0 - lr * e.weight_decay);
        s.nstep = (float)(-(lr / bias1));
        float* p = e.p + off;
        float* g = e.g + off;
        float* m = e.m + off;
        float* v = e.v + off;
        int done = 0;
        if (opt_vec(e)) {
            const int n4 = cnt >> 2;
            if (skip) {
#pragma unroll
                for (int k = 0; k < OPT_V4; ++k) {
                    const int i = tid + k * OPT_T;
                    if (i < n4) ((float4*)g)[i] = zero4;
                }
            } else {
#pragma unroll
                for (int k = 0; k < OPT_V4; ++k) {
                    const int i = tid + k * OPT_T;
                    if (i < n4) {
                        float4 p4 = ((const float4*)p)[i], m4 = ((const float4*)m)[i], v4 = ((const float4*)v)[i];
                        const float4 g4 = ((const float4*)g)[i];
                        opt_element4(p4, g4, m4, v4, s);
                        ((float4*)p)[i] = p4;
                        ((float4*)m)[i] = m4;
                        ((float4*)v)[i] = v4;
                        if (zero_grads) ((float4*)g)[i] = zero4;
                    }
                }
            }
            done = n4 << 2;
        }
        for (int i = done + tid; i < cnt; i += OPT_T) {
            if (!skip) {
                float pe = p[i], me = m[i], ve = v[i];
                opt_element(pe, g[i], me, ve, s);
                p[i] = pe;
                m[i] = me;
                v[i] = ve;
            }
            if (zero_grads) g[i] = 0.f;
        }
    }
}

__global__ __launch_bounds__(OPT_T) void k_optim_zero(const ph_optim_tensor* __restrict__ tab, int nt, int nitems) {
    __shared__ int32_t first[PH_OPTIM_MAX_TENSORS];
    const int tid = threadIdx.x;
    opt_load_column(tab, nt, first);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int t = opt_find(first, nt, item);
        const ph_optim_tensor e = tab[t];
        if (e.g == nullptr) continue;
        const int64_t off = (int64_t)(item - first[t]) * PH_OPTIM_CHUNK;
        const int64_t left = e.n - off;
        const int cnt = left < PH_OPTIM_CHUNK ? (int)left : PH_OPTIM_CHUNK;
        float* g = e.g + off;
        int done = 0;
        if (((uintptr_t)e.g & 15) == 0) {
            const int n4 = cnt >> 2;
#pragma unroll
            for (int k = 0; k < OPT_V4; ++k) {
                const int i = tid + k * OPT_T;
                if (i < n4) ((float4*)g)[i] = zero4;
            }
            done = n4 << 2;
        }
        for (int i = done + tid; i < cnt; i += OPT_T) g[i] = 0.f;
    }
}

// every check of the table, in the header's order; -> the item count in *nitems
int opt_check_table(const char* fn, const ph_optim_tensor* tab, const ph_optim_tensor* tab_dev, int nt, int64_t* nitems) {
    PH_CHECK_ARG_AS(fn, nt > 0, "ntensors must be positive");
    PH_CHECK_ARG_AS(fn, tab != nullptr && tab_dev != nullptr, "null table_host / table_dev");
    if (nt > PH_OPTIM_MAX_TENSORS) {
        ph_set_error("%s: ntensors %d above PH_OPTIM_MAX_TENSORS %d", fn, nt, PH_OPTIM_MAX_TENSORS);
        return PH_EUNSUPPORTED;
    }
    PH_CHECK_ARG_AS(fn, ((uintptr_t)tab_dev & 7) == 0, "table_dev must be 8-byte aligned");
    int64_t items = 0;
    for (int i = 0; i < nt; ++i) {
        const ph_optim_tensor& e = tab[i];
        if (e.n < 0) {
            ph_set_error("%s: tensor %d: negative n", fn, i);
            return PH_EINVAL;
        }
        if (e.n > 0 && (e.p == nullptr || e.m == nullptr || e.v == nullptr)) {
            ph_set_error("%s: tensor %d: null p / m / v with n > 0", fn, i);
            return PH_EINVAL;
        }
        if ((((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v) & 3) != 0) {
            ph_set_error("%s: tensor %d: p / g / m / v must be 4-byte aligned", fn, i);
            return PH_EINVAL;
        }
        if (e.first_item != items) {
            ph_set_error("%s: tensor %d: first_item %lld is not the running item count %lld", fn, i, (long long)e.first_item, (long long)items);
            return PH_EINVAL;
        }
        items += (e.n + PH_OPTIM_CHUNK - 1) / PH_OPTIM_CHUNK;
        if (items > INT32_MAX) {
            ph_set_error("%s: more than 2^31 - 1 work items", fn);
            return PH_EUNSUPPORTED;
        }
    }
    *nitems = items;
    return PH_OK;
}

unsigned opt_blocks(int64_t nitems, int max_blocks) {
    const int cus = ph_num_cus();
    int64_t b = cus > 0 ? (int64_t)cus * 8 : 2048;           // memory-bound: 8 workgroups per CU, the rest by the grid-stride loop
    if (max_blocks > 0 && max_blocks < b) b = max_blocks;
    if (nitems < b) b = nitems;
    return (unsigned)(b > 0 ? b : 1);
}

size_t opt_workspace(int64_t nitems) { return al256((size_t)(nitems > 0 ? nitems : 1) * sizeof(double)); }

}  // namespace

extern "C" size_t ph_optim_workspace_bytes(const ph_optim_tensor* table_host, int ntensors) {
    int64_t nitems = 0;
    if (opt_check_table("ph_optim_workspace_bytes", table_host, table_host, ntensors, &nitems) != PH_OK) return 0;
    return opt_workspace(nitems);
}

extern "C" int ph_optim_step(const ph_optim_cfg* cfg, const ph_optim_tensor* table_host, const ph_optim_tensor* table_dev, int ntensors,
                             float lr_factor, const float* lr_factor_dev, ph_optim_state* state, void* workspace, size_t workspace_bytes,
                             void* stream) {
    PH_CHECK_ARG(cfg != nullptr, "null cfg");
    int64_t nitems = 0;
    PH_RUN(opt_check_table("ph_optim_step", table_host, table_dev, ntensors, &nitems));
    PH_CHECK_ARG(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0, "beta1 must lie in [0, 1)");
    PH_CHECK_ARG(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0, "beta2 must lie in [0, 1)");
    PH_CHECK_ARG(cfg->eps > 0.0, "eps must be positive");
    PH_CHECK_ARG(cfg->max_blocks >= 0, "max_blocks must not be negative");
    PH_CHECK_ARG(state != nullptr && ((uintptr_t)state & 7) == 0, "state must be a non-null, 8-byte aligned device pointer");
    PH_CHECK_ARG(((uintptr_t)lr_factor_dev & 3) == 0, "lr_factor_dev must be 4-byte aligned");
    PH_RUN(ph_check_buffers("ph_optim_step", nullptr, workspace, workspace_bytes, opt_workspace(nitems)));
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = opt_blocks(nitems, cfg->max_blocks);
    const bool want_norm = cfg->max_norm > 0.0 || (cfg->flags & PH_OPTIM_SKIP_NONFINITE) != 0;
    double* partial = (double*)workspace;
    if (want_norm && nitems > 0) hipLaunchKernelGGL(k_optim_sumsq, dim3(blocks), dim3(OPT_T), 0, s, table_dev, ntensors, (int)nitems, partial);
    hipLaunchKernelGGL(k_optim_finalize, dim3(1), dim3(OPT_T), 0, s, (const double*)partial, want_norm ? (int)nitems : 0, *cfg, state);
    if (nitems > 0)
        hipLaunchKernelGGL(k_optim_update, dim3(blocks), dim3(OPT_T), 0, s, table_dev, ntensors, (int)nitems, (const ph_optim_state*)state,
                           (float)cfg->beta2, (float)(1.0 - cfg->beta1), (float)(1.0 - cfg->beta2), (float)cfg->eps,
                           (cfg->flags & PH_OPTIM_ZERO_GRADS) != 0 ? 1 : 0, lr_factor, lr_factor_dev);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

extern "C" int ph_optim_zero_grads(const ph_optim_tensor* table_host, const ph_optim_tensor* table_dev, int ntensors, int max_blocks,
                                   void* stream) {
    int64_t nitems = 0;
    PH_RUN(opt_check_table("ph_optim_zero_grads", table_host, table_dev, ntensors, &nitems));
    PH_CHECK_ARG(max_blocks >= 0, "max_blocks must not be negative");
    if (nitems > 0)
        hipLaunchKernelGGL(k_optim_zero, dim3(opt_blocks(nitems, max_blocks)), dim3(OPT_T), 0, (hipStream_t)stream, table_dev, ntensors, (int)nitems);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
