// The backbone as a native object (include/polyhead.h ph_resnet_cfg .. ph_resnet_plan_run): the BatchNorm fold and the weight packing
// of resnet.ResNet._pack in one kernel of its own (k_resnet_pack: the shared packer's table holds 30 pointers, its tap addressing
// assumes 256 input channels and it does not fold), and the block table, the buffer plan and the launch sequence of engine.ResNetPlan.
// The host code calls the public entry points of ph_resnet.hip on the caller's stream; pack / create / run allocate no device
// memory, do not synchronise and read no environment variable.  Bytes / layout / workspace / create / geometry-of / info are the
// shared scaffold's (ph_plan_inl.h); the pack call is this file's.
#include <algorithm>
#include <string>
#include <vector>

#include "ph_plan_inl.h"

#pragma clang fp contract(off)

constexpr int RN_STEM_K = 176;          // resnet.STEM_K: 7 kernel rows x 24 (21 values (kw, c) + 3 zeros) = 168, padded to 16

// ---------------------------------------------------------------------------------------------
// k_resnet_pack: one convolution's two pieces and the padding behind each, [u0, u0 + total_u) in 16-byte units of the pack; every
// unit is written by one thread with one 16-byte store (the padding as zeros, so two packings of the same weights are byte-equal).
// What resnet.fold_bn -> permute(0, 2, 3, 1).reshape (or stem_matrix) -> engine._planes_of(., 1, f16) -> pack.pack_b32 do on the host:
//   s[n] = gamma[n] / sqrt(var[n] + eps) in float64 from the fp32 inputs widened to double
//   W'   = fp32(w * s) (the product in float64, rounded once), then rounded to the grade: the double rounding is _planes_of's
//   b'   = fp32(beta - mean * s), the product and the difference both rounded in float64 (no FMA: contract(off) above)
// A W unit is 8 consecutive k of one row of W2 [rows][K]: fragment order [ct][ks][g][n][e] holds W2[32 ct + n][16 ks + 8 g + e]; rows
// at or above Cout (a channel tile of 32 that Cout does not fill) are zero.  k = tap * Cin + c of a parameter stored [n][c][tap]:
// Cin is a multiple of 8, so a unit lies in one tap and its 8 sources are `taps` floats apart.  Stem: k = 24 kh + 3 kw + c.
struct RPArgs {
    const float *w, *gamma, *beta, *mean, *var;
    double eps;
    uint32_t w_units, w_end;             // W: units that carry data, units up to the b piece
    uint32_t b_units, total_u;           // b likewise, from w_end
    int Cout, Cin, taps, K, stem, f16;
};

__device__ __forceinline__ double rp_scale(const RPArgs& a, int n) { return (double)a.gamma[n] / sqrt((double)a.var[n] + a.eps); }

__global__ __launch_bounds__(256) void k_resnet_pack(const RPArgs a, uint4* __restrict__ pack) {
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < a.total_u; u += gridDim.x * 256u) {
        uint4 out = make_uint4(0u, 0u, 0u, 0u);
        if (u < a.w_units) {
            const uint32_t i = u * 8u, KS = (uint32_t)a.K / 16u, n = (i >> 3) & 31u, gq = (i >> 8) & 1u, r = i >> 9;
            const int row = (int)(32u * (r / KS) + n), kk = (int)(16u * (r % KS) + 8u * gq);
            if (row < a.Cout) {
                const double s = rp_scale(a, row);
                uint32_t v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float w32 = 0.f;
                    if (a.stem) {
                        const int k = kk + e, kh = k / 24, j = k - kh * 24, kw = j / 3, c = j - kw * 3;
                        if (k < 168 && j < 21) w32 = (float)((double)a.w[((row * 3 + c) * 7 + kh) * 7 + kw] * s);
                    } else {
                        const int tap = kk / a.Cin, c = kk - tap * a.Cin + e;
                        w32 = (float)((double)a.w[((size_t)row * a.Cin + c) * a.taps + tap] * s);
                    }
                    v[e] = a.f16 ? f2h(w32) : f2bf(w32);
                }
                out = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
            }
        } else if (u >= a.w_end && u - a.w_end < a.b_units) {
            uint32_t v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = (int)(u - a.w_end) * 4 + e;
                v[e] = n < a.Cout ? __float_as_uint((float)((double)a.beta[n] - (double)a.mean[n] * rp_scale(a, n))) : 0u;
            }
            out = make_uint4(v[0], v[1], v[2], v[3]);
        }
        pack[u] = out;
    }
}

// ---------------------------------------------------------------------------------------------
// the block table (resnet.ResNet.block_table): convolutions in state_dict order -- the stem, then per block conv1, conv2, conv3 and,
// where the block has one, the downsample
struct RConv {
    int ks, stride, cin, cout, relu;
    int stage, block, which;             // which: 0 .. 2 = conv1 .. conv3, 3 = downsample; the stem: stage -1
    int h, w;                            // input size
    int src, res, dst;                   // workspace planes of its launch (RBuf; res -1: none)
};
enum RBuf { RB_P0, RB_PA, RB_PB, RB_T1, RB_T2, RB_PD, RB_COUNT };

static const int* arch_of(int depth) {
    static const int a50[4] = {3, 4, 6, 3}, a101[4] = {3, 4, 23, 3}, a152[4] = {3, 8, 36, 3};
    return depth == 50 ? a50 : depth == 101 ? a101 : depth == 152 ? a152 : nullptr;
}

static int nconvs_of(const int* arch) { return 1 + 3 * (arch[0] + arch[1] + arch[2] + arch[3]) + 4; }

// `cv` in state_dict order, sizes and planes left for resolve()
static int build_convs(const int* arch, RConv* cv) {
    int n = 0, inpl = 64;
    cv[n++] = RConv{7, 2, 3, 64, 1, -1, 0, 0};
    for (int si = 0; si < 4; ++si) {
        const int planes = 64 << si;
        for (int j = 0; j < arch[si]; ++j) {
            const int s = (j == 0 && si > 0) ? 2 : 1, cin = j == 0 ? inpl : 4 * planes;
            cv[n++] = RConv{1, 1, cin, planes, 1, si, j, 0};
            cv[n++] = RConv{3, s, planes, planes, 1, si, j, 1};
            cv[n++] = RConv{1, 1, planes, 4 * planes, 1, si, j, 2};
            if (j == 0) cv[n++] = RConv{1, s, cin, 4 * planes, 0, si, j, 3};
        }
        inpl = 4 * planes;
    }
    return n;
}

// parameter 5 c + j: convolution c's weight (j = 0), then its norm's weight, bias, running_mean, running_var; one table per depth,
// built on first use
static std::vector<std::string> make_names(int depth) {
    static const char* const bn[4] = {"weight", "bias", "running_mean", "running_var"};
    std::vector<std::string> t;
    RConv cv[PH_RESNET_MAX_CONVS];
    const int n = build_convs(arch_of(depth), cv);
    for (int c = 0; c < n; ++c) {
        const std::string pre = cv[c].stage < 0 ? "" : "layer" + std::to_string(cv[c].stage + 1) + "." + std::to_string(cv[c].block) + ".";
        const std::string k = std::to_string(cv[c].which + 1);
        t.push_back(pre + (cv[c].which == 3 ? "downsample.0" : "conv" + k) + ".weight");
        for (int j = 0; j < 4; ++j) t.push_back(pre + (cv[c].which == 3 ? "downsample.1" : "bn" + k) + "." + bn[j]);
    }
    return t;
}

static const std::vector<std::string>* names_of(int depth) {
    static const std::vector<std::string> t50 = make_names(50), t101 = make_names(101), t152 = make_names(152);
    return depth == 50 ? &t50 : depth == 101 ? &t101 : depth == 152 ? &t152 : nullptr;
}

// ---------------------------------------------------------------------------------------------
// geometry: resolve() is the one rule of the native plan (cfg checks, pack pieces, workspace pieces, launch sequence)
struct RGeo {
    int B, H, W, depth, prec, x_dtype, out_dtype, out_mask, last;       // last: the highest stage run
    double eps;
    int nconvs;                          // of the depth (the pack's)
    RConv cv[PH_RESNET_MAX_CONVS];       // state_dict order
    int order[PH_RESNET_MAX_CONVS];      // convolutions 1 .. nconvs - 1 in launch order
    int stage_first[5];                  // stage si's launches: order[stage_first[si] .. stage_first[si + 1])
    int stage_src[4];                    // the plane that holds stage si's result
    int c[4], h[4], w[4];
    int stem_wg, conv_wg[PH_RESNET_MAX_CONVS], nchw_wg[4];               // conv_wg by convolution index
    size_t o_buf[RB_COUNT], total;       // workspace pieces
    ph_resnet_layout lay;                // pack pieces
    size_t pack_total;
};

// a workgroup query of ph_resnet.hip (asked with the error string cleared) refused the size: its words under this call's name; it
// has none when the count alone is too large
static int refused(const char* fn) {
    const std::string why = ph_last_error_string() ? ph_last_error_string() : "";
    if (!why.empty()) { ph_set_error("%s: H, W: %s", fn, why.c_str()); return PH_EINVAL; }
    ph_set_error("%s: B, H, W: a launch of this size has more than 2^31 - 1 workgroups", fn);
    return PH_EUNSUPPORTED;
}

static int resolve(const ph_resnet_cfg* c, RGeo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = RGeo{};
    g.B = c->B; g.H = c->H; g.W = c->W; g.depth = c->depth; g.eps = c->eps;
    if (!(g.B > 0)) { ph_set_error("%s: bad size (B > 0)", fn); return PH_EINVAL; }
    if (g.B > 4096) { ph_set_error("%s: B: at most 4096 frames per call", fn); return PH_EUNSUPPORTED; }
    if (!(g.H > 0 && g.W > 0)) { ph_set_error("%s: bad size (H, W > 0)", fn); return PH_EINVAL; }
    const int* arch = arch_of(g.depth);
    if (!arch) { ph_set_error("%s: depth = %d: the Bottleneck depths 50, 101 and 152 are built", fn, g.depth); return PH_EUNSUPPORTED; }
    g.prec = ph_mode_grade(c->mode);
    if (g.prec < 0) { ph_set_error("%s: bad mode", fn); return PH_EINVAL; }
    if (g.prec == PH_PREC_SPLIT) {
        ph_set_error("%s: mode = %d: the backbone has one-plane grades only (PH_MODE_BF16, PH_MODE_FP16); a hi + lo grade is not built", fn,
                     c->mode);
        return PH_EUNSUPPORTED;
    }
    g.x_dtype = c->x_dtype; g.out_dtype = c->out_dtype; g.out_mask = c->out_mask;
    if (!(g.x_dtype == PH_OUT_F32 || g.x_dtype == PH_OUT_BF16)) { ph_set_error("%s: x_dtype must be PH_OUT_F32 or PH_OUT_BF16", fn); return PH_EINVAL; }
    if (!(g.out_dtype == PH_OUT_F32 || g.out_dtype == PH_OUT_BF16 || g.out_dtype == PH_OUT_F16)) {
        ph_set_error("%s: out_dtype must be PH_OUT_F32, PH_OUT_BF16 or PH_OUT_F16", fn);
        return PH_EINVAL;
    }
    if (!(g.out_mask > 0 && g.out_mask < 16)) { ph_set_error("%s: out_mask = %d: must be non-zero and within the low 4 bits", fn, g.out_mask); return PH_EINVAL; }
    if (!(g.eps >= 0 && g.eps < 1e300)) { ph_set_error("%s: eps must be finite and >= 0", fn); return PH_EINVAL; }
    for (int i = 0; i < 4; ++i)
        if (g.out_mask >> i & 1) g.last = i;

    // the block table, its sizes, planes and launch order (engine.ResNetPlan)
    g.nconvs = build_convs(arch, g.cv);
    ph_set_error("%s", "");
    g.stem_wg = ph_resnet_stem_workgroups(g.H, g.W, g.B);
    if (g.stem_wg <= 0) return refused(fn);
    int h = ((g.H - 1) / 2 + 1 - 1) / 2 + 1, w = ((g.W - 1) / 2 + 1 - 1) / 2 + 1;       // engine.stem_out_size
    g.cv[0].h = g.H; g.cv[0].w = g.W; g.cv[0].src = -1; g.cv[0].res = -1; g.cv[0].dst = RB_P0;
    size_t io = 0, inner = 0, down = 0;
    int cur = RB_P0, nxt = RB_PA, n = 1, no = 0;
    for (int si = 0; si < 4; ++si) {
        g.stage_first[si] = no;
        for (int j = 0; j < arch[si]; ++j) {
            RConv *c1 = &g.cv[n], *c2 = c1 + 1, *c3 = c1 + 2, *cd = j == 0 ? c1 + 3 : nullptr;
            const int s = c2->stride, ho = (h + 2 - 3) / s + 1, wo = (w + 2 - 3) / s + 1, planes = c2->cout;     // engine.conv_out_size
            c1->h = c2->h = h; c1->w = c2->w = w; c3->h = ho; c3->w = wo;
            c1->src = cur; c1->res = -1; c1->dst = RB_T1;
            c2->src = RB_T1; c2->res = -1; c2->dst = RB_T2;
            c3->src = RB_T2; c3->res = cd ? RB_PD : cur; c3->dst = nxt;
            g.order[no++] = n; g.order[no++] = n + 1;
            if (cd) { cd->h = h; cd->w = w; cd->src = cur; cd->res = -1; cd->dst = RB_PD; g.order[no++] = n + 3; }
            g.order[no++] = n + 2;
            const size_t in_px = (size_t)h * w, out_px = (size_t)ho * wo;
            inner = std::max(inner, std::max(in_px, out_px) * planes);
            io = std::max(io, out_px * 4 * planes);
            if (cd) down = std::max(down, out_px * 4 * planes);
            n += cd ? 4 : 3;
            cur = nxt; nxt = nxt == RB_PA ? RB_PB : RB_PA;
            h = ho; w = wo;
        }
        g.stage_src[si] = cur;
        g.c[si] = 256 << si; g.h[si] = h; g.w[si] = w;
    }
    g.stage_first[4] = no;
    for (int i = 1; i < g.nconvs; ++i) {
        const RConv& v = g.cv[i];
        g.conv_wg[i] = ph_conv_cl_workgroups(v.ks, v.stride, v.cin, v.cout, v.h, v.w, g.B);
        if (g.conv_wg[i] <= 0) return refused(fn);
    }
    for (int si = 0; si < 4; ++si) {
        g.nchw_wg[si] = ph_cl_to_nchw_workgroups(g.B, (int64_t)g.h[si] * g.w[si], g.c[si]);
        if (g.nchw_wg[si] <= 0) return refused(fn);
    }

    // pack pieces (resnet.ResNet._pack): per convolution W, then b
    size_t o = 0;
    for (int i = 0; i < g.nconvs; ++i) {
        const RConv& v = g.cv[i];
        const uint64_t K = i ? (uint64_t)v.ks * v.ks * v.cin : RN_STEM_K, rows = ((uint64_t)v.cout + 31) / 32 * 32;
        g.lay.bytes[PH_RPACK_W(i)] = rows * K * 2;
        g.lay.bytes[PH_RPACK_B(i)] = (uint64_t)v.cout * 4;
        for (int pc = PH_RPACK_W(i); pc <= PH_RPACK_B(i); ++pc) { g.lay.offset[pc] = o; o += al256(g.lay.bytes[pc]); }
    }
    g.lay.nconvs = g.nconvs;
    g.pack_total = o;

    // workspace (engine.ResNetPlan's buffers)
    const size_t B = g.B, p0 = (size_t)g.h[0] * g.w[0] * 64;             // layer1 keeps the stem's size
    const size_t elems[RB_COUNT] = {p0, io, io, inner, inner, std::max(down, (size_t)8)};
    o = 0;
    for (int b = 0; b < RB_COUNT; ++b) { g.o_buf[b] = o; o += al256(B * elems[b] * 2); }
    g.total = o;
    return PH_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" int ph_resnet_nparams(const ph_resnet_cfg* cfg) {
    const int* arch = cfg ? arch_of(cfg->depth) : nullptr;
    return arch ? 5 * nconvs_of(arch) : PH_EINVAL;
}

extern "C" const char* ph_resnet_param_name(const ph_resnet_cfg* cfg, int index) {
    const std::vector<std::string>* t = cfg ? names_of(cfg->depth) : nullptr;
    return t && index >= 0 && index < (int)t->size() ? (*t)[index].c_str() : nullptr;
}

extern "C" int64_t ph_resnet_param_numel(const ph_resnet_cfg* cfg, int index) {
    const int* arch = cfg ? arch_of(cfg->depth) : nullptr;
    if (!arch || index < 0 || index >= 5 * nconvs_of(arch)) return -1;
    RConv cv[PH_RESNET_MAX_CONVS];
    build_convs(arch, cv);
    const RConv& v = cv[index / 5];
    return index % 5 ? v.cout : (int64_t)v.cout * v.cin * v.ks * v.ks;
}

static void fill_geometry(const RGeo& g, ph_resnet_geometry* out) {
    *out = ph_resnet_geometry{};
    out->prec = g.prec;
    out->nconvs = g.stage_first[g.last + 1];
    out->stem_workgroups = g.stem_wg;
    int written = 0;
    for (int si = 0; si < 4; ++si) {
        out->c[si] = g.c[si]; out->h[si] = g.h[si]; out->w[si] = g.w[si];
        if (g.out_mask >> si & 1) { out->nchw_workgroups[si] = g.nchw_wg[si]; ++written; }
    }
    for (int i = 0; i < out->nconvs; ++i) out->conv_workgroups[i] = g.conv_wg[g.order[i]];
    out->launches = 1 + out->nconvs + written;
}

struct ph_resnet_plan {
    RGeo g;
    const char* pack;
    char* ws;
};

// the family's description for the shared scaffold (no build_table / kPackBlocks: the pack call is ph_resnet_pack's own)
struct ResNetFam {
    typedef ph_resnet_cfg Cfg; typedef RGeo Geo; typedef ph_resnet_layout Layout; typedef ph_resnet_geometry Geometry; typedef ph_resnet_plan Plan;
    static constexpr auto resolve = &::resolve;
    static constexpr auto fill_geometry = &::fill_geometry;
};

extern "C" size_t ph_resnet_pack_bytes(const ph_resnet_cfg* cfg) { return plan::pack_bytes<ResNetFam>(cfg, __func__); }

extern "C" int ph_resnet_pack_layout(const ph_resnet_cfg* cfg, ph_resnet_layout* layout) {
    return plan::pack_layout<ResNetFam>(cfg, layout, __func__);
}

// one launch per convolution: its pointers travel by value, and each launch writes every unit from its W piece to the next convolution's
extern "C" int ph_resnet_pack(const ph_resnet_cfg* cfg, const float* const* params, void* pack, void* stream) {
    RGeo g;
    PH_RUN(resolve(cfg, g, __func__));
    PH_CHECK_ARG(params && pack, "null params or pack");
    for (int i = 0; i < 5 * g.nconvs; ++i)
        if (!params[i]) { ph_set_error("%s: parameter %d (%s) is NULL", __func__, i, ph_resnet_param_name(cfg, i)); return PH_EINVAL; }
    PH_CHECK_ARG(((uintptr_t)pack & 255) == 0, "pack must be 256-byte aligned");
    PH_CHECK_ARG(g.pack_total / 16 < (1ull << 32), "pack too large");
    for (int i = 0; i < g.nconvs; ++i) {
        const RConv& v = g.cv[i];
        const uint64_t *off = g.lay.offset, *by = g.lay.bytes;
        const uint64_t end = i + 1 < g.nconvs ? off[PH_RPACK_W(i + 1)] : g.pack_total;
        RPArgs a{params[5 * i], params[5 * i + 1], params[5 * i + 2], params[5 * i + 3], params[5 * i + 4], g.eps,
                 (uint32_t)(by[PH_RPACK_W(i)] / 16), (uint32_t)((off[PH_RPACK_B(i)] - off[PH_RPACK_W(i)]) / 16),
                 (uint32_t)((by[PH_RPACK_B(i)] + 15) / 16), (uint32_t)((end - off[PH_RPACK_W(i)]) / 16),
                 v.cout, v.cin, v.ks * v.ks, i ? v.ks * v.ks * v.cin : RN_STEM_K, i == 0, g.prec == PH_PREC_F16};
        const unsigned blocks = (a.total_u + 255u) / 256u;
        hipLaunchKernelGGL(k_resnet_pack, dim3(blocks < 2048u ? blocks : 2048u), dim3(256), 0, (hipStream_t)stream, a,
                           (uint4*)((char*)pack + off[PH_RPACK_W(i)]));
        PH_CHECK_LAUNCH();
    }
    return PH_OK;
}

extern "C" size_t ph_resnet_plan_workspace_bytes(const ph_resnet_cfg* cfg) { return plan::workspace_bytes<ResNetFam>(cfg, __func__); }

extern "C" int ph_resnet_plan_create(const ph_resnet_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes,
                                     ph_resnet_plan** out) {
    return plan::create<ResNetFam>(cfg, pack, workspace, workspace_bytes, out, __func__);
}

extern "C" int ph_resnet_geometry_of(const ph_resnet_cfg* cfg, ph_resnet_geometry* out) {
    return plan::geometry_of<ResNetFam>(cfg, out, __func__);
}

extern "C" int ph_resnet_plan_info(const ph_resnet_plan* p, ph_resnet_geometry* out) { return plan::info<ResNetFam>(p, out, __func__); }

extern "C" void ph_resnet_plan_destroy(ph_resnet_plan* p) { delete p; }

// ---------------------------------------------------------------------------------------------
// every pointer check of the three run calls, before any of them launches; stage < 0: all that run
static int check_io(const RGeo& g, const ph_resnet_io* io, const char* fn, bool image, bool outs, int stage) {
    if (image && !io->image) { ph_set_error("%s: null image", fn); return PH_EINVAL; }
    for (int si = 0; outs && si <= g.last; ++si) {
        if (!(g.out_mask >> si & 1) || (stage >= 0 && stage != si)) continue;
        if (!io->stages[si]) { ph_set_error("%s: the cfg's out_mask needs stages[%d]", fn, si); return PH_EINVAL; }
        if ((uintptr_t)io->stages[si] & 3) { ph_set_error("%s: stages[%d] must be 4-byte aligned", fn, si); return PH_EINVAL; }
    }
    return PH_OK;
}

static uint16_t* plane(const ph_resnet_plan* p, int b) { return b < 0 ? nullptr : (uint16_t*)(p->ws + p->g.o_buf[b]); }

static int run_stem(const ph_resnet_plan* p, const ph_resnet_io* io, void* s) {
    const RGeo& g = p->g;
    return ph_resnet_stem(io->image, g.x_dtype, (const uint16_t*)(p->pack + g.lay.offset[PH_RPACK_W(0)]),
                          (const float*)(p->pack + g.lay.offset[PH_RPACK_B(0)]), plane(p, RB_P0), g.B, g.H, g.W, g.prec, s);
}

static int run_stage(const ph_resnet_plan* p, int si, const ph_resnet_io* io, void* s) {
    const RGeo& g = p->g;
    for (int q = g.stage_first[si]; q < g.stage_first[si + 1]; ++q) {
        const int i = g.order[q];
        const RConv& v = g.cv[i];
        PH_RUN(ph_conv_cl(plane(p, v.src), (const uint16_t*)(p->pack + g.lay.offset[PH_RPACK_W(i)]),
                          (const float*)(p->pack + g.lay.offset[PH_RPACK_B(i)]), plane(p, v.res), plane(p, v.dst), v.ks, v.stride, v.relu, g.B,
                          v.h, v.w, v.cin, v.cout, g.prec, s));
    }
    if (g.out_mask >> si & 1)
        return ph_cl_to_nchw(plane(p, g.stage_src[si]), io->stages[si], g.out_dtype, g.B, (int64_t)g.h[si] * g.w[si], g.c[si], g.prec, s);
    return PH_OK;
}

extern "C" int ph_resnet_plan_run_stem(ph_resnet_plan* p, const ph_resnet_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_RUN(check_io(p->g, io, __func__, true, false, -1));
    return run_stem(p, io, stream);
}

extern "C" int ph_resnet_plan_run_stage(ph_resnet_plan* p, int stage, const ph_resnet_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_CHECK_ARG(stage >= 0 && stage < 4, "stage must be 0 .. 3");
    PH_RUN(check_io(p->g, io, __func__, false, true, stage));
    return run_stage(p, stage, io, stream);
}

extern "C" int ph_resnet_plan_run(ph_resnet_plan* p, const ph_resnet_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_RUN(check_io(p->g, io, __func__, true, true, -1));
    PH_RUN(run_stem(p, io, stream));
    for (int si = 0; si <= p->g.last; ++si) PH_RUN(run_stage(p, si, io, stream));
    return PH_OK;
}
