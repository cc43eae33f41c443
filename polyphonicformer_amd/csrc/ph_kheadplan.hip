// A1 as a native object (include/polyhead.h ph_khead_cfg .. ph_khead_plan_timeouts): the parameter packing of
// engine.KernelHeadPack as one HIP kernel, and the geometry rules, the buffer plan and the launch sequence of
// engine.KernelHeadPlan.  Host code only calls the other entry points of this library, on the caller's stream; pack / create /
// run allocate no device memory, do not synchronise and read no environment variable.  The pack / create / info scaffold is the
// shared one (ph_plan_inl.h).
#include "ph_plan_inl.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// parameter table (polyhead.h: the reference's state_dict names of KernelHead's own layers)
static const char* const kParamNames[PH_KHEAD_NPARAMS] = {
    "loc_convs.0.conv.weight", "loc_convs.0.gn.weight", "loc_convs.0.gn.bias",
    "seg_convs.0.conv.weight", "seg_convs.0.gn.weight", "seg_convs.0.gn.bias",
    "depth_convs.0.conv.weight", "depth_convs.0.gn.weight", "depth_convs.0.gn.bias",
    "init_kernels.weight", "conv_seg.weight", "conv_seg.bias", "conv_direct_depth.weight", "conv_direct_depth.bias"};
enum { P_CONV = 0, P_INIT = 9, P_SEG = 10, P_SEG_B = 11, P_DD = 12, P_DD_B = 13 };

static int64_t param_numel(const ph_khead_cfg* c, int i) {
    if (i < 0 || i >= PH_KHEAD_NPARAMS) return -1;
    if (i < P_INIT) return i % 3 == 0 ? 256 * 256 : 256;
    if (i == P_INIT) return (int64_t)c->num_proposals * 256;
    if (i == P_SEG) return (int64_t)c->num_classes * 256;
    if (i == P_SEG_B) return c->num_classes;
    return i == P_DD ? 256 : 1;
}

// ---------------------------------------------------------------------------------------------
// geometry: resolve() is the ONE launch-geometry rule of a1 -- the native plan's and, through ph_khead_geometry_of,
// engine.KernelHeadPlan's; the environment switches of the Python side arrive as the cfg's fields (engine.native_khead_cfg)
struct KGeo {
    int B, H, W, Nq, n_seg, n_thing, n_stuff, N, Npad, NqPad, groups, prec, P, logit_dtype, logit_bytes, emit_f32, onepass, nsplit;
    int64_t HW, HWp;
    size_t ws1_bytes, ws2_bytes, o_ws1, o_ws2, o_partial, total;     // workspace pieces
    ph_khead_layout lay;                                             // pack pieces
    size_t pack_total;
};

// `need_device`: the one-pass rule asks the current device for its CU count; the pack entry points do not need it
static int resolve(const ph_khead_cfg* c, KGeo& g, const char* fn, bool need_device) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = KGeo{};
    g.B = c->B; g.H = c->H; g.W = c->W; g.Nq = c->num_proposals; g.n_seg = c->num_classes; g.n_thing = c->num_thing_classes;
    g.groups = c->groups;
    if (!(g.B > 0 && g.H > 0 && g.W > 0)) { ph_set_error("%s: bad size (B, H, W > 0)", fn); return PH_EINVAL; }
    if ((int64_t)g.H * g.W > (1ll << 30)) { ph_set_error("%s: H * W must be <= 2^30", fn); return PH_EUNSUPPORTED; }
    if (g.B > 4096) { ph_set_error("%s: at most 4096 frames per call", fn); return PH_EUNSUPPORTED; }
    if (!(g.Nq > 0 && g.Nq <= 256)) { ph_set_error("%s: num_proposals must be 1 .. 256", fn); return PH_EINVAL; }
    if (!(g.n_seg > 0 && g.n_seg <= 256)) { ph_set_error("%s: num_classes must be 1 .. 256", fn); return PH_EINVAL; }
    if (!(g.n_thing >= 0 && g.n_thing <= g.n_seg)) { ph_set_error("%s: num_thing_classes must be 0 .. num_classes", fn); return PH_EINVAL; }
    if (!(g.groups > 0 && 256 % g.groups == 0)) { ph_set_error("%s: groups must divide 256", fn); return PH_EINVAL; }
    g.prec = ph_mode_grade(c->mode);
    if (g.prec < 0) { ph_set_error("%s: bad mode", fn); return PH_EINVAL; }
    g.P = g.prec == PH_PREC_SPLIT ? 2 : 1;
    if (!(c->logit_dtype == PH_OUT_F32 || c->logit_dtype == PH_OUT_F16)) { ph_set_error("%s: logit_dtype must be PH_OUT_F32 or PH_OUT_F16", fn); return PH_EINVAL; }
    if (!(c->onepass == PH_KNOB_AUTO || c->onepass == PH_KNOB_ON || c->onepass == PH_KNOB_OFF) || c->nsplit < 0) {
        ph_set_error("%s: bad knob value (onepass: PH_KNOB_AUTO / _ON / _OFF, nsplit >= 0)", fn);
        return PH_EINVAL;
    }
    g.logit_dtype = c->logit_dtype;
    g.logit_bytes = c->logit_dtype == PH_OUT_F32 ? 4 : 2;
    g.emit_f32 = c->emit_f32 ? 1 : 0;
    g.n_stuff = c->cat_stuff ? g.n_seg - g.n_thing : 0;
    g.N = g.Nq + g.n_stuff;
    if (g.N > 256) { ph_set_error("%s: num_proposals + stuff rows must be <= 256", fn); return PH_EUNSUPPORTED; }
    g.Npad = ph_n_padded(g.N);
    g.NqPad = ph_n_padded(g.Nq);
    g.HW = (int64_t)g.H * g.W;
    g.HWp = ph_hw_padded(g.HW);
    if ((int64_t)g.B * g.Npad > 65535) { ph_set_error("%s: B * Npad must be <= 65535", fn); return PH_EUNSUPPORTED; }
    g.nsplit = c->nsplit ? c->nsplit : ph_pool_default_nsplit(g.B, g.HW, c->frame_invariant != 0);
    if (g.nsplit > g.HWp / 64) { ph_set_error("%s: nsplit out of range (at most H*W / 64 rounded up to 128)", fn); return PH_EINVAL; }

    // pack pieces (engine.KernelHeadPack)
    const size_t P = g.P, r_init = g.NqPad, r_seg = ph_n_padded(g.n_seg);
    uint64_t* by = g.lay.bytes;
    by[PH_KPACK_WPLANES] = P * 3 * 256 * 256 * 2;
    by[PH_KPACK_GN] = 3 * 2 * 256 * 4;
    by[PH_KPACK_INIT_PLANES] = by[PH_KPACK_INIT_FRAG] = P * r_init * 256 * 2;
    by[PH_KPACK_SEG_PLANES] = by[PH_KPACK_SEG_FRAG] = P * r_seg * 256 * 2;
    by[PH_KPACK_DD_PLANES] = by[PH_KPACK_DD_FRAG] = P * 32 * 256 * 2;
    by[PH_KPACK_SEG_BIAS] = r_seg * 4;
    by[PH_KPACK_DD_BIAS] = 32 * 4;
    by[PH_KPACK_CONV_FRAG] = g.P == 1 ? (size_t)3 * 256 * 256 * 2 : 0;
    by[PH_KPACK_W_INIT_F32] = (size_t)g.Nq * 256 * 4;
    by[PH_KPACK_W_SEG_F32] = (size_t)g.n_seg * 256 * 4;
    by[PH_KPACK_W_DD_F32] = 256 * 4;
    size_t o = 0;
    for (int i = 0; i < PH_KPACK_COUNT; ++i) { g.lay.offset[i] = o; o += al256(by[i]); }
    g.pack_total = o;
    if (!need_device) return PH_OK;

    // one pass or two (engine.KernelHeadPlan: the fp32 input form has the stricter condition, HW % 4 == 0)
    const bool sup = ph_khead_onepass_supported(g.B, g.HW, g.groups, g.prec, PH_IN_F32_NCHW) != 0;
    if (c->onepass == PH_KNOB_ON && !sup) {
        ph_set_error("%s: ph_khead_onepass cannot run this geometry / grade on the current device (H*W / 128 rounded up <= CUs, "
                     "32 groups, a one-plane grade, H*W %% 4 == 0)", fn);
        return PH_EUNSUPPORTED;
    }
    g.onepass = c->onepass != PH_KNOB_OFF && sup;
    if (g.logit_dtype != PH_OUT_F32 && !g.onepass) {
        ph_set_error("%s: 16-bit KernelHead logits need the one-pass form", fn);
        return PH_EUNSUPPORTED;
    }
    // workspace: [one-pass hand-off state] [two-pass workspace] [pooled partial sums]
    g.ws1_bytes = g.onepass ? ph_khead_onepass_workspace_bytes(g.B, g.HW) : 0;
    g.ws2_bytes = ph_khead_workspace_bytes(g.B, g.HW, g.groups);
    o = 0;
    g.o_ws1 = o; o += al256(g.ws1_bytes);
    g.o_ws2 = o; o += al256(g.ws2_bytes);
    g.o_partial = o; o += al256((size_t)g.B * g.nsplit * g.NqPad * 512 * 4);
    g.total = o;
    return PH_OK;
}

// ---------------------------------------------------------------------------------------------
// the pack's pieces for ph_pack_pieces (engine.KernelHeadPack's tensors)
static void build_table(const KGeo& g, PhPackTable& t) {
    auto set = [&](int piece, int kind, int first, int pstep, int nmat, int rows32, int rows_valid) {
        ph_pack_piece(t, g.lay.offset, g.lay.bytes, piece, kind, first, kind == PH_PIECE_FRAG32 ? 1 : 0, rows32, 256, rows_valid, nmat, pstep);
    };
    const int r_seg = ph_n_padded(g.n_seg);
    set(PH_KPACK_WPLANES, PH_PIECE_PLANES, P_CONV, 3, 3, 256, 256);
    set(PH_KPACK_GN, PH_PIECE_GN, 0, 0, 1, 0, 0);
    set(PH_KPACK_INIT_PLANES, PH_PIECE_PLANES, P_INIT, 0, 1, g.NqPad, g.Nq);
    set(PH_KPACK_SEG_PLANES, PH_PIECE_PLANES, P_SEG, 0, 1, r_seg, g.n_seg);
    set(PH_KPACK_DD_PLANES, PH_PIECE_PLANES, P_DD, 0, 1, 32, 1);
    set(PH_KPACK_SEG_BIAS, PH_PIECE_BIAS, P_SEG_B, 0, 1, 0, g.n_seg);
    set(PH_KPACK_DD_BIAS, PH_PIECE_BIAS, P_DD_B, 0, 1, 0, 1);
    set(PH_KPACK_INIT_FRAG, PH_PIECE_FRAG32, P_INIT, 0, 1, g.NqPad, g.Nq);
    set(PH_KPACK_SEG_FRAG, PH_PIECE_FRAG32, P_SEG, 0, 1, r_seg, g.n_seg);
    set(PH_KPACK_DD_FRAG, PH_PIECE_FRAG32, P_DD, 0, 1, 32, 1);
    set(PH_KPACK_CONV_FRAG, PH_PIECE_FRAG32, P_CONV, 3, 3, 256, 256);
    set(PH_KPACK_W_INIT_F32, PH_PIECE_F32, P_INIT, 0, 1, 0, 0);
    set(PH_KPACK_W_SEG_F32, PH_PIECE_F32, P_SEG, 0, 1, 0, 0);
    set(PH_KPACK_W_DD_F32, PH_PIECE_F32, P_DD, 0, 1, 0, 0);
    t.npieces = PH_KPACK_COUNT;
    t.total_u = (uint32_t)(g.pack_total / 16);
    t.f16 = g.prec == PH_PREC_F16;
}

// conv_direct_depth.weight into every row of depth_proposal [rows][256] (kernel_head.py:286-289, the dense form of the view)
__global__ __launch_bounds__(256) void k_khead_depth_proposal(const float4* __restrict__ w_dd, float4* __restrict__ out, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) out[i] = w_dd[i & 63];
}

// ---------------------------------------------------------------------------------------------
extern "C" const char* ph_khead_param_name(int index) {
    return index >= 0 && index < PH_KHEAD_NPARAMS ? kParamNames[index] : nullptr;
}

extern "C" int64_t ph_khead_param_numel(const ph_khead_cfg* cfg, int index) {
    if (!cfg) return -1;
    return param_numel(cfg, index);
}

static void fill_geometry(const KGeo& g, ph_khead_geometry* out) {
    out->onepass = g.onepass; out->nsplit = g.nsplit; out->N = g.N; out->Npad = g.Npad; out->HWp = (int32_t)g.HWp; out->P = g.P;
    out->prec = g.prec; out->n_stuff = g.n_stuff;
}

struct ph_khead_plan {
    KGeo g;
    const char* pack;
    char* ws;
};

// the family's descriptions for the shared scaffold: the pack calls resolve without the device, the plan calls with it
struct KheadPackFam {
    typedef ph_khead_cfg Cfg; typedef KGeo Geo; typedef ph_khead_layout Layout; typedef ph_khead_geometry Geometry; typedef ph_khead_plan Plan;
    static int resolve(const ph_khead_cfg* c, KGeo& g, const char* fn) { return ::resolve(c, g, fn, false); }
    static constexpr auto build_table = &::build_table;
    static constexpr auto fill_geometry = &::fill_geometry;
    static int nparams(const KGeo&) { return PH_KHEAD_NPARAMS; }
    static const char* param_name(const ph_khead_cfg*, int i) { return kParamNames[i]; }
    static constexpr unsigned kPackBlocks = 1024;
};
struct KheadPlanFam : KheadPackFam {
    static int resolve(const ph_khead_cfg* c, KGeo& g, const char* fn) { return ::resolve(c, g, fn, true); }
};

extern "C" size_t ph_khead_pack_bytes(const ph_khead_cfg* cfg) { return plan::pack_bytes<KheadPackFam>(cfg, __func__); }

extern "C" int ph_khead_pack_layout(const ph_khead_cfg* cfg, ph_khead_layout* layout) {
    return plan::pack_layout<KheadPackFam>(cfg, layout, __func__);
}

extern "C" int ph_khead_pack(const ph_khead_cfg* cfg, const float* const* params, void* pack, void* stream) {
    return plan::pack<KheadPackFam>(cfg, params, pack, stream, __func__);
}

extern "C" size_t ph_khead_plan_workspace_bytes(const ph_khead_cfg* cfg) { return plan::workspace_bytes<KheadPlanFam>(cfg, __func__); }

extern "C" int ph_khead_plan_create(const ph_khead_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes,
                                    ph_khead_plan** out) {
    return plan::create<KheadPlanFam>(cfg, pack, workspace, workspace_bytes, out, __func__);
}

extern "C" int ph_khead_geometry_of(const ph_khead_cfg* cfg, ph_khead_geometry* out) {
    return plan::geometry_of<KheadPlanFam>(cfg, out, __func__);
}

extern "C" int ph_khead_plan_info(const ph_khead_plan* p, ph_khead_geometry* out) { return plan::info<KheadPlanFam>(p, out, __func__); }

extern "C" void ph_khead_plan_destroy(ph_khead_plan* p) { delete p; }

extern "C" int ph_khead_plan_run(ph_khead_plan* p, const ph_khead_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    const KGeo& g = p->g;
    PH_CHECK_ARG(io->input_format == PH_IN_F32_NCHW || io->input_format == PH_IN_PLANES, "bad input_format");
    PH_CHECK_ARG(io->f0 && io->f1 && io->f2, "null input map");
    PH_CHECK_ARG(io->xp && io->dp && io->bits && io->mask_preds && io->seg_preds && io->depth_pred && io->proposal, "null output pointer");
    if (g.emit_f32) PH_CHECK_ARG(io->x_f32 && io->dfe_f32, "the cfg's emit_f32 needs x_f32 and dfe_f32");
    else PH_CHECK_ARG(!io->x_f32 && !io->dfe_f32, "x_f32 / dfe_f32 must be NULL without the cfg's emit_f32");
    PH_CHECK_ARG(((uintptr_t)io->depth_proposal & 15) == 0, "depth_proposal must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int B = g.B, fmt = io->input_format;
    const int64_t HW = g.HW;
    const ph_khead_layout& L = g.lay;
    auto u16 = [&](int piece) { return (const uint16_t*)(p->pack + L.offset[piece]); };
    auto f32 = [&](int piece) { return (const float*)(p->pack + L.offset[piece]); };
    void* ws1 = p->ws + g.o_ws1;
    void* ws2 = p->ws + g.o_ws2;
    float* partial = (float*)(p->ws + g.o_partial);
    if (g.onepass) {
        PH_RUN(ph_khead_onepass(io->f0, io->f1, io->f2, u16(PH_KPACK_CONV_FRAG), f32(PH_KPACK_GN), g.groups, 1e-5f,
                                u16(PH_KPACK_INIT_FRAG), g.Nq, u16(PH_KPACK_SEG_FRAG), f32(PH_KPACK_SEG_BIAS), g.n_seg,
                                u16(PH_KPACK_DD_FRAG), f32(PH_KPACK_DD_BIAS), g.n_thing, g.n_stuff, io->xp, io->dp, io->x_f32,
                                io->dfe_f32, io->mask_preds, io->seg_preds, io->depth_pred, g.logit_dtype, io->bits, g.Npad, ws1,
                                g.ws1_bytes, B, HW, g.prec, fmt, s));
        // the in-call fallback, predicated on the one-pass launch's status word (the first word of its hand-off state)
        PH_RUN(ph_khead_fused_if(io->f0, io->f1, io->f2, u16(PH_KPACK_WPLANES), f32(PH_KPACK_GN), g.groups, 1e-5f,
                                 u16(PH_KPACK_INIT_FRAG), g.Nq, u16(PH_KPACK_SEG_FRAG), f32(PH_KPACK_SEG_BIAS), g.n_seg,
                                 u16(PH_KPACK_DD_FRAG), f32(PH_KPACK_DD_BIAS), g.n_thing, g.n_stuff, io->xp, io->dp, io->x_f32,
                                 io->dfe_f32, io->mask_preds, io->seg_preds, io->depth_pred, g.logit_dtype, (const uint32_t*)ws1,
                                 ws2, g.ws2_bytes, B, HW, g.prec, fmt, s));
        PH_RUN(ph_binarize_if(io->mask_preds, g.logit_dtype, 0, io->bits, B, g.N, HW, (const uint32_t*)ws1, s));
    } else {
        PH_RUN(ph_khead_fused_if(io->f0, io->f1, io->f2, u16(PH_KPACK_WPLANES), f32(PH_KPACK_GN), g.groups, 1e-5f,
                                 u16(PH_KPACK_INIT_FRAG), g.Nq, u16(PH_KPACK_SEG_FRAG), f32(PH_KPACK_SEG_BIAS), g.n_seg,
                                 u16(PH_KPACK_DD_FRAG), f32(PH_KPACK_DD_BIAS), g.n_thing, g.n_stuff, io->xp, io->dp, io->x_f32,
                                 io->dfe_f32, io->mask_preds, io->seg_preds, io->depth_pred, PH_OUT_F32, nullptr, ws2, g.ws2_bytes,
                                 B, HW, g.prec, fmt, s));
        PH_RUN(ph_binarize((const float*)io->mask_preds, 0, io->bits, B, g.N, HW, s));
    }
    // object features: pool x over the THING rows of the bit tensor (kernel_head.py:314-320), add them to the kernels (:324-326)
    PH_RUN(ph_pool_rows(io->xp, nullptr, io->bits, g.Npad, partial, B, g.Nq, HW, g.nsplit, g.prec, s));
    PH_RUN(ph_khead_proposals(partial, g.nsplit, f32(PH_KPACK_W_INIT_F32),
                               g.n_stuff ? f32(PH_KPACK_W_SEG_F32) + (size_t)g.n_thing * 256 : nullptr, io->proposal, B, g.Nq,
                               g.n_stuff, s));
    if (io->depth_proposal) {
        const int64_t n4 = (int64_t)B * g.N * 64;
        const int64_t blocks = (n4 + 255) / 256;
        hipLaunchKernelGGL(k_khead_depth_proposal, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s,
                           (const float4*)f32(PH_KPACK_W_DD_F32), (float4*)io->depth_proposal, n4);
        PH_CHECK_LAUNCH();
    }
    return PH_OK;
}

extern "C" int ph_khead_plan_status(const ph_khead_plan* p, void* stream) {
    if (!p) { ph_set_error("ph_khead_plan_status: null plan"); return PH_EINVAL; }
    if (!p->g.onepass) return 0;
    return ph_khead_onepass_status(p->ws + p->g.o_ws1, p->g.B, stream);
}

extern "C" int ph_khead_plan_timeouts(const ph_khead_plan* p, void* stream) {
    if (!p) { ph_set_error("ph_khead_plan_timeouts: null plan"); return PH_EINVAL; }
    if (!p->g.onepass) return 0;
    return ph_khead_onepass_timeouts(p->ws + p->g.o_ws1, p->g.B, p->g.HW, stream);
}
