// N3 as a native object (include/polyhead.h ph_neck_cfg .. ph_neck_plan_run_outputs): the parameter packing of
// SemanticFPNWrapper._pack as one HIP kernel, the sine positional encoding as one HIP kernel, and the geometry rules, the buffer
// plan and the launch sequence of engine.NeckPlan.  Host code only calls the other entry points of this library, on the caller's
// stream(s); pack / posenc / create / run allocate no device memory, do not synchronise and read no environment variable.  The pack /
// create / info scaffold is the shared one (ph_plan_inl.h).
#include <math.h>

#include "ph_plan_inl.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// parameter table (polyhead.h: the reference's state_dict names of SemanticFPNWrapper), three per conv
enum { NCONV_MAX = 10, NCONV_TOWERS = 7, C_PRED = 7 };
static const char* const kParamNames[PH_NECK_NPARAMS] = {
    "convs_all_levels.0.conv0.conv.weight", "convs_all_levels.0.conv0.gn.weight", "convs_all_levels.0.conv0.gn.bias",
    "convs_all_levels.1.conv0.conv.weight", "convs_all_levels.1.conv0.gn.weight", "convs_all_levels.1.conv0.gn.bias",
    "convs_all_levels.2.conv0.conv.weight", "convs_all_levels.2.conv0.gn.weight", "convs_all_levels.2.conv0.gn.bias",
    "convs_all_levels.2.conv1.conv.weight", "convs_all_levels.2.conv1.gn.weight", "convs_all_levels.2.conv1.gn.bias",
    "convs_all_levels.3.conv0.conv.weight", "convs_all_levels.3.conv0.gn.weight", "convs_all_levels.3.conv0.gn.bias",
    "convs_all_levels.3.conv1.conv.weight", "convs_all_levels.3.conv1.gn.weight", "convs_all_levels.3.conv1.gn.bias",
    "convs_all_levels.3.conv2.conv.weight", "convs_all_levels.3.conv2.gn.weight", "convs_all_levels.3.conv2.gn.bias",
    "conv_pred.conv.weight", "conv_pred.gn.weight", "conv_pred.gn.bias",
    "aux_convs.0.conv.weight", "aux_convs.0.gn.weight", "aux_convs.0.gn.bias",
    "aux_convs.1.conv.weight", "aux_convs.1.gn.weight", "aux_convs.1.gn.bias"};
// first conv of each level's tower and the convs in it (semantic_fpn.py:75-150 for levels 0-3, upsample_times 2)
static const int kLevelFirst[4] = {0, 1, 2, 4}, kLevelConvs[4] = {1, 1, 2, 3};

static inline int conv_taps(int c) { return c < NCONV_TOWERS ? 9 : 1; }

// ---------------------------------------------------------------------------------------------
// geometry: resolve() is the ONE launch-geometry rule of the neck -- the native plan's and, through ph_neck_geometry_of,
// engine.NeckPlan's; the environment switches of the Python side arrive as the cfg's fields (engine.native_neck_cfg)
struct NLevelBufs { size_t xa, xb, y, stats, partial; };
struct NGeo {
    int B, h[4], w[4], Ho, Wo, groups, prec, P, num_outs, nconvs, pos_level, emit_planes, emit_f32, fused_out, c16, tower_buffers;
    int tile_rows[NCONV_MAX];
    float eps;
    int64_t HWo, HWp;
    size_t ws2_bytes, o_xb, o_ys[4], o_lstats[4], o_y, o_stats, o_partial, o_ws2, total;    // workspace pieces
    NLevelBufs lv[4];                                                                       // a level's own (or the shared) buffers
    ph_neck_layout lay;                                                                     // pack pieces
    size_t pack_total;
};

static int resolve(const ph_neck_cfg* c, NGeo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = NGeo{};
    g.B = c->B; g.groups = c->groups; g.num_outs = c->num_outs; g.pos_level = c->pos_level;
    if (!(g.B > 0)) { ph_set_error("%s: bad size (B > 0)", fn); return PH_EINVAL; }
    if (g.B > 4096) { ph_set_error("%s: at most 4096 frames per call", fn); return PH_EUNSUPPORTED; }
    for (int l = 0; l < 4; ++l) {
        g.h[l] = c->h[l]; g.w[l] = c->w[l];
        if (!(g.h[l] > 0 && g.w[l] > 0)) { ph_set_error("%s: bad size (h, w > 0 at every level)", fn); return PH_EINVAL; }
    }
    if ((int64_t)g.h[0] * g.w[0] > (1ll << 26)) { ph_set_error("%s: h * w of level 0 must be <= 2^26", fn); return PH_EUNSUPPORTED; }
    for (int l = 0; l < 3; ++l)
        if (g.h[l + 1] != (g.h[l] + 1) / 2 || g.w[l + 1] != (g.w[l] + 1) / 2) {
            ph_set_error("%s: FPN level sizes ((%d, %d), (%d, %d), (%d, %d), (%d, %d)) are not a stride-2 pyramid", fn, g.h[0], g.w[0],
                         g.h[1], g.w[1], g.h[2], g.w[2], g.h[3], g.w[3]);
            return PH_EUNSUPPORTED;
        }
    g.Ho = g.h[1]; g.Wo = g.w[1];
    // levels 2 and 3 reach the stride-8 size by x2 upsampling (once, twice): engine.NeckPlan._tower's check, made before any launch
    if (2 * g.h[2] != g.Ho || 2 * g.w[2] != g.Wo || 4 * g.h[3] != g.Ho || 4 * g.w[3] != g.Wo) {
        ph_set_error("%s: level does not end at the stride-8 size (levels 2 and 3 are upsampled x2 and x4: (%d, %d) needs (%d, %d) and "
                     "(%d, %d) above it)", fn, g.Ho, g.Wo, g.Ho / 2, g.Wo / 2, g.Ho / 4, g.Wo / 4);
        return PH_EUNSUPPORTED;
    }
    if (!(g.groups > 0 && 256 % g.groups == 0)) { ph_set_error("%s: groups must divide 256", fn); return PH_EINVAL; }
    g.prec = ph_mode_grade(c->mode);
    if (g.prec < 0) { ph_set_error("%s: bad mode", fn); return PH_EINVAL; }
    g.P = g.prec == PH_PREC_SPLIT ? 2 : 1;
    if (!(g.num_outs >= 1 && g.num_outs <= 3)) { ph_set_error("%s: num_outs must be 1 .. 3 (conv_pred + 0 .. 2 aux convs)", fn); return PH_EINVAL; }
    if (!(g.pos_level >= -1 && g.pos_level <= 3)) { ph_set_error("%s: pos_level must be 0 .. 3, or -1 for none", fn); return PH_EINVAL; }
    g.emit_planes = c->emit_planes ? 1 : 0;
    g.emit_f32 = c->emit_f32 ? 1 : 0;
    if (!g.emit_planes && !g.emit_f32) { ph_set_error("%s: at least one of emit_planes / emit_f32 must be set", fn); return PH_EINVAL; }
    if (!(c->fused_out == PH_KNOB_AUTO || c->fused_out == PH_KNOB_ON || c->fused_out == PH_KNOB_OFF) ||
        !(c->c16 == PH_KNOB_AUTO || c->c16 == PH_KNOB_OFF) || !(c->tower_buffers == 0 || c->tower_buffers == 1)) {
        ph_set_error("%s: bad knob value (fused_out: PH_KNOB_AUTO / _ON / _OFF, c16: PH_KNOB_AUTO / _OFF, tower_buffers: 0 / 1)", fn);
        return PH_EINVAL;
    }
    if (!(c->eps >= 0.f)) { ph_set_error("%s: eps must be >= 0 (0 = 1e-5)", fn); return PH_EINVAL; }
    g.eps = c->eps > 0.f ? c->eps : 1e-5f;
    g.nconvs = NCONV_TOWERS + g.num_outs;
    g.tower_buffers = c->tower_buffers;
    // the recompute output stage: three maps, 32 groups, one plane
    const bool can_fuse = g.num_outs == 3 && g.groups == 32 && g.P == 1;
    if (c->fused_out == PH_KNOB_ON && !can_fuse) {
        ph_set_error("%s: ph_neck_out_convs needs num_outs == 3, groups == 32 and a one-plane grade", fn);
        return PH_EUNSUPPORTED;
    }
    g.fused_out = c->fused_out != PH_KNOB_OFF && can_fuse;
    g.c16 = c->c16 != PH_KNOB_OFF && g.P == 1;            // chunk-major planes into level 0's stride-2 conv (one-plane grades)
    g.HWo = (int64_t)g.Ho * g.Wo;
    g.HWp = ph_hw_padded(g.HWo);

    // output size of every conv launch -> its row-tile form (conv_th's rule, nothing forced)
    const PhNeckKnobs kn{};
    const int oh[NCONV_MAX] = {g.Ho, g.Ho, g.h[2], g.Ho, g.h[3], 2 * g.h[3], g.Ho, g.Ho, g.Ho, g.Ho};
    const int ow[NCONV_MAX] = {g.Wo, g.Wo, g.w[2], g.Wo, g.w[3], 2 * g.w[3], g.Wo, g.Wo, g.Wo, g.Wo};
    for (int i = 0; i < g.nconvs; ++i) g.tile_rows[i] = ph_conv_nhwc_tile_rows_k(kn, oh[i], ow[i], g.prec, g.B);

    // pack pieces (SemanticFPNWrapper._pack)
    uint64_t* by = g.lay.bytes;
    for (int i = 0; i < g.nconvs; ++i) {
        by[PH_NPACK_WP(i)] = (uint64_t)g.P * 256 * (conv_taps(i) * 256) * 2;
        by[PH_NPACK_GAMMA(i)] = by[PH_NPACK_BETA(i)] = 256 * 4;
    }
    if (g.num_outs == 3) {
        by[PH_NPACK_OUTS_W] = (uint64_t)g.P * 3 * 256 * 256 * 2;
        by[PH_NPACK_OUTS_GN] = 3 * 2 * 256 * 4;
    }
    size_t o = 0;
    for (int i = 0; i < PH_NPACK_COUNT; ++i) { g.lay.offset[i] = o; o += al256(by[i]); }
    g.pack_total = o;

    // workspace (engine.NeckPlan's buffers): the level sum's planes, the last conv output + statistics of every level, the output
    // stage's conv output / statistics / partial sums (per-map form) or ph_neck_out_convs' workspace (fused form); then the towers'
    // ping / pong planes, conv output, statistics and partial sums -- one set for all levels, or one per level (tower_buffers)
    const size_t B = g.B, P = g.P, HWo = g.HWo;
    const size_t map_f32 = B * HWo * 256 * 4, stats_b = B * 256 * 2 * 4, partial_b = ph_conv_nhwc_partial_floats(g.B, g.Ho, g.Wo) * 4;
    o = 0;
    g.o_xb = o; o += al256(P * B * HWo * 256 * 2);
    for (int l = 0; l < 4; ++l) { g.o_ys[l] = o; o += al256(map_f32); }
    for (int l = 0; l < 4; ++l) { g.o_lstats[l] = o; o += al256(stats_b); }
    if (g.fused_out) {
        g.ws2_bytes = ph_neck_out_convs_workspace_bytes(g.B, g.HWo, g.groups);
        g.o_ws2 = o; o += al256(g.ws2_bytes);
    } else {
        g.o_y = o; o += al256(map_f32);
        g.o_stats = o; o += al256(stats_b);
        g.o_partial = o; o += al256(partial_b);
    }
    if (g.tower_buffers) {
        for (int l = 0; l < 4; ++l) {
            // the towers of levels 2 and 3 upsample up to the output size between their convs; levels 0 and 1 are a single conv
            const size_t n_in = (size_t)g.h[l] * g.w[l], n_small = l >= 2 ? HWo : 0;
            NLevelBufs& b = g.lv[l];
            b.xa = o; o += al256(P * B * (n_in > n_small ? n_in : n_small) * 256 * 2);
            b.xb = o; o += al256(P * B * n_small * 256 * 2);
            b.y = o; o += al256(B * n_small * 256 * 4);
            b.stats = o; o += al256(n_small ? stats_b : 0);
            b.partial = o; o += al256(partial_b);
        }
    } else {
        NLevelBufs b;
        b.xa = o; o += al256(P * B * (size_t)g.h[0] * g.w[0] * 256 * 2);       // level 0 is the largest map of a pyramid
        if (g.fused_out) {                                                     // no output-stage buffers to share
            b.y = o; o += al256(map_f32);
            b.stats = o; o += al256(stats_b);
            b.partial = o; o += al256(partial_b);
        } else {
            b.y = g.o_y; b.stats = g.o_stats; b.partial = g.o_partial;
        }
        b.xb = g.o_xb;                                                         // the towers are done before the level sum is written
        for (int l = 0; l < 4; ++l) g.lv[l] = b;
    }
    g.total = o;
    return PH_OK;
}

// ---------------------------------------------------------------------------------------------
// the pack's pieces for ph_pack_pieces (SemanticFPNWrapper._pack's tensors)
static void build_table(const NGeo& g, PhPackTable& t) {
    auto set = [&](int piece, int kind, int first, int taps = 0, int nmat = 1) {
        ph_pack_piece(t, g.lay.offset, g.lay.bytes, piece, kind, first, taps, 256, 256 * (taps ? taps : 1), 256, nmat, 3);
    };
    for (int i = 0; i < NCONV_MAX; ++i) {       // the pieces of an absent aux conv are empty
        set(PH_NPACK_WP(i), PH_PIECE_FRAG32, 3 * i, conv_taps(i));
        set(PH_NPACK_GAMMA(i), PH_PIECE_F32, 3 * i + 1);
        set(PH_NPACK_BETA(i), PH_PIECE_F32, 3 * i + 2);
    }
    set(PH_NPACK_OUTS_W, PH_PIECE_PLANES, 3 * C_PRED, 0, 3);       // [P][3][256][256] (out, in) planes of the three 1x1 weights
    set(PH_NPACK_OUTS_GN, PH_PIECE_GN, 3 * C_PRED);
    t.npieces = PH_NPACK_COUNT;
    t.total_u = (uint32_t)(g.pack_total / 16);
    t.f16 = g.prec == PH_PREC_F16;
}

// ---------------------------------------------------------------------------------------------
// k_neck_posenc: mmdet SinePositionalEncoding(normalize=True) for an empty ignore mask (positional_encoding.py:56-91), evaluated in
// fp64 and rounded once to fp32.  out [2 F][H][W]: channels [0, F) the y block, [F, 2 F) the x block; channel i of a block is
// sin (i even) or cos (i odd) of  embed / temperature^(2 (i / 2) / F),  embed = (row or column + 1) / (H or W + eps) * scale.
__global__ __launch_bounds__(256) void k_neck_posenc(float* __restrict__ out, int H, int W, int F, double temperature, double scale,
                                                     double eps) {
    const int64_t HW = (int64_t)H * W, total = 2 * (int64_t)F * HW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ch = (int)(i / HW);
        const int px = (int)(i % HW), row = px / W, col = px % W;
        const bool yblk = ch < F;
        const int f = yblk ? ch : ch - F;
        const double embed = yblk ? (double)(row + 1) / ((double)H + eps) * scale : (double)(col + 1) / ((double)W + eps) * scale;
        const double dim_t = pow(temperature, 2.0 * (double)(f / 2) / (double)F);
        const double a = embed / dim_t;
        out[i] = (float)((f & 1) ? cos(a) : sin(a));
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" const char* ph_neck_param_name(int index) {
    return index >= 0 && index < PH_NECK_NPARAMS ? kParamNames[index] : nullptr;
}

extern "C" int64_t ph_neck_param_numel(const ph_neck_cfg* cfg, int index) {
    if (!cfg || index < 0 || index >= PH_NECK_NPARAMS) return -1;
    return index % 3 == 0 ? (int64_t)256 * 256 * conv_taps(index / 3) : 256;
}

static void fill_geometry(const NGeo& g, ph_neck_geometry* out) {
    out->Ho = g.Ho; out->Wo = g.Wo; out->HWp = (int32_t)g.HWp; out->P = g.P; out->prec = g.prec; out->fused_out = g.fused_out;
    out->c16 = g.c16; out->tower_buffers = g.tower_buffers; out->nconvs = g.nconvs;
    for (int i = 0; i < NCONV_MAX; ++i) out->tile_rows[i] = g.tile_rows[i];
}

struct ph_neck_plan {
    NGeo g;
    const char* pack;
    char* ws;
};

// the family's description for the shared scaffold
struct NeckFam {
    typedef ph_neck_cfg Cfg; typedef NGeo Geo; typedef ph_neck_layout Layout; typedef ph_neck_geometry Geometry; typedef ph_neck_plan Plan;
    static constexpr auto resolve = &::resolve;
    static constexpr auto build_table = &::build_table;
    static constexpr auto fill_geometry = &::fill_geometry;
    static int nparams(const NGeo& g) { return 3 * g.nconvs; }
    static const char* param_name(const ph_neck_cfg*, int i) { return kParamNames[i]; }
    static constexpr unsigned kPackBlocks = 2048;
};

extern "C" size_t ph_neck_pack_bytes(const ph_neck_cfg* cfg) { return plan::pack_bytes<NeckFam>(cfg, __func__); }

extern "C" int ph_neck_pack_layout(const ph_neck_cfg* cfg, ph_neck_layout* layout) { return plan::pack_layout<NeckFam>(cfg, layout, __func__); }

extern "C" int ph_neck_pack(const ph_neck_cfg* cfg, const float* const* params, void* pack, void* stream) {
    return plan::pack<NeckFam>(cfg, params, pack, stream, __func__);
}

extern "C" int ph_neck_posenc(int H, int W, int num_feats, double temperature, double scale, double eps, float* out, void* stream) {
    PH_CHECK_ARG(H > 0 && W > 0 && num_feats > 0 && (int64_t)H * W <= (1ll << 26) && num_feats <= 4096, "bad size");
    PH_CHECK_ARG(temperature > 0 && eps >= 0, "temperature must be > 0 and eps >= 0");
    PH_CHECK_ARG(out != nullptr, "null out");
    const int64_t total = 2 * (int64_t)num_feats * H * W, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_neck_posenc, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, out, H, W,
                       num_feats, temperature, scale, eps);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

extern "C" size_t ph_neck_plan_workspace_bytes(const ph_neck_cfg* cfg) { return plan::workspace_bytes<NeckFam>(cfg, __func__); }

extern "C" int ph_neck_plan_create(const ph_neck_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes,
                                   ph_neck_plan** out) {
    return plan::create<NeckFam>(cfg, pack, workspace, workspace_bytes, out, __func__);
}

extern "C" int ph_neck_geometry_of(const ph_neck_cfg* cfg, ph_neck_geometry* out) { return plan::geometry_of<NeckFam>(cfg, out, __func__); }

extern "C" int ph_neck_plan_info(const ph_neck_plan* p, ph_neck_geometry* out) { return plan::info<NeckFam>(p, out, __func__); }

extern "C" void ph_neck_plan_destroy(ph_neck_plan* p) { delete p; }

// the plan's launches take their knobs from here, never from the switch table: the defaults the public entry points use when
// PH_SWITCH_CONV_TILE_ROWS / PH_SWITCH_GNSUM_WGS / PH_SWITCH_CPLANES_TPW are 0
static const PhNeckKnobs kNeck{};

// every pointer check of the three run calls, before any of them launches
static int check_io(const NGeo& g, const ph_neck_io* io, const char* fn, bool feats, int level, bool outs) {
    if (feats)
        for (int l = 0; l < 4; ++l)
            if ((level < 0 || level == l) && !io->feats[l]) { ph_set_error("%s: null feature map of level %d", fn, l); return PH_EINVAL; }
    if ((g.pos_level < 0) != (io->posenc == nullptr)) {
        ph_set_error("%s: posenc must be NULL exactly when the cfg's pos_level < 0", fn);
        return PH_EINVAL;
    }
    if (outs)
        for (int i = 0; i < g.num_outs; ++i) {
            if (g.emit_planes && !io->out_planes[i]) { ph_set_error("%s: the cfg's emit_planes needs out_planes[%d]", fn, i); return PH_EINVAL; }
            if (g.emit_f32 && !io->out_f32[i]) { ph_set_error("%s: the cfg's emit_f32 needs out_f32[%d]", fn, i); return PH_EINVAL; }
            if (((g.emit_planes ? (uintptr_t)io->out_planes[i] : 0) | (g.emit_f32 ? (uintptr_t)io->out_f32[i] : 0)) & 15) {
                ph_set_error("%s: output %d must be 16-byte aligned", fn, i);
                return PH_EINVAL;
            }
        }
    return PH_OK;
}

// conv + GroupNorm statistics (engine.NeckPlan._conv_gn)
static int conv_gn(const NGeo& g, const ph_neck_plan* p, const uint16_t* x, int conv, int H, int W, int layout, float* y, float* stats,
                   float* partial, hipStream_t s) {
    const int taps = conv_taps(conv), k = taps == 9 ? 3 : 1, stride = conv == 0 ? 2 : 1;
    const int Ho = (H + 2 * (k / 2) - k) / stride + 1, Wo = (W + 2 * (k / 2) - k) / stride + 1;
    const uint16_t* wp = (const uint16_t*)(p->pack + g.lay.offset[PH_NPACK_WP(conv)]);
    PH_RUN(ph_conv_nhwc_k(kNeck, x, wp, (int64_t)256 * 256 * taps, y, partial, k, stride, g.B, H, W, g.prec | layout, s));
    PH_RUN(ph_gn_finalize(partial, stats, ph_conv_nhwc_workgroups_b(k, stride, Ho, Wo, g.prec, g.B), g.groups, (int64_t)Ho * Wo, g.eps,
                          g.B, s));
    return PH_OK;
}

// one level (engine.NeckPlan._tower): ingest -> (conv + GN + ReLU + x2 upsample)* -> last conv (its GroupNorm is applied by the level sum);
// io == nullptr: no ingest, the caller has written the level's planes (ph_neck_plan_run_level_planes)
static int run_tower(const ph_neck_plan* p, int lvl, const ph_neck_io* io, hipStream_t s) {
    const NGeo& g = p->g;
    const NLevelBufs& b = g.lv[lvl];
    uint16_t* xa = (uint16_t*)(p->ws + b.xa);
    uint16_t* xb = (uint16_t*)(p->ws + b.xb);
    float* y = (float*)(p->ws + b.y);
    float* stats = (float*)(p->ws + b.stats);
    float* partial = (float*)(p->ws + b.partial);
    int H = g.h[lvl], W = g.w[lvl];
    const int c16 = (lvl == 0 && g.c16) ? PH_PLANES_C16 : 0;
    if (io) PH_RUN(ph_nhwc_ingest(io->feats[lvl], lvl == g.pos_level ? io->posenc : nullptr, xa, g.B, (int64_t)H * W, g.prec | c16, s));
    uint16_t* src = xa;
    for (int j = 0; j < kLevelConvs[lvl]; ++j) {
        const int conv = kLevelFirst[lvl] + j, lay = j == 0 ? c16 : 0;
        if (j + 1 < kLevelConvs[lvl]) {      // every non-final conv of levels 2 and 3 is followed by an x2 upsample
            PH_RUN(conv_gn(g, p, src, conv, H, W, lay, y, stats, partial, s));
            uint16_t* dst = src == xa ? xb : xa;
            PH_RUN(ph_gn_apply_k(kNeck, y, stats, (const float*)(p->pack + g.lay.offset[PH_NPACK_GAMMA(conv)]),
                                 (const float*)(p->pack + g.lay.offset[PH_NPACK_BETA(conv)]), g.groups, PH_GN_UP2_PLANES, 0, dst, nullptr,
                                 g.B, H, W, g.prec, s));
            H *= 2; W *= 2; src = dst;
        } else {
            PH_RUN(conv_gn(g, p, src, conv, H, W, lay, (float*)(p->ws + g.o_ys[lvl]), (float*)(p->ws + g.o_lstats[lvl]), partial, s));
        }
    }
    return PH_OK;
}

// the level sum and conv_pred / the aux convs (the tail of engine.NeckPlan.run)
static int run_outputs(const ph_neck_plan* p, const ph_neck_io* io, hipStream_t s) {
    const NGeo& g = p->g;
    const float *ys[4], *st[4], *ga[4], *be[4];
    for (int l = 0; l < 4; ++l) {
        const int last = kLevelFirst[l] + kLevelConvs[l] - 1;
        ys[l] = (const float*)(p->ws + g.o_ys[l]);
        st[l] = (const float*)(p->ws + g.o_lstats[l]);
        ga[l] = (const float*)(p->pack + g.lay.offset[PH_NPACK_GAMMA(last)]);
        be[l] = (const float*)(p->pack + g.lay.offset[PH_NPACK_BETA(last)]);
    }
    uint16_t* xb = (uint16_t*)(p->ws + g.o_xb);
    // sum over levels of ReLU(GN(.)) straight to conv input planes
    PH_RUN(ph_gn_sum_planes_k(kNeck, ys, st, ga, be, 4, g.groups, xb, g.B, g.HWo, g.prec, s));
    uint16_t* op[3] = {nullptr, nullptr, nullptr};
    float* of[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < g.num_outs; ++i) {
        if (g.emit_planes) op[i] = io->out_planes[i];
        if (g.emit_f32) of[i] = io->out_f32[i];
    }
    if (g.fused_out)
        return ph_neck_out_convs(xb, 1, (const uint16_t*)(p->pack + g.lay.offset[PH_NPACK_OUTS_W]),
                                 (const float*)(p->pack + g.lay.offset[PH_NPACK_OUTS_GN]), g.groups, g.eps, op[0], op[1], op[2], of[0],
                                 of[1], of[2], p->ws + g.o_ws2, g.ws2_bytes, g.B, g.HWo, g.prec, s);
    float* y = (float*)(p->ws + g.o_y);
    float* stats = (float*)(p->ws + g.o_stats);
    for (int i = 0; i < g.num_outs; ++i) {
        const int conv = C_PRED + i;
        const float* gamma = (const float*)(p->pack + g.lay.offset[PH_NPACK_GAMMA(conv)]);
        const float* beta = (const float*)(p->pack + g.lay.offset[PH_NPACK_BETA(conv)]);
        PH_RUN(conv_gn(g, p, xb, conv, g.Ho, g.Wo, 0, y, stats, (float*)(p->ws + g.o_partial), s));
        if (op[i]) PH_RUN(ph_gn_apply_k(kNeck, y, stats, gamma, beta, g.groups, PH_GN_TO_CPLANES, 0, op[i], nullptr, g.B, g.Ho, g.Wo, g.prec, s));
        if (of[i]) PH_RUN(ph_gn_apply_k(kNeck, y, stats, gamma, beta, g.groups, PH_GN_TO_NCHW, 0, nullptr, of[i], g.B, g.Ho, g.Wo, g.prec, s));
    }
    return PH_OK;
}

extern "C" int ph_neck_plan_run_level(ph_neck_plan* p, int level, const ph_neck_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_CHECK_ARG(level >= 0 && level < 4, "level must be 0 .. 3");
    PH_RUN(check_io(p->g, io, "ph_neck_plan_run_level", true, level, false));
    return run_tower(p, level, io, (hipStream_t)stream);
}

extern "C" int ph_neck_plan_level_input(const ph_neck_plan* p, int level, uint16_t** planes, int32_t* prec_layout) {
    PH_CHECK_ARG(p && planes && prec_layout, "null plan, planes or prec_layout");
    PH_CHECK_ARG(level >= 0 && level < 4, "level must be 0 .. 3");
    *planes = (uint16_t*)(p->ws + p->g.lv[level].xa);
    *prec_layout = p->g.prec | ((level == 0 && p->g.c16) ? PH_PLANES_C16 : 0);
    return PH_OK;
}

extern "C" int ph_neck_plan_run_level_planes(ph_neck_plan* p, int level, void* stream) {
    PH_CHECK_ARG(p != nullptr, "null plan");
    PH_CHECK_ARG(level >= 0 && level < 4, "level must be 0 .. 3");
    return run_tower(p, level, nullptr, (hipStream_t)stream);
}

extern "C" int ph_neck_plan_run_outputs(ph_neck_plan* p, const ph_neck_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_RUN(check_io(p->g, io, "ph_neck_plan_run_outputs", false, -1, true));
    return run_outputs(p, io, (hipStream_t)stream);
}

extern "C" int ph_neck_plan_run(ph_neck_plan* p, const ph_neck_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_RUN(check_io(p->g, io, "ph_neck_plan_run", true, -1, true));
    for (int l = 0; l < 4; ++l) PH_RUN(run_tower(p, l, io, (hipStream_t)stream));
    return run_outputs(p, io, (hipStream_t)stream);
}
