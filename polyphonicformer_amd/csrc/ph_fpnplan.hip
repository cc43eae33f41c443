// The FPN as a native object (include/polyhead.h ph_fpn_cfg .. ph_fpn_plan_run): the parameter packing of fpn.FPN._pack through the
// shared packer (ph_wpack.hip), and the geometry rules, the buffer plan and the launch sequence of engine.FpnPlan.  Host code only:
// it calls the other entry points of this library on the caller's stream; pack / create / run allocate no device memory, do not
// synchronise and read no environment variable.  The pack / create / info scaffold is the shared one (ph_plan_inl.h).
#include "ph_plan_inl.h"

// ---------------------------------------------------------------------------------------------
// parameter table (polyhead.h: the reference's state_dict names of FPN, in state_dict order); piece i of the pack is parameter i
static const char* const kParamNames[PH_FPN_NPARAMS] = {
    "lateral_convs.0.conv.weight", "lateral_convs.0.conv.bias", "lateral_convs.1.conv.weight", "lateral_convs.1.conv.bias",
    "lateral_convs.2.conv.weight", "lateral_convs.2.conv.bias", "lateral_convs.3.conv.weight", "lateral_convs.3.conv.bias",
    "fpn_convs.0.conv.weight", "fpn_convs.0.conv.bias", "fpn_convs.1.conv.weight", "fpn_convs.1.conv.bias",
    "fpn_convs.2.conv.weight", "fpn_convs.2.conv.bias", "fpn_convs.3.conv.weight", "fpn_convs.3.conv.bias"};

static bool k_ok(int k) { return k >= 64 && k <= 4096 && k % 64 == 0; }

// ---------------------------------------------------------------------------------------------
// geometry: resolve() is the one rule of the native plan (cfg checks, pack pieces, workspace pieces)
struct FGeo {
    int B, k[4], h[4], w[4], prec, P, x_dtype, emit_f32, emit_planes, tile_rows[4];
    size_t o_lat[4], o_y, o_partial, total;     // workspace pieces
    ph_fpn_layout lay;                          // pack pieces
    size_t pack_total;
};

static int resolve(const ph_fpn_cfg* c, FGeo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = FGeo{};
    g.B = c->B;
    if (!(g.B > 0)) { ph_set_error("%s: bad size (B > 0)", fn); return PH_EINVAL; }
    if (g.B > 4096) { ph_set_error("%s: at most 4096 frames per call", fn); return PH_EUNSUPPORTED; }
    for (int l = 0; l < 4; ++l) {
        g.k[l] = c->k[l]; g.h[l] = c->h[l]; g.w[l] = c->w[l];
        if (!k_ok(g.k[l])) { ph_set_error("%s: k[%d] = %d: stage channels must be a multiple of 64 in [64, 4096]", fn, l, g.k[l]); return PH_EINVAL; }
        if (!(g.h[l] > 0 && g.w[l] > 0)) { ph_set_error("%s: bad size (h, w > 0 at every level)", fn); return PH_EINVAL; }
    }
    if ((int64_t)g.h[0] * g.w[0] > (1ll << 26)) { ph_set_error("%s: h * w of level 0 must be <= 2^26", fn); return PH_EUNSUPPORTED; }
    for (int l = 0; l < 3; ++l)
        if (!ph_fpn_size_rule(g.h[l], g.h[l + 1]) || !ph_fpn_size_rule(g.w[l], g.w[l + 1])) {      // ph_fpn_lateral's
            ph_set_error("%s: level %d (%d, %d) over level %d (%d, %d): each size must be 2 n or 2 n - 1 of the coarser level's (the sizes "
                         "at which the integer nearest index is torch's)", fn, l, g.h[l], g.w[l], l + 1, g.h[l + 1], g.w[l + 1]);
            return PH_EUNSUPPORTED;
        }
    g.prec = ph_mode_grade(c->mode);
    if (g.prec < 0) { ph_set_error("%s: bad mode", fn); return PH_EINVAL; }
    g.P = g.prec == PH_PREC_SPLIT ? 2 : 1;
    g.x_dtype = c->x_dtype;
    if (!(g.x_dtype == PH_OUT_F32 || g.x_dtype == PH_OUT_BF16 || g.x_dtype == PH_OUT_F16)) {
        ph_set_error("%s: x_dtype must be PH_OUT_F32, PH_OUT_BF16 or PH_OUT_F16", fn);
        return PH_EINVAL;
    }
    g.emit_f32 = c->emit_f32 ? 1 : 0;
    g.emit_planes = c->emit_planes ? 1 : 0;
    if (!g.emit_f32 && !g.emit_planes) { ph_set_error("%s: at least one of emit_f32 / emit_planes must be set", fn); return PH_EINVAL; }

    const PhNeckKnobs kn{};
    for (int l = 0; l < 4; ++l) g.tile_rows[l] = ph_conv_nhwc_tile_rows_k(kn, g.h[l], g.w[l], g.prec, g.B);

    // pack pieces (fpn.FPN._pack)
    uint64_t* by = g.lay.bytes;
    for (int l = 0; l < 4; ++l) {
        by[PH_FPACK_LAT_W(l)] = (uint64_t)g.P * 256 * g.k[l] * 2;
        by[PH_FPACK_OUT_W(l)] = (uint64_t)g.P * 256 * (9 * 256) * 2;
        by[PH_FPACK_LAT_B(l)] = by[PH_FPACK_OUT_B(l)] = 256 * 4;
    }
    size_t o = 0;
    for (int i = 0; i < PH_FPACK_COUNT; ++i) { g.lay.offset[i] = o; o += al256(by[i]); }
    g.pack_total = o;

    // workspace (engine.FpnPlan's buffers): the four lateral sums, one conv output of the largest level, the conv's partial sums
    const size_t B = g.B, P = g.P;
    size_t big = 0, partial = 0;
    o = 0;
    for (int l = 0; l < 4; ++l) {
        const size_t hw = (size_t)g.h[l] * g.w[l], pf = ph_conv_nhwc_partial_floats(g.B, g.h[l], g.w[l]);
        g.o_lat[l] = o; o += al256(P * B * hw * 256 * 2);
        if (hw > big) big = hw;
        if (pf > partial) partial = pf;
    }
    g.o_y = o; o += al256(B * big * 256 * 4);
    g.o_partial = o; o += al256(partial * 4);
    g.total = o;
    return PH_OK;
}

static void build_table(const FGeo& g, PhPackTable& t) {
    for (int l = 0; l < 4; ++l) {
        // a lateral's parameter is [256][k] as stored (taps = 0); an output conv's is [256][256][9], K order (tap, channel)
        ph_pack_piece(t, g.lay.offset, g.lay.bytes, PH_FPACK_LAT_W(l), PH_PIECE_FRAG32, PH_FPACK_LAT_W(l), 0, 256, g.k[l], 256);
        ph_pack_piece(t, g.lay.offset, g.lay.bytes, PH_FPACK_OUT_W(l), PH_PIECE_FRAG32, PH_FPACK_OUT_W(l), 9, 256, 9 * 256, 256);
        ph_pack_piece(t, g.lay.offset, g.lay.bytes, PH_FPACK_LAT_B(l), PH_PIECE_F32, PH_FPACK_LAT_B(l));
        ph_pack_piece(t, g.lay.offset, g.lay.bytes, PH_FPACK_OUT_B(l), PH_PIECE_F32, PH_FPACK_OUT_B(l));
    }
    t.npieces = PH_FPACK_COUNT;
    t.total_u = (uint32_t)(g.pack_total / 16);
    t.f16 = g.prec == PH_PREC_F16;
}

// ---------------------------------------------------------------------------------------------
extern "C" const char* ph_fpn_param_name(int index) { return index >= 0 && index < PH_FPN_NPARAMS ? kParamNames[index] : nullptr; }

extern "C" int64_t ph_fpn_param_numel(const ph_fpn_cfg* cfg, int index) {
    if (!cfg || index < 0 || index >= PH_FPN_NPARAMS) return -1;
    if (index & 1) return 256;
    if (index >= 8) return (int64_t)256 * 256 * 9;
    return k_ok(cfg->k[index / 2]) ? (int64_t)256 * cfg->k[index / 2] : -1;
}

static void fill_geometry(const FGeo& g, ph_fpn_geometry* out) {
    out->P = g.P; out->prec = g.prec;
    for (int l = 0; l < 4; ++l) out->tile_rows[l] = g.tile_rows[l];
}

struct ph_fpn_plan {
    FGeo g;
    const char* pack;
    char* ws;
};

// the family's description for the shared scaffold
struct FpnFam {
    typedef ph_fpn_cfg Cfg; typedef FGeo Geo; typedef ph_fpn_layout Layout; typedef ph_fpn_geometry Geometry; typedef ph_fpn_plan Plan;
    static constexpr auto resolve = &::resolve;
    static constexpr auto build_table = &::build_table;
    static constexpr auto fill_geometry = &::fill_geometry;
    static int nparams(const FGeo&) { return PH_FPN_NPARAMS; }
    static const char* param_name(const ph_fpn_cfg*, int i) { return kParamNames[i]; }
    static constexpr unsigned kPackBlocks = 2048;
};

extern "C" size_t ph_fpn_pack_bytes(const ph_fpn_cfg* cfg) { return plan::pack_bytes<FpnFam>(cfg, __func__); }

extern "C" int ph_fpn_pack_layout(const ph_fpn_cfg* cfg, ph_fpn_layout* layout) { return plan::pack_layout<FpnFam>(cfg, layout, __func__); }

extern "C" int ph_fpn_pack(const ph_fpn_cfg* cfg, const float* const* params, void* pack, void* stream) {
    return plan::pack<FpnFam>(cfg, params, pack, stream, __func__);
}

extern "C" size_t ph_fpn_plan_workspace_bytes(const ph_fpn_cfg* cfg) { return plan::workspace_bytes<FpnFam>(cfg, __func__); }

extern "C" int ph_fpn_plan_create(const ph_fpn_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes, ph_fpn_plan** out) {
    return plan::create<FpnFam>(cfg, pack, workspace, workspace_bytes, out, __func__);
}

extern "C" int ph_fpn_geometry_of(const ph_fpn_cfg* cfg, ph_fpn_geometry* out) { return plan::geometry_of<FpnFam>(cfg, out, __func__); }

extern "C" int ph_fpn_plan_info(const ph_fpn_plan* p, ph_fpn_geometry* out) { return plan::info<FpnFam>(p, out, __func__); }

extern "C" void ph_fpn_plan_destroy(ph_fpn_plan* p) { delete p; }

// the conv launches take their knobs from here, never from the environment (ph_neckplan.hip)
static const PhNeckKnobs kNeck{};

// every pointer check of the three run calls, before any of them launches; level < 0: all four
static int check_io(const FGeo& g, const ph_fpn_io* io, const char* fn, bool stages, bool outs, int level) {
    for (int l = 0; l < 4; ++l) {
        if (stages && !io->stages[l]) { ph_set_error("%s: null stage %d", fn, l); return PH_EINVAL; }
        if (!outs || (level >= 0 && level != l)) continue;
        if (g.emit_f32 && !io->out_f32[l]) { ph_set_error("%s: the cfg's emit_f32 needs out_f32[%d]", fn, l); return PH_EINVAL; }
        if (g.emit_planes) {
            if (!io->out_planes[l]) { ph_set_error("%s: the cfg's emit_planes needs out_planes[%d]", fn, l); return PH_EINVAL; }
            if ((uintptr_t)io->out_planes[l] & 15) { ph_set_error("%s: out_planes[%d] must be 16-byte aligned", fn, l); return PH_EINVAL; }
            if (io->planes_layout[l] != 0 && io->planes_layout[l] != PH_PLANES_C16) {
                ph_set_error("%s: planes_layout[%d] must be 0 or PH_PLANES_C16", fn, l);
                return PH_EINVAL;
            }
            if (io->planes_layout[l] && g.prec == PH_PREC_SPLIT) {
                ph_set_error("%s: planes_layout[%d]: PH_PLANES_C16 needs a one-plane grade", fn, l);
                return PH_EINVAL;
            }
        }
    }
    return PH_OK;
}

static int run_laterals(const ph_fpn_plan* p, const ph_fpn_io* io, hipStream_t s) {
    const FGeo& g = p->g;
    for (int l = 3; l >= 0; --l) {               // coarse to fine: each lateral adds the finished one above it
        const uint16_t* coarse = l < 3 ? (const uint16_t*)(p->ws + g.o_lat[l + 1]) : nullptr;
        PH_RUN(ph_fpn_lateral(io->stages[l], g.x_dtype, (const uint16_t*)(p->pack + g.lay.offset[PH_FPACK_LAT_W(l)]), (int64_t)256 * g.k[l],
                              (const float*)(p->pack + g.lay.offset[PH_FPACK_LAT_B(l)]), coarse, l < 3 ? g.h[l + 1] : 0, l < 3 ? g.w[l + 1] : 0,
                              (uint16_t*)(p->ws + g.o_lat[l]), g.B, g.k[l], g.h[l], g.w[l], g.prec, s));
    }
    return PH_OK;
}

static int run_output(const ph_fpn_plan* p, int l, const ph_fpn_io* io, hipStream_t s) {
    const FGeo& g = p->g;
    float* y = (float*)(p->ws + g.o_y);
    const float* bias = (const float*)(p->pack + g.lay.offset[PH_FPACK_OUT_B(l)]);
    const int64_t HW = (int64_t)g.h[l] * g.w[l];
    PH_RUN(ph_conv_nhwc_k(kNeck, (const uint16_t*)(p->ws + g.o_lat[l]), (const uint16_t*)(p->pack + g.lay.offset[PH_FPACK_OUT_W(l)]),
                          (int64_t)256 * 256 * 9, y, (float*)(p->ws + g.o_partial), 3, 1, g.B, g.h[l], g.w[l], g.prec, s));
    if (g.emit_planes)
        return ph_fpn_output_planes(y, bias, io->add[l], io->out_planes[l], g.emit_f32 ? io->out_f32[l] : nullptr, g.B, HW,
                                    g.prec | io->planes_layout[l], s);
    return ph_fpn_output(y, bias, io->out_f32[l], g.B, HW, s);
}

extern "C" int ph_fpn_plan_run_laterals(ph_fpn_plan* p, const ph_fpn_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_RUN(check_io(p->g, io, "ph_fpn_plan_run_laterals", true, false, -1));
    return run_laterals(p, io, (hipStream_t)stream);
}

extern "C" int ph_fpn_plan_run_output(ph_fpn_plan* p, int level, const ph_fpn_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_CHECK_ARG(level >= 0 && level < 4, "level must be 0 .. 3");
    PH_RUN(check_io(p->g, io, "ph_fpn_plan_run_output", false, true, level));
    return run_output(p, level, io, (hipStream_t)stream);
}

extern "C" int ph_fpn_plan_run(ph_fpn_plan* p, const ph_fpn_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    PH_RUN(check_io(p->g, io, "ph_fpn_plan_run", true, true, -1));
    PH_RUN(run_laterals(p, io, (hipStream_t)stream));
    for (int l = 0; l < 4; ++l) PH_RUN(run_output(p, l, io, (hipStream_t)stream));
    return PH_OK;
}
