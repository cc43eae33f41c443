// N2: the S-stage decode as a native object (include/polyhead.h ph_decode_*): the launch geometry rule of every decode plan
// (resolve(): engine.DecodePlan asks it through ph_decode_geometry_of), the launch sequence and the buffer plan of
// engine.DecodePlan, and the stage packing of pack.py as one HIP kernel.  Host code only calls the other
// entry points of this library, on the caller's stream; nothing here allocates device memory or synchronises.  Workspace bytes,
// geometry-of and info are the shared scaffold's (ph_plan_inl.h); the stage layout, the packer and create are its own.
#include <math.h>
#include <string.h>

#include "ph_plan_inl.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// parameter table (polyhead.h: the reference's state_dict names of one KernelUpdateHead stage)
static const char* const kParamNames[PH_DECODE_NPARAMS] = {
    "attention.attn.in_proj_weight", "attention.attn.in_proj_bias", "attention.attn.out_proj.weight", "attention.attn.out_proj.bias",
    "attention_depth.attn.in_proj_weight", "attention_depth.attn.in_proj_bias", "attention_depth.attn.out_proj.weight",
    "attention_depth.attn.out_proj.bias", "attention_norm.weight", "attention_norm.bias", "attention_norm_depth.weight",
    "attention_norm_depth.bias",
#define PH_KU(P)                                                                                                          \
    P "dynamic_layer.weight", P "dynamic_layer.bias", P "input_layer.weight", P "input_layer.bias", P "input_gate.weight", \
        P "input_gate.bias", P "update_gate.weight", P "update_gate.bias", P "norm_in.weight", P "norm_in.bias",            \
        P "norm_out.weight", P "norm_out.bias", P "input_norm_in.weight", P "input_norm_in.bias", P "input_norm_out.weight", \
        P "input_norm_out.bias", P "fc_layer.weight", P "fc_layer.bias", P "fc_norm.weight", P "fc_norm.bias"
    PH_KU("kernel_update_conv."), PH_KU("kernel_update_conv_depth."),
#undef PH_KU
    "feat_transform.conv.weight", "feat_transform.conv.bias", "feat_depth_transform.conv.weight", "feat_depth_transform.conv.bias",
    "ffn.layers.0.0.weight", "ffn.layers.0.0.bias", "ffn.layers.1.weight", "ffn.layers.1.bias", "ffn_norm.weight", "ffn_norm.bias",
    "ffn_depth.layers.0.0.weight", "ffn_depth.layers.0.0.bias", "ffn_depth.layers.1.weight", "ffn_depth.layers.1.bias",
    "ffn_norm_depth.weight", "ffn_norm_depth.bias",
    "cls_fcs.0.weight", "cls_fcs.1.weight", "cls_fcs.1.bias", "fc_cls.weight", "fc_cls.bias",
    "mask_fcs.0.weight", "mask_fcs.1.weight", "mask_fcs.1.bias",
    "depth_regs.0.weight", "depth_regs.1.weight", "depth_regs.1.bias",
    "fc_mask.weight", "fc_mask.bias", "fc_depth.weight", "fc_depth.bias"};

// indices into the table; branch 0 = mask, 1 = depth
enum { P_QKV = 0, P_QKV_B = 1, P_OUT = 2, P_OUT_B = 3, P_LN_ATT = 8, P_KU = 12, P_FT = 52, P_FFN = 56, P_CLS_FCS = 68, P_FC_CLS = 71,
       P_MASK_FCS = 73, P_DEPTH_REGS = 76, P_FC_MASK = 79, P_FC_DEPTH = 81 };

static int64_t param_numel(int F, int L, int i) {
    if (i < 0 || i >= PH_DECODE_NPARAMS) return -1;
    if (i == 0 || i == 4) return 768 * 256;
    if (i == 1 || i == 5) return 768;
    if (i == 2 || i == 6) return 256 * 256;
    if (i >= P_KU && i < P_FT) {
        const int j = (i - P_KU) % 20;
        if (j == 0 || j == 2) return 512 * 256;   // dynamic_layer, input_layer
        if (j == 1 || j == 3) return 512;
        if (j == 4 || j == 6 || j == 16) return 256 * 256;
        return 256;
    }
    if (i == P_FT || i == P_FT + 2) return 256 * 256;
    if (i >= P_FFN && i < P_CLS_FCS) {
        const int j = (i - P_FFN) % 6;
        if (j == 0 || j == 2) return (int64_t)F * 256;
        if (j == 1) return F;
        return 256;
    }
    if (i == P_CLS_FCS || i == P_MASK_FCS || i == P_DEPTH_REGS || i == P_FC_MASK || i == P_FC_DEPTH) return 256 * 256;
    if (i == P_FC_CLS) return (int64_t)L * 256;
    if (i == P_FC_CLS + 1) return L;
    return 256;
}

// ---------------------------------------------------------------------------------------------
// geometry: resolve() is the ONE launch-geometry rule of the decode -- the native plan's and, through ph_decode_geometry_of,
// engine.DecodePlan's; the environment switches of the Python side arrive as the cfg's fields (engine.native_cfg)
struct Geo {
    int B, N, H, W, S, L, F;
    int64_t HW, HWp;
    int Npad;
    int feat, query, conv, kern_fmt, FP, KP, feat16;   // feat16: PH_OUT_* of 16-bit feature inputs, -1 = none (fp32 mode)
    int out_dtype, out_bytes;
    int frame_invariant, shares_gpu;
    int nsplit, nsplit_px, poolx, fused_up, up2_wgs;
    int wb_planes;                                      // planes of the packed weights (pack.py: 2 for split / hybrid)
    // workspace pieces (byte offsets)
    size_t o_xp, o_dp, o_bits, o_partial, o_pcount, o_ws, o_stage, stage_bytes, o_depth, o_partial_px, o_pcount_px, total;
    size_t ws_bytes;                                    // ph_query_workspace_bytes (what the query kernel is told)
    size_t s_obj, s_dobj, s_cls, s_kern, s_kbias;       // offsets inside one stage's piece
};

static int knob_ok(int k) { return k >= PH_KNOB_AUTO && k <= PH_KNOB_WHERE_SUPPORTED; }

static int resolve(const ph_decode_cfg* c, Geo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = Geo{};
    g.B = c->B; g.N = c->N; g.H = c->H; g.W = c->W; g.S = c->S; g.L = c->L; g.F = c->F;
    if (!(g.B > 0 && g.N > 0 && g.H > 0 && g.W > 0 && g.S >= 1 && g.S <= 16)) { ph_set_error("%s: bad size (B, N, H, W > 0, 1 <= S <= 16)", fn); return PH_EINVAL; }
    if (g.N > 256) { ph_set_error("%s: at most 256 queries", fn); return PH_EUNSUPPORTED; }
    if (!(g.L > 0 && g.L <= 1024)) { ph_set_error("%s: bad num_classes (1 .. 1024)", fn); return PH_EINVAL; }
    if (!(g.F > 0 && g.F % 256 == 0 && g.F <= 16384)) { ph_set_error("%s: F must be a multiple of 256 (at most 16384)", fn); return PH_EINVAL; }
    if (!(c->out_dtype == PH_OUT_F32 || c->out_dtype == PH_OUT_BF16 || c->out_dtype == PH_OUT_F16)) { ph_set_error("%s: bad out_dtype", fn); return PH_EINVAL; }
    if (!knob_ok(c->poolx) || !knob_ok(c->fused_up) || c->nsplit < 0 || c->nsplit_px < 0 || c->up2_wgs < 0) {
        ph_set_error("%s: bad knob value", fn);
        return PH_EINVAL;
    }
    const int QH = c->query_full_split ? PH_PREC_SPLIT : PH_PREC_QHYBRID;
    switch (c->mode) {   // engine.MODES
        case PH_MODE_BF16: g.feat = PH_PREC_BF16; g.query = PH_PREC_BF16; g.conv = PH_PREC_BF16; g.kern_fmt = PH_KERN_BF16_PLANES; g.FP = 1; g.KP = 1; g.feat16 = PH_OUT_BF16; break;
        case PH_MODE_MIXED: g.feat = PH_PREC_BF16; g.query = PH_PREC_SPLIT; g.conv = PH_PREC_BF16_KSPLIT; g.kern_fmt = PH_KERN_BF16_PLANES; g.FP = 1; g.KP = 2; g.feat16 = PH_OUT_BF16; break;
        case PH_MODE_MIXED16: g.feat = PH_PREC_BF16; g.query = QH; g.conv = PH_PREC_BF16_KF16; g.kern_fmt = PH_KERN_F16; g.FP = 1; g.KP = 1; g.feat16 = PH_OUT_BF16; break;
        case PH_MODE_FP16: g.feat = PH_PREC_F16; g.query = QH; g.conv = PH_PREC_F16; g.kern_fmt = PH_KERN_F16; g.FP = 1; g.KP = 1; g.feat16 = PH_OUT_F16; break;
        case PH_MODE_FP32: g.feat = PH_PREC_SPLIT; g.query = PH_PREC_SPLIT; g.conv = PH_PREC_SPLIT; g.kern_fmt = PH_KERN_BF16_PLANES; g.FP = 2; g.KP = 2; g.feat16 = -1; break;
        default: ph_set_error("%s: bad mode", fn); return PH_EINVAL;
    }
    g.wb_planes = (g.query == PH_PREC_SPLIT || g.query == PH_PREC_QHYBRID) ? 2 : 1;
    g.out_dtype = c->out_dtype;
    g.out_bytes = c->out_dtype == PH_OUT_F32 ? 4 : 2;
    g.frame_invariant = c->frame_invariant ? 1 : 0;
    g.shares_gpu = c->shares_gpu ? 1 : 0;
    g.HW = (int64_t)g.H * g.W;
    g.HWp = ph_hw_padded(g.HW);
    g.Npad = ph_n_padded(g.N);
    if ((int64_t)g.B * g.Npad > 65535) { ph_set_error("%s: B * Npad must be <= 65535", fn); return PH_EUNSUPPORTED; }
    if ((int64_t)g.B * g.N * g.HW / 8 >= (1ll << 31)) { ph_set_error("%s: B * N * H * W / 8 must be < 2^31", fn); return PH_EUNSUPPORTED; }
    const bool fi = g.frame_invariant != 0;
    g.nsplit = c->nsplit ? c->nsplit : ph_pool_default_nsplit(g.B, g.HW, fi);
    if (g.nsplit > g.HWp / 64) { ph_set_error("%s: nsplit out of range (at most H*W / 64 rounded up to 128)", fn); return PH_EINVAL; }

    // Final stage: conv + x2 upsample in ONE kernel where it exists (W = 256, one-plane conv grades, 16-bit outputs): the
    // low-resolution logits are not written and re-read, the depth branch's are not written at all unless the caller asks (no
    // caller of simple_test / simple_test_mask_preds ever receives them: kernel_update.py:338-345,401).
    // Chosen when the batch has at least two image rows per CU (B * H >= 512): below that a workgroup's range is one or two rows
    // and the silent halo row above it doubles its work -- one frame per launch: 34 us against 26 us for the two kernels, equal
    // at 2-4 frames, ahead from 8 (same box).  `frame_invariant` plans decide as a one-frame launch would.  The knob forces the
    // fused form at any size (WHERE_SUPPORTED / ON: tests, PH_CONV_UP2=1) or the two-kernel form (OFF).
    const bool up2_sup = g.KP == 1 && ph_dynconv_up2_supported(g.N, g.H, g.W, g.conv, g.out_dtype);
    if (c->fused_up == PH_KNOB_ON && !up2_sup) {
        ph_set_error("%s: the fused final stage (ph_dynconv_up2) cannot run this geometry / arithmetic (W == 256, 65 <= N <= 224, "
                     "one 16-bit kernel plane, 16-bit output of the conv's format)", fn);
        return PH_EUNSUPPORTED;
    }
    g.fused_up = c->fused_up == PH_KNOB_OFF ? 0
               : (c->fused_up == PH_KNOB_AUTO ? (up2_sup && (int64_t)(fi ? 1 : g.B) * g.H >= 512) : up2_sup);
    g.up2_wgs = c->up2_wgs;   // 0: 1.5 per CU (ph_num_cus: the count the process asked for first), filled in by ph_decode_create

    // Between the stages: a non-final stage's mask conv also pools the x map for the NEXT stage from the same read of the plane
    // (ph_dynconv_poolx), the next stage then pools depth_feats alone: 33.5 MB instead of 50 MB per frame and stage boundary at
    // cfg2.  One workgroup per (frame, pixel range) and CU: for launches that fill the chip (B * nsplit_px >= 192), at least 16
    // tiles of 64 pixels per workgroup (its prologue loads the frame's kernels, its epilogue writes Npad x 256 sums).  Throughput
    // plans split by B (256 / B ranges).  `frame_invariant` plans: the kernel's pixel ranges are k_pool's, and in the bf16 / fp16
    // grades its sums are k_pool's bit for bit at the same split (tests/test_gpu_kernels.py) -- with the plan's one-frame split
    // the choice between the two forms is invisible in a frame's outputs and may follow B, given 8 tiles per range; `mixed16`
    // pools the fp16-converted tile (1e-6 apart): its invariant plans keep the separate kernels.
    bool px_ok;
    if (fi) {
        if (c->nsplit_px && c->nsplit_px != g.nsplit) { ph_set_error("%s: frame_invariant plans pool with nsplit (nsplit_px must be 0 or equal)", fn); return PH_EINVAL; }
        g.nsplit_px = g.nsplit;
        px_ok = (g.conv == PH_PREC_BF16 || g.conv == PH_PREC_F16) && g.HWp / (64 * (g.nsplit_px > 1 ? g.nsplit_px : 1)) >= 8;
    } else {
        if (c->nsplit_px) g.nsplit_px = c->nsplit_px;
        else {
            const int64_t a = 256 / g.B, b = g.HWp / (64 * 16);
            const int64_t m = a < b ? a : b;
            g.nsplit_px = (int)(m > 1 ? m : 1);
        }
        px_ok = true;
    }
    if (g.nsplit_px > g.HWp / 64) { ph_set_error("%s: nsplit_px out of range", fn); return PH_EINVAL; }
    const bool px_sup = g.KP == 1 && g.S > 1 && px_ok && ph_dynconv_poolx_supported(g.N, g.conv);
    if (c->poolx == PH_KNOB_ON && !px_sup) {
        ph_set_error("%s: the fused conv + pooling (ph_dynconv_poolx) cannot run this geometry / arithmetic (S > 1, 33 <= N <= 192, "
                     "one 16-bit kernel plane; frame_invariant: bf16 / fp16 conv and 8 tiles per pixel range)", fn);
        return PH_EUNSUPPORTED;
    }
    g.poolx = c->poolx == PH_KNOB_OFF ? 0
            : (c->poolx == PH_KNOB_AUTO ? (px_sup && (int64_t)g.B * g.nsplit_px >= 192) : px_sup);

    // workspace: the buffers engine.DecodePlan allocates besides its inputs and the caller's outputs
    const size_t B = g.B, Npad = g.Npad, HWp = g.HWp, N = g.N, HW = g.HW;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o += al256(bytes); return r; };
    g.o_xp = take((size_t)g.FP * B * 256 * HWp * 2);
    g.o_dp = take((size_t)g.FP * B * 256 * HWp * 2);
    g.o_bits = take(B * Npad * (HWp / 32) * 4);
    g.o_partial = take(B * g.nsplit * Npad * 512 * 4);
    g.o_pcount = take(B * g.nsplit * Npad * 4);
    g.ws_bytes = ph_query_workspace_bytes(g.B, g.N, g.query);
    g.o_ws = take(g.ws_bytes);
    // one stage: obj, dobj, cls (not for the last stage: those are the caller's), kern, kbias
    size_t so = 0;
    auto stake = [&](size_t bytes) { const size_t r = so; so += al256(bytes); return r; };
    g.s_kern = stake((size_t)g.KP * 2 * B * Npad * 256 * 2);
    g.s_kbias = stake(2 * B * Npad * 4);
    g.s_obj = stake(B * N * 256 * 4);
    g.s_dobj = stake(B * N * 256 * 4);
    g.s_cls = stake(B * N * g.L * 4);
    g.stage_bytes = so;
    g.o_stage = o;
    o += (size_t)(g.S - 1) * so + (g.s_obj);     // the last stage needs kern + kbias only
    g.o_depth = g.fused_up ? 0 : take(B * N * HW * g.out_bytes);
    if (g.poolx) {
        g.o_partial_px = take(B * g.nsplit_px * Npad * 512 * 4);
        g.o_pcount_px = take(B * g.nsplit_px * Npad * 4);
    }
    g.total = o;
    return PH_OK;
}

// ---------------------------------------------------------------------------------------------
// pack layout: pack.py pack_stage, segment by segment (matrices into the fragment planes, vectors into wf)
enum { SEG_COPY = 0, SEG_FOLD_DYN = 1, SEG_FOLD_KERN = 2, SEG_FOLD_DYN_CNT = 3, SEG_FOLD_KERN_B = 4 };
struct MatSeg {              // rows (padded to 16) x K of one Linear, in fragment order at `dst` of each plane
    int32_t dst;
    uint16_t rows, K;
    uint8_t kind, a, b, c;   // parameter indices; COPY: a = the weight (valid rows = numel / K)
    uint8_t post, pad[3];    // hybrid grade: ONE fp16 plane (the POST kernel's matrices)
};
struct VecSeg {
    int32_t dst;
    uint16_t len, valid;
    uint8_t kind, a, b, c;
};
constexpr int kMaxMat = 24, kMaxVec = 57;
struct PackTable {
    const float* p[PH_DECODE_NPARAMS];
    MatSeg m[kMaxMat];
    VecSeg v[kMaxVec];
    int64_t plane_elems;     // distance between the hi and the lo plane
    int32_t wf_off;          // element offset of wf in the pack, as uint16 (bytes / 2)
    int32_t gap[2][2];       // [begin, end) in uint16 of the alignment padding after the planes and after wf: written as zeros
    int32_t nm, nv, planes, hybrid, L;
};
static_assert(sizeof(PackTable) <= 2048, "the pack table travels as a kernel argument");

struct Layout {
    PackTable t;
    ph_stage_layout lay;
    size_t wf_bytes, wf_byte_off, total;
};

static int build_layout(const Geo& g, Layout& out) {
    memset(&out, 0, sizeof(out));
    PackTable& t = out.t;
    ph_stage_layout& lay = out.lay;
    int64_t woff = 0, voff = 0;
    auto pad16 = [](int r) { return (r + 15) / 16 * 16; };
    auto add_w = [&](int br, int idx, int rows, int K, int kind, int a, int b, int c) {
        static const bool kPost[PH_W_COUNT] = {false, false, false, false, false, true, true, true, true, true, true, true, true};
        MatSeg& s = t.m[t.nm++];
        s.dst = (int32_t)woff; s.rows = (uint16_t)pad16(rows); s.K = (uint16_t)K;
        s.kind = (uint8_t)kind; s.a = (uint8_t)a; s.b = (uint8_t)b; s.c = (uint8_t)c; s.post = kPost[idx];
        lay.w[br][idx] = woff;
        woff += (int64_t)s.rows * K;
    };
    auto add_v = [&](int br, int idx, int len, int valid, int kind, int a, int b, int c) {
        VecSeg& s = t.v[t.nv++];
        s.dst = (int32_t)voff; s.len = (uint16_t)len; s.valid = (uint16_t)valid;
        s.kind = (uint8_t)kind; s.a = (uint8_t)a; s.b = (uint8_t)b; s.c = (uint8_t)c;
        lay.v[br][idx] = voff;
        voff += len;
    };
    const int F = g.F, L = g.L, Lp = pad16(L);
    for (int br = 0; br < 2; ++br) {
        const int ku = P_KU + 20 * br, Wx = P_FT + 2 * br, bx = Wx + 1, at = 4 * br, ff = P_FFN + 6 * br;
        add_w(br, PH_W_DYN, 512, 256, SEG_FOLD_DYN, ku + 0, Wx, 0);
        add_v(br, PH_V_DYN_CNT, 512, 512, SEG_FOLD_DYN_CNT, ku + 0, bx, 0);
        add_v(br, PH_V_DYN_B, 512, 512, SEG_COPY, ku + 1, 0, 0);
        add_w(br, PH_W_INP, 512, 256, SEG_COPY, ku + 2, 0, 0);
        add_v(br, PH_V_INP_B, 512, 512, SEG_COPY, ku + 3, 0, 0);
        add_w(br, PH_W_IG, 256, 256, SEG_COPY, ku + 4, 0, 0);
        add_v(br, PH_V_IG_B, 256, 256, SEG_COPY, ku + 5, 0, 0);
        add_w(br, PH_W_UG, 256, 256, SEG_COPY, ku + 6, 0, 0);
        add_v(br, PH_V_UG_B, 256, 256, SEG_COPY, ku + 7, 0, 0);
        // (name, key) = (LN_IG, input_norm_in), (LN_UG, norm_in), (LN_PO, norm_out), (LN_IO, input_norm_out), (LN_FC, fc_norm)
        const int lnv[5] = {PH_V_LN_IG_G, PH_V_LN_UG_G, PH_V_LN_PO_G, PH_V_LN_IO_G, PH_V_LN_FC_G};
        const int lnp[5] = {ku + 12, ku + 8, ku + 10, ku + 14, ku + 18};
        for (int i = 0; i < 5; ++i) {
            add_v(br, lnv[i], 256, 256, SEG_COPY, lnp[i], 0, 0);
            add_v(br, lnv[i] + 1, 256, 256, SEG_COPY, lnp[i] + 1, 0, 0);
        }
        add_w(br, PH_W_FC, 256, 256, SEG_COPY, ku + 16, 0, 0);
        add_v(br, PH_V_FC_B, 256, 256, SEG_COPY, ku + 17, 0, 0);
        add_w(br, PH_W_QKV, 768, 256, SEG_COPY, at + P_QKV, 0, 0);
        add_v(br, PH_V_QKV_B, 768, 768, SEG_COPY, at + P_QKV_B, 0, 0);
        add_w(br, PH_W_OUT, 256, 256, SEG_COPY, at + P_OUT, 0, 0);
        add_v(br, PH_V_OUT_B, 256, 256, SEG_COPY, at + P_OUT_B, 0, 0);
        add_v(br, PH_V_LN_ATT_G, 256, 256, SEG_COPY, P_LN_ATT + 2 * br, 0, 0);
        add_v(br, PH_V_LN_ATT_B, 256, 256, SEG_COPY, P_LN_ATT + 2 * br + 1, 0, 0);
        add_w(br, PH_W_FFN1, F, 256, SEG_COPY, ff + 0, 0, 0);
        add_v(br, PH_V_FFN1_B, F, F, SEG_COPY, ff + 1, 0, 0);
        add_w(br, PH_W_FFN2, 256, F, SEG_COPY, ff + 2, 0, 0);
        add_v(br, PH_V_FFN2_B, 256, 256, SEG_COPY, ff + 3, 0, 0);
        add_v(br, PH_V_LN_FFN_G, 256, 256, SEG_COPY, ff + 4, 0, 0);
        add_v(br, PH_V_LN_FFN_B, 256, 256, SEG_COPY, ff + 5, 0, 0);
        int Wk, bk;
        if (br == 0) {
            add_w(br, PH_W_H0A, 256, 256, SEG_COPY, P_CLS_FCS, 0, 0);
            add_v(br, PH_V_LN_H0A_G, 256, 256, SEG_COPY, P_CLS_FCS + 1, 0, 0);
            add_v(br, PH_V_LN_H0A_B, 256, 256, SEG_COPY, P_CLS_FCS + 2, 0, 0);
            add_w(br, PH_W_H0B, 256, 256, SEG_COPY, P_MASK_FCS, 0, 0);
            add_v(br, PH_V_LN_H0B_G, 256, 256, SEG_COPY, P_MASK_FCS + 1, 0, 0);
            add_v(br, PH_V_LN_H0B_B, 256, 256, SEG_COPY, P_MASK_FCS + 2, 0, 0);
            add_w(br, PH_W_CLS, L, 256, SEG_COPY, P_FC_CLS, 0, 0);
            add_v(br, PH_V_CLS_B, Lp, L, SEG_COPY, P_FC_CLS + 1, 0, 0);
            Wk = P_FC_MASK; bk = P_FC_MASK + 1;
        } else {
            add_w(br, PH_W_H0A, 256, 256, SEG_COPY, P_DEPTH_REGS, 0, 0);
            add_v(br, PH_V_LN_H0A_G, 256, 256, SEG_COPY, P_DEPTH_REGS + 1, 0, 0);
            add_v(br, PH_V_LN_H0A_B, 256, 256, SEG_COPY, P_DEPTH_REGS + 2, 0, 0);
            Wk = P_FC_DEPTH; bk = P_FC_DEPTH + 1;
        }
        add_w(br, PH_W_KERN, 272, 256, SEG_FOLD_KERN, Wx, Wk, bx);
        add_v(br, PH_V_KERN_B, 272, 272, SEG_FOLD_KERN_B, Wx, bk, bx);
    }
    t.plane_elems = woff;
    t.planes = g.wb_planes;
    t.hybrid = g.query == PH_PREC_QHYBRID;
    t.L = L;
    lay.wb_plane_elems = woff;
    lay.ffn_dim = F;
    lay.num_classes = L;
    out.wf_byte_off = al256((size_t)t.planes * woff * 2);
    out.wf_bytes = (size_t)voff * 4;
    out.total = out.wf_byte_off + al256(out.wf_bytes);
    t.wf_off = (int32_t)(out.wf_byte_off / 2);
    t.gap[0][0] = (int32_t)(t.planes * woff);
    t.gap[0][1] = t.wf_off;
    t.gap[1][0] = (int32_t)((out.wf_byte_off + out.wf_bytes) / 2);
    t.gap[1][1] = (int32_t)(out.total / 2);
    return PH_OK;
}

// one element of a folded matrix / vector: float64 products (exact for fp32 operands), k ascending
__device__ double fold_mat(const PackTable& t, const MatSeg& s, int r, int col) {
    double acc = 0.0;
    if (s.kind == SEG_FOLD_DYN) {            // (dynamic_layer.weight @ feat_transform.weight)[r][col]
        const float* A = t.p[s.a] + (int64_t)r * 256;
        const float* X = t.p[s.b] + col;
        for (int k = 0; k < 256; ++k) acc += (double)A[k] * (double)X[(int64_t)k * 256];
    } else {                                  // rows 0 .. 255: (Wx^T @ Wk)[r][col]; row 256: (bx @ Wk)[col]; beyond: 0
        const float* X = t.p[s.a];
        const float* K = t.p[s.b] + col;
        if (r < 256)
            for (int k = 0; k < 256; ++k) acc += (double)X[(int64_t)k * 256 + r] * (double)K[(int64_t)k * 256];
        else if (r == 256) {
            const float* bx = t.p[s.c];
            for (int k = 0; k < 256; ++k) acc += (double)bx[k] * (double)K[(int64_t)k * 256];
        }
    }
    return acc;
}

__device__ float vec_value(const PackTable& t, const VecSeg& s, int i) {
    if (i >= s.valid) return 0.f;
    if (s.kind == SEG_COPY) return t.p[s.a][i];
    double acc = 0.0;
    if (s.kind == SEG_FOLD_DYN_CNT) {         // dynamic_layer.weight @ feat_transform.bias
        const float* A = t.p[s.a] + (int64_t)i * 256;
        const float* bx = t.p[s.b];
        for (int k = 0; k < 256; ++k) acc += (double)A[k] * (double)bx[k];
    } else {                                  // KERN_B: (Wx^T @ bk)[i] for i < 256, bx . bk at 256, 0 beyond
        const float* bk = t.p[s.b];
        if (i < 256) {
            const float* X = t.p[s.a];
            for (int k = 0; k < 256; ++k) acc += (double)X[(int64_t)k * 256 + i] * (double)bk[k];
        } else if (i == 256) {
            const float* bx = t.p[s.c];
            for (int k = 0; k < 256; ++k) acc += (double)bx[k] * (double)bk[k];
        }
    }
    return (float)acc;
}

// grid (x, segments + 1): blockIdx.y < nm = a matrix segment, then the vector segments, the last row zeroes the alignment padding
// (every byte of a pack is defined: two packings of the same weights are byte-equal); grid-stride over the segment's elements
__global__ __launch_bounds__(256) void k_decode_pack(const PackTable t, uint16_t* __restrict__ pack) {
    const int seg = blockIdx.y;
    const int stride = gridDim.x * blockDim.x;
    if (seg < t.nm) {
        const MatSeg s = t.m[seg];
        const int K = s.K, nks = K / 32;
        const int64_t n = (int64_t)s.rows * K;
        const int valid_rows = s.kind == SEG_COPY ? (s.a == P_FC_CLS ? t.L : (int)(s.rows)) : 0;
        uint16_t* hi = pack + s.dst;
        uint16_t* lo = hi + t.plane_elems;
        for (int64_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
            // fragment order (pack.py pack_b_fragments): [ct][ks][g][j][e] holds W[16 ct + j][32 ks + 8 g + e]
            const int e = (int)(idx & 7), j = (int)((idx >> 3) & 15), gq = (int)((idx >> 7) & 3);
            const int64_t blk = idx >> 9;
            const int ks = (int)(blk % nks), ct = (int)(blk / nks);
            const int r = 16 * ct + j, col = 32 * ks + 8 * gq + e;
            float w;
            if (s.kind == SEG_COPY) w = r < valid_rows ? t.p[s.a][(int64_t)r * K + col] : 0.f;
            else w = (float)fold_mat(t, s, r, col);
            uint32_t h, l;
            if (t.hybrid && s.post) { h = f2h(w); l = 0; }
            else f2bf_split(w, h, l);
            hi[idx] = (uint16_t)h;
            if (t.planes == 2) lo[idx] = (uint16_t)l;
        }
    } else if (seg == t.nm + t.nv) {
        for (int r = 0; r < 2; ++r)
            for (int i = t.gap[r][0] + blockIdx.x * blockDim.x + threadIdx.x; i < t.gap[r][1]; i += stride) pack[i] = 0;
    } else {
        const VecSeg s = t.v[seg - t.nm];
        float* wf = reinterpret_cast<float*>(pack + t.wf_off) + s.dst;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.len; i += stride) wf[i] = vec_value(t, s, i);
    }
}

// 16-bit NCHW rows -> plane 0 [B*256][HWp], padding pixels zero (engine.DecodePlan.set_inputs' copy into zeroed planes)
__global__ __launch_bounds__(256) void k_decode_rows16(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t HW,
                                                       int64_t HWp) {
    const int64_t row = blockIdx.y;
    for (int64_t px = blockIdx.x * blockDim.x + threadIdx.x; px < HWp; px += (int64_t)gridDim.x * blockDim.x)
        dst[row * HWp + px] = px < HW ? src[row * HW + px] : (uint16_t)0;
}

// ---------------------------------------------------------------------------------------------
extern "C" const char* ph_decode_param_name(int index) {
    return index >= 0 && index < PH_DECODE_NPARAMS ? kParamNames[index] : nullptr;
}

extern "C" int64_t ph_decode_param_numel(const ph_decode_cfg* cfg, int index) {
    if (!cfg) return -1;
    return param_numel(cfg->F, cfg->L, index);
}

extern "C" int ph_decode_pack_layout(const ph_decode_cfg* cfg, ph_stage_layout* layout, size_t* wf_byte_offset) {
    Geo g;
    int rc = resolve(cfg, g, "ph_decode_pack_layout");
    if (rc) return rc;
    Layout L;
    build_layout(g, L);
    if (layout) *layout = L.lay;
    if (wf_byte_offset) *wf_byte_offset = L.wf_byte_off;
    return PH_OK;
}

extern "C" size_t ph_decode_pack_bytes(const ph_decode_cfg* cfg) {
    Geo g;
    if (resolve(cfg, g, "ph_decode_pack_bytes")) return 0;
    Layout L;
    build_layout(g, L);
    return L.total;
}

extern "C" int ph_decode_pack_stage(const ph_decode_cfg* cfg, const float* const* params, void* pack, void* stream) {
    Geo g;
    int rc = resolve(cfg, g, "ph_decode_pack_stage");
    if (rc) return rc;
    PH_CHECK_ARG(params && pack, "null params or pack");
    for (int i = 0; i < PH_DECODE_NPARAMS; ++i)
        if (!params[i]) { ph_set_error("ph_decode_pack_stage: parameter %d (%s) is NULL", i, kParamNames[i]); return PH_EINVAL; }
    PH_CHECK_ARG(((uintptr_t)pack & 255) == 0, "pack must be 256-byte aligned");
    Layout L;
    build_layout(g, L);
    for (int i = 0; i < PH_DECODE_NPARAMS; ++i) L.t.p[i] = params[i];
    const dim3 grid(64, (unsigned)(L.t.nm + L.t.nv + 1));
    hipLaunchKernelGGL(k_decode_pack, grid, dim3(256), 0, (hipStream_t)stream, L.t, (uint16_t*)pack);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

struct ph_decode {
    Geo g;
    ph_stage_layout lay;
    size_t wf_byte_off;
    const void* packs[16];
    char* ws;
};

extern "C" int ph_decode_create(const ph_decode_cfg* cfg, const void* const* packs, void* workspace, size_t workspace_bytes,
                                ph_decode** out) {
    Geo g;
    int rc = resolve(cfg, g, "ph_decode_create");
    if (rc) return rc;
    PH_CHECK_ARG(out && packs && workspace, "null packs, workspace or out");
    *out = nullptr;
    for (int s = 0; s < g.S; ++s)
        if (!packs[s] || ((uintptr_t)packs[s] & 255)) { ph_set_error("ph_decode_create: pack %d is NULL or not 256-byte aligned", s); return PH_EINVAL; }
    PH_RUN(ph_check_buffers("ph_decode_create", nullptr, workspace, workspace_bytes, g.total));
    ph_decode* p = new (std::nothrow) ph_decode;
    if (!p) { ph_set_error("ph_decode_create: out of host memory"); return PH_EINVAL; }
    if (!g.up2_wgs) {      // engine.DecodePlan's 3 * multi_processor_count / 2, with the CU count the process asked for first (ph_num_cus)
        const int cus = ph_num_cus();
        if (cus <= 0) {
            delete p;
            ph_set_error("ph_decode_create: the CU count of the HIP device could not be read");
            return PH_EINVAL;
        }
        g.up2_wgs = 3 * cus / 2;
    }
    p->g = g;
    Layout L;
    build_layout(g, L);
    p->lay = L.lay;
    p->wf_byte_off = L.wf_byte_off;
    for (int s = 0; s < g.S; ++s) p->packs[s] = packs[s];
    p->ws = (char*)workspace;
    *out = p;
    return PH_OK;
}

// workgroups of the fused final stage's launches: a part of a multi-stream step (`shares_gpu`) takes 1.5 per CU (g.up2_wgs) -- the
// other parts' query kernels hold CUs when the launch starts, and what cannot start at once leaves a shorter tail; 0 = one per CU
static int up2_workgroups(const Geo& g) {
    return (g.fused_up && g.shares_gpu && (int64_t)g.B * g.H >= 4 * (int64_t)g.up2_wgs) ? g.up2_wgs : 0;
}

static void fill_geometry(const Geo& g, ph_decode_geometry* out) {
    out->nsplit = g.nsplit; out->nsplit_px = g.nsplit_px; out->poolx = g.poolx; out->fused_up = g.fused_up;
    out->up2_workgroups = up2_workgroups(g);
    out->feat_prec = g.feat; out->query_prec = g.query; out->conv_prec = g.conv; out->kern_format = g.kern_fmt;
    out->feat_planes = g.FP;
}

// the family's description for the shared scaffold
struct DecodeFam {
    typedef ph_decode_cfg Cfg; typedef ::Geo Geo; typedef ph_decode_geometry Geometry; typedef ph_decode Plan;
    static constexpr auto resolve = &::resolve;
    static constexpr auto fill_geometry = &::fill_geometry;
};

extern "C" size_t ph_decode_workspace_bytes(const ph_decode_cfg* cfg) { return plan::workspace_bytes<DecodeFam>(cfg, __func__); }

extern "C" int ph_decode_geometry_of(const ph_decode_cfg* cfg, ph_decode_geometry* out) { return plan::geometry_of<DecodeFam>(cfg, out, __func__); }

extern "C" int ph_decode_info(const ph_decode* p, ph_decode_geometry* out) { return plan::info<DecodeFam>(p, out, __func__); }

extern "C" void ph_decode_destroy(ph_decode* p) { delete p; }

// the plan's launches take their knobs from here, never from the environment: the defaults the public entry points use when no
// PH_CONV_* / PH_UP2_* / PH_QUERY_* variable is set (the up2 workgroup count is the cfg's, see ph_decode_cfg.up2_wgs)
static const PhConvKnobs kConv{};
static const PhUp2Knobs kUp2{};
static const PhQueryKnobs kQuery{};

extern "C" int ph_decode_run(ph_decode* p, const ph_decode_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    const Geo& g = p->g;
    PH_CHECK_ARG(io->x && io->depth_feats && io->k0 && io->q0 && io->obj && io->dobj && io->cls && io->mask && io->mask_up && io->depth_up,
                 "null input or output pointer");
    PH_CHECK_ARG(io->feat_format == PH_FEAT_F32 || io->feat_format == PH_FEAT_16 || io->feat_format == PH_FEAT_PLANES, "bad feat_format");
    if (io->feat_format == PH_FEAT_PLANES) PH_CHECK_ARG(io->bits != nullptr, "PH_FEAT_PLANES needs bits");
    else {
        PH_CHECK_ARG(io->m0 != nullptr, "null m0");
        PH_CHECK_ARG(io->m0_dtype == PH_OUT_F32 || io->m0_dtype == PH_OUT_BF16 || io->m0_dtype == PH_OUT_F16, "bad m0_dtype");
    }
    if (io->feat_format == PH_FEAT_16 && g.feat16 < 0) {
        ph_set_error("ph_decode_run: 16-bit feature inputs need a mode with that plane format (bf16 / mixed / mixed16: bf16, fp16: fp16)");
        return PH_EINVAL;
    }
    if (io->feat_format != PH_FEAT_PLANES && (int64_t)g.B * 256 > 65535) {
        ph_set_error("ph_decode_run: fp32 / 16-bit NCHW feature inputs need B * 256 <= 65535 (one row of workgroups per channel)");
        return PH_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    const int B = g.B, N = g.N, H = g.H, W = g.W, Npad = g.Npad;
    const int64_t HW = g.HW, HWp = g.HWp;
    uint16_t* xp = (uint16_t*)(p->ws + g.o_xp);
    uint16_t* dp = (uint16_t*)(p->ws + g.o_dp);
    uint32_t* bits = (uint32_t*)(p->ws + g.o_bits);
    float* partial = (float*)(p->ws + g.o_partial);
    int32_t* pcount = (int32_t*)(p->ws + g.o_pcount);
    void* ws = p->ws + g.o_ws;
    float* partial_px = g.poolx ? (float*)(p->ws + g.o_partial_px) : nullptr;
    int32_t* pcount_px = g.poolx ? (int32_t*)(p->ws + g.o_pcount_px) : nullptr;

    // ingest (engine.DecodePlan.ingest / set_inputs / run_from_planes)
    const uint16_t *xr = xp, *dr = dp;
    if (io->feat_format == PH_FEAT_F32) {
        PH_RUN(ph_ingest_features((const float*)io->x, xp, B, HW, g.feat, s));
        PH_RUN(ph_ingest_features((const float*)io->depth_feats, dp, B, HW, g.feat, s));
    } else if (io->feat_format == PH_FEAT_16) {
        const dim3 grid((unsigned)((HWp + 255) / 256 < 8 ? (HWp + 255) / 256 : 8), (unsigned)(B * 256));
        hipLaunchKernelGGL(k_decode_rows16, grid, dim3(256), 0, s, (const uint16_t*)io->x, xp, HW, HWp);
        hipLaunchKernelGGL(k_decode_rows16, grid, dim3(256), 0, s, (const uint16_t*)io->depth_feats, dp, HW, HWp);
        PH_CHECK_LAUNCH();
    } else {
        xr = (const uint16_t*)io->x;
        dr = (const uint16_t*)io->depth_feats;
    }
    if (io->feat_format == PH_FEAT_PLANES) {
        if (hipMemcpyAsync(bits, io->bits, (size_t)B * Npad * (HWp / 32) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            ph_set_error("ph_decode_run: copy of the mask bits failed: %s", hipGetErrorString(hipGetLastError()));
            return PH_ELAUNCH;
        }
    } else {
        PH_RUN(ph_binarize_if(io->m0, io->m0_dtype, 0, bits, B, N, HW, nullptr, s));
    }

    // the S stages (engine.DecodePlan.stages)
    const float *k = io->k0, *q = io->q0;
    const int phases = PH_QUERY_BOTH | (g.shares_gpu ? PH_QUERY_WIDE : 0);
    const int64_t kb = (int64_t)B * Npad * 256;      // one branch of one kernel plane
    for (int st = 0; st < g.S; ++st) {
        const bool last = st == g.S - 1;
        char* so = p->ws + g.o_stage + (size_t)st * g.stage_bytes;
        uint16_t* kern = (uint16_t*)(so + g.s_kern);
        float* kbias = (float*)(so + g.s_kbias);
        float* obj = last ? io->obj : (float*)(so + g.s_obj);
        float* dobj = last ? io->dobj : (float*)(so + g.s_dobj);
        float* cls = last ? io->cls : (float*)(so + g.s_cls);
        const float* part;
        const int32_t* cnt;
        int ns;
        if (st > 0 && g.poolx) {
            PH_RUN(ph_pool_counts(dr, nullptr, bits, partial_px + 256, pcount_px, B, N, HW, g.nsplit_px, g.feat, s));
            part = partial_px; cnt = pcount_px; ns = g.nsplit_px;
        } else {
            PH_RUN(ph_pool_counts(xr, dr, bits, partial, pcount, B, N, HW, g.nsplit, g.feat, s));
            part = partial; cnt = pcount; ns = g.nsplit;
        }
        const uint16_t* wb = (const uint16_t*)p->packs[st];
        const float* wf = (const float*)((const char*)p->packs[st] + p->wf_byte_off);
        PH_RUN(ph_query_stage_counts_k(kQuery, part, ns, bits, cnt, k, q, wb, wf, &p->lay, obj, dobj, cls, last ? 1 : 0, kern, kbias, ws,
                                      g.ws_bytes, B, N, HW, g.query, g.kern_fmt, phases, s));
        if (!last) {
            if (g.poolx)
                PH_RUN(ph_dynconv_poolx(xr, kern, Npad * 256, kbias, Npad, bits, partial_px, g.nsplit_px, B, N, HW, g.conv, s));
            else
                PH_RUN(ph_dynconv_k(kConv, xr, kern, 2 * kb, Npad * 256, kbias, Npad, bits, nullptr, PH_OUT_F32, (int64_t)N * HW, B, N, HW,
                                   g.conv, s));
        } else if (g.fused_up) {
            const int wg = up2_workgroups(g);
            PH_RUN(ph_dynconv_up2_k(kUp2, xr, kern, Npad * 256, kbias, Npad, io->mask, io->mask_up, g.out_dtype, B, N, H, W, g.conv, wg, s));
            PH_RUN(ph_dynconv_up2_k(kUp2, dr, kern + kb, Npad * 256, kbias + (int64_t)B * Npad, Npad, io->depth, io->depth_up, g.out_dtype,
                                       B, N, H, W, g.conv, wg, s));
        } else {
            void* depth = io->depth ? io->depth : (void*)(p->ws + g.o_depth);
            PH_RUN(ph_dynconv_k(kConv, xr, kern, 2 * kb, Npad * 256, kbias, Npad, nullptr, io->mask, g.out_dtype, (int64_t)N * HW, B, N, HW,
                               g.conv, s));
            PH_RUN(ph_upsample2x(io->mask, io->mask_up, g.out_dtype, (int64_t)B * N, H, W, s));
            PH_RUN(ph_dynconv_k(kConv, dr, kern + kb, 2 * kb, Npad * 256, kbias + (int64_t)B * Npad, Npad, nullptr, depth, g.out_dtype,
                               (int64_t)N * HW, B, N, HW, g.conv, s));
            PH_RUN(ph_upsample2x(depth, io->depth_up, g.out_dtype, (int64_t)B * N, H, W, s));
        }
        k = obj;
        q = dobj;
    }
    return PH_OK;
}
