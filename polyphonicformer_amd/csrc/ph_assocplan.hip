// N1 as a native object (include/polyhead.h ph_track_cfg .. ph_assoc_plan_match): the track head's parameter packing of
// QuasiDenseMaskEmbedHeadGTMask._get_pack as one HIP kernel, and the association step video.VideoAssociator strings together from
// Python -- things for tracking, segment boxes, FPN RoIAlign, the track embedding head, the tracker, the sem / track maps -- as a plan
// over ph_panoptic_merge's device records.  Three small kernels live here (k_assoc_things, k_assoc_gather, k_assoc_paint); the
// arithmetic is ph_track.hip's kernels in their batched / device-count forms.  pack / create / run allocate no device memory, do not
// synchronise and read no environment variable; ph_assoc_plan_match is the one stateful, synchronising call, and ph_assoc_plan_track
// (the device tracker, ph_dtracker.hip, and k_assoc_trklut) its launch-only counterpart.  The track pack's and the plan's pack / create /
// info scaffold is the shared one (ph_plan_inl.h).
#include <string.h>

#include <vector>

#include "ph_plan_inl.h"

#pragma clang fp contract(off)

enum { ASSOC_K_MAX = 1024 };       // record rows per frame: the look-up tables live in LDS, the things scan is one thread's

// ---------------------------------------------------------------------------------------------
// the track head's parameter table and pack layout
static const char* const kConvNames[PH_TRACK_MAX_CONVS][3] = {
    {"convs.0.conv.weight", "convs.0.gn.weight", "convs.0.gn.bias"}, {"convs.1.conv.weight", "convs.1.gn.weight", "convs.1.gn.bias"},
    {"convs.2.conv.weight", "convs.2.gn.weight", "convs.2.gn.bias"}, {"convs.3.conv.weight", "convs.3.gn.weight", "convs.3.gn.bias"},
    {"convs.4.conv.weight", "convs.4.gn.weight", "convs.4.gn.bias"}, {"convs.5.conv.weight", "convs.5.gn.weight", "convs.5.gn.bias"},
    {"convs.6.conv.weight", "convs.6.gn.weight", "convs.6.gn.bias"}, {"convs.7.conv.weight", "convs.7.gn.weight", "convs.7.gn.bias"}};
static const char* const kTailNames[4] = {"fcs.0.weight", "fcs.0.bias", "fc_embed.weight", "fc_embed.bias"};
enum { TRACK_NPARAMS_MAX = 3 * PH_TRACK_MAX_CONVS + 4, FC_K = 49 * 256 };

struct TGeo {
    int num_convs, F, E, groups, prec, P, nparams;
    float eps;
    ph_track_layout lay;
    size_t pack_total;
};

static int resolve_track(const ph_track_cfg* c, TGeo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = TGeo{};
    g.num_convs = c->num_convs; g.F = c->fc_out_channels; g.E = c->embed_channels; g.groups = c->groups; g.prec = c->prec;
    if (!(g.num_convs >= 1 && g.num_convs <= PH_TRACK_MAX_CONVS)) { ph_set_error("%s: num_convs must be 1 .. %d", fn, PH_TRACK_MAX_CONVS); return PH_EINVAL; }
    if (!(g.F > 0 && g.F % 16 == 0)) { ph_set_error("%s: fc_out_channels must be a positive multiple of 16", fn); return PH_EINVAL; }
    if (!(g.E > 0 && g.E % 16 == 0)) { ph_set_error("%s: embed_channels must be a positive multiple of 16", fn); return PH_EINVAL; }
    if (!(g.groups > 0 && 256 % g.groups == 0)) { ph_set_error("%s: groups must divide 256", fn); return PH_EINVAL; }
    if (!(g.prec == PH_PREC_BF16 || g.prec == PH_PREC_SPLIT)) { ph_set_error("%s: prec must be PH_PREC_BF16 or PH_PREC_SPLIT", fn); return PH_EINVAL; }
    if (!(c->eps >= 0.f)) { ph_set_error("%s: eps must be >= 0 (0 = 1e-5)", fn); return PH_EINVAL; }
    if (g.F % 32 != 0) { ph_set_error("%s: fc_out_channels must be a multiple of 32 (fc_embed's k-steps)", fn); return PH_EUNSUPPORTED; }
    if (g.F > 16384 || g.E > 4096) { ph_set_error("%s: fc_out_channels <= 16384 and embed_channels <= 4096", fn); return PH_EUNSUPPORTED; }
    g.eps = c->eps > 0.f ? c->eps : 1e-5f;
    g.P = g.prec == PH_PREC_SPLIT ? 2 : 1;
    g.nparams = 3 * g.num_convs + 4;
    uint64_t* by = g.lay.bytes;
    for (int i = 0; i < g.num_convs; ++i) {
        by[PH_TPACK_CONV(i)] = (uint64_t)g.P * 256 * 2304 * 2;
        by[PH_TPACK_GAMMA(i)] = by[PH_TPACK_BETA(i)] = 256 * 4;
    }
    by[PH_TPACK_FC] = (uint64_t)g.P * g.F * FC_K * 2;
    by[PH_TPACK_FC_B] = (uint64_t)g.F * 4;
    by[PH_TPACK_EMB] = (uint64_t)g.P * g.E * g.F * 2;
    by[PH_TPACK_EMB_B] = (uint64_t)g.E * 4;
    size_t o = 0;
    for (int i = 0; i < PH_TPACK_COUNT; ++i) { g.lay.offset[i] = o; o += al256(by[i]); }
    g.pack_total = o;
    return PH_OK;
}

static int64_t track_numel(const TGeo& g, int index) {
    if (index < 0 || index >= g.nparams) return -1;
    if (index < 3 * g.num_convs) return index % 3 == 0 ? (int64_t)256 * 2304 : 256;
    switch (index - 3 * g.num_convs) {
        case 0: return (int64_t)g.F * FC_K;
        case 1: return g.F;
        case 2: return (int64_t)g.E * g.F;
        default: return g.E;
    }
}

// ---------------------------------------------------------------------------------------------
// the pack's pieces for ph_pack_pieces (QuasiDenseMaskEmbedHeadGTMask._get_pack's tensors): the 3x3 convs and fcs.0 are tap-permuted
// 16-row fragments (fcs.0 has taps = 49: its K axis goes from ci * 49 + pos to pos * 256 + ci), fc_embed's K is as stored
static void build_table(const TGeo& g, PhPackTable& t) {
    auto set = [&](int piece, int kind, int first, int taps = 0, int rows = 0, int K = 0) {
        ph_pack_piece(t, g.lay.offset, g.lay.bytes, piece, kind, first, taps, rows, K, rows);
    };
    for (int i = 0; i < PH_TRACK_MAX_CONVS; ++i) {       // the pieces of an absent conv are empty
        const int pr = i < g.num_convs ? 3 * i : 0;
        set(PH_TPACK_CONV(i), PH_PIECE_FRAG16, pr, 9, 256, 2304);
        set(PH_TPACK_GAMMA(i), PH_PIECE_F32, pr + 1);
        set(PH_TPACK_BETA(i), PH_PIECE_F32, pr + 2);
    }
    const int tail = 3 * g.num_convs;
    set(PH_TPACK_FC, PH_PIECE_FRAG16, tail, 49, g.F, FC_K);
    set(PH_TPACK_FC_B, PH_PIECE_F32, tail + 1);
    set(PH_TPACK_EMB, PH_PIECE_FRAG16, tail + 2, 0, g.E, g.F);
    set(PH_TPACK_EMB_B, PH_PIECE_F32, tail + 3);
    t.npieces = PH_TPACK_COUNT;
    t.total_u = (uint32_t)(g.pack_total / 16);
    t.f16 = 0;                                           // the track head's grades are bf16 and the bf16 split
}

extern "C" const char* ph_track_param_name(const ph_track_cfg* cfg, int index) {
    if (!cfg || cfg->num_convs < 1 || cfg->num_convs > PH_TRACK_MAX_CONVS || index < 0 || index >= 3 * cfg->num_convs + 4) return nullptr;
    return index < 3 * cfg->num_convs ? kConvNames[index / 3][index % 3] : kTailNames[index - 3 * cfg->num_convs];
}

extern "C" int64_t ph_track_param_numel(const ph_track_cfg* cfg, int index) {
    TGeo g;
    if (resolve_track(cfg, g, "ph_track_param_numel")) return -1;
    return track_numel(g, index);
}

// the track pack's description for the shared scaffold
struct TrackFam {
    typedef ph_track_cfg Cfg; typedef TGeo Geo; typedef ph_track_layout Layout;
    static constexpr auto resolve = &resolve_track;
    static constexpr auto build_table = &::build_table;
    static int nparams(const TGeo& g) { return g.nparams; }
    static constexpr auto param_name = &ph_track_param_name;
    static constexpr unsigned kPackBlocks = 4096;
};

extern "C" size_t ph_track_pack_bytes(const ph_track_cfg* cfg) { return plan::pack_bytes<TrackFam>(cfg, __func__); }

extern "C" int ph_track_pack_layout(const ph_track_cfg* cfg, ph_track_layout* layout) { return plan::pack_layout<TrackFam>(cfg, layout, __func__); }

extern "C" int ph_track_pack(const ph_track_cfg* cfg, const float* const* params, void* pack, void* stream) {
    return plan::pack<TrackFam>(cfg, params, pack, stream, __func__);
}

// ---------------------------------------------------------------------------------------------
// the plan's geometry
struct AGeo {
    int B, Ho, Wo, K, cap, n_thing, n_stuff, nlev, h[4], w[4], words, vec8;
    float inv_stride[4], finest;
    TGeo t;
    int S[3], steps[3];                                   // conv, fc, fc_embed
    size_t segws_bytes, part_bytes;
    size_t o_segws, o_rois, o_ext, o_lut, o_trk, o_roi, o_xa, o_xb, o_y, o_h, o_part, total, staging;
};

static int resolve(const ph_assoc_cfg* c, AGeo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    g = AGeo{};
    g.B = c->B; g.Ho = c->Ho; g.Wo = c->Wo; g.K = c->K; g.cap = c->max_things; g.n_thing = c->num_thing_classes;
    g.n_stuff = c->num_stuff_classes; g.nlev = c->nlev; g.finest = c->finest_scale;
    if (!(g.B > 0 && g.Ho > 0 && g.Wo > 0 && g.K > 0)) { ph_set_error("%s: bad size (B, Ho, Wo, K > 0)", fn); return PH_EINVAL; }
    if (!(g.cap >= 1 && g.cap <= g.K)) { ph_set_error("%s: max_things must be 1 .. K (%d), got %d", fn, g.K, g.cap); return PH_EINVAL; }
    if (!(g.nlev >= 1 && g.nlev <= 4)) { ph_set_error("%s: nlev must be 1 .. 4", fn); return PH_EINVAL; }
    if (!(g.n_thing >= 0 && g.n_stuff >= 0 && g.n_thing + g.n_stuff <= 255)) {
        ph_set_error("%s: class counts must be >= 0 and the void label num_thing_classes + num_stuff_classes <= 255", fn);
        return PH_EINVAL;
    }
    for (int l = 0; l < g.nlev; ++l) {
        g.h[l] = c->h[l]; g.w[l] = c->w[l]; g.inv_stride[l] = c->inv_stride[l];
        if (!(g.h[l] > 0 && g.w[l] > 0 && g.inv_stride[l] > 0.f)) { ph_set_error("%s: bad level %d (h, w, inv_stride > 0)", fn, l); return PH_EINVAL; }
        if ((int64_t)g.h[l] * g.w[l] * 256 >= (1ll << 31)) { ph_set_error("%s: level %d: 256 h w must be < 2^31", fn, l); return PH_EUNSUPPORTED; }
    }
    if (!(g.finest > 0.f)) { ph_set_error("%s: finest_scale must be > 0", fn); return PH_EINVAL; }
    const int rc = resolve_track(&c->track, g.t, fn);
    if (rc) return rc;
    if (g.B > 4096) { ph_set_error("%s: at most 4096 frames per call", fn); return PH_EUNSUPPORTED; }
    if (g.K > ASSOC_K_MAX) { ph_set_error("%s: K must be <= %d", fn, (int)ASSOC_K_MAX); return PH_EUNSUPPORTED; }
    if (g.cap > 256) { ph_set_error("%s: max_things must be <= 256", fn); return PH_EUNSUPPORTED; }
    if ((int64_t)g.Ho * g.Wo > (1ll << 26)) { ph_set_error("%s: Ho * Wo must be <= 2^26", fn); return PH_EUNSUPPORTED; }
    if (g.t.E != 256) { ph_set_error("%s: the tracker needs embed_channels == 256", fn); return PH_EUNSUPPORTED; }
    g.words = 2 + 7 * g.cap;
    g.vec8 = g.Wo % 8 == 0;
    ph_gemm_split(49 * g.cap, 256, 2304, g.S[0], g.steps[0]);
    ph_gemm_split(g.cap, g.t.F, FC_K, g.S[1], g.steps[1]);
    ph_gemm_split(g.cap, g.t.E, g.t.F, g.S[2], g.steps[2]);
    g.segws_bytes = (size_t)g.B * ph_segment_boxes_workspace_bytes(g.K);
    size_t part = ph_gemm_rows_workspace_bytes(49 * g.cap, 256, 2304);
    const size_t p1 = ph_gemm_rows_workspace_bytes(g.cap, g.t.F, FC_K), p2 = ph_gemm_rows_workspace_bytes(g.cap, g.t.E, g.t.F);
    part = part > p1 ? part : p1;
    part = part > p2 ? part : p2;
    g.part_bytes = (size_t)g.B * part;
    const size_t B = g.B, P = g.t.P, planes = P * B * g.cap * 49 * 256 * 2;
    size_t o = 0;
    g.o_segws = o; o += al256(g.segws_bytes);
    g.o_rois = o; o += al256(B * g.K * 5 * 4);
    g.o_ext = o; o += al256(B * g.K * 4 * 4);
    g.o_lut = o; o += al256(B * (g.K + 1));
    g.o_trk = o; o += al256(B * (g.K + 1) * 8);
    g.o_roi = o; o += al256(planes);          // RoIAlign's output, kept for the whole run
    g.o_xa = o; o += al256(planes);
    g.o_xb = o; o += al256(planes);
    g.o_y = o; o += al256(B * g.cap * 49 * 256 * 4);
    g.o_h = o; o += al256(P * B * g.cap * g.t.F * 2);
    g.o_part = o; o += al256(g.part_bytes);
    g.total = o;
    g.staging = al256(B * g.words * 4) + B * (g.K + 1) * 8;
    return PH_OK;
}

// ---------------------------------------------------------------------------------------------
// k_assoc_things: one workgroup per frame.  records row: nseg | seg[K][4] = {new id, candidate index, label, area} in id order |
// scores[K] (fp32 bits).  Writes the frame's things table (nthing | seg_id[cap] | label[cap] | box[cap][5] | overflow, everything
// zero first) and its semantic look-up table lut[K + 1] (void, then label at every listed segment id).  The things are the rows
// with label < num_thing_classes in row order; the scan is one thread's (K <= 1024 rows, once per frame).
__global__ __launch_bounds__(256) void k_assoc_things(const int32_t* __restrict__ records, int K, int cap, int words, int n_thing, int void_label,
                                                      int32_t* __restrict__ things, uint8_t* __restrict__ lut) {
    const int b = blockIdx.x;
    const int32_t* rec = records + (int64_t)b * (1 + 5 * K);
    int32_t* tab = things + (int64_t)b * words;
    uint8_t* l = lut + (int64_t)b * (K + 1);
    for (int i = threadIdx.x; i < words; i += blockDim.x) tab[i] = 0;
    for (int i = threadIdx.x; i <= K; i += blockDim.x) l[i] = (uint8_t)void_label;
    __syncthreads();
    int nseg = rec[0];
    nseg = nseg < 0 ? 0 : (nseg > K ? K : nseg);
    const int32_t* seg = rec + 1;
    const int32_t* scores = rec + 1 + 4 * K;
    for (int i = threadIdx.x; i < nseg; i += blockDim.x) {
        const int id = seg[4 * i];
        if (id >= 1 && id <= K) l[id] = (uint8_t)seg[4 * i + 2];
    }
    if (threadIdx.x == 0) {
        int n = 0, over = 0;
        for (int i = 0; i < nseg; ++i) {
            const int id = seg[4 * i], k = seg[4 * i + 1], label = seg[4 * i + 2];
            if (label < 0 || label >= n_thing || id < 1 || id > K) continue;
            if (n == cap) { over = 1; break; }
            tab[1 + n] = id;
            tab[1 + cap + n] = label;
            tab[1 + 2 * cap + 5 * n + 4] = (k >= 0 && k < K) ? scores[k] : 0;
            ++n;
        }
        tab[0] = n;
        tab[words - 1] = over;
    }
}

// the extent boxes of a frame's things into box[..][0:4]; grid (B), cap threads
__global__ void k_assoc_gather(const float* __restrict__ ext /*[B][K][4]*/, int K, int cap, int words, int32_t* __restrict__ things) {
    int32_t* tab = things + (int64_t)blockIdx.x * words;
    const int i = threadIdx.x;
    if (i >= tab[0]) return;
    const float* e = ext + ((int64_t)blockIdx.x * K + (tab[1 + i] - 1)) * 4;
    float* box = (float*)(tab + 1 + 2 * cap + 5 * i);
    box[0] = e[0]; box[1] = e[1]; box[2] = e[2]; box[3] = e[3];
}

// one frame's track look-up table from the device tracker's outputs, as ph_assoc_plan_match forms it on the host: ids + 1, negatives
// to 0, painted in segment order onto the ids in the order the tracker returns them; kept_count == 0 (a skipped or refused frame):
// all zero.  One workgroup per frame, grid (frames): frame b's table at tab + b * words, its tracker outputs at ids + b * ids_stride
// and kept_count + b * kc_stride (the streams of a bank, one frame each), its look-up table at lut + b * (K + 1); ids_out (nullable):
// the frame's [cap] painted values.  active (nullable, int32 [frames]): a zero word is an idle stream, whose tracker outputs are not
// read -- all zero
__global__ __launch_bounds__(256) void k_assoc_trklut(const int32_t* __restrict__ tab, int words, int K, int cap, const int64_t* __restrict__ ids,
                                                      int64_t ids_stride, const int32_t* __restrict__ kept_count, int64_t kc_stride,
                                                      const int32_t* __restrict__ active, double* __restrict__ lut,
                                                      int64_t* __restrict__ ids_out) {
    const int b = blockIdx.x;
    tab += (int64_t)b * words; ids += b * ids_stride; kept_count += b * kc_stride; lut += (int64_t)b * (K + 1);
    if (ids_out) ids_out += (int64_t)b * cap;
    for (int i = threadIdx.x; i <= K; i += blockDim.x) lut[i] = 0.0;
    __syncthreads();
    int n = tab[0];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int k = (active && active[b] == 0) ? 0 : kept_count[0];
    for (int j = threadIdx.x; j < cap; j += blockDim.x) {
        int64_t v = 0;
        if (j < n && j < k) {
            v = ids[j] + 1;
            if (v < 0) v = 0;
            const int id = tab[1 + j];
            if (id >= 0 && id <= K) lut[id] = (double)v;
        }
        if (ids_out) ids_out[j] = v;
    }
}

// out[b][p] = lut[b][pan[b][p]] (ids outside 0 .. K read entry 0); the frame's table is staged in LDS.  T = uint8_t (sem) or double (track)
template <typename T>
__global__ __launch_bounds__(256) void k_assoc_paint(const int32_t* __restrict__ pan, const T* __restrict__ lut, T* __restrict__ out, int64_t HW,
                                                     int K) {
    __shared__ T l[ASSOC_K_MAX + 1];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i <= K; i += blockDim.x) l[i] = lut[(int64_t)b * (K + 1) + i];
    __syncthreads();
    pan += (int64_t)b * HW;
    out += (int64_t)b * HW;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < HW; p += (int64_t)gridDim.x * blockDim.x) {
        const int id = pan[p];
        out[p] = l[(id >= 0 && id <= K) ? id : 0];
    }
}

template <typename T>
static void launch_paint(const AGeo& g, const int32_t* pan, const T* lut, T* out, hipStream_t s) {
    const int64_t HW = (int64_t)g.Ho * g.Wo, blocks = (HW + 1023) / 1024;          // ~4 pixels per thread
    hipLaunchKernelGGL(k_assoc_paint<T>, dim3((unsigned)(blocks < 2048 ? blocks : 2048), g.B), dim3(256), 0, s, pan, lut, out, HW, g.K);
}

// ---------------------------------------------------------------------------------------------
static void fill_geometry(const AGeo& g, ph_assoc_geometry* out) {
    memset(out, 0, sizeof(*out));
    out->things_words = g.words; out->P = g.t.P;
    out->conv_splits = g.S[0]; out->conv_steps = g.steps[0]; out->fc_splits = g.S[1]; out->fc_steps = g.steps[1];
    out->emb_splits = g.S[2]; out->emb_steps = g.steps[2];
    out->vec8 = g.vec8;
    out->staging_bytes = g.staging;
    out->rois_offset = g.o_rois;
    out->roi_planes_offset = g.o_roi;
}

struct ph_assoc_plan {
    AGeo g;
    const char* pack;
    char* ws;
    // host scratch of ph_assoc_plan_match
    std::vector<float> boxes;
    std::vector<int64_t> labels, ids;
    std::vector<int32_t> counts, kept, kept_counts;
    std::vector<const float*> embs;
};

// the plan's description for the shared scaffold
struct AssocFam {
    typedef ph_assoc_cfg Cfg; typedef AGeo Geo; typedef ph_assoc_geometry Geometry; typedef ph_assoc_plan Plan;
    static constexpr auto resolve = &::resolve;
    static constexpr auto fill_geometry = &::fill_geometry;
};

extern "C" size_t ph_assoc_plan_workspace_bytes(const ph_assoc_cfg* cfg) { return plan::workspace_bytes<AssocFam>(cfg, __func__); }

extern "C" int ph_assoc_plan_create(const ph_assoc_cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes,
                                    ph_assoc_plan** out) {
    PH_RUN(plan::create<AssocFam>(cfg, pack, workspace, workspace_bytes, out, __func__));
    ph_assoc_plan* p = *out;
    const size_t tot = (size_t)p->g.B * p->g.cap;
    p->boxes.resize(tot * 5); p->labels.resize(tot); p->ids.resize(tot); p->kept.resize(tot);
    p->counts.resize(p->g.B); p->kept_counts.resize(p->g.B); p->embs.resize(p->g.B);
    return PH_OK;
}

extern "C" int ph_assoc_plan_info(const ph_assoc_plan* p, ph_assoc_geometry* out) { return plan::info<AssocFam>(p, out, __func__); }

extern "C" void ph_assoc_plan_destroy(ph_assoc_plan* p) { delete p; }

extern "C" int ph_assoc_plan_run(ph_assoc_plan* p, const ph_assoc_io* io, void* stream) {
    PH_CHECK_ARG(p && io, "null plan or io");
    const AGeo& g = p->g;
    PH_CHECK_ARG(io->pan && io->seg_records, "null pan or seg_records");
    PH_CHECK_ARG(io->sem_out && io->things_out && io->embeds_out, "null sem_out, things_out or embeds_out");
    PH_CHECK_ARG(!g.vec8 || ((uintptr_t)io->pan & 15) == 0, "pan must be 16-byte aligned when Wo % 8 == 0");
    PH_CHECK_ARG(((uintptr_t)io->embeds_out & 15) == 0 && ((uintptr_t)io->things_out & 3) == 0, "embeds_out must be 16-byte aligned");
    PH_CHECK_ARG(((uintptr_t)io->roi_planes & 15) == 0, "roi_planes must be 16-byte aligned");
    for (int l = 0; l < g.nlev; ++l) {
        if (!io->levels[l]) { ph_set_error("ph_assoc_plan_run: null feature map of level %d", l); return PH_EINVAL; }
        if (g.B > 1 && io->level_stride[l] < (int64_t)256 * g.h[l] * g.w[l]) {
            ph_set_error("ph_assoc_plan_run: level_stride[%d] is smaller than one frame (256 h w elements)", l);
            return PH_EINVAL;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const TGeo& t = g.t;
    char* ws = p->ws;
    uint8_t* lut = (uint8_t*)(ws + g.o_lut);
    float* rois = (float*)(ws + g.o_rois);
    float* ext = (float*)(ws + g.o_ext);
    const PhThings th{io->things_out, g.words, g.cap};

    hipLaunchKernelGGL(k_assoc_things, dim3(g.B), dim3(256), 0, s, io->seg_records, g.K, g.cap, g.words, g.n_thing, g.n_thing + g.n_stuff,
                       io->things_out, lut);
    launch_paint<uint8_t>(g, io->pan, lut, io->sem_out, s);
    PH_CHECK_LAUNCH();
    PH_RUN(ph_segment_boxes_b("ph_assoc_plan_run", io->pan, g.B, g.Ho, g.Wo, g.K, rois, ext, ws + g.o_segws, g.segws_bytes, s));
    hipLaunchKernelGGL(k_assoc_gather, dim3(g.B), dim3(g.cap), 0, s, ext, g.K, g.cap, g.words, io->things_out);
    PH_CHECK_LAUNCH();

    int32_t hw[8];
    for (int l = 0; l < g.nlev; ++l) { hw[2 * l] = g.h[l]; hw[2 * l + 1] = g.w[l]; }
    uint16_t* xa = (uint16_t*)(ws + g.o_xa);
    uint16_t* xb = (uint16_t*)(ws + g.o_xb);
    uint16_t* roi = (uint16_t*)(ws + g.o_roi);
    const uint16_t* cur = io->roi_planes ? io->roi_planes : roi;
    float* y = (float*)(ws + g.o_y);
    uint16_t* h = (uint16_t*)(ws + g.o_h);
    void* part = ws + g.o_part;
    if (!io->roi_planes) PH_RUN(ph_roi_align_fpn_cnt(io->levels, hw, g.inv_stride, io->level_stride, g.nlev, rois, g.K, th, g.B, g.finest, roi, t.prec, s));
    const int M = 49 * g.cap;
    for (int i = 0; i < t.num_convs; ++i) {
        const uint16_t* wp = (const uint16_t*)(p->pack + t.lay.offset[PH_TPACK_CONV(i)]);
        PH_RUN(ph_gemm_rows_splitk_cnt(cur, 1, wp, (int64_t)256 * 2304, nullptr, 0, y, nullptr, M, 256, 2304, t.prec, th, 49, g.B, part, s));
        uint16_t* nxt = i % 2 == 0 ? xa : xb;              // ping / pong; the RoI features are never overwritten
        PH_RUN(ph_gn_relu_cl_cnt(y, (const float*)(p->pack + t.lay.offset[PH_TPACK_GAMMA(i)]),
                                 (const float*)(p->pack + t.lay.offset[PH_TPACK_BETA(i)]), t.groups, t.eps, nxt, th, g.B, t.prec, s));
        cur = nxt;
    }
    PH_RUN(ph_gemm_rows_splitk_cnt(cur, 0, (const uint16_t*)(p->pack + t.lay.offset[PH_TPACK_FC]), (int64_t)t.F * FC_K,
                                   (const float*)(p->pack + t.lay.offset[PH_TPACK_FC_B]), 1, nullptr, h, g.cap, t.F, FC_K, t.prec, th, 1, g.B,
                                   part, s));
    PH_RUN(ph_gemm_rows_splitk_cnt(h, 0, (const uint16_t*)(p->pack + t.lay.offset[PH_TPACK_EMB]), (int64_t)t.E * t.F,
                                   (const float*)(p->pack + t.lay.offset[PH_TPACK_EMB_B]), 0, io->embeds_out, nullptr, g.cap, t.E, t.F, t.prec,
                                   th, 1, g.B, part, s));
    return PH_OK;
}

extern "C" int ph_assoc_plan_match(ph_assoc_plan* p, ph_tracker* tracker, const int32_t* pan, const int32_t* things_dev,
                                   const float* embeds_dev, void* host_staging, size_t staging_bytes, int64_t first_frame_id,
                                   double* track_out, int64_t* ids_host_out, void* stream) {
    PH_CHECK_ARG(p && tracker && pan && things_dev && embeds_dev && host_staging && track_out, "null pointer");
    const AGeo& g = p->g;
    if (staging_bytes < g.staging) { ph_set_error("ph_assoc_plan_match: host staging too small (%zu < %zu)", staging_bytes, g.staging); return PH_EWORKSPACE; }
    PH_CHECK_ARG(((uintptr_t)host_staging & 7) == 0, "host_staging must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int32_t* tabs = (int32_t*)host_staging;
    double* trk = (double*)((char*)host_staging + al256((size_t)g.B * g.words * 4));
    const size_t tab_bytes = (size_t)g.B * g.words * 4;
    // the one synchronisation of this call: the things tables behind ph_assoc_plan_run's launches
    hipError_t e = hipMemcpyAsync(tabs, things_dev, tab_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { ph_set_error("ph_assoc_plan_match: reading the things tables failed: %s", hipGetErrorString(e)); return PH_ELAUNCH; }
    size_t off = 0;
    for (int b = 0; b < g.B; ++b) {
        const int32_t* tab = tabs + (size_t)b * g.words;
        const int n = tab[0];
        if (n < 0 || n > g.cap) { ph_set_error("ph_assoc_plan_match: frame %d: bad things table (nthing = %d)", b, n); return PH_EINVAL; }
        if (tab[g.words - 1]) {
            ph_set_error("ph_assoc_plan_match: frame %d has more than max_things = %d things", b, g.cap);
            return PH_EUNSUPPORTED;
        }
        p->counts[b] = n;
        p->embs[b] = embeds_dev + (size_t)b * g.cap * 256;
        memcpy(&p->boxes[off * 5], tab + 1 + 2 * g.cap, (size_t)n * 5 * sizeof(float));
        for (int i = 0; i < n; ++i) p->labels[off + i] = tab[1 + g.cap + i];
        off += (size_t)n;
    }
    int matched = 0;
    for (int b = 0; b < g.B; ++b) p->kept_counts[b] = 0;
    if (off > 0) {
        matched = ph_tracker_match_frames(tracker, p->boxes.data(), p->labels.data(), p->embs.data(), p->counts.data(), g.B, first_frame_id,
                                          p->kept.data(), p->ids.data(), p->kept_counts.data(), stream);
        if (matched < 0) return matched;
    }
    // generate_track_id_maps: ids + 1, negatives to 0, zipped in segment order with the ids as the tracker returned them
    off = 0;
    for (int b = 0; b < g.B; ++b) {
        const int32_t* tab = tabs + (size_t)b * g.words;
        double* l = trk + (size_t)b * (g.K + 1);
        for (int i = 0; i <= g.K; ++i) l[i] = 0.0;
        const int n = p->counts[b], k = p->kept_counts[b];
        for (int j = 0; j < g.cap; ++j) {
            int64_t v = 0;
            if (j < n && j < k) { v = p->ids[off + j] + 1; if (v < 0) v = 0; l[tab[1 + j]] = (double)v; }
            if (ids_host_out) ids_host_out[(size_t)b * g.cap + j] = v;
        }
        off += (size_t)n;
    }
    double* trk_dev = (double*)(p->ws + g.o_trk);
    e = hipMemcpyAsync(trk_dev, trk, (size_t)g.B * (g.K + 1) * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { ph_set_error("ph_assoc_plan_match: uploading the track tables failed: %s", hipGetErrorString(e)); return PH_ELAUNCH; }
    launch_paint<double>(g, pan, trk_dev, track_out, s);
    PH_CHECK_LAUNCH();
    return matched;
}

extern "C" int ph_assoc_plan_track(ph_assoc_plan* p, ph_dtracker* tracker, const int32_t* pan, const int32_t* things_dev, const float* embeds_dev,
                                   double* track_out, int64_t* ids_dev_out, void* stream) {
    PH_CHECK_ARG(p && tracker && pan && things_dev && embeds_dev && track_out, "null pointer");
    const AGeo& g = p->g;
    const PhDtrkScratch sc = ph_dtracker_scratch(tracker);
    if (g.cap > sc.max_dets) {
        ph_set_error("ph_assoc_plan_track: max_things = %d is more than the tracker's max_dets = %d", g.cap, sc.max_dets);
        return PH_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    double* trk_dev = (double*)(p->ws + g.o_trk);
    // one frame at a time: the tracker's per-frame outputs are its own buffer's, so the plan's workspace is what it was
    for (int b = 0; b < g.B; ++b) {
        const int32_t* tab = things_dev + (size_t)b * g.words;
        ph_dtracker_io io{};
        io.counts = tab;
        io.labels = tab + 1 + g.cap;
        io.boxes = (const float*)(tab + 1 + 2 * g.cap);
        io.refuse = tab + g.words - 1;
        io.embeds = embeds_dev + (size_t)b * g.cap * 256;
        io.kept_out = sc.kept; io.ids_out = sc.ids; io.kept_counts = sc.kept_count;
        PH_RUN(ph_dtracker_run(tracker, &io, 1, stream));
        hipLaunchKernelGGL(k_assoc_trklut, dim3(1), dim3(256), 0, s, tab, g.words, g.K, g.cap, sc.ids, (int64_t)0, sc.kept_count, (int64_t)0,
                           nullptr, trk_dev + (size_t)b * (g.K + 1), ids_dev_out ? ids_dev_out + (size_t)b * g.cap : nullptr);
    }
    launch_paint<double>(g, pan, trk_dev, track_out, s);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

extern "C" int ph_assoc_plan_track_streams(ph_assoc_plan* p, ph_dtracker* tracker, const int32_t* pan, const int32_t* things_dev,
                                           const float* embeds_dev, const int32_t* active, double* track_out, int64_t* ids_dev_out,
                                           void* stream) {
    PH_CHECK_ARG(p && tracker && pan && things_dev && embeds_dev && track_out, "null pointer");
    const AGeo& g = p->g;
    const PhDtrkScratch sc = ph_dtracker_scratch(tracker);
    if (g.B != sc.streams) {
        ph_set_error("ph_assoc_plan_track_streams: the plan has B = %d frames, the tracker %d streams", g.B, sc.streams);
        return PH_EINVAL;
    }
    if (g.cap > sc.max_dets) {
        ph_set_error("ph_assoc_plan_track_streams: max_things = %d is more than the tracker's max_dets = %d", g.cap, sc.max_dets);
        return PH_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    double* trk_dev = (double*)(p->ws + g.o_trk);
    // frame b is stream b's next frame: the things tables' own strides index the streams
    ph_dtracker_io io{};
    io.counts = things_dev; io.count_stride = g.words;
    io.labels = things_dev + 1 + g.cap; io.label_stride = g.words;
    io.boxes = (const float*)(things_dev + 1 + 2 * g.cap); io.box_stride = g.words;
    io.refuse = things_dev + g.words - 1; io.refuse_stride = g.words;
    io.embeds = embeds_dev; io.embed_stride = (int64_t)g.cap * 256;
    PH_RUN(ph_dtracker_step_scratch(tracker, &io, active, stream));
    hipLaunchKernelGGL(k_assoc_trklut, dim3(g.B), dim3(256), 0, s, things_dev, g.words, g.K, g.cap, sc.ids, sc.ids_stride, sc.kept_count,
                       sc.kc_stride, active, trk_dev, ids_dev_out);
    launch_paint<double>(g, pan, trk_dev, track_out, s);
    PH_CHECK_LAUNCH();
    return PH_OK;
}
