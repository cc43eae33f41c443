// libpolyhead: the quasi-dense embedding tracker with its state ON THE DEVICE (include/polyhead.h ph_dtracker_*).  The specification
// is ph_tracker.hip's ph_tracker_match / ph_tracker_match_frames (quasi_dense_embed_tracker.py:47-207): the same decisions in the
// same order, so the same integer ids, tables and pool rows.  There the bookkeeping is C++ on the host and a frame costs an upload, a
// synchronising score download and another upload; here the tables live next to the pool in one caller-owned device buffer, two
// single-workgroup kernels walk them (k_dtrk_prepare, k_dtrk_assign: n <= 128 detections, m <= 4096 columns, latency-bound by design)
// and a frame is seven launches that no host code waits for -- ph_dtracker_run can be captured into a graph.
//
// A BANK is S such trackers in one buffer: stream s has its whole block (state, scratch, io_* pieces; resolve()'s layout) at
// s * total_bytes, every kernel has one grid dimension of size S and derives its stream's DState from the base and the stride and its
// DFrame from the io strides, so a step of S streams is the same seven launches.  Streams share nothing: no atomics, no hand-off
// between workgroups, and a workgroup of an idle stream returns before it touches that stream.  The single tracker is the bank of one.
//
// Arithmetic: thresholds are compared in fp32, iou1 is one rounded operation per statement with a correctly rounded division (what
// the host's iou1 does under `fp contract(off)`), the EMA is k_trk_update's two rounded products and one rounded sum, and the scores
// are ph_track_affinity's own kernels in their device-count forms (ph_track.hip), bit for bit.
// The single-workgroup kernels need no atomics: every table has one writer between two barriers.
#include <limits.h>

#include <new>

#include "ph_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TE = 256;                                  // embedding width
constexpr int DT_MAXN = 128, DT_MAXC = 4096, DT_MAXG = 16;

// the frame record k_dtrk_prepare leaves for the other kernels of the frame (int32 words; 0 .. 2 are ph_track_affinity_cnt's cnt)
enum { REC_K = 0, REC_M = 1, REC_NEED = 2, REC_MODE = 3, REC_CODE = 4, REC_ROWS = 5 };
enum { MODE_RUN = 0, MODE_EMPTY = 1, MODE_STICKY = 2, MODE_REFUSE = 3 };

struct DState {
    // state
    float* pool; int64_t* trk_id; int64_t* trk_seen; int32_t* trk_label; int32_t* trk_slot; float* trk_box;
    int32_t* bd_count; int32_t* bd_label; int32_t* bd_slot; float* bd_box; int32_t* free_stack; int64_t* status;
    // per-frame scratch
    int32_t* rec; int32_t* kept; int32_t* det_lab; float* kbox; int32_t* memo_slot; int32_t* memo_lab; int32_t* act;
    int64_t* tmp_id; int64_t* tmp_seen; int32_t* tmp_label; int32_t* tmp_slot; float* tmp_box;
    float* det; float* memo; float* score; void* aff_ws;
    // one frame's outputs for ph_assoc_plan_track
    int32_t* io_kept; int64_t* io_ids; int32_t* io_kc;
    int capacity, max_dets, gens;
};

struct DFrame {
    const float* boxes; const int32_t* labels; const int32_t* count; const int32_t* refuse; const float* embeds;
    int32_t* kept_out; int64_t* ids_out; int32_t* kept_count;
};

// the S streams of a launch: stream s's block starts s * stride bytes behind stream 0's; active (nullable): int32 [S], 0 = idle
struct DBank { DState st; size_t stride; const int32_t* active; };
// the S frames of a launch: frame s at base + s * stride (elements), outputs included; zero_idle: an idle stream's kept_count is
// written 0 (the caller's array; never when the outputs are the streams' own io_* pieces)
struct DIo {
    ph_dtracker_io io;
    int64_t kept_stride, ids_stride, kc_stride;
    int zero_idle;
};

template <class T>
__device__ __forceinline__ T* shifted(T* p, size_t bytes) { return (T*)((char*)p + bytes); }

__device__ __forceinline__ DState stream_state(const DBank& bk, int s) {
    const size_t o = (size_t)s * bk.stride;
    const DState& b = bk.st;
    DState d;
    d.pool = shifted(b.pool, o); d.trk_id = shifted(b.trk_id, o); d.trk_seen = shifted(b.trk_seen, o); d.trk_label = shifted(b.trk_label, o);
    d.trk_slot = shifted(b.trk_slot, o); d.trk_box = shifted(b.trk_box, o);
    d.bd_count = shifted(b.bd_count, o); d.bd_label = shifted(b.bd_label, o); d.bd_slot = shifted(b.bd_slot, o); d.bd_box = shifted(b.bd_box, o);
    d.free_stack = shifted(b.free_stack, o); d.status = shifted(b.status, o);
    d.rec = shifted(b.rec, o); d.kept = shifted(b.kept, o); d.det_lab = shifted(b.det_lab, o); d.kbox = shifted(b.kbox, o);
    d.memo_slot = shifted(b.memo_slot, o); d.memo_lab = shifted(b.memo_lab, o); d.act = shifted(b.act, o);
    d.tmp_id = shifted(b.tmp_id, o); d.tmp_seen = shifted(b.tmp_seen, o); d.tmp_label = shifted(b.tmp_label, o); d.tmp_slot = shifted(b.tmp_slot, o);
    d.tmp_box = shifted(b.tmp_box, o);
    d.det = shifted(b.det, o); d.memo = shifted(b.memo, o); d.score = shifted(b.score, o); d.aff_ws = shifted((char*)b.aff_ws, o);
    d.io_kept = shifted(b.io_kept, o); d.io_ids = shifted(b.io_ids, o); d.io_kc = shifted(b.io_kc, o);
    d.capacity = b.capacity; d.max_dets = b.max_dets; d.gens = b.gens;
    return d;
}

__device__ __forceinline__ DFrame stream_frame(const DIo& d, int s) {
    const ph_dtracker_io& io = d.io;
    return DFrame{io.boxes + s * io.box_stride, io.labels + s * io.label_stride, io.counts + s * io.count_stride,
                  io.refuse ? io.refuse + s * io.refuse_stride : nullptr, io.embeds + s * io.embed_stride,
                  io.kept_out + s * d.kept_stride, io.ids_out + s * d.ids_stride, io.kept_counts + s * d.kc_stride};
}

__device__ __forceinline__ bool stream_idle(const DBank& bk, int s) { return bk.active && bk.active[s] == 0; }

struct Geo {
    ph_dtracker_layout lay;
    size_t o[19];                                        // the scratch pieces, in DState's order
};

int resolve(const ph_tracker_cfg* c, int capacity, int max_dets, Geo& g, const char* fn) {
    if (!c) { ph_set_error("%s: null cfg", fn); return PH_EINVAL; }
    if (capacity < 16 || capacity > DT_MAXC) { ph_set_error("%s: capacity must be 16 .. %d rows, got %d", fn, DT_MAXC, capacity); return PH_EINVAL; }
    if (max_dets < 1 || max_dets > DT_MAXN) { ph_set_error("%s: max_dets must be 1 .. %d, got %d", fn, DT_MAXN, max_dets); return PH_EINVAL; }
    if (c->metric < 0 || c->metric > 2) { ph_set_error("%s: metric must be 0 (bisoftmax), 1 (softmax) or 2 (cosine), got %d", fn, c->metric); return PH_EINVAL; }
    if (c->memo_tracklet_frames < 0) { ph_set_error("%s: memo_tracklet_frames must be >= 0", fn); return PH_EINVAL; }
    if (c->memo_backdrop_frames < 0 || c->memo_backdrop_frames > DT_MAXG) {
        ph_set_error("%s: memo_backdrop_frames must be 0 .. %d, got %d", fn, DT_MAXG, c->memo_backdrop_frames);
        return PH_EINVAL;
    }
    const size_t C = capacity, N = max_dets, G = c->memo_backdrop_frames;
    g = Geo{};
    ph_dtracker_layout& l = g.lay;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
    l.pool = take(C * TE * 4);
    l.trk_id = take(C * 8); l.trk_seen = take(C * 8); l.trk_label = take(C * 4); l.trk_slot = take(C * 4); l.trk_box = take(C * 20);
    l.bd_count = take(G * 4); l.bd_label = take(G * N * 4); l.bd_slot = take(G * N * 4); l.bd_box = take(G * N * 20);
    l.free_stack = take(C * 4);
    l.status = take(PH_DTRK_ST_WORDS * 8);
    l.workspace = o;
    const size_t pieces[19] = {32, N * 4, N * 4, N * 20, C * 4, C * 4, N * 8,            // rec kept det_lab kbox memo_slot memo_lab act
                               C * 8, C * 8, C * 4, C * 4, C * 20,                      // tmp_*
                               N * TE * 4, C * TE * 4, N * C * 4, ph_track_affinity_workspace_bytes((int)N, (int)C),
                               N * 4, N * 8, 4};                                        // io_*
    for (int i = 0; i < 19; ++i) g.o[i] = take(pieces[i]);
    l.total_bytes = o;
    l.capacity = capacity; l.max_dets = max_dets; l.generations = (int)G;
    return PH_OK;
}

// ---- iou of two boxes, the host's iou1 (ph_tracker.hip) operation for operation: std::max / std::min as comparisons, every
// arithmetic result rounded to fp32 on its own, one correctly rounded division
__device__ __forceinline__ float dmax(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float dmin(float a, float b) { return b < a ? b : a; }
__device__ float iou1(const float* a, const float* b) {
    const float x1 = dmax(a[0], b[0]), y1 = dmax(a[1], b[1]), x2 = dmin(a[2], b[2]), y2 = dmin(a[3], b[3]);
    const float dw = __fsub_rn(x2, x1);
    const float dh = __fsub_rn(y2, y1);
    const float w = dmax(dw, 0.f), h = dmax(dh, 0.f);
    const float inter = __fmul_rn(w, h);
    const float aw = __fsub_rn(a[2], a[0]);
    const float ah = __fsub_rn(a[3], a[1]);
    const float bw = __fsub_rn(b[2], b[0]);
    const float bh = __fsub_rn(b[3], b[1]);
    const float a1 = __fmul_rn(aw, ah);
    const float a2 = __fmul_rn(bw, bh);
    const float s = __fadd_rn(a1, a2);
    const float d = __fsub_rn(s, inter);
    const float u = dmax(d, 1e-6f);
    return __fdiv_rn(inter, u);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- one launch: empty tables, full free stack (slot 0 on top, as ph_tracker_create leaves it), counter, status; grid (x, S), the
// streams outside `mask` are untouched
__global__ __launch_bounds__(256) void k_dtrk_reset(DBank bk, unsigned long long mask, int64_t first_frame_id) {
    const int s = blockIdx.y;
    if (!((mask >> s) & 1ull)) return;
    const DState st = stream_state(bk, s);
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (int i = i0; i < st.capacity; i += step) {
        st.free_stack[i] = st.capacity - 1 - i;
        st.trk_id[i] = 0; st.trk_seen[i] = 0; st.trk_label[i] = 0; st.trk_slot[i] = 0;
        for (int e = 0; e < 5; ++e) st.trk_box[i * 5 + e] = 0.f;
    }
    for (int i = i0; i < st.gens * st.max_dets; i += step) {
        st.bd_label[i] = 0; st.bd_slot[i] = 0;
        for (int e = 0; e < 5; ++e) st.bd_box[i * 5 + e] = 0.f;
    }
    for (int i = i0; i < st.gens; i += step) st.bd_count[i] = 0;
    if (i0 == 0) {
        for (int i = 0; i < PH_DTRK_ST_WORDS; ++i) st.status[i] = 0;
        st.status[PH_DTRK_ST_REFUSED_FRAME] = -1;
        st.status[PH_DTRK_ST_FRAME_ID] = first_frame_id;
        st.status[PH_DTRK_ST_FREE] = st.capacity;
    }
}

// ---- k_dtrk_prepare, one workgroup: what ph_tracker_match does before its first upload.  Stable descending-score order by counting
// (rank = scores above + equal scores at a lower index: std::stable_sort's order), de-duplication against EVERY higher-scored
// detection, kept or not (:147-155) -- so parallel over the positions --, compaction to the kept list, and the memory columns:
// tracklets in creation order, then the backdrops newest first.  Writes the frame record and the row / label / slot tables.  Grid (S).
__global__ __launch_bounds__(256) void k_dtrk_prepare(DBank bk, ph_tracker_cfg c, DIo io) {
    if (stream_idle(bk, blockIdx.x)) return;
    const DState st = stream_state(bk, blockIdx.x);
    const DFrame f = stream_frame(io, blockIdx.x);
    __shared__ float sbox[DT_MAXN * 5];
    __shared__ float skey[DT_MAXN];
    __shared__ int order[DT_MAXN];
    __shared__ int keep[DT_MAXN];
    const int t = threadIdx.x;
    const int n = f.count[0];
    int mode = MODE_RUN, code = PH_DTRK_OK;
    if (st.status[PH_DTRK_ST_ERROR] != 0) mode = MODE_STICKY;
    else if (n < 0 || n > st.max_dets) { mode = MODE_REFUSE; code = PH_DTRK_ECOUNT; }
    else if (f.refuse && f.refuse[0] != 0) { mode = MODE_REFUSE; code = PH_DTRK_EREFUSED; }
    else if (n == 0) mode = MODE_EMPTY;
    if (mode != MODE_RUN) {                              // uniform over the workgroup
        if (t == 0) {
            st.rec[REC_K] = 0; st.rec[REC_M] = 0; st.rec[REC_NEED] = 0; st.rec[REC_MODE] = mode; st.rec[REC_CODE] = code; st.rec[REC_ROWS] = 0;
        }
        return;
    }
    for (int e = t; e < n * 5; e += 256) sbox[e] = f.boxes[e];
    __syncthreads();
    if (t < n) { const float s = sbox[t * 5 + 4]; skey[t] = s == s ? s : -INFINITY; }      // a NaN score sorts last: the ranks stay a permutation
    __syncthreads();
    if (t < n) {
        const float s = skey[t];
        int r = 0;
        for (int j = 0; j < n; ++j) { const float v = skey[j]; r += (v > s || (v == s && j < t)) ? 1 : 0; }
        order[r] = t;
    }
    __syncthreads();
    if (t < n) {
        const float* bi = sbox + order[t] * 5;
        const float thr = bi[4] < c.obj_score_thr ? c.nms_backdrop_iou_thr : c.nms_class_iou_thr;
        int kp = 1;
        for (int j = 0; j < t && kp; ++j) kp = iou1(bi, sbox + order[j] * 5) > thr ? 0 : 1;
        keep[t] = kp;
    }
    __syncthreads();
    int pos = 0, k = 0;
    for (int j = 0; j < n; ++j) { pos += j < t ? keep[j] : 0; k += keep[j]; }
    if (t < n && keep[t]) {
        const int src = order[t];
        st.kept[pos] = src; f.kept_out[pos] = src; st.det_lab[pos] = f.labels[src];
        for (int e = 0; e < 5; ++e) st.kbox[pos * 5 + e] = sbox[src * 5 + e];
    }
    const int rows = clampi((int)st.status[PH_DTRK_ST_ROWS], 0, st.capacity);
    for (int j = t; j < rows; j += 256) { st.memo_slot[j] = st.trk_slot[j]; st.memo_lab[j] = st.trk_label[j]; }
    int m = rows;
    for (int g = 0; g < st.gens; ++g) {
        const int cnt = clampi(st.bd_count[g], 0, min(st.max_dets, st.capacity - m));      // rows + backdrops own distinct slots: m <= capacity
        for (int r = t; r < cnt; r += 256) {
            st.memo_slot[m + r] = st.bd_slot[g * st.max_dets + r];
            st.memo_lab[m + r] = st.bd_label[g * st.max_dets + r];
        }
        m += cnt;
    }
    if (t == 0) {
        st.rec[REC_K] = k; st.rec[REC_M] = m; st.rec[REC_NEED] = (k > 0 && rows > 0 && m > 0) ? 1 : 0;       // `empty` looks at the tracklets only (:39-41)
        st.rec[REC_MODE] = MODE_RUN; st.rec[REC_CODE] = PH_DTRK_OK; st.rec[REC_ROWS] = rows;
    }
}

// ---- k_trk_gather (ph_tracker.hip) in device-count form: grid (max_dets + capacity, S), workgroups beyond the counts return
__global__ __launch_bounds__(256) void k_dtrk_gather(DBank bk, DIo io) {
    if (stream_idle(bk, blockIdx.y)) return;
    const DState st = stream_state(bk, blockIdx.y);
    const float* __restrict__ det_src = io.io.embeds + blockIdx.y * io.io.embed_stride;
    const int r = blockIdx.x;
    if (r < st.max_dets) {
        if (r >= st.rec[REC_K]) return;
        st.det[(int64_t)r * TE + threadIdx.x] = det_src[(int64_t)st.kept[r] * TE + threadIdx.x];
    } else {
        const int j = r - st.max_dets;
        if (!st.rec[REC_NEED] || j >= st.rec[REC_M]) return;
        const int slot = clampi(st.memo_slot[j], 0, st.capacity - 1);
        st.memo[(int64_t)j * TE + threadIdx.x] = st.pool[(int64_t)slot * TE + threadIdx.x];
    }
}

// ---- k_trk_update (ph_tracker.hip) in device-count form: grid (max_dets, S)
__global__ __launch_bounds__(256) void k_dtrk_update(DBank bk, float one_minus, float mom) {
    if (stream_idle(bk, blockIdx.y)) return;
    const DState st = stream_state(bk, blockIdx.y);
    const int i = blockIdx.x;
    if (i >= st.rec[REC_K]) return;
    const int slot = clampi(st.act[2 * i], 0, st.capacity - 1), mode = st.act[2 * i + 1];
    if (mode == 0) return;
    const float v = st.det[(int64_t)i * TE + threadIdx.x];
    float* p = st.pool + (int64_t)slot * TE + threadIdx.x;
    *p = mode == 2 ? v : __fadd_rn(__fmul_rn(one_minus, *p), __fmul_rn(mom, v));
}

// ---- k_dtrk_assign, one workgroup: everything ph_tracker_match does between its score download and its update launch.
// A matched detection's tracklet row IS its column (columns 0 .. rows - 1 are the rows in creation order) and a new id is in no row
// (ids are unique and below num_tracklets), so the host's searches for an id become `mrow`.  Grid (S).
__global__ __launch_bounds__(256) void k_dtrk_assign(DBank bk, ph_tracker_cfg c, DIo io) {
    __shared__ float red_v[256];
    __shared__ int red_j[256];
    __shared__ unsigned char taken[DT_MAXC];
    __shared__ int64_t ids[DT_MAXN];
    __shared__ int mrow[DT_MAXN];
    __shared__ int cov[DT_MAXN];
    __shared__ float kb[DT_MAXN * 5];
    __shared__ int old_slots[DT_MAXN];
    __shared__ int part[256];
    __shared__ int s_born, s_refuse, s_free, s_rows;
    const int t = threadIdx.x;
    if (stream_idle(bk, blockIdx.x)) {                   // uniform: no frame in this step, nothing of the stream is read or written
        if (io.zero_idle && t == 0) io.io.kept_counts[blockIdx.x * io.kc_stride] = 0;
        return;
    }
    const DState st = stream_state(bk, blockIdx.x);
    const DFrame f = stream_frame(io, blockIdx.x);
    int64_t* S = st.status;
    const int mode = st.rec[REC_MODE];
    if (mode != MODE_RUN) {                              // an empty frame, a frame behind an error, or a frame refused by its own tables
        if (t == 0) {
            f.kept_count[0] = 0;
            if (mode == MODE_REFUSE) { S[PH_DTRK_ST_ERROR] = st.rec[REC_CODE]; S[PH_DTRK_ST_REFUSED_FRAME] = S[PH_DTRK_ST_FRAMES_SEEN]; }
            S[PH_DTRK_ST_FRAMES_SEEN] += 1;
        }
        return;
    }
    const int N = st.max_dets, G = st.gens;
    const int k = clampi(st.rec[REC_K], 0, N), m = clampi(st.rec[REC_M], 0, st.capacity), need_aff = st.rec[REC_NEED], rows = st.rec[REC_ROWS];
    const int64_t fid = S[PH_DTRK_ST_FRAME_ID], num0 = S[PH_DTRK_ST_NUM_TRACKLETS];
    const int free0 = clampi((int)S[PH_DTRK_ST_FREE], 0, st.capacity);
    for (int e = t; e < k * 5; e += 256) kb[e] = st.kbox[e];
    if (t < k) { ids[t] = -1; mrow[t] = -1; }
    for (int j = t; j < m; j += 256) taken[j] = 0;
    __syncthreads();
    // ---- greedy, in detection (score) order: the first maximal still-free column (:183-197); ties go to the lower index
    if (need_aff) {
        for (int i = 0; i < k; ++i) {
            const float* row = st.score + (size_t)i * m;
            float bv = 0.f;
            int bj = INT_MAX;
            for (int j = t; j < m; j += 256) {
                const float v = taken[j] ? 0.f : row[j];
                if (bj == INT_MAX || v > bv) { bv = v; bj = j; }
            }
            red_v[t] = bv; red_j[t] = bj;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (t < s) {
                    const float ov = red_v[t + s];
                    const int oj = red_j[t + s];
                    if (oj != INT_MAX && (red_j[t] == INT_MAX || ov > red_v[t] || (ov == red_v[t] && oj < red_j[t]))) { red_v[t] = ov; red_j[t] = oj; }
                }
                __syncthreads();
            }
            const float conf = red_v[0];
            const int best = red_j[0];
            if (t == 0 && best < rows && conf > c.match_score_thr) {        // best >= rows: a backdrop (id -1)
                if (kb[i * 5 + 4] > c.obj_score_thr) { ids[i] = st.trk_id[best]; mrow[i] = best; taken[best] = 1; }
                else if (conf > c.nms_conf_thr) ids[i] = -2;
            }
            __syncthreads();
        }
    }
    // ---- new tracks (:198-205)
    if (t == 0) {
        int born = 0;
        for (int i = 0; i < k; ++i)
            if (ids[i] == -1 && kb[i * 5 + 4] > c.init_score_thr) ids[i] = num0 + born++;
        s_born = born;
    }
    __syncthreads();
    // an unmatched detection becomes a backdrop unless an earlier kept one covers it
    if (t < k) {
        int cv = 0;
        if (ids[t] == -1 && G > 0)
            for (int j = 0; j < t && !cv; ++j) cv = iou1(kb + t * 5, kb + j * 5) > c.nms_backdrop_iou_thr ? 1 : 0;
        cov[t] = cv;
    }
    __syncthreads();
    // ---- every pool slot this frame takes is reserved BEFORE the first mutation
    if (t == 0) {
        int need = 0;
        for (int i = 0; i < k; ++i) {
            if (ids[i] > -1) need += mrow[i] < 0 ? 1 : 0;
            else if (ids[i] == -1 && G > 0) need += cov[i] ? 0 : 1;
        }
        s_refuse = need > free0 ? 1 : 0;
    }
    __syncthreads();
    if (s_refuse) {
        if (t == 0) {
            f.kept_count[0] = 0;
            st.rec[REC_K] = 0;                           // the update launch behind this one does nothing
            S[PH_DTRK_ST_ERROR] = PH_DTRK_EPOOL; S[PH_DTRK_ST_REFUSED_FRAME] = S[PH_DTRK_ST_FRAMES_SEEN];
            S[PH_DTRK_ST_FRAMES_SEEN] += 1;
        }
        return;
    }
    // ---- update_memo (:47-102).  The backdrop generations move one place down first; the oldest hands its slots back after this
    // frame's takes, as the host's pop_back does.  Thread t owns entry t of every generation.
    int old_cnt = 0;
    if (G > 0) {
        old_cnt = clampi(st.bd_count[G - 1], 0, N);
        if (t < old_cnt) old_slots[t] = st.bd_slot[(G - 1) * N + t];
        __syncthreads();
        if (t < N)
            for (int g = G - 1; g >= 1; --g) {
                st.bd_label[g * N + t] = st.bd_label[(g - 1) * N + t];
                st.bd_slot[g * N + t] = st.bd_slot[(g - 1) * N + t];
                for (int e = 0; e < 5; ++e) st.bd_box[(g * N + t) * 5 + e] = st.bd_box[((g - 1) * N + t) * 5 + e];
            }
        __syncthreads();
    }
    if (t == 0) {
        int fc = free0, nrows = rows, nb = 0;
        for (int g = G - 1; g >= 1; --g) st.bd_count[g] = st.bd_count[g - 1];
        for (int i = 0; i < k; ++i) {
            int sl = 0, md = 0;
            const float* bi = kb + i * 5;
            if (ids[i] > -1) {
                int r = mrow[i];
                if (r >= 0) { sl = st.trk_slot[r]; md = 1; }
                else {
                    r = nrows++; sl = st.free_stack[--fc]; md = 2;       // reserved above
                    st.trk_id[r] = ids[i]; st.trk_slot[r] = sl;
                }
                st.trk_label[r] = st.det_lab[i]; st.trk_seen[r] = fid;
                for (int e = 0; e < 5; ++e) st.trk_box[r * 5 + e] = bi[e];
            } else if (ids[i] == -1 && G > 0 && !cov[i]) {
                sl = st.free_stack[--fc]; md = 2;                        // reserved above
                st.bd_label[nb] = st.det_lab[i]; st.bd_slot[nb] = sl;
                for (int e = 0; e < 5; ++e) st.bd_box[nb * 5 + e] = bi[e];
                ++nb;
            }
            st.act[2 * i] = sl; st.act[2 * i + 1] = md;
        }
        if (G > 0) {
            st.bd_count[0] = nb;
            for (int q = 0; q < old_cnt; ++q) st.free_stack[fc++] = old_slots[q];
        }
        s_free = fc; s_rows = nrows;
    }
    __syncthreads();
    // ---- expiry: tracklets unseen for memo_tracklet_frames frames leave, the others keep their order (a stable compaction through
    // the tmp_* tables); the slots go back in row order
    const int R = s_rows;
    int fc = s_free;
    const int per = (R + 255) / 256, r0 = min(t * per, R), r1 = min(r0 + per, R);
    int live = 0;
    for (int r = r0; r < r1; ++r) live += (fid - st.trk_seen[r] < (int64_t)c.memo_tracklet_frames) ? 1 : 0;
    part[t] = live;
    __syncthreads();
    int before = 0, total = 0;
    for (int q = 0; q < 256; ++q) { before += q < t ? part[q] : 0; total += part[q]; }
    if (total != R) {                                    // uniform
        int w = before, x = fc + (r0 - before);
        for (int r = r0; r < r1; ++r) {
            if (fid - st.trk_seen[r] < (int64_t)c.memo_tracklet_frames) {
                st.tmp_id[w] = st.trk_id[r]; st.tmp_seen[w] = st.trk_seen[r]; st.tmp_label[w] = st.trk_label[r]; st.tmp_slot[w] = st.trk_slot[r];
                for (int e = 0; e < 5; ++e) st.tmp_box[w * 5 + e] = st.trk_box[r * 5 + e];
                ++w;
            } else if (x < st.capacity)
                st.free_stack[x++] = st.trk_slot[r];
        }
        __syncthreads();
        for (int r = t; r < total; r += 256) {
            st.trk_id[r] = st.tmp_id[r]; st.trk_seen[r] = st.tmp_seen[r]; st.trk_label[r] = st.tmp_label[r]; st.trk_slot[r] = st.tmp_slot[r];
            for (int e = 0; e < 5; ++e) st.trk_box[r * 5 + e] = st.tmp_box[r * 5 + e];
        }
        fc += R - total;
    }
    if (t < k) f.ids_out[t] = ids[t];
    if (t == 0) {
        f.kept_count[0] = k;
        S[PH_DTRK_ST_MATCHED] += 1;
        S[PH_DTRK_ST_NUM_TRACKLETS] = num0 + s_born;
        S[PH_DTRK_ST_ROWS] = total;
        S[PH_DTRK_ST_FREE] = fc;
        S[PH_DTRK_ST_FRAME_ID] = fid + 1;
        S[PH_DTRK_ST_FRAMES_SEEN] += 1;
    }
}

}  // namespace

struct ph_dtracker {
    ph_tracker_cfg c;
    Geo g;
    DState st;                                           // stream 0's
    int streams;
    size_t stride;                                       // bytes between two streams' blocks: g.lay.total_bytes
};

namespace {

constexpr int DT_MAXS = 64;

int check_streams(int streams, const char* fn) {
    if (streams < 1 || streams > DT_MAXS) { ph_set_error("%s: streams must be 1 .. %d, got %d", fn, DT_MAXS, streams); return PH_EINVAL; }
    return PH_OK;
}

int create(const ph_tracker_cfg* cfg, void* device_mem, size_t device_bytes, int capacity, int max_dets, int streams, ph_dtracker** out,
           const char* fn) {
    Geo g;
    int rc = resolve(cfg, capacity, max_dets, g, fn);
    if (!rc) rc = check_streams(streams, fn);
    if (rc) return rc;
    if (!out) { ph_set_error("%s: null out", fn); return PH_EINVAL; }
    *out = nullptr;
    PH_RUN(ph_check_buffers(fn, nullptr, device_mem, device_bytes, g.lay.total_bytes * (size_t)streams));
    ph_dtracker* t = new (std::nothrow) ph_dtracker;
    if (!t) { ph_set_error("%s: out of host memory", fn); return PH_EINVAL; }
    t->c = *cfg;
    t->g = g;
    t->streams = streams;
    t->stride = g.lay.total_bytes;
    char* b = (char*)device_mem;
    const ph_dtracker_layout& l = g.lay;
    DState& s = t->st;
    s.pool = (float*)(b + l.pool);
    s.trk_id = (int64_t*)(b + l.trk_id); s.trk_seen = (int64_t*)(b + l.trk_seen);
    s.trk_label = (int32_t*)(b + l.trk_label); s.trk_slot = (int32_t*)(b + l.trk_slot); s.trk_box = (float*)(b + l.trk_box);
    s.bd_count = (int32_t*)(b + l.bd_count); s.bd_label = (int32_t*)(b + l.bd_label); s.bd_slot = (int32_t*)(b + l.bd_slot);
    s.bd_box = (float*)(b + l.bd_box);
    s.free_stack = (int32_t*)(b + l.free_stack);
    s.status = (int64_t*)(b + l.status);
    const size_t* o = g.o;
    s.rec = (int32_t*)(b + o[0]); s.kept = (int32_t*)(b + o[1]); s.det_lab = (int32_t*)(b + o[2]); s.kbox = (float*)(b + o[3]);
    s.memo_slot = (int32_t*)(b + o[4]); s.memo_lab = (int32_t*)(b + o[5]); s.act = (int32_t*)(b + o[6]);
    s.tmp_id = (int64_t*)(b + o[7]); s.tmp_seen = (int64_t*)(b + o[8]); s.tmp_label = (int32_t*)(b + o[9]); s.tmp_slot = (int32_t*)(b + o[10]);
    s.tmp_box = (float*)(b + o[11]);
    s.det = (float*)(b + o[12]); s.memo = (float*)(b + o[13]); s.score = (float*)(b + o[14]); s.aff_ws = b + o[15];
    s.io_kept = (int32_t*)(b + o[16]); s.io_ids = (int64_t*)(b + o[17]); s.io_kc = (int32_t*)(b + o[18]);
    s.capacity = capacity; s.max_dets = max_dets; s.gens = l.generations;
    *out = t;
    return PH_OK;
}

int check_io(const ph_dtracker_io* io, const char* fn) {
    if (!(io->boxes && io->labels && io->counts && io->embeds)) { ph_set_error("%s: null boxes, labels, counts or embeds", fn); return PH_EINVAL; }
    if (!(io->kept_out && io->ids_out && io->kept_counts)) { ph_set_error("%s: null kept_out, ids_out or kept_counts", fn); return PH_EINVAL; }
    return PH_OK;
}

// one frame of each of S streams: the seven launches
int launch_frames(const ph_dtracker* t, const DIo& io, int S, const int32_t* active, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const DState& st = t->st;
    const ph_tracker_cfg& c = t->c;
    const DBank bk{st, t->stride, active};
    hipLaunchKernelGGL(k_dtrk_prepare, dim3(S), dim3(256), 0, s, bk, c, io);
    hipLaunchKernelGGL(k_dtrk_gather, dim3(st.max_dets + st.capacity, S), dim3(TE), 0, s, bk, io);
    ph_track_affinity_cnt(st.det, st.det_lab, st.memo, st.memo_lab, st.max_dets, st.capacity, st.rec, c.metric, c.with_cats, st.score, st.aff_ws, S,
                          t->stride, active, stream);
    hipLaunchKernelGGL(k_dtrk_assign, dim3(S), dim3(256), 0, s, bk, c, io);
    hipLaunchKernelGGL(k_dtrk_update, dim3(st.max_dets, S), dim3(TE), 0, s, bk, c.one_minus_momentum, c.memo_momentum);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

int reset_streams(ph_dtracker* t, uint64_t mask, int64_t first_frame_id, void* stream) {
    const DBank bk{t->st, t->stride, nullptr};
    hipLaunchKernelGGL(k_dtrk_reset, dim3((t->st.capacity + 255) / 256, t->streams), dim3(256), 0, (hipStream_t)stream, bk,
                       (unsigned long long)mask, first_frame_id);
    PH_CHECK_LAUNCH();
    return PH_OK;
}

}  // namespace

extern "C" size_t ph_dtracker_device_bytes(const ph_tracker_cfg* cfg, int capacity, int max_dets) {
    Geo g;
    if (resolve(cfg, capacity, max_dets, g, "ph_dtracker_device_bytes")) return 0;
    return g.lay.total_bytes;
}

extern "C" size_t ph_dtracker_bank_bytes(const ph_tracker_cfg* cfg, int capacity, int max_dets, int streams) {
    Geo g;
    if (resolve(cfg, capacity, max_dets, g, "ph_dtracker_bank_bytes") || check_streams(streams, "ph_dtracker_bank_bytes")) return 0;
    return g.lay.total_bytes * (size_t)streams;
}

extern "C" int ph_dtracker_create(const ph_tracker_cfg* cfg, void* device_mem, size_t device_bytes, int capacity, int max_dets, ph_dtracker** out) {
    return create(cfg, device_mem, device_bytes, capacity, max_dets, 1, out, "ph_dtracker_create");
}

extern "C" int ph_dtracker_bank_create(const ph_tracker_cfg* cfg, void* device_mem, size_t device_bytes, int capacity, int max_dets, int streams,
                                       ph_dtracker** out) {
    return create(cfg, device_mem, device_bytes, capacity, max_dets, streams, out, "ph_dtracker_bank_create");
}

extern "C" void ph_dtracker_destroy(ph_dtracker* t) { delete t; }

extern "C" int ph_dtracker_get_layout(const ph_dtracker* t, ph_dtracker_layout* out) {
    PH_CHECK_ARG(t && out, "null tracker or out");
    *out = t->g.lay;
    return PH_OK;
}

extern "C" int ph_dtracker_get_streams(const ph_dtracker* t, int* streams_out, uint64_t* stride_bytes_out) {
    PH_CHECK_ARG(t && streams_out && stride_bytes_out, "null tracker or out");
    *streams_out = t->streams;
    *stride_bytes_out = t->stride;
    return PH_OK;
}

PhDtrkScratch ph_dtracker_scratch(const ph_dtracker* t) {
    return PhDtrkScratch{t->st.io_kept, t->st.io_ids, t->st.io_kc, t->st.max_dets, t->streams, (int64_t)(t->stride / 4), (int64_t)(t->stride / 8),
                         (int64_t)(t->stride / 4)};
}

extern "C" int ph_dtracker_reset(ph_dtracker* t, int64_t first_frame_id, void* stream) {
    PH_CHECK_ARG(t != nullptr, "null tracker");
    return reset_streams(t, ~0ull, first_frame_id, stream);
}

extern "C" int ph_dtracker_reset_streams(ph_dtracker* t, int64_t mask_bits, int64_t first_frame_id, void* stream) {
    PH_CHECK_ARG(t != nullptr, "null tracker");
    const uint64_t mask = (uint64_t)mask_bits;
    PH_CHECK_ARG(t->streams == DT_MAXS || (mask >> t->streams) == 0, "the mask names a stream the tracker does not have");
    return reset_streams(t, mask, first_frame_id, stream);
}

extern "C" int ph_dtracker_run(ph_dtracker* t, const ph_dtracker_io* io, int B, void* stream) {
    PH_CHECK_ARG(t && io, "null tracker or io");
    PH_CHECK_ARG(t->streams == 1, "a tracker of several streams takes its frames side by side: ph_dtracker_step");
    PH_CHECK_ARG(B >= 1 && B <= 4096, "B must be 1 .. 4096 frames");
    PH_RUN(check_io(io, "ph_dtracker_run"));
    const int N = t->st.max_dets;
    for (int b = 0; b < B; ++b) {                        // in order through the one state: frame b is a step of the bank of one
        DIo f{*io, 0, 0, 0, 0};
        f.io.boxes += b * io->box_stride; f.io.labels += b * io->label_stride; f.io.counts += b * io->count_stride;
        if (io->refuse) f.io.refuse += b * io->refuse_stride;
        f.io.embeds += b * io->embed_stride;
        f.io.kept_out += (int64_t)b * N; f.io.ids_out += (int64_t)b * N; f.io.kept_counts += b;
        PH_RUN(launch_frames(t, f, 1, nullptr, stream));
    }
    return PH_OK;
}

extern "C" int ph_dtracker_step(ph_dtracker* t, const ph_dtracker_io* io, const int32_t* active, void* stream) {
    PH_CHECK_ARG(t && io, "null tracker or io");
    PH_RUN(check_io(io, "ph_dtracker_step"));
    const int N = t->st.max_dets;
    return launch_frames(t, DIo{*io, N, N, 1, 1}, t->streams, active, stream);
}

// ph_dtracker_step with the outputs in the streams' own io_* pieces (ph_dtracker_scratch), for ph_assoc_plan_track / _track_streams
int ph_dtracker_step_scratch(ph_dtracker* t, const ph_dtracker_io* in, const int32_t* active, void* stream) {
    const PhDtrkScratch sc = ph_dtracker_scratch(t);
    DIo f{*in, sc.kept_stride, sc.ids_stride, sc.kc_stride, 0};
    f.io.kept_out = sc.kept; f.io.ids_out = sc.ids; f.io.kept_counts = sc.kept_count;
    return launch_frames(t, f, t->streams, active, stream);
}
