// ph_gt_segments / ph_gt_index_maps: a frame's ground truth from the dataset's panoptic id map (include/polyhead.h).
// Replaces, per frame, the loader's numpy work in front of ph_gt_prepare: to_coco (datasets/cityscapes_dvps.py:89-109), np.unique and one
// full-frame compare per segment (datasets/pipelines/loading.py:201-220), bitmasks2bboxes (:11-21), and the nearest resize, flip, crop
// and pad of the [G][H][W] stack and the depth map (datasets/pipelines/transforms.py).  The stack never exists: the id map stays one
// id per pixel through every one of those transforms, which are separable nearest gathers.
//
// ph_gt_segments, four launches over `frames` maps (key = the raw id = class * raw_divisor + instance, n_map * raw_divisor keys):
//   k_gtseg_clear     zeroes the frame's presence bitmap and its flag word in the workspace
//   k_gtseg_presence  grid (workgroups, frames): every workgroup marks the keys of its pixels in an LDS bitmap (a word is read before
//                     it is OR-ed, so after the first pixels of a segment no atomic is issued) and ORs its non-zero words into the
//                     frame's bitmap
//   k_gtseg_list      one workgroup per frame: the keys present by prefix popcount, their mapped ids, the rank of every mapped id
//                     among the others (at most 254, all against all in LDS); writes ids and empty boxes into the table, and the
//                     keys (ascending) with their table rows into the workspace
//   k_gtseg_boxes     grid (workgroups, frames): a thread walks 8 consecutive pixels, finds a pixel's row by a search of the sorted
//                     keys in LDS (the previous pixel's key first) and folds each run of one segment into LDS min / max / add;
//                     the rows a workgroup touched are merged into the table with the same integer atomics
// Integer min / max / add / or only: no result depends on the order the workgroups run in.
//
// ph_gt_index_maps, two launches:
//   k_gtseg_index     a thread owns 16 adjacent output columns of one output row: 16 gathers through src_y / src_x, raw id -> mapped
//                     id -> index by a search of the frame's kept ids in LDS (the previous pixel's key first), one 16-byte store
//   k_gtseg_depth     a thread owns 4 adjacent columns of one row of the PADDED output: min(u / depth_div, depth_max) / scale_mean in
//                     fp32 with IEEE divisions, zeros in the pad, one 16-byte store
#include <limits.h>

#include "ph_common.h"

namespace {

constexpr int GS_T = 256;                  // threads per workgroup
constexpr int GS_MAXW = PH_GTSEG_MAX_KEYS / 32;   // words of a presence bitmap: 32 KB of LDS
constexpr int GS_HDR = 64;                 // int32 words in front of a frame's lists in the workspace: [0] segments, [1] flags
constexpr int GS_PX = 8;                   // consecutive pixels per thread of k_gtseg_boxes
constexpr int GS_C = 16;                   // output columns per thread of k_gtseg_index: one 16-byte store
constexpr int GS_DC = 4;                   // output columns per thread of k_gtseg_depth
constexpr int GS_MAX_WGS = 128;            // workgroups per frame of the two passes over the map
constexpr int GS_ROW = PH_GTSEG_ROW_WORDS;

struct GsMap {
    int16_t m[256];                        // raw class -> training class, -1: not a class of the dataset; entries from n_map on are -1
    int32_t n_map, raw_div, div, no_obj;
};
struct GsFrames {
    int16_t kept_n[PH_GTPREP_MAX_FRAMES];
    float scale_mean[PH_GTPREP_MAX_FRAMES];
};

// a frame's piece of the workspace: bitmap [nwords] | header [GS_HDR] | keys [256] | rows [256], all int32
__host__ __device__ inline size_t gs_frame_words(int nwords) { return (size_t)(nwords + GS_HDR + 512 + 63) / 64 * 64; }

__global__ __launch_bounds__(GS_T) void k_gtseg_clear(uint32_t* __restrict__ ws, int nwords, size_t fwords) {
    uint32_t* __restrict__ w = ws + (size_t)blockIdx.y * fwords;
    const int i = blockIdx.x * GS_T + threadIdx.x;
    if (i < nwords + GS_HDR) w[i] = 0u;
}

template <typename T>
__global__ __launch_bounds__(GS_T) void k_gtseg_presence(const T* __restrict__ raw, int64_t npix, int nkeys, int nwords,
                                                          uint32_t* __restrict__ ws, size_t fwords) {
    __shared__ uint32_t bm[GS_MAXW];
    const int f = blockIdx.y, t = threadIdx.x;
    for (int w = t; w < nwords; w += GS_T) bm[w] = 0u;
    __syncthreads();
    const T* __restrict__ src = raw + (int64_t)f * npix;
    bool outside = false;
    for (int64_t p = (int64_t)blockIdx.x * GS_T + t; p < npix; p += (int64_t)gridDim.x * GS_T) {
        const int64_t key = (int64_t)src[p];
        if (key < 0 || key >= nkeys) {
            outside = true;
            continue;
        }
        const uint32_t bit = 1u << ((int)key & 31);
        if (!(bm[(int)key >> 5] & bit)) atomicOr(&bm[(int)key >> 5], bit);
    }
    __syncthreads();
    uint32_t* __restrict__ g = ws + (size_t)f * fwords;
    for (int w = t; w < nwords; w += GS_T)
        if (bm[w]) atomicOr(&g[w], bm[w]);
    if (outside) atomicOr(&g[nwords + 1], (uint32_t)PH_GTSEG_EOUTSIDE);
}

__global__ __launch_bounds__(GS_T) void k_gtseg_list(GsMap mp, int nwords, uint32_t* __restrict__ ws, size_t fwords,
                                                      int32_t* __restrict__ tables, int32_t* __restrict__ status) {
    __shared__ int32_t scan[GS_T];
    __shared__ int32_t skey[GS_T], smid[GS_T];
    __shared__ uint32_t sflags;
    const int f = blockIdx.x, t = threadIdx.x;
    uint32_t* __restrict__ g = ws + (size_t)f * fwords;
    int32_t* __restrict__ hdr = reinterpret_cast<int32_t*>(g) + nwords;
    const int wpt = (nwords + GS_T - 1) / GS_T, w0 = t * wpt, w1 = min(nwords, w0 + wpt);
    if (t == 0) sflags = g[nwords + 1];
    // the segments among this thread's keys; a key whose class maps to -1 is a flag, one that maps to no_obj no segment
    int cnt = 0;
    uint32_t flags = 0u;
    for (int w = w0; w < w1; ++w) {
        uint32_t bits = g[w];
        while (bits) {
            const int key = w * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            const int m = mp.m[key / mp.raw_div];
            if (m < 0) flags |= PH_GTSEG_EUNMAPPED;
            else if (m != mp.no_obj) ++cnt;
        }
    }
    scan[t] = cnt;
    __syncthreads();
    if (flags) atomicOr(&sflags, flags);
    for (int d = 1; d < GS_T; d <<= 1) {
        const int v = t >= d ? scan[t - d] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const int n = scan[GS_T - 1];
    int at = scan[t] - cnt;
    for (int w = w0; w < w1 && at < PH_GTPREP_MAX_SEGMENTS; ++w) {
        uint32_t bits = g[w];
        while (bits && at < PH_GTPREP_MAX_SEGMENTS) {
            const int key = w * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            const int c = key / mp.raw_div, m = mp.m[c];
            if (m >= 0 && m != mp.no_obj) {
                skey[at] = key;
                smid[at] = m * mp.div + (key - c * mp.raw_div);
                ++at;
            }
        }
    }
    __syncthreads();
    const uint32_t fl = sflags | (n > PH_GTPREP_MAX_SEGMENTS ? (uint32_t)PH_GTSEG_ETOOMANY : 0u);
    if (t == 0) {
        status[f] = (int32_t)fl;
        hdr[0] = fl ? 0 : n;               // a refused frame has no segments for k_gtseg_boxes
    }
    if (fl) return;                        // its table stays as the caller left it
    int32_t* __restrict__ tab = tables + (size_t)f * PH_GTSEG_TABLE_WORDS;
    int32_t* __restrict__ keys = hdr + GS_HDR;
    int32_t* __restrict__ rows = keys + 256;
    if (t == 0) tab[0] = n;
    if (t < n) {
        const int mine = smid[t];
        int r = 0;
        for (int j = 0; j < n; ++j) r += smid[j] < mine ? 1 : 0;          // the class map is one-to-one, so the mapped ids differ
        keys[t] = skey[t];
        rows[t] = r;
        int32_t* __restrict__ row = tab + 1 + r * GS_ROW;
        row[0] = mine;
        row[1] = INT_MAX;
        row[2] = INT_MAX;
        row[3] = -1;
        row[4] = -1;
        row[5] = 0;
    } else if (t < PH_GTPREP_MAX_SEGMENTS) {
        int32_t* __restrict__ row = tab + 1 + t * GS_ROW;
#pragma unroll
        for (int k = 0; k < GS_ROW; ++k) row[k] = 0;
    }
}

// index of `key` in the ascending list s[0 .. n), -1 when it is not there
__device__ __forceinline__ int gs_find(const int32_t* s, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && s[lo] == key ? lo : -1;
}

template <typename T>
__global__ __launch_bounds__(GS_T) void k_gtseg_boxes(const T* __restrict__ raw, int Ws, int64_t npix, int nkeys, int nwords,
                                                       const uint32_t* __restrict__ ws, size_t fwords, int32_t* __restrict__ tables) {
    __shared__ int32_t skey[GS_T], srow[GS_T];
    __shared__ int32_t acc[PH_GTPREP_MAX_SEGMENTS * 5];
    const int f = blockIdx.y, t = threadIdx.x;
    const int32_t* __restrict__ hdr = reinterpret_cast<const int32_t*>(ws + (size_t)f * fwords) + nwords;
    const int n = min(hdr[0], PH_GTPREP_MAX_SEGMENTS);
    if (n <= 0) return;
    skey[t] = t < n ? hdr[GS_HDR + t] : INT_MAX;
    srow[t] = t < n ? hdr[GS_HDR + 256 + t] : -1;
    for (int i = t; i < n * 5; i += GS_T) {
        const int k = i % 5;
        acc[i] = k < 2 ? INT_MAX : (k < 4 ? -1 : 0);
    }
    __syncthreads();
    const T* __restrict__ src = raw + (int64_t)f * npix;
    const int64_t nitems = (npix + GS_PX - 1) / GS_PX;
    for (int64_t item = (int64_t)blockIdx.x * GS_T + t; item < nitems; item += (int64_t)gridDim.x * GS_T) {
        const int64_t p0 = item * GS_PX;
        const int live = (int)min((int64_t)GS_PX, npix - p0);
        int y = (int)(p0 / Ws), x = (int)(p0 - (int64_t)y * Ws);
        int64_t last_key = -1;
        int last_row = -1;
        int cur = -1, rx0 = 0, rx1 = 0, ry = 0, rc = 0;                 // the run of one segment in one image row
        auto flush = [&]() {
            if (cur >= 0 && cur < n) {
                int32_t* a = acc + cur * 5;
                atomicMin(&a[0], rx0);
                atomicMin(&a[1], ry);
                atomicMax(&a[2], rx1);
                atomicMax(&a[3], ry);
                atomicAdd(&a[4], rc);
            }
        };
        for (int i = 0; i < live; ++i) {
            const int64_t key = (int64_t)src[p0 + i];
            int row;
            if (key == last_key) {
                row = last_row;
            } else {
                const int at = key >= 0 && key < nkeys ? gs_find(skey, n, (int)key) : -1;
                row = at >= 0 ? srow[at] : -1;
                last_key = key;
                last_row = row;
            }
            if (row != cur || x == 0 || i == 0) {
                if (i) flush();
                cur = row;
                rx0 = x;
                ry = y;
                rc = 0;
            }
            rx1 = x;
            ++rc;
            if (++x == Ws) {
                x = 0;
                ++y;
            }
        }
        flush();
    }
    __syncthreads();
    int32_t* __restrict__ tab = tables + (size_t)f * PH_GTSEG_TABLE_WORDS + 1;
    for (int r = t; r < n; r += GS_T) {
        const int32_t* a = acc + r * 5;
        if (a[4] > 0) {
            int32_t* __restrict__ row = tab + r * GS_ROW;
            atomicMin(&row[1], a[0]);
            atomicMin(&row[2], a[1]);
            atomicMax(&row[3], a[2]);
            atomicMax(&row[4], a[3]);
            atomicAdd(&row[5], a[4]);
        }
    }
}

// VEC: Wc is a multiple of 16 and the output base 16-byte aligned, so a thread's sixteen bytes are one aligned store
template <typename T, bool VEC>
__global__ __launch_bounds__(GS_T) void k_gtseg_index(const T* __restrict__ raw, GsMap mp, GsFrames fr, const int32_t* __restrict__ kept_id,
                                                       const int32_t* __restrict__ src_y, const int32_t* __restrict__ src_x, int Hs, int Ws,
                                                       int Hc, int Wc, uint8_t* __restrict__ seg) {
    __shared__ int32_t skept[GS_T];
    const int f = blockIdx.y, t = threadIdx.x;
    const int n = min((int)fr.kept_n[f], PH_GTPREP_MAX_SEGMENTS);
    skept[t] = t < n ? kept_id[(int64_t)f * 256 + t] : INT_MAX;
    __syncthreads();
    const int nx = (Wc + GS_C - 1) / GS_C;
    const int idx = blockIdx.x * GS_T + t;
    if (idx >= Hc * nx) return;
    const int y = idx / nx, x = (idx - y * nx) * GS_C;
    const int live = min(GS_C, Wc - x);
    const int nkeys = mp.n_map * mp.raw_div;
    const int sy = src_y[(int64_t)f * Hc + y];
    const bool row_in = sy >= 0 && sy < Hs;
    const T* __restrict__ srow = raw + ((int64_t)f * Hs + (row_in ? sy : 0)) * Ws;
    const int32_t* __restrict__ sxp = src_x + (int64_t)f * Wc + x;
    uint32_t out[GS_C / 4] = {0u, 0u, 0u, 0u};
    int64_t last_key = -1;
    int last_v = 255;
#pragma unroll
    for (int c = 0; c < GS_C; ++c) {
        int v = 255;
        if (c < live) {
            const int sx = sxp[c];
            if (row_in && sx >= 0 && sx < Ws) {                       // an index outside the file is a pixel of no segment
                const int64_t key = (int64_t)srow[sx];
                if (key == last_key) {
                    v = last_v;
                } else {
                    if (key >= 0 && key < nkeys) {
                        const int k = (int)key, cl = k / mp.raw_div, m = mp.m[cl];
                        if (m >= 0 && m != mp.no_obj) {
                            const int at = gs_find(skept, n, m * mp.div + (k - cl * mp.raw_div));
                            v = at >= 0 ? at : 255;
                        }
                    }
                    last_key = key;
                    last_v = v;
                }
            }
        }
        out[c >> 2] |= (uint32_t)v << (8 * (c & 3));
    }
    uint8_t* __restrict__ o = seg + ((int64_t)f * Hc + y) * Wc + x;
    if (VEC) {
        *reinterpret_cast<uint4*>(o) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int c = 0; c < GS_C; ++c)
            if (c < live) o[c] = (uint8_t)(out[c >> 2] >> (8 * (c & 3)));
    }
}

template <bool VEC>
__global__ __launch_bounds__(GS_T) void k_gtseg_depth(const uint16_t* __restrict__ raw_depth, GsFrames fr, const int32_t* __restrict__ src_y,
                                                       const int32_t* __restrict__ src_x, int Hs, int Ws, int Hc, int Wc, int Hp, int Wp,
                                                       float depth_div, float depth_max, float* __restrict__ depth) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const int nx = (Wp + GS_DC - 1) / GS_DC;
    const int idx = blockIdx.x * GS_T + threadIdx.x;
    if (idx >= Hp * nx) return;
    const int y = idx / nx, x = (idx - y * nx) * GS_DC;
    const int live = min(GS_DC, Wp - x);
    const float sm = fr.scale_mean[f];
    int sy = -1;
    if (y < Hc) sy = src_y[(int64_t)f * Hc + y];
    const bool row_in = sy >= 0 && sy < Hs;
    const uint16_t* __restrict__ srow = raw_depth + ((int64_t)f * Hs + (row_in ? sy : 0)) * Ws;
    float v[GS_DC];
#pragma unroll
    for (int c = 0; c < GS_DC; ++c) {
        v[c] = 0.f;
        if (row_in && x + c < Wc) {
            const int sx = src_x[(int64_t)f * Wc + x + c];
            if (sx >= 0 && sx < Ws) {
                const float d = (float)srow[sx] / depth_div;          // loading.py:171-173: / 256., then values >= 80 become 80
                v[c] = (d >= depth_max ? depth_max : d) / sm;         // transforms.py:32
            }
        }
    }
    float* __restrict__ o = depth + ((int64_t)f * Hp + y) * Wp + x;
    if (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < GS_DC; ++c)
            if (c < live) o[c] = v[c];
    }
}

// the mapping arguments both calls share; fills `mp`
int gs_check_map(const char* fn, const int32_t* class_map, int n_map, int raw_divisor, int divisor, int no_obj_class, GsMap& mp) {
    PH_CHECK_ARG_AS(fn, class_map, "null class_map");
    PH_CHECK_ARG_AS(fn, n_map >= 1 && n_map <= 256, "1 .. 256 raw classes");
    PH_CHECK_ARG_AS(fn, raw_divisor >= 1 && divisor >= raw_divisor && divisor <= (1 << 23),
                    "1 <= raw_divisor <= divisor <= 2^23 (an instance part keeps its value, a mapped id fits int32)");
    PH_CHECK_ARG_AS(fn, no_obj_class >= 0 && no_obj_class <= 255, "no_obj_class in 0 .. 255");
    if ((int64_t)n_map * raw_divisor > PH_GTSEG_MAX_KEYS) {
        ph_set_error("%s: n_map * raw_divisor = %lld raw ids, the presence bitmap holds %d", fn, (long long)n_map * raw_divisor,
                     PH_GTSEG_MAX_KEYS);
        return PH_EUNSUPPORTED;
    }
    bool seen[256] = {false};
    for (int c = 0; c < 256; ++c) mp.m[c] = -1;
    for (int c = 0; c < n_map; ++c) {
        const int m = class_map[c];
        if (m < -1 || m > 255) {
            ph_set_error("%s: class_map[%d] = %d; a training class is 0 .. 255, -1 means not a class of the dataset", fn, c, m);
            return PH_EINVAL;
        }
        if (m >= 0 && m != no_obj_class) {
            if (seen[m]) {
                ph_set_error("%s: class_map maps two raw classes to %d (the second is %d): their segments would share ids", fn, m, c);
                return PH_EINVAL;
            }
            seen[m] = true;
        }
        mp.m[c] = (int16_t)m;
    }
    mp.n_map = n_map;
    mp.raw_div = raw_divisor;
    mp.div = divisor;
    mp.no_obj = no_obj_class;
    return PH_OK;
}

int gs_check_maps(const char* fn, const void* raw, int dtype, int frames, int Hs, int Ws) {
    PH_CHECK_ARG_AS(fn, raw, "null raw id maps");
    PH_CHECK_ARG_AS(fn, dtype == PH_GTSEG_I32 || dtype == PH_GTSEG_U16, "dtype is PH_GTSEG_I32 or PH_GTSEG_U16");
    PH_CHECK_ARG_AS(fn, frames >= 1 && frames <= PH_GTPREP_MAX_FRAMES, "1 .. 64 frames per call");
    PH_CHECK_ARG_AS(fn, Hs >= 1 && Ws >= 1 && Hs <= 65536 && Ws <= 65536 && (int64_t)Hs * Ws < ((int64_t)1 << 31),
                    "map sizes of 1 .. 65536 and fewer than 2^31 pixels");
    PH_CHECK_ARG_AS(fn, ((uintptr_t)raw & (dtype == PH_GTSEG_I32 ? 3 : 1)) == 0, "the raw id maps are aligned to their element");
    return PH_OK;
}

}  // namespace

extern "C" size_t ph_gt_segments_workspace_bytes(int frames, int n_map, int raw_divisor) {
    if (frames < 1 || frames > PH_GTPREP_MAX_FRAMES || n_map < 1 || n_map > 256 || raw_divisor < 1 ||
        (int64_t)n_map * raw_divisor > PH_GTSEG_MAX_KEYS) {
        ph_set_error("ph_gt_segments_workspace_bytes: 1 .. 64 frames, 1 .. 256 raw classes and n_map * raw_divisor <= %d; got %d, %d, %d",
                     PH_GTSEG_MAX_KEYS, frames, n_map, raw_divisor);
        return 0;
    }
    const int nwords = (n_map * raw_divisor + 31) / 32;
    return al256((size_t)frames * gs_frame_words(nwords) * 4);
}

extern "C" int ph_gt_segments(const void* raw, int dtype, int frames, int Hs, int Ws, const int32_t* class_map, int n_map, int raw_divisor,
                              int divisor, int no_obj_class, int32_t* tables, int32_t* status, void* workspace, size_t workspace_bytes,
                              void* stream) {
    PH_RUN(gs_check_maps(__func__, raw, dtype, frames, Hs, Ws));
    GsMap mp;
    PH_RUN(gs_check_map(__func__, class_map, n_map, raw_divisor, divisor, no_obj_class, mp));
    PH_CHECK_ARG(tables && status, "null tables or status");
    PH_CHECK_ARG(((uintptr_t)tables & 3) == 0 && ((uintptr_t)status & 3) == 0, "tables and status are int32");
    PH_RUN(ph_check_buffers(__func__, nullptr, workspace, workspace_bytes, ph_gt_segments_workspace_bytes(frames, n_map, raw_divisor)));
    const int nkeys = n_map * raw_divisor, nwords = (nkeys + 31) / 32;
    const size_t fwords = gs_frame_words(nwords);
    const int64_t npix = (int64_t)Hs * Ws;
    uint32_t* ws = static_cast<uint32_t*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(GS_T);
    hipLaunchKernelGGL(k_gtseg_clear, dim3((nwords + GS_HDR + GS_T - 1) / GS_T, frames), block, 0, st, ws, nwords, fwords);
    const unsigned wgs_a = (unsigned)min((int64_t)GS_MAX_WGS, (npix + GS_T * 16 - 1) / (GS_T * 16));
    const unsigned wgs_b = (unsigned)min((int64_t)GS_MAX_WGS, (npix + GS_T * GS_PX - 1) / (GS_T * GS_PX));
    if (dtype == PH_GTSEG_I32) {
        hipLaunchKernelGGL(k_gtseg_presence<int32_t>, dim3(wgs_a, frames), block, 0, st, static_cast<const int32_t*>(raw), npix, nkeys, nwords, ws,
                           fwords);
    } else {
        hipLaunchKernelGGL(k_gtseg_presence<uint16_t>, dim3(wgs_a, frames), block, 0, st, static_cast<const uint16_t*>(raw), npix, nkeys, nwords,
                           ws, fwords);
    }
    hipLaunchKernelGGL(k_gtseg_list, dim3(frames), block, 0, st, mp, nwords, ws, fwords, tables, status);
    if (dtype == PH_GTSEG_I32) {
        hipLaunchKernelGGL(k_gtseg_boxes<int32_t>, dim3(wgs_b, frames), block, 0, st, static_cast<const int32_t*>(raw), Ws, npix, nkeys, nwords, ws,
                           fwords, tables);
    } else {
        hipLaunchKernelGGL(k_gtseg_boxes<uint16_t>, dim3(wgs_b, frames), block, 0, st, static_cast<const uint16_t*>(raw), Ws, npix, nkeys, nwords,
                           ws, fwords, tables);
    }
    PH_CHECK_LAUNCH();
    return PH_OK;
}

extern "C" int ph_gt_index_maps(const void* raw, int dtype, const uint16_t* raw_depth, int frames, int Hs, int Ws, const int32_t* class_map,
                                int n_map, int raw_divisor, int divisor, int no_obj_class, const int32_t* kept_id, const int32_t* kept_n,
                                const int32_t* src_y_host, const int32_t* src_x_host, const int32_t* src_y, const int32_t* src_x, int Hc, int Wc,
                                int Hp, int Wp, float depth_div, float depth_max, const float* scale_mean, uint8_t* seg, float* depth,
                                void* stream) {
    PH_RUN(gs_check_maps(__func__, raw, dtype, frames, Hs, Ws));
    GsMap mp;
    PH_RUN(gs_check_map(__func__, class_map, n_map, raw_divisor, divisor, no_obj_class, mp));
    PH_CHECK_ARG(kept_id && kept_n && src_y_host && src_x_host && src_y && src_x && seg, "null argument");
    PH_CHECK_ARG(Hc >= 1 && Wc >= 1 && Hp >= Hc && Wp >= Wc && Hp <= 65536 && Wp <= 65536, "1 <= Hc <= Hp <= 65536 and 1 <= Wc <= Wp <= 65536");
    PH_CHECK_ARG(((uintptr_t)kept_id & 3) == 0 && ((uintptr_t)src_y & 3) == 0 && ((uintptr_t)src_x & 3) == 0, "kept_id, src_y and src_x are int32");
    PH_CHECK_ARG(!raw_depth == !depth, "raw_depth and depth come together");
    GsFrames fr;
    for (int b = 0; b < PH_GTPREP_MAX_FRAMES; ++b) {
        fr.kept_n[b] = 0;
        fr.scale_mean[b] = 1.f;
    }
    if (raw_depth) {
        PH_CHECK_ARG(scale_mean, "the depth map needs scale_mean");
        PH_CHECK_ARG(((uintptr_t)raw_depth & 1) == 0 && ((uintptr_t)depth & 3) == 0, "raw_depth is uint16, depth fp32");
        PH_CHECK_ARG(depth_div > 0.f && depth_max > 0.f, "depth_div and depth_max are positive");
    }
    for (int b = 0; b < frames; ++b) {
        if (kept_n[b] < 0 || kept_n[b] > PH_GTPREP_MAX_SEGMENTS) {
            ph_set_error("ph_gt_index_maps: 0 .. %d kept segments per frame (index 255 means none); frame %d has %d", PH_GTPREP_MAX_SEGMENTS, b,
                         kept_n[b]);
            return PH_EINVAL;
        }
        fr.kept_n[b] = (int16_t)kept_n[b];
        if (raw_depth) {
            if (!(scale_mean[b] > 0.f)) {
                ph_set_error("ph_gt_index_maps: scale_mean[%d] = %g; a scale is positive", b, (double)scale_mean[b]);
                return PH_EINVAL;
            }
            fr.scale_mean[b] = scale_mean[b];
        }
        for (int y = 0; y < Hc; ++y) {
            const int v = src_y_host[(size_t)b * Hc + y];
            if (v < -1 || v >= Hs) {
                ph_set_error("ph_gt_index_maps: src_y[%d][%d] = %d; a file row is 0 .. %d, -1 means none", b, y, v, Hs - 1);
                return PH_EINVAL;
            }
        }
        for (int x = 0; x < Wc; ++x) {
            const int v = src_x_host[(size_t)b * Wc + x];
            if (v < -1 || v >= Ws) {
                ph_set_error("ph_gt_index_maps: src_x[%d][%d] = %d; a file column is 0 .. %d, -1 means none", b, x, v, Ws - 1);
                return PH_EINVAL;
            }
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(GS_T);
    {
        const int nx = (Wc + GS_C - 1) / GS_C;
        const dim3 grid((unsigned)(((int64_t)Hc * nx + GS_T - 1) / GS_T), frames);
        const bool vec = Wc % GS_C == 0 && ((uintptr_t)seg & 15) == 0;
#define GS_INDEX(T, V)                                                                                                                 \
    hipLaunchKernelGGL((k_gtseg_index<T, V>), grid, block, 0, st, static_cast<const T*>(raw), mp, fr, kept_id, src_y, src_x, Hs, Ws, Hc, Wc, \
                       seg)
        if (dtype == PH_GTSEG_I32) {
            if (vec) GS_INDEX(int32_t, true);
            else GS_INDEX(int32_t, false);
        } else {
            if (vec) GS_INDEX(uint16_t, true);
            else GS_INDEX(uint16_t, false);
        }
#undef GS_INDEX
    }
    if (raw_depth) {
        const int nx = (Wp + GS_DC - 1) / GS_DC;
        const dim3 grid((unsigned)(((int64_t)Hp * nx + GS_T - 1) / GS_T), frames);
        const bool vec = Wp % GS_DC == 0 && ((uintptr_t)depth & 15) == 0;
        if (vec)
            hipLaunchKernelGGL(k_gtseg_depth<true>, grid, block, 0, st, raw_depth, fr, src_y, src_x, Hs, Ws, Hc, Wc, Hp, Wp, depth_div, depth_max,
                               depth);
        else
            hipLaunchKernelGGL(k_gtseg_depth<false>, grid, block, 0, st, raw_depth, fr, src_y, src_x, Hs, Ws, Hc, Wc, Hp, Wp, depth_div, depth_max,
                               depth);
    }
    PH_CHECK_LAUNCH();
    return PH_OK;
}
