// libpolyhead: version / error / switch plumbing of the C ABI (include/polyhead.h).
#include <stdarg.h>

#include <atomic>
#include <mutex>

#include "ph_common.h"

static thread_local char g_err[512] = "";

void ph_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int ph_check_buffers(const char* fn, const void* pack_or_null, const void* workspace, size_t workspace_bytes, size_t need) {
    PH_CHECK_ARG_AS(fn, ((uintptr_t)pack_or_null & 255) == 0, "pack must be 256-byte aligned");
    PH_CHECK_ARG_AS(fn, workspace != nullptr, "null workspace");
    if (workspace_bytes < need) {
        ph_set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
        return PH_EWORKSPACE;
    }
    PH_CHECK_ARG_AS(fn, ((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    return PH_OK;
}

int ph_num_cus() {
    static const int n = [] {
        int dev = 0, cu = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        return cu > 0 ? cu : 0;
    }();
    return n;
}

// ---- the switch table (include/polyhead.h PH_SWITCH_*): the ONE place of this library that reads the environment
static std::atomic<int> g_switch[PH_SWITCH_COUNT];

static bool switch_value_ok(int id, int v) {
    if (id == PH_SWITCH_CONV_TILE_ROWS) return v == 0 || v == 2 || v == 4;
    if (id == PH_SWITCH_QUERY_TIMELINE || id == PH_SWITCH_PAN_GENERIC) return v == 0 || v == 1;
    return v >= 0;
}

static void switches_from_env() {
    static const char* const names[PH_SWITCH_COUNT + 1] = {"PH_CONV_WGS", "PH_UP2_WGS", "PH_QUERY_NRT", "PH_QUERY_TIMELINE", "PH_CONV_TH",
                                                           "PH_GNSUM_WGS", "PH_CPLANES_TPW", "PH_PAN_GENERIC", "PH_CONV_TH_NOW"};
    static std::once_flag once;
    std::call_once(once, [] {
        for (int i = 0; i <= PH_SWITCH_COUNT; ++i) {
            const char* e = getenv(names[i]);
            if (!e) continue;
            const int id = i == PH_SWITCH_COUNT ? PH_SWITCH_CONV_TILE_ROWS : i;     // the retired spelling: read last, so it wins
            int v = atoi(e);
            if (id == PH_SWITCH_PAN_GENERIC) v = 1;                                  // set to anything
            if (id == PH_SWITCH_QUERY_TIMELINE) v = v != 0;
            if (switch_value_ok(id, v)) g_switch[id].store(v, std::memory_order_relaxed);
        }
    });
}

int ph_switch(int id) {
    switches_from_env();
    return g_switch[id].load(std::memory_order_relaxed);
}

extern "C" int ph_set_switch(int id, int value) {
    PH_CHECK_ARG(id >= 0 && id < PH_SWITCH_COUNT, "id must be a PH_SWITCH_*");
    PH_CHECK_ARG(switch_value_ok(id, value), "value outside the switch's range");
    switches_from_env();           // first: a later first use must not put the environment's value over this one
    g_switch[id].store(value, std::memory_order_relaxed);
    return PH_OK;
}

extern "C" int ph_get_switch(int id, int* value) {
    PH_CHECK_ARG(id >= 0 && id < PH_SWITCH_COUNT && value, "id must be a PH_SWITCH_*, value non-null");
    *value = ph_switch(id);
    return PH_OK;
}

extern "C" int ph_version(void) { return PH_VERSION; }
extern "C" const char* ph_last_error_string(void) { return g_err; }
