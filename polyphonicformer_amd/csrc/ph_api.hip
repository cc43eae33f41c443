// libpolyhead: version / error plumbing of the C ABI (include/polyhead.h).
#include <stdarg.h>

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

extern "C" int ph_version(void) { return PH_VERSION; }
extern "C" const char* ph_last_error_string(void) { return g_err; }
