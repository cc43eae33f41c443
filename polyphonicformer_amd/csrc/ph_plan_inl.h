// The host scaffold every native plan family shares: pack bytes / layout / pack, workspace bytes, create, geometry-of
// and info, written once over a per-family description.  The extern "C" entry points stay in the families' files and forward here
// with their own name (`fn`, which starts every message).  A description F is a struct of
//   types:      Cfg, Geo (with .pack_total / .lay of a pack family, .total of a plan family), Layout, Geometry,
//               Plan (with .g, .pack, .ws)
//   functions:  int resolve(const Cfg*, Geo&, const char* fn)   the family's one rule: cfg checks, pack and workspace pieces
//               void build_table(const Geo&, PhPackTable&)      the pack's pieces for ph_pack_pieces
//               int nparams(const Geo&), const char* param_name(const Cfg*, int)
//               void fill_geometry(const Geo&, Geometry*)
//   constant:   kPackBlocks, the workgroup cap of the family's ph_pack_pieces launch
// and holds only what the templates it is used with read.  Order of the checks in every call: resolve, null arguments, the rest.
#pragma once
#include <new>

#include "ph_common.h"

namespace plan {

template <class F> size_t pack_bytes(const typename F::Cfg* cfg, const char* fn) {
    typename F::Geo g;
    return F::resolve(cfg, g, fn) ? 0 : g.pack_total;
}

template <class F> int pack_layout(const typename F::Cfg* cfg, typename F::Layout* layout, const char* fn) {
    typename F::Geo g;
    PH_RUN(F::resolve(cfg, g, fn));
    PH_CHECK_ARG_AS(fn, layout != nullptr, "null layout");
    *layout = g.lay;
    return PH_OK;
}

template <class F> int pack(const typename F::Cfg* cfg, const float* const* params, void* blob, void* stream, const char* fn) {
    typename F::Geo g;
    PH_RUN(F::resolve(cfg, g, fn));
    PH_CHECK_ARG_AS(fn, params && blob, "null params or pack");
    const int n = F::nparams(g);
    for (int i = 0; i < n; ++i)
        if (!params[i]) { ph_set_error("%s: parameter %d (%s) is NULL", fn, i, F::param_name(cfg, i)); return PH_EINVAL; }
    PH_CHECK_ARG_AS(fn, ((uintptr_t)blob & 255) == 0, "pack must be 256-byte aligned");
    PH_CHECK_ARG_AS(fn, g.pack_total / 16 < (1ull << 32), "pack too large");      // the table counts 16-byte units in 32 bits
    PhPackTable t{};
    F::build_table(g, t);
    for (int i = 0; i < n; ++i) t.p[i] = params[i];
    return ph_pack_pieces(fn, t, blob, F::kPackBlocks, stream);
}

template <class F> size_t workspace_bytes(const typename F::Cfg* cfg, const char* fn) {
    typename F::Geo g;
    return F::resolve(cfg, g, fn) ? 0 : g.total;
}

// *out: the new plan with g / pack / ws set, for the family to finish
template <class F> int create(const typename F::Cfg* cfg, const void* pack, void* workspace, size_t workspace_bytes, typename F::Plan** out,
                              const char* fn) {
    typename F::Geo g;
    PH_RUN(F::resolve(cfg, g, fn));
    PH_CHECK_ARG_AS(fn, out && pack && workspace, "null pack, workspace or out");
    *out = nullptr;
    PH_RUN(ph_check_buffers(fn, pack, workspace, workspace_bytes, g.total));
    typename F::Plan* p = new (std::nothrow) typename F::Plan;
    if (!p) { ph_set_error("%s: out of host memory", fn); return PH_EINVAL; }
    p->g = g;
    p->pack = (const char*)pack;
    p->ws = (char*)workspace;
    *out = p;
    return PH_OK;
}

template <class F> int geometry_of(const typename F::Cfg* cfg, typename F::Geometry* out, const char* fn) {
    typename F::Geo g;
    PH_RUN(F::resolve(cfg, g, fn));
    PH_CHECK_ARG_AS(fn, out != nullptr, "null out");
    F::fill_geometry(g, out);
    return PH_OK;
}

template <class F> int info(const typename F::Plan* p, typename F::Geometry* out, const char* fn) {
    PH_CHECK_ARG_AS(fn, p && out, "null plan or out");
    F::fill_geometry(p->g, out);
    return PH_OK;
}

}  // namespace plan
