// wc_args.h -- how an entry point refuses bad arguments, before any device work (host code only;
// included from wc_common.h).  wc_graph_louvain (wc_louvain.hip) is the example to copy: shapes,
// NULL pointers, then one table of input spans and one of output spans through wc_check_spans;
// wc_graph_louvain_sign (wc_louvain_sign.hip) for a seeded entry with a workspace of slots.
#pragma once
#include <stdarg.h>
#include <stdint.h>

// printf into the thread's error buffer; returns code.  fmt == nullptr leaves the buffer alone: a
// *_workspace_size query shares its entry point's shape checks and has no message.
__attribute__((format(printf, 2, 3))) inline int wc_fail(int code, const char* fmt, ...) {
    if (fmt) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(wc_errbuf(), 512, fmt, ap);
        va_end(ap);
    }
    return code;
}

// do [a, a + na) and [b, b + nb) share a byte
inline bool wc_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// one pointer argument; p == nullptr: an optional one left out, which passes every check below
struct WcSpan {
    const char* name;
    const void* p;
    size_t bytes;  // of the whole array
    int align;     // a power of two
};

inline int wc_check_align(const char* fn, const WcSpan* s, int n) {
    for (int k = 0; k < n; ++k)
        if ((uintptr_t)s[k].p & (uintptr_t)(s[k].align - 1))
            return wc_fail(WC_EINVAL, "%s: %s must be %d-byte aligned", fn, s[k].name, s[k].align);
    return WC_OK;
}

// no outs[o] may overlap an ins[k]
inline int wc_check_alias(const char* fn, const WcSpan* outs, int nouts, const WcSpan* ins, int nins) {
    for (int o = 0; o < nouts; ++o)
        for (int k = 0; k < nins; ++k)
            if (outs[o].p && ins[k].p && wc_overlap(outs[o].p, outs[o].bytes, ins[k].p, ins[k].bytes))
                return wc_fail(WC_EINVAL, "%s: %s must not alias %s", fn, outs[o].name, ins[k].name);
    return WC_OK;
}

// no outs[o] may overlap an earlier one
inline int wc_check_disjoint(const char* fn, const WcSpan* outs, int nouts) {
    for (int o = 1; o < nouts; ++o)
        if (int rc = wc_check_alias(fn, outs + o, 1, outs, o)) return rc;
    return WC_OK;
}

// the usual order: every alignment, then no output over an input or an earlier output.  An entry
// whose order differs calls the passes above one by one.
inline int wc_check_spans(const char* fn, const WcSpan* ins, int nins, const WcSpan* outs, int nouts) {
    if (int rc = wc_check_align(fn, ins, nins)) return rc;
    if (int rc = wc_check_align(fn, outs, nouts)) return rc;
    if (int rc = wc_check_alias(fn, outs, nouts, ins, nins)) return rc;
    return wc_check_disjoint(fn, outs, nouts);
}

// a seeded batch, B matrices times R seeds, a run each: B >= 1, R >= 1, N in [nmin, nmax], B R < 2^31, in
// that order.  The caller's clauses: why nmin (nullptr: the bare "N < nmin"), why nmax, and what B R
// counts (nullptr: no bound on it).
inline int wc_check_seeded(const char* fn, int B, int R, int N, int nmin, const char* nmin_why, int nmax,
                           const char* nmax_why, const char* runs) {
    if (B < 1) return wc_fail(WC_EINVAL, "%s: B < 1", fn);
    if (R < 1) return wc_fail(WC_EINVAL, "%s: R < 1", fn);
    if (N < nmin && !nmin_why) return wc_fail(WC_EINVAL, "%s: N < %d", fn, nmin);
    if (N < nmin) return wc_fail(WC_EINVAL, "%s: N = %d < %d (%s)", fn, N, nmin, nmin_why);
    if (N > nmax) return wc_fail(WC_EUNSUPPORTED, "%s: N = %d > %d (%s)", fn, N, nmax, nmax_why);
    if (runs && (int64_t)B * R > INT32_MAX)
        return wc_fail(WC_EINVAL, "%s: 2^31 %s or more (B times R)", fn, runs);
    return WC_OK;
}

// a workspace of one slot per workgroup, the workgroups striding over the runs: min(ws_bytes / slot, runs)
// slots and the span they cover, for the table of outputs; slot_what is the slot's formula, as "16 N^2"
struct WcSlots {
    size_t slots;
    WcSpan span;
};

inline int wc_plan_slots(const char* fn, const void* workspace, size_t ws_bytes, size_t slot, const char* slot_what,
                         size_t runs, WcSlots* plan) {
    if (ws_bytes < slot)
        return wc_fail(WC_EINVAL, "%s: ws_bytes = %zu is less than one slot of %s = %zu bytes", fn, ws_bytes, slot_what,
                       slot);
    plan->slots = ws_bytes / slot < runs ? ws_bytes / slot : runs;
    plan->span = {"workspace", workspace, plan->slots * slot, 8};
    return WC_OK;
}

// size_fn names the query that returns need
inline int wc_check_workspace(const char* fn, const char* size_fn, const void* workspace, size_t ws_bytes, size_t need) {
    if (workspace && ws_bytes >= need) return WC_OK;
    return wc_fail(WC_EWORKSPACE, "%s: workspace NULL or %zu bytes < %s() = %zu", fn, ws_bytes, size_fn, need);
}

// a kernel's dynamic LDS above the 64 KiB every kernel may have
template <class Kernel>
int wc_raise_lds(const char* fn, Kernel kernel, size_t bytes) {
    if (bytes <= 65536) return WC_OK;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e == hipSuccess ? WC_OK : wc_fail(WC_EHIP, "%s: %s", fn, hipGetErrorString(e));
}

// f(start, count) over [0, total) in steps of per_launch: a grid that would pass a launch's limit
template <class F>
void wc_chunks(int64_t total, int64_t per_launch, F&& f) {
    for (int64_t i0 = 0; i0 < total; i0 += per_launch) f(i0, total - i0 < per_launch ? total - i0 : per_launch);
}
