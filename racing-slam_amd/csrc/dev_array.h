// dev_array.h — rs_dev_array<T>: the one owner of a device array that only grows (the resident map's image, the fuse
// scratch, the two per-context tables).  It holds a pointer and a capacity that always agree, is move-only and frees
// itself: whoever destroys the owner has made the device current and drained the stream first.  Included from common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/rsgpu.h"

struct rs_context;
enum rs_grow_policy { RS_GROW_DOUBLE, RS_GROW_ROUND_UP };      // doubled from `first` | `need` rounded up to a multiple of `first`
// reserve()'s slow path (context.hip), untyped: entries of `elem` bytes
int rs_dev_array_grow(rs_context* ctx, void** p, size_t* cap, size_t elem, size_t need, size_t first, size_t keep_entries, rs_grow_policy policy);

template <typename T>
struct rs_dev_array {
    T* p = nullptr;
    size_t cap = 0;                     // entries

    rs_dev_array() = default;
    rs_dev_array(rs_dev_array&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    rs_dev_array& operator=(rs_dev_array&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~rs_dev_array() { if (p) (void)hipFree(p); }
    operator T*() const { return p; }

    // Room for `need` entries; one compare when there is room already.  Otherwise a fresh allocation of `first` entries or the
    // current capacity, doubled until it holds `need` (RS_GROW_ROUND_UP: `need` rounded up to a multiple of `first`).  The
    // context stream is synchronised before the old block is freed, and the first keep_entries entries move to the new one;
    // everything else in it is undefined: *grew is set (never cleared) so that the caller fills it.  When the allocation
    // fails (RS_ERR_NOMEM) the array is unchanged (keep_entries > 0) or empty.
    int reserve(rs_context* ctx, size_t need, size_t first, size_t keep_entries = 0, bool* grew = nullptr, rs_grow_policy policy = RS_GROW_DOUBLE)
    {
        if (need <= cap) return RS_OK;
        const int rc = rs_dev_array_grow(ctx, (void**)&p, &cap, sizeof(T), need, first, keep_entries, policy);
        if (grew && rc == RS_OK) *grew = true;
        return rc;
    }
};
