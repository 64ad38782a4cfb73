// dev_array.h — rs_dev_array<T>: the one owner of a device array that only grows (the resident map's image, the fuse
// scratch, the two per-context tables).  It holds a pointer and a capacity that always agree, is move-only and frees
// itself: whoever destroys the owner has made the device current and drained the stream first.  Included from common.h.
// rs_dev_block / rs_pin_block: the one owner of a block of fixed size, device or pinned host memory, under the same rule; an
// object of fixed capacity has one of each at most and cuts it into its arrays with a layout (carve.h).  (Per-call
// blocks from the context's workspace and pinned buffer are cut the same way through rs_carve_from, common.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/rsgpu.h"
#include "carve.h"

struct rs_context;
int rs_fail(rs_context* ctx, int code, const char* fmt, ...);
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

template <bool PINNED>
struct rs_block {
    void* p = nullptr;
    size_t bytes = 0;
    rs_block() = default;
    rs_block(rs_block&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    rs_block& operator=(rs_block&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~rs_block() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); }

    // An empty owner takes a block of n bytes.  A failure leaves it empty and HIP's last error clear, so that the next launch
    // check does not report this one.
    int alloc(rs_context* ctx, size_t n, const char* what)
    {
        if ((PINNED ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n)) == hipSuccess) { bytes = n; return RS_OK; }
        p = nullptr;
        (void)hipGetLastError();
        return rs_fail(ctx, RS_ERR_NOMEM, "%s of %zu bytes", what, n);
    }
    // size, allocate, place: layout(rs_carve&) runs on a null carver, then on the new block
    template <class L>
    int carve(rs_context* ctx, const char* what, L&& layout)
    {
        rs_carve size;
        layout(size);
        if (const int rc = alloc(ctx, size.bytes(), what)) return rc;
        rs_carve place(p);
        layout(place);
        return RS_OK;
    }
};
using rs_dev_block = rs_block<false>;
using rs_pin_block = rs_block<true>;
