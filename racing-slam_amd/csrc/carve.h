// carve.h — rs_carve: the one way a block of memory is cut into typed pieces.  A layout is a function that takes an
// rs_carve& and assigns an object's pointers from take(): run on a null base it only sizes (every take returns null), run
// on the block it places.  Each piece's type and count so stand on one line, once.  Pieces start on 256-byte boundaries, in
// the order taken.  Plain C++: no HIP include, so the host tests build it with g++.  Users: rs_dev_block / rs_pin_block
// (dev_array.h), the per-call blocks of a solve (rs_carve_from, common.h; ba_blocks.h), the sub-workspaces of the BA solves.
#pragma once
#include <stddef.h>

static inline size_t rs_align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct rs_carve {
    char* base;
    size_t off = 0;

    explicit rs_carve(void* block = nullptr) : base((char*)block) {}
    template <typename T>
    T* take(size_t count)
    {
        T* p = base ? (T*)(base + off) : nullptr;
        off += rs_align256(sizeof(T) * count);
        return p;
    }
    size_t bytes() const { return off; }
};
