// carve.h — a cursor that cuts one buffer into typed arrays, each starting on a
// 256-byte boundary.  A layout is written once, as a function of a Carve: run
// over a null base it yields the byte total to allocate (every take returns
// null), run over the buffer it yields the pointers, so the two cannot disagree.
// No HIP here: tests/native/carve_check.cpp compiles it for the host.
#pragma once
#include <stddef.h>

namespace livo {

struct Carve {
    char* base;  // null: the sizing pass
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t total() const { return (off + 255) & ~(size_t)255; }  // (the last array padded like the others)
};

}  // namespace livo
