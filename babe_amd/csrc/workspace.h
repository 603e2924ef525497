// Bump carver of a caller-owned workspace: the ONE statement of a workspace's layout.  An entry point runs its carve function on
// the caller's buffer; its babe_*_workspace_bytes runs the same function dry (base = nullptr: nothing but counting, every take
// returns nullptr) and returns `used`.  Plain C++, no HIP: a host-only program can include it (tests/test_workspace_cpu.py).
#pragma once
#include <cstddef>

struct Carver {
    char* base;         // nullptr: dry
    size_t cap;         // bytes the caller declared (not looked at dry)
    size_t granule;     // every piece starts on, and is rounded up to, a multiple of it: 256 bytes, or 4 for whole floats
    size_t used = 0;    // high-water mark: the bytes every take so far asked for, refused ones included
    bool ok = true;     // false once a piece did not fit; that take and every later one return nullptr
    template <typename T>
    T* take(size_t n) {
        const size_t at = (used + alignof(T) - 1) / alignof(T) * alignof(T);      // (a no-op unless granule < alignof(T))
        used = at + (n * sizeof(T) + granule - 1) / granule * granule;
        if (!base) return nullptr;
        if (used > cap) ok = false;
        return ok ? reinterpret_cast<T*>(base + at) : nullptr;
    }
};
