// Bump allocator over a caller-owned workspace.  Every solver workspace is laid out by ONE function that carves a struct of typed
// pointers (plus `bytes`) through a Carve: the exported *_workspace_bytes function is that layout called with ws == NULL (sizes only,
// every pointer NULL), the entry point calls it with the caller's pointer and checks workspace_bytes >= layout.bytes from the same call.
// A layout lists its takes in the order of its struct's members (a braced list is evaluated left to right).
#pragma once
#include <stddef.h>
#include <stdint.h>

struct Carve {
    char *raw, *w;           // the caller's pointer (NULL: sizes only) and the aligned base
    size_t granule, slack, off = 0;
    // granule: every buffer's size is rounded up to it; base_align: the caller's pointer is rounded up to it, and bytes() counts that much
    // on top (1: carve from the pointer as it is).  Carve(ws): every buffer starts on 256 bytes
    explicit Carve(void* ws, size_t granule = 256, size_t base_align = 256)
        : raw(static_cast<char*>(ws)), w(reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + base_align - 1) / base_align * base_align)),
          granule(granule), slack(base_align > 1 ? base_align : 0) {}
    static Carve packed(void* ws) { return Carve(ws, 1, 1); }      // back to back from the caller's pointer as it is
    template <class T> T* take(size_t n) {
        T* p = raw ? reinterpret_cast<T*>(w + off) : nullptr;
        off += (n * sizeof(T) + granule - 1) / granule * granule;
        return p;
    }
    size_t bytes() const { return off + slack; }
    void* end() const { return raw ? raw + bytes() : nullptr; }    // bytes() past the caller's pointer: where a part sized on top of this one starts
};
