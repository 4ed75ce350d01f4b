// lidf_carve.h — how every layout of caller-provided memory (workspaces, pack blobs, kept activations) is written:
// ONE function per layout takes its slots from a Carver, in order, and keeps the typed pointers. Run over NULL
// the function sizes the layout (every pointer NULL, used() the byte count); run over the caller's pointer it hands
// the slots out. Sizes and addresses therefore cannot disagree. Plain C++17, no HIP.
//   nested layout   the inner function takes from the same carver (or from Carver(c.take_bytes(n)) where the outer
//                   slot has a size of its own; from c.here(a) + c.take_bytes(inner.used()) at another alignment)
//   optional slot   take_if(on, ..): 0 bytes and NULL when off
//   union           either(a, b): both views start at the same byte, the slot is the larger
#pragma once
#include <stddef.h>

static inline bool lidf_covers(const void* p, size_t have, size_t need) { return p && have >= need; }

struct Carver {
    char* base;      // NULL: a sizing pass
    size_t align;    // every slot occupies a multiple of it (the layouts start aligned, so every slot is)
    size_t off = 0;
    explicit Carver(const void* b = nullptr, size_t a = 256) : base((char*)b), align(a) {}

    void* take_bytes(size_t bytes) {
        void* p = base ? base + off : nullptr;   // (no arithmetic on NULL)
        off += (bytes + align - 1) / align * align;
        return p;
    }
    template <class T> T* take(size_t count) { return (T*)take_bytes(count * sizeof(T)); }
    template <class T> T* take_if(bool on, size_t count) { return on ? take<T>(count) : nullptr; }
    // a carver of its own at the next byte (another alignment; account for it with take_bytes(inner.used()))
    Carver here(size_t a) const { return Carver(base ? base + off : nullptr, a); }
    template <class A, class B> void either(A a, B b) {
        const size_t start = off;
        a(*this);
        const size_t end_a = off;
        off = start;
        b(*this);
        if (end_a > off) off = end_a;
        off = (off + align - 1) / align * align;
    }
    size_t used() const { return off; }
    // does the caller's (ptr, bytes) hold what was carved?
    bool covers(const void* p, size_t bytes) const { return lidf_covers(p, bytes, off); }
};

// the size of a layout: its function run over NULL
template <class F> static inline size_t carved(F lay) {
    Carver c;
    lay(c);
    return c.used();
}
