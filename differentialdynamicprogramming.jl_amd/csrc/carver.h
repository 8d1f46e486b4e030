// carver.h — one device block handed out in 256-byte-aligned pieces (the backward-pass dispatcher tests the alignment of its operands).
// A layout is written once, as a function of a Carver: run from address 0 it measures the block, run from the block's base it places the
// pieces.  Plain host code: a layout can be run without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct Carver {
    uintptr_t p;
    explicit Carver(void *base = nullptr) : p((uintptr_t)base) {}
    template <class T> T *take(size_t count) { T *r = (T *)p; p += (count * sizeof(T) + 255) & ~(size_t)255; return r; }
    template <class T> T *take_if(bool want, size_t count) { return want ? take<T>(count) : nullptr; }
};
