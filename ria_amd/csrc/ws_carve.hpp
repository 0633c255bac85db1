// ria_amd/csrc/ws_carve.hpp — typed areas of one workspace block.  Plain C++17, no HIP: tests/helpers/ws_carve_check.cpp
// builds it with g++.
//
// A workspace is described once, by a function that walks a Carver and returns a struct of typed pointers:
//     FooWs foo_carve(Carver& c, size_t n) { FooWs w; w.a = c.take<float>(n); w.b = c.take<uint8_t>(4 * n); return w; }
// Run on a null base it gives the size of the block (carved_size), run on the block it gives the pointers (carve_at):
// the type and the count of an area are written in one place.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ria {

inline size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

class Carver {
public:
    explicit Carver(void* base = nullptr) : base_(reinterpret_cast<uintptr_t>(base)) {}
    // `count` elements at the current offset; the next area starts on the next multiple of 256 bytes
    template <typename T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base_ + off_);
        off_ = up256(off_ + count * sizeof(T));
        return p;
    }
    // one area that holds n rows of several arrays back to back, in the order given (widest element first keeps each
    // array aligned for its type): n * (sizeof(Ts) + ...) bytes
    template <typename... Ts>
    void take_list(size_t n, Ts*&... arrays) {
        uintptr_t p = base_ + off_;
        ((arrays = reinterpret_cast<Ts*>(p), p += n * sizeof(Ts)), ...);
        off_ = up256(p - base_);
    }
    size_t offset() const { return off_; }   // bytes taken so far: the size of the block once the walk is done
private:
    uintptr_t base_;
    size_t off_ = 0;
};

template <class F>
size_t carved_size(F&& carve) { Carver c; carve(c); return c.offset(); }
template <class F>
auto carve_at(void* base, F&& carve) { Carver c(base); return carve(c); }
// bytes from area `from` up to area `to` of one block (a memset over neighbouring areas)
inline size_t span_bytes(const void* from, const void* to) { return static_cast<size_t>(static_cast<const char*>(to) - static_cast<const char*>(from)); }

}  // namespace ria
