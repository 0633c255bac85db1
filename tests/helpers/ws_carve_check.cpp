// CPU check of ria_amd/csrc/ws_carve.hpp (the Carver alone): g++ -std=c++17 ws_carve_check.cpp && ./a.out
// Prints "failures 0" when every property holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ria_gpu.h"
#include "../../ria_amd/csrc/ws_carve.hpp"

using ria::Carver;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

struct Area { size_t off, bytes; };
struct Odd { char c[7]; };   // a size that is no multiple of anything

static size_t offset_of(const void* p, const char* base) { return reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(base); }
// A walk with every kind of call; records each area as (offset from base, bytes used).
template <typename T>
static void take(Carver& c, const char* base, size_t count, std::vector<Area>& out) {
    T* p = c.take<T>(count);
    out.push_back({offset_of(p, base), count * sizeof(T)});
}
static std::vector<Area> walk(Carver& c, const char* base, size_t n) {
    std::vector<Area> a;
    take<float>(c, base, n, a);
    take<uint8_t>(c, base, n, a);                 // n bytes: ends off a boundary unless n is a multiple of 256
    take<Odd>(c, base, n, a);
    take<double>(c, base, 0, a);                  // zero count
    uint64_t* o; ria_frame_meta* m; uint32_t* w; uint8_t* s;
    c.take_list(n, o, m, w, s);
    a.push_back({offset_of(o, base), n * (sizeof(uint64_t) + sizeof(ria_frame_meta) + sizeof(uint32_t) + 1)});
    take<uint16_t>(c, base, 3 * n, a);
    take<uint32_t>(c, base, 1, a);
    return a;
}

int main() {
    CHECK(ria::up256(0) == 0 && ria::up256(1) == 256 && ria::up256(256) == 256 && ria::up256(257) == 512);
    for (size_t n : {size_t(1), size_t(2), size_t(63), size_t(64), size_t(255), size_t(256), size_t(257), size_t(1000)}) {
        // 1. the null-base pass and the real-base pass give the same offsets and the same total
        Carver sizing;
        const std::vector<Area> a0 = walk(sizing, nullptr, n);
        const size_t total = sizing.offset();
        char* block = static_cast<char*>(std::aligned_alloc(256, total));   // total is a multiple of 256
        CHECK(block != nullptr && total % 256 == 0);
        Carver real(block);
        const std::vector<Area> a1 = walk(real, block, n);
        CHECK(real.offset() == total && a0.size() == a1.size());
        for (size_t i = 0; i < a0.size(); ++i) CHECK(a0[i].off == a1[i].off && a0[i].bytes == a1[i].bytes);
        CHECK(ria::carved_size([&](Carver& c) { return walk(c, nullptr, n); }) == total);
        // 2. every area starts on a 256-byte boundary; 3. areas are disjoint, in call order, inside the block
        size_t end = 0;
        for (const Area& a : a1) {
            CHECK(a.off % 256 == 0 && reinterpret_cast<uintptr_t>(block + a.off) % 256 == 0);
            CHECK(a.off >= end);
            CHECK(a.off == ria::up256(end));          // no hole larger than the alignment asks for
            end = a.off + a.bytes;
        }
        CHECK(end <= total && total == ria::up256(end));
        // each area filled with its own byte keeps it: nothing overlaps (and a sanitizer build sees every write in bounds)
        for (size_t i = 0; i < a1.size(); ++i) std::memset(block + a1[i].off, static_cast<int>(i + 1), a1[i].bytes);
        for (size_t i = 0; i < a1.size(); ++i)
            for (size_t b = 0; b < a1[i].bytes; ++b) if (block[a1[i].off + b] != static_cast<char>(i + 1)) { CHECK(!"area overwritten"); break; }
        // 4. a zero-count take consumes nothing and yields a usable pointer (never dereferenced): the next area starts there
        CHECK(a1[3].bytes == 0 && a1[3].off == a1[4].off);
        {
            Carver c(block);
            (void)c.take<float>(1);
            const size_t before = c.offset();
            double* z = c.take<double>(0);
            CHECK(c.offset() == before && reinterpret_cast<char*>(z) == block + before);
            Carver e;                                          // an empty walk has size 0
            CHECK(e.take<int>(0) == nullptr && e.offset() == 0);
        }
        // 5. take_list: the arrays lie back to back in the order given, the rows add up to the per-row byte sum
        {
            Carver c(block);
            (void)c.take<uint8_t>(5);
            const size_t at = c.offset();
            uint64_t* o; ria_frame_meta* m; uint32_t* w; uint8_t* s;
            c.take_list(n, o, m, w, s);
            const size_t row = sizeof(uint64_t) + sizeof(ria_frame_meta) + sizeof(uint32_t) + 1;
            CHECK(reinterpret_cast<char*>(o) == block + at);
            CHECK(reinterpret_cast<char*>(m) == block + at + n * sizeof(uint64_t));
            CHECK(reinterpret_cast<char*>(w) == block + at + n * (sizeof(uint64_t) + sizeof(ria_frame_meta)));
            CHECK(reinterpret_cast<char*>(s) == block + at + n * (sizeof(uint64_t) + sizeof(ria_frame_meta) + sizeof(uint32_t)));
            CHECK(c.offset() == ria::up256(at + n * row));
            CHECK(reinterpret_cast<uintptr_t>(m) % alignof(ria_frame_meta) == 0 && reinterpret_cast<uintptr_t>(w) % alignof(uint32_t) == 0);
            // the five arrays of an MC-DPSK list: 8 + 4 + 4 + 1 + 1 bytes per row
            float* f; uint8_t* b;
            const size_t at2 = c.offset();
            c.take_list(n, o, f, w, s, b);
            CHECK(b == s + n && reinterpret_cast<char*>(s) == block + at2 + n * 16 && c.offset() == ria::up256(at2 + n * 18));
        }
        CHECK(ria::span_bytes(block + a1[1].off, block + a1[4].off) == a1[4].off - a1[1].off);
        std::free(block);
    }
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
