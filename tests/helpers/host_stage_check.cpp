// CPU check of ria_amd/csrc/host_stage.hpp (the StageCarver alone): g++ -std=c++17 host_stage_check.cpp && ./a.out
// A layout of two optional inputs behind a mandatory one and three optional outputs in front of a mandatory one, in every
// combination of present / wanted, at several sizes.  Prints "failures 0" when every property holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ria_amd/csrc/host_stage.hpp"

using ria::StageCarver;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

struct Odd { char c[7]; };   // a size that is no multiple of anything
struct Stage { float* x; Odd* meta; int32_t* count; float* llr; uint8_t* info; Odd* st; uint16_t* it; };
// the caller's own buffers; a null pointer is an input that is absent / an output that nobody reads
struct Host { const float* x; const Odd* meta; const int32_t* count; float* llr; uint8_t* info; Odd* st; uint16_t* it; };

static Stage carve(StageCarver& c, size_t n, const Host& h) {
    Stage w;
    w.x = c.in(n, h.x, n - n / 3);              // the tail of the area is zero padding
    w.meta = c.in(n, h.meta);
    w.count = c.in(1, h.count);
    w.llr = c.out(3 * n, h.llr, 2 * n);         // only the first 2 n are handed out
    w.info = c.out(n, h.info);
    w.st = c.out(n, h.st);
    w.it = c.out(n, h.it);
    return w;
}

int main() {
    for (size_t n : {size_t(1), size_t(3), size_t(64), size_t(255), size_t(256), size_t(257), size_t(1000)}) {
        std::vector<float> x(n), llr(3 * n);
        std::vector<Odd> meta(n), st(n);
        std::vector<uint8_t> info(n);
        std::vector<uint16_t> it(n);
        int32_t count = 77;
        for (size_t i = 0; i < n; ++i) { x[i] = 1.0f + i; std::memset(&meta[i], 0x5A, sizeof(Odd)); }
        for (int combo = 0; combo < 32; ++combo) {
            Host h{x.data(), (combo & 1) ? meta.data() : nullptr, (combo & 2) ? &count : nullptr, (combo & 4) ? llr.data() : nullptr,
                   (combo & 8) ? info.data() : nullptr, (combo & 16) ? st.data() : nullptr, it.data()};
            // 1. the size pass equals the placed pass
            StageCarver sizing;
            const Stage s0 = carve(sizing, n, h);
            const size_t total = sizing.size();
            CHECK(sizing.valid() && total % 256 == 0);
            char* block = static_cast<char*>(std::aligned_alloc(256, total));
            char* device = static_cast<char*>(std::aligned_alloc(256, total));   // stands for the device block
            CHECK(block != nullptr && device != nullptr);
            std::memset(block, 0xEE, total);
            std::memset(device, 0xDD, total);
            StageCarver placed(block);
            const Stage s1 = carve(placed, n, h);
            CHECK(placed.valid() && placed.size() == total && placed.upload_end() == sizing.upload_end() &&
                  placed.first_output() == sizing.first_output() && placed.download_begin() == sizing.download_begin());
            // 2. the layout does not depend on what is present or wanted: every area is 256-byte aligned, in order, disjoint
            const size_t off[8] = {0, ria::up256(n * 4), ria::up256(n * 4) + ria::up256(n * 7), 0, 0, 0, 0, 0};
            const size_t o_llr = off[2] + 256, o_info = o_llr + ria::up256(12 * n), o_st = o_info + ria::up256(n), o_it = o_st + ria::up256(7 * n);
            CHECK(total == o_it + ria::up256(2 * n));
            CHECK(reinterpret_cast<char*>(s1.x) == block && s0.x == nullptr);
            CHECK((s1.meta == nullptr) == !(combo & 1) && (!s1.meta || reinterpret_cast<char*>(s1.meta) == block + off[1]));
            CHECK((s1.count == nullptr) == !(combo & 2) && (!s1.count || reinterpret_cast<char*>(s1.count) == block + off[2]));
            CHECK(reinterpret_cast<char*>(s1.llr) == block + o_llr && reinterpret_cast<char*>(s1.info) == block + o_info);
            CHECK(reinterpret_cast<char*>(s1.st) == block + o_st && reinterpret_cast<char*>(s1.it) == block + o_it);
            // 3. the upload covers the present inputs, to the byte, and no output
            const size_t up = placed.upload_end();
            CHECK(up == ((combo & 2) ? off[2] + 4 : (combo & 1) ? off[1] + 7 * n : 4 * n));
            CHECK(up <= placed.first_output() && placed.first_output() == o_llr);
            // 4. the download starts at the first output that is wanted and ends with the block
            const size_t down = placed.download_begin();
            CHECK(down == ((combo & 4) ? o_llr : (combo & 8) ? o_info : (combo & 16) ? o_st : o_it));
            CHECK(down >= placed.first_output() && down < total);
            // 5. fill, the two copies and drain move what they should: the device block stands between them
            placed.fill();
            std::memcpy(device, block, up);
            for (size_t i = 0; i < n - n / 3; ++i) CHECK(reinterpret_cast<float*>(device)[i] == x[i]);
            for (size_t i = n - n / 3; i < n; ++i) CHECK(reinterpret_cast<float*>(device)[i] == 0.0f);
            if (combo & 1) CHECK(std::memcmp(device + off[1], meta.data(), 7 * n) == 0);
            if (combo & 2) CHECK(*reinterpret_cast<int32_t*>(device + off[2]) == 77);
            CHECK(static_cast<unsigned char>(device[o_llr]) == 0xDD);   // no output went up
            for (size_t b = o_llr; b < total; ++b) device[b] = static_cast<char>(b * 31 + combo);   // the batch form's results
            std::fill(llr.begin(), llr.end(), -1.0f);
            std::memset(info.data(), 0, n); std::memset(st.data(), 0, 7 * n); std::memset(it.data(), 0, 2 * n);
            std::memcpy(block + down, device + down, total - down);
            placed.drain();
            if (combo & 4) CHECK(std::memcmp(llr.data(), device + o_llr, 8 * n) == 0 && llr[2 * n] == -1.0f);   // 2 n handed out, no more
            if (combo & 8) CHECK(std::memcmp(info.data(), device + o_info, n) == 0);
            if (combo & 16) CHECK(std::memcmp(st.data(), device + o_st, 7 * n) == 0);
            CHECK(std::memcmp(it.data(), device + o_it, 2 * n) == 0);
            std::free(block);
            std::free(device);
        }
    }
    // an input behind an output, and more areas of a kind than are recorded, make the walk invalid
    {
        float f = 0; StageCarver c;
        (void)c.out(4, &f); (void)c.in(4, &f);
        CHECK(!c.valid());
        StageCarver many;
        for (int i = 0; i <= StageCarver::kMaxAreas; ++i) (void)many.in(1, &f);
        CHECK(!many.valid());
        StageCarver none;                                   // nothing present, nothing wanted: nothing is copied
        (void)none.in(4, static_cast<const float*>(nullptr)); (void)none.out(4, static_cast<float*>(nullptr));
        CHECK(none.valid() && none.upload_end() == 0 && none.download_begin() == none.size() && none.size() == 512);
    }
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
