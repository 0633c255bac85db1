// tests/helpers/ring_rules_check.cpp — walks ria_amd/csrc/ring_rules.hpp case by case and prints one line per case: the rule's
// name, its arguments, "->", its results.  tests/test_ring_rules_host.py computes every line again in Python from the
// statements of streaming_decoder.cpp and compares.  Built with g++ alone, once plain and once with
// -fsanitize=address,undefined.  The record layouts of include/ria_gpu.h are asserted at compile time.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/ria_gpu.h"
#include "../../ria_amd/csrc/ring_rules.hpp"

using namespace ria;

static_assert(sizeof(ria_ring_state) == 48 && offsetof(ria_ring_state, total_fed) == 0 && offsetof(ria_ring_state, correlation_pos) == 8 &&
              offsetof(ria_ring_state, noise_floor) == 16 && offsetof(ria_ring_state, last_decoded_sync_pos) == 32 &&
              offsetof(ria_ring_state, overflow_events) == 36 && offsetof(ria_ring_state, overflow_dropped) == 40, "ria_ring_state");
static_assert(sizeof(ria_ring_search_result) == 144 && sizeof(ria_search_result) == 112 &&
              offsetof(ria_ring_search_result, abs_position) == offsetof(ria_search_result, abs_position) &&
              offsetof(ria_ring_search_result, root) == offsetof(ria_search_result, root) &&
              offsetof(ria_ring_search_result, reserved2) == offsetof(ria_search_result, reserved2) &&
              offsetof(ria_ring_search_result, abs_search_start) == 112 && offsetof(ria_ring_search_result, overflow_dropped) == 120 &&
              offsetof(ria_ring_search_result, overflows) == 128 && offsetof(ria_ring_search_result, span_wraps) == 140, "ria_ring_search_result");

int main() {
    const long long R = kSrchRing;
    const std::vector<long long> totals = {0, 1, 31119, 31120, 67304, 500000, R - 4801, R - 4800, R - 1, R, R + 1, R + 4800, R + 20000, R + 100000, 2 * R - 1, 2 * R,
                                           2 * R + 1, 2 * R + 140000, 3 * R, 1000 * R + 5, kRingMaxCapture};
    // the closed form: every total against ring indices around 0, the write position and the ring's end
    for (long long t : totals) {
        const int wp = ring_write_pos(t);
        for (int d = -3; d <= 3; ++d)
            for (long long base : {0LL, static_cast<long long>(wp), R / 2, R - 1}) {
                const int p = static_cast<int>(((base + d) % R + R) % R);
                std::printf("source %lld %d -> %lld %lld %d\n", t, p, ring_source(t, p), ring_pos_to_absolute(t, p), wp);
            }
    }
    // feedAudio: cursors behind, at and ahead of the write position; steps that fit, that reach 960 000 exactly, that overflow
    for (long long t : totals) {
        if (t == kRingMaxCapture) continue;
        const int wp = ring_write_pos(t);
        for (int off : {0, 1, 4800, 9599, 9600, 9601, 67304, 360000, 600000, 950399, 950400, 950401, 959999})
            for (int ahead = 0; ahead < 2; ++ahead)
                for (int step : {0, 1, 4800, 9600, 360000, 600000, 959999, 960000, 2000000})
                    for (long long room : {0LL, 100LL, 3000000LL}) {
                        const int cursor = static_cast<int>(((ahead ? wp + off : wp - off) % R + R) % R);
                        int c = cursor, s = 7;
                        long long f = t;
                        unsigned ev = 0xFFFFFFFEu;
                        unsigned long long total = 5;
                        RingFeedCounts fc{1u, 2u, 3ull};
                        const long long cap = t + room;
                        const long long n = ring_feed(&c, &f, &s, &ev, &total, &fc, cap, step);
                        std::printf("feed %d %lld 7 %lld %d -> %lld %d %lld %d %u %llu %u %u %llu\n", cursor, t, cap, step, n, c, f, s, ev, total, fc.overflows,
                                    fc.drift_snaps, fc.overflow_dropped);
                    }
    }
    // the waits with the cursor initialisation, the catch-up, the backtrack, the span flag
    for (int m : {31120, 67304, 120000})
        for (long long t : totals) {
            const int wp = ring_write_pos(t);
            for (int cursor : {0, 1, 5000, 9599, 9600, 19199, 19200, wp, (wp + 1) % kSrchRing, (wp + kSrchRing - 1) % kSrchRing, (wp + kSrchRing - m) % kSrchRing,
                               (wp + kSrchRing - m + 1) % kSrchRing, (wp + kSrchRing - m - 1) % kSrchRing, (wp + 3000) % kSrchRing, (wp + 9600) % kSrchRing,
                               (wp + 19200) % kSrchRing, 959999}) {
                int c = cursor;
                unsigned inits = 0;
                const bool w = ring_wait(&c, t, m, &inits);
                std::printf("wait %d %lld %d -> %d %d %u\n", cursor, t, m, w ? 1 : 0, c, inits);
                for (int zc = 0; zc < 2; ++zc) {
                    const int start = ring_search_start(cursor, t, zc != 0);
                    std::printf("start %d %lld %d %d -> %d %d\n", cursor, t, zc, m, start, ring_span_wraps(start, t, m) ? 1 : 0);
                }
            }
        }
    {
        const int m = 31120;
        for (int wp : {0, 20000, 35919, 35920, 35921, 500000, 959999})
            for (long long num : {10LL, 15LL, 16LL, 25LL, 26LL, 30LL, 300LL})
                for (int d : {-1, 0, 1}) {
                    const int unsearched = static_cast<int>((num * m + 9) / 10) + d;
                    if (unsearched >= kSrchRing) continue;
                    const int cursor = (wp + kSrchRing - unsearched) % kSrchRing;
                    int c = cursor;
                    const int k = ring_catch_up(&c, wp, m);
                    std::printf("catch %d %d %d -> %d %d\n", cursor, wp, m, k, c);
                }
    }
    // feedAudio's two overflow branches by name: need_to_drop == unsearched (count >= 360 000 on a backlog) and < unsearched
    {
        struct Case { int cursor; long long t; int step; } cases[] = {{100000, 200000, 900000}, {150000, R + 100000, 100000}};
        for (const Case& k : cases) {
            int c = k.cursor, s = 0;
            long long f = k.t;
            unsigned ev = 0;
            unsigned long long total = 0;
            RingFeedCounts fc{0u, 0u, 0ull};
            ring_feed(&c, &f, &s, &ev, &total, &fc, 3000000, k.step);
            std::printf("drop %d %lld %d -> %d %lld %u %llu\n", k.cursor, k.t, k.step, c, f, fc.overflows, fc.overflow_dropped);
        }
    }
    // the stream loop's direct total_fed assignment: the window call leaves the absolute cursor at most `full` behind span
    // sample 0, the search left the ring cursor `ahead` past it, and no feed ran between: backlog + arrivals < full
    for (int full : {98440, 169008, 959999})
        for (long long abs_start : {0LL, 5000LL, R - 50000, R + 12345, 2 * R + 700000})
            for (int ahead : {1200, 4800, 9600 + 4800, 19200 + 1200})
                for (long long lag : {0LL, 1LL, 31120LL, 120000LL, 900000LL})                // total_fed past the search's cursor
                    for (long long next : {0LL, 1LL, static_cast<long long>(ahead), static_cast<long long>(full) / 2, static_cast<long long>(full)}) {
                        const long long t = abs_start + ahead + lag, abs_cursor = abs_start + next;
                        long long unsearched, count;
                        const long long sum = ring_window_arrival(t, abs_start, ahead, abs_cursor, &unsearched, &count);
                        // the same arrivals as a feedAudio: did its overflow test fire?
                        int c = ring_mod(abs_start + ahead), s = 0;
                        long long f = t;
                        unsigned ev = 0;
                        unsigned long long total = 0;
                        RingFeedCounts fc{0u, 0u, 0ull};
                        if (count > 0 && count <= 2147483647LL) ring_feed(&c, &f, &s, &ev, &total, &fc, t + count, static_cast<int>(count));
                        std::printf("arrive %d %lld %d %lld %lld -> %lld %lld %lld %lld %u\n", full, abs_start, ahead, lag, next, unsearched, count, sum,
                                    ring_stream_fed(t, 4000000000LL, abs_cursor), fc.overflows);
                    }
    for (int last : {INT32_MIN, 0, 100, 479999, 480000, 480001, 959999})
        for (int start : {0, 50, 480000, 959999})
            for (int wl : {INT32_MIN, -500000, -1, 0, 150, 600000})
                std::printf("last %d %d %d -> %d %d %d\n", last, start, wl, ring_rebase_last_sync(last, start), ring_last_sync(kStreamMcdpsk, true, 7, last, wl, start),
                            ring_last_sync(kStreamOfdm, wl == 0, 7, last, wl, start));
    for (int start : {0, 1, 940696, 955400, 959999})
        for (int s : {0, 1, 4600, 4601, 19303, 19304, 119999}) std::printf("sync %d %d -> %d\n", start, s, ring_sync_position(start, s));
    return 0;
}
