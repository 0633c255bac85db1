// tests/helpers/mcdpsk_ring_rules_check.cpp — walks ria_amd/csrc/mcdpsk_ring_rules.hpp over its domain and prints one line
// per case: the rule's name, its arguments, "->", its results.  tests/test_mcdpsk_ring_rules_host.py computes every line again
// in Python (tests/mcdpsk_ring_restatement.py) and compares.  Built with g++ alone, once plain and once with
// -fsanitize=address,undefined.  The record layout of include/ria_gpu.h is asserted at compile time.
#include <cinttypes>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../include/ria_gpu.h"
#include "../../ria_amd/csrc/mcdpsk_ring_rules.hpp"

using namespace ria;

static_assert(sizeof(ria_mcdpsk_ring_state) == 80 && offsetof(ria_mcdpsk_ring_state, ring) == 0 && offsetof(ria_mcdpsk_ring_state, pending_total_cw) == 48 &&
              offsetof(ria_mcdpsk_ring_state, need_samples) == 52 && offsetof(ria_mcdpsk_ring_state, pend_search_start) == 56 &&
              offsetof(ria_mcdpsk_ring_state, pend_sync_position) == 60 && offsetof(ria_mcdpsk_ring_state, pend_known_cfo_hz) == 64 &&
              offsetof(ria_mcdpsk_ring_state, pend_correlation) == 76, "ria_mcdpsk_ring_state");
static_assert(kMcRingMaxSpan == 959999, "the longest span a stream waits for");

int main() {
    const long long R = kSrchRing;
    // the audio clock on absolute positions: both sides of every lap, the capture domain's last index, a clock that wraps
    for (uint64_t t0 : {UINT64_C(0), UINT64_C(1), UINT64_C(1) << 63, ~UINT64_C(0) - 19999, ~UINT64_C(0) - 20000, ~UINT64_C(0)})
        for (long long pos : {0LL, 47LL, 48LL, R - 2, R - 1, R, R + 47, R + 48, 2 * R - 1, 2 * R, 1000 * R + 5, kRingMaxCapture - 1})
            std::printf("now %" PRIu64 " %lld %d -> %" PRIu64 "\n", t0, pos, 48000, mcring_now_ms(t0, pos, 48000));
    // the pending fields' domain: every clause on both sides of its bound, before, across and behind the wrap
    const int m = 31120;
    for (int pending : {-1, 0, 3, 255, 256})
        for (long long start : {-1LL, 0LL, 14001LL, R - 40000, R - 1, R, R + 300000, 3 * R + 17})
            for (int sync_off : {0, 21712})
                for (int need : {-1, 0, 56832, 959999 - 21712, 959999 - 21712 + 1, 959999, 960000})
                    for (long long fed_off : {-1LL, 0LL, 40000LL, R - m, R - m + 1})            // total_fed - (start + search_len)
                        for (long long cap_off : {0LL, 1LL, 100000LL}) {                        // capture_len - max(total_fed, 1)
                            const long long sync = start + sync_off, fed = start + m + fed_off;
                            if (fed < 0) continue;
                            const long long cap = (fed > 0 ? fed : 1) + cap_off;
                            if (cap > kRingMaxCapture || sync > 2147483647LL) continue;
                            std::printf("domain %d %d %lld %lld %lld %d %lld -> %d\n", pending, need, start, sync, cap, m, fed,
                                        mcring_pending_domain_ok(pending, need, static_cast<int>(start), static_cast<int>(sync), static_cast<int>(cap), m, fed) ? 1 : 0);
                        }
    // the re-entry: fit at equality and a sample short, the window's length with the span below, at and above `full`, and the
    // two assignments of total_fed with the bound of backlog plus arrivals, for spans up to 959 999
    for (int full : {100752, 959999})
        for (long long start : {0LL, 14001LL, R - 40000, R - 1, R + 300000})
            for (int ahead : {1, 1200, 19200 + 1200})
                for (int sync_off : {0, 21712})
                    for (long long span : {static_cast<long long>(sync_off), 56832LL, static_cast<long long>(full) - 1, static_cast<long long>(full),
                                           static_cast<long long>(full) + 1, 959999LL}) {
                        if (span < sync_off || span > kMcRingMaxSpan) continue;
                        const int need = static_cast<int>(span - sync_off);
                        const long long sync = start + sync_off;
                        for (long long cap : {sync + need - 1, sync + need, sync + need + 5000, start + full, start + 2 * R}) {
                            if (cap <= sync || cap < start + m) continue;
                            const bool fits = mcstream_reentry_fits(static_cast<int>(cap), static_cast<int>(sync), need);
                            std::printf("fits %lld %lld %d -> %d\n", cap, sync, need, fits ? 1 : 0);
                            if (!fits) continue;
                            const int wl = mcstream_reentry_window_len(full, static_cast<int>(cap), static_cast<int>(start), static_cast<int>(sync), need);
                            std::printf("window %d %lld %lld %lld %d -> %d\n", full, cap, start, sync, need, wl);
                            // total_fed when the stream comes back: from the search span's end to one ring behind the window's start
                            for (long long fed : {start + m, start + m + 4800, sync + need - 1, sync + need, start + R}) {
                                if (fed < start + m || fed > cap || fed - start > R || fed < start + ahead) continue;
                                std::printf("fed %lld %lld %d -> %lld\n", fed, sync, need, mcring_reentry_fed(fed, static_cast<int>(sync), need));
                                for (long long next : {-1LL, 0LL, static_cast<long long>(sync_off) + need, static_cast<long long>(wl)}) {
                                    long long after;
                                    const long long sum = mcring_reentry_arrival(fed, static_cast<int>(start), static_cast<int>(sync), need, ahead, cap,
                                                                                 next < 0 ? -1 : start + next, &after);
                                    std::printf("arrive %lld %lld %lld %d %d %lld %lld -> %lld %lld %d\n", fed, start, sync, need, ahead, cap, next, sum, after,
                                                sum < R ? 1 : 0);
                                }
                            }
                        }
                    }
    return 0;
}
