// tests/helpers/mcdpsk_stream_rules_check.cpp — walks ria_amd/csrc/mcdpsk_stream_rules.hpp over its domain and prints one
// line per case: the rule's name, its arguments, "->", its result.  tests/test_mcdpsk_stream_cpu.py computes every line again
// in Python (tests/mcdpsk_stream_restatement.py) and compares.  Built with g++ alone, once plain and once with
// -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../ria_amd/csrc/mcdpsk_stream_rules.hpp"

using namespace ria;

int main() {
    // the audio clock: a clock at 0, in the middle and at the end of its range; a sync at sample 0, on both sides of the first
    // millisecond and at the capture's last sample
    for (uint64_t t0 : {UINT64_C(0), UINT64_C(1), UINT64_C(1) << 63, ~UINT64_C(0) - 19999, ~UINT64_C(0)})
        for (int sync : {0, 47, 48, 95, 96, 48000, 479999, 959998})
            std::printf("now %" PRIu64 " %d %d -> %" PRIu64 "\n", t0, sync, 48000, mcstream_now_ms(t0, sync, 48000));
    // the re-entry fit at equality, one sample short and one over; the window with need_samples below, at and above `full`
    for (int full : {70000, 100752})
        for (int start : {0, 14001})
            for (int sync_off : {0, 2512, 31119})
                for (int need : {0, 13312, full - sync_off - 1, full - sync_off, full - sync_off + 1, 400000}) {
                    const int sync = start + sync_off;
                    for (int cap : {sync + need - 1, sync + need, sync + need + 1, start + full - 1, start + full, start + full + 1, 959999}) {
                        if (cap <= sync || cap > 959999) continue;
                        const bool fits = mcstream_reentry_fits(cap, sync, need);
                        std::printf("fits %d %d %d -> %d\n", cap, sync, need, fits ? 1 : 0);
                        std::printf("window %d %d %d %d %d -> %d\n", full, cap, start, sync, need, mcstream_reentry_window_len(full, cap, start, sync, need));
                        if (fits)
                            for (int fed : {0, sync, sync + need - 1, sync + need, cap})
                                std::printf("fed %d %d %d -> %d\n", fed, sync, need, mcstream_reentry_fed(fed, sync, need));
                    }
                }
    // which window outcomes keep the wait: all seven RIA_MWIN_*, and one past each end
    for (int outcome = -1; outcome <= 7; ++outcome) std::printf("keeps %d -> %d\n", outcome, mcstream_keeps_pending(outcome) ? 1 : 0);
    // the pending fields' domain
    for (int pending : {-1, 0, 1, 3, 255, 256})
        for (int need : {-1, 0, 30720})
            for (int start : {-1, 0, 14001, 99999, 100000})
                for (int sync : {-1, 0, 16513, 99999, 100000})
                    for (int cap : {0, 45120, 100000})
                        std::printf("domain %d %d %d %d %d %d -> %d\n", pending, need, start, sync, cap, 31120,
                                    mcstream_pending_domain_ok(pending, need, start, sync, cap, 31120) ? 1 : 0);
    return 0;
}
