// tests/helpers/stream_rules_check.cpp — walks ria_amd/csrc/stream_rules.hpp over its domain and prints one line per case:
// the rule's name, its arguments, "->", its results; floats as their bit patterns in hex.  tests/test_stream_rules_host.py
// computes every line again in Python (tests/stream_restatement.py) and compares.  Built with g++ alone, once plain and once
// with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ria_amd/csrc/stream_rules.hpp"

using namespace ria;

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int32_t none = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    // the window length at capture_len - search_start = full - 1, full, full + 1 and 0 (and a whole capture)
    for (int full : {70000, 193480, 386040})
        for (int start : {0, 1, 4801, 500001})
            for (int left : {0, 1, full - 1, full, full + 1, 959999 - start})
                std::printf("window %d %d %d -> %d\n", full, start + left, start, stream_window_len(full, start + left, start));
    const std::vector<float> vals = {0.0f, 0.15f, 0.55f, 0.72f, 0.720001f, 1.0f, -1.0f, nan, inf, -inf};
    for (float a : vals)
        for (float b : vals) std::printf("conf %08x %08x -> %08x\n", bits(a), bits(b), bits(stream_min_confidence(a, b)));
    // last_decoded_sync: none, positions around the window, and both sides of the clip
    for (int32_t last : {none, none + 1, none + 2, -959999, -1, 0, 1, 4800, 500000, 959998, imax - 1, imax})
        for (int start : {0, 1, 4800, 500001, 959998})
            std::printf("rebase %d %d -> %d\n", last, start, stream_rebase_last_sync(last, start));
    // every window outcome of both families (one past each end too)
    for (int family : {kStreamOfdm, kStreamMcdpsk})
        for (int outcome = 0; outcome <= 7; ++outcome) {
            std::printf("moved %d %d -> %d\n", family, outcome, stream_moved(family, outcome) ? 1 : 0);
            for (int next_pos : {-1, 0, 1, 80000})
                for (int start : {0, 12345})
                    std::printf("cursor %d %d %d %d %d %d %d -> %d\n", family, outcome, next_pos, start, start + 9600, 36864, start + 14400,
                                stream_cursor(family, outcome, next_pos, start, start + 9600, 36864, start + 14400));
            // the close rule: max_events reached and not, a cursor at 959 998, 959 999 and 960 000
            for (int n_events : {1, 7, 8})
                for (int max_events : {1, 8})
                    for (int cursor : {0, 959998, 959999, 960000, 1000000}) {
                        if (n_events > max_events) continue;
                        std::printf("close %d %d %d %d %d -> %d\n", family, outcome, n_events, max_events, cursor,
                                    stream_close(family, outcome, n_events, max_events, cursor));
                    }
        }
    for (int family : {kStreamOfdm, kStreamMcdpsk})
        for (int delivered : {0, 1})
            for (int32_t state_last : {none, 0, 77777})
                for (int32_t window_last : {none, none + 1, -20000, -1, 0, 9600, imax})
                    for (int start : {0, 1, 500001})
                        std::printf("last %d %d %d %d %d %d -> %d\n", family, delivered, start + 9600, state_last, window_last, start,
                                    stream_last_sync(family, delivered != 0, start + 9600, state_last, window_last, start));
    // fed below and above the new cursor, and above capture_len
    for (int cap : {0, 100000, 959999})
        for (int fed : {0, 4800, 99999, 100000})
            for (int cursor : {0, 4799, 4800, 4801, 99999, 100000, 100001, 959999, 1100000}) {
                if (fed > cap) continue;
                std::printf("fed %d %d %d -> %d\n", fed, cap, cursor, stream_fed(fed, cap, cursor));
            }
    return 0;
}
