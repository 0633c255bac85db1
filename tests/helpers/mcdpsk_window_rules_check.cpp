// tests/helpers/mcdpsk_window_rules_check.cpp — host program for ria_amd/csrc/mcdpsk_window_rules.hpp: walks the rules'
// whole scalar domain (every pending count, header type and total_cw, the window edges, INT32 extremes, NaN / Inf rms values)
// and compares them with the reference's statements written out as the loop of passes decodeCurrentFrame() makes.  Built plain
// and with -fsanitize=address,undefined by tests/test_mcdpsk_window_cpu.py; prints "failures N".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../../ria_amd/csrc/mcdpsk_window_rules.hpp"

using namespace ria;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (++failures <= 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

// the reference's passes from pending_total_cw_ = pending on (:989-991, :1081-1082, :1611-1624), one turn per pass
static MwinStep passes_by_loop(const MwinGeom& g, int sync_start, int pending) {
    MwinStep st{kMwinOpen, 0, pending, 0, 0, 0};
    for (int turn = 0; turn < 4; ++turn) {
        const long long frame_len = 4608 + static_cast<long long>(pending) * g.cw_samples;
        st.pending = pending;
        if (sync_start + frame_len > g.window_len) { st.outcome = kMwinNeedSamples; st.need_samples = static_cast<int>(frame_len); return st; }
        if (pending > g.max_level) { st.outcome = kMwinTooLong; return st; }
        ++st.passes;
        const long long n_llr = static_cast<long long>(pending) * g.cw_bits;
        const int avail_cw = static_cast<int>(n_llr / 648);
        if (g.disconnected) {
            const int min_handshake_cw = 3;
            if (avail_cw < min_handshake_cw && pending < min_handshake_cw) { pending = min_handshake_cw; st.peek |= kMpeekHandshakeWindow; continue; }
        }
        st.level = pending;
        return st;
    }
    st.outcome = -1;     // more than three passes: never
    return st;
}

int main() {
    // anti-replay
    CHECK(!mwin_replay(0, INT32_MIN) && !mwin_replay(INT32_MAX, INT32_MIN) && !mwin_replay(INT32_MIN, INT32_MIN));
    CHECK(mwin_replay(1000, 1000) && mwin_replay(1000, 801) && !mwin_replay(1000, 800) && mwin_replay(1000, 1199) && !mwin_replay(1000, 1200));
    CHECK(!mwin_replay(INT32_MAX, INT32_MIN + 1) && !mwin_replay(0, INT32_MAX) && mwin_replay(INT32_MAX, INT32_MAX - 199));
    for (int last = -300; last <= 300; ++last) CHECK(mwin_replay(0, last) == (std::abs(last) < 200));

    // the PING ratio
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(mwin_is_ping(0.0f, 0.0f) && mwin_is_ping(0.001f, 5.0f) && mwin_is_ping(0.0f, inf));      // training_rms <= 0.001: ratio 0
    CHECK(mwin_is_ping(nan, 1.0f) && mwin_is_ping(inf, 1.0f) && !mwin_is_ping(1.0f, nan) && !mwin_is_ping(1.0f, inf) && !mwin_is_ping(inf, inf));
    CHECK(mwin_is_ping(0.5f, 0.29999998f) && !mwin_is_ping(0.5f, 0.3f) && !mwin_is_ping(0.5f, 0.30000004f));
    CHECK(mwin_is_ping(1.0f, std::nextafterf(0.6f, 0.0f)) && !mwin_is_ping(1.0f, 0.6f));

    // the escalation chain against the loop of passes, over every pending count, the window edges and both modes
    for (int disconnected = 0; disconnected < 2; ++disconnected)
        for (int geom = 0; geom < 4; ++geom) {
            // 10 carriers DBPSK, 10 carriers DQPSK, 20 carriers DQPSK, 10 carriers DBPSK at 4x spreading
            const int cw_samples[4] = {65 * 512, 33 * 512, 17 * 512, 65 * 512 * 4}, cw_bits[4] = {650, 660, 680, 650};
            for (int max_level = 2; max_level <= 8; max_level += 3)
                for (int pending = 1; pending <= 255; ++pending) {
                    MwinGeom g{0, cw_samples[geom], cw_bits[geom], disconnected, max_level};
                    const long long len = mwin_frame_len(g, pending), len3 = mwin_frame_len(g, 3);
                    const long long edges[6] = {len - 1, len, len + 1, len3 - 1, len3, 40000000};
                    for (long long wl : edges) {
                        if (wl > INT32_MAX) continue;
                        g.window_len = static_cast<int>(wl);
                        for (int sync : {0, 1, 2000}) {
                            const MwinStep a = mwin_escalate(g, sync, pending), b = passes_by_loop(g, sync, pending);
                            CHECK(a.outcome == b.outcome && a.level == b.level && a.pending == b.pending && a.need_samples == b.need_samples &&
                                  a.passes == b.passes && a.peek == b.peek);
                            if (a.outcome == kMwinOpen) CHECK(a.level >= pending && a.level <= max_level && sync + mwin_frame_len(g, a.level) <= wl &&
                                                              (!disconnected || a.level >= 3));
                        }
                    }
                }
        }
    // INT32 extremes of the sync position and the window: no overflow
    {
        MwinGeom g{INT32_MAX, 65 * 512 * 4, 650, 1, 8};
        const MwinStep a = mwin_escalate(g, INT32_MAX - 10, 255);
        CHECK(a.outcome == kMwinNeedSamples && a.pending == 255 && a.need_samples == 4608 + 255 * 65 * 512 * 4);
        CHECK(mwin_escalate(g, 0, 255).outcome == kMwinTooLong);
    }

    // the peek: every header the CW0 decode can give, at the soft-bit counts of a pass 0
    for (int disconnected = 0; disconnected < 2; ++disconnected)
        for (int n_llr : {1, 20, 647, 648, 650, 660, 680, 1295, 1296, 1944, 2000})
            for (int have = 0; have < 2; ++have)
                for (int valid = 0; valid < 2; ++valid)
                    for (int type = 0; type < 256; ++type)
                        for (int total = 0; total < 256; ++total) {
                            int peek = -1;
                            const int pending = mwin_peek(disconnected, n_llr, have != 0, valid != 0, type, total, &peek);
                            const int avail = n_llr / 648, what = peek & kMpeekWhatMask;
                            // the statements in the reference's order
                            int want = 0, want_what = kMpeekNone, want_bits = 0;
                            bool decided = false;
                            if (n_llr >= 648) {
                                const int min_hs = disconnected ? 3 : 0;
                                want_what = kMpeekNoHeader;
                                if (have && valid) {
                                    int needed = total;
                                    want_what = kMpeekHeaderSingle;
                                    if ((type == 0x12 || type == 0x13 || type == 0x14) && min_hs > 0 && needed < min_hs) { needed = min_hs; want_what = kMpeekConnectForced; }
                                    if (needed > 1 && avail < needed) { want = needed; decided = true; if (want_what != kMpeekConnectForced) want_what = kMpeekHeaderMulti; }
                                }
                                if (!decided && min_hs > 1 && avail < min_hs) { want = min_hs; want_bits = kMpeekHandshakeFallback; decided = true; }
                            }
                            if (!decided && disconnected && n_llr < 648) { want = 1; want_bits = kMpeekEarlyWindow; decided = true; }
                            if (!decided && disconnected && avail < 3) { want = 3; want_bits = kMpeekHandshakeWindow; decided = true; }
                            CHECK(pending == want && what == want_what && (peek & ~kMpeekWhatMask) == want_bits);
                            CHECK(pending == 0 || pending > avail || (n_llr < 648 && pending == 1));
                        }
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
