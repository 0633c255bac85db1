// tests/helpers/search_rules_check.cpp — walks ria_amd/csrc/search_rules.hpp over its domain and prints one line per case:
// the rule's name, its arguments, "->", its results; floats as their bit patterns in hex.  tests/test_search_rules_host.py
// computes every line again in Python and compares.  Built with g++ alone, once plain and once with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ria_amd/csrc/search_rules.hpp"

using namespace ria;

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static float next(float f, int dir) { unsigned u = bits(f); u += dir; float r; std::memcpy(&r, &u, 4); return r; }   // positive floats

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const std::vector<float> special = {nan, inf, -inf, 0.0f, -0.0f};
    for (int mode = 0; mode < 3; ++mode) std::printf("min_search %d -> %d\n", mode, srch_min_search(mode));
    // feed: nothing left, a partial chunk, cursor ahead of / at / behind the write position
    for (int cap : {0, 4799, 4800, 100000})
        for (int fed : {0, 4800, 99999, 100000})
            for (int cursor : {0, 4799, 4800, 4801, 200000})
                for (int step : {0, 1, 4800}) {
                    if (fed > cap) continue;
                    int c = cursor, f = fed, s = 7;
                    const int n = srch_feed(&c, &f, &s, cap, step);
                    std::printf("feed %d %d 7 %d %d -> %d %d %d %d\n", cursor, fed, cap, step, n, c, f, s);
                }
    for (int min_search : {31120, 67304, 120000})
        for (int fed : {0, min_search - 1, min_search, min_search + 5000, 500000})
            for (int cursor : {0, 1, 4999, 5000, 5001, 600000})
                std::printf("wait %d %d %d -> %d\n", cursor, fed, min_search, srch_wait(cursor, fed, min_search) ? 1 : 0);
    // catch-up at 1.5x and 2.5x exactly and one either side (integer scaling: the boundary is scaled > 15 / > 25)
    {
        const int m = 31120;
        for (long long num : {10LL, 15LL, 16LL, 25LL, 26LL, 30LL})
            for (int d : {-1, 0, 1})
                for (int cursor : {0, 1000}) {
                    const int unsearched = static_cast<int>((num * m + 9) / 10) + d;   // the first count whose scaled value is num, and its neighbours
                    int c = cursor;
                    const int k = srch_catch_up(&c, cursor + unsearched, m);
                    std::printf("catch %d %d %d -> %d %d\n", cursor, cursor + unsearched, m, k, c);
                }
        for (int unsearched : {m * 3 / 2 - 1, m * 3 / 2, m * 3 / 2 + 1, m * 5 / 2 - 1, m * 5 / 2, m * 5 / 2 + 1, m + 48000 + 1, 900000}) {
            int c = 0;
            const int k = srch_catch_up(&c, unsearched, m);
            std::printf("catch %d %d %d -> %d %d\n", 0, unsearched, m, k, c);
        }
    }
    // tracker and gate: clamps at both ends, one ulp either side, NaN and infinities
    {
        std::vector<float> floors = {0.0005f, 0.001f, 0.002f, 0.01f, 0.03f, 1.0f};
        for (float lim : {0.015f / 2.2f, 0.040f / 2.2f, 0.014f / 1.8f, 0.030f / 1.8f}) { floors.push_back(next(lim, -1)); floors.push_back(lim); floors.push_back(next(lim, 1)); }
        for (float v : special) floors.push_back(v);
        std::vector<float> rmss = {0.0f, 0.001f, 0.0029f, 0.003f, 0.0031f, 0.02f, 0.5f, nan, inf};
        for (float fl : floors)
            for (float rms : rmss) {
                bool fast;
                const float n = srch_noise_floor(fl, rms, &fast);
                std::printf("floor %08x %08x -> %d %08x\n", bits(fl), bits(rms), fast ? 1 : 0, bits(n));
            }
        for (int light = 0; light < 2; ++light)
            for (float fl : floors)
                for (int streak = 0; streak <= 40; ++streak)
                    std::printf("gate %d %08x %d -> %08x\n", light, bits(fl), streak, bits(srch_gate(light != 0, fl, streak)));
    }
    for (int zc = 0; zc < 2; ++zc)
        for (int cursor : {0, 9599, 9600, 9601, 19199, 19200, 19201, 500000})
            std::printf("start %d %d -> %d %d\n", cursor, zc, srch_search_start(cursor, zc != 0), srch_step(zc != 0));
    // confidence tiers: every class, streaks 0..40, hints on both sides of each boundary
    {
        std::vector<float> fades = {0.0f, next(0.50f, -1), 0.50f, next(0.70f, -1), 0.70f, next(1.00f, -1), 1.00f, nan, inf, -inf};
        std::vector<float> snrs = {next(10.0f, -1), 10.0f, next(14.0f, -1), 14.0f, next(18.0f, -1), 18.0f, 0.0f, nan, inf, -inf};
        for (int cls = 0; cls < 4; ++cls)
            for (int connected = 0; connected < 2; ++connected)
                for (int streak = 0; streak <= 40; ++streak)
                    for (float fa : fades)
                        for (float sn : snrs) {
                            if (cls != 0 && !(fa == 0.0f && sn == 18.0f) && streak % 8) continue;   // the hints only move the differential class
                            float conf, fl;
                            srch_confidence(cls, connected != 0, streak, fa, sn, &conf, &fl);
                            std::printf("conf %d %d %d %08x %08x -> %08x %08x %08x\n", cls, connected, streak, bits(fa), bits(sn), bits(conf), bits(fl),
                                        bits(srch_detect_threshold(cls, conf)));
                        }
    }
    {
        std::vector<float> corrs = {0.0f, 0.19f, 0.20f, 0.29f, 0.30f, 0.31f, 0.55f, 0.62f, 0.63f, 0.64f, next(0.64f, 1), 0.70f, 0.71f, 0.72f, 0.77f, 0.78f, 0.82f, 0.85f, 0.89f, 0.90f, 1.0f, nan, inf, -inf};
        for (int streak : {0, 1, 5})
            for (float c : corrs)
                for (float fl : {0.20f, 0.30f, nan})
                    std::printf("near %d %08x %08x -> %d\n", streak, bits(c), bits(fl), srch_near_miss(streak, c, fl));
        for (int cls = 0; cls < 4; ++cls)
            for (int connected = 0; connected < 2; ++connected)
                for (int streak : {0, 2, 3, 4, 7, 40})
                    for (float c : corrs) {
                        float conf, fl;
                        srch_confidence(cls, true, 0, 0.0f, 20.0f, &conf, &fl);
                        std::printf("weak %d %d %d %08x %08x %08x -> %d %d %d\n", cls, connected, streak, bits(c), bits(conf), bits(fl),
                                    srch_weak_accept(cls, connected != 0, streak, c, conf, fl) ? 1 : 0, srch_streak_after_accept(streak, true),
                                    srch_streak_after_accept(streak, false));
                    }
    }
    for (int last : {INT32_MIN, 0, 5000, 959900})
        for (int d : {-201, -200, -199, -1, 0, 1, 199, 200, 201}) {
            const int base = last == INT32_MIN ? 5000 : last;
            const int sync = ((base + d) % kSrchRing + kSrchRing) % kSrchRing;
            std::printf("replay %d %d -> %d %d\n", sync, last, srch_replay(sync, last) ? 1 : 0, srch_replay_cursor(sync));
        }
    {
        std::vector<float> knowns = {0.0f, 0.01f, -0.01f, next(0.01f, 1), -next(0.01f, 1), 5.0f, -5.0f, nan, inf, -inf};
        std::vector<float> diffs = {0.0f, 1.0f, -1.0f, next(1.0f, 1), -next(1.0f, 1), 0.5f, 3.0f, nan, inf, -inf};
        for (int connected = 0; connected < 2; ++connected)
            for (float k : knowns)
                for (float d : diffs) {
                    const float nw = k + d;
                    bool taken;
                    const float r = srch_cfo_sanity(connected != 0, nw, k, &taken);
                    std::printf("cfo %d %08x %08x -> %d %08x\n", connected, bits(nw), bits(k), taken ? 1 : 0, bits(r));
                }
    }
    for (float c : {-1.0f, 0.0f, 0.15f, 0.3f, 0.5f, 1.0f, 1.05f, 1.06f, 2.0f, nan, inf, -inf}) std::printf("snr %08x -> %08x\n", bits(c), bits(srch_snr(c)));
    return 0;
}
