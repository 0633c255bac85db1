// Checks ria_amd/csrc/window_rules.hpp - the float32 CFO clamp and the consumed rule of ria_gpu_rx_window_batch - against the
// reference's statements written out another way (streaming_decoder.cpp:1414-1434, :1994-2013).  Plain C++: builds with g++,
// also under -fsanitize=address,undefined.  Prints "failures N".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../ria_amd/csrc/var_frames.hpp"
#include "../../ria_amd/csrc/window_rules.hpp"

static uint32_t word(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

// the reference's statements, in its own order
static float clamp_ref(float corrected_cfo, float current_cfo) {
    constexpr float MAX_PILOT_CFO_DRIFT_HZ = 2.0f;
    float drift = corrected_cfo - current_cfo;
    if (std::abs(drift) > MAX_PILOT_CFO_DRIFT_HZ) corrected_cfo = current_cfo + std::copysign(MAX_PILOT_CFO_DRIFT_HZ, drift);
    return corrected_cfo;
}

int main() {
    int failures = 0, checked = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float cur[] = {0.0f, -0.0f, 1.5f, -37.25f, 2.0f, 1e-30f, 12345.678f, inf, -inf, nan};
    const float est[] = {0.0f, -0.0f, 1.9999999f, 2.0f, 2.0000002f, -2.0f, -2.0000002f, 5.0f, -5.0f, 3.5f, -35.25f, -35.249996f, -39.25f,
                         -39.250004f, 1e30f, -1e30f, inf, -inf, nan, 12347.678f, 12347.679f};
    for (float c : cur)
        for (float e : est) {
            const float got = ria::win_clamp_cfo(e, c), want = clamp_ref(e, c);
            const bool same = word(got) == word(want) || (std::isnan(got) && std::isnan(want));
            if (!same) { ++failures; printf("clamp %g %g: %g != %g\n", e, c, got, want); }
            ++checked;
        }
    // exact landings and pass-through
    if (word(ria::win_clamp_cfo(5.0f, 0.0f)) != word(2.0f) || word(ria::win_clamp_cfo(-5.0f, 0.0f)) != word(-2.0f)) { ++failures; printf("landing\n"); }
    if (word(ria::win_clamp_cfo(2.0f, 0.0f)) != word(2.0f) || word(ria::win_clamp_cfo(-0.0f, 0.0f)) != word(-0.0f)) { ++failures; printf("pass\n"); }
    if (!std::isnan(ria::win_clamp_cfo(nan, 1.0f))) { ++failures; printf("nan\n"); }

    // consumed: getMinSamplesForCWCount is var_frame_samples of 81 bytes per codeword
    const int bps_set[] = {53, 106, 153, 159, 188, 212, 408, 424};
    const int types[] = {0x10, 0x11, 0x12, 0x13, 0x14, 0x15, 0x16, 0x17, 0x20, 0x21, 0x30, 0x31, 0x40, 0x00, 0xFF};
    for (int bps : bps_set) {
        for (int cw = 1; cw <= 4; ++cw) {
            if (ria::win_samples_for_cw(bps, cw) != ria::var_frame_samples(bps, 81 * cw)) { ++failures; printf("samples %d %d\n", bps, cw); }
            ++checked;
        }
        const int lens[] = {ria::var_frame_samples(bps, 81), ria::var_frame_samples(bps, 162), ria::var_frame_samples(bps, 324), 10368};
        for (int len : lens)
            for (int t : types)
                for (int success = 0; success <= 1; ++success)
                    for (int ok = 0; ok <= 4; ++ok)
                        for (int bad = 0; bad + ok <= 4; ++bad)
                            for (int nbytes : {0, 2, 3, 20}) {
                                const bool ctl = t == 0x10 || t == 0x11 || t == 0x16 || t == 0x17 || t == 0x20 || t == 0x21 || t == 0x15 || t == 0x40;
                                const bool con = t == 0x12 || t == 0x13 || t == 0x14;
                                int want = len;
                                if (success && nbytes >= 3 && (ctl || con) && ok + bad > 0) {
                                    const int exact = ria::var_frame_samples(bps, 81 * (ok + bad));
                                    if (exact < want) want = exact;
                                }
                                if (ria::win_consumed(len, success != 0, nbytes, t, ok, bad, bps) != want) { ++failures; printf("consumed %d %d %d\n", bps, len, t); }
                                ++checked;
                            }
    }
    printf("checked %d, failures %d\n", checked, failures);
    return failures ? 1 : 0;
}
