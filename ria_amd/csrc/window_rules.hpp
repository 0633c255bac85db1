// ria_amd/csrc/window_rules.hpp — the two scalar rules of ria_gpu_rx_window_batch that the device and the host share.
// Plain C++17, no HIP needed: tests/helpers/window_rules_check.cpp builds it with g++.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RIA_WIN_HD __host__ __device__ inline
#else
#define RIA_WIN_HD inline
#endif

namespace ria {

// The pilot CFO feedback (streaming_decoder.cpp:1414-1434, :1922-1931): estimatedCFO() replaces last_cfo_, moved by at most
// 2 Hz; a NaN drift leaves the estimate as it is (std::abs(NaN) > 2 is false).  All in float32.
RIA_WIN_HD float win_clamp_cfo(float estimated, float current) {
    const float drift = estimated - current;
    if (fabsf(drift) > 2.0f) return current + copysignf(2.0f, drift);
    return estimated;
}

// Consumed samples (:1994-2013): frame_len, or for a successful control / connect frame at most the exact size of its
// codewords; samples_per_cw(k) = getMinSamplesForCWCount(k).  bits_per_symbol > 0.
RIA_WIN_HD int win_samples_for_cw(int bits_per_symbol, int cw) {
    return (2 + (648 * cw + bits_per_symbol - 1) / bits_per_symbol) * 1152;
}
RIA_WIN_HD bool win_is_non_data(int type) {     // isControlFrame || isConnectFrame (frame_v2.hpp:222-228, :348-351)
    return type == 0x10 || type == 0x11 || type == 0x16 || type == 0x17 || type == 0x20 || type == 0x21 || type == 0x15 ||
           type == 0x40 || type == 0x12 || type == 0x13 || type == 0x14;
}
RIA_WIN_HD int win_consumed(int frame_len, bool success, int frame_bytes, int type, int cw_ok, int cw_failed, int bits_per_symbol) {
    int consumed = frame_len;
    if (success && frame_bytes >= 3 && win_is_non_data(type)) {
        const int actual = cw_ok + cw_failed;
        if (actual > 0) {
            const int exact = win_samples_for_cw(bits_per_symbol, actual);
            if (exact < consumed) consumed = exact;
        }
    }
    return consumed;
}

}  // namespace ria
