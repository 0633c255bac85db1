// ria_amd/csrc/cfo_theta0.h — the CFO correction phase at a frame's first sample, from (cfo_hz, abs_position).
//
// OFDMChirpWaveform::process (ofdm_chirp_waveform.cpp:402-411) computes -2 pi cfo pos / 48000 in double, rounds it to
// float and wraps it into [-pi, pi] with `while (ip > pi) ip -= 2 pi` on that float.  The wrap is path dependent (every
// step rounds to float), so it is restated as the same loop, not as an fmod.
//
// The loop ends only while a step still changes the float: up to |ip| = 2^27 the spacing of floats is at most 8, and
// ip - 6.28.. rounds to a smaller float; above 2^27 the spacing is 16 or more and ip - 6.28.. rounds back to ip.  The
// reference never returns there, nor for an infinite ip.  This helper returns 0 instead whenever the rounded |ip| is
// above 2^27 or ip is not finite (NaN included, where the reference's loop would end with NaN); inside the bound it is
// the reference's loop bit for bit; every step moves ip by at least 6, so it takes fewer than 2^27 / 6 = 2.3e7 steps.
// As a limit on the metadata:
// |cfo_hz * abs_position| <= 2^27 * 48000 / (2 pi) = 1.025e12 Hz*samples (include/ria_gpu.h, ria_frame_meta).
// tests/test_cfo_theta0_host.py compiles this header for the host and checks it against the oracle's wrap.
#pragma once
#include "devmath.h"

namespace ria {

RIA_HD float cfo_theta0(float cfo_hz, uint64_t abs_position) {
    const double pi = 3.14159265358979323846;
    float ip = static_cast<float>(-2.0f * pi * static_cast<double>(cfo_hz) * static_cast<double>(abs_position) / 48000.0);
    if (!(ip >= -134217728.0f && ip <= 134217728.0f)) return 0.0f;
    while (static_cast<double>(ip) > pi) ip = static_cast<float>(static_cast<double>(ip) - 2.0f * pi);
    while (static_cast<double>(ip) < -pi) ip = static_cast<float>(static_cast<double>(ip) + 2.0f * pi);
    return ip;
}

}  // namespace ria
