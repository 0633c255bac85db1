// ria_amd/csrc/mcdpsk_window_rules.hpp — the scalar rules of ria_gpu_mcdpsk_window_batch that the device and the host share:
// the anti-replay test, the PING ratio, the CW0-peek decision and the escalation chain of StreamingDecoder::decodeCurrentFrame
// for MC-DPSK (src/gui/modem/streaming_decoder.cpp).  Plain C++17, no HIP needed: tests/helpers/mcdpsk_window_rules_check.cpp
// builds it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RIA_MWIN_HD __host__ __device__ inline
#else
#define RIA_MWIN_HD inline
#endif

namespace ria {

// mirrors of include/ria_gpu.h (RIA_MWIN_*, RIA_MPEEK_*); kMwinOpen is internal: the window still has a pass to run
constexpr int kMwinNotAccepted = 0, kMwinReplay = 1, kMwinPing = 2, kMwinProcessFailed = 3, kMwinDecoded = 4, kMwinNeedSamples = 5,
              kMwinTooLong = 6, kMwinOpen = 255;
constexpr int kMpeekNone = 0, kMpeekNoHeader = 1, kMpeekHeaderSingle = 2, kMpeekHeaderMulti = 3, kMpeekConnectForced = 4, kMpeekWhatMask = 0x0F,
              kMpeekHandshakeFallback = 0x10, kMpeekEarlyWindow = 0x20, kMpeekHandshakeWindow = 0x40, kMpeekDeinterleaved = 0x80,
              kMpeekSalvage = 0x100;
constexpr int kMwinTrainSkip = 4608, kMwinCheckLen = 5000, kMwinMinAvail = kMwinTrainSkip + kMwinCheckLen;   // 9608
constexpr int kMwinHandshakeCw = 3;     // max(2, calculateCodewords(ConnectFrame::PAYLOAD_SIZE = 25, R1/4))

struct MwinGeom {
    int window_len;
    int cw_samples;      // samples of one codeword: ceil(648 / (carriers * bps)) * 512 * spreading
    int cw_bits;         // soft bits of one codeword's symbols: ceil(648 / (carriers * bps)) * carriers * bps
    int disconnected;
    int max_level;       // largest codeword count a pass can run at (<= 8)
};
RIA_MWIN_HD long long mwin_frame_len(const MwinGeom& g, int cw) {                 // getMinSamplesForCWCount (mc_dpsk_waveform.cpp:470-485)
    return kMwinTrainSkip + static_cast<long long>(cw) * g.cw_samples;
}
RIA_MWIN_HD int mwin_avail_cw(const MwinGeom& g, int cw) { return static_cast<int>(static_cast<long long>(cw) * g.cw_bits / 648); }

// anti-replay (:876-889) inside one window: |sync - last| < 200; INT32_MIN = no last position
RIA_MWIN_HD bool mwin_replay(int sync_start, int last_decoded_sync) {
    if (last_decoded_sync == INT32_MIN) return false;
    const long long d = static_cast<long long>(sync_start) - last_decoded_sync;
    return (d < 0 ? -d : d) < 200;
}

// the legacy PING test (:1222-1223); a NaN training rms gives ratio 0 (a PING), a NaN data rms a NaN ratio (not a PING)
RIA_MWIN_HD bool mwin_is_ping(float training_rms, float rms) {
    const float ratio = training_rms > 0.001f ? rms / training_rms : 0.0f;
    return ratio < 0.6f;
}

struct MwinStep {
    int outcome;         // kMwinOpen: run a pass at `level` codewords; else the window's outcome
    int level;
    int pending;         // pending_total_cw_ as the chain leaves it
    int need_samples;
    int passes;          // passes of decodeCurrentFrame that ran process() in the chain
    int peek;            // kMpeek* bits the chain adds
};

// pending_total_cw_ = pending > 0 and state SYNC_FOUND: the passes that follow until one decodes.  Each pass waits for
// getMinSamplesForCWCount(pending) samples (:989-991; the window ends there: NEED_SAMPLES), runs process() - which a span of
// that length cannot fail - skips the peek (:1444), and under !connected_ raises fewer than three codewords to three (:1611-1624).
RIA_MWIN_HD MwinStep mwin_escalate(const MwinGeom& g, int sync_start, int pending) {
    MwinStep st{kMwinOpen, 0, pending, 0, 0, 0};
    for (;;) {
        st.pending = pending;
        const long long len = mwin_frame_len(g, pending);
        if (sync_start + len > g.window_len) { st.outcome = kMwinNeedSamples; st.need_samples = static_cast<int>(len < INT32_MAX ? len : INT32_MAX); return st; }
        if (pending > g.max_level) { st.outcome = kMwinTooLong; return st; }
        ++st.passes;
        if (g.disconnected && mwin_avail_cw(g, pending) < kMwinHandshakeCw && pending < kMwinHandshakeCw) {
            st.peek |= kMpeekHandshakeWindow;
            pending = kMwinHandshakeCw;
            continue;
        }
        st.level = pending;
        return st;
    }
}

// The CW0 peek (:1444-1503) and the two rules behind it (:1600-1624) on a pass with pending_total_cw_ == 0 that gave n_llr > 0
// soft bits.  have_cw0: robustDecodeSingleCW (raw or de-interleaved) ok with the magic; header_valid / type / total_cw:
// parseHeader of it.  Returns pending_total_cw_ (0: this pass's soft bits are decoded) and the kMpeek* bits.
RIA_MWIN_HD int mwin_peek(int disconnected, int n_llr, bool have_cw0, bool header_valid, int type, int total_cw, int* peek) {
    const int avail_cw = n_llr / 648;
    const int min_handshake_cw = disconnected ? kMwinHandshakeCw : 0;
    int bits = kMpeekNone;
    if (n_llr >= 648) {
        bits = kMpeekNoHeader;
        if (have_cw0 && header_valid) {
            int needed = total_cw;
            bits = kMpeekHeaderSingle;
            const bool connect_handshake = type == 0x12 || type == 0x13 || type == 0x14;   // isConnectFrame && != DISCONNECT
            if (connect_handshake && min_handshake_cw > 0 && needed < min_handshake_cw) { needed = min_handshake_cw; bits = kMpeekConnectForced; }
            if (needed > 1 && avail_cw < needed) {
                if (bits != kMpeekConnectForced) bits = kMpeekHeaderMulti;
                *peek = bits;
                return needed;
            }
        }
        if (min_handshake_cw > 1 && avail_cw < min_handshake_cw) { *peek = bits | kMpeekHandshakeFallback; return min_handshake_cw; }
    } else if (disconnected) {
        *peek = kMpeekEarlyWindow;                         // :1600-1609
        return 1;
    }
    if (disconnected && avail_cw < kMwinHandshakeCw) { *peek = bits | kMpeekHandshakeWindow; return kMwinHandshakeCw; }   // :1611-1624, pending 0 < 3
    *peek = bits;
    return 0;
}

}  // namespace ria
