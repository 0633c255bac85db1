// ria_amd/csrc/mcdpsk_stream_rules.hpp — the scalar rules ria_gpu_mcdpsk_stream_batch adds to stream_rules.hpp's: the audio
// clock the chase caches see, and the SYNC_FOUND wait of gui::StreamingDecoder (src/gui/modem/streaming_decoder.cpp:943-1019,
// pending_total_cw_) carried from one call to the next in ria_mcdpsk_stream_state.  Integers only, no arithmetic of the
// receiver.  Plain C++17, no HIP types: tests/helpers/mcdpsk_stream_rules_check.cpp builds it with g++.
#pragma once
#include <stdint.h>

#include "stream_rules.hpp"

namespace ria {

// the time a window of a stream is decoded at: the caller's clock at sample 0 plus the sync's place on the recording, in
// whole milliseconds; unsigned and modulo 2^64, as the pool's own arithmetic is.  sample_rate is the handle's (48000).
RIA_STRM_HD uint64_t mcstream_now_ms(uint64_t t0_ms, int sync_position, int sample_rate) {
    return t0_ms + static_cast<uint64_t>(static_cast<uint32_t>(sync_position)) * 1000u / static_cast<uint64_t>(static_cast<uint32_t>(sample_rate));
}

// the pending fields' domain (pending_total_cw > 0 only: a stream that searches carries zeros or anything else)
// search_len: the mode's search span; the window that waited held it, so a capture that no longer does is no capture of
// this stream
RIA_STRM_HD bool mcstream_pending_domain_ok(int pending_total_cw, int need_samples, int pend_search_start, int pend_sync_position, int capture_len,
                                            int search_len) {
    if (pending_total_cw < 0 || pending_total_cw > 255) return false;
    if (pending_total_cw == 0) return true;
    return need_samples >= 0 && pend_search_start >= 0 && pend_search_start < capture_len && pend_sync_position >= 0 &&
           pend_sync_position < capture_len && capture_len - pend_search_start >= search_len;
}

// have the samples the waiting window asked for arrived?  capture_len >= pend_sync_position + need_samples
RIA_STRM_HD bool mcstream_reentry_fits(int capture_len, int pend_sync_position, int need_samples) {
    return static_cast<long long>(capture_len) >= static_cast<long long>(pend_sync_position) + static_cast<long long>(need_samples);
}

// the re-entered window: from the sample 0 of the window that waited, `full` samples or up to the end of the span it
// waits for, whichever is longer, cut at the capture's end
RIA_STRM_HD int mcstream_reentry_window_len(int full, int capture_len, int pend_search_start, int pend_sync_position, int need_samples) {
    long long want = static_cast<long long>(pend_sync_position) - static_cast<long long>(pend_search_start) + static_cast<long long>(need_samples);
    if (want < full) want = full;
    const long long left = static_cast<long long>(capture_len) - static_cast<long long>(pend_search_start);
    return static_cast<int>(left < want ? left : want);
}

// the samples the wait was for have arrived: fed = max(fed, pend_sync_position + need_samples), applied when the window fits
RIA_STRM_HD int mcstream_reentry_fed(int fed, int pend_sync_position, int need_samples) {
    const int upto = pend_sync_position + need_samples;
    return fed < upto ? upto : fed;
}

// does this window outcome leave the stream waiting at its sync (the eight pending fields written), or clear them?
RIA_STRM_HD bool mcstream_keeps_pending(int mwin_outcome) { return mwin_outcome == kStrmMwinNeedSamples; }

}  // namespace ria
