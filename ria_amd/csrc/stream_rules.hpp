// ria_amd/csrc/stream_rules.hpp — the scalar rules of ria_gpu_rx_stream_batch that the device and the host share: what
// the host does between ria_gpu_search_batch and the window call of the mode, and behind it ("From a
// capture to its windows"; gui::StreamingDecoder::processBuffer, src/gui/modem/streaming_decoder.cpp:293-384, with the
// state decodeCurrentFrame leaves, :1994-2013).  The window a found stream gets, the window parameters the search result
// names, the state update behind the window call and the rule that closes a stream.  Integers and float32 copies only:
// no arithmetic of the receiver is restated here.  Plain C++17, no HIP types: tests/helpers/stream_rules_check.cpp builds
// it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RIA_STRM_HD __host__ __device__ __forceinline__
#else
#define RIA_STRM_HD inline
#endif

namespace ria {

// the two families of window outcomes: RIA_WIN_* (ria_gpu_rx_window_batch) and RIA_MWIN_* (ria_gpu_mcdpsk_window_batch)
constexpr int kStreamOfdm = 0, kStreamMcdpsk = 1;
// mirrors of include/ria_gpu.h
constexpr int kStrmWinBurst = 1, kStrmWinControlProfile = 2, kStrmWinDecoded = 3, kStrmWinNeedSamples = 4, kStrmWinTooLong = 5;
constexpr int kStrmMwinDecoded = 4, kStrmMwinNeedSamples = 5, kStrmMwinTooLong = 6;
// RIA_STREAM_*: why a stream closed; 1..3 are the search's outcomes (a found stream goes on to its window, so 1 is never reported)
constexpr int kStreamOpen = 0, kStreamSearchNeedSamples = 2, kStreamSearchLimit = 3, kStreamWindowNeedSamples = 4, kStreamEventsFull = 5,
              kStreamRingEnd = 6;
constexpr int32_t kStreamNoLastSync = INT32_MIN;      // SIZE_MAX of last_decoded_sync_pos_, in both records
constexpr int kStreamRingLast = 959999;               // a cursor at or past it closes the stream: the ring would wrap

// the window of a found stream: [search_start, search_start + min(full, capture_len - search_start))
RIA_STRM_HD int stream_window_len(int full, int capture_len, int search_start) {
    const int left = capture_len - search_start;
    return left < full ? left : full;
}

// min(min_confidence, correlation) with a NaN of either side kept, the first one first
RIA_STRM_HD float stream_min_confidence(float min_confidence, float correlation) {
    if (min_confidence != min_confidence) return min_confidence;
    if (correlation != correlation) return correlation;
    return correlation < min_confidence ? correlation : min_confidence;
}

// last_decoded_sync_pos_ as the MC-DPSK window call takes it: relative to the window, "none" kept, clipped so that a
// position far outside the window can never turn into "none"
RIA_STRM_HD int32_t stream_rebase_last_sync(int32_t last_decoded_sync_pos, int search_start) {
    if (last_decoded_sync_pos == kStreamNoLastSync) return kStreamNoLastSync;
    long long rel = static_cast<long long>(last_decoded_sync_pos) - static_cast<long long>(search_start);
    if (rel < -2147483647LL) rel = -2147483647LL;
    if (rel > 2147483647LL) rel = 2147483647LL;
    return static_cast<int32_t>(rel);
}

// did the window move last_cfo_ and the fading hint?  (a decoded window; for OFDM also the control profile)
RIA_STRM_HD bool stream_moved(int family, int outcome) {
    return family == kStreamOfdm ? (outcome == kStrmWinDecoded || outcome == kStrmWinControlProfile) : outcome == kStrmMwinDecoded;
}

// last_decoded_sync_pos_ behind the window.  OFDM: the sync position of a window that delivered, else unchanged.  MC-DPSK:
// what the window call leaves, back in capture indices.
RIA_STRM_HD int32_t stream_last_sync(int family, bool delivered, int sync_position, int32_t state_last, int32_t window_last, int search_start) {
    if (family == kStreamOfdm) return delivered ? sync_position : state_last;
    if (window_last == kStreamNoLastSync) return kStreamNoLastSync;
    return static_cast<int32_t>(static_cast<uint32_t>(window_last) + static_cast<uint32_t>(search_start));
}

// the cursor behind the window: behind the consumed samples; behind the first frame of a window the host passes on to
// another call (BURST, TOO_LONG); else where the search left it
RIA_STRM_HD int stream_cursor(int family, int outcome, int next_pos, int search_start, int sync_position, int first_frame, int cursor) {
    if (next_pos >= 0) return search_start + next_pos;
    const bool passed_on = family == kStreamOfdm ? (outcome == kStrmWinBurst || outcome == kStrmWinTooLong) : outcome == kStrmMwinTooLong;
    return passed_on ? sync_position + first_frame : cursor;
}

// the samples the window consumed have arrived: fed = max(fed, min(capture_len, cursor))
RIA_STRM_HD int stream_fed(int fed, int capture_len, int cursor) {
    const int upto = capture_len < cursor ? capture_len : cursor;
    return fed < upto ? upto : fed;
}

// why the stream closes behind this window (kStreamOpen: it does not); n_events counts this window's event
RIA_STRM_HD int stream_close(int family, int outcome, int n_events, int max_events, int cursor) {
    if (outcome == (family == kStreamOfdm ? kStrmWinNeedSamples : kStrmMwinNeedSamples)) return kStreamWindowNeedSamples;
    if (n_events >= max_events) return kStreamEventsFull;
    if (cursor >= kStreamRingLast) return kStreamRingEnd;
    return kStreamOpen;
}

}  // namespace ria
