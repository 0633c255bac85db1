// ria_amd/csrc/mcdpsk_ring_rules.hpp — the scalar rules ria_gpu_mcdpsk_ring_batch adds to ring_rules.hpp's and
// mcdpsk_stream_rules.hpp's: the audio clock of the chase caches on an ABSOLUTE (capture) index, and the SYNC_FOUND wait of
// gui::StreamingDecoder (src/gui/modem/streaming_decoder.cpp:943-1019, pending_total_cw_) carried across the ring's wrap in
// ria_mcdpsk_ring_state.  Where the arithmetic is the stream call's (the fit test, the re-entered window's length) that
// header's function is used as it is: the absolute indices fit 32 bits, captures end at 2^31 - 1 - 960000.  Integers only, no
// arithmetic of the receiver.  Plain C++17, no HIP types: tests/helpers/mcdpsk_ring_rules_check.cpp builds it with g++.
#pragma once
#include <stdint.h>

#include "mcdpsk_stream_rules.hpp"
#include "ring_rules.hpp"

namespace ria {

constexpr int kMcRingMaxSpan = kSrchRing - 1;         // the longest span a stream can wait for: one ring less a sample

// the time a window is decoded at: mcstream_now_ms on the sync's ABSOLUTE position.  On the ring index the clock would jump
// back 20 s at every lap; the cache's age (chase_policy.hpp: now - last access, read as signed) would be negative behind
// the wrap, and an entry older than its TTL would be combined all the same.
RIA_SRCH_HD uint64_t mcring_now_ms(uint64_t t0_ms, long long abs_position, int sample_rate) {
    return mcstream_now_ms(t0_ms, static_cast<int>(abs_position), sample_rate);
}

// the pending fields' domain: the stream call's (in absolute indices), and what the ring adds -
//   the span from the window's sample 0 to the end of what it waits for fits one ring (<= 959 999): a longer one the
//   reference could not wait for, its first samples would be overwritten before the last arrived;
//   the ring still holds the window's sample 0 (total_fed - pend_search_start <= 960000) and has been fed the search span
//   behind it (pend_search_start + search_len <= total_fed): the search that found the sync read that span, and the wait
//   feeds nothing.
RIA_SRCH_HD bool mcring_pending_domain_ok(int pending_total_cw, int need_samples, int pend_search_start, int pend_sync_position, int capture_len,
                                          int search_len, long long total_fed) {
    if (!mcstream_pending_domain_ok(pending_total_cw, need_samples, pend_search_start, pend_sync_position, capture_len, search_len)) return false;
    if (pending_total_cw == 0) return true;
    const long long span = static_cast<long long>(pend_sync_position) - pend_search_start + need_samples;
    if (span > kMcRingMaxSpan) return false;
    if (total_fed - pend_search_start > kSrchRing) return false;
    return static_cast<long long>(pend_search_start) + search_len <= total_fed;
}

// the samples the wait was for have arrived: total_fed = max(total_fed, pend_sync_position + need_samples)
RIA_SRCH_HD long long mcring_reentry_fed(long long total_fed, int pend_sync_position, int need_samples) {
    const long long upto = static_cast<long long>(pend_sync_position) + need_samples;
    return total_fed < upto ? upto : total_fed;
}

// Why the two assignments of a re-entry (mcring_reentry_fed, then ring_stream_fed behind the window) are no feedAudio:
// ring_window_arrival's argument with the re-entered window's length L in place of `full`.  The search that found the sync
// left the cursor `ahead` >= 1 samples past the window's sample 0 (pend_search_start) and nothing was fed during the wait.
// The backlog is unsearched = total_fed - (pend_search_start + ahead).  The first assignment brings total_fed to at most
// pend_sync_position + need_samples <= pend_search_start + L (the window fits, so L covers the span), the second to at most
// the absolute cursor <= pend_search_start + L.  Backlog plus all arrivals is therefore at most
//   max(total_fed, pend_search_start + L) - pend_search_start - ahead.
// L <= 959 999 (the domain: full and the span are), and total_fed - pend_search_start <= 960000 (the domain), so the sum is at
// most 960000 - ahead < 960000: feedAudio's overflow test (unsearched + count >= 960000, :242) cannot fire.
// Returns the backlog plus the arrivals of both steps; *fed_out: total_fed behind them.
RIA_SRCH_HD long long mcring_reentry_arrival(long long total_fed, int pend_search_start, int pend_sync_position, int need_samples, int ahead,
                                             long long capture_len, long long abs_cursor, long long* fed_out) {
    long long unsearched, count;
    const long long t1 = mcring_reentry_fed(total_fed, pend_sync_position, need_samples);
    ring_window_arrival(total_fed, pend_search_start, ahead, t1, &unsearched, &count);
    const long long backlog = unsearched, first = count;
    const long long t2 = abs_cursor >= 0 ? ring_stream_fed(t1, capture_len, abs_cursor) : t1;
    ring_window_arrival(t1, pend_search_start, ahead, t2, &unsearched, &count);
    *fed_out = t2;
    return backlog + first + count;
}

}  // namespace ria
