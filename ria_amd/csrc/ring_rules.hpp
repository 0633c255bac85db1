// ria_amd/csrc/ring_rules.hpp — the scalar rules of ria_gpu_search_ring_batch that the device and the host share: the
// statements of StreamingDecoder::feedAudio (src/gui/modem/streaming_decoder.cpp:184-291, whole) and searchForSync
// (:386-941) that depend on MAX_BUFFER_SAMPLES, write_pos_ = total_fed_ % 960000 and total_fed_.  Everything that does not
// depend on the ring (tracker, gate, confidence tiers, near miss, weak accept, anti-replay distance, CFO sanity, SNR) is
// search_rules.hpp's, used as it is.  Plain C++17, no HIP needed: tests/helpers/ring_rules_check.cpp builds it with g++.
//
//   computeUnsearched, both branches (:193-202)        ring_unsearched_feed
//   the pre-wrap clamp (:204, :289)                     ring_feed
//   the drift guard (:232-238, CORR_INVARIANT_GUARD)    ring_feed
//   the overflow drop (:242-278)                        ring_feed
//   the two waits on circular unsearched (:449, :475)   ring_wait
//   correlation_pos_ == 0 after the wrap (:458-464)     ring_wait
//   ZC catch-up on circular unsearched (:488-522)       ring_catch_up
//   the post-wrap backtrack (:597-605)                  ring_search_start
//   sync_position_ (:858)                               ring_sync_position
//   ringPosToAbsolute (:862-874)                        ring_pos_to_absolute
//   anti-replay and its cursor (:876-889)               srch_replay / srch_replay_cursor (already circular)
//
// The ring's content in closed form.  feedAudio writes sample k of the stream (k = 0, 1, ..) to ring index k % 960000
// (:281-284: write_pos_ starts at 0 and advances by one per sample, whatever the overflow path did to the cursor).  After T
// samples ring index p therefore holds the LAST k < T with k % 960000 == p.  For T < 960000 that is k = p (p < T; a p >= T was
// never written and holds the buffer's initial 0).  Otherwise k = T - 1 - j for the smallest j >= 0 with
// (T - 1 - j) % 960000 == p, that is j = (T - 1 - p) mod 960000, so p holds x[T - 1 - ((T - 1 - p) mod 960000)].
#pragma once
#include "search_rules.hpp"
#include "stream_rules.hpp"

namespace ria {

constexpr int kRingGuard = 9600;                      // CORR_INVARIANT_GUARD
constexpr int kRingKeep = 360000;                     // OVERFLOW_RECOVERY_KEEP
constexpr long long kRingMaxCapture = 2147483647LL - kSrchRing;

RIA_SRCH_HD int ring_write_pos(long long total_fed) { return static_cast<int>(total_fed % kSrchRing); }

// the capture index that ring index p (0..959 999) holds after total_fed samples; -1: never written (the ring's initial 0)
RIA_SRCH_HD long long ring_source(long long total_fed, int p) {
    if (total_fed < kSrchRing) return p < total_fed ? p : -1;
    return total_fed - 1 - ((total_fed - 1 - p) % kSrchRing);
}

// the circular distance from the cursor forward to the write position (:466-472)
RIA_SRCH_HD int ring_unsearched(int write_pos, int cursor) {
    return write_pos >= cursor ? write_pos - cursor : kSrchRing - cursor + write_pos;
}
// computeUnsearched (:193-202): before the wrap a cursor ahead of the write position counts as no backlog
RIA_SRCH_HD int ring_unsearched_feed(long long total_fed, int write_pos, int cursor) {
    if (total_fed < kSrchRing) return write_pos >= cursor ? write_pos - cursor : 0;
    return ring_unsearched(write_pos, cursor);
}

struct RingFeedCounts {          // this call's counters
    unsigned int overflows, drift_snaps;
    unsigned long long overflow_dropped;
};

// feedAudio (:184-291) for count = min(feed_step, capture_len - total_fed) samples: none arriving changes nothing (:185).
// overflow_events / overflow_total are the state's running counters (overflow_events_, stats_.overflow_samples_dropped).
// Returns the samples fed.
RIA_SRCH_HD long long ring_feed(int* cursor, long long* total_fed, int* streak, unsigned int* overflow_events, unsigned long long* overflow_total,
                                RingFeedCounts* counts, long long capture_len, int feed_step) {
    long long count = capture_len - *total_fed;
    if (feed_step < count) count = feed_step;
    if (count <= 0) return 0;
    const int wp = ring_write_pos(*total_fed);
    if (*total_fed < kSrchRing && *cursor > wp) { *cursor = wp; *streak = 0; }                    // :204-225
    long long unsearched = ring_unsearched_feed(*total_fed, wp, *cursor);                          // :227
    if (*total_fed >= kSrchRing && unsearched > kSrchRing - kRingGuard) {                          // :232-238
        *cursor = wp;
        unsearched = 0;
        ++counts->drift_snaps;
    }
    if (unsearched + count >= kSrchRing) {                                                         // :242-278
        const long long incoming_total = unsearched + count;
        const long long target_after_write = kRingKeep < kSrchRing - 1 ? kRingKeep : kSrchRing - 1;
        long long need_to_drop = 0;
        if (incoming_total > target_after_write) need_to_drop = unsearched < incoming_total - target_after_write ? unsearched : incoming_total - target_after_write;
        *cursor = static_cast<int>((*cursor + need_to_drop) % kSrchRing);
        ++*overflow_events;
        *overflow_total += static_cast<unsigned long long>(need_to_drop);
        ++counts->overflows;
        counts->overflow_dropped += static_cast<unsigned long long>(need_to_drop);
    }
    *total_fed += count;                                                                           // :281-286
    if (*total_fed < kSrchRing && *cursor > ring_write_pos(*total_fed)) *cursor = ring_write_pos(*total_fed);   // :289-291
    return count;
}

// the two waits (:449, :475) with the cursor initialisation between them (:458-464), which stays done when the second
// wait returns.  Before the wrap a cursor ahead of the write position is a wait: ria_gpu_search_batch's documented limit.
RIA_SRCH_HD bool ring_wait(int* cursor, long long total_fed, int min_search, unsigned int* cursor_inits) {
    if (total_fed < min_search) return true;
    const int wp = ring_write_pos(total_fed);
    if (*cursor == 0 && total_fed >= kSrchRing) { *cursor = wp; ++*cursor_inits; }                 // :462
    if (total_fed < kSrchRing && *cursor > wp) return true;
    return ring_unsearched(wp, *cursor) < min_search;
}

// ZC backlog catch-up (:488-522) on the circular backlog: 0 none, 1 moderate, 2 severe
RIA_SRCH_HD int ring_catch_up(int* cursor, int write_pos, int min_search) {
    const long long unsearched = ring_unsearched(write_pos, *cursor);
    const long long scaled = unsearched * 10 / min_search;
    if (scaled > 25) {
        *cursor = static_cast<int>((static_cast<long long>(write_pos) + kSrchRing - min_search - 4800) % kSrchRing);
        return 2;
    }
    if (scaled > 15) {
        long long catch_up = (unsearched - min_search) / 2;
        if (24000 < catch_up) catch_up = 24000;
        if (catch_up < 4800) catch_up = 4800;
        *cursor = static_cast<int>((*cursor + catch_up) % kSrchRing);
        return 1;
    }
    return 0;
}

// backtrack (:597-605)
RIA_SRCH_HD int ring_search_start(int cursor, long long total_fed, bool zc) {
    const int backtrack = zc ? kSrchBacktrackZc : kSrchBacktrack;
    if (cursor >= backtrack) return cursor - backtrack;
    if (total_fed < kSrchRing) return 0;
    return (kSrchRing + cursor - backtrack) % kSrchRing;
}

// the search span [search_start, search_start + min_search) modulo the ring has the write position strictly inside it:
// its samples are then the stream's newest followed by its oldest, not a contiguous piece of the capture
RIA_SRCH_HD bool ring_span_wraps(int search_start, long long total_fed, int min_search) {
    if (total_fed < kSrchRing) return false;
    const int d = ring_unsearched(ring_write_pos(total_fed), search_start);     // write_pos - search_start, circular
    return d > 0 && d < min_search;
}

// sync_position_ (:858)
RIA_SRCH_HD int ring_sync_position(int search_start, int start_sample) { return (search_start + start_sample) % kSrchRing; }

// ringPosToAbsolute (:862-874)
RIA_SRCH_HD long long ring_pos_to_absolute(long long total_fed, int ring_pos) {
    if (total_fed < kSrchRing) return ring_pos;
    const long long oldest_abs = total_fed - kSrchRing;
    const int oldest_pos = ring_write_pos(total_fed);
    const long long offset = ring_pos >= oldest_pos ? ring_pos - oldest_pos : kSrchRing - oldest_pos + ring_pos;
    return oldest_abs + offset;
}

// ---- the stream loop on the ring (ria_gpu_rx_ring_batch): stream_rules.hpp's rules where they touch ring indices.  The window
// is cut from the capture by absolute index; cursor and last decoded position go back to ring indices.
constexpr int kStreamSpanLost = 7;                    // RIA_STREAM_SPAN_LOST

RIA_SRCH_HD int ring_mod(long long v) { const long long m = v % kSrchRing; return static_cast<int>(m < 0 ? m + kSrchRing : m); }

// last_decoded_sync_pos_ (a ring index) as the MC-DPSK window call takes it: the circular difference to the window's origin,
// in -480 000 .. 479 999; "none" kept
RIA_SRCH_HD int32_t ring_rebase_last_sync(int32_t last_decoded_sync_pos, int search_start) {
    if (last_decoded_sync_pos == kStreamNoLastSync) return kStreamNoLastSync;
    int d = ring_mod(static_cast<long long>(last_decoded_sync_pos) - search_start);
    if (d >= kSrchRing / 2) d -= kSrchRing;
    return d;
}

// last_decoded_sync_pos_ behind the window, a ring index again
RIA_SRCH_HD int32_t ring_last_sync(int family, bool delivered, int sync_position, int32_t state_last, int32_t window_last, int search_start) {
    if (family == kStreamOfdm) return delivered ? sync_position : state_last;
    if (window_last == kStreamNoLastSync) return kStreamNoLastSync;
    return ring_mod(static_cast<long long>(window_last) + search_start);
}

// the absolute cursor behind the window (stream_cursor's rule); -1: the cursor stays where the search left it
RIA_SRCH_HD long long ring_abs_cursor(int family, int outcome, int next_pos, long long abs_search_start, long long abs_position, int first_frame) {
    if (next_pos >= 0) return abs_search_start + next_pos;
    const bool passed_on = family == kStreamOfdm ? (outcome == kStrmWinBurst || outcome == kStrmWinTooLong) : outcome == kStrmMwinTooLong;
    return passed_on ? abs_position + first_frame : -1;
}

// the samples the window consumed have arrived: total_fed = max(total_fed, min(capture_len, absolute cursor)).  A direct
// assignment, not a feedAudio: see ring_window_arrival for why the overflow drop could not have fired.
RIA_SRCH_HD long long ring_stream_fed(long long total_fed, long long capture_len, long long abs_cursor) {
    const long long upto = capture_len < abs_cursor ? capture_len : abs_cursor;
    return total_fed < upto ? upto : total_fed;
}

// What that assignment would be as a feed.  The search that found the sync left the cursor `ahead` = backtrack + step samples
// (or, clipped before the wrap, at least one step) past span sample 0 and ran no feed since; the window call moves the
// absolute cursor to at most abs_search_start + full.  So the backlog at the assignment is unsearched = total_fed - (abs_search_start + ahead),
// the arrivals are count = max(0, abs_cursor - total_fed), and unsearched + count <= full - ahead < full <= 959 999: feedAudio's
// overflow test (unsearched + count >= 960000, :242) cannot fire.  Returns unsearched + count.
RIA_SRCH_HD long long ring_window_arrival(long long total_fed, long long abs_search_start, int ahead, long long abs_cursor, long long* unsearched, long long* count) {
    *unsearched = total_fed - (abs_search_start + ahead);
    *count = abs_cursor > total_fed ? abs_cursor - total_fed : 0;
    return *unsearched + *count;
}

// why the stream closes behind this window (kStreamOpen: it does not): stream_close without the ring's end
RIA_SRCH_HD int ring_stream_close(int family, int outcome, int n_events, int max_events) {
    if (outcome == (family == kStreamOfdm ? kStrmWinNeedSamples : kStrmMwinNeedSamples)) return kStreamWindowNeedSamples;
    if (n_events >= max_events) return kStreamEventsFull;
    return kStreamOpen;
}

}  // namespace ria
