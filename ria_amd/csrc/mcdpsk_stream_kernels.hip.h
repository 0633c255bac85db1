// ria_amd/csrc/mcdpsk_stream_kernels.hip.h — device side of ria_gpu_mcdpsk_stream_batch (include/ria_gpu.h): what the call
// adds to stream_kernels.hip.h's loop for the MC-DPSK modes - chase caches on an audio clock, and the SYNC_FOUND wait carried
// from call to call.  The found, group and open lists and the gather are stream_list_kernel's and stream_gather_kernel's: the
// pending list below writes the search records they read.  Nothing here is receiver arithmetic: lists, copies,
// stream_rules.hpp and mcdpsk_stream_rules.hpp.
//
//   mcstream_check_kernel    a thread per stream, ahead of everything: the search's domain, the pending fields' domain, the
//                            cache ids (an owner word per cache, claimed with a compare-and-swap as the decode-frame call's
//                            are); counts the pending streams.  Nothing is written but the control block and the owner words.
//   mcstream_init_kernel     a thread per stream: the result record cleared, the search part of the state into the
//                            contiguous records the search works on.
//   mcstream_pending_kernel  one block, acq_block_scan, ascending: the streams that wait at a sync.  One whose samples have
//                            arrived gets its re-entered window's length, a search record that names the stored detection and
//                            the arrival rule; one whose samples have not closes with RIA_STREAM_WINDOW_NEED_SAMPLES.
//   mcstream_params_kernel   a thread per window of the chunk: stream_params_kernel's MC-DPSK record with pending_total_cw,
//                            and the window's cache id and time.
//   mcstream_apply_kernel    a thread per window of the chunk: stream_apply_kernel's MC-DPSK branch, then the window's chase
//                            record into the event's row and the eight pending fields written or cleared.
//   mcstream_finish_kernel   a thread per stream: the search part of the state back into the caller's records.
//
// A stream's records depend on its own capture, state and cache only, and every list comes from a scan: chunking, grouping
// and scheduling change nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "mcdpsk_stream_rules.hpp"
#include "search_kernels.hip.h"
#include "stream_kernels.hip.h"

namespace ria {

struct McStreamCtl {             // read back by the host once, ahead of the first write
    unsigned int bad;            // 1: a state or capture outside the domain; 2: a cache id twice, or not below n_caches
    unsigned int n_pending;      // streams that come in with pending_total_cw > 0
    unsigned int pad_[2];
};
constexpr unsigned kMcStreamBadDomain = 1u, kMcStreamBadCache = 2u;

struct McStreamArgs {
    StreamArgs S;                            // S.state: the contiguous search states [n_streams] the loop works on
    ria_mcdpsk_stream_state* mstate;         // [n_streams] the caller's records
    const int32_t* cache_id;                 // [n_streams], null without a pool
    const uint64_t* t0_ms;                   // [n_streams], null without a pool
    int32_t* owner; int n_caches;            // the pool's owner words, null without a pool
    ria_mcdpsk_harq_result* harq;            // [n_streams][max_events], nullable
    ria_search_result* sres_w;               // S.sres, writable: the pending list names the stored detections in it
    McStreamCtl* mctl;
    int sample_rate, search_len;
    int pending_round;                       // the chunk's windows are re-entries
    // one chunk of a group
    int32_t* w_cache_id; uint64_t* w_now_ms; // [n_chunk]
    const ria_mcdpsk_harq_result* w_harq;    // [n_chunk] the window call's
};

__global__ __launch_bounds__(256) void mcstream_check_kernel(McStreamArgs M) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= M.S.n_streams) return;
    const ria_mcdpsk_stream_state st = M.mstate[b];
    const int cap = M.S.capture_len[b];
    unsigned bad = 0;
    if (!search_domain_ok(st.search, cap, M.S.stride) ||
        !mcstream_pending_domain_ok(st.pending_total_cw, st.need_samples, st.pend_search_start, st.pend_sync_position, cap, M.search_len))
        bad |= kMcStreamBadDomain;
    else if (st.pending_total_cw > 0) atomicAdd(&M.mctl->n_pending, 1u);
    if (M.cache_id) {
        const int c = M.cache_id[b];
        if (c >= 0 && (c >= M.n_caches || atomicCAS(&M.owner[c], -1, b) != -1)) bad |= kMcStreamBadCache;
    }
    if (bad) atomicOr(&M.mctl->bad, bad);
}

__global__ __launch_bounds__(256) void mcstream_init_kernel(McStreamArgs M) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= M.S.n_streams) return;
    ria_stream_result r{};
    r.mode = M.S.mode;
    M.S.res[b] = r;
    M.S.state[b] = M.mstate[b].search;
}

__global__ __launch_bounds__(kAcqScanThreads) void mcstream_pending_kernel(McStreamArgs M) {
    const StreamArgs& A = M.S;
    int running = 0;
    for (int base = 0; base < A.n_streams; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        bool flag = false;
        int len = 0;
        if (b < A.n_streams) {
            const ria_mcdpsk_stream_state st = M.mstate[b];
            if (st.pending_total_cw > 0) {
                const int cap = A.capture_len[b];
                flag = mcstream_reentry_fits(cap, st.pend_sync_position, st.need_samples);
                if (flag) {
                    len = mcstream_reentry_window_len(A.full, cap, st.pend_search_start, st.pend_sync_position, st.need_samples);
                    ria_search_result r{};
                    r.outcome = kSearchSyncFound;
                    r.search_start = st.pend_search_start; r.search_len = M.search_len; r.sync_position = st.pend_sync_position;
                    r.abs_position = st.pend_sync_position;
                    r.correlation = st.pend_correlation; r.known_cfo_hz = st.pend_known_cfo_hz; r.detect_threshold = st.pend_detect_threshold;
                    r.min_confidence = st.pend_min_confidence;
                    r.sync_cfo_hz = st.search.last_cfo_hz; r.sync_snr_db = st.search.snr_hint;
                    r.marker = -1; r.root = -1;
                    M.sres_w[b] = r;
                    A.state[b].fed = mcstream_reentry_fed(A.state[b].fed, st.pend_sync_position, st.need_samples);
                } else {
                    A.res[b].closed = kStreamWindowNeedSamples;
                }
            }
        }
        int total;
        const int pos = running + acq_block_scan(flag, &total);
        if (flag) { A.found[pos] = static_cast<uint32_t>(b); A.found_len[pos] = len; }
        running += total;
    }
    if (threadIdx.x == 0) A.ctl->n_found = static_cast<unsigned>(running);
}

__global__ __launch_bounds__(256) void mcstream_params_kernel(McStreamArgs M) {
    const StreamArgs& A = M.S;
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_search_result& r = A.sres[b];
    ria_mcdpsk_acq_params p{};
    p.known_cfo_hz = r.known_cfo_hz; p.detect_threshold = r.detect_threshold;
    p.min_confidence = stream_min_confidence(r.min_confidence, r.correlation);
    p.abs_base = static_cast<uint64_t>(r.search_start);
    p.last_decoded_sync = stream_rebase_last_sync(A.state[b].last_decoded_sync_pos, r.search_start);
    p.pending_total_cw = M.pending_round ? static_cast<uint32_t>(M.mstate[b].pending_total_cw) : 0u;
    A.mpar[e] = p;
    M.w_cache_id[e] = M.cache_id ? M.cache_id[b] : -1;
    M.w_now_ms[e] = mcstream_now_ms(M.t0_ms ? M.t0_ms[b] : 0u, r.sync_position, M.sample_rate);
}

__global__ __launch_bounds__(256) void mcstream_apply_kernel(McStreamArgs M) {
    const StreamArgs& A = M.S;
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_search_result& r = A.sres[b];
    ria_search_state s = A.state[b];
    const int n_before = A.res[b].n_events;
    if (n_before < 0 || n_before >= A.max_events) return;       // an open stream has room: the close rule
    const ria_mcdpsk_window_result w = A.mres[e];
    const ria_mcdpsk_acq_result a = A.macq[e];
    const ria_mcdpsk_acq_params p = A.mpar[e];
    const bool delivered = w.deliver != 0;
    ria_stream_event ev{};
    ev.frame_bytes = a.frame_bytes; ev.need_samples = w.need_samples; ev.pending_total_cw = w.pending_total_cw;
    ev.success = a.success; ev.codewords_ok = a.codewords_ok; ev.codewords_failed = a.codewords_failed; ev.frame_type = a.frame_type;
    ev.sync_position = r.sync_position; ev.search_start = r.search_start; ev.window_len = A.window_len; ev.outcome = w.outcome;
    ev.next_pos = w.next_pos >= 0 ? r.search_start + w.next_pos : -1;
    ev.delivered = delivered ? 1 : 0;
    ev.correlation = r.correlation; ev.cfo_hz = a.cfo_hz; ev.fading_index = a.fading_index; ev.snr_db = r.sync_snr_db;
    // the state
    if (stream_moved(kStreamMcdpsk, w.outcome)) { s.last_cfo_hz = a.cfo_hz; s.fading_hint = a.fading_index; }
    s.last_decoded_sync_pos = stream_last_sync(kStreamMcdpsk, delivered, r.sync_position, s.last_decoded_sync_pos, w.last_decoded_sync, r.search_start);
    s.correlation_pos = stream_cursor(kStreamMcdpsk, w.outcome, w.next_pos, r.search_start, r.sync_position, A.first_frame, s.correlation_pos);
    s.fed = stream_fed(s.fed, A.capture_len[b], s.correlation_pos);
    A.state[b] = s;
    // the wait at the sync: written by a window that asks for samples, cleared by every other
    ria_mcdpsk_stream_state* ms = M.mstate + b;
    const bool keep = mcstream_keeps_pending(w.outcome);
    ms->pending_total_cw = keep ? w.pending_total_cw : 0;
    ms->need_samples = keep ? w.need_samples : 0;
    ms->pend_search_start = keep ? r.search_start : 0;
    ms->pend_sync_position = keep ? r.sync_position : 0;
    ms->pend_known_cfo_hz = keep ? p.known_cfo_hz : 0.0f;
    ms->pend_detect_threshold = keep ? p.detect_threshold : 0.0f;
    ms->pend_min_confidence = keep ? p.min_confidence : 0.0f;
    ms->pend_correlation = keep ? r.correlation : 0.0f;
    // the event, its chase record and its payload row (cleared at the start of the call)
    const size_t row = static_cast<size_t>(b) * static_cast<size_t>(A.max_events) + static_cast<size_t>(n_before);
    A.events[row] = ev;
    if (M.harq) M.harq[row] = M.w_harq[e];
    if (delivered) {
        int nbytes = ev.frame_bytes;
        if (nbytes > A.wframe_row) nbytes = A.wframe_row;
        if (nbytes > A.frame_row) nbytes = A.frame_row;
        const uint8_t* __restrict__ src = A.wframes + static_cast<size_t>(e) * static_cast<size_t>(A.wframe_row);
        uint8_t* __restrict__ dst = A.frames + row * static_cast<size_t>(A.frame_row);
        for (int i = 0; i < nbytes; ++i) dst[i] = src[i];
    }
    A.res[b].n_events = n_before + 1;
    A.res[b].closed = stream_close(kStreamMcdpsk, w.outcome, n_before + 1, A.max_events, s.correlation_pos);
}

__global__ __launch_bounds__(256) void mcstream_finish_kernel(McStreamArgs M) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= M.S.n_streams) return;
    M.mstate[b].search = M.S.state[b];
}

}  // namespace ria
