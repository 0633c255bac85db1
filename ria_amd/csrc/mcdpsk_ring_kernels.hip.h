// ria_amd/csrc/mcdpsk_ring_kernels.hip.h — device side of ria_gpu_mcdpsk_ring_batch (include/ria_gpu.h): what
// mcdpsk_stream_kernels.hip.h adds to the stream loop - chase caches on an audio clock, the SYNC_FOUND wait carried from call
// to call - on ring_kernels.hip.h's loop, where windows are cut from the capture by absolute index and cursor and last
// decoded position live on the ring.  The found, group and open lists are ring_stream_list_kernel's: the pending list below
// writes the ring search records it reads.  Nothing here is receiver arithmetic: lists, copies, ring_rules.hpp,
// mcdpsk_stream_rules.hpp and mcdpsk_ring_rules.hpp.
//
//   mcring_check_kernel    a thread per stream, ahead of everything: the ring search's domain, the pending fields' domain,
//                          the cache ids (an owner word per cache, claimed with a compare-and-swap: only whether a second
//                          claim happened is read, not which came first); counts the pending streams.  Nothing is written
//                          but the control block and the owner words.
//   mcring_init_kernel     a thread per stream: the result record cleared, the `ring` part of the state into the contiguous
//                          records the ring search works on.
//   mcring_pending_kernel  one block, acq_block_scan, ascending: the streams that wait at a sync.  One whose samples have
//                          arrived gets its re-entered window's length, a ring search record that names the stored detection
//                          (ring indices from the absolute ones) and the arrival rule; one whose samples have not closes with
//                          RIA_STREAM_WINDOW_NEED_SAMPLES.
//   mcring_gather_kernel   grid (x, windows of the chunk): [abs_search_start, abs_search_start + window_len) of the stream's
//                          own capture row into the window workspace.  The source has no alignment (abs_search_start is any
//                          index), so it is read a float at a time - consecutive lanes read consecutive quads, every line
//                          fetched is used whole - and only inside [0, capture_len); the destination rows start on 16 bytes
//                          and are a multiple of four floats long, so it is written in 16-byte stores, zero past the capture.
//                          Every index is 64-bit: a batch of minutes-long recordings is longer than 2^32 bytes.
//   mcring_params_kernel   a thread per window of the chunk: ring_stream_params_kernel's MC-DPSK record with
//                          pending_total_cw, and the window's cache id and its time on the absolute sync position.
//   mcring_apply_kernel    a thread per window of the chunk: ring_stream_apply_kernel's MC-DPSK branch, then the window's
//                          chase record into the event's row and the eight pending fields written or cleared.
//   mcring_finish_kernel   a thread per stream: the `ring` part of the state back into the caller's records.
//
// A stream's records depend on its own capture, state and cache only, and every list comes from a scan: chunking, grouping
// and scheduling change nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "mcdpsk_ring_rules.hpp"
#include "mcdpsk_stream_kernels.hip.h"
#include "ring_kernels.hip.h"

namespace ria {

struct McRingArgs {
    RingStreamArgs S;                        // S.state: the contiguous ring states [n_streams] the loop works on
    ria_mcdpsk_ring_state* mstate;           // [n_streams] the caller's records
    const int32_t* cache_id;                 // [n_streams], null without a pool
    const uint64_t* t0_ms;                   // [n_streams], null without a pool
    int32_t* owner; int n_caches;            // the pool's owner words, null without a pool
    ria_mcdpsk_harq_result* harq;            // [n_streams][max_events], nullable
    ria_ring_search_result* sres_w;          // S.sres, writable: the pending list names the stored detections in it
    McStreamCtl* mctl;
    int sample_rate, search_len;
    int pending_round;                       // the chunk's windows are re-entries
    // one chunk of a group
    int32_t* w_cache_id; uint64_t* w_now_ms; // [n_chunk]
    const ria_mcdpsk_harq_result* w_harq;    // [n_chunk] the window call's
};

__global__ __launch_bounds__(256) void mcring_check_kernel(McRingArgs M) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= M.S.n_streams) return;
    const ria_mcdpsk_ring_state* st = M.mstate + b;
    const int cap = M.S.capture_len[b];
    unsigned bad = 0;
    if (!ring_domain_ok(&st->ring, cap, M.S.stride) ||
        !mcring_pending_domain_ok(st->pending_total_cw, st->need_samples, st->pend_search_start, st->pend_sync_position, cap, M.search_len,
                                  st->ring.total_fed))
        bad |= kMcStreamBadDomain;
    else if (st->pending_total_cw > 0) atomicAdd(&M.mctl->n_pending, 1u);
    if (M.cache_id) {
        const int c = M.cache_id[b];
        if (c >= 0 && (c >= M.n_caches || atomicCAS(&M.owner[c], -1, b) != -1)) bad |= kMcStreamBadCache;
    }
    if (bad) atomicOr(&M.mctl->bad, bad);
}

__global__ __launch_bounds__(256) void mcring_init_kernel(McRingArgs M) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= M.S.n_streams) return;
    ria_ring_stream_result r{};
    r.mode = M.S.mode;
    M.S.res[b] = r;
    M.S.state[b] = M.mstate[b].ring;
}

__global__ __launch_bounds__(kAcqScanThreads) void mcring_pending_kernel(McRingArgs M) {
    const RingStreamArgs& A = M.S;
    int running = 0;
    for (int base = 0; base < A.n_streams; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        bool flag = false;
        int len = 0;
        if (b < A.n_streams) {
            const ria_mcdpsk_ring_state* st = M.mstate + b;
            if (st->pending_total_cw > 0) {
                const int cap = A.capture_len[b];
                const int start = st->pend_search_start, sync = st->pend_sync_position, need = st->need_samples;
                flag = mcstream_reentry_fits(cap, sync, need);
                if (flag) {
                    len = mcstream_reentry_window_len(A.full, cap, start, sync, need);
                    ria_ring_search_result r{};
                    r.outcome = kSearchSyncFound;
                    r.search_start = ring_mod(start); r.search_len = M.search_len; r.sync_position = ring_mod(sync);
                    r.abs_position = sync; r.abs_search_start = start;
                    r.correlation = st->pend_correlation; r.known_cfo_hz = st->pend_known_cfo_hz; r.detect_threshold = st->pend_detect_threshold;
                    r.min_confidence = st->pend_min_confidence;
                    r.sync_cfo_hz = st->ring.last_cfo_hz; r.sync_snr_db = st->ring.snr_hint;
                    r.marker = -1; r.root = -1;
                    M.sres_w[b] = r;
                    A.state[b].total_fed = mcring_reentry_fed(A.state[b].total_fed, sync, need);
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

// grid (x, n_chunk): window blockIdx.y of the chunk.  A thread takes quads of the window; the row's last quad may reach past
// window_len, inside the row (win_stride is window_len rounded up to four, or more), and is zero there.
__global__ __launch_bounds__(256) void mcring_gather_kernel(McRingArgs M) {
    const RingStreamArgs& A = M.S;
    const int e = static_cast<int>(blockIdx.y);
    const uint32_t b = A.group[A.first + e];
    const long long cap = A.capture_len[b];
    long long start = A.sres[b].abs_search_start;
    long long have = cap - start;                       // samples of the window that the capture holds
    if (start < 0 || have < 0) { start = 0; have = 0; } // no such window comes out of the search or the check: read nothing
    if (have > A.window_len) have = A.window_len;
    const float* __restrict__ src = A.samples + static_cast<long long>(b) * A.stride + start;
    float4* __restrict__ dst = reinterpret_cast<float4*>(A.win + static_cast<long long>(e) * A.win_stride);
    const long long quads = (static_cast<long long>(A.window_len) + 3) >> 2;
    for (long long q = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; q < quads; q += static_cast<long long>(gridDim.x) * 256) {
        const long long i = q << 2;
        float4 v;
        v.x = i < have ? src[i] : 0.0f;
        v.y = i + 1 < have ? src[i + 1] : 0.0f;
        v.z = i + 2 < have ? src[i + 2] : 0.0f;
        v.w = i + 3 < have ? src[i + 3] : 0.0f;
        dst[q] = v;
    }
}

__global__ __launch_bounds__(256) void mcring_params_kernel(McRingArgs M) {
    const RingStreamArgs& A = M.S;
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_ring_search_result* r = A.sres + b;
    ria_mcdpsk_acq_params p{};
    p.known_cfo_hz = r->known_cfo_hz; p.detect_threshold = r->detect_threshold;
    p.min_confidence = stream_min_confidence(r->min_confidence, r->correlation);
    p.abs_base = static_cast<uint64_t>(r->abs_search_start);
    p.last_decoded_sync = ring_rebase_last_sync(A.state[b].last_decoded_sync_pos, r->search_start);
    p.pending_total_cw = M.pending_round ? static_cast<uint32_t>(M.mstate[b].pending_total_cw) : 0u;
    A.mpar[e] = p;
    M.w_cache_id[e] = M.cache_id ? M.cache_id[b] : -1;
    M.w_now_ms[e] = mcring_now_ms(M.t0_ms ? M.t0_ms[b] : 0u, r->abs_position, M.sample_rate);
}

__global__ __launch_bounds__(256) void mcring_apply_kernel(McRingArgs M) {
    const RingStreamArgs& A = M.S;
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_ring_search_result* r = A.sres + b;
    ria_ring_state* sp = A.state + b;
    const int n_before = A.res[b].n_events;
    if (n_before < 0 || n_before >= A.max_events) return;       // an open stream has room: the close rule
    const ria_mcdpsk_window_result w = A.mres[e];
    const ria_mcdpsk_acq_result a = A.macq[e];
    const ria_mcdpsk_acq_params p = A.mpar[e];
    const bool delivered = w.deliver != 0;
    const long long abs_start = r->abs_search_start, abs_sync = r->abs_position;
    const long long abs_cursor = ring_abs_cursor(kStreamMcdpsk, w.outcome, w.next_pos, abs_start, abs_sync, A.first_frame);
    ria_stream_event ev{};
    ev.frame_bytes = a.frame_bytes; ev.need_samples = w.need_samples; ev.pending_total_cw = w.pending_total_cw;
    ev.success = a.success; ev.codewords_ok = a.codewords_ok; ev.codewords_failed = a.codewords_failed; ev.frame_type = a.frame_type;
    ev.sync_position = static_cast<int32_t>(abs_sync); ev.search_start = static_cast<int32_t>(abs_start); ev.window_len = A.window_len;
    ev.outcome = w.outcome;
    ev.next_pos = w.next_pos >= 0 ? static_cast<int32_t>(abs_start + w.next_pos) : -1;
    ev.delivered = delivered ? 1 : 0;
    ev.correlation = r->correlation; ev.cfo_hz = a.cfo_hz; ev.fading_index = a.fading_index; ev.snr_db = r->sync_snr_db;
    // the state: step 5 of ria_gpu_rx_ring_batch
    if (stream_moved(kStreamMcdpsk, w.outcome)) { sp->last_cfo_hz = a.cfo_hz; sp->fading_hint = a.fading_index; }
    sp->last_decoded_sync_pos = ring_last_sync(kStreamMcdpsk, delivered, r->sync_position, sp->last_decoded_sync_pos, w.last_decoded_sync, r->search_start);
    if (abs_cursor >= 0) {
        sp->correlation_pos = ring_mod(abs_cursor);
        sp->total_fed = ring_stream_fed(sp->total_fed, A.capture_len[b], abs_cursor);
    }
    // the wait at the sync, in absolute indices: written by a window that asks for samples, cleared by every other
    ria_mcdpsk_ring_state* ms = M.mstate + b;
    const bool keep = mcstream_keeps_pending(w.outcome);
    ms->pending_total_cw = keep ? w.pending_total_cw : 0;
    ms->need_samples = keep ? w.need_samples : 0;
    ms->pend_search_start = keep ? static_cast<int32_t>(abs_start) : 0;
    ms->pend_sync_position = keep ? static_cast<int32_t>(abs_sync) : 0;
    ms->pend_known_cfo_hz = keep ? p.known_cfo_hz : 0.0f;
    ms->pend_detect_threshold = keep ? p.detect_threshold : 0.0f;
    ms->pend_min_confidence = keep ? p.min_confidence : 0.0f;
    ms->pend_correlation = keep ? r->correlation : 0.0f;
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
    A.res[b].closed = ring_stream_close(kStreamMcdpsk, w.outcome, n_before + 1, A.max_events);
}

__global__ __launch_bounds__(256) void mcring_finish_kernel(McRingArgs M) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= M.S.n_streams) return;
    M.mstate[b].ring = M.S.state[b];
}

}  // namespace ria
