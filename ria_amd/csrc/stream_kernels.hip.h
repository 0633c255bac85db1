// ria_amd/csrc/stream_kernels.hip.h — device side of ria_gpu_rx_stream_batch (include/ria_gpu.h): the host's part of
// StreamingDecoder::processBuffer's loop (streaming_decoder.cpp:293-384) between ria_gpu_search_batch and the window call of
// the mode, for a batch of captures.  Nothing here is receiver arithmetic: lists, copies and stream_rules.hpp.
//
//   stream_init_kernel    a thread per stream: the result record cleared (behind the first search leg, whose domain check
//                         fails the call before anything is written).
//   stream_list_kernel    one block, acq_block_scan, ascending: the open streams (kStreamListOpen); behind the search the
//                         found streams with their window lengths, the search's counters added to the result and the
//                         streams that did not find a sync closed (kStreamListFound); the found streams of one window
//                         length (kStreamListGroup).
//   stream_gather_kernel  a chunk of a group: each stream's window [search_start, search_start + window_len) into a strided
//                         workspace.  search_start and capture_len are arbitrary, so the loads are dwords.
//   stream_params_kernel  a thread per window of the chunk: search result -> ria_acq_params / ria_mcdpsk_acq_params.
//   stream_apply_kernel   a thread per window of the chunk: window result -> state, the event record, the payload row, and
//                         whether the stream closes.
//
// A stream's records depend on its own capture and state only, and every list comes from a scan: chunking, grouping and
// scheduling change nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "search_rules.hpp"
#include "stream_rules.hpp"

namespace ria {

struct StreamCtl {               // read back by the host with the two lists behind it (one copy)
    unsigned int n_open, n_found;
    unsigned int pad_[2];
};
constexpr int kStreamListOpen = 0, kStreamListFound = 1, kStreamListGroup = 2;

struct StreamArgs {
    const float* samples; long long stride;
    const int32_t* capture_len;
    ria_search_state* state;             // [n_streams], read and written in place
    const ria_search_result* sres;       // [n_streams], by stream: the last search leg's
    ria_stream_result* res;              // [n_streams]
    ria_stream_event* events;            // [n_streams][max_events]
    uint8_t* frames; int frame_row;      // [n_streams][max_events][frame_row]
    int n_streams, mode, family, full, first_frame, max_events;
    StreamCtl* ctl;
    uint32_t* found; int32_t* found_len; // [n_streams] behind ctl: found streams, ascending, and their window lengths
    uint32_t* open;                      // [n_streams] open streams, ascending
    uint32_t* group;                     // [n_streams] found streams of one window length, ascending
    int n_open, n_found;                 // the lists' lengths, as the host read them
    // one chunk of a group
    int window_len, first, n_chunk;
    float* win; long long win_stride;    // [n_chunk][win_stride]
    ria_acq_params* par; ria_mcdpsk_acq_params* mpar;                                   // [n_chunk], one of them
    const ria_window_result* wres;                                                      // OFDM
    const ria_mcdpsk_window_result* mres; const ria_mcdpsk_acq_result* macq;            // MC-DPSK
    const uint8_t* wframes; int wframe_row;                                             // [n_chunk][wframe_row]
};

__global__ __launch_bounds__(256) void stream_init_kernel(StreamArgs A) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= A.n_streams) return;
    ria_stream_result r{};
    r.mode = A.mode;
    A.res[b] = r;
}

__global__ __launch_bounds__(kAcqScanThreads) void stream_list_kernel(StreamArgs A, int what) {
    const int n = what == kStreamListOpen ? A.n_streams : what == kStreamListFound ? A.n_open : A.n_found;
    int running = 0;
    for (int base = 0; base < n; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        bool flag = false;
        uint32_t b = 0;
        int len = 0;
        if (i < n) {
            if (what == kStreamListOpen) {
                b = static_cast<uint32_t>(i);
                flag = A.res[i].closed == kStreamOpen;
            } else if (what == kStreamListFound) {
                b = A.open ? A.open[i] : static_cast<uint32_t>(i);      // no list: the first round, every stream
                const ria_search_result& r = A.sres[b];
                ria_stream_result* o = A.res + b;
                o->search_legs += 1;
                o->invocations += r.invocations; o->waits += r.waits; o->rms_skips += r.rms_skips; o->detector_runs += r.detector_runs;
                o->rejects += r.rejects; o->near_misses += r.near_misses; o->weak_accepts += r.weak_accepts; o->replays += r.replays;
                o->catchups_moderate += r.catchups_moderate; o->catchups_severe += r.catchups_severe;
                flag = r.outcome == kSearchSyncFound;
                if (flag) len = stream_window_len(A.full, A.capture_len[b], r.search_start);
                else o->closed = r.outcome;
            } else {
                b = A.found[i];
                flag = A.found_len[i] == A.window_len;
            }
        }
        int total;
        const int pos = running + acq_block_scan(flag, &total);
        if (flag) {
            if (what == kStreamListOpen) A.open[pos] = b;
            else if (what == kStreamListFound) { A.found[pos] = b; A.found_len[pos] = len; }
            else A.group[pos] = b;
        }
        running += total;
    }
    if (threadIdx.x == 0) {
        if (what == kStreamListOpen) A.ctl->n_open = static_cast<unsigned>(running);
        else if (what == kStreamListFound) A.ctl->n_found = static_cast<unsigned>(running);
    }
}

// grid (x, n_chunk): window blockIdx.y of the chunk.  The window lies inside the capture by the rule that sized it; the
// copy is bounded by the capture all the same, and what lies past it would be zero.
__global__ __launch_bounds__(256) void stream_gather_kernel(StreamArgs A) {
    const int e = static_cast<int>(blockIdx.y);
    const uint32_t b = A.group[A.first + e];
    const int start = A.sres[b].search_start;
    int have = A.capture_len[b] - start;
    if (start < 0 || have < 0) have = 0;
    if (have > A.window_len) have = A.window_len;
    const float* __restrict__ src = A.samples + static_cast<long long>(b) * A.stride + start;
    float* __restrict__ dst = A.win + static_cast<long long>(e) * A.win_stride;
    for (int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x); i < A.window_len; i += static_cast<int>(gridDim.x) * 256)
        dst[i] = i < have ? src[i] : 0.0f;
}

__global__ __launch_bounds__(256) void stream_params_kernel(StreamArgs A) {
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_search_result& r = A.sres[b];
    const float conf = stream_min_confidence(r.min_confidence, r.correlation);
    if (A.family == kStreamOfdm) {
        ria_acq_params p{};
        p.known_cfo_hz = r.known_cfo_hz; p.detect_threshold = r.detect_threshold; p.min_confidence = conf;
        p.abs_base = static_cast<uint64_t>(r.search_start);
        A.par[e] = p;
    } else {
        ria_mcdpsk_acq_params p{};
        p.known_cfo_hz = r.known_cfo_hz; p.detect_threshold = r.detect_threshold; p.min_confidence = conf;
        p.abs_base = static_cast<uint64_t>(r.search_start);
        p.last_decoded_sync = stream_rebase_last_sync(A.state[b].last_decoded_sync_pos, r.search_start);
        A.mpar[e] = p;
    }
}

__global__ __launch_bounds__(256) void stream_apply_kernel(StreamArgs A) {
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_search_result& r = A.sres[b];
    ria_search_state s = A.state[b];
    const int n_before = A.res[b].n_events;
    if (n_before < 0 || n_before >= A.max_events) return;       // an open stream has room: the close rule
    ria_stream_event ev{};
    int outcome, next_pos;
    bool delivered;
    float cfo, fading;
    int32_t window_last = kStreamNoLastSync;
    if (A.family == kStreamOfdm) {
        const ria_window_result w = A.wres[e];
        outcome = w.outcome; next_pos = w.next_pos;
        delivered = w.frame.success != 0 || w.frame.codewords_ok != 0;
        cfo = w.sync_cfo_hz; fading = w.fading_index;
        ev.frame_bytes = w.frame.frame_bytes; ev.need_samples = w.need_samples; ev.pending_total_cw = w.pending_total_cw;
        ev.success = w.frame.success; ev.codewords_ok = w.frame.codewords_ok; ev.codewords_failed = w.frame.codewords_failed;
        ev.frame_type = w.frame.frame_type;
    } else {
        const ria_mcdpsk_window_result w = A.mres[e];
        const ria_mcdpsk_acq_result a = A.macq[e];
        outcome = w.outcome; next_pos = w.next_pos;
        delivered = w.deliver != 0;
        cfo = a.cfo_hz; fading = a.fading_index;
        window_last = w.last_decoded_sync;
        ev.frame_bytes = a.frame_bytes; ev.need_samples = w.need_samples; ev.pending_total_cw = w.pending_total_cw;
        ev.success = a.success; ev.codewords_ok = a.codewords_ok; ev.codewords_failed = a.codewords_failed; ev.frame_type = a.frame_type;
    }
    ev.sync_position = r.sync_position; ev.search_start = r.search_start; ev.window_len = A.window_len; ev.outcome = outcome;
    ev.next_pos = next_pos >= 0 ? r.search_start + next_pos : -1;
    ev.delivered = delivered ? 1 : 0;
    ev.correlation = r.correlation; ev.cfo_hz = cfo; ev.fading_index = fading; ev.snr_db = r.sync_snr_db;
    // the state
    if (stream_moved(A.family, outcome)) { s.last_cfo_hz = cfo; s.fading_hint = fading; }
    s.last_decoded_sync_pos = stream_last_sync(A.family, delivered, r.sync_position, s.last_decoded_sync_pos, window_last, r.search_start);
    s.correlation_pos = stream_cursor(A.family, outcome, next_pos, r.search_start, r.sync_position, A.first_frame, s.correlation_pos);
    s.fed = stream_fed(s.fed, A.capture_len[b], s.correlation_pos);
    A.state[b] = s;
    // the event and its payload row (cleared at the start of the call)
    const size_t row = static_cast<size_t>(b) * static_cast<size_t>(A.max_events) + static_cast<size_t>(n_before);
    A.events[row] = ev;
    if (delivered) {
        int nbytes = ev.frame_bytes;
        if (nbytes > A.wframe_row) nbytes = A.wframe_row;
        if (nbytes > A.frame_row) nbytes = A.frame_row;
        const uint8_t* __restrict__ src = A.wframes + static_cast<size_t>(e) * static_cast<size_t>(A.wframe_row);
        uint8_t* __restrict__ dst = A.frames + row * static_cast<size_t>(A.frame_row);
        for (int i = 0; i < nbytes; ++i) dst[i] = src[i];
    }
    A.res[b].n_events = n_before + 1;
    A.res[b].closed = stream_close(A.family, outcome, n_before + 1, A.max_events, s.correlation_pos);
}

}  // namespace ria
