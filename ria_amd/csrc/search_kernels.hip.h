// ria_amd/csrc/search_kernels.hip.h — device side of ria_gpu_search_batch (include/ria_gpu.h): StreamingDecoder::searchForSync
// (streaming_decoder.cpp:386-941) for a batch of captures, each walked from its cursor to the next accepted sync.
//
//   search_walk_kernel    one wavefront per stream: the stream's invocations back to back - feed, wait, ZC catch-up, the
//                         1000-sample RMS in the reference's ascending float32 chain (burst_gate_rms), the noise-floor tracker,
//                         the gate, the skip - until the stream ends or an invocation passes the gate; that invocation's
//                         search_start, step and thresholds are fixed and the stream is marked due.
//   search_list_kernel    one block: the streams whose detector is due, by acq_block_scan over ALL streams in ascending order.
//   search_gather_kernel  a chunk of the list: each stream's [search_start, search_start + min_search) span into a strided
//                         workspace (the reference's search_buffer, :606-609) with its known CFO and threshold, so that the
//                         three detectors run through their own launchers.
//   search_accept_kernel  one thread per listed stream: the detector's record through the waveform's mapping to SyncResult,
//                         near miss, reject, weak accept, sync_position, anti-replay, CFO sanity, SNR; the state is set.
//
// A stream's result depends on its own capture and state only: no kernel reads another stream's record, and the list's order
// comes from a scan, so chunking and scheduling change nothing.  The rules are search_rules.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "burst_kernels.hip.h"
#include "mcdpsk_acquire_kernels.hip.h"
#include "search_rules.hpp"

namespace ria {

struct SearchCtl {               // read back by the host once per round
    unsigned int n_list;         // streams whose detector is due
    unsigned int bad;            // a stream's capture_len or state is outside the call's domain
    unsigned int pad_[2];
};
struct SearchPar { float known_cfo_hz, detect_threshold; };   // one per gathered span: the detectors' per-buffer records

struct SearchArgs {
    const float* samples; long long stride;
    const int32_t* capture_len;
    ria_search_state* state;     // [n_streams], read and written in place
    ria_search_result* res;      // [n_streams]; outcome holds kSearchOpen / kSearchDue while the call runs
    const uint32_t* subset;      // nullable: the n_streams streams to search, ascending (ria_gpu_rx_stream_batch's open streams);
                                 // samples, capture_len, state and res stay indexed by stream.  Null: streams 0 .. n_streams - 1
    int n_streams, mode, cls, connected, feed_step, max_invocations, min_search;
    SearchCtl* ctl;
    uint32_t* list;              // [n_streams] due streams, ascending
    // one chunk of the list
    int first, n_chunk;
    float* span; SearchPar* par; // [n_chunk][min_search], [n_chunk]
    const ria_lts_result* lts; const ria_zc_result* zc; const ria_chirp_result* chirp;   // [n_chunk], one of them
};

constexpr int kSearchWalkWaves = 4;     // 4 x 1000 floats of LDS per workgroup: 16 KB, ten workgroups per CU

__device__ inline int search_stream(const SearchArgs& A, int i) { return A.subset ? static_cast<int>(A.subset[i]) : i; }

__device__ inline bool search_domain_ok(const ria_search_state& s, int capture_len, long long stride) {
    return capture_len >= 0 && capture_len <= kSrchMaxCapture && capture_len <= stride && s.fed >= 0 && s.fed <= capture_len &&
           s.correlation_pos >= 0 && s.correlation_pos < kSrchRing && s.reject_streak >= 0;
}

// the call's input domain, a thread per stream, ahead of the first walk: one stream outside it fails the whole call before any
// state or result is written (the walk returns at once when the flag is set)
__global__ __launch_bounds__(256) void search_check_kernel(SearchArgs A) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= A.n_streams) return;
    const int b = search_stream(A, i);
    if (!search_domain_ok(A.state[b], A.capture_len[b], A.stride)) atomicOr(&A.ctl->bad, 1u);
}

// the invocations that need no detector; `first` = the call's first round (the result is cleared).  The kernel touches the
// fields it owns one by one: a record copied whole through registers leaves its untouched words on the stack.
__global__ __launch_bounds__(64 * kSearchWalkWaves) void search_walk_kernel(SearchArgs A, int first) {
    __shared__ __attribute__((aligned(16))) float sq_all[kSearchWalkWaves][kSrchRmsLen];
    const int wave = static_cast<int>(threadIdx.x) >> 6, lane = static_cast<int>(threadIdx.x) & 63;
    const int i = static_cast<int>(blockIdx.x) * kSearchWalkWaves + wave;
    if (i >= A.n_streams || A.ctl->bad) return;
    const int b = search_stream(A, i);
    ria_search_state* sp = A.state + b;
    ria_search_result* rp = A.res + b;
    const int cap = A.capture_len[b];
    int cursor = sp->correlation_pos, fed = sp->fed, streak = sp->reject_streak;      // every lane carries the same scalars
    float noise_floor = sp->noise_floor;
    unsigned invocations = 0, waits = 0, rms_skips = 0, detector_runs = 0, moderate = 0, severe = 0;
    if (first) {
        if (lane == 0) {
            rp->search_start = 0; rp->search_len = A.min_search; rp->sync_position = -1; rp->abs_position = -1;
            rp->correlation = 0.0f; rp->known_cfo_hz = 0.0f; rp->sync_cfo_hz = 0.0f; rp->sync_snr_db = 0.0f; rp->detect_threshold = 0.0f;
            rp->min_confidence = 0.0f; rp->weak_accept = 0; rp->marker = -1; rp->root = -1;
            rp->rejects = 0; rp->near_misses = 0; rp->weak_accepts = 0; rp->replays = 0;
            rp->reserved0 = 0; rp->reserved1 = 0; rp->reserved2 = 0;
        }
    } else {
        if (rp->outcome != kSearchOpen) return;
        invocations = rp->invocations; waits = rp->waits; rms_skips = rp->rms_skips; detector_runs = rp->detector_runs;
        moderate = rp->catchups_moderate; severe = rp->catchups_severe;
    }
    const float* x = A.samples + static_cast<long long>(b) * A.stride;
    const bool zc = A.mode == kSearchZc, light = A.mode != kSearchChirp;
    int outcome = kSearchOpen, search_start = 0;
    float conf = 0.0f, weak_floor = 0.0f;
    while (outcome == kSearchOpen) {
        if (static_cast<int>(invocations) >= A.max_invocations) { outcome = kSearchLimit; break; }
        ++invocations;
        if (srch_wait(cursor, fed, A.min_search)) {
            ++waits;
            if (srch_feed(&cursor, &fed, &streak, cap, A.feed_step) == 0) outcome = kSearchNeedSamples;
            continue;
        }
        if (zc) {
            const int c = srch_catch_up(&cursor, fed, A.min_search);
            if (c == 1) ++moderate;
            if (c == 2) ++severe;
        }
        const float rms = burst_gate_rms(x + cursor, kSrchRmsLen, sq_all[wave], lane);   // cursor + min_search <= fed <= capture_len
        bool fast;
        noise_floor = srch_noise_floor(noise_floor, rms, &fast);
        const float gate = srch_gate(light, noise_floor, streak);
        if (rms < gate) {
            ++rms_skips;
            cursor = (cursor + kSrchStep) % kSrchRing;
            srch_feed(&cursor, &fed, &streak, cap, A.feed_step);
            continue;
        }
        search_start = srch_search_start(cursor, zc);
        cursor = (cursor + srch_step(zc)) % kSrchRing;
        srch_confidence(A.cls, A.connected != 0, streak, sp->fading_hint, sp->snr_hint, &conf, &weak_floor);
        ++detector_runs;
        outcome = kSearchDue;
    }
    if (lane == 0) {
        rp->outcome = outcome;
        rp->invocations = invocations; rp->waits = waits; rp->rms_skips = rms_skips; rp->detector_runs = detector_runs;
        rp->catchups_moderate = moderate; rp->catchups_severe = severe;
        if (outcome == kSearchDue) {                    // search_start .. root are the last detector run's
            rp->search_start = search_start;
            rp->min_confidence = conf;
            rp->detect_threshold = srch_detect_threshold(A.cls, conf);
            rp->known_cfo_hz = sp->last_cfo_hz;
            rp->sync_position = -1; rp->abs_position = -1;
        }
        sp->correlation_pos = cursor; sp->fed = fed; sp->reject_streak = streak; sp->noise_floor = noise_floor;
    }
}

__global__ __launch_bounds__(kAcqScanThreads) void search_list_kernel(SearchArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_streams; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        const int b = i < A.n_streams ? search_stream(A, i) : 0;
        const bool due = i < A.n_streams && A.res[b].outcome == kSearchDue;
        int total;
        const int pos = running + acq_block_scan(due, &total);
        if (due) A.list[pos] = static_cast<uint32_t>(b);
        running += total;
    }
    if (threadIdx.x == 0) A.ctl->n_list = static_cast<unsigned>(running);
}

// grid (x, n_chunk): entry blockIdx.y of the chunk; the span lies below the stream's `fed` (the walk's wait test)
__global__ __launch_bounds__(256) void search_gather_kernel(SearchArgs A) {
    const int e = static_cast<int>(blockIdx.y);
    const uint32_t b = A.list[A.first + e];
    const ria_search_result& r = A.res[b];
    const float* __restrict__ src = A.samples + static_cast<long long>(b) * A.stride + r.search_start;
    float* __restrict__ dst = A.span + static_cast<size_t>(e) * static_cast<size_t>(A.min_search);
    for (int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x); i < A.min_search; i += static_cast<int>(gridDim.x) * 256) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) { SearchPar p; p.known_cfo_hz = r.known_cfo_hz; p.detect_threshold = r.detect_threshold; A.par[e] = p; }
}

__global__ __launch_bounds__(256) void search_accept_kernel(SearchArgs A) {
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.list[A.first + e];
    ria_search_state s = A.state[b];
    ria_search_result r = A.res[b];
    // the waveform's SyncResult
    MacqSync sr;
    if (A.lts) {
        const ria_lts_result d = A.lts[e];
        sr.det = d.detected != 0; sr.start = sr.det ? d.start_sample : -1; sr.corr = d.correlation; sr.cfo = d.cfo_hz;
        r.marker = sr.det ? d.burst_interleaved : 0;
    } else if (A.zc) {
        const ria_zc_result d = A.zc[e];
        sr = macq_sync_of(d);
        r.marker = d.frame_type; r.root = d.root_detected;
    } else {
        sr = macq_sync_of(A.chirp[e]);
    }
    bool found = sr.det, weak = false;
    const bool connected = A.connected != 0;
    if (A.mode != kSearchChirp) {
        float conf, weak_floor;
        srch_confidence(A.cls, connected, s.reject_streak, s.fading_hint, s.snr_hint, &conf, &weak_floor);   // conf == r.min_confidence: the streak has not moved
        if (A.mode == kSearchZc && !found) {
            const int d = srch_near_miss(s.reject_streak, sr.corr, weak_floor);
            if (d > 0) ++r.near_misses;
            s.reject_streak += d;
        }
        if (found && sr.corr < conf) {
            if (srch_weak_accept(A.cls, connected, s.reject_streak, sr.corr, conf, weak_floor)) { weak = true; ++r.weak_accepts; }
            else { ++s.reject_streak; ++r.rejects; found = false; }
        }
        if (found) s.reject_streak = srch_streak_after_accept(s.reject_streak, weak);
    }
    r.correlation = sr.corr;
    r.weak_accept = weak ? 1 : 0;
    int outcome = kSearchOpen;
    if (found) {
        const int sync_position = (r.search_start + sr.start) % kSrchRing;
        r.sync_position = sync_position;
        r.abs_position = sync_position;                 // before the wrap the ring index is the absolute index (:862-866)
        if (srch_replay(sync_position, s.last_decoded_sync_pos)) {
            ++r.replays;
            s.correlation_pos = srch_replay_cursor(sync_position);
        } else {
            bool taken;
            r.sync_cfo_hz = srch_cfo_sanity(connected, sr.cfo, s.last_cfo_hz, &taken);
            r.sync_snr_db = srch_snr(sr.corr);
            s.snr_hint = r.sync_snr_db;
            s.last_cfo_hz = r.sync_cfo_hz;
            outcome = kSearchSyncFound;
        }
    }
    if (outcome == kSearchOpen) {
        int cursor = s.correlation_pos, fed = s.fed, streak = s.reject_streak;
        srch_feed(&cursor, &fed, &streak, A.capture_len[b], A.feed_step);
        s.correlation_pos = cursor; s.fed = fed; s.reject_streak = streak;
    }
    r.outcome = outcome;
    A.res[b] = r;
    A.state[b] = s;
}

}  // namespace ria
