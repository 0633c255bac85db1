// ria_amd/csrc/ring_kernels.hip.h — device side of ria_gpu_search_ring_batch (include/ria_gpu.h): searchForSync
// (streaming_decoder.cpp:386-941) and the whole of feedAudio (:184-291) for a batch of captures longer than the 960 000-sample
// ring buffer.  No ring is materialised: ring index p of a stream that has been fed T samples is read from the linear capture
// at ring_source(T, p) (ring_rules.hpp's closed form; a never-written index reads as the buffer's initial 0).
//
//   ring_check_kernel    the call's input domain, a thread per stream, before anything is written or any sample read.
//   ring_walk_kernel     one wavefront per stream: the stream's invocations back to back, as search_walk_kernel does, on the
//                        ring rules - the waits on the circular backlog, the cursor initialisation, the circular ZC catch-up,
//                        the 1000-sample RMS at (cursor + i) % 960000 in the reference's ascending float32 chain, the tracker,
//                        the gate, the skip, the feed with drift guard and overflow drop - until the stream ends or an
//                        invocation passes the gate.  Every loop is bounded by max_invocations.
//   ring_list_kernel     one block: the streams whose detector is due, by acq_block_scan in ascending order.
//   ring_gather_kernel   a chunk of the list: ring span [search_start, search_start + min_search) % 960000 into the strided
//                        workspace of ria_gpu_search_batch; consecutive threads read consecutive capture samples inside
//                        each of the span's (at most three) contiguous pieces.  The three detectors run on the workspace
//                        through their own launchers, unchanged.
//   ring_accept_kernel   one thread per listed stream: the acceptance rules (search_rules.hpp), sync_position modulo the
//                        ring, ringPosToAbsolute, the circular anti-replay, then the feed.
//
// The kernels touch record fields one by one: no record is copied whole through registers.  A stream's result depends on
// its own capture and state only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "ring_rules.hpp"
#include "search_kernels.hip.h"
#include "stream_kernels.hip.h"

namespace ria {

struct RingArgs {
    const float* samples; long long stride;
    const int32_t* capture_len;
    ria_ring_state* state;           // [n_streams], read and written in place
    ria_ring_search_result* res;     // [n_streams]; outcome holds kSearchOpen / kSearchDue while the call runs
    const uint32_t* subset;          // nullable: the n_streams streams to search, ascending (ria_gpu_rx_ring_batch's open streams);
                                     // samples, capture_len, state and res stay indexed by stream
    int n_streams, mode, cls, connected, feed_step, max_invocations, min_search;
    SearchCtl* ctl;
    uint32_t* list;                  // [n_streams] due streams, ascending
    int first, n_chunk;              // one chunk of the list
    float* span; SearchPar* par;     // [n_chunk][min_search], [n_chunk]
    const ria_lts_result* lts; const ria_zc_result* zc; const ria_chirp_result* chirp;   // [n_chunk], one of them
};

__device__ inline int ring_stream(const RingArgs& A, int i) { return A.subset ? static_cast<int>(A.subset[i]) : i; }

__device__ inline bool ring_domain_ok(const ria_ring_state* s, int capture_len, long long stride) {
    const long long t = s->total_fed;
    const int last = s->last_decoded_sync_pos;
    return capture_len >= 0 && capture_len <= kRingMaxCapture && capture_len <= stride && t >= 0 && t <= capture_len &&
           s->correlation_pos >= 0 && s->correlation_pos < kSrchRing && s->reject_streak >= 0 &&
           (last == INT32_MIN || (last >= 0 && last < kSrchRing));
}

__global__ __launch_bounds__(256) void ring_check_kernel(RingArgs A) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= A.n_streams) return;
    const int b = ring_stream(A, i);
    if (!ring_domain_ok(A.state + b, A.capture_len[b], A.stride)) atomicOr(&A.ctl->bad, 1u);
}

// ring index p of a stream fed t samples (t <= capture_len <= stride, by the domain check): its capture sample, or the
// unwritten ring's 0
__device__ __forceinline__ float ring_sample(const float* __restrict__ x, long long t, int p) {
    const long long k = ring_source(t, p);
    return (k >= 0 && k < t) ? x[k] : 0.0f;
}

// burst_gate_rms's chain on buffer_[(cursor + i) % 960000], i < 1000
__device__ inline float ring_rms(const float* __restrict__ x, long long t, int cursor, float* __restrict__ sq, int lane) {
    for (int i = lane; i < kSrchRmsLen; i += 64) {
        int p = cursor + i;
        if (p >= kSrchRing) p -= kSrchRing;
        const float v = ring_sample(x, t, p);
        sq[i] = v * v;
    }
    wave_sync();
    float rms = 0.0f;
    if (lane == 0) {
        float acc = 0.0f;
        for (int i = 0; i < kSrchRmsLen; i += 4) {
            const float4 q = *reinterpret_cast<const float4*>(sq + i);
            acc += q.x; acc += q.y; acc += q.z; acc += q.w;
        }
        rms = sqrtf(acc / static_cast<float>(kSrchRmsLen));
    }
    wave_sync();
    return __shfl(rms, 0);
}

__global__ __launch_bounds__(64 * kSearchWalkWaves) void ring_walk_kernel(RingArgs A, int first) {
    __shared__ __attribute__((aligned(16))) float sq_all[kSearchWalkWaves][kSrchRmsLen];
    const int wave = static_cast<int>(threadIdx.x) >> 6, lane = static_cast<int>(threadIdx.x) & 63;
    const int i = static_cast<int>(blockIdx.x) * kSearchWalkWaves + wave;
    if (i >= A.n_streams || A.ctl->bad) return;
    const int b = ring_stream(A, i);
    ria_ring_state* sp = A.state + b;
    ria_ring_search_result* rp = A.res + b;
    const long long cap = A.capture_len[b];
    int cursor = sp->correlation_pos, streak = sp->reject_streak;      // every lane carries the same scalars
    long long fed = sp->total_fed;
    float noise_floor = sp->noise_floor;
    unsigned int ov_events = sp->overflow_events;
    unsigned long long ov_total = sp->overflow_dropped;
    unsigned invocations = 0, waits = 0, rms_skips = 0, detector_runs = 0, moderate = 0, severe = 0, cursor_inits = 0;
    RingFeedCounts fc{0u, 0u, 0ull};
    if (first) {
        if (lane == 0) {
            rp->search_start = 0; rp->search_len = A.min_search; rp->sync_position = -1; rp->abs_position = -1;
            rp->correlation = 0.0f; rp->known_cfo_hz = 0.0f; rp->sync_cfo_hz = 0.0f; rp->sync_snr_db = 0.0f; rp->detect_threshold = 0.0f;
            rp->min_confidence = 0.0f; rp->weak_accept = 0; rp->marker = -1; rp->root = -1;
            rp->rejects = 0; rp->near_misses = 0; rp->weak_accepts = 0; rp->replays = 0;
            rp->reserved0 = 0; rp->reserved1 = 0; rp->reserved2 = 0;
            rp->abs_search_start = 0; rp->span_wraps = 0;
        }
    } else {
        if (rp->outcome != kSearchOpen) return;
        invocations = rp->invocations; waits = rp->waits; rms_skips = rp->rms_skips; detector_runs = rp->detector_runs;
        moderate = rp->catchups_moderate; severe = rp->catchups_severe; cursor_inits = rp->cursor_inits;
        fc.overflows = rp->overflows; fc.drift_snaps = rp->drift_snaps; fc.overflow_dropped = rp->overflow_dropped;
    }
    const float* x = A.samples + static_cast<long long>(b) * A.stride;
    const bool zc = A.mode == kSearchZc, light = A.mode != kSearchChirp;
    int outcome = kSearchOpen, search_start = 0;
    float conf = 0.0f, weak_floor = 0.0f;
    while (outcome == kSearchOpen) {
        if (static_cast<int>(invocations) >= A.max_invocations) { outcome = kSearchLimit; break; }
        ++invocations;
        if (ring_wait(&cursor, fed, A.min_search, &cursor_inits)) {
            ++waits;
            if (ring_feed(&cursor, &fed, &streak, &ov_events, &ov_total, &fc, cap, A.feed_step) == 0) outcome = kSearchNeedSamples;
            continue;
        }
        if (zc) {
            const int c = ring_catch_up(&cursor, ring_write_pos(fed), A.min_search);
            if (c == 1) ++moderate;
            if (c == 2) ++severe;
        }
        const float rms = ring_rms(x, fed, cursor, sq_all[wave], lane);
        bool fast;
        noise_floor = srch_noise_floor(noise_floor, rms, &fast);
        const float gate = srch_gate(light, noise_floor, streak);
        if (rms < gate) {
            ++rms_skips;
            cursor = (cursor + kSrchStep) % kSrchRing;
            ring_feed(&cursor, &fed, &streak, &ov_events, &ov_total, &fc, cap, A.feed_step);
            continue;
        }
        search_start = ring_search_start(cursor, fed, zc);
        cursor = (cursor + srch_step(zc)) % kSrchRing;
        srch_confidence(A.cls, A.connected != 0, streak, sp->fading_hint, sp->snr_hint, &conf, &weak_floor);
        ++detector_runs;
        outcome = kSearchDue;
    }
    if (lane == 0) {
        rp->outcome = outcome;
        rp->invocations = invocations; rp->waits = waits; rp->rms_skips = rms_skips; rp->detector_runs = detector_runs;
        rp->catchups_moderate = moderate; rp->catchups_severe = severe; rp->cursor_inits = cursor_inits;
        rp->overflows = fc.overflows; rp->drift_snaps = fc.drift_snaps; rp->overflow_dropped = fc.overflow_dropped;
        if (outcome == kSearchDue) {                    // search_start .. root are the last detector run's
            rp->search_start = search_start;
            rp->abs_search_start = ring_pos_to_absolute(fed, search_start);
            rp->span_wraps = ring_span_wraps(search_start, fed, A.min_search) ? 1u : 0u;
            rp->min_confidence = conf;
            rp->detect_threshold = srch_detect_threshold(A.cls, conf);
            rp->known_cfo_hz = sp->last_cfo_hz;
            rp->sync_position = -1; rp->abs_position = -1;
        }
        sp->correlation_pos = cursor; sp->total_fed = fed; sp->reject_streak = streak; sp->noise_floor = noise_floor;
        sp->overflow_events = ov_events; sp->overflow_dropped = ov_total;
    }
}

__global__ __launch_bounds__(kAcqScanThreads) void ring_list_kernel(RingArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_streams; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        const int b = i < A.n_streams ? ring_stream(A, i) : 0;
        const bool due = i < A.n_streams && A.res[b].outcome == kSearchDue;
        int total;
        const int pos = running + acq_block_scan(due, &total);
        if (due) A.list[pos] = static_cast<uint32_t>(b);
        running += total;
    }
    if (threadIdx.x == 0) A.ctl->n_list = static_cast<unsigned>(running);
}

// grid (x, n_chunk): entry blockIdx.y of the chunk
__global__ __launch_bounds__(256) void ring_gather_kernel(RingArgs A) {
    const int e = static_cast<int>(blockIdx.y);
    const uint32_t b = A.list[A.first + e];
    const ria_ring_search_result* r = A.res + b;
    const long long t = A.state[b].total_fed;
    const int start = r->search_start;
    const float* __restrict__ x = A.samples + static_cast<long long>(b) * A.stride;
    float* __restrict__ dst = A.span + static_cast<size_t>(e) * static_cast<size_t>(A.min_search);
    for (int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x); i < A.min_search; i += static_cast<int>(gridDim.x) * 256) {
        int p = start + i;                              // start < 960000 and i < min_search <= 120000
        if (p >= kSrchRing) p -= kSrchRing;
        dst[i] = ring_sample(x, t, p);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { A.par[e].known_cfo_hz = r->known_cfo_hz; A.par[e].detect_threshold = r->detect_threshold; }
}

__global__ __launch_bounds__(256) void ring_accept_kernel(RingArgs A) {
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.list[A.first + e];
    ria_ring_state* sp = A.state + b;
    ria_ring_search_result* rp = A.res + b;
    // the waveform's SyncResult
    MacqSync sr;
    if (A.lts) {
        const ria_lts_result* d = A.lts + e;
        sr.det = d->detected != 0; sr.start = sr.det ? d->start_sample : -1; sr.corr = d->correlation; sr.cfo = d->cfo_hz;
        rp->marker = sr.det ? d->burst_interleaved : 0;
    } else if (A.zc) {
        const ria_zc_result d = A.zc[e];
        sr = macq_sync_of(d);
        rp->marker = d.frame_type; rp->root = d.root_detected;
    } else {
        sr = macq_sync_of(A.chirp[e]);
    }
    bool found = sr.det, weak = false;
    const bool connected = A.connected != 0;
    int streak = sp->reject_streak;
    if (A.mode != kSearchChirp) {
        float conf, weak_floor;
        srch_confidence(A.cls, connected, streak, sp->fading_hint, sp->snr_hint, &conf, &weak_floor);   // conf == min_confidence: the streak has not moved
        if (A.mode == kSearchZc && !found) {
            const int d = srch_near_miss(streak, sr.corr, weak_floor);
            if (d > 0) rp->near_misses += 1;
            streak += d;
        }
        if (found && sr.corr < conf) {
            if (srch_weak_accept(A.cls, connected, streak, sr.corr, conf, weak_floor)) { weak = true; rp->weak_accepts += 1; }
            else { ++streak; rp->rejects += 1; found = false; }
        }
        if (found) streak = srch_streak_after_accept(streak, weak);
    }
    rp->correlation = sr.corr;
    rp->weak_accept = weak ? 1 : 0;
    int outcome = kSearchOpen, cursor = sp->correlation_pos;
    long long fed = sp->total_fed;
    if (found) {
        const int sync_position = ring_sync_position(rp->search_start, sr.start);
        rp->sync_position = sync_position;
        rp->abs_position = ring_pos_to_absolute(fed, sync_position);
        if (srch_replay(sync_position, sp->last_decoded_sync_pos)) {
            rp->replays += 1;
            cursor = srch_replay_cursor(sync_position);
        } else {
            bool taken;
            const float cfo = srch_cfo_sanity(connected, sr.cfo, sp->last_cfo_hz, &taken);
            const float snr = srch_snr(sr.corr);
            rp->sync_cfo_hz = cfo; rp->sync_snr_db = snr;
            sp->snr_hint = snr; sp->last_cfo_hz = cfo;
            outcome = kSearchSyncFound;
        }
    }
    if (outcome == kSearchOpen) {
        unsigned int ov_events = sp->overflow_events;
        unsigned long long ov_total = sp->overflow_dropped;
        RingFeedCounts fc{rp->overflows, rp->drift_snaps, rp->overflow_dropped};
        ring_feed(&cursor, &fed, &streak, &ov_events, &ov_total, &fc, A.capture_len[b], A.feed_step);
        rp->overflows = fc.overflows; rp->drift_snaps = fc.drift_snaps; rp->overflow_dropped = fc.overflow_dropped;
        sp->overflow_events = ov_events; sp->overflow_dropped = ov_total; sp->total_fed = fed;
    }
    sp->correlation_pos = cursor; sp->reject_streak = streak;
    rp->outcome = outcome;
}

// ------------------------------------------------------------------------------------------------ the stream loop on the ring
// Device side of ria_gpu_rx_ring_batch: stream_kernels.hip.h's five kernels on ria_ring_state / ria_ring_search_result, with
// the window leg in absolute indices (ring_rules.hpp).  Nothing here is receiver arithmetic: lists, copies and rules.
struct RingStreamArgs {
    const float* samples; long long stride;
    const int32_t* capture_len;
    ria_ring_state* state;               // [n_streams], read and written in place
    const ria_ring_search_result* sres;  // [n_streams], by stream: the last search leg's
    ria_ring_stream_result* res;         // [n_streams]
    ria_stream_event* events;            // [n_streams][max_events]
    uint8_t* frames; int frame_row;      // [n_streams][max_events][frame_row]
    int n_streams, mode, family, full, first_frame, max_events;
    StreamCtl* ctl;
    uint32_t* found; int32_t* found_len; // [n_streams] behind ctl: found streams, ascending, and their window lengths
    uint32_t* open;                      // [n_streams] open streams, ascending
    uint32_t* group;                     // [n_streams] found streams of one window length, ascending
    int n_open, n_found;
    int window_len, first, n_chunk;      // one chunk of a group
    float* win; long long win_stride;    // [n_chunk][win_stride]
    ria_acq_params* par; ria_mcdpsk_acq_params* mpar;
    const ria_window_result* wres;
    const ria_mcdpsk_window_result* mres; const ria_mcdpsk_acq_result* macq;
    const uint8_t* wframes; int wframe_row;
};

__global__ __launch_bounds__(256) void ring_stream_init_kernel(RingStreamArgs A) {
    const int b = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (b >= A.n_streams) return;
    ria_ring_stream_result r{};
    r.mode = A.mode;
    A.res[b] = r;
}

__global__ __launch_bounds__(kAcqScanThreads) void ring_stream_list_kernel(RingStreamArgs A, int what) {
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
                const ria_ring_search_result* r = A.sres + b;
                ria_ring_stream_result* o = A.res + b;
                o->search_legs += 1;
                o->invocations += r->invocations; o->waits += r->waits; o->rms_skips += r->rms_skips; o->detector_runs += r->detector_runs;
                o->rejects += r->rejects; o->near_misses += r->near_misses; o->weak_accepts += r->weak_accepts; o->replays += r->replays;
                o->catchups_moderate += r->catchups_moderate; o->catchups_severe += r->catchups_severe;
                o->overflow_dropped += r->overflow_dropped; o->overflows += r->overflows; o->drift_snaps += r->drift_snaps;
                o->cursor_inits += r->cursor_inits;
                flag = r->outcome == kSearchSyncFound;
                if (flag && r->span_wraps) { flag = false; o->closed = kStreamSpanLost; }
                else if (flag) {
                    const long long left = static_cast<long long>(A.capture_len[b]) - r->abs_search_start;
                    len = static_cast<int>(left < A.full ? left : A.full);
                } else o->closed = r->outcome;
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

// grid (x, n_chunk): window blockIdx.y of the chunk, [abs_search_start, abs_search_start + window_len) of the capture; the
// copy is bounded by the capture, and what lies past it would be zero
__global__ __launch_bounds__(256) void ring_stream_gather_kernel(RingStreamArgs A) {
    const int e = static_cast<int>(blockIdx.y);
    const uint32_t b = A.group[A.first + e];
    const long long start = A.sres[b].abs_search_start;
    long long have = static_cast<long long>(A.capture_len[b]) - start;
    if (start < 0 || have < 0) have = 0;
    if (have > A.window_len) have = A.window_len;
    const float* __restrict__ src = A.samples + static_cast<long long>(b) * A.stride + (start < 0 ? 0 : start);
    float* __restrict__ dst = A.win + static_cast<long long>(e) * A.win_stride;
    for (int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x); i < A.window_len; i += static_cast<int>(gridDim.x) * 256)
        dst[i] = i < have ? src[i] : 0.0f;
}

__global__ __launch_bounds__(256) void ring_stream_params_kernel(RingStreamArgs A) {
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_ring_search_result* r = A.sres + b;
    const float conf = stream_min_confidence(r->min_confidence, r->correlation);
    if (A.family == kStreamOfdm) {
        ria_acq_params p{};
        p.known_cfo_hz = r->known_cfo_hz; p.detect_threshold = r->detect_threshold; p.min_confidence = conf;
        p.abs_base = static_cast<uint64_t>(r->abs_search_start);
        A.par[e] = p;
    } else {
        ria_mcdpsk_acq_params p{};
        p.known_cfo_hz = r->known_cfo_hz; p.detect_threshold = r->detect_threshold; p.min_confidence = conf;
        p.abs_base = static_cast<uint64_t>(r->abs_search_start);
        p.last_decoded_sync = ring_rebase_last_sync(A.state[b].last_decoded_sync_pos, r->search_start);
        A.mpar[e] = p;
    }
}

__global__ __launch_bounds__(256) void ring_stream_apply_kernel(RingStreamArgs A) {
    const int e = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (e >= A.n_chunk) return;
    const uint32_t b = A.group[A.first + e];
    const ria_ring_search_result* r = A.sres + b;
    ria_ring_state* sp = A.state + b;
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
    const long long abs_start = r->abs_search_start, abs_sync = r->abs_position;
    const long long abs_cursor = ring_abs_cursor(A.family, outcome, next_pos, abs_start, abs_sync, A.first_frame);
    ev.sync_position = static_cast<int32_t>(abs_sync); ev.search_start = static_cast<int32_t>(abs_start); ev.window_len = A.window_len;
    ev.outcome = outcome;
    ev.next_pos = next_pos >= 0 ? static_cast<int32_t>(abs_start + next_pos) : -1;
    ev.delivered = delivered ? 1 : 0;
    ev.correlation = r->correlation; ev.cfo_hz = cfo; ev.fading_index = fading; ev.snr_db = r->sync_snr_db;
    // the state
    if (stream_moved(A.family, outcome)) { sp->last_cfo_hz = cfo; sp->fading_hint = fading; }
    sp->last_decoded_sync_pos = ring_last_sync(A.family, delivered, r->sync_position, sp->last_decoded_sync_pos, window_last, r->search_start);
    if (abs_cursor >= 0) {
        sp->correlation_pos = ring_mod(abs_cursor);
        sp->total_fed = ring_stream_fed(sp->total_fed, A.capture_len[b], abs_cursor);
    }
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
    A.res[b].closed = ring_stream_close(A.family, outcome, n_before + 1, A.max_events);
}

}  // namespace ria
