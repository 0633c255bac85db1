// ria_amd/csrc/acquire_kernels.hip.h — device side of ria_gpu_rx_acquire_batch (include/ria_gpu.h): the plan kernel that
// turns LTS detections into the round-0 work list, and the two round kernels that scatter a round's compact outputs to
// their windows and list the windows still failing at their next timing candidate (streaming_decoder.cpp:1855-1965).
//
// A work list is four parallel arrays (sample offset, ria_frame_meta, window index, candidate index) in ascending window
// order: every list is built by a block-wide scan over the previous one, so its order - and with it every result - does
// not depend on scheduling.  The demodulation and decode of a list is ria_gpu_rx_batch's own path, run on it as a batch
// of frames at offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"

namespace ria {

// timing candidates in the reference's order: the primary, then retry_deltas[] (:1858)
constexpr int kAcqCandidates = 9;
__device__ __constant__ const int kAcqDelta[kAcqCandidates] = {0, 8, -8, 16, -16, 24, -24, 32, -32};

struct AcqCtl {                  // written by the plan / next kernels, read back by the host once per round
    unsigned int n_list;         // entries of the list the next round runs
    unsigned int fault;          // a compact decode status of any round carried the work-queue fault marker
    unsigned int pad_[2];
};

struct FrameList {               // a work list of the acquire and burst rounds
    uint64_t* offset;            // sample offset from samples_dev: window * stride + candidate start
    ria_frame_meta* meta;
    uint32_t* window;
    uint8_t* state;              // acquire rounds: index into kAcqDelta; burst stage lists: 0 dropped, 1 runs the next round, 2 group complete
};

struct AcqArgs {
    const ria_lts_result* lts;   // [n_windows] detector output
    const ria_acq_params* params;
    int n_windows, window_len, frame_samples;
    long long stride;
    ria_acq_result* acq;
    AcqCtl* ctl;
    // round kernels
    FrameList cur, next;
    int n_cur;
    int round;                   // 0: primary round (scatter every entry)
    int retry;                   // 0: RIA_ACQ_NO_TIMING_RETRY or the last round - list nothing
    const uint8_t* info_c; const ria_decode_status* dst_c; const ria_frame_status* fst_c;
    int info_bytes;
    uint8_t* info_out; ria_decode_status* dst_out; ria_frame_status* fst_out;   // fst_out nullable
};

constexpr int kAcqScanThreads = 1024;

// exclusive position of this thread's flag within the block's tile, and the tile's total (all threads)
__device__ inline int acq_block_scan(bool flag, int* total) {
    __shared__ int wsum[kAcqScanThreads / 64];
    __shared__ int tile_total;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long m = __ballot(flag);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < kAcqScanThreads / 64; ++i) { const int v = wsum[i]; wsum[i] = acc; acc += v; }
        tile_total = acc;
    }
    __syncthreads();
    const int pos = wsum[w] + pre;
    *total = tile_total;
    __syncthreads();              // wsum / tile_total are reused by the next tile
    return pos;
}

__device__ inline bool acq_fits(int s, int frame_samples, int window_len) {
    return s >= 0 && static_cast<long long>(s) + frame_samples <= window_len;
}

// One block: the acceptance rule (streaming_decoder.cpp:752-771) per window, the ria_acq_result fields known before any
// decode, and the round-0 list of accepted windows at their primary candidate.
__global__ __launch_bounds__(kAcqScanThreads) void acq_plan_kernel(AcqArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_windows; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        bool acc = false;
        int start = -1;
        uint32_t burst = 0;
        if (b < A.n_windows) {
            const ria_lts_result r = A.lts[b];
            const ria_acq_params p = A.params[b];
            const bool det = r.detected != 0;
            start = det ? r.start_sample : -1;
            burst = det && r.burst_interleaved ? 1u : 0u;
            acc = det && !(r.correlation < p.min_confidence) && acq_fits(start, A.frame_samples, A.window_len);
            ria_acq_result o;
            o.detected = det ? 1 : 0;
            o.accepted = acc ? 1 : 0;
            o.sync_start = start;
            o.frame_start = acc ? start : -1;
            o.correlation = r.correlation;
            o.cfo_hz = 0.0f;
            o.delta = 0;
            o.candidates = 0;
            o.burst_interleaved = static_cast<uint8_t>(burst);
            o.reserved = 0;
            A.acq[b] = o;
        }
        int total;
        const int pos = running + acq_block_scan(acc, &total);
        if (acc) {
            const ria_acq_params p = A.params[b];
            A.next.offset[pos] = static_cast<uint64_t>(b) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(start);
            ria_frame_meta m;
            m.cfo_hz = p.known_cfo_hz;
            m.flags = burst;
            m.abs_position = p.abs_base + static_cast<uint64_t>(start);
            A.next.meta[pos] = m;
            A.next.window[pos] = static_cast<uint32_t>(b);
            A.next.state[pos] = 0;
        }
        running += total;
    }
    if (threadIdx.x == 0) { A.ctl->n_list = static_cast<unsigned>(running); A.ctl->fault = 0u; }
}

// One 64-lane wave per entry of the round's list: in round 0 every entry's outputs go to its window's slots, in later
// rounds only those of a candidate that decoded a codeword.  Every entry counts one candidate for its window.
__global__ __launch_bounds__(256) void acq_scatter_kernel(AcqArgs A) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < A.n_cur; i += gridDim.x * 4) {
        const ria_decode_status st = A.dst_c[i];
        const uint32_t w = A.cur.window[i];
        const int k = A.cur.state[i];
        const bool any = st.cw_ok[0] | st.cw_ok[1] | st.cw_ok[2] | st.cw_ok[3];
        if (A.round == 0 || any) {
            const uint8_t* src = A.info_c + static_cast<size_t>(i) * A.info_bytes;
            uint8_t* dst = A.info_out + static_cast<size_t>(w) * A.info_bytes;
            for (int q = lane; q < A.info_bytes; q += 64) dst[q] = src[q];
        }
        if (lane == 0) {
            if (st.reserved[1] == kDecodeFaultMarker) atomicOr(&A.ctl->fault, 1u);
            ria_acq_result& o = A.acq[w];
            if (A.round == 0 || any) {
                A.dst_out[w] = st;
                if (A.fst_out) A.fst_out[w] = A.fst_c[i];
                o.cfo_hz = A.fst_c[i].cfo_hz;
                o.delta = static_cast<int16_t>(kAcqDelta[k]);
                o.frame_start = o.sync_start + kAcqDelta[k];
            }
            o.candidates = static_cast<uint8_t>(o.candidates + 1);
        }
    }
}

// One block: the entries of the round whose candidate decoded nothing, each at its next candidate that fits the window,
// appended in list order (ascending window index) to the next list.
__global__ __launch_bounds__(kAcqScanThreads) void acq_next_kernel(AcqArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_cur; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        int nk = -1, s = 0;
        uint32_t w = 0;
        if (A.retry && i < A.n_cur) {
            const ria_decode_status st = A.dst_c[i];
            if (!(st.cw_ok[0] | st.cw_ok[1] | st.cw_ok[2] | st.cw_ok[3])) {
                w = A.cur.window[i];
                const int sync = A.acq[w].sync_start;
                for (int k = A.cur.state[i] + 1; k < kAcqCandidates; ++k) {
                    if (acq_fits(sync + kAcqDelta[k], A.frame_samples, A.window_len)) { nk = k; s = sync + kAcqDelta[k]; break; }
                }
            }
        }
        int total;
        const int pos = running + acq_block_scan(nk >= 0, &total);
        if (nk >= 0) {
            const ria_acq_params p = A.params[w];
            A.next.offset[pos] = static_cast<uint64_t>(w) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(s);
            ria_frame_meta m;
            m.cfo_hz = p.known_cfo_hz;
            m.flags = 0u;          // the burst marker is a one-shot of the first process() (ofdm_chirp_waveform.cpp:421-427)
            m.abs_position = p.abs_base + static_cast<uint64_t>(s);
            A.next.meta[pos] = m;
            A.next.window[pos] = w;
            A.next.state[pos] = static_cast<uint8_t>(nk);
        }
        running += total;
    }
    if (threadIdx.x == 0) A.ctl->n_list = static_cast<unsigned>(running);
}

}  // namespace ria
