// ria_amd/csrc/mcdpsk_acquire_kernels.hip.h — device side of ria_gpu_mcdpsk_acquire_batch (include/ria_gpu.h): the plan
// kernel that turns ZC / dual-chirp detections into the round-0 work list, the decodeMCDPSKFrame stage over a round's
// list (streaming_decoder.cpp:2595-2819) and the kernel that lists the windows still searching at their next handshake
// candidate (:1646-1797).
//
// A work list is five parallel arrays (sample offset, CFO, window index, candidate index, bits per symbol) in ascending
// window order: every list is built by a block-wide scan over the previous one (acq_block_scan of acquire_kernels.hip.h),
// so its order - and with it every result - does not depend on scheduling.  A round demodulates its list with the MC-DPSK
// demodulator's offset-list form, decodes CW0 of every entry (round A), parses the headers (one wave per entry), decodes
// CW1..n-1 of the entries whose header asks for them (round B, a compact list of (entry, codeword) rows) and reassembles.
//
// With channel interleaving (RIA_MACQ_CHANNEL_INTERLEAVE, :2614-2623, :2651-2672, :2741) round A2 sits between round A and
// the headers: the entries whose raw CW0 is not (ok and magic) are listed, their CW0 is decoded again through
// ChannelInterleaver::deinterleave (row[i] = llr[(i * step) % 648]) and a merge puts the winning CW0 where the header
// kernel reads it; the entry's flag then makes round B, and the chase stage's sum gather, apply the same permutation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "recovery_kernels.hip.h"

namespace ria {

// candidates in the reference's order: 0 the primary, 1 the alternate modulation at the same start (:1646-1690), then
// retry_deltas[] (:1694) each with the primary (even) and the alternate (odd) modulation
constexpr int kMacqCandidates = 26, kMacqLdpcBlock = 648, kMacqCwBytes = 20;
__device__ __constant__ const int kMacqDelta[12] = {8, -8, 16, -16, 24, -24, 32, -32, 48, -48, 64, -64};
__device__ __forceinline__ int macq_delta(int k) { return k < 2 ? 0 : kMacqDelta[(k - 2) >> 1]; }
__device__ __forceinline__ bool macq_alt(int k) { return k == 1 || (k >= 2 && ((k - 2) & 1)); }

struct MacqCtl {                 // read back by the host twice per round
    unsigned int n_list;         // entries of the list the next round runs
    unsigned int n_rows;         // codeword rows of this round's round B
    unsigned int dup;            // HARQ calls: two windows claimed one cache, or a cache id the pool does not have
    unsigned int n_sums;         // HARQ calls: combined sums this round decodes
};
struct MacqCiCtl {               // channel interleaving: a control word of its own, so that the other reads stay what they were
    unsigned int n_a2;           // entries of this round's A2 list
};

struct MacqList {
    uint64_t* offset;            // sample offset from samples_dev: window * stride + candidate start
    float* cfo;
    uint32_t* window;
    uint8_t* cand;               // candidate index (macq_delta / macq_alt)
    uint8_t* bps;                // 1 DBPSK, 2 DQPSK
};

struct MacqArgs {
    const ria_zc_result* zc;     // one of the two detector outputs, [n_windows]
    const ria_chirp_result* chirp;
    const ria_mcdpsk_acq_params* params;
    int n_windows, window_len, frame_len;
    long long stride;
    int connected;               // the connected CFO rule (ZC path)
    int retry;                   // RIA_MACQ_DISCONNECTED without RIA_MACQ_NO_RETRY: the handshake fallbacks
    int bps;                     // primary bits per symbol
    ria_mcdpsk_acq_result* acq;
    MacqCtl* ctl;
    // one round
    MacqList cur, next;
    int n_cur;
    const ria_mcdpsk_status* mst;        // [n_cur] demodulator status
    const float* llr; int llr_ws;        // [n_cur][llr_ws] soft bits
    float* rows;                         // [rows][648] codeword LLRs gathered for the robust decoder
    uint32_t* row_entry; uint8_t* row_cw;   // round B rows
    const uint8_t* out_a; const uint8_t* ok_a;   // round A: [n_cur][dec_bytes], [n_cur]
    const uint8_t* out_b; const uint8_t* ok_b;   // round B: [n_rows][dec_bytes], [n_rows]
    int dec_bytes;                       // ceil(ldpc_k / 8) = 21 at R1/4
    int* hdr_total;                      // [n_cur] total_cw of a valid CW0 header, 0 = none
    int* need_rows;                      // [n_cur] round-B rows of the entry
    uint32_t* row_base;                  // [n_cur] first round-B row of the entry
    uint8_t* done;                       // [n_cur] the window stops searching
    const uint16_t* crc_bit; const uint16_t* crc_init;
    uint8_t* frame_out; int frame_row;   // [n_windows][frame_row]
    float* llr_out; int llr_stride;      // nullable
    // channel interleaving; ci_flag null = off
    int ci_step;                         // ChannelInterleaver(interleaver_bits, 648)'s step
    uint8_t* ci_flag;                    // [n_cur] kMacqCiDeint | kMacqCiTried
    uint32_t* ci_list;                   // [n_a2] round A2's entries, ascending
    MacqCiCtl* ci_ctl;
};
constexpr uint8_t kMacqCiDeint = 1, kMacqCiTried = 2;   // cw0_deinterleaved / the de-interleaved CW0 decode ran

__device__ __forceinline__ size_t macq_ci_src(size_t j, int step) { return (j * static_cast<size_t>(step)) % kMacqLdpcBlock; }

__device__ inline bool macq_fits(int s, int frame_len, int window_len) {
    return s >= 0 && static_cast<long long>(s) + frame_len <= window_len;
}

// MCDPSKWaveform::detectSync / detectDataSync's SyncResult (mc_dpsk_waveform.cpp:176-292) from the detector's record;
// start is -1 when nothing was detected.  Shared with search_accept_kernel (search_kernels.hip.h).
struct MacqSync { bool det; int start; float corr, cfo; };
__device__ __forceinline__ MacqSync macq_sync_of(const ria_chirp_result& r) {
    MacqSync o;
    o.det = r.success != 0;
    o.start = o.det ? r.down_chirp_start + 24000 + 4800 : -1;
    o.corr = r.up_correlation > r.down_correlation ? r.up_correlation : r.down_correlation;   // std::max(up, down)
    o.cfo = r.cfo_hz;
    return o;
}
__device__ __forceinline__ MacqSync macq_sync_of(const ria_zc_result& r) {
    MacqSync o;
    o.det = r.detected != 0;
    o.start = o.det ? r.start_sample : -1;
    o.corr = r.correlation;
    o.cfo = r.cfo_hz;
    return o;
}

// One block: detection results -> ria_mcdpsk_acq_result fields known before any decode, the acceptance rule and the CFO
// every candidate of the window is demodulated with (mc_dpsk_waveform.cpp:176-292, streaming_decoder.cpp:903-917), and the
// round-0 list of accepted windows at their primary candidate.
__global__ __launch_bounds__(kAcqScanThreads) void macq_plan_kernel(MacqArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_windows; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        bool acc = false;
        int start = -1;
        float cfo = 0.0f;
        if (b < A.n_windows) {
            const ria_mcdpsk_acq_params p = A.params[b];
            const MacqSync sr = A.chirp ? macq_sync_of(A.chirp[b]) : macq_sync_of(A.zc[b]);
            const bool det = sr.det;
            const float corr = sr.corr;
            start = sr.start;
            cfo = sr.cfo;
            if (A.connected && fabs_(p.known_cfo_hz) > 0.01f && fabs_(cfo - p.known_cfo_hz) > 1.0f) cfo = p.known_cfo_hz;
            acc = det && !(corr < p.min_confidence) && macq_fits(start, A.frame_len, A.window_len);
            ria_mcdpsk_acq_result o;
            o.detected = det ? 1 : 0;
            o.accepted = acc ? 1 : 0;
            o.sync_start = start;
            o.frame_start = acc ? start : -1;
            o.correlation = corr;
            o.cfo_hz = acc ? cfo : 0.0f;
            o.fading_index = 0.0f;
            o.delta = 0;
            o.modulation = static_cast<uint8_t>(A.bps == 2 ? RIA_MOD_DQPSK : RIA_MOD_DBPSK);
            o.candidates = 0;
            o.success = 0; o.codewords_ok = 0; o.codewords_failed = 0; o.frame_type = 0x10;
            o.header_total_cw = 0; o.frame_bytes = 0; o.n_llr = 0;
            o.reserved[0] = o.reserved[1] = o.reserved[2] = o.reserved[3] = 0;
            A.acq[b] = o;
        }
        int total;
        const int pos = running + acq_block_scan(acc, &total);
        if (acc) {
            A.next.offset[pos] = static_cast<uint64_t>(b) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(start);
            A.next.cfo[pos] = cfo;
            A.next.window[pos] = static_cast<uint32_t>(b);
            A.next.cand[pos] = 0;
            A.next.bps[pos] = static_cast<uint8_t>(A.bps);
        }
        running += total;
    }
    if (threadIdx.x == 0) { A.ctl->n_list = static_cast<unsigned>(running); A.ctl->n_rows = 0u; }
}

// rows of 648 LLRs for the robust decoder: round A (row_entry null) row r = CW0 of entry r, round B the listed rows,
// de-interleaved for the entries whose CW0 was (:2741, :2764)
__global__ __launch_bounds__(256) void macq_gather_kernel(MacqArgs A, int n_rows) {
    const size_t total = static_cast<size_t>(n_rows) * kMacqLdpcBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
        const size_t r = i / kMacqLdpcBlock, j = i - r * kMacqLdpcBlock;
        const size_t e = A.row_entry ? A.row_entry[r] : r;
        const size_t cw = A.row_entry ? A.row_cw[r] : 0;
        const size_t src = (A.ci_flag && A.row_entry && (A.ci_flag[e] & kMacqCiDeint)) ? macq_ci_src(j, A.ci_step) : j;
        A.rows[i] = A.llr[e * A.llr_ws + cw * kMacqLdpcBlock + src];
    }
}

// ---- round A2 (channel interleaving)
// One block: the entries whose raw CW0 is not (ok and magic) and that hold a codeword, ascending, and every entry's flag.
__global__ __launch_bounds__(kAcqScanThreads) void macq_ci_list_kernel(MacqArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_cur; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        bool f = false;
        if (i < A.n_cur) {
            const uint8_t* d = A.out_a + static_cast<size_t>(i) * A.dec_bytes;
            f = A.mst[i].n_llr >= kMacqLdpcBlock && !(A.ok_a[i] && d[0] == 0x55 && d[1] == 0x4C);
            A.ci_flag[i] = f ? kMacqCiTried : 0;
        }
        int total;
        const int pos = running + acq_block_scan(f, &total);
        if (f) A.ci_list[pos] = static_cast<uint32_t>(i);
        running += total;
    }
    if (threadIdx.x == 0) A.ci_ctl->n_a2 = static_cast<unsigned>(running);
}
// row r = deinterleave(CW0 of entry ci_list[r])
__global__ __launch_bounds__(256) void macq_ci_gather_kernel(MacqArgs A, int n_a2) {
    const size_t total = static_cast<size_t>(n_a2) * kMacqLdpcBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
        const size_t r = i / kMacqLdpcBlock, j = i - r * kMacqLdpcBlock;
        A.rows[i] = A.llr[static_cast<size_t>(A.ci_list[r]) * A.llr_ws + macq_ci_src(j, A.ci_step)];
    }
}
// One thread per A2 row: a de-interleaved CW0 that is ok with the magic becomes the entry's CW0 (:2666-2670); otherwise the
// raw one stays, which the header kernel rejects as before.
__global__ __launch_bounds__(256) void macq_ci_merge_kernel(MacqArgs A, int n_a2, uint8_t* out_a, uint8_t* ok_a, const uint8_t* out_a2, const uint8_t* ok_a2) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n_a2; r += gridDim.x * 256) {
        const uint8_t* d = out_a2 + static_cast<size_t>(r) * A.dec_bytes;
        if (!(ok_a2[r] && d[0] == 0x55 && d[1] == 0x4C)) continue;
        const uint32_t e = A.ci_list[r];
        uint8_t* dst = out_a + static_cast<size_t>(e) * A.dec_bytes;
        for (int q = 0; q < A.dec_bytes; ++q) dst[q] = d[q];
        ok_a[e] = 1;
        A.ci_flag[e] = kMacqCiTried | kMacqCiDeint;
    }
}

// ---- ChannelInterleaver::interleave(Bytes) over rows of 81 coded bytes (ldpc_decoder.cpp:627-650): bit i of a row, MSB
// first, goes to bit (i * step) % 648.  One wave per codeword: the row is staged in LDS, each lane assembles output bytes
// in a register from the bits at p * step_inv (step * step_inv = 1 mod 648) and stores them.
constexpr int kMacqCwCoded = kMacqLdpcBlock / 8;   // 81
__global__ __launch_bounds__(256) void macq_interleave_kernel(const uint8_t* in, uint8_t* out, int n_cw, int step_inv) {
    __shared__ uint8_t stage[4][kMacqCwCoded + 3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int base = blockIdx.x * 4; base < n_cw; base += gridDim.x * 4) {   // the same trip count for the block's four waves
        const int cw = base + wv;
        if (cw < n_cw)
            for (int q = lane; q < kMacqCwCoded; q += 64) stage[wv][q] = in[static_cast<size_t>(cw) * kMacqCwCoded + q];
        __syncthreads();
        if (cw < n_cw)
            for (int q = lane; q < kMacqCwCoded; q += 64) {
                unsigned v = 0;
                for (int b = 0; b < 8; ++b) {
                    const int i = ((q * 8 + b) * step_inv) % kMacqLdpcBlock;
                    v = (v << 1) | ((stage[wv][i >> 3] >> (7 - (i & 7))) & 1u);
                }
                out[static_cast<size_t>(cw) * kMacqCwCoded + q] = static_cast<uint8_t>(v);
            }
        __syncthreads();
    }
}

// One 64-lane wave per entry: CW0's magic, parseHeader with both CRC forms (frame_v2.cpp:1195-1252, rec_parse_header), the
// CONNECT guard (:2713-2722) and the number of round-B rows (CW1..total_cw-1 when the soft bits hold total_cw codewords).
__global__ __launch_bounds__(256) void macq_header_kernel(MacqArgs A) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < A.n_cur; i += gridDim.x * 4) {
        const int avail = A.mst[i].n_llr / kMacqLdpcBlock;
        const uint8_t* d = A.out_a + static_cast<size_t>(i) * A.dec_bytes;
        int total = 0;
        if (avail >= 1 && A.ok_a[i] && d[0] == 0x55 && d[1] == 0x4C) {
            RecCtx x{};
            x.crc_bit = A.crc_bit; x.crc_init = A.crc_init; x.lane = lane;
            bool ctl; int plen;
            if (rec_parse_header(x, d, kMacqCwBytes, &ctl, &plen)) {
                total = ctl ? 1 : d[12];
                const int t = d[2];
                if ((t == 0x12 || t == 0x13 || t == 0x14) && total < 3) total = 0;   // max(2, calculateCodewords(25, R1/4))
            }
        }
        if (lane == 0) {
            A.hdr_total[i] = total;
            A.need_rows[i] = (total > 1 && avail >= total) ? total - 1 : 0;
        }
    }
}

// One block: the round-B row list (entries in list order, codewords ascending) and its length.
__global__ __launch_bounds__(kAcqScanThreads) void macq_rows_kernel(MacqArgs A) {
    // an entry has at most 15 rows: the exclusive prefix sum of the row counts is the sum, over r, of the flag scans of
    // (rows > r)
    int running = 0;
    for (int base = 0; base < A.n_cur; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        const int need = i < A.n_cur ? A.need_rows[i] : 0;
        int pos = 0, tile = 0;
        for (int r = 0; r < 16; ++r) {            // exclusive prefix sum of `need` = sum over r of the scan of (need > r)
            int t;
            pos += acq_block_scan(need > r, &t);
            tile += t;
        }
        if (i < A.n_cur) {
            const int first = running + pos;
            A.row_base[i] = static_cast<uint32_t>(first);
            for (int r = 0; r < need; ++r) { A.row_entry[first + r] = static_cast<uint32_t>(i); A.row_cw[first + r] = static_cast<uint8_t>(1 + r); }
        }
        running += tile;
    }
    if (threadIdx.x == 0) A.ctl->n_rows = static_cast<unsigned>(running);
}

// One wave per entry: the entry's DecodeResult (decodeMCDPSKFrame's tail, CodewordStatus::reassemble, reassembleCodewords
// frame_v2.cpp:959-989) and, for the primary or a full success, the window's outputs.  Every entry counts one candidate.
__global__ __launch_bounds__(256) void macq_finish_kernel(MacqArgs A) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < A.n_cur; i += gridDim.x * 4) {
        const int T = A.hdr_total[i];
        const int n_llr = A.mst[i].n_llr, avail = n_llr / kMacqLdpcBlock;
        const uint8_t* d0 = A.out_a + static_cast<size_t>(i) * A.dec_bytes;
        const uint32_t w = A.cur.window[i];
        const int k = A.cur.cand[i];
        int success = 0, ok = 0, failed = 0, ftype = 0x10, nbytes = 0;
        bool full = false;
        if (T > 0) {
            ftype = d0[2]; ok = 1;
            if (T == 1) { success = 1; nbytes = kMacqCwBytes; }
            else if (avail < T) { nbytes = kMacqCwBytes; }
            else {
                const uint32_t rb = A.row_base[i];
                for (int r = 0; r < T - 1; ++r) { if (A.ok_b[rb + r]) ++ok; else ++failed; }
                if (failed == 0) { success = 1; full = true; }
            }
        }
        const bool report = k == 0 || success;
        if (report) {
            uint8_t* fo = A.frame_out + static_cast<size_t>(w) * A.frame_row;
            if (full) {
                // CW0's 20 bytes, then CW1.. without their 0xD5 marker + index, up to the header's frame size
                const uint32_t rb = A.row_base[i];
                const uint8_t* out_b = A.out_b;
                const int dec_bytes = A.dec_bytes;
                nbytes = rec_reassemble_cws(rec_is_control(ftype), (d0[13] << 8) | d0[14],
                                            [&](int c) { return c == 0 ? d0 : out_b + static_cast<size_t>(rb + c - 1) * dec_bytes; },
                                            T, kMacqCwBytes, lane, fo);
            } else {
                for (int q = lane; q < nbytes; q += 64) fo[q] = d0[q];
            }
            for (int q = nbytes + lane; q < A.frame_row; q += 64) fo[q] = 0;
            if (A.llr_out) {
                const float* src = A.llr + static_cast<size_t>(i) * A.llr_ws;
                float* dst = A.llr_out + static_cast<size_t>(w) * A.llr_stride;
                for (int q = lane; q < A.llr_stride; q += 64) dst[q] = q < n_llr ? src[q] : 0.0f;
            }
        }
        if (lane == 0) {
            ria_mcdpsk_acq_result& o = A.acq[w];
            if (report) {
                o.frame_start = o.sync_start + macq_delta(k);
                o.delta = static_cast<int16_t>(macq_delta(k));
                o.modulation = static_cast<uint8_t>(A.cur.bps[i] == 2 ? RIA_MOD_DQPSK : RIA_MOD_DBPSK);
                o.fading_index = A.mst[i].fading_index;
                o.success = static_cast<uint8_t>(success);
                o.codewords_ok = static_cast<uint8_t>(ok);
                o.codewords_failed = static_cast<uint8_t>(failed);
                o.frame_type = static_cast<uint8_t>(ftype);
                o.header_total_cw = T;
                o.frame_bytes = nbytes;
                o.n_llr = n_llr;
                if (A.ci_flag) o.reserved[0] = A.ci_flag[i];
            }
            o.candidates = static_cast<uint8_t>(o.candidates + 1);
            // the primary stops on a success, on header salvage (codewords_ok > 0) and without the handshake fallbacks;
            // the fallback candidates stop only on a full success (:1640-1797)
            A.done[i] = static_cast<uint8_t>(success || (k == 0 && (ok > 0 || !A.retry)));
        }
    }
}

// One block: the entries still searching, each at its next candidate that fits the window, appended in list order
// (ascending window index) to the next list.
__global__ __launch_bounds__(kAcqScanThreads) void macq_next_kernel(MacqArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_cur; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        int nk = -1, s = 0;
        uint32_t w = 0;
        if (i < A.n_cur && !A.done[i]) {
            w = A.cur.window[i];
            const int sync = A.acq[w].sync_start;
            for (int k = A.cur.cand[i] + 1; k < kMacqCandidates; ++k) {
                if (macq_fits(sync + macq_delta(k), A.frame_len, A.window_len)) { nk = k; s = sync + macq_delta(k); break; }
            }
        }
        int total;
        const int pos = running + acq_block_scan(nk >= 0, &total);
        if (nk >= 0) {
            A.next.offset[pos] = static_cast<uint64_t>(w) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(s);
            A.next.cfo[pos] = A.cur.cfo[i];
            A.next.window[pos] = w;
            A.next.cand[pos] = static_cast<uint8_t>(nk);
            A.next.bps[pos] = static_cast<uint8_t>(macq_alt(nk) ? 3 - A.bps : A.bps);
        }
        running += total;
    }
    if (threadIdx.x == 0) A.ctl->n_list = static_cast<unsigned>(running);
}

}  // namespace ria
