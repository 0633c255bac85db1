// ria_amd/csrc/mcdpsk_harq_kernels.hip.h — device side of the HARQ chase cache in decodeMCDPSKFrame
// (streaming_decoder.cpp:2729-2731, :2766-2789, :2796-2799, :2808-2811; include/ria_gpu.h) and of
// ria_gpu_mcdpsk_decode_frame_batch's list builder.
//
// The stages sit between round B and the finish of mcdpsk_acquire_kernels.hip.h and work on that round's arrays: the store
// stage walks an entry's codewords ascending with round B's outcomes in hand, the sum list is built by a block scan (its
// order is that of the round-B rows), the resolve stage writes a recovered codeword's bytes and flag over round B's, so
// macq_finish_kernel reassembles what the reference would.  One wave owns one cache for the length of a kernel (the call
// refuses two windows with one cache id): lane 0 runs the policy of chase_policy.hpp, the wave moves the floats.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chase_policy.hpp"
#include "mcdpsk_acquire_kernels.hip.h"

namespace ria {

struct HarqArgs {
    ChaseCache* caches;                  // [n_caches]
    float* sums;                         // [n_caches][max_entries][16][648]
    int32_t* owner;                      // [n_caches] the window that uses the cache in this call, -1 none
    int n_caches;
    ChaseCfg cfg;
    const int32_t* cache_id;             // [n_windows]
    const uint64_t* now_ms;              // [n_windows]
    ria_mcdpsk_harq_result* harq;        // [n_windows], never null inside the library
    // per round-B row
    uint8_t* sum_flag;                   // the row's combined sum is to be decoded
    uint32_t* sum_src;                   // which sum: (cache * max_entries + slot) * 16 + cw
    int32_t* sum_pos;                    // its place in the list of sums, -1 none
    uint32_t* sum_list;                  // the list: round-B rows, ascending
    uint8_t* out_b; uint8_t* ok_b;       // round B's outputs, writable
    const uint8_t* out_c; const uint8_t* ok_c;   // the decodes of the listed sums
};

__device__ __forceinline__ ChaseKey harq_key(const uint8_t* d) {   // parseHeader, frame_v2.cpp:1213-1223
    ChaseKey k;
    k.seq = static_cast<uint16_t>((d[4] << 8) | d[5]);
    k.src_hash = (static_cast<uint32_t>(d[6]) << 16) | (static_cast<uint32_t>(d[7]) << 8) | d[8];
    k.dst_hash = (static_cast<uint32_t>(d[9]) << 16) | (static_cast<uint32_t>(d[10]) << 8) | d[11];
    return k;
}
__device__ __forceinline__ size_t harq_sum_index(const HarqArgs& H, int cache, int slot, int cw) {
    return (static_cast<size_t>(cache) * H.cfg.max_entries + slot) * RIA_CHASE_MAX_CW + cw;
}

// Every window: its harq result zeroed, its cache claimed.  A cache claimed twice, or an id the pool does not have, raises
// the control block's flag; the host reads it with the first control read, before any cache is touched.
__global__ __launch_bounds__(256) void harq_claim_kernel(HarqArgs H, int n_windows, MacqCtl* ctl) {
    for (int w = blockIdx.x * 256 + threadIdx.x; w < n_windows; w += gridDim.x * 256) {
        ria_mcdpsk_harq_result z{};
        H.harq[w] = z;
        const int c = H.cache_id[w];
        if (c < 0) continue;
        if (c >= H.n_caches || atomicCAS(&H.owner[c], -1, w) != -1) atomicOr(&ctl->dup, 1u);
    }
}

// Stage 4, one wave per entry.
__global__ __launch_bounds__(256) void harq_store_kernel(MacqArgs A, HarqArgs H) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < A.n_cur; i += gridDim.x * 4) {
        const uint32_t w = A.cur.window[i];
        const int c = H.cache_id[w];
        const int T = A.hdr_total[i], need = A.need_rows[i];
        const uint32_t rb = need > 0 ? A.row_base[i] : 0u;
        if (c < 0 || T == 0) {                       // chase off, or no header: round B's rows (if any) have no sums
            if (lane == 0) for (int r = 0; r < need; ++r) H.sum_flag[rb + r] = 0;
            continue;
        }
        const uint8_t* d0 = A.out_a + static_cast<size_t>(i) * A.dec_bytes;
        const ChaseKey key = harq_key(d0);
        const int ftype = d0[2];
        const uint64_t now = H.now_ms[w];
        ChaseCache& cache = H.caches[c];
        unsigned stored = 0, summed = 0, maxc = 0;
        for (int r = 0; r < need; ++r) {             // T == 1 and avail < T return before the cache is used: need == 0
            const int cw = r + 1;
            const uint32_t row = rb + r;
            if (A.ok_b[row]) {
                if (lane == 0) { chase_mark_decoded(cache, H.cfg, key, cw); H.sum_flag[row] = 0; }
                continue;
            }
            int act = 0, slot = -1;
            if (lane == 0) act = chase_store(cache, H.cfg, key, cw, T, ftype, now, &slot);
            act = __shfl(act, 0);
            slot = __shfl(slot, 0);
            if (act != kChaseRefused) {
                float* dst = H.sums + harq_sum_index(H, c, slot, cw) * kMacqLdpcBlock;
                const float* src = A.llr + static_cast<size_t>(i) * A.llr_ws + static_cast<size_t>(cw) * kMacqLdpcBlock;
                if (act == kChaseCopy) for (int q = lane; q < kMacqLdpcBlock; q += 64) dst[q] = src[q];
                else for (int q = lane; q < kMacqLdpcBlock; q += 64) dst[q] = dst[q] + src[q];
            }
            if (lane == 0) {
                const int hit = chase_get_combined(cache, H.cfg, key, cw);
                const int count = chase_combine_count(cache, H.cfg, key, cw);
                const bool decode = hit >= 0 && count > 1;
                H.sum_flag[row] = decode ? 1 : 0;
                if (decode) { H.sum_src[row] = static_cast<uint32_t>(harq_sum_index(H, c, hit, cw)); summed |= 1u << cw; }
                if (act != kChaseRefused) stored |= 1u << cw;
                if (static_cast<unsigned>(count) > maxc) maxc = static_cast<unsigned>(count);
            }
        }
        if (lane == 0) {
            ria_mcdpsk_harq_result o{};
            o.seq = key.seq; o.valid = 1; o.src_hash = key.src_hash; o.dst_hash = key.dst_hash;
            o.stored_mask = static_cast<uint16_t>(stored); o.sum_mask = static_cast<uint16_t>(summed);
            o.max_combine = static_cast<uint8_t>(maxc); o.cache_id = c;
            H.harq[w] = o;
        }
    }
}

// One block: the list of the rows whose sum is decoded, ascending, and its length.
__global__ __launch_bounds__(kAcqScanThreads) void harq_sum_list_kernel(HarqArgs H, int n_rows, MacqCtl* ctl) {
    int running = 0;
    for (int base = 0; base < n_rows; base += kAcqScanThreads) {
        const int r = base + static_cast<int>(threadIdx.x);
        const bool f = r < n_rows && H.sum_flag[r] != 0;
        int total;
        const int pos = running + acq_block_scan(f, &total);
        if (r < n_rows) H.sum_pos[r] = f ? pos : -1;
        if (f) H.sum_list[pos] = static_cast<uint32_t>(r);
        running += total;
    }
    if (threadIdx.x == 0) ctl->n_sums = static_cast<unsigned>(running);
}

// Stage 5's rows: the listed sums out of the pool.  The pool holds raw sums (the store stage copies and adds the soft bits
// as received, :2769-2770); a sum of an entry whose CW0 was de-interleaved is de-interleaved here, as it is gathered (:2778).
__global__ __launch_bounds__(256) void harq_sum_gather_kernel(HarqArgs H, float* rows, int n_sums, const uint32_t* row_entry,
                                                              const uint8_t* ci_flag, int ci_step) {
    const size_t total = static_cast<size_t>(n_sums) * kMacqLdpcBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
        const size_t q = i / kMacqLdpcBlock, j = i - q * kMacqLdpcBlock;
        const uint32_t row = H.sum_list[q];
        const size_t src = (ci_flag && (ci_flag[row_entry[row]] & kMacqCiDeint)) ? macq_ci_src(j, ci_step) : j;
        rows[i] = H.sums[static_cast<size_t>(H.sum_src[row]) * kMacqLdpcBlock + src];
    }
}

// Stage 6 and the cache's part of stage 7, one wave per entry: a recovered codeword's bytes and flag replace round B's
// (:2779-2783), every decoded codeword is marked (:2796-2799; for one that decoded at once the store stage did it already
// and this would repeat it, so only the recovered ones are marked here, twice as the reference does), a full success
// removes the entry (:2808-2811).  have_sums 0: the list was empty and stage 5 did not run.
__global__ __launch_bounds__(256) void harq_resolve_kernel(MacqArgs A, HarqArgs H, int have_sums) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < A.n_cur; i += gridDim.x * 4) {
        const uint32_t w = A.cur.window[i];
        const int c = H.cache_id[w];
        const int T = A.hdr_total[i], need = A.need_rows[i];
        if (c < 0 || T == 0 || need == 0) continue;
        const uint8_t* d0 = A.out_a + static_cast<size_t>(i) * A.dec_bytes;
        const ChaseKey key = harq_key(d0);
        ChaseCache& cache = H.caches[c];
        const uint32_t rb = A.row_base[i];
        unsigned recovered = 0;
        bool all_ok = true;
        for (int r = 0; r < need; ++r) {
            const int cw = r + 1;
            const uint32_t row = rb + r;
            bool ok = H.ok_b[row] != 0;              // read by the whole wave before lane 0 may set it
            if (!ok && have_sums && H.sum_flag[row]) {
                const int pos = H.sum_pos[row];
                if (H.ok_c[pos]) {                   // data_chase.size() >= bytes_per_cw holds: the decoder returns 21 bytes
                    ok = true;
                    recovered |= 1u << cw;
                    for (int q = lane; q < A.dec_bytes; q += 64)
                        H.out_b[static_cast<size_t>(row) * A.dec_bytes + q] = H.out_c[static_cast<size_t>(pos) * A.dec_bytes + q];
                    if (lane == 0) {
                        chase_mark_decoded(cache, H.cfg, key, cw);
                        cache.stats.recoveries++;
                        chase_mark_decoded(cache, H.cfg, key, cw);
                        H.ok_b[row] = 1;
                    }
                }
            }
            all_ok = all_ok && ok;
        }
        if (lane == 0) {
            int entry;
            if (all_ok) entry = chase_remove(cache, H.cfg, key) ? RIA_HARQ_ENTRY_REMOVED : RIA_HARQ_ENTRY_NONE;
            else entry = chase_find(cache, H.cfg, key) >= 0 ? RIA_HARQ_ENTRY_KEPT : RIA_HARQ_ENTRY_NONE;
            H.harq[w].recovered_mask = static_cast<uint16_t>(recovered);
            H.harq[w].entry = static_cast<uint8_t>(entry);
        }
    }
}

// ChaseCache::clear for the listed caches (ids null: all n)
__global__ __launch_bounds__(256) void harq_clear_kernel(ChaseCache* caches, int n_caches, const int32_t* ids, int n) {
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const int c = ids ? ids[q] : q;
        if (c >= 0 && c < n_caches) chase_clear(caches[c]);
    }
}

// ---- ria_gpu_mcdpsk_decode_frame_batch: rows of soft bits as a round's list, and the DecodeResult out of the finish
__global__ __launch_bounds__(256) void mdf_list_kernel(MacqArgs A, const int32_t* n_llr, ria_mcdpsk_status* mst) {
    for (int f = blockIdx.x * 256 + threadIdx.x; f < A.n_cur; f += gridDim.x * 256) {
        int n = n_llr ? n_llr[f] : A.llr_ws;
        n = n < 0 ? 0 : (n > A.llr_ws ? A.llr_ws : n);
        ria_mcdpsk_status st{};
        st.n_llr = n;
        mst[f] = st;
        A.cur.window[f] = static_cast<uint32_t>(f);
        A.cur.cand[f] = 0;
        A.cur.bps[f] = 1;
        ria_mcdpsk_acq_result o{};
        o.frame_type = 0x10;
        A.acq[f] = o;
    }
}
__global__ __launch_bounds__(256) void mdf_result_kernel(const ria_mcdpsk_acq_result* acq, int n, ria_mcdpsk_dframe_result* out) {
    for (int f = blockIdx.x * 256 + threadIdx.x; f < n; f += gridDim.x * 256) {
        const ria_mcdpsk_acq_result a = acq[f];
        ria_mcdpsk_dframe_result o{};
        o.success = a.success; o.codewords_ok = a.codewords_ok; o.codewords_failed = a.codewords_failed; o.frame_type = a.frame_type;
        o.header_total_cw = a.header_total_cw; o.frame_bytes = a.frame_bytes;
        o.reserved = a.reserved[0];          // the channel-interleaving bits of the ci call, 0 otherwise
        out[f] = o;
    }
}

}  // namespace ria
