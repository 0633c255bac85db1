// ria_amd/csrc/decode_frame_kernels.hip.h — device side of ria_gpu_decode_frame_batch (include/ria_gpu.h): the OFDM branch
// of StreamingDecoder::decodeFrame (src/gui/modem/streaming_decoder.cpp:2821-3059), its "try both" strategy, over a batch
// of soft-bit rows.
//
// A row walks through up to six stages (R1/4 control probe, raw CW0 probe at the link rate, decodeFixedFrame, salvage at
// R1/4, salvage at the link rate, legacy CW1+).  Each stage runs on a compact list of the rows still open, built by a
// block-wide scan over ALL rows in ascending order (acq_block_scan of acquire_kernels.hip.h), so a list - and with it every
// result - does not depend on scheduling, and a stage never runs for a row an earlier one resolved.  The probe kernels read
// their list's length from the device: the host only learns the two lengths it must size a launch with (the fixed batch,
// the legacy codeword rows).
//
// dframe_probe_kernel decodes CW0 of a row and classifies it in the same wave: the decoded bytes go from the decoder's
// LDS image to an LDS scratch row, the magic, parseHeader (rec_parse_header) and total_cw are evaluated there, and one
// 80-byte probe record leaves the wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "ldpc_fast.hip.h"
#include "recovery_kernels.hip.h"

namespace ria {

constexpr int kDfBlock = 648, kDfFrameBits = 2592, kDfMaxCw = 32;
constexpr uint32_t kDfNoIndex = 0xFFFFFFFFu;
enum { kDfProbeR14 = 0, kDfProbeRate = 1, kDfSalvR14 = 2, kDfSalvRate = 3 };                 // probe records of a row
enum { kDfListR14 = 0, kDfListRate = 1, kDfListFixed = 2, kDfListSalvR14 = 3, kDfListSalvRate = 4, kDfNumLists = 5 };
enum { kDfStageInit = 0, kDfStageAfterR14, kDfStageAfterRate, kDfStageAfterFixed, kDfStageAfterSalvR14, kDfStageLegacy };

struct DfCtl {                   // zeroed per call; read back by the host twice
    unsigned int n[kDfNumLists]; // list lengths
    unsigned int n_rows;         // legacy codeword rows
    unsigned int fault;          // the fixed stage reported a decode work-queue fault
    unsigned int pad_;
};

struct DfProbe {                 // 80 bytes: what one CW0 decode of a row found (zeroed per call: ran 0 = the stage did not run)
    uint8_t ran, ok, magic, valid;   // valid: ok, magic and parseHeader valid with total_cw >= 1
    uint8_t type, total_cw, tries, pad0;
    uint16_t iters, plen;
    uint8_t bytes[68];           // decoded bytes truncated to the probe rate's bytes per codeword
};

struct DfRow {                   // 20 bytes of per-row state
    int32_t n_llr;               // clamped to [0, llr_stride]
    uint8_t path;                // RIA_DFRAME_* once a stage resolved the row, else 0
    uint8_t stages;              // ria_dframe_result.stages
    uint8_t try_fi;              // try_frame_interleave
    uint8_t legacy;              // the rate probe was ok with magic: the legacy block runs
    uint32_t fixed_idx;          // row of the fixed batch, kDfNoIndex if none
    uint32_t row_base;           // first legacy codeword row
    int32_t need;                // legacy codeword rows (total_cw - 1), 0 if none
};

struct DfArgs {
    const float* llr; int llr_stride; const int32_t* n_llr; int n_frames;
    int rate_is_r14;             // the handle's code is R1/4: no fast path, one salvage
    int bpc, bpc14;              // bytes per codeword at the handle's rate / at R1/4
    DfRow* row; DfProbe* probe;  // [n], [4][n]
    uint32_t* list;              // [kDfNumLists][n]
    DfCtl* ctl;
    float* fx_llr; uint8_t* fx_info; ria_decode_status* fx_st;   // the fixed batch: [n][2592], [n][4 * bpc], [n]
    const uint16_t* perm;        // [648] per-codeword channel de-interleave (identity without it)
    float* lg_rows; uint32_t* lg_entry; uint8_t* lg_cw;          // legacy rows: [rows][648], frame and codeword of a row
    const uint8_t* lg_out; const uint8_t* lg_ok; int dec_bytes;  // their decodes: [rows][dec_bytes], [rows]
    const uint16_t* crc_bit; const uint16_t* crc_init;
    uint8_t* frame_out; int frame_row; ria_dframe_result* result; ria_decode_status* st_out; uint8_t* info_out;
};

__device__ __forceinline__ bool df_control_hit(const DfProbe& p) { return p.ran && p.valid && p.total_cw == 1; }

// One wavefront per listed row: CW0 = soft bits [0, 648) of the row, decoded once at (c.max_iter, 0.75) - codec_->decode -
// or, kRobust, down the factor ladder of robustDecodeSingleCW; then magic, truncation to `bpc` bytes and parseHeader.
template <class S, bool kRobust>
__global__ __launch_bounds__(64) void dframe_probe_kernel(FastCode c, DfArgs A, int which_list, int which_probe, int bpc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    FastState<S> st;
    fast_load_tables(st, c, smem, lane);
    const int nb = (c.k + 7) / 8;
    unsigned n_list = A.ctl->n[which_list];
    if (n_list > static_cast<unsigned>(A.n_frames)) n_list = static_cast<unsigned>(A.n_frames);
    for (unsigned q = blockIdx.x; q < n_list; q += gridDim.x) {
        const uint32_t row = A.list[static_cast<size_t>(which_list) * A.n_frames + q];
        const float* l = A.llr + static_cast<size_t>(row) * A.llr_stride;
        const int ln = opaque_lane(lane);
#pragma unroll
        for (int r = 0; r < S::NC; ++r) { const uint32_t j = c.col_at[ln + 64 * r]; st.li[r] = (j != 0xFFFFu) ? llr_canon(l[j]) : 0.0f; }
#pragma unroll
        for (int r = 0; r < S::NR; ++r) { const uint32_t i = c.check_at[ln + 64 * r]; st.lp[r] = (i != 0xFFFFu) ? llr_canon(l[c.k + i]) : kIdleRowLlr; }
        bool ok = false;
        int it = 0, tries = 0;
        if (kRobust) {
#pragma unroll 1
            for (int f = 0; f < kNumFactors && !ok; ++f) { it = fast_decode(st, c, smem, kFactors[f], c.max_iter, lane, &ok); ++tries; }
        } else {
            it = fast_decode(st, c, smem, 0.75f, c.max_iter, lane, &ok);
            tries = 1;
        }
        // the bytes stay in the wave: fast_pack reads the hard-bit masks at smem[0, 72) and writes the scratch row behind them
        // (the c2v area, free once the decode is over)
        uint8_t* d = smem + 128;
        fast_pack(st, c, smem, d, nb, lane);
        const bool magic = ok && d[0] == 0x55 && d[1] == 0x4C;
        bool valid = false, ctl = false;
        int plen = 0, total = 0;
        if (magic) {
            RecCtx x{};
            x.crc_bit = A.crc_bit; x.crc_init = A.crc_init; x.lane = lane;
            if (rec_parse_header(x, d, bpc, &ctl, &plen)) {
                total = ctl ? 1 : d[12];
                valid = total != 0;      // total_cw 0: undefined in the reference, an invalid header here
            }
        }
        DfProbe* p = A.probe + static_cast<size_t>(which_probe) * A.n_frames + row;
        for (int b = lane; b < 68; b += 64) p->bytes[b] = b < bpc ? d[b] : static_cast<uint8_t>(0);
        if (lane == 0) {
            p->ran = 1; p->ok = ok ? 1 : 0; p->magic = magic ? 1 : 0; p->valid = valid ? 1 : 0;
            p->type = magic ? d[2] : static_cast<uint8_t>(0); p->total_cw = static_cast<uint8_t>(valid ? total : 0);
            p->tries = static_cast<uint8_t>(tries); p->pad0 = 0;
            p->iters = static_cast<uint16_t>(it); p->plen = static_cast<uint16_t>(plen);
        }
        wave_sync();     // the scratch row is read above, the next decode rewrites the c2v area
    }
}

// One block: folds the stage that just ran into the rows' state and lists, in ascending row order, the rows of the next.
__global__ __launch_bounds__(kAcqScanThreads) void dframe_list_kernel(DfArgs A, int stage) {
    const int n = A.n_frames;
    int running = 0;
    int out_list = -1;
    for (int base = 0; base < n; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        bool flag = false;
        int need = 0;
        DfRow R{};
        if (b < n) {
            if (stage == kDfStageInit) {
                int v = A.n_llr ? A.n_llr[b] : A.llr_stride;
                v = v < 0 ? 0 : (v > A.llr_stride ? A.llr_stride : v);
                R.n_llr = v; R.fixed_idx = kDfNoIndex;
                flag = v >= kDfBlock;
            } else {
                R = A.row[b];
                const DfProbe* P = A.probe + b;
                if (stage == kDfStageAfterR14) {
                    const DfProbe p = P[static_cast<size_t>(kDfProbeR14) * n];
                    if (p.ran) R.stages |= 1;
                    if (df_control_hit(p)) R.path = RIA_DFRAME_CONTROL_R14;
                    flag = R.n_llr >= kDfBlock && R.path == 0;
                } else if (stage == kDfStageAfterRate) {
                    const DfProbe p = P[static_cast<size_t>(kDfProbeRate) * n];
                    if (p.ran) R.stages |= 2;
                    R.legacy = (p.ran && p.magic) ? 1 : 0;
                    R.try_fi = 1;
                    if (R.legacy) {
                        R.try_fi = 0;
                        if (p.valid) {
                            if (p.total_cw == 1) R.path = RIA_DFRAME_CONTROL_CW0;
                            else if (p.total_cw == 4) R.try_fi = 1;
                        }
                    }
                    flag = R.path == 0 && R.try_fi && R.n_llr >= kDfFrameBits;
                } else if (stage == kDfStageAfterFixed) {
                    if (R.fixed_idx != kDfNoIndex) {
                        R.stages |= 4;
                        const ria_decode_status s = A.fx_st[R.fixed_idx];
                        if (s.reserved[1] == kDecodeFaultMarker) A.ctl->fault = 1u;
                        if (s.cw_ok[0] && s.cw_ok[1] && s.cw_ok[2] && s.cw_ok[3]) R.path = RIA_DFRAME_FIXED;
                        else flag = true;
                    }
                } else if (stage == kDfStageAfterSalvR14) {
                    const DfProbe p = P[static_cast<size_t>(kDfSalvR14) * n];
                    if (p.ran) R.stages |= 8;
                    if (R.path == 0 && p.ran && p.ok && df_control_hit(p)) R.path = RIA_DFRAME_SALVAGE_R14;
                    flag = (R.stages & 4) && R.path == 0 && !A.rate_is_r14;
                } else {   // kDfStageLegacy: the rate salvage, then the rows of CW1.. of the frames the legacy block decodes
                    const DfProbe p = P[static_cast<size_t>(kDfSalvRate) * n];
                    if (p.ran) R.stages |= 16;
                    if (R.path == 0 && p.ran && p.ok && df_control_hit(p)) R.path = RIA_DFRAME_SALVAGE_RATE;
                    if (R.path == 0 && R.legacy) {
                        const DfProbe p1 = P[static_cast<size_t>(kDfProbeRate) * n];
                        if (p1.valid && R.n_llr / kDfBlock >= p1.total_cw) need = p1.total_cw - 1;   // >= 1: total_cw 1 was resolved
                    }
                    if (need > kDfMaxCw - 1) need = 0;   // cannot happen: n_llr <= 32 codewords
                    R.need = need;
                    if (need) R.stages |= 32;
                }
            }
        }
        if (stage == kDfStageLegacy) {
            int pos = 0, tile = 0;
            const int max_need = A.llr_stride / kDfBlock - 1;   // a row holds at most llr_stride / 648 codewords
            for (int r = 0; r < max_need; ++r) {   // exclusive prefix sum of `need` = sum over r of the scan of (need > r)
                int t;
                pos += acq_block_scan(need > r, &t);
                tile += t;
            }
            if (b < n) {
                R.row_base = static_cast<uint32_t>(running + pos);
                for (int r = 0; r < need; ++r) { A.lg_entry[R.row_base + r] = static_cast<uint32_t>(b); A.lg_cw[R.row_base + r] = static_cast<uint8_t>(1 + r); }
            }
            running += tile;
        } else {
            out_list = stage == kDfStageInit ? (A.rate_is_r14 ? kDfListRate : kDfListR14)
                     : stage == kDfStageAfterR14 ? kDfListRate
                     : stage == kDfStageAfterRate ? kDfListFixed
                     : stage == kDfStageAfterFixed ? kDfListSalvR14 : kDfListSalvRate;
            int total;
            const int pos = running + acq_block_scan(flag, &total);
            if (flag) {
                A.list[static_cast<size_t>(out_list) * n + pos] = static_cast<uint32_t>(b);
                if (stage == kDfStageAfterRate) R.fixed_idx = static_cast<uint32_t>(pos);
            }
            running += total;
        }
        if (b < n) A.row[b] = R;
    }
    if (threadIdx.x == 0) {
        if (stage == kDfStageLegacy) A.ctl->n_rows = static_cast<unsigned>(running);
        else A.ctl->n[out_list] = static_cast<unsigned>(running);
    }
}

// the first 2592 soft bits of the listed rows, as one contiguous decodeFixedFrame batch (bit copies: NaNs keep their payload)
__global__ __launch_bounds__(256) void dframe_fixed_gather_kernel(DfArgs A, int n_fixed) {
    const size_t total = static_cast<size_t>(n_fixed) * kDfFrameBits;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(A.llr);
    uint32_t* dst = reinterpret_cast<uint32_t*>(A.fx_llr);
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
        const size_t q = i / kDfFrameBits, j = i - q * kDfFrameBits;
        dst[i] = src[static_cast<size_t>(A.list[static_cast<size_t>(kDfListFixed) * A.n_frames + q]) * A.llr_stride + j];
    }
}

// one 648-float row per (frame, codeword >= 1) of the legacy block, through ChannelInterleaver::deinterleave when enabled
__global__ __launch_bounds__(256) void dframe_legacy_rows_kernel(DfArgs A, int n_rows) {
    const size_t total = static_cast<size_t>(n_rows) * kDfBlock;
    for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
        const size_t r = i / kDfBlock, j = i - r * kDfBlock;
        A.lg_rows[i] = A.llr[static_cast<size_t>(A.lg_entry[r]) * A.llr_stride + static_cast<size_t>(A.lg_cw[r]) * kDfBlock + A.perm[j]];
    }
}

// One wave per row: the DecodeResult as decodeFrame leaves it, the frame bytes and the fixed attempt's status and bytes.
__global__ __launch_bounds__(256) void dframe_finish_kernel(DfArgs A) {
    const int lane = threadIdx.x & 63, n = A.n_frames;
    for (int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < n; b += gridDim.x * 4) {
        const DfRow R = A.row[b];
        const DfProbe* p0 = A.probe + static_cast<size_t>(kDfProbeR14) * n + b;
        const DfProbe* p1 = A.probe + static_cast<size_t>(kDfProbeRate) * n + b;
        const DfProbe* s0 = A.probe + static_cast<size_t>(kDfSalvR14) * n + b;
        const DfProbe* s1 = A.probe + static_cast<size_t>(kDfSalvRate) * n + b;
        int path = R.path, success = 0, ok = 0, failed = 0, ftype = 0x10, nbytes = 0, htotal = 0;
        uint8_t* fo = A.frame_out + static_cast<size_t>(b) * A.frame_row;
        const uint8_t* src = nullptr;      // a plain copy of nbytes bytes
        const bool fixed_ran = (R.stages & 4) != 0;
        const uint8_t* fx_info = fixed_ran ? A.fx_info + static_cast<size_t>(R.fixed_idx) * 4 * A.bpc : nullptr;
        ria_decode_status fst{};
        if (fixed_ran) fst = A.fx_st[R.fixed_idx];
        if (path == RIA_DFRAME_CONTROL_R14) {
            success = 1; ok = 1; ftype = p0->type; htotal = 1; nbytes = A.bpc14; src = p0->bytes;
        } else {
            if (p1->valid) { ftype = p1->type; htotal = p1->total_cw; }
            if (fixed_ran) for (int c = 0; c < 4; ++c) { if (fst.cw_ok[c]) ++ok; else ++failed; }
            if (path == RIA_DFRAME_CONTROL_CW0) {
                success = 1; ok = 1; nbytes = A.bpc; src = p1->bytes;
            } else if (path == RIA_DFRAME_FIXED) {
                success = fst.frame_valid ? 1 : 0;
                if (success) {
                    const int t = fx_info[2];
                    const int bpc = A.bpc;
                    nbytes = rec_reassemble_cws(rec_is_control(t), (fx_info[13] << 8) | fx_info[14],
                                                [&](int c) { return fx_info + c * bpc; }, 4, bpc, lane, fo);
                    ftype = t;
                }
            } else if (path == RIA_DFRAME_SALVAGE_R14 || path == RIA_DFRAME_SALVAGE_RATE) {
                const bool a = path == RIA_DFRAME_SALVAGE_R14;
                const DfProbe* s = a ? s0 : s1;
                success = 1; ok = 1; failed = 0; ftype = s->type; htotal = 1;
                nbytes = (a || A.rate_is_r14) ? A.bpc14 : A.bpc; src = s->bytes;
            } else if (R.legacy) {
                ok = 1;                       // codewords_failed is NOT reset: a count left by the fixed attempt stays
                if (!p1->valid) path = RIA_DFRAME_BAD_HEADER;
                else if (R.need == 0) { path = RIA_DFRAME_PARTIAL; nbytes = A.bpc; src = p1->bytes; }
                else {
                    path = RIA_DFRAME_LEGACY;
                    int bad = 0;
                    for (int r = 0; r < R.need; ++r) { if (A.lg_ok[R.row_base + r]) ++ok; else { ++failed; ++bad; } }
                    if (bad == 0) {
                        success = 1;
                        const uint8_t* d0 = p1->bytes;
                        const uint8_t* out_b = A.lg_out;
                        const uint32_t rb = R.row_base;
                        const int dec_bytes = A.dec_bytes;
                        nbytes = rec_reassemble_cws(rec_is_control(p1->type), p1->plen,
                                                    [&](int c) { return c == 0 ? d0 : out_b + static_cast<size_t>(rb + c - 1) * dec_bytes; },
                                                    R.need + 1, A.bpc, lane, fo);
                    }
                }
            } else {
                path = fixed_ran ? RIA_DFRAME_FIXED_FAILED : RIA_DFRAME_NONE;
            }
        }
        if (src) for (int q = lane; q < nbytes; q += 64) fo[q] = src[q];
        for (int q = nbytes + lane; q < A.frame_row; q += 64) fo[q] = 0;
        if (A.info_out) {
            uint8_t* io = A.info_out + static_cast<size_t>(b) * 4 * A.bpc;
            for (int q = lane; q < 4 * A.bpc; q += 64) io[q] = fixed_ran ? fx_info[q] : static_cast<uint8_t>(0);
        }
        if (lane == 0) {
            if (A.st_out) A.st_out[b] = fst;
            ria_dframe_result o{};
            o.success = static_cast<uint8_t>(success); o.codewords_ok = static_cast<uint8_t>(ok);
            o.codewords_failed = static_cast<uint8_t>(failed); o.frame_type = static_cast<uint8_t>(ftype);
            o.path = static_cast<uint8_t>(path); o.header_total_cw = static_cast<uint8_t>(htotal); o.stages = R.stages;
            o.frame_bytes = nbytes;
            o.iters_r14 = p0->iters; o.iters_cw0 = p1->iters;
            o.tries_r14 = s0->tries; o.tries_rate = s1->tries;
            A.result[b] = o;
        }
    }
}

}  // namespace ria
