// ria_amd/csrc/mcdpsk_window_kernels.hip.h — device side of ria_gpu_mcdpsk_window_batch (include/ria_gpu.h): what
// StreamingDecoder::decodeCurrentFrame does with one MC-DPSK window around the demodulation and decode rounds of
// ria_gpu_mcdpsk_acquire_batch (mcdpsk_acquire_kernels.hip.h, mcdpsk_harq_kernels.hip.h), which it reuses as they are:
//   mwin_plan_kernel     detection -> acceptance on the pass-0 span, CFO, anti-replay, argument check of the per-window inputs
//   mwin_energy_kernel   the PING energy test (:1127-1160, :1217-1266), one wavefront per window, and the passes that need no
//                        soft bits (re-entry with a pending count, the early window)
//   mwin_list_kernel     the pass planner: the open windows of one codeword count as an ascending round-0 list
//   mwin_peek_kernel     the CW0 peek (:1444-1503, :1599-1624) on round A's (and A2's) decodes of the peek pass
//   mwin_close_kernel    the end of a decoded pass: header salvage (:1631-1644), consumed samples, the delivered result
// The scalar rules live in mcdpsk_window_rules.hpp, shared with the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "burst_kernels.hip.h"
#include "mcdpsk_acquire_kernels.hip.h"
#include "mcdpsk_window_rules.hpp"

namespace ria {

struct MwinSt {                  // one per window
    int32_t open;                // 1: a pass at `level` codewords is still to run (level 0: the peek pass on the 1-codeword span)
    int32_t level;
    int32_t first_pass;          // the pass runs with pending_total_cw_ == 0 (header salvage may follow it)
    int32_t span0;               // the pass-0 span in samples, 0 where not accepted
};
struct MwinCtl { unsigned int bad; unsigned int pad[3]; };

struct MwinArgs {
    MacqArgs M;                  // detector outputs, params, geometry, acq rows, ctl, the list to build; peek: round A's outputs
    MwinGeom g;
    const float* samples;
    ria_mcdpsk_window_result* res;
    MwinSt* st;
    MwinCtl* wctl;
    const uint8_t* tries_a;      // [n_cur] tries of round A's decodes in the peek pass
    uint8_t* tries_deint;        // [n_cur] tries of the de-interleaved CW0 decode, 0 where it did not run
    const uint8_t* tries_a2;     // [n_a2]
};

constexpr int kMwinEnergyWaves = 2;      // 2 x 5000 floats = 40 000 bytes of LDS per workgroup: three workgroups fit a CU's 160 KB

__device__ inline void mwin_apply_step(const MwinStep& s, ria_mcdpsk_window_result& r, MwinSt& st) {
    r.peek |= s.peek;
    r.passes += s.passes;
    r.pending_total_cw = s.pending;
    if (s.outcome == kMwinOpen) { st.open = 1; st.level = s.level; st.first_pass = 0; return; }
    st.open = 0;
    r.outcome = s.outcome;
    r.need_samples = s.need_samples;
}

// One thread per window: ria_gpu_mcdpsk_acquire_batch's steps 1-2 with the pass-0 span in the fit rule, then anti-replay.
__global__ __launch_bounds__(256) void mwin_plan_kernel(MwinArgs A) {
    const MacqArgs& M = A.M;
    for (int b = blockIdx.x * 256 + threadIdx.x; b < M.n_windows; b += gridDim.x * 256) {
        const ria_mcdpsk_acq_params p = M.params[b];
        bool det;
        int start;
        float corr, cfo;
        if (M.chirp) {
            const ria_chirp_result r = M.chirp[b];
            det = r.success != 0;
            start = det ? r.down_chirp_start + 24000 + 4800 : -1;
            corr = r.up_correlation > r.down_correlation ? r.up_correlation : r.down_correlation;
            cfo = r.cfo_hz;
        } else {
            const ria_zc_result r = M.zc[b];
            det = r.detected != 0;
            start = det ? r.start_sample : -1;
            corr = r.correlation;
            cfo = r.cfo_hz;
        }
        if (M.connected && fabs_(p.known_cfo_hz) > 0.01f && fabs_(cfo - p.known_cfo_hz) > 1.0f) cfo = p.known_cfo_hz;
        const long long fl1 = mwin_frame_len(A.g, 1);
        const uint32_t pending_in = p.pending_total_cw, first_avail = p.first_avail;
        bool bad = pending_in > 255u || (first_avail != 0u && first_avail < static_cast<uint32_t>(kMwinMinAvail));
        if (!A.g.disconnected && pending_in == 0u && first_avail != 0u && first_avail < fl1) bad = true;   // a connected pass 0 waits for a codeword (:1007)
        if (bad) A.wctl->bad = 1u;
        long long span = fl1;
        if (pending_in > 0u) span = mwin_frame_len(A.g, static_cast<int>(pending_in));
        else if (first_avail != 0u && first_avail < span) span = first_avail;
        const bool acc = !bad && det && !(corr < p.min_confidence) && start >= 0 && start + span <= M.window_len;
        ria_mcdpsk_acq_result o;
        o.detected = det ? 1 : 0;
        o.accepted = acc ? 1 : 0;
        o.sync_start = start;
        o.frame_start = acc ? start : -1;
        o.correlation = corr;
        o.cfo_hz = acc ? cfo : 0.0f;
        o.fading_index = 0.0f;
        o.delta = 0;
        o.modulation = static_cast<uint8_t>(M.bps == 2 ? RIA_MOD_DQPSK : RIA_MOD_DBPSK);
        o.candidates = 0;
        o.success = 0; o.codewords_ok = 0; o.codewords_failed = 0; o.frame_type = 0x10;
        o.header_total_cw = 0; o.frame_bytes = 0; o.n_llr = 0;
        o.reserved[0] = o.reserved[1] = o.reserved[2] = o.reserved[3] = 0;
        M.acq[b] = o;
        ria_mcdpsk_window_result r{};
        r.outcome = RIA_MWIN_NOT_ACCEPTED;
        r.next_pos = -1;
        r.last_decoded_sync = p.last_decoded_sync;
        MwinSt st{0, 0, 0, 0};
        if (acc) {
            st.span0 = static_cast<int32_t>(span);
            if (mwin_replay(start, p.last_decoded_sync)) {
                r.outcome = RIA_MWIN_REPLAY;
                r.next_pos = start + 9600 + 4800;          // SEARCH_BACKTRACK + CORRELATION_STEP (:885-886)
                st.span0 = 0;                              // nothing else runs
            }
        }
        A.res[b] = r;
        A.st[b] = st;
    }
}

// One wavefront per accepted window that is no replay: training_rms over [0, min(4608, len)) and rms over the next
// min(len - 4608, 5000) samples of the pass-0 span, each the reference's ascending float32 chain (burst_gate_rms), the PING
// decision under !connected_, and then the passes that need no soft bits: a re-entry's pending count and the early window go
// through the escalation chain here; every other window is left open for the peek pass (level 0).
__global__ __launch_bounds__(64 * kMwinEnergyWaves) void mwin_energy_kernel(MwinArgs A) {
    __shared__ __attribute__((aligned(16))) float sq_all[kMwinEnergyWaves][kMwinCheckLen];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * kMwinEnergyWaves + wave;
    if (b >= A.M.n_windows) return;                        // wave-uniform; the kernel has no block-wide barrier
    MwinSt st = A.st[b];
    if (st.span0 == 0) return;
    const int start = A.M.acq[b].sync_start, len = st.span0;
    const float* x = A.samples + static_cast<size_t>(b) * static_cast<size_t>(A.M.stride) + static_cast<size_t>(start);
    const int train_len = min(kMwinTrainSkip, len);
    const int check_len = min(len - train_len, kMwinCheckLen);
    const float training_rms = burst_gate_rms(x, train_len, sq_all[wave], lane);
    const float rms = burst_gate_rms(x + train_len, check_len, sq_all[wave], lane);
    if (lane != 0) return;
    ria_mcdpsk_window_result r = A.res[b];
    const ria_mcdpsk_acq_params p = A.M.params[b];
    r.training_rms = training_rms;
    r.rms = rms;
    r.passes = 1;
    if (A.g.disconnected && mwin_is_ping(training_rms, rms)) {
        ria_mcdpsk_acq_result& o = A.M.acq[b];
        o.success = 1; o.frame_type = 0x01;                // FrameType::PING, no bytes
        r.outcome = RIA_MWIN_PING;
        r.is_ping = 1; r.deliver = 1;
        r.next_pos = start + static_cast<int>(mwin_frame_len(A.g, 1));     // getMinSamplesForFrame (:1259-1260)
        r.last_decoded_sync = start;
        st.open = 0;
    } else if (p.pending_total_cw > 0u) {
        r.passes = 0;
        mwin_apply_step(mwin_escalate(A.g, start, static_cast<int>(p.pending_total_cw)), r, st);
    } else if (len < mwin_frame_len(A.g, 1)) {
        // the early window: (len - 4608) / 512 / spreading >= 2 symbols, fewer than 648 soft bits: process() succeeds and no
        // soft bit is read (:1600-1609)
        int peek = 0;
        const int pending = mwin_peek(A.g.disconnected, 1, false, false, 0, 0, &peek);
        r.peek = peek;
        mwin_apply_step(mwin_escalate(A.g, start, pending), r, st);
    } else {
        st.open = 1; st.level = 0; st.first_pass = 1;
    }
    A.res[b] = r;
    A.st[b] = st;
}

// The pass planner, one block: the open windows at `level` codewords (0: the peek pass) in ascending window order, each at
// its primary candidate, as the round-0 list of ria_gpu_mcdpsk_acquire_batch's rounds.
__global__ __launch_bounds__(kAcqScanThreads) void mwin_list_kernel(MwinArgs A, int level) {
    const MacqArgs& M = A.M;
    int running = 0;
    for (int base = 0; base < M.n_windows; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        bool in = false;
        if (b < M.n_windows) { const MwinSt st = A.st[b]; in = st.open && st.level == level; }
        int total;
        const int pos = running + acq_block_scan(in, &total);
        if (in) {
            const ria_mcdpsk_acq_result o = M.acq[b];
            M.next.offset[pos] = static_cast<uint64_t>(b) * static_cast<uint64_t>(M.stride) + static_cast<uint64_t>(o.sync_start);
            M.next.cfo[pos] = o.cfo_hz;
            M.next.window[pos] = static_cast<uint32_t>(b);
            M.next.cand[pos] = 0;
            M.next.bps[pos] = static_cast<uint8_t>(M.bps);
        }
        running += total;
    }
    if (threadIdx.x == 0) { M.ctl->n_list = static_cast<unsigned>(running); M.ctl->n_rows = 0u; }
}

// tries of the de-interleaved CW0 decodes, by entry (the A2 list's length is read on the device)
__global__ __launch_bounds__(256) void mwin_a2_tries_kernel(MwinArgs A) {
    const int n_a2 = static_cast<int>(A.M.ci_ctl->n_a2);
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n_a2 && r < A.M.n_cur; r += gridDim.x * 256) A.tries_deint[A.M.ci_list[r]] = A.tries_a2[r];
}

// One wave per entry of the peek pass: magic, parseHeader with both CRC forms on the whole decoded vector (it reads bytes
// 0..19 only, so decodeMCDPSKFrame's truncation to 20 bytes changes nothing), the forcing CONNECT guard, the escalation
// rules and the statement that decided.
__global__ __launch_bounds__(256) void mwin_peek_kernel(MwinArgs A) {
    const MacqArgs& M = A.M;
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < M.n_cur; i += gridDim.x * 4) {
        const int n_llr = M.mst[i].n_llr;
        const uint8_t* d = M.out_a + static_cast<size_t>(i) * M.dec_bytes;
        const bool have = n_llr >= kMacqLdpcBlock && M.ok_a[i] && d[0] == 0x55 && d[1] == 0x4C;
        bool valid = false, ctl = false;
        int plen = 0;
        if (have) {
            RecCtx x{};
            x.crc_bit = M.crc_bit; x.crc_init = M.crc_init; x.lane = lane;
            valid = rec_parse_header(x, d, kMacqCwBytes, &ctl, &plen);
        }
        if (lane != 0) continue;
        const uint32_t w = M.cur.window[i];
        ria_mcdpsk_window_result r = A.res[w];
        MwinSt st = A.st[w];
        const int total = valid ? (ctl ? 1 : d[12]) : 0;
        int peek = 0;
        const int pending = mwin_peek(A.g.disconnected, n_llr, have, valid, have ? d[2] : 0, total, &peek);
        if (M.ci_flag && (M.ci_flag[i] & kMacqCiDeint)) peek |= kMpeekDeinterleaved;
        r.peek = peek;
        r.peek_total_cw = total;
        r.peek_tries = static_cast<uint8_t>((n_llr >= kMacqLdpcBlock ? A.tries_a[i] : 0) + (M.ci_flag ? A.tries_deint[i] : 0));
        if (pending > 0) mwin_apply_step(mwin_escalate(A.g, M.acq[w].sync_start, pending), r, st);
        else { st.open = 1; st.level = 1; st.first_pass = 1; }
        A.res[w] = r;
        A.st[w] = st;
    }
}

// One thread per window, after the rounds of `level`: header salvage (:1631-1644) or the window's end (:1967-2013, :2121).
__global__ __launch_bounds__(256) void mwin_close_kernel(MwinArgs A, int level) {
    const MacqArgs& M = A.M;
    for (int b = blockIdx.x * 256 + threadIdx.x; b < M.n_windows; b += gridDim.x * 256) {
        MwinSt st = A.st[b];
        if (!st.open || st.level != level) continue;
        ria_mcdpsk_window_result r = A.res[b];
        ria_mcdpsk_acq_result& o = M.acq[b];
        const int len = static_cast<int>(mwin_frame_len(A.g, level));
        if (!o.success && st.first_pass && o.codewords_ok > 0 && o.header_total_cw > 1 && mwin_avail_cw(A.g, level) < o.header_total_cw) {
            r.peek |= kMpeekSalvage;
            o.candidates = 0;
            mwin_apply_step(mwin_escalate(A.g, o.sync_start, o.header_total_cw), r, st);
        } else {
            st.open = 0;
            r.outcome = RIA_MWIN_DECODED;
            r.frame_len = len;
            r.next_pos = o.frame_start + len;              // frame_start follows a recovered candidate (:1771); never the exact-size shortcut
            r.deliver = static_cast<uint8_t>(o.success || o.codewords_ok > 0);
            r.last_decoded_sync = o.frame_start;
        }
        A.res[b] = r;
        A.st[b] = st;
    }
}

}  // namespace ria
