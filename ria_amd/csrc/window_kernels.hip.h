// ria_amd/csrc/window_kernels.hip.h — device side of ria_gpu_rx_window_batch (include/ria_gpu.h): the ladder that joins the
// control hypothesis, the span demodulator, the robust single-codeword decoder and decodeFrame into what
// gui::StreamingDecoder does with one connected-mode OFDM-CHIRP window (src/gui/modem/streaming_decoder.cpp:1268-2013).
//
//   win_stage_kernel    one thread per window: folds the stage that just ran into the window's state (WinRow) and result.
//                       The peek classifier (:1505-1597, header parse results from the probe records, pending_total_cw_,
//                       the float32 CFO clamp, what the next pass demodulates), the small-frame classifier (:1806-1853), the
//                       timing-recovery walk (:1859-1965) and the consumed rule (:1994-2013) are its cases.
//   win_list_kernel     one block: the windows that wait for a demodulation, one ascending list per span length (a pass has at
//                       most five: the control span, and 1, 2, 3, 4 codewords of the data profile) with offset and
//                       ria_frame_meta per entry; or the ascending list of windows that wait for a robust CW0 decode.  Built by
//                       acq_block_scan over ALL windows in order, so no result depends on scheduling.
//   win_scatter_kernel  the compact rows of a pass's demodulations (soft bits, status) to their windows' rows
//
// The demodulations, the CW0 decodes (dframe_probe_kernel) and decodeFrame itself are the existing launchers' and kernels',
// unchanged.  Plain C++ and vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "decode_frame_kernels.hip.h"
#include "window_rules.hpp"

namespace ria {

constexpr int kWinGroups = 5;           // span lengths of a call: [0] the control span n_ctl, [c] c codewords of the data profile
constexpr uint8_t kWinNoJob = 0xFF;
enum { kWinProbeR14 = 0, kWinProbeRate = 1 };      // probe records of a window
enum { kWinPhasePeek = 0, kWinPhasePass2, kWinPhaseSmall, kWinPhaseRecover };
enum { kWinInit = 0, kWinPeek1, kWinPeekR14, kWinPeekRate, kWinEscalate, kWinPass2, kWinPrepDecode, kWinDecoded1, kWinSmall1,
       kWinSmallR14, kWinSmallRate, kWinSmallExact, kWinDecoded2, kWinRecInit, kWinRecDemod, kWinRecDecoded, kWinFinal };

struct WinCtl {                  // read back by the host once per demodulation pass
    unsigned int n[kWinGroups];  // list lengths
    unsigned int pad_[3];
};

struct WinRow {                  // 32 bytes of per-window state
    int32_t start;               // sync_position_ as detected (sync_start)
    int32_t frame_len;           // frame_len
    float sync_cfo;              // sync_cfo_ == last_cfo_
    float fading;                // last_fading_index_
    float peek_cfo;              // estimatedCFO() of the peek span
    uint8_t open;                // the ladder still runs for this window
    uint8_t job;                 // span group the window waits to be demodulated at, kWinNoJob if none
    uint8_t probe;               // 1 / 2: waits for the robust CW0 decode at R1/4 / at the rate
    uint8_t decode;              // takes part in the next decodeFrame
    uint8_t cand;                // index into kAcqDelta of the span demodulated last
    uint8_t phase;               // kWinPhase*
    uint8_t candidates;          // spans demodulated at a timing candidate, the primary included
    uint8_t adopted;             // index into kAcqDelta of the reported candidate
    uint8_t pad_[4];
};

struct WinArgs {
    int n, window_len; long long stride;
    const ria_acq_params* params; ria_acq_result* acq;
    const ria_control_result* cres; const uint8_t* cframes; const ria_frame_status* cfst;   // the control hypothesis, per window
    int len[kWinGroups];
    int bps, is_qam, rate_is_r14, retry;
    WinRow* row; WinCtl* ctl;
    FrameList list[kWinGroups];
    const float* llr_c; const ria_frame_status* fst_c;   // compact rows of the pass's demodulations, group after group
    int base[kWinGroups], cnt[kWinGroups];               // scatter: first compact row and rows of each group
    float* llr_w; ria_frame_status* fst_w; int llr_stride; int32_t* n_llr_d;   // per window
    const DfProbe* probe; uint32_t* plist; DfCtl* pctl;
    const uint8_t* df_frames; int df_row; const ria_dframe_result* df_res;
    uint8_t* frame_out; int frame_row; ria_window_result* result; ria_frame_status* fst_out;   // fst_out nullable
};

__device__ inline int win_group(const WinArgs& A, int len) {
    for (int g = 0; g < kWinGroups; ++g) if (A.len[g] == len) return g;
    return kWinNoJob;     // cannot happen: every span length of the ladder is one of the five
}

__device__ inline void win_close(WinRow& R) { R.open = 0; R.job = kWinNoJob; R.probe = 0; R.decode = 0; }

// the result decodeFrame left for window w becomes the window's: DecodeResult, frame bytes, the span's status
__device__ inline void win_adopt(const WinArgs& A, int w) {
    A.result[w].frame = A.df_res[w];
    const uint8_t* src = A.df_frames + static_cast<size_t>(w) * A.df_row;
    uint8_t* dst = A.frame_out + static_cast<size_t>(w) * A.frame_row;
    for (int q = 0; q < A.df_row; ++q) dst[q] = src[q];
    if (A.fst_out) A.fst_out[w] = A.fst_w[w];
    A.acq[w].cfo_hz = A.fst_w[w].cfo_hz;
}

// the next timing candidate after R.cand whose span fits the window (ria_gpu_rx_acquire_batch's fit rule); closes the window
// when there is none
__device__ inline void win_next_candidate(const WinArgs& A, WinRow& R) {
    for (int k = R.cand + 1; k < kAcqCandidates; ++k) {
        if (acq_fits(R.start + kAcqDelta[k], R.frame_len, A.window_len)) {
            R.cand = static_cast<uint8_t>(k);
            R.job = static_cast<uint8_t>(win_group(A, R.frame_len));
            return;
        }
    }
    win_close(R);
}

// a pass's process() on window w: false (fewer than 648 soft bits) ends the window as the reference returns to SEARCHING
// (:1352-1360); else the fading index and the CFO feedback (:1376, :1414-1434)
__device__ inline bool win_pass_done(const WinArgs& A, int w, WinRow& R) {
    const ria_frame_status fs = A.fst_w[w];
    R.job = kWinNoJob;
    if (fs.n_llr < kDfBlock) {
        if (A.fst_out) A.fst_out[w] = fs;
        win_close(R);
        return false;
    }
    R.fading = fs.fading_index;
    R.sync_cfo = win_clamp_cfo(fs.cfo_hz, R.sync_cfo);
    return true;
}

__global__ __launch_bounds__(256) void win_stage_kernel(WinArgs A, int stage) {
    const int w = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
    if (w >= A.n) return;
    WinRow R = A.row[w];
    ria_window_result& O = A.result[w];
    const DfProbe* P14 = A.probe + static_cast<size_t>(kWinProbeR14) * A.n + w;
    const DfProbe* PR = A.probe + static_cast<size_t>(kWinProbeRate) * A.n + w;
    switch (stage) {
    case kWinInit: {
        const ria_acq_result a = A.acq[w];
        const ria_control_result c = A.cres[w];
        R = WinRow{};
        R.start = a.sync_start; R.frame_len = A.len[0]; R.sync_cfo = A.params[w].known_cfo_hz;
        R.job = kWinNoJob;
        ria_window_result o{};
        o.next_pos = -1;
        o.sync_cfo_hz = R.sync_cfo;
        if (!a.accepted) o.outcome = RIA_WIN_NOT_ACCEPTED;
        else if (!c.tried) o.outcome = RIA_WIN_BURST;
        else if (c.success) {                                  // :1298-1335
            o.outcome = RIA_WIN_CONTROL_PROFILE;
            o.frame.success = 1; o.frame.codewords_ok = 1; o.frame.frame_type = c.frame_type; o.frame.header_total_cw = 1;
            o.frame.frame_bytes = kCtlFrameBytes;
            for (int q = 0; q < kCtlFrameBytes; ++q) A.frame_out[static_cast<size_t>(w) * A.frame_row + q] = A.cframes[static_cast<size_t>(w) * kCtlFrameBytes + q];
            o.frame_len = A.len[0];
            o.next_pos = a.sync_start + A.len[0];
            o.fading_index = A.cfst[w].fading_index;
            if (A.fst_out) A.fst_out[w] = A.cfst[w];
        } else {
            o.outcome = RIA_WIN_DECODED;
            R.open = 1; R.job = 0; R.phase = kWinPhasePeek; R.candidates = 1;
            A.acq[w].cfo_hz = 0.0f;      // the control span's until a span of the data profile is reported
        }
        O = o;
        break;
    }
    case kWinPeek1:
        if (R.open && R.job == 0 && R.phase == kWinPhasePeek) {
            const float est = A.fst_w[w].cfo_hz;
            if (!win_pass_done(A, w, R)) break;
            R.peek_cfo = est;
            const int s1 = A.fst_w[w].n_llr;
            if (s1 < 2 * kDfBlock) R.probe = 1;                                                        // :1511
            else if (s1 < 4 * kDfBlock && A.is_qam) { O.peek = RIA_PEEK_QAM_PARTIAL; O.pending_total_cw = 4; }   // :1582-1597
            else { O.peek = RIA_PEEK_DIRECT; R.decode = 1; }
        }
        break;
    case kWinPeekR14:
        if (R.open && R.probe == 1 && R.phase == kWinPhasePeek) {
            const DfProbe p = *P14;
            R.probe = 0;
            O.tries_peek_r14 = p.tries;
            if (p.magic && p.valid && p.total_cw == 1) { O.peek = RIA_PEEK_R14_ONE; R.decode = 1; }
            else if (p.magic && p.valid) { O.peek = RIA_PEEK_R14_MULTI; O.pending_total_cw = p.total_cw; }
            else if (!A.rate_is_r14) R.probe = 2;
            else { O.peek = RIA_PEEK_FAILED; O.pending_total_cw = 4; }
        }
        break;
    case kWinPeekRate:
        if (R.open && R.probe == 2 && R.phase == kWinPhasePeek) {
            const DfProbe p = *PR;
            R.probe = 0;
            O.tries_peek_rate = p.tries;
            if (p.magic && p.valid && p.total_cw == 1) { O.peek = RIA_PEEK_RATE_ONE; R.decode = 1; }
            else if (p.magic && p.valid) { O.peek = RIA_PEEK_RATE_MULTI; O.pending_total_cw = p.total_cw; }
            else if (p.magic) { O.peek = RIA_PEEK_RATE_BAD_HEADER; O.pending_total_cw = 4; }
            else { O.peek = RIA_PEEK_FAILED; O.pending_total_cw = 4; }
        }
        break;
    case kWinEscalate:
        if (R.open && R.phase == kWinPhasePeek && O.pending_total_cw > 0) {
            const int len = win_samples_for_cw(A.bps, O.pending_total_cw);
            R.frame_len = len;
            if (static_cast<long long>(R.start) + len > A.window_len) { O.outcome = RIA_WIN_NEED_SAMPLES; O.need_samples = len; win_close(R); }
            else if (O.pending_total_cw > 4) { O.outcome = RIA_WIN_TOO_LONG; win_close(R); }
            else { R.job = O.pending_total_cw; R.phase = kWinPhasePass2; }
        }
        break;
    case kWinPass2:
        if (R.open && R.job != kWinNoJob && R.phase == kWinPhasePass2) {
            if (win_pass_done(A, w, R)) R.decode = 1;
        }
        break;
    case kWinPrepDecode:
        A.n_llr_d[w] = (R.open && R.decode) ? A.fst_w[w].n_llr : 0;
        break;
    case kWinDecoded1:
        if (R.open && R.decode) {
            R.decode = 0;
            win_adopt(A, w);
            if (!A.df_res[w].success && A.len[1] <= R.frame_len) { O.small_frame = 1; R.job = 1; R.phase = kWinPhaseSmall; }   // :1806-1810
            else if (A.df_res[w].success) win_close(R);
            else R.phase = kWinPhaseSmall;
        }
        break;
    case kWinSmall1:
        if (R.open && R.job == 1 && R.phase == kWinPhaseSmall) {
            R.job = kWinNoJob;
            if (A.fst_w[w].n_llr >= kDfBlock) R.probe = 1;     // short_bits.size() >= LDPC_BLOCK
        }
        break;
    case kWinSmallR14:
    case kWinSmallRate:
        if (R.open && R.phase == kWinPhaseSmall && R.probe == (stage == kWinSmallR14 ? 1 : 2)) {
            const DfProbe p = stage == kWinSmallR14 ? *P14 : *PR;
            R.probe = 0;
            const uint8_t at_rate = stage == kWinSmallR14 ? 0 : 0x10;
            if (stage == kWinSmallR14) O.tries_small_r14 = p.tries; else O.tries_small_rate = p.tries;
            if (p.magic && p.valid && p.total_cw == 1) {                                   // :1823-1827
                O.small_frame = static_cast<uint8_t>(2 | at_rate); R.decode = 1; R.frame_len = A.len[1];
            } else if (p.magic && p.valid && p.total_cw < 4) {                             // :1828-1843
                const int exact = min(win_samples_for_cw(A.bps, p.total_cw), R.frame_len);
                O.small_frame = static_cast<uint8_t>(3 | at_rate); R.job = static_cast<uint8_t>(win_group(A, exact)); R.frame_len = exact;
            } else if (stage == kWinSmallR14 && !A.rate_is_r14) R.probe = 2;
        }
        break;
    case kWinSmallExact:
        if (R.open && R.job != kWinNoJob && R.phase == kWinPhaseSmall) { R.job = kWinNoJob; R.decode = 1; }
        break;
    case kWinDecoded2:
        if (R.open && R.decode) { R.decode = 0; win_adopt(A, w); }
        break;
    case kWinRecInit:
        if (R.open) {
            const ria_dframe_result f = O.frame;
            R.phase = kWinPhaseRecover;
            if (!f.success && f.codewords_ok == 0 && A.retry) win_next_candidate(A, R);    // :1859
            else win_close(R);
        }
        break;
    case kWinRecDemod:
        if (R.open && R.job != kWinNoJob && R.phase == kWinPhaseRecover) {
            R.job = kWinNoJob;
            R.candidates = static_cast<uint8_t>(R.candidates + 1);
            if (A.fst_w[w].n_llr >= kDfBlock) R.decode = 1;      // retry_ok
            else win_next_candidate(A, R);
        }
        break;
    case kWinRecDecoded:
        if (R.open && R.decode) {
            R.decode = 0;
            const ria_dframe_result f = A.df_res[w];
            if (f.success || f.codewords_ok > 0) {                // :1915-1939
                win_adopt(A, w);
                R.sync_cfo = win_clamp_cfo(A.fst_w[w].cfo_hz, R.sync_cfo);
                R.fading = A.fst_w[w].fading_index;
                R.adopted = R.cand;
                win_close(R);
            } else win_next_candidate(A, R);
        }
        break;
    default: {   // kWinFinal
        if (O.outcome == RIA_WIN_CONTROL_PROFILE || O.outcome == RIA_WIN_NOT_ACCEPTED || O.outcome == RIA_WIN_BURST) break;
        ria_acq_result& a = A.acq[w];
        const int delta = kAcqDelta[R.adopted];
        O.frame_len = R.frame_len;
        O.sync_cfo_hz = R.sync_cfo; O.peek_cfo_hz = R.peek_cfo; O.fading_index = R.fading;
        a.candidates = R.candidates;
        if (O.outcome == RIA_WIN_DECODED) {
            a.delta = static_cast<int16_t>(delta);
            a.frame_start = R.start + delta;
            const ria_dframe_result f = O.frame;
            const int type = f.frame_bytes >= 3 ? A.frame_out[static_cast<size_t>(w) * A.frame_row + 2] : 0;
            O.next_pos = a.frame_start + win_consumed(R.frame_len, f.success != 0, f.frame_bytes, type, f.codewords_ok, f.codewords_failed, A.bps);
        }
        break;
    }
    }
    A.row[w] = R;
}

// mode 0: the demodulation lists, one per span group, of the windows with a job; mode 1 / 2: the list of windows that wait
// for the robust CW0 decode at R1/4 / at the rate (list 0 of the probe kernel's DfArgs)
__global__ __launch_bounds__(kAcqScanThreads) void win_list_kernel(WinArgs A, int mode) {
    int running[kWinGroups] = {0, 0, 0, 0, 0};
    for (int base = 0; base < A.n; base += kAcqScanThreads) {
        const int w = base + static_cast<int>(threadIdx.x);
        WinRow R{};
        R.job = kWinNoJob;
        if (w < A.n) R = A.row[w];
        if (mode != 0) {
            const bool flag = w < A.n && R.open && R.probe == mode;
            int total;
            const int pos = running[0] + acq_block_scan(flag, &total);
            if (flag) A.plist[pos] = static_cast<uint32_t>(w);
            running[0] += total;
            continue;
        }
        for (int g = 0; g < kWinGroups; ++g) {
            const bool flag = w < A.n && R.open && R.job == g;
            int total;
            const int pos = running[g] + acq_block_scan(flag, &total);
            if (flag) {
                const ria_acq_params p = A.params[w];
                const int s = R.start + (R.phase == kWinPhaseRecover ? kAcqDelta[R.cand] : 0);
                const FrameList& l = A.list[g];
                l.offset[pos] = static_cast<uint64_t>(w) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(s);
                ria_frame_meta m;
                m.cfo_hz = R.sync_cfo;
                m.flags = 0u;        // the control hypothesis's process() has consumed the one-shot marker (ofdm_chirp_waveform.cpp:421-440)
                m.abs_position = p.abs_base + static_cast<uint64_t>(s);
                l.meta[pos] = m;
                l.window[pos] = static_cast<uint32_t>(w);
                l.state[pos] = R.cand;
            }
            running[g] += total;
        }
    }
    if (threadIdx.x == 0) {
        if (mode != 0) A.pctl->n[0] = static_cast<unsigned>(running[0]);
        else for (int g = 0; g < kWinGroups; ++g) A.ctl->n[g] = static_cast<unsigned>(running[g]);
    }
}

// one block per compact row of the pass: its soft bits (bit copies) and status to its window's row
__global__ __launch_bounds__(256) void win_scatter_kernel(WinArgs A, int total) {
    for (int i = blockIdx.x; i < total; i += gridDim.x) {
        int g = 0;
        while (g + 1 < kWinGroups && (A.cnt[g] == 0 || i >= A.base[g] + A.cnt[g])) ++g;
        const uint32_t w = A.list[g].window[i - A.base[g]];
        const int made = (A.len[g] / 1152 - 2) * A.bps;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(A.llr_c) + static_cast<size_t>(i) * A.llr_stride;
        uint32_t* dst = reinterpret_cast<uint32_t*>(A.llr_w) + static_cast<size_t>(w) * A.llr_stride;
        for (int q = threadIdx.x; q < made && q < A.llr_stride; q += 256) dst[q] = src[q];
        if (threadIdx.x == 0) A.fst_w[w] = A.fst_c[i];
    }
}

}  // namespace ria
