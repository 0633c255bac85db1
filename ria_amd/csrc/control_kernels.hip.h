// ria_amd/csrc/control_kernels.hip.h — device side of the variable-length demodulator call and of the control hypothesis
// (ria_gpu_demod_var_batch, ria_gpu_rx_control_batch, ria_gpu_control_acquire_batch in include/ria_gpu.h): what
// gui::StreamingDecoder does with a connected-mode window before it tries the data profile
// (src/gui/modem/streaming_decoder.cpp:1268-1344).
//
//   var_offsets_kernel    frame f of a call without offsets starts at f * n_samples: the split demodulator derives its
//                         default start from whole symbols, a span need not be one
//   control_plan_kernel   acq_plan_kernel's acceptance rule (:752-771) for a span of n_samples instead of a fixed frame, and
//                         the windows whose detector reports the burst marker left out under RIA_BURST_INTERLEAVE (:1087-1092)
//   control_decode_kernel one wave per demodulated span: robustDecodeSingleCW on its first 648 soft bits (:1290), then the
//                         reference's tests in its order - ok, 4 bytes, magic, truncation to 20 bytes, parseHeader,
//                         total_cw == 1, isControlFrame - and the row's outputs, at the span's window where a list is given
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"
#include "ldpc_fast.hip.h"
#include "recovery_kernels.hip.h"

namespace ria {

constexpr int kCtlFrameBytes = 20;   // v2::getBytesPerCodeword(R1_4): a control frame is one R1/4 codeword's payload

__global__ __launch_bounds__(256) void var_offsets_kernel(uint64_t* __restrict__ off, int n_frames, int n_samples) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_frames) off[f] = static_cast<uint64_t>(f) * static_cast<uint64_t>(n_samples);
}

struct ControlArgs {
    // plan
    const ria_lts_result* lts; const ria_acq_params* params;
    int n_windows, window_len, n_samples, skip_marked;
    long long stride;
    ria_acq_result* acq;                 // [n_windows], nullable in the pre-synced call
    AcqCtl* ctl;
    FrameList list;
    // decode
    const float* llr; int llr_stride;    // compact rows of the demodulated spans
    const ria_frame_status* fst;         // compact
    const uint32_t* window;              // nullable: output row of compact row i (else i)
    int n_rows;
    const uint16_t* crc_bit; const uint16_t* crc_init;
    uint8_t* frame_out; ria_control_result* result; ria_frame_status* fst_out;   // fst_out nullable
};

__global__ __launch_bounds__(kAcqScanThreads) void control_plan_kernel(ControlArgs A) {
    int running = 0;
    for (int base = 0; base < A.n_windows; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        bool acc = false, run = false;
        int start = -1;
        uint32_t burst = 0;
        if (b < A.n_windows) {
            const ria_lts_result r = A.lts[b];
            const ria_acq_params p = A.params[b];
            const bool det = r.detected != 0;
            start = det ? r.start_sample : -1;
            burst = det && r.burst_interleaved ? 1u : 0u;
            acc = det && !(r.correlation < p.min_confidence) && acq_fits(start, A.n_samples, A.window_len);
            run = acc && !(A.skip_marked && burst);
            ria_acq_result o;
            o.detected = det ? 1 : 0;
            o.accepted = acc ? 1 : 0;
            o.sync_start = start;
            o.frame_start = acc ? start : -1;
            o.correlation = r.correlation;
            o.cfo_hz = 0.0f;
            o.delta = 0;
            o.candidates = run ? 1 : 0;
            o.burst_interleaved = static_cast<uint8_t>(burst);
            o.reserved = 0;
            A.acq[b] = o;
        }
        int total;
        const int pos = running + acq_block_scan(run, &total);
        if (run) {
            const ria_acq_params p = A.params[b];
            A.list.offset[pos] = static_cast<uint64_t>(b) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(start);
            ria_frame_meta m;
            m.cfo_hz = p.known_cfo_hz;
            m.flags = burst;
            m.abs_position = p.abs_base + static_cast<uint64_t>(start);
            A.list.meta[pos] = m;
            A.list.window[pos] = static_cast<uint32_t>(b);
            A.list.state[pos] = 0;
        }
        running += total;
    }
    if (threadIdx.x == 0) { A.ctl->n_list = static_cast<unsigned>(running); A.ctl->fault = 0u; }
}

// c: the R1/4 code of the control handle.  A row whose span gave fewer than 648 soft bits (process() false) is not decoded.
template <class S>
__global__ __launch_bounds__(64) void control_decode_kernel(FastCode c, ControlArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    FastState<S> st;
    fast_load_tables(st, c, smem, lane);
    const int nb = (c.k + 7) / 8;
    for (int q = blockIdx.x; q < A.n_rows; q += gridDim.x) {
        const uint32_t row = A.window ? A.window[q] : static_cast<uint32_t>(q);
        const ria_frame_status fs = A.fst[q];
        const bool process_ok = fs.n_llr >= 648;
        bool ok = false, magic = false, valid = false, ctl = false;
        int it = 0, tries = 0, plen = 0, total = 0;
        uint8_t* d = smem + 128;
        if (process_ok) {       // wave-uniform
            const float* l = A.llr + static_cast<size_t>(q) * A.llr_stride;
            const int ln = opaque_lane(lane);
#pragma unroll
            for (int r = 0; r < S::NC; ++r) { const uint32_t j = c.col_at[ln + 64 * r]; st.li[r] = (j != 0xFFFFu) ? llr_canon(l[j]) : 0.0f; }
#pragma unroll
            for (int r = 0; r < S::NR; ++r) { const uint32_t i = c.check_at[ln + 64 * r]; st.lp[r] = (i != 0xFFFFu) ? llr_canon(l[c.k + i]) : kIdleRowLlr; }
#pragma unroll 1
            for (int f = 0; f < kNumFactors && !ok; ++f) { it = fast_decode(st, c, smem, kFactors[f], c.max_iter, lane, &ok); ++tries; }
            // as dframe_probe_kernel: the decoded bytes go to a scratch row behind the hard-bit masks, in the c2v area
            fast_pack(st, c, smem, d, nb, lane);
            magic = ok && nb >= 4 && d[0] == 0x55 && d[1] == 0x4C;
            if (magic) {
                RecCtx x{};
                x.crc_bit = A.crc_bit; x.crc_init = A.crc_init; x.lane = lane;
                const int len = nb > kCtlFrameBytes ? kCtlFrameBytes : nb;          // data_r14.resize(bpc_r14)
                if (rec_parse_header(x, d, len, &ctl, &plen)) { valid = true; total = ctl ? 1 : d[12]; }
            }
        }
        const bool success = valid && total == 1 && ctl;                            // isControlFrame(hdr.type)
        if (lane < kCtlFrameBytes) A.frame_out[static_cast<size_t>(row) * kCtlFrameBytes + lane] = success ? d[lane] : static_cast<uint8_t>(0);
        if (lane == 0) {
            ria_control_result o{};
            o.process_ok = process_ok ? 1 : 0;
            o.cw_ok = ok ? 1 : 0;
            o.magic = magic ? 1 : 0;
            o.header_valid = valid ? 1 : 0;
            o.total_cw = static_cast<uint8_t>(valid ? total : 0);
            o.frame_type = magic ? d[2] : static_cast<uint8_t>(0);
            o.success = success ? 1 : 0;
            o.tries = static_cast<uint8_t>(tries);
            o.seq = valid ? static_cast<uint16_t>((d[4] << 8) | d[5]) : static_cast<uint16_t>(0);
            o.iterations = static_cast<uint16_t>(it);
            o.n_llr = fs.n_llr;
            o.tried = 1;
            A.result[row] = o;
            if (A.fst_out) A.fst_out[row] = fs;
            if (A.acq) A.acq[row].cfo_hz = fs.cfo_hz;
        }
        wave_sync();     // the scratch row is read above, the next decode rewrites the c2v area
    }
}

}  // namespace ria
