// ria_amd/csrc/burst_kernels.hip.h — device side of ria_gpu_rx_burst_batch (include/ria_gpu.h): burst-interleaved groups
// (StreamingDecoder::accumulateBurstFrames / tryDemodulateNextBurstFrame / finalizeBurstGroup, streaming_decoder.cpp:3065-3239)
// and burst continuation behind a decoded data frame (:2015-2114), on the work lists of acquire_kernels.hip.h.
//
// Round f of the call demodulates physical frame f of every window still live.  Two lists per round, both in ascending
// window order: the group list (demodulated only; the group is decoded once it is complete) and the continuation list
// (demodulated and decoded).  Between two rounds burst_step_kernel looks at what round f-1 produced for each entry, takes
// the reference's decisions for frame f (soft bits present, CFO chain, decode outcome, fit, energy gate) and writes the
// entry's next frame beside a keep flag; burst_list_kernel compacts the kept entries with the block scan, so the lists -
// and with them every result - do not depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "acquire_kernels.hip.h"

namespace ria {

constexpr int kBurstSlots = RIA_BURST_MAX_FRAMES;   // output slots per window
constexpr int kBurstMaxGroup = 8;
constexpr int kBurstGateSkip = 1024;                // the gate skips the training area (:3156)
constexpr int kBurstGateLen = 5000;                 // and sums at most this many squares (:3157)
constexpr int kBurstStepWaves = 2;                  // windows per workgroup of burst_step_kernel (2 x 20 000 B of LDS)
constexpr int kBurstFrameBits = 2592;               // soft bits decodeFixedFrame reads

struct BurstCtl {                // read back by the host once per round
    unsigned int n_group;        // entries of the next round's group list
    unsigned int n_cont;         // entries of the next round's continuation list
    unsigned int n_done;         // complete groups listed for the decode
    unsigned int fault;          // a decode status carried the work-queue fault marker
};

struct BurstArgs {
    const float* samples;
    long long stride;
    int n_windows, window_len, frame_samples, group_size;
    uint32_t flags;
    const ria_lts_result* lts;
    const ria_acq_params* params;
    ria_burst_result* res;
    BurstCtl* ctl;
    // frame 0 of continuation windows: the acquire rounds' own outputs, one row per window
    AcqCtl* acq_ctl; FrameList acq_first; ria_acq_result* acq0;
    const uint8_t* info0; const ria_decode_status* dst0; const ria_frame_status* fst0;
    uint32_t* c_win0;            // the continuation windows in list order (the acquire rounds overwrite their lists)
    // round state
    FrameList g_cur, c_cur, g_stage, c_stage;
    int n_g, n_c, round;         // round = index of the physical frame the NEXT round would demodulate
    int first;                   // 1: the continuation entries are c_win0 and their frame-0 results are indexed by window
    const ria_frame_status* g_fst;                                                         // compact, group list order
    const ria_frame_status* c_fst; const ria_decode_status* c_dst; const uint8_t* c_info;  // compact, continuation list order
    int info_bytes;
    // outputs, kBurstSlots per window (fst_out, cfo_used, rms nullable)
    uint8_t* info_out; ria_decode_status* dst_out; ria_frame_status* fst_out; float* cfo_used; float* rms;
    // complete groups
    uint32_t* gpos;              // [n_windows * kBurstMaxGroup]: row of (window, physical frame) in that round's list
    uint32_t* done;              // complete groups' windows, ascending
    const float* gllr;           // soft bits of list row i, physical frame f at gllr + (i * group_size + f) * llr_stride
    int llr_stride;
    float* dec_in;               // [n_done * group_size][kBurstFrameBits] logical soft bits
    const uint8_t* dec_info; const ria_decode_status* dec_dst; int n_done;
};

// StreamingDecoder's drift clamp between the frames of a burst (:1397-1406, :2075-2082, :3190-3197)
__device__ inline float burst_cfo_next(float used, float corrected) {
    const float drift = corrected - used;
    if (fabsf(drift) > 2.0f) corrected = used + copysignf(2.0f, drift);
    return corrected;
}

// isControlFrame || isConnectFrame (frame_v2.hpp:222-228, :348-351)
__device__ inline bool burst_non_data_type(int t) {
    return t == 0x10 || t == 0x11 || t == 0x16 || t == 0x17 || t == 0x20 || t == 0x21 || t == 0x15 || t == 0x40 ||
           t == 0x12 || t == 0x13 || t == 0x14;
}

// One block: acceptance (as acq_plan_kernel), the mode of every window, the ria_burst_result fields known before any
// demodulation, the round-0 group list (frame 0 with the marker flag, demodulated only) and the round-0 list of the acquire
// rounds for the continuation-mode windows.
__global__ __launch_bounds__(kAcqScanThreads) void burst_plan_kernel(BurstArgs A) {
    int run_g = 0, run_c = 0;
    for (int base = 0; base < A.n_windows; base += kAcqScanThreads) {
        const int b = base + static_cast<int>(threadIdx.x);
        int mode = 0, start = -1;
        uint32_t burst = 0;
        ria_acq_params p{};
        if (b < A.n_windows) {
            const ria_lts_result r = A.lts[b];
            p = A.params[b];
            const bool det = r.detected != 0;
            start = det ? r.start_sample : -1;
            burst = det && r.burst_interleaved ? 1u : 0u;
            const bool acc = det && !(r.correlation < p.min_confidence) && acq_fits(start, A.frame_samples, A.window_len);
            mode = !acc ? 0 : ((A.flags & RIA_BURST_INTERLEAVE) && burst) ? 2 : 1;
            ria_burst_result o{};
            o.detected = det ? 1 : 0;
            o.accepted = acc ? 1 : 0;
            o.sync_start = start;
            o.frame_start = acc ? start : -1;
            o.correlation = r.correlation;
            o.cfo_hz = acc ? p.known_cfo_hz : 0.0f;
            o.burst_interleaved = static_cast<uint8_t>(burst);
            o.mode = static_cast<uint8_t>(mode);
            A.res[b] = o;
            ria_acq_result a{};
            a.detected = o.detected; a.accepted = o.accepted; a.sync_start = start; a.frame_start = o.frame_start;
            a.correlation = r.correlation; a.burst_interleaved = static_cast<uint8_t>(burst);
            A.acq0[b] = a;
        }
        int tot_g, tot_c;
        const int pg = run_g + acq_block_scan(mode == 2, &tot_g);
        const int pc = run_c + acq_block_scan(mode == 1, &tot_c);
        if (mode != 0) {
            ria_frame_meta m;
            m.cfo_hz = p.known_cfo_hz;
            m.flags = burst;          // mode 2 implies the marker
            m.abs_position = p.abs_base + static_cast<uint64_t>(start);
            const uint64_t off = static_cast<uint64_t>(b) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(start);
            if (mode == 2) {
                A.g_cur.offset[pg] = off; A.g_cur.meta[pg] = m; A.g_cur.window[pg] = static_cast<uint32_t>(b);
                A.gpos[static_cast<size_t>(b) * kBurstMaxGroup] = static_cast<uint32_t>(pg);
            } else {
                A.acq_first.offset[pc] = off; A.acq_first.meta[pc] = m; A.acq_first.window[pc] = static_cast<uint32_t>(b);
                A.acq_first.state[pc] = 0;
                A.c_win0[pc] = static_cast<uint32_t>(b);
            }
            if (A.cfo_used) A.cfo_used[static_cast<size_t>(b) * kBurstSlots] = p.known_cfo_hz;
        }
        run_g += tot_g; run_c += tot_c;
    }
    if (threadIdx.x == 0) {
        A.ctl->n_group = static_cast<unsigned>(run_g); A.ctl->n_cont = static_cast<unsigned>(run_c);
        A.ctl->n_done = 0u; A.ctl->fault = 0u;
        A.acq_ctl->n_list = static_cast<unsigned>(run_c); A.acq_ctl->fault = 0u;
    }
}

// The energy gate of one block (:3154-3171 = :2047-2059) by one wavefront: the lanes load the samples coalesced, square
// them and park the squares in LDS; lane 0 then adds them in ascending order - the reference's float32 chain, which no
// tree can reproduce - reading four squares per LDS access.  Returns the rms in every lane.
__device__ inline float burst_gate_rms(const float* __restrict__ x, int len, float* __restrict__ sq, int lane) {
    for (int i = lane; i < len; i += 64) { const float v = x[i]; sq[i] = v * v; }
    wave_sync();
    float rms = 0.0f;
    if (lane == 0 && len > 0) {
        float acc = 0.0f;
        int i = 0;
        for (; i + 4 <= len; i += 4) {
            const float4 q = *reinterpret_cast<const float4*>(sq + i);
            acc += q.x; acc += q.y; acc += q.z; acc += q.w;
        }
        for (; i < len; ++i) acc += sq[i];
        rms = sqrtf(acc / static_cast<float>(len));
    }
    wave_sync();                  // the squares are dead: the wave may reuse its LDS
    return __shfl(rms, 0);
}

// One wavefront per entry of the two lists of the round that has just run (frame f = round - 1 of its window): what the
// reference does between process() of frame f and process() of frame f + 1.
__global__ __launch_bounds__(64 * kBurstStepWaves) void burst_step_kernel(BurstArgs A) {
    __shared__ __attribute__((aligned(16))) float sq_all[kBurstStepWaves][kBurstGateLen];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * kBurstStepWaves + wave;
    if (e >= A.n_g + A.n_c) return;                       // wave-uniform; the kernel has no block-wide barrier
    const bool group = e < A.n_g;
    const int i = group ? e : e - A.n_g;
    const uint32_t w = group ? A.g_cur.window[i] : A.first ? A.c_win0[i] : A.c_cur.window[i];
    const int f = A.round - 1;
    const size_t slot = static_cast<size_t>(w) * kBurstSlots + f;
    const size_t ci = (!group && A.first) ? w : static_cast<size_t>(i);   // row of the entry's continuation outputs
    ria_burst_result* rp = A.res + w;             // fields one by one: a local copy of the record would live in scratch
    const int sync_start = rp->sync_start;
    float cfo = rp->cfo_hz;
    int frames = rp->frames, frames_decoded = rp->frames_decoded;
    int frame_start = rp->frame_start, delta = 0, candidates = 0;
    const ria_frame_status* fp = group ? A.g_fst + i : A.c_fst + ci;
    const int n_llr = fp->n_llr;
    int stop = RIA_BURST_STOP_NONE;
    bool go = true, complete = false;
    if (n_llr == 0) {                                  // process() false / no soft bits: nothing of the frame counts
        stop = RIA_BURST_STOP_PROCESS; go = false;
    } else {
        frames += 1;
        cfo = burst_cfo_next(cfo, fp->cfo_hz);
        if (group) {
            if (A.fst_out && lane < 8) reinterpret_cast<uint32_t*>(A.fst_out + slot)[lane] = reinterpret_cast<const uint32_t*>(fp)[lane];
            if (f + 1 == A.group_size) { complete = true; go = false; }
        }
    }
    if (!group) {
        const ria_decode_status* sp = A.c_dst + ci;
        const bool ok0 = sp->cw_ok[0], ok1 = sp->cw_ok[1], ok2 = sp->cw_ok[2], ok3 = sp->cw_ok[3];
        if (sp->reserved[1] == kDecodeFaultMarker && lane == 0) atomicOr(&A.ctl->fault, 1u);
        if (f == 0 || n_llr != 0) {                    // the block's outputs go to slot f
            const uint8_t* src = A.c_info + ci * A.info_bytes;
            uint8_t* dst = A.info_out + slot * A.info_bytes;
            for (int q = lane; q < A.info_bytes; q += 64) dst[q] = src[q];
            if (lane < static_cast<int>(sizeof(ria_decode_status)))
                reinterpret_cast<uint8_t*>(A.dst_out + slot)[lane] = reinterpret_cast<const uint8_t*>(sp)[lane];
            if (A.fst_out && lane < 8) reinterpret_cast<uint32_t*>(A.fst_out + slot)[lane] = reinterpret_cast<const uint32_t*>(fp)[lane];
        }
        const bool any = ok0 | ok1 | ok2 | ok3;
        if (f == 0) {
            const ria_acq_result* ap = A.acq0 + w;
            frame_start = ap->frame_start; delta = ap->delta; candidates = ap->candidates;
            frames_decoded = 1;
            if (go) {
                const bool success = ok0 && ok1 && ok2 && ok3 && sp->frame_valid;
                go = false;
                if (A.flags & RIA_BURST_NO_CONTINUE) stop = RIA_BURST_STOP_NONE;
                else if (!success) stop = RIA_BURST_STOP_DECODE;
                else if (burst_non_data_type(A.c_info[ci * A.info_bytes + 2])) stop = RIA_BURST_STOP_NOT_DATA;
                else if (delta != 0) stop = RIA_BURST_STOP_RECOVERED;
                else go = true;
            }
        } else if (go) {
            frames_decoded += 1;
            if (!any) { stop = RIA_BURST_STOP_DECODE; go = false; }
            else if (f == kBurstSlots - 1) { stop = RIA_BURST_STOP_LIMIT; go = false; }
        }
    }
    // the next block: fit, energy gate
    const long long s = static_cast<long long>(sync_start) + static_cast<long long>(A.round) * A.frame_samples;
    // (round < kBurstSlots wherever go is set: a continuation has stopped with STOP_LIMIT at f == 8, a group at group_size <= 8)
    if (go && s + A.frame_samples > A.window_len) { stop = RIA_BURST_STOP_WINDOW; go = false; }
    if (go) {                                             // wave-uniform
        const int skip = min(kBurstGateSkip, A.frame_samples);
        const int len = min(A.frame_samples - skip, kBurstGateLen);
        const float* x = A.samples + static_cast<size_t>(w) * static_cast<size_t>(A.stride) + static_cast<size_t>(s) + skip;
        const float rms = burst_gate_rms(x, len, sq_all[wave], lane);
        if (A.rms && lane == 0) A.rms[slot + 1] = rms;
        if (rms < 0.04f) { stop = RIA_BURST_STOP_ENERGY; go = false; }
    }
    if (lane == 0) {
        rp->cfo_hz = cfo;
        rp->frames = static_cast<uint8_t>(frames);
        rp->frames_decoded = static_cast<uint8_t>(frames_decoded);
        rp->stop = static_cast<uint8_t>(stop);
        if (!group && f == 0) { rp->frame_start = frame_start; rp->delta = static_cast<int16_t>(delta); rp->candidates = static_cast<uint8_t>(candidates); }
        (group ? A.g_stage.state : A.c_stage.state)[i] = go ? 1 : complete ? 2 : 0;
        (group ? A.g_stage.window : A.c_stage.window)[i] = w;
        if (go) {
            (group ? A.g_stage.offset : A.c_stage.offset)[i] = static_cast<uint64_t>(w) * static_cast<uint64_t>(A.stride) + static_cast<uint64_t>(s);
            ria_frame_meta* mp = (group ? A.g_stage.meta : A.c_stage.meta) + i;
            mp->cfo_hz = cfo;
            mp->flags = 0u;
            mp->abs_position = A.params[w].abs_base + static_cast<uint64_t>(sync_start);   // never moved inside a burst
            if (A.cfo_used) A.cfo_used[slot + 1] = cfo;
        }
    }
}

// One block: the kept entries of the two stage lists, in list order, become the next round's lists; the groups that are
// complete are listed for the decode.
__global__ __launch_bounds__(kAcqScanThreads) void burst_list_kernel(BurstArgs A) {
    int run_g = 0, run_d = 0, run_c = 0;
    for (int base = 0; base < A.n_g; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        const int k = i < A.n_g ? A.g_stage.state[i] : 0;
        int tot_g, tot_d;
        const int pg = run_g + acq_block_scan(k == 1, &tot_g);
        const int pd = run_d + acq_block_scan(k == 2, &tot_d);
        if (k == 1) {
            const uint32_t w = A.g_stage.window[i];
            A.g_cur.offset[pg] = A.g_stage.offset[i]; A.g_cur.meta[pg] = A.g_stage.meta[i]; A.g_cur.window[pg] = w;
            A.gpos[static_cast<size_t>(w) * kBurstMaxGroup + A.round] = static_cast<uint32_t>(pg);
        }
        if (k == 2) A.done[pd] = A.g_stage.window[i];
        run_g += tot_g; run_d += tot_d;
    }
    for (int base = 0; base < A.n_c; base += kAcqScanThreads) {
        const int i = base + static_cast<int>(threadIdx.x);
        const int k = i < A.n_c ? A.c_stage.state[i] : 0;
        int tot_c;
        const int pc = run_c + acq_block_scan(k == 1, &tot_c);
        if (k == 1) { A.c_cur.offset[pc] = A.c_stage.offset[i]; A.c_cur.meta[pc] = A.c_stage.meta[i]; A.c_cur.window[pc] = A.c_stage.window[i]; }
        run_c += tot_c;
    }
    if (threadIdx.x == 0) {
        A.ctl->n_group = static_cast<unsigned>(run_g); A.ctl->n_cont = static_cast<unsigned>(run_c);
        if (run_d) A.ctl->n_done = static_cast<unsigned>(run_d);   // groups complete in one round only (round == group_size)
    }
}

// BurstInterleaver::deinterleave (burst_interleaver.cpp:8-78) of the complete groups, from the rounds' soft-bit rows straight
// into the decode batch: logical[f][b] = physical[(N*b+f)/324][(N*b+f)%324], eight soft bits per byte.
__global__ __launch_bounds__(256) void burst_gather_kernel(BurstArgs A) {
    const int N = A.group_size;
    const long long total = static_cast<long long>(A.n_done) * N * 324;
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < total; t += gridDim.x * 256ll) {
        const int b = static_cast<int>(t % 324), f = static_cast<int>((t / 324) % N), g = static_cast<int>(t / (324ll * N));
        const int flat = N * b + f, pf = flat / 324, pb = flat % 324;
        const uint32_t w = A.done[g];
        const size_t row = static_cast<size_t>(A.gpos[static_cast<size_t>(w) * kBurstMaxGroup + pf]) * N + pf;
        const float* src = A.gllr + row * A.llr_stride + pb * 8;
        float* dst = A.dec_in + (static_cast<size_t>(g) * N + f) * kBurstFrameBits + b * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = src[k];
    }
}

// One wavefront per decoded logical frame: its bytes and decode status go to (window, slot = logical index).
__global__ __launch_bounds__(256) void burst_scatter_kernel(BurstArgs A) {
    const int lane = threadIdx.x & 63, N = A.group_size;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < A.n_done * N; t += gridDim.x * 4) {
        const int g = t / N, f = t % N;
        const uint32_t w = A.done[g];
        const size_t slot = static_cast<size_t>(w) * kBurstSlots + f;
        const uint8_t* src = A.dec_info + static_cast<size_t>(t) * A.info_bytes;
        uint8_t* dst = A.info_out + slot * A.info_bytes;
        for (int q = lane; q < A.info_bytes; q += 64) dst[q] = src[q];
        if (lane == 0) {
            const ria_decode_status st = A.dec_dst[t];
            if (st.reserved[1] == kDecodeFaultMarker) atomicOr(&A.ctl->fault, 1u);
            A.dst_out[slot] = st;
            if (f == 0) A.res[w].frames_decoded = static_cast<uint8_t>(N);
        }
    }
}

}  // namespace ria
