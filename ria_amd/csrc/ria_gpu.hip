// ria_amd/csrc/ria_gpu.hip — C-ABI implementation of libria_gpu.so (include/ria_gpu.h).
// Host-side orchestration only: table upload, workspace, kernel launches.  No torch types, no CPU
// fallback: every entry point fails loudly if the HIP device or a launch is unavailable.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ria_gpu.h"
#include "host_tables.hpp"
#include "../host/link_adaptation.hpp"
#include "frame_recovery.hpp"
#include "ws_carve.hpp"
#include "host_stage.hpp"
#include "device_buffers.hpp"
#include "ldpc_kernels.hip.h"
#include "ldpc_fast.hip.h"
#ifdef RIA_WITH_DUAL_DECODER   // experiment record (two codewords per wave; measured slower): not in the default library
#include "ldpc_dual.hip.h"
#endif
#include "recovery_kernels.hip.h"
#include "demod_kernels.hip.h"
#include "tx_kernels.hip.h"
#include "sync_kernels.hip.h"
#include "mcdpsk_kernels.hip.h"
#include "cox_kernels.hip.h"
#include "cfo_kernels.hip.h"
#include "acquire_kernels.hip.h"
#include "mcdpsk_acquire_kernels.hip.h"
#include "burst_kernels.hip.h"
#include "decode_frame_kernels.hip.h"
#include "mcdpsk_harq_kernels.hip.h"
#include "var_frames.hpp"
#include "control_kernels.hip.h"
#include "window_kernels.hip.h"
#include "mcdpsk_window_kernels.hip.h"
#include "ring_kernels.hip.h"
#include "search_kernels.hip.h"
#include "stream_kernels.hip.h"
#include "mcdpsk_stream_kernels.hip.h"
#include "mcdpsk_ring_kernels.hip.h"

using namespace ria;

// A pool of chase caches (include/ria_gpu.h): metadata, sums and owner words, allocated once at create.  The handle owns it.
struct ria_chase_pool_s {
    ria_gpu* h = nullptr;
    ria_chase_config cfg{};
    DevBuf d_meta, d_sums, d_owner;   // ChaseCache [n_caches]; float [n_caches][max_entries][16][648]; int32 [n_caches]
};

constexpr int kMaxParts = 4;   // ria_gpu_rx_batch overlaps up to this many parts of a batch on internal streams
// Every device and pinned block of a handle is a DevBuf / PinBuf member: ria_gpu_destroy frees them by deleting the handle.
struct ria_gpu {
    ria_gpu_config cfg{};
    ria_gpu_geometry geo{};
    CarrierPlan plan{};
    LdpcCode code;
    std::string err;
    int device = 0;
    // device tables
    DevBuf d_gather, d_gather_nochan, d_crc_bit, d_crc_init, d_zc_ref;
    // dual-chirp acquisition: tables (built at first use) and the per-chunk workspace
    DevBuf d_ch_tw, d_ch_tmpl, d_ch_tmpl_fft; float ch_energy[2] = {0, 0};
    DevBuf d_ch_w1, d_ch_w2, d_ch_mag, d_ch_cum, d_ch_st;
    hipStream_t ch_side = nullptr; hipEvent_t ch_ev[2] = {nullptr, nullptr};   // the time-domain fallback runs beside the FFT path
    DevBuf d_txcfo_ws;    // transmitter-CFO impairment (cfo_kernels.hip.h): two complex arrays + the phase table, grown on demand
    DevBuf d_zc_ws;       // baseband workspace of the long-buffer ZC search
    DevBuf d_chan_nstd;   // per-frame noise sigma (float) of the reference-identical channel
    // MC-DPSK: modulator and mixer tables per carrier count, Hilbert taps, CFO workspace
    std::map<int, DevBuf> d_mc_carrier, d_mc_train, d_mc_mixer;
    DevBuf d_mc_hilbert, d_hilbert65, d_sync_host, d_mc_ws;
    DevBuf d_twiddle, d_nco;
    // Schmidl-Cox acquisition: LTS passband templates (built at first use) and the metric-table workspace
    DevBuf d_cox_tI, d_cox_tQ; float cox_energy_ref = 0.0f; DevBuf d_cox_ws;
    DevBuf d_demod_const;
    DevBuf d_demod_ws[kMaxParts];   // split demodulator: bins / CFO / phase markers of one chunk, per stream slot
    DevBuf d_tx_const;
    DevBuf d_llr_ws;                // float [max_batch * llrs_per_frame] (fused path)
    FastCode fast{};
    CoreTables ftab;
    DevBuf d_f[5];                  // row_addr, col_addr, check_at, col_at, col_pos of `fast`
    int wave_lds = 0;
    hipStream_t aux_stream[4] = {nullptr, nullptr, nullptr, nullptr};   // ria_gpu_rx_batch: the parts of a large batch overlap here
    hipEvent_t aux_event[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf d_ctl;                   // DecodeCtl [kMaxParts]: cascade work-list control block per stream slot
    DevBuf d_seed_ws;               // uint32_t [kMaxParts][cascade grid][kSeedWsWords]: per stream slot, per persistent workgroup
    DevBuf d_decode_ws;             // the per-frame arrays of the decode (decode_ws_carve), for ws_frames frames
    int ws_frames = 0;
    int split_parts = 0;                  // RIA_OPT_SPLIT_PARTS (0 = library default)
    int dual_decoder = 0;                 // RIA_OPT_DUAL_DECODER: 0 = default (environment RIA_DUAL, else off), 1 = on, -1 = off
    int fallback_queue_all = 0;           // RIA_OPT_FALLBACK_QUEUE_ALL: 1 = the recovery fill also runs the re-decodes no trial can read
    DevBuf d_state_ws;              // uint32_t [kMaxParts][state grid][kStateWsWords]: per stream slot, per persistent workgroup (rates with the repeated-state exit only)
    int state_exit = 1;                   // RIA_OPT_STATE_EXIT: 1 (default) = the retry kernels end a failing decode whose message state repeats
    // host-buffer entry points (the single-frame IWaveform adaptor path): one device + one pinned staging block and a
    // stream, kept for the life of the handle, grown on demand - no allocation and no device-wide sync per call
    DevBuf d_hstage; PinBuf p_hstage; hipStream_t hstream = nullptr;
    int zc_lds_opted = 0, mc_lds_opted = 0, lts_lds_opted = 0;   // dynamic-LDS opt-ins made on this handle's device
    // CRC recovery: the device lists (recovery_carve) for rec_frames frames; the host restatement's staging, device and
    // pinned mirror (recovery_stage_carve), for rec_host_frames frames
    DevBuf d_rec_ws, d_rec_stage; PinBuf p_rec_stage;
    int rec_frames = 0, rec_host_frames = 0;
    Crc16Tables crc;
    // ria_gpu_rx_acquire_batch: detector results, two work lists, the compact outputs of one round and the control block
    // (device + pinned mirror), one block (acq_carve) sized for acq_windows windows, grown on demand
    DevBuf d_acq_ws; int acq_windows = 0; PinBuf p_acq_ctl;
    // ria_gpu_mcdpsk_acquire_batch: detector results, two work lists, one round's soft bits, codeword rows, decoder outputs and
    // header state, and the control block (device + pinned mirror), grown on demand (macq_carve)
    DevBuf d_macq_ws; PinBuf p_macq_ctl;
    // ria_gpu_rx_burst_batch: frame-0 rows of the acquire rounds, the round lists, the groups' soft bits and decode batch,
    // and the control block (device + pinned mirror), grown on demand (burst_carve)
    DevBuf d_burst_ws; PinBuf p_burst_ctl;
    // ria_gpu_decode_frame_batch: the R1/4 code of a handle of another rate (built at first use), the per-codeword channel
    // de-interleave table and the identity, and the workspace (dframe_carve) with its control block (device + pinned mirror),
    // grown on demand
    FastCode fast14{}; DevBuf d_f14[5]; int wave_lds14 = 0; bool have14 = false;
    DevBuf d_cw_perm[2];
    DevBuf d_df_ws; PinBuf p_df_ctl;
    // HARQ: the chase pools created on this handle; the per-row arrays of the chase stages (harq_carve) and, for
    // ria_gpu_mcdpsk_decode_frame_batch, the round's arrays (macq_carve without soft bits) with their control block
    std::vector<std::unique_ptr<ria_chase_pool_s>> chase_pools;
    DevBuf d_harq_ws, d_mdf_ws; PinBuf p_mdf_ctl;
    // variable-length demodulation and the control hypothesis (control_carve): frame offsets, the spans' soft bits and
    // status, detector results, the work list and the control block (device + pinned mirror), for ctrl_rows rows
    DevBuf d_ctrl_ws; int ctrl_rows = 0; PinBuf p_ctrl_ctl;
    // ria_gpu_rx_window_batch (window_carve): per-window state, soft bits and status, the span lists, one pass's compact
    // demodulations, probe records, decodeFrame's outputs and the control hypothesis's, with the control block's pinned mirror
    DevBuf d_win_ws; PinBuf p_win_ctl;
    // ria_gpu_mcdpsk_window_batch (mwin_carve): per-window pass state, the peek's decoder tries and the control word with its
    // pinned mirror; the rounds use d_macq_ws, carved for the longest pass
    DevBuf d_mwin_ws; PinBuf p_mwin_ctl;
    // ria_gpu_search_batch (search_carve): the due list, one chunk's gathered spans, detector records and per-span parameters,
    // and the control word with its pinned mirror
    DevBuf d_search_ws; PinBuf p_search_ctl;
    DevBuf d_ring_rec;                    // ria_gpu_rx_ring_host: the recording on the device
    int search_chunk = 0;                 // RIA_OPT_SEARCH_CHUNK (0 = as many streams as 256 MiB of spans hold)
    // ria_gpu_rx_stream_batch (stream_carve): the control word with the found list behind it and their pinned mirror, the
    // open and group lists, the search's result records, and one chunk's windows, parameters and window-call outputs
    DevBuf d_stream_ws; PinBuf p_stream_ctl;
};

namespace {

int fail(ria_gpu_handle h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    // a failed HIP call leaves its code in the runtime's per-thread "last error"; the caller has been told through the
    // return value, so do not let it surface again in whoever calls hipGetLastError next (e.g. the host framework)
    if (code == RIA_ERR_HIP) (void)hipGetLastError();
    return code;
}

#define HIP_TRY(h, expr)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(h, RIA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

uint16_t crc16_host(const uint8_t* d, int n, uint16_t init) {  // frame_v2.cpp:115-128
    uint16_t crc = init;
    for (int i = 0; i < n; ++i) {
        crc ^= static_cast<uint16_t>(d[i]) << 8;
        for (int j = 0; j < 8; ++j) crc = (crc & 0x8000) ? static_cast<uint16_t>((crc << 1) ^ 0x1021) : static_cast<uint16_t>(crc << 1);
    }
    return crc;
}

}  // namespace

// ---- rate -> compiled code shape ------------------------------------------------------------------
template <class F>
static void dispatch_shape(int rate, F&& f) {
    switch (rate) {
        case RIA_RATE_1_4: f(ShapeR14{}); break;
        case RIA_RATE_2_3: f(ShapeR23{}); break;
        case RIA_RATE_3_4: f(ShapeR34{}); break;
        case RIA_RATE_5_6: f(ShapeR56{}); break;
        case RIA_RATE_1_3: f(ShapeR13{}); break;
        default: f(ShapeR12{}); break;
    }
}
// the compiled round structure must be the one host_tables.hpp derives from the generated H
static bool shape_fits(int rate, const CoreTables& t, int* wave_lds) {
    bool ok = false;
    dispatch_shape(rate, [&](auto s) {
        using S = decltype(s);
        using I = ShapeInfo<S>;
        ok = static_cast<int>(t.ne.size()) == S::NR && static_cast<int>(t.dv.size()) == S::NC;
        for (int r = 0; ok && r < S::NR; ++r) ok = t.ne[r] == S::ne(r) && t.nm[r] == S::nm(r);
        for (int r = 0; ok && r < S::NC; ++r) ok = t.dv[r] == S::dv(r);
        ok = ok && t.ts == I::TS && t.td == I::TD && t.tot_word == I::tot_word && t.zero_word == I::zero_word && t.dump_word == I::dump_word && t.big_word == I::big_word && t.n_mixed == I::TM && 4 * I::words <= 65536;
        *wave_lds = I::lds_bytes;
    });
    return ok;
}
// workgroups of the persistent retry kernels (256 CUs x 12 waves); RIA_PERSIST_GRID overrides it for experiments
static int persist_grid_size(bool dual) {
    static const int grid_env = getenv("RIA_PERSIST_GRID") ? std::max(64, atoi(getenv("RIA_PERSIST_GRID"))) : 0;
    return grid_env ? grid_env : (dual ? 2048 : 3072);
}
// the per-frame arrays of the decode, 4 codewords per frame
struct DecodeWs {
    unsigned int *entries, *best, *list1;
    CwResult* res;
    uint8_t* res_bytes;           // [4 * n][kNumFactors][bytes_per_cw]
    CascadeWin* win;
    float* staged;                // [4 * n][kStageFloats]
    unsigned int *l1idx, *l1hash;
    unsigned int* late;           // [n]
};
static DecodeWs decode_ws_carve(Carver& c, size_t n_frames, size_t bytes_per_cw) {
    const size_t n4 = 4 * n_frames;
    DecodeWs w;
    w.entries = c.take<unsigned int>(n4);
    w.best = c.take<unsigned int>(n4);
    w.list1 = c.take<unsigned int>(n4);
    w.res = c.take<CwResult>(n4);
    w.res_bytes = c.take<uint8_t>(n4 * kNumFactors * bytes_per_cw);
    w.win = c.take<CascadeWin>(n4);
    w.staged = c.take<float>(n4 * kStageFloats);
    w.l1idx = c.take<unsigned int>(n4);
    w.l1hash = c.take<unsigned int>(n4);
    w.late = c.take<unsigned int>(n_frames);
    return w;
}
// workgroups that own an area of d_state_ws: the persistent grid of phase 0 and the cascade, or the fill's
constexpr int kFillGrid = 3072;
constexpr int kTwoPartFrames = 32768;   // ria_gpu_rx_batch: from this batch size on the default split is two parts, below it three
constexpr int kLateGrid = 256;   // workgroups of fast_late_kernel: a handful of frames per 100 000 reach it
static int state_grid_size() { return std::max(persist_grid_size(false), kFillGrid); }
static hipError_t ensure_decode_ws(ria_gpu_handle h, int n_frames) {
    bool state_exit_rate = false;
    dispatch_shape(h->cfg.code_rate, [&](auto sh) { state_exit_rate = decltype(sh)::kStateExit; });
    if (n_frames <= h->ws_frames && h->d_ctl && h->d_seed_ws && (h->d_state_ws || !state_exit_rate)) return hipSuccess;
    h->ws_frames = 0;   // nothing is valid until every allocation below has succeeded
    hipError_t e;
    if (!h->d_ctl) {   // one per stream slot; zeroed here because ria_gpu_debug_queue_fault reads the slots no call has used yet as well
        if ((e = h->d_ctl.reserve(kMaxParts * sizeof(DecodeCtl))) != hipSuccess) return e;
        if ((e = hipMemset(h->d_ctl.as<>(), 0, kMaxParts * sizeof(DecodeCtl))) != hipSuccess) { h->d_ctl.release(); return e; }
    }
    // the cascade's seeded RNG states: one area per workgroup of its grid and per stream slot (the parts of a batch run concurrently)
    if ((e = h->d_seed_ws.reserve(static_cast<size_t>(kMaxParts) * persist_grid_size(false) * kSeedWsWords * sizeof(uint32_t))) != hipSuccess) return e;
    // the state copies of the repeated-state exit, likewise (phase 0, the cascade and the fill of a slot follow each other on one stream)
    if (state_exit_rate &&
        (e = h->d_state_ws.reserve(static_cast<size_t>(kMaxParts) * state_grid_size() * kStateWsWords * sizeof(uint32_t))) != hipSuccess) return e;
    const size_t bpc = h->geo.bytes_per_codeword;
    if ((e = h->d_decode_ws.reserve(carved_size([&](Carver& c) { return decode_ws_carve(c, n_frames, bpc); }))) != hipSuccess) return e;
    h->ws_frames = n_frames;
    return hipSuccess;
}
static void set_fast_attributes(int rate, int wb) {
    dispatch_shape(rate, [&](auto s) {
        using S = decltype(s);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_primary_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, wb);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_phase0_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, wb);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_late_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, wb);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_cascade_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, wb);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_rows_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, wb);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fast_robust_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, wb);
#ifdef RIA_WITH_DUAL_DECODER
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(dual_phase0_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, DualInfo<S>::lds_bytes);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(dual_cascade_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, DualInfo<S>::lds_bytes);
#endif
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(recovery_fill_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, wb);
    });
}

// ---- CRC-guided false-positive recovery glue (host logic in frame_recovery.hpp) -----------------
template <class F>
static void parallel_for(int n, F&& f) {
    int nt = static_cast<int>(std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())));
    if (n < 64 || nt == 1) { for (int i = 0; i < n; ++i) f(i); return; }
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&]() { for (;;) { int i0 = next.fetch_add(32); if (i0 >= n) return; for (int i = i0; i < std::min(n, i0 + 32); ++i) f(i); } });
    for (auto& t : th) t.join();
}

struct RecoveryWs { unsigned int *rctl, *overflow, *flagged, *list2, *stage2; };
static RecoveryWs recovery_carve(Carver& c, size_t n) {
    RecoveryWs w;
    w.rctl = c.take<unsigned int>(8 * kMaxParts);   // one 32-byte counter block per stream slot
    w.overflow = c.take<unsigned int>(n);
    w.flagged = c.take<unsigned int>(n);
    w.list2 = c.take<unsigned int>(n * 16);
    w.stage2 = c.take<unsigned int>(n);
    return w;
}
// staging of the host restatement: the flagged frames' compact rows, on the device and in pinned memory
struct RecoveryStage {
    unsigned int *rctl, *flagged;   // pinned block only: the device's are in RecoveryWs
    uint8_t* info_c; float* rows_c; uint8_t* redec_ok; uint8_t* redec_bytes; ria_decode_status* st_c;
};
static RecoveryStage recovery_stage_carve(Carver& c, size_t n, size_t info_bytes, size_t bytes_per_cw, bool pinned) {
    RecoveryStage w{};
    if (pinned) { w.rctl = c.take<unsigned int>(4); w.flagged = c.take<unsigned int>(n); }
    w.info_c = c.take<uint8_t>(n * info_bytes);
    w.rows_c = c.take<float>(n * 4 * 648);
    w.redec_ok = c.take<uint8_t>(n * 16);
    w.redec_bytes = c.take<uint8_t>(n * 16 * bytes_per_cw);
    w.st_c = c.take<ria_decode_status>(n);
    return w;
}
static RecoveryWs recovery_ws(ria_gpu_handle h) {
    return carve_at(h->d_rec_ws.as<>(), [&](Carver& c) { return recovery_carve(c, h->rec_frames); });
}
static RecoveryStage recovery_stage(ria_gpu_handle h, bool pinned) {
    return carve_at(pinned ? h->p_rec_stage.as<>() : h->d_rec_stage.as<>(), [&](Carver& c) {
        return recovery_stage_carve(c, h->rec_host_frames, h->geo.info_bytes_per_frame, h->geo.bytes_per_codeword, pinned); });
}
static hipError_t ensure_recovery_ws(ria_gpu_handle h, int n_frames, bool host_staging) {
    const size_t n = static_cast<size_t>(n_frames), ib = h->geo.info_bytes_per_frame, bpc = h->geo.bytes_per_codeword;
    hipError_t e;
    if (n_frames > h->rec_frames) {
        h->rec_frames = 0;   // nothing is valid until the allocation has succeeded
        if ((e = h->d_rec_ws.reserve(carved_size([&](Carver& c) { return recovery_carve(c, n); }))) != hipSuccess) return e;
        // the counter blocks of every stream slot: ria_gpu_debug_recovery_counts reads the slots no call has used yet as well
        if ((e = hipMemset(h->d_rec_ws.as<>(), 0, 8 * kMaxParts * sizeof(unsigned int))) != hipSuccess) { h->d_rec_ws.release(); return e; }
        h->rec_frames = n_frames;
    }
    if (host_staging && n_frames > h->rec_host_frames) {
        h->rec_host_frames = 0;
        if ((e = h->d_rec_stage.reserve(carved_size([&](Carver& c) { return recovery_stage_carve(c, n, ib, bpc, false); }))) != hipSuccess) return e;
        if ((e = h->p_rec_stage.reserve(carved_size([&](Carver& c) { return recovery_stage_carve(c, n, ib, bpc, true); }))) != hipSuccess) return e;
        h->rec_host_frames = n_frames;
    }
    return hipSuccess;
}
// Everything launch_decode grows for n_frames frames under `flags`.  A reserve step does all of its stage's growing and
// nothing else (no launch, no memset on the caller's stream): the stage's entry point calls it, and so does every composite
// call that runs the stage later, up front, before anything is in flight - a block that grows frees the old one.
static hipError_t decode_reserve(ria_gpu_handle h, int n_frames, uint32_t flags) {
    hipError_t e = ensure_decode_ws(h, n_frames);
    if (e == hipSuccess && (flags & RIA_DECODE_CRC_RECOVER)) e = ensure_recovery_ws(h, std::max(n_frames, h->cfg.max_batch), false);
    return e;
}

__global__ void recovery_status_gather_kernel(const unsigned int* n_flagged, const unsigned int* flagged,
                                              const ria_decode_status* st, ria_decode_status* st_c) {
    unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < *n_flagged) st_c[q] = st[flagged[q]];
}
__global__ void recovery_scatter_kernel(int nf, const unsigned int* __restrict__ flagged, const uint8_t* __restrict__ info_c,
                                        const ria_decode_status* __restrict__ st_c, int info_bytes,
                                        uint8_t* __restrict__ info_out, ria_decode_status* __restrict__ st_out) {
    int f = blockIdx.x;
    if (f >= nf) return;
    unsigned dst = flagged[f];
    for (int i = threadIdx.x; i < info_bytes; i += blockDim.x)
        info_out[static_cast<size_t>(dst) * info_bytes + i] = info_c[static_cast<size_t>(f) * info_bytes + i];
    if (threadIdx.x == 0) st_out[dst] = st_c[f];
}

// Runs after the decode kernels when RIA_DECODE_CRC_RECOVER is set (frame_v2.cpp:1564-1880).
// The GPU lists the flagged frames and completes the min-sum-factor result table for them (the fallback
// stage re-decodes with 0.75/0.625/0.5/0.875: the same decodes phase 0 makes); then one wave per flagged
// frame runs the CRC-guided searches (recovery_kernels.hip.h).  Nothing leaves the device and nothing
// synchronises.  RIA_RECOVERY_HOST=1 selects the host restatement of the same searches
// (frame_recovery.hpp) instead, which the tests use to cross-check the two implementations.
static int run_crc_recovery_host(ria_gpu_handle h, const FastDecodeArgs& D, hipStream_t s);
static int run_crc_recovery(ria_gpu_handle h, const FastDecodeArgs& D, hipStream_t s, int slot = 0, int ws_off = 0) {
    const char* env = getenv("RIA_RECOVERY_HOST");   // read per call: tests flip it
    const bool on_host = env != nullptr && env[0] == '1';
    if (on_host) return run_crc_recovery_host(h, D, s);
    const int n_frames = D.n_frames;   // launch_decode's decode_reserve has grown the lists for ws_off + n_frames frames
    RecoveryArgs R{};
    R.d = D;
    const RecoveryWs W = recovery_ws(h);
    unsigned int* rctl = W.rctl + 8 * slot;
    R.n_flagged = rctl; R.n_list2 = rctl + 1; R.n_stage2 = rctl + 2; R.next_fill = rctl + 3; R.n_overflow = rctl + 4;
    R.n_queued = rctl + 5; R.queue_all = h->fallback_queue_all;
    R.flagged = W.flagged + ws_off; R.list2 = W.list2 + static_cast<size_t>(ws_off) * 16; R.stage2 = W.stage2 + ws_off;
    R.overflow = W.overflow + ws_off;
#ifdef RIA_DEBUG_STAMPS   // diagnostic builds only (tools/build_variant.sh ... -DRIA_DEBUG_STAMPS): a raw device pointer from the environment
    if (const char* e = getenv("RIA_DEBUG_REC_STAMPS")) R.dbg = reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0));
#endif
    R.list_units_now = 0;
    if (hipMemsetAsync(rctl, 0, 32, s) != hipSuccess) return fail(h, RIA_ERR_HIP, "hipMemsetAsync failed");
    const int rl = recovery_lds_bytes(h->geo.bytes_per_codeword);
    hipLaunchKernelGGL(recovery_list_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, s, R);
    hipLaunchKernelGGL(recovery_stage1_kernel, dim3(n_frames), dim3(64), rl, s, R);
    dispatch_shape(h->cfg.code_rate, [&](auto sh) {
        using S = decltype(sh);
        hipLaunchKernelGGL(recovery_fill_kernel<S>, dim3(std::min(n_frames * 16, kFillGrid)), dim3(64), h->wave_lds, s, R);
    });
    hipLaunchKernelGGL(recovery_stage2_kernel, dim3(n_frames), dim3(64), rl, s, R);
    // a work-queue fault recorded anywhere in this call (cascade, phase 0, recovery fill) turns every frame into a failure
    hipLaunchKernelGGL(decode_fault_kernel, dim3((n_frames + 3) / 4), dim3(256), 0, s, static_cast<const DecodeCtl*>(D.ctl), D.status, D.info_out,
                       h->geo.bytes_per_codeword, n_frames);
    if (hipGetLastError() != hipSuccess) return fail(h, RIA_ERR_HIP, "recovery kernel launch failed");
    return RIA_OK;
}

static int run_crc_recovery_host(ria_gpu_handle h, const FastDecodeArgs& D, hipStream_t s) {
    static const bool tdbg = getenv("RIA_DEBUG_RECOVERY") != nullptr;
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const int n_frames = D.n_frames;
    double tA = now();
    hipError_t e0 = ensure_recovery_ws(h, std::max(n_frames, h->cfg.max_batch), true);
    if (e0 != hipSuccess) return fail(h, RIA_ERR_HIP, "recovery workspace: %s", hipGetErrorString(e0));
    const int bpc = h->geo.bytes_per_codeword, ib = h->geo.info_bytes_per_frame;
    RecoveryArgs R{};
    R.d = D;
    const RecoveryWs W = recovery_ws(h);
    const RecoveryStage Dv = recovery_stage(h, false), P = recovery_stage(h, true);
    R.n_flagged = W.rctl; R.n_list2 = W.rctl + 1; R.next_fill = W.rctl + 3;
    R.flagged = W.flagged; R.list2 = W.list2; R.list_units_now = 1;
    R.info_c = Dv.info_c; R.rows_c = Dv.rows_c; R.redec_ok = Dv.redec_ok; R.redec_bytes = Dv.redec_bytes;
#define R_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(h, RIA_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
    R_TRY(hipMemsetAsync(W.rctl, 0, 16, s));
    hipLaunchKernelGGL(recovery_list_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, s, R);
    const int wb = h->wave_lds;
    dispatch_shape(h->cfg.code_rate, [&](auto sh) {
        using S = decltype(sh);
        hipLaunchKernelGGL(recovery_fill_kernel<S>, dim3(std::min(n_frames * 16, kFillGrid)), dim3(64), wb, s, R);
    });
    hipLaunchKernelGGL(recovery_gather_kernel, dim3(n_frames), dim3(256), 0, s, R);
    hipLaunchKernelGGL(recovery_status_gather_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, s, W.rctl, W.flagged,
                       D.status, Dv.st_c);
    R_TRY(hipGetLastError());
    R_TRY(hipMemcpyAsync(P.rctl, W.rctl, 16, hipMemcpyDeviceToHost, s));
    R_TRY(hipStreamSynchronize(s));
    double tB = now();
    const int nf = static_cast<int>(P.rctl[0]);
    if (nf == 0) return RIA_OK;
    R_TRY(hipMemcpyAsync(P.flagged, W.flagged, static_cast<size_t>(nf) * 4, hipMemcpyDeviceToHost, s));
    R_TRY(hipMemcpyAsync(P.info_c, Dv.info_c, static_cast<size_t>(nf) * ib, hipMemcpyDeviceToHost, s));
    R_TRY(hipMemcpyAsync(P.rows_c, Dv.rows_c, static_cast<size_t>(nf) * 4 * 648 * 4, hipMemcpyDeviceToHost, s));
    R_TRY(hipMemcpyAsync(P.redec_ok, Dv.redec_ok, static_cast<size_t>(nf) * 16, hipMemcpyDeviceToHost, s));
    R_TRY(hipMemcpyAsync(P.redec_bytes, Dv.redec_bytes, static_cast<size_t>(nf) * 16 * bpc, hipMemcpyDeviceToHost, s));
    R_TRY(hipMemcpyAsync(P.st_c, Dv.st_c, static_cast<size_t>(nf) * sizeof(ria_decode_status), hipMemcpyDeviceToHost, s));
    R_TRY(hipStreamSynchronize(s));
    double tC = now();
    FrameRecovery rec(h->crc, bpc);
    std::atomic<int> n_stage2{0};
    parallel_for(nf, [&](int i) {
        uint8_t cw[4][68];
        std::memset(cw, 0, sizeof(cw));
        uint8_t* inf = P.info_c + static_cast<size_t>(i) * ib;
        for (int c = 0; c < 4; ++c) std::memcpy(cw[c], inf + c * bpc, bpc);
        bool good = rec.recover_search(cw, P.rows_c + static_cast<size_t>(i) * 4 * 648);
        if (!good) {
            n_stage2++;
            uint8_t rd[4][4][68], rok[4][4];
            for (int at = 0; at < 4; ++at)
                for (int c = 0; c < 4; ++c) {
                    rok[at][c] = P.redec_ok[static_cast<size_t>(i) * 16 + at * 4 + c];
                    std::memcpy(rd[at][c], P.redec_bytes + (static_cast<size_t>(i) * 16 + at * 4 + c) * bpc, bpc);
                }
            good = rec.recover_fallback(cw, rok, rd);
        }
        ria_decode_status& sn = P.st_c[i];
        sn.needs_recovery = 0;
        sn.frame_valid = good ? 1 : 0;
        for (int c = 0; c < 4; ++c) {
            sn.cw_ok[c] = good ? 1 : 0;
            if (good) std::memcpy(inf + c * bpc, cw[c], bpc); else std::memset(inf + c * bpc, 0, bpc);
        }
    });
    double tD = now();
    R_TRY(hipMemcpyAsync(Dv.info_c, P.info_c, static_cast<size_t>(nf) * ib, hipMemcpyHostToDevice, s));
    R_TRY(hipMemcpyAsync(Dv.st_c, P.st_c, static_cast<size_t>(nf) * sizeof(ria_decode_status), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(recovery_scatter_kernel, dim3(nf), dim3(64), 0, s, nf, W.flagged, Dv.info_c, Dv.st_c, ib, D.info_out,
                       D.status);
    R_TRY(hipGetLastError());
    R_TRY(hipStreamSynchronize(s));
#undef R_TRY
    if (tdbg) fprintf(stderr, "[ria_gpu] recovery: frames %d flagged %d stage2 %d | gpu(decode+prep) %.2f ms, D2H %.2f ms, host search %.2f ms, H2D+scatter %.2f ms\n",
                      n_frames, nf, n_stage2.load(), tB - tA, tC - tB, tD - tC, now() - tD);
    return RIA_OK;
}

// control block -> its pinned mirror (allocated by the caller), one stream sync; a set fault flag fails the call with fault_fmt,
// which may print `arg`
static unsigned int ctl_fault(const MacqCtl&) { return 0; }   // the robust decoder has no work queue
static unsigned int ctl_fault(const MacqCiCtl&) { return 0; }
static unsigned int ctl_fault(const MwinCtl&) { return 0; }   // a flag of its own, read by the caller
static unsigned int ctl_fault(const SearchCtl&) { return 0; } // a flag of its own, read by the caller
static unsigned int ctl_fault(const WinCtl&) { return 0; }    // list lengths only: the stages behind them report their own faults
template <class Ctl>
static unsigned int ctl_fault(const Ctl& c) { return c.fault; }
template <class Ctl>
static int read_ctl(ria_gpu_handle h, PinBuf& mirror, const Ctl* ctl_dev, hipStream_t s, const char* fault_fmt = "", int arg = 0) {
    HIP_TRY(h, hipMemcpyAsync(mirror.as<Ctl>(), ctl_dev, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (ctl_fault(*mirror.as<Ctl>())) return fail(h, RIA_ERR_HIP, fault_fmt, arg);
    return RIA_OK;
}

// the decoder core's five tables on the device, and the pointers of the FastCode that reads them
static hipError_t upload_core_tables(const CoreTables& t, DevBuf (&d)[5], FastCode& f) {
    const std::vector<uint16_t>* src[5] = {&t.row_addr, &t.col_addr, &t.check_at, &t.col_at, &t.col_pos};
    for (int i = 0; i < 5; ++i)
        if (hipError_t e = upload(d[i], *src[i])) return e;
    f.row_addr = d[0].as<const uint16_t>(); f.col_addr = d[1].as<const uint16_t>(); f.check_at = d[2].as<const uint16_t>();
    f.col_at = d[3].as<const uint16_t>(); f.col_pos = d[4].as<const uint16_t>();
    return hipSuccess;
}

// the lane/slot assignment against LDS bank conflicts (host_tables.hpp): the layout annealed offline and shipped with the
// library (validated against this build's H), or - RIA_BANKOPT_MOVES set, or no valid shipped layout - annealed here, once
// per rate and process
static CoreTables core_tables_for(int rate, const LdpcCode& code) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, CoreTables> cache;
    const char* mv = getenv("RIA_BANKOPT_MOVES");
    const int moves = mv ? atoi(mv) : -1;              // -1: shipped layout, annealing (1 M moves) as the fallback
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_pair(rate, moves);
    auto it = cache.find(key);
    if (it == cache.end()) {
        CoreTables t;
        if (moves >= 0 || !load_saved_core_tables(code, t)) t = build_core_tables(code, moves >= 0 ? moves : 1000000);
        it = cache.emplace(key, std::move(t)).first;
    }
    return it->second;
}

extern "C" {

int ria_gpu_abi_version(void) { return RIA_GPU_ABI_VERSION; }
static bool demod_fused_selected() {   // read once per process
    static const bool fused = getenv("RIA_DEMOD_FUSED") && getenv("RIA_DEMOD_FUSED")[0] == '1';
    return fused;
}
int ria_gpu_demod_variant(void) { return demod_fused_selected() ? 1 : 0; }

void ria_gpu_default_config(ria_gpu_config* cfg) {
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->abi_version = RIA_GPU_ABI_VERSION;
    cfg->device = 0;
    cfg->modulation = RIA_MOD_QAM16;
    cfg->code_rate = RIA_RATE_1_2;
    cfg->fft_size = 1024;
    cfg->num_carriers = 59;
    cfg->cyclic_prefix = 128;
    cfg->sample_rate = 48000;
    cfg->center_freq = 1500;
    cfg->max_batch = 4096;
}

const char* ria_gpu_last_error(ria_gpu_handle h) { return h ? h->err.c_str() : "null handle"; }

void ria_gpu_destroy(ria_gpu_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (hipStream_t st_ : {h->aux_stream[0], h->aux_stream[1], h->aux_stream[2], h->aux_stream[3], h->hstream, h->ch_side}) if (st_) (void)hipStreamDestroy(st_);
    for (auto& ev_ : h->ch_ev) if (ev_) (void)hipEventDestroy(ev_);
    for (auto& ev_ : h->aux_event) if (ev_) (void)hipEventDestroy(ev_);
    delete h;   // its DevBuf / PinBuf members free the memory
}

int ria_gpu_create(const ria_gpu_config* cfg, ria_gpu_handle* out) {
    if (!cfg || !out) return RIA_ERR_INVALID;
    *out = nullptr;
    if (cfg->abi_version != RIA_GPU_ABI_VERSION) return RIA_ERR_INVALID;
    if (cfg->fft_size != 1024 || cfg->num_carriers != 59 || cfg->cyclic_prefix != 128 ||
        cfg->sample_rate != 48000 || cfg->center_freq != 1500)
        return RIA_ERR_UNSUPPORTED;  // the production OFDM-CHIRP shape (types.hpp:252-268)
    if (bits_per_carrier(cfg->modulation) == 0) return RIA_ERR_UNSUPPORTED;
    if (cfg->code_rate < RIA_RATE_1_4 || cfg->code_rate > RIA_RATE_5_6) return RIA_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device) return RIA_ERR_NO_DEVICE;
    ria_gpu_handle h = new ria_gpu();
    if (const char* se = getenv("RIA_STATE_EXIT")) h->state_exit = se[0] != '0';   // the default of RIA_OPT_STATE_EXIT, for A/B runs of programs that never set it
    h->cfg = *cfg;
    h->device = cfg->device;
    if (h->cfg.max_batch <= 0) h->cfg.max_batch = 4096;
    if (hipSetDevice(h->device) != hipSuccess) { delete h; return RIA_ERR_NO_DEVICE; }

    h->plan = build_carrier_plan(cfg->modulation, cfg->code_rate);
    h->code = build_ldpc(cfg->code_rate);
    ria_gpu_geometry& g = h->geo;
    g.pilot_spacing = h->plan.spacing;
    g.n_pilots = h->plan.n_pilot;
    g.n_data_carriers = h->plan.n_data;
    g.bits_per_carrier = bits_per_carrier(cfg->modulation);
    g.bits_per_symbol = g.n_data_carriers * g.bits_per_carrier;
    g.n_data_symbols = (kFrameBits + g.bits_per_symbol - 1) / g.bits_per_symbol;
    g.samples_per_symbol = kSym;
    g.frame_samples = (2 + g.n_data_symbols) * kSym;
    g.llrs_per_frame = g.n_data_symbols * g.bits_per_symbol;
    g.info_bits = info_bits_for(cfg->code_rate);
    g.bytes_per_codeword = g.info_bits / 8;
    g.info_bytes_per_frame = 4 * g.bytes_per_codeword;
    g.ldpc_max_iterations = recommended_iterations(cfg->code_rate);
    g.ldpc_edges = h->code.n_edges;
    g.ldpc_k = h->code.k;
    if (const char* why = tx_const_misfit(h->plan, h->code, g)) {   // before build_tx_const copies by these counts
        fprintf(stderr, "ria_gpu_create: the transmit constant block does not hold this configuration: %s\n", why);
        delete h;
        return RIA_ERR_UNSUPPORTED;
    }

#define CREATE_TRY(expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "ria_gpu_create: %s failed: %s\n", #expr, hipGetErrorString(e_));        \
            ria_gpu_destroy(h);                                                                       \
            return RIA_ERR_HIP;                                                                       \
        }                                                                                             \
    } while (0)

    CREATE_TRY(upload(h->d_gather, build_rx_gather(g.bits_per_symbol, true)));
    CREATE_TRY(upload(h->d_gather_nochan, build_rx_gather(g.bits_per_symbol, false)));
    {
        // CRC-16 linear decomposition: crc(M) = crc_init[L] ^ XOR_{set bits} crc_bit[distance from end]
        std::vector<uint16_t> bit(4 * 68 * 8 + 16), init(4 * 68 + 2);
        std::vector<uint8_t> z(4 * 68 + 2, 0);
        for (size_t q = 0; q < bit.size(); ++q) {
            std::vector<uint8_t> msg(q / 8 + 1, 0);
            msg[0] = static_cast<uint8_t>(1u << (q % 8));
            bit[q] = crc16_host(msg.data(), static_cast<int>(msg.size()), 0);
        }
        for (size_t L = 0; L < init.size(); ++L) init[L] = crc16_host(z.data(), static_cast<int>(L), 0xFFFF);
        CREATE_TRY(upload(h->d_crc_bit, bit));
        CREATE_TRY(upload(h->d_crc_init, init));
    }
    h->crc.build(4 * 68);
    {
        std::vector<float> zc(static_cast<size_t>(4) * kZcRepSamples * 2), re, im;
        for (int r = 0; r < 4; ++r) {
            build_zc_reference(2 * r + 1, re, im);
            for (int i = 0; i < kZcRepSamples; ++i) { zc[(static_cast<size_t>(r) * kZcRepSamples + i) * 2] = re[i]; zc[(static_cast<size_t>(r) * kZcRepSamples + i) * 2 + 1] = im[i]; }
        }
        CREATE_TRY(upload(h->d_zc_ref, zc));
    }
    CREATE_TRY(upload(h->d_twiddle, build_twiddles()));
    CREATE_TRY(upload(h->d_nco, build_nco_table(g.frame_samples)));
    {
        DemodConst dc = build_demod_const(h->plan, cfg->modulation, g);
        std::vector<DemodConst> v(1, dc);
        CREATE_TRY(upload(h->d_demod_const, v));
        TxConst tc = build_tx_const(h->plan, h->code, cfg->modulation, g);
        std::vector<TxConst> tv(1, tc);
        CREATE_TRY(upload(h->d_tx_const, tv));
    }
    CREATE_TRY(h->d_llr_ws.reserve(static_cast<size_t>(h->cfg.max_batch) * g.llrs_per_frame * sizeof(float)));

    h->ftab = core_tables_for(cfg->code_rate, h->code);
    CREATE_TRY(upload_core_tables(h->ftab, h->d_f, h->fast));
    h->fast.k = h->code.k; h->fast.m = h->code.m; h->fast.max_iter = g.ldpc_max_iterations; h->fast.bytes_per_cw = g.bytes_per_codeword;
    if (!shape_fits(cfg->code_rate, h->ftab, &h->wave_lds)) { ria_gpu_destroy(h); return RIA_ERR_UNSUPPORTED; }
    set_fast_attributes(cfg->code_rate, h->wave_lds);
    CREATE_TRY(ensure_decode_ws(h, h->cfg.max_batch));
    CREATE_TRY(demod_set_attributes());
#undef CREATE_TRY
    *out = h;
    return RIA_OK;
}

int ria_gpu_get_geometry(ria_gpu_handle h, ria_gpu_geometry* out) {
    if (!h || !out) return RIA_ERR_INVALID;
    *out = h->geo;
    return RIA_OK;
}

int ria_gpu_set_option(ria_gpu_handle h, int option, int value) {
    if (!h) return RIA_ERR_INVALID;
    if (option == RIA_OPT_SPLIT_PARTS && value >= 0 && value <= kMaxParts) { h->split_parts = value; return RIA_OK; }
    if (option == RIA_OPT_DUAL_DECODER && value >= -1 && value <= 1) {
#ifndef RIA_WITH_DUAL_DECODER
        if (value > 0) return fail(h, RIA_ERR_UNSUPPORTED, "ria_gpu_set_option: this build does not contain the two-codewords-per-wave kernels (-DRIA_WITH_DUAL_DECODER)");
#endif
        h->dual_decoder = value; return RIA_OK;
    }
    if (option == RIA_OPT_FALLBACK_QUEUE_ALL && value >= 0 && value <= 1) { h->fallback_queue_all = value; return RIA_OK; }
    if (option == RIA_OPT_STATE_EXIT && value >= 0 && value <= 1) { h->state_exit = value; return RIA_OK; }
    if (option == RIA_OPT_SEARCH_CHUNK && value >= 0 && value <= 65535) { h->search_chunk = value; return RIA_OK; }
    return fail(h, RIA_ERR_INVALID, "ria_gpu_set_option: unknown option %d or value %d out of range", option, value);
}

// ------------------------------------------------------------------------------------------------ decode
int ria_gpu_ldpc_decode_batch(ria_gpu_handle h, const float* llr_dev, int n_cw, int max_iterations,
                              float min_sum_factor, uint8_t* out_dev, uint8_t* ok_dev, uint16_t* iters_dev,
                              void* stream) {
    if (!h || !llr_dev || !out_dev || !ok_dev || !iters_dev || n_cw < 0 || max_iterations < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_ldpc_decode_batch: bad argument");
    if (n_cw == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    dispatch_shape(h->cfg.code_rate, [&](auto sh) {
        using S = decltype(sh);
        hipLaunchKernelGGL(fast_rows_kernel<S>, dim3(std::min(n_cw, 16384)), dim3(64), h->wave_lds,
                           static_cast<hipStream_t>(stream), h->fast, llr_dev, n_cw, max_iterations, min_sum_factor,
                           out_dev, ok_dev, iters_dev);
    });
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_ldpc_decode_robust_batch(ria_gpu_handle h, const float* llr_dev, int n_cw, uint8_t* out_dev, uint8_t* ok_dev,
                                     uint16_t* iters_dev, uint8_t* tries_dev, void* stream) {
    if (!h || !llr_dev || !out_dev || !ok_dev || !iters_dev || n_cw < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_ldpc_decode_robust_batch: bad argument");
    if (n_cw == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    dispatch_shape(h->cfg.code_rate, [&](auto sh) {
        using S = decltype(sh);
        hipLaunchKernelGGL(fast_robust_kernel<S>, dim3(std::min(n_cw, 16384)), dim3(64), h->wave_lds,
                           static_cast<hipStream_t>(stream), h->fast, llr_dev, n_cw, out_dev, ok_dev, iters_dev, tries_dev);
    });
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// slot / ws_off: which control block and which frame range of the per-handle workspace this launch owns
// (ria_gpu_rx_batch runs the two halves of a large batch on two streams: slot 0 at offset 0, slot 1 behind it)
static int launch_decode(ria_gpu_handle h, const float* llr_dev, int llr_stride, int n_frames, uint32_t flags,
                         uint8_t* info_out_dev, ria_decode_status* status_dev, hipStream_t s, int slot = 0, int ws_off = 0) {
    hipError_t e = decode_reserve(h, ws_off + n_frames, flags);   // a no-op behind a caller that reserved for the whole call
    if (e != hipSuccess) return fail(h, RIA_ERR_HIP, "decode workspace: %s", hipGetErrorString(e));
    FastDecodeArgs A;
    const size_t o4 = static_cast<size_t>(ws_off) * 4, bpc = h->geo.bytes_per_codeword;
    const DecodeWs W = carve_at(h->d_decode_ws.as<>(), [&](Carver& c) { return decode_ws_carve(c, h->ws_frames, bpc); });
    if ((e = hipMemsetAsync(W.res + o4, 0, static_cast<size_t>(n_frames) * 4 * sizeof(CwResult), s)) != hipSuccess)
        return fail(h, RIA_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    A.c = h->fast;
    A.gather = ((flags & RIA_DECODE_NO_CHANNEL_DEINTERLEAVE) ? h->d_gather_nochan : h->d_gather).as<const uint16_t>();
    A.llr = llr_dev;
    A.llr_stride = llr_stride;
    A.n_frames = n_frames;
    A.flags = flags;
    A.info_out = info_out_dev;
    A.status = status_dev;
    A.crc_bit = h->d_crc_bit.as<const uint16_t>();
    A.crc_init = h->d_crc_init.as<const uint16_t>();
    A.ctl = h->d_ctl.as<DecodeCtl>() + slot;
    A.entries = W.entries + o4;
    A.best = W.best + o4;
    A.list1 = W.list1 + o4;
    A.res = W.res + o4;
    A.res_bytes = W.res_bytes + o4 * kNumFactors * bpc;
    A.win = W.win + o4;
    A.staged = W.staged + o4 * kStageFloats;
    A.l1idx = W.l1idx + o4;
    A.l1hash = W.l1hash + o4;
    A.late = W.late + ws_off;
    A.seed_ws = h->d_seed_ws.as<uint32_t>() + static_cast<size_t>(slot) * persist_grid_size(false) * kSeedWsWords;
    dispatch_shape(h->cfg.code_rate, [&](auto sh) { A.state_exit = decltype(sh)::kStateExit ? h->state_exit : 0; });
    A.state_ws = h->d_state_ws ? h->d_state_ws.as<uint32_t>() + static_cast<size_t>(slot) * state_grid_size() * kStateWsWords : nullptr;
    if ((e = hipMemsetAsync(A.ctl, 0, sizeof(DecodeCtl), s)) != hipSuccess)
        return fail(h, RIA_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    const int wb = h->wave_lds;
    // RIA_OPT_DUAL_DECODER / RIA_DUAL=1: the retry kernels decode two codewords per wave (ldpc_dual.hip.h) on 2 waves per
    // SIMD instead of one codeword per wave on 3.  Same results (tested); measured slower on the bench workload
    // (DESIGN.md section 4), so it is not the default.
#ifdef RIA_WITH_DUAL_DECODER
    static const bool dual_env = getenv("RIA_DUAL") && getenv("RIA_DUAL")[0] == '1';
    const bool dual = h->dual_decoder > 0 || (h->dual_decoder == 0 && dual_env);
#else
    const bool dual = false;
#endif
    const int persist_grid = persist_grid_size(dual);
    static const bool dbg = getenv("RIA_DEBUG_SYNC") != nullptr;   // stage-by-stage sync + trace on stderr
    auto stage = [&](const char* name) {
        if (!dbg) return;
        hipError_t e2 = hipStreamSynchronize(s);
        fprintf(stderr, "[ria_gpu] %s: %s\n", name, hipGetErrorString(e2));
        fflush(stderr);
    };
    dispatch_shape(h->cfg.code_rate, [&](auto sh) {
        using S = decltype(sh);
        hipLaunchKernelGGL(fast_primary_kernel<S>, dim3(n_frames), dim3(64), wb, s, A);
        stage("primary");
        if (flags & (RIA_DECODE_PHASE0 | RIA_DECODE_PERTURB)) {
#ifdef RIA_WITH_DUAL_DECODER
            if (dual) hipLaunchKernelGGL(dual_phase0_kernel<S>, dim3(std::min(n_frames * 8, persist_grid)), dim3(64), DualInfo<S>::lds_bytes, s, A);
            else
#endif
            hipLaunchKernelGGL(fast_phase0_kernel<S>, dim3(std::min(n_frames * 16, persist_grid)), dim3(64), wb, s, A);
        }
        stage("phase0");
        hipLaunchKernelGGL(fast_chain_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, s, A);
        stage("chain");
        // a first decode is skipped under RIA_DECODE_PERTURB only, and the chain reads a skipped one behind a phase-0 rescue only
        if ((flags & RIA_DECODE_PERTURB) && (flags & RIA_DECODE_PHASE0)) {
            hipLaunchKernelGGL(fast_late_kernel<S>, dim3(std::min(n_frames, kLateGrid)), dim3(64), wb, s, A);
            stage("late");
        }
        if (flags & RIA_DECODE_PERTURB) {
            // persistent waves over the device-side work list; sized to fill the chip (256 CUs x 12)
#ifdef RIA_WITH_DUAL_DECODER
            if (dual) hipLaunchKernelGGL(dual_cascade_kernel<S>, dim3(persist_grid), dim3(64), DualInfo<S>::lds_bytes, s, A);
            else
#endif
            hipLaunchKernelGGL(fast_cascade_kernel<S>, dim3(persist_grid), dim3(64), wb, s, A);
            stage("cascade");
            hipLaunchKernelGGL(fast_finalize_kernel, dim3(std::min((4 * n_frames + 255) / 256, 1024)), dim3(256), 0, s, A);
            stage("finalize");
        }
    });
    hipLaunchKernelGGL(frame_validate_kernel, dim3((n_frames + 3) / 4), dim3(256), 0, s, info_out_dev,
                       h->geo.bytes_per_codeword, n_frames, A.crc_bit, A.crc_init, status_dev, static_cast<const DecodeCtl*>(A.ctl));
    stage("validate");
    if (hipGetLastError() != hipSuccess) return fail(h, RIA_ERR_HIP, "decode kernel launch failed");
    if (flags & RIA_DECODE_CRC_RECOVER) return run_crc_recovery(h, A, s, slot, ws_off);
    return RIA_OK;
}

int ria_gpu_decode_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, int n_frames, uint32_t flags,
                         uint8_t* info_out_dev, ria_decode_status* status_dev, void* stream) {
    if (h && n_frames == 0) return RIA_OK;
    if (!h || !llr_dev || !info_out_dev || !status_dev || n_frames < 0 || llr_stride < kFrameBits)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_decode_batch: bad argument (llr_stride must be >= 2592)");
    HIP_TRY(h, hipSetDevice(h->device));
    return launch_decode(h, llr_dev, llr_stride, n_frames, flags, info_out_dev, status_dev, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ demod
// the demodulator's arguments: the handle's tables and one call's arrays (shared with the span form, demod_var_launch)
static DemodArgs demod_args(ria_gpu_handle h, const float* samples_dev, const uint64_t* offsets_dev, const ria_frame_meta* meta_dev, int n_frames,
                            float* llr_out_dev, int llr_stride, ria_frame_status* status_dev) {
    DemodArgs A{};
    A.k = h->d_demod_const.as<const DemodConst>();
    A.twiddle = h->d_twiddle.as<const float2>();
    A.nco = h->d_nco.as<const float2>();
    A.samples = samples_dev; A.offsets = offsets_dev; A.meta = meta_dev; A.n_frames = n_frames;
    A.llr_out = llr_out_dev; A.llr_stride = llr_stride; A.status = status_dev; A.dbg = nullptr;
    return A;
}
static int demod_batch_slot(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev, const ria_frame_meta* meta_dev,
                            int n_frames, float* llr_out_dev, ria_frame_status* status_dev, hipStream_t stream, int slot,
                            int llr_stride = 0 /* floats between the soft-bit rows of two frames; 0 = llrs_per_frame */) {
    DemodArgs A = demod_args(h, samples_dev, frame_offsets_dev, meta_dev, n_frames, llr_out_dev, llr_stride ? llr_stride : h->geo.llrs_per_frame, status_dev);
#ifdef RIA_DEBUG_STAMPS
    if (const char* e = getenv("RIA_DEBUG_DEMOD_STAMPS")) A.dbg = reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0));
#endif
    if (demod_fused_selected()) launch_demod_fused(A, stream);
    else {
        HIP_TRY(h, h->d_demod_ws[slot].reserve(demod_ws_bytes(2 + h->geo.n_data_symbols)));   // at the slot's first use
        launch_demod(A, h->geo, h->cfg.modulation, h->d_demod_ws[slot].as<>(), stream);
    }
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_demod_batch(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                        const ria_frame_meta* meta_dev, int n_frames, float* llr_out_dev,
                        ria_frame_status* status_dev, void* stream) {
    if (h && n_frames == 0) return RIA_OK;
    if (!h || !samples_dev || !llr_out_dev || n_frames < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_demod_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    return demod_batch_slot(h, samples_dev, frame_offsets_dev, meta_dev, n_frames, llr_out_dev, status_dev, static_cast<hipStream_t>(stream), 0);
}

int ria_gpu_rx_batch(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                     const ria_frame_meta* meta_dev, int n_frames, uint32_t flags, uint8_t* info_out_dev,
                     ria_decode_status* decode_status_dev, float* llr_out_dev, ria_frame_status* demod_status_dev,
                     void* stream) {
    if (h && n_frames == 0) return RIA_OK;
    if (!h || !samples_dev || !info_out_dev || !decode_status_dev || n_frames < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // Demodulate (LLRs stay in the HBM workspace / L2), then decode.  A large chunk is cut in parts (default 3, 2 from kTwoPartFrames frames on) that run
    // on internal streams: the low-occupancy phases of one part (first decodes, phase 0, finalise, CRC recovery)
    // overlap with the cascade of another.  Results do not depend on the split
    // (tests/test_gpu_modes.py::test_rx_batch_split_modes_are_bit_identical_and_match_the_reference).
    const char* rh = getenv("RIA_RECOVERY_HOST");
    const bool single_stream_only = (rh && rh[0] == '1') || getenv("RIA_DEBUG_SYNC") != nullptr;   // host recovery / stage tracing own slot 0
    // The default number of parts: a part's cascade is a persistent grid that holds the chip until it drains, so the parts'
    // cascades run one behind the other and the recovery of the part that ends last is the step's tail.  Since the first
    // decodes walk a frame (fast_primary_kernel) the first part reaches its cascade before the others have started their
    // phase 0; at the bench size two parts then measure 2.4 % under three.  Batches under
    // kTwoPartFrames were not measured again and keep three.
    int want_parts = h->split_parts;              // per handle (ria_gpu_set_option); 0: environment, else the default
    bool default_parts = false;
    if (want_parts == 0) {
        const char* sp = getenv("RIA_SPLIT_PARTS");
        default_parts = !getenv("RIA_NO_SPLIT") && !sp;
        want_parts = getenv("RIA_NO_SPLIT") ? 1 : sp ? std::max(1, std::min(kMaxParts, atoi(sp))) : 3;
    }
    if (single_stream_only) { want_parts = 1; default_parts = false; }
    for (int done = 0; done < n_frames;) {
        int nb = n_frames - done;
        if (!llr_out_dev && nb > h->cfg.max_batch) nb = h->cfg.max_batch;
        float* llr = llr_out_dev ? llr_out_dev + static_cast<size_t>(done) * h->geo.llrs_per_frame : h->d_llr_ws.as<float>();
        const int n_parts = (nb >= 4096) ? ((default_parts && nb >= kTwoPartFrames) ? 2 : want_parts) : 1;
        // grow the workspaces BEFORE anything is in flight: the parts share them
        if (hipError_t e = decode_reserve(h, nb, flags)) return fail(h, RIA_ERR_HIP, "rx workspace: %s", hipGetErrorString(e));
        if (n_parts > 1 && !h->aux_stream[0]) {
            for (auto& st_ : h->aux_stream) HIP_TRY(h, hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
            for (auto& ev_ : h->aux_event) HIP_TRY(h, hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
        }
        if (n_parts > 1) {
            HIP_TRY(h, hipEventRecord(h->aux_event[0], s));
            for (int part = 0; part < n_parts; ++part) HIP_TRY(h, hipStreamWaitEvent(h->aux_stream[part], h->aux_event[0], 0));
        }
        const int share = (n_parts > 1) ? (((nb + n_parts - 1) / n_parts + 7) & ~7) : nb;
        for (int part = 0; part < n_parts; ++part) {
            const int p0 = part * share, pn = std::min(share, nb - p0);
            if (pn <= 0) break;
            hipStream_t ps = (n_parts > 1) ? h->aux_stream[part] : s;
            const int g0 = done + p0;
            const uint64_t* offs = frame_offsets_dev ? frame_offsets_dev + g0 : nullptr;
            const float* smp = frame_offsets_dev ? samples_dev : samples_dev + static_cast<size_t>(g0) * h->geo.frame_samples;
            float* pl = llr + static_cast<size_t>(p0) * h->geo.llrs_per_frame;
            int rc = demod_batch_slot(h, smp, offs, meta_dev ? meta_dev + g0 : nullptr, pn, pl,
                                      demod_status_dev ? demod_status_dev + g0 : nullptr, ps, part);
            if (rc != RIA_OK) return rc;
            rc = launch_decode(h, pl, h->geo.llrs_per_frame, pn, flags, info_out_dev + static_cast<size_t>(g0) * h->geo.info_bytes_per_frame,
                               decode_status_dev + g0, ps, part, p0);
            if (rc != RIA_OK) return rc;
        }
        if (n_parts > 1) {
            for (int part = 0; part < n_parts; ++part) {
                HIP_TRY(h, hipEventRecord(h->aux_event[1 + part], h->aux_stream[part]));
                HIP_TRY(h, hipStreamWaitEvent(s, h->aux_event[1 + part], 0));
            }
        }
        done += nb;
    }
    return RIA_OK;
}

// staging block of the host-buffer entry points: `bytes` of device memory and as many of pinned host memory
static int ensure_host_stage(ria_gpu_handle h, size_t bytes) {
    if (!h->hstream) HIP_TRY(h, hipStreamCreateWithFlags(&h->hstream, hipStreamNonBlocking));
    bytes = (bytes + (size_t(1) << 20) - 1) & ~((size_t(1) << 20) - 1);
    if (bytes <= h->d_hstage.bytes() && bytes <= h->p_hstage.bytes()) return RIA_OK;
    HIP_TRY(h, hipStreamSynchronize(h->hstream));   // one drain of the handle's stream for both blocks
    HIP_TRY(h, h->d_hstage.reserve(bytes));
    HIP_TRY(h, h->p_hstage.reserve(bytes));
    return RIA_OK;
}
// One host-buffer call on the handle's staging block and stream.  `carve` lays the block out around the caller's host
// pointers (host_stage.hpp); `call` is the batch form on the device block's areas.  The inputs go up in one copy, the
// outputs from the first wanted one on come back in one copy, one stream sync, and the caller's buffers hold the results.
extern "C++" {   // a template has no C linkage
template <class Carve, class Call>
static int host_staged(ria_gpu_handle h, Carve&& carve, Call&& call) {
    StageCarver size_pass;
    carve(size_pass);
    if (!size_pass.valid()) return fail(h, RIA_ERR_INVALID, "staging block: an input behind an output, or too many areas");
    if (int rc = ensure_host_stage(h, size_pass.size())) return rc;
    unsigned char *D = h->d_hstage.as<unsigned char>(), *P = h->p_hstage.as<unsigned char>();
    StageCarver pinned(P), device(D);
    carve(pinned);
    const auto on_device = carve(device);
    hipStream_t s = h->hstream;
    pinned.fill();
    HIP_TRY(h, hipMemcpyAsync(D, P, pinned.upload_end(), hipMemcpyHostToDevice, s));
    if (int rc = call(on_device, s)) return rc;
    const size_t out0 = pinned.download_begin();
    HIP_TRY(h, hipMemcpyAsync(P + out0, D + out0, pinned.size() - out0, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    pinned.drain();
    return RIA_OK;
}
}

int ria_gpu_rx_frames_host(ria_gpu_handle h, const float* samples_host, const ria_frame_meta* meta_host, int n_frames,
                           uint32_t flags, uint8_t* info_out_host, ria_decode_status* decode_status_host,
                           float* llr_out_host, ria_frame_status* demod_status_host) {
    const bool demod_only = (flags & RIA_RX_DEMOD_ONLY) != 0;
    if (!h || !samples_host || n_frames <= 0 || (!demod_only && (!info_out_host || !decode_status_host)) || (demod_only && !llr_out_host))
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_frames_host: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    const ria_gpu_geometry& g = h->geo;
    const size_t n = static_cast<size_t>(n_frames);
    struct Stage { float* x; ria_frame_meta* meta; float* llr; uint8_t* info; ria_decode_status* ds; ria_frame_status* fs; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.x = c.in(n * g.frame_samples, samples_host); w.meta = c.in(n, meta_host);   // without meta only the samples go up
        w.llr = c.out(n * g.llrs_per_frame, llr_out_host);
        w.info = c.out(n * g.info_bytes_per_frame, demod_only ? nullptr : info_out_host); w.ds = c.out(n, demod_only ? nullptr : decode_status_host);
        w.fs = c.out(n, demod_status_host);
        return w;
    };
    if (int rc = host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
            if (demod_only) return ria_gpu_demod_batch(h, d.x, nullptr, d.meta, n_frames, d.llr, d.fs, s);
            return ria_gpu_rx_batch(h, d.x, nullptr, d.meta, n_frames, flags, d.info, d.ds, d.llr, d.fs, s); })) return rc;
    if (!demod_only && decode_status_host[0].reserved[1] == kDecodeFaultMarker) return fail(h, RIA_ERR_HIP, "decode work-queue fault: no frame of this call was decoded");
    return RIA_OK;
}

int ria_gpu_decode_frames_host(ria_gpu_handle h, const float* llr_host, int llr_stride, int n_frames, uint32_t flags,
                               uint8_t* info_out_host, ria_decode_status* status_host) {
    if (!h || !llr_host || !info_out_host || !status_host || n_frames <= 0 || llr_stride < kFrameBits)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_decode_frames_host: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = static_cast<size_t>(n_frames);
    struct Stage { float* llr; uint8_t* info; ria_decode_status* ds; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.llr = c.in(n * llr_stride, llr_host); w.info = c.out(n * h->geo.info_bytes_per_frame, info_out_host); w.ds = c.out(n, status_host);
        return w;
    };
    if (int rc = host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
            return ria_gpu_decode_batch(h, d.llr, llr_stride, n_frames, flags, d.info, d.ds, s); })) return rc;
    if (status_host[0].reserved[1] == kDecodeFaultMarker) return fail(h, RIA_ERR_HIP, "decode work-queue fault: no frame of this call was decoded");
    return RIA_OK;
}

// ------------------------------------------------------------------------------------------------ TX / channel
int ria_gpu_make_frames(ria_gpu_handle h, uint64_t seed, int first_seq, int n_frames, uint8_t* info_out_dev,
                        void* stream) {
    if (!h || !info_out_dev || n_frames < 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_make_frames: bad argument");
    if (n_frames == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    launch_make_frames(h->d_tx_const.as<const TxConst>(), h->d_crc_bit.as<const uint16_t>(),
                       h->d_crc_init.as<const uint16_t>(), seed, first_seq, n_frames, h->geo, info_out_dev,
                       static_cast<hipStream_t>(stream));
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_tx_batch(ria_gpu_handle h, const uint8_t* info_dev, int n_frames, float peak_normalize,
                     float* samples_out_dev, void* stream) {
    if (!h || !info_dev || !samples_out_dev || n_frames < 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_tx_batch: bad argument");
    if (n_frames == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    launch_tx(h->d_tx_const.as<const TxConst>(), h->d_twiddle.as<const float2>(),
              h->d_nco.as<const float2>(), info_dev, n_frames, peak_normalize, h->geo, samples_out_dev,
              static_cast<hipStream_t>(stream));
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_encode_frames_batch(ria_gpu_handle h, const uint8_t* info_dev, int n_frames, uint8_t* coded_out_dev, void* stream) {
    if (!h || !info_dev || !coded_out_dev || n_frames < 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_encode_frames_batch: bad argument");
    if (n_frames == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    launch_tx_mode<1>(h->d_tx_const.as<const TxConst>(), h->d_twiddle.as<const float2>(),
                      h->d_nco.as<const float2>(), info_dev, n_frames, 0.0f, h->geo, nullptr, coded_out_dev,
                      static_cast<hipStream_t>(stream));
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_tx_coded_batch(ria_gpu_handle h, const uint8_t* coded_dev, int n_frames, float peak_normalize,
                           float* samples_out_dev, void* stream) {
    if (!h || !coded_dev || !samples_out_dev || n_frames < 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_tx_coded_batch: bad argument");
    if (n_frames == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    launch_tx_mode<2>(h->d_tx_const.as<const TxConst>(), h->d_twiddle.as<const float2>(),
                      h->d_nco.as<const float2>(), coded_dev, n_frames, peak_normalize, h->geo, samples_out_dev, nullptr,
                      static_cast<hipStream_t>(stream));
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_channel_batch(ria_gpu_handle h, int kind, float snr_db, uint64_t seed, uint64_t first_frame,
                          float* samples_dev, int n_frames, void* stream) {
    if (!h || !samples_dev || n_frames < 0 || kind < 0 || kind > 4)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_channel_batch: bad argument");
    if (n_frames == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    launch_channel(kind, snr_db, seed, first_frame, samples_dev, n_frames, h->geo.frame_samples,
                   static_cast<hipStream_t>(stream));
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// per-frame workspace of channel_power_kernel, grown on demand (a growth waits for the stream's earlier users of the old block)
static int chan_ws(ria_gpu_handle h, int n_frames, hipStream_t s) {
    HIP_TRY(h, h->d_chan_nstd.reserve(static_cast<size_t>(std::max(n_frames, 4096)) * sizeof(float), &s));
    return RIA_OK;
}

int ria_gpu_channel_exact_batch(ria_gpu_handle h, int kind, float snr_db, uint32_t seed, uint64_t first_frame,
                                float* samples_dev, int64_t stride, int frame_samples, int n_frames, void* stream) {
    if (!h || n_frames < 0 || kind < 0 || kind > 4 || frame_samples < 0 || stride < frame_samples)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_channel_exact_batch: bad argument");
    if (n_frames == 0 || frame_samples == 0) return RIA_OK;
    if (!samples_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_channel_exact_batch: null samples");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = chan_ws(h, n_frames, static_cast<hipStream_t>(stream))) return rc;
    launch_channel_exact(kind, snr_db, seed, first_frame, samples_dev, stride, frame_samples, n_frames, static_cast<hipStream_t>(stream), h->d_chan_nstd.as<float>());
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_channel_exact_seeded_batch(ria_gpu_handle h, int kind, float snr_db, const uint32_t* seeds_dev, float* samples_dev,
                                       int64_t stride, int frame_samples, int n_frames, void* stream) {
    if (!h || n_frames < 0 || kind < 0 || kind > 4 || frame_samples < 0 || stride < frame_samples)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_channel_exact_seeded_batch: bad argument");
    if (n_frames == 0 || frame_samples == 0) return RIA_OK;
    if (!samples_dev || !seeds_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_channel_exact_seeded_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = chan_ws(h, n_frames, static_cast<hipStream_t>(stream))) return rc;
    launch_channel_exact(kind, snr_db, 0u, 0u, samples_dev, stride, frame_samples, n_frames, static_cast<hipStream_t>(stream), h->d_chan_nstd.as<float>(), seeds_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_channel_exact_cfo_batch(ria_gpu_handle h, int kind, float snr_db, const uint32_t* seeds_dev, const float* cfo_hz_dev,
                                    float random_cfo_max_hz, float* actual_cfo_out_dev, float* samples_dev, int64_t stride,
                                    int frame_samples, int n_frames, void* stream) {
    if (!h || n_frames < 0 || kind < 0 || kind > 4 || frame_samples < 0 || stride < frame_samples || !(random_cfo_max_hz >= 0.0f))
        return fail(h, RIA_ERR_INVALID, "ria_gpu_channel_exact_cfo_batch: bad argument");
    if (n_frames == 0 || frame_samples == 0) return RIA_OK;
    if (!samples_dev || !seeds_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_channel_exact_cfo_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = chan_ws(h, n_frames, static_cast<hipStream_t>(stream))) return rc;
    launch_channel_exact(kind, snr_db, 0u, 0u, samples_dev, stride, frame_samples, n_frames, static_cast<hipStream_t>(stream), h->d_chan_nstd.as<float>(), seeds_dev,
                         cfo_hz_dev, 0.0f, random_cfo_max_hz, actual_cfo_out_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// ------------------------------------------------------------------------------------------------ debug
__global__ void debug_math_kernel(int op, const float* a, const float* b, int n, float* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b ? b[i] : 0.0f, r;
    switch (op) {
        case 0: r = sinf_glibc(x); break;
        case 1: r = cosf_glibc(x); break;
        case 2: r = logf_glibc(x); break;
        case 3: r = atan2f_glibc(x, y); break;
        case 4: r = hypotf_glibc(x, y); break;
        case 5: r = fdiv(x, y); break;
        default: r = fsqrt(x); break;
    }
    out[i] = r;
}

// threshold_dev / param_stride: per-buffer threshold and known CFO records (ZcArgs); null / 1 = the public call
static int sync_zc_impl(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                        float threshold, uint32_t root_mask, const float* known_cfo_dev, ria_zc_result* out_dev,
                        void* stream, const float* threshold_dev, int param_stride) {
    if (!h) return RIA_ERR_INVALID;
    if (n_buffers == 0) return RIA_OK;
    if (!samples_dev || !out_dev || n_buffers < 0 || buf_len < 0 || buf_len > kZcMaxBuf || stride < buf_len)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_sync_zc_batch: bad arguments");
    ZcArgs A{};
    A.samples = samples_dev; A.stride = stride; A.buf_len = buf_len; A.n_buffers = n_buffers; A.threshold = threshold;
    A.root_mask = root_mask & 15u; A.known_cfo = known_cfo_dev; A.ref = h->d_zc_ref.as<const float2>(); A.out = out_dev;
    A.threshold_dev = threshold_dev; A.param_stride = param_stride;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (buf_len <= kZcLdsBuf) {   // the mixed-down buffer fits one workgroup's LDS
        const int lds = buf_len * static_cast<int>(sizeof(float2)) + 4 * static_cast<int>(sizeof(ZcRootOut));
        if (lds > h->zc_lds_opted) {   // the opt-in is a per-device attribute: kept per handle (= per device), not per process
            HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(zc_detect_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            h->zc_lds_opted = lds;
        }
        hipLaunchKernelGGL(zc_detect_kernel<true>, dim3(n_buffers), dim3(256), lds, s, A);
    } else {                      // long search windows: baseband in a global workspace, chunks of buffers under 256 MiB
        const size_t per = static_cast<size_t>(buf_len) * sizeof(float2);
        const int chunk = static_cast<int>(std::min<size_t>(n_buffers, std::max<size_t>(1, (size_t(256) << 20) / per)));
        HIP_TRY(h, h->d_zc_ws.reserve(per * chunk, &s));   // a growth waits for the stream's earlier users of the old block
        A.bb_ws = h->d_zc_ws.as<float2>();
        for (int first = 0; first < n_buffers; first += chunk) {
            A.samples = samples_dev + static_cast<int64_t>(first) * stride; A.n_buffers = std::min(chunk, n_buffers - first);
            A.known_cfo = known_cfo_dev ? known_cfo_dev + static_cast<int64_t>(first) * param_stride : nullptr; A.out = out_dev + first;
            A.threshold_dev = threshold_dev ? threshold_dev + static_cast<int64_t>(first) * param_stride : nullptr;
            hipLaunchKernelGGL(zc_detect_kernel<false>, dim3(A.n_buffers), dim3(256), 4 * static_cast<int>(sizeof(ZcRootOut)), s, A);
        }
    }
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_sync_zc_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                          float threshold, uint32_t root_mask, const float* known_cfo_dev, ria_zc_result* out_dev,
                          void* stream) {
    return sync_zc_impl(h, samples_dev, stride, buf_len, n_buffers, threshold, root_mask, known_cfo_dev, out_dev, stream, nullptr, 1);
}

int ria_gpu_zc_preamble(ria_gpu_handle h, int root, float* out_host, int max_n) {
    if (!h || !out_host) return RIA_ERR_INVALID;
    std::vector<float> p = build_zc_preamble(root);
    if (static_cast<int>(p.size()) > max_n) return -static_cast<int>(p.size());
    std::memcpy(out_host, p.data(), p.size() * sizeof(float));
    return static_cast<int>(p.size());
}

// forward or inverse 131072-point FFT of the active buffers of a chunk (see sync_kernels.hip.h)
static void chirp_fft_forward(const ChirpArgs& A, int chunk, hipStream_t s, bool real_input, bool product) {
    // 17 radix-2 stages as 6 + 6 + 5 register-resident butterfly networks (64 / 64 / 32 points per thread): three trips over the
    // 1 MiB per buffer instead of the four of 4 + 4 + 4 + 5 (measured: 83 k -> 96 k preambles/s)
    const dim3 g64(kChFft / 64 / 256, chunk), g32(kChFft / 32 / 256, chunk), blk(256);
    if (real_input) hipLaunchKernelGGL((chirp_fft_pass<6, 0, 1, false>), g64, blk, 0, s, A, static_cast<const float2*>(nullptr), A.w1);
    else hipLaunchKernelGGL((chirp_fft_pass<6, 0, 2, false>), g64, blk, 0, s, A, static_cast<const float2*>(A.w2), A.w1);
    hipLaunchKernelGGL((chirp_fft_pass<6, 6, 0, false>), g64, blk, 0, s, A, static_cast<const float2*>(nullptr), A.w1);
    if (product) hipLaunchKernelGGL((chirp_fft_pass<5, 12, 3, false>), g32, blk, 0, s, A, static_cast<const float2*>(nullptr), A.w1);
    else hipLaunchKernelGGL((chirp_fft_pass<5, 12, 0, false>), g32, blk, 0, s, A, static_cast<const float2*>(nullptr), A.w1);
}
static void chirp_fft_inverse_mag(const ChirpArgs& A, int chunk, hipStream_t s) {
    const dim3 g64(kChFft / 64 / 256, chunk), g32(kChFft / 32 / 256, chunk), blk(256);
    (void)hipMemsetAsync(A.best, 0, static_cast<size_t>(chunk) * sizeof(unsigned long long), s);
    hipLaunchKernelGGL((chirp_fft_pass<6, 0, 2, true>), g64, blk, 0, s, A, static_cast<const float2*>(A.w1), A.w2);
    hipLaunchKernelGGL((chirp_fft_pass<6, 6, 0, true>), g64, blk, 0, s, A, static_cast<const float2*>(nullptr), A.w2);
    hipLaunchKernelGGL((chirp_fft_pass<5, 12, 4, true>), g32, blk, 0, s, A, static_cast<const float2*>(nullptr), A.w2);
}
__global__ void chirp_template_stage_kernel(const float* tmpl, int down, float2* dst, ChirpBufState* st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { st[0].active = 1; st[0].win_start = 0; st[0].win_len = kChFft; }
    if (i >= kChFft) return;
    // complex template cos + j*sin, zero padded (chirp_sync.hpp:589-594)
    dst[i] = (i < kChLen) ? make_float2(tmpl[(2 * down + 1) * kChLen + i], tmpl[(2 * down) * kChLen + i]) : make_float2(0.f, 0.f);
}
__global__ void chirp_template_conj_kernel(const float2* src, float2* dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kChFft) dst[i] = make_float2(src[i].x, -src[i].y);
}

static int chirp_prepare(ria_gpu_handle h, int chunk, int outer, hipStream_t s) {
    hipError_t e;
#define C_TRY(expr) if ((e = (expr)) != hipSuccess) return fail(h, RIA_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e))
    const size_t c = static_cast<size_t>(chunk);
    C_TRY(h->d_ch_w1.reserve(c * kChFft * sizeof(float2)));
    C_TRY(h->d_ch_w2.reserve(c * kChFft * sizeof(float2)));
    C_TRY(h->d_ch_mag.reserve(c * sizeof(unsigned long long)));   // packed first-maximum keys
    C_TRY(h->d_ch_cum.reserve(static_cast<size_t>(outer) * (kChFft + 1) * sizeof(float)));
    C_TRY(h->d_ch_st.reserve(static_cast<size_t>(outer) * sizeof(ChirpBufState)));
    if (!h->d_ch_tmpl_fft) {
        ChirpTables t = build_chirp_tables();
        if (!h->d_ch_tw) C_TRY(upload(h->d_ch_tw, t.tw));
        C_TRY(upload(h->d_ch_tmpl, t.tmpl));
        h->ch_energy[0] = t.energy[0]; h->ch_energy[1] = t.energy[1];
        C_TRY(h->d_ch_tmpl_fft.reserve(static_cast<size_t>(2) * kChFft * sizeof(float2)));
        // conj(FFT(template)) with the same butterflies the signal goes through (chirp_sync.hpp:573-623)
        ChirpArgs A{};
        A.n_buffers = 1; A.tw = h->d_ch_tw.as<const float2>(); A.w1 = h->d_ch_w1.as<float2>();
        A.w2 = h->d_ch_w2.as<float2>(); A.st = h->d_ch_st.as<ChirpBufState>();
        for (int d = 0; d < 2; ++d) {
            hipLaunchKernelGGL(chirp_template_stage_kernel, dim3(kChFft / 256), dim3(256), 0, s, h->d_ch_tmpl.as<const float>(), d, A.w2, A.st);
            chirp_fft_forward(A, 1, s, false, false);
            hipLaunchKernelGGL(chirp_template_conj_kernel, dim3(kChFft / 256), dim3(256), 0, s, static_cast<const float2*>(A.w1),
                               h->d_ch_tmpl_fft.as<float2>() + static_cast<size_t>(d) * kChFft);
        }
        C_TRY(hipGetLastError());
    }
#undef C_TRY
    return RIA_OK;
}

static int sync_chirp_impl(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                           float threshold, ria_chirp_result* out_dev, void* stream, const float* threshold_dev, int param_stride);
int ria_gpu_sync_chirp_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                             float threshold, ria_chirp_result* out_dev, void* stream) {
    return sync_chirp_impl(h, samples_dev, stride, buf_len, n_buffers, threshold, out_dev, stream, nullptr, 1);
}

static int sync_chirp_impl(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                           float threshold, ria_chirp_result* out_dev, void* stream, const float* threshold_dev, int param_stride) {
    if (!h) return RIA_ERR_INVALID;
    if (n_buffers == 0) return RIA_OK;
    if (!samples_dev || !out_dev || n_buffers < 0 || buf_len < 0 || stride < buf_len)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_sync_chirp_batch: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // Two levels of chunking.  The FFT workspace (2.5 MiB per buffer) is sized for 64 buffers so that it stays
    // within the 256 MiB Infinity Cache across the eight passes of a transform pair.  The serial pieces (energy
    // cumsum: one wave per buffer; time-domain fallback) are latency-bound and want as many buffers in flight as
    // possible, so they run once per OUTER chunk of up to 2048 buffers (0.5 MiB of running sums each).
    const int chunk = std::min(n_buffers, 64), outer = std::min(n_buffers, 2048);
    int rc = chirp_prepare(h, chunk, outer, s);
    if (rc != RIA_OK) return rc;
    if (!h->ch_side) {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->ch_side, hipStreamNonBlocking));
        for (auto& ev_ : h->ch_ev) HIP_TRY(h, hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
    }
    ChirpArgs A{};
    A.samples = samples_dev; A.stride = stride; A.buf_len = buf_len; A.threshold = threshold;
    A.tw = h->d_ch_tw.as<const float2>(); A.tmpl_fft = h->d_ch_tmpl_fft.as<const float2>();
    A.tmpl = h->d_ch_tmpl.as<const float>(); A.tmpl_energy[0] = h->ch_energy[0]; A.tmpl_energy[1] = h->ch_energy[1];
    A.w1 = h->d_ch_w1.as<float2>(); A.w2 = h->d_ch_w2.as<float2>(); A.best = h->d_ch_mag.as<unsigned long long>();
    A.cum = h->d_ch_cum.as<float>(); A.st = h->d_ch_st.as<ChirpBufState>(); A.out = out_dev;
    A.threshold_dev = threshold_dev; A.param_stride = param_stride;
    for (int first = 0; first < n_buffers; first += outer) {
        const int nb = std::min(outer, n_buffers - first);
        A.first = first; A.n_buffers = nb;
        for (int down = 0; down < 2; ++down) {
            A.down = down; A.sub = 0; A.n_sub = nb;
            hipLaunchKernelGGL(chirp_window_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, A);
            hipLaunchKernelGGL(chirp_cumsum_kernel, dim3((nb + kCumB - 1) / kCumB), dim3(64), 0, s, A);
            if (down) {
                // the time-domain fallback (short down windows: a few buffers, 24 000-term sums per candidate, one workgroup
                // per buffer) touches other buffers than the FFT path and is latency-bound: it runs beside it on a side stream
                HIP_TRY(h, hipEventRecord(h->ch_ev[0], s));
                HIP_TRY(h, hipStreamWaitEvent(h->ch_side, h->ch_ev[0], 0));
                hipLaunchKernelGGL(chirp_td_kernel, dim3(nb), dim3(256), 0, h->ch_side, A);
                HIP_TRY(h, hipEventRecord(h->ch_ev[1], h->ch_side));
            }
            for (int sub = 0; sub < nb; sub += chunk) {
                A.sub = sub; A.n_sub = std::min(chunk, nb - sub);
                chirp_fft_forward(A, A.n_sub, s, true, true);
                chirp_fft_inverse_mag(A, A.n_sub, s);
                hipLaunchKernelGGL(chirp_peak_kernel, dim3((A.n_sub + 63) / 64), dim3(64), 0, s, A);
            }
            if (down) HIP_TRY(h, hipStreamWaitEvent(s, h->ch_ev[1], 0));
        }
        A.sub = 0; A.n_sub = nb;
        hipLaunchKernelGGL(chirp_finish_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, A);
    }
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// SimulatedChannel::applyTxCFO for a batch of transmissions (cfo_kernels.hip.h)
int ria_gpu_tx_cfo_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int n_samples, int n_buffers,
                         const float* cfo_hz_dev, float* phase_inout_dev, float* out_dev, int64_t out_stride, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_buffers == 0 || n_samples == 0) return RIA_OK;
    if (!samples_dev || !out_dev || !cfo_hz_dev || n_buffers < 0 || n_samples < 0 || stride < n_samples || out_stride < n_samples || samples_dev == out_dev)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_tx_cfo_batch: bad arguments");
    if (n_samples > (1 << kTxCfoMaxLog)) return fail(h, RIA_ERR_UNSUPPORTED, "ria_gpu_tx_cfo_batch: at most 131072 samples per transmission");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!h->d_ch_tw) { ChirpTables t = build_chirp_tables(); HIP_TRY(h, upload(h->d_ch_tw, t.tw)); }
    int L = 0;
    while ((1 << L) < n_samples) ++L;
    const size_t N = size_t(1) << L, per = 2 * N * sizeof(float2) + static_cast<size_t>(n_samples) * sizeof(float);
    // buffers per pass: the workspace of one pass stays under 256 MiB (and the grid's y extent under 65536)
    const int chunk = static_cast<int>(std::min<size_t>(std::min(n_buffers, 32768), std::max<size_t>(1, (size_t(256) << 20) / per)));
    HIP_TRY(h, h->d_txcfo_ws.reserve(per * static_cast<size_t>(chunk), &s));   // a growth waits for the stream's earlier users of the old block
    for (int first = 0; first < n_buffers; first += chunk) {
        const int nb = std::min(chunk, n_buffers - first);
        TxCfoArgs A{};
        A.in = samples_dev + static_cast<int64_t>(first) * stride; A.in_stride = stride;
        A.out = out_dev + static_cast<int64_t>(first) * out_stride; A.out_stride = out_stride;
        A.n = n_samples; A.log2n = L; A.n_buffers = nb; A.cfo_hz = cfo_hz_dev + first; A.phase = phase_inout_dev ? phase_inout_dev + first : nullptr;
        A.tw = h->d_ch_tw.as<const float2>();
        A.w1 = h->d_txcfo_ws.as<float2>(); A.w2 = A.w1 + static_cast<size_t>(nb) * N; A.ph = reinterpret_cast<float*>(A.w2 + static_cast<size_t>(nb) * N);
        hipLaunchKernelGGL(txcfo_phase_kernel, dim3((nb + 63) / 64), dim3(64), 0, s, A);
        for (int inv = 0; inv < 2; ++inv) {
            float2* dst = inv ? A.w2 : A.w1;
            for (int S0 = 0; S0 < L;) {
                const int G = std::min(6, L - S0);
                const int mode = (S0 == 0) ? (inv ? 2 : 1) : 0;
                const dim3 grid(static_cast<unsigned>(((N >> G) + 255) / 256), nb), blk(256);
                const float2* src = A.w1;
                switch (G) {
                    case 1: hipLaunchKernelGGL(txcfo_fft_pass<1>, grid, blk, 0, s, A, src, dst, S0, mode, inv); break;
                    case 2: hipLaunchKernelGGL(txcfo_fft_pass<2>, grid, blk, 0, s, A, src, dst, S0, mode, inv); break;
                    case 3: hipLaunchKernelGGL(txcfo_fft_pass<3>, grid, blk, 0, s, A, src, dst, S0, mode, inv); break;
                    case 4: hipLaunchKernelGGL(txcfo_fft_pass<4>, grid, blk, 0, s, A, src, dst, S0, mode, inv); break;
                    case 5: hipLaunchKernelGGL(txcfo_fft_pass<5>, grid, blk, 0, s, A, src, dst, S0, mode, inv); break;
                    default: hipLaunchKernelGGL(txcfo_fft_pass<6>, grid, blk, 0, s, A, src, dst, S0, mode, inv); break;
                }
                S0 += G;
            }
        }
        hipLaunchKernelGGL(txcfo_rotate_kernel, dim3((n_samples + 255) / 256, nb), dim3(256), 0, s, A);
    }
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_chirp_preamble(ria_gpu_handle h, float* out_host, int max_n) {
    if (!h || !out_host) return RIA_ERR_INVALID;
    std::vector<float> p = build_chirp_preamble();
    if (static_cast<int>(p.size()) > max_n) return -static_cast<int>(p.size());
    std::memcpy(out_host, p.data(), p.size() * sizeof(float));
    return static_cast<int>(p.size());
}

// the LTS detector's tables and LDS opt-in, made once per handle
static int lts_prepare(ria_gpu_handle h) {
    if (!h->d_hilbert65) HIP_TRY(h, upload(h->d_hilbert65, build_hilbert(65)));
    if (!h->lts_lds_opted) {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(lts_sync_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lts_lds_bytes()));
        h->lts_lds_opted = 1;
    }
    return RIA_OK;
}

int ria_gpu_sync_lts_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                           const float* known_cfo_dev, float threshold, ria_lts_result* out_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_buffers == 0) return RIA_OK;
    if (!samples_dev || !out_dev || n_buffers < 0 || buf_len < 0 || stride < buf_len)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_sync_lts_batch: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = lts_prepare(h)) return rc;
    LtsArgs A{};
    A.samples = samples_dev; A.stride = stride; A.buf_len = buf_len; A.n_buffers = n_buffers; A.known_cfo = known_cfo_dev;
    A.threshold = threshold; A.hilbert = h->d_hilbert65.as<const float>(); A.out = out_dev;
    hipLaunchKernelGGL(lts_sync_kernel, dim3(n_buffers), dim3(kLtsThreads), lts_lds_bytes(), static_cast<hipStream_t>(stream), A);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_sync_cox_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                           float threshold, const float* noise_floor_dev, ria_cox_result* out_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_buffers == 0) return RIA_OK;
    if (!samples_dev || !out_dev || n_buffers < 0 || buf_len < 0 || buf_len > kCoxMaxBuf || stride < buf_len)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_sync_cox_batch: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!h->d_cox_tI || !h->d_cox_tQ) {
        const CoxTemplate t = build_cox_template(h->plan);
        HIP_TRY(h, upload(h->d_cox_tI, t.tI));
        HIP_TRY(h, upload(h->d_cox_tQ, t.tQ));
        h->cox_energy_ref = t.energy_ref;
    }
    const bool searched = buf_len >= kCoxMinSearch && buf_len >= kCoxTotal + kCoxWindow;
    const int nM = searched ? cox_n_metric(buf_len) : 0, nE = searched ? cox_n_energy(buf_len) : 0;
    const size_t per = 2 * static_cast<size_t>(nM) + static_cast<size_t>(nE);
    // buffers per pass: the tables of one pass stay under 256 MiB and the grid's y extent under 65536
    int chunk = n_buffers;
    if (per) chunk = static_cast<int>(std::min<size_t>(chunk, std::max<size_t>(1, (size_t(64) << 20) / per)));
    chunk = std::min(chunk, 32768);
    HIP_TRY(h, h->d_cox_ws.reserve((per * static_cast<size_t>(chunk) + 16) * sizeof(float), &s));   // a growth waits for the stream's earlier users of the old block
    for (int first = 0; first < n_buffers; first += chunk) {
        const int nb = std::min(chunk, n_buffers - first);
        CoxArgs A{};
        A.samples = samples_dev + static_cast<int64_t>(first) * stride; A.stride = stride; A.buf_len = buf_len; A.n_buffers = nb;
        A.threshold = threshold; A.noise_in = noise_floor_dev ? noise_floor_dev + first : nullptr;
        A.twiddle = h->d_twiddle.as<const float2>();
        A.tI = h->d_cox_tI.as<const float>(); A.tQ = h->d_cox_tQ.as<const float>(); A.energy_ref = h->cox_energy_ref;
        float* ws = h->d_cox_ws.as<float>();
        A.dc = ws; A.metric = ws + static_cast<size_t>(nM) * nb; A.energy = ws + 2 * static_cast<size_t>(nM) * nb;
        A.nM = nM; A.nE = nE; A.out = out_dev + first;
        if (nM > 0) {
            hipLaunchKernelGGL(cox_prepare_kernel, dim3((nM + 255) / 256, nb), dim3(256), 0, s, A);
            hipLaunchKernelGGL(cox_metric_kernel<0>, dim3(((nM + 7) / 8 + 3) / 4, nb), dim3(256), 0, s, A);
            hipLaunchKernelGGL(cox_metric_kernel<1>, dim3((nM + 3) / 4, nb), dim3(256), 0, s, A);
        }
        hipLaunchKernelGGL(cox_scan_kernel, dim3(nb), dim3(1024), 0, s, A);
    }
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_cox_preamble(ria_gpu_handle h, float* out_host, int max_n) {
    if (!h || !out_host) return RIA_ERR_INVALID;
    std::vector<float> p = build_cox_preamble(h->plan);
    if (static_cast<int>(p.size()) > max_n) return -static_cast<int>(p.size());
    std::memcpy(out_host, p.data(), p.size() * sizeof(float));
    return static_cast<int>(p.size());
}

// ------------------------------------------------------------------------------------------------ acquire + decode
// one work list of n rows: its four arrays back to back in one area, widest first
static void take_frame_list(Carver& c, FrameList& l, size_t n) { c.take_list(n, l.offset, l.meta, l.window, l.state); }

// the acquisition workspace for n windows
struct AcqWs {
    ria_lts_result* lts;
    FrameList list[2];
    uint8_t* info; ria_decode_status* dst; ria_frame_status* fst;   // compact outputs of one round
    AcqCtl* ctl;
};
static AcqWs acq_carve(Carver& c, size_t n, size_t info_bytes) {
    AcqWs w;
    w.lts = c.take<ria_lts_result>(n);
    for (FrameList& l : w.list) take_frame_list(c, l, n);
    w.info = c.take<uint8_t>(n * info_bytes);
    w.dst = c.take<ria_decode_status>(n);
    w.fst = c.take<ria_frame_status>(n);
    w.ctl = c.take<AcqCtl>(1);
    return w;
}

// grows the acquisition workspace to n_windows; nothing of an earlier call is in flight: every call ends on a stream sync
static int acq_ensure_ws(ria_gpu_handle h, int n_windows, AcqWs* out) {
    const size_t ib = static_cast<size_t>(h->geo.info_bytes_per_frame);
    if (n_windows > h->acq_windows) {
        h->acq_windows = 0;
        HIP_TRY(h, h->d_acq_ws.reserve(carved_size([&](Carver& c) { return acq_carve(c, n_windows, ib); })));
        h->acq_windows = n_windows;
    }
    HIP_TRY(h, h->p_acq_ctl.reserve(sizeof(AcqCtl)));
    *out = carve_at(h->d_acq_ws.as<>(), [&](Carver& c) { return acq_carve(c, h->acq_windows, ib); });
    return RIA_OK;
}

// LTS detection of every window with its own threshold and known CFO (ria_acq_params); lts_prepare has run
static void launch_lts_acquire(ria_gpu_handle h, const float* samples_dev, int64_t stride, int search_len, int n_windows,
                               const ria_acq_params* params_dev, ria_lts_result* out, hipStream_t s) {
    LtsArgs S{};
    S.samples = samples_dev; S.stride = stride; S.buf_len = search_len; S.n_buffers = n_windows;
    S.known_cfo = &params_dev->known_cfo_hz; S.threshold_dev = &params_dev->detect_threshold;
    S.param_stride = static_cast<int>(sizeof(ria_acq_params) / sizeof(float));
    S.hilbert = h->d_hilbert65.as<const float>();
    S.out = out;
    hipLaunchKernelGGL(lts_sync_kernel, dim3(n_windows), dim3(kLtsThreads), lts_lds_bytes(), s, S);
}

// The rounds of ria_gpu_rx_acquire_batch on a planned round-0 list (lists[0] of the handle's workspace, its length in
// A.ctl): round 0 runs every accepted window at its primary candidate, round r >= 1 the windows whose previous candidate
// decoded nothing at their next candidate that fits; at most 8 recovery rounds (each advances every window it holds by at
// least one of the 8 deltas).  A.acq / A.info_out / A.dst_out / A.fst_out take one row per window.
static int acq_run_rounds(ria_gpu_handle h, const char* who, const float* samples_dev, AcqArgs A, const AcqWs& W, int n_windows,
                          uint32_t flags, hipStream_t s) {
    A.info_c = W.info; A.dst_c = W.dst; A.fst_c = W.fst;
    const uint32_t dflags = flags & (RIA_DECODE_FULL | RIA_DECODE_NO_CHANNEL_DEINTERLEAVE);
    for (int round = 0;; ++round) {
        if (int rc = read_ctl(h, h->p_acq_ctl, A.ctl, s, "decode work-queue fault in round %d: no window of this call was decoded", round - 1)) return rc;
        const int n_list = static_cast<int>(h->p_acq_ctl.as<AcqCtl>()->n_list);
        if (n_list == 0) break;
        if (n_list > n_windows || round >= kAcqCandidates) return fail(h, RIA_ERR_HIP, "%s: work list of round %d broke its bound (%d)", who, round, n_list);
        A.cur = W.list[round & 1];
        A.next = W.list[(round + 1) & 1];
        A.n_cur = n_list;
        A.round = round;
        A.retry = !(flags & RIA_ACQ_NO_TIMING_RETRY) && round + 1 < kAcqCandidates;
        int rc = ria_gpu_rx_batch(h, samples_dev, A.cur.offset, A.cur.meta, n_list, dflags, W.info, W.dst, nullptr, W.fst, s);
        if (rc != RIA_OK) return rc;
        hipLaunchKernelGGL(acq_scatter_kernel, dim3(std::min((n_list + 3) / 4, 4096)), dim3(256), 0, s, A);
        hipLaunchKernelGGL(acq_next_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
        HIP_TRY(h, hipGetLastError());
    }
    return RIA_OK;
}

int ria_gpu_rx_acquire_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int search_len, int window_len,
                             int n_windows, const ria_acq_params* params_dev, uint32_t flags,
                             uint8_t* info_out_dev, ria_decode_status* decode_status_dev, ria_acq_result* acq_dev,
                             ria_frame_status* demod_status_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    const uint32_t known_flags = RIA_DECODE_FULL | RIA_DECODE_NO_CHANNEL_DEINTERLEAVE | RIA_ACQ_NO_TIMING_RETRY;
    if (n_windows < 0 || search_len < 0 || window_len < search_len || stride < window_len || (flags & ~known_flags) != 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_acquire_batch: bad argument (0 <= search_len <= window_len <= stride; flags: RIA_DECODE_* and RIA_ACQ_NO_TIMING_RETRY only)");
    if (n_windows == 0) return RIA_OK;
    if (!samples_dev || !params_dev || !info_out_dev || !decode_status_dev || !acq_dev)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_acquire_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lts_prepare(h)) return rc;
    const size_t n = static_cast<size_t>(n_windows), ib = static_cast<size_t>(h->geo.info_bytes_per_frame);
    AcqWs W;
    if (int rc = acq_ensure_ws(h, n_windows, &W)) return rc;
    HIP_TRY(h, hipMemsetAsync(info_out_dev, 0, n * ib, s));
    HIP_TRY(h, hipMemsetAsync(decode_status_dev, 0, n * sizeof(ria_decode_status), s));
    if (demod_status_dev) HIP_TRY(h, hipMemsetAsync(demod_status_dev, 0, n * sizeof(ria_frame_status), s));

    // 1. LTS detection with each window's threshold and known CFO
    launch_lts_acquire(h, samples_dev, stride, search_len, n_windows, params_dev, W.lts, s);
    // 2. acceptance + the round-0 list
    AcqArgs A{};
    A.lts = W.lts; A.params = params_dev; A.n_windows = n_windows; A.window_len = window_len;
    A.frame_samples = h->geo.frame_samples; A.stride = stride; A.acq = acq_dev;
    A.ctl = W.ctl;
    A.next = W.list[0];
    hipLaunchKernelGGL(acq_plan_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
    HIP_TRY(h, hipGetLastError());
    A.info_bytes = static_cast<int>(ib); A.info_out = info_out_dev; A.dst_out = decode_status_dev; A.fst_out = demod_status_dev;
    return acq_run_rounds(h, "ria_gpu_rx_acquire_batch", samples_dev, A, W, n_windows, flags, s);
}

// ------------------------------------------------------------------------------------------------ frames of any length, control hypothesis
int ria_gpu_var_frame_samples(ria_gpu_handle h, int coded_bytes) {
    if (!h) return RIA_ERR_INVALID;
    if (coded_bytes < 1 || coded_bytes > kVarMaxCodedBytes) return fail(h, RIA_ERR_INVALID, "ria_gpu_var_frame_samples: coded_bytes must be 1..324");
    return var_frame_samples(h->geo.bits_per_symbol, coded_bytes);
}

static bool is_control_handle(ria_gpu_handle h) { return h && h->cfg.modulation == RIA_MOD_DQPSK && h->cfg.code_rate == RIA_RATE_1_4; }

int ria_gpu_control_frame_samples(ria_gpu_handle control_h, ria_gpu_handle data_h) {
    if (!control_h || !data_h) return RIA_ERR_INVALID;
    if (!is_control_handle(control_h) || control_h->cfg.num_carriers != data_h->cfg.num_carriers)
        return fail(control_h, RIA_ERR_INVALID, "ria_gpu_control_frame_samples: the control handle must be DQPSK R1/4 with the data handle's carriers");
    if (is_control_handle(data_h)) return var_frame_samples(control_h->geo.bits_per_symbol, 81);
    return control_frame_samples(data_h->geo.bits_per_symbol, false, data_h->cfg.num_carriers);
}

int ria_gpu_tx_coded_var_batch(ria_gpu_handle h, const uint8_t* coded_dev, int coded_bytes, int n_frames, float peak_normalize,
                               float* samples_out_dev, int64_t out_stride, void* stream) {
    if (!h || n_frames < 0 || coded_bytes < 1 || coded_bytes > kVarMaxCodedBytes)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_tx_coded_var_batch: bad argument (coded_bytes 1..324)");
    const int n_out = var_frame_samples(h->geo.bits_per_symbol, coded_bytes);
    if (out_stride < n_out || out_stride > 0x7fffffff) return fail(h, RIA_ERR_INVALID, "ria_gpu_tx_coded_var_batch: out_stride must hold the frame's %d samples", n_out);
    if (n_frames == 0) return RIA_OK;
    if (!coded_dev || !samples_out_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_tx_coded_var_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    launch_tx_mode<3>(h->d_tx_const.as<const TxConst>(), h->d_twiddle.as<const float2>(), h->d_nco.as<const float2>(), coded_dev,
                      n_frames, peak_normalize, h->geo, samples_out_dev, nullptr, static_cast<hipStream_t>(stream), coded_bytes,
                      static_cast<int>(out_stride));
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// the workspace of the calls below for n rows (spans or windows); llr_row = soft bits of a whole frame
struct ControlWs {
    uint64_t* offsets;            // frame starts of a call without offsets
    float* llr; ria_frame_status* fst;
    ria_lts_result* lts;
    FrameList list;
    AcqCtl* ctl;
};
static ControlWs control_carve(Carver& c, size_t n, size_t llr_row) {
    ControlWs w;
    w.offsets = c.take<uint64_t>(n);
    w.llr = c.take<float>(n * llr_row);
    w.fst = c.take<ria_frame_status>(n);
    w.lts = c.take<ria_lts_result>(n);
    take_frame_list(c, w.list, n);
    w.ctl = c.take<AcqCtl>(1);
    return w;
}
// The reserve step of the span demodulator (demod_var_launch), and the one place that refuses the fused kernel; `who` is
// the public call, for the message.
static int demod_span_reserve(ria_gpu_handle h, const char* who) {
    if (demod_fused_selected()) return fail(h, RIA_ERR_UNSUPPORTED, "%s: RIA_DEMOD_FUSED=1 demodulates fixed frames only", who);
    HIP_TRY(h, h->d_demod_ws[0].reserve(demod_ws_bytes(2 + h->geo.n_data_symbols)));
    return RIA_OK;
}
// The reserve step of the control calls: demod_span_reserve, and the workspace grown to n rows; the caller's stream is
// drained first when the block has to move (an earlier call on it may still read the old one)
static int control_ensure_ws(ria_gpu_handle h, const char* who, int n, hipStream_t s, ControlWs* out) {
    if (int rc = demod_span_reserve(h, who)) return rc;
    const size_t row = static_cast<size_t>(h->geo.llrs_per_frame);
    if (n > h->ctrl_rows) {
        if (h->ctrl_rows) HIP_TRY(h, hipStreamSynchronize(s));
        h->ctrl_rows = 0;
        HIP_TRY(h, h->d_ctrl_ws.reserve(carved_size([&](Carver& c) { return control_carve(c, static_cast<size_t>(n), row); })));
        h->ctrl_rows = n;
    }
    HIP_TRY(h, h->p_ctrl_ctl.reserve(sizeof(AcqCtl)));
    *out = carve_at(h->d_ctrl_ws.as<>(), [&](Carver& c) { return control_carve(c, static_cast<size_t>(h->ctrl_rows), row); });
    return RIA_OK;
}

// spans of n_samples at offsets (never NULL here) through the split pipeline; the caller has run demod_span_reserve
static int demod_var_launch(ria_gpu_handle h, const float* samples_dev, const uint64_t* offsets_dev, const ria_frame_meta* meta_dev,
                            int n_frames, int n_samples, float* llr_out_dev, int llr_stride, ria_frame_status* status_dev, hipStream_t s) {
    const DemodArgs A = demod_args(h, samples_dev, offsets_dev, meta_dev, n_frames, llr_out_dev, llr_stride, status_dev);
    launch_demod<true>(A, h->geo, h->cfg.modulation, h->d_demod_ws[0].as<>(), s, n_samples / kSym);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}
static bool var_span_ok(ria_gpu_handle h, int n_samples) { return n_samples >= 3 * kSym && n_samples <= h->geo.frame_samples; }

int ria_gpu_demod_var_batch(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                            const ria_frame_meta* meta_dev, int n_frames, int n_samples,
                            float* llr_out_dev, int llr_stride, ria_frame_status* status_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_frames < 0 || !var_span_ok(h, n_samples))
        return fail(h, RIA_ERR_INVALID, "ria_gpu_demod_var_batch: bad argument (3 * 1152 <= n_samples <= frame_samples)");
    if (llr_stride < (n_samples / kSym - 2) * h->geo.bits_per_symbol)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_demod_var_batch: llr_stride must hold the span's %d soft bits", (n_samples / kSym - 2) * h->geo.bits_per_symbol);
    if (n_frames == 0) return RIA_OK;
    if (!samples_dev || !llr_out_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_demod_var_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const char* who = "ria_gpu_demod_var_batch";
    if (frame_offsets_dev) {
        if (int rc = demod_span_reserve(h, who)) return rc;
    } else {
        ControlWs W;
        if (int rc = control_ensure_ws(h, who, n_frames, s, &W)) return rc;
        hipLaunchKernelGGL(var_offsets_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, s, W.offsets, n_frames, n_samples);
        frame_offsets_dev = W.offsets;
    }
    return demod_var_launch(h, samples_dev, frame_offsets_dev, meta_dev, n_frames, n_samples, llr_out_dev, llr_stride, status_dev, s);
}

int ria_gpu_demod_var_host(ria_gpu_handle h, const float* samples_host, int n_samples, const ria_frame_meta* meta_host,
                           float* llr_out_host, int max_llr, ria_frame_status* status_out) {
    if (!h) return RIA_ERR_INVALID;
    if (!samples_host || !llr_out_host || max_llr < 0 || !var_span_ok(h, n_samples))
        return fail(h, RIA_ERR_INVALID, "ria_gpu_demod_var_host: bad argument (3 * 1152 <= n_samples <= frame_samples)");
    HIP_TRY(h, hipSetDevice(h->device));
    const int made = (n_samples / kSym - 2) * h->geo.bits_per_symbol;
    struct Stage { float* x; ria_frame_meta* meta; float* llr; ria_frame_status* fs; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.x = c.in(static_cast<size_t>(n_samples), samples_host); w.meta = c.in(1, meta_host);
        w.llr = c.out(static_cast<size_t>(made), llr_out_host, static_cast<size_t>(std::min(made, max_llr))); w.fs = c.out(1, status_out);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        return ria_gpu_demod_var_batch(h, d.x, nullptr, d.meta, 1, n_samples, d.llr, made, d.fs, s); });
}

static_assert(sizeof(ria_control_result) == 32, "ria_control_result is 32 bytes (include/ria_gpu.h)");
static_assert(offsetof(ria_control_result, seq) == 8 && offsetof(ria_control_result, n_llr) == 12 && offsetof(ria_control_result, tried) == 16,
              "ria_control_result layout (ria_amd/engine.py CONTROL_RESULT)");

static void launch_control_decode(ria_gpu_handle h, const ControlArgs& A, hipStream_t s) {
    dispatch_shape(h->cfg.code_rate, [&](auto sh) {
        using S = decltype(sh);
        static bool attr = false;
        if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(control_decode_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize, h->wave_lds); attr = true; }
        hipLaunchKernelGGL(control_decode_kernel<S>, dim3(std::min(A.n_rows, 16384)), dim3(64), h->wave_lds, s, h->fast, A);
    });
}

int ria_gpu_rx_control_batch(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                             const ria_frame_meta* meta_dev, int n_frames, int n_samples,
                             uint8_t* frame_out_dev, ria_control_result* result_dev, ria_frame_status* demod_status_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (!is_control_handle(h)) return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_control_batch: the handle must be DQPSK R1/4");
    if (n_frames < 0 || !var_span_ok(h, n_samples))
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_control_batch: bad argument (3 * 1152 <= n_samples <= frame_samples)");
    if (n_frames == 0) return RIA_OK;
    if (!samples_dev || !frame_out_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_control_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ControlWs W;
    if (int rc = control_ensure_ws(h, "ria_gpu_rx_control_batch", n_frames, s, &W)) return rc;   // before anything is in flight
    if (!frame_offsets_dev) {
        hipLaunchKernelGGL(var_offsets_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, s, W.offsets, n_frames, n_samples);
        frame_offsets_dev = W.offsets;
    }
    if (int rc = demod_var_launch(h, samples_dev, frame_offsets_dev, meta_dev, n_frames, n_samples, W.llr,
                                  h->geo.llrs_per_frame, W.fst, s)) return rc;
    ControlArgs A{};
    A.llr = W.llr; A.llr_stride = h->geo.llrs_per_frame; A.fst = W.fst; A.window = nullptr; A.n_rows = n_frames;
    A.crc_bit = h->d_crc_bit.as<const uint16_t>(); A.crc_init = h->d_crc_init.as<const uint16_t>();
    A.frame_out = frame_out_dev; A.result = result_dev; A.fst_out = demod_status_dev; A.acq = nullptr;
    launch_control_decode(h, A, s);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_control_acquire_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int search_len, int window_len,
                                  int n_windows, int n_samples, const ria_acq_params* params_dev, uint32_t flags,
                                  uint8_t* frame_out_dev, ria_control_result* result_dev, ria_acq_result* acq_dev,
                                  ria_frame_status* demod_status_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (!is_control_handle(h)) return fail(h, RIA_ERR_INVALID, "ria_gpu_control_acquire_batch: the handle must be DQPSK R1/4");
    if (n_windows < 0 || search_len < 0 || window_len < search_len || stride < window_len || (flags & ~RIA_BURST_INTERLEAVE) != 0 || !var_span_ok(h, n_samples))
        return fail(h, RIA_ERR_INVALID, "ria_gpu_control_acquire_batch: bad argument (0 <= search_len <= window_len <= stride; 3 * 1152 <= n_samples <= frame_samples; flags: RIA_BURST_INTERLEAVE only)");
    if (n_windows == 0) return RIA_OK;
    if (!samples_dev || !params_dev || !frame_out_dev || !result_dev || !acq_dev)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_control_acquire_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = static_cast<size_t>(n_windows);
    ControlWs W;
    if (int rc = control_ensure_ws(h, "ria_gpu_control_acquire_batch", n_windows, s, &W)) return rc;   // before anything is in flight
    if (int rc = lts_prepare(h)) return rc;
    HIP_TRY(h, hipMemsetAsync(frame_out_dev, 0, n * kCtlFrameBytes, s));
    HIP_TRY(h, hipMemsetAsync(result_dev, 0, n * sizeof(ria_control_result), s));
    if (demod_status_dev) HIP_TRY(h, hipMemsetAsync(demod_status_dev, 0, n * sizeof(ria_frame_status), s));
    launch_lts_acquire(h, samples_dev, stride, search_len, n_windows, params_dev, W.lts, s);
    ControlArgs A{};
    A.lts = W.lts; A.params = params_dev; A.n_windows = n_windows; A.window_len = window_len; A.n_samples = n_samples;
    A.skip_marked = (flags & RIA_BURST_INTERLEAVE) ? 1 : 0; A.stride = stride; A.acq = acq_dev; A.ctl = W.ctl; A.list = W.list;
    hipLaunchKernelGGL(control_plan_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
    HIP_TRY(h, hipGetLastError());
    if (int rc = read_ctl(h, h->p_ctrl_ctl, W.ctl, s)) return rc;          // the call's one synchronisation
    const int n_list = static_cast<int>(h->p_ctrl_ctl.as<AcqCtl>()->n_list);
    if (n_list == 0) return RIA_OK;
    if (n_list > n_windows) return fail(h, RIA_ERR_HIP, "ria_gpu_control_acquire_batch: work list broke its bound (%d)", n_list);
    if (int rc = demod_var_launch(h, samples_dev, W.list.offset, W.list.meta, n_list, n_samples, W.llr,
                                  h->geo.llrs_per_frame, W.fst, s)) return rc;
    A.llr = W.llr; A.llr_stride = h->geo.llrs_per_frame; A.fst = W.fst; A.window = W.list.window; A.n_rows = n_list;
    A.crc_bit = h->d_crc_bit.as<const uint16_t>(); A.crc_init = h->d_crc_init.as<const uint16_t>();
    A.frame_out = frame_out_dev; A.result = result_dev; A.fst_out = demod_status_dev;
    launch_control_decode(h, A, s);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// ------------------------------------------------------------------------------------------------ burst groups + continuation
static_assert(sizeof(ria_burst_result) == 64, "ria_burst_result is 64 bytes (include/ria_gpu.h)");
static_assert(offsetof(ria_burst_result, cfo_hz) == 20 && offsetof(ria_burst_result, delta) == 24 && offsetof(ria_burst_result, mode) == 28 &&
              offsetof(ria_burst_result, stop) == 31 && offsetof(ria_burst_result, reserved) == 32, "ria_burst_result field offsets");

// the burst workspace for n windows and groups of N frames
struct BurstWs {
    ria_acq_result* acq0; uint8_t* info0; ria_decode_status* dst0; ria_frame_status* fst0; uint32_t* cwin0;
    FrameList list[4];            // group / continuation lists of the round, then their stage lists
    ria_frame_status* gfst; uint32_t* gpos; uint32_t* done;
    BurstCtl* ctl;
    float* gllr; float* dec_in; uint8_t* dec_info; ria_decode_status* dec_dst;
};
static BurstWs burst_carve(Carver& c, size_t n, size_t N, size_t info_bytes, size_t llrs) {
    BurstWs w;
    w.acq0 = c.take<ria_acq_result>(n);
    w.info0 = c.take<uint8_t>(n * info_bytes);
    w.dst0 = c.take<ria_decode_status>(n);
    w.fst0 = c.take<ria_frame_status>(n);
    w.cwin0 = c.take<uint32_t>(n);
    for (FrameList& l : w.list) take_frame_list(c, l, n);
    w.gfst = c.take<ria_frame_status>(n);
    w.gpos = c.take<uint32_t>(n * kBurstMaxGroup);
    w.done = c.take<uint32_t>(n);
    w.ctl = c.take<BurstCtl>(1);
    w.gllr = c.take<float>(n * N * llrs);
    w.dec_in = c.take<float>(n * N * kBurstFrameBits);
    w.dec_info = c.take<uint8_t>(n * N * info_bytes);
    w.dec_dst = c.take<ria_decode_status>(n * N);
    return w;
}

int ria_gpu_rx_burst_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int search_len, int window_len,
                           int n_windows, int group_size, const ria_acq_params* params_dev, uint32_t flags,
                           uint8_t* info_out_dev, ria_decode_status* decode_status_dev, ria_burst_result* burst_dev,
                           ria_frame_status* demod_status_dev, float* cfo_used_dev, float* rms_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    const uint32_t known_flags = RIA_DECODE_FULL | RIA_DECODE_NO_CHANNEL_DEINTERLEAVE | RIA_ACQ_NO_TIMING_RETRY | RIA_BURST_INTERLEAVE | RIA_BURST_NO_CONTINUE;
    if (n_windows < 0 || search_len < 0 || window_len < search_len || stride < window_len || (flags & ~known_flags) != 0 ||
        group_size < 2 || group_size > kBurstMaxGroup)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_burst_batch: bad argument (0 <= search_len <= window_len <= stride; group_size 2..8; flags: RIA_DECODE_*, RIA_ACQ_NO_TIMING_RETRY and RIA_BURST_* only)");
    if (n_windows == 0) return RIA_OK;
    if (!samples_dev || !params_dev || !info_out_dev || !decode_status_dev || !burst_dev)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_burst_batch: null pointer");
    if (static_cast<size_t>(n_windows) * ((flags & RIA_BURST_INTERLEAVE) ? static_cast<size_t>(group_size) : 1) > static_cast<size_t>(INT32_MAX / 8))
        return fail(h, RIA_ERR_INVALID, "ria_gpu_rx_burst_batch: n_windows * group_size too large");   // before anything is sized or allocated
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = lts_prepare(h)) return rc;
    const size_t n = static_cast<size_t>(n_windows), N = static_cast<size_t>(group_size), ib = static_cast<size_t>(h->geo.info_bytes_per_frame);
    const size_t llrs = static_cast<size_t>(h->geo.llrs_per_frame);
    const bool interleave = (flags & RIA_BURST_INTERLEAVE) != 0;
    // every workspace grows here, before anything of this call is in flight (an earlier call has ended on a stream sync)
    AcqWs W;
    if (int rc = acq_ensure_ws(h, n_windows, &W)) return rc;
    auto carve = [&](Carver& c) { return burst_carve(c, n, interleave ? N : 0, ib, llrs); };
    HIP_TRY(h, h->d_burst_ws.reserve(carved_size(carve)));
    HIP_TRY(h, h->p_burst_ctl.reserve(sizeof(BurstCtl)));
    const BurstWs B = carve_at(h->d_burst_ws.as<>(), carve);
    if (hipError_t e = decode_reserve(h, static_cast<int>(n * (interleave ? N : 1)), flags))
        return fail(h, RIA_ERR_HIP, "burst workspace: %s", hipGetErrorString(e));
    HIP_TRY(h, hipMemsetAsync(info_out_dev, 0, n * kBurstSlots * ib, s));
    HIP_TRY(h, hipMemsetAsync(decode_status_dev, 0, n * kBurstSlots * sizeof(ria_decode_status), s));
    if (demod_status_dev) HIP_TRY(h, hipMemsetAsync(demod_status_dev, 0, n * kBurstSlots * sizeof(ria_frame_status), s));
    if (cfo_used_dev) HIP_TRY(h, hipMemsetAsync(cfo_used_dev, 0, n * kBurstSlots * sizeof(float), s));
    if (rms_dev) HIP_TRY(h, hipMemsetAsync(rms_dev, 0, n * kBurstSlots * sizeof(float), s));
    HIP_TRY(h, hipMemsetAsync(B.info0, 0, span_bytes(B.info0, B.cwin0), s));   // frame-0 bytes, decode and demod status rows

    // 1. LTS detection with each window's threshold and known CFO
    launch_lts_acquire(h, samples_dev, stride, search_len, n_windows, params_dev, W.lts, s);
    // 2. acceptance, modes and the two round-0 lists
    BurstArgs A{};
    A.samples = samples_dev; A.stride = stride; A.n_windows = n_windows; A.window_len = window_len;
    A.frame_samples = h->geo.frame_samples; A.group_size = group_size; A.flags = flags;
    A.lts = W.lts; A.params = params_dev; A.res = burst_dev;
    A.ctl = B.ctl;
    A.acq_ctl = W.ctl;
    A.acq_first = W.list[0];
    A.acq0 = B.acq0;
    A.info0 = B.info0; A.dst0 = B.dst0; A.fst0 = B.fst0;
    A.c_win0 = B.cwin0;
    A.g_cur = B.list[0]; A.c_cur = B.list[1];
    A.g_stage = B.list[2]; A.c_stage = B.list[3];
    A.g_fst = B.gfst;
    A.info_bytes = static_cast<int>(ib);
    A.info_out = info_out_dev; A.dst_out = decode_status_dev; A.fst_out = demod_status_dev; A.cfo_used = cfo_used_dev; A.rms = rms_dev;
    A.gpos = B.gpos; A.done = B.done;
    A.gllr = B.gllr; A.llr_stride = static_cast<int>(llrs);
    A.dec_in = B.dec_in; A.dec_info = B.dec_info;
    A.dec_dst = B.dec_dst;
    hipLaunchKernelGGL(burst_plan_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
    HIP_TRY(h, hipGetLastError());
    const uint32_t dflags = flags & (RIA_DECODE_FULL | RIA_DECODE_NO_CHANNEL_DEINTERLEAVE);
    const BurstCtl& ctl = *h->p_burst_ctl.as<BurstCtl>();
    auto read_burst_ctl = [&]() { return read_ctl(h, h->p_burst_ctl, A.ctl, s, "ria_gpu_rx_burst_batch: decode work-queue fault: no window of this call was decoded"); };
    // demodulates the group list's frames as physical frame f: row i of the list writes soft-bit row i * N + f
    auto demod_groups = [&](int n_g, int f) -> int {
        return demod_batch_slot(h, samples_dev, A.g_cur.offset, A.g_cur.meta, n_g, B.gllr + static_cast<size_t>(f) * llrs, B.gfst, s, 0,
                                static_cast<int>(N * llrs));
    };
    if (int rc = read_burst_ctl()) return rc;
    int n_g = static_cast<int>(ctl.n_group), n_c = static_cast<int>(ctl.n_cont);
    if (n_g + n_c > n_windows || (n_g && !interleave)) return fail(h, RIA_ERR_HIP, "ria_gpu_rx_burst_batch: round-0 lists broke their bound (%d, %d)", n_g, n_c);
    // 3. frame 0: the groups' first frames are demodulated, the other windows go through ria_gpu_rx_acquire_batch's rounds
    if (n_g) { if (int rc = demod_groups(n_g, 0)) return rc; }
    if (n_c) {
        AcqArgs Q{};
        Q.lts = W.lts; Q.params = params_dev; Q.n_windows = n_windows; Q.window_len = window_len;
        Q.frame_samples = h->geo.frame_samples; Q.stride = stride; Q.acq = A.acq0; Q.ctl = A.acq_ctl;
        Q.info_bytes = static_cast<int>(ib); Q.info_out = B.info0; Q.dst_out = B.dst0; Q.fst_out = B.fst0;
        if (int rc = acq_run_rounds(h, "ria_gpu_rx_burst_batch", samples_dev, Q, W, n_windows, flags, s)) return rc;
    }
    // 4. rounds: round f runs physical frame f of the windows still live; a group needs rounds 1 .. group_size - 1, a
    // continuation at most rounds 1 .. 8, and the step after the last of them lists nothing
    int n_done = 0;
    for (int round = 1; n_g + n_c > 0; ++round) {
        if (round > kBurstSlots) return fail(h, RIA_ERR_HIP, "ria_gpu_rx_burst_batch: round %d is past the bound (%d, %d)", round, n_g, n_c);
        A.n_g = n_g; A.n_c = n_c; A.round = round; A.first = round == 1;
        if (round == 1) { A.c_fst = A.fst0; A.c_dst = A.dst0; A.c_info = A.info0; }
        else { A.c_fst = W.fst; A.c_dst = W.dst; A.c_info = W.info; }
        hipLaunchKernelGGL(burst_step_kernel, dim3((n_g + n_c + kBurstStepWaves - 1) / kBurstStepWaves), dim3(64 * kBurstStepWaves), 0, s, A);
        hipLaunchKernelGGL(burst_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
        HIP_TRY(h, hipGetLastError());
        if (int rc = read_burst_ctl()) return rc;
        const int ng2 = static_cast<int>(ctl.n_group), nc2 = static_cast<int>(ctl.n_cont);
        n_done = static_cast<int>(ctl.n_done);
        if (ng2 > n_g || nc2 > n_c || n_done > n_windows || (ng2 && round >= group_size))
            return fail(h, RIA_ERR_HIP, "ria_gpu_rx_burst_batch: lists of round %d broke their bound (%d, %d, %d)", round, ng2, nc2, n_done);
        n_g = ng2; n_c = nc2;
        if (n_g) { if (int rc = demod_groups(n_g, round)) return rc; }
        if (n_c) {
            int rc = ria_gpu_rx_batch(h, samples_dev, A.c_cur.offset, A.c_cur.meta, n_c, dflags, W.info, W.dst, nullptr, W.fst, s);
            if (rc != RIA_OK) return rc;
        }
    }
    // 5. complete groups: de-interleave into one decode batch, decodeFixedFrame on every logical frame, scatter
    if (n_done) {
        A.n_done = n_done;
        const long long items = static_cast<long long>(n_done) * group_size * 324;
        hipLaunchKernelGGL(burst_gather_kernel, dim3(static_cast<unsigned>(std::min<long long>((items + 255) / 256, 16384))), dim3(256), 0, s, A);
        int rc = launch_decode(h, A.dec_in, kBurstFrameBits, n_done * group_size, dflags, B.dec_info, B.dec_dst, s);
        if (rc != RIA_OK) return rc;
        hipLaunchKernelGGL(burst_scatter_kernel, dim3(std::min((n_done * group_size + 3) / 4, 4096)), dim3(256), 0, s, A);
        HIP_TRY(h, hipGetLastError());
        if (int rc2 = read_burst_ctl()) return rc2;
    }
    return RIA_OK;
}

int ria_gpu_sync_host(ria_gpu_handle h, int kind, const float* samples_host, int n_samples, float threshold, float param,
                      uint32_t root_mask, void* result_out) {
    if (!h || !samples_host || !result_out || n_samples < 0 || kind < 0 || kind > 3) return RIA_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->d_sync_host.reserve(static_cast<size_t>(n_samples) * sizeof(float) + 64));   // no drain: every call ends on a device sync
    unsigned char* base = h->d_sync_host.as<unsigned char>();
    float* d_param = reinterpret_cast<float*>(base);
    void* d_res = base + 16;
    float* d_x = reinterpret_cast<float*>(base + 64);
    HIP_TRY(h, hipMemcpy(d_x, samples_host, static_cast<size_t>(n_samples) * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_param, &param, sizeof(float), hipMemcpyHostToDevice));
    int rc;
    if (kind == 0) rc = ria_gpu_sync_chirp_batch(h, d_x, n_samples, n_samples, 1, threshold, static_cast<ria_chirp_result*>(d_res), nullptr);
    else if (kind == 1) rc = ria_gpu_sync_lts_batch(h, d_x, n_samples, n_samples, 1, d_param, threshold, static_cast<ria_lts_result*>(d_res), nullptr);
    else if (kind == 3) rc = ria_gpu_sync_cox_batch(h, d_x, n_samples, n_samples, 1, threshold, d_param, static_cast<ria_cox_result*>(d_res), nullptr);
    else rc = ria_gpu_sync_zc_batch(h, d_x, n_samples, n_samples, 1, threshold, root_mask, d_param, static_cast<ria_zc_result*>(d_res), nullptr);
    if (rc != RIA_OK) return rc;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(result_out, d_res, 32, hipMemcpyDeviceToHost));
    return RIA_OK;
}

static bool mcdpsk_config_ok(const ria_mcdpsk_config* c) {
    return c && c->num_carriers >= 1 && c->num_carriers <= kMcMaxCarriers && (c->bits_per_symbol == 1 || c->bits_per_symbol == 2) &&
           (c->spreading == 1 || c->spreading == 2 || c->spreading == 4);
}

// the tables the demodulator's kernels hand to each other for a chunk of F frames: the CFO-corrected samples and phases
// (with a CFO array only), the symbol sums of sym_items = symbols x carriers, the three arrays of data_items = data symbols
// x carriers, the carriers' relative gains and the frame's scale
struct McWs { float* xc; float2* Yg; float *cph, *cmag, *pe2, *rel, *scale; };
static McWs mc_carve(Carver& c, size_t F, size_t frame_samples, size_t sym_items, size_t data_items, bool with_cfo) {
    McWs w;
    w.xc = c.take<float>(with_cfo ? F * 2 * frame_samples : 0);
    w.Yg = c.take<float2>(sym_items * F);
    for (float** a : {&w.cph, &w.cmag, &w.pe2}) *a = c.take<float>(data_items * F);
    w.rel = c.take<float>(static_cast<size_t>(kMcMaxCarriers) * F);
    w.scale = c.take<float>(F);
    return w;
}

// offsets_dev / bps_dev (nullable): the offset-list form (McArgs::offset, bps_list) of ria_gpu_mcdpsk_acquire_batch, whose
// caller has checked the arguments (llr_stride for two bits per symbol)
static int mcdpsk_demod_impl(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                             const uint64_t* offsets_dev, const uint8_t* bps_dev,
                             int frame_samples, int n_frames, const float* cfo_hz_dev, const float* phase0_dev,
                             float* llr_out_dev, int llr_stride, ria_mcdpsk_status* status_dev, void* stream) {
    const int nc = cfg->num_carriers, num_rx = (frame_samples - (kMcTrain + 1) * kMcSps) / kMcSps;
    const int nds = std::max(1, num_rx / cfg->spreading);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf& mixer = h->d_mc_mixer[nc];
    if (!mixer) HIP_TRY(h, upload(mixer, build_mcdpsk_mixer(nc)));
    if (!h->d_mc_hilbert) HIP_TRY(h, upload(h->d_mc_hilbert, build_hilbert127()));
    const int lds = mcdpsk_lds_bytes(nc, frame_samples);
    if (lds > 160 * 1024) return fail(h, RIA_ERR_UNSUPPORTED, "ria_gpu_mcdpsk_demod_batch: frame too long for one workgroup's LDS");
    if (lds > h->mc_lds_opted) {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(mcdpsk_corr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        h->mc_lds_opted = lds;
    }
    // the tables handed from kernel to kernel (and the CFO-corrected samples when a CFO array is given) live in a per-handle
    // workspace; a batch is walked in chunks of frames that fit it
    const size_t n_sym = static_cast<size_t>(3 + num_rx);
    auto carve = [&](size_t F) {
        return [=](Carver& c) { return mc_carve(c, F, static_cast<size_t>(frame_samples), n_sym * nc, static_cast<size_t>(nds) * nc, cfo_hz_dev != nullptr); };
    };
    const int chunk = static_cast<int>(std::min<size_t>(static_cast<size_t>(n_frames), std::max<size_t>(1, (size_t(256) << 20) / carved_size(carve(1)))));
    HIP_TRY(h, h->d_mc_ws.reserve(carved_size(carve(static_cast<size_t>(chunk))), &s));   // a growth waits for the stream's earlier users of the old block
    McArgs A{};
    A.samples = samples_dev; A.stride = stride; A.frame_samples = frame_samples; A.nc = nc; A.bps = cfg->bits_per_symbol;
    A.spreading = cfg->spreading; A.cfo = cfo_hz_dev; A.phase0 = phase0_dev; A.mixer = mixer.as<const float2>();
    A.hilbert = h->d_mc_hilbert.as<const float>(); A.llr = llr_out_dev;
    A.llr_stride = llr_stride; A.status = status_dev; A.chunk = mcdpsk_corr_chunk(nc, frame_samples);
    A.offset = offsets_dev; A.bps_list = bps_dev;
    for (int first = 0; first < n_frames; first += chunk) {
        A.first = first; A.n_frames = std::min(chunk, n_frames - first);
        const size_t F = static_cast<size_t>(A.n_frames);
        const McWs W = carve_at(h->d_mc_ws.as<>(), carve(F));   // the arrays are indexed [item][frame of the chunk]
        A.ws = W.xc; A.Yg = W.Yg; A.cph = W.cph; A.cmag = W.cmag; A.pe2 = W.pe2; A.rel = W.rel; A.scale = W.scale;
        hipLaunchKernelGGL(mcdpsk_corr_kernel, dim3(A.n_frames), dim3(256), lds, s, A);
        hipLaunchKernelGGL(mcdpsk_chain_kernel, dim3(static_cast<unsigned>((F * nc + 255) / 256)), dim3(256), 0, s, A);
        hipLaunchKernelGGL(mcdpsk_stats_kernel, dim3(static_cast<unsigned>((F + 63) / 64)), dim3(64), 0, s, A);
        hipLaunchKernelGGL(mcdpsk_llr_kernel, dim3(static_cast<unsigned>((F * nds * nc + 255) / 256)), dim3(256), 0, s, A);
    }
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_mcdpsk_demod_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                               int frame_samples, int n_frames, const float* cfo_hz_dev, const float* phase0_dev,
                               float* llr_out_dev, int llr_stride, ria_mcdpsk_status* status_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_frames == 0) return RIA_OK;
    if (!mcdpsk_config_ok(cfg) || !samples_dev || !llr_out_dev || !status_dev || n_frames < 0 || stride < frame_samples ||
        frame_samples < (kMcTrain + 2) * kMcSps)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_demod_batch: bad arguments");
    const int nc = cfg->num_carriers, num_rx = (frame_samples - (kMcTrain + 1) * kMcSps) / kMcSps;
    const int nds = std::max(1, num_rx / cfg->spreading);
    if (llr_stride < nds * nc * cfg->bits_per_symbol) return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_demod_batch: llr_stride too small");
    return mcdpsk_demod_impl(h, cfg, samples_dev, stride, nullptr, nullptr, frame_samples, n_frames, cfo_hz_dev, phase0_dev,
                             llr_out_dev, llr_stride, status_dev, stream);
}

// Host-buffer forms for the single-frame MC-DPSK plug-in adaptor (GpuMcDpskWaveform): staged through the handle's pinned +
// device block on the handle's own stream, like ria_gpu_rx_frames_host.
int ria_gpu_mcdpsk_demod_host(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_host, int n_samples, float cfo_hz,
                              float phase0, float* llr_out_host, int max_llr, ria_mcdpsk_status* status_out) {
    if (!h || !mcdpsk_config_ok(cfg) || !samples_host || !llr_out_host || !status_out || n_samples < (kMcTrain + 2) * kMcSps)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_demod_host: bad arguments");
    const int num_rx = (n_samples - (kMcTrain + 1) * kMcSps) / kMcSps;
    const int n_llr = std::max(1, num_rx / cfg->spreading) * cfg->num_carriers * cfg->bits_per_symbol;
    if (max_llr < n_llr) return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_demod_host: llr buffer too small (%d needed)", n_llr);
    HIP_TRY(h, hipSetDevice(h->device));
    const float par[2] = {cfo_hz, phase0};
    struct Stage { float *x, *par, *llr; ria_mcdpsk_status* st; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.x = c.in(static_cast<size_t>(n_samples), samples_host); w.par = c.in(2, par);
        w.llr = c.out(static_cast<size_t>(n_llr), llr_out_host); w.st = c.out(1, status_out);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        return ria_gpu_mcdpsk_demod_batch(h, cfg, d.x, n_samples, n_samples, 1, d.par, d.par + 1, d.llr, n_llr, d.st, s); });
}

int ria_gpu_ldpc_decode_robust_host(ria_gpu_handle h, const float* llr_host, int n_cw, uint8_t* out_host, uint8_t* ok_host,
                                    uint16_t* iters_host, uint8_t* tries_host) {
    if (!h || !llr_host || !out_host || !ok_host || n_cw <= 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_ldpc_decode_robust_host: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = static_cast<size_t>(n_cw), nb = static_cast<size_t>((h->code.k + 7) / 8);
    struct Stage { float* llr; uint8_t *out, *ok; uint16_t* it; uint8_t* tries; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.llr = c.in(n * 648, llr_host);
        w.out = c.out(n * nb, out_host); w.ok = c.out(n, ok_host); w.it = c.out(n, iters_host); w.tries = c.out(n, tries_host);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        return ria_gpu_ldpc_decode_robust_batch(h, d.llr, n_cw, d.out, d.ok, d.it, d.tries, s); });
}

int ria_gpu_mcdpsk_modulate_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const uint8_t* data_dev, int n_bytes, int n_frames,
                                  float* out_dev, int64_t out_stride, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_frames == 0) return RIA_OK;
    if (!mcdpsk_config_ok(cfg) || !data_dev || !out_dev || n_bytes < 0 || n_frames < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_modulate_batch: bad arguments");
    const int nc = cfg->num_carriers, bits_per_sym = nc * cfg->bits_per_symbol;
    const int n_data_sym = (n_bytes * 8 + bits_per_sym - 1) / bits_per_sym;
    const int64_t frame_samples = static_cast<int64_t>(kMcTrain + 1 + n_data_sym * cfg->spreading) * kMcSps;
    if (out_stride < frame_samples) return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_modulate_batch: out_stride too small (%lld samples per frame)", static_cast<long long>(frame_samples));
    const int lds = n_data_sym * nc * static_cast<int>(sizeof(float2)) + 16;
    if (lds > 64 * 1024) return fail(h, RIA_ERR_UNSUPPORTED, "ria_gpu_mcdpsk_modulate_batch: too many data symbols for one workgroup");
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf &carrier = h->d_mc_carrier[nc], &train = h->d_mc_train[nc];
    if (!carrier || !train) {
        std::vector<float> car, tr;
        build_mcdpsk_mod_tables(nc, car, tr);
        HIP_TRY(h, upload(carrier, car));
        HIP_TRY(h, upload(train, tr));
    }
    McModArgs A{};
    A.data = data_dev; A.n_bytes = n_bytes; A.n_frames = n_frames; A.nc = nc; A.bps = cfg->bits_per_symbol; A.spreading = cfg->spreading;
    A.n_data_sym = n_data_sym; A.carrier = carrier.as<const float2>(); A.train = train.as<const float2>();
    A.out = out_dev; A.stride = out_stride;
    hipLaunchKernelGGL(mcdpsk_modulate_kernel, dim3(n_frames), dim3(256), lds, static_cast<hipStream_t>(stream), A);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_mcdpsk_modulate_host(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const uint8_t* data, int n_bytes,
                                 float* out_host, int max_n) {
    if (!h || !mcdpsk_config_ok(cfg) || !data || !out_host || n_bytes < 0) return RIA_ERR_INVALID;
    std::vector<float> f = build_mcdpsk_frame(cfg->num_carriers, cfg->bits_per_symbol, cfg->spreading, data, n_bytes);
    if (static_cast<int>(f.size()) > max_n) return -static_cast<int>(f.size());
    std::memcpy(out_host, f.data(), f.size() * sizeof(float));
    return static_cast<int>(f.size());
}

// ------------------------------------------------------------------------------------------------ MC-DPSK acquire + decode
static_assert(sizeof(ria_mcdpsk_acq_params) == 32, "ria_mcdpsk_acq_params is 32 bytes (include/ria_gpu.h)");
static_assert(sizeof(ria_mcdpsk_acq_result) == 64, "ria_mcdpsk_acq_result is 64 bytes (include/ria_gpu.h)");
static_assert(offsetof(ria_mcdpsk_acq_params, abs_base) == 16 && offsetof(ria_mcdpsk_acq_result, delta) == 28 &&
              offsetof(ria_mcdpsk_acq_result, header_total_cw) == 36, "ria_mcdpsk_acq_* field offsets");
static_assert(sizeof(ria_chirp_result) == 32 && sizeof(ria_zc_result) == 32, "one detector area serves either detector");
// the MC-DPSK acquisition workspace for n windows, llr_ws soft bits and max_cw codewords per candidate
struct MacqWs {
    uint8_t* det;                 // [n] ria_chirp_result or ria_zc_result
    MacqList list[2];
    ria_mcdpsk_status* mst; float* llr; float* rows; uint32_t* row_entry; uint8_t* row_cw;
    uint8_t *out_a, *ok_a; uint16_t* it_a;   // round A: n rows
    uint8_t *out_b, *ok_b; uint16_t* it_b;   // round B: n * (max_cw - 1) rows
    int *hdr, *need; uint32_t* base; uint8_t* done;
    MacqCtl* ctl;
    uint8_t* ci_flag; uint32_t* ci_list; uint8_t *out_a2, *ok_a2; uint16_t* it_a2;   // round A2: n rows with channel interleaving, else none
    MacqCiCtl* ci_ctl;
};
static MacqWs macq_carve(Carver& c, size_t n, size_t llr_ws, size_t max_cw, size_t dec_bytes, bool ci) {
    const size_t nr = n * max_cw;   // rows of round A (n) and round B (n * (max_cw - 1))
    MacqWs w;
    w.det = c.take<uint8_t>(n * 32);
    for (MacqList& l : w.list) c.take_list(n, l.offset, l.cfo, l.window, l.cand, l.bps);   // the five arrays of one list, widest first
    w.mst = c.take<ria_mcdpsk_status>(n);
    w.llr = c.take<float>(n * llr_ws);
    w.rows = c.take<float>(nr * kMacqLdpcBlock);
    w.row_entry = c.take<uint32_t>(nr);
    w.row_cw = c.take<uint8_t>(nr);
    w.out_a = c.take<uint8_t>(n * dec_bytes);
    w.ok_a = c.take<uint8_t>(n);
    w.it_a = c.take<uint16_t>(n);
    w.out_b = c.take<uint8_t>(nr * dec_bytes);
    w.ok_b = c.take<uint8_t>(nr);
    w.it_b = c.take<uint16_t>(nr);
    w.hdr = c.take<int>(n);
    w.need = c.take<int>(n);
    w.base = c.take<uint32_t>(n);
    w.done = c.take<uint8_t>(n);
    w.ctl = c.take<MacqCtl>(1);
    const size_t n2 = ci ? n : 0;
    w.ci_flag = c.take<uint8_t>(n2);
    w.ci_list = c.take<uint32_t>(n2);
    w.out_a2 = c.take<uint8_t>(n2 * dec_bytes);
    w.ok_a2 = c.take<uint8_t>(n2);
    w.it_a2 = c.take<uint16_t>(n2);
    w.ci_ctl = c.take<MacqCiCtl>(ci ? 1 : 0);
    return w;
}
// ChannelInterleaver(interleaver_bits, 648)'s step (coprime with 648: 647 is prime, so the first search always ends)
static bool macq_ci_step(int interleaver_bits, int* step) {
    if (interleaver_bits < 1 || interleaver_bits > kMacqLdpcBlock) return false;
    *step = channel_interleaver_step(interleaver_bits, kMacqLdpcBlock);
    return true;
}
// Round A2 of a round whose round A has run (mcdpsk_acquire_kernels.hip.h), shared by the acquire and the decode-frame
// call: the A2 list, one control read for its length, the de-interleaved CW0 decodes and the merge into round A's outputs.
static int macq_round_a2(ria_gpu_handle h, const char* who, const MacqArgs& A, const MacqWs& W, PinBuf& mirror, hipStream_t s,
                         uint8_t* tries_a2 = nullptr /* [n_cur], the window call's peek */) {
    hipLaunchKernelGGL(macq_ci_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
    HIP_TRY(h, hipGetLastError());
    if (int rc = read_ctl(h, mirror, A.ci_ctl, s)) return rc;     // the mirror's other words are read again before they are used
    const int n_a2 = static_cast<int>(mirror.as<MacqCiCtl>()->n_a2);
    if (n_a2 < 0 || n_a2 > A.n_cur) return fail(h, RIA_ERR_HIP, "%s: the list of de-interleaved CW0 decodes broke its bound (%d)", who, n_a2);
    if (n_a2 == 0) return RIA_OK;
    hipLaunchKernelGGL(macq_ci_gather_kernel, dim3(static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(n_a2) * kMacqLdpcBlock + 255) / 256, 16384))),
                       dim3(256), 0, s, A, n_a2);
    int rc = ria_gpu_ldpc_decode_robust_batch(h, A.rows, n_a2, W.out_a2, W.ok_a2, W.it_a2, tries_a2, s);
    if (rc != RIA_OK) return rc;
    hipLaunchKernelGGL(macq_ci_merge_kernel, dim3(static_cast<unsigned>(std::min((n_a2 + 255) / 256, 1024))), dim3(256), 0, s, A, n_a2,
                       W.out_a, W.ok_a, W.out_a2, W.ok_a2);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// ---- the chase stages of decodeMCDPSKFrame (mcdpsk_harq_kernels.hip.h), shared by the two HARQ calls
struct HarqWs {
    ria_mcdpsk_harq_result* harq;                                   // [n] when the caller passes none
    uint8_t* sum_flag; uint32_t* sum_src; int32_t* sum_pos; uint32_t* sum_list;   // [rows]
    uint8_t *out_c, *ok_c; uint16_t* it_c;                          // [rows] the decodes of the sums
};
static HarqWs harq_carve(Carver& c, size_t n, size_t rows, size_t dec_bytes) {
    HarqWs w;
    w.harq = c.take<ria_mcdpsk_harq_result>(n);
    w.sum_flag = c.take<uint8_t>(rows);
    w.sum_src = c.take<uint32_t>(rows);
    w.sum_pos = c.take<int32_t>(rows);
    w.sum_list = c.take<uint32_t>(rows);
    w.out_c = c.take<uint8_t>(rows * dec_bytes);
    w.ok_c = c.take<uint8_t>(rows);
    w.it_c = c.take<uint16_t>(rows);
    return w;
}
static bool chase_pool_alive(ria_gpu_handle h, ria_chase_pool pool) {
    for (const auto& p : h->chase_pools) if (p.get() == pool) return true;
    return false;
}
// Allocates the stages' arrays (before anything of the call is in flight), clears the owner words and the control block's
// flags and claims every window's cache.  The caller reads ctl.dup with its first control read.
static int harq_begin(ria_gpu_handle h, const char* who, ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                      ria_mcdpsk_harq_result* harq_dev, int n, size_t rows, size_t dec_bytes, MacqCtl* ctl_dev, hipStream_t s,
                      HarqArgs* H, HarqWs* HW) {
    if (!chase_pool_alive(h, pool)) return fail(h, RIA_ERR_INVALID, "%s: the pool does not belong to this handle", who);
    if (!cache_id_dev || !now_ms_dev) return fail(h, RIA_ERR_INVALID, "%s: a pool needs cache_id_dev and now_ms_dev", who);
    auto carve = [&](Carver& c) { return harq_carve(c, static_cast<size_t>(n), rows, dec_bytes); };
    HIP_TRY(h, h->d_harq_ws.reserve(carved_size(carve), &s));
    *HW = carve_at(h->d_harq_ws.as<>(), carve);
    H->caches = pool->d_meta.as<ChaseCache>();
    H->sums = pool->d_sums.as<float>();
    H->owner = pool->d_owner.as<int32_t>();
    H->n_caches = pool->cfg.n_caches;
    H->cfg.max_entries = pool->cfg.max_entries;
    H->cfg.ttl_ms = pool->cfg.ttl_ms;
    H->cache_id = cache_id_dev; H->now_ms = now_ms_dev;
    H->harq = harq_dev ? harq_dev : HW->harq;
    H->sum_flag = HW->sum_flag; H->sum_src = HW->sum_src; H->sum_pos = HW->sum_pos; H->sum_list = HW->sum_list;
    H->out_c = HW->out_c; H->ok_c = HW->ok_c;
    HIP_TRY(h, hipMemsetAsync(H->owner, 0xFF, static_cast<size_t>(pool->cfg.n_caches) * sizeof(int32_t), s));
    HIP_TRY(h, hipMemsetAsync(ctl_dev, 0, sizeof(MacqCtl), s));
    hipLaunchKernelGGL(harq_claim_kernel, dim3(static_cast<unsigned>(std::min((n + 255) / 256, 1024))), dim3(256), 0, s, *H, n, ctl_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}
// Stages 4-6 of a round with n_rows round-B rows, between round B's decode and the finish.  One control read (the length
// of the list of sums) when the round has rows.
static int harq_stages(ria_gpu_handle h, const char* who, const MacqArgs& A, HarqArgs H, const HarqWs& HW, PinBuf& mirror, int n_rows,
                       unsigned waves, hipStream_t s) {
    H.out_b = const_cast<uint8_t*>(A.out_b); H.ok_b = const_cast<uint8_t*>(A.ok_b);
    hipLaunchKernelGGL(harq_store_kernel, dim3(waves), dim3(256), 0, s, A, H);
    int n_sums = 0;
    if (n_rows > 0) {
        hipLaunchKernelGGL(harq_sum_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, H, n_rows, A.ctl);
        HIP_TRY(h, hipGetLastError());
        if (int rc = read_ctl(h, mirror, A.ctl, s)) return rc;
        n_sums = static_cast<int>(mirror.as<MacqCtl>()->n_sums);
        if (n_sums < 0 || n_sums > n_rows) return fail(h, RIA_ERR_HIP, "%s: the list of sums broke its bound (%d)", who, n_sums);
    }
    if (n_sums > 0) {
        hipLaunchKernelGGL(harq_sum_gather_kernel, dim3(static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(n_sums) * kMacqLdpcBlock + 255) / 256, 16384))),
                           dim3(256), 0, s, H, A.rows, n_sums, A.row_entry, A.ci_flag, A.ci_step);
        int rc = ria_gpu_ldpc_decode_robust_batch(h, A.rows, n_sums, HW.out_c, HW.ok_c, HW.it_c, nullptr, s);
        if (rc != RIA_OK) return rc;
    }
    hipLaunchKernelGGL(harq_resolve_kernel, dim3(waves), dim3(256), 0, s, A, H, n_sums > 0 ? 1 : 0);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// ---- one MC-DPSK round (mcdpsk_acquire_kernels.hip.h), shared by the acquire, the window and the decode-frame calls
// the part of a round's arguments that only names workspace areas and per-handle tables
static void macq_bind(MacqArgs& A, const MacqWs& W, ria_gpu_handle h, bool ci, int ci_step) {
    A.ctl = W.ctl; A.mst = W.mst;
    A.rows = W.rows; A.row_entry = W.row_entry; A.row_cw = W.row_cw;
    A.out_a = W.out_a; A.ok_a = W.ok_a; A.out_b = W.out_b; A.ok_b = W.ok_b;
    A.dec_bytes = (h->geo.ldpc_k + 7) / 8;
    A.hdr_total = W.hdr; A.need_rows = W.need; A.row_base = W.base; A.done = W.done;
    A.crc_bit = h->d_crc_bit.as<const uint16_t>(); A.crc_init = h->d_crc_init.as<const uint16_t>();
    if (ci) { A.ci_step = ci_step; A.ci_flag = W.ci_flag; A.ci_list = W.ci_list; A.ci_ctl = W.ci_ctl; }
}
static unsigned macq_gather_grid(int n_rows) { return static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(n_rows) * kMacqLdpcBlock + 255) / 256, 16384)); }
// Round A on the A.n_cur entries of A.cur, their soft bits in A.llr: CW0 of every entry gathered and decoded, then with
// `ci` the de-interleaved retry (one control read into `mirror`).  tries / tries_a2, where given, take the decoders' tries.
static int macq_round_cw0(ria_gpu_handle h, const char* who, const MacqArgs& A, const MacqWs& W, bool ci, PinBuf& mirror, hipStream_t s,
                          uint8_t* tries = nullptr, uint8_t* tries_a2 = nullptr) {
    MacqArgs G = A;
    G.row_entry = nullptr;
    hipLaunchKernelGGL(macq_gather_kernel, dim3(macq_gather_grid(A.n_cur)), dim3(256), 0, s, G, A.n_cur);
    if (int rc = ria_gpu_ldpc_decode_robust_batch(h, A.rows, A.n_cur, W.out_a, W.ok_a, W.it_a, tries, s)) return rc;
    return ci ? macq_round_a2(h, who, A, W, mirror, s, tries_a2) : RIA_OK;
}
// The rest of the round: the headers and the round-B row list (one control read into `mirror`; with dup_noun the read is
// also where a pool's ctl.dup is tested, and the word names the entries in the message), CW1..total_cw-1 of the entries
// whose header asks for them, the chase stages with a pool, the finish.  max_cw bounds the codewords of an entry.
static int macq_round_rest(ria_gpu_handle h, const char* who, const MacqArgs& A, const MacqWs& W, ria_chase_pool pool, const HarqArgs& H,
                           const HarqWs& HW, PinBuf& mirror, int max_cw, const char* dup_noun, hipStream_t s) {
    const unsigned waves = static_cast<unsigned>(std::min((A.n_cur + 3) / 4, 4096));
    hipLaunchKernelGGL(macq_header_kernel, dim3(waves), dim3(256), 0, s, A);
    hipLaunchKernelGGL(macq_rows_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
    HIP_TRY(h, hipGetLastError());
    if (int rc = read_ctl(h, mirror, A.ctl, s)) return rc;
    const MacqCtl& ctl = *mirror.as<MacqCtl>();
    if (pool && dup_noun && ctl.dup)
        return fail(h, RIA_ERR_INVALID, "%s: two %s of one call use one cache id, or an id is not below n_caches; no cache was touched", who, dup_noun);
    const int n_rows = static_cast<int>(ctl.n_rows);
    if (n_rows < 0 || n_rows > static_cast<long long>(A.n_cur) * (max_cw - 1))
        return fail(h, RIA_ERR_HIP, "%s: the codeword rows of a round broke their bound (%d)", who, n_rows);
    if (n_rows > 0) {
        hipLaunchKernelGGL(macq_gather_kernel, dim3(macq_gather_grid(n_rows)), dim3(256), 0, s, A, n_rows);
        if (int rc = ria_gpu_ldpc_decode_robust_batch(h, A.rows, n_rows, W.out_b, W.ok_b, W.it_b, nullptr, s)) return rc;
    }
    if (pool) { if (int rc = harq_stages(h, who, A, H, HW, mirror, n_rows, waves, s)) return rc; }
    hipLaunchKernelGGL(macq_finish_kernel, dim3(waves), dim3(256), 0, s, A);
    return RIA_OK;
}

// The rounds of one list (steps 3-5): round 0 runs W.list[0] (its length in ctl.n_list) at the primary candidate, round r >= 1
// the windows still searching at their next candidate that fits (at most 25 more rounds: each advances every window it holds by
// at least one candidate).  A carries everything but the per-round fields; llr_ws and max_cw belong to A.frame_len.
static int macq_rounds(ria_gpu_handle h, const char* who, const ria_mcdpsk_config& c, const float* samples_dev, int64_t stride, MacqArgs& A,
                       const MacqWs& W, ria_chase_pool pool, const HarqArgs& H, const HarqWs& HW, bool ci, int llr_ws, int max_cw,
                       bool check_dup, hipStream_t s) {
    const MacqCtl& ctl = *h->p_macq_ctl.as<MacqCtl>();
    const int n_windows = A.n_windows, frame_len = A.frame_len;
    for (int round = 0;; ++round) {
        if (int rc = read_ctl(h, h->p_macq_ctl, A.ctl, s)) return rc;
        if (pool && check_dup && round == 0 && ctl.dup)
            return fail(h, RIA_ERR_INVALID, "%s: two windows of one call use one cache id, or an id is not below n_caches; no cache was touched", who);
        const int n_list = static_cast<int>(ctl.n_list);
        if (n_list == 0) break;
        if (n_list > n_windows || round >= kMacqCandidates)
            return fail(h, RIA_ERR_HIP, "%s: work list of round %d broke its bound (%d)", who, round, n_list);
        A.cur = W.list[round & 1];
        A.next = W.list[(round + 1) & 1];
        A.n_cur = n_list;
        int rc = mcdpsk_demod_impl(h, &c, samples_dev, stride, A.cur.offset, A.cur.bps, frame_len, n_list, A.cur.cfo, nullptr, W.llr, llr_ws, W.mst, s);
        if (rc != RIA_OK) return rc;
        if ((rc = macq_round_cw0(h, who, A, W, ci, h->p_macq_ctl, s)) != RIA_OK) return rc;
        if ((rc = macq_round_rest(h, who, A, W, pool, H, HW, h->p_macq_ctl, max_cw, nullptr, s)) != RIA_OK) return rc;
        hipLaunchKernelGGL(macq_next_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
        HIP_TRY(h, hipGetLastError());
    }
    return RIA_OK;
}

// What the acquire and the window call derive from their flags and configuration, behind the checks they share.  own_bad
// is the call's own extra condition and bad_text the list of them all; ci_call: the entry point takes interleaver_bits.
struct MacqSetup { bool chirp, disconnected, retry, ci; int ci_step, sym_per_cw; };
static int macq_setup(ria_gpu_handle h, const char* who, const ria_mcdpsk_config* cfg, int64_t stride, int search_len, int window_len, int n_windows,
                      uint32_t flags, bool own_bad, const char* bad_text, bool ci_call, int interleaver_bits, MacqSetup* out) {
    const uint32_t known_flags = RIA_MACQ_SYNC_CHIRP | RIA_MACQ_DISCONNECTED | RIA_MACQ_NO_RETRY | RIA_MACQ_CHANNEL_INTERLEAVE;
    MacqSetup u{};
    u.chirp = (flags & RIA_MACQ_SYNC_CHIRP) != 0; u.disconnected = (flags & RIA_MACQ_DISCONNECTED) != 0;
    if (!mcdpsk_config_ok(cfg) || n_windows < 0 || search_len < 0 || window_len < search_len || stride < window_len || own_bad ||
        (flags & ~known_flags) != 0 || (u.disconnected && !u.chirp) || (!u.chirp && search_len > kZcMaxBuf))
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (%s)", who, bad_text);
    if (h->cfg.code_rate != RIA_RATE_1_4) return fail(h, RIA_ERR_INVALID, "%s: MC-DPSK frames are R1/4: the handle's rate must be RIA_RATE_1_4", who);
    u.ci = ci_call && (flags & RIA_MACQ_CHANNEL_INTERLEAVE) != 0;
    if ((flags & RIA_MACQ_CHANNEL_INTERLEAVE) && !ci_call)
        return fail(h, RIA_ERR_UNSUPPORTED, "%s: MC-DPSK channel interleaving is ria_gpu_mcdpsk_acquire_ci_batch's", who);
    if (u.ci && !macq_ci_step(interleaver_bits, &u.ci_step)) return fail(h, RIA_ERR_INVALID, "%s: interleaver_bits %d outside 1..648", who, interleaver_bits);
    u.retry = u.disconnected && !(flags & RIA_MACQ_NO_RETRY);
    u.sym_per_cw = (kMacqLdpcBlock + cfg->num_carriers * cfg->bits_per_symbol - 1) / (cfg->num_carriers * cfg->bits_per_symbol);
    *out = u;
    return RIA_OK;
}
// The first launches of the two calls, on an A that names the call's own arrays and sizes; the rest of A is filled here.
// The outputs are cleared; the chase stages begin for `rows` codeword rows (without a pool the caller's harq rows are
// cleared); each window is searched with its own threshold (and known CFO for ZC) into W.det.
static int macq_begin(ria_gpu_handle h, const char* who, const MacqSetup& u, const MacqWs& W, MacqArgs& A, const float* samples_dev, int search_len,
                      ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev, ria_mcdpsk_harq_result* harq_dev, size_t rows,
                      hipStream_t s, HarqArgs* H, HarqWs* HW) {
    const size_t n = static_cast<size_t>(A.n_windows);
    A.connected = !u.disconnected; A.retry = u.retry; A.llr = W.llr; A.next = W.list[0];
    macq_bind(A, W, h, u.ci, u.ci_step);
    HIP_TRY(h, hipMemsetAsync(A.frame_out, 0, n * static_cast<size_t>(A.frame_row), s));
    if (A.llr_out) HIP_TRY(h, hipMemsetAsync(A.llr_out, 0, n * static_cast<size_t>(A.llr_stride) * sizeof(float), s));
    if (pool) {
        if (int rc = harq_begin(h, who, pool, cache_id_dev, now_ms_dev, harq_dev, A.n_windows, rows, static_cast<size_t>(A.dec_bytes), W.ctl, s, H, HW)) return rc;
    } else if (harq_dev) {
        HIP_TRY(h, hipMemsetAsync(harq_dev, 0, n * sizeof(ria_mcdpsk_harq_result), s));
    }
    const int pstride = static_cast<int>(sizeof(ria_mcdpsk_acq_params) / sizeof(float));
    if (u.chirp) {
        ria_chirp_result* det = reinterpret_cast<ria_chirp_result*>(W.det);
        A.chirp = det;
        return sync_chirp_impl(h, samples_dev, A.stride, search_len, A.n_windows, 0.15f, det, s, &A.params->detect_threshold, pstride);
    }
    ria_zc_result* det = reinterpret_cast<ria_zc_result*>(W.det);
    A.zc = det;
    return sync_zc_impl(h, samples_dev, A.stride, search_len, A.n_windows, 0.2f, 12u /* DATA | CONTROL */, &A.params->known_cfo_hz, det, s,
                        &A.params->detect_threshold, pstride);
}

static int macq_impl(ria_gpu_handle h, const char* who, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                     int search_len, int window_len, int n_windows, int frame_cw,
                     const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                     uint8_t* frame_out_dev, ria_mcdpsk_acq_result* acq_dev,
                     float* llr_out_dev, int llr_stride, ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                     ria_mcdpsk_harq_result* harq_dev, bool ci_call, int interleaver_bits, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    MacqSetup u;
    if (int rc = macq_setup(h, who, cfg, stride, search_len, window_len, n_windows, flags, frame_cw < 1 || frame_cw > 8,
                            "config, 0 <= search_len <= window_len <= stride, frame_cw 1..8, known flags, ZC only when connected",
                            ci_call, interleaver_bits, &u)) return rc;
    const bool ci = u.ci, retry = u.retry;
    const int nc = cfg->num_carriers, bps = cfg->bits_per_symbol, sp = cfg->spreading, sym_per_cw = u.sym_per_cw;
    const int frame_len = (kMcTrain + 1) * kMcSps + frame_cw * sym_per_cw * kMcSps * sp;      // getMinSamplesForCWCount
    if (mcdpsk_lds_bytes(nc, frame_len) > 160 * 1024)
        return fail(h, RIA_ERR_UNSUPPORTED, "%s: frame of %d samples too long for the MC-DPSK demodulator", who, frame_len);
    const int nds = frame_cw * sym_per_cw;
    const int llr_ws = nds * nc * 2;                                   // either modulation
    const int llr_need = nds * nc * (retry ? 2 : bps);                 // candidates that can run
    const int max_cw = llr_ws / kMacqLdpcBlock;                        // <= 2 * frame_cw
    if (llr_out_dev && llr_stride < llr_need)
        return fail(h, RIA_ERR_INVALID, "%s: llr_stride %d < %d soft bits", who, llr_stride, llr_need);
    if (max_cw > 2 * frame_cw) return fail(h, RIA_ERR_UNSUPPORTED, "%s: codeword bound broken", who);
    if (n_windows == 0) return RIA_OK;
    if (!samples_dev || !params_dev || !frame_out_dev || !acq_dev)
        return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = static_cast<size_t>(n_windows), dec_bytes = static_cast<size_t>((h->geo.ldpc_k + 7) / 8);
    auto carve = [&](Carver& c) { return macq_carve(c, n, static_cast<size_t>(llr_ws), static_cast<size_t>(max_cw), dec_bytes, ci); };
    HIP_TRY(h, h->d_macq_ws.reserve(carved_size(carve)));   // nothing of an earlier call is in flight: every call ends on a stream sync
    HIP_TRY(h, h->p_macq_ctl.reserve(sizeof(MacqCtl)));
    const MacqWs W = carve_at(h->d_macq_ws.as<>(), carve);
    // 1. the outputs cleared, the chase stages' begin, detection
    HarqArgs H{};
    HarqWs HW{};
    MacqArgs A{};
    A.params = params_dev; A.n_windows = n_windows; A.window_len = window_len; A.frame_len = frame_len; A.stride = stride;
    A.bps = bps; A.acq = acq_dev; A.llr_ws = llr_ws;
    A.frame_out = frame_out_dev; A.frame_row = RIA_MACQ_FRAME_BYTES(frame_cw); A.llr_out = llr_out_dev; A.llr_stride = llr_stride;
    if (int rc = macq_begin(h, who, u, W, A, samples_dev, search_len, pool, cache_id_dev, now_ms_dev, harq_dev, n * static_cast<size_t>(max_cw), s, &H, &HW)) return rc;
    // 2. acceptance + the round-0 list
    hipLaunchKernelGGL(macq_plan_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
    HIP_TRY(h, hipGetLastError());
    const ria_mcdpsk_config c = *cfg;
    // 3.-5. the rounds
    return macq_rounds(h, who, c, samples_dev, stride, A, W, pool, H, HW, ci, llr_ws, max_cw, true, s);
}

int ria_gpu_mcdpsk_acquire_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                 int search_len, int window_len, int n_windows, int frame_cw,
                                 const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                 uint8_t* frame_out_dev, ria_mcdpsk_acq_result* acq_dev,
                                 float* llr_out_dev, int llr_stride, void* stream) {
    return macq_impl(h, "ria_gpu_mcdpsk_acquire_batch", cfg, samples_dev, stride, search_len, window_len, n_windows, frame_cw, params_dev, flags,
                     frame_out_dev, acq_dev, llr_out_dev, llr_stride, nullptr, nullptr, nullptr, nullptr, false, 0, stream);
}
int ria_gpu_mcdpsk_acquire_harq_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                      int search_len, int window_len, int n_windows, int frame_cw,
                                      const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                      uint8_t* frame_out_dev, ria_mcdpsk_acq_result* acq_dev,
                                      float* llr_out_dev, int llr_stride,
                                      ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                      ria_mcdpsk_harq_result* harq_dev, void* stream) {
    return macq_impl(h, "ria_gpu_mcdpsk_acquire_harq_batch", cfg, samples_dev, stride, search_len, window_len, n_windows, frame_cw, params_dev, flags,
                     frame_out_dev, acq_dev, llr_out_dev, llr_stride, pool, cache_id_dev, now_ms_dev, harq_dev, false, 0, stream);
}
int ria_gpu_mcdpsk_acquire_ci_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                    int search_len, int window_len, int n_windows, int frame_cw,
                                    const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                    uint8_t* frame_out_dev, ria_mcdpsk_acq_result* acq_dev,
                                    float* llr_out_dev, int llr_stride,
                                    ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                    ria_mcdpsk_harq_result* harq_dev, int interleaver_bits, void* stream) {
    return macq_impl(h, "ria_gpu_mcdpsk_acquire_ci_batch", cfg, samples_dev, stride, search_len, window_len, n_windows, frame_cw, params_dev, flags,
                     frame_out_dev, acq_dev, llr_out_dev, llr_stride, pool, cache_id_dev, now_ms_dev, harq_dev, true, interleaver_bits, stream);
}

// ------------------------------------------------------------------------------------------------ one MC-DPSK window
static_assert(sizeof(ria_mcdpsk_window_result) == 64, "ria_mcdpsk_window_result is 64 bytes (include/ria_gpu.h)");
static_assert(offsetof(ria_mcdpsk_acq_params, pending_total_cw) == 12 && offsetof(ria_mcdpsk_acq_params, first_avail) == 24 &&
              offsetof(ria_mcdpsk_acq_params, last_decoded_sync) == 28 && offsetof(ria_mcdpsk_window_result, training_rms) == 32 &&
              offsetof(ria_mcdpsk_window_result, deliver) == 44, "ria_gpu_mcdpsk_window_batch field offsets");
static_assert(RIA_MWIN_NOT_ACCEPTED == kMwinNotAccepted && RIA_MWIN_REPLAY == kMwinReplay && RIA_MWIN_PING == kMwinPing &&
              RIA_MWIN_PROCESS_FAILED == kMwinProcessFailed && RIA_MWIN_DECODED == kMwinDecoded && RIA_MWIN_NEED_SAMPLES == kMwinNeedSamples &&
              RIA_MWIN_TOO_LONG == kMwinTooLong && RIA_MPEEK_NO_HEADER == kMpeekNoHeader && RIA_MPEEK_HEADER_SINGLE == kMpeekHeaderSingle &&
              RIA_MPEEK_HEADER_MULTI == kMpeekHeaderMulti && RIA_MPEEK_CONNECT_FORCED == kMpeekConnectForced &&
              RIA_MPEEK_HANDSHAKE_FALLBACK == kMpeekHandshakeFallback && RIA_MPEEK_EARLY_WINDOW == kMpeekEarlyWindow &&
              RIA_MPEEK_HANDSHAKE_WINDOW == kMpeekHandshakeWindow && RIA_MPEEK_DEINTERLEAVED == kMpeekDeinterleaved &&
              RIA_MPEEK_SALVAGE == kMpeekSalvage, "mcdpsk_window_rules.hpp mirrors include/ria_gpu.h");
struct MwinWs { MwinSt* st; MwinCtl* wctl; uint8_t *tries_a, *tries_deint, *tries_a2; };
static MwinWs mwin_carve(Carver& c, size_t n) {
    MwinWs w;
    w.st = c.take<MwinSt>(n);
    w.wctl = c.take<MwinCtl>(1);
    w.tries_a = c.take<uint8_t>(n);
    w.tries_deint = c.take<uint8_t>(n);
    w.tries_a2 = c.take<uint8_t>(n);
    return w;
}

int ria_gpu_mcdpsk_window_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                int search_len, int window_len, int n_windows,
                                const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                uint8_t* frame_out_dev, int frame_row, ria_mcdpsk_window_result* result_dev,
                                ria_mcdpsk_acq_result* acq_dev, float* llr_out_dev, int llr_stride,
                                ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                ria_mcdpsk_harq_result* harq_dev, int interleaver_bits, void* stream) {
    const char* who = "ria_gpu_mcdpsk_window_batch";
    if (!h) return RIA_ERR_INVALID;
    MacqSetup u;
    if (int rc = macq_setup(h, who, cfg, stride, search_len, window_len, n_windows, flags, frame_row < RIA_MACQ_FRAME_BYTES(8),
                            "config, 0 <= search_len <= window_len <= stride, known flags, ZC only when connected, frame_row >= RIA_MACQ_FRAME_BYTES(8)",
                            true, interleaver_bits, &u)) return rc;
    const bool ci = u.ci, retry = u.retry, disconnected = u.disconnected;
    const int nc = cfg->num_carriers, bps = cfg->bits_per_symbol, sp = cfg->spreading, sym_per_cw = u.sym_per_cw;
    MwinGeom g{};
    g.window_len = window_len; g.cw_samples = sym_per_cw * kMcSps * sp; g.cw_bits = sym_per_cw * nc * bps; g.disconnected = disconnected ? 1 : 0;
    // the longest pass: 8 codewords, what the window holds (a longer span never fits), what the demodulator's workgroup holds
    int max_level = 0;
    while (max_level < 8 && mwin_frame_len(g, max_level + 1) <= window_len &&
           mcdpsk_lds_bytes(nc, static_cast<int>(mwin_frame_len(g, max_level + 1))) <= 160 * 1024) ++max_level;
    int lds_level = 0;
    while (lds_level < 8 && mcdpsk_lds_bytes(nc, static_cast<int>(mwin_frame_len(g, lds_level + 1))) <= 160 * 1024) ++lds_level;
    g.max_level = lds_level;       // a count above it that fits the window is TOO_LONG; one that does not fit is NEED_SAMPLES first
    auto llr_ws_of = [&](int cw) { return cw * sym_per_cw * nc * 2; };                           // either modulation
    const int top = std::max(max_level, 1);
    const int llr_need = top * sym_per_cw * nc * (retry ? 2 : bps);
    if (llr_out_dev && llr_stride < llr_need) return fail(h, RIA_ERR_INVALID, "%s: llr_stride %d < %d soft bits", who, llr_stride, llr_need);
    if (n_windows == 0) return RIA_OK;
    if (!samples_dev || !params_dev || !frame_out_dev || !result_dev || !acq_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = static_cast<size_t>(n_windows), dec_bytes = static_cast<size_t>((h->geo.ldpc_k + 7) / 8);
    const int top_max_cw = llr_ws_of(top) / kMacqLdpcBlock;
    auto carve = [&](Carver& c) { return macq_carve(c, n, static_cast<size_t>(llr_ws_of(top)), static_cast<size_t>(top_max_cw), dec_bytes, ci); };
    auto wcarve = [&](Carver& c) { return mwin_carve(c, n); };
    HIP_TRY(h, h->d_macq_ws.reserve(carved_size(carve)));   // nothing of an earlier call is in flight: every call ends on a stream sync
    HIP_TRY(h, h->d_mwin_ws.reserve(carved_size(wcarve)));
    HIP_TRY(h, h->p_macq_ctl.reserve(sizeof(MacqCtl)));
    HIP_TRY(h, h->p_mwin_ctl.reserve(sizeof(MwinCtl)));
    const MacqWs W = carve_at(h->d_macq_ws.as<>(), carve);
    const MwinWs WW = carve_at(h->d_mwin_ws.as<>(), wcarve);
    HIP_TRY(h, hipMemsetAsync(WW.wctl, 0, sizeof(MwinCtl), s));
    HIP_TRY(h, hipMemsetAsync(WW.tries_deint, 0, n, s));
    // 1. the outputs cleared, the chase stages' begin, detection
    HarqArgs H{};
    HarqWs HW{};
    MwinArgs B{};
    MacqArgs& A = B.M;
    A.params = params_dev; A.n_windows = n_windows; A.window_len = window_len; A.stride = stride; A.bps = bps; A.acq = acq_dev;
    A.frame_out = frame_out_dev; A.frame_row = frame_row; A.llr_out = llr_out_dev; A.llr_stride = llr_stride;
    if (int rc = macq_begin(h, who, u, W, A, samples_dev, search_len, pool, cache_id_dev, now_ms_dev, harq_dev, n * static_cast<size_t>(top_max_cw), s, &H, &HW)) return rc;
    B.g = g; B.samples = samples_dev; B.res = result_dev; B.st = WW.st; B.wctl = WW.wctl;
    B.tries_a = WW.tries_a; B.tries_deint = WW.tries_deint; B.tries_a2 = WW.tries_a2;
    const ria_mcdpsk_config c = *cfg;
    const unsigned tgrid = static_cast<unsigned>(std::min((n_windows + 255) / 256, 1024));
    // 2.-3. acceptance, anti-replay, the energy test and the passes that need no soft bits; then the peek list
    hipLaunchKernelGGL(mwin_plan_kernel, dim3(tgrid), dim3(256), 0, s, B);
    hipLaunchKernelGGL(mwin_energy_kernel, dim3(static_cast<unsigned>((n_windows + kMwinEnergyWaves - 1) / kMwinEnergyWaves)), dim3(64 * kMwinEnergyWaves), 0, s, B);
    hipLaunchKernelGGL(mwin_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, B, 0);
    HIP_TRY(h, hipGetLastError());
    if (int rc = read_ctl(h, h->p_mwin_ctl, WW.wctl, s)) return rc;
    if (h->p_mwin_ctl.as<MwinCtl>()->bad)
        return fail(h, RIA_ERR_INVALID, "%s: a window's pending_total_cw is above 255, or its first_avail is below 9608 (connected: below the "
                                        "1-codeword span); no cache was touched", who);
    if (int rc = read_ctl(h, h->p_macq_ctl, A.ctl, s)) return rc;
    const MacqCtl& ctl = *h->p_macq_ctl.as<MacqCtl>();
    if (pool && ctl.dup)
        return fail(h, RIA_ERR_INVALID, "%s: two windows of one call use one cache id, or an id is not below n_caches; no cache was touched", who);
    // 4. the peek pass: process() on the 1-codeword span, CW0 (and the de-interleaved CW0), the rules
    const int n_peek = static_cast<int>(ctl.n_list);
    if (n_peek < 0 || n_peek > n_windows) return fail(h, RIA_ERR_HIP, "%s: the peek list broke its bound (%d)", who, n_peek);
    if (n_peek > 0) {
        if (max_level < 1) return fail(h, RIA_ERR_HIP, "%s: a peek pass without a span that fits", who);
        A.frame_len = static_cast<int>(mwin_frame_len(g, 1));
        A.llr_ws = llr_ws_of(1);
        A.cur = W.list[0]; A.next = W.list[1]; A.n_cur = n_peek;
        int rc = mcdpsk_demod_impl(h, &c, samples_dev, stride, A.cur.offset, A.cur.bps, A.frame_len, n_peek, A.cur.cfo, nullptr, W.llr, A.llr_ws, W.mst, s);
        if (rc != RIA_OK) return rc;
        if ((rc = macq_round_cw0(h, who, A, W, ci, h->p_macq_ctl, s, WW.tries_a, WW.tries_a2)) != RIA_OK) return rc;
        if (ci) {
            hipLaunchKernelGGL(mwin_a2_tries_kernel, dim3(static_cast<unsigned>(std::min((n_peek + 255) / 256, 1024))), dim3(256), 0, s, B);
        }
        hipLaunchKernelGGL(mwin_peek_kernel, dim3(static_cast<unsigned>(std::min((n_peek + 3) / 4, 4096))), dim3(256), 0, s, B);
        HIP_TRY(h, hipGetLastError());
    }
    // 5.-10. one list per codeword count, ascending: escalation and salvage only ever raise a window's count
    for (int level = 1; level <= max_level; ++level) {
        A.frame_len = static_cast<int>(mwin_frame_len(g, level));
        A.llr_ws = llr_ws_of(level);
        A.next = W.list[0];
        hipLaunchKernelGGL(mwin_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, B, level);
        HIP_TRY(h, hipGetLastError());
        if (int rc = macq_rounds(h, who, c, samples_dev, stride, A, W, pool, H, HW, ci, A.llr_ws, A.llr_ws / kMacqLdpcBlock, false, s)) return rc;
        hipLaunchKernelGGL(mwin_close_kernel, dim3(tgrid), dim3(256), 0, s, B, level);
        HIP_TRY(h, hipGetLastError());
    }
    return RIA_OK;
}

// One window from host memory (ria_host::mcdpskWindow): staged through the handle's pinned + device block on the handle's own
// stream, like ria_gpu_decode_frame_host.  No chase pool.
int ria_gpu_mcdpsk_window_host(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_host, int search_len, int window_len,
                               const ria_mcdpsk_acq_params* params_host, uint32_t flags, uint8_t* frame_out_host, int max_bytes,
                               ria_mcdpsk_window_result* result_out, ria_mcdpsk_acq_result* acq_out, int interleaver_bits) {
    if (!h) return RIA_ERR_INVALID;
    const int frame_row = RIA_MACQ_FRAME_BYTES(8);
    if (!samples_host || !params_host || !frame_out_host || !result_out || !acq_out || window_len < 1 || max_bytes < frame_row)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_window_host: bad argument (null pointer, window_len >= 1, max_bytes >= RIA_MACQ_FRAME_BYTES(8))");
    HIP_TRY(h, hipSetDevice(h->device));
    struct Stage { float* x; ria_mcdpsk_acq_params* par; uint8_t* frame; ria_mcdpsk_window_result* res; ria_mcdpsk_acq_result* acq; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.x = c.in(static_cast<size_t>(window_len), samples_host); w.par = c.in(1, params_host);
        w.frame = c.out(static_cast<size_t>(frame_row), frame_out_host); w.res = c.out(1, result_out); w.acq = c.out(1, acq_out);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        return ria_gpu_mcdpsk_window_batch(h, cfg, d.x, window_len, search_len, window_len, 1, d.par, flags, d.frame, frame_row, d.res, d.acq,
                                           nullptr, 0, nullptr, nullptr, nullptr, nullptr, interleaver_bits, s); });
}

int ria_gpu_mcdpsk_interleave_batch(ria_gpu_handle h, int interleaver_bits, const uint8_t* coded_dev, int n_cw, uint8_t* out_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    int step = 0;
    if (!macq_ci_step(interleaver_bits, &step) || n_cw < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_interleave_batch: bad argument (interleaver_bits 1..648, n_cw >= 0)");
    if (n_cw == 0) return RIA_OK;
    if (!coded_dev || !out_dev || coded_dev == out_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_mcdpsk_interleave_batch: null pointer, or in place");
    int step_inv = 1;
    while ((step * step_inv) % kMacqLdpcBlock != 1) ++step_inv;       // step is coprime with 648
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(macq_interleave_kernel, dim3(static_cast<unsigned>(std::min((n_cw + 3) / 4, 4096))), dim3(256), 0, static_cast<hipStream_t>(stream),
                       coded_dev, out_dev, n_cw, step_inv);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

// ------------------------------------------------------------------------------------------------ from a capture to its next window
static_assert(sizeof(ria_search_state) == 32 && sizeof(ria_search_result) == 112 && offsetof(ria_search_result, abs_position) == 16 &&
              offsetof(ria_search_result, invocations) == 60, "ria_gpu_search_batch record layouts (include/ria_gpu.h)");
static_assert(RIA_SEARCH_OFDM_LTS == kSearchLts && RIA_SEARCH_MCDPSK_ZC == kSearchZc && RIA_SEARCH_MCDPSK_CHIRP == kSearchChirp &&
              RIA_SEARCH_SYNC_FOUND == kSearchSyncFound && RIA_SEARCH_NEED_SAMPLES == kSearchNeedSamples && RIA_SEARCH_LIMIT == kSearchLimit,
              "search_rules.hpp mirrors include/ria_gpu.h");
struct SearchWs { uint32_t* list; SearchCtl* ctl; float* span; SearchPar* par; ria_zc_result* det; };   // det: 32 bytes for each of the three detectors
static_assert(sizeof(ria_zc_result) == 32 && sizeof(ria_lts_result) == 32 && sizeof(ria_chirp_result) == 32, "one detector record area");
static SearchWs search_carve(Carver& c, size_t n, size_t chunk, size_t min_search) {
    SearchWs w;
    w.list = c.take<uint32_t>(n);
    w.ctl = c.take<SearchCtl>(1);
    w.span = c.take<float>(chunk * min_search);
    w.par = c.take<SearchPar>(chunk);
    w.det = c.take<ria_zc_result>(chunk);
    return w;
}
static int search_class(int mode, int modulation) {
    if (mode != RIA_SEARCH_OFDM_LTS) return kSrchZc;
    if (modulation == RIA_MOD_QPSK || modulation == RIA_MOD_BPSK) return kSrchCoherentPsk;
    if (modulation == RIA_MOD_QAM16 || modulation == RIA_MOD_QAM32 || modulation == RIA_MOD_QAM64 || modulation == RIA_MOD_QAM256) return kSrchCoherentQam;
    return kSrchDifferential;
}

// every block of a ring search call, before anything of it is in flight: the call's own workspace and the detector's
// (search_impl's steps; that function stays as it is).
// *chunk_out: the streams whose spans one chunk of the due list holds.
static int search_reserve(ria_gpu_handle h, int mode, int n_streams, int min_search, hipStream_t s, int* chunk_out) {
    const size_t per = static_cast<size_t>(min_search) * sizeof(float);
    int chunk = static_cast<int>(std::min<size_t>(static_cast<size_t>(n_streams), std::max<size_t>(1, (size_t(256) << 20) / per)));
    chunk = std::min(chunk, 65535);                    // the gather's grid y extent
    if (h->search_chunk > 0) chunk = std::min(chunk, h->search_chunk);
    auto carve = [&](Carver& c) { return search_carve(c, static_cast<size_t>(n_streams), static_cast<size_t>(chunk), static_cast<size_t>(min_search)); };
    HIP_TRY(h, h->d_search_ws.reserve(carved_size(carve), &s));
    HIP_TRY(h, h->p_search_ctl.reserve(sizeof(SearchCtl)));
    if (mode == RIA_SEARCH_OFDM_LTS) {
        if (int rc = lts_prepare(h)) return rc;
    } else if (mode == RIA_SEARCH_MCDPSK_ZC) {
        const size_t zper = static_cast<size_t>(min_search) * sizeof(float2);
        HIP_TRY(h, h->d_zc_ws.reserve(zper * std::min<size_t>(static_cast<size_t>(chunk), std::max<size_t>(1, (size_t(256) << 20) / zper)), &s));
    } else {
        if (int rc = chirp_prepare(h, std::min(chunk, 64), std::min(chunk, 2048), s)) return rc;
    }
    *chunk_out = chunk;
    return RIA_OK;
}

// the mode's detector on the nb gathered spans of W through its own launcher; the one record pointer of the mode is set
static int search_detect(ria_gpu_handle h, int mode, const SearchWs& W, int min_search, int nb, hipStream_t s, const ria_lts_result** lts,
                         const ria_zc_result** zc, const ria_chirp_result** chirp) {
    const int pstride = static_cast<int>(sizeof(SearchPar) / sizeof(float));
    if (mode == RIA_SEARCH_OFDM_LTS) {
        ria_lts_result* det = reinterpret_cast<ria_lts_result*>(W.det);
        LtsArgs S{};
        S.samples = W.span; S.stride = min_search; S.buf_len = min_search; S.n_buffers = nb;
        S.known_cfo = &W.par->known_cfo_hz; S.threshold_dev = &W.par->detect_threshold; S.param_stride = pstride;
        S.hilbert = h->d_hilbert65.as<const float>(); S.out = det;
        hipLaunchKernelGGL(lts_sync_kernel, dim3(nb), dim3(kLtsThreads), lts_lds_bytes(), s, S);
        *lts = det;
    } else if (mode == RIA_SEARCH_MCDPSK_ZC) {
        *zc = W.det;
        if (int rc = sync_zc_impl(h, W.span, min_search, min_search, nb, 0.2f, 12u /* DATA | CONTROL */, &W.par->known_cfo_hz, W.det, s,
                                  &W.par->detect_threshold, pstride)) return rc;
    } else {
        ria_chirp_result* det = reinterpret_cast<ria_chirp_result*>(W.det);
        *chirp = det;
        if (int rc = sync_chirp_impl(h, W.span, min_search, min_search, nb, 0.15f, det, s, nullptr, 1)) return rc;
    }
    return RIA_OK;
}

// The search on n_streams streams: all of them, or those subset_dev lists (ascending stream indices; captures, lengths,
// states and results stay indexed by stream, so nothing is copied).  ria_gpu_rx_stream_batch searches its open streams so.
static int search_impl(ria_gpu_handle h, const char* who, int mode, uint32_t flags, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                       const int32_t* capture_len_dev, int n_streams, const uint32_t* subset_dev, ria_search_state* state_dev, int feed_step,
                       int max_invocations, ria_search_result* result_dev, void* stream) {
    const bool mc = mode == RIA_SEARCH_MCDPSK_ZC || mode == RIA_SEARCH_MCDPSK_CHIRP;
    if ((mode != RIA_SEARCH_OFDM_LTS && !mc) || (flags & ~RIA_SEARCH_CONNECTED) != 0 || n_streams < 0 || stride < 0 || feed_step < 0 ||
        max_invocations < 1 || (mc && !mcdpsk_config_ok(cfg)))
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (mode RIA_SEARCH_*, flags RIA_SEARCH_CONNECTED only, n_streams >= 0, stride >= 0, feed_step >= 0, "
                                        "max_invocations >= 1, an MC-DPSK config for the MC-DPSK modes)", who);
    if (n_streams == 0) return RIA_OK;
    if (!samples_dev || !capture_len_dev || !state_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int min_search = srch_min_search(mode);
    const size_t per = static_cast<size_t>(min_search) * sizeof(float);
    int chunk = static_cast<int>(std::min<size_t>(static_cast<size_t>(n_streams), std::max<size_t>(1, (size_t(256) << 20) / per)));
    chunk = std::min(chunk, 65535);                    // the gather's grid y extent
    if (h->search_chunk > 0) chunk = std::min(chunk, h->search_chunk);
    // every block of the call, before anything of it is in flight: the call's own workspace and the detector's
    auto carve = [&](Carver& c) { return search_carve(c, static_cast<size_t>(n_streams), static_cast<size_t>(chunk), static_cast<size_t>(min_search)); };
    HIP_TRY(h, h->d_search_ws.reserve(carved_size(carve), &s));
    HIP_TRY(h, h->p_search_ctl.reserve(sizeof(SearchCtl)));
    if (mode == RIA_SEARCH_OFDM_LTS) {
        if (int rc = lts_prepare(h)) return rc;
    } else if (mode == RIA_SEARCH_MCDPSK_ZC) {
        const size_t zper = static_cast<size_t>(min_search) * sizeof(float2);
        HIP_TRY(h, h->d_zc_ws.reserve(zper * std::min<size_t>(static_cast<size_t>(chunk), std::max<size_t>(1, (size_t(256) << 20) / zper)), &s));
    } else {
        if (int rc = chirp_prepare(h, std::min(chunk, 64), std::min(chunk, 2048), s)) return rc;
    }
    const SearchWs W = carve_at(h->d_search_ws.as<>(), carve);
    HIP_TRY(h, hipMemsetAsync(W.ctl, 0, sizeof(SearchCtl), s));
    SearchArgs A{};
    A.samples = samples_dev; A.stride = stride; A.capture_len = capture_len_dev; A.state = state_dev; A.res = result_dev;
    A.subset = subset_dev;
    A.n_streams = n_streams; A.mode = mode; A.cls = search_class(mode, h->cfg.modulation);
    A.connected = (mode != RIA_SEARCH_MCDPSK_CHIRP || (flags & RIA_SEARCH_CONNECTED)) ? 1 : 0;
    A.feed_step = feed_step; A.max_invocations = max_invocations; A.min_search = min_search;
    A.ctl = W.ctl; A.list = W.list; A.span = W.span; A.par = W.par;
    const unsigned wgrid = static_cast<unsigned>((n_streams + kSearchWalkWaves - 1) / kSearchWalkWaves);
    const int pstride = static_cast<int>(sizeof(SearchPar) / sizeof(float));
    hipLaunchKernelGGL(search_check_kernel, dim3(static_cast<unsigned>((n_streams + 255) / 256)), dim3(256), 0, s, A);
    for (int round = 0;; ++round) {
        if (round > max_invocations) return fail(h, RIA_ERR_HIP, "%s: round %d past max_invocations", who, round);
        hipLaunchKernelGGL(search_walk_kernel, dim3(wgrid), dim3(64 * kSearchWalkWaves), 0, s, A, round == 0 ? 1 : 0);
        hipLaunchKernelGGL(search_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
        HIP_TRY(h, hipGetLastError());
        if (int rc = read_ctl(h, h->p_search_ctl, W.ctl, s)) return rc;
        const SearchCtl ctl = *h->p_search_ctl.as<SearchCtl>();
        if (ctl.bad)
            return fail(h, RIA_ERR_INVALID, "%s: a stream's capture_len is above min(stride, 959999), or its state is outside the call's domain "
                                            "(0 <= fed <= capture_len, 0 <= correlation_pos < 960000, reject_streak >= 0); no state or result was written", who);
        const int n_list = static_cast<int>(ctl.n_list);
        if (n_list < 0 || n_list > n_streams) return fail(h, RIA_ERR_HIP, "%s: the due list broke its bound (%d)", who, n_list);
        if (n_list == 0) break;
        for (int first = 0; first < n_list; first += chunk) {
            const int nb = std::min(chunk, n_list - first);
            A.first = first; A.n_chunk = nb; A.lts = nullptr; A.zc = nullptr; A.chirp = nullptr;
            hipLaunchKernelGGL(search_gather_kernel, dim3(static_cast<unsigned>(std::min((min_search + 1023) / 1024, 64)), static_cast<unsigned>(nb)), dim3(256), 0, s, A);
            HIP_TRY(h, hipGetLastError());
            if (mode == RIA_SEARCH_OFDM_LTS) {
                ria_lts_result* det = reinterpret_cast<ria_lts_result*>(W.det);
                LtsArgs S{};
                S.samples = W.span; S.stride = min_search; S.buf_len = min_search; S.n_buffers = nb;
                S.known_cfo = &W.par->known_cfo_hz; S.threshold_dev = &W.par->detect_threshold; S.param_stride = pstride;
                S.hilbert = h->d_hilbert65.as<const float>(); S.out = det;
                hipLaunchKernelGGL(lts_sync_kernel, dim3(nb), dim3(kLtsThreads), lts_lds_bytes(), s, S);
                A.lts = det;
            } else if (mode == RIA_SEARCH_MCDPSK_ZC) {
                A.zc = W.det;
                if (int rc = sync_zc_impl(h, W.span, min_search, min_search, nb, 0.2f, 12u /* DATA | CONTROL */, &W.par->known_cfo_hz, W.det, s,
                                          &W.par->detect_threshold, pstride)) return rc;
            } else {
                ria_chirp_result* det = reinterpret_cast<ria_chirp_result*>(W.det);
                A.chirp = det;
                if (int rc = sync_chirp_impl(h, W.span, min_search, min_search, nb, 0.15f, det, s, nullptr, 1)) return rc;
            }
            hipLaunchKernelGGL(search_accept_kernel, dim3(static_cast<unsigned>((nb + 255) / 256)), dim3(256), 0, s, A);
            HIP_TRY(h, hipGetLastError());
        }
    }
    return RIA_OK;
}

int ria_gpu_search_batch(ria_gpu_handle h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                         const int32_t* capture_len_dev, int n_streams, ria_search_state* state_dev, int feed_step, int max_invocations,
                         ria_search_result* result_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    return search_impl(h, "ria_gpu_search_batch", mode, flags, cfg, samples_dev, stride, capture_len_dev, n_streams, nullptr, state_dev, feed_step,
                       max_invocations, result_dev, stream);
}

// ------------------------------------------------------------------------------------------------ the search past the ring buffer's wrap
static_assert(sizeof(ria_ring_state) == 48 && offsetof(ria_ring_state, overflow_dropped) == 40 && sizeof(ria_ring_search_result) == 144 &&
              offsetof(ria_ring_search_result, abs_position) == 16 && offsetof(ria_ring_search_result, invocations) == 60 &&
              offsetof(ria_ring_search_result, abs_search_start) == 112 && offsetof(ria_ring_search_result, span_wraps) == 140,
              "ria_gpu_search_ring_batch record layouts (include/ria_gpu.h)");

// The ring search on n_streams streams: all of them, or those subset_dev lists (ascending; ria_gpu_rx_ring_batch's open streams)
static int ring_search_impl(ria_gpu_handle h, const char* who, int mode, uint32_t flags, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                            const int32_t* capture_len_dev, int n_streams, const uint32_t* subset_dev, ria_ring_state* state_dev, int feed_step,
                            int max_invocations, ria_ring_search_result* result_dev, void* stream) {
    const bool mc = mode == RIA_SEARCH_MCDPSK_ZC || mode == RIA_SEARCH_MCDPSK_CHIRP;
    if ((mode != RIA_SEARCH_OFDM_LTS && !mc) || (flags & ~RIA_SEARCH_CONNECTED) != 0 || n_streams < 0 || stride < 0 || feed_step < 0 ||
        max_invocations < 1 || (mc && !mcdpsk_config_ok(cfg)))
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (mode RIA_SEARCH_*, flags RIA_SEARCH_CONNECTED only, n_streams >= 0, stride >= 0, feed_step >= 0, "
                                        "max_invocations >= 1, an MC-DPSK config for the MC-DPSK modes)", who);
    if (n_streams == 0) return RIA_OK;
    if (!samples_dev || !capture_len_dev || !state_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int min_search = srch_min_search(mode);
    int chunk;
    if (int rc = search_reserve(h, mode, n_streams, min_search, s, &chunk)) return rc;
    auto carve = [&](Carver& c) { return search_carve(c, static_cast<size_t>(n_streams), static_cast<size_t>(chunk), static_cast<size_t>(min_search)); };
    const SearchWs W = carve_at(h->d_search_ws.as<>(), carve);
    HIP_TRY(h, hipMemsetAsync(W.ctl, 0, sizeof(SearchCtl), s));
    RingArgs A{};
    A.samples = samples_dev; A.stride = stride; A.capture_len = capture_len_dev; A.state = state_dev; A.res = result_dev;
    A.subset = subset_dev;
    A.n_streams = n_streams; A.mode = mode; A.cls = search_class(mode, h->cfg.modulation);
    A.connected = (mode != RIA_SEARCH_MCDPSK_CHIRP || (flags & RIA_SEARCH_CONNECTED)) ? 1 : 0;
    A.feed_step = feed_step; A.max_invocations = max_invocations; A.min_search = min_search;
    A.ctl = W.ctl; A.list = W.list; A.span = W.span; A.par = W.par;
    const unsigned wgrid = static_cast<unsigned>((n_streams + kSearchWalkWaves - 1) / kSearchWalkWaves);
    hipLaunchKernelGGL(ring_check_kernel, dim3(static_cast<unsigned>((n_streams + 255) / 256)), dim3(256), 0, s, A);
    for (int round = 0;; ++round) {
        if (round > max_invocations) return fail(h, RIA_ERR_HIP, "%s: round %d past max_invocations", who, round);
        hipLaunchKernelGGL(ring_walk_kernel, dim3(wgrid), dim3(64 * kSearchWalkWaves), 0, s, A, round == 0 ? 1 : 0);
        hipLaunchKernelGGL(ring_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A);
        HIP_TRY(h, hipGetLastError());
        if (int rc = read_ctl(h, h->p_search_ctl, W.ctl, s)) return rc;
        const SearchCtl ctl = *h->p_search_ctl.as<SearchCtl>();
        if (ctl.bad)
            return fail(h, RIA_ERR_INVALID, "%s: a stream's capture_len is above min(stride, 2^31 - 1 - 960000), or its state is outside the call's domain "
                                            "(0 <= total_fed <= capture_len, 0 <= correlation_pos < 960000, reject_streak >= 0, last_decoded_sync_pos in "
                                            "0..959999 or INT32_MIN); no state or result was written", who);
        const int n_list = static_cast<int>(ctl.n_list);
        if (n_list < 0 || n_list > n_streams) return fail(h, RIA_ERR_HIP, "%s: the due list broke its bound (%d)", who, n_list);
        if (n_list == 0) break;
        for (int first = 0; first < n_list; first += chunk) {
            const int nb = std::min(chunk, n_list - first);
            A.first = first; A.n_chunk = nb; A.lts = nullptr; A.zc = nullptr; A.chirp = nullptr;
            hipLaunchKernelGGL(ring_gather_kernel, dim3(static_cast<unsigned>(std::min((min_search + 1023) / 1024, 64)), static_cast<unsigned>(nb)), dim3(256), 0, s, A);
            HIP_TRY(h, hipGetLastError());
            if (int rc = search_detect(h, mode, W, min_search, nb, s, &A.lts, &A.zc, &A.chirp)) return rc;
            hipLaunchKernelGGL(ring_accept_kernel, dim3(static_cast<unsigned>((nb + 255) / 256)), dim3(256), 0, s, A);
            HIP_TRY(h, hipGetLastError());
        }
    }
    return RIA_OK;
}

int ria_gpu_search_ring_batch(ria_gpu_handle h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                              const int32_t* capture_len_dev, int n_streams, ria_ring_state* state_dev, int feed_step, int max_invocations,
                              ria_ring_search_result* result_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    return ring_search_impl(h, "ria_gpu_search_ring_batch", mode, flags, cfg, samples_dev, stride, capture_len_dev, n_streams, nullptr, state_dev, feed_step,
                            max_invocations, result_dev, stream);
}

// ------------------------------------------------------------------------------------------------ the chase pool
static_assert(sizeof(ria_chase_config) == 32 && sizeof(ria_chase_stats) == 56 && sizeof(ria_chase_entry) == 80 && sizeof(ChaseCache) == 1344 &&
              sizeof(ria_mcdpsk_harq_result) == 32 && sizeof(ria_mcdpsk_dframe_result) == 16, "HARQ record sizes (include/ria_gpu.h)");

void ria_gpu_chase_default_config(ria_chase_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->n_caches = 1; cfg->max_entries = RIA_CHASE_MAX_ENTRIES; cfg->ttl_ms = 30000;
}
int ria_gpu_chase_create(ria_gpu_handle h, const ria_chase_config* cfg, ria_chase_pool* out) {
    if (!h) return RIA_ERR_INVALID;
    if (!cfg || !out || cfg->n_caches < 1 || cfg->max_entries < 1 || cfg->max_entries > RIA_CHASE_MAX_ENTRIES || cfg->ttl_ms < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_chase_create: bad argument (n_caches >= 1, max_entries 1..16, ttl_ms >= 0)");
    *out = nullptr;
    HIP_TRY(h, hipSetDevice(h->device));
    auto p = std::make_unique<ria_chase_pool_s>();
    p->h = h; p->cfg = *cfg;
    const size_t nc = static_cast<size_t>(cfg->n_caches);
    HIP_TRY(h, p->d_meta.reserve(nc * sizeof(ChaseCache)));
    HIP_TRY(h, p->d_sums.reserve(nc * static_cast<size_t>(cfg->max_entries) * RIA_CHASE_MAX_CW * kMacqLdpcBlock * sizeof(float)));
    HIP_TRY(h, p->d_owner.reserve(nc * sizeof(int32_t)));
    HIP_TRY(h, hipMemset(p->d_meta.as<>(), 0, nc * sizeof(ChaseCache)));
    HIP_TRY(h, hipMemset(p->d_sums.as<>(), 0, p->d_sums.bytes()));
    *out = p.get();
    h->chase_pools.push_back(std::move(p));
    return RIA_OK;
}
void ria_gpu_chase_destroy(ria_chase_pool pool) {
    if (!pool || !pool->h) return;
    ria_gpu_handle h = pool->h;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();      // work that reads the pool may still be in flight
    auto& v = h->chase_pools;
    v.erase(std::remove_if(v.begin(), v.end(), [&](const std::unique_ptr<ria_chase_pool_s>& p) { return p.get() == pool; }), v.end());
}
int ria_gpu_chase_clear(ria_chase_pool pool, const int32_t* cache_ids_dev, int n, void* stream) {
    if (!pool || !pool->h) return RIA_ERR_INVALID;
    ria_gpu_handle h = pool->h;
    if (cache_ids_dev && n < 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_chase_clear: n < 0");
    const int count = cache_ids_dev ? n : pool->cfg.n_caches;
    if (count == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(harq_clear_kernel, dim3(static_cast<unsigned>(std::min((count + 255) / 256, 1024))), dim3(256), 0, static_cast<hipStream_t>(stream),
                       pool->d_meta.as<ChaseCache>(), pool->cfg.n_caches, cache_ids_dev, count);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}
static int chase_read_cache(ria_chase_pool pool, const char* who, int cache_id, ChaseCache* out) {
    ria_gpu_handle h = pool->h;
    if (cache_id < 0 || cache_id >= pool->cfg.n_caches) return fail(h, RIA_ERR_INVALID, "%s: cache_id %d outside the pool", who, cache_id);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(out, pool->d_meta.as<ChaseCache>() + cache_id, sizeof(ChaseCache), hipMemcpyDeviceToHost));
    return RIA_OK;
}
int ria_gpu_chase_stats(ria_chase_pool pool, int cache_id, ria_chase_stats* out_host) {
    if (!pool || !pool->h) return RIA_ERR_INVALID;
    if (!out_host) return fail(pool->h, RIA_ERR_INVALID, "ria_gpu_chase_stats: null pointer");
    ChaseCache c;
    if (int rc = chase_read_cache(pool, "ria_gpu_chase_stats", cache_id, &c)) return rc;
    *out_host = c.stats;
    return RIA_OK;
}
int ria_gpu_chase_export(ria_chase_pool pool, int cache_id, ria_chase_entry* entries_out_host, float* sums_out_host) {
    if (!pool || !pool->h) return RIA_ERR_INVALID;
    ria_gpu_handle h = pool->h;
    ChaseCache c;
    if (int rc = chase_read_cache(pool, "ria_gpu_chase_export", cache_id, &c)) return rc;
    const int me = pool->cfg.max_entries;
    const size_t per_entry = static_cast<size_t>(RIA_CHASE_MAX_CW) * kMacqLdpcBlock;
    if (entries_out_host) std::memset(entries_out_host, 0, static_cast<size_t>(me) * sizeof(ria_chase_entry));
    if (sums_out_host) std::memset(sums_out_host, 0, static_cast<size_t>(me) * per_entry * sizeof(float));
    int n = 0;
    for (int s = 0; s < me; ++s) {
        if (!c.e[s].used) continue;
        if (entries_out_host) entries_out_host[n] = c.e[s];
        if (sums_out_host) {
            const float* src = pool->d_sums.as<float>() + (static_cast<size_t>(cache_id) * me + s) * per_entry;
            for (int cw = 0; cw < RIA_CHASE_MAX_CW; ++cw)
                if (c.e[s].has_sum[cw])
                    HIP_TRY(h, hipMemcpy(sums_out_host + (static_cast<size_t>(n) * RIA_CHASE_MAX_CW + cw) * kMacqLdpcBlock, src + static_cast<size_t>(cw) * kMacqLdpcBlock,
                                         kMacqLdpcBlock * sizeof(float), hipMemcpyDeviceToHost));
        }
        ++n;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------ decodeMCDPSKFrame on soft bits
struct MdfWs { MacqWs m; ria_mcdpsk_acq_result* acq; };
static int mdf_impl(ria_gpu_handle h, const char* who, const float* llr_dev, int llr_stride, const int32_t* n_llr_dev, int n_frames,
                    ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                    uint8_t* frame_out_dev, int frame_row, ria_mcdpsk_dframe_result* result_dev,
                    ria_mcdpsk_harq_result* harq_dev, uint32_t flags, int interleaver_bits, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (flags & ~RIA_MACQ_CHANNEL_INTERLEAVE) return fail(h, RIA_ERR_INVALID, "%s: flags is 0 or RIA_MACQ_CHANNEL_INTERLEAVE", who);
    const bool ci = flags != 0;
    int ci_step = 0;
    if (ci && !macq_ci_step(interleaver_bits, &ci_step)) return fail(h, RIA_ERR_INVALID, "%s: interleaver_bits %d outside 1..648", who, interleaver_bits);
    if (n_frames < 0 || llr_stride < kMacqLdpcBlock || llr_stride > RIA_CHASE_MAX_CW * kMacqLdpcBlock || frame_row < kMacqCwBytes * (llr_stride / kMacqLdpcBlock))
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (648 <= llr_stride <= 16 * 648, frame_row >= 20 * (llr_stride / 648))", who);
    if (h->cfg.code_rate != RIA_RATE_1_4) return fail(h, RIA_ERR_INVALID, "%s: MC-DPSK frames are R1/4: the handle's rate must be RIA_RATE_1_4", who);
    if (n_frames == 0) return RIA_OK;
    if (!llr_dev || !frame_out_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = static_cast<size_t>(n_frames), max_cw = static_cast<size_t>(llr_stride / kMacqLdpcBlock);
    const size_t dec_bytes = static_cast<size_t>((h->geo.ldpc_k + 7) / 8);
    auto carve = [&](Carver& c) { MdfWs w; w.m = macq_carve(c, n, 0, max_cw, dec_bytes, ci); w.acq = c.take<ria_mcdpsk_acq_result>(n); return w; };
    HIP_TRY(h, h->d_mdf_ws.reserve(carved_size(carve), &s));
    HIP_TRY(h, h->p_mdf_ctl.reserve(sizeof(MacqCtl)));
    const MdfWs MW = carve_at(h->d_mdf_ws.as<>(), carve);
    const MacqWs& W = MW.m;
    HarqArgs H{};
    HarqWs HW{};
    if (pool) {
        if (int rc = harq_begin(h, who, pool, cache_id_dev, now_ms_dev, harq_dev, n_frames, n * max_cw, dec_bytes, W.ctl, s, &H, &HW)) return rc;
    } else if (harq_dev) {
        HIP_TRY(h, hipMemsetAsync(harq_dev, 0, n * sizeof(ria_mcdpsk_harq_result), s));
    }
    MacqArgs A{};
    A.n_windows = n_frames; A.retry = 0; A.bps = 1; A.acq = MW.acq;
    A.cur = W.list[0]; A.next = W.list[1]; A.n_cur = n_frames;
    macq_bind(A, W, h, ci, ci_step);
    A.llr = llr_dev; A.llr_ws = llr_stride;
    A.frame_out = frame_out_dev; A.frame_row = frame_row;
    // the rows as one round's list (every row, in order), then that round's stages; ctl.dup is tested with the round's
    // row-list read, the first that every call makes
    const unsigned tgrid = static_cast<unsigned>(std::min((n_frames + 255) / 256, 1024));
    hipLaunchKernelGGL(mdf_list_kernel, dim3(tgrid), dim3(256), 0, s, A, n_llr_dev, W.mst);
    if (int rc = macq_round_cw0(h, who, A, W, ci, h->p_mdf_ctl, s)) return rc;
    if (int rc = macq_round_rest(h, who, A, W, pool, H, HW, h->p_mdf_ctl, static_cast<int>(max_cw), "rows", s)) return rc;
    hipLaunchKernelGGL(mdf_result_kernel, dim3(tgrid), dim3(256), 0, s, MW.acq, n_frames, result_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}
int ria_gpu_mcdpsk_decode_frame_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, const int32_t* n_llr_dev, int n_frames,
                                      ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                      uint8_t* frame_out_dev, int frame_row, ria_mcdpsk_dframe_result* result_dev,
                                      ria_mcdpsk_harq_result* harq_dev, void* stream) {
    return mdf_impl(h, "ria_gpu_mcdpsk_decode_frame_batch", llr_dev, llr_stride, n_llr_dev, n_frames, pool, cache_id_dev, now_ms_dev, frame_out_dev,
                    frame_row, result_dev, harq_dev, 0u, 0, stream);
}
int ria_gpu_mcdpsk_decode_frame_ci_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, const int32_t* n_llr_dev, int n_frames,
                                         ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                         uint8_t* frame_out_dev, int frame_row, ria_mcdpsk_dframe_result* result_dev,
                                         ria_mcdpsk_harq_result* harq_dev, uint32_t flags, int interleaver_bits, void* stream) {
    return mdf_impl(h, "ria_gpu_mcdpsk_decode_frame_ci_batch", llr_dev, llr_stride, n_llr_dev, n_frames, pool, cache_id_dev, now_ms_dev, frame_out_dev,
                    frame_row, result_dev, harq_dev, flags, interleaver_bits, stream);
}

// ------------------------------------------------------------------------------------------------ decodeFrame (OFDM branch)
static_assert(sizeof(ria_dframe_result) == 32, "ria_dframe_result is 32 bytes (include/ria_gpu.h)");
static_assert(offsetof(ria_dframe_result, frame_bytes) == 8 && offsetof(ria_dframe_result, iters_r14) == 12 &&
              offsetof(ria_dframe_result, tries_r14) == 16 && offsetof(ria_dframe_result, reserved) == 20, "ria_dframe_result field offsets");
static_assert(sizeof(DfProbe) == 80 && sizeof(DfRow) == 20, "decode_frame_kernels.hip.h record sizes");

// the R1/4 code on a handle of another rate: H, the core layout of the per-rate cache, the tables on the device
static int dframe_ensure_r14(ria_gpu_handle h) {
    if (h->have14) return RIA_OK;
    const LdpcCode code = build_ldpc(RIA_RATE_1_4);
    const CoreTables t = core_tables_for(RIA_RATE_1_4, code);
    if (!shape_fits(RIA_RATE_1_4, t, &h->wave_lds14)) return fail(h, RIA_ERR_UNSUPPORTED, "ria_gpu_decode_frame_batch: the R1/4 code does not fit its compiled shape");
    FastCode& f = h->fast14;
    HIP_TRY(h, upload_core_tables(t, h->d_f14, f));
    f.k = code.k; f.m = code.m; f.max_iter = recommended_iterations(RIA_RATE_1_4); f.bytes_per_cw = info_bits_for(RIA_RATE_1_4) / 8;
    set_fast_attributes(RIA_RATE_1_4, h->wave_lds14);
    h->have14 = true;
    return RIA_OK;
}

// the decodeFrame workspace for n rows of up to max_cw codewords.  The control block, row state, probe records and lists lie
// in front of the bulk areas: one memset clears them.
struct DfWs {
    DfCtl* ctl; DfRow* row; DfProbe* probe; uint32_t* list;
    float* fx_llr; uint8_t* fx_info; ria_decode_status* fx_st;                                             // the fixed batch
    float* lg_rows; uint32_t* lg_entry; uint8_t* lg_cw; uint8_t* lg_out; uint8_t* lg_ok; uint16_t* lg_it;   // legacy rows: CW1.. of every frame
};
static DfWs dframe_carve(Carver& c, size_t n, size_t max_cw, size_t bpc, size_t dec_bytes) {
    const size_t nr = n * (max_cw - 1);
    DfWs w;
    w.ctl = c.take<DfCtl>(1);
    w.row = c.take<DfRow>(n);
    w.probe = c.take<DfProbe>(4 * n);
    w.list = c.take<uint32_t>(kDfNumLists * n);
    w.fx_llr = c.take<float>(n * kDfFrameBits);
    w.fx_info = c.take<uint8_t>(n * 4 * bpc);
    w.fx_st = c.take<ria_decode_status>(n);
    w.lg_rows = c.take<float>(nr * kDfBlock);
    w.lg_entry = c.take<uint32_t>(nr);
    w.lg_cw = c.take<uint8_t>(nr);
    w.lg_out = c.take<uint8_t>(nr * dec_bytes);
    w.lg_ok = c.take<uint8_t>(nr);
    w.lg_it = c.take<uint16_t>(nr);
    return w;
}
// The reserve step of decodeFrame for n_frames rows of up to max_cw codewords: the R1/4 code on a handle of another rate,
// the de-interleave table the flags select, the workspace with its control block, and decodeFixedFrame's (decode_reserve).
// Nothing of an earlier call is in flight: every call ends on a stream sync.  `who` is the public call, for the message.
static int dframe_reserve(ria_gpu_handle h, const char* who, int n_frames, size_t max_cw, uint32_t flags, DfWs* out) {
    if (h->cfg.code_rate != RIA_RATE_1_4) { if (int rc = dframe_ensure_r14(h)) return rc; }
    const bool ch_deint = (flags & RIA_DECODE_NO_CHANNEL_DEINTERLEAVE) == 0;
    DevBuf& perm = h->d_cw_perm[ch_deint ? 1 : 0];
    if (!perm) HIP_TRY(h, upload(perm, build_cw_deinterleave(h->geo.bits_per_symbol, ch_deint)));
    auto carve = [&](Carver& c) {
        return dframe_carve(c, static_cast<size_t>(n_frames), max_cw, static_cast<size_t>(h->geo.bytes_per_codeword), static_cast<size_t>((h->geo.ldpc_k + 7) / 8));
    };
    hipError_t e = h->d_df_ws.reserve(carved_size(carve));
    if (e == hipSuccess) e = h->p_df_ctl.reserve(sizeof(DfCtl));
    if (e == hipSuccess) e = decode_reserve(h, n_frames, flags);
    if (e != hipSuccess) return fail(h, RIA_ERR_HIP, "%s workspace: %s", who, hipGetErrorString(e));
    *out = carve_at(h->d_df_ws.as<>(), carve);
    return RIA_OK;
}

int ria_gpu_decode_frame_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, const int32_t* n_llr_dev, int n_frames,
                               uint32_t flags, uint8_t* frame_out_dev, int frame_row, ria_dframe_result* result_dev,
                               ria_decode_status* decode_status_dev, uint8_t* info_out_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    const int bpc = h->geo.bytes_per_codeword;
    if (n_frames < 0 || llr_stride < kDfBlock || llr_stride > kDfMaxCw * kDfBlock || (flags & ~(RIA_DECODE_FULL | RIA_DECODE_NO_CHANNEL_DEINTERLEAVE)) != 0 ||
        frame_row < std::max(4, llr_stride / kDfBlock) * bpc)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_decode_frame_batch: bad argument (648 <= llr_stride <= 32 * 648, frame_row >= max(4, llr_stride / 648) * "
                                        "bytes_per_codeword, RIA_DECODE_* flags only)");
    if (n_frames == 0) return RIA_OK;
    if (!llr_dev || !frame_out_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "ria_gpu_decode_frame_batch: null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool r14 = h->cfg.code_rate == RIA_RATE_1_4;
    const size_t n = static_cast<size_t>(n_frames), max_cw = static_cast<size_t>(llr_stride / kDfBlock);
    // everything the call may need is allocated here, before any of it is in flight
    DfWs W;
    if (int rc = dframe_reserve(h, "ria_gpu_decode_frame_batch", n_frames, max_cw, flags, &W)) return rc;
    const DfCtl& ctl = *h->p_df_ctl.as<DfCtl>();
    DfArgs A{};
    A.llr = llr_dev; A.llr_stride = llr_stride; A.n_llr = n_llr_dev; A.n_frames = n_frames;
    A.rate_is_r14 = r14 ? 1 : 0; A.bpc = bpc; A.bpc14 = info_bits_for(RIA_RATE_1_4) / 8;
    A.row = W.row; A.probe = W.probe; A.list = W.list; A.ctl = W.ctl;
    A.fx_llr = W.fx_llr; A.fx_info = W.fx_info; A.fx_st = W.fx_st;
    A.perm = h->d_cw_perm[(flags & RIA_DECODE_NO_CHANNEL_DEINTERLEAVE) ? 0 : 1].as<const uint16_t>();
    A.lg_rows = W.lg_rows; A.lg_entry = W.lg_entry; A.lg_cw = W.lg_cw;
    A.lg_out = W.lg_out; A.lg_ok = W.lg_ok; A.dec_bytes = (h->geo.ldpc_k + 7) / 8;
    A.crc_bit = h->d_crc_bit.as<const uint16_t>(); A.crc_init = h->d_crc_init.as<const uint16_t>();
    A.frame_out = frame_out_dev; A.frame_row = frame_row; A.result = result_dev; A.st_out = decode_status_dev; A.info_out = info_out_dev;
    // control block, row state, probe records and lists in one memset (they lie in front of the bulk areas)
    HIP_TRY(h, hipMemsetAsync(W.ctl, 0, span_bytes(W.ctl, W.fx_llr), s));
    const unsigned probe_grid = static_cast<unsigned>(std::min(n_frames, 16384));
    auto list = [&](int stage) { hipLaunchKernelGGL(dframe_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, stage); };
    auto probe_rate = [&](bool robust, int which_list, int which_probe, unsigned grid) {
        dispatch_shape(h->cfg.code_rate, [&](auto sh) {
            using S = decltype(sh);
            if (robust) hipLaunchKernelGGL((dframe_probe_kernel<S, true>), dim3(grid), dim3(64), ShapeInfo<S>::lds_bytes, s, h->fast, A, which_list, which_probe, bpc);
            else hipLaunchKernelGGL((dframe_probe_kernel<S, false>), dim3(grid), dim3(64), ShapeInfo<S>::lds_bytes, s, h->fast, A, which_list, which_probe, bpc);
        });
    };
    auto probe_r14 = [&](bool robust, int which_list, int which_probe, unsigned grid) {
        if (robust) hipLaunchKernelGGL((dframe_probe_kernel<ShapeR14, true>), dim3(grid), dim3(64), ShapeInfo<ShapeR14>::lds_bytes, s, h->fast14, A, which_list, which_probe, A.bpc14);
        else hipLaunchKernelGGL((dframe_probe_kernel<ShapeR14, false>), dim3(grid), dim3(64), ShapeInfo<ShapeR14>::lds_bytes, s, h->fast14, A, which_list, which_probe, A.bpc14);
    };
    // 1.-2. the two plain CW0 probes, each over the rows still open
    list(kDfStageInit);
    if (!r14) {
        probe_r14(false, kDfListR14, kDfProbeR14, probe_grid);
        list(kDfStageAfterR14);
    }
    probe_rate(false, kDfListRate, kDfProbeRate, probe_grid);
    list(kDfStageAfterRate);
    HIP_TRY(h, hipGetLastError());
    if (int rc = read_ctl(h, h->p_df_ctl, A.ctl, s, "decode work-queue fault: no frame of this call was decoded")) return rc;   // read 1 of 2: the length of the fixed batch
    const int n_fixed = static_cast<int>(ctl.n[kDfListFixed]);
    if (n_fixed < 0 || n_fixed > n_frames) return fail(h, RIA_ERR_HIP, "ria_gpu_decode_frame_batch: the fixed list broke its bound (%d)", n_fixed);
    // 3.-4. decodeFixedFrame over the try_frame_interleave rows, then the two salvage decoders over what it left
    if (n_fixed > 0) {
        hipLaunchKernelGGL(dframe_fixed_gather_kernel, dim3(static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(n_fixed) * kDfFrameBits + 255) / 256, 16384))),
                           dim3(256), 0, s, A, n_fixed);
        int rc = launch_decode(h, A.fx_llr, kDfFrameBits, n_fixed, flags, A.fx_info, A.fx_st, s);
        if (rc != RIA_OK) return rc;
        const unsigned sg = static_cast<unsigned>(std::min(n_fixed, 16384));
        list(kDfStageAfterFixed);
        if (r14) probe_rate(true, kDfListSalvR14, kDfSalvR14, sg); else probe_r14(true, kDfListSalvR14, kDfSalvR14, sg);
        list(kDfStageAfterSalvR14);
        if (!r14) probe_rate(true, kDfListSalvRate, kDfSalvRate, sg);
    }
    // 5. legacy: the rows of CW1.. of the non-interleaved multi-codeword frames
    list(kDfStageLegacy);
    HIP_TRY(h, hipGetLastError());
    if (int rc = read_ctl(h, h->p_df_ctl, A.ctl, s, "decode work-queue fault: no frame of this call was decoded")) return rc;   // read 2 of 2: the legacy rows (and the fault flag)
    const long long n_rows = static_cast<long long>(ctl.n_rows);
    if (n_rows < 0 || static_cast<size_t>(n_rows) > n * (max_cw - 1)) return fail(h, RIA_ERR_HIP, "ria_gpu_decode_frame_batch: the legacy rows broke their bound (%lld)", n_rows);
    if (n_rows > 0) {
        const int nr = static_cast<int>(n_rows);
        hipLaunchKernelGGL(dframe_legacy_rows_kernel, dim3(static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(nr) * kDfBlock + 255) / 256, 16384))),
                           dim3(256), 0, s, A, nr);
        int rc = ria_gpu_ldpc_decode_batch(h, A.lg_rows, nr, h->geo.ldpc_max_iterations, 0.75f, W.lg_out, W.lg_ok, W.lg_it, s);
        if (rc != RIA_OK) return rc;
    }
    // 6. results
    hipLaunchKernelGGL(dframe_finish_kernel, dim3(static_cast<unsigned>(std::min((n_frames + 3) / 4, 4096))), dim3(256), 0, s, A);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_decode_frame_host(ria_gpu_handle h, const float* llr_host, int n_llr, uint32_t flags, uint8_t* frame_out_host, int max_bytes,
                              ria_dframe_result* result_out, ria_decode_status* decode_status_out) {
    if (!h) return RIA_ERR_INVALID;
    if (n_llr < 0 || (n_llr > 0 && !llr_host) || !frame_out_host || !result_out)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_decode_frame_host: bad argument");
    const int n_use = std::min(n_llr, kDfMaxCw * kDfBlock);                 // the cap of 32 codewords per row
    const int stride = std::max(kDfBlock, n_use);
    const int frame_row = std::max(4, stride / kDfBlock) * h->geo.bytes_per_codeword;
    if (max_bytes < frame_row) return fail(h, RIA_ERR_INVALID, "ria_gpu_decode_frame_host: max_bytes %d < %d (max(4, n_llr / 648) * bytes_per_codeword)", max_bytes, frame_row);
    HIP_TRY(h, hipSetDevice(h->device));
    const int32_t n_used = n_use;
    const float none = 0.0f;   // a row without soft bits is still a row of zeros
    struct Stage { float* llr; int32_t* n_llr; uint8_t* frame; ria_dframe_result* res; ria_decode_status* ds; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        // the row is padded with zeros to a whole codeword
        w.llr = c.in(static_cast<size_t>(stride), n_use > 0 ? llr_host : &none, static_cast<size_t>(n_use)); w.n_llr = c.in(1, &n_used);
        w.frame = c.out(static_cast<size_t>(frame_row), frame_out_host); w.res = c.out(1, result_out); w.ds = c.out(1, decode_status_out);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        return ria_gpu_decode_frame_batch(h, d.llr, stride, d.n_llr, 1, flags, d.frame, frame_row, d.res, d.ds, nullptr, s); });
}

// ------------------------------------------------------------------------------------------------ one connected-mode window
static_assert(sizeof(ria_window_result) == 64, "ria_window_result is 64 bytes (include/ria_gpu.h)");
static_assert(offsetof(ria_window_result, outcome) == 32 && offsetof(ria_window_result, frame_len) == 40 &&
              offsetof(ria_window_result, sync_cfo_hz) == 52 && offsetof(ria_window_result, fading_index) == 60, "ria_window_result field offsets");
static_assert(sizeof(WinRow) == 32 && sizeof(WinCtl) == 32, "window_kernels.hip.h record sizes");

// the window workspace for n windows: soft-bit rows of llr_row floats, decodeFrame rows of df_row bytes
struct WinWs {
    WinCtl* ctl; DfCtl* pctl; WinRow* row; uint32_t* plist; DfProbe* probe; int32_t* n_llr_d;
    FrameList list[kWinGroups];
    float* llr_c; ria_frame_status* fst_c;           // one pass's demodulations, compact
    float* llr_w; ria_frame_status* fst_w;           // per window
    uint8_t* df_frames; ria_dframe_result* df_res;   // decodeFrame's outputs, per window
    ria_control_result* cres; uint8_t* cframes; ria_frame_status* cfst;   // the control hypothesis's, per window
};
static WinWs window_carve(Carver& c, size_t n, size_t llr_row, size_t df_row) {
    WinWs w;
    w.ctl = c.take<WinCtl>(1);
    w.pctl = c.take<DfCtl>(1);
    w.row = c.take<WinRow>(n);
    w.plist = c.take<uint32_t>(n);
    w.probe = c.take<DfProbe>(2 * n);
    w.n_llr_d = c.take<int32_t>(n);
    for (FrameList& l : w.list) take_frame_list(c, l, n);
    w.llr_c = c.take<float>(n * llr_row);
    w.fst_c = c.take<ria_frame_status>(n);
    w.llr_w = c.take<float>(n * llr_row);
    w.fst_w = c.take<ria_frame_status>(n);
    w.df_frames = c.take<uint8_t>(n * df_row);
    w.df_res = c.take<ria_dframe_result>(n);
    w.cres = c.take<ria_control_result>(n);
    w.cframes = c.take<uint8_t>(n * kCtlFrameBytes);
    w.cfst = c.take<ria_frame_status>(n);
    return w;
}

// One demodulation pass: the windows with a job, listed per span length; the host reads the five lengths (one
// synchronisation), launches the span demodulator once per non-empty list and scatters the rows to their windows.
static int win_demod_pass(ria_gpu_handle h, const float* samples_dev, WinArgs& A, const WinWs& W, hipStream_t s, int* total_out) {
    hipLaunchKernelGGL(win_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, 0);
    HIP_TRY(h, hipGetLastError());
    if (int rc = read_ctl(h, h->p_win_ctl, W.ctl, s)) return rc;
    const WinCtl c = *h->p_win_ctl.as<WinCtl>();
    long long total = 0;
    for (int g = 0; g < kWinGroups; ++g) {
        A.base[g] = static_cast<int>(total);
        A.cnt[g] = static_cast<int>(c.n[g]);
        total += c.n[g];
        if (total > A.n) return fail(h, RIA_ERR_HIP, "ria_gpu_rx_window_batch: a span list broke its bound (%lld)", total);
    }
    *total_out = static_cast<int>(total);
    if (total == 0) return RIA_OK;
    for (int g = 0; g < kWinGroups; ++g) {
        if (A.cnt[g] == 0) continue;
        if (int rc = demod_var_launch(h, samples_dev, A.list[g].offset, A.list[g].meta, A.cnt[g], A.len[g],
                                      W.llr_c + static_cast<size_t>(A.base[g]) * A.llr_stride, A.llr_stride, W.fst_c + A.base[g], s)) return rc;
    }
    hipLaunchKernelGGL(win_scatter_kernel, dim3(static_cast<unsigned>(std::min<long long>(total, 16384))), dim3(256), 0, s, A, static_cast<int>(total));
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_rx_window_batch(ria_gpu_handle control_h, ria_gpu_handle h, const float* samples_dev, int64_t stride, int search_len,
                            int window_len, int n_windows, const ria_acq_params* params_dev, uint32_t flags, uint8_t* frame_out_dev,
                            int frame_row, ria_window_result* result_dev, ria_acq_result* acq_dev, ria_control_result* control_dev,
                            ria_frame_status* demod_status_dev, void* stream) {
    if (!h || !control_h) return RIA_ERR_INVALID;
    const char* who = "ria_gpu_rx_window_batch";
    if (!is_control_handle(control_h) || control_h->cfg.num_carriers != h->cfg.num_carriers || control_h->device != h->device)
        return fail(h, RIA_ERR_INVALID, "%s: the control handle must be DQPSK R1/4 with the data handle's carriers, on its device", who);
    const uint32_t known_flags = RIA_DECODE_FULL | RIA_DECODE_NO_CHANNEL_DEINTERLEAVE | RIA_BURST_INTERLEAVE | RIA_ACQ_NO_TIMING_RETRY;
    const int bpc = h->geo.bytes_per_codeword, llr_row = h->geo.llrs_per_frame;
    const int df_row = std::max(4, llr_row / kDfBlock) * bpc;
    if (n_windows < 0 || search_len < 0 || window_len < search_len || stride < window_len || (flags & ~known_flags) != 0 || frame_row < std::max(df_row, kCtlFrameBytes))
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (0 <= search_len <= window_len <= stride; frame_row >= max(4, llrs_per_frame / 648) * bytes_per_codeword; "
                                        "flags: RIA_DECODE_*, RIA_BURST_INTERLEAVE, RIA_ACQ_NO_TIMING_RETRY)", who);
    if (n_windows == 0) return RIA_OK;
    if (!samples_dev || !params_dev || !frame_out_dev || !result_dev || !acq_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = demod_span_reserve(h, who)) return rc;
    const int n_ctl = ria_gpu_control_frame_samples(control_h, h);
    if (n_ctl < 0) return n_ctl;
    if (n_ctl > h->geo.frame_samples) return fail(h, RIA_ERR_UNSUPPORTED, "%s: the control span (%d samples) is longer than a frame of the data profile", who, n_ctl);
    const bool r14 = h->cfg.code_rate == RIA_RATE_1_4;
    const uint32_t dflags = flags & (RIA_DECODE_FULL | RIA_DECODE_NO_CHANNEL_DEINTERLEAVE);
    const size_t n = static_cast<size_t>(n_windows);

    // every workspace of the call and of the calls it makes, before anything is in flight: the reserve steps of the span
    // demodulator (above), of ria_gpu_control_acquire_batch on the control handle and of ria_gpu_decode_frame_batch
    ControlWs cw;
    DfWs dw;
    if (int rc = control_ensure_ws(control_h, who, n_windows, s, &cw)) return fail(h, rc, "%s: %s", who, ria_gpu_last_error(control_h));
    if (int rc = lts_prepare(control_h)) return fail(h, rc, "%s: %s", who, ria_gpu_last_error(control_h));
    if (int rc = dframe_reserve(h, who, n_windows, static_cast<size_t>(llr_row / kDfBlock), dflags, &dw)) return rc;
    auto carve = [&](Carver& c) { return window_carve(c, n, static_cast<size_t>(llr_row), static_cast<size_t>(df_row)); };
    HIP_TRY(h, h->d_win_ws.reserve(carved_size(carve), &s));
    HIP_TRY(h, h->p_win_ctl.reserve(sizeof(WinCtl)));
    const WinWs W = carve_at(h->d_win_ws.as<>(), carve);

    HIP_TRY(h, hipMemsetAsync(frame_out_dev, 0, n * static_cast<size_t>(frame_row), s));
    if (demod_status_dev) HIP_TRY(h, hipMemsetAsync(demod_status_dev, 0, n * sizeof(ria_frame_status), s));
    ria_control_result* cres = control_dev ? control_dev : W.cres;

    // 1.-2. detection, acceptance and the control hypothesis: ria_gpu_control_acquire_batch's
    if (int rc = ria_gpu_control_acquire_batch(control_h, samples_dev, stride, search_len, window_len, n_windows, n_ctl, params_dev,
                                               flags & RIA_BURST_INTERLEAVE, W.cframes, cres, acq_dev, W.cfst, s))
        return fail(h, rc, "%s: %s", who, ria_gpu_last_error(control_h));

    WinArgs A{};
    A.n = n_windows; A.window_len = window_len; A.stride = stride; A.params = params_dev; A.acq = acq_dev;
    A.cres = cres; A.cframes = W.cframes; A.cfst = W.cfst;
    A.bps = h->geo.bits_per_symbol;
    A.len[0] = n_ctl;
    for (int c = 1; c < kWinGroups; ++c) A.len[c] = win_samples_for_cw(A.bps, c);
    A.is_qam = (h->cfg.modulation == RIA_MOD_QAM16 || h->cfg.modulation == RIA_MOD_QAM32 || h->cfg.modulation == RIA_MOD_QAM64 ||
                h->cfg.modulation == RIA_MOD_QAM256) ? 1 : 0;
    A.rate_is_r14 = r14 ? 1 : 0; A.retry = (flags & RIA_ACQ_NO_TIMING_RETRY) ? 0 : 1;
    A.row = W.row; A.ctl = W.ctl;
    for (int g = 0; g < kWinGroups; ++g) A.list[g] = W.list[g];
    A.llr_c = W.llr_c; A.fst_c = W.fst_c; A.llr_w = W.llr_w; A.fst_w = W.fst_w; A.llr_stride = llr_row; A.n_llr_d = W.n_llr_d;
    A.probe = W.probe; A.plist = W.plist; A.pctl = W.pctl;
    A.df_frames = W.df_frames; A.df_row = df_row; A.df_res = W.df_res;
    A.frame_out = frame_out_dev; A.frame_row = frame_row; A.result = result_dev; A.fst_out = demod_status_dev;

    // a launch that fails is reported under its own stage: the lambdas keep the first error, `launched` hands it on
    hipError_t launch_err = hipSuccess;
    auto note = [&]() { const hipError_t e = hipGetLastError(); if (launch_err == hipSuccess) launch_err = e; };
    auto stage = [&](int st) { hipLaunchKernelGGL(win_stage_kernel, dim3(static_cast<unsigned>((n_windows + 255) / 256)), dim3(256), 0, s, A, st); note(); };
    // robustDecodeSingleCW of the listed windows' first 648 soft bits, with magic, truncation and parseHeader (dframe_probe_kernel)
    auto probe = [&](bool at_rate) {
        hipLaunchKernelGGL(win_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, at_rate ? 2 : 1);
        note();
        DfArgs D{};
        D.llr = W.llr_w; D.llr_stride = llr_row; D.n_frames = n_windows; D.probe = W.probe; D.list = W.plist; D.ctl = W.pctl;
        D.crc_bit = h->d_crc_bit.as<const uint16_t>(); D.crc_init = h->d_crc_init.as<const uint16_t>();
        const unsigned grid = static_cast<unsigned>(std::min(n_windows, 16384));
        const int bpc14 = info_bits_for(RIA_RATE_1_4) / 8;
        if (at_rate || r14) {
            dispatch_shape(h->cfg.code_rate, [&](auto sh) {
                using S = decltype(sh);
                hipLaunchKernelGGL((dframe_probe_kernel<S, true>), dim3(grid), dim3(64), ShapeInfo<S>::lds_bytes, s, h->fast, D, 0,
                                   at_rate ? kWinProbeRate : kWinProbeR14, at_rate ? bpc : bpc14);
            });
        } else {
            hipLaunchKernelGGL((dframe_probe_kernel<ShapeR14, true>), dim3(grid), dim3(64), ShapeInfo<ShapeR14>::lds_bytes, s, h->fast14, D, 0, kWinProbeR14, bpc14);
        }
        note();
    };
    // decodeFrame of the windows with the decode flag: ria_gpu_decode_frame_batch over all rows, n_llr 0 where a window has none
    auto decode = [&]() -> int {
        stage(kWinPrepDecode);
        HIP_TRY(h, launch_err);
        return ria_gpu_decode_frame_batch(h, W.llr_w, llr_row, W.n_llr_d, n_windows, dflags, W.df_frames, df_row, W.df_res, nullptr, nullptr, s);
    };
    auto finish = [&]() -> int {
        stage(kWinFinal);
        HIP_TRY(h, launch_err);
        return RIA_OK;
    };

    int total = 0;
    stage(kWinInit);
    // 3. pass 1, the peek span with the data profile at the known CFO; CFO feedback; the CW0 peek
    if (int rc = win_demod_pass(h, samples_dev, A, W, s, &total)) return rc;
    if (total == 0) return finish();
    stage(kWinPeek1);
    probe(false);
    stage(kWinPeekR14);
    if (!r14) { probe(true); stage(kWinPeekRate); }
    stage(kWinEscalate);
    // 4. pass 2 at the fed-back CFO, one launch per span length
    if (int rc = win_demod_pass(h, samples_dev, A, W, s, &total)) return rc;
    if (total) stage(kWinPass2);
    // 5. decodeFrame
    if (int rc = decode()) return rc;
    stage(kWinDecoded1);
    // 6. small-frame recovery
    if (int rc = win_demod_pass(h, samples_dev, A, W, s, &total)) return rc;
    if (total) {
        stage(kWinSmall1);
        probe(false);
        stage(kWinSmallR14);
        if (!r14) { probe(true); stage(kWinSmallRate); }
        if (int rc = win_demod_pass(h, samples_dev, A, W, s, &total)) return rc;
        if (total) stage(kWinSmallExact);
        if (int rc = decode()) return rc;
        stage(kWinDecoded2);
    }
    // 7. timing recovery: every round runs the windows still failing, each at its own next candidate that fits
    stage(kWinRecInit);
    for (int round = 1;; ++round) {
        if (int rc = win_demod_pass(h, samples_dev, A, W, s, &total)) return rc;
        if (total == 0) break;
        if (round >= kAcqCandidates) return fail(h, RIA_ERR_HIP, "%s: the recovery rounds broke their bound", who);
        stage(kWinRecDemod);
        if (int rc = decode()) return rc;
        stage(kWinRecDecoded);
    }
    // 8. consumed samples and the receiver state
    return finish();
}

// ------------------------------------------------------------------------------------------------ recordings in, frames out
static_assert(sizeof(ria_stream_event) == 64 && offsetof(ria_stream_event, next_pos) == 16 && offsetof(ria_stream_event, delivered) == 32 &&
              offsetof(ria_stream_event, correlation) == 40 && sizeof(ria_stream_result) == 64 && offsetof(ria_stream_result, invocations) == 16,
              "ria_gpu_rx_stream_batch record layouts (include/ria_gpu.h)");
static_assert(RIA_WIN_BURST == kStrmWinBurst && RIA_WIN_CONTROL_PROFILE == kStrmWinControlProfile && RIA_WIN_DECODED == kStrmWinDecoded &&
              RIA_WIN_NEED_SAMPLES == kStrmWinNeedSamples && RIA_WIN_TOO_LONG == kStrmWinTooLong && RIA_MWIN_DECODED == kStrmMwinDecoded &&
              RIA_MWIN_NEED_SAMPLES == kStrmMwinNeedSamples && RIA_MWIN_TOO_LONG == kStrmMwinTooLong &&
              RIA_STREAM_SEARCH_NEED_SAMPLES == kStreamSearchNeedSamples && RIA_STREAM_SEARCH_LIMIT == kStreamSearchLimit &&
              RIA_STREAM_SEARCH_NEED_SAMPLES == RIA_SEARCH_NEED_SAMPLES && RIA_STREAM_SEARCH_LIMIT == RIA_SEARCH_LIMIT &&
              RIA_STREAM_WINDOW_NEED_SAMPLES == kStreamWindowNeedSamples && RIA_STREAM_EVENTS_FULL == kStreamEventsFull &&
              RIA_STREAM_RING_END == kStreamRingEnd && kStreamRingLast == kSrchMaxCapture,
              "stream_rules.hpp mirrors include/ria_gpu.h");
static_assert(sizeof(ria_acq_params) == 32 && sizeof(ria_mcdpsk_acq_params) == 32 && sizeof(ria_window_result) == 64 &&
              sizeof(ria_mcdpsk_window_result) == 64 && sizeof(ria_acq_result) <= 64 && sizeof(ria_mcdpsk_acq_result) == 64, "one area per record kind");
struct StreamWs {
    uint32_t* head;               // StreamCtl (4 words), found [n], found_len [n]: what the host reads per round, in one copy
    uint32_t *open, *group;
    ria_search_result* sres;
    float* win;
    ria_acq_params* par;          // either parameter record
    ria_window_result* wres;      // either window result
    ria_mcdpsk_acq_result* acq;   // either acquire result
    uint8_t* wframes;
};
static StreamWs stream_carve(Carver& c, size_t n, size_t chunk, size_t win_floats, size_t wframe_row) {
    StreamWs w;
    w.head = c.take<uint32_t>(4 + 2 * n);
    w.open = c.take<uint32_t>(n);
    w.group = c.take<uint32_t>(n);
    w.sres = c.take<ria_search_result>(n);
    w.win = c.take<float>(win_floats);
    w.par = c.take<ria_acq_params>(chunk);
    w.wres = c.take<ria_window_result>(chunk);
    w.acq = c.take<ria_mcdpsk_acq_result>(chunk);
    w.wframes = c.take<uint8_t>(chunk * wframe_row);
    return w;
}
// what ria_gpu_mcdpsk_stream_batch adds to the loop (null: ria_gpu_rx_stream_batch), and its part of the workspace
struct McStreamExt {
    ria_mcdpsk_stream_state* mstate;
    uint32_t window_flags; int interleaver_bits;
    ria_chase_pool pool; const int32_t* cache_id; const uint64_t* t0_ms;
    ria_mcdpsk_harq_result* harq;
};
struct McStreamWs {
    McStreamCtl* mctl;
    ria_search_state* sstate;     // [n] the search part of the caller's records, contiguous: what the search reads and writes
    int32_t* w_cache_id; uint64_t* w_now_ms; ria_mcdpsk_harq_result* w_harq;   // [chunk]
};
static McStreamWs mcstream_carve(Carver& c, size_t n, size_t chunk) {
    McStreamWs w;
    w.mctl = c.take<McStreamCtl>(1);
    w.sstate = c.take<ria_search_state>(n);
    w.w_cache_id = c.take<int32_t>(chunk);
    w.w_now_ms = c.take<uint64_t>(chunk);
    w.w_harq = c.take<ria_mcdpsk_harq_result>(chunk);
    return w;
}
// mode / flags / cfg / handles / sizes of the two stream calls; *family, *full, *first_frame, *min_row from them
static int stream_setup(ria_gpu_handle h, ria_gpu_handle control_h, const char* who, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                        int max_events, int frame_row, int* full, int* first_frame, int* min_row) {
    const bool mc = mode == RIA_SEARCH_MCDPSK_ZC || mode == RIA_SEARCH_MCDPSK_CHIRP;
    if ((mode != RIA_SEARCH_OFDM_LTS && !mc) || (flags & ~RIA_SEARCH_CONNECTED) != 0 || (mc && !mcdpsk_config_ok(cfg)) || max_events < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (mode RIA_SEARCH_*, flags RIA_SEARCH_CONNECTED only, an MC-DPSK config for the MC-DPSK modes, "
                                        "max_events >= 1)", who);
    const int min_search = srch_min_search(mode);
    if (mc) {
        if (control_h) return fail(h, RIA_ERR_INVALID, "%s: control_h is for RIA_SEARCH_OFDM_LTS only", who);
        if (h->cfg.code_rate != RIA_RATE_1_4) return fail(h, RIA_ERR_INVALID, "%s: MC-DPSK frames are R1/4: the handle's rate must be RIA_RATE_1_4", who);
        const int sym_per_cw = (kMacqLdpcBlock + cfg->num_carriers * cfg->bits_per_symbol - 1) / (cfg->num_carriers * cfg->bits_per_symbol);
        const long long cw = static_cast<long long>(sym_per_cw) * kMcSps * cfg->spreading, pre = (kMcTrain + 1) * kMcSps;
        if (min_search + pre + 8 * cw > kSrchRing) return fail(h, RIA_ERR_INVALID, "%s: the 8-codeword span of this configuration is longer than a capture", who);
        *first_frame = static_cast<int>(pre + cw);
        *full = static_cast<int>(min_search + pre + 8 * cw);
        *min_row = RIA_MACQ_FRAME_BYTES(8);
    } else {
        if (!control_h || !is_control_handle(control_h) || control_h->cfg.num_carriers != h->cfg.num_carriers || control_h->device != h->device)
            return fail(h, RIA_ERR_INVALID, "%s: RIA_SEARCH_OFDM_LTS needs the control handle: DQPSK R1/4 with the data handle's carriers, on its device", who);
        *first_frame = h->geo.frame_samples;
        *full = min_search + h->geo.frame_samples + 32;
        *min_row = std::max(std::max(4, h->geo.llrs_per_frame / kDfBlock) * h->geo.bytes_per_codeword, kCtlFrameBytes);
    }
    if (frame_row < *min_row) return fail(h, RIA_ERR_INVALID, "%s: frame_row %d is below the window call's minimum %d", who, frame_row, *min_row);
    return RIA_OK;
}

// The loop of the two stream calls.  x null: ria_gpu_rx_stream_batch, on state_dev.  x set: ria_gpu_mcdpsk_stream_batch, on
// x->mstate (state_dev is null) - the up-front check, the re-entry round ahead of the first search leg, the window call with
// x's pool, time and interleaving, and the search part of the state written back behind the last round.
static int stream_impl(ria_gpu_handle h, ria_gpu_handle control_h, const char* who, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                       const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                       ria_search_state* state_dev, int feed_step, int max_invocations, int max_events,
                       ria_stream_event* events_dev, uint8_t* frames_dev, int frame_row, ria_stream_result* result_dev, void* stream,
                       const McStreamExt* x) {
    int full = 0, first_frame = 0, min_row = 0;
    if (int rc = stream_setup(h, control_h, who, mode, flags, cfg, max_events, frame_row, &full, &first_frame, &min_row)) return rc;
    if (n_streams < 0 || stride < 0 || feed_step < 0 || max_invocations < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (n_streams >= 0, stride >= 0, feed_step >= 0, max_invocations >= 1)", who);
    if (n_streams == 0) return RIA_OK;
    if (!samples_dev || !capture_len_dev || (!state_dev && !x) || !events_dev || !frames_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool ofdm = mode == RIA_SEARCH_OFDM_LTS;
    const size_t n = static_cast<size_t>(n_streams);
    const int search_len = srch_min_search(mode);
    const long long win_stride = (static_cast<long long>(full) + 3) & ~3LL;          // rows of the window workspace start on 16 bytes
    int chunk = static_cast<int>(std::min<size_t>(n, std::max<size_t>(1, (size_t(256) << 20) / (static_cast<size_t>(win_stride) * sizeof(float)))));
    chunk = std::min(chunk, 65535);                    // the gather's grid y extent
    // a re-entered window runs to the end of the span it waited for, which may lie past `full`: room for one capture at least
    const size_t win_floats = std::max<size_t>(static_cast<size_t>(chunk) * static_cast<size_t>(win_stride), x ? static_cast<size_t>(kSrchRing) : 0);
    auto carve = [&](Carver& c) {
        std::pair<StreamWs, McStreamWs> w;
        w.first = stream_carve(c, n, static_cast<size_t>(chunk), win_floats, static_cast<size_t>(min_row));
        if (x) w.second = mcstream_carve(c, n, static_cast<size_t>(chunk));
        return w;
    };
    const size_t head_bytes = (4 + 2 * n) * sizeof(uint32_t);
    HIP_TRY(h, h->d_stream_ws.reserve(carved_size(carve), &s));
    HIP_TRY(h, h->p_stream_ctl.reserve(head_bytes));
    const auto carved = carve_at(h->d_stream_ws.as<>(), carve);
    const StreamWs& W = carved.first;
    const McStreamWs& XW = carved.second;
    uint32_t* mirror = h->p_stream_ctl.as<uint32_t>();
    if (x) state_dev = XW.sstate;

    StreamArgs A{};
    A.samples = samples_dev; A.stride = stride; A.capture_len = capture_len_dev; A.state = state_dev; A.sres = W.sres;
    A.res = result_dev; A.events = events_dev; A.frames = frames_dev; A.frame_row = frame_row;
    A.n_streams = n_streams; A.mode = mode; A.family = ofdm ? kStreamOfdm : kStreamMcdpsk; A.full = full; A.first_frame = first_frame;
    A.max_events = max_events;
    A.ctl = reinterpret_cast<StreamCtl*>(W.head); A.found = W.head + 4; A.found_len = reinterpret_cast<int32_t*>(W.head + 4 + n);
    A.open = nullptr; A.group = W.group; A.n_open = n_streams;
    A.win = W.win; A.win_stride = win_stride; A.wframes = W.wframes; A.wframe_row = min_row;
    if (ofdm) { A.par = W.par; A.wres = W.wres; }
    else { A.mpar = reinterpret_cast<ria_mcdpsk_acq_params*>(W.par); A.mres = reinterpret_cast<const ria_mcdpsk_window_result*>(W.wres); A.macq = W.acq; }
    const uint32_t mflags = mode == RIA_SEARCH_MCDPSK_CHIRP ? (RIA_MACQ_SYNC_CHIRP | ((flags & RIA_SEARCH_CONNECTED) ? 0u : RIA_MACQ_DISCONNECTED)) : 0u;
    const unsigned sgrid = static_cast<unsigned>((n_streams + 255) / 256);
    bool window_ran = false;
    McStreamArgs M{};
    uint32_t xflags = mflags;
    if (x) {
        M.mstate = x->mstate; M.harq = x->harq; M.sres_w = W.sres; M.mctl = XW.mctl;
        M.sample_rate = h->cfg.sample_rate; M.search_len = search_len;
        M.w_cache_id = XW.w_cache_id; M.w_now_ms = XW.w_now_ms; M.w_harq = XW.w_harq;
        if (x->pool) { M.cache_id = x->cache_id; M.t0_ms = x->t0_ms; M.owner = x->pool->d_owner.as<int32_t>(); M.n_caches = x->pool->cfg.n_caches; }
        xflags |= x->window_flags;
    }

    // the found list as the host read it (n_found streams, their window lengths behind mirror[4 + n]): one pass per distinct
    // window length, ascending (steps 3.-6. of a round)
    auto run_windows = [&](int n_found, int longest) -> int {
        A.n_found = n_found;
        std::vector<int> lens(mirror + 4 + n, mirror + 4 + n + n_found);
        std::sort(lens.begin(), lens.end());
        for (size_t at = 0; at < lens.size();) {
            const int wl = lens[at];
            size_t end = at;
            while (end < lens.size() && lens[end] == wl) ++end;
            const int n_group = static_cast<int>(end - at);
            at = end;
            if (wl < search_len || wl > longest) return fail(h, RIA_ERR_HIP, "%s: a window of %d samples, outside %d..%d", who, wl, search_len, longest);
            // windows up to `full` lie in rows of win_stride; a longer one (re-entry only) in rows of its own length
            const long long row_stride = wl <= full ? win_stride : (static_cast<long long>(wl) + 3) & ~3LL;
            const int row_chunk = wl <= full ? chunk : static_cast<int>(std::min<size_t>(static_cast<size_t>(chunk), win_floats / static_cast<size_t>(row_stride)));
            A.window_len = wl; A.win_stride = row_stride;
            hipLaunchKernelGGL(stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListGroup);
            for (int first = 0; first < n_group; first += row_chunk) {
                const int nb = std::min(row_chunk, n_group - first);
                A.first = first; A.n_chunk = nb;
                const unsigned tgrid = static_cast<unsigned>((nb + 255) / 256);
                hipLaunchKernelGGL(stream_gather_kernel, dim3(static_cast<unsigned>(std::min((wl + 1023) / 1024, 64)), static_cast<unsigned>(nb)), dim3(256), 0, s, A);
                if (x) { M.S = A; hipLaunchKernelGGL(mcstream_params_kernel, dim3(tgrid), dim3(256), 0, s, M); }
                else hipLaunchKernelGGL(stream_params_kernel, dim3(tgrid), dim3(256), 0, s, A);
                HIP_TRY(h, hipGetLastError());
                // a window call may grow its workspaces: the first of the call finds the stream drained by the read above
                if (window_ran) HIP_TRY(h, hipStreamSynchronize(s));
                window_ran = true;
                int rc;
                if (ofdm)
                    rc = ria_gpu_rx_window_batch(control_h, h, W.win, row_stride, search_len, wl, nb, W.par, RIA_DECODE_FULL, W.wframes, min_row, W.wres,
                                                 reinterpret_cast<ria_acq_result*>(W.acq), nullptr, nullptr, s);
                else if (x)
                    rc = ria_gpu_mcdpsk_window_batch(h, cfg, W.win, row_stride, search_len, wl, nb, reinterpret_cast<const ria_mcdpsk_acq_params*>(W.par), xflags,
                                                     W.wframes, min_row, reinterpret_cast<ria_mcdpsk_window_result*>(W.wres), W.acq, nullptr, 0, x->pool,
                                                     XW.w_cache_id, XW.w_now_ms, XW.w_harq, x->interleaver_bits, s);
                else
                    rc = ria_gpu_mcdpsk_window_batch(h, cfg, W.win, row_stride, search_len, wl, nb, reinterpret_cast<const ria_mcdpsk_acq_params*>(W.par), mflags,
                                                     W.wframes, min_row, reinterpret_cast<ria_mcdpsk_window_result*>(W.wres), W.acq, nullptr, 0, nullptr,
                                                     nullptr, nullptr, nullptr, 0, s);
                if (rc != RIA_OK) return rc;
                if (x) hipLaunchKernelGGL(mcstream_apply_kernel, dim3(tgrid), dim3(256), 0, s, M);
                else hipLaunchKernelGGL(stream_apply_kernel, dim3(tgrid), dim3(256), 0, s, A);
                HIP_TRY(h, hipGetLastError());
            }
        }
        return RIA_OK;
    };
    // the streams still open (step 7. of a round); *n_open_out 0: the call is over
    auto list_open = [&](int bound, int* n_open_out) -> int {
        A.open = W.open;
        hipLaunchKernelGGL(stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListOpen);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, W.head, sizeof(StreamCtl), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n_open = static_cast<int>(mirror[0]);
        if (n_open < 0 || n_open > bound) return fail(h, RIA_ERR_HIP, "%s: the open list broke its bound (%d)", who, n_open);
        *n_open_out = n_open;
        A.n_open = n_open;
        return RIA_OK;
    };
    // the search part of the state back into the caller's records
    auto finish = [&]() -> int {
        if (x) {
            M.S = A;
            hipLaunchKernelGGL(mcstream_finish_kernel, dim3(sgrid), dim3(256), 0, s, M);
            HIP_TRY(h, hipGetLastError());
        }
        return RIA_OK;
    };

    if (x) {
        // 0. the up-front check - the search's domain, the pending fields', the cache ids across the whole call - read before
        //    anything is written; then the outputs cleared, and the streams that wait at a found sync in a round of their own
        if (x->pool) HIP_TRY(h, hipMemsetAsync(M.owner, 0xFF, static_cast<size_t>(M.n_caches) * sizeof(int32_t), s));
        HIP_TRY(h, hipMemsetAsync(XW.mctl, 0, sizeof(McStreamCtl), s));
        M.S = A;
        hipLaunchKernelGGL(mcstream_check_kernel, dim3(sgrid), dim3(256), 0, s, M);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, XW.mctl, sizeof(McStreamCtl), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const McStreamCtl mc = *reinterpret_cast<const McStreamCtl*>(mirror);
        if (mc.bad & kMcStreamBadDomain)
            return fail(h, RIA_ERR_INVALID, "%s: a stream's capture_len is above min(stride, 959999), its search state is outside the search's domain, its "
                                            "pending_total_cw is outside 0..255, or its pending fields do not lie in its capture; nothing was written", who);
        if (mc.bad & kMcStreamBadCache)
            return fail(h, RIA_ERR_INVALID, "%s: two streams of one call use one cache id, or an id is not below n_caches; nothing was written", who);
        if (mc.n_pending > static_cast<unsigned>(n_streams)) return fail(h, RIA_ERR_HIP, "%s: the pending count broke its bound (%u)", who, mc.n_pending);
        HIP_TRY(h, hipMemsetAsync(events_dev, 0, n * static_cast<size_t>(max_events) * sizeof(ria_stream_event), s));
        HIP_TRY(h, hipMemsetAsync(frames_dev, 0, n * static_cast<size_t>(max_events) * static_cast<size_t>(frame_row), s));
        if (x->harq) HIP_TRY(h, hipMemsetAsync(x->harq, 0, n * static_cast<size_t>(max_events) * sizeof(ria_mcdpsk_harq_result), s));
        hipLaunchKernelGGL(mcstream_init_kernel, dim3(sgrid), dim3(256), 0, s, M);
        if (mc.n_pending > 0) {
            hipLaunchKernelGGL(mcstream_pending_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, M);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(mirror, W.head, head_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipStreamSynchronize(s));
            const int n_fit = static_cast<int>(mirror[1]);
            if (n_fit < 0 || n_fit > static_cast<int>(mc.n_pending)) return fail(h, RIA_ERR_HIP, "%s: the pending list broke its bound (%d)", who, n_fit);
            M.pending_round = 1;
            if (n_fit > 0) if (int rc = run_windows(n_fit, kSrchMaxCapture)) return rc;
            M.pending_round = 0;
            int n_open = 0;
            if (int rc = list_open(n_streams, &n_open)) return rc;
            if (n_open == 0) return finish();
        }
        HIP_TRY(h, hipGetLastError());
    }
    for (int round = 0;; ++round) {
        if (round > max_events) return fail(h, RIA_ERR_HIP, "%s: round %d past max_events + 1", who, round + 1);
        // 1. the search on the open streams: in the first round all of them (x: all that do not wait at a sync), and nothing
        //    of this call is written before its domain check has passed
        if (int rc = search_impl(h, who, mode, flags, cfg, samples_dev, stride, capture_len_dev, A.n_open, A.open, state_dev, feed_step,
                                 max_invocations, W.sres, s)) return rc;
        if (round == 0 && !x) {
            HIP_TRY(h, hipMemsetAsync(events_dev, 0, n * static_cast<size_t>(max_events) * sizeof(ria_stream_event), s));
            HIP_TRY(h, hipMemsetAsync(frames_dev, 0, n * static_cast<size_t>(max_events) * static_cast<size_t>(frame_row), s));
            hipLaunchKernelGGL(stream_init_kernel, dim3(sgrid), dim3(256), 0, s, A);
        }
        // 2. the found streams and their window lengths
        hipLaunchKernelGGL(stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListFound);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, W.head, head_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n_found = static_cast<int>(mirror[1]);
        if (n_found < 0 || n_found > A.n_open) return fail(h, RIA_ERR_HIP, "%s: the found list broke its bound (%d)", who, n_found);
        if (n_found == 0) break;
        // 3.-6. one pass per distinct window length, ascending
        if (int rc = run_windows(n_found, full)) return rc;
        // 7. the streams still open
        int n_open = 0;
        if (int rc = list_open(n_found, &n_open)) return rc;
        if (n_open == 0) break;
    }
    return finish();
}

int ria_gpu_rx_stream_batch(ria_gpu_handle h, ria_gpu_handle control_h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                            const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                            ria_search_state* state_dev, int feed_step, int max_invocations, int max_events,
                            ria_stream_event* events_dev, uint8_t* frames_dev, int frame_row, ria_stream_result* result_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    return stream_impl(h, control_h, "ria_gpu_rx_stream_batch", mode, flags, cfg, samples_dev, stride, capture_len_dev, n_streams, state_dev, feed_step,
                       max_invocations, max_events, events_dev, frames_dev, frame_row, result_dev, stream, nullptr);
}

// ------------------------------------------------------------------------------------------------ the MC-DPSK stream loop: chase pool, interleaving, re-entry
static_assert(sizeof(ria_mcdpsk_stream_state) == 64 && offsetof(ria_mcdpsk_stream_state, pending_total_cw) == 32 &&
              offsetof(ria_mcdpsk_stream_state, pend_known_cfo_hz) == 48, "ria_gpu_mcdpsk_stream_batch record layout (include/ria_gpu.h)");
// the arguments ria_gpu_mcdpsk_stream_batch adds, checked on the host before anything is launched
static int mcstream_setup(ria_gpu_handle h, const char* who, int mode, uint32_t window_flags, int interleaver_bits, ria_chase_pool pool,
                          const int32_t* cache_id, const uint64_t* t0_ms) {
    if (mode != RIA_SEARCH_MCDPSK_ZC && mode != RIA_SEARCH_MCDPSK_CHIRP)
        return fail(h, RIA_ERR_INVALID, "%s: mode is RIA_SEARCH_MCDPSK_ZC or RIA_SEARCH_MCDPSK_CHIRP", who);
    if ((window_flags & ~static_cast<uint32_t>(RIA_MACQ_CHANNEL_INTERLEAVE)) != 0)
        return fail(h, RIA_ERR_INVALID, "%s: window_flags is 0 or RIA_MACQ_CHANNEL_INTERLEAVE", who);
    int step = 0;
    if ((window_flags & RIA_MACQ_CHANNEL_INTERLEAVE) && !macq_ci_step(interleaver_bits, &step))
        return fail(h, RIA_ERR_INVALID, "%s: interleaver_bits %d outside 1..648", who, interleaver_bits);
    if (pool && !chase_pool_alive(h, pool)) return fail(h, RIA_ERR_INVALID, "%s: the pool does not belong to this handle", who);
    if (pool && (!cache_id || !t0_ms)) return fail(h, RIA_ERR_INVALID, "%s: a pool needs cache_id_dev and t0_ms_dev", who);
    return RIA_OK;
}

int ria_gpu_mcdpsk_stream_batch(ria_gpu_handle h, int mode, uint32_t flags, uint32_t window_flags, int interleaver_bits, const ria_mcdpsk_config* cfg,
                                const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                                ria_mcdpsk_stream_state* state_dev, int feed_step, int max_invocations, int max_events,
                                ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* t0_ms_dev,
                                ria_stream_event* events_dev, uint8_t* frames_dev, int frame_row, ria_mcdpsk_harq_result* harq_dev,
                                ria_stream_result* result_dev, void* stream) {
    const char* who = "ria_gpu_mcdpsk_stream_batch";
    if (!h) return RIA_ERR_INVALID;
    if (int rc = mcstream_setup(h, who, mode, window_flags, interleaver_bits, pool, cache_id_dev, t0_ms_dev)) return rc;
    if (n_streams > 0 && !state_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    McStreamExt x{};
    x.mstate = state_dev; x.window_flags = window_flags; x.interleaver_bits = interleaver_bits;
    x.pool = pool; x.cache_id = cache_id_dev; x.t0_ms = t0_ms_dev; x.harq = harq_dev;
    return stream_impl(h, nullptr, who, mode, flags, cfg, samples_dev, stride, capture_len_dev, n_streams, nullptr, feed_step, max_invocations, max_events,
                       events_dev, frames_dev, frame_row, result_dev, stream, &x);
}

// One recording from host memory, as ria_gpu_rx_stream_host; the pool's caches stay on the device.
int ria_gpu_mcdpsk_stream_host(ria_gpu_handle h, int mode, uint32_t flags, uint32_t window_flags, int interleaver_bits, const ria_mcdpsk_config* cfg,
                               const float* samples_host, int n_samples, ria_mcdpsk_stream_state* state_host, int feed_step, int max_invocations,
                               int max_events, ria_chase_pool pool, int32_t cache_id, uint64_t t0_ms, ria_stream_event* events_out_host,
                               uint8_t* frames_out_host, int frame_row, ria_mcdpsk_harq_result* harq_out_host, ria_stream_result* result_out_host) {
    const char* who = "ria_gpu_mcdpsk_stream_host";
    if (!h) return RIA_ERR_INVALID;
    if (int rc = mcstream_setup(h, who, mode, window_flags, interleaver_bits, pool, &cache_id, &t0_ms)) return rc;
    int full = 0, first_frame = 0, min_row = 0;
    if (int rc = stream_setup(h, nullptr, who, mode, flags, cfg, max_events, frame_row, &full, &first_frame, &min_row)) return rc;
    if (n_samples < 0 || n_samples > kSrchMaxCapture || feed_step < 0 || max_invocations < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (0 <= n_samples <= 959999, feed_step >= 0, max_invocations >= 1)", who);
    if (!samples_host || !state_host || !events_out_host || !frames_out_host || !result_out_host) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    const int32_t cap = n_samples;
    const size_t ne = static_cast<size_t>(max_events);
    struct Stage { float* x; int32_t* cap; int32_t* id; uint64_t* t0; ria_mcdpsk_stream_state* st_in; ria_mcdpsk_stream_state* st; ria_stream_event* ev;
                   uint8_t* frames; ria_mcdpsk_harq_result* harq; ria_stream_result* res; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.x = c.in(static_cast<size_t>(std::max(n_samples, 1)), samples_host, static_cast<size_t>(n_samples));
        w.t0 = c.in(1, const_cast<const uint64_t*>(&t0_ms));
        w.cap = c.in(1, &cap); w.id = c.in(1, const_cast<const int32_t*>(&cache_id));
        w.st_in = c.in(1, const_cast<const ria_mcdpsk_stream_state*>(state_host));
        w.st = c.out(1, state_host); w.ev = c.out(ne, events_out_host); w.frames = c.out(ne * static_cast<size_t>(frame_row), frames_out_host);
        w.harq = c.out(ne, harq_out_host);
        w.res = c.out(1, result_out_host);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        int rc = ria_gpu_mcdpsk_stream_batch(h, mode, flags, window_flags, interleaver_bits, cfg, d.x, std::max(n_samples, 1), d.cap, 1, d.st_in, feed_step,
                                             max_invocations, max_events, pool, d.id, d.t0, d.ev, d.frames, frame_row, d.harq, d.res, s);
        if (rc != RIA_OK) return rc;
        if (hipMemcpyAsync(d.st, d.st_in, sizeof(ria_mcdpsk_stream_state), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(h, RIA_ERR_HIP, "%s: the state's copy failed", who);
        return static_cast<int>(RIA_OK); });
}

// One stream from host memory (the single-stream adaptor path): staged through the handle's pinned + device block on the
// handle's own stream, like ria_gpu_mcdpsk_window_host.  The state goes up as an input and comes back as an output.
int ria_gpu_rx_stream_host(ria_gpu_handle h, ria_gpu_handle control_h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                           const float* samples_host, int n_samples, ria_search_state* state_host, int feed_step, int max_invocations,
                           int max_events, ria_stream_event* events_out_host, uint8_t* frames_out_host, int frame_row,
                           ria_stream_result* result_out_host) {
    const char* who = "ria_gpu_rx_stream_host";
    if (!h) return RIA_ERR_INVALID;
    int full = 0, first_frame = 0, min_row = 0;
    if (int rc = stream_setup(h, control_h, who, mode, flags, cfg, max_events, frame_row, &full, &first_frame, &min_row)) return rc;
    if (n_samples < 0 || n_samples > kSrchMaxCapture || feed_step < 0 || max_invocations < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (0 <= n_samples <= 959999, feed_step >= 0, max_invocations >= 1)", who);
    if (!samples_host || !state_host || !events_out_host || !frames_out_host || !result_out_host) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    const int32_t cap = n_samples;
    const size_t ne = static_cast<size_t>(max_events);
    struct Stage { float* x; int32_t* cap; ria_search_state* st_in; ria_search_state* st; ria_stream_event* ev; uint8_t* frames; ria_stream_result* res; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.x = c.in(static_cast<size_t>(std::max(n_samples, 1)), samples_host, static_cast<size_t>(n_samples));
        w.cap = c.in(1, &cap); w.st_in = c.in(1, const_cast<const ria_search_state*>(state_host));
        w.st = c.out(1, state_host); w.ev = c.out(ne, events_out_host); w.frames = c.out(ne * static_cast<size_t>(frame_row), frames_out_host);
        w.res = c.out(1, result_out_host);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        int rc = ria_gpu_rx_stream_batch(h, control_h, mode, flags, cfg, d.x, std::max(n_samples, 1), d.cap, 1, d.st_in, feed_step, max_invocations,
                                         max_events, d.ev, d.frames, frame_row, d.res, s);
        if (rc != RIA_OK) return rc;
        if (hipMemcpyAsync(d.st, d.st_in, sizeof(ria_search_state), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(h, RIA_ERR_HIP, "%s: the state's copy failed", who);
        return static_cast<int>(RIA_OK); });
}

// ------------------------------------------------------------------------------------------------ the stream loop on the ring
static_assert(sizeof(ria_ring_stream_result) == 88 && offsetof(ria_ring_stream_result, invocations) == 16 &&
              offsetof(ria_ring_stream_result, overflow_dropped) == 64 && offsetof(ria_ring_stream_result, cursor_inits) == 80 &&
              RIA_STREAM_SPAN_LOST == kStreamSpanLost, "ria_gpu_rx_ring_batch record layout (include/ria_gpu.h)");
struct RingStreamWs {
    uint32_t* head;               // StreamCtl (4 words), found [n], found_len [n]: what the host reads per round, in one copy
    uint32_t *open, *group;
    ria_ring_search_result* sres;
    float* win;
    ria_acq_params* par;          // either parameter record
    ria_window_result* wres;      // either window result
    ria_mcdpsk_acq_result* acq;   // either acquire result
    uint8_t* wframes;
};
static RingStreamWs ring_stream_carve(Carver& c, size_t n, size_t chunk, size_t win_floats, size_t wframe_row) {
    RingStreamWs w;
    w.head = c.take<uint32_t>(4 + 2 * n);
    w.open = c.take<uint32_t>(n);
    w.group = c.take<uint32_t>(n);
    w.sres = c.take<ria_ring_search_result>(n);
    w.win = c.take<float>(win_floats);
    w.par = c.take<ria_acq_params>(chunk);
    w.wres = c.take<ria_window_result>(chunk);
    w.acq = c.take<ria_mcdpsk_acq_result>(chunk);
    w.wframes = c.take<uint8_t>(chunk * wframe_row);
    return w;
}

int ria_gpu_rx_ring_batch(ria_gpu_handle h, ria_gpu_handle control_h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                          const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                          ria_ring_state* state_dev, int feed_step, int max_invocations, int max_events,
                          ria_stream_event* events_dev, uint8_t* frames_dev, int frame_row, ria_ring_stream_result* result_dev, void* stream) {
    const char* who = "ria_gpu_rx_ring_batch";
    if (!h) return RIA_ERR_INVALID;
    int full = 0, first_frame = 0, min_row = 0;
    if (int rc = stream_setup(h, control_h, who, mode, flags, cfg, max_events, frame_row, &full, &first_frame, &min_row)) return rc;
    if (full > kSrchRing - 1) return fail(h, RIA_ERR_INVALID, "%s: the window of this configuration (%d samples) is longer than 959999", who, full);
    if (n_streams < 0 || stride < 0 || feed_step < 0 || max_invocations < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (n_streams >= 0, stride >= 0, feed_step >= 0, max_invocations >= 1)", who);
    if (n_streams == 0) return RIA_OK;
    if (!samples_dev || !capture_len_dev || !state_dev || !events_dev || !frames_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool ofdm = mode == RIA_SEARCH_OFDM_LTS;
    const size_t n = static_cast<size_t>(n_streams);
    const int search_len = srch_min_search(mode);
    const long long win_stride = (static_cast<long long>(full) + 3) & ~3LL;          // rows of the window workspace start on 16 bytes
    int chunk = static_cast<int>(std::min<size_t>(n, std::max<size_t>(1, (size_t(256) << 20) / (static_cast<size_t>(win_stride) * sizeof(float)))));
    chunk = std::min(chunk, 65535);                    // the gather's grid y extent
    auto carve = [&](Carver& c) { return ring_stream_carve(c, n, static_cast<size_t>(chunk), static_cast<size_t>(chunk) * static_cast<size_t>(win_stride), static_cast<size_t>(min_row)); };
    const size_t head_bytes = (4 + 2 * n) * sizeof(uint32_t);
    HIP_TRY(h, h->d_stream_ws.reserve(carved_size(carve), &s));
    HIP_TRY(h, h->p_stream_ctl.reserve(head_bytes));
    const RingStreamWs W = carve_at(h->d_stream_ws.as<>(), carve);
    uint32_t* mirror = h->p_stream_ctl.as<uint32_t>();

    RingStreamArgs A{};
    A.samples = samples_dev; A.stride = stride; A.capture_len = capture_len_dev; A.state = state_dev; A.sres = W.sres;
    A.res = result_dev; A.events = events_dev; A.frames = frames_dev; A.frame_row = frame_row;
    A.n_streams = n_streams; A.mode = mode; A.family = ofdm ? kStreamOfdm : kStreamMcdpsk; A.full = full; A.first_frame = first_frame;
    A.max_events = max_events;
    A.ctl = reinterpret_cast<StreamCtl*>(W.head); A.found = W.head + 4; A.found_len = reinterpret_cast<int32_t*>(W.head + 4 + n);
    A.open = nullptr; A.group = W.group; A.n_open = n_streams;
    A.win = W.win; A.win_stride = win_stride; A.wframes = W.wframes; A.wframe_row = min_row;
    if (ofdm) { A.par = W.par; A.wres = W.wres; }
    else { A.mpar = reinterpret_cast<ria_mcdpsk_acq_params*>(W.par); A.mres = reinterpret_cast<const ria_mcdpsk_window_result*>(W.wres); A.macq = W.acq; }
    const uint32_t mflags = mode == RIA_SEARCH_MCDPSK_CHIRP ? (RIA_MACQ_SYNC_CHIRP | ((flags & RIA_SEARCH_CONNECTED) ? 0u : RIA_MACQ_DISCONNECTED)) : 0u;
    const unsigned sgrid = static_cast<unsigned>((n_streams + 255) / 256);
    bool window_ran = false;

    for (int round = 0;; ++round) {
        if (round > max_events) return fail(h, RIA_ERR_HIP, "%s: round %d past max_events + 1", who, round + 1);
        // 1. the ring search on the open streams: in the first round all of them, and nothing of this call is written before
        //    its domain check has passed
        if (int rc = ring_search_impl(h, who, mode, flags, cfg, samples_dev, stride, capture_len_dev, A.n_open, A.open, state_dev, feed_step,
                                      max_invocations, W.sres, s)) return rc;
        if (round == 0) {
            HIP_TRY(h, hipMemsetAsync(events_dev, 0, n * static_cast<size_t>(max_events) * sizeof(ria_stream_event), s));
            HIP_TRY(h, hipMemsetAsync(frames_dev, 0, n * static_cast<size_t>(max_events) * static_cast<size_t>(frame_row), s));
            hipLaunchKernelGGL(ring_stream_init_kernel, dim3(sgrid), dim3(256), 0, s, A);
        }
        // 2. the found streams and their window lengths
        hipLaunchKernelGGL(ring_stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListFound);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, W.head, head_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n_found = static_cast<int>(mirror[1]);
        if (n_found < 0 || n_found > A.n_open) return fail(h, RIA_ERR_HIP, "%s: the found list broke its bound (%d)", who, n_found);
        if (n_found == 0) break;
        A.n_found = n_found;
        std::vector<int> lens(mirror + 4 + n, mirror + 4 + n + n_found);
        std::sort(lens.begin(), lens.end());
        // 3.-6. one pass per distinct window length, ascending
        for (size_t at = 0; at < lens.size();) {
            const int wl = lens[at];
            size_t end = at;
            while (end < lens.size() && lens[end] == wl) ++end;
            const int n_group = static_cast<int>(end - at);
            at = end;
            if (wl < search_len || wl > full) return fail(h, RIA_ERR_HIP, "%s: a window of %d samples, outside %d..%d", who, wl, search_len, full);
            A.window_len = wl;
            hipLaunchKernelGGL(ring_stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListGroup);
            for (int first = 0; first < n_group; first += chunk) {
                const int nb = std::min(chunk, n_group - first);
                A.first = first; A.n_chunk = nb;
                const unsigned tgrid = static_cast<unsigned>((nb + 255) / 256);
                hipLaunchKernelGGL(ring_stream_gather_kernel, dim3(static_cast<unsigned>(std::min((wl + 1023) / 1024, 64)), static_cast<unsigned>(nb)), dim3(256), 0, s, A);
                hipLaunchKernelGGL(ring_stream_params_kernel, dim3(tgrid), dim3(256), 0, s, A);
                HIP_TRY(h, hipGetLastError());
                // a window call may grow its workspaces: the first of the call finds the stream drained by the read above
                if (window_ran) HIP_TRY(h, hipStreamSynchronize(s));
                window_ran = true;
                int rc;
                if (ofdm)
                    rc = ria_gpu_rx_window_batch(control_h, h, W.win, win_stride, search_len, wl, nb, W.par, RIA_DECODE_FULL, W.wframes, min_row, W.wres,
                                                 reinterpret_cast<ria_acq_result*>(W.acq), nullptr, nullptr, s);
                else
                    rc = ria_gpu_mcdpsk_window_batch(h, cfg, W.win, win_stride, search_len, wl, nb, reinterpret_cast<const ria_mcdpsk_acq_params*>(W.par), mflags,
                                                     W.wframes, min_row, reinterpret_cast<ria_mcdpsk_window_result*>(W.wres), W.acq, nullptr, 0, nullptr,
                                                     nullptr, nullptr, nullptr, 0, s);
                if (rc != RIA_OK) return rc;
                hipLaunchKernelGGL(ring_stream_apply_kernel, dim3(tgrid), dim3(256), 0, s, A);
                HIP_TRY(h, hipGetLastError());
            }
        }
        // 7. the streams still open
        A.open = W.open;
        hipLaunchKernelGGL(ring_stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListOpen);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, W.head, sizeof(StreamCtl), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n_open = static_cast<int>(mirror[0]);
        if (n_open < 0 || n_open > A.n_open) return fail(h, RIA_ERR_HIP, "%s: the open list broke its bound (%d)", who, n_open);
        if (n_open == 0) break;
        A.n_open = n_open;
    }
    return RIA_OK;
}

// a recording of n_samples (checked by the caller) from host memory into the handle's device buffer, in pieces through the
// pinned block; *rec_out: where it lies.  The handle's stream is idle when this returns.
static int ring_stage_recording(ria_gpu_handle h, const float* samples_host, int n_samples, float** rec_out) {
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t piece = size_t(1) << 18;                            // samples per piece: 1 MiB of the pinned block
    if (int rc = ensure_host_stage(h, piece * sizeof(float))) return rc;
    hipStream_t hs = h->hstream;
    HIP_TRY(h, h->d_ring_rec.reserve(static_cast<size_t>(std::max(n_samples, 1)) * sizeof(float), &hs));
    float* rec = h->d_ring_rec.as<float>();
    for (size_t at = 0; at < static_cast<size_t>(n_samples); at += piece) {
        const size_t cnt = std::min(piece, static_cast<size_t>(n_samples) - at);
        std::memcpy(h->p_hstage.as<unsigned char>(), samples_host + at, cnt * sizeof(float));
        HIP_TRY(h, hipMemcpyAsync(rec + at, h->p_hstage.as<unsigned char>(), cnt * sizeof(float), hipMemcpyHostToDevice, hs));
        HIP_TRY(h, hipStreamSynchronize(hs));                        // the pinned block is free for the next piece
    }
    *rec_out = rec;
    return RIA_OK;
}

// One recording of any length in the domain from host memory.  It goes up in pieces through the handle's pinned block into
// a device buffer the handle owns, grown before anything is in flight; the small records are staged like
// ria_gpu_rx_stream_host's.
int ria_gpu_rx_ring_host(ria_gpu_handle h, ria_gpu_handle control_h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                         const float* samples_host, int n_samples, ria_ring_state* state_host, int feed_step, int max_invocations,
                         int max_events, ria_stream_event* events_out_host, uint8_t* frames_out_host, int frame_row,
                         ria_ring_stream_result* result_out_host) {
    const char* who = "ria_gpu_rx_ring_host";
    if (!h) return RIA_ERR_INVALID;
    int full = 0, first_frame = 0, min_row = 0;
    if (int rc = stream_setup(h, control_h, who, mode, flags, cfg, max_events, frame_row, &full, &first_frame, &min_row)) return rc;
    if (full > kSrchRing - 1) return fail(h, RIA_ERR_INVALID, "%s: the window of this configuration (%d samples) is longer than 959999", who, full);
    if (n_samples < 0 || n_samples > kRingMaxCapture || feed_step < 0 || max_invocations < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (0 <= n_samples <= 2^31 - 1 - 960000, feed_step >= 0, max_invocations >= 1)", who);
    if (!samples_host || !state_host || !events_out_host || !frames_out_host || !result_out_host) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    float* rec = nullptr;
    if (int rc = ring_stage_recording(h, samples_host, n_samples, &rec)) return rc;
    const int32_t cap = n_samples;
    const size_t ne = static_cast<size_t>(max_events);
    struct Stage { int32_t* cap; ria_ring_state* st_in; ria_ring_state* st; ria_stream_event* ev; uint8_t* frames; ria_ring_stream_result* res; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.cap = c.in(1, &cap); w.st_in = c.in(1, const_cast<const ria_ring_state*>(state_host));
        w.st = c.out(1, state_host); w.ev = c.out(ne, events_out_host); w.frames = c.out(ne * static_cast<size_t>(frame_row), frames_out_host);
        w.res = c.out(1, result_out_host);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        int rc = ria_gpu_rx_ring_batch(h, control_h, mode, flags, cfg, rec, std::max(n_samples, 1), d.cap, 1, d.st_in, feed_step, max_invocations,
                                       max_events, d.ev, d.frames, frame_row, d.res, s);
        if (rc != RIA_OK) return rc;
        if (hipMemcpyAsync(d.st, d.st_in, sizeof(ria_ring_state), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(h, RIA_ERR_HIP, "%s: the state's copy failed", who);
        return static_cast<int>(RIA_OK); });
}

// ------------------------------------------------------------------------------------------------ the MC-DPSK loop on the ring: chase pool, interleaving, re-entry
static_assert(sizeof(ria_mcdpsk_ring_state) == 80 && offsetof(ria_mcdpsk_ring_state, pending_total_cw) == 48 &&
              offsetof(ria_mcdpsk_ring_state, pend_search_start) == 56 && offsetof(ria_mcdpsk_ring_state, pend_known_cfo_hz) == 64,
              "ria_gpu_mcdpsk_ring_batch record layout (include/ria_gpu.h)");
struct McRingWs {
    McStreamCtl* mctl;
    ria_ring_state* rstate;       // [n] the `ring` part of the caller's records, contiguous: what the ring search reads and writes
    int32_t* w_cache_id; uint64_t* w_now_ms; ria_mcdpsk_harq_result* w_harq;   // [chunk]
};
static McRingWs mcring_carve(Carver& c, size_t n, size_t chunk) {
    McRingWs w;
    w.mctl = c.take<McStreamCtl>(1);
    w.rstate = c.take<ria_ring_state>(n);
    w.w_cache_id = c.take<int32_t>(chunk);
    w.w_now_ms = c.take<uint64_t>(chunk);
    w.w_harq = c.take<ria_mcdpsk_harq_result>(chunk);
    return w;
}

int ria_gpu_mcdpsk_ring_batch(ria_gpu_handle h, int mode, uint32_t flags, uint32_t window_flags, int interleaver_bits, const ria_mcdpsk_config* cfg,
                              const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                              ria_mcdpsk_ring_state* state_dev, int feed_step, int max_invocations, int max_events,
                              ria_chase_pool pool, const int32_t* cache_id_dev, const uint64_t* t0_ms_dev,
                              ria_stream_event* events_dev, uint8_t* frames_dev, int frame_row, ria_mcdpsk_harq_result* harq_dev,
                              ria_ring_stream_result* result_dev, void* stream) {
    const char* who = "ria_gpu_mcdpsk_ring_batch";
    if (!h) return RIA_ERR_INVALID;
    if (int rc = mcstream_setup(h, who, mode, window_flags, interleaver_bits, pool, cache_id_dev, t0_ms_dev)) return rc;
    int full = 0, first_frame = 0, min_row = 0;
    if (int rc = stream_setup(h, nullptr, who, mode, flags, cfg, max_events, frame_row, &full, &first_frame, &min_row)) return rc;
    if (full > kMcRingMaxSpan) return fail(h, RIA_ERR_INVALID, "%s: the window of this configuration (%d samples) is longer than 959999", who, full);
    if (n_streams < 0 || stride < 0 || feed_step < 0 || max_invocations < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (n_streams >= 0, stride >= 0, feed_step >= 0, max_invocations >= 1)", who);
    if (n_streams == 0) return RIA_OK;
    if (!samples_dev || !capture_len_dev || !state_dev || !events_dev || !frames_dev || !result_dev) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = static_cast<size_t>(n_streams);
    const int search_len = srch_min_search(mode);
    const long long win_stride = (static_cast<long long>(full) + 3) & ~3LL;          // rows of the window workspace start on 16 bytes
    int chunk = static_cast<int>(std::min<size_t>(n, std::max<size_t>(1, (size_t(256) << 20) / (static_cast<size_t>(win_stride) * sizeof(float)))));
    chunk = std::min(chunk, 65535);                    // the gather's grid y extent
    // a re-entered window runs to the end of the span it waited for, up to 959 999 samples: room for one such row at least
    const size_t win_floats = std::max<size_t>(static_cast<size_t>(chunk) * static_cast<size_t>(win_stride), static_cast<size_t>(kSrchRing));
    auto carve = [&](Carver& c) {
        std::pair<RingStreamWs, McRingWs> w;
        w.first = ring_stream_carve(c, n, static_cast<size_t>(chunk), win_floats, static_cast<size_t>(min_row));
        w.second = mcring_carve(c, n, static_cast<size_t>(chunk));
        return w;
    };
    const size_t head_bytes = (4 + 2 * n) * sizeof(uint32_t);
    HIP_TRY(h, h->d_stream_ws.reserve(carved_size(carve), &s));
    HIP_TRY(h, h->p_stream_ctl.reserve(std::max(head_bytes, sizeof(McStreamCtl))));
    const auto carved = carve_at(h->d_stream_ws.as<>(), carve);
    const RingStreamWs& W = carved.first;
    const McRingWs& XW = carved.second;
    uint32_t* mirror = h->p_stream_ctl.as<uint32_t>();

    McRingArgs M{};
    RingStreamArgs& A = M.S;
    A.samples = samples_dev; A.stride = stride; A.capture_len = capture_len_dev; A.state = XW.rstate; A.sres = W.sres;
    A.res = result_dev; A.events = events_dev; A.frames = frames_dev; A.frame_row = frame_row;
    A.n_streams = n_streams; A.mode = mode; A.family = kStreamMcdpsk; A.full = full; A.first_frame = first_frame;
    A.max_events = max_events;
    A.ctl = reinterpret_cast<StreamCtl*>(W.head); A.found = W.head + 4; A.found_len = reinterpret_cast<int32_t*>(W.head + 4 + n);
    A.open = nullptr; A.group = W.group; A.n_open = n_streams;
    A.win = W.win; A.win_stride = win_stride; A.wframes = W.wframes; A.wframe_row = min_row;
    A.mpar = reinterpret_cast<ria_mcdpsk_acq_params*>(W.par); A.mres = reinterpret_cast<const ria_mcdpsk_window_result*>(W.wres); A.macq = W.acq;
    M.mstate = state_dev; M.harq = harq_dev; M.sres_w = W.sres; M.mctl = XW.mctl;
    M.sample_rate = h->cfg.sample_rate; M.search_len = search_len;
    M.w_cache_id = XW.w_cache_id; M.w_now_ms = XW.w_now_ms; M.w_harq = XW.w_harq;
    if (pool) { M.cache_id = cache_id_dev; M.t0_ms = t0_ms_dev; M.owner = pool->d_owner.as<int32_t>(); M.n_caches = pool->cfg.n_caches; }
    const uint32_t xflags = (mode == RIA_SEARCH_MCDPSK_CHIRP ? (RIA_MACQ_SYNC_CHIRP | ((flags & RIA_SEARCH_CONNECTED) ? 0u : RIA_MACQ_DISCONNECTED)) : 0u) |
                            window_flags;
    const unsigned sgrid = static_cast<unsigned>((n_streams + 255) / 256);
    bool window_ran = false;

    // the found list as the host read it (n_found streams, their window lengths behind mirror[4 + n]): one pass per distinct
    // window length, ascending (steps 2.-6. of a round)
    auto run_windows = [&](int n_found, int longest) -> int {
        A.n_found = n_found;
        std::vector<int> lens(mirror + 4 + n, mirror + 4 + n + n_found);
        std::sort(lens.begin(), lens.end());
        for (size_t at = 0; at < lens.size();) {
            const int wl = lens[at];
            size_t end = at;
            while (end < lens.size() && lens[end] == wl) ++end;
            const int n_group = static_cast<int>(end - at);
            at = end;
            if (wl < search_len || wl > longest) return fail(h, RIA_ERR_HIP, "%s: a window of %d samples, outside %d..%d", who, wl, search_len, longest);
            // windows up to `full` lie in rows of win_stride; a longer one (re-entry only) in rows of its own length
            const long long row_stride = wl <= full ? win_stride : (static_cast<long long>(wl) + 3) & ~3LL;
            const int row_chunk = wl <= full ? chunk : static_cast<int>(std::min<size_t>(static_cast<size_t>(chunk), win_floats / static_cast<size_t>(row_stride)));
            A.window_len = wl; A.win_stride = row_stride;
            hipLaunchKernelGGL(ring_stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListGroup);
            for (int first = 0; first < n_group; first += row_chunk) {
                const int nb = std::min(row_chunk, n_group - first);
                A.first = first; A.n_chunk = nb;
                const unsigned tgrid = static_cast<unsigned>((nb + 255) / 256);
                hipLaunchKernelGGL(mcring_gather_kernel, dim3(static_cast<unsigned>(std::min((wl + 1023) / 1024, 64)), static_cast<unsigned>(nb)), dim3(256), 0, s, M);
                hipLaunchKernelGGL(mcring_params_kernel, dim3(tgrid), dim3(256), 0, s, M);
                HIP_TRY(h, hipGetLastError());
                // a window call may grow its workspaces: the first of the call finds the stream drained by the read above
                if (window_ran) HIP_TRY(h, hipStreamSynchronize(s));
                window_ran = true;
                if (int rc = ria_gpu_mcdpsk_window_batch(h, cfg, W.win, row_stride, search_len, wl, nb, reinterpret_cast<const ria_mcdpsk_acq_params*>(W.par), xflags,
                                                         W.wframes, min_row, reinterpret_cast<ria_mcdpsk_window_result*>(W.wres), W.acq, nullptr, 0, pool,
                                                         XW.w_cache_id, XW.w_now_ms, XW.w_harq, interleaver_bits, s)) return rc;
                hipLaunchKernelGGL(mcring_apply_kernel, dim3(tgrid), dim3(256), 0, s, M);
                HIP_TRY(h, hipGetLastError());
            }
        }
        return RIA_OK;
    };
    // the streams still open (step 7. of a round); *n_open_out 0: the call is over
    auto list_open = [&](int bound, int* n_open_out) -> int {
        A.open = W.open;
        hipLaunchKernelGGL(ring_stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListOpen);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, W.head, sizeof(StreamCtl), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n_open = static_cast<int>(mirror[0]);
        if (n_open < 0 || n_open > bound) return fail(h, RIA_ERR_HIP, "%s: the open list broke its bound (%d)", who, n_open);
        *n_open_out = n_open;
        A.n_open = n_open;
        return RIA_OK;
    };
    // the `ring` part of the state back into the caller's records
    auto finish = [&]() -> int {
        hipLaunchKernelGGL(mcring_finish_kernel, dim3(sgrid), dim3(256), 0, s, M);
        HIP_TRY(h, hipGetLastError());
        return RIA_OK;
    };

    // 0. the up-front check - the ring search's domain, the pending fields', the cache ids across the whole call - read before
    //    anything is written; then the outputs cleared, and the streams that wait at a found sync in a round of their own
    if (pool) HIP_TRY(h, hipMemsetAsync(M.owner, 0xFF, static_cast<size_t>(M.n_caches) * sizeof(int32_t), s));
    HIP_TRY(h, hipMemsetAsync(XW.mctl, 0, sizeof(McStreamCtl), s));
    hipLaunchKernelGGL(mcring_check_kernel, dim3(sgrid), dim3(256), 0, s, M);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(mirror, XW.mctl, sizeof(McStreamCtl), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    const McStreamCtl mc = *reinterpret_cast<const McStreamCtl*>(mirror);
    if (mc.bad & kMcStreamBadDomain)
        return fail(h, RIA_ERR_INVALID, "%s: a stream's capture_len is above min(stride, 2^31 - 1 - 960000), its ring state is outside the ring search's domain, "
                                        "its pending_total_cw is outside 0..255, or its pending fields do not lie in its capture, span more than 959999 "
                                        "samples or name a window the ring no longer holds; nothing was written", who);
    if (mc.bad & kMcStreamBadCache)
        return fail(h, RIA_ERR_INVALID, "%s: two streams of one call use one cache id, or an id is not below n_caches; nothing was written", who);
    if (mc.n_pending > static_cast<unsigned>(n_streams)) return fail(h, RIA_ERR_HIP, "%s: the pending count broke its bound (%u)", who, mc.n_pending);
    HIP_TRY(h, hipMemsetAsync(events_dev, 0, n * static_cast<size_t>(max_events) * sizeof(ria_stream_event), s));
    HIP_TRY(h, hipMemsetAsync(frames_dev, 0, n * static_cast<size_t>(max_events) * static_cast<size_t>(frame_row), s));
    if (harq_dev) HIP_TRY(h, hipMemsetAsync(harq_dev, 0, n * static_cast<size_t>(max_events) * sizeof(ria_mcdpsk_harq_result), s));
    hipLaunchKernelGGL(mcring_init_kernel, dim3(sgrid), dim3(256), 0, s, M);
    if (mc.n_pending > 0) {
        hipLaunchKernelGGL(mcring_pending_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, M);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, W.head, head_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n_fit = static_cast<int>(mirror[1]);
        if (n_fit < 0 || n_fit > static_cast<int>(mc.n_pending)) return fail(h, RIA_ERR_HIP, "%s: the pending list broke its bound (%d)", who, n_fit);
        M.pending_round = 1;
        if (n_fit > 0) if (int rc = run_windows(n_fit, kMcRingMaxSpan)) return rc;
        M.pending_round = 0;
        int n_open = 0;
        if (int rc = list_open(n_streams, &n_open)) return rc;
        if (n_open == 0) return finish();
    }
    HIP_TRY(h, hipGetLastError());
    for (int round = 0;; ++round) {
        if (round > max_events) return fail(h, RIA_ERR_HIP, "%s: round %d past max_events + 1", who, round + 1);
        // 1. the ring search on the open streams: all that do not wait at a sync
        if (int rc = ring_search_impl(h, who, mode, flags, cfg, samples_dev, stride, capture_len_dev, A.n_open, A.open, XW.rstate, feed_step,
                                      max_invocations, W.sres, s)) return rc;
        // 2. the found streams and their window lengths
        hipLaunchKernelGGL(ring_stream_list_kernel, dim3(1), dim3(kAcqScanThreads), 0, s, A, kStreamListFound);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(mirror, W.head, head_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const int n_found = static_cast<int>(mirror[1]);
        if (n_found < 0 || n_found > A.n_open) return fail(h, RIA_ERR_HIP, "%s: the found list broke its bound (%d)", who, n_found);
        if (n_found == 0) break;
        // 3.-6. one pass per distinct window length, ascending
        if (int rc = run_windows(n_found, full)) return rc;
        // 7. the streams still open
        int n_open = 0;
        if (int rc = list_open(n_found, &n_open)) return rc;
        if (n_open == 0) break;
    }
    return finish();
}

// One recording of any length in the domain from host memory, as ria_gpu_rx_ring_host; the pool's caches stay on the device.
int ria_gpu_mcdpsk_ring_host(ria_gpu_handle h, int mode, uint32_t flags, uint32_t window_flags, int interleaver_bits, const ria_mcdpsk_config* cfg,
                             const float* samples_host, int n_samples, ria_mcdpsk_ring_state* state_host, int feed_step, int max_invocations,
                             int max_events, ria_chase_pool pool, int32_t cache_id, uint64_t t0_ms, ria_stream_event* events_out_host,
                             uint8_t* frames_out_host, int frame_row, ria_mcdpsk_harq_result* harq_out_host, ria_ring_stream_result* result_out_host) {
    const char* who = "ria_gpu_mcdpsk_ring_host";
    if (!h) return RIA_ERR_INVALID;
    if (int rc = mcstream_setup(h, who, mode, window_flags, interleaver_bits, pool, &cache_id, &t0_ms)) return rc;
    int full = 0, first_frame = 0, min_row = 0;
    if (int rc = stream_setup(h, nullptr, who, mode, flags, cfg, max_events, frame_row, &full, &first_frame, &min_row)) return rc;
    if (full > kMcRingMaxSpan) return fail(h, RIA_ERR_INVALID, "%s: the window of this configuration (%d samples) is longer than 959999", who, full);
    if (n_samples < 0 || n_samples > kRingMaxCapture || feed_step < 0 || max_invocations < 1)
        return fail(h, RIA_ERR_INVALID, "%s: bad argument (0 <= n_samples <= 2^31 - 1 - 960000, feed_step >= 0, max_invocations >= 1)", who);
    if (!samples_host || !state_host || !events_out_host || !frames_out_host || !result_out_host) return fail(h, RIA_ERR_INVALID, "%s: null pointer", who);
    float* rec = nullptr;
    if (int rc = ring_stage_recording(h, samples_host, n_samples, &rec)) return rc;
    const int32_t cap = n_samples;
    const size_t ne = static_cast<size_t>(max_events);
    struct Stage { int32_t* cap; int32_t* id; uint64_t* t0; ria_mcdpsk_ring_state* st_in; ria_mcdpsk_ring_state* st; ria_stream_event* ev;
                   uint8_t* frames; ria_mcdpsk_harq_result* harq; ria_ring_stream_result* res; };
    auto carve = [&](StageCarver& c) {
        Stage w;
        w.t0 = c.in(1, const_cast<const uint64_t*>(&t0_ms));
        w.st_in = c.in(1, const_cast<const ria_mcdpsk_ring_state*>(state_host));
        w.cap = c.in(1, &cap); w.id = c.in(1, const_cast<const int32_t*>(&cache_id));
        w.st = c.out(1, state_host); w.ev = c.out(ne, events_out_host); w.frames = c.out(ne * static_cast<size_t>(frame_row), frames_out_host);
        w.harq = c.out(ne, harq_out_host);
        w.res = c.out(1, result_out_host);
        return w;
    };
    return host_staged(h, carve, [&](const Stage& d, hipStream_t s) {
        int rc = ria_gpu_mcdpsk_ring_batch(h, mode, flags, window_flags, interleaver_bits, cfg, rec, std::max(n_samples, 1), d.cap, 1, d.st_in, feed_step,
                                           max_invocations, max_events, pool, d.id, d.t0, d.ev, d.frames, frame_row, d.harq, d.res, s);
        if (rc != RIA_OK) return rc;
        if (hipMemcpyAsync(d.st, d.st_in, sizeof(ria_mcdpsk_ring_state), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(h, RIA_ERR_HIP, "%s: the state's copy failed", who);
        return static_cast<int>(RIA_OK); });
}

int ria_gpu_chase_combine_batch(ria_gpu_handle h, float* acc_dev, int32_t* count_dev, const uint8_t* decoded_dev,
                                const float* soft_dev, int n_cw, uint8_t* stored_out_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_cw == 0) return RIA_OK;
    if (!acc_dev || !count_dev || !soft_dev || n_cw < 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_chase_combine_batch: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(chase_combine_kernel, dim3(n_cw), dim3(256), 0, static_cast<hipStream_t>(stream), acc_dev, count_dev, decoded_dev,
                       soft_dev, n_cw, stored_out_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

void ria_link_recommend(float snr_db, float fading_index, ria_link_recommendation* out) { if (out) *out = recommend_waveform_and_rate(snr_db, fading_index); }
void ria_link_data_mode(float snr_db, int waveform, float fading_index, ria_link_recommendation* out) {
    if (!out) return;
    *out = recommend_data_mode(snr_db, waveform, fading_index);
    if (waveform != kWaveMcDpsk) out->estimated_throughput_bps = 0.0f;
}
int ria_link_ofdm_code_rate(float snr_db, float fading_index) { return select_ofdm_code_rate(snr_db, fading_index); }
int ria_link_cap_initial_rate(float snr_db, float fading_index, int candidate_rate) { return cap_initial_ofdm_rate(snr_db, fading_index, candidate_rate); }

int ria_gpu_burst_deinterleave_batch(ria_gpu_handle h, const float* physical_llr_dev, int llr_stride, int burst_frames,
                                     int n_groups, float* logical_llr_out_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_groups == 0 || burst_frames == 0) return RIA_OK;
    if (!physical_llr_dev || !logical_llr_out_dev || physical_llr_dev == logical_llr_out_dev || llr_stride < 2592 || burst_frames < 0 || n_groups < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_burst_deinterleave_batch: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    const int total = n_groups * burst_frames * 324;
    hipLaunchKernelGGL(burst_deinterleave_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), physical_llr_dev,
                       llr_stride, burst_frames, n_groups, logical_llr_out_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}
int ria_gpu_burst_interleave_batch(ria_gpu_handle h, const uint8_t* logical_bytes_dev, int burst_frames, int n_groups,
                                   uint8_t* physical_bytes_out_dev, void* stream) {
    if (!h) return RIA_ERR_INVALID;
    if (n_groups == 0 || burst_frames == 0) return RIA_OK;
    if (!logical_bytes_dev || !physical_bytes_out_dev || logical_bytes_dev == physical_bytes_out_dev || burst_frames < 0 || n_groups < 0)
        return fail(h, RIA_ERR_INVALID, "ria_gpu_burst_interleave_batch: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    const int total = n_groups * burst_frames * 324;
    hipLaunchKernelGGL(burst_interleave_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), logical_bytes_dev,
                       burst_frames, n_groups, physical_bytes_out_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

int ria_gpu_ldpc_encode_host(ria_gpu_handle h, const uint8_t* info, int n_cw, uint8_t* coded_out) {
    if (!h || !info || !coded_out || n_cw < 0) return RIA_ERR_INVALID;
    const LdpcCode& c = h->code;
    const int kb = (c.k + 7) / 8;
    std::vector<uint8_t> bits(648);
    for (int w = 0; w < n_cw; ++w) {
        const uint8_t* in = info + static_cast<size_t>(w) * kb;
        for (int j = 0; j < c.k; ++j) bits[j] = (in[j >> 3] >> (7 - (j & 7))) & 1;
        for (int i = 0; i < c.m; ++i) {   // H = [H_data | I]: parity i = XOR of the information bits of row i
            int p = 0;
            const auto& row = c.rows[i];
            for (size_t s2 = 0; s2 + 1 < row.size(); ++s2) p ^= bits[row[s2]];
            bits[c.k + i] = static_cast<uint8_t>(p);
        }
        uint8_t* out = coded_out + static_cast<size_t>(w) * 81;
        std::memset(out, 0, 81);
        for (int j = 0; j < 648; ++j) out[j >> 3] |= static_cast<uint8_t>(bits[j] << (7 - (j & 7)));
    }
    return RIA_OK;
}

int ria_gpu_debug_queue_fault(ria_gpu_handle h) {
    if (!h) return RIA_ERR_INVALID;
    if (!h->d_ctl) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    DecodeCtl c[kMaxParts];
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(c, h->d_ctl.as<>(), sizeof(c), hipMemcpyDeviceToHost));
    int bad = 0;
    for (const DecodeCtl& q : c) bad |= q.queue_fault ? 1 : 0;
    return bad;
}

int ria_gpu_debug_recovery_counts(ria_gpu_handle h, int slot, uint32_t out[4]) {
    if (!h || !out || slot < 0 || slot >= kMaxParts) return fail(h, RIA_ERR_INVALID, "ria_gpu_debug_recovery_counts: bad argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (h->rec_frames == 0) return RIA_OK;   // no call has run the recovery yet
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned int c[8];
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(c, recovery_ws(h).rctl + 8 * slot, sizeof(c), hipMemcpyDeviceToHost));
    out[0] = c[0]; out[1] = c[2]; out[2] = c[1]; out[3] = c[5];   // n_flagged, n_stage2, n_list2, n_queued
    return RIA_OK;
}

int ria_gpu_debug_state_exits(ria_gpu_handle h, int slot, uint32_t out[4]) {
    if (!h || !out || slot < 0 || slot >= kMaxParts) return fail(h, RIA_ERR_INVALID, "ria_gpu_debug_state_exits: bad argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!h->d_ctl) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    DecodeCtl c;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(&c, h->d_ctl.as<DecodeCtl>() + slot, sizeof(c), hipMemcpyDeviceToHost));
    out[1] = c.exits[kExitsPhase0]; out[2] = c.exits[kExitsCascade]; out[3] = c.exits[kExitsFill];
    out[0] = out[1] + out[2] + out[3];
    return RIA_OK;
}

int ria_gpu_debug_first_decodes(ria_gpu_handle h, int slot, uint32_t out[2]) {
    if (!h || !out || slot < 0 || slot >= kMaxParts) return fail(h, RIA_ERR_INVALID, "ria_gpu_debug_first_decodes: bad argument");
    out[0] = out[1] = 0;
    if (!h->d_ctl) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    DecodeCtl c;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(&c, h->d_ctl.as<DecodeCtl>() + slot, sizeof(c), hipMemcpyDeviceToHost));
    out[0] = c.skipped; out[1] = c.late_made;
    return RIA_OK;
}

int ria_gpu_debug_math(ria_gpu_handle h, int op, const float* a_dev, const float* b_dev, int n, float* out_dev,
                       void* stream) {
    if (!h || !a_dev || !out_dev || n < 0) return fail(h, RIA_ERR_INVALID, "ria_gpu_debug_math: bad argument");
    if (n == 0) return RIA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), op,
                       a_dev, b_dev, n, out_dev);
    HIP_TRY(h, hipGetLastError());
    return RIA_OK;
}

}  // extern "C"
