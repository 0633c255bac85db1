// ria_amd/csrc/tx_const.hpp — the constant block of the transmit kernels (tx_kernels.hip.h) and the sizes of their LDS areas.
// Host C++ only, so that a CPU program can build it for every configuration (tests/helpers/tx_const_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/ria_gpu.h"
#include "host_tables.hpp"

namespace ria {

constexpr int kTxMaxCarriers = 64;   // data_bin / pilot_bin / sync rows of TxConst; one lane per data carrier
constexpr int kTxMaxSymbols = 64;    // rows of the differential state dstate[kTxMaxSymbols][kTxMaxCarriers]
constexpr int kTxFftTile = 1088;     // float2 slots of one IFFT tile (= kFftBufFloats2 of demod_kernels.hip.h)
constexpr int kTxMaxBytesPerCw = 68; // make_frames_kernel stages a frame in 4 * 68 bytes

struct TxConst {
    int mod, n_data, n_pilot, bits_per_carrier, bits_per_symbol, n_data_symbols;
    int k, m, bytes_per_cw;
    int data_bin[kTxMaxCarriers], pilot_bin[kTxMaxCarriers];
    float pilot_seq[kTxMaxCarriers];
    float sync_re[kTxMaxCarriers], sync_im[kTxMaxCarriers];   // by data ordinal
    uint8_t row_deg[kCwBits];
    uint16_t row_var[kMaxRowDeg * kCwBits];   // [kMaxRowDeg][m]
    uint16_t scatter[kFrameBits];             // coded bit i of codeword cw -> position in the 2592-bit stream
};
static_assert(kCarriers <= kTxMaxCarriers, "a lane and a TxConst slot per carrier");
static_assert(kFrameBits == 4 * kCwBits, "four codewords a frame");

// 4 IFFT tiles + interleaved bits + codeword bits + differential state + reduction scratch
inline int tx_lds_bytes() { return 4 * kTxFftTile * 8 + kFrameBits * 2 + kTxMaxSymbols * kTxMaxCarriers * 8 + 64; }
static_assert(4 * kTxFftTile * 8 + kFrameBits * 2 + kTxMaxSymbols * kTxMaxCarriers * 8 + 64 <= 160 * 1024, "LDS of a gfx950 workgroup");

// nullptr when TxConst and the kernels' LDS areas hold the configuration, else what does not fit.  ria_gpu_create asks
// before it builds the block: build_tx_const copies by the configuration's own counts.
inline const char* tx_const_misfit(const CarrierPlan& p, const LdpcCode& c, const ria_gpu_geometry& g) {
    if (p.n_data < 1 || p.n_data > kCarriers || p.n_pilot < 0 || p.n_pilot > kCarriers) return "carrier counts";
    if (g.n_data_carriers != p.n_data || g.bits_per_symbol != p.n_data * g.bits_per_carrier || g.bits_per_carrier < 1) return "geometry";
    if (g.n_data_symbols < 1 || g.n_data_symbols > kTxMaxSymbols) return "data symbols per frame";
    if (g.n_data_symbols * g.bits_per_symbol < kFrameBits) return "the symbols do not hold the frame";
    if (g.bytes_per_codeword < 5 || g.bytes_per_codeword > kTxMaxBytesPerCw) return "bytes per codeword";
    if (c.k < 1 || c.m < 1 || c.k + c.m != kCwBits) return "code length";
    if (static_cast<int>(c.row_deg.size()) != c.m || c.row_var.size() != static_cast<size_t>(kMaxRowDeg) * c.m) return "parity table shape";
    for (int i = 0; i < c.m; ++i) {
        if (c.row_deg[i] < 1 || c.row_deg[i] > kMaxRowDeg) return "check degree";
        for (int s = 0; s + 1 < c.row_deg[i]; ++s) if (c.row_var[static_cast<size_t>(s) * c.m + i] >= c.k) return "parity table entry";
        if (c.row_var[static_cast<size_t>(c.row_deg[i] - 1) * c.m + i] != c.k + i) return "identity column";
    }
    const auto sc = build_rx_gather(g.bits_per_symbol, true);
    if (sc.size() != static_cast<size_t>(kFrameBits)) return "interleaver table size";
    for (uint16_t v : sc) if (v >= kFrameBits) return "interleaver table entry";
    return nullptr;
}

inline TxConst build_tx_const(const CarrierPlan& p, const LdpcCode& c, int mod, const ria_gpu_geometry& g) {
    TxConst t{};
    t.mod = mod;
    t.n_data = p.n_data; t.n_pilot = p.n_pilot;
    t.bits_per_carrier = g.bits_per_carrier; t.bits_per_symbol = g.bits_per_symbol;
    t.n_data_symbols = g.n_data_symbols;
    t.k = c.k; t.m = c.m; t.bytes_per_cw = g.bytes_per_codeword;
    for (int i = 0; i < p.n_data; ++i) { t.data_bin[i] = p.data_bin[i]; t.sync_re[i] = p.sync_re[i % kCarriers]; t.sync_im[i] = p.sync_im[i % kCarriers]; }
    for (int i = 0; i < p.n_pilot; ++i) { t.pilot_bin[i] = p.pilot_bin[i]; t.pilot_seq[i] = p.pilot_seq[i]; }
    for (int i = 0; i < c.m; ++i) t.row_deg[i] = c.row_deg[i];
    for (size_t i = 0; i < c.row_var.size(); ++i) t.row_var[i] = c.row_var[i];
    auto sc = build_rx_gather(g.bits_per_symbol, true);
    for (size_t i = 0; i < sc.size(); ++i) t.scatter[i] = sc[i];
    return t;
}

}  // namespace ria
