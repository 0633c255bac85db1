// CPU check of the transmit kernels' constant block (ria_amd/csrc/tx_const.hpp) for all 9 modulations x 6 code rates:
// tx_const_misfit accepts the configuration, build_tx_const stays inside TxConst (run under -fsanitize=address,undefined),
// the counts fit the LDS areas of tx_frames_kernel, every data_bin / pilot_bin is distinct and inside 0..1023, the parity
// table has kMaxRowDeg rows of m entries and the scatter table is a permutation of 0..2591.
// Prints one line per configuration and "configurations <n> failures <n>".
#include <cstdio>
#include <set>
#include "../../ria_amd/csrc/tx_const.hpp"

static ria_gpu_geometry geometry_of(const ria::CarrierPlan& p, const ria::LdpcCode& c, int mod, int rate) {   // as ria_gpu_create derives it
    ria_gpu_geometry g{};
    g.pilot_spacing = p.spacing; g.n_pilots = p.n_pilot; g.n_data_carriers = p.n_data;
    g.bits_per_carrier = ria::bits_per_carrier(mod);
    g.bits_per_symbol = g.n_data_carriers * g.bits_per_carrier;
    g.n_data_symbols = (ria::kFrameBits + g.bits_per_symbol - 1) / g.bits_per_symbol;
    g.samples_per_symbol = ria::kSym;
    g.frame_samples = (2 + g.n_data_symbols) * ria::kSym;
    g.llrs_per_frame = g.n_data_symbols * g.bits_per_symbol;
    g.info_bits = ria::info_bits_for(rate);
    g.bytes_per_codeword = g.info_bits / 8;
    g.info_bytes_per_frame = 4 * g.bytes_per_codeword;
    g.ldpc_k = c.k;
    return g;
}

int main() {
    const int mods[9] = {RIA_MOD_DBPSK, RIA_MOD_BPSK, RIA_MOD_DQPSK, RIA_MOD_QPSK, RIA_MOD_D8PSK, RIA_MOD_QAM16, RIA_MOD_QAM32, RIA_MOD_QAM64, RIA_MOD_QAM256};
    int n = 0, failures = 0;
    for (int mod : mods)
        for (int rate = RIA_RATE_1_4; rate <= RIA_RATE_5_6; ++rate) {
            const ria::CarrierPlan p = ria::build_carrier_plan(mod, rate);
            const ria::LdpcCode c = ria::build_ldpc(rate);
            const ria_gpu_geometry g = geometry_of(p, c, mod, rate);
            int bad = 0;
            auto need = [&](bool ok, const char* what) { if (!ok) { printf("  mod %d rate %d: %s\n", mod, rate, what); ++bad; } };
            const char* why = ria::tx_const_misfit(p, c, g);
            need(why == nullptr, why ? why : "");
            need(p.n_data + p.n_pilot == ria::kCarriers && p.n_data <= ria::kTxMaxCarriers && p.n_pilot <= ria::kTxMaxCarriers, "carrier counts");
            need(g.n_data_symbols <= ria::kTxMaxSymbols, "n_data_symbols <= 64");
            need(c.row_var.size() == static_cast<size_t>(7) * c.m && c.row_var.size() <= sizeof(ria::TxConst::row_var) / 2, "row_var has 7 rows of m");
            need(static_cast<size_t>(c.m) <= sizeof(ria::TxConst::row_deg), "row_deg");
            need(ria::build_rx_gather(g.bits_per_symbol, true).size() == 2592 && sizeof(ria::TxConst::scatter) == 2592 * 2, "scatter has 2592 entries");
            if (!why) {
                const ria::TxConst t = ria::build_tx_const(p, c, mod, g);
                std::set<int> bins, pos;
                for (int i = 0; i < t.n_data; ++i) { need(t.data_bin[i] >= 0 && t.data_bin[i] < ria::kFFT, "data_bin range"); bins.insert(t.data_bin[i]); }
                for (int i = 0; i < t.n_pilot; ++i) { need(t.pilot_bin[i] >= 0 && t.pilot_bin[i] < ria::kFFT, "pilot_bin range"); bins.insert(t.pilot_bin[i]); }
                need(static_cast<int>(bins.size()) == t.n_data + t.n_pilot, "bins distinct");
                for (int i = 0; i < ria::kFrameBits; ++i) pos.insert(t.scatter[i]);
                need(static_cast<int>(pos.size()) == ria::kFrameBits && *pos.rbegin() == ria::kFrameBits - 1, "scatter is a permutation");
                for (int i = 0; i < t.m; ++i)
                    for (int s = 0; s + 1 < t.row_deg[i]; ++s) need(t.row_var[s * t.m + i] < t.k, "parity loop reads information bits only");
                need(t.k + t.m == ria::kCwBits && t.bytes_per_cw * 4 <= 4 * ria::kTxMaxBytesPerCw, "code and frame bytes");
                // the last data symbol starts inside the stream: no symbol of the frame is all padding
                need((t.n_data_symbols - 1) * t.bits_per_symbol < ria::kFrameBits, "last symbol carries bits");
            }
            printf("mod %2d rate %d: n_data %d n_pilot %d symbols %d k %d m %d %s\n", mod, rate, p.n_data, p.n_pilot, g.n_data_symbols, c.k, c.m, bad ? "FAIL" : "ok");
            ++n; failures += bad != 0;
        }
    printf("lds bytes %d\n", ria::tx_lds_bytes());
    printf("configurations %d failures %d\n", n, failures);
    return failures ? 1 : 0;
}
