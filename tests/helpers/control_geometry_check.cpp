// Checks ria_amd/csrc/var_frames.hpp - the sample counts behind ria_gpu_var_frame_samples and
// ria_gpu_control_frame_samples - for all 9 modulations x 6 code rates against the reference's statements written out
// another way: getMinSamplesForCWCount (ofdm_chirp_waveform.cpp:616-648) by counting symbols one at a time, and
// getOFDMControlFrameSamples (streaming_decoder.cpp:42-69).  Plain C++: builds with g++, also under
// -fsanitize=address,undefined.  Prints "failures N".
#include <cstdio>
#include "../../ria_amd/csrc/host_tables.hpp"
#include "../../ria_amd/csrc/var_frames.hpp"

static int symbols_for_bits(int bits, int bits_per_symbol) {   // the symbols a modulator emits: one more while bits remain
    int n = 0;
    for (int left = bits; left > 0; left -= bits_per_symbol) ++n;
    return n;
}

int main() {
    const int mods[9] = {RIA_MOD_DBPSK, RIA_MOD_BPSK, RIA_MOD_DQPSK, RIA_MOD_QPSK, RIA_MOD_D8PSK, RIA_MOD_QAM16, RIA_MOD_QAM32,
                         RIA_MOD_QAM64, RIA_MOD_QAM256};
    const int carriers = ria::kCarriers;
    int failures = 0, checked = 0;
    for (int mod : mods)
        for (int rate = RIA_RATE_1_4; rate <= RIA_RATE_5_6; ++rate) {
            const ria::CarrierPlan p = ria::build_carrier_plan(mod, rate);
            const int pilots = (carriers + p.spacing - 1) / p.spacing;            // getMinSamplesForCWCount's own count
            const int bps = (carriers - pilots) * ria::bits_per_carrier(mod);
            if (pilots != p.n_pilot || bps != p.n_data * ria::bits_per_carrier(mod)) { ++failures; printf("plan %d %d\n", mod, rate); }
            for (int nb = 1; nb <= ria::kVarMaxCodedBytes; ++nb) {
                const int want = (2 + symbols_for_bits(8 * nb, bps)) * 1152;
                if (ria::var_frame_samples(bps, nb) != want) { ++failures; printf("var %d %d %d: %d != %d\n", mod, rate, nb, ria::var_frame_samples(bps, nb), want); }
                ++checked;
            }
            // the fixed frame and getMinSamplesForCWCount(1)
            if (ria::var_frame_samples(bps, 324) != (2 + (ria::kFrameBits + bps - 1) / bps) * 1152) { ++failures; printf("fixed %d %d\n", mod, rate); }
            const int own = (2 + symbols_for_bits(648, bps)) * 1152;
            const bool is_ctl = mod == RIA_MOD_DQPSK && rate == RIA_RATE_1_4;
            const int robust_carriers = carriers - (carriers + 9) / 10;
            const int robust = (2 + symbols_for_bits(648, 2 * robust_carriers)) * 1152;
            const int want = is_ctl ? own : (own > robust ? own : robust);
            if (ria::control_frame_samples(bps, is_ctl, carriers) != want) { ++failures; printf("control %d %d: %d != %d\n", mod, rate, ria::control_frame_samples(bps, is_ctl, carriers), want); }
            ++checked;
        }
    // the numbers of the production link: an ACK at DQPSK R1/4 is 9 symbols, and that is the span behind a QAM16 R1/2 link too
    {
        const ria::CarrierPlan c = ria::build_carrier_plan(RIA_MOD_DQPSK, RIA_RATE_1_4), d = ria::build_carrier_plan(RIA_MOD_QAM16, RIA_RATE_1_2);
        if (ria::var_frame_samples(c.n_data * 2, 81) != 10368) { ++failures; printf("ack size\n"); }
        if (ria::control_frame_samples(d.n_data * 4, false, carriers) != 10368) { ++failures; printf("qam16 control span\n"); }
        const ria::CarrierPlan b = ria::build_carrier_plan(RIA_MOD_DBPSK, RIA_RATE_1_2);
        if (ria::control_frame_samples(b.n_data, false, carriers) != ria::var_frame_samples(b.n_data, 81)) { ++failures; printf("dbpsk control span\n"); }
    }
    printf("checked %d, failures %d\n", checked, failures);
    return failures ? 1 : 0;
}
