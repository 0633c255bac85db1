// ria_amd/csrc/var_frames.hpp — sample counts of frames that are not the fixed 4-codeword frame.  Plain C++17, no HIP:
// tests/helpers/control_geometry_check.cpp builds it with g++.
#pragma once

namespace ria {

constexpr int kVarSym = 1152;            // samples per OFDM symbol (FFT 1024 + cyclic prefix 128)
constexpr int kVarMaxCodedBytes = 324;   // 4 codewords of 81 bytes: the fixed frame

// OFDMChirpWaveform::getMinSamplesForCWCount's formula for any byte count (ofdm_chirp_waveform.cpp:616-648): two training
// symbols and the data symbols that hold 8 * coded_bytes bits
inline int var_data_symbols(int bits_per_symbol, int coded_bytes) { return (8 * coded_bytes + bits_per_symbol - 1) / bits_per_symbol; }
inline int var_frame_samples(int bits_per_symbol, int coded_bytes) { return (2 + var_data_symbols(bits_per_symbol, coded_bytes)) * kVarSym; }

// getOFDMControlFrameSamples (streaming_decoder.cpp:42-69): the data profile's own 1-codeword size, and for any profile
// but DQPSK R1/4 at least the DQPSK control profile's size at pilot spacing 10
inline int control_frame_samples(int data_bits_per_symbol, bool data_is_dqpsk_r14, int carriers) {
    const int own = var_frame_samples(data_bits_per_symbol, 81);
    if (data_is_dqpsk_r14) return own;
    const int pilots = (carriers + 9) / 10;
    int data_carriers = carriers - pilots;
    if (data_carriers < 1) data_carriers = 1;
    const int robust = (2 + (648 + 2 * data_carriers - 1) / (2 * data_carriers)) * kVarSym;
    return own > robust ? own : robust;
}

}  // namespace ria
