/* oracle/ria_oracle.h — CPU restatement of the RIA RX hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and the cpu_baseline leg of
 * bench.py may load this library; the product (ria_amd/, libria_gpu.so) never does.
 *
 * Every function restates a reference routine in plain C (cited file:line, paths relative to the
 * reference repository root).  It is pinned against the compiled, unmodified reference
 * (oracle/_ref/libria_ref.so, built by oracle/Makefile in the build container) by
 * oracle/check_against_ref.py and by the golden vectors committed under tests/golden/.
 */
#ifndef RIA_ORACLE_H
#define RIA_ORACLE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum values follow include/ultra/types.hpp:28-39 (Modulation) and :91-100 (CodeRate) */
enum { RO_DBPSK = 0, RO_BPSK = 1, RO_DQPSK = 2, RO_QPSK = 3, RO_D8PSK = 4, RO_QAM8 = 5,
       RO_QAM16 = 6, RO_QAM32 = 7, RO_QAM64 = 8, RO_QAM256 = 10 };
enum { RO_R1_4 = 0, RO_R1_3 = 1, RO_R1_2 = 2, RO_R2_3 = 3, RO_R3_4 = 4, RO_R5_6 = 5, RO_R7_8 = 6 };

#define RO_FFT 1024
#define RO_CP 128
#define RO_SYM (RO_FFT + RO_CP)
#define RO_NCAR 59
#define RO_CW_BITS 648
#define RO_FRAME_BITS 2592
#define RO_MAX_EDGES 4096

typedef struct ro_geom {
    int mod, rate;
    int pilot_spacing, n_pilot, n_data;
    int bits_per_carrier, bits_per_symbol; /* n_data * bits_per_carrier */
    int n_data_symbols;                    /* ceil(2592 / bits_per_symbol) */
    int frame_samples;                     /* (2 + n_data_symbols) * 1152 */
    int n_llr;                             /* n_data_symbols * bits_per_symbol */
    int info_bits, bytes_per_cw, max_iter; /* LDPC k, k/8, recommended iterations */
    int all_idx[RO_NCAR];                  /* logical carrier -> FFT bin */
    int is_pilot[RO_NCAR];
    int data_idx[RO_NCAR], pilot_idx[RO_NCAR]; /* FFT bins */
    int data_logical[RO_NCAR], pilot_logical[RO_NCAR];
    float sync_re[RO_NCAR], sync_im[RO_NCAR];  /* ZC-59 LTS sequence */
    float pilot_seq[RO_NCAR];                  /* +-1 */
    int interp_lo[RO_NCAR], interp_hi[RO_NCAR]; /* per data carrier: pilot ordinal or -1 */
    float interp_alpha[RO_NCAR];
} ro_geom;

int ro_geom_init(ro_geom* g, int mod, int rate);

/* ---- RNG (std::mt19937 + libstdc++ std::normal_distribution<float>) */
typedef struct ro_mt { uint32_t s[624]; int idx; } ro_mt;
void ro_mt_seed(ro_mt* m, uint32_t seed);
uint32_t ro_mt_next(ro_mt* m);
typedef struct ro_normal { float saved; int has_saved; } ro_normal;
float ro_normal_draw(ro_normal* n, ro_mt* m, float mean, float stddev);

/* ---- LDPC (src/fec/ldpc_encoder.cpp, src/fec/ldpc_decoder.cpp) */
typedef struct ro_ldpc {
    int rate, k, m, n, n_edges;
    int row_ptr[RO_CW_BITS + 1];
    int edge_var[RO_MAX_EDGES]; /* row-major edge list: variable index */
} ro_ldpc;
int ro_ldpc_build(ro_ldpc* c, int rate);
int ro_ldpc_encode(const ro_ldpc* c, const uint8_t* info, int n_info_bytes, uint8_t* coded81);
/* returns 1 on success; out gets ceil(k/8) bytes; *iters as LDPCDecoder::lastIterations() */
int ro_ldpc_decode(const ro_ldpc* c, const float* llr, int n_llr, int max_iter, float factor,
                   uint8_t* out, int* iters);

/* ---- interleavers */
int ro_channel_interleaver_step(int bits_per_symbol, int total);
void ro_rx_gather_table(int bits_per_symbol, int use_channel, int* table /*[4*648]*/);

/* ---- frame build / TX (src/protocol/frame_v2.cpp, src/ofdm/modulator.cpp) */
uint16_t ro_crc16(const uint8_t* d, int n);
int ro_make_frame(const uint8_t* payload, int payload_len, int seq, int rate, uint8_t* info_out);
int ro_encode_fixed_frame(const uint8_t* info, int n_info, int rate, int ch_interleave, int bps,
                          uint8_t* coded324);
int ro_modulate(const ro_geom* g, const uint8_t* coded, int n_coded, float* samples, int max_samples);

/* ---- channel (src/sim/hf_channel.hpp) kind: 0 awgn 1 good 2 moderate 3 poor 4 flutter */
int ro_channel(int kind, float snr_db, uint32_t seed, const float* in, int n, float* out);
/* the same with Config::cfo_hz / random_cfo_max_hz: the constructor's CFO draw (hf_channel.hpp:97-102) and applyCFO
 * (:182-241) after the noise; actual_cfo_out (nullable) = getActualCFO() */
int ro_channel_cfo(int kind, float snr_db, uint32_t seed, float cfo_hz, float random_cfo_max_hz, const float* in, int n, float* out,
                   float* actual_cfo_out);

/* ---- RX demod (src/ofdm/demodulator.cpp, channel_equalizer.cpp, soft_demap.hpp) */
typedef struct ro_rx_aux {
    float snr_db, cfo_hz, fading_index, noise_variance, lts_phase_slope, snr_linear,
          corr_phase, snr_symbol_count;
    float h[2 * RO_NCAR];
} ro_rx_aux;
int ro_rx_process(const ro_geom* g, const float* samples, int n, float cfo_hz, long long abs_pos,
                  float* llr_out, int max_llr, ro_rx_aux* aux);
/* the correction phase at the first sample, wrapped into [-pi, pi] as OFDMChirpWaveform::process does; like the
 * reference it does not return for |2 pi cfo_hz abs_pos / 48000| above 2^27 or infinite */
float ro_theta0(float cfo_hz, long long abs_pos);
/* test instrumentation: how often the last ro_rx_process[_flags]() of the calling thread took each data-dependent branch.
 * H_SMALL: a training pair failed |H| > 0.01; MAG_SMALL: failed mag > 1e-6; CNT_SMALL: 10 or fewer pairs for the residual
 * CFO; RERUN: the 0.3 .. 5 Hz re-run; SNR_LOW / SNR_HIGH: the training SNR clamped at 3.16 / 10000; HM_SMALL: a pilot's
 * previous |H| failed hm > 0.01; SNV_SMALL: noise variance below 1e-6 replaced; DEN_SMALL: den < 1e-10; CNV_LOW / CNV_HIGH:
 * the per-carrier noise clamped at 1e-6 / 100; D8PSK_TWO_PASS: symbols through the fading > 0.30 gate; SP_SMALL: the
 * 1-bit demapper's sp < 1e-6 */
enum { RO_BC_H_SMALL, RO_BC_MAG_SMALL, RO_BC_CNT_SMALL, RO_BC_RERUN, RO_BC_SNR_LOW, RO_BC_SNR_HIGH, RO_BC_HM_SMALL, RO_BC_SNV_SMALL,
       RO_BC_DEN_SMALL, RO_BC_CNV_LOW, RO_BC_CNV_HIGH, RO_BC_D8PSK_TWO_PASS, RO_BC_SP_SMALL, RO_BC_N };
void ro_branch_counts(unsigned* out /* [RO_BC_N] */);

/* (a + bi)(c + di) as std::complex<float> operator* computes it (libgcc __mulsc3: C99 Annex G.5.1 recovery of infinities);
 * ria_oracle.c's cf_mul for the other translation unit */
void ro_cmul(float a, float b, float c, float d, float* re, float* im);

/* The same for the four acquisition detectors: how often the last ro_zc_detect / ro_chirp_detect / ro_detect_data_sync /
 * ro_cox_search of this thread found each data-dependent condition true (_T) and false (_F), and how often a maximum search
 * met a lag whose metric equals the running maximum bit for bit (_TIE: the first-maximum rule decided).
 * ZC: DENOM denom > 1e-10 (:556), PEAK peak > threshold at a peak >= 1016 (:262), EARLIER earlier repetition > 0.4 peak (:268),
 * COMBINE 0 < peak < 0.25 with room for the second repetition (:280), CFO_OK both repetitions above 0.1 (:349), DETECT
 * best > threshold (:375), SNR_LOW corr <= 0.01, SNR_HIGH corr >= 0.99 (:628-633).
 * CH: FFT transform path (_F: time-domain path, chirp_sync.hpp:735), DENOM denom > 1e-10 (:686), THR best < threshold (:707),
 * TD_DENOM denom < 1e-10 (:847), TD_COARSE no coarse candidate or below 0.3 threshold (:777), TD_THR best >= threshold (:812),
 * CFO_REJ |cfo| > 100 Hz (:489).
 * LTS: NOISE noise floor < 0.05 (ofdm_chirp_waveform.cpp:241), ENERGY a 64-sample window above the gate (:252), EXIT
 * corr > 0.95 (:312), DETECT best > threshold (:320, :356), MARKER compensated peak negative (:372).
 * COX: NF_INIT floor < 1e-20, ENERGY energy >= 4 floors (ofdm_sync.cpp:36-49), NORM norm < 1e-10 (:156), THR corr > threshold
 * (demodulator.cpp:1494), PLATEAU c >= 0.90 (:1502), RULE plateau >= 15 (:1509), LTS_NORM norm > 1e-6 (ofdm_sync.cpp:437),
 * EARLIER_LTS previous copy >= 0.92 best (:460), CONFIRM best < 0.05 (:470). */
#define RO_SBC_PAIRS(X) X(ZC_DENOM) X(ZC_PEAK) X(ZC_EARLIER) X(ZC_COMBINE) X(ZC_CFO_OK) X(ZC_DETECT) X(ZC_SNR_LOW) X(ZC_SNR_HIGH) \
    X(CH_FFT) X(CH_DENOM) X(CH_THR) X(CH_TD_DENOM) X(CH_TD_COARSE) X(CH_TD_THR) X(CH_CFO_REJ) \
    X(LTS_NOISE) X(LTS_ENERGY) X(LTS_EXIT) X(LTS_DETECT) X(LTS_MARKER) \
    X(COX_NF_INIT) X(COX_ENERGY) X(COX_NORM) X(COX_THR) X(COX_PLATEAU) X(COX_RULE) X(COX_LTS_NORM) X(COX_EARLIER_LTS) X(COX_CONFIRM)
#define RO_SBC_ENUM(n) RO_SBC_##n##_T, RO_SBC_##n##_F,
enum { RO_SBC_PAIRS(RO_SBC_ENUM) RO_SBC_ZC_TIE, RO_SBC_CH_TIE, RO_SBC_LTS_TIE, RO_SBC_COX_TIE, RO_SBC_N };
extern _Thread_local unsigned ro_sbc[RO_SBC_N];
#define SBC(n, cond) ((cond) ? (ro_sbc[RO_SBC_##n##_T]++, 1) : (ro_sbc[RO_SBC_##n##_F]++, 0))
void ro_sync_branch_counts(unsigned* out /* [RO_SBC_N] */);
int ro_sync_branch_n(void);

/* the same with OFDMChirpWaveform's one-shot burst marker: flags bit0 = the first LTS symbol was negated on air
 * (ofdm_chirp_waveform.cpp:421-440) */
int ro_rx_process_flags(const ro_geom* g, const float* samples, int n, float cfo_hz, long long abs_pos, int flags,
                        float* llr_out, int max_llr, ro_rx_aux* aux);
/* fec::BurstInterleaver (src/fec/burst_interleaver.cpp:8-78) */
void ro_burst_interleave(int n_frames, const uint8_t* logical, uint8_t* physical);
void ro_burst_deinterleave(int n_frames, const float* physical, int stride, float* logical);

/* ---- decode (src/protocol/frame_v2.cpp:1335-1883) */
/* flags bit0: run retry cascade phase 0; bit1: phases 1-6; bit2: CRC false-positive recovery */
int ro_decode_fixed_frame(const float* llr, int n, int rate, int ch_deint, int bps, int flags,
                          uint8_t* data_out, uint8_t* ok_out, int* iters_out, int* attempts_out);
/* which step of the CRC recovery ended this thread's last ro_decode_fixed_frame (coverage bookkeeping of the tests only;
 * the reference has no such getter).  detail: the fallback's substitution index (attempt * 4 + codeword), else -1. */
enum { RO_REC_NONE = 0, RO_REC_HDR1, RO_REC_HDR2, RO_REC_SINGLE, RO_REC_CRC, RO_REC_PAIR, RO_REC_TRIPLE, RO_REC_QUAD,
       RO_REC_FILL, RO_REC_FAILED };
int ro_last_recovery_stage(int* detail);

#ifdef __cplusplus
}
#endif
/* ---- acquisition correlators (ria_oracle_sync.c) ---- */
/* sync::ZCSync, src/sync/zc_sync.hpp: preamble synthesis and detection.
 * out7 = {detected, frame_type, start_sample, correlation, cfo_hz, snr_estimate, root_detected} */
int ro_zc_preamble_samples(void);
int ro_zc_generate(int root, float* out, int max_n);
int ro_zc_detect(const float* rx, int n, float threshold, int root_mask, float known_cfo_hz, float* out7);
/* sync::ChirpSync, src/sync/chirp_sync.hpp: dual-chirp synthesis (57 600 samples) and detectDualChirp.
 * out6 = {success, up_chirp_start, down_chirp_start, cfo_hz, up_correlation, down_correlation} */
int ro_chirp_generate(float* out, int max_n);
int ro_chirp_detect(const float* s, int n, float threshold, float* out6);
/* MultiCarrierDPSK (src/psk/multi_carrier_dpsk.hpp): training + reference + data audio, and the demodulator chain
 * of processGotChirp after an external chirp detection.  aux4 = {cfo, fading, frequency fading, temporal fading}. */
int ro_mcdpsk_modulate(int nc, int bps, int spreading, const uint8_t* data, int n_bytes, float* out, int max_n);
int ro_mcdpsk_demod(int nc, int bps, int spreading, const float* samples, int n, float cfo_hz, float phase0,
                    float* llr_out, int max_llr, float* aux4);
/* the same chain, also returning what processTraining and demodulateSoft compute and the reference exposes no getter for:
 * the training CFO residual (:473-505, Hz) and the number of data symbols kept by the trailing-silence trim (:600-640).
 * Returns the LLR count like ro_mcdpsk_demod. */
int ro_mcdpsk_demod_ex(int nc, int bps, int spreading, const float* samples, int n, float cfo_hz, float phase0,
                       float* llr_out, int max_llr, float* aux4, float* residual_out, int* valid_out);
/* How often each data-dependent condition of the MC-DPSK demodulator was true (_T) and false (_F) during this thread's last
 * ro_mcdpsk_demod / ro_mcdpsk_demod_ex.  Test instrumentation only: no result depends on it.
 * CFO_GATE |cfo| > 0.1 (:857); REF_AMP reference-symbol amplitude > 0.001 (:512); SYM_MAG combined magnitude > 0.0001 (:567);
 * NDS4 nds >= 4 (:604); REF_MAG mean total of the first four symbols > 0.001 (:611); TRIM_ROOM valid > 4 and TRIM_LOW last
 * symbol's total < 0.2 ref_mag (:614); PNV_FLOOR 0.01 < noise variance, SCALE_CAP 20 < scale (:640-642); MEAN_OK carrier
 * mean > 1e-4 (:652); MEAN_DEAD mean <= 1e-4 and GMEAN_DEAD gmean <= 1e-4 (:665); VAR_POS 0 < var; RATIO_CAP ratio < 1.25;
 * MW_FLOOR 0.10 < min(1.25, ratio); RATIO_020 ratio < 0.20; RATIO_035 ratio < 0.35; W_CAP w < 1.25; W_FLOOR 0.12 < w
 * (:668-690); LLR_HI soft bit < 20 and LLR_LO -20 < soft bit (:650-667); VALID4 valid >= 4 and TFI_MEAN carrier mean < 0.001
 * (:705-733); FFI_MEAN mean over the carriers < 0.001 (:404-437).  REF_AMP_EDGE / SYM_MAG_EDGE: the amplitude / magnitude equals
 * its threshold exactly (where `>` and `>=` part). */
#define RO_MBC_PAIRS(X) X(CFO_GATE) X(REF_AMP) X(SYM_MAG) X(NDS4) X(REF_MAG) X(TRIM_ROOM) X(TRIM_LOW) X(PNV_FLOOR) X(SCALE_CAP) \
    X(MEAN_OK) X(MEAN_DEAD) X(GMEAN_DEAD) X(VAR_POS) X(RATIO_CAP) X(MW_FLOOR) X(RATIO_020) X(RATIO_035) X(W_CAP) X(W_FLOOR) \
    X(LLR_HI) X(LLR_LO) X(VALID4) X(TFI_MEAN) X(FFI_MEAN) X(REF_AMP_EDGE) X(SYM_MAG_EDGE)
#define RO_MBC_ENUM(n) RO_MBC_##n##_T, RO_MBC_##n##_F,
enum { RO_MBC_PAIRS(RO_MBC_ENUM) RO_MBC_N };
void ro_mcdpsk_branch_counts(unsigned* out /* [RO_MBC_N] */);
int ro_mcdpsk_branch_n(void);
/* OFDMChirpWaveform::detectDataSync (LTS light sync); out4 = {detected, start_sample, correlation, burst_interleaved} */
int ro_detect_data_sync(const float* x, int n, float known_cfo_hz, float threshold, float* out4);
/* SimulatedChannel::applyTxCFO (tools/cli_simulator.cpp:298-341): the simulator's transmitter frequency offset - FFT of
 * the next power of two, frequency-domain Hilbert, inverse FFT, rotation by a wrapped float phase (in/out), real part */
int ro_apply_tx_cfo(const float* in, int n, float cfo_hz, float* phase_inout, float* out);
/* ---- helper arithmetic of the reference's own test programs (their scenarios are composed in pyoracle.py)
 * ro_tool_add_noise: addNoise of tools/test_zc_sync.cpp:22-39 == tools/test_spreading.cpp:15-30 (AWGN at an SNR against the
 *   mean power of ALL samples; a fresh std::normal_distribution<float>(0, sigma) per call on the caller's generator)
 * ro_tool_apply_cfo: applyCFO of tools/test_zc_sync.cpp:43-63 (HilbertTransform(127), src/dsp/filters.cpp:266-317, rotation
 *   by a float phase wrapped into (-pi, pi], real part)
 * ro_tool_chase_reception: generateNoisyCodeword + addNoise of tools/test_chase_cache.cpp:21-62 (coded bits as +-4, a
 *   reception is 2 (sign + n) snr with n ~ N(0, 1 / snr)) */
void ro_tool_add_noise(float* x, int n, float snr_db, ro_mt* rng);
void ro_tool_apply_cfo(float* x, int n, float cfo_hz, float sample_rate);
void ro_tool_chase_reception(const uint8_t* coded81, float snr_db, ro_mt* rng, float* llr648);
/* fec::ChaseCache::store arithmetic for one codeword slot (src/fec/chase_cache.cpp:27-88) */
int ro_chase_store(float* existing, int* combine_count, int decoded, const float* soft);

#endif
/* Schmidl-Cox acquisition: OFDMDemodulator::searchForSync (src/ofdm/demodulator.cpp:1450-1542, ofdm_sync.cpp).
 * out3 = {found, first-LTS position, cfo_hz}; noise_floor in/out = Impl::noise_floor_energy (may be NULL = 0). */
#ifdef __cplusplus
extern "C" {
#endif
void ro_cox_lts_template(const ro_geom* g, float* tI, float* tQ);
int ro_cox_search(const ro_geom* g, const float* x, int n, float threshold, float* noise_floor, float* out3);
#ifdef __cplusplus
}
#endif
