/* include/ria_gpu.h — C ABI of libria_gpu.so: the MI355X (gfx950) RX signal chain for the RIA modem.
 *
 * This is the drop-in boundary.  Every entry point replaces one call the unmodified
 * host code (gui::StreamingDecoder, tools/cli_simulator, tools/test_waveform_simple) makes today;
 * the reference interface each one stands in for is cited as file:line relative to the reference
 * repository.  INTEGRATION.md shows the adaptor class a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C, no exceptions: every function returns RIA_OK (0) or a negative ria_status; the text
 *     of the last error of a handle is available from ria_gpu_last_error().
 *   - "dev" pointers are device (HBM) addresses valid on the handle's GPU; "host" variants copy
 *     over PCIe themselves.  `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     device-pointer calls are asynchronous on that stream, host-pointer calls return when done.
 *   - a handle is bound to one (modulation, code rate) pair like one configured IWaveform object
 *     (waveform_interface.hpp:69 configure()); it is not thread-safe, like the reference
 *     (streaming_decoder.cpp:719 holds waveform_mutex_ around every call).
 *   - enum values are the reference's own (include/ultra/types.hpp:28-39, :91-100).
 */
#ifndef RIA_GPU_H
#define RIA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RIA_GPU_ABI_VERSION 1

typedef enum ria_status {
    RIA_OK = 0,
    RIA_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    RIA_ERR_NO_DEVICE = -2,    /* no gfx950 device or HIP runtime failure at create */
    RIA_ERR_HIP = -3,          /* a HIP call failed (see ria_gpu_last_error) */
    RIA_ERR_UNSUPPORTED = -4   /* valid request this build does not implement yet */
} ria_status;

/* Modulation (types.hpp:28-39) and CodeRate (types.hpp:91-100) */
enum { RIA_MOD_DBPSK = 0, RIA_MOD_BPSK = 1, RIA_MOD_DQPSK = 2, RIA_MOD_QPSK = 3, RIA_MOD_D8PSK = 4,
       RIA_MOD_QAM16 = 6, RIA_MOD_QAM32 = 7, RIA_MOD_QAM64 = 8, RIA_MOD_QAM256 = 10 };
enum { RIA_RATE_1_4 = 0, RIA_RATE_1_3 = 1, RIA_RATE_1_2 = 2, RIA_RATE_2_3 = 3, RIA_RATE_3_4 = 4,
       RIA_RATE_5_6 = 5 };

/* Immutable per-handle configuration: the subset of ultra::ModemConfig (types.hpp:193-289) the
 * OFDM-CHIRP RX path reads.  Zero-initialise, then ria_gpu_default_config(). */
typedef struct ria_gpu_config {
    int32_t abi_version;     /* RIA_GPU_ABI_VERSION */
    int32_t device;          /* HIP device ordinal */
    int32_t modulation;      /* RIA_MOD_* */
    int32_t code_rate;       /* RIA_RATE_* */
    int32_t fft_size;        /* 1024 */
    int32_t num_carriers;    /* 59 */
    int32_t cyclic_prefix;   /* 128 (CyclicPrefixMode::LONG at FFT 1024) */
    int32_t sample_rate;     /* 48000 */
    int32_t center_freq;     /* 1500 */
    int32_t max_batch;       /* frames per call the workspace is sized for */
    int32_t reserved[6];
} ria_gpu_config;

/* Frame geometry derived from the configuration (ofdm_chirp_waveform.cpp:616-648,
 * ofdm_link_adaptation.hpp:26-70, frame_v2.hpp:671-691). */
typedef struct ria_gpu_geometry {
    int32_t pilot_spacing, n_pilots, n_data_carriers;
    int32_t bits_per_carrier, bits_per_symbol;
    int32_t n_data_symbols;      /* data symbols in a fixed 4-codeword frame */
    int32_t samples_per_symbol;  /* 1152 */
    int32_t frame_samples;       /* (2 LTS + n_data_symbols) * 1152 = 18432 for QAM16 R1/2 */
    int32_t llrs_per_frame;      /* n_data_symbols * bits_per_symbol = 2632 */
    int32_t info_bits, bytes_per_codeword, info_bytes_per_frame; /* 324, 40, 160 */
    int32_t ldpc_max_iterations; /* ldpc_codec.hpp:86-95 */
    int32_t ldpc_edges;
    int32_t ldpc_k;              /* information bits of the LDPC code itself (ldpc_decoder.cpp:21-36): what the single-codeword
                                    decoders return, ceil(ldpc_k / 8) bytes.  Equals info_bits except at R1/3, whose table entry
                                    uses the (324, 324) code while the frame layer counts 216 bits (27 bytes) per codeword */
    int32_t reserved[1];
} ria_gpu_geometry;

/* Per-frame input of the demodulator: the three setters the host calls before process()
 * (streaming_decoder.cpp:896 setAbsoluteTrainingPosition, :1347 setFrequencyOffset).
 *
 * Limit: |cfo_hz * abs_position| <= 1.025e12 Hz*samples (2^27 * 48000 / (2 pi); at 60 Hz about 99 hours of samples).
 * The correction phase at the first sample is -2 pi cfo_hz abs_position / 48000 rounded to float and wrapped into
 * [-pi, pi] by repeated subtraction of 2 pi on that float (ofdm_chirp_waveform.cpp:402-411).  Up to |phase| = 2^27
 * every step changes the float and the library reproduces the reference's wrap bit for bit (ria_amd/csrc/cfo_theta0.h;
 * about |cfo_hz * abs_position| / 48000 steps of one lane, fewer than 2.3e7 at the limit).  Above 2^27, and
 * for an infinite phase (cfo_hz +-inf), the float no longer changes and the reference's loop does not return at all; the
 * library starts such a frame at phase 0 instead, at once.  For a NaN phase (cfo_hz NaN, or +-inf at position 0) the
 * reference's loops end at once with a NaN phase; the library deliberately starts that frame at phase 0 too.  Apart
 * from that cfo_hz is not validated: a non-finite value gives non-finite outputs.  flags bits 1..31 are ignored.
 *
 * Non-finite samples.  Samples may be NaN, +-inf or so large that sums overflow.  The demodulator then follows the
 * reference bit for bit, including what its std::complex arithmetic does there: operator* and operator/ recover an
 * infinity where both parts of a result come out NaN (C99 Annex G.5.1, libgcc __mulsc3 / __divsc3), and hypotf(inf, NaN)
 * is +inf.  The LLRs stay finite in every case the tests record: the demappers clamp to [-20, 20] with std::min / std::max, which turn a NaN into the
 * bound.  The float status words (ria_frame_status: fading_index, noise_variance, lts_phase_slope, snr_linear,
 * corr_phase, snr_db) can be NaN or inf for such a frame; a NaN there is a NaN in the reference, but its sign and payload
 * are the GPU's (0x7FC00000), not the host's. */
typedef struct ria_frame_meta {
    float    cfo_hz;          /* IWaveform::setFrequencyOffset */
    uint32_t flags;           /* bit0: first LTS symbol is negated (burst marker, ofdm_chirp_waveform.cpp:421-440) */
    uint64_t abs_position;    /* IWaveform::setAbsoluteTrainingPosition */
} ria_frame_meta;

/* Per-frame output of the demodulator: what the host reads back through IWaveform
 * (estimatedSNR :151, estimatedCFO :154, getFadingIndex :159) plus estimator taps for parity tests. */
typedef struct ria_frame_status {
    float snr_db;            /* OFDMDemodulator::getEstimatedSNR */
    float cfo_hz;            /* corrected CFO fed back to the waveform (ofdm_chirp_waveform.cpp:457-464) */
    float fading_index;      /* last_fading_index */
    float noise_variance;    /* LTS noise variance */
    float lts_phase_slope;
    float snr_linear;
    float corr_phase;        /* freq_correction_phase after the last sample */
    int32_t n_llr;           /* soft bits produced (0 if process() would have returned false) */
} ria_frame_status;

/* Per-frame output of decodeFixedFrame (frame_v2.hpp:637-664 CodewordStatus). */
typedef struct ria_decode_status {
    uint8_t  cw_ok[4];        /* CodewordStatus::decoded */
    uint16_t iterations[4];   /* LDPCDecoder::lastIterations() of the accepted (or last) attempt */
    uint8_t  attempts[4];     /* 1 = first decode, 2..5 phase 0, 6.. retry phases 1-6 */
    uint8_t  frame_valid;     /* 1: header+frame CRC verified on the reassembled frame */
    uint8_t  needs_recovery;  /* 1: all codewords converged but the frame CRC failed (LDPC false
                                 positive, frame_v2.cpp:1564-1880): ria_gpu_decode_* finishes it */
    uint8_t  reserved[2];     /* reserved[1] == 0xEE: an internal work queue of this call broke its bound; then every frame of the
                                 call is reported failed (cw_ok 0, frame_valid 0, zero bytes) and the host-buffer forms return RIA_ERR_HIP */
} ria_decode_status;

/* decode flags */
#define RIA_DECODE_PHASE0      0x1u  /* min-sum factor diversity retries   (frame_v2.cpp:1398-1413) */
#define RIA_DECODE_PERTURB     0x2u  /* stochastic retry phases 1-6        (frame_v2.cpp:1415-1546) */
#define RIA_DECODE_CRC_RECOVER 0x4u  /* CRC-guided false-positive recovery (frame_v2.cpp:1564-1880) */
#define RIA_DECODE_FULL        0x7u  /* exactly v2::decodeFixedFrame */
#define RIA_DECODE_NO_CHANNEL_DEINTERLEAVE 0x100u
#define RIA_RX_DEMOD_ONLY      0x200u  /* ria_gpu_rx_frames_host: process() + getSoftBits() only, no decode (info / decode
                                          status pointers may be NULL, llr_out_host must not be) */

typedef struct ria_gpu* ria_gpu_handle;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int  ria_gpu_abi_version(void);
/* Which implementation of the demodulator this process uses (fixed at the first call of any entry point that
 * demodulates, or of this function): 0 the split pipeline (demod_fft / decide / walk / est kernels), 1 the
 * one-wave-per-frame demod_frames_kernel (environment RIA_DEMOD_FUSED=1).  Both give the same bits. */
int  ria_gpu_demod_variant(void);
void ria_gpu_default_config(ria_gpu_config* cfg);
/* replaces: std::make_unique<OFDMChirpWaveform>(config) + configure(mod, rate)
 * (streaming_decoder.cpp:2299,2328; ofdm_chirp_waveform.cpp:81-107) */
int  ria_gpu_create(const ria_gpu_config* cfg, ria_gpu_handle* out);
void ria_gpu_destroy(ria_gpu_handle h);
const char* ria_gpu_last_error(ria_gpu_handle h);
int  ria_gpu_get_geometry(ria_gpu_handle h, ria_gpu_geometry* out);

/* Execution knobs of a handle.  None of them changes a result; the parity tests run the fused call under every
 * value and compare.
 *   RIA_OPT_SPLIT_PARTS  ria_gpu_rx_batch cuts a batch of >= 4096 frames into this many parts that run on internal
 *                        streams (1..4; 1 = one stream, no overlap; 0 = library default (3; 2 from 32768 frames on), which the environment
 *                        variables RIA_SPLIT_PARTS / RIA_NO_SPLIT may override). */
#define RIA_OPT_SPLIT_PARTS 1
/*   RIA_OPT_DUAL_DECODER the retry kernels (phase 0, cascade) decode two codewords per wavefront on an interleaved LDS
 *                        image (ldpc_dual.hip.h): 1 = on, -1 = off, 0 = library default (off).  An experiment record that
 *                        measured slower: only in builds made with -DRIA_WITH_DUAL_DECODER; elsewhere 1 is RIA_ERR_UNSUPPORTED. */
#define RIA_OPT_DUAL_DECODER 2
/*   RIA_OPT_FALLBACK_QUEUE_ALL  the CRC recovery's fallback stage re-decodes each codeword of an unrepaired frame at four
 *                        factors and substitutes one result at a time.  0 (default): only the re-decodes of codewords
 *                        through which a substitution can make the frame verify are run - codeword 0 always, codeword
 *                        c >= 1 only if the header in codeword 0 parses and the frame's bytes reach into c.  1: every missing
 *                        re-decode is run, the others for nothing (the behaviour before the rule; kept to measure it). */
#define RIA_OPT_FALLBACK_QUEUE_ALL 3
/*   RIA_OPT_STATE_EXIT   the retry kernels whose failed decodes leave no bits behind (phase 0, cascade, recovery fill) end
 *                        a decode that has not converged once its complete message state equals, bit for bit, the state
 *                        24 iterations earlier (compared after iterations 46 and 70): it can only repeat itself, so it is
 *                        reported as the 80-iteration failure it would become.  The state is the 36 words a lane carries
 *                        from one iteration into the next; its copy lives in an area of device memory per persistent
 *                        workgroup and stream slot (113 MB at the default grid, reserved at R1/2 and R1/3 only).
 *                        1 (default) = on at R1/2 and R1/3, the shapes that keep every such word in registers (no effect
 *                        at other rates).  0 = off: every failing decode runs to its last iteration, the same kernels
 *                        make no copy.  Outputs are identical either way.  The
 *                        environment variable RIA_STATE_EXIT=1 / 0 sets the default of handles created after it.
 *                        ria_gpu_debug_state_exits counts the exits. */
#define RIA_OPT_STATE_EXIT 4
int  ria_gpu_set_option(ria_gpu_handle h, int option, int value);

/* ---- RX: demodulate  (IWaveform::process + getSoftBits, waveform_interface.hpp:124,135;
 *          OFDMChirpWaveform::process ofdm_chirp_waveform.cpp:391-468) ------------------------- */
/* samples_dev: frame f starts at samples_dev + (frame_offsets_dev ? frame_offsets_dev[f] : f*frame_samples)
 * and must hold frame_samples floats from the first LTS sample on.  meta_dev may be NULL (cfo 0).
 * llr_out_dev: n_frames * llrs_per_frame floats.  status_dev may be NULL. */
int ria_gpu_demod_batch(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                        const ria_frame_meta* meta_dev, int n_frames,
                        float* llr_out_dev, ria_frame_status* status_dev, void* stream);

/* ---- LLR input domain of every LDPC decode (ria_gpu_ldpc_decode_batch, ria_gpu_ldpc_decode_robust_batch,
 * ria_gpu_decode_batch, ria_gpu_rx_batch, ria_gpu_rx_acquire_batch, ria_gpu_mcdpsk_acquire_batch) -----------------
 * Each LLR x goes through canon(x) before the first iteration:
 *   NaN -> +1e30;  x > +1e30 (+inf included) -> +1e30;  x < -1e30 (-inf included) -> -1e30;  -0.0 -> +0.0;
 *   every other value unchanged (f32 denormals are kept, not flushed).
 * Bit-exact with LDPCDecoder::decodeBP (ok, lastIterations(), bytes) for every finite |x| <= 1e30, zeros and
 * denormals included, at any max_iterations >= 0 and any min-sum factor in (0, 1]: the reference itself treats -0.0 and
 * +0.0 alike (it only tests x < 0 and |x|).  For NaN, +-inf and finite |x| > 1e30 the result is the reference's
 * answer on canon(x), which differs from its answer on the raw value where the raw value would turn its sums into
 * inf or NaN.  max_iterations 0: ok 0, iterations 0, bytes = the hard bits (x < 0) of the input. */

/* ---- RX: decode  (protocol::v2::decodeFixedFrame, frame_v2.hpp:848, frame_v2.cpp:1335-1883) --- */
/* llr_dev: frame f at llr_dev + f*llr_stride (first 2592 used).  info_out_dev: n_frames *
 * info_bytes_per_frame.  status_dev: n_frames entries. */
int ria_gpu_decode_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, int n_frames,
                         uint32_t flags, uint8_t* info_out_dev, ria_decode_status* status_dev, void* stream);

/* Single-codeword decoder (LDPCDecoder::decodeSoft, include/ultra/fec.hpp:48-81): n_cw rows of 648
 * LLRs already in decoder order; out: n_cw * ceil(ldpc_k/8) bytes (ria_gpu_geometry.ldpc_k); ok/iters: n_cw entries. */
int ria_gpu_ldpc_decode_batch(ria_gpu_handle h, const float* llr_dev, int n_cw, int max_iterations,
                              float min_sum_factor, uint8_t* out_dev, uint8_t* ok_dev,
                              uint16_t* iters_dev, void* stream);

/* robustDecodeSingleCW (src/gui/modem/streaming_decoder.cpp:1028-1058; the per-codeword decoder of the MC-DPSK and
 * control-frame paths, :1290,:1454,:2620): a fresh LDPCDecoder at getRecommendedIterations(rate), min-sum factor
 * 0.9375, then 0.875 / 0.75 / 0.625 / 0.5 until one converges.  n_cw rows of 648 LLRs in decoder order; out: n_cw *
 * ceil(ldpc_k/8) bytes (the last attempt's hard bits; the reference returns them only when ok); tries_dev (nullable):
 * decodes made, 1..5; iters_dev: lastIterations() of the last one. */
int ria_gpu_ldpc_decode_robust_batch(ria_gpu_handle h, const float* llr_dev, int n_cw, uint8_t* out_dev, uint8_t* ok_dev,
                                     uint16_t* iters_dev, uint8_t* tries_dev, void* stream);

/* ---- RX: fused samples -> payload (process + getSoftBits + decodeFixedFrame in one pass) ------ */
/* llr_out_dev and demod_status_dev may be NULL. */
int ria_gpu_rx_batch(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                     const ria_frame_meta* meta_dev, int n_frames, uint32_t flags,
                     uint8_t* info_out_dev, ria_decode_status* decode_status_dev,
                     float* llr_out_dev, ria_frame_status* demod_status_dev, void* stream);

/* Host-buffer forms for the single-frame IWaveform adaptor (n_frames small): the caller's buffers are ordinary host
 * memory; the library stages them through a pinned + device block it keeps for the life of the handle (no allocation
 * per call), runs on its own stream and returns when the results are in the caller's buffers. */
int ria_gpu_rx_frames_host(ria_gpu_handle h, const float* samples_host, const ria_frame_meta* meta_host,
                           int n_frames, uint32_t flags, uint8_t* info_out_host,
                           ria_decode_status* decode_status_host, float* llr_out_host,
                           ria_frame_status* demod_status_host);

/* Host-buffer decodeFixedFrame (llr_host: n_frames rows of llr_stride floats, first 2592 used). */
int ria_gpu_decode_frames_host(ria_gpu_handle h, const float* llr_host, int llr_stride, int n_frames, uint32_t flags,
                               uint8_t* info_out_host, ria_decode_status* status_host);

/* ---- TX synthesis for Monte-Carlo sweeps (v2::encodeFixedFrame frame_v2.cpp:1285-1328 +
 *      OFDMModulator::generateTrainingSymbols/modulate modulator.cpp:534-583, :348-477) ---------- */
/* info_dev: n_frames * info_bytes_per_frame (already serialized frames, zero padded; any bytes are taken: the encoder reads
 * the first min(ldpc_k, 8 * bytes_per_codeword) bits of each codeword's bytes and pads the rest of the code's k bits with zeros);
 * samples_out_dev: n_frames * frame_samples.  peak_normalize: scale every frame to this peak
 * (0 = leave the modulator's output_scale 40 level; tools/test_waveform_simple.cpp:365-371 uses 0.8).
 * The rule, in float32, per frame: where peak_normalize > 0 is true, every sample s becomes s * (peak_normalize / max|s|),
 * the quotient correctly rounded; otherwise (0, -0.0, any negative value, NaN) the samples stay at the modulator's level.
 * Nothing else is checked: a tiny value gives denormal samples (not flushed), a value whose quotient or products overflow
 * gives +-inf there (3e38 does for a frame that peaks under 0.88), and +inf gives +-inf at every non-zero sample and, by
 * the same rule, NaN at an exactly zero sample (0 * inf; the tests have no such sample, the NaN's bits are not pinned).
 * max|s| > 0 always, the two training symbols are never silent.  n_frames 0 is RIA_OK and writes nothing. */
int ria_gpu_tx_batch(ria_gpu_handle h, const uint8_t* info_dev, int n_frames, float peak_normalize,
                     float* samples_out_dev, void* stream);
/* The same in two steps, split at the coded bytes where the burst interleaver works (streaming_encoder.cpp:302-389):
 * encodeFixedFrame alone (coded_out_dev: n_frames * 324 bytes, channel interleaved, MSB first), and the modulator on such
 * bytes (e.g. ria_gpu_burst_interleave_batch's output).  tx_coded(encode_frames(info)) is ria_gpu_tx_batch(info) bit for bit. */
int ria_gpu_encode_frames_batch(ria_gpu_handle h, const uint8_t* info_dev, int n_frames, uint8_t* coded_out_dev, void* stream);
int ria_gpu_tx_coded_batch(ria_gpu_handle h, const uint8_t* coded_dev, int n_frames, float peak_normalize,
                           float* samples_out_dev, void* stream);

/* Builds serialized v2 data frames (makeFixedDataFrame("TEST","RX",seq,payload).serialize(),
 * frame_v2.cpp:1890-1912, :502-554) with payload bytes drawn from a counter RNG: seq = first_seq + f.
 * Frame f depends on (seed, first_seq + f) alone, not on how a batch is split: its payload comes from Philox4x32-10 with
 * key = the two 32-bit words of seed and counter word 0 = (first_seq + f) mod 2^32, all 32 bits; the frame's seq field is
 * the low 16 bits of that number.  So first_seq and first_seq + 65536 give the same seq and different payloads.  A negative
 * first_seq is taken as first_seq + 2^32 (make_frames(seed, -1, 2) builds the frames 2^32 - 1 and 0): it is not refused. */
int ria_gpu_make_frames(ria_gpu_handle h, uint64_t seed, int first_seq, int n_frames,
                        uint8_t* info_out_dev, void* stream);

/* ---- channel simulator (sim::WattersonChannel, src/sim/hf_channel.hpp:35-303, presets :411-488)
 * kind: 0 awgn, 1 good, 2 moderate, 3 poor, 4 flutter.  In place on n_frames * frame_samples.
 * Frame f uses the counter-RNG stream (seed, first_frame + f): results do not depend on how frames
 * are split over calls or GPUs.  Statistical (not bit) parity with the reference's mt19937 stream. */
int ria_gpu_channel_batch(ria_gpu_handle h, int kind, float snr_db, uint64_t seed, uint64_t first_frame,
                          float* samples_dev, int n_frames, void* stream);

/* ---- acquisition: Zadoff-Chu preamble (sync::ZCSync, src/sync/zc_sync.hpp) -----------------------
 * ria_gpu_sync_zc_batch replaces ZCSync::detect(samples, threshold, debug=false, root_mask, known_cfo_hz)
 * (zc_sync.hpp:192-391) for n_buffers capture buffers of buf_len samples each (buffer b starts at
 * samples_dev + b*stride).  root_mask bits 0..3 = PING/PONG/DATA/CONTROL roots 1/3/5/7 (ZC_ROOT_MASK_*).
 * known_cfo_dev: per-buffer known CFO in Hz, or NULL for 0.  Results are bit-identical to the reference's
 * ZCSyncResult for every field (snr_estimate included).  buf_len <= 1048576: buffers up to 16384 samples are mixed down
 * into the workgroup's LDS (the batched acquisition sweeps), longer ones (the host's connected-mode search windows of
 * 31 000 - 48 000 samples, streaming_decoder.cpp:424-431) into a device workspace the handle keeps.
 *
 * Input domain of the four detectors (ZC, dual chirp, LTS light sync, Schmidl-Cox).  Samples may be any float32: NaN,
 * +-inf, denormals, +-FLT_MAX or so large that the window energies overflow.  The threshold, the known CFO and the initial
 * noise floor may be any float32 too, NaN and +-inf included.  None of these makes the reference undefined: it converts no
 * float of the data to an index, every compare with a NaN is false, and its complex products go through std::complex's
 * operator* (C99 Annex G: an infinite factor gives an infinite product), so nothing is out of contract and the answer is
 * the reference's in every case.  What follows from that: a correlation that comes out NaN never wins a maximum search;
 * std::max(combined, peak) keeps a NaN combined metric (zc_sync.hpp:289), which drops that root; a NaN threshold detects
 * nothing where the compare is `corr > threshold` (ZC, LTS, Schmidl-Cox) and rejects nothing where it is
 * `corr < threshold` (the chirp transform path, chirp_sync.hpp:707); a NaN noise floor fails every energy gate of
 * searchForSync and is returned as it came.  A float field of a result may be NaN; the sign and payload of such a NaN are
 * not part of the contract.  tests/sync_domain_inputs.py holds the buffers these statements are tested on. */
typedef struct ria_zc_result {
    int32_t detected;        /* ZCSyncResult::detected */
    int32_t frame_type;      /* ZCFrameType: 0 PING 1 PONG 2 DATA 3 CONTROL 255 UNKNOWN */
    int32_t start_sample;    /* first sample after the preamble, -1 if not detected */
    int32_t root_detected;   /* best root even below threshold, -1 if none */
    float correlation;
    float cfo_hz;
    float snr_estimate;
    float reserved;
} ria_zc_result;             /* 32 bytes */
int ria_gpu_sync_zc_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                          float threshold, uint32_t root_mask, const float* known_cfo_dev,
                          ria_zc_result* out_dev, void* stream);
/* ZCSync::generatePreambleForRoot (zc_sync.hpp:133-190) into a HOST buffer (2512 samples); returns the
 * sample count, or -needed if max_n is too small.  Bit-identical audio. */
int ria_gpu_zc_preamble(ria_gpu_handle h, int root, float* out_host, int max_n);

/* ---- acquisition: dual chirp (sync::ChirpSync, src/sync/chirp_sync.hpp) ----------------------------
 * ria_gpu_sync_chirp_batch replaces ChirpSync::detectDualChirp(samples, threshold) (chirp_sync.hpp:352-512)
 * with the OFDM-CHIRP configuration (300 -> 2700 Hz, 500 ms, 100 ms gap, dual chirp; getChirpConfig,
 * ofdm_chirp_waveform.cpp:46-56) for n_buffers buffers of buf_len samples (buffer b at samples_dev + b*stride).
 * Every field is bit-identical to the reference's DualChirpResult. */
typedef struct ria_chirp_result {
    int32_t success;
    int32_t up_chirp_start;      /* CFO-corrected, -1 if not detected */
    int32_t down_chirp_start;
    float cfo_hz;
    float up_correlation;
    float down_correlation;
    int32_t reserved[2];
} ria_chirp_result;              /* 32 bytes */
int ria_gpu_sync_chirp_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                             float threshold, ria_chirp_result* out_dev, void* stream);
/* ChirpSync::generate (chirp_sync.hpp:61-108): the 57 600-sample dual-chirp preamble into a HOST buffer;
 * returns the sample count or -needed. */
int ria_gpu_chirp_preamble(ria_gpu_handle h, float* out_host, int max_n);

/* ---- acquisition: LTS light sync (OFDMChirpWaveform::detectDataSync, ofdm_chirp_waveform.cpp:207-384) -------
 * Training-only preamble of connected-mode DATA frames: energy gate, Hilbert-65 analytic signal, one-symbol
 * autocorrelation (coarse step 8, early exit above 0.95, +-4 refinement), burst-interleave marker.
 * Replaces detectDataSync(samples, result, known_cfo_hz, threshold) for n_buffers buffers; every field of
 * SyncResult it sets is bit-identical (start_sample = first sample of the first LTS symbol). */
typedef struct ria_lts_result {
    int32_t detected;
    int32_t start_sample;
    float correlation;
    float cfo_hz;               /* = known_cfo_hz (SyncResult::cfo_hz) */
    int32_t burst_interleaved;  /* wasBurstInterleaved() */
    int32_t reserved[3];
} ria_lts_result;               /* 32 bytes */
int ria_gpu_sync_lts_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                           const float* known_cfo_dev, float threshold, ria_lts_result* out_dev, void* stream);

/* ---- Schmidl-Cox acquisition of the OFDM-COX waveform
 * Replaces OFDMDemodulator::searchForSync(samples, out_position, out_cfo_hz, threshold)
 * (src/ofdm/demodulator.cpp:1450-1542) as OFDMNvisWaveform::detectSync drives it
 * (src/waveform/ofdm_cox_waveform.cpp:125-158), for n_buffers capture buffers: energy gate with the
 * demodulator's noise-floor tracker (ofdm_sync.cpp:20-50), half-symbol Schmidl-Cox metric on the FFT-Hilbert
 * analytic signal (ofdm_sync.cpp:56-86,118-163) on the 64-sample search grid and the 8-sample plateau grid,
 * plateau rule (>= 15 of 38 points at >= 0.90), passband LTS fine timing with the earlier-LTS preference and
 * the 0.05 confirmation threshold (ofdm_sync.cpp:386-484), coarse CFO (ofdm_sync.cpp:230-261).  All fields
 * bit-identical.  noise_floor_dev (may be NULL = fresh demodulator, 0) holds Impl::noise_floor_energy per buffer
 * before the call; the value after the call is returned in the result.  buf_len <= 240000
 * (MAX_BUFFER_SAMPLES). */
typedef struct ria_cox_result {
    int32_t found;
    int32_t start_sample;       /* first sample of the first LTS symbol (SyncResult::start_sample) */
    float cfo_hz;
    float noise_floor;          /* Impl::noise_floor_energy after the search */
    int32_t sts_position;       /* Schmidl-Cox plateau peak the LTS refinement started from */
    int32_t reserved[3];
} ria_cox_result;               /* 32 bytes */
int ria_gpu_sync_cox_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int buf_len, int n_buffers,
                           float threshold, const float* noise_floor_dev, ria_cox_result* out_dev, void* stream);
/* OFDMModulator::generatePreamble (src/ofdm/modulator.cpp:479-532) for the handle's configuration: one symbol
 * of silence, 4 STS, 2 LTS = 8064 samples, bit-identical.  Returns the sample count (negative = needed). */
int ria_gpu_cox_preamble(ria_gpu_handle h, float* out_host, int max_n);

/* Single-buffer convenience forms for the IWaveform adaptor (host memory in, result by value; they stage
 * through device memory and synchronise).  kind: 0 dual chirp (ria_chirp_result), 1 LTS light sync
 * (ria_lts_result), 2 ZC (ria_zc_result), 3 Schmidl-Cox (ria_cox_result); param = known CFO in Hz (kinds 1, 2) or
 * the initial noise floor (kind 3), root_mask only for kind 2. */
int ria_gpu_sync_host(ria_gpu_handle h, int kind, const float* samples_host, int n_samples, float threshold, float param,
                      uint32_t root_mask, void* result_out /* 32 bytes */);

/* ---- MC-DPSK demodulator (src/psk/multi_carrier_dpsk.hpp) and HARQ chase combine (src/fec/chase_cache.cpp)
 * ria_gpu_mcdpsk_demod_batch replaces MultiCarrierDPSKDemodulator as MCDPSKWaveform::process drives it after
 * an external chirp detection (setChirpDetected + process, multi_carrier_dpsk.hpp:797-896): each frame is
 * training (8 x 512) + reference (512) + data symbols, frame f at samples_dev + f*stride; per-frame CFO (Hz)
 * and initial CFO phase (rad) may be NULL (0).  LLRs come out as demodulateSoft returns them
 * ((frame_samples/512 - 9)/spreading * carriers * bits_per_symbol values), bit-identical. */
typedef struct ria_mcdpsk_config {
    int32_t num_carriers;      /* 1..20 (reference default 8; MC-DPSK modes use 10); one carrier sits on 1500 Hz; MCDPSKWaveform clamps to 3..20 */
    int32_t bits_per_symbol;   /* 1 DBPSK, 2 DQPSK */
    int32_t spreading;         /* 1, 2 or 4 (SpreadingMode) */
    int32_t reserved;
} ria_mcdpsk_config;
typedef struct ria_mcdpsk_status {
    float cfo_hz;                  /* getEstimatedCFO() after the frame */
    float fading_index;            /* getFadingIndex() */
    float freq_fading_index;
    float temporal_fading_index;
    float training_cfo_residual;   /* processTraining's estimate (not applied after an external chirp) */
    int32_t n_llr;
    int32_t valid_symbols;
    int32_t reserved;
} ria_mcdpsk_status;               /* 32 bytes */
int ria_gpu_mcdpsk_demod_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                               int frame_samples, int n_frames, const float* cfo_hz_dev, const float* phase0_dev,
                               float* llr_out_dev, int llr_stride, ria_mcdpsk_status* status_dev, void* stream);
/* Host-buffer forms for the single-frame MC-DPSK plug-in adaptor (MCDPSKWaveform::process -> getSoftBits,
 * src/waveform/mc_dpsk_waveform.cpp:294-338; robustDecodeSingleCW, streaming_decoder.cpp:1028-1058): ordinary host memory
 * in and out, staged on the handle's own stream, return when done.  demod: one frame (training + reference + data,
 * n_samples >= 10 * 512); llr_out_host gets the soft bits as demodulateSoft returns them (count in status_out->n_llr). */
int ria_gpu_mcdpsk_demod_host(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_host, int n_samples, float cfo_hz,
                              float phase0, float* llr_out_host, int max_llr, ria_mcdpsk_status* status_out);
int ria_gpu_ldpc_decode_robust_host(ria_gpu_handle h, const float* llr_host, int n_cw, uint8_t* out_host, uint8_t* ok_host,
                                    uint16_t* iters_host /* nullable */, uint8_t* tries_host /* nullable */);
/* MultiCarrierDPSKModulator: generateTrainingSequence + generateReferenceSymbol + modulate(data) into a HOST
 * buffer (multi_carrier_dpsk.hpp:141-281); returns the sample count or -needed.  Bit-identical audio. */
int ria_gpu_mcdpsk_modulate_host(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const uint8_t* data, int n_bytes,
                                 float* out_host, int max_n);
/* The same modulator for a batch on the device: data_dev = n_frames rows of n_bytes coded bytes, frame f written to
 * out_dev + f*out_stride ((9 + ceil(8 n_bytes / (carriers * bits)) * spreading) * 512 samples).  Bit-identical audio. */
int ria_gpu_mcdpsk_modulate_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const uint8_t* data_dev, int n_bytes, int n_frames,
                                  float* out_dev, int64_t out_stride, void* stream);
/* fec::ChaseCache::store arithmetic for n_cw codeword slots of 648 LLRs (chase_cache.cpp:27-88): count 0 ->
 * copy, else add; skipped when decoded_dev[cw] != 0 or count >= 4.  stored_out_dev (nullable) gets 1/0.
 * decoded_dev is nullable (nothing decoded); n_cw 0 returns RIA_OK without reading a pointer.  The add is one float add per
 * element on the raw values: NaN, infinities and denormals go in and come out as IEEE arithmetic gives them (inf + -inf
 * = NaN, no flush to zero; a NaN's sign and payload are unspecified).  The call itself only produces counts 0 .. 4; handed
 * another one it treats a count above 4 like 4 (skipped) and a negative count like 1 .. 3 (added, count + 1). */
int ria_gpu_chase_combine_batch(ria_gpu_handle h, float* acc_dev, int32_t* count_dev, const uint8_t* decoded_dev,
                                const float* soft_dev, int n_cw, uint8_t* stored_out_dev, void* stream);

/* ---- link adaptation ladder (host scalars; src/protocol/waveform_selection.hpp:49-104,112-222,250-314) -----
 * waveform: protocol::WaveformMode value (4 MC_DPSK, 5 OFDM_CHIRP); spreading 1/2/4. */
typedef struct ria_link_recommendation {
    int32_t waveform;
    int32_t modulation;
    int32_t code_rate;
    int32_t spreading;
    int32_t num_carriers;
    float estimated_throughput_bps;   /* 0 from ria_link_data_mode for OFDM (the reference does not report one) */
} ria_link_recommendation;
void ria_link_recommend(float snr_db, float fading_index, ria_link_recommendation* out);          /* recommendWaveformAndRate */
void ria_link_data_mode(float snr_db, int waveform, float fading_index, ria_link_recommendation* out);   /* recommendDataMode */
int ria_link_ofdm_code_rate(float snr_db, float fading_index);                                     /* selectOFDMCodeRate */
int ria_link_cap_initial_rate(float snr_db, float fading_index, int candidate_rate);               /* capInitialOFDMRate */

/* LDPCEncoder::encode for n_cw codewords on the host (src/fec/ldpc_encoder.cpp:193-257): info = n_cw * ceil(k/8)
 * bytes (MSB first), coded_out = n_cw * 81 bytes.  Used to synthesise MC-DPSK frames (the OFDM TX kernel
 * encodes on the device). */
int ria_gpu_ldpc_encode_host(ria_gpu_handle h, const uint8_t* info, int n_cw, uint8_t* coded_out);

/* The same channel with the REFERENCE's random stream: frame f is sim::WattersonChannel(cfg, seed32) with
 * seed32 = (uint32_t)(seed + first_frame + f) (std::mt19937 + std::normal_distribution<float>, five draws per
 * sample), so the output is bit-identical to the reference channel (and to tools/test_waveform_simple.cpp's
 * "channel seed = base + frame" convention).  Any frame length; frame f at samples_dev + f*stride; in place.
 *
 * Input domain of the three reference-identical channel calls (this one, _seeded_batch, _cfo_batch).  Samples, snr_db and
 * the per-frame offsets cfo_hz_dev[f] may be any float32: NaN, +-inf, denormals, +-FLT_MAX.  Seeds are any uint32;
 * seed + first_frame + f is taken modulo 2^32 (first_frame 2^32 + 5 is first_frame 5).  None of these makes the reference
 * undefined (it converts no sample to an index and every compare with a NaN is false), so the answer is the reference's:
 *   - a sample counts for the signal power when |x| > 1e-6f: exactly +-1e-6f, denormals and NaN do not count, +-inf does;
 *     a frame without a counted sample has rms 0.1; a power that overflows (one sample of 3e19) makes the noise sigma +inf
 *     and every output sample non-finite;
 *   - snr_db 800 gives the denormal sigma 1e-40 * rms (powf does not underflow to 0 there), 1e30 and +inf give sigma 0
 *     (the noiseless fade), -inf and NaN leave no finite output sample;
 *   - one NaN sample gives a NaN at its index and, in the two-path presets, delay + 1 samples later (the delay line
 *     holds delay + 1 = 25, 49 or 97 samples), nowhere else; under applyCFO every sample from its index on is NaN;
 *   - the channel applies its offset when |offset| > 0.001f is true and the frame has at least 256 samples: exactly
 *     +-0.001f and NaN are NOT applied (ria_gpu_tx_cfo_batch's gate is the other way round, see there).  The phase starts
 *     at 0, grows by float(2 pi offset / 48000) and wraps at most once per sample and only downwards (phase > 2 pi), so
 *     a negative offset never wraps and an increment above 2 pi (48000.5 Hz, 1e6 Hz) grows without bound; cos and sin of
 *     such phases are the correctly reduced glibc values.  An infinite offset rotates sample 0 by the phase 0 (finite)
 *     and leaves NaN from sample 1 on;
 *   - random_cfo_max_hz > 0 draws (2 max) * u - max in float: FLT_MAX gives +inf (or NaN for u = 0), +inf gives NaN, the
 *     smallest denormal gives +-denormal or 0, which the gate then drops.
 * Bits are compared wherever the reference's value is not NaN; where it is NaN the device's value is NaN, sign and payload
 * of a NaN are not part of the contract.  Refused with RIA_ERR_INVALID, nothing launched: kind outside 0..4, n_frames < 0,
 * frame_samples < 0, stride < frame_samples, a null samples or seeds pointer with a non-empty batch, random_cfo_max_hz
 * negative or NaN.  n_frames == 0 or frame_samples == 0 is RIA_OK and writes nothing.  Samples between frame_samples and
 * stride are neither read nor written.  tests/channel_domain_inputs.py holds the rows these statements are tested on. */
int ria_gpu_channel_exact_batch(ria_gpu_handle h, int kind, float snr_db, uint32_t seed, uint64_t first_frame,
                                float* samples_dev, int64_t stride, int frame_samples, int n_frames, void* stream);

/* The same channel with one mt19937 seed PER FRAME (seeds_dev[f]): Monte-Carlo drivers derive the seed of a trial from
 * (base seed, sweep point, transmission number, global trial index), so that a trial's noise does not depend on how
 * trials are batched, compacted or spread over GPUs.  Frame f = sim::WattersonChannel(cfg, seeds_dev[f]), bit-identical. */
int ria_gpu_channel_exact_seeded_batch(ria_gpu_handle h, int kind, float snr_db, const uint32_t* seeds_dev, float* samples_dev,
                                       int64_t stride, int frame_samples, int n_frames, void* stream);

/* The same channel object with its CFO impairment (hf_channel.hpp:47-51 Config::cfo_hz / random_cfo_max_hz): frame f =
 * sim::WattersonChannel(cfg{cfo_hz = cfo_hz_dev[f] (NULL: 0), random_cfo_max_hz}, seeds_dev[f]).process(frame f).
 * random_cfo_max_hz > 0 replaces the configured offset by the constructor's uniform draw from the frame's own generator
 * (:97-102; it takes the first random word, so every later noise value shifts); the noise / fading pass is followed by
 * applyCFO (:172-174, :182-241: mix to baseband at 1500 Hz, 48-sample running-sum average, rotate, mix back) whenever
 * |offset| > 0.001 Hz and the frame has at least 256 samples.  actual_cfo_out_dev (nullable, n_frames floats) =
 * getActualCFO().  Bit-identical output. */
int ria_gpu_channel_exact_cfo_batch(ria_gpu_handle h, int kind, float snr_db, const uint32_t* seeds_dev, const float* cfo_hz_dev,
                                    float random_cfo_max_hz, float* actual_cfo_out_dev, float* samples_dev, int64_t stride,
                                    int frame_samples, int n_frames, void* stream);

/* The simulator's transmitter frequency offset: SimulatedChannel::applyTxCFO(samples, phase_acc)
 * (tools/cli_simulator.cpp:298-341; BASELINE.json config 4's "+-50 Hz CFO" by analytic-signal rotation) for n_buffers
 * transmissions of n_samples each (buffer b at samples_dev + b*stride, result at out_dev + b*out_stride, not in place):
 * FFT of the next power of two, frequency-domain Hilbert, inverse FFT, rotation by cfo_hz_dev[b] with the wrapped float
 * phase accumulator phase_inout_dev[b] (NULL: starts at 0, not returned), real part.  |cfo| < 0.001 Hz copies the
 * samples and leaves the accumulator alone, as the reference does.  n_samples <= 131072.  Bit-identical output.
 *
 * Input domain.  cfo_hz_dev[b] and phase_inout_dev[b] may be any float32.  The gate is `|cfo| < 0.001f copies`: exactly
 * +-0.001f and NaN ROTATE here, while the channel calls above apply their offset only when |offset| > 0.001f; the two
 * gates are the reference's and differ at exactly +-0.001f.  Below the gate the output is a bit copy and the accumulator is
 * not touched, whatever it holds (NaN, 100.0).  The increment is 2 * float(pi) * cfo / 48000 in float (1e38 overflows to
 * +inf in the first product); after each sample the phase wraps once, p > float(pi) -> p - 2 float(pi), else
 * p < -float(pi) -> p + 2 float(pi): an accumulator outside (-pi, pi] (3.2, 100.0, 1e9) or an increment above 2 pi comes
 * back by one turn per sample only, and cos / sin are taken of the phase as it is.  A NaN or infinite accumulator or
 * increment gives NaN output from the sample it is first used for and is returned as the reference returns it (bits
 * compared where the reference's value is not NaN, "is NaN" where it is).  A call that continues from a returned
 * accumulator walks the same phases as one call over both lengths.  Samples may be any finite float32 whose transform
 * stays finite (denormals, +-FLT_MAX/4 at n <= 4, silence: bit-identical).  A NaN or infinite sample in a rotated buffer is
 * outside bit identity: the reference's butterflies multiply with std::complex's operator* (C99 Annex G turns a NaN + NaN i
 * product with an infinite factor into an infinity), the kernels multiply by hand.  For such a buffer every output sample
 * is non-finite (as in the reference), the accumulator is the reference's, and every other buffer of the batch is
 * unaffected; so is a finite buffer whose transform overflows.  Below the gate such samples are copied like any other.
 * Refused with RIA_ERR_INVALID, nothing launched: out_dev == samples_dev, a null samples, offsets or output pointer,
 * n_buffers < 0, n_samples < 0, stride or out_stride < n_samples; n_samples > 131072 is RIA_ERR_UNSUPPORTED.
 * n_samples == 0 or n_buffers == 0 is RIA_OK and writes nothing.  The input is never written; output samples between
 * n_samples and out_stride are not written.  Batches above 32 768 buffers or 256 MiB of workspace (two complex
 * N-point arrays and one float per sample for every buffer) run as several passes with the same result. */
int ria_gpu_tx_cfo_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int n_samples, int n_buffers,
                         const float* cfo_hz_dev, float* phase_inout_dev, float* out_dev, int64_t out_stride, void* stream);

/* ---- burst interleaver (fec::BurstInterleaver, src/fec/burst_interleaver.cpp:8-78) -----------------
 * A burst of N physical frames carries N logical frames byte-interleaved: physical[(N*b+f)/324][(N*b+f)%324] =
 * logical[f][b].  deinterleave works on the soft bits (8 per byte) of n_groups bursts of N frames each:
 * frame j of group g at llr_dev + (g*N + j)*llr_stride (first 2592 used), same layout out.  interleave is the
 * TX side on coded bytes (324 per frame).  N < 2 copies. */
int ria_gpu_burst_deinterleave_batch(ria_gpu_handle h, const float* physical_llr_dev, int llr_stride, int burst_frames,
                                     int n_groups, float* logical_llr_out_dev, void* stream);
int ria_gpu_burst_interleave_batch(ria_gpu_handle h, const uint8_t* logical_bytes_dev, int burst_frames, int n_groups,
                                   uint8_t* physical_bytes_out_dev, void* stream);

/* ---- acquire + decode: connected-mode OFDM-CHIRP data frames with timing recovery ------------------
 * ria_gpu_rx_acquire_batch replaces what gui::StreamingDecoder does with one search window of a connected-mode DATA frame
 * (src/gui/modem/streaming_decoder.cpp): detectDataSync on the window with the known CFO (:723-735), the acceptance test
 * against light_sync_min_confidence (:679-699, :752-771), setAbsoluteTrainingPosition + setFrequencyOffset + process()
 * at the found position (:891-897, :1345-1349), decodeFixedFrame (:2936-2940), and multi-candidate timing recovery
 * (:1855-1965): when no codeword decodes, the frame is demodulated and decoded again at +8, -8, +16, -16, +24, -24, +32,
 * -32 samples and the first candidate that decodes anything is kept.
 *
 * Window geometry: window b starts at samples_dev + b*stride and holds window_len samples; the detector sees its first
 * search_len (search_len <= window_len <= stride).  A candidate starting at s runs only if s >= 0 and
 * s + frame_samples <= window_len.  If the primary candidate (s = sync_start) does not fit, the window is not accepted.
 * A recovery candidate that does not fit is skipped and not counted (the reference reads older ring-buffer samples
 * there instead).
 *
 * Primary candidate: delta 0, meta.flags bit0 = the detector's burst marker, abs_position = abs_base + sync_start,
 * CFO = known_cfo_hz.  Recovery runs only when the primary's decode status has no cw_ok set (the reference's
 * `!success && codewords_ok == 0`); every recovery candidate has meta.flags 0 (process() consumes the burst marker as a
 * one-shot, ofdm_chirp_waveform.cpp:421-427, and reset() does not re-arm it, :474-485), abs_position = abs_base +
 * sync_start + delta and the same known CFO.  The first candidate with any cw_ok is reported (its bytes, decode status
 * and demod status); if none decodes anything, the primary's outputs are reported with delta 0.  Windows that are not
 * accepted get zero bytes and zero statuses; detected, sync_start and correlation are still filled in.
 *
 * flags: the RIA_DECODE_* bits (RIA_DECODE_NO_CHANNEL_DEINTERLEAVE included) plus RIA_ACQ_NO_TIMING_RETRY (primary
 * candidate only); RIA_RX_DEMOD_ONLY is RIA_ERR_INVALID.  A decode work-queue fault in any internal part of any round
 * fails the whole call with RIA_ERR_HIP.  The call synchronises its stream once per round for one small device-to-host
 * read (the length of the round's work list); no samples, soft bits or payloads go to the host.  Work grows with the
 * number of windows that fail: each round demodulates and decodes only the windows still failing, each at its own next
 * candidate.  Workspaces live on the handle and grow with n_windows.
 *
 * Not covered (the caller's side or other paths): decodeFrame's control-frame hypotheses on the soft bits (the R1/4 fast
 * path, the raw CW0 probe, the 1-CW salvage and the legacy path, :2866-3058) are ria_gpu_decode_frame_batch's, which takes
 * the soft bits this call can return; the control-first re-demodulation with the DQPSK R1/4 profile (:1268-1344) is
 * ria_gpu_control_acquire_batch's, run ahead of this call on a control handle; the short-span data-profile demodulation that
 * moves last_cfo_ (:1346-1434), the 1-CW peek buffer, the pending_total_cw_ escalation (:1505-1597) and the small-frame
 * recovery (:1806-1853) are ria_gpu_rx_window_batch's, which runs the whole window in one call; the weak-accept and reject-streak state (fold them into min_confidence, or take both from ria_gpu_search_batch, whose result
 * names this call's window and parameters), the PING
 * energy check, burst groups and burst continuation (ria_gpu_rx_burst_batch), chase combining, Schmidl-Cox
 * acquisition, OFDM-COX, ring-buffer wrap-around, and the +-2 Hz clamp of the reported CFO the host applies before it
 * feeds it back (:1912-1918).  MC-DPSK frames (ZC and dual-chirp acquisition, the disconnected handshake fallbacks) are
 * ria_gpu_mcdpsk_acquire_batch's. */
typedef struct ria_acq_params {      /* one per window, 32 bytes */
    float    known_cfo_hz;           /* detectDataSync's known CFO (last_cfo_, :726) and the CFO every candidate is demodulated with */
    float    detect_threshold;       /* detectDataSync threshold (CORR_DETECT_THRESHOLD 0.15 for OFDM, streaming_decoder.hpp:457) */
    float    min_confidence;         /* accepted iff detected && correlation >= min_confidence (light_sync_min_confidence) */
    uint32_t reserved0;
    uint64_t abs_base;               /* absolute sample index of window sample 0 (ringPosToAbsolute) */
    uint32_t reserved[2];
} ria_acq_params;

typedef struct ria_acq_result {      /* 32 bytes */
    int32_t detected;                /* the LTS detector's result */
    int32_t accepted;                /* detected && correlation >= min_confidence && the primary candidate fits the window */
    int32_t sync_start;              /* detector start_sample, -1 if not detected */
    int32_t frame_start;             /* start of the reported candidate = sync_start + delta, -1 if not accepted */
    float   correlation;
    float   cfo_hz;                  /* ria_frame_status.cfo_hz of the reported candidate (the estimatedCFO the host clamps), 0 if not accepted */
    int16_t delta;                   /* 0 = primary, else the recovery delta that was accepted */
    uint8_t candidates;              /* candidates demodulated and decoded: 0 (not accepted) .. 9 */
    uint8_t burst_interleaved;       /* detector's burst marker */
    int32_t reserved;
} ria_acq_result;

#define RIA_ACQ_NO_TIMING_RETRY 0x400u   /* primary candidate only */

/* info_out_dev: n_windows * info_bytes_per_frame; decode_status_dev, acq_dev: n_windows entries; demod_status_dev
 * (nullable): n_windows entries; params_dev: n_windows entries. */
int ria_gpu_rx_acquire_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int search_len, int window_len,
                             int n_windows, const ria_acq_params* params_dev, uint32_t flags,
                             uint8_t* info_out_dev, ria_decode_status* decode_status_dev, ria_acq_result* acq_dev,
                             ria_frame_status* demod_status_dev, void* stream);

/* ---- burst groups and burst continuation: what the receiver does behind the first data frame of a window -------------
 * ria_gpu_rx_burst_batch continues where ria_gpu_rx_acquire_batch stops (src/gui/modem/streaming_decoder.cpp).  Window
 * geometry, ria_acq_params, the detector, the acceptance rule (steps 1-2 above) and the RIA_DECODE_* /
 * RIA_DECODE_NO_CHANNEL_DEINTERLEAVE / RIA_ACQ_NO_TIMING_RETRY flags are ria_gpu_rx_acquire_batch's; two flags are new.
 * Every per-frame output has RIA_BURST_MAX_FRAMES slots per window (window b, slot f at index b * 9 + f); every slot of
 * every output the call does not fill is zero.
 *
 * Positions.  Physical frame f of a window starts at s_f = sync_start + f * frame_samples.  Frame 0's abs_position is
 * abs_base + sync_start and every later frame of the window is demodulated with the SAME abs_position: between the frames
 * of a burst the reference calls neither setAbsoluteTrainingPosition nor reset() (group path :3173-3175; continuation path
 * :2066-2067 - nothing between :1434 and :2015 on the path of a successful 4-codeword data frame calls either: the only
 * calls are in the timing-recovery candidates, :1891-1897, which such a frame does not reach).
 *
 * Energy gate of frame f >= 1 (:3154-3171 = :2047-2059): sum of x[s_f + 1024 + i]^2 for i < min(frame_samples - 1024, 5000),
 * in float32, ascending i, each product rounded before it is added (the library is built with -ffp-contract=off);
 * rms = sqrtf(sum / (float)len); the gate fails iff rms < 0.04f (a NaN passes).  rms_dev holds the value bit for bit, also
 * that of the frame the gate stopped.
 *
 * CFO chain (:1397-1406, :3190-3197, :2075-2082): c_0 = known_cfo_hz.  After frame f was demodulated with c_f and reports
 * e = ria_frame_status.cfo_hz: d = e - c_f; c_{f+1} = |d| > 2 ? c_f + copysignf(2, d) : e (a NaN drift leaves e).
 * cfo_used_dev[f] = c_f; ria_burst_result.cfo_hz = the last c computed = what the host would hold in last_cfo_.
 *
 * Group mode (mode 2): RIA_BURST_INTERLEAVE (use_burst_interleave_) is set and the accepted window's detector reports the
 * negated-LTS marker (:1378-1410, accumulateBurstFrames / tryDemodulateNextBurstFrame :3065-3208).  Frame 0 is
 * demodulated once with meta.flags = 1 and no timing recovery (nothing is decoded yet); n_llr == 0 is STOP_PROCESS.  Then
 * for f = 1 .. group_size - 1, in this order: the frame must lie in the window (s_f + frame_samples <= window_len, else
 * STOP_WINDOW: the reference would wait for samples), pass the gate (else STOP_ENERGY), be demodulated with flags 0 and
 * c_f (n_llr == 0: STOP_PROCESS), chain step.  Any stop aborts the group as the reference discards it (:3093-3108):
 * frames = the physical frames demodulated so far, frames_decoded = 0, no bytes and no decode status; the demod status,
 * cfo_used and rms slots of the frames that ran stay filled.  A complete group goes through
 * ria_gpu_burst_deinterleave_batch's permutation (finalizeBurstGroup :3210-3239) and decodeFixedFrame with the call's
 * decode flags on each logical frame: logical frame i in slot i of the bytes and decode status, frames_decoded =
 * group_size; the demod status slots hold the PHYSICAL frames.
 *
 * Continuation mode (mode 1): every other accepted window (:2015-2114).  Frame 0 is exactly what ria_gpu_rx_acquire_batch
 * reports for the window, timing recovery included, in slot 0 (a marked window without RIA_BURST_INTERLEAVE still has its
 * first LTS un-negated).  A frame 0 whose reported candidate has no soft bits (n_llr == 0) is STOP_PROCESS with frames = 0,
 * whatever RIA_BURST_NO_CONTINUE says: slot 0 and frames_decoded = 1 stay what the acquire rounds report, and the chain
 * does not step (cfo_hz = known_cfo_hz).  Continuation runs only if RIA_BURST_NO_CONTINUE is clear (else STOP_NONE), frame 0 is a success -
 * all four cw_ok and frame_valid, which is CodewordStatus::allSuccess() with a non-empty reassemble() for a fixed frame
 * (frame_v2.cpp:1030-1063) (else STOP_DECODE), byte 2 of the frame is neither a control nor a connect type
 * (frame_v2.hpp:222-228, :348-351; streaming_decoder.cpp:1994-1998) (else STOP_NOT_DATA), and delta == 0 (else
 * STOP_RECOVERED: the reference runs its recovery candidates with a sync_cfo_ the primary has already moved, :1433, :1903,
 * while ria_gpu_rx_acquire_batch deliberately uses the known CFO for them, so the chain's start would not be the
 * reference's; the caller continues such a window itself).  c_1 comes from frame 0's cfo_hz by the chain rule (:1412-1434).
 * For k = 1 .. 8 (MAX_BURST_BLOCKS, streaming_decoder.hpp:418), in this order: fit (else STOP_WINDOW), gate (else
 * STOP_ENERGY), demodulate with c_k (n_llr == 0: STOP_PROCESS, the block is not counted), chain step, decodeFixedFrame into
 * slot k; a block that decodes no codeword is kept and counted as the reference counts it, and ends the burst
 * (STOP_DECODE, :2112); after block 8 STOP_LIMIT.
 *
 * Scope as ria_gpu_rx_acquire_batch: decodeFrame is decodeFixedFrame only; the control-frame hypotheses (:2866-3000), the
 * burst timeout (:3066-3088), the frame queue and statistics stay with the caller.  A decode work-queue fault in any round
 * fails the whole call with RIA_ERR_HIP; so does a work list that breaks its bound (the call never loops on one).  The call
 * synchronises its stream once per round for one small device-to-host read; rounds <= 9 (acquire) + 9.  No samples, soft
 * bits or payloads go to the host.  Workspaces live on the handle, grow with n_windows (and group_size) and are allocated
 * before anything of the call is in flight. */
#define RIA_BURST_MAX_FRAMES 9            /* 1 + MAX_BURST_BLOCKS; an interleaved group uses group_size <= 8 of them */
#define RIA_BURST_INTERLEAVE   0x800u     /* use_burst_interleave_: a marked window is accumulated as a group */
#define RIA_BURST_NO_CONTINUE  0x1000u    /* unmarked windows: first frame only (= ria_gpu_rx_acquire_batch) */

typedef struct ria_burst_result {         /* 64 bytes, one per window */
    int32_t detected, accepted, sync_start, frame_start;   /* as ria_acq_result; frame_start of frame 0 */
    float   correlation;
    float   cfo_hz;            /* the value the host would hold in last_cfo_ after the window (0 if not accepted) */
    int16_t delta;             /* timing-recovery delta of frame 0 (continuation mode), 0 in group mode */
    uint8_t candidates;        /* as ria_acq_result, frame 0 only (0 in group mode) */
    uint8_t burst_interleaved; /* detector's marker */
    uint8_t mode;              /* 0 not accepted, 1 single frame / continuation, 2 interleaved group */
    uint8_t frames;            /* physical frames demodulated (soft bits produced) */
    uint8_t frames_decoded;    /* logical frames / blocks handed to decodeFixedFrame: slots 0..frames_decoded-1 are valid */
    uint8_t stop;              /* RIA_BURST_STOP_* */
    int32_t reserved[8];
} ria_burst_result;
enum { RIA_BURST_STOP_NONE = 0,        /* group complete / not accepted / RIA_BURST_NO_CONTINUE */
       RIA_BURST_STOP_ENERGY = 1,      /* rms < 0.04 */
       RIA_BURST_STOP_PROCESS = 2,     /* process() false or no soft bits (n_llr == 0) */
       RIA_BURST_STOP_WINDOW = 3,      /* next block does not lie in the window (the reference would wait) */
       RIA_BURST_STOP_DECODE = 4,      /* block decoded nothing (continuation) / frame 0 not a success */
       RIA_BURST_STOP_NOT_DATA = 5,    /* frame 0 is a control / connect frame (frame_v2.hpp:222-228, :348-351) */
       RIA_BURST_STOP_LIMIT = 6,       /* MAX_BURST_BLOCKS reached */
       RIA_BURST_STOP_RECOVERED = 7 }; /* frame 0 came from timing recovery (delta != 0): no continuation */

int ria_gpu_rx_burst_batch(ria_gpu_handle h, const float* samples_dev, int64_t stride, int search_len, int window_len,
                           int n_windows, int group_size /* 2..8 */, const ria_acq_params* params_dev, uint32_t flags,
                           uint8_t* info_out_dev,               /* n_windows * 9 * info_bytes_per_frame */
                           ria_decode_status* decode_status_dev,/* n_windows * 9 */
                           ria_burst_result* burst_dev,         /* n_windows */
                           ria_frame_status* demod_status_dev,  /* nullable, n_windows * 9: physical frame f */
                           float* cfo_used_dev,                 /* nullable, n_windows * 9: CFO handed to process() of frame f */
                           float* rms_dev,                      /* nullable, n_windows * 9: the gate's rms of frame f (slot 0 = 0) */
                           void* stream);

/* ---- acquire + decode: MC-DPSK frames with the disconnected-handshake fallbacks ------------------------
 * ria_gpu_mcdpsk_acquire_batch replaces what gui::StreamingDecoder does with one search window of an MC-DPSK frame
 * (src/gui/modem/streaming_decoder.cpp), in the reference's order:
 *   1. detection on the first search_len samples: MCDPSKWaveform::detectDataSync (ZC, roots DATA | CONTROL, the window's
 *      known CFO, mc_dpsk_waveform.cpp:227-292) or, with RIA_MACQ_SYNC_CHIRP, detectSync (dual chirp, training start =
 *      down_chirp_start + 24000 + 4800, :176-225).  Accepted iff detected, correlation >= min_confidence and the primary
 *      frame [sync_start, sync_start + frame_len) lies in the window (the disconnected chirp path has no confidence test,
 *      :829-834: pass min_confidence 0).
 *   2. the CFO: the detector's; when connected, the known CFO instead if |known| > 0.01 Hz and the measurement differs
 *      from it by more than 1 Hz (:903-917).  Every candidate is demodulated by a fresh demodulator with this CFO and
 *      phase 0 over frame_len samples, frame_len = getMinSamplesForCWCount(frame_cw) of the PRIMARY modulation
 *      (mc_dpsk_waveform.cpp:470-485) = 4608 + frame_cw * ceil(648 / (carriers * bps)) * 512 * spreading.
 *   3. decodeMCDPSKFrame at R1/4 (:2595-2819, raw path): robustDecodeSingleCW of CW0, magic 0x55 0x4C, truncation to
 *      20 bytes, parseHeader (control CRC over 18 bytes / data-header CRC over 15), a CONNECT / CONNECT_ACK /
 *      CONNECT_NAK with total_cw < 3 rejected (:2713-2722); total_cw 1 is a success; fewer soft bits than total_cw
 *      codewords is a partial result (CW0's 20 bytes, codewords_ok 1); else CW1..total_cw-1 robustly decoded and the
 *      frame reassembled (CodewordStatus::reassemble, frame_v2.cpp:1030-1063).  A data header with total_cw 0 (undefined
 *      behaviour in the reference) is treated as an invalid header.
 *   4. connected, RIA_MACQ_NO_RETRY, a success or codewords_ok > 0 (header salvage: header_total_cw tells the caller how
 *      many codewords to wait for): done.
 *   5. RIA_MACQ_DISCONNECTED: the alternate modulation (DBPSK <-> DQPSK) over the same samples, accepted only as a full
 *      success (:1646-1690); then timing recovery at +8, -8, +16, -16, +24, -24, +32, -32, +48, -48, +64, -64 samples,
 *      each with the primary and then the alternate modulation; the first full success wins (:1692-1797).  A candidate
 *      whose samples do not lie in the window (s < 0 or s + frame_len > window_len) is skipped and not counted (the
 *      reference reads older ring-buffer samples there instead).  If nothing succeeds, the primary is reported.
 *
 * Window geometry as ria_gpu_rx_acquire_batch: window b at samples_dev + b*stride, window_len samples, the detector sees
 * the first search_len (search_len <= window_len <= stride).  The handle's code rate must be RIA_RATE_1_4 (MC-DPSK is
 * always R1/4, so decodeMCDPSKFrame's R1/4 fallbacks do not arise); cfg gives the carriers, spreading and the PRIMARY
 * modulation.  frame_cw 1..8; a frame length the MC-DPSK demodulator cannot take is RIA_ERR_UNSUPPORTED.
 *
 * Outputs (every window, accepted or not): acq_dev; frame_out_dev rows of RIA_MACQ_FRAME_BYTES(frame_cw) bytes (a
 * DQPSK alternate over a DBPSK frame length carries up to 2 * frame_cw codewords) holding the DecodeResult's frame_data
 * (frame_bytes of them), zero elsewhere; llr_out_dev (nullable) rows of llr_stride floats with the reported candidate's
 * soft bits (n_llr of them, the rest zero; llr_stride must hold every candidate that can run), e.g. for
 * ria_gpu_chase_combine_batch.  This call leaves out the chase cache (:2729-2731, :2766-2789, :2796-2799, :2808-2811):
 * ria_gpu_mcdpsk_acquire_harq_batch below is the same call with it.  It also leaves out channel interleaving
 * (:2614-2623, :2651-2672, :2741; RIA_MACQ_CHANNEL_INTERLEAVE is RIA_ERR_UNSUPPORTED here and in the HARQ call):
 * ria_gpu_mcdpsk_acquire_ci_batch below is the same call with both.  PING classification and the CW0-peek escalation are
 * ria_gpu_mcdpsk_window_batch's, further below.
 *
 * Work: round r demodulates and decodes the list of windows still searching, each at its own next candidate that fits,
 * with two small device-to-host reads (the round's codeword-row count and the next list's length); no samples, soft bits
 * or payloads go to the host.  The robust decoder has no work queue, so the call has no work-queue fault path.
 * Workspaces live on the handle and grow with n_windows. */
typedef struct ria_mcdpsk_acq_params {   /* one per window, 32 bytes */
    float    known_cfo_hz;               /* connected: detectDataSync's known CFO and the CFO rule's reference */
    float    detect_threshold;           /* ZC 0.2 / chirp 0.15 in the reference's MC-DPSK calls */
    float    min_confidence;             /* accepted iff detected && correlation >= min_confidence && the frame fits */
    uint32_t pending_total_cw;           /* the next three: ria_gpu_mcdpsk_window_batch only, ignored by the other calls */
    uint64_t abs_base;                   /* absolute sample index of window sample 0: reported only (not used) */
    uint32_t first_avail;
    int32_t  last_decoded_sync;
} ria_mcdpsk_acq_params;

typedef struct ria_mcdpsk_acq_result {   /* 64 bytes */
    int32_t detected;
    int32_t accepted;
    int32_t sync_start;                  /* training start (ZC start_sample / down chirp + 28800), -1 if not detected */
    int32_t frame_start;                 /* start of the reported candidate = sync_start + delta, -1 if not accepted */
    float   correlation;                 /* ZC correlation / max(up, down) chirp correlation */
    float   cfo_hz;                      /* CFO every candidate was demodulated with, 0 if not accepted */
    float   fading_index;                /* the reported candidate's demodulator getFadingIndex() */
    int16_t delta;                       /* 0 primary / alternate, else the recovery delta that was accepted */
    uint8_t modulation;                  /* RIA_MOD_DBPSK / RIA_MOD_DQPSK of the reported candidate */
    uint8_t candidates;                  /* candidates demodulated + decoded: 0 (not accepted) .. 26 */
    uint8_t success;                     /* DecodeResult of the reported candidate: success, codewords_ok, codewords_failed, */
    uint8_t codewords_ok;                /* frame_type (0x10 PROBE = DecodeResult's default when no header was parsed) */
    uint8_t codewords_failed;
    uint8_t frame_type;
    int32_t header_total_cw;             /* total_cw of a valid CW0 header, 0 if none */
    int32_t frame_bytes;                 /* frame_data length: reassembled on success, 20 for a partial frame, else 0 */
    int32_t n_llr;                       /* soft bits of the reported candidate */
    int32_t reserved[4];
} ria_mcdpsk_acq_result;

#define RIA_MACQ_SYNC_CHIRP           0x1u   /* dual-chirp detectSync instead of ZC detectDataSync */
#define RIA_MACQ_DISCONNECTED         0x2u   /* handshake fallbacks on, connected CFO rule off (ZC + DISCONNECTED: RIA_ERR_INVALID) */
#define RIA_MACQ_NO_RETRY             0x4u   /* primary candidate only */
#define RIA_MACQ_CHANNEL_INTERLEAVE   0x8u   /* use_mc_dpsk_channel_interleave_: the *_ci_batch calls; RIA_ERR_UNSUPPORTED in the others */
#define RIA_MACQ_FRAME_BYTES(frame_cw) (40 * (frame_cw))

int ria_gpu_mcdpsk_acquire_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                 int search_len, int window_len, int n_windows, int frame_cw,
                                 const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                 uint8_t* frame_out_dev, ria_mcdpsk_acq_result* acq_dev,
                                 float* llr_out_dev /* nullable */, int llr_stride, void* stream);

/* ---- HARQ chase combining: fec::ChaseCache on the device (src/fec/chase_cache.{hpp,cpp}) ----------------------------
 * A pool holds n_caches independent caches, one per link or Monte-Carlo trial, as one StreamingDecoder owns one ChaseCache.
 * A cache holds up to max_entries entries keyed by the header's (seq, src_hash, dst_hash); an entry keeps total_cw,
 * frame_type, last_access and, per codeword (up to the reference's sanity limit of 16), a 648-float sum, combine_count and
 * decoded.  The policy is the reference's statement for statement (ria_amd/csrc/chase_policy.hpp, one host/device header):
 *   store         argument checks in the reference's order (cw_index in [0, total_cw), total_cw in 1..16), then stores++,
 *                 pruneExpired, and for a new key evictIfNeeded and a fresh entry holding this codeword (count 1); for an
 *                 existing entry: last_access = now, then refuse cw_index >= entry.total_cw, a decoded codeword, a count of
 *                 MAX_COMBINES = 4; copy on the codeword's first reception, else one float += per element and combines++.
 *   getCombined   a hit iff the entry exists, the index is in range, the codeword has a sum and is not decoded; else a miss.
 *   markDecoded   acts on an existing entry only: sets decoded, drops the sum, erases the entry when all are decoded.
 *   removeEntry, clear (entries go, counters stay), Stats (seven counters; recoveries is counted by the decode path).
 * Time is the caller's: one now_ms per row or window, used by every cache operation of that row in the call.  An entry is
 * expired iff (int64)(now - last_access) > ttl_ms, so a `now` earlier than last_access does not expire it.
 * Eviction takes the smallest last_access as the reference does.  The reference's clock advances strictly, so it never sees
 * two entries with one last_access; here one now_ms may serve several stores, and entries are ordered by (last_access_ms,
 * the cache's store sequence number at the moment last_access was set): among equal times the one touched first goes.
 * The difference now - last_access is taken modulo 2^64 before it is read as int64, so any uint64 is a valid now_ms: a
 * difference of 2^63 or more counts as negative and expires nothing, and ttl_ms INT64_MAX never expires an entry.
 * An entry keeps the total_cw and frame_type of the store that created it.  A later frame with the same key and another
 * header is stored against those: a codeword index at or above the entry's total_cw is refused, its getCombined misses and
 * its count is 0.  A store that the entry refuses (index, decoded, MAX_COMBINES) has already set last_access (and the
 * order) and so keeps the entry alive; a store that fails the argument checks touches nothing.
 * Sums are raw: store copies and adds the soft bits as they are, with one IEEE float add per element and no flush of
 * denormals.  NaN, infinities, -0.0 and denormals are kept in the pool and returned by ria_gpu_chase_export bit for bit
 * (inf + -inf = NaN, FLT_MAX + FLT_MAX = inf; a NaN's sign and payload are unspecified).  Only the decode of a gathered sum
 * maps its input (NaN -> +1e30, clamp to +-1e30, -0.0 -> +0.0).  A slot whose entry went keeps stale floats; the first
 * store of a codeword into a new entry copies, and the export is zero wherever has_sum is 0.
 * Memory: n_caches * max_entries * 16 * 648 * 4 bytes of sums (41 472 bytes per entry, 663 552 per cache at 16 entries)
 * plus 1 344 bytes of metadata and 4 bytes of owner word per cache, all allocated by ria_gpu_chase_create and owned by the
 * handle (ria_gpu_destroy frees the pools still alive; a pool must not be used after its handle is destroyed). */
#define RIA_CHASE_MAX_CW       16
#define RIA_CHASE_MAX_ENTRIES  16
#define RIA_CHASE_MAX_COMBINES 4
typedef struct ria_chase_config {        /* 32 bytes */
    int32_t n_caches;                    /* >= 1 */
    int32_t max_entries;                 /* 1..16, reference default 16 */
    int64_t ttl_ms;                      /* >= 0, reference default 30000 */
    int32_t reserved[4];
} ria_chase_config;
typedef struct ria_chase_stats {         /* ChaseCache::Stats, 56 bytes */
    uint64_t cache_hits, cache_misses, stores, combines, entries_evicted, entries_expired, recoveries;
} ria_chase_stats;
typedef struct ria_chase_entry {         /* 80 bytes */
    uint64_t last_access_ms;
    uint64_t order;                      /* the cache's store sequence number when last_access was set (eviction tie-break) */
    uint32_t src_hash, dst_hash;
    uint16_t seq;
    uint8_t  used;                       /* always 1 in what ria_gpu_chase_export returns */
    uint8_t  total_cw, frame_type;
    uint8_t  reserved[3];
    uint8_t  combine_count[RIA_CHASE_MAX_CW];
    uint8_t  decoded[RIA_CHASE_MAX_CW];
    uint8_t  has_sum[RIA_CHASE_MAX_CW];  /* cw_soft_bits[i] is not empty */
} ria_chase_entry;
typedef struct ria_chase_pool_s* ria_chase_pool;

void ria_gpu_chase_default_config(ria_chase_config* cfg);   /* 1 cache, 16 entries, 30000 ms */
int  ria_gpu_chase_create(ria_gpu_handle h, const ria_chase_config* cfg, ria_chase_pool* out);
void ria_gpu_chase_destroy(ria_chase_pool pool);
/* ChaseCache::clear (what setMode does at streaming_decoder.cpp:2206) for the n caches listed in cache_ids_dev (device,
 * int32; ids out of range are skipped, an id may repeat) or, with NULL, for every cache of the pool (n ignored).  With a list,
 * n 0 clears nothing and n < 0 is RIA_ERR_INVALID.  Counters stay.  The clear is ordered on `stream` like a decode call. */
int  ria_gpu_chase_clear(ria_chase_pool pool, const int32_t* cache_ids_dev /* nullable = all */, int n, void* stream);
/* getStats of one cache into host memory.  Synchronises the device.  A cache_id outside the pool (here and in the export) and
 * a NULL out_host are RIA_ERR_INVALID. */
int  ria_gpu_chase_stats(ria_chase_pool pool, int cache_id, ria_chase_stats* out_host);
/* The live entries of one cache in slot order: returns their number (size(), >= 0) or a negative ria_status.
 * entries_out_host (nullable) takes max_entries records, sums_out_host (nullable) max_entries * 16 * 648 floats: entry e's
 * codeword c at (e * 16 + c) * 648, zero where has_sum is 0.  Synchronises the device. */
int  ria_gpu_chase_export(ria_chase_pool pool, int cache_id, ria_chase_entry* entries_out_host, float* sums_out_host);

/* ---- RX: decodeMCDPSKFrame on soft bits, with the chase cache (streaming_decoder.cpp:2595-2819) -----------------------
 * ria_gpu_mcdpsk_decode_frame_batch is step 3 of ria_gpu_mcdpsk_acquire_batch on rows of soft bits, taken like
 * ria_gpu_decode_frame_batch: row f is n_llr_dev[f] soft bits (clamped to [0, llr_stride]; NULL: llr_stride each) at
 * llr_dev + f * llr_stride, 648 <= llr_stride <= 16 * 648, frame_row >= 20 * (llr_stride / 648).  The handle's rate must be
 * RIA_RATE_1_4.  With a pool, row f uses cache cache_id_dev[f] of it (-1: chase off for the row, the result is that of
 * the plain decode) at time now_ms_dev[f]; pool NULL turns chase off for the call (cache_id_dev, now_ms_dev unused).
 * Stages, each over a compact ascending list, so that no result depends on scheduling:
 *   1. CW0 robust decode   2. header + CONNECT guard   3. CW1.. robust decode
 *   4. chase store: one wave per row with a cache, i = 1 .. total_cw-1 ascending with both outcomes in hand: a codeword that
 *      decoded -> markDecoded (:2796-2799; a no-op while the key has no entry, which is why "store all failures, then mark
 *      all successes" would be wrong: it would refuse a later store of a codeword that decoded before the entry existed);
 *      a codeword that failed -> store, getCombined, getCombineCount (:2766-2776); count > 1 lists (row, i) for stage 5
 *   5. the listed sums gathered from the pool and robustly decoded
 *   6. chase resolve: ok_chase (:2779) -> markDecoded, recoveries++, the codeword's bytes and flag replaced
 *   7. reassembly (the finish of the acquire call), removeEntry on full success (:2808-2811)
 * A sum decode touches only its own codeword's state, so running 5-6 after all of 4 gives the reference's result.
 * cw_decoded[0] is never set on this path (CW0 is not handed to the cache), so markDecoded's "all decoded -> erase" never
 * fires here; it is implemented all the same.
 * Two rows of one call with the same cache id >= 0 (or an id >= n_caches) are RIA_ERR_INVALID: they would need an order
 * between them.  This is found on the device (an owner word per cache, atomicCAS) and read with the call's first control
 * read, before any cache is touched.  Retransmissions of one link go into successive calls.  A pool created on another
 * handle is RIA_ERR_INVALID too.  Every negative id turns chase off for its row as -1 does, and negative ids may repeat.
 * The call synchronises its stream once for the codeword-row count and, with a pool and at least one such row, once more
 * for the length of the list of sums; stage 5 is skipped when that list is empty.  Every row of every output is written. */
typedef struct ria_mcdpsk_dframe_result {   /* 16 bytes: the DecodeResult */
    uint8_t success, codewords_ok, codewords_failed;
    uint8_t frame_type;                  /* 0x10 when no header was parsed */
    int32_t header_total_cw;             /* total_cw of a valid CW0 header, 0 if none */
    int32_t frame_bytes;                 /* frame_data length in the row of frame_out_dev */
    int32_t reserved;
} ria_mcdpsk_dframe_result;
enum { RIA_HARQ_ENTRY_NONE = 0,          /* the key has no entry after the row */
       RIA_HARQ_ENTRY_KEPT = 1,          /* it has one */
       RIA_HARQ_ENTRY_REMOVED = 2 };     /* it had one and the frame's full success removed it */
typedef struct ria_mcdpsk_harq_result {  /* 32 bytes, one per row / window; all zero unless a valid header met a cache id >= 0 */
    uint16_t seq;                        /* the key (:2730) */
    uint8_t  valid;                      /* 1: the key and cache_id below hold */
    uint8_t  entry;                      /* RIA_HARQ_ENTRY_*; NONE also when no CW1+ was walked (total_cw 1, or too few soft bits) */
    uint32_t src_hash, dst_hash;
    uint16_t stored_mask;                /* bit i: store() of codeword i returned true */
    uint16_t sum_mask;                   /* bit i: the combined sum of codeword i was decoded (count > 1) */
    uint16_t recovered_mask;             /* bit i: that decode recovered it */
    uint8_t  max_combine;                /* largest getCombineCount after the store, over the codewords that failed */
    uint8_t  reserved0;
    int32_t  cache_id;
    int32_t  reserved[2];
} ria_mcdpsk_harq_result;
int ria_gpu_mcdpsk_decode_frame_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, const int32_t* n_llr_dev /* nullable */,
                                      int n_frames, ria_chase_pool pool /* nullable */, const int32_t* cache_id_dev,
                                      const uint64_t* now_ms_dev, uint8_t* frame_out_dev, int frame_row,
                                      ria_mcdpsk_dframe_result* result_dev, ria_mcdpsk_harq_result* harq_dev /* nullable */,
                                      void* stream);
/* ria_gpu_mcdpsk_acquire_batch with decodeMCDPSKFrame's chase statements: window b uses cache cache_id_dev[b] (-1: off) at
 * now_ms_dev[b].  The reference calls decodeMCDPSKFrame for every candidate, so in disconnected mode a candidate that
 * decodes a header but not the frame stores into the cache too and the window's next candidate sees it; rounds run one
 * after the other on one stream, which gives that order.  harq_dev[b] (nullable) describes the window's last candidate in
 * which a valid header met the cache.  pool NULL: every output is that of ria_gpu_mcdpsk_acquire_batch and no extra read
 * is made.  Duplicate ids among the windows are RIA_ERR_INVALID as above, read with the first control read.  With a pool,
 * each round that has codeword rows makes one more small device-to-host read (the length of its list of sums). */
int ria_gpu_mcdpsk_acquire_harq_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                      int search_len, int window_len, int n_windows, int frame_cw,
                                      const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                      uint8_t* frame_out_dev, ria_mcdpsk_acq_result* acq_dev,
                                      float* llr_out_dev /* nullable */, int llr_stride,
                                      ria_chase_pool pool /* nullable */, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                      ria_mcdpsk_harq_result* harq_dev /* nullable */, void* stream);

/* ---- MC-DPSK channel interleaving (use_mc_dpsk_channel_interleave_, negotiated per link) -------------------------------
 * With the mode on, the encoder permutes every codeword of every MC-DPSK frame that is not a 20-byte control frame
 * (streaming_encoder.cpp:778-787) with ChannelInterleaver(B, 648) (ldpc_decoder.cpp:552-650): step = findCoprimeStep(B, 648),
 * bit i of the 648 coded bits (81 bytes, MSB first) goes to bit (i * step) % 648; deinterleave(x)[i] = x[(i * step) % 648].
 * B = interleaver_bits is the width of the receiver's interleaver_, an argument of the call and the same for every
 * candidate of a window: carriers * bits(modulation) after setMCDPSKCarriers / setModulation (and in the encoder),
 * carriers * 2 after setMode whatever the modulation.
 *
 * decodeMCDPSKFrame with the mode on (flags = RIA_MACQ_CHANNEL_INTERLEAVE, interleaver_bits 1..648 or RIA_ERR_INVALID):
 *   - the raw CW0 first; ok with the magic: the frame is handled as without the mode, CW1.. raw (cw0_deinterleaved false)
 *   - else deinterleave(CW0); ok with the magic: its bytes are CW0's, cw0_deinterleaved true; else the default result
 *   - header, CONNECT guard, 1-CW success and the partial result on whichever CW0 won
 *   - CW1.. and the combined sums of the chase cache are de-interleaved iff cw0_deinterleaved; store() receives the raw
 *     soft bits, so a pool's sums are raw sums whatever the frames were (ria_gpu_chase_export returns them raw)
 * The two bits of the reported candidate: ria_mcdpsk_dframe_result.reserved / ria_mcdpsk_acq_result.reserved[0]
 * bit0 = cw0_deinterleaved, bit1 = the de-interleaved CW0 decode ran; both 0 without the flag.
 *
 * ria_gpu_mcdpsk_decode_frame_ci_batch is ria_gpu_mcdpsk_decode_frame_batch plus (flags, interleaver_bits): flags 0 or
 * RIA_MACQ_CHANNEL_INTERLEAVE (anything else RIA_ERR_INVALID); with 0, interleaver_bits is ignored and every output is
 * the old call's.  ria_gpu_mcdpsk_acquire_ci_batch is ria_gpu_mcdpsk_acquire_harq_batch (pool nullable) plus
 * interleaver_bits, and accepts RIA_MACQ_CHANNEL_INTERLEAVE in flags; without it, it is that call.
 * Work with the flag: round A2 after a round's CW0 decode - a compact ascending list of the entries whose raw CW0 is not
 * (ok and magic) and that hold 648 soft bits, their de-interleaved CW0 decoded, merged into what the header stage reads.
 * Each round (the decode-frame call is one round) makes one more small device-to-host read, the length of that list;
 * without the flag there is no additional read or launch.  A list longer than the round's is RIA_ERR_HIP.
 *
 * ria_gpu_mcdpsk_interleave_batch is ChannelInterleaver::interleave(Bytes) over n_cw rows of 81 coded bytes (coded_dev ->
 * out_dev, not in place), e.g. ria_gpu_ldpc_encode_host output before ria_gpu_mcdpsk_modulate_batch. */
int ria_gpu_mcdpsk_decode_frame_ci_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, const int32_t* n_llr_dev /* nullable */,
                                         int n_frames, ria_chase_pool pool /* nullable */, const int32_t* cache_id_dev,
                                         const uint64_t* now_ms_dev, uint8_t* frame_out_dev, int frame_row,
                                         ria_mcdpsk_dframe_result* result_dev, ria_mcdpsk_harq_result* harq_dev /* nullable */,
                                         uint32_t flags, int interleaver_bits, void* stream);
int ria_gpu_mcdpsk_acquire_ci_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                    int search_len, int window_len, int n_windows, int frame_cw,
                                    const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                    uint8_t* frame_out_dev, ria_mcdpsk_acq_result* acq_dev,
                                    float* llr_out_dev /* nullable */, int llr_stride,
                                    ria_chase_pool pool /* nullable */, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                    ria_mcdpsk_harq_result* harq_dev /* nullable */, int interleaver_bits, void* stream);
int ria_gpu_mcdpsk_interleave_batch(ria_gpu_handle h, int interleaver_bits, const uint8_t* coded_dev, int n_cw, uint8_t* out_dev,
                                    void* stream);

/* ---- one MC-DPSK window: anti-replay, PING energy test, CW0 peek, escalation, decode, handshake fallbacks ---------------------
 * ria_gpu_mcdpsk_window_batch is StreamingDecoder::decodeCurrentFrame() for the MC-DPSK mode (src/gui/modem/
 * streaming_decoder.cpp:1060-1266, :1346-1376, :1436-1503, :1599-1797, :1967-2013) for a batch of windows, statement for
 * statement.  h is created at R1/4; cfg, the window geometry and the flags are ria_gpu_mcdpsk_acquire_ci_batch's
 * (RIA_MACQ_SYNC_CHIRP, RIA_MACQ_DISCONNECTED, RIA_MACQ_NO_RETRY, RIA_MACQ_CHANNEL_INTERLEAVE).  There is no frame_cw: the call
 * finds the codeword count.  Per-window inputs in ria_mcdpsk_acq_params, read by this call only:
 *   pending_total_cw   0 for a fresh sync; n > 0 (<= 255, else RIA_ERR_INVALID) is the re-entry of a window that answered
 *                      RIA_MWIN_NEED_SAMPLES: the peek is skipped, as the reference skips it when pending_total_cw_ != 0.
 *   first_avail        the samples behind the sync that were there when the first pass ran (checkIfReadyToDecode's early
 *                      half-window, :1005-1011; frame_len = min(1-CW length, available), :1110).  0: a whole 1-codeword span.
 *                      Otherwise >= 9608, else RIA_ERR_INVALID; so is a value below the 1-codeword span without
 *                      RIA_MACQ_DISCONNECTED (a connected decoder waits for the whole span, :1007).
 *   last_decoded_sync  window-relative position of the last decoded frame for the anti-replay rule (:876-889); INT32_MIN: off.
 * Per window, in the reference's order:
 *   1. Detection, acceptance and CFO: steps 1-2 of ria_gpu_mcdpsk_acquire_batch; the fit rule uses the pass-0 span,
 *      min(getMinSamplesForCWCount(1), first_avail), or getMinSamplesForCWCount(pending) on re-entry.  Else RIA_MWIN_NOT_ACCEPTED.
 *   2. Anti-replay: |sync_start - last_decoded_sync| < 200 is RIA_MWIN_REPLAY, next_pos = sync_start + 9600 + 4800; nothing else runs.
 *   3. The PING energy test, under RIA_MACQ_DISCONNECTED only (allow_ping_detection = !connected_): training_rms over samples
 *      [0, min(4608, len)) of the span, rms over the next min(len - 4608, 5000); each a float32 sum of squares in ascending
 *      order divided by the count, then sqrtf; ratio = training_rms > 0.001f ? rms / training_rms : 0; a PING iff ratio < 0.6f:
 *      RIA_MWIN_PING, success 1, frame type 0x01, no bytes, next_pos = sync_start + getMinSamplesForCWCount(1), last_decoded_sync
 *      = sync_start.  Both values are reported on every accepted window that is no replay.  Every later pass of the reference
 *      repeats the test on a span that starts with the same >= 9608 samples (carriers 1..20 and two modulations make the
 *      shortest 1-codeword span 4608 + 17 * 512 = 13 312 samples), so it is computed once.  The CSS branch is out of scope.
 *   4. Pass 0 and the CW0 peek: process() on the pass-0 span at the window's CFO.  With >= 648 soft bits and pending 0:
 *      robustDecodeSingleCW of CW0 at R1/4; without the magic and under RIA_MACQ_CHANNEL_INTERLEAVE the de-interleaved CW0
 *      (:1456-1467); parseHeader on the whole decoded vector - it reads bytes 0..19 only (frame_v2.cpp:1195-1252), so
 *      decodeMCDPSKFrame's truncation to 20 bytes cannot differ; the peek's CONNECT guard FORCES a CONNECT / CONNECT_ACK /
 *      CONNECT_NAK with total_cw < 3 up to 3 when disconnected (:1473-1480; decodeMCDPSKFrame's guard rejects);
 *      needed_cw > 1 && avail_cw < needed_cw: pending = needed_cw; otherwise, disconnected, pending = 3 while avail_cw < 3
 *      (:1496-1502).  With < 648 soft bits, disconnected and pending 0: pending = 1 (:1600-1609).  Disconnected with avail_cw < 3
 *      and pending < 3: pending = 3 (:1611-1624) - the rule a re-entry with pending 1 or 2, or an early window, hits.  A data
 *      header with total_cw 0 is valid for the peek (needed_cw 0: no escalation) and invalid for the decode, as in the older calls.
 *      A span of >= 9608 samples holds >= 2 data symbols at any spreading, so process() cannot fail and the soft bits are never
 *      empty: RIA_MWIN_PROCESS_FAILED (:1352-1372) is defined and never produced.  An early window gives fewer than 648 soft
 *      bits whatever the samples are, so it is not demodulated.
 *   5. Escalation, pending n > 0: frame_len = getMinSamplesForCWCount(n); sync_start + frame_len > window_len is
 *      RIA_MWIN_NEED_SAMPLES (the reference's SYNC_FOUND wait; need_samples = frame_len and pending_total_cw = n to come back
 *      with); else n > 8, or a span the MC-DPSK demodulator's workgroup cannot hold, is RIA_MWIN_TOO_LONG (pending_total_cw = the
 *      header's count); else process() on the longer span, without another peek.
 *   6. decodeFrame -> decodeMCDPSKFrame on the last pass's soft bits: ria_gpu_mcdpsk_acquire_ci_batch's rounds at frame_cw = n
 *      (chase store / combine / resolve with a pool, channel-interleave rounds with the flag).
 *   7. Header salvage (:1631-1644): !success, pending 0, codewords_ok > 0 and a valid header with total_cw > avail_cw: pending =
 *      total_cw, back to 5.  The peek of the same pass has parsed the same CW0 decode and has escalated every such header
 *      already (the only headers it treats differently are the CONNECT ones, which decodeMCDPSKFrame rejects with codewords_ok
 *      0), so no input reaches this at R1/4; it is implemented all the same (RIA_MPEEK_SALVAGE).
 *   8. Handshake fallbacks under RIA_MACQ_DISCONNECTED without RIA_MACQ_NO_RETRY, if !success && codewords_ok == 0: steps 4-5
 *      of ria_gpu_mcdpsk_acquire_batch at frame_cw = pending, its fit rule, first full success wins; a recovered candidate
 *      moves sync_position_, so next_pos follows it.
 *   9. Consumed: next_pos = frame_start + frame_len (MC-DPSK never takes the exact-size shortcut of :2001).
 *  10. deliver = success || codewords_ok > 0 (:1977); last_decoded_sync = frame_start (:2121).  RIA_MWIN_DECODED.
 * Out of scope: the ZC-miss -> chirp fallback of connected search (:790-828; call again with RIA_MACQ_SYNC_CHIRP),
 * estimateSNRFromChirp (the correlation is reported), the frame timeout, CSS, ring-buffer wrap, MFSK.
 *
 * Outputs, every row written, zero where nothing applies: result_dev; acq_dev (the reported candidate's DecodeResult, as in the
 * acquire call; candidates counts the last pass's); frame_out_dev rows of frame_row >= RIA_MACQ_FRAME_BYTES(8) bytes; llr_out_dev
 * (nullable) rows of llr_stride floats, llr_stride >= the soft bits of the longest pass the window length allows (either
 * modulation when the fallbacks can run); harq_dev (nullable).  pool NULL: no chase.  Duplicate cache ids are RIA_ERR_INVALID,
 * read with the first control read, as are the per-window input errors above.  n_windows == 0 is RIA_OK.
 * Work: one wavefront per window for the energy test (the serial float32 chain runs on one lane out of LDS); the peek pass is
 * one demodulator launch, round A (and A2) of the acquire rounds and one wave per window for the rules; then, for each
 * codeword count 1..8 in ascending order - escalation only ever raises a window's count - the open windows of that count as
 * one ascending list through the acquire call's rounds, on one stream, one after the other: no result depends on scheduling
 * or on which batch a window is in, and chase rounds keep ria_gpu_mcdpsk_acquire_harq_batch's order.  A window that falls
 * through the peek is demodulated again at count 1 (the reference decodes its CW0 twice as well).
 * Small device-to-host reads, worst case: 2 (the per-window input check, the peek list with the duplicate-id flag) + 1 (the
 * peek's A2 list) + 8 counts x (26 rounds x 4 + 1) = 843; a connected call without pool or interleaving makes at most
 * 2 + 8 x 3 = 26, one per count that no window is at.  No samples, soft bits or payloads go to the host.  Workspaces live on the handle, are carved once
 * per size and reserved before anything of the call is in flight. */
enum { RIA_MWIN_NOT_ACCEPTED = 0, RIA_MWIN_REPLAY = 1, RIA_MWIN_PING = 2, RIA_MWIN_PROCESS_FAILED = 3, RIA_MWIN_DECODED = 4,
       RIA_MWIN_NEED_SAMPLES = 5, RIA_MWIN_TOO_LONG = 6 };
/* ria_mcdpsk_window_result.peek: what CW0 said in the low four bits, then the statements that set pending_total_cw_ */
enum { RIA_MPEEK_NONE = 0,                   /* the peek did not run (pending on input, early window, fewer than 648 soft bits) */
       RIA_MPEEK_NO_HEADER = 1,              /* no CW0 with the magic and a valid header */
       RIA_MPEEK_HEADER_SINGLE = 2,          /* a valid header that asks for no more than the span holds */
       RIA_MPEEK_HEADER_MULTI = 3,           /* needed_cw > 1 && avail_cw < needed_cw (:1482-1489) */
       RIA_MPEEK_CONNECT_FORCED = 4,         /* the same after the CONNECT guard forced total_cw up to 3 (:1475-1480) */
       RIA_MPEEK_WHAT_MASK = 0x0F,
       RIA_MPEEK_HANDSHAKE_FALLBACK = 0x10,  /* :1496-1502 */
       RIA_MPEEK_EARLY_WINDOW = 0x20,        /* :1600-1609 */
       RIA_MPEEK_HANDSHAKE_WINDOW = 0x40,    /* :1611-1624 */
       RIA_MPEEK_DEINTERLEAVED = 0x80,       /* the de-interleaved CW0 was the one that spoke */
       RIA_MPEEK_SALVAGE = 0x100 };          /* :1631-1644 (unreached at R1/4, see above) */
typedef struct ria_mcdpsk_window_result {    /* 64 bytes, one per window */
    int32_t outcome;                     /* RIA_MWIN_* */
    int32_t peek;                        /* RIA_MPEEK_* */
    int32_t next_pos;                    /* position behind the consumed samples within the window, -1 where nothing was consumed */
    int32_t need_samples;                /* RIA_MWIN_NEED_SAMPLES: the samples from sync_start the next pass waits for, else 0 */
    int32_t pending_total_cw;            /* pending_total_cw_ as the window leaves it (0: pass 0's own soft bits were decoded) */
    int32_t frame_len;                   /* RIA_MWIN_DECODED: the decoded pass's span in samples, else 0 */
    int32_t passes;                      /* passes of decodeCurrentFrame up to the outcome (every one runs the energy test and process()) */
    int32_t peek_total_cw;               /* total_cw of the header the peek parsed, before the guard; 0 if none */
    float   training_rms;
    float   rms;
    int32_t last_decoded_sync;           /* last_decoded_sync_pos_ as the window leaves it (the input where it does not move) */
    uint8_t deliver;                     /* the host queues the DecodeResult: success || codewords_ok > 0, or a PING */
    uint8_t is_ping;
    uint8_t peek_tries;                  /* decodes of the robust decoder in the peek: raw CW0 plus the de-interleaved one */
    uint8_t reserved0;
    int32_t reserved[4];
} ria_mcdpsk_window_result;
int ria_gpu_mcdpsk_window_batch(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride,
                                int search_len, int window_len, int n_windows,
                                const ria_mcdpsk_acq_params* params_dev, uint32_t flags,
                                uint8_t* frame_out_dev, int frame_row, ria_mcdpsk_window_result* result_dev,
                                ria_mcdpsk_acq_result* acq_dev, float* llr_out_dev /* nullable */, int llr_stride,
                                ria_chase_pool pool /* nullable */, const int32_t* cache_id_dev, const uint64_t* now_ms_dev,
                                ria_mcdpsk_harq_result* harq_dev /* nullable */, int interleaver_bits, void* stream);
/* One window from host memory, without a chase pool (the single-window adaptor path, ria_host::mcdpskWindow): staged through
 * the handle's pinned block on the handle's own stream; synchronises that stream.  frame_out_host takes
 * RIA_MACQ_FRAME_BYTES(8) bytes (max_bytes below that is RIA_ERR_INVALID). */
int ria_gpu_mcdpsk_window_host(ria_gpu_handle h, const ria_mcdpsk_config* cfg, const float* samples_host, int search_len, int window_len,
                               const ria_mcdpsk_acq_params* params_host, uint32_t flags, uint8_t* frame_out_host, int max_bytes,
                               ria_mcdpsk_window_result* result_out, ria_mcdpsk_acq_result* acq_out, int interleaver_bits);

/* ---- RX: decodeFrame, OFDM branch (StreamingDecoder::decodeFrame, src/gui/modem/streaming_decoder.cpp:2821-3059) ----
 * The "try both" strategy every OFDM frame's soft bits go through, statement for statement, over a batch of rows.  Row f is
 * n_llr_dev[f] soft bits (clamped to [0, llr_stride]; NULL: llr_stride each) at llr_dev + f*llr_stride.  `rate` is the
 * handle's code rate (connected_ ? code_rate_ : R1_4: a disconnected receiver is a handle created at RIA_RATE_1_4), bps its
 * bits_per_symbol, apply_channel_deinterleave is true unless RIA_DECODE_NO_CHANNEL_DEINTERLEAVE is set.  A "plain decode"
 * is codec_->decode: LDPCDecoder::decodeSoft at getRecommendedIterations(rate of that decode), min-sum factor 0.75
 * (ldpc_decoder.cpp:44, ldpc_codec.cpp:65-77); it returns ceil(ldpc_k/8) bytes and the frame layer truncates them to that
 * rate's bytes per codeword (the R1/3 peculiarity of ria_gpu_geometry.ldpc_k applies unchanged).
 *   0. n_llr < 648: the default DecodeResult (success 0, counts 0, frame_type 0x10, no bytes).              RIA_DFRAME_NONE
 *   1. R1/4 fast path (:2867-2890), only if rate != R1_4: plain decode of [0, 648) at R1/4; ok, magic 55 4C and a valid
 *      header (parseHeader, frame_v2.cpp:1195-1253) with total_cw 1: success, 1 codeword, those 20 bytes. RIA_DFRAME_CONTROL_R14
 *   2. raw CW0 probe (:2892-2930): plain decode of [0, 648) at `rate`, no channel de-interleave.  ok with magic: truncate,
 *      parse; a valid header sets frame_type; total_cw 1 is a success with the truncated CW0 (RIA_DFRAME_CONTROL_CW0);
 *      total_cw 4 sets try_frame_interleave; any other count goes to the legacy path.  Magic with an invalid header: neither
 *      (the row ends in step 4).  Not ok or no magic: try_frame_interleave.
 *   3. fixed frame (:2932-3010), if try_frame_interleave and n_llr >= 2592: decodeFixedFrame of the first 2592 soft bits with
 *      the call's RIA_DECODE_* bits (RIA_DECODE_FULL is the reference); codewords_ok / codewords_failed from its four flags.
 *      All four ok: RIA_DFRAME_FIXED; success = ria_decode_status.frame_valid; frame_data = the reassembled frame
 *      (CodewordStatus::reassemble: 17 + payload_len + 2 bytes, or 20), frame_type = its byte 2; with success 0 the result
 *      keeps 4 / 0 and no bytes (under RIA_DECODE_FULL a frame that does not verify comes back with all four flags cleared,
 *      so success 0 arises only without RIA_DECODE_CRC_RECOVER).  Not all ok: robustDecodeSingleCW (:1028-1058) of [0, 648)
 *      at R1/4 and then, if rate != R1_4, at `rate`; the first with ok, magic and a valid header with total_cw 1 gives
 *      success, 1 / 0 and the bytes truncated to that rate's codeword (RIA_DFRAME_SALVAGE_R14 / _RATE).  Neither: step 4
 *      with the fixed attempt's counts.
 *   4. legacy (:3012-3058), only if the step-2 probe was ok with magic: codewords_ok = 1 while codewords_failed is NOT
 *      reset (a count left by step 3 stays and is added to, as in the reference).  Invalid header: return
 *      (RIA_DFRAME_BAD_HEADER).  avail_cw = n_llr / 648 < total_cw: frame_data = CW0's bytes (RIA_DFRAME_PARTIAL).  Else CW
 *      i = 1 .. total_cw-1: soft bits [648 i, 648 (i+1)) through ChannelInterleaver(bps, 648)::deinterleave when
 *      apply_channel_deinterleave, plain decode at `rate`; all ok: success, frame_data = reassemble() (RIA_DFRAME_LEGACY;
 *      success 0 when a codeword failed).  A data header with total_cw 0 is undefined behaviour in the reference
 *      (decoded[0] of an empty vector); it is treated as an invalid header, as ria_gpu_mcdpsk_acquire_batch does.
 *   5. anything else: the result as it stands: RIA_DFRAME_FIXED_FAILED when the fixed attempt ran, else RIA_DFRAME_NONE.
 *
 * Arguments: 648 <= llr_stride <= 32 * 648 and frame_row >= max(4, llr_stride / 648) * bytes_per_codeword, else
 * RIA_ERR_INVALID.  The cap of 32 codewords per row is this library's: a legacy frame that does not fit the row is
 * RIA_DFRAME_PARTIAL by the reference's own rule.  flags: the RIA_DECODE_* bits and RIA_DECODE_NO_CHANNEL_DEINTERLEAVE,
 * anything else is RIA_ERR_INVALID.
 * Outputs: every row of every output is written, zero where nothing applies: result_dev; frame_out_dev rows of frame_row
 * bytes (frame_bytes of frame_data, then zeros); decode_status_dev (nullable) and info_out_dev (nullable, 4 *
 * bytes_per_codeword per row): the fixed attempt's status and codeword bytes, zero where it did not run.  header_total_cw
 * is the total_cw of the valid header behind the path: 1 for the control and salvage paths, the CW0 probe's count for
 * LEGACY / PARTIAL, 4 or 0 (CW0 probe failed) for FIXED / FIXED_FAILED, 0 otherwise.
 * Work: each stage runs on a compact, ascending list of the rows the stages before left open (stages, iters_* and tries_*
 * show which ran for a row), so results do not depend on scheduling.  The call synchronises its stream exactly twice for
 * one 32-byte device-to-host read each (the length of the fixed batch; the number of legacy codeword rows); no soft bits
 * or payloads go to the host.  A decode work-queue fault in the fixed stage fails the whole call with RIA_ERR_HIP.  A handle
 * whose rate is not R1/4 builds its R1/4 code at the first call; all workspace lives on the handle, is grown on demand
 * (about 11 KB per row plus the size of the soft-bit rows behind the first codeword) and is allocated before anything of
 * the call is in flight.  Not covered: see ria_gpu_rx_acquire_batch; the control hypothesis on SAMPLES (a span demodulated
 * with the DQPSK R1/4 profile, :1268-1344) is ria_gpu_rx_control_batch's, the escalation (:1505-1597) and the small-frame
 * recovery (:1806-1853) are ria_gpu_rx_window_batch's. */
typedef struct ria_dframe_result {      /* 32 bytes, one per row */
    uint8_t  success;          /* DecodeResult: success, codewords_ok, codewords_failed, frame_type */
    uint8_t  codewords_ok;
    uint8_t  codewords_failed;
    uint8_t  frame_type;       /* 0x10 (DecodeResult's default) when no header was parsed */
    uint8_t  path;             /* RIA_DFRAME_*: which statement produced the result */
    uint8_t  header_total_cw;  /* total_cw of the valid header that decided the path, 0 if none */
    uint8_t  stages;           /* bit0 R1/4 probe ran, bit1 rate probe, bit2 decodeFixedFrame, bit3 salvage R1/4, bit4 salvage rate, bit5 legacy CW1+ */
    uint8_t  reserved0;
    int32_t  frame_bytes;      /* length of frame_data in the row of frame_out_dev */
    uint16_t iters_r14;        /* lastIterations() of the two plain probes (0 if the stage did not run) */
    uint16_t iters_cw0;
    uint8_t  tries_r14;        /* decodes made by the two salvage decoders, 0..5 */
    uint8_t  tries_rate;
    uint8_t  reserved1[2];
    int32_t  reserved[3];
} ria_dframe_result;
enum { RIA_DFRAME_NONE = 0, RIA_DFRAME_CONTROL_R14 = 1, RIA_DFRAME_CONTROL_CW0 = 2, RIA_DFRAME_FIXED = 3,
       RIA_DFRAME_SALVAGE_R14 = 4, RIA_DFRAME_SALVAGE_RATE = 5, RIA_DFRAME_FIXED_FAILED = 6,
       RIA_DFRAME_LEGACY = 7, RIA_DFRAME_PARTIAL = 8, RIA_DFRAME_BAD_HEADER = 9 };

int ria_gpu_decode_frame_batch(ria_gpu_handle h, const float* llr_dev, int llr_stride, const int32_t* n_llr_dev /* nullable: llr_stride each */,
                               int n_frames, uint32_t flags, uint8_t* frame_out_dev, int frame_row,
                               ria_dframe_result* result_dev,
                               ria_decode_status* decode_status_dev /* nullable: the fixed attempt's, zero where it did not run */,
                               uint8_t* info_out_dev /* nullable: the fixed attempt's 4 * bytes_per_codeword, zero where it did not run */,
                               void* stream);
/* One row from host memory, staged through the handle's pinned block and stream like ria_gpu_decode_frames_host.  Soft bits
 * beyond 32 * 648 are ignored; max_bytes must be >= max(4, min(n_llr, 32 * 648) / 648) * bytes_per_codeword, of which
 * result_out->frame_bytes hold frame_data and the rest is zeroed. */
int ria_gpu_decode_frame_host(ria_gpu_handle h, const float* llr_host, int n_llr, uint32_t flags, uint8_t* frame_out_host, int max_bytes,
                              ria_dframe_result* result_out, ria_decode_status* decode_status_out /* nullable */);

/* ---- frames of any length: 1..324 coded bytes on the air, spans of 3 symbols up to a frame at the receiver ------------
 * A connected-mode link carries, beside the fixed 4-codeword data frames, control frames of ONE codeword (81 coded bytes:
 * 2 training + ceil(648 / bits_per_symbol) data symbols; 9 symbols = 10 368 samples with the DQPSK R1/4 control profile,
 * streaming_encoder.cpp:216-245), and the receiver runs process() on spans shorter than a frame (streaming_decoder.cpp:1284).
 *
 * ria_gpu_var_frame_samples: getMinSamplesForCWCount's formula for any byte count (ofdm_chirp_waveform.cpp:616-648):
 * (2 + ceil(8 * coded_bytes / bits_per_symbol)) * 1152, the samples ria_gpu_tx_coded_var_batch writes per frame; a negative
 * ria_status for coded_bytes outside 1..324.
 * ria_gpu_control_frame_samples: getOFDMControlFrameSamples (streaming_decoder.cpp:42-69) for a data handle and its control
 * handle (RIA_MOD_DQPSK / RIA_RATE_1_4): the data handle's own 1-codeword size when it is DQPSK R1/4 itself, else the larger
 * of that size and (2 + ceil(648 / (2 * (carriers - ceil(carriers / 10))))) * 1152.  Negative ria_status on a bad handle. */
int ria_gpu_var_frame_samples(ria_gpu_handle h, int coded_bytes);
int ria_gpu_control_frame_samples(ria_gpu_handle control_h, ria_gpu_handle data_h);

/* generateDataPreamble() ++ modulate(coded) (modulator.cpp:534-583, :348-477) for coded_bytes bytes per frame, 1..324, at the
 * handle's modulation: coded_dev holds n_frames rows of coded_bytes bytes, read MSB first; a carrier whose bits run out is
 * filled with zero bits, the carriers behind the last bit are silent, differential references carry on per carrier; frame f
 * is ria_gpu_var_frame_samples(h, coded_bytes) samples at samples_out_dev + f * out_stride (out_stride at least that; the
 * floats between two frames are not written).  peak_normalize: ria_gpu_tx_batch's rule.  At coded_bytes 324 the samples are
 * ria_gpu_tx_coded_batch's bit for bit. */
int ria_gpu_tx_coded_var_batch(ria_gpu_handle h, const uint8_t* coded_dev, int coded_bytes, int n_frames, float peak_normalize,
                               float* samples_out_dev, int64_t out_stride, void* stream);

/* process() + getSoftBits() on spans of n_samples samples (one value per call), 3 * 1152 <= n_samples <= frame_samples, else
 * RIA_ERR_INVALID (below two whole symbols the reference reads past its buffer).  Frame f starts at samples_dev +
 * (frame_offsets_dev ? frame_offsets_dev[f] : f * n_samples); meta_dev as ria_gpu_demod_batch (NULL: CFO 0 and correction phase
 * +0.0; a meta of zeros gives the reference's own product, -0.0).  The demodulator works on whole
 * symbols (demodulator.cpp:1362): data symbols = n_samples / 1152 - 2, the samples behind the last whole symbol are not
 * read.  Row f of llr_out_dev (llr_stride floats apart, llr_stride >= data symbols * bits_per_symbol) takes the soft bits in
 * order; the rest of the row is not written.  Every status word is the reference's after the last symbol present:
 * corr_phase is freq_correction_phase after the last sample of the last whole symbol, where the phase walk ends; n_llr is
 * the count produced if that is at least 648, else 0 (process() returns false, demodulator.cpp:1413) - the row holds what
 * was produced all the same.  At n_samples == frame_samples soft bits and status are ria_gpu_demod_batch's bit for bit.
 * Every modulation of the demodulator.  Under RIA_DEMOD_FUSED=1 (the one-wave-per-frame A/B kernel, whose symbol count is a
 * constant of the handle) the call returns RIA_ERR_UNSUPPORTED. */
int ria_gpu_demod_var_batch(ria_gpu_handle h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                            const ria_frame_meta* meta_dev, int n_frames, int n_samples,
                            float* llr_out_dev, int llr_stride, ria_frame_status* status_dev, void* stream);
/* One span from host memory, staged like ria_gpu_rx_frames_host: llr_out_host takes up to max_llr soft bits (the count
 * produced is (n_samples / 1152 - 2) * bits_per_symbol; status_out->n_llr follows the rule above).  meta_host and status_out
 * may be NULL. */
int ria_gpu_demod_var_host(ria_gpu_handle h, const float* samples_host, int n_samples, const ria_frame_meta* meta_host,
                           float* llr_out_host, int max_llr, ria_frame_status* status_out);

/* ---- the control hypothesis: a connected-mode window tried as a DQPSK R1/4 control frame first --------------------------
 * (src/gui/modem/streaming_decoder.cpp:1268-1344).  control_h is an ordinary handle created at RIA_MOD_DQPSK / RIA_RATE_1_4
 * with the data handle's carrier configuration; any other handle is RIA_ERR_INVALID.  configure() keeps the waveform's
 * position, CFO and one-shot marker and only rebuilds the demodulator (ofdm_chirp_waveform.cpp:81-107, :421-440), so a span
 * demodulated on the control handle with the window's meta is what the reconfigured waveform computes.
 *
 * ria_gpu_rx_control_batch runs :1284-1338 on pre-synced spans (arguments as ria_gpu_demod_var_batch), in this order:
 * process() on the span; with at least 648 soft bits, robustDecodeSingleCW of the first 648 at R1/4; then ok, at least 4
 * bytes, magic 55 4C, truncation to 20 bytes, parseHeader valid, total_cw == 1, isControlFrame(type).  frame_out_dev takes
 * 20 bytes per row: the frame on success, zeros otherwise.  Every row of every output is written, zero where nothing
 * applies; no soft bits or payloads go to the host; the call makes no synchronisation.  Escalation (pending_total_cw_,
 * :1505-1597) and the short-span data-profile CFO feedback (:1346-1434) are ria_gpu_rx_window_batch's. */
typedef struct ria_control_result {      /* 32 bytes, one per row / window */
    uint8_t  process_ok;       /* process() returned true: the span gave at least 648 soft bits */
    uint8_t  cw_ok;            /* robustDecodeSingleCW converged */
    uint8_t  magic;            /* cw_ok, at least 4 bytes, 55 4C */
    uint8_t  header_valid;     /* parseHeader(...).valid on the 20 bytes */
    uint8_t  total_cw;         /* of a valid header (1 for a control type, byte 12 for a data type), else 0 */
    uint8_t  frame_type;       /* byte 2 where magic holds, else 0 */
    uint8_t  success;          /* header_valid && total_cw == 1 && isControlFrame(frame_type) */
    uint8_t  tries;            /* decodes the robust decoder made, 1..5; 0 where it did not run */
    uint16_t seq;              /* of a valid header, else 0 */
    uint16_t iterations;       /* lastIterations() of the last decode */
    int32_t  n_llr;            /* ria_frame_status.n_llr of the span */
    uint8_t  tried;            /* 1: the hypothesis ran for this row (always in ria_gpu_rx_control_batch) */
    uint8_t  reserved0[3];
    int32_t  reserved[3];
} ria_control_result;
int ria_gpu_rx_control_batch(ria_gpu_handle control_h, const float* samples_dev, const uint64_t* frame_offsets_dev,
                             const ria_frame_meta* meta_dev, int n_frames, int n_samples,
                             uint8_t* frame_out_dev /* n_frames * 20 */, ria_control_result* result_dev,
                             ria_frame_status* demod_status_dev /* nullable */, void* stream);

/* ria_gpu_rx_acquire_batch's window geometry, ria_acq_params, LTS detection and acceptance rule, then the control
 * hypothesis on the span of n_samples samples at sync_start (n_samples: ria_gpu_control_frame_samples of the link), with
 * abs_position = abs_base + sync_start, the known CFO and the detector's marker in meta.flags bit 0.  There is no timing
 * recovery: the reference has none on this path.  Not tried (tried 0, every other field of the row zero): a window that is
 * not accepted - not detected, below min_confidence, or sync_start + n_samples > window_len, where the reference would wait
 * for samples - and, under the flag RIA_BURST_INTERLEAVE (the only flag; anything else RIA_ERR_INVALID), an accepted window
 * whose detector reports the marker (:1087-1092: such a window is accumulated as a burst group, full buffer, no peek).
 * acq_dev is a ria_acq_result with delta 0, candidates = tried, frame_start = sync_start where accepted and cfo_hz = the
 * span's ria_frame_status.cfo_hz where tried.  The call synchronises its stream once, for the length of the list of windows
 * to try.  Workspaces live on the handle, are carved once per size and reserved before anything of the call is in flight. */
int ria_gpu_control_acquire_batch(ria_gpu_handle control_h, const float* samples_dev, int64_t stride, int search_len,
                                  int window_len, int n_windows, int n_samples, const ria_acq_params* params_dev, uint32_t flags,
                                  uint8_t* frame_out_dev /* n_windows * 20 */, ria_control_result* result_dev,
                                  ria_acq_result* acq_dev, ria_frame_status* demod_status_dev /* nullable */, void* stream);

/* ---- one connected-mode OFDM-CHIRP window: peek, escalation, small-frame recovery, timing recovery ---------------------------
 * ria_gpu_rx_window_batch joins the calls above into what gui::StreamingDecoder does with one window of a connected link
 * (src/gui/modem/streaming_decoder.cpp), statement by statement per window, and leaves the DecodeResult and the receiver state
 * (sync_cfo_ / last_cfo_, last_fading_index_, frame_len, the position behind the consumed samples).  control_h: the DQPSK R1/4
 * handle with data_h's carrier configuration, on its device (else RIA_ERR_INVALID).  Window geometry and ria_acq_params are
 * ria_gpu_rx_acquire_batch's.  "The rate" is data_h's code rate.
 *   1. Detection and acceptance, then the control hypothesis (:1268-1344): exactly ria_gpu_control_acquire_batch on control_h
 *      with n_ctl = ria_gpu_control_frame_samples(control_h, data_h): a window is accepted iff detected, correlation >=
 *      min_confidence and sync_start + n_ctl <= window_len (RIA_WIN_NOT_ACCEPTED otherwise); under RIA_BURST_INTERLEAVE an
 *      accepted window with the detector's marker is left to ria_gpu_rx_burst_batch (RIA_WIN_BURST, :1087-1092); a control frame
 *      ends the window (RIA_WIN_CONTROL_PROFILE: frame = its 20 bytes, success 1, codewords 1 / 0, frame_len = n_ctl, next_pos =
 *      sync_start + n_ctl (:1328), fading_index = the control span's, sync_cfo_hz = known_cfo_hz: no feedback on this path).
 *   2. Pass 1, the peek (:1346-1434): process() with the data profile on the same n_ctl samples, known CFO, abs_position =
 *      abs_base + sync_start, marker OFF - the control hypothesis's process() has consumed the one-shot
 *      (ofdm_chirp_waveform.cpp:421-440) - in this and every later pass.  Kept object: when data_h is DQPSK R1/4 itself the
 *      reference runs process() twice on one demodulator without reset(); processPresynced() (demodulator.cpp:1264-1309) clears
 *      every per-frame member and process() sets CFO and phase anew, so nothing carries over and the second pass equals a pass
 *      on a fresh object; the same holds for every later process() of the ladder.  Fewer than 648 soft bits: the window ends
 *      (RIA_WIN_DECODED with an all-zero frame, :1352-1360).  Then last_fading_index_, and the CFO feedback in float32:
 *      sync_cfo = estimatedCFO, moved to known +- 2.0 when it lies further away (a NaN estimate stays); peek_cfo_hz is the
 *      estimate before the clamp.
 *   3. The CW0 peek (:1511-1597) on S1 = the span's soft bits.  648 <= S1 < 1296: robustDecodeSingleCW at R1/4, magic,
 *      truncation to 20 bytes, parseHeader: total_cw 1 falls through (RIA_PEEK_R14_ONE), > 1 is pending (R14_MULTI); otherwise,
 *      if the rate is not R1/4, the same at the rate: RATE_ONE, RATE_MULTI, magic with an invalid header pending 4
 *      (RATE_BAD_HEADER); nothing resolved: pending 4 (FAILED).  1296 <= S1 < 2592 on QAM16/32/64/256: pending 4 (QAM_PARTIAL).
 *      Otherwise the peek span's own soft bits are decoded (DIRECT).  A data header with total_cw 0 is an invalid header, as in
 *      ria_gpu_decode_frame_batch.
 *   4. Pass 2, if pending > 0: frame_len = getMinSamplesForCWCount(pending).  sync_start + frame_len > window_len: the reference
 *      would wait for samples - RIA_WIN_NEED_SAMPLES, need_samples = that frame_len.  Else pending > 4: RIA_WIN_TOO_LONG - this
 *      library's limit, the span demodulator takes at most a 4-codeword frame; pending_total_cw holds the header's count.  Else
 *      process() at sync_cfo, then fading index and CFO feedback again against the updated last_cfo_.
 *   5. decodeFrame (:1626) on that pass's soft bits: ria_gpu_decode_frame_batch's stages with the span's n_llr.
 *   6. Small-frame recovery (:1806-1853), if !success: process() at sync_cfo on the first getMinSamplesForCWCount(1) samples;
 *      with >= 648 soft bits trySmallFrame at R1/4 and then, if the rate is not R1/4, at the rate: robust decode, magic,
 *      parseHeader; total_cw 1: decodeFrame of the short span's bits, frame_len = that size; total_cw 2 or 3: process() on
 *      min(getMinSamplesForCWCount(total_cw), frame_len) samples and decodeFrame of those, frame_len = that size; the new result
 *      replaces the old one also where it fails.  No CFO feedback and no fading index are taken here (the reference reads neither).
 *   7. Timing recovery (:1859-1965), if !success && codewords_ok == 0 and RIA_ACQ_NO_TIMING_RETRY is clear:
 *      ria_gpu_rx_acquire_batch's candidates and fit rule on spans of the current frame_len at the current sync_cfo, marker off,
 *      abs_position = abs_base + sync_start + delta; a candidate with fewer than 648 soft bits is counted and skipped; each is
 *      decoded with decodeFrame; the first with success || codewords_ok > 0 is kept, its CFO estimate clamped against the
 *      current last_cfo_, its fading index taken.  A candidate that does not fit the window is skipped and not counted (the
 *      reference reads older ring-buffer samples, or a shorter span, there).
 *   8. Consumed (:1994-2013): frame_len, or for a successful control / connect frame min(frame_len,
 *      getMinSamplesForCWCount(codewords_ok + codewords_failed)); next_pos = frame_start + consumed, where a caller continues
 *      (ria_gpu_rx_burst_batch's continuation).
 * Out of scope: the PING energy test (disconnected only, :1168), burst groups and continuation, ring-buffer wrap-around, the
 * frame timeout, chase combining, OFDM-COX, and the weak-accept / reject-streak state (fold it into min_confidence).
 *
 * flags: the RIA_DECODE_* bits, RIA_DECODE_NO_CHANNEL_DEINTERLEAVE, RIA_BURST_INTERLEAVE, RIA_ACQ_NO_TIMING_RETRY; anything
 * else RIA_ERR_INVALID.  frame_row >= max(4, llrs_per_frame / 648) * bytes_per_codeword.  Under RIA_DEMOD_FUSED=1 the call
 * returns RIA_ERR_UNSUPPORTED.  n_windows == 0 is RIA_OK.  Every row of every output is written, zero where nothing applies.
 * acq_dev: ria_gpu_control_acquire_batch's row, with cfo_hz = ria_frame_status.cfo_hz of the reported span, delta / frame_start
 * of the reported candidate and candidates = spans demodulated at a timing candidate (1 + recovery candidates).  control_dev
 * (nullable): the control hypothesis's rows.  demod_status_dev (nullable): the status of the span behind the reported result
 * (the control span for RIA_WIN_CONTROL_PROFILE; zero for NEED_SAMPLES / TOO_LONG).
 * Work: every stage runs on ascending lists of the windows still open, one span-demodulator launch per span length (a pass
 * has at most five: n_ctl and 1..4 codewords), so results do not depend on scheduling or on the batch a window is in.  The
 * call synchronises its stream once per list whose length the host needs: at most 1 (control) + 4 demodulation passes + 2 x 2
 * (decodeFrame) + 8 x (1 + 2) recovery rounds + 1 = 34 small device-to-host reads; no samples, soft bits or payloads go to the
 * host.  A decode work-queue fault in a fixed stage fails the call with RIA_ERR_HIP.  Workspaces live on the two handles, are
 * carved once per size and reserved before anything of the call is in flight. */
enum { RIA_WIN_NOT_ACCEPTED = 0, RIA_WIN_BURST = 1, RIA_WIN_CONTROL_PROFILE = 2, RIA_WIN_DECODED = 3, RIA_WIN_NEED_SAMPLES = 4,
       RIA_WIN_TOO_LONG = 5 };
enum { RIA_PEEK_NONE = 0, RIA_PEEK_R14_ONE = 1, RIA_PEEK_R14_MULTI = 2, RIA_PEEK_RATE_ONE = 3, RIA_PEEK_RATE_MULTI = 4,
       RIA_PEEK_RATE_BAD_HEADER = 5, RIA_PEEK_FAILED = 6, RIA_PEEK_QAM_PARTIAL = 7, RIA_PEEK_DIRECT = 8 };
typedef struct ria_window_result {   /* 64 bytes, one per window */
    ria_dframe_result frame;         /* result: the DecodeResult delivered (all zero where nothing was decoded) */
    uint8_t  outcome;                /* RIA_WIN_* */
    uint8_t  peek;                   /* RIA_PEEK_*: which statement of :1505-1597 decided pass 1; NONE where the peek did not run */
    uint8_t  pending_total_cw;       /* pending_total_cw_ after the peek; 0 = fell through on the peek span */
    uint8_t  small_frame;            /* 0 not run, 1 ran and found nothing, 2 one-codeword branch, 3 exact-size (2..3) branch; bit 4: taken at the rate, not R1/4 */
    uint8_t  tries_peek_r14, tries_peek_rate, tries_small_r14, tries_small_rate;   /* decodes of the robust decoder, 0..5 */
    int32_t  frame_len;              /* frame_len as the reference leaves it, in samples */
    int32_t  next_pos;               /* sync_position_ + consumed within the window, -1 where nothing was consumed */
    int32_t  need_samples;           /* RIA_WIN_NEED_SAMPLES: the samples from sync_start pass 2 asks for, else 0 */
    float    sync_cfo_hz;            /* last_cfo_ / sync_cfo_ as the reference leaves them */
    float    peek_cfo_hz;            /* estimatedCFO() of the peek span before the clamp */
    float    fading_index;           /* last_fading_index_ as this window leaves it, 0 where no process() of the window set it */
} ria_window_result;

int ria_gpu_rx_window_batch(ria_gpu_handle control_h, ria_gpu_handle data_h, const float* samples_dev, int64_t stride,
                            int search_len, int window_len, int n_windows, const ria_acq_params* params_dev, uint32_t flags,
                            uint8_t* frame_out_dev, int frame_row, ria_window_result* result_dev, ria_acq_result* acq_dev,
                            ria_control_result* control_dev /* nullable */, ria_frame_status* demod_status_dev /* nullable: the reported span's */,
                            void* stream);

/* ---- from a capture to its next window: StreamingDecoder::searchForSync for a batch of captures ------------------------
 * ria_gpu_search_batch walks n_streams captures, each from its own cursor to the next accepted sync.  It replaces
 * gui::StreamingDecoder::searchForSync (src/gui/modem/streaming_decoder.cpp:386-941) with the part of feedAudio it depends
 * on (:184-225, :286-291): the search-buffer sizing (:404-438), the two waits for audio (:449-481), the ZC backlog catch-up
 * (:488-522), the 1000-sample RMS with the noise-floor tracker and the adaptive gate (:525-573), backtrack and step
 * (:589-612), light_sync_min_confidence / weak_sync_floor with the fading and SNR hints, the reject-streak relaxation and the
 * ZC reject-loop breaker (:662-716), the detector call with near miss, reject and weak accept (:725-783), sync_position_
 * (:858), anti-replay (:876-889), the +-1 Hz CFO sanity rule (:903-917) and estimateSNRFromChirp (:2587-2590).  The rules
 * are float32 with the reference's own argument order in std::max / std::min / std::clamp (ria_amd/csrc/search_rules.hpp), so
 * a NaN noise floor becomes 0.001 at the tracker, a NaN gate passes, and every result is the reference's bit for bit.
 *
 * Stream s lies at samples_dev + s*stride and holds capture_len_dev[s] samples, 0 <= capture_len <= min(stride, 959 999):
 * the 960 000-sample ring buffer never wraps, so a ring index is a capture index.  A longer capture, a state with fed outside
 * 0..capture_len, a cursor outside 0..959 999 or a negative streak is RIA_ERR_INVALID for the whole call: the domain is checked
 * on the device ahead of the walk, and no stream's state or result is written and no sample read.
 *
 * Modes.  RIA_SEARCH_OFDM_LTS: connected OFDM-CHIRP light sync (detectDataSync of OFDMChirpWaveform, min_search 67 304); the
 * modulation class - coherent PSK 0.90 / 0.85, QAM 0.78 / 0.70, differential 0.72 / 0.55 with the hint tiers - is the
 * handle's.  RIA_SEARCH_MCDPSK_ZC: connected MC-DPSK (ZC detectDataSync on roots DATA | CONTROL, min_search 31 120, backtrack
 * 19 200, step 1200, catch-up, near miss, breaker).  RIA_SEARCH_MCDPSK_CHIRP: the dual-chirp detectSync of the MC-DPSK
 * waveform (min_search 120 000, threshold 0.15, no acceptance rule): the disconnected handshake, or with
 * RIA_SEARCH_CONNECTED the connected "weak profile" (DBPSK with spreading, :417-421), which turns the CFO sanity rule on.
 * RIA_SEARCH_CONNECTED is implied by the first two modes.  cfg (the two MC-DPSK modes; NULL for LTS) is checked like the other
 * MC-DPSK calls' and does not change a result: preamble, detector and rules do not depend on it.
 *
 * Time model.  One invocation is one searchForSync().  After every invocation that leaves the stream open, feed_step
 * samples arrive through feedAudio's rule: count = min(feed_step, capture_len - fed); nothing happens for count 0; else a
 * cursor ahead of fed is clamped to it with the streak cleared, and fed += count.  That is the reference's own harness
 * (4800-sample chunks, one processBuffer() per chunk); feed_step 0 = the recording is all there.  The feed behind the last
 * invocation of a call is applied before the state is written, so a RIA_SEARCH_LIMIT state given to a second call continues
 * exactly as one longer call would.  A stream ends with
 *   RIA_SEARCH_SYNC_FOUND    the reference's state_ = SYNC_FOUND;
 *   RIA_SEARCH_NEED_SAMPLES  the invocation waits for audio (:449 or :475) and no more can arrive in this call (feed_step 0
 *                            or fed == capture_len).  A cursor AHEAD of fed is a wait too (counted in waits): the reference
 *                            would read ring-buffer samples that were never written; this library does not - its limit;
 *   RIA_SEARCH_LIMIT         max_invocations (>= 1) invocations have run.
 *
 * ria_search_state is read and written in place: correlation_pos_, total_fed_ = write_pos_, noise_floor_,
 * sync_reject_streak_, last_cfo_ (set to sync_cfo_ on SYNC_FOUND), last_fading_index_, last_snr_ (set to sync_snr_ on
 * SYNC_FOUND) and last_decoded_sync_pos_ (INT32_MIN for SIZE_MAX, as in ria_mcdpsk_acq_params; the caller sets it when a
 * frame is delivered).  A fresh decoder is {0, fed, 0.001f, 0, 0, 0, 0, INT32_MIN}.
 *
 * ria_search_result: the counters are this call's; search_start .. root are those of the stream's last detector run in
 * this call (search_start 0, sync_position -1, marker -1 where none ran).  With RIA_SEARCH_SYNC_FOUND, search_start,
 * search_len, known_cfo_hz, detect_threshold and min(min_confidence, correlation) are exactly the window geometry and the
 * ria_acq_params / ria_mcdpsk_acq_params fields that make ria_gpu_rx_window_batch / ria_gpu_mcdpsk_window_batch repeat this
 * detection on the window that starts at search_start (sync_start = sync_position - search_start, the same correlation):
 * neither call needed a change.
 *
 * Work: rounds of walk -> list -> (gather -> detect -> accept, in chunks of the list) until no detector is due; one small
 * device-to-host read per round (the list's length); no samples go to the host.  The walk runs a stream's invocations back
 * to back up to the first that passes the gate, so silence costs no round.  A chunk's spans live in a workspace of at most
 * 256 MiB on the handle (RIA_OPT_SEARCH_CHUNK: at most that many streams per chunk; 0 = the default), carved and reserved
 * before anything of the call is in flight.  No result depends on scheduling, on chunking or on the other streams.
 *
 * Not covered: the ZC-miss -> chirp fallback (:785-828; wall-clock state, connected_since_), ring-buffer wrap and the
 * overflow path of feedAudio (:227-278), disconnected OFDM (chirp) search, OFDM-COX and the frame timeout.  (A one-stream
 * host-memory form is ria_gpu_rx_stream_host's, below.) */
enum { RIA_SEARCH_OFDM_LTS = 0, RIA_SEARCH_MCDPSK_ZC = 1, RIA_SEARCH_MCDPSK_CHIRP = 2 };
enum { RIA_SEARCH_SYNC_FOUND = 1, RIA_SEARCH_NEED_SAMPLES = 2, RIA_SEARCH_LIMIT = 3 };
#define RIA_SEARCH_CONNECTED 0x1u
/*   RIA_OPT_SEARCH_CHUNK  ria_gpu_search_batch runs the detector on at most this many streams at a time (1..65535; 0 = as
 *                        many as 256 MiB of gathered spans hold). */
#define RIA_OPT_SEARCH_CHUNK 5
typedef struct ria_search_state {    /* 32 bytes, one per stream */
    int32_t correlation_pos;
    int32_t fed;
    float   noise_floor;
    int32_t reject_streak;
    float   last_cfo_hz;
    float   fading_hint;
    float   snr_hint;
    int32_t last_decoded_sync_pos;   /* INT32_MIN = none */
} ria_search_state;
typedef struct ria_search_result {   /* 112 bytes, one per stream */
    int32_t  outcome;                /* RIA_SEARCH_* */
    int32_t  search_start;
    int32_t  search_len;             /* min_search of the mode */
    int32_t  sync_position;          /* search_start + SyncResult::start_sample, -1 where nothing was found */
    int64_t  abs_position;           /* ringPosToAbsolute(sync_position): equal before the wrap */
    float    correlation;
    float    known_cfo_hz;           /* last_cfo_ the detector was called with */
    float    sync_cfo_hz;            /* sync_cfo_ after the CFO sanity rule (SYNC_FOUND) */
    float    sync_snr_db;            /* sync_snr_ (SYNC_FOUND) */
    float    detect_threshold;
    float    min_confidence;         /* light_sync_min_confidence of that invocation */
    int32_t  weak_accept;
    int32_t  marker;                 /* LTS: wasBurstInterleaved(); ZC: ZCFrameType; chirp: -1 */
    int32_t  root;                   /* ZC: root_detected; else -1 */
    uint32_t invocations, waits, rms_skips, detector_runs, rejects, near_misses, weak_accepts, replays;
    uint32_t catchups_moderate, catchups_severe;
    uint32_t reserved0, reserved1, reserved2;
} ria_search_result;
int ria_gpu_search_batch(ria_gpu_handle h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg /* NULL for RIA_SEARCH_OFDM_LTS */,
                         const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                         ria_search_state* state_dev, int feed_step, int max_invocations, ria_search_result* result_dev, void* stream);

/* ---- the same search for captures longer than the ring buffer ------------------------------------------------------------
 * ria_gpu_search_ring_batch is ria_gpu_search_batch - its arguments, its three modes, its time model, its outcomes, its
 * re-entrance (a RIA_SEARCH_LIMIT state continues exactly) and RIA_OPT_SEARCH_CHUNK - with the 960 000-sample ring buffer of
 * gui::StreamingDecoder and the whole of feedAudio (src/gui/modem/streaming_decoder.cpp:184-291), so a capture may be minutes
 * long.  Beyond what ria_gpu_search_batch replaces, it replaces the statements that depend on MAX_BUFFER_SAMPLES, write_pos_ =
 * total_fed_ % 960000 and total_fed_ (ria_amd/csrc/ring_rules.hpp): computeUnsearched on both branches (:193-202), the pre-wrap
 * clamp (:204, :289), the drift guard (:232-238, CORR_INVARIANT_GUARD 9600: a backlog above 950 400 after the wrap snaps the
 * cursor to the write position), the overflow drop (:242-278, OVERFLOW_RECOVERY_KEEP 360 000, need_to_drop, overflow_events_
 * and overflow_samples_dropped), the two waits on the circular backlog (:449, :466-481), the cursor initialisation
 * correlation_pos_ == 0 && total_fed_ >= 960000 -> write_pos_ (:458-464, which stays done when the second wait returns), the
 * ZC catch-up on the circular backlog (:488-522), the post-wrap backtrack (:597-605), sync_position_ modulo the ring (:858),
 * ringPosToAbsolute (:862-874) and the circular anti-replay with its cursor (:876-889): a sync at the ring index of the last
 * decoded frame one lap later is a replay, as in the reference.
 *
 * No ring is materialised.  With T = total_fed, ring index p holds x[p] for T < 960000 (0 for p >= T: never written) and
 * x[T - 1 - ((T - 1 - p) mod 960000)] otherwise; the kernels read the capture through that form.
 *
 * Time model: one invocation is one searchForSync(); after every invocation that leaves the stream open, count =
 * min(feed_step, capture_len - total_fed) samples arrive through the whole of feedAudio (count 0: nothing happens).  Before
 * the wrap a cursor ahead of total_fed is a wait, ria_gpu_search_batch's documented limit: on a capture of at most 959 999
 * samples the two calls give the same result and state.  After the wrap the reference's own arithmetic holds everywhere.
 *
 * Domain: 0 <= capture_len <= min(stride, 2^31 - 1 - 960000), 0 <= total_fed <= capture_len, correlation_pos in 0..959 999,
 * reject_streak >= 0, last_decoded_sync_pos in 0..959 999 or INT32_MIN.  Anything else is RIA_ERR_INVALID for the whole call,
 * checked on the device before any state or result is written or any sample read.
 *
 * ria_ring_state: ria_search_state's decoder with total_fed_ in 64 bits, correlation_pos and last_decoded_sync_pos as RING
 * indices, and the running overflow_events_ / stats_.overflow_samples_dropped.  A fresh decoder is {total_fed, 0, 0, 0.001f,
 * 0, 0, 0, INT32_MIN, 0, 0}.  ria_ring_search_result: ria_search_result's fields in its layout (search_start and
 * sync_position are ring indices; abs_position = ringPosToAbsolute(sync_position)), then abs_search_start =
 * ringPosToAbsolute(search_start), the capture index of span sample 0, this call's overflow_dropped, overflows, drift_snaps and
 * cursor_inits (executions of :462), and span_wraps: 1 when the last detector run's span [search_start, search_start +
 * search_len) modulo the ring had the write position strictly inside it.  Such a span holds the stream's newest samples
 * followed by its oldest, so it is not a contiguous piece of the capture and the window calls cannot repeat the detection at
 * abs_search_start; it needs a backlog above 960 000 minus the backtrack.  The search itself is exact there.
 *
 * Work: as ria_gpu_search_batch, on the same workspace; the gather reads the span through the closed form.
 *
 * Not covered: the ZC-miss -> chirp fallback (:785-828), disconnected OFDM (chirp) search, OFDM-COX and the frame timeout.
 * The stream loop on this search is ria_gpu_rx_ring_batch, behind ria_gpu_rx_stream_batch below. */
typedef struct ria_ring_state {      /* 48 bytes, one per stream */
    int64_t  total_fed;
    int32_t  correlation_pos;        /* ring index */
    int32_t  reject_streak;
    float    noise_floor;
    float    last_cfo_hz;
    float    fading_hint;
    float    snr_hint;
    int32_t  last_decoded_sync_pos;  /* ring index, INT32_MIN = none */
    uint32_t overflow_events;
    uint64_t overflow_dropped;
} ria_ring_state;
typedef struct ria_ring_search_result {   /* 144 bytes, one per stream: ria_search_result's 112, then the ring's */
    int32_t  outcome;                /* RIA_SEARCH_* */
    int32_t  search_start;           /* ring index */
    int32_t  search_len;
    int32_t  sync_position;          /* ring index, -1 where nothing was found */
    int64_t  abs_position;           /* ringPosToAbsolute(sync_position) */
    float    correlation;
    float    known_cfo_hz;
    float    sync_cfo_hz;
    float    sync_snr_db;
    float    detect_threshold;
    float    min_confidence;
    int32_t  weak_accept;
    int32_t  marker;
    int32_t  root;
    uint32_t invocations, waits, rms_skips, detector_runs, rejects, near_misses, weak_accepts, replays;
    uint32_t catchups_moderate, catchups_severe;
    uint32_t reserved0, reserved1, reserved2;
    int64_t  abs_search_start;       /* ringPosToAbsolute(search_start) */
    uint64_t overflow_dropped;
    uint32_t overflows, drift_snaps, cursor_inits;
    uint32_t span_wraps;
} ria_ring_search_result;
int ria_gpu_search_ring_batch(ria_gpu_handle h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg /* NULL for RIA_SEARCH_OFDM_LTS */,
                              const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                              ria_ring_state* state_dev, int feed_step, int max_invocations, ria_ring_search_result* result_dev, void* stream);

/* ---- recordings in, frames out: the receive loop of StreamingDecoder for a batch of captures ----------------------------------
 * ria_gpu_rx_stream_batch runs gui::StreamingDecoder::processBuffer's loop (src/gui/modem/streaming_decoder.cpp:293-384) -
 * searchForSync (:386-941), decodeCurrentFrame (:943-2013), the state both leave - over n_streams captures, as a composition
 * of this library's calls with the host's part between them done on the device: ria_gpu_search_batch on the streams still
 * open, then the window call of the mode on every stream that found a sync, then the state update, and again.  It adds no
 * receiver arithmetic; every rule between the calls is ria_amd/csrc/stream_rules.hpp's.  Captures, capture_len_dev, state_dev,
 * mode, flags, cfg, feed_step and max_invocations (per search leg) are ria_gpu_search_batch's, with its domain and its errors.
 *
 * Per round, for the open streams:
 *   1. the search.  A stream that does not end with RIA_SEARCH_SYNC_FOUND closes with the search's outcome.
 *   2. A found stream gets the window [search_start, search_start + min(full, capture_len - search_start)), full =
 *      search_len + frame_samples + 32 for RIA_SEARCH_OFDM_LTS and search_len + the 8-codeword span of cfg (9 x 512 +
 *      8 x ceil(648 / (carriers x bits)) x 512 x spreading samples) for the MC-DPSK modes: the window calls' documented minimum.
 *   3. Its parameters are the search result's: known_cfo_hz, detect_threshold, min(min_confidence, correlation), abs_base =
 *      search_start; for MC-DPSK last_decoded_sync = last_decoded_sync_pos - search_start (INT32_MIN kept, clipped to
 *      -(2^31 - 1) .. 2^31 - 1), pending_total_cw 0, first_avail 0.
 *   4. The window call: ria_gpu_rx_window_batch(control_h, h) with RIA_DECODE_FULL for OFDM; ria_gpu_mcdpsk_window_batch on h
 *      for MC-DPSK - RIA_MACQ_SYNC_CHIRP for the chirp mode, RIA_MACQ_DISCONNECTED with it unless RIA_SEARCH_CONNECTED - with
 *      no chase pool, no channel interleaving and no soft-bit output.
 *   5. The state (:1994-2013, :1414-1434): last_cfo_hz = the window's CFO and fading_hint = its fading index where the outcome
 *      is DECODED (OFDM: or CONTROL_PROFILE); last_decoded_sync_pos = sync_position of an OFDM window that delivered (success or
 *      codewords_ok > 0), or what the MC-DPSK window call leaves, back in capture indices; the cursor = search_start + next_pos
 *      where next_pos >= 0, sync_position + the one-frame span (frame_samples; the 1-codeword span of cfg) for RIA_WIN_BURST /
 *      RIA_WIN_TOO_LONG / RIA_MWIN_TOO_LONG, which the host passes on to another call, else unchanged; then fed = max(fed,
 *      min(capture_len, cursor)): the samples a window consumed have arrived, so the next feed does not clamp the cursor back.
 *   6. The event is recorded and the stream closes on a window NEED_SAMPLES, on max_events events, or on a cursor >= 959 999.
 * state_dev is read and written in place, the fed rule applied before it is written: a second call with the state a first
 * call left continues exactly as one call with a larger max_events would.
 *
 * Event e of stream s is events_dev[s * max_events + e], its payload row (s * max_events + e) of frames_dev (frame_row bytes;
 * frame_bytes of them where delivered, zero otherwise).  Every row of every output is written.  frame_row >= the window
 * call's minimum: max(4, llrs_per_frame / 648) * bytes_per_codeword for OFDM, RIA_MACQ_FRAME_BYTES(8) for MC-DPSK.  control_h:
 * ria_gpu_rx_window_batch's control handle for RIA_SEARCH_OFDM_LTS, NULL for the other modes.  The MC-DPSK modes need a handle
 * at RIA_RATE_1_4.  max_events >= 1.  n_streams == 0 is RIA_OK.  A failure of the search's domain check fails the whole call
 * before anything is written.
 *
 * Out of scope: burst groups and continuation (reported as events: RIA_WIN_BURST), chase pools and channel interleaving,
 * re-entry of an MC-DPSK NEED_SAMPLES window (the event carries need_samples and pending_total_cw for the caller) - these
 * three are ria_gpu_mcdpsk_stream_batch's, below -, ring wrap, the ZC-miss -> chirp fallback, OFDM-COX.
 *
 * Work: rounds of search -> found list -> (gather -> parameters -> window call -> apply, once per distinct window length in
 * ascending order, in chunks of at most 256 MiB of windows) -> open list.  A stream gains an event or closes in every round,
 * so there are at most max_events + 1 rounds.  Per round the call itself makes two small device-to-host reads - the found
 * list with its window lengths (16 + 8 x n_streams bytes) and the number of streams still open - beside those of the search
 * and of the window calls; most streams share `full`, only windows cut at a capture's end differ, so a round usually makes one
 * window call.  No samples, soft bits, result records or payloads go to the host.  The search runs on the open streams through
 * an index list, without copying their captures.  The call's workspace lives on h, is carved once per size and reserved before
 * the call's first launch; the window calls' own workspaces grow, where they must, on a drained stream. */
enum { RIA_STREAM_SEARCH_NEED_SAMPLES = 2, RIA_STREAM_SEARCH_LIMIT = 3,    /* = RIA_SEARCH_NEED_SAMPLES, RIA_SEARCH_LIMIT */
       RIA_STREAM_WINDOW_NEED_SAMPLES = 4, RIA_STREAM_EVENTS_FULL = 5, RIA_STREAM_RING_END = 6 };
typedef struct ria_stream_event {    /* 64 bytes */
    int32_t sync_position;           /* the search's, a capture index */
    int32_t search_start;            /* sample 0 of the window */
    int32_t window_len;
    int32_t outcome;                 /* RIA_WIN_* (OFDM) / RIA_MWIN_* (MC-DPSK) */
    int32_t next_pos;                /* the window's next_pos as a capture index, -1 where nothing was consumed */
    int32_t frame_bytes;             /* bytes of the DecodeResult's frame_data */
    int32_t need_samples;
    int32_t pending_total_cw;
    uint8_t delivered;               /* the host queues the result: its frame_bytes bytes are in the payload row */
    uint8_t success, codewords_ok, codewords_failed;
    uint8_t frame_type;
    uint8_t reserved0[3];
    float   correlation;             /* the search's */
    float   cfo_hz;                  /* ria_window_result.sync_cfo_hz / ria_mcdpsk_acq_result.cfo_hz */
    float   fading_index;
    float   snr_db;                  /* the search's sync_snr_db */
    int32_t reserved[2];
} ria_stream_event;
typedef struct ria_stream_result {   /* 64 bytes, one per stream */
    int32_t  n_events;
    int32_t  closed;                 /* RIA_STREAM_* */
    int32_t  mode;                   /* RIA_SEARCH_*: names the family of the events' outcomes */
    int32_t  search_legs;            /* searches the stream took part in */
    uint32_t invocations, waits, rms_skips, detector_runs, rejects, near_misses, weak_accepts, replays;   /* summed over the legs */
    uint32_t catchups_moderate, catchups_severe;
    uint32_t reserved[2];
} ria_stream_result;
int ria_gpu_rx_stream_batch(ria_gpu_handle h, ria_gpu_handle control_h /* RIA_SEARCH_OFDM_LTS only, else NULL */,
                            int mode /* RIA_SEARCH_* */, uint32_t flags /* RIA_SEARCH_CONNECTED only */,
                            const ria_mcdpsk_config* cfg /* NULL for RIA_SEARCH_OFDM_LTS */,
                            const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                            ria_search_state* state_dev, int feed_step, int max_invocations, int max_events,
                            ria_stream_event* events_dev /* n_streams * max_events */,
                            uint8_t* frames_dev /* n_streams * max_events * frame_row */, int frame_row,
                            ria_stream_result* result_dev /* n_streams */, void* stream);
/* One stream from host memory: the capture (n_samples <= 959 999) and *state_host are staged through the handle's pinned block
 * on the handle's own stream, the state, max_events events, their payload rows and the result are copied back; synchronises
 * that stream. */
int ria_gpu_rx_stream_host(ria_gpu_handle h, ria_gpu_handle control_h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                           const float* samples_host, int n_samples, ria_search_state* state_host /* in and out */,
                           int feed_step, int max_invocations, int max_events, ria_stream_event* events_out_host,
                           uint8_t* frames_out_host, int frame_row, ria_stream_result* result_out_host);

/* ---- the MC-DPSK stream loop with a chase pool, channel interleaving and re-entry ---------------------------------------------
 * ria_gpu_mcdpsk_stream_batch is ria_gpu_rx_stream_batch for the two MC-DPSK modes (RIA_SEARCH_OFDM_LTS is RIA_ERR_INVALID)
 * with the three things that call leaves out; ria_gpu_mcdpsk_window_batch has them all, and every decode is that call's.  The
 * loop, the events, the results, the RIA_STREAM_* close reasons, the domain of captures and search states, feed_step,
 * max_invocations, max_events and frame_row (>= RIA_MACQ_FRAME_BYTES(8)) are the stream call's; h is at RIA_RATE_1_4.  The
 * rules it adds are ria_amd/csrc/mcdpsk_stream_rules.hpp's.  With pool NULL, window_flags 0 and no stream pending, every
 * output - events, payload rows, results and the `search` part of the state - equals ria_gpu_rx_stream_batch's byte for byte.
 *
 * Time for the cache.  The caller owns the clock, the call turns it into an audio clock: every window of stream s is decoded
 * at now_ms = t0_ms_dev[s] + (uint64)sync_position * 1000 / sample_rate (48000, the handle's), integer and modulo 2^64 as the
 * pool's own arithmetic; a re-entered window has the same sync_position, hence the same now_ms.  Stream s uses cache
 * cache_id_dev[s] (< 0: no chase for that stream).  Successive windows of a stream run in successive rounds, the order a
 * cache needs: a retransmission on the same recording finds what the first reception stored.  pool NULL: no chase;
 * cache_id_dev and t0_ms_dev are then not read.  A pool of another handle is RIA_ERR_INVALID.
 *
 * The up-front check runs on the device ahead of everything and is read with the call's first control read, before any state,
 * cache or output is written.  RIA_ERR_INVALID for the whole call: a capture or search state outside ria_gpu_search_batch's
 * domain; two streams with the same cache id >= 0 (negative ids may repeat), or an id >= n_caches - the window call's own
 * check sees one length group of one round only; pending_total_cw outside 0..255; with pending_total_cw > 0, a negative
 * need_samples, a pend_search_start or pend_sync_position outside the capture, or a capture that no longer holds the search
 * span behind pend_search_start.
 *
 * Channel interleaving: window_flags (0 or RIA_MACQ_CHANNEL_INTERLEAVE) and interleaver_bits go to the window call unchanged;
 * their domain and errors are the *_ci_batch calls' (another flag, or interleaver_bits outside 1..648 with the flag, is
 * RIA_ERR_INVALID before anything is launched).
 *
 * Pending, written.  A window that answers RIA_MWIN_NEED_SAMPLES records its event and closes the stream with
 * RIA_STREAM_WINDOW_NEED_SAMPLES as in the stream call, and leaves the reference's SYNC_FOUND wait (streaming_decoder.cpp:
 * 943-1019) in the state: pending_total_cw, need_samples, pend_search_start, pend_sync_position, the three window parameters
 * it was called with and the search's correlation.  Every other window outcome writes the eight fields as zero.  The cursor
 * and fed follow the stream call's rules.
 *
 * Pending, read.  A stream that comes in with pending_total_cw > 0 is not searched in the first round.
 *   - capture_len >= pend_sync_position + need_samples: it gets, in a round of its own ahead of the first search leg, the
 *     window [pend_search_start, pend_search_start + min(capture_len - pend_search_start, max(full, pend_sync_position -
 *     pend_search_start + need_samples))) with the stored parameters and pending_total_cw as the window call's re-entry
 *     input.  fed = max(fed, pend_sync_position + need_samples) is applied first, last_decoded_sync is rebased as usual,
 *     then the ordinary state rule runs.  The event's sync_position, search_start and correlation come from the pending
 *     fields, snr_db from search.snr_hint (which the search set to sync_snr_ when it found this sync).  After that the
 *     stream searches on like any other.
 *   - otherwise it closes at once with RIA_STREAM_WINDOW_NEED_SAMPLES, no event, and its state unchanged bit for bit.
 * A caller that gives up (the reference's frame timeout) zeroes pending_total_cw: the stream then searches from its cursor.
 *
 * Outputs: every row of every output is written, zero where nothing applies - events_dev, frames_dev, result_dev and
 * harq_dev (nullable; row s * max_events + e is the ria_mcdpsk_harq_result of event e's window).  n_streams == 0 is RIA_OK.
 * RIA_ERR_INVALID leaves everything as it was.  After any other error (RIA_ERR_HIP from a launch or a broken internal bound)
 * state_dev is unspecified: the pending fields are written window by window, the search part only behind the last round.
 *
 * Work: the stream call's rounds; ahead of them the up-front check (one small device-to-host read more than the stream
 * call's worst case) and, only when a stream comes in pending, the re-entry round (the pending list, its window calls and
 * the open list: the reads of one more round).  Thread per stream or per window, every list an ascending scan: no result
 * depends on chunking, grouping or scheduling.  The search works on a contiguous copy of the states' search parts, written
 * back behind the last round.  The workspace lives on h, is carved once per size - with room for one re-entered window of a
 * whole capture - and reserved before the call's first launch.
 *
 * Still out of scope: burst groups and OFDM, ring wrap (that is ria_gpu_mcdpsk_ring_batch, below), the ZC-miss -> chirp
 * fallback, and the frame timeout (the caller's clock: it zeroes pending_total_cw). */
typedef struct ria_mcdpsk_stream_state {   /* 64 bytes, one per stream */
    ria_search_state search;               /* as ria_gpu_rx_stream_batch reads and writes it */
    int32_t pending_total_cw;              /* 0: searching; n > 0: waiting at a found sync (SYNC_FOUND with pending_total_cw_ = n) */
    int32_t need_samples;                  /* samples from pend_sync_position the next pass waits for */
    int32_t pend_search_start;             /* sample 0 of the window that answered NEED_SAMPLES */
    int32_t pend_sync_position;            /* capture index */
    float   pend_known_cfo_hz, pend_detect_threshold, pend_min_confidence, pend_correlation;
                                           /* the window parameters that repeat the detection, and the event's correlation */
} ria_mcdpsk_stream_state;
int ria_gpu_mcdpsk_stream_batch(ria_gpu_handle h, int mode /* RIA_SEARCH_MCDPSK_ZC | RIA_SEARCH_MCDPSK_CHIRP */,
                                uint32_t flags /* RIA_SEARCH_CONNECTED */, uint32_t window_flags /* 0 | RIA_MACQ_CHANNEL_INTERLEAVE */,
                                int interleaver_bits, const ria_mcdpsk_config* cfg,
                                const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                                ria_mcdpsk_stream_state* state_dev, int feed_step, int max_invocations, int max_events,
                                ria_chase_pool pool /* nullable */, const int32_t* cache_id_dev /* [n_streams], < 0: off */,
                                const uint64_t* t0_ms_dev /* [n_streams] */,
                                ria_stream_event* events_dev, uint8_t* frames_dev, int frame_row,
                                ria_mcdpsk_harq_result* harq_dev /* nullable, [n_streams * max_events], parallel to events_dev */,
                                ria_stream_result* result_dev, void* stream);
/* One recording from host memory, as ria_gpu_rx_stream_host: staged through the handle's pinned block on the handle's own
 * stream, which it synchronises.  pool (nullable) stays on the device; the stream uses cache cache_id at clock t0_ms.
 * harq_out_host (nullable) takes max_events records. */
int ria_gpu_mcdpsk_stream_host(ria_gpu_handle h, int mode, uint32_t flags, uint32_t window_flags, int interleaver_bits,
                               const ria_mcdpsk_config* cfg, const float* samples_host, int n_samples,
                               ria_mcdpsk_stream_state* state_host /* in and out */, int feed_step, int max_invocations, int max_events,
                               ria_chase_pool pool /* nullable */, int32_t cache_id, uint64_t t0_ms,
                               ria_stream_event* events_out_host, uint8_t* frames_out_host, int frame_row,
                               ria_mcdpsk_harq_result* harq_out_host /* nullable */, ria_stream_result* result_out_host);

/* ---- recordings longer than the ring buffer in, frames out -----------------------------------------------------------------
 * ria_gpu_rx_ring_batch is ria_gpu_rx_stream_batch's loop on ria_gpu_search_ring_batch, with the window leg in absolute
 * indices.  Arguments as for the stream call, with ria_ring_state; domain and errors are the ring search's.
 *   1. the ring search on the open streams.  A stream that does not end with RIA_SEARCH_SYNC_FOUND closes with the search's
 *      outcome; a found one whose span crossed the write position (span_wraps) closes with RIA_STREAM_SPAN_LOST: its window
 *      is no contiguous piece of the capture (reachable only with a backlog above 960 000 minus the backtrack).
 *   2. A found stream gets the window [abs_search_start, abs_search_start + min(full, capture_len - abs_search_start)) of
 *      the capture; full is the stream call's.  A configuration whose full exceeds 959 999 is RIA_ERR_INVALID.
 *   3. Parameters: the stream call's, with abs_base = abs_search_start; for MC-DPSK last_decoded_sync = the circular
 *      difference last_decoded_sync_pos - search_start on the ring, in -480 000 .. 479 999 (INT32_MIN kept).
 *   4. The window call of the mode, unchanged.
 *   5. The state: last_cfo_hz / fading_hint as in the stream call; last_decoded_sync_pos a ring index (sync_position on a
 *      delivered OFDM frame; what the MC-DPSK window call leaves, plus search_start, modulo the ring); the cursor =
 *      (search_start + next_pos) % 960000, behind the first frame of a RIA_WIN_BURST / TOO_LONG window (sync + first frame,
 *      modulo the ring), else where the search left it; total_fed = max(total_fed, min(capture_len, absolute cursor)) - a
 *      direct assignment, not a feedAudio: backlog plus arrivals stay below full <= 959 999 there, so the overflow drop
 *      could not have fired (ria_amd/csrc/ring_rules.hpp, ring_window_arrival).
 *   6. The event: a ria_stream_event whose sync_position, search_start and next_pos are CAPTURE (absolute) indices.
 * A stream closes with RIA_STREAM_SEARCH_NEED_SAMPLES, RIA_STREAM_SEARCH_LIMIT, RIA_STREAM_WINDOW_NEED_SAMPLES,
 * RIA_STREAM_EVENTS_FULL or RIA_STREAM_SPAN_LOST; there is no RIA_STREAM_RING_END.  ria_ring_stream_result is
 * ria_stream_result's 64 bytes, then the ring search's overflow_dropped, overflows, drift_snaps and cursor_inits summed over
 * the legs.  Re-entrant through ria_ring_state as the stream call is.  The workspace is carved once and reserved before the
 * first launch.  Feed long recordings with feed_step > 0 (4800): one that is "all there" shows the decoder only its last
 * 960 000 samples, as the reference's would.
 * Still out of scope: burst groups and continuation, the ZC-miss -> chirp fallback, OFDM-COX and the frame timeout; chase
 * pools, channel interleaving and MC-DPSK NEED_SAMPLES re-entry are ria_gpu_mcdpsk_ring_batch's, below.
 * ria_gpu_rx_ring_host takes one recording of any length in the domain from host memory: it is copied in pieces through the
 * handle's pinned block into a device buffer the handle owns, grown before anything is in flight. */
#define RIA_STREAM_SPAN_LOST 7
typedef struct ria_ring_stream_result {   /* 88 bytes, one per stream: ria_stream_result's 64, then the ring's */
    int32_t  n_events;
    int32_t  closed;                 /* RIA_STREAM_* */
    int32_t  mode;
    int32_t  search_legs;
    uint32_t invocations, waits, rms_skips, detector_runs, rejects, near_misses, weak_accepts, replays;
    uint32_t catchups_moderate, catchups_severe;
    uint32_t reserved[2];
    uint64_t overflow_dropped;
    uint32_t overflows, drift_snaps, cursor_inits;
    uint32_t reserved1;
} ria_ring_stream_result;
int ria_gpu_rx_ring_batch(ria_gpu_handle h, ria_gpu_handle control_h /* RIA_SEARCH_OFDM_LTS only, else NULL */, int mode, uint32_t flags,
                          const ria_mcdpsk_config* cfg, const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                          ria_ring_state* state_dev, int feed_step, int max_invocations, int max_events,
                          ria_stream_event* events_dev /* n_streams * max_events */, uint8_t* frames_dev, int frame_row,
                          ria_ring_stream_result* result_dev, void* stream);
int ria_gpu_rx_ring_host(ria_gpu_handle h, ria_gpu_handle control_h, int mode, uint32_t flags, const ria_mcdpsk_config* cfg,
                         const float* samples_host, int n_samples, ria_ring_state* state_host /* in and out */,
                         int feed_step, int max_invocations, int max_events, ria_stream_event* events_out_host,
                         uint8_t* frames_out_host, int frame_row, ria_ring_stream_result* result_out_host);

/* ---- the MC-DPSK link on recordings longer than the ring buffer ---------------------------------------------------------------
 * ria_gpu_mcdpsk_ring_batch is ria_gpu_rx_ring_batch's loop for the two MC-DPSK modes (RIA_SEARCH_OFDM_LTS is RIA_ERR_INVALID)
 * with what ria_gpu_mcdpsk_stream_batch adds to the stream call: a chase pool on the audio clock, channel interleaving, and
 * re-entry at a NEED_SAMPLES window.  It replaces, for such recordings, gui::StreamingDecoder::processBuffer's loop
 * (src/gui/modem/streaming_decoder.cpp:293-384) with the SYNC_FOUND wait (:943-1019, pending_total_cw_) and the ChaseCache the
 * reference's MC-DPSK decode keeps between receptions.  Steps 1 to 6 are the ring call's: the ring search, RIA_STREAM_SPAN_LOST,
 * windows cut from the capture by absolute index with abs_base = abs_search_start, last_decoded_sync rebased on the ring, the
 * cursor and last_decoded_sync_pos written back as ring indices, total_fed assigned by its rule, events in capture indices,
 * ria_ring_stream_result with its counters; every decode is ria_gpu_mcdpsk_window_batch's.  The rules it adds are
 * ria_amd/csrc/mcdpsk_ring_rules.hpp's.  h is at RIA_RATE_1_4; frame_row >= RIA_MACQ_FRAME_BYTES(8).  With pool NULL,
 * window_flags 0 and no stream pending, events, payload rows, results and the `ring` part of the state equal
 * ria_gpu_rx_ring_batch's byte for byte; on captures of at most 959 999 samples the call equals ria_gpu_mcdpsk_stream_batch.
 *
 * Time for the cache.  Every window of stream s is decoded at now_ms = t0_ms_dev[s] + (uint64)abs_position * 1000 / sample_rate,
 * abs_position the sync's ABSOLUTE (capture) index, never its ring index: on the ring index the cache's clock would jump back
 * 20 s at every lap, and the pool's age (now - last access, signed) would turn negative there, so an entry past its TTL
 * would still combine.  A re-entered window uses pend_sync_position, hence the same now_ms as before.  Cache ids, pool NULL, a pool of another handle, window_flags / interleaver_bits with their errors, and "successive
 * windows of a stream run in successive rounds" are the MC-DPSK stream call's, unchanged.
 *
 * The up-front check runs on the device ahead of everything and is read with the call's first control read, before any state,
 * cache or output is written.  RIA_ERR_INVALID for the whole call: a capture or `ring` state outside
 * ria_gpu_search_ring_batch's domain; a configuration whose `full` window exceeds 959 999; two streams with the same cache id
 * >= 0, or an id >= n_caches; pending_total_cw outside 0..255; with pending_total_cw > 0, a negative need_samples, a
 * pend_search_start or pend_sync_position outside [0, capture_len), capture_len - pend_search_start < search_len, a span
 * pend_sync_position - pend_search_start + need_samples above 959 999 (it does not fit one ring: the reference cannot wait for
 * it), or a window whose first sample the ring no longer holds or whose search span it was never fed (ring.total_fed -
 * pend_search_start > 960 000, or pend_search_start + search_len > ring.total_fed): no state the reference can reach.
 *
 * Pending, written.  A window that answers RIA_MWIN_NEED_SAMPLES records its event, closes the stream with
 * RIA_STREAM_WINDOW_NEED_SAMPLES and writes the eight pending fields, pend_search_start = abs_search_start and
 * pend_sync_position = abs_position (CAPTURE indices; they fit int32_t, captures end at 2^31 - 1 - 960 000), the three window
 * parameters it was called with and the search's correlation.  Every other window outcome writes the eight fields as zero.
 *
 * Pending, read.  A stream that comes in with pending_total_cw > 0 is not searched in the first round.
 *   - capture_len >= pend_sync_position + need_samples: it gets, in a round of its own ahead of the first search leg, the
 *     window [pend_search_start, pend_search_start + min(capture_len - pend_search_start, max(full, pend_sync_position -
 *     pend_search_start + need_samples))) with the stored parameters, abs_base = pend_search_start and pending_total_cw as
 *     the window call's re-entry input.  total_fed = max(total_fed, pend_sync_position + need_samples) is applied first, then
 *     last_decoded_sync is rebased against pend_search_start modulo the ring, then the ring call's state rule (its step 5)
 *     runs.  Neither assignment of total_fed is a feedAudio: backlog plus arrivals stay below 960 000 because the re-entered
 *     span is at most 959 999 (mcdpsk_ring_rules.hpp, mcring_reentry_arrival).  The event's positions and correlation come
 *     from the pending fields, snr_db from ring.snr_hint.  After that the stream searches on like any other.
 *   - otherwise it closes at once with RIA_STREAM_WINDOW_NEED_SAMPLES, no event, and its state unchanged bit for bit.
 *
 * Outputs: every row of every output is written, zero where nothing applies - events_dev, frames_dev, result_dev and
 * harq_dev (nullable; row s * max_events + e is the ria_mcdpsk_harq_result of event e's window).  n_streams == 0 is RIA_OK.
 * RIA_ERR_INVALID leaves everything as it was.  After RIA_ERR_HIP state_dev is unspecified, as in the MC-DPSK stream call.
 *
 * Work: ria_gpu_rx_ring_batch's rounds and reads; ahead of them the up-front check (one small device-to-host read) and, only
 * when a stream comes in pending, the re-entry round (the pending list, its window calls and the open list).  Thread per
 * stream or per window, every list an ascending scan: no result depends on chunking, grouping or scheduling.  The window
 * gather indexes the captures in 64 bits and reads only inside a stream's own [0, capture_len).  The ring search works on a
 * contiguous copy of the states' `ring` parts, written back behind the last round.  The workspace lives on h, is carved once
 * per size - with room for one re-entered window of 959 999 samples - and reserved before the call's first launch; windows go
 * in chunks of at most 256 MiB.
 *
 * Still out of scope: OFDM and burst groups on the ring, the ZC-miss -> chirp fallback, OFDM-COX, and the frame timeout (the
 * caller's clock: it zeroes pending_total_cw, and the stream then searches from its cursor).
 * ria_gpu_mcdpsk_ring_host takes one recording of any length in the domain from host memory, staged in pieces as
 * ria_gpu_rx_ring_host does; pool (nullable) stays on the device, the stream uses cache cache_id at clock t0_ms; harq_out_host
 * (nullable) takes max_events records. */
typedef struct ria_mcdpsk_ring_state {   /* 80 bytes, one per stream */
    ria_ring_state ring;                 /* as ria_gpu_rx_ring_batch reads and writes it */
    int32_t pending_total_cw;            /* 0: searching; n > 0: waiting at a found sync (SYNC_FOUND with pending_total_cw_ = n) */
    int32_t need_samples;                /* samples from pend_sync_position the next pass waits for */
    int32_t pend_search_start;           /* CAPTURE (absolute) index of sample 0 of the window that answered NEED_SAMPLES */
    int32_t pend_sync_position;          /* CAPTURE (absolute) index */
    float   pend_known_cfo_hz, pend_detect_threshold, pend_min_confidence, pend_correlation;
                                         /* the window parameters that repeat the detection, and the event's correlation */
} ria_mcdpsk_ring_state;
int ria_gpu_mcdpsk_ring_batch(ria_gpu_handle h, int mode /* RIA_SEARCH_MCDPSK_ZC | RIA_SEARCH_MCDPSK_CHIRP */,
                              uint32_t flags /* RIA_SEARCH_CONNECTED */, uint32_t window_flags /* 0 | RIA_MACQ_CHANNEL_INTERLEAVE */,
                              int interleaver_bits, const ria_mcdpsk_config* cfg,
                              const float* samples_dev, int64_t stride, const int32_t* capture_len_dev, int n_streams,
                              ria_mcdpsk_ring_state* state_dev, int feed_step, int max_invocations, int max_events,
                              ria_chase_pool pool /* nullable */, const int32_t* cache_id_dev /* [n_streams], < 0: off */,
                              const uint64_t* t0_ms_dev /* [n_streams] */,
                              ria_stream_event* events_dev, uint8_t* frames_dev, int frame_row,
                              ria_mcdpsk_harq_result* harq_dev /* nullable, [n_streams * max_events], parallel to events_dev */,
                              ria_ring_stream_result* result_dev, void* stream);
int ria_gpu_mcdpsk_ring_host(ria_gpu_handle h, int mode, uint32_t flags, uint32_t window_flags, int interleaver_bits,
                             const ria_mcdpsk_config* cfg, const float* samples_host, int n_samples,
                             ria_mcdpsk_ring_state* state_host /* in and out */, int feed_step, int max_invocations, int max_events,
                             ria_chase_pool pool /* nullable */, int32_t cache_id, uint64_t t0_ms,
                             ria_stream_event* events_out_host, uint8_t* frames_out_host, int frame_row,
                             ria_mcdpsk_harq_result* harq_out_host /* nullable */, ria_ring_stream_result* result_out_host);

/* ---- debug / test hooks ----------------------------------------------------------------------- */
/* op: 0 sinf 1 cosf 2 logf 3 atan2f(a,b) 4 hypotf(a,b) 5 a/b 6 sqrtf(a); evaluates the device
 * math the kernels use on n arguments (tests compare against the host libm). */
int ria_gpu_debug_math(ria_gpu_handle h, int op, const float* a_dev, const float* b_dev, int n,
                       float* out_dev, void* stream);
/* 1 if, in the handle's last decode calls, a persistent work-queue wave left its loop through the iteration bound
 * instead of the queue's end (a broken queue loop terminates and is reported, it does not hang the GPU); 0 if not;
 * negative = error.  Synchronises the device. */
int ria_gpu_debug_queue_fault(ria_gpu_handle h);
/* Counters of the CRC recovery (device path) of the last call that ran it on stream slot `slot` (0 for every call but the
 * parts 1.. of a split ria_gpu_rx_batch): out[0] frames flagged (four converged codewords, frame check fails), out[1]
 * frames stage 1 could not repair (they reach the fallback stage), out[2] codewords with re-decodes queued for it,
 * out[3] (codeword, factor) re-decodes queued.  All zero before the first such call.  Synchronises the device. */
int ria_gpu_debug_recovery_counts(ria_gpu_handle h, int slot, uint32_t out[4]);
/* Decodes that the repeated-state exit (RIA_OPT_STATE_EXIT) ended in the last decode call on stream slot `slot`: out[0] all,
 * out[1] in phase 0, out[2] in the cascade, out[3] in the recovery fill.  Attempts behind a codeword's winner and factor
 * decodes behind its first converging one run or not depending on timing, so the counts vary a little from call to call.
 * All zero before the first call, with the option off and at a rate without the exit.  Synchronises the device. */
int ria_gpu_debug_state_exits(ria_gpu_handle h, int slot, uint32_t out[4]);
/* First decodes (factor 0.9375) of the last decode call on stream slot `slot`: out[0] those the frame walk did not make
 * because an earlier codeword of the frame had failed (the decoder then stays at 0.875 and nobody reads them), out[1] those
 * of them that were made after all because a phase-0 rescue put the decoder back to 0.9375.  Both are functions of the
 * input alone.  Zero before the first call and without RIA_DECODE_PERTURB.  Synchronises the device. */
int ria_gpu_debug_first_decodes(ria_gpu_handle h, int slot, uint32_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* RIA_GPU_H */
