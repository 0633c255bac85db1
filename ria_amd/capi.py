"""ctypes binding of include/ria_gpu.h.  Device memory comes from torch (plumbing only): every
wrapper takes CUDA/HIP tensors and passes raw device pointers across the C ABI."""
import ctypes as C
import os

from . import build as _build

RIA_OK = 0
MOD = {"DBPSK": 0, "BPSK": 1, "DQPSK": 2, "QPSK": 3, "D8PSK": 4, "QAM16": 6, "QAM32": 7, "QAM64": 8, "QAM256": 10}
RATE = {"R1_4": 0, "R1_3": 1, "R1_2": 2, "R2_3": 3, "R3_4": 4, "R5_6": 5}
DECODE_PHASE0, DECODE_PERTURB, DECODE_CRC_RECOVER, DECODE_FULL = 1, 2, 4, 7
DECODE_NO_CHANNEL_DEINTERLEAVE = 0x100
RX_DEMOD_ONLY = 0x200
OPT_SPLIT_PARTS = 1
OPT_DUAL_DECODER = 2
OPT_FALLBACK_QUEUE_ALL = 3
OPT_STATE_EXIT = 4
OPT_SEARCH_CHUNK = 5
ACQ_NO_TIMING_RETRY = 0x400
BURST_MAX_FRAMES = 9
BURST_INTERLEAVE = 0x800
BURST_NO_CONTINUE = 0x1000
BURST_STOP = {"NONE": 0, "ENERGY": 1, "PROCESS": 2, "WINDOW": 3, "DECODE": 4, "NOT_DATA": 5, "LIMIT": 6, "RECOVERED": 7}
MACQ_SYNC_CHIRP = 0x1
MACQ_DISCONNECTED = 0x2
MACQ_NO_RETRY = 0x4
MACQ_CHANNEL_INTERLEAVE = 0x8
# RIA_DFRAME_*: which statement of decodeFrame produced a row's result (ria_dframe_result.path)
DFRAME_PATH = {"NONE": 0, "CONTROL_R14": 1, "CONTROL_CW0": 2, "FIXED": 3, "SALVAGE_R14": 4, "SALVAGE_RATE": 5, "FIXED_FAILED": 6,
               "LEGACY": 7, "PARTIAL": 8, "BAD_HEADER": 9}
DFRAME_MAX_CW = 32
# RIA_WIN_* (ria_window_result.outcome) and RIA_PEEK_* (ria_window_result.peek)
WIN_OUTCOME = {"NOT_ACCEPTED": 0, "BURST": 1, "CONTROL_PROFILE": 2, "DECODED": 3, "NEED_SAMPLES": 4, "TOO_LONG": 5}
WIN_PEEK = {"NONE": 0, "R14_ONE": 1, "R14_MULTI": 2, "RATE_ONE": 3, "RATE_MULTI": 4, "RATE_BAD_HEADER": 5, "FAILED": 6, "QAM_PARTIAL": 7,
            "DIRECT": 8}
# RIA_MWIN_* (ria_mcdpsk_window_result.outcome) and RIA_MPEEK_* (its peek word: MPEEK_WHAT in the low four bits, then MPEEK_BITS)
MWIN_OUTCOME = {"NOT_ACCEPTED": 0, "REPLAY": 1, "PING": 2, "PROCESS_FAILED": 3, "DECODED": 4, "NEED_SAMPLES": 5, "TOO_LONG": 6}
MPEEK_WHAT = {"NONE": 0, "NO_HEADER": 1, "HEADER_SINGLE": 2, "HEADER_MULTI": 3, "CONNECT_FORCED": 4}
MPEEK_WHAT_MASK = 0x0F
MPEEK_BITS = {"HANDSHAKE_FALLBACK": 0x10, "EARLY_WINDOW": 0x20, "HANDSHAKE_WINDOW": 0x40, "DEINTERLEAVED": 0x80, "SALVAGE": 0x100}
MWIN_NO_LAST_SYNC = -2 ** 31
CHASE_MAX_CW, CHASE_MAX_ENTRIES, CHASE_MAX_COMBINES = 16, 16, 4
HARQ_ENTRY = {"NONE": 0, "KEPT": 1, "REMOVED": 2}
# RIA_SEARCH_*: the modes and outcomes of ria_gpu_search_batch
SEARCH_MODE = {"OFDM_LTS": 0, "MCDPSK_ZC": 1, "MCDPSK_CHIRP": 2}
SEARCH_OUTCOME = {"SYNC_FOUND": 1, "NEED_SAMPLES": 2, "LIMIT": 3}
SEARCH_CONNECTED = 0x1
SEARCH_MIN_SEARCH = {0: 67304, 1: 31120, 2: 120000}
SEARCH_MAX_CAPTURE = 959999
SEARCH_NO_LAST_SYNC = -2 ** 31
# ria_gpu_search_ring_batch: the ring buffer's length and the longest capture
RING_SAMPLES = 960000
RING_MAX_CAPTURE = 2 ** 31 - 1 - RING_SAMPLES
# RIA_STREAM_*: why a stream of ria_gpu_rx_stream_batch closed (2 and 3 are the search's outcomes)
STREAM_CLOSED = {"SEARCH_NEED_SAMPLES": 2, "SEARCH_LIMIT": 3, "WINDOW_NEED_SAMPLES": 4, "EVENTS_FULL": 5, "RING_END": 6}
# why a stream of ria_gpu_rx_ring_batch closed: no RING_END, and RIA_STREAM_SPAN_LOST
RING_STREAM_CLOSED = {"SEARCH_NEED_SAMPLES": 2, "SEARCH_LIMIT": 3, "WINDOW_NEED_SAMPLES": 4, "EVENTS_FULL": 5, "SPAN_LOST": 7}

# every symbol include/ria_gpu.h declares
EXPORTS = [
    "ria_gpu_abi_version", "ria_gpu_demod_variant", "ria_gpu_default_config", "ria_gpu_create", "ria_gpu_destroy", "ria_gpu_last_error",
    "ria_gpu_get_geometry", "ria_gpu_set_option", "ria_gpu_demod_batch", "ria_gpu_decode_batch", "ria_gpu_ldpc_decode_batch", "ria_gpu_ldpc_decode_robust_batch",
    "ria_gpu_rx_batch", "ria_gpu_rx_frames_host", "ria_gpu_decode_frames_host", "ria_gpu_tx_batch", "ria_gpu_make_frames",
    "ria_gpu_channel_batch", "ria_gpu_channel_exact_batch", "ria_gpu_channel_exact_seeded_batch", "ria_gpu_debug_math", "ria_gpu_debug_queue_fault", "ria_gpu_debug_recovery_counts", "ria_gpu_debug_state_exits", "ria_gpu_debug_first_decodes", "ria_gpu_sync_zc_batch", "ria_gpu_zc_preamble", "ria_gpu_sync_chirp_batch", "ria_gpu_chirp_preamble", "ria_gpu_mcdpsk_demod_batch",
    "ria_gpu_mcdpsk_modulate_host", "ria_gpu_chase_combine_batch", "ria_gpu_sync_lts_batch", "ria_gpu_sync_host", "ria_gpu_ldpc_encode_host", "ria_gpu_burst_deinterleave_batch", "ria_gpu_burst_interleave_batch",
    "ria_gpu_rx_acquire_batch", "ria_gpu_mcdpsk_acquire_batch", "ria_gpu_rx_burst_batch", "ria_gpu_encode_frames_batch", "ria_gpu_tx_coded_batch",
    "ria_gpu_sync_cox_batch", "ria_gpu_cox_preamble", "ria_gpu_channel_exact_cfo_batch", "ria_gpu_tx_cfo_batch",
    "ria_gpu_mcdpsk_demod_host", "ria_gpu_ldpc_decode_robust_host", "ria_gpu_mcdpsk_modulate_batch",
    "ria_gpu_decode_frame_batch", "ria_gpu_decode_frame_host",
    "ria_gpu_chase_default_config", "ria_gpu_chase_create", "ria_gpu_chase_destroy", "ria_gpu_chase_clear", "ria_gpu_chase_stats", "ria_gpu_chase_export",
    "ria_gpu_mcdpsk_decode_frame_batch", "ria_gpu_mcdpsk_acquire_harq_batch",
    "ria_gpu_mcdpsk_decode_frame_ci_batch", "ria_gpu_mcdpsk_acquire_ci_batch", "ria_gpu_mcdpsk_interleave_batch",
    "ria_gpu_var_frame_samples", "ria_gpu_control_frame_samples", "ria_gpu_tx_coded_var_batch", "ria_gpu_demod_var_batch", "ria_gpu_demod_var_host",
    "ria_gpu_rx_control_batch", "ria_gpu_control_acquire_batch", "ria_gpu_rx_window_batch",
    "ria_gpu_mcdpsk_window_batch", "ria_gpu_mcdpsk_window_host", "ria_gpu_search_batch", "ria_gpu_search_ring_batch",
    "ria_gpu_rx_stream_batch", "ria_gpu_rx_stream_host", "ria_gpu_rx_ring_batch", "ria_gpu_rx_ring_host",
    "ria_gpu_mcdpsk_stream_batch", "ria_gpu_mcdpsk_stream_host",
    "ria_gpu_mcdpsk_ring_batch", "ria_gpu_mcdpsk_ring_host",
    "ria_link_recommend", "ria_link_data_mode", "ria_link_ofdm_code_rate", "ria_link_cap_initial_rate",
]


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "device", "modulation", "code_rate", "fft_size",
                                          "num_carriers", "cyclic_prefix", "sample_rate", "center_freq",
                                          "max_batch")] + [("reserved", C.c_int32 * 6)]


class LinkRecommendation(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("waveform", "modulation", "code_rate", "spreading", "num_carriers")] + \
               [("estimated_throughput_bps", C.c_float)]


class McdpskConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_carriers", "bits_per_symbol", "spreading", "reserved")]


class Geometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pilot_spacing", "n_pilots", "n_data_carriers", "bits_per_carrier",
                                          "bits_per_symbol", "n_data_symbols", "samples_per_symbol",
                                          "frame_samples", "llrs_per_frame", "info_bits", "bytes_per_codeword",
                                          "info_bytes_per_frame", "ldpc_max_iterations", "ldpc_edges", "ldpc_k")] + \
               [("reserved", C.c_int32 * 1)]


class FrameMeta(C.Structure):
    _fields_ = [("cfo_hz", C.c_float), ("flags", C.c_uint32), ("abs_position", C.c_uint64)]


class FrameStatus(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("snr_db", "cfo_hz", "fading_index", "noise_variance", "lts_phase_slope",
                                          "snr_linear", "corr_phase")] + [("n_llr", C.c_int32)]


class DecodeStatus(C.Structure):
    _fields_ = [("cw_ok", C.c_uint8 * 4), ("iterations", C.c_uint16 * 4), ("attempts", C.c_uint8 * 4),
                ("frame_valid", C.c_uint8), ("needs_recovery", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class AcqParams(C.Structure):
    _fields_ = [("known_cfo_hz", C.c_float), ("detect_threshold", C.c_float), ("min_confidence", C.c_float),
                ("reserved0", C.c_uint32), ("abs_base", C.c_uint64), ("reserved", C.c_uint32 * 2)]


class AcqResult(C.Structure):
    _fields_ = [("detected", C.c_int32), ("accepted", C.c_int32), ("sync_start", C.c_int32), ("frame_start", C.c_int32),
                ("correlation", C.c_float), ("cfo_hz", C.c_float), ("delta", C.c_int16), ("candidates", C.c_uint8),
                ("burst_interleaved", C.c_uint8), ("reserved", C.c_int32)]


class BurstResult(C.Structure):
    _fields_ = [("detected", C.c_int32), ("accepted", C.c_int32), ("sync_start", C.c_int32), ("frame_start", C.c_int32),
                ("correlation", C.c_float), ("cfo_hz", C.c_float), ("delta", C.c_int16), ("candidates", C.c_uint8),
                ("burst_interleaved", C.c_uint8), ("mode", C.c_uint8), ("frames", C.c_uint8), ("frames_decoded", C.c_uint8),
                ("stop", C.c_uint8), ("reserved", C.c_int32 * 8)]


class McAcqParams(C.Structure):
    """pending_total_cw, first_avail and last_decoded_sync are read by ria_gpu_mcdpsk_window_batch only"""
    _fields_ = [("known_cfo_hz", C.c_float), ("detect_threshold", C.c_float), ("min_confidence", C.c_float),
                ("pending_total_cw", C.c_uint32), ("abs_base", C.c_uint64), ("first_avail", C.c_uint32), ("last_decoded_sync", C.c_int32)]


class McWindowResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("outcome", "peek", "next_pos", "need_samples", "pending_total_cw", "frame_len", "passes",
                                          "peek_total_cw")] + \
               [("training_rms", C.c_float), ("rms", C.c_float), ("last_decoded_sync", C.c_int32), ("deliver", C.c_uint8),
                ("is_ping", C.c_uint8), ("peek_tries", C.c_uint8), ("reserved0", C.c_uint8), ("reserved", C.c_int32 * 4)]


class McAcqResult(C.Structure):
    _fields_ = [("detected", C.c_int32), ("accepted", C.c_int32), ("sync_start", C.c_int32), ("frame_start", C.c_int32),
                ("correlation", C.c_float), ("cfo_hz", C.c_float), ("fading_index", C.c_float), ("delta", C.c_int16),
                ("modulation", C.c_uint8), ("candidates", C.c_uint8), ("success", C.c_uint8), ("codewords_ok", C.c_uint8),
                ("codewords_failed", C.c_uint8), ("frame_type", C.c_uint8), ("header_total_cw", C.c_int32),
                ("frame_bytes", C.c_int32), ("n_llr", C.c_int32), ("reserved", C.c_int32 * 4)]


class DframeResult(C.Structure):
    _fields_ = [("success", C.c_uint8), ("codewords_ok", C.c_uint8), ("codewords_failed", C.c_uint8), ("frame_type", C.c_uint8),
                ("path", C.c_uint8), ("header_total_cw", C.c_uint8), ("stages", C.c_uint8), ("reserved0", C.c_uint8),
                ("frame_bytes", C.c_int32), ("iters_r14", C.c_uint16), ("iters_cw0", C.c_uint16), ("tries_r14", C.c_uint8),
                ("tries_rate", C.c_uint8), ("reserved1", C.c_uint8 * 2), ("reserved", C.c_int32 * 3)]


class ControlResult(C.Structure):
    _fields_ = [(n, C.c_uint8) for n in ("process_ok", "cw_ok", "magic", "header_valid", "total_cw", "frame_type", "success", "tries")] + \
               [("seq", C.c_uint16), ("iterations", C.c_uint16), ("n_llr", C.c_int32), ("tried", C.c_uint8), ("reserved0", C.c_uint8 * 3),
                ("reserved", C.c_int32 * 3)]


class ChaseConfig(C.Structure):
    _fields_ = [("n_caches", C.c_int32), ("max_entries", C.c_int32), ("ttl_ms", C.c_int64), ("reserved", C.c_int32 * 4)]


class ChaseStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("cache_hits", "cache_misses", "stores", "combines", "entries_evicted", "entries_expired",
                                          "recoveries")]


class ChaseEntry(C.Structure):
    _fields_ = [("last_access_ms", C.c_uint64), ("order", C.c_uint64), ("src_hash", C.c_uint32), ("dst_hash", C.c_uint32),
                ("seq", C.c_uint16), ("used", C.c_uint8), ("total_cw", C.c_uint8), ("frame_type", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("combine_count", C.c_uint8 * 16), ("decoded", C.c_uint8 * 16), ("has_sum", C.c_uint8 * 16)]


class McDframeResult(C.Structure):
    _fields_ = [("success", C.c_uint8), ("codewords_ok", C.c_uint8), ("codewords_failed", C.c_uint8), ("frame_type", C.c_uint8),
                ("header_total_cw", C.c_int32), ("frame_bytes", C.c_int32), ("reserved", C.c_int32)]


class McHarqResult(C.Structure):
    _fields_ = [("seq", C.c_uint16), ("valid", C.c_uint8), ("entry", C.c_uint8), ("src_hash", C.c_uint32), ("dst_hash", C.c_uint32),
                ("stored_mask", C.c_uint16), ("sum_mask", C.c_uint16), ("recovered_mask", C.c_uint16), ("max_combine", C.c_uint8),
                ("reserved0", C.c_uint8), ("cache_id", C.c_int32), ("reserved", C.c_int32 * 2)]


class WindowResult(C.Structure):
    _fields_ = [("frame", DframeResult)] + \
               [(n, C.c_uint8) for n in ("outcome", "peek", "pending_total_cw", "small_frame", "tries_peek_r14", "tries_peek_rate",
                                         "tries_small_r14", "tries_small_rate")] + \
               [("frame_len", C.c_int32), ("next_pos", C.c_int32), ("need_samples", C.c_int32), ("sync_cfo_hz", C.c_float),
                ("peek_cfo_hz", C.c_float), ("fading_index", C.c_float)]


class SearchState(C.Structure):
    _fields_ = [("correlation_pos", C.c_int32), ("fed", C.c_int32), ("noise_floor", C.c_float), ("reject_streak", C.c_int32),
                ("last_cfo_hz", C.c_float), ("fading_hint", C.c_float), ("snr_hint", C.c_float), ("last_decoded_sync_pos", C.c_int32)]


class SearchResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("outcome", "search_start", "search_len", "sync_position")] + [("abs_position", C.c_int64)] + \
               [(n, C.c_float) for n in ("correlation", "known_cfo_hz", "sync_cfo_hz", "sync_snr_db", "detect_threshold", "min_confidence")] + \
               [(n, C.c_int32) for n in ("weak_accept", "marker", "root")] + \
               [(n, C.c_uint32) for n in ("invocations", "waits", "rms_skips", "detector_runs", "rejects", "near_misses", "weak_accepts",
                                          "replays", "catchups_moderate", "catchups_severe", "reserved0", "reserved1", "reserved2")]


class RingState(C.Structure):
    _fields_ = [("total_fed", C.c_int64), ("correlation_pos", C.c_int32), ("reject_streak", C.c_int32), ("noise_floor", C.c_float),
                ("last_cfo_hz", C.c_float), ("fading_hint", C.c_float), ("snr_hint", C.c_float), ("last_decoded_sync_pos", C.c_int32),
                ("overflow_events", C.c_uint32), ("overflow_dropped", C.c_uint64)]


class RingSearchResult(C.Structure):
    _fields_ = SearchResult._fields_ + [("abs_search_start", C.c_int64), ("overflow_dropped", C.c_uint64)] + \
               [(n, C.c_uint32) for n in ("overflows", "drift_snaps", "cursor_inits", "span_wraps")]


class StreamEvent(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sync_position", "search_start", "window_len", "outcome", "next_pos", "frame_bytes", "need_samples",
                                          "pending_total_cw")] + \
               [(n, C.c_uint8) for n in ("delivered", "success", "codewords_ok", "codewords_failed", "frame_type")] + [("reserved0", C.c_uint8 * 3)] + \
               [(n, C.c_float) for n in ("correlation", "cfo_hz", "fading_index", "snr_db")] + [("reserved", C.c_int32 * 2)]


class StreamResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_events", "closed", "mode", "search_legs")] + \
               [(n, C.c_uint32) for n in ("invocations", "waits", "rms_skips", "detector_runs", "rejects", "near_misses", "weak_accepts", "replays",
                                          "catchups_moderate", "catchups_severe")] + [("reserved", C.c_uint32 * 2)]


class McStreamState(C.Structure):
    _fields_ = [("search", SearchState)] + \
               [(n, C.c_int32) for n in ("pending_total_cw", "need_samples", "pend_search_start", "pend_sync_position")] + \
               [(n, C.c_float) for n in ("pend_known_cfo_hz", "pend_detect_threshold", "pend_min_confidence", "pend_correlation")]


class McRingState(C.Structure):          # ria_mcdpsk_ring_state, 80 bytes: the pending positions are capture (absolute) indices
    _fields_ = [("ring", RingState)] + McStreamState._fields_[1:]


class RingStreamResult(C.Structure):
    _fields_ = StreamResult._fields_ + [("overflow_dropped", C.c_uint64)] + \
               [(n, C.c_uint32) for n in ("overflows", "drift_snaps", "cursor_inits", "reserved1")]


def macq_frame_bytes(frame_cw):
    """RIA_MACQ_FRAME_BYTES: bytes of one frame_out row of ria_gpu_mcdpsk_acquire_batch"""
    return 40 * int(frame_cw)


_lib = None


def library_path():
    return _build.LIB


def load(build_if_needed=True):
    """Loads libria_gpu.so; raises (never falls back) if it cannot be built or loaded."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (soname libamdhip64.so.7).  Import it first so that this
    # process holds ONE runtime: libria_gpu.so's DT_NEEDED then resolves to the copy torch loaded,
    # and device pointers / streams from torch are valid inside the library.
    import torch  # noqa: F401
    path = _build.build() if build_if_needed else _build.LIB
    path = os.environ.get("RIA_GPU_LIB", path)   # developer A/B switch: an alternative build of the same sources
    if not os.path.exists(path):
        raise RuntimeError("libria_gpu.so is missing: run `python -m ria_amd.build`")
    L = C.CDLL(path)
    vp, i32, u32, u64, f32 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float
    L.ria_gpu_abi_version.restype = i32
    L.ria_gpu_default_config.argtypes = [C.POINTER(Config)]
    L.ria_gpu_default_config.restype = None
    L.ria_gpu_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.ria_gpu_destroy.argtypes = [vp]
    L.ria_gpu_destroy.restype = None
    L.ria_gpu_last_error.argtypes = [vp]
    L.ria_gpu_last_error.restype = C.c_char_p
    L.ria_gpu_get_geometry.argtypes = [vp, C.POINTER(Geometry)]
    L.ria_gpu_set_option.argtypes = [vp, i32, i32]
    L.ria_gpu_demod_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.ria_gpu_decode_batch.argtypes = [vp, vp, i32, i32, u32, vp, vp, vp]
    L.ria_gpu_ldpc_decode_batch.argtypes = [vp, vp, i32, i32, f32, vp, vp, vp, vp]
    L.ria_gpu_ldpc_decode_robust_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.ria_gpu_rx_batch.argtypes = [vp, vp, vp, vp, i32, u32, vp, vp, vp, vp, vp]
    L.ria_gpu_rx_frames_host.argtypes = [vp, vp, vp, i32, u32, vp, vp, vp, vp]
    L.ria_gpu_decode_frames_host.argtypes = [vp, vp, i32, i32, u32, vp, vp]
    L.ria_gpu_tx_batch.argtypes = [vp, vp, i32, f32, vp, vp]
    L.ria_gpu_encode_frames_batch.argtypes = [vp, vp, i32, vp, vp]
    L.ria_gpu_tx_coded_batch.argtypes = [vp, vp, i32, f32, vp, vp]
    L.ria_gpu_make_frames.argtypes = [vp, u64, i32, i32, vp, vp]
    L.ria_gpu_channel_batch.argtypes = [vp, i32, f32, u64, u64, vp, i32, vp]
    L.ria_gpu_debug_math.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    L.ria_gpu_debug_queue_fault.argtypes = [vp]
    L.ria_gpu_debug_recovery_counts.argtypes = [vp, i32, vp]
    L.ria_gpu_debug_state_exits.argtypes = [vp, i32, vp]
    L.ria_gpu_debug_first_decodes.argtypes = [vp, i32, vp]
    L.ria_gpu_channel_exact_batch.argtypes = [vp, i32, f32, u32, u64, vp, C.c_int64, i32, i32, vp]
    L.ria_gpu_channel_exact_seeded_batch.argtypes = [vp, i32, f32, vp, vp, C.c_int64, i32, i32, vp]
    L.ria_gpu_channel_exact_cfo_batch.argtypes = [vp, i32, f32, vp, vp, f32, vp, vp, C.c_int64, i32, i32, vp]
    L.ria_gpu_mcdpsk_modulate_batch.argtypes = [vp, vp, vp, i32, i32, vp, C.c_int64, vp]
    L.ria_gpu_mcdpsk_demod_host.argtypes = [vp, vp, vp, i32, f32, f32, vp, i32, vp]
    L.ria_gpu_ldpc_decode_robust_host.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.ria_gpu_tx_cfo_batch.argtypes = [vp, vp, C.c_int64, i32, i32, vp, vp, vp, C.c_int64, vp]
    L.ria_gpu_sync_zc_batch.argtypes = [vp, vp, C.c_int64, i32, i32, f32, u32, vp, vp, vp]
    L.ria_gpu_zc_preamble.argtypes = [vp, i32, vp, i32]
    L.ria_gpu_sync_chirp_batch.argtypes = [vp, vp, C.c_int64, i32, i32, f32, vp, vp]
    L.ria_gpu_chirp_preamble.argtypes = [vp, vp, i32]
    L.ria_gpu_mcdpsk_demod_batch.argtypes = [vp, vp, vp, C.c_int64, i32, i32, vp, vp, vp, i32, vp, vp]
    L.ria_gpu_mcdpsk_modulate_host.argtypes = [vp, vp, vp, i32, vp, i32]
    L.ria_gpu_chase_combine_batch.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    L.ria_gpu_sync_lts_batch.argtypes = [vp, vp, C.c_int64, i32, i32, vp, f32, vp, vp]
    L.ria_gpu_sync_cox_batch.argtypes = [vp, vp, C.c_int64, i32, i32, f32, vp, vp, vp]
    L.ria_gpu_cox_preamble.argtypes = [vp, vp, i32]
    L.ria_gpu_sync_host.argtypes = [vp, i32, vp, i32, f32, f32, u32, vp]
    L.ria_gpu_ldpc_encode_host.argtypes = [vp, vp, i32, vp]
    L.ria_gpu_burst_deinterleave_batch.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.ria_gpu_burst_interleave_batch.argtypes = [vp, vp, i32, i32, vp, vp]
    L.ria_gpu_rx_acquire_batch.argtypes = [vp, vp, C.c_int64, i32, i32, i32, vp, u32, vp, vp, vp, vp, vp]
    L.ria_gpu_rx_burst_batch.argtypes = [vp, vp, C.c_int64, i32, i32, i32, i32, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.ria_gpu_mcdpsk_acquire_batch.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, vp, u32, vp, vp, vp, i32, vp]
    L.ria_gpu_decode_frame_batch.argtypes = [vp, vp, i32, vp, i32, u32, vp, i32, vp, vp, vp, vp]
    L.ria_gpu_decode_frame_host.argtypes = [vp, vp, i32, u32, vp, i32, vp, vp]
    L.ria_gpu_chase_default_config.argtypes = [C.POINTER(ChaseConfig)]
    L.ria_gpu_chase_default_config.restype = None
    L.ria_gpu_chase_create.argtypes = [vp, C.POINTER(ChaseConfig), C.POINTER(vp)]
    L.ria_gpu_chase_destroy.argtypes = [vp]
    L.ria_gpu_chase_destroy.restype = None
    L.ria_gpu_chase_clear.argtypes = [vp, vp, i32, vp]
    L.ria_gpu_chase_stats.argtypes = [vp, i32, C.POINTER(ChaseStats)]
    L.ria_gpu_chase_export.argtypes = [vp, i32, vp, vp]
    L.ria_gpu_mcdpsk_decode_frame_batch.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]
    L.ria_gpu_mcdpsk_acquire_harq_batch.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, vp, u32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.ria_gpu_mcdpsk_decode_frame_ci_batch.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, u32, i32, vp]
    L.ria_gpu_mcdpsk_acquire_ci_batch.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, i32, vp, u32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.ria_gpu_mcdpsk_interleave_batch.argtypes = [vp, i32, vp, i32, vp, vp]
    L.ria_gpu_var_frame_samples.argtypes = [vp, i32]
    L.ria_gpu_control_frame_samples.argtypes = [vp, vp]
    L.ria_gpu_tx_coded_var_batch.argtypes = [vp, vp, i32, i32, f32, vp, C.c_int64, vp]
    L.ria_gpu_demod_var_batch.argtypes = [vp, vp, vp, vp, i32, i32, vp, i32, vp, vp]
    L.ria_gpu_demod_var_host.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.ria_gpu_rx_control_batch.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.ria_gpu_control_acquire_batch.argtypes = [vp, vp, C.c_int64, i32, i32, i32, i32, vp, u32, vp, vp, vp, vp, vp]
    L.ria_gpu_rx_window_batch.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, vp, u32, vp, i32, vp, vp, vp, vp, vp]
    L.ria_gpu_mcdpsk_window_batch.argtypes = [vp, vp, vp, C.c_int64, i32, i32, i32, vp, u32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.ria_gpu_mcdpsk_window_host.argtypes = [vp, vp, vp, i32, i32, vp, u32, vp, i32, vp, vp, i32]
    L.ria_gpu_search_batch.argtypes = [vp, i32, u32, vp, vp, C.c_int64, vp, i32, vp, i32, i32, vp, vp]
    L.ria_gpu_search_ring_batch.argtypes = [vp, i32, u32, vp, vp, C.c_int64, vp, i32, vp, i32, i32, vp, vp]
    L.ria_gpu_rx_stream_batch.argtypes = [vp, vp, i32, u32, vp, vp, C.c_int64, vp, i32, vp, i32, i32, i32, vp, vp, i32, vp, vp]
    L.ria_gpu_rx_stream_host.argtypes = [vp, vp, i32, u32, vp, vp, i32, vp, i32, i32, i32, vp, vp, i32, vp]
    L.ria_gpu_rx_ring_batch.argtypes = [vp, vp, i32, u32, vp, vp, C.c_int64, vp, i32, vp, i32, i32, i32, vp, vp, i32, vp, vp]
    L.ria_gpu_rx_ring_host.argtypes = [vp, vp, i32, u32, vp, vp, i32, vp, i32, i32, i32, vp, vp, i32, vp]
    L.ria_gpu_mcdpsk_stream_batch.argtypes = [vp, i32, u32, u32, i32, vp, vp, C.c_int64, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.ria_gpu_mcdpsk_stream_host.argtypes = [vp, i32, u32, u32, i32, vp, vp, i32, vp, i32, i32, i32, vp, C.c_int32, u64, vp, vp, i32, vp, vp]
    # ria_mcdpsk_ring_state is 80 bytes: ria_ring_state's 48, then the eight pending fields (RxEngine.MCRING_STATE)
    L.ria_gpu_mcdpsk_ring_batch.argtypes = [vp, i32, u32, u32, i32, vp, vp, C.c_int64, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.ria_gpu_mcdpsk_ring_host.argtypes = [vp, i32, u32, u32, i32, vp, vp, i32, vp, i32, i32, i32, vp, C.c_int32, u64, vp, vp, i32, vp, vp]
    L.ria_link_recommend.argtypes = [f32, f32, C.POINTER(LinkRecommendation)]
    L.ria_link_recommend.restype = None
    L.ria_link_data_mode.argtypes = [f32, i32, f32, C.POINTER(LinkRecommendation)]
    L.ria_link_data_mode.restype = None
    L.ria_link_ofdm_code_rate.argtypes = [f32, f32]
    L.ria_link_cap_initial_rate.argtypes = [f32, f32, i32]
    for name in EXPORTS:
        if name not in ("ria_gpu_chase_default_config", "ria_gpu_chase_destroy", "ria_gpu_default_config", "ria_gpu_destroy", "ria_gpu_last_error", "ria_link_recommend", "ria_link_data_mode"):
            getattr(L, name).restype = i32
    _lib = L
    return L


class RiaError(RuntimeError):
    pass
