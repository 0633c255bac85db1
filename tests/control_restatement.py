"""CPU restatement of the variable-length frame calls and of the control hypothesis (ria_gpu_tx_coded_var_batch,
ria_gpu_demod_var_batch, ria_gpu_rx_control_batch, ria_gpu_control_acquire_batch) on the checkers (pyoracle.Oracle, or
pyoracle.Ref where it is built): what gui::StreamingDecoder does with a connected-mode OFDM window before it tries the data
profile, written out step by step (src/gui/modem/streaming_decoder.cpp):

1. getOFDMControlFrameSamples (:42-69) gives the span; getMinSamplesForCWCount (ofdm_chirp_waveform.cpp:616-648) a frame's size
2. configure(DQPSK, R1_4) keeps position, CFO and the one-shot marker (ofdm_chirp_waveform.cpp:81-107, :421-440); process()
   on the span with them (:1284)
3. at least 648 soft bits: robustDecodeSingleCW of the first 648 at R1/4 (:1290, :1028-1058)
4. ok, at least 4 bytes, magic 55 4C, truncation to 20 bytes, parseHeader valid, total_cw == 1, isControlFrame (:1294-1299)
5. from a window: detectDataSync and the acceptance rule of the data path first (acquire_restatement.py); a marked window
   under use_burst_interleave_ is accumulated as a burst group and never peeked (:1087-1092)
6. control first, then the data path for the windows the hypothesis did not take (rx_acquire_control_first)

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
from acquire_restatement import acquire_window, po_oracle
from mcdpsk_acquire_restatement import CONTROL_TYPES, control_frame, crc16, data_frame   # noqa: F401

SYM = 1152
ACK, NACK, DATA = 0x20, 0x21, 0x30
STATUS_WORDS = ("snr_db", "cfo_hz", "fading_index", "noise_variance", "lts_phase_slope", "snr_linear", "corr_phase")
RESULT_FIELDS = ("process_ok", "cw_ok", "magic", "header_valid", "total_cw", "frame_type", "success", "tries", "seq", "iterations",
                 "n_llr", "tried")


# ---- geometry
def bits_per_symbol(mod, rate):
    return po_oracle(None).geom(mod, rate).bits_per_symbol


def var_frame_samples(mod, rate, coded_bytes):
    """getMinSamplesForCWCount's formula for any byte count"""
    bps = bits_per_symbol(mod, rate)
    return (2 + -(-8 * coded_bytes // bps)) * SYM


def control_frame_samples(data_mod, data_rate, carriers=59):
    """getOFDMControlFrameSamples (streaming_decoder.cpp:42-69)"""
    own = var_frame_samples(data_mod, data_rate, 81)
    if (data_mod, data_rate) == (po.DQPSK, po.R1_4):
        return own
    data_carriers = max(1, carriers - -(-carriers // 10))
    return max(own, (2 + -(-648 // (2 * data_carriers))) * SYM)


# ---- frames
def encode_control(frame20):
    """one R1/4 codeword: 20 bytes padded to the code's 21 information bytes -> 81 coded bytes"""
    return po_oracle(None).ldpc_encode(po.R1_4, np.concatenate([np.asarray(frame20, np.uint8), np.zeros(1, np.uint8)]))


def tx_var(checker, mod, rate, coded, peak=0.8):
    """generateDataPreamble() ++ modulate(coded), peak-normalised by ria_gpu_tx_batch's rule"""
    s = checker.modulate(mod, rate, coded)
    if peak > 0:
        s = (s * (np.float32(peak) / np.abs(s).max())).astype(np.float32)
    return s


# ---- process() on a span
def process_span(checker, mod, rate, span, cfo_hz=0.0, abs_pos=0, marker=False):
    """-> (soft bits, status words dict, n_llr as ria_frame_status reports it)"""
    span = np.ascontiguousarray(span, np.float32)
    if isinstance(checker, po.Ref):
        if marker:      # the waveform negates the first LTS symbol on a copy before the demodulator sees it (:421-440)
            span = span.copy()
            span[:SYM] = -span[:SYM]
        llr, aux, _, _ = checker.rx_process(mod, rate, span, float(cfo_hz), int(abs_pos))
        st = {k: np.float32(aux[i]) for i, k in enumerate(STATUS_WORDS)}
    else:
        llr, aux = checker.rx_process(mod, rate, span, float(cfo_hz), int(abs_pos), burst_marker=bool(marker))
        st = {k: np.float32(getattr(aux, k)) for k in STATUS_WORDS}
    return llr, st, (len(llr) if len(llr) >= 648 else 0)


def zero_result():
    r = {k: 0 for k in RESULT_FIELDS}
    r["frame"] = np.zeros(20, np.uint8)
    r["status"] = None
    return r


def control_hypothesis(checker, span, cfo_hz=0.0, abs_pos=0, marker=False):
    """:1284-1338 on one pre-synced span -> dict of the ria_control_result fields, `frame` (20 bytes) and `status`"""
    llr, st, n_llr = process_span(checker, po.DQPSK, po.R1_4, span, cfo_hz, abs_pos, marker)
    r = zero_result()
    r.update(tried=1, n_llr=n_llr, status=st, process_ok=int(n_llr >= 648))
    if not r["process_ok"]:
        return r
    ok, data, it, tries = checker.robust_decode(po.R1_4, llr[:648])
    r.update(cw_ok=int(ok), iterations=int(it), tries=int(tries))
    if not (ok and len(data) >= 4 and data[0] == 0x55 and data[1] == 0x4C):
        return r
    d = np.asarray(data[:20], np.uint8)                       # data_r14.resize(bpc_r14)
    r.update(magic=1, frame_type=int(d[2]))
    is_ctl = int(d[2]) in CONTROL_TYPES
    if len(d) < 20:
        return r
    if is_ctl:                                                 # parseHeader, frame_v2.cpp:1195-1252
        valid, total = crc16(d[:18]) == ((int(d[18]) << 8) | int(d[19])), 1
    else:
        valid, total = crc16(d[:15]) == ((int(d[15]) << 8) | int(d[16])), int(d[12])
    if not valid:
        return r
    r.update(header_valid=1, total_cw=total, seq=(int(d[4]) << 8) | int(d[5]))
    if total == 1 and is_ctl:
        r.update(success=1, frame=d.copy())
    return r


def control_acquire_window(checker, data_mod, data_rate, x, search_len, n_samples, known_cfo=0.0, detect_threshold=0.15,
                           min_confidence=0.78, abs_base=0, interleave=False):
    """One window -> (control result dict, acq dict with the ria_acq_result fields)"""
    x = np.ascontiguousarray(x, np.float32)
    if isinstance(checker, po.Ref):
        det = checker.detect_data_sync(x[:search_len], known_cfo, detect_threshold, data_mod, data_rate)
    else:
        det = checker.detect_data_sync(x[:search_len], known_cfo, detect_threshold)
    detected, corr, burst = bool(det[0]), np.float32(det[2]), int(det[3]) if det[0] else 0
    start = int(det[1]) if detected else -1
    accepted = detected and not (corr < np.float32(min_confidence)) and start >= 0 and start + n_samples <= len(x)
    tried = accepted and not (interleave and burst)
    acq = dict(detected=int(detected), accepted=int(accepted), sync_start=start, frame_start=start if accepted else -1,
               correlation=corr, cfo_hz=np.float32(0.0), delta=0, candidates=int(tried), burst_interleaved=burst)
    if not tried:
        return zero_result(), acq
    r = control_hypothesis(checker, x[start:start + n_samples], known_cfo, abs_base + start, bool(burst))
    acq["cfo_hz"] = r["status"]["cfo_hz"]
    return r, acq


def rx_acquire_control_first(checker, data_mod, data_rate, x, search_len, n_samples, **kw):
    """The control hypothesis, then the data path (acquire_restatement.acquire_window) unless it succeeded
    -> (control result, control acq, data result or None)"""
    r, acq = control_acquire_window(checker, data_mod, data_rate, x, search_len, n_samples, **kw)
    if r["success"]:
        return r, acq, None
    return r, acq, acquire_window(checker, data_mod, data_rate, x, search_len, kw.get("known_cfo", 0.0), kw.get("detect_threshold", 0.15),
                                  kw.get("min_confidence", 0.78), kw.get("abs_base", 0))
