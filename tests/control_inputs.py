"""The pinned inputs of the variable-length frame and control-hypothesis tests (test_control_cpu.py, test_gpu_var_frames.py,
test_gpu_control.py): every input is a function of small integers - frame kind, seq, channel kind, SNR, seed, lead, span -
so nothing large is committed.

Span kinds (frames built with the oracle's encoders, sent with the checker's modulator at DQPSK R1/4, peak 0.8):
    ack / nack  a 20-byte ACK / NACK control frame, one R1/4 codeword (81 coded bytes, 9 symbols, 10 368 samples)
    data1       a one-codeword frame with a valid DATA header (17 + 1 + 2 bytes): header valid, total_cw 1, not a control type
    badcrc      an ACK whose CRC bytes are inverted before encoding: the codeword decodes, the magic holds, parseHeader fails
    fixed       the head of a fixed 4-codeword DQPSK R1/4 data frame (frame + channel interleaved: CW0 is no header)
    noise       the channel's noise alone
    silence     zeros (no channel)

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
import control_restatement as R

CTRL = (po.DQPSK, po.R1_4)
CTRL_SAMPLES = 9 * R.SYM
AWGN, MODERATE = 0, 2
# (channel kind, snr_db, seed) at which the ACK of that row converges on the robust decoder's n-th factor (0: on none of the five)
TRIES = {2: (MODERATE, 0.0, 329), 3: (MODERATE, 0.0, 114), 4: (MODERATE, 0.0, 685), 5: (MODERATE, 1.0, 87884), 0: (MODERATE, 0.0, 112)}

# (name, kind, seq, channel kind, snr_db, seed, span samples, cfo_hz, abs_position, marker)
SPANS = [
    ("ack_awgn20", "ack", 1, AWGN, 20.0, 11, CTRL_SAMPLES, 0.0, 0, 0),
    ("nack_awgn20", "nack", 2, AWGN, 20.0, 12, CTRL_SAMPLES, 0.0, 0, 0),
    ("ack_mod10", "ack", 3, MODERATE, 10.0, 13, CTRL_SAMPLES, 0.0, 0, 0),
    ("nack_mod10", "nack", 4, MODERATE, 10.0, 14, CTRL_SAMPLES, 0.0, 0, 0),
    ("ack_cfo_marker", "ack", 5, AWGN, 20.0, 15, CTRL_SAMPLES, 1.5, 480123, 1),
    ("ack_long_span", "ack", 6, AWGN, 20.0, 16, 15 * R.SYM, -1.5, 77, 0),
    # rows whose robust decode needs 2, 3, 4 and 5 tries, and one that fails all five (seeds found by tools/record_control_golden.py --search)
    ("ack_tries2", "ack", 7, *TRIES[2], CTRL_SAMPLES, 0.0, 0, 0),
    ("ack_tries3", "ack", 8, *TRIES[3], CTRL_SAMPLES, 0.0, 0, 0),
    ("ack_tries4", "ack", 9, *TRIES[4], CTRL_SAMPLES, 0.0, 0, 0),
    ("ack_tries5", "ack", 10, *TRIES[5], CTRL_SAMPLES, 0.0, 0, 0),
    ("ack_lost", "ack", 11, *TRIES[0], CTRL_SAMPLES, 0.0, 0, 0),
    ("fixed_head", "fixed", 12, AWGN, 20.0, 17, CTRL_SAMPLES, 0.0, 0, 0),
    ("data1", "data1", 13, AWGN, 20.0, 18, CTRL_SAMPLES, 0.0, 0, 0),
    ("badcrc", "badcrc", 14, AWGN, 20.0, 19, CTRL_SAMPLES, 0.0, 0, 0),
    ("noise", "noise", 0, AWGN, 20.0, 20, CTRL_SAMPLES, 0.0, 0, 0),
    ("silence", "silence", 0, AWGN, 20.0, 21, CTRL_SAMPLES, 0.0, 0, 0),
    ("ack_short", "ack", 15, AWGN, 20.0, 22, 8 * R.SYM, 0.0, 0, 0),          # 6 data symbols: 636 soft bits, process() false
    ("ack_odd_span", "ack", 16, AWGN, 20.0, 23, CTRL_SAMPLES + 700, 0.0, 0, 0),
]


def frame_bytes(kind, seq):
    if kind == "ack":
        return R.control_frame(R.ACK, seq)
    if kind == "nack":
        return R.control_frame(R.NACK, seq)
    if kind == "data1":
        return R.data_frame(R.DATA, seq, np.array([seq & 255], np.uint8), total_cw=1)
    if kind == "badcrc":
        d = R.control_frame(R.ACK, seq)
        d[18:20] ^= 0xFF
        return d
    raise ValueError(kind)


def clean_samples(checker, kind, seq):
    """the transmitted frame (None: nothing is sent)"""
    if kind in ("noise", "silence"):
        return None
    if kind == "fixed":
        s = checker.tx_frame(po.DQPSK, po.R1_4, (np.arange(60) * 3 + seq).astype(np.uint8) % 251, seq)[0]
        return (s * (np.float32(0.8) / np.abs(s).max())).astype(np.float32)
    return R.tx_var(checker, *CTRL, R.encode_control(frame_bytes(kind, seq)))


def span(checker, row):
    """the received span of a SPANS row: the frame at sample 0 of `n` samples (cut or zero padded), then the channel"""
    _, kind, seq, ch, snr, seed, n = row[:7]
    x = np.zeros(n, np.float32)
    s = clean_samples(checker, kind, seq)
    if s is not None:
        m = min(n, len(s))
        x[:m] = s[:m]
    if kind == "silence":
        return x
    return checker.channel(ch, snr, int(seed), x)


# (name, frame kind (None: noise only), seq, lead, window_len, channel kind, snr_db, seed, min_confidence offset, marked)
#   min_confidence offset: None = 0.5; else the window's own correlation plus this (just above / just below it)
WINDOW_LEN, SEARCH_LEN = 21000, 12000
WINDOWS = [
    ("ack_w", "ack", 21, 300, WINDOW_LEN, AWGN, 20.0, 31, None, 0),
    ("nack_w_mod", "nack", 22, 1234, WINDOW_LEN, MODERATE, 10.0, 32, None, 0),
    # the detector places both frames at sample 1860 (the coarse grid and the cyclic prefix put it ahead of the lead)
    ("ack_fits", "ack", 23, 2000, 1860 + CTRL_SAMPLES, AWGN, 25.0, 33, None, 0),              # the span ends on the window's last sample
    ("ack_fits_not", "ack", 24, 2000, 1860 + CTRL_SAMPLES - 1, AWGN, 25.0, 33, None, 0),      # one sample short
    ("ack_conf_below", "ack", 25, 500, WINDOW_LEN, AWGN, 20.0, 35, -1e-4, 0),
    ("ack_conf_above", "ack", 26, 500, WINDOW_LEN, AWGN, 20.0, 35, +1e-4, 0),
    ("ack_marked", "ack", 27, 700, WINDOW_LEN, AWGN, 20.0, 37, None, 1),
    ("data1_w", "data1", 28, 900, WINDOW_LEN, AWGN, 20.0, 38, None, 0),
    ("noise_w", None, 0, 0, WINDOW_LEN, AWGN, 20.0, 39, None, 0),
]


def window(checker, row):
    """the window of a WINDOWS row: the frame at `lead` of WINDOW_LEN zeros, the channel over all of it, then cut to the row's
    window_len (what lies behind the cut does not change what lies before it)"""
    _, kind, seq, lead, wlen, ch, snr, seed, _, marked = row
    w = np.zeros(max(wlen, WINDOW_LEN), np.float32)
    if kind is not None:
        s = clean_samples(checker, kind, seq).copy()
        if marked:
            s[:R.SYM] = -s[:R.SYM]
        m = min(len(s), len(w) - lead)
        w[lead:lead + m] = s[:m]
    return np.ascontiguousarray(checker.channel(ch, snr, int(seed), w)[:wlen])
