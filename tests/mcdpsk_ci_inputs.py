"""Row and window recipes shared by tests/test_mcdpsk_ci_cpu.py (which asserts, on the restatement, what every recipe does)
and tests/test_gpu_mcdpsk_ci.py (which runs them on the device).  Test infrastructure only (not collected)."""
import numpy as np

import pyoracle as po
from mcdpsk_acquire_restatement import ACK, CONNECT, control_frame, data_frame, encode_frame, frame_len
from mcdpsk_ci_restatement import interleave_bytes

GOOD, WEAK2, WEAK3, DEAD = 2.0, 0.6, 0.42, 0.12   # the amplitudes of tests/test_gpu_mcdpsk_harq.py


def data3(seq):
    """the 3-codeword data frame of sequence number seq"""
    return data_frame(0x30, seq, np.arange(25, dtype=np.uint8))


def data1(seq):
    """a data frame of one codeword: 17 header bytes, 1 payload byte, 2 CRC bytes"""
    return data_frame(0x30, seq, np.array([0xA7], np.uint8))


def coded_cws(frame, il):
    """coded bytes of frame, codeword c interleaved with ChannelInterleaver(il[c], 648) where il[c] is not None; il may be
    one value for every codeword"""
    coded = encode_frame(frame).reshape(-1, 81)
    if not isinstance(il, (tuple, list)):
        il = [il] * len(coded)
    return np.concatenate([cw if b is None else interleave_bytes(cw, b) for cw, b in zip(coded, il)])


def row(frame, amps, seed, il=None, stride=3 * 648):
    """soft bits: codeword c of frame at amplitude amps[c], interleaved per il, plus seeded unit Gaussian noise; noise alone
    behind the frame.  frame None: noise only"""
    x = np.random.default_rng(seed).standard_normal(max(stride, 16 * 648))
    if frame is not None:
        bits = np.unpackbits(coded_cws(frame, il)).astype(np.float64)
        x[:len(bits)] += np.repeat(np.asarray(amps, np.float64)[:len(bits) // 648], 648) * (1.0 - 2.0 * bits)
    return x[:stride].astype(np.float32)


def decode_rows(B):
    """The twelve rows of the decode-frame test for interleaver width B -> (rows, n_llr, cache ids, what each must do)"""
    other = 20 if B == 10 else 10
    G3 = (GOOD, GOOD, GOOD)
    ack = control_frame(ACK, 40)
    rows = [row(data3(5), G3, 11, B), row(ack, (GOOD,), 12), row(data3(6), G3, 13), row(data3(7), G3, 14, (B, None, B)),
            row(data3(8), G3, 15, (None, B, B)), row(None, (), 16), row(data3(9), G3, 17, B), row(data3(10), G3, 18, B),
            row(data3(11), G3, 19, other), row(data1(12), (GOOD,), 20, B), None, None]
    rows[10], rows[11] = rows[0], rows[1]
    n_llr = [1944, 1944, 1944, 1944, 1944, 1944, 1296, 500, 1944, 1944, 1944, 1944]
    ids = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1, -1]
    # (success, codewords_ok, codewords_failed, header_total_cw, frame bytes, cw0_deinterleaved, ci_tried)
    want = [(1, 3, 0, 3, 44, 1, 1), (1, 1, 0, 1, 20, 0, 0), (1, 3, 0, 3, 44, 0, 0), (0, 2, 1, 3, 0, 1, 1), (0, 1, 2, 3, 0, 0, 0),
            (0, 0, 0, 0, 0, 0, 1), (0, 1, 0, 3, 20, 1, 1), (0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 1), (1, 1, 0, 1, 20, 1, 1),
            (1, 3, 0, 3, 44, 1, 1), (1, 1, 0, 1, 20, 0, 0)]
    return rows, n_llr, ids, want


def outcome(r):
    return (r["success"], r["codewords_ok"], r["codewords_failed"], r["header_total_cw"], len(r["frame"]), r["cw0_deinterleaved"], r["ci_tried"])


def chase_calls(B):
    """Four receptions of four links into caches 0..3 -> list of (rows, ids): link 0 is interleaved with CW1 at WEAK2 twice,
    link 1 interleaved with CW2 at WEAK3 three times, link 2 the ordering trap, interleaved, link 3 interleaved in reception
    1 and plain afterwards with CW1 dead in the first two"""
    trap = [(GOOD, GOOD, DEAD), (GOOD, DEAD, GOOD), (GOOD, DEAD, DEAD), (GOOD, GOOD, GOOD)]
    calls = []
    for t in range(4):
        rows = [row(data3(5), (GOOD, WEAK2 if t < 2 else GOOD, GOOD), 100 + 50 * t, B),
                row(data3(6), (GOOD, GOOD, WEAK3 if t < 3 else GOOD), 223 + 50 * t, B),
                row(data3(8), trap[t], 400 + t, B),
                row(data3(9), (GOOD, DEAD if t < 2 else GOOD, GOOD), 500 + t, B if t == 0 else None)]
        calls.append((rows, [0, 1, 2, 3]))
    return calls


def boundary_rows(B):
    """1030 rows of one codeword tiled from 8 distinct ones in a seeded order -> (the 8 rows, index of every row)"""
    other = 20 if B == 10 else 10
    ack = control_frame(ACK, 41)
    base = [row(ack, (GOOD,), 31, stride=648), row(data1(13), (GOOD,), 32, B, stride=648), row(None, (), 33, stride=648),
            row(data1(14), (GOOD,), 34, other, stride=648), row(ack, (GOOD,), 35, stride=648), row(data1(15), (GOOD,), 36, B, stride=648),
            row(None, (), 37, stride=648), row(data3(16), (GOOD,) * 3, 38, B, stride=648)]
    order = np.random.default_rng(1030).integers(0, 8, 1030)
    order[:8] = np.arange(8)
    order[1022:1030] = np.arange(8)[::-1]            # every kind on both sides of the 1024-thread scan tile's end
    return base, order


BOUNDARY_WANT = [(1, 1, 0, 1, 20, 0, 0), (1, 1, 0, 1, 20, 1, 1), (0, 0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 0, 0, 1), (1, 1, 0, 1, 20, 0, 0),
                 (1, 1, 0, 1, 20, 1, 1), (0, 0, 0, 0, 0, 0, 1), (0, 1, 0, 3, 20, 1, 1)]


# ---- acquire windows, 10 carriers
def weak_tail_window(checker, coded, mod, chirp, lead, window_len, kind, snr_db, seed, from_symbol, gain, scale=0.8):
    """mcdpsk_acquire_restatement.window with the data symbols from `from_symbol` on scaled by `gain` before the channel:
    the codewords carried there arrive weak"""
    w = np.zeros(window_len, np.float32)
    s = checker.mcdpsk_wf_tx(10, mod, po.R1_4, 1, not chirp, coded)
    s = (s * np.float32(scale / np.abs(s).max())).astype(np.float32)
    n_pre = 57600 if chirp else 2512
    cut = n_pre + (9 + from_symbol) * 512
    s[cut:] *= np.float32(gain)
    n = min(len(s), window_len - lead)
    w[lead:lead + n] = s[:n]
    return checker.channel(kind, snr_db, int(seed), w)


ZC_LEAD = 2000
ZC_FL = frame_len(3, 10, 2, 1)
ZC_WL = ZC_LEAD + 2512 + ZC_FL + 2000
ZC_SEARCH = ZC_LEAD + 2512 + 8 * 512
CHIRP_LEAD = 2000
CHIRP_SEARCH = CHIRP_LEAD + 57600 + 8 * 512


def chirp_window_len(bps):
    return CHIRP_LEAD + 57600 + frame_len(3, 10, bps, 1) + 2000


def zc_windows(checker):
    """ZC, connected, DQPSK, frame_cw 3, B = 20 -> the windows of two calls: an interleaved data frame, a plain ACK, noise,
    and an interleaved data frame whose CW2 (the data symbols from 65 on) arrives weak in both calls"""
    from mcdpsk_acquire_restatement import window
    data = coded_cws(data3(20), 20)
    weak = coded_cws(data3(21), 20)
    fixed = [window(checker, data, 10, po.DQPSK, 1, False, ZC_LEAD, ZC_WL, 1, 3.0, 61),
             window(checker, encode_frame(control_frame(ACK, 22)), 10, po.DQPSK, 1, False, ZC_LEAD, ZC_WL, 1, 3.0, 62),
             window(checker, None, 10, po.DQPSK, 1, False, ZC_LEAD, ZC_WL, 1, 3.0, 63)]
    return [np.stack(fixed + [weak_tail_window(checker, weak, po.DQPSK, False, ZC_LEAD, ZC_WL, 1, 3.0, 50 + call, 65, 0.26)]) for call in range(2)]


def handshake_windows(checker):
    """Dual chirp, disconnected, primary DBPSK, frame_cw 3, B = 20: a CONNECT interleaved at 20 sent DBPSK in place; sent DBPSK
    16 samples behind the detector's place over the good channel at -6 dB; sent DQPSK in place"""
    from mcdpsk_acquire_restatement import window
    coded = coded_cws(data_frame(CONNECT, 7, np.arange(25, dtype=np.uint8)), 20)
    wl = chirp_window_len(1)
    return np.stack([window(checker, coded, 10, po.DBPSK, 1, True, CHIRP_LEAD, wl, 0, 10.0, 1),
                     window(checker, coded, 10, po.DBPSK, 1, True, CHIRP_LEAD, wl, 1, -6.0, 106, shift=16),
                     window(checker, coded, 10, po.DQPSK, 1, True, CHIRP_LEAD, wl, 0, 12.0, 5)])
