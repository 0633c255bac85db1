"""The pinned rows of the decodeFrame tests (test_decode_frame_cpu.py, test_gpu_decode_frame.py): each row is a function of
small integers - frame kind, seq, amplitude, noise sigma, numpy seed, n_llr - so nothing large is committed.

    soft bit = amp * (1 - 2 bit) + sigma * N(0, 1)   over the row's signal part
    soft bit = amp * N(0, 1)                          behind it, up to the row stride (also behind n_llr: the library must
                                                      not look there)

Kinds (frames built with the oracle's encoders; `rate` is the handle's):
    ack14        ACK control frame, one codeword at R1/4
    ctl          ACK control frame, one codeword at `rate`
    fixed        encodeFixedFrame data frame (4 codewords, frame + channel interleaved)
    fixed_badhdr the same with the header CRC inverted before encoding: all codewords decode, reassemble fails
    legacyT      non-interleaved data frame of T codewords at `rate`, CW1.. channel-interleaved per codeword when enabled
    legacy3_cut  legacy3 with CW2 replaced by noise
    badhdr       a legacy CW0 (magic intact) whose header CRC is inverted
    total0       a legacy CW0 whose header says total_cw 0 (header CRC valid)
    noise        no signal at all

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
import decode_frame_restatement as R
from mcdpsk_acquire_restatement import ACK

DATA = 0x30
STRIDE = 6 * 648
MODES = {"QAM16_R1_2": (po.QAM16, po.R1_2), "DQPSK_R1_4": (po.DQPSK, po.R1_4), "QAM64_R3_4": (po.QAM64, po.R3_4)}

# (name, kind, seq, amp, sigma, seed, n_llr, path the recipe is meant to reach)
_CLEAN = (4.0, 0.0)
ROWS = {
    "QAM16_R1_2": [
        ("ack14_648", "ack14", 1, *_CLEAN, 11, 648, "CONTROL_R14"),
        ("ack14_long", "ack14", 2, *_CLEAN, 12, 2700, "CONTROL_R14"),
        ("ack14_over", "ack14", 3, *_CLEAN, 13, STRIDE + 1000, "CONTROL_R14"),
        ("ctl_rate", "ctl", 4, *_CLEAN, 14, 648, "CONTROL_CW0"),
        ("ctl_rate_long", "ctl", 5, *_CLEAN, 15, 2592, "CONTROL_CW0"),
        ("fixed_clean", "fixed", 6, *_CLEAN, 16, 2592, "FIXED"),
        ("fixed_retry", "fixed", 7, 2.0, 1.5, 127, 2632, "FIXED"),
        ("fixed_noisy", "fixed", 8, 2.0, 3.5, 18, 2592, "FIXED_FAILED"),
        ("salv14", "ack14", 9, 2.0, 2.2, 3, 2592, "SALVAGE_R14"),
        ("salv_rate", "ctl", 10, 2.0, 1.5, 0, 2592, "SALVAGE_RATE"),
        ("legacy2", "legacy2", 11, *_CLEAN, 21, 2 * 648, "LEGACY"),
        ("legacy3", "legacy3", 12, *_CLEAN, 22, 3 * 648 + 5, "LEGACY"),
        ("legacy5", "legacy5", 13, *_CLEAN, 23, 5 * 648, "LEGACY"),
        ("legacy3_cut", "legacy3_cut", 14, *_CLEAN, 24, 3 * 648, "LEGACY"),
        ("partial", "legacy5", 15, *_CLEAN, 25, 3 * 648, "PARTIAL"),
        ("legacy4", "legacy4", 16, *_CLEAN, 26, 2592, "LEGACY"),
        ("legacy4_short", "legacy4", 17, *_CLEAN, 27, 2591, "PARTIAL"),
        ("badhdr", "badhdr", 18, *_CLEAN, 28, 2592, "BAD_HEADER"),
        ("total0", "total0", 19, *_CLEAN, 29, 1296, "BAD_HEADER"),
        ("none_0", "noise", 0, 2.0, 0.0, 30, 0, "NONE"),
        ("none_647", "noise", 0, 2.0, 0.0, 31, 647, "NONE"),
        ("none_648", "noise", 0, 2.0, 0.0, 32, 648, "NONE"),
        ("none_2591", "noise", 0, 2.0, 0.0, 33, 2591, "NONE"),
        ("noise_2592", "noise", 0, 2.0, 0.0, 34, 2592, "FIXED_FAILED"),
    ],
    "DQPSK_R1_4": [
        ("ack14_648", "ack14", 1, *_CLEAN, 41, 648, "CONTROL_CW0"),
        ("fixed_clean", "fixed", 2, *_CLEAN, 42, 2592, "FIXED"),
        ("fixed_noisy", "fixed", 3, 2.0, 4.5, 43, 2592, "FIXED_FAILED"),
        ("salv14", "ack14", 4, 2.0, 2.2, 3, 2592, "SALVAGE_R14"),
        ("legacy2", "legacy2", 5, *_CLEAN, 45, 2 * 648, "LEGACY"),
        ("legacy5", "legacy5", 6, *_CLEAN, 46, 5 * 648, "LEGACY"),
        ("legacy4", "legacy4", 7, *_CLEAN, 47, 2592, "LEGACY"),
        ("partial", "legacy3", 8, *_CLEAN, 48, 2 * 648, "PARTIAL"),
    ],
    "QAM64_R3_4": [
        ("ack14_long", "ack14", 1, *_CLEAN, 51, 2592, "CONTROL_R14"),
        ("ctl_rate", "ctl", 2, *_CLEAN, 52, 648, "CONTROL_CW0"),
        ("fixed_clean", "fixed", 3, *_CLEAN, 53, 2592, "FIXED"),
        ("fixed_noisy", "fixed", 4, 2.0, 3.0, 54, 2592, "FIXED_FAILED"),
        ("salv14", "ack14", 5, 2.0, 2.2, 6, 2592, "SALVAGE_R14"),
        ("salv_rate", "ctl", 6, 2.0, 0.9, 64, 2592, "SALVAGE_RATE"),
        ("legacy3", "legacy3", 7, *_CLEAN, 57, 3 * 648, "LEGACY"),
        ("legacy4", "legacy4", 8, *_CLEAN, 58, 2592, "LEGACY"),
    ],
}
# rows run without RIA_DECODE_CRC_RECOVER (flags 3): the only way to "all four decoded, reassemble failed"
ROWS_NO_RECOVER = [
    ("fixed_badhdr", "fixed_badhdr", 1, *_CLEAN, 61, 2592, "FIXED"),
    ("fixed_clean", "fixed", 2, *_CLEAN, 62, 2592, "FIXED"),
    ("ack14_648", "ack14", 3, *_CLEAN, 63, 648, "CONTROL_R14"),
]


def _bits(coded):
    return np.unpackbits(np.asarray(coded, np.uint8))


def _encode_cw(rate, data):
    """one codeword: `data` (bytes_per_cw bytes at most) zero-padded to the code's information bytes -> 648 coded bits"""
    O = R.oracle()
    kb = (O.code(rate).k + 7) // 8
    info = np.zeros(kb, np.uint8)
    info[:len(data)] = data
    return _bits(O.ldpc_encode(rate, info))[:648]


def legacy_frame(rate, seq, total_cw, header_total=None):
    """serialized data frame that takes exactly total_cw codewords at `rate` (CW0 bpc bytes, CW1+ marker, index, bpc - 2)"""
    bpc = R.bytes_per_cw(rate)
    n_payload = bpc + (total_cw - 1) * (bpc - 2) - 19 - 3
    payload = (np.arange(n_payload) * 7 + seq) % 251
    return R.data_frame(DATA, seq, payload.astype(np.uint8), total_cw=total_cw if header_total is None else header_total)


def legacy_bits(rate, bps, ch_deint, frame):
    bpc = R.bytes_per_cw(rate)
    P = R.channel_perm(bps)
    out = [_encode_cw(rate, frame[:bpc])]
    off, i = bpc, 1
    while off < len(frame):
        cw = np.zeros(bpc, np.uint8)
        cw[0], cw[1] = 0xD5, i
        chunk = frame[off:off + bpc - 2]
        cw[2:2 + len(chunk)] = chunk
        coded = _encode_cw(rate, cw)
        if ch_deint:
            tx = np.zeros(648, np.uint8)
            tx[P] = coded                      # the receiver reads decoder input i at position P[i]
            coded = tx
        out.append(coded)
        off += bpc - 2
        i += 1
    return np.concatenate(out)


def signal_bits(kind, mode, ch_deint, seq):
    mod, rate = MODES[mode]
    O = R.oracle()
    bps = O.geom(mod, rate).bits_per_symbol
    bpc = R.bytes_per_cw(rate)
    if kind == "noise":
        return np.zeros(0, np.uint8)
    if kind == "ack14":
        return _encode_cw(po.R1_4, R.control_frame(ACK, seq))
    if kind == "ctl":
        return _encode_cw(rate, R.control_frame(ACK, seq))
    if kind in ("fixed", "fixed_badhdr"):
        info = O.make_frame(((np.arange(4 * bpc - 24) * 5 + seq) % 249).astype(np.uint8), seq, rate)
        if kind == "fixed_badhdr":
            info[15] ^= 0xFF
            info[16] ^= 0xFF
        return _bits(O.encode_fixed_frame(info, rate, ch_deint, bps))[:2592]
    if kind == "badhdr":
        f = legacy_frame(rate, seq, 2).copy()
        f[15] ^= 0xFF
        f[16] ^= 0xFF
        return _encode_cw(rate, f[:bpc])
    if kind == "total0":
        return _encode_cw(rate, legacy_frame(rate, seq, 2, header_total=0)[:bpc])
    if kind.startswith("legacy"):
        total = int(kind[6])
        return legacy_bits(rate, bps, ch_deint, legacy_frame(rate, seq, total))
    raise ValueError(kind)


def build_row(recipe, mode, ch_deint=True):
    """-> (float32 [STRIDE] row, n_llr as passed to the library (may exceed STRIDE))"""
    _, kind, seq, amp, sigma, seed, n_llr, _ = recipe
    bits = signal_bits(kind, mode, ch_deint, seq)
    noise = np.random.default_rng(seed).standard_normal(STRIDE)
    row = amp * noise
    n = len(bits)
    row[:n] = amp * (1.0 - 2.0 * bits) + sigma * noise[:n]
    if kind == "legacy3_cut":
        row[2 * 648:3 * 648] = amp * noise[2 * 648:3 * 648]
    return row.astype(np.float32), int(n_llr)


def batches():
    """every pinned batch: (label, mode, ch_deint, flags, recipes)"""
    out = []
    for mode in MODES:
        out.append((mode, mode, True, 7, ROWS[mode]))
    out.append(("QAM16_R1_2_nochan", "QAM16_R1_2", False, 7, ROWS["QAM16_R1_2"]))
    out.append(("QAM16_R1_2_norecover", "QAM16_R1_2", True, 3, ROWS_NO_RECOVER))
    return out


_expected = {}


def expected(checker_name, checker, label):
    """(rows float32 [n, STRIDE], n_llr int32 [n], list of restatement results), computed once per checker and batch"""
    key = (checker_name, label)
    if key not in _expected:
        _, mode, ch, flags, recipes = next(b for b in batches() if b[0] == label)
        mod, rate = MODES[mode]
        bps = R.oracle().geom(mod, rate).bits_per_symbol
        rows, ns = zip(*(build_row(r, mode, ch) for r in recipes))
        res = [R.decode_frame(checker, row[:min(n, STRIDE)], rate, bps, ch, flags) for row, n in zip(rows, ns)]
        _expected[key] = (np.stack(rows), np.array(ns, np.int32), res)
    return _expected[key]
