"""CPU restatement of ria_gpu_decode_frame_batch on the checkers (pyoracle.Oracle, or pyoracle.Ref where it is built): the
OFDM branch of StreamingDecoder::decodeFrame (src/gui/modem/streaming_decoder.cpp:2821-3059) written out statement by
statement on checker.ldpc_decode (codec_->decode: recommended iterations of the decode's rate, min-sum factor 0.75),
checker.robust_decode (robustDecodeSingleCW), checker.decode_fixed_frame and ro_crc16.

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
from burst_restatement import frame_valid
from mcdpsk_acquire_restatement import CONTROL_TYPES, control_frame, crc16, data_frame, oracle  # noqa: F401  (re-exported)

NONE, CONTROL_R14, CONTROL_CW0, FIXED, SALVAGE_R14, SALVAGE_RATE, FIXED_FAILED, LEGACY, PARTIAL, BAD_HEADER = range(10)
PATH_NAMES = ("NONE", "CONTROL_R14", "CONTROL_CW0", "FIXED", "SALVAGE_R14", "SALVAGE_RATE", "FIXED_FAILED", "LEGACY", "PARTIAL",
              "BAD_HEADER")
RESULT_FIELDS = ("success", "codewords_ok", "codewords_failed", "frame_type", "path", "header_total_cw", "stages", "frame_bytes",
                 "iters_r14", "iters_cw0", "tries_r14", "tries_rate")
MAX_CW = 32
_perm = {}


def bytes_per_cw(rate):
    return oracle().geom(po.QAM16, rate).bytes_per_cw


def recommended_iterations(rate):
    return oracle().geom(po.QAM16, rate).max_iter


def channel_perm(bps):
    """P with dec_in[i] = rx[P[i]]: ChannelInterleaver(bps, 648)::deinterleave of one codeword, read off the oracle's two
    gather tables: gather_table(bps, True)[c*648 + i] == gather_table(bps, False)[c*648 + P[i]], the same P for every c."""
    if bps not in _perm:
        t_ch, t_no = oracle().gather_table(bps, True), oracle().gather_table(bps, False)
        P = None
        for c in range(4):
            inv = {int(v): j for j, v in enumerate(t_no[c * 648:(c + 1) * 648])}
            Pc = np.array([inv[int(v)] for v in t_ch[c * 648:(c + 1) * 648]], np.int64)
            assert P is None or np.array_equal(P, Pc)
            P = Pc
        assert sorted(P) == list(range(648))
        _perm[bps] = P
    return _perm[bps]


def parse_header(d):
    """parseHeader (frame_v2.cpp:1195-1253) on >= 20 bytes with magic -> (valid, type, total_cw, payload_len).  A data header
    with total_cw 0 (undefined behaviour in the reference) is an invalid header."""
    if len(d) < 20 or d[0] != 0x55 or d[1] != 0x4C:
        return False, 0x10, 0, 0
    t = int(d[2])
    if t in CONTROL_TYPES:
        return crc16(d[:18]) == (int(d[18]) << 8 | int(d[19])), t, 1, 0
    if crc16(d[:15]) != (int(d[15]) << 8 | int(d[16])) or int(d[12]) == 0:
        return False, t, 0, 0
    return True, t, int(d[12]), int(d[13]) << 8 | int(d[14])


def reassemble(cws, ftype, plen):
    """CodewordStatus::reassemble + reassembleCodewords (frame_v2.cpp:1030-1063, :959-989), header already parsed"""
    expected = 20 if ftype in CONTROL_TYPES else 17 + plen + 2
    out = []
    for i, cw in enumerate(cws):
        remaining = expected - len(out)
        if remaining == 0:
            break
        src = cw[2:] if (i and cw[0] == 0xD5) else cw
        out += list(src[:remaining])
    return np.array(out, np.uint8)


def _probe(checker, rate, llr648, robust):
    """-> (ok with magic, bytes truncated to the rate's codeword, iterations, tries)"""
    if robust:
        ok, d, it, tries = checker.robust_decode(rate, llr648)
    else:
        ok, d, it = checker.ldpc_decode(rate, llr648, recommended_iterations(rate), 0.75)
        tries = 1
    magic = bool(ok) and len(d) >= 2 and d[0] == 0x55 and d[1] == 0x4C
    return magic, np.asarray(d[:bytes_per_cw(rate)], np.uint8), int(it), int(tries)


def decode_frame(checker, llr, rate, bps, ch_deint=True, flags=7):
    """One row of soft bits -> dict with every ria_dframe_result field, frame (frame_data) and the fixed attempt: fixed_ran,
    fixed_ok [4], fixed_info [4 * bpc] (None on Ref unless a codeword decoded: Ref zeroes failed codewords), and on the
    oracle fixed_iters, fixed_attempts, fixed_valid, fixed_needs_recovery."""
    llr = np.ascontiguousarray(llr, np.float32)[:MAX_CW * 648]
    bpc = bytes_per_cw(rate)
    is_oracle = isinstance(checker, po.Oracle)
    r = dict(success=0, codewords_ok=0, codewords_failed=0, frame_type=0x10, path=NONE, header_total_cw=0, stages=0, frame_bytes=0,
             iters_r14=0, iters_cw0=0, tries_r14=0, tries_rate=0, frame=np.zeros(0, np.uint8), fixed_ran=False)

    def done(path, **kw):
        r.update(path=path, **kw)
        r["frame_bytes"] = len(r["frame"])
        return r

    if len(llr) < 648:                                                    # step 0
        return done(NONE)
    cw0 = llr[:648]
    if rate != po.R1_4:                                                   # step 1 (:2867-2890)
        magic, d, it, _ = _probe(checker, po.R1_4, cw0, False)
        r["stages"] |= 1
        r["iters_r14"] = it
        if magic:
            valid, t, total, _ = parse_header(d)
            if valid and total == 1:
                return done(CONTROL_R14, success=1, codewords_ok=1, frame=d, frame_type=t, header_total_cw=1)
    magic0, d0, it, _ = _probe(checker, rate, cw0, False)                 # step 2 (:2892-2930)
    r["stages"] |= 2
    r["iters_cw0"] = it
    try_fi, hdr = False, (False, 0x10, 0, 0)
    if magic0:
        hdr = parse_header(d0)
        if hdr[0]:
            r.update(frame_type=hdr[1], header_total_cw=hdr[2])
            if hdr[2] == 1:
                return done(CONTROL_CW0, success=1, codewords_ok=1, frame=d0)
            if hdr[2] == 4:
                try_fi = True
    else:
        try_fi = True
    if try_fi and len(llr) >= 2592:                                       # step 3 (:2932-3010)
        r["stages"] |= 4
        r["fixed_ran"] = True
        if is_oracle:
            data, ok, iters, att = checker.decode_fixed_frame(llr[:2592], rate, ch_deint, bps, flags=flags)
            valid = frame_valid(data, ok, bpc) if ok.all() else 0
            r.update(fixed_iters=iters.astype(np.uint16), fixed_attempts=att.astype(np.uint8), fixed_valid=valid,
                     fixed_needs_recovery=int(bool(ok.all()) and not valid))
        else:
            assert flags == 7, "the compiled reference runs the whole of decodeFixedFrame"
            data, ok = checker.decode_fixed_frame(llr[:2592], rate, ch_deint, bps)
            valid = int(ok.all())
        data = np.asarray(data[:4 * bpc], np.uint8)
        r.update(fixed_ok=np.asarray(ok, np.uint8), fixed_info=data, codewords_ok=int((ok != 0).sum()), codewords_failed=int((ok == 0).sum()))
        if ok.all():
            if valid:
                _, t, _, plen = parse_header(data[:bpc])
                return done(FIXED, success=1, frame=reassemble([data[c * bpc:(c + 1) * bpc] for c in range(4)], t, plen), frame_type=t)
            return done(FIXED)
        for srate, stage, key, path in ((po.R1_4, 8, "tries_r14", SALVAGE_R14), (rate, 16, "tries_rate", SALVAGE_RATE)):
            if path == SALVAGE_RATE and rate == po.R1_4:
                break
            magic, d, _, tries = _probe(checker, srate, cw0, True)
            r["stages"] |= stage
            r[key] = tries
            if magic:
                valid, t, total, _ = parse_header(d)
                if valid and total == 1:
                    return done(path, success=1, codewords_ok=1, codewords_failed=0, frame=d, frame_type=t, header_total_cw=1)
    if not magic0:                                                        # step 5
        return done(FIXED_FAILED if r["fixed_ran"] else NONE)
    r["codewords_ok"] = 1                                                 # step 4 (:3012-3058): codewords_failed is NOT reset
    if not hdr[0]:
        return done(BAD_HEADER)
    _, t, total, plen = hdr
    if len(llr) // 648 < total:
        return done(PARTIAL, frame=d0)
    r["stages"] |= 32
    P = channel_perm(bps)
    cws, all_ok = [d0], True
    for i in range(1, total):
        bits = llr[i * 648:(i + 1) * 648]
        if ch_deint:
            bits = bits[P]
        ok, d, _ = checker.ldpc_decode(rate, bits, recommended_iterations(rate), 0.75)
        if ok and len(d) >= bpc:
            cws.append(np.asarray(d[:bpc], np.uint8))
            r["codewords_ok"] += 1
        else:
            all_ok = False
            r["codewords_failed"] += 1
    if all_ok:
        return done(LEGACY, success=1, frame=reassemble(cws, t, plen))
    return done(LEGACY)
