"""CPU restatement of ria_gpu_rx_window_batch on the checkers (pyoracle.Oracle, or pyoracle.Ref where it is built): what
gui::StreamingDecoder does with one connected-mode OFDM-CHIRP window (src/gui/modem/streaming_decoder.cpp), step by step:

1. detection and acceptance (acquire_restatement / control_restatement.control_acquire_window), a marked window under
   use_burst_interleave_ left to the burst path (:1087-1092)
2. the control hypothesis on n_ctl samples (:1268-1344, control_restatement.control_hypothesis)
3. pass 1: process() with the data profile on the same span, marker off, known CFO; fading index; CFO feedback clamped to
   +-2 Hz in float32 (:1346-1434); the CW0 peek and the QAM partial-frame escalation (:1505-1597)
4. pass 2 on getMinSamplesForCWCount(pending) samples at the fed-back CFO, feedback again
5. decodeFrame (:1626, decode_frame_restatement.decode_frame)
6. small-frame recovery (:1806-1853)
7. timing recovery with decodeFrame on spans of frame_len at sync_cfo (:1859-1965)
8. consumed samples (:1994-2013)

Every process() of the ladder is restated as a process() on a fresh object: processPresynced() clears every per-frame member
of the demodulator (demodulator.cpp:1264-1309) and process() sets CFO and phase anew, so a kept object carries nothing over.

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
import control_restatement as CR
import decode_frame_restatement as DF
from acquire_restatement import RETRY_DELTAS, po_oracle

NOT_ACCEPTED, BURST, CONTROL_PROFILE, DECODED, NEED_SAMPLES, TOO_LONG = range(6)
OUTCOME_NAMES = ("NOT_ACCEPTED", "BURST", "CONTROL_PROFILE", "DECODED", "NEED_SAMPLES", "TOO_LONG")
PEEK_NONE, R14_ONE, R14_MULTI, RATE_ONE, RATE_MULTI, RATE_BAD_HEADER, FAILED, QAM_PARTIAL, DIRECT = range(9)
PEEK_NAMES = ("NONE", "R14_ONE", "R14_MULTI", "RATE_ONE", "RATE_MULTI", "RATE_BAD_HEADER", "FAILED", "QAM_PARTIAL", "DIRECT")
NON_DATA_TYPES = (0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40, 0x12, 0x13, 0x14)   # isControlFrame || isConnectFrame
WINDOW_FIELDS = ("outcome", "peek", "pending_total_cw", "small_frame", "tries_peek_r14", "tries_peek_rate", "tries_small_r14",
                 "tries_small_rate", "frame_len", "next_pos", "need_samples")
WINDOW_WORDS = ("sync_cfo_hz", "peek_cfo_hz", "fading_index")
f32 = np.float32


def qam_mods():
    return tuple(getattr(po, k) for k in ("QAM16", "QAM32", "QAM64", "QAM256") if hasattr(po, k))


def clamp_cfo(estimated, current):
    """:1414-1434 in float32; a NaN drift leaves the estimate"""
    estimated, current = f32(estimated), f32(current)
    drift = f32(estimated - current)
    if abs(drift) > f32(2.0):
        return f32(current + np.copysign(f32(2.0), drift))
    return estimated


def samples_for_cw(bps, cw):
    """getMinSamplesForCWCount"""
    return (2 + -(-648 * cw // bps)) * CR.SYM


def consumed(frame_len, frame, bps):
    """:1994-2013"""
    c = frame_len
    if frame["success"] and len(frame["frame"]) >= 3 and int(frame["frame"][2]) in NON_DATA_TYPES:
        actual = frame["codewords_ok"] + frame["codewords_failed"]
        if actual > 0:
            c = min(c, samples_for_cw(bps, actual))
    return c


def zero_frame():
    r = {k: 0 for k in DF.RESULT_FIELDS}
    r["frame"] = np.zeros(0, np.uint8)
    return r


def robust_header(checker, rate, llr648, truncate):
    """robustDecodeSingleCW, magic, optional truncation to the rate's codeword, parseHeader -> (magic, valid, total_cw, tries)"""
    ok, d, _, tries = checker.robust_decode(rate, llr648)
    if not (ok and len(d) >= 4 and d[0] == 0x55 and d[1] == 0x4C):
        return False, False, 0, int(tries)
    d = np.asarray(d, np.uint8)
    if truncate:
        d = d[:DF.bytes_per_cw(rate)]
    valid, _, total, _ = DF.parse_header(d)
    return True, bool(valid), int(total) if valid else 0, int(tries)


def rx_window(checker, mod, rate, x, search_len, known_cfo=0.0, detect_threshold=0.15, min_confidence=0.78, abs_base=0,
              interleave=False, retry=True, ch_deint=True, flags=7, carriers=59):
    """One window -> dict: the ria_window_result fields (WINDOW_FIELDS, WINDOW_WORDS as float32), `frame` (the
    decode_frame_restatement result of the reported span, or the control frame's), `acq` (ria_acq_result fields), `control`
    (the control hypothesis's result) and `status` (the checker's status words of the reported span, None if there is none),
    `spans`: the (samples, start, cfo) of every process() of the data profile, in order."""
    x = np.ascontiguousarray(x, np.float32)
    bps = po_oracle(checker).geom(mod, rate).bits_per_symbol
    n_ctl = CR.control_frame_samples(mod, rate, carriers)
    ctl, acq = CR.control_acquire_window(checker, mod, rate, x, search_len, n_ctl, known_cfo, detect_threshold, min_confidence, abs_base, interleave)
    out = dict(outcome=NOT_ACCEPTED, peek=PEEK_NONE, pending_total_cw=0, small_frame=0, tries_peek_r14=0, tries_peek_rate=0,
               tries_small_r14=0, tries_small_rate=0, frame_len=0, next_pos=-1, need_samples=0, sync_cfo_hz=f32(known_cfo),
               peek_cfo_hz=f32(0), fading_index=f32(0), frame=zero_frame(), acq=acq, control=ctl, status=None, spans=[])
    if not acq["accepted"]:
        return out
    if not ctl["tried"]:
        out["outcome"] = BURST
        return out
    start = acq["sync_start"]
    if ctl["success"]:                                                      # :1298-1335
        fr = zero_frame()
        fr.update(success=1, codewords_ok=1, frame_type=ctl["frame_type"], header_total_cw=1, frame_bytes=20, frame=ctl["frame"].copy())
        out.update(outcome=CONTROL_PROFILE, frame=fr, frame_len=n_ctl, next_pos=start + n_ctl, fading_index=ctl["status"]["fading_index"],
                   status=ctl["status"], status_n_llr=ctl["n_llr"])
        return out
    out["outcome"] = DECODED
    acq["cfo_hz"] = f32(0)
    st = dict(sync_cfo=f32(known_cfo), frame_len=n_ctl)

    def process(s, n, cfo):
        out["spans"].append((s, n, f32(cfo)))
        return CR.process_span(checker, mod, rate, x[s:s + n], float(cfo), abs_base + s, False)

    def report(frame, status, n_llr):
        out.update(frame=frame, status=status, status_n_llr=n_llr)
        acq["cfo_hz"] = status["cfo_hz"]

    def decode(llr):
        return DF.decode_frame(checker, llr, rate, bps, ch_deint, flags)

    def finish():
        out.update(frame_len=st["frame_len"], sync_cfo_hz=st["sync_cfo"])
        if out["outcome"] == DECODED:
            acq["frame_start"] = start + acq["delta"]
            out["next_pos"] = acq["frame_start"] + consumed(st["frame_len"], out["frame"], bps)
        return out

    def pass_done(status, n_llr):
        """False: process() returned false (:1352-1360)"""
        if n_llr < 648:
            out.update(status=status, status_n_llr=n_llr)
            return False
        out["fading_index"] = status["fading_index"]
        st["sync_cfo"] = clamp_cfo(status["cfo_hz"], st["sync_cfo"])
        return True

    # 3. pass 1
    llr, status, n_llr = process(start, n_ctl, known_cfo)
    if not pass_done(status, n_llr):
        return finish()
    out["peek_cfo_hz"] = status["cfo_hz"]
    pending = 0
    if n_llr < 1296:                                                        # :1511-1575
        magic, valid, total, out["tries_peek_r14"] = robust_header(checker, po.R1_4, llr[:648], True)
        if magic and valid and total == 1:
            out["peek"] = R14_ONE
        elif magic and valid and total > 1:
            out["peek"], pending = R14_MULTI, total
        elif rate != po.R1_4:
            magic, valid, total, out["tries_peek_rate"] = robust_header(checker, rate, llr[:648], True)
            if magic and valid and total == 1:
                out["peek"] = RATE_ONE
            elif magic and valid and total > 1:
                out["peek"], pending = RATE_MULTI, total
            elif magic:
                out["peek"], pending = RATE_BAD_HEADER, 4
            else:
                out["peek"], pending = FAILED, 4
        else:
            out["peek"], pending = FAILED, 4
    elif n_llr < 2592 and mod in qam_mods():                                # :1582-1597
        out["peek"], pending = QAM_PARTIAL, 4
    else:
        out["peek"] = DIRECT
    out["pending_total_cw"] = pending
    # 4. pass 2
    if pending:
        st["frame_len"] = samples_for_cw(bps, pending)
        if start + st["frame_len"] > len(x):
            out.update(outcome=NEED_SAMPLES, need_samples=st["frame_len"])
            return finish()
        if pending > 4:
            out["outcome"] = TOO_LONG
            return finish()
        llr, status, n_llr = process(start, st["frame_len"], st["sync_cfo"])
        if not pass_done(status, n_llr):
            return finish()
    # 5. decodeFrame
    report(decode(llr), status, n_llr)
    # 6. small-frame recovery
    one_cw = samples_for_cw(bps, 1)
    if not out["frame"]["success"] and one_cw <= st["frame_len"]:
        out["small_frame"] = 1
        s_llr, s_status, s_n = process(start, one_cw, st["sync_cfo"])
        if s_n >= 648:
            for srate, key, bit in ((po.R1_4, "tries_small_r14", 0), (rate, "tries_small_rate", 0x10)):
                if bit and rate == po.R1_4:
                    break
                magic, valid, total, out[key] = robust_header(checker, srate, s_llr[:648], False)
                if magic and valid and total == 1:
                    out["small_frame"] = 2 | bit
                    report(decode(s_llr), s_status, s_n)
                    st["frame_len"] = one_cw
                    break
                if magic and valid and 1 < total < 4:
                    exact = min(samples_for_cw(bps, total), st["frame_len"])
                    out["small_frame"] = 3 | bit
                    e_llr, e_status, e_n = process(start, exact, st["sync_cfo"])
                    report(decode(e_llr), e_status, e_n)
                    st["frame_len"] = exact
                    break
    # 7. timing recovery
    if not out["frame"]["success"] and out["frame"]["codewords_ok"] == 0 and retry:
        for d in RETRY_DELTAS:
            s = start + d
            if not (s >= 0 and s + st["frame_len"] <= len(x)):
                continue
            acq["candidates"] += 1
            c_llr, c_status, c_n = process(s, st["frame_len"], st["sync_cfo"])
            if c_n < 648:
                continue
            r = decode(c_llr)
            if not (r["success"] or r["codewords_ok"] > 0):
                continue
            report(r, c_status, c_n)
            st["sync_cfo"] = clamp_cfo(c_status["cfo_hz"], st["sync_cfo"])
            out["fading_index"] = c_status["fading_index"]
            acq["delta"] = d
            break
    return finish()
