"""CPU restatement of ria_gpu_mcdpsk_window_batch on the checkers (pyoracle.Oracle, or pyoracle.Ref where it is built):
StreamingDecoder::decodeCurrentFrame() for the MC-DPSK mode (src/gui/modem/streaming_decoder.cpp:1060-1266, :1346-1376,
:1436-1503, :1599-1797, :1967-2013) written out as the loop of passes the reference makes - every pass copies its span, runs
the energy test and process() again, exactly as the reference does between SYNC_FOUND and DECODING - on mcdpsk_wf_rx (the
detectors), mcdpsk_demod (process() after an external detection), robust_decode and ro_crc16.  The decode of the last pass
and the handshake fallbacks are mcdpsk_ci_restatement.decode_mcdpsk_frame_ci and mcdpsk_acquire_restatement's candidates.

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
from mcdpsk_acquire_restatement import CONNECT, CONNECT_ACK, CONNECT_NAK, CONTROL_TYPES, crc16, frame_candidates, frame_len
from mcdpsk_ci_restatement import decode_mcdpsk_frame_ci, deinterleave
from mcdpsk_harq_restatement import empty_harq

NOT_ACCEPTED, REPLAY, PING, PROCESS_FAILED, DECODED, NEED_SAMPLES, TOO_LONG = range(7)
OUTCOMES = ("NOT_ACCEPTED", "REPLAY", "PING", "PROCESS_FAILED", "DECODED", "NEED_SAMPLES", "TOO_LONG")
PEEK_NONE, NO_HEADER, HEADER_SINGLE, HEADER_MULTI, CONNECT_FORCED = range(5)
WHAT = ("NONE", "NO_HEADER", "HEADER_SINGLE", "HEADER_MULTI", "CONNECT_FORCED")
HANDSHAKE_FALLBACK, EARLY_WINDOW, HANDSHAKE_WINDOW, DEINTERLEAVED, SALVAGE = 0x10, 0x20, 0x40, 0x80, 0x100
BITS = dict(HANDSHAKE_FALLBACK=HANDSHAKE_FALLBACK, EARLY_WINDOW=EARLY_WINDOW, HANDSHAKE_WINDOW=HANDSHAKE_WINDOW, DEINTERLEAVED=DEINTERLEAVED,
            SALVAGE=SALVAGE)
NO_LAST_SYNC = -2 ** 31
MIN_HANDSHAKE_CW = 3          # max(2, calculateCodewords(ConnectFrame::PAYLOAD_SIZE = 25, R1/4))
MIN_AVAIL = 4608 + 5000

RESULT_FIELDS = ("outcome", "peek", "next_pos", "need_samples", "pending_total_cw", "frame_len", "passes", "peek_total_cw",
                 "last_decoded_sync", "deliver", "is_ping", "peek_tries")
RESULT_WORDS = ("training_rms", "rms")
ACQ_FIELDS = ("detected", "accepted", "sync_start", "frame_start", "delta", "modulation", "candidates", "success", "codewords_ok",
              "codewords_failed", "frame_type", "header_total_cw", "frame_bytes", "n_llr", "cw0_deinterleaved", "ci_tried")
ACQ_WORDS = ("correlation", "cfo_hz", "fading_index")
HARQ_FIELDS = ("valid", "seq", "src_hash", "dst_hash", "stored_mask", "sum_mask", "recovered_mask", "max_combine", "entry")


def chain_rms(v):
    """float32 sum of squares in ascending order / count, sqrtf (:1142-1160); 0 for an empty span"""
    v = np.ascontiguousarray(v, np.float32)
    if len(v) == 0:
        return np.float32(0.0)
    with np.errstate(all="ignore"):
        sq = (v * v).astype(np.float32)
        # np.cumsum over float32 adds in ascending order, one rounding per element
        acc = np.cumsum(sq, dtype=np.float32)[-1]
        return np.float32(np.sqrt(np.float32(acc / np.float32(len(v)))))


def energy(span):
    """-> (training_rms, rms, is_ping) of the legacy PING test (:1127-1160, :1222-1223)"""
    train_len = min(4608, len(span))
    t = chain_rms(span[:train_len])
    check_len = min(len(span) - train_len, 5000)
    r = chain_rms(span[train_len:train_len + check_len])
    with np.errstate(all="ignore"):
        ratio = np.float32(r / t) if t > np.float32(0.001) else np.float32(0.0)
    return t, r, bool(ratio < np.float32(0.6))


def parse_header(d):
    """v2::parseHeader on the whole decoded vector (frame_v2.cpp:1195-1252: it reads bytes 0..19) -> (valid, type, total_cw)"""
    if len(d) < 20 or d[0] != 0x55 or d[1] != 0x4C:
        return False, 0, 0
    t = int(d[2])
    if t in CONTROL_TYPES:
        if crc16(d[:18]) != (int(d[18]) << 8 | int(d[19])):
            return False, t, 0
        return True, t, 1
    if crc16(d[:15]) != (int(d[15]) << 8 | int(d[16])):
        return False, t, 0
    return True, t, int(d[12])


def _magic(ok, d):
    return bool(ok) and len(d) >= 4 and d[0] == 0x55 and d[1] == 0x4C


def mcdpsk_window(checker, x, search_len, carriers=10, bps=1, spreading=1, chirp=True, disconnected=None, known_cfo=0.0,
                  detect_threshold=None, min_confidence=0.0, retry=True, B=None, cache=None, now=0, pending_total_cw=0,
                  first_avail=0, last_decoded_sync=NO_LAST_SYNC, max_cw=8):
    """One window -> dict of RESULT_FIELDS / RESULT_WORDS, acq (ria_mcdpsk_acq_result fields with frame and llr), harq"""
    if disconnected is None:
        disconnected = chirp
    assert 0 <= pending_total_cw <= 255 and (first_avail == 0 or first_avail >= MIN_AVAIL)
    x = np.ascontiguousarray(x, np.float32)
    mod = po.DBPSK if bps == 1 else po.DQPSK
    fl = lambda n: frame_len(n, carriers, bps, spreading)
    assert disconnected or pending_total_cw or first_avail == 0 or first_avail >= fl(1)
    span0 = fl(pending_total_cw) if pending_total_cw else (min(fl(1), first_avail) if first_avail else fl(1))
    thr = (0.15 if chirp else 0.2) if detect_threshold is None else detect_threshold
    sync4, _, _ = checker.mcdpsk_wf_rx(carriers, mod, po.R1_4, spreading, not chirp, x[:search_len], known_cfo, thr, span0)
    detected = bool(sync4[0])
    start = int(sync4[1]) if detected else -1
    corr = np.float32(sync4[2])
    accepted = detected and not (corr < np.float32(min_confidence)) and start >= 0 and start + span0 <= len(x)
    acq = dict(detected=int(detected), accepted=int(accepted), sync_start=start, frame_start=start if accepted else -1, correlation=corr,
               cfo_hz=np.float32(0.0), fading_index=np.float32(0.0), delta=0, modulation=po.DQPSK if bps == 2 else po.DBPSK,
               candidates=0, success=0, codewords_ok=0, codewords_failed=0, frame_type=0x10, header_total_cw=0, frame_bytes=0,
               n_llr=0, frame=np.zeros(0, np.uint8), llr=np.zeros(0, np.float32), cw0_deinterleaved=0, ci_tried=0)
    out = dict(outcome=NOT_ACCEPTED, peek=0, next_pos=-1, need_samples=0, pending_total_cw=0, frame_len=0, passes=0, peek_total_cw=0,
               training_rms=np.float32(0.0), rms=np.float32(0.0), last_decoded_sync=int(last_decoded_sync), deliver=0, is_ping=0,
               peek_tries=0, acq=acq, harq=empty_harq())
    if not accepted:
        return out
    cfo = np.float32(sync4[3])
    if not disconnected and abs(known_cfo) > 0.01 and abs(np.float32(cfo) - np.float32(known_cfo)) > 1.0:      # :903-917
        cfo = np.float32(known_cfo)
    acq["cfo_hz"] = cfo
    if last_decoded_sync != NO_LAST_SYNC and abs(start - last_decoded_sync) < 200:                              # :876-889
        out.update(outcome=REPLAY, next_pos=start + 9600 + 4800)
        return out

    pending = int(pending_total_cw)
    first = True
    while True:                                             # one turn = one decodeCurrentFrame()
        if pending > 0:
            n_span = fl(pending)
            if start + n_span > len(x):                     # checkIfReadyToDecode never lets this pass start (:989-991)
                out.update(outcome=NEED_SAMPLES, need_samples=n_span, pending_total_cw=pending)
                return out
        else:
            n_span = span0
        span = x[start:start + n_span]
        t_rms, d_rms, is_ping = energy(span)
        if first:
            out.update(training_rms=t_rms, rms=d_rms)
        else:                                               # the same >= 9608 samples: the same floats
            assert t_rms.view(np.uint32) == out["training_rms"].view(np.uint32) and d_rms.view(np.uint32) == out["rms"].view(np.uint32)
        first = False
        if disconnected and is_ping:                        # allow_ping_detection = !connected_
            acq.update(success=1, frame_type=0x01)
            out.update(outcome=PING, passes=out["passes"] + 1, is_ping=1, deliver=1, next_pos=start + fl(1), last_decoded_sync=start)
            return out
        if pending > max_cw:                                # the library's limit: process() would run on a span it cannot take
            out.update(outcome=TOO_LONG, pending_total_cw=pending)
            return out
        out["passes"] += 1
        llr, aux = checker.mcdpsk_demod(carriers, bps, spreading, span, float(cfo), 0.0)
        assert len(llr) > 0                                 # PROCESS_FAILED: no span of >= 9608 samples gets here
        avail_cw = len(llr) // 648
        if pending == 0 and len(llr) >= 648:                # the CW0 peek (:1444-1503)
            min_hs = MIN_HANDSHAKE_CW if disconnected else 0
            ok, d, _, tries = checker.robust_decode(po.R1_4, llr[:648])
            out["peek_tries"] = tries
            if not _magic(ok, d) and B is not None:
                ok_i, d_i, _, tries_i = checker.robust_decode(po.R1_4, deinterleave(llr[:648], B))
                out["peek_tries"] += tries_i
                if _magic(ok_i, d_i):
                    ok, d = True, d_i
                    out["peek"] |= DEINTERLEAVED
            what = NO_HEADER
            if _magic(ok, d):
                valid, t, total = parse_header(d)
                if valid:
                    out["peek_total_cw"] = total
                    what = HEADER_SINGLE
                    needed = total
                    if t in (CONNECT, CONNECT_ACK, CONNECT_NAK) and min_hs > 0 and needed < min_hs:
                        needed = min_hs
                        what = CONNECT_FORCED
                    if needed > 1 and avail_cw < needed:
                        out["peek"] |= what if what == CONNECT_FORCED else HEADER_MULTI
                        pending = needed
                        continue
            out["peek"] |= what
            if min_hs > 1 and avail_cw < min_hs:
                out["peek"] |= HANDSHAKE_FALLBACK
                pending = min_hs
                continue
        if disconnected and pending == 0 and len(llr) < 648:   # :1600-1609
            out["peek"] |= EARLY_WINDOW
            pending = 1
            continue
        if disconnected and avail_cw < MIN_HANDSHAKE_CW and pending < MIN_HANDSHAKE_CW:   # :1611-1624
            out["peek"] |= HANDSHAKE_WINDOW
            pending = MIN_HANDSHAKE_CW
            continue

        # decodeFrame -> decodeMCDPSKFrame on this pass's soft bits, then the fallbacks on spans of this pass's length
        harq = [empty_harq()]

        def candidate(delta, alt):
            b = (3 - bps) if alt else bps
            s = start + delta
            if delta == 0 and not alt:
                l, a = llr, aux
            else:
                l, a = checker.mcdpsk_demod(carriers, b, spreading, x[s:s + n_span], float(cfo), 0.0)
            r, hq = decode_mcdpsk_frame_ci(checker, l, B, cache, now)
            if hq is not None:
                harq[0] = hq
            return delta, b, l, np.float32(a[1]), r

        def report(c):
            delta, b, l, fading, r = c
            acq.update(frame_start=start + delta, delta=delta, modulation=po.DQPSK if b == 2 else po.DBPSK, fading_index=fading,
                       success=r["success"], codewords_ok=r["codewords_ok"], codewords_failed=r["codewords_failed"],
                       frame_type=r["frame_type"], header_total_cw=r["header_total_cw"], frame_bytes=len(r["frame"]),
                       n_llr=len(l), frame=r["frame"], llr=l, cw0_deinterleaved=r["cw0_deinterleaved"], ci_tried=r["ci_tried"])

        cands = frame_candidates(disconnected and retry)
        primary = candidate(*cands[0])
        acq["candidates"] = 1
        report(primary)
        out["harq"] = harq[0]
        r = primary[4]
        if not r["success"] and pending == 0 and r["codewords_ok"] > 0:          # header salvage (:1631-1644)
            valid, _, total = parse_header(r["frame"])
            if valid and total > 1 and avail_cw < total:
                out["peek"] |= SALVAGE
                pending = total
                continue
        if not (r["success"] or r["codewords_ok"] > 0) and disconnected and retry:
            fits = lambda s: s >= 0 and s + n_span <= len(x)
            for delta, alt in cands[1:]:
                if not fits(start + delta):
                    continue
                c = candidate(delta, alt)
                acq["candidates"] += 1
                out["harq"] = harq[0]
                if c[4]["success"]:
                    report(c)
                    break
        out.update(outcome=DECODED, frame_len=n_span, pending_total_cw=pending, next_pos=acq["frame_start"] + n_span,
                   deliver=int(bool(acq["success"] or acq["codewords_ok"] > 0)), last_decoded_sync=acq["frame_start"])
        return out
