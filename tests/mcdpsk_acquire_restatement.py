"""CPU restatement of ria_gpu_mcdpsk_acquire_batch on the checkers (pyoracle.Oracle, or pyoracle.Ref where it is built):
StreamingDecoder's MC-DPSK path written out step by step (src/gui/modem/streaming_decoder.cpp):

1. detection on the search span: mcdpsk_wf_rx's detectDataSync (ZC) / detectSync (dual chirp); accepted iff detected,
   correlation >= min_confidence and the primary frame fits the window
2. the CFO mcdpsk_wf_rx demodulates with (the connected rule :903-917 included); every candidate is a fresh demodulator
   over frame_len samples at that CFO and phase 0
3. decodeMCDPSKFrame at R1/4 (:2595-2819) on robust_decode and ro_crc16
4. connected / no retry / success / codewords_ok > 0: done
5. disconnected: the alternate modulation (:1646-1690), then 12 deltas x (primary, alternate) (:1692-1797), first full
   success wins; candidates outside the window are skipped

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po

RETRY_DELTAS = (8, -8, 16, -16, 24, -24, 32, -32, 48, -48, 64, -64)
CONTROL_TYPES = (0x10, 0x11, 0x16, 0x17, 0x20, 0x21, 0x15, 0x40)
CONNECT, CONNECT_ACK, CONNECT_NAK, ACK = 0x12, 0x13, 0x14, 0x20
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = po.Oracle()
    return _oracle


def crc16(b):
    b = np.ascontiguousarray(b, np.uint8)
    return int(oracle().lib.ro_crc16(po.up(b), len(b)))


def frame_len(frame_cw, carriers, bps, spreading):
    """getMinSamplesForCWCount (mc_dpsk_waveform.cpp:470-485)"""
    return 9 * 512 + frame_cw * -(-648 // (carriers * bps)) * 512 * spreading


def frame_candidates(retry):
    """(delta, alternate?) in the reference's order"""
    c = [(0, False)]
    if retry:
        c.append((0, True))
        for d in RETRY_DELTAS:
            c += [(d, False), (d, True)]
    return c


# ---- frames (frame_v2.cpp): serialized v2 frames, split into R1/4 codewords, LDPC-encoded
def control_frame(ftype, seq, body=b""):
    """20-byte control frame: magic, type, flags 0, seq, 6 hash bytes, body up to 6 bytes, CRC16 over 18"""
    d = np.zeros(20, np.uint8)
    d[:6] = [0x55, 0x4C, ftype, 0, seq >> 8, seq & 255]
    d[6:12] = [0x12, 0x34, 0x56, 0x65, 0x43, 0x21]
    d[12:12 + len(body)] = np.frombuffer(bytes(body), np.uint8)[:6]
    c = crc16(d[:18])
    d[18], d[19] = c >> 8, c & 255
    return d


def data_frame(ftype, seq, payload, total_cw=None):
    """header (17) + payload + frame CRC; total_cw defaults to the codewords the frame takes (calculateCodewords)"""
    payload = np.asarray(payload, np.uint8)
    if total_cw is None:
        total_cw = -(-(17 + len(payload) + 2) * 8 // 162)
    h = np.zeros(17, np.uint8)
    h[:12] = [0x55, 0x4C, ftype, 0, seq >> 8, seq & 255, 0x12, 0x34, 0x56, 0x65, 0x43, 0x21]
    h[12], h[13], h[14] = total_cw, len(payload) >> 8, len(payload) & 255
    c = crc16(h[:15])
    h[15], h[16] = c >> 8, c & 255
    f = np.concatenate([h, payload])
    c = crc16(f)
    return np.concatenate([f, np.array([c >> 8, c & 255], np.uint8)])


def split_codewords(frame):
    """encodeFrameWithLDPC's split at R1/4 (frame_v2.cpp:1098-1130): CW0 = 20 bytes, CW1+ = 0xD5, index, 18 bytes"""
    cws = [np.zeros(20, np.uint8)]
    cws[0][:min(20, len(frame))] = frame[:20]
    off, i = 20, 1
    while off < len(frame):
        cw = np.zeros(20, np.uint8)
        cw[0], cw[1] = 0xD5, i
        chunk = frame[off:off + 18]
        cw[2:2 + len(chunk)] = chunk
        cws.append(cw)
        off += 18
        i += 1
    return cws


def encode_frame(frame):
    """coded bytes (81 per codeword) of a serialized frame at R1/4"""
    O = oracle()
    return np.concatenate([O.ldpc_encode(po.R1_4, np.concatenate([cw, np.zeros(1, np.uint8)])) for cw in split_codewords(frame)])


def window(checker, coded, carriers, mod, spreading, chirp, lead, window_len, kind, snr_db, seed, scale=0.8, shift=0):
    """lead zeros, the MC-DPSK waveform TX (chirp or ZC DATA preamble + modulated coded bytes) peak-normalised to
    `scale`, zeros to window_len, the checker's channel over the whole window.  coded None: noise only.  shift > 0 splices
    that many zeros between the preamble and the frame, shift < 0 drops the preamble's last -shift samples: the frame then
    starts `shift` samples away from where the detector places it (timing-recovery windows)."""
    w = np.zeros(window_len, np.float32)
    if coded is not None:
        s = checker.mcdpsk_wf_tx(carriers, mod, po.R1_4, spreading, not chirp, coded)
        if shift:
            n_pre = 57600 if chirp else 2512
            pre, body = s[:n_pre], s[n_pre:]
            s = np.concatenate([pre, np.zeros(shift, np.float32), body]) if shift > 0 else np.concatenate([pre[:shift], body])
        s = (s * np.float32(scale / np.abs(s).max())).astype(np.float32)
        n = min(len(s), window_len - lead)
        w[lead:lead + n] = s[:n]
    return checker.channel(kind, snr_db, int(seed), w)


# ---- the receiver
def decode_mcdpsk_frame(checker, llr):
    """decodeMCDPSKFrame at R1/4, raw path -> dict(success, codewords_ok, codewords_failed, frame_type, header_total_cw,
    frame)"""
    r = dict(success=0, codewords_ok=0, codewords_failed=0, frame_type=0x10, header_total_cw=0, frame=np.zeros(0, np.uint8))
    if len(llr) < 648:
        return r
    ok0, d0, _, _ = checker.robust_decode(po.R1_4, llr[:648])
    if not ok0 or len(d0) < 2 or d0[0] != 0x55 or d0[1] != 0x4C:
        return r
    d0 = np.asarray(d0[:20], np.uint8)
    t = int(d0[2])
    if t in CONTROL_TYPES:
        if crc16(d0[:18]) != (int(d0[18]) << 8 | int(d0[19])):
            return r
        total = 1
    else:
        if crc16(d0[:15]) != (int(d0[15]) << 8 | int(d0[16])):
            return r
        total = int(d0[12])
    if total == 0:                                    # undefined in the reference: treated as an invalid header
        return r
    if t in (CONNECT, CONNECT_ACK, CONNECT_NAK) and total < 3:
        return r
    r.update(frame_type=t, codewords_ok=1, header_total_cw=total)
    if total == 1:
        r.update(success=1, frame=d0)
        return r
    if len(llr) // 648 < total:
        r["frame"] = d0
        return r
    cws = [d0]
    for i in range(1, total):
        ok, d, _, _ = checker.robust_decode(po.R1_4, llr[i * 648:(i + 1) * 648])
        if ok and len(d) >= 20:
            cws.append(np.asarray(d[:20], np.uint8))
            r["codewords_ok"] += 1
        else:
            cws.append(None)
            r["codewords_failed"] += 1
    if r["codewords_failed"]:
        return r
    expected = 20 if t in CONTROL_TYPES else 17 + (int(d0[13]) << 8 | int(d0[14])) + 2
    out = []
    for i, cw in enumerate(cws):
        remaining = expected - len(out)
        if remaining == 0:
            break
        src = cw[2:] if (i and cw[0] == 0xD5) else cw
        out += list(src[:remaining])
    r.update(success=1, frame=np.array(out, np.uint8))
    return r


def acquire_window(checker, x, search_len, frame_cw, carriers=10, bps=1, spreading=1, chirp=True, disconnected=None,
                   known_cfo=0.0, detect_threshold=None, min_confidence=0.0, retry=True):
    """One window -> dict with the ria_mcdpsk_acq_result fields plus frame (bytes) and llr (the reported soft bits)"""
    if disconnected is None:
        disconnected = chirp
    x = np.ascontiguousarray(x, np.float32)
    mod = po.DBPSK if bps == 1 else po.DQPSK
    fl = frame_len(frame_cw, carriers, bps, spreading)
    thr = (0.15 if chirp else 0.2) if detect_threshold is None else detect_threshold
    sync4, _, aux5 = checker.mcdpsk_wf_rx(carriers, mod, po.R1_4, spreading, not chirp, x[:search_len], known_cfo, thr, fl)
    detected = bool(sync4[0])
    start = int(sync4[1]) if detected else -1
    corr = np.float32(sync4[2])
    fits = lambda s: s >= 0 and s + fl <= len(x)
    accepted = detected and not (corr < np.float32(min_confidence)) and fits(start)
    out = dict(detected=int(detected), accepted=int(accepted), sync_start=start, frame_start=-1, correlation=corr,
               cfo_hz=np.float32(0.0), fading_index=np.float32(0.0), delta=0, modulation=po.DQPSK if bps == 2 else po.DBPSK,
               candidates=0, success=0, codewords_ok=0, codewords_failed=0, frame_type=0x10, header_total_cw=0, frame_bytes=0,
               n_llr=0, frame=np.zeros(0, np.uint8), llr=np.zeros(0, np.float32))
    if not accepted:
        return out
    cfo = np.float32(sync4[3])
    if not disconnected and abs(known_cfo) > 0.01 and abs(np.float32(cfo) - np.float32(known_cfo)) > 1.0:   # :903-917
        cfo = np.float32(known_cfo)
    if isinstance(checker, po.Oracle):
        assert np.float32(aux5[3]) == cfo or (np.isnan(aux5[3]) and np.isnan(cfo))   # the CFO mcdpsk_wf_rx demodulated with
    out["cfo_hz"] = cfo

    def candidate(delta, alt):
        b = (3 - bps) if alt else bps
        s = start + delta
        llr, aux = checker.mcdpsk_demod(carriers, b, spreading, x[s:s + fl], float(cfo), 0.0)
        return delta, b, llr, np.float32(aux[1]), decode_mcdpsk_frame(checker, llr)

    def report(c):
        delta, b, llr, fading, r = c
        out.update(frame_start=start + delta, delta=delta, modulation=po.DQPSK if b == 2 else po.DBPSK, fading_index=fading,
                   success=r["success"], codewords_ok=r["codewords_ok"], codewords_failed=r["codewords_failed"],
                   frame_type=r["frame_type"], header_total_cw=r["header_total_cw"], frame_bytes=len(r["frame"]),
                   n_llr=len(llr), frame=r["frame"], llr=llr)

    cands = frame_candidates(disconnected and retry)
    primary = candidate(*cands[0])
    out["candidates"] = 1
    report(primary)
    r = primary[4]
    if r["success"] or r["codewords_ok"] > 0 or not (disconnected and retry):
        return out
    for delta, alt in cands[1:]:
        if not fits(start + delta):
            continue
        c = candidate(delta, alt)
        out["candidates"] += 1
        if c[4]["success"]:
            report(c)
            break
    return out
