"""CPU restatement of ria_gpu_rx_acquire_batch on the checkers (pyoracle.Oracle, or pyoracle.Ref where it is built):
StreamingDecoder's connected-mode OFDM data path written out step by step (src/gui/modem/streaming_decoder.cpp):

1. detectDataSync on the search span with the known CFO and the detect threshold (:723-735)
2. accepted iff detected and correlation >= min_confidence (:752-771) and the frame fits the window
3. process() at the found start with abs_position = abs_base + start, the known CFO and the burst marker (:891-897, :1345-1349)
4. decodeFixedFrame (:2936-2940)
5. if no codeword decoded: the same at +8, -8, +16, -16, +24, -24, +32, -32 (marker off, :1855-1965), first candidate
   with any codeword wins; candidates that do not fit the window are skipped

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po

RETRY_DELTAS = (8, -8, 16, -16, 24, -24, 32, -32)


def acquire_window(checker, mod, rate, x, search_len, known_cfo=0.0, detect_threshold=0.15, min_confidence=0.78, abs_base=0,
                   retry=True, ch_deint=True):
    """One window -> dict with the ria_acq_result fields plus info (bytes), cw_ok, iterations, attempts (None from Ref)
    and aux (the checker's demod status of the reported candidate, None if not accepted)."""
    geo = po_oracle(checker).geom(mod, rate)
    fs, bps, ib = geo.frame_samples, geo.bits_per_symbol, 4 * geo.bytes_per_cw
    x = np.ascontiguousarray(x, np.float32)
    if isinstance(checker, po.Ref):
        det = checker.detect_data_sync(x[:search_len], known_cfo, detect_threshold, mod, rate)
    else:
        det = checker.detect_data_sync(x[:search_len], known_cfo, detect_threshold)
    detected, corr, burst = bool(det[0]), np.float32(det[2]), int(det[3]) if det[0] else 0
    start = int(det[1]) if detected else -1
    fits = lambda s: s >= 0 and s + fs <= len(x)
    accepted = detected and not (corr < np.float32(min_confidence)) and fits(start)
    out = dict(detected=int(detected), accepted=int(accepted), sync_start=start, frame_start=-1, correlation=corr,
               cfo_hz=np.float32(0.0), delta=0, candidates=0, burst_interleaved=burst, info=np.zeros(ib, np.uint8),
               cw_ok=np.zeros(4, np.uint8), iterations=np.zeros(4, np.uint16), attempts=np.zeros(4, np.uint8), aux=None)
    if not accepted:
        return out

    def candidate(delta, marker):
        s = start + delta
        seg = x[s:s + fs]
        if isinstance(checker, po.Ref):
            assert not marker, "the reference shim's process() has no burst-marker input"
            llr, aux, _, _ = checker.rx_process(mod, rate, seg, float(known_cfo), abs_base + s)
            data, ok = checker.decode_fixed_frame(llr, rate, ch_deint, bps)
            return data[:ib], ok, None, None, np.float32(aux[1]), aux
        llr, aux = checker.rx_process(mod, rate, seg, float(known_cfo), abs_base + s, burst_marker=marker)
        data, ok, iters, att = checker.decode_fixed_frame(llr, rate, ch_deint, bps, flags=7)
        return data, ok, iters.astype(np.uint16), att.astype(np.uint8), np.float32(aux.cfo_hz), aux

    def report(delta, c):
        data, ok, iters, att, cfo, aux = c
        out.update(frame_start=start + delta, delta=delta, info=np.asarray(data, np.uint8), cw_ok=np.asarray(ok, np.uint8),
                   iterations=iters, attempts=att, cfo_hz=cfo, aux=aux)

    primary = candidate(0, bool(burst))
    out["candidates"] = 1
    report(0, primary)
    if primary[1].any() or not retry:
        return out
    for d in RETRY_DELTAS:
        if not fits(start + d):
            continue
        c = candidate(d, False)
        out["candidates"] += 1
        if c[1].any():
            report(d, c)
            break
    return out


_geom_oracle = None


def po_oracle(checker):
    """An Oracle for the frame geometry (Ref has no geom())."""
    global _geom_oracle
    if isinstance(checker, po.Oracle):
        return checker
    if _geom_oracle is None:
        _geom_oracle = po.Oracle()
    return _geom_oracle


def window(checker, mod, rate, payload, seq, lead, window_len, kind, snr_db, seed, two_ray=None, negate_first_lts=False,
           frame_scale=0.8):
    """A window built on the CPU: oracle TX (peak-normalised to frame_scale) at sample `lead` of window_len zeros,
    optional two-ray copy (delay, gain) of the frame added, optional negated first LTS symbol (burst marker), then the
    checker's channel over the whole window.  lead = None: no frame (noise only).  Returns (window, sent info)."""
    w = np.zeros(window_len, np.float32)
    info = None
    if lead is not None:
        s, info, _ = checker.tx_frame(mod, rate, payload, seq)[:3]
        s = (s * np.float32(frame_scale / np.abs(s).max())).astype(np.float32)
        if negate_first_lts:
            s[:1152] = -s[:1152]
        n = min(len(s), window_len - lead)
        w[lead:lead + n] = s[:n]
        if two_ray is not None:
            d, gain = two_ray
            m = min(len(s), window_len - lead - d)
            w[lead + d:lead + d + m] += np.float32(gain) * s[:m]
    return checker.channel(kind, snr_db, int(seed), w), info
