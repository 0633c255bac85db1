"""CPU restatement of MC-DPSK channel interleaving (ria_gpu_mcdpsk_decode_frame_ci_batch, ria_gpu_mcdpsk_acquire_ci_batch,
ria_gpu_mcdpsk_interleave_batch):

- deinterleave / interleave_bytes: ChannelInterleaver(B, 648) (ldpc_decoder.cpp:552-650) in numpy.
- decode_mcdpsk_frame_ci: decodeMCDPSKFrame at R1/4 (streaming_decoder.cpp:2595-2819) with the
  use_mc_dpsk_channel_interleave_ statements (:2614-2623, :2651-2672, :2741, :2764, :2778) and the chase statements, on
  checker.robust_decode.  B None: the mode is off and the function is mcdpsk_harq_restatement.decode_mcdpsk_frame.
- acquire_window_ci: mcdpsk_harq_restatement.acquire_window with every candidate decoded that way, all with the caller's B.

Test infrastructure only (not collected: no test_ prefix)."""
from math import gcd

import numpy as np

import pyoracle as po
from mcdpsk_acquire_restatement import CONNECT, CONNECT_ACK, CONNECT_NAK, CONTROL_TYPES, crc16, frame_candidates, frame_len
from mcdpsk_harq_restatement import empty_harq, header_key

N = 648


def coprime_step(B, total=N):
    """findCoprimeStep (ldpc_decoder.cpp:552-577)"""
    target = B * 3
    if target >= total:
        target = total // 2
    for s in range(target, total):
        if gcd(s, total) == 1:
            return s
    for s in range(B + 1, total):
        if gcd(s, total) == 1:
            return s
    return B + 1


def permutation(B):
    """p[i] = (i * step) % 648: deinterleave(x) = x[p], interleave(bits)[p] = bits"""
    return (np.arange(N, dtype=np.int64) * coprime_step(B)) % N


def deinterleave(x, B):
    return np.ascontiguousarray(np.asarray(x)[permutation(B)])


def interleave_bytes(coded, B):
    """ChannelInterleaver::interleave(Bytes) on every 81 bytes of coded (MSB first)"""
    coded = np.ascontiguousarray(coded, np.uint8)
    bits = np.unpackbits(coded.reshape(-1, 81), axis=1)
    out = np.zeros_like(bits)
    out[:, permutation(B)] = bits
    return np.packbits(out, axis=1).reshape(coded.shape)


def _magic(ok, d):
    return bool(ok) and len(d) >= 2 and d[0] == 0x55 and d[1] == 0x4C


def decode_mcdpsk_frame_ci(checker, llr, B=None, cache=None, now=0):
    """-> (DecodeResult dict with cw0_deinterleaved and ci_tried, harq dict or None)"""
    r = dict(success=0, codewords_ok=0, codewords_failed=0, frame_type=0x10, header_total_cw=0, frame=np.zeros(0, np.uint8),
             cw0_deinterleaved=0, ci_tried=0)
    llr = np.asarray(llr, np.float32)
    if len(llr) < N:
        return r, None

    def decode_cw(soft, deint):
        return checker.robust_decode(po.R1_4, deinterleave(soft, B) if deint else np.ascontiguousarray(soft))[:2]

    ok0, d0 = decode_cw(llr[:N], False)
    deint = False
    if not _magic(ok0, d0) and B is not None:
        r["ci_tried"] = 1
        ok_i, d_i = decode_cw(llr[:N], True)
        if _magic(ok_i, d_i):
            ok0, d0, deint = True, d_i, True
            r["cw0_deinterleaved"] = 1
    if not _magic(ok0, d0):
        return r, None
    d0 = np.asarray(d0[:20], np.uint8)
    t = int(d0[2])
    if t in CONTROL_TYPES:
        if crc16(d0[:18]) != (int(d0[18]) << 8 | int(d0[19])):
            return r, None
        total = 1
    else:
        if crc16(d0[:15]) != (int(d0[15]) << 8 | int(d0[16])):
            return r, None
        total = int(d0[12])
    if total == 0:
        return r, None
    if t in (CONNECT, CONNECT_ACK, CONNECT_NAK) and total < 3:
        return r, None
    r.update(frame_type=t, codewords_ok=1, header_total_cw=total)
    key = header_key(d0)
    hq = None
    if cache is not None:
        hq = empty_harq()
        hq.update(valid=1, seq=key[0], src_hash=key[1], dst_hash=key[2])
    if total == 1:
        r.update(success=1, frame=d0)
        return r, hq
    if len(llr) // N < total:
        r["frame"] = d0
        return r, hq
    cws = [d0]
    for i in range(1, total):
        soft = llr[i * N:(i + 1) * N]
        ok, d = decode_cw(soft, deint)
        if not ok and cache is not None:
            if cache.store(key, i, soft, total, t, now):               # the raw soft bits (:2769-2770)
                hq["stored_mask"] |= 1 << i
            combined = cache.get_combined(key, i)
            count = cache.get_combine_count(key, i)
            hq["max_combine"] = max(hq["max_combine"], count)
            if combined is not None and len(combined) == N and count > 1:
                hq["sum_mask"] |= 1 << i
                ok_c, d_c = decode_cw(combined, deint)                 # (:2778)
                if ok_c and len(d_c) >= 20:
                    ok, d = True, d_c
                    cache.mark_decoded(key, i)
                    cache.increment_recoveries()
                    hq["recovered_mask"] |= 1 << i
        if ok and len(d) >= 20:
            cws.append(np.asarray(d[:20], np.uint8))
            r["codewords_ok"] += 1
            if cache is not None:
                cache.mark_decoded(key, i)
        else:
            cws.append(None)
            r["codewords_failed"] += 1
    if r["codewords_failed"]:
        if cache is not None:
            hq["entry"] = 1 if key in cache.cache else 0
        return r, hq
    expected = 20 if t in CONTROL_TYPES else 17 + (int(d0[13]) << 8 | int(d0[14])) + 2
    out = []
    for i, cw in enumerate(cws):
        remaining = expected - len(out)
        if remaining == 0:
            break
        src = cw[2:] if (i and cw[0] == 0xD5) else cw
        out += list(src[:remaining])
    r.update(success=1, frame=np.array(out, np.uint8))
    if cache is not None:
        hq["entry"] = 2 if cache.remove_entry(key) else 0
    return r, hq


def acquire_window_ci(checker, x, search_len, frame_cw, B=None, cache=None, now=0, carriers=10, bps=1, spreading=1, chirp=True,
                      disconnected=None, known_cfo=0.0, detect_threshold=None, min_confidence=0.0, retry=True):
    """One window -> (dict with the ria_mcdpsk_acq_result fields, frame, llr, cw0_deinterleaved and ci_tried of the reported
    candidate; harq dict of the window's last candidate in which a valid header met the cache).  Every candidate uses B."""
    if disconnected is None:
        disconnected = chirp
    x = np.ascontiguousarray(x, np.float32)
    mod = po.DBPSK if bps == 1 else po.DQPSK
    fl = frame_len(frame_cw, carriers, bps, spreading)
    thr = (0.15 if chirp else 0.2) if detect_threshold is None else detect_threshold
    sync4, _, _ = checker.mcdpsk_wf_rx(carriers, mod, po.R1_4, spreading, not chirp, x[:search_len], known_cfo, thr, fl)
    detected = bool(sync4[0])
    start = int(sync4[1]) if detected else -1
    corr = np.float32(sync4[2])
    fits = lambda s: s >= 0 and s + fl <= len(x)
    accepted = detected and not (corr < np.float32(min_confidence)) and fits(start)
    out = dict(detected=int(detected), accepted=int(accepted), sync_start=start, frame_start=-1, correlation=corr,
               cfo_hz=np.float32(0.0), fading_index=np.float32(0.0), delta=0, modulation=po.DQPSK if bps == 2 else po.DBPSK,
               candidates=0, success=0, codewords_ok=0, codewords_failed=0, frame_type=0x10, header_total_cw=0, frame_bytes=0,
               n_llr=0, frame=np.zeros(0, np.uint8), llr=np.zeros(0, np.float32), cw0_deinterleaved=0, ci_tried=0)
    harq = [empty_harq()]
    if not accepted:
        return out, harq[0]
    cfo = np.float32(sync4[3])
    if not disconnected and abs(known_cfo) > 0.01 and abs(np.float32(cfo) - np.float32(known_cfo)) > 1.0:
        cfo = np.float32(known_cfo)
    out["cfo_hz"] = cfo

    def candidate(delta, alt):
        b = (3 - bps) if alt else bps
        s = start + delta
        llr, aux = checker.mcdpsk_demod(carriers, b, spreading, x[s:s + fl], float(cfo), 0.0)
        r, hq = decode_mcdpsk_frame_ci(checker, llr, B, cache, now)
        if hq is not None:
            harq[0] = hq
        return delta, b, llr, np.float32(aux[1]), r

    def report(c):
        delta, b, llr, fading, r = c
        out.update(frame_start=start + delta, delta=delta, modulation=po.DQPSK if b == 2 else po.DBPSK, fading_index=fading,
                   success=r["success"], codewords_ok=r["codewords_ok"], codewords_failed=r["codewords_failed"],
                   frame_type=r["frame_type"], header_total_cw=r["header_total_cw"], frame_bytes=len(r["frame"]),
                   n_llr=len(llr), frame=r["frame"], llr=llr, cw0_deinterleaved=r["cw0_deinterleaved"], ci_tried=r["ci_tried"])

    cands = frame_candidates(disconnected and retry)
    primary = candidate(*cands[0])
    out["candidates"] = 1
    report(primary)
    r = primary[4]
    if r["success"] or r["codewords_ok"] > 0 or not (disconnected and retry):
        return out, harq[0]
    for delta, alt in cands[1:]:
        if not fits(start + delta):
            continue
        c = candidate(delta, alt)
        out["candidates"] += 1
        if c[4]["success"]:
            report(c)
            break
    return out, harq[0]
