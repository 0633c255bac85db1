"""CPU restatement of the HARQ calls (ria_gpu_mcdpsk_decode_frame_batch, ria_gpu_mcdpsk_acquire_harq_batch):

- ChaseCache: fec::ChaseCache (src/fec/chase_cache.{hpp,cpp}) in plain Python, method for method.  Time is the caller's
  (now_ms per call, a uint64); expiry is (int64)(now - last_access) > ttl, the difference taken modulo 2^64 as
  include/ria_gpu.h states it; eviction takes the smallest (last_access, store sequence number), which is the reference's
  "smallest last_access" made definite for equal times.
- decode_mcdpsk_frame: tests/mcdpsk_acquire_restatement.py's with the chase statements (streaming_decoder.cpp:2729-2731,
  :2766-2789, :2796-2799, :2808-2811); with cache None it is that function.  The soft bits handed to the robust decoder go
  through canon() (the decoder's input mapping, tests/ldpc_domain_inputs.py); what the cache stores and sums is raw.
- acquire_window: that file's with a cache that persists across calls; every candidate goes through the cache.

Test infrastructure only (not collected: no test_ prefix)."""
import numpy as np

import pyoracle as po
from mcdpsk_acquire_restatement import CONNECT, CONNECT_ACK, CONNECT_NAK, CONTROL_TYPES, crc16, frame_candidates, frame_len

MAX_COMBINES, LDPC_BLOCK = 4, 648
STATS = ("cache_hits", "cache_misses", "stores", "combines", "entries_evicted", "entries_expired", "recoveries")


def age_ms(now, last_access):
    """now - last_access modulo 2^64, read as int64 (chase_policy.hpp's chase_expired)"""
    d = (int(now) - int(last_access)) & (2 ** 64 - 1)
    return d - 2 ** 64 if d >= 2 ** 63 else d


def canon(x):
    """the decoder's input mapping (include/ria_gpu.h; tests/ldpc_domain_inputs.canon): NaN -> +1e30, clamp to +-1e30,
    -0.0 -> +0.0"""
    x = np.array(x, np.float32, copy=True)
    x[np.isnan(x)] = np.float32(1e30)
    x = np.clip(x, np.float32(-1e30), np.float32(1e30))
    x[x == 0] = np.float32(0.0)
    return x


class Entry:
    def __init__(self, key, total_cw, frame_type, now, order):
        self.key, self.total_cw, self.frame_type = key, total_cw, frame_type
        self.soft = [None] * total_cw              # cw_soft_bits: None = empty
        self.count = [0] * total_cw
        self.decoded = [False] * total_cw
        self.last_access, self.order = now, order


class ChaseCache:
    def __init__(self, max_entries=16, ttl_ms=30000):
        self.max_entries, self.ttl = max_entries, ttl_ms
        self.cache = {}
        self.stats = dict.fromkeys(STATS, 0)
        self.seq = 0

    def store(self, key, cw, soft, total_cw, frame_type, now):
        if len(soft) != LDPC_BLOCK:
            return False
        if cw < 0 or cw >= total_cw:
            return False
        if total_cw <= 0 or total_cw > 16:
            return False
        self.stats["stores"] += 1
        self.seq += 1
        self.prune_expired(now)
        e = self.cache.get(key)
        if e is None:
            self.evict_if_needed()
            e = Entry(key, total_cw, frame_type, now, self.seq)
            e.soft[cw] = np.array(soft, np.float32)
            e.count[cw] = 1
            self.cache[key] = e
            return True
        e.last_access, e.order = now, self.seq
        if cw >= e.total_cw:
            return False
        if e.decoded[cw]:
            return False
        if e.count[cw] >= MAX_COMBINES:
            return False
        if e.soft[cw] is None:
            e.soft[cw] = np.array(soft, np.float32)
            e.count[cw] = 1
        else:
            with np.errstate(all="ignore"):            # inf + -inf and overflow are part of the domain
                e.soft[cw] = (e.soft[cw] + np.asarray(soft, np.float32)).astype(np.float32)   # one float add per element
            e.count[cw] += 1
            self.stats["combines"] += 1
        return True

    def get_combined(self, key, cw):
        e = self.cache.get(key)
        if e is None or cw < 0 or cw >= len(e.soft) or e.soft[cw] is None or e.decoded[cw]:
            self.stats["cache_misses"] += 1
            return None
        self.stats["cache_hits"] += 1
        return e.soft[cw]

    def get_combine_count(self, key, cw):
        e = self.cache.get(key)
        if e is None or cw < 0 or cw >= len(e.count):
            return 0
        return e.count[cw]

    def mark_decoded(self, key, cw):
        e = self.cache.get(key)
        if e is None:
            return
        if 0 <= cw < len(e.decoded):
            e.decoded[cw] = True
            e.soft[cw] = None
        if all(e.decoded):
            del self.cache[key]

    def remove_entry(self, key):
        return self.cache.pop(key, None) is not None

    def clear(self):
        self.cache.clear()

    def size(self):
        return len(self.cache)

    def increment_recoveries(self):
        self.stats["recoveries"] += 1

    def evict_if_needed(self):
        while len(self.cache) >= self.max_entries:
            oldest = min(self.cache.values(), key=lambda e: (e.last_access, e.order))
            del self.cache[oldest.key]
            self.stats["entries_evicted"] += 1

    def prune_expired(self, now):
        for k in [k for k, e in self.cache.items() if age_ms(now, e.last_access) > self.ttl]:
            del self.cache[k]
            self.stats["entries_expired"] += 1


def header_key(d0):
    """(seq, src_hash, dst_hash) of parseHeader (frame_v2.cpp:1213-1223)"""
    d = [int(v) for v in d0[:12]]
    return (d[4] << 8 | d[5], d[6] << 16 | d[7] << 8 | d[8], d[9] << 16 | d[10] << 8 | d[11])


def empty_harq():
    return dict(valid=0, seq=0, src_hash=0, dst_hash=0, stored_mask=0, sum_mask=0, recovered_mask=0, max_combine=0, entry=0)


def decode_mcdpsk_frame(checker, llr, cache=None, now=0, wrong_order=False):
    """decodeMCDPSKFrame at R1/4, raw path, chase enabled iff cache is not None -> (DecodeResult dict, harq dict or None;
    None: no valid header met a cache).  wrong_order: "store all failures, then mark all successes", the batching the
    ordering trap forbids (for the test that shows it differs)."""
    r = dict(success=0, codewords_ok=0, codewords_failed=0, frame_type=0x10, header_total_cw=0, frame=np.zeros(0, np.uint8))
    llr = np.asarray(llr, np.float32)
    if len(llr) < 648:
        return r, None
    ok0, d0, _, _ = checker.robust_decode(po.R1_4, canon(llr[:648]))
    if not ok0 or len(d0) < 2 or d0[0] != 0x55 or d0[1] != 0x4C:
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
    if len(llr) // 648 < total:
        r["frame"] = d0
        return r, hq
    cws = [d0]
    deferred_marks = []
    for i in range(1, total):
        soft = llr[i * 648:(i + 1) * 648]
        ok, d, _, _ = checker.robust_decode(po.R1_4, canon(soft))
        if not ok and cache is not None:
            if cache.store(key, i, soft, total, t, now):
                hq["stored_mask"] |= 1 << i
            combined = cache.get_combined(key, i)
            count = cache.get_combine_count(key, i)
            hq["max_combine"] = max(hq["max_combine"], count)
            if combined is not None and len(combined) == 648 and count > 1:
                hq["sum_mask"] |= 1 << i
                ok_c, d_c, _, _ = checker.robust_decode(po.R1_4, canon(combined))
                if ok_c and len(d_c) >= 20:
                    ok, d = True, d_c
                    cache.mark_decoded(key, i)
                    cache.increment_recoveries()
                    hq["recovered_mask"] |= 1 << i
        if ok and len(d) >= 20:
            cws.append(np.asarray(d[:20], np.uint8))
            r["codewords_ok"] += 1
            if cache is not None:
                if wrong_order:
                    deferred_marks.append(i)
                else:
                    cache.mark_decoded(key, i)
        else:
            cws.append(None)
            r["codewords_failed"] += 1
    for i in deferred_marks:
        cache.mark_decoded(key, i)
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


def acquire_window(checker, x, search_len, frame_cw, cache=None, now=0, carriers=10, bps=1, spreading=1, chirp=True, disconnected=None,
                   known_cfo=0.0, detect_threshold=None, min_confidence=0.0, retry=True):
    """mcdpsk_acquire_restatement.acquire_window with the cache: one window -> (dict with the ria_mcdpsk_acq_result fields
    plus frame and llr, harq dict of the window's last candidate in which a valid header met the cache)"""
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
        r, hq = decode_mcdpsk_frame(checker, llr, cache, now)
        if hq is not None:
            harq[0] = hq
        return delta, b, llr, np.float32(aux[1]), r

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


def cache_snapshot(cache):
    """{key: (total_cw, frame_type, last_access, counts, decoded, has_sum, sums [total_cw, 648])} for comparisons with
    ria_gpu_chase_export"""
    out = {}
    for k, e in cache.cache.items():
        sums = np.zeros((16, 648), np.float32)
        for i, s in enumerate(e.soft):
            if s is not None:
                sums[i] = s
        out[k] = dict(total_cw=e.total_cw, frame_type=e.frame_type, last_access=e.last_access, order=e.order,
                      count=list(e.count) + [0] * (16 - e.total_cw), decoded=[int(v) for v in e.decoded] + [0] * (16 - e.total_cw),
                      has_sum=[int(s is not None) for s in e.soft] + [0] * (16 - e.total_cw), sums=sums)
    return out
