"""StreamingDecoder::feedAudio (src/gui/modem/streaming_decoder.cpp:184-291, whole) and searchForSync (:386-941) restated
statement for statement in numpy float32 on a LITERAL 960 000-float buffer_, on the oracle's detectors, under the time model
of ria_gpu_search_ring_batch (include/ria_gpu.h): one invocation = one searchForSync(); after every invocation that leaves
the stream open, min(feed_step, capture_len - total_fed) samples arrive through the whole of feedAudio.  feed() writes the
buffer sample by sample modulo the ring (:281-284) and every read is buffer_[(pos + i) % 960000]: nothing here knows the
closed form the kernels read the capture through (ria_amd/csrc/ring_rules.hpp), which tests/test_ring_cpu.py checks against
this buffer.  A state given with total_fed > 0 is reached by writing x[0:total_fed] through the same loop first.

Before the wrap a cursor ahead of total_fed is a wait (ria_gpu_search_batch's documented limit, kept).  Not restated (the
library leaves them out too): the ZC-miss -> chirp fallback (:785-828).  Test infrastructure (no test_ prefix)."""
import numpy as np

import search_restatement as SR
from search_restatement import (CHIRP, COHERENT_PSK, COHERENT_QAM, DIFFERENTIAL, LIMIT, LTS, NEED_SAMPLES, SYNC_FOUND, ZC, ZC_MODE, Trace, confidence,  # noqa: F401
                                min_search_of, modulation_class, std_clamp, std_max, std_min)

F = np.float32
MAX_BUFFER_SAMPLES = 960000
CORRELATION_STEP = 4800
CORR_INVARIANT_GUARD = 9600
OVERFLOW_RECOVERY_KEEP = 360000
NO_LAST_SYNC = -2 ** 31            # SIZE_MAX

STATE = np.dtype([("total_fed", "<i8"), ("correlation_pos", "<i4"), ("reject_streak", "<i4"), ("noise_floor", "<f4"), ("last_cfo_hz", "<f4"),
                  ("fading_hint", "<f4"), ("snr_hint", "<f4"), ("last_decoded_sync_pos", "<i4"), ("overflow_events", "<u4"), ("overflow_dropped", "<u8")])
RESULT = np.dtype(SR.RESULT.descr + [("abs_search_start", "<i8"), ("overflow_dropped", "<u8"), ("overflows", "<u4"), ("drift_snaps", "<u4"),
                                     ("cursor_inits", "<u4"), ("span_wraps", "<u4")])
assert STATE.itemsize == 48 and RESULT.itemsize == 144


def fresh_state(n, total_fed=0):
    s = np.zeros(n, STATE)
    s["total_fed"] = total_fed
    s["noise_floor"] = F(0.001)
    s["last_decoded_sync_pos"] = NO_LAST_SYNC
    return s


def from_search_state(s):
    """a SR.STATE record (or array) as a ring state: the same decoder before the wrap"""
    s = np.atleast_1d(s)
    out = fresh_state(len(s))
    out["total_fed"] = s["fed"]
    for f in ("correlation_pos", "reject_streak", "noise_floor", "last_cfo_hz", "fading_hint", "snr_hint", "last_decoded_sync_pos"):
        out[f] = s[f]
    return out


def to_search_state(s):
    s = np.atleast_1d(s)
    out = np.zeros(len(s), SR.STATE)
    out["fed"] = s["total_fed"]
    for f in ("correlation_pos", "reject_streak", "noise_floor", "last_cfo_hz", "fading_hint", "snr_hint", "last_decoded_sync_pos"):
        out[f] = s[f]
    return out


class Ring:
    """buffer_ and write_pos_ (:281-284)"""

    def __init__(self):
        self.buffer = np.zeros(MAX_BUFFER_SAMPLES, F)
        self.write_pos = 0

    def write(self, samples):
        # for (i < count) { buffer_[write_pos_] = samples[i]; write_pos_ = (write_pos_ + 1) % MAX; } in pieces that end at the ring's end
        i = 0
        while i < len(samples):
            n = min(len(samples) - i, MAX_BUFFER_SAMPLES - self.write_pos)
            self.buffer[self.write_pos:self.write_pos + n] = samples[i:i + n]
            self.write_pos = (self.write_pos + n) % MAX_BUFFER_SAMPLES
            i += n

    def read(self, pos, n):
        """buffer_[(pos + i) % MAX] for i < n"""
        return self.buffer[(pos + np.arange(n)) % MAX_BUFFER_SAMPLES]


def ring_of(x, total_fed):
    r = Ring()
    r.write(np.ascontiguousarray(x[:total_fed], F))
    return r


def search(O, x, capture_len, state, mode, cls, connected, feed_step, max_invocations, trace=None):
    """One stream.  state: one STATE record (not modified).  -> (RESULT record, STATE record)"""
    x = np.ascontiguousarray(x, F)
    hit = trace.hit if trace is not None else (lambda what: None)
    corr_pos, total_fed = int(state["correlation_pos"]), int(state["total_fed"])
    noise_floor_, streak = F(state["noise_floor"]), int(state["reject_streak"])
    last_cfo, fading_hint, snr_hint = F(state["last_cfo_hz"]), F(state["fading_hint"]), F(state["snr_hint"])
    last_decoded = int(state["last_decoded_sync_pos"])
    overflow_events_, overflow_total = int(state["overflow_events"]), int(state["overflow_dropped"])
    assert 0 <= total_fed <= capture_len <= min(len(x), 2 ** 31 - 1 - MAX_BUFFER_SAMPLES) and 0 <= corr_pos < MAX_BUFFER_SAMPLES and streak >= 0
    assert last_decoded == NO_LAST_SYNC or 0 <= last_decoded < MAX_BUFFER_SAMPLES
    ring = ring_of(x, total_fed)
    min_search = min_search_of(mode)
    connected_ = True if mode != CHIRP else bool(connected)
    connected_light_sync = mode != CHIRP
    connected_zc_mode = mode == ZC
    is_zc_mode = cls == ZC_MODE
    is_coherent = cls in (COHERENT_PSK, COHERENT_QAM)
    r = np.zeros((), RESULT)
    r["search_len"] = min_search
    r["sync_position"] = r["abs_position"] = r["marker"] = r["root"] = -1

    def feed():
        """feedAudio(chunk) for the samples that can still arrive; False when none can"""
        nonlocal corr_pos, total_fed, streak, overflow_events_, overflow_total
        count = min(feed_step, capture_len - total_fed)
        if count <= 0:                                   # :185
            return False
        write_pos = ring.write_pos
        assert write_pos == total_fed % MAX_BUFFER_SAMPLES

        def compute_unsearched(write_pos, corr):         # :193-202
            if total_fed < MAX_BUFFER_SAMPLES:
                return write_pos - corr if write_pos >= corr else 0
            return write_pos - corr if write_pos >= corr else MAX_BUFFER_SAMPLES - corr + write_pos

        if total_fed < MAX_BUFFER_SAMPLES and corr_pos > write_pos:      # :204-225
            corr_pos = write_pos
            streak = 0
            hit("feed_clamp")
        unsearched = compute_unsearched(write_pos, corr_pos)
        hit("unsearched_prewrap" if total_fed < MAX_BUFFER_SAMPLES else ("unsearched_ahead" if write_pos >= corr_pos else "unsearched_behind"))
        if total_fed >= MAX_BUFFER_SAMPLES and unsearched > MAX_BUFFER_SAMPLES - CORR_INVARIANT_GUARD:    # :232-238
            corr_pos = write_pos
            unsearched = 0
            r["drift_snaps"] += 1
            hit("drift_guard")
        if unsearched + count >= MAX_BUFFER_SAMPLES:     # :242-278
            incoming_total = unsearched + count
            target_after_write = min(OVERFLOW_RECOVERY_KEEP, MAX_BUFFER_SAMPLES - 1)
            need_to_drop = 0
            if incoming_total > target_after_write:
                need_to_drop = min(unsearched, incoming_total - target_after_write)
            hit("overflow_drop_all" if need_to_drop == unsearched else "overflow_drop_part")
            corr_pos = (corr_pos + need_to_drop) % MAX_BUFFER_SAMPLES
            overflow_events_ = (overflow_events_ + 1) & 0xFFFFFFFF
            overflow_total += need_to_drop
            r["overflows"] += 1
            r["overflow_dropped"] += need_to_drop
        before = total_fed
        ring.write(x[total_fed:total_fed + count])       # :281-284
        total_fed += count                               # :286
        if before < MAX_BUFFER_SAMPLES <= total_fed:
            hit("feed_crosses_wrap")
            if before == MAX_BUFFER_SAMPLES - 1:
                hit("feed_from_959999")
        if total_fed == MAX_BUFFER_SAMPLES:
            hit("total_exactly_ring")
        if total_fed >= MAX_BUFFER_SAMPLES and ring.write_pos == 0:
            hit("write_pos_zero_at_multiple")
        if total_fed < MAX_BUFFER_SAMPLES and corr_pos > ring.write_pos:   # :289-291
            corr_pos = ring.write_pos
            hit("feed_clamp_after")
        return True

    def ring_pos_to_absolute(ring_pos):                  # :862-874
        if total_fed < MAX_BUFFER_SAMPLES:
            return ring_pos
        oldest_abs = total_fed - MAX_BUFFER_SAMPLES
        oldest_pos = ring.write_pos
        if ring_pos >= oldest_pos:
            hit("abs_at_or_after_write_pos")
            offset = ring_pos - oldest_pos
        else:
            hit("abs_before_write_pos")
            offset = MAX_BUFFER_SAMPLES - oldest_pos + ring_pos
        return oldest_abs + offset

    outcome = 0
    with np.errstate(all="ignore"):
        while True:
            if int(r["invocations"]) >= max_invocations:
                outcome = LIMIT
                if total_fed >= MAX_BUFFER_SAMPLES:
                    hit("limit_after_wrap")
                break
            r["invocations"] += 1
            write_pos = ring.write_pos
            if total_fed == MAX_BUFFER_SAMPLES:
                hit("total_exactly_ring")
            if total_fed >= MAX_BUFFER_SAMPLES and write_pos == 0:
                hit("write_pos_zero_at_multiple")
            # ---- the waits (:449-481) with the cursor initialisation between them (:458-464)
            waiting = total_fed < min_search            # :449
            if not waiting:
                if corr_pos == 0 and total_fed > 0:
                    if total_fed < MAX_BUFFER_SAMPLES:
                        corr_pos = 0
                    else:
                        corr_pos = write_pos             # :462
                        r["cursor_inits"] += 1
                        hit("cursor_init_after_wrap")
                if write_pos >= corr_pos:
                    unsearched = write_pos - corr_pos
                else:
                    unsearched = MAX_BUFFER_SAMPLES - corr_pos + write_pos
                    hit("unsearched_circular")
                if total_fed < MAX_BUFFER_SAMPLES and corr_pos > write_pos:
                    waiting = True                       # the library's limit: the reference reads unwritten ring samples
                elif unsearched < min_search:
                    waiting = True
                    if total_fed >= MAX_BUFFER_SAMPLES:
                        hit("wait_after_wrap")
            if waiting:
                r["waits"] += 1
                if not feed():
                    outcome = NEED_SAMPLES
                    hit("wait_unresolved")
                    if total_fed >= MAX_BUFFER_SAMPLES:      # :475 on either branch of :468-472 (:449 cannot fire after the wrap)
                        hit("need_samples_after_wrap_linear" if write_pos >= corr_pos else "need_samples_after_wrap_circular")
                    break
                hit("wait_fed")
                continue
            # ---- ZC backlog catch-up (:488-522)
            if connected_zc_mode:
                scaled_unsearched = (unsearched * 10) // min_search
                if scaled_unsearched > 25:
                    if write_pos < min_search + 4800:
                        hit("severe_snap_wraps_back")
                    if write_pos < corr_pos:
                        hit("severe_circular")
                    corr_pos = (write_pos + MAX_BUFFER_SAMPLES - min_search - 4800) % MAX_BUFFER_SAMPLES
                    r["catchups_severe"] += 1
                elif scaled_unsearched > 15:
                    if write_pos < corr_pos:
                        hit("moderate_circular")
                    excess = unsearched - min_search
                    catch_up = max(min(excess // 2, 24000), 4800)
                    corr_pos = (corr_pos + catch_up) % MAX_BUFFER_SAMPLES
                    r["catchups_moderate"] += 1
            # ---- RMS, tracker, gate (:525-573)
            if corr_pos > MAX_BUFFER_SAMPLES - 1000:
                hit("rms_straddles_ring_end")
            seg = ring.read(corr_pos, 1000)
            rms = np.cumsum(seg * seg, dtype=F)[-1]      # rms += s * s, ascending, float32
            rms = F(np.sqrt(rms / F(1000.0)))
            noise_floor = std_max(F(0.001), noise_floor_)
            if rms < noise_floor * F(3.0):
                noise_floor_ = F(0.98) * noise_floor + F(0.02) * rms
            else:
                noise_floor_ = F(0.995) * noise_floor + F(0.005) * rms
            if connected_light_sync:
                rms_gate = std_clamp(noise_floor_ * F(2.2), F(0.015), F(0.040))
                if streak >= 8:
                    rms_gate = std_max(F(0.012), rms_gate - std_min(F(0.010), F(0.001) * F(streak - 7)))
            else:
                rms_gate = std_clamp(noise_floor_ * F(1.8), F(0.014), F(0.030))
                if streak >= 8:
                    rms_gate = std_max(F(0.010), rms_gate - std_min(F(0.008), F(0.001) * F(streak - 7)))
            if rms < rms_gate:
                r["rms_skips"] += 1
                corr_pos = (corr_pos + CORRELATION_STEP) % MAX_BUFFER_SAMPLES
                feed()
                continue
            # ---- backtrack and step (:589-612)
            backtrack = 19200 if connected_zc_mode else 9600
            step = 1200 if connected_zc_mode else CORRELATION_STEP
            if corr_pos >= backtrack:
                search_start = corr_pos - backtrack
            elif total_fed < MAX_BUFFER_SAMPLES:
                search_start = 0                         # :601
                hit("start_clipped")
            else:
                search_start = (MAX_BUFFER_SAMPLES + corr_pos - backtrack) % MAX_BUFFER_SAMPLES   # :604
                hit("backtrack_underflow")
            if search_start + min_search > MAX_BUFFER_SAMPLES:
                hit("span_straddles_ring_end")
            search_buffer = ring.read(search_start, min_search)
            # the span crosses the write position: ring indices write_pos - 1 and write_pos both lie inside it
            span_wraps = total_fed >= MAX_BUFFER_SAMPLES and 0 < (write_pos - search_start) % MAX_BUFFER_SAMPLES < min_search
            if span_wraps:
                hit("span_wraps")
            corr_pos = (corr_pos + step) % MAX_BUFFER_SAMPLES
            # ---- thresholds (:662-716)
            conf, weak_floor = confidence(cls, connected_, streak, fading_hint, snr_hint)
            known_cfo = last_cfo
            detect_threshold = conf if is_zc_mode else F(0.15)
            r["search_start"] = search_start
            r["abs_search_start"] = ring_pos_to_absolute(search_start)
            r["span_wraps"] = int(span_wraps)
            r["sync_position"] = r["abs_position"] = -1          # search_start .. root are the last detector run's
            r["min_confidence"], r["detect_threshold"], r["known_cfo_hz"] = conf, detect_threshold, known_cfo
            r["detector_runs"] += 1
            # ---- the detector and the acceptance rules (:725-834)
            weak_accept = False
            if connected_light_sync:
                if mode == LTS:
                    d = O.detect_data_sync(search_buffer, float(known_cfo), float(detect_threshold))
                    found, start, corr, cfo = bool(d[0]), int(d[1]), F(d[2]), known_cfo
                    r["marker"] = int(d[3]) if found else 0
                else:
                    d = O.zc_detect(search_buffer, float(detect_threshold), 12, float(known_cfo))
                    found, start, corr, cfo = bool(d[0]), int(d[2]), F(d[3]), F(d[4])
                    r["marker"], r["root"] = int(d[1]), int(d[6])
                if is_zc_mode and not found:
                    if corr >= weak_floor:
                        streak += 1
                        r["near_misses"] += 1
                    elif streak > 0:
                        streak -= 1
                if found and corr < conf:
                    allow = (not is_coherent) and connected_ and streak >= 3 and corr >= std_max(weak_floor, conf - F(0.08))
                    if allow:
                        weak_accept = True
                        r["weak_accepts"] += 1
                    else:
                        streak += 1
                        r["rejects"] += 1
                        found = False
                if found:
                    streak = max(1, streak // 2) if weak_accept else 0
            else:
                d = O.chirp_detect(search_buffer, 0.15)
                found, corr, cfo = bool(d[0]), F(std_max(F(d[4]), F(d[5]))), F(d[3])
                start = int(d[2]) + 24000 + 4800 if found else -1
            r["correlation"] = corr
            r["weak_accept"] = int(weak_accept)
            if found:
                sync_position = (search_start + start) % MAX_BUFFER_SAMPLES       # :858
                if search_start + start >= MAX_BUFFER_SAMPLES:
                    hit("sync_position_wraps")
                r["sync_position"] = sync_position
                r["abs_position"] = ring_pos_to_absolute(sync_position)
                replay = False
                if last_decoded != NO_LAST_SYNC:             # :876-889
                    d1 = sync_position - last_decoded if sync_position >= last_decoded else MAX_BUFFER_SAMPLES - last_decoded + sync_position
                    replay = min(d1, MAX_BUFFER_SAMPLES - d1) < 200
                if replay:
                    r["replays"] += 1
                    hit("replay")
                    if sync_position < last_decoded and d1 < 200:
                        hit("replay_across_ring_end")
                    if sync_position == last_decoded:
                        hit("replay_same_ring_index")
                    if sync_position + 9600 + CORRELATION_STEP >= MAX_BUFFER_SAMPLES:
                        hit("replay_cursor_wraps")
                    corr_pos = (sync_position + 9600 + CORRELATION_STEP) % MAX_BUFFER_SAMPLES
                else:
                    new_cfo = cfo                                # :903-917
                    if connected_ and abs(known_cfo) > F(0.01):
                        cfo_diff = new_cfo - known_cfo
                        if abs(cfo_diff) > F(1.0):
                            new_cfo = known_cfo
                    snr = (corr - F(0.15)) / F(0.03)           # estimateSNRFromChirp
                    snr = std_max(F(-5.0), std_min(F(30.0), snr))
                    r["sync_cfo_hz"], r["sync_snr_db"] = new_cfo, snr
                    last_cfo, snr_hint = F(new_cfo), F(snr)
                    outcome = SYNC_FOUND
                    if total_fed >= MAX_BUFFER_SAMPLES:
                        hit(("sync_after_wrap", mode))
                    break
            feed()
    hit(("outcome", outcome))
    r["outcome"] = outcome
    s = np.zeros((), STATE)
    s["correlation_pos"], s["total_fed"], s["noise_floor"], s["reject_streak"] = corr_pos, total_fed, noise_floor_, streak
    s["last_cfo_hz"], s["fading_hint"], s["snr_hint"], s["last_decoded_sync_pos"] = last_cfo, fading_hint, snr_hint, last_decoded
    s["overflow_events"], s["overflow_dropped"] = overflow_events_, overflow_total
    return r, s
