"""StreamingDecoder::searchForSync (src/gui/modem/streaming_decoder.cpp:386-941) with the part of feedAudio it depends on
(:184-225, :286-291), restated statement for statement in numpy float32 on the oracle's detectors, under the time model of
ria_gpu_search_batch (include/ria_gpu.h): one invocation = one searchForSync(); after every invocation that leaves the stream
open, min(feed_step, capture_len - fed) samples arrive.  The ring buffer never wraps (capture_len <= 959 999), so buffer_[i]
is x[i].  Returns the same result and state records as the library: the yardstick of tests/test_gpu_search.py.

Not restated (the library leaves them out too): the ZC-miss -> chirp fallback (:785-828), the wrap and overflow paths."""
import numpy as np

F = np.float32
MAX_BUFFER_SAMPLES = 960000
CORRELATION_STEP = 4800
NO_LAST_SYNC = -2 ** 31            # SIZE_MAX
LTS, ZC, CHIRP = 0, 1, 2
SYNC_FOUND, NEED_SAMPLES, LIMIT = 1, 2, 3
DIFFERENTIAL, COHERENT_PSK, COHERENT_QAM, ZC_MODE = 0, 1, 2, 3      # current_modulation_'s class; ZC_MODE: mode_ == MC_DPSK

STATE = np.dtype([("correlation_pos", "<i4"), ("fed", "<i4"), ("noise_floor", "<f4"), ("reject_streak", "<i4"),
                  ("last_cfo_hz", "<f4"), ("fading_hint", "<f4"), ("snr_hint", "<f4"), ("last_decoded_sync_pos", "<i4")])
RESULT = np.dtype([("outcome", "<i4"), ("search_start", "<i4"), ("search_len", "<i4"), ("sync_position", "<i4"),
                   ("abs_position", "<i8"), ("correlation", "<f4"), ("known_cfo_hz", "<f4"), ("sync_cfo_hz", "<f4"),
                   ("sync_snr_db", "<f4"), ("detect_threshold", "<f4"), ("min_confidence", "<f4"), ("weak_accept", "<i4"),
                   ("marker", "<i4"), ("root", "<i4"), ("invocations", "<u4"), ("waits", "<u4"), ("rms_skips", "<u4"),
                   ("detector_runs", "<u4"), ("rejects", "<u4"), ("near_misses", "<u4"), ("weak_accepts", "<u4"),
                   ("replays", "<u4"), ("catchups_moderate", "<u4"), ("catchups_severe", "<u4"), ("reserved0", "<u4"), ("reserved1", "<u4"), ("reserved2", "<u4")])


def fresh_state(n, fed=0):
    s = np.zeros(n, STATE)
    s["fed"] = fed
    s["noise_floor"] = F(0.001)
    s["last_decoded_sync_pos"] = NO_LAST_SYNC
    return s


def std_max(a, b):
    return b if a < b else a


def std_min(a, b):
    return b if b < a else a


def std_clamp(v, lo, hi):
    return lo if v < lo else (hi if hi < v else v)


def min_search_of(mode):
    """:408-438 with getDataPreambleSamples() = 2304 (OFDM-CHIRP), 7120 (MC-DPSK) and getPreambleSamples() = 57600"""
    chirp_max, light_min = 120000, 9600
    if mode == ZC:
        return max(min(7120 + 24000, 48000), light_min)
    if mode == LTS:
        return max(min(2304 + 65000, chirp_max), light_min)
    return min(57600 + 65000, chirp_max)


def modulation_class(mode, modulation="DQPSK"):
    if mode != LTS:
        return ZC_MODE
    if modulation in ("QPSK", "BPSK"):
        return COHERENT_PSK
    if modulation in ("QAM16", "QAM32", "QAM64", "QAM256"):
        return COHERENT_QAM
    return DIFFERENTIAL


def confidence(cls, connected, streak, fading_hint, snr_hint):
    """:679-716 -> (light_sync_min_confidence, weak_sync_floor)"""
    is_zc_mode, psk, qam = cls == ZC_MODE, cls == COHERENT_PSK, cls == COHERENT_QAM
    conf = F(0.40) if is_zc_mode else (F(0.90) if psk else (F(0.78) if qam else F(0.72)))
    floor = F(0.30) if is_zc_mode else (F(0.85) if psk else (F(0.70) if qam else F(0.55)))
    if not (psk or qam) and not is_zc_mode:
        if fading_hint >= F(1.00) or snr_hint < F(10.0):
            conf = F(0.62)
        elif fading_hint >= F(0.70) or snr_hint < F(14.0):
            conf = F(0.65)
        elif fading_hint >= F(0.50) or snr_hint < F(18.0):
            conf = F(0.68)
        if connected and streak >= 8:
            extra_relax = std_min(F(0.12), F(0.015) * F(streak - 7))
            conf = std_max(F(0.56), conf - extra_relax)
    if is_zc_mode and connected and streak >= 4:
        extra_relax = std_min(F(0.15), F(0.025) * F(streak - 3))
        conf = std_max(F(0.25), conf - extra_relax)
        floor = std_max(F(0.20), floor - extra_relax)
    return F(conf), F(floor)


class Trace:
    """what the rows of tests/search_inputs.py must reach; filled by search() when given"""

    def __init__(self):
        self.seen = set()

    def hit(self, what):
        self.seen.add(what)


def search(O, x, capture_len, state, mode, cls, connected, feed_step, max_invocations, trace=None):
    """One stream.  state: one STATE record (not modified).  -> (RESULT record, STATE record)"""
    x = np.ascontiguousarray(x, F)
    hit = trace.hit if trace is not None else (lambda what: None)
    corr_pos, fed = int(state["correlation_pos"]), int(state["fed"])
    noise_floor_, streak = F(state["noise_floor"]), int(state["reject_streak"])
    last_cfo, fading_hint, snr_hint = F(state["last_cfo_hz"]), F(state["fading_hint"]), F(state["snr_hint"])
    last_decoded = int(state["last_decoded_sync_pos"])
    assert 0 <= fed <= capture_len <= MAX_BUFFER_SAMPLES - 1 and 0 <= corr_pos < MAX_BUFFER_SAMPLES and streak >= 0
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
        nonlocal corr_pos, fed, streak
        count = min(feed_step, capture_len - fed)
        if count <= 0:                                   # :185
            return False
        if corr_pos > fed:                               # :204-225 (write_pos_ = total_fed_ before the wrap)
            corr_pos = fed
            streak = 0
            hit("feed_clamp")
        fed += count
        return True

    outcome = 0
    with np.errstate(all="ignore"):
        while True:
            if int(r["invocations"]) >= max_invocations:
                outcome = LIMIT
                break
            r["invocations"] += 1
            # ---- the waits (:449-481); a cursor ahead of write_pos_ is the library's limit: a wait
            if fed < min_search or corr_pos > fed or fed - corr_pos < min_search:
                r["waits"] += 1
                if not feed():
                    outcome = NEED_SAMPLES
                    hit("wait_unresolved")
                    break
                hit("wait_fed")
                continue
            unsearched = fed - corr_pos
            # ---- ZC backlog catch-up (:488-522)
            if connected_zc_mode:
                scaled_unsearched = (unsearched * 10) // min_search
                if scaled_unsearched > 25:
                    corr_pos = (fed + MAX_BUFFER_SAMPLES - min_search - 4800) % MAX_BUFFER_SAMPLES
                    r["catchups_severe"] += 1
                elif scaled_unsearched > 15:
                    excess = unsearched - min_search
                    catch_up = max(min(excess // 2, 24000), 4800)
                    corr_pos = (corr_pos + catch_up) % MAX_BUFFER_SAMPLES
                    r["catchups_moderate"] += 1
            # ---- RMS, tracker, gate (:525-573)
            seg = x[corr_pos:corr_pos + 1000]
            rms = np.cumsum(seg * seg, dtype=F)[-1]      # rms += s * s, ascending, float32
            rms = F(np.sqrt(rms / F(1000.0)))
            if not np.isfinite(rms):
                hit("rms_nan" if np.isnan(rms) else "rms_inf")
            noise_floor = std_max(F(0.001), noise_floor_)
            if rms < noise_floor * F(3.0):
                noise_floor_ = F(0.98) * noise_floor + F(0.02) * rms
                hit("tracker_fast")
            else:
                noise_floor_ = F(0.995) * noise_floor + F(0.005) * rms
                hit("tracker_slow")
            if connected_light_sync:
                raw = noise_floor_ * F(2.2)
                rms_gate = std_clamp(raw, F(0.015), F(0.040))
                hit("gate_low" if raw < F(0.015) else ("gate_high" if F(0.040) < raw else "gate_mid"))
                if streak >= 8:
                    relax = std_min(F(0.010), F(0.001) * F(streak - 7))
                    rms_gate = std_max(F(0.012), rms_gate - relax)
                    hit("gate_relaxed")
            else:
                raw = noise_floor_ * F(1.8)
                rms_gate = std_clamp(raw, F(0.014), F(0.030))
                hit("gate_low" if raw < F(0.014) else ("gate_high" if F(0.030) < raw else "gate_mid"))
                if streak >= 8:
                    relax = std_min(F(0.008), F(0.001) * F(streak - 7))
                    rms_gate = std_max(F(0.010), rms_gate - relax)
                    hit("gate_relaxed")
            if rms < rms_gate:
                r["rms_skips"] += 1
                hit("rms_skip")
                corr_pos = (corr_pos + CORRELATION_STEP) % MAX_BUFFER_SAMPLES
                feed()
                continue
            # ---- backtrack and step (:589-612)
            backtrack = 19200 if connected_zc_mode else 9600
            step = 1200 if connected_zc_mode else CORRELATION_STEP
            if corr_pos >= backtrack:
                search_start = corr_pos - backtrack
            else:
                search_start = 0
                hit("start_clipped")
            search_buffer = x[search_start:search_start + min_search]
            corr_pos = (corr_pos + step) % MAX_BUFFER_SAMPLES
            # ---- thresholds (:662-716)
            conf, weak_floor = confidence(cls, connected_, streak, fading_hint, snr_hint)
            hit(("conf", int(cls), float(conf)))
            if is_zc_mode and connected_ and streak >= 4:
                hit("zc_breaker")
            known_cfo = last_cfo
            detect_threshold = conf if is_zc_mode else F(0.15)
            r["search_start"] = search_start
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
                        hit("near_miss_up")
                    elif streak > 0:
                        streak -= 1
                        hit("near_miss_down")
                if found and corr < conf:
                    allow = (not is_coherent) and connected_ and streak >= 3 and corr >= std_max(weak_floor, conf - F(0.08))
                    if allow:
                        weak_accept = True
                        r["weak_accepts"] += 1
                        hit("weak_accept")
                    else:
                        if is_coherent and streak >= 3 and corr >= std_max(weak_floor, conf - F(0.08)):
                            hit("weak_refused_coherent")
                        streak += 1
                        r["rejects"] += 1
                        hit("reject")
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
                sync_position = (search_start + start) % MAX_BUFFER_SAMPLES
                r["sync_position"] = r["abs_position"] = sync_position
                replay = False
                if last_decoded != NO_LAST_SYNC:             # :876-889
                    d1 = sync_position - last_decoded if sync_position >= last_decoded else MAX_BUFFER_SAMPLES - last_decoded + sync_position
                    replay = min(d1, MAX_BUFFER_SAMPLES - d1) < 200
                if replay:
                    r["replays"] += 1
                    hit("replay")
                    corr_pos = (sync_position + 9600 + CORRELATION_STEP) % MAX_BUFFER_SAMPLES
                else:
                    new_cfo = cfo                                # :903-917
                    if connected_ and abs(known_cfo) > F(0.01):
                        cfo_diff = new_cfo - known_cfo
                        if abs(cfo_diff) > F(1.0):
                            new_cfo = known_cfo
                            hit("cfo_sanity_taken")
                        else:
                            hit("cfo_sanity_kept")
                    snr = (corr - F(0.15)) / F(0.03)           # estimateSNRFromChirp
                    snr = std_max(F(-5.0), std_min(F(30.0), snr))
                    r["sync_cfo_hz"], r["sync_snr_db"] = new_cfo, snr
                    last_cfo, snr_hint = F(new_cfo), F(snr)
                    outcome = SYNC_FOUND
                    break
            feed()
    hit(("outcome", outcome))
    r["outcome"] = outcome
    s = np.zeros((), STATE)
    s["correlation_pos"], s["fed"], s["noise_floor"], s["reject_streak"] = corr_pos, fed, noise_floor_, streak
    s["last_cfo_hz"], s["fading_hint"], s["snr_hint"], s["last_decoded_sync_pos"] = last_cfo, fading_hint, snr_hint, last_decoded
    return r, s
