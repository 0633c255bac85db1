// ria_amd/csrc/search_rules.hpp — the scalar rules of ria_gpu_search_batch that the device and the host share: what
// StreamingDecoder::searchForSync (src/gui/modem/streaming_decoder.cpp:386-941) and feedAudio (:184-291) decide before the
// ring buffer wraps.  float32 throughout; std::max / std::min / std::clamp are spelled out with the reference's argument
// order, so a NaN goes where the reference sends it.  Plain C++17, no HIP needed: tests/helpers/search_rules_check.cpp
// builds it with g++.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RIA_SRCH_HD __host__ __device__ __forceinline__
#else
#define RIA_SRCH_HD inline
#endif

namespace ria {

// mirrors of include/ria_gpu.h (RIA_SEARCH_*); kSearchOpen / kSearchDue are internal: the stream walks on / its detector is due
constexpr int kSearchLts = 0, kSearchZc = 1, kSearchChirp = 2;
constexpr int kSearchSyncFound = 1, kSearchNeedSamples = 2, kSearchLimit = 3, kSearchDue = 254, kSearchOpen = 255;
// the modulation classes of :662-682 (is_zc_mode = the MC-DPSK waveform, whatever the detector)
constexpr int kSrchDifferential = 0, kSrchCoherentPsk = 1, kSrchCoherentQam = 2, kSrchZc = 3;
constexpr int kSrchRing = 960000;                     // MAX_BUFFER_SAMPLES
constexpr int kSrchMaxCapture = kSrchRing - 1;        // the ring never wraps
constexpr int kSrchStep = 4800, kSrchStepZc = 1200;   // CORRELATION_STEP, CORRELATION_STEP_ZC
constexpr int kSrchBacktrack = 9600, kSrchBacktrackZc = 19200;
constexpr int kSrchRmsLen = 1000;
constexpr int kSrchLtsPreamble = 2 * 1152;            // OFDMChirpWaveform::getDataPreambleSamples
constexpr int kSrchZcPreamble = 2512 + 8 * 512 + 512; // MCDPSKWaveform::getDataPreambleSamples: ZC + training + reference
constexpr int kSrchChirpPreamble = 57600;             // ChirpSync::getTotalSamples

// std::max(a, b), std::min(a, b), std::clamp(v, lo, hi) as the library defines them
RIA_SRCH_HD float srch_max(float a, float b) { return (a < b) ? b : a; }
RIA_SRCH_HD float srch_min(float a, float b) { return (b < a) ? b : a; }
RIA_SRCH_HD float srch_clamp(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }

// min_search (:408-438)
RIA_SRCH_HD int srch_min_search(int mode) {
    const int chirp_max = 120000, light_min = 9600;
    int m;
    if (mode == kSearchZc) m = (kSrchZcPreamble + 24000 < 48000) ? kSrchZcPreamble + 24000 : 48000;
    else if (mode == kSearchLts) m = (kSrchLtsPreamble + 65000 < chirp_max) ? kSrchLtsPreamble + 65000 : chirp_max;
    else return (kSrchChirpPreamble + 65000 < chirp_max) ? kSrchChirpPreamble + 65000 : chirp_max;
    return m < light_min ? light_min : m;
}

// feedAudio before the wrap (:184-225, :286-291) for min(feed_step, capture_len - fed) samples: none arriving changes
// nothing (:185); a cursor ahead of the write position is clamped to it and the streak cleared.  Returns the samples fed.
RIA_SRCH_HD int srch_feed(int* cursor, int* fed, int* streak, int capture_len, int feed_step) {
    int count = capture_len - *fed;
    if (feed_step < count) count = feed_step;
    if (count <= 0) return 0;
    if (*cursor > *fed) { *cursor = *fed; *streak = 0; }
    *fed += count;
    return count;
}

// the two waits (:449, :475); a cursor ahead of `fed` is the library's limit (the reference reads unwritten ring samples)
RIA_SRCH_HD bool srch_wait(int cursor, int fed, int min_search) {
    if (fed < min_search) return true;
    if (cursor > fed) return true;
    return fed - cursor < min_search;
}

// ZC backlog catch-up (:488-522) with the integer scaling as written: 0 none, 1 moderate, 2 severe
RIA_SRCH_HD int srch_catch_up(int* cursor, int fed, int min_search) {
    const long long unsearched = static_cast<long long>(fed) - *cursor;
    const long long scaled = unsearched * 10 / min_search;
    if (scaled > 25) {
        *cursor = static_cast<int>((static_cast<long long>(fed) + kSrchRing - min_search - 4800) % kSrchRing);
        return 2;
    }
    if (scaled > 15) {
        long long catch_up = (unsearched - min_search) / 2;
        if (24000 < catch_up) catch_up = 24000;
        if (catch_up < 4800) catch_up = 4800;
        *cursor = static_cast<int>((*cursor + catch_up) % kSrchRing);
        return 1;
    }
    return 0;
}

// the noise-floor tracker (:536-541): the slow branch when rms >= 3 * floor (or the compare is with a NaN)
RIA_SRCH_HD float srch_noise_floor(float noise_floor_prev, float rms, bool* fast) {
    const float noise_floor = srch_max(0.001f, noise_floor_prev);
    *fast = rms < noise_floor * 3.0f;
    return *fast ? 0.98f * noise_floor + 0.02f * rms : 0.995f * noise_floor + 0.005f * rms;
}

// the adaptive gate (:543-563) on the updated floor: light sync (LTS, ZC) or the chirp path
RIA_SRCH_HD float srch_gate(bool light_sync, float noise_floor, int streak) {
    float gate;
    if (light_sync) {
        gate = srch_clamp(noise_floor * 2.2f, 0.015f, 0.040f);
        if (streak >= 8) gate = srch_max(0.012f, gate - srch_min(0.010f, 0.001f * static_cast<float>(streak - 7)));
    } else {
        gate = srch_clamp(noise_floor * 1.8f, 0.014f, 0.030f);
        if (streak >= 8) gate = srch_max(0.010f, gate - srch_min(0.008f, 0.001f * static_cast<float>(streak - 7)));
    }
    return gate;
}

// backtrack and step (:589-612) before the wrap
RIA_SRCH_HD int srch_search_start(int cursor, bool zc) {
    const int backtrack = zc ? kSrchBacktrackZc : kSrchBacktrack;
    return cursor >= backtrack ? cursor - backtrack : 0;
}
RIA_SRCH_HD int srch_step(bool zc) { return zc ? kSrchStepZc : kSrchStep; }

// light_sync_min_confidence / weak_sync_floor (:679-716)
RIA_SRCH_HD void srch_confidence(int cls, bool connected, int streak, float fading_hint, float snr_hint, float* min_confidence, float* weak_floor) {
    const bool zc = cls == kSrchZc, psk = cls == kSrchCoherentPsk, qam = cls == kSrchCoherentQam;
    float conf = zc ? 0.40f : (psk ? 0.90f : (qam ? 0.78f : 0.72f));
    float floor = zc ? 0.30f : (psk ? 0.85f : (qam ? 0.70f : 0.55f));
    if (!psk && !qam && !zc) {
        if (fading_hint >= 1.00f || snr_hint < 10.0f) conf = 0.62f;
        else if (fading_hint >= 0.70f || snr_hint < 14.0f) conf = 0.65f;
        else if (fading_hint >= 0.50f || snr_hint < 18.0f) conf = 0.68f;
        if (connected && streak >= 8) conf = srch_max(0.56f, conf - srch_min(0.12f, 0.015f * static_cast<float>(streak - 7)));
    }
    if (zc && connected && streak >= 4) {
        const float extra_relax = srch_min(0.15f, 0.025f * static_cast<float>(streak - 3));
        conf = srch_max(0.25f, conf - extra_relax);
        floor = srch_max(0.20f, floor - extra_relax);
    }
    *min_confidence = conf;
    *weak_floor = floor;
}

// the detector's threshold (:732)
RIA_SRCH_HD float srch_detect_threshold(int cls, float min_confidence) { return cls == kSrchZc ? min_confidence : 0.15f; }

// ZC near miss (:739-750) on a detection that was not found: +1 (counted), -1 or 0
RIA_SRCH_HD int srch_near_miss(int streak, float correlation, float weak_floor) {
    if (correlation >= weak_floor) return 1;
    return streak > 0 ? -1 : 0;
}

// a found detection below the confidence (:754-759): weak accept or reject
RIA_SRCH_HD bool srch_weak_accept(int cls, bool connected, int streak, float correlation, float min_confidence, float weak_floor) {
    const bool coherent = cls == kSrchCoherentPsk || cls == kSrchCoherentQam;
    return !coherent && connected && streak >= 3 && correlation >= srch_max(weak_floor, min_confidence - 0.08f);
}
RIA_SRCH_HD int srch_streak_after_accept(int streak, bool weak_accept) { return weak_accept ? (streak / 2 < 1 ? 1 : streak / 2) : 0; }

// anti-replay (:876-889): circular distance on the ring; INT32_MIN = no decoded position.  The cursor a replay leaves behind.
RIA_SRCH_HD bool srch_replay(int sync_position, int last_decoded_sync_pos) {
    if (last_decoded_sync_pos == INT32_MIN) return false;
    const long long d1 = sync_position >= last_decoded_sync_pos ? static_cast<long long>(sync_position) - last_decoded_sync_pos
                                                                  : static_cast<long long>(kSrchRing) - last_decoded_sync_pos + sync_position;
    const long long dist = (kSrchRing - d1 < d1) ? kSrchRing - d1 : d1;
    return dist < 200;
}
RIA_SRCH_HD int srch_replay_cursor(int sync_position) { return static_cast<int>((static_cast<long long>(sync_position) + 9600 + kSrchStep) % kSrchRing); }

// CFO sanity (:903-915)
RIA_SRCH_HD float srch_cfo_sanity(bool connected, float new_cfo, float known_cfo, bool* taken) {
    *taken = false;
    if (connected && fabsf(known_cfo) > 0.01f) {
        const float cfo_diff = new_cfo - known_cfo;
        if (fabsf(cfo_diff) > 1.0f) { *taken = true; return known_cfo; }
    }
    return new_cfo;
}

// estimateSNRFromChirp (:2587-2590)
RIA_SRCH_HD float srch_snr(float correlation) {
    const float snr = (correlation - 0.15f) / 0.03f;
    return srch_max(-5.0f, srch_min(30.0f, snr));
}

}  // namespace ria
