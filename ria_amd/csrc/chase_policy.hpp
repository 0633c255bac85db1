// ria_amd/csrc/chase_policy.hpp — fec::ChaseCache's policy (src/fec/chase_cache.{hpp,cpp}) over plain metadata: find, prune,
// evict, the store decision, getCombined, markDecoded, removeEntry, clear and the seven counters.  One host/device header:
// the HARQ kernels (mcdpsk_harq_kernels.hip.h) call it from one lane of the wave that owns a cache and spread the 648-float
// copy or add over the wave; tests/helpers/chase_policy_check.cpp builds it with g++ and drives it from scripts.
//
// The sums are not here: store() says what to do with them (ChaseAct) and where (the entry's slot).  A slot whose entry
// went (prune, evict, remove, clear, markDecoded's erase) keeps stale floats; has_sum is what says a sum exists.
#pragma once
#include <stdint.h>

#include "../../include/ria_gpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RIA_CHASE_HD __host__ __device__ inline
#else
#define RIA_CHASE_HD inline
#endif

namespace ria {

struct ChaseKey { uint16_t seq; uint32_t src_hash, dst_hash; };
struct ChaseCache {                       // 1344 bytes
    ria_chase_stats stats;
    uint64_t store_seq;                   // stores that passed the argument checks
    ria_chase_entry e[RIA_CHASE_MAX_ENTRIES];
};
struct ChaseCfg { int max_entries; int64_t ttl_ms; };
enum ChaseAct { kChaseRefused = 0, kChaseCopy = 1, kChaseAdd = 2 };

RIA_CHASE_HD int chase_find(const ChaseCache& c, const ChaseCfg& g, const ChaseKey& k) {
    for (int s = 0; s < g.max_entries; ++s) {
        const ria_chase_entry& e = c.e[s];
        if (e.used && e.seq == k.seq && e.src_hash == k.src_hash && e.dst_hash == k.dst_hash) return s;
    }
    return -1;
}
RIA_CHASE_HD int chase_size(const ChaseCache& c, const ChaseCfg& g) {
    int n = 0;
    for (int s = 0; s < g.max_entries; ++s) n += c.e[s].used ? 1 : 0;
    return n;
}
// isExpired: (now - last_access) > ttl, signed
RIA_CHASE_HD bool chase_expired(const ria_chase_entry& e, const ChaseCfg& g, uint64_t now_ms) {
    return static_cast<int64_t>(now_ms - e.last_access_ms) > g.ttl_ms;
}
RIA_CHASE_HD void chase_prune(ChaseCache& c, const ChaseCfg& g, uint64_t now_ms) {
    for (int s = 0; s < g.max_entries; ++s)
        if (c.e[s].used && chase_expired(c.e[s], g, now_ms)) { c.e[s].used = 0; c.stats.entries_expired++; }
}
// evictIfNeeded: while size >= max_entries, the smallest (last_access, order) goes
RIA_CHASE_HD void chase_evict(ChaseCache& c, const ChaseCfg& g) {
    while (chase_size(c, g) >= g.max_entries) {
        int oldest = -1;
        for (int s = 0; s < g.max_entries; ++s) {
            const ria_chase_entry& e = c.e[s];
            if (!e.used) continue;
            if (oldest < 0 || e.last_access_ms < c.e[oldest].last_access_ms ||
                (e.last_access_ms == c.e[oldest].last_access_ms && e.order < c.e[oldest].order)) oldest = s;
        }
        if (oldest < 0) break;
        c.e[oldest].used = 0;
        c.stats.entries_evicted++;
    }
}
// store (chase_cache.cpp:27-88) without the floats: what to do with this reception's 648 soft bits, and in which slot
RIA_CHASE_HD ChaseAct chase_store(ChaseCache& c, const ChaseCfg& g, const ChaseKey& k, int cw, int total_cw, int frame_type, uint64_t now_ms,
                            int* slot) {
    *slot = -1;
    if (cw < 0 || cw >= total_cw) return kChaseRefused;
    if (total_cw <= 0 || total_cw > RIA_CHASE_MAX_CW) return kChaseRefused;
    c.stats.stores++;
    c.store_seq++;
    chase_prune(c, g, now_ms);
    int s = chase_find(c, g, k);
    if (s < 0) {
        chase_evict(c, g);
        for (s = 0; s < g.max_entries && c.e[s].used; ++s) {}
        if (s >= g.max_entries) return kChaseRefused;   // not reached: evict left a free slot
        ria_chase_entry& e = c.e[s];
        e.last_access_ms = now_ms; e.order = c.store_seq;
        e.src_hash = k.src_hash; e.dst_hash = k.dst_hash; e.seq = k.seq;
        e.used = 1; e.total_cw = static_cast<uint8_t>(total_cw); e.frame_type = static_cast<uint8_t>(frame_type);
        e.reserved[0] = e.reserved[1] = e.reserved[2] = 0;
        for (int i = 0; i < RIA_CHASE_MAX_CW; ++i) { e.combine_count[i] = 0; e.decoded[i] = 0; e.has_sum[i] = 0; }
        e.combine_count[cw] = 1; e.has_sum[cw] = 1;
        *slot = s;
        return kChaseCopy;
    }
    ria_chase_entry& e = c.e[s];
    e.last_access_ms = now_ms; e.order = c.store_seq;
    if (cw >= e.total_cw) return kChaseRefused;
    if (e.decoded[cw]) return kChaseRefused;
    if (e.combine_count[cw] >= RIA_CHASE_MAX_COMBINES) return kChaseRefused;
    *slot = s;
    if (!e.has_sum[cw]) { e.has_sum[cw] = 1; e.combine_count[cw] = 1; return kChaseCopy; }
    e.combine_count[cw]++;
    c.stats.combines++;
    return kChaseAdd;
}
// getCombined (:90-122): the slot of the sum, or -1 (a miss)
RIA_CHASE_HD int chase_get_combined(ChaseCache& c, const ChaseCfg& g, const ChaseKey& k, int cw) {
    const int s = chase_find(c, g, k);
    if (s < 0 || cw < 0 || cw >= c.e[s].total_cw || !c.e[s].has_sum[cw] || c.e[s].decoded[cw]) { c.stats.cache_misses++; return -1; }
    c.stats.cache_hits++;
    return s;
}
RIA_CHASE_HD int chase_combine_count(const ChaseCache& c, const ChaseCfg& g, const ChaseKey& k, int cw) {
    const int s = chase_find(c, g, k);
    if (s < 0 || cw < 0 || cw >= c.e[s].total_cw) return 0;
    return c.e[s].combine_count[cw];
}
// markDecoded (:138-158)
RIA_CHASE_HD void chase_mark_decoded(ChaseCache& c, const ChaseCfg& g, const ChaseKey& k, int cw) {
    const int s = chase_find(c, g, k);
    if (s < 0) return;
    ria_chase_entry& e = c.e[s];
    if (cw >= 0 && cw < e.total_cw) { e.decoded[cw] = 1; e.has_sum[cw] = 0; }
    bool all = true;
    for (int i = 0; i < e.total_cw; ++i) all = all && e.decoded[i];
    if (all) e.used = 0;
}
RIA_CHASE_HD bool chase_remove(ChaseCache& c, const ChaseCfg& g, const ChaseKey& k) {   // true: there was an entry
    const int s = chase_find(c, g, k);
    if (s < 0) return false;
    c.e[s].used = 0;
    return true;
}
RIA_CHASE_HD void chase_clear(ChaseCache& c) {
    for (int s = 0; s < RIA_CHASE_MAX_ENTRIES; ++s) c.e[s].used = 0;
}

}  // namespace ria
