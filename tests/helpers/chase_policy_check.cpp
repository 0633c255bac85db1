// Host driver of ria_amd/csrc/chase_policy.hpp (tests/test_mcdpsk_harq_cpu.py): runs a script of cache operations, one per
// line, and prints what each returns and, on "dump", the counters and the live entries sorted by key.  The 648 floats of a
// sum are stood in for by one float per (slot, codeword), moved exactly as the kernels move the real ones: copied on
// kChaseCopy, added on kChaseAdd.
//   cfg <max_entries> <ttl_ms>
//   store <seq> <src> <dst> <cw> <total_cw> <frame_type> <now_ms> <value>   -> store <0|1>
//   get <seq> <src> <dst> <cw>                                                -> get <0|1> <sum bits, hex>
//   count <seq> <src> <dst> <cw>                                              -> count <n>
//   mark | remove <seq> <src> <dst> [<cw>]    clear    recover    dump
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../ria_amd/csrc/chase_policy.hpp"

using namespace ria;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    auto cache = std::make_unique<ChaseCache>();
    std::memset(cache.get(), 0, sizeof(ChaseCache));
    std::vector<float> sums(RIA_CHASE_MAX_ENTRIES * RIA_CHASE_MAX_CW, 0.0f);
    ChaseCfg g{16, 30000};
    char op[32];
    while (std::fscanf(f, "%31s", op) == 1) {
        ChaseKey k{};
        unsigned seq, src, dst;
        int cw;
        auto key = [&] { if (std::fscanf(f, "%u %u %u", &seq, &src, &dst) != 3) std::exit(3); k.seq = static_cast<uint16_t>(seq); k.src_hash = src; k.dst_hash = dst; };
        if (!std::strcmp(op, "cfg")) {
            long long ttl;
            if (std::fscanf(f, "%d %lld", &g.max_entries, &ttl) != 2) return 3;
            g.ttl_ms = ttl;
        } else if (!std::strcmp(op, "store")) {
            int total, ftype, slot;
            unsigned long long now;
            float v;
            key();
            if (std::fscanf(f, "%d %d %d %llu %f", &cw, &total, &ftype, &now, &v) != 5) return 3;
            const ChaseAct a = chase_store(*cache, g, k, cw, total, ftype, now, &slot);
            if (a == kChaseCopy) sums[slot * RIA_CHASE_MAX_CW + cw] = v;
            if (a == kChaseAdd) sums[slot * RIA_CHASE_MAX_CW + cw] += v;
            std::printf("store %d\n", a != kChaseRefused);
        } else if (!std::strcmp(op, "get")) {
            key();
            if (std::fscanf(f, "%d", &cw) != 1) return 3;
            const int s = chase_get_combined(*cache, g, k, cw);
            uint32_t bits = 0;
            if (s >= 0) std::memcpy(&bits, &sums[s * RIA_CHASE_MAX_CW + cw], 4);
            std::printf("get %d %08x\n", s >= 0, bits);
        } else if (!std::strcmp(op, "count")) {
            key();
            if (std::fscanf(f, "%d", &cw) != 1) return 3;
            std::printf("count %d\n", chase_combine_count(*cache, g, k, cw));
        } else if (!std::strcmp(op, "mark")) {
            key();
            if (std::fscanf(f, "%d", &cw) != 1) return 3;
            chase_mark_decoded(*cache, g, k, cw);
        } else if (!std::strcmp(op, "remove")) {
            key();
            chase_remove(*cache, g, k);
        } else if (!std::strcmp(op, "clear")) {
            chase_clear(*cache);
        } else if (!std::strcmp(op, "recover")) {
            cache->stats.recoveries++;
        } else if (!std::strcmp(op, "dump")) {
            const ria_chase_stats& s = cache->stats;
            std::printf("stats %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s.cache_hits, s.cache_misses, s.stores,
                        s.combines, s.entries_evicted, s.entries_expired, s.recoveries);
            std::vector<const ria_chase_entry*> live;
            for (int i = 0; i < g.max_entries; ++i) if (cache->e[i].used) live.push_back(&cache->e[i]);
            std::sort(live.begin(), live.end(), [](const ria_chase_entry* a, const ria_chase_entry* b) {
                if (a->seq != b->seq) return a->seq < b->seq;
                if (a->src_hash != b->src_hash) return a->src_hash < b->src_hash;
                return a->dst_hash < b->dst_hash;
            });
            std::printf("size %d\n", chase_size(*cache, g));
            for (const ria_chase_entry* e : live) {
                std::printf("entry %u %u %u total %d type %d last %" PRIu64 " order %" PRIu64 " :", e->seq, e->src_hash, e->dst_hash, e->total_cw, e->frame_type,
                            e->last_access_ms, e->order);
                for (int i = 0; i < e->total_cw; ++i) std::printf(" %d/%d/%d", e->combine_count[i], e->decoded[i], e->has_sum[i]);
                std::printf("\n");
            }
        } else {
            return 4;
        }
    }
    std::fclose(f);
    std::printf("done\n");
    return 0;
}
