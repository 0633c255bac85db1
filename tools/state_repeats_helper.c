/* tools/state_repeats_helper.c - CPU helper of tools/count_state_repeats.py (developer aid, never the product).
 *
 * Restates the oracle's min-sum decoder (ro_ldpc_decode, oracle/ria_oracle.c) with the check-to-variable vector of every
 * iteration kept, so that the first iteration at which the decoder's complete message state equals an earlier one, and
 * the distance between the two, can be read off; and walks the retry cascade of ro_decode_fixed_frame with that decoder,
 * one record per decode.  Compiled together with the oracle's sources (which it only reads) into one library by the
 * Python tool; tests/test_state_repeats_cpu.py pins both restatements against the oracle's own functions. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "ria_oracle.h"

#define SR_MAX_ITER 128

typedef struct sr_result {
    int32_t ok, iters;      /* as ro_ldpc_decode: converged, lastIterations */
    int32_t rep_t, rep_p;   /* first iteration t >= 2 whose message state equals that of iteration t - p >= 1 (smallest p); -1: none */
} sr_result;

static uint32_t bits_of(float x) { uint32_t u; x = x + 0.0f; memcpy(&u, &x, 4); return u; }   /* -0.0 and +0.0 are one state */

/* Same values as ro_ldpc_decode bit for bit: the minimum over the other edges of a row is the row's second smallest
 * magnitude for the edge that holds the smallest and the smallest for every other edge; sign * min_abs * factor in the
 * oracle's order of operations. */
int sr_decode(const ro_ldpc* c, const float* llr, int max_iter, float factor, uint8_t* out, sr_result* res) {
    const int n = c->n, k = c->k, m = c->m, ne = c->n_edges;
    static _Thread_local float llr_in[RO_CW_BITS], tot[RO_CW_BITS], v2c[RO_MAX_EDGES], c2v[RO_MAX_EDGES];
    static _Thread_local uint32_t* hist = NULL;   /* [SR_MAX_ITER][RO_MAX_EDGES] bit patterns of c2v */
    static _Thread_local uint64_t hash[SR_MAX_ITER];
    if (!hist) hist = (uint32_t*)malloc(sizeof(uint32_t) * SR_MAX_ITER * RO_MAX_EDGES);
    if (max_iter > SR_MAX_ITER) max_iter = SR_MAX_ITER;
    for (int j = 0; j < n; ++j) { llr_in[j] = llr[j]; tot[j] = llr_in[j]; }
    for (int e = 0; e < ne; ++e) { v2c[e] = llr_in[c->edge_var[e]]; c2v[e] = 0.0f; }
    int success = 0, it;
    res->rep_t = res->rep_p = -1;
    for (it = 0; it < max_iter; ++it) {
        for (int i = 0; i < m; ++i) {
            const int e0 = c->row_ptr[i], e1 = c->row_ptr[i + 1];
            float min1 = 3.402823466e+38f, min2 = 3.402823466e+38f;
            int imin = -1, neg = 0;
            for (int e = e0; e < e1; ++e) {
                const float a = fabsf(v2c[e]);
                if (v2c[e] < 0) neg ^= 1;
                if (a < min1) { min2 = min1; min1 = a; imin = e; }
                else if (a < min2) min2 = a;
            }
            for (int e = e0; e < e1; ++e) {
                const int s = neg ^ (v2c[e] < 0 ? 1 : 0);
                const float sign = s ? -1.0f : 1.0f;
                c2v[e] = sign * (e == imin ? min2 : min1) * factor;
            }
        }
        for (int j = 0; j < n; ++j) tot[j] = llr_in[j];
        for (int e = 0; e < ne; ++e) tot[c->edge_var[e]] += c2v[e];
        for (int e = 0; e < ne; ++e) {
            float v = tot[c->edge_var[e]] - c2v[e];
            v = v < 50.0f ? v : 50.0f;
            v2c[e] = v > -50.0f ? v : -50.0f;
        }
        int ok = 1;
        for (int i = 0; i < m && ok; ++i) {
            int s = 0;
            for (int e = c->row_ptr[i]; e < c->row_ptr[i + 1]; ++e) s ^= (tot[c->edge_var[e]] < 0);
            if (s) ok = 0;
        }
        if (ok) { success = 1; break; }
        /* the state after this iteration's check pass, against the earlier ones */
        uint32_t* h = hist + (size_t)it * RO_MAX_EDGES;
        uint64_t hs = 1469598103934665603ull;
        for (int e = 0; e < ne; ++e) { h[e] = bits_of(c2v[e]); hs = (hs ^ h[e]) * 1099511628211ull; }
        hash[it] = hs;
        if (res->rep_t < 0 && it >= 2)
            for (int p = 1; it - p >= 1; ++p)
                if (hash[it - p] == hs && memcmp(hist + (size_t)(it - p) * RO_MAX_EDGES, h, sizeof(uint32_t) * (size_t)ne) == 0) {
                    res->rep_t = it; res->rep_p = p;
                    break;
                }
    }
    res->ok = success; res->iters = it;
    const int nb = (k + 7) / 8;
    memset(out, 0, (size_t)nb);
    for (int j = 0; j < k; ++j) if (tot[j] < 0) out[j / 8] |= (uint8_t)(1u << (7 - (j % 8)));
    return success;
}

/* One decode of the walk.  stage 0: the codeword's first decode (idx = 0 at factor 0.9375, 1 at the inherited 0.875);
 * stage 1: min-sum factor idx = 1..4 (0.875, 0.75, 0.625, 0.5) on the unmodified soft bits; stage 2: cascade attempt
 * idx = 0..33.  needed: ro_decode_fixed_frame runs this decode (the others only with all != 0). */
typedef struct sr_rec { int32_t cw, stage, idx, needed, ok, iters, rep_t, rep_p; } sr_rec;

/* Retry cascade of ro_decode_fixed_frame (phase 0 and the perturbation phases; the CRC recovery is not walked).
 * Returns the number of records.  all != 0: also the four factor decodes of every codeword and all 34 attempts of every
 * codeword that enters the cascade, i.e. every decode a GPU kernel may run. */
int sr_walk_frame(const float* llr, int rate, int bps, int max_iter, int all, uint8_t* ok_out, int32_t* iters_out, int32_t* attempts_out,
                  sr_rec* rec, int max_rec) {
    static _Thread_local ro_ldpc code;
    static _Thread_local int table[4 * RO_CW_BITS];
    static _Thread_local int table_key = -1;
    if (code.rate != rate || code.n == 0) ro_ldpc_build(&code, rate);
    if (table_key != bps) { ro_rx_gather_table(bps, 1, table); table_key = bps; }
    static const float f0[4] = { 0.875f, 0.75f, 0.625f, 0.5f };
    static const float s1[15] = { 0.3f, 0.7f, 0.3f, 1.0f, 0.5f, 1.5f, 0.3f, 2.0f, 0.5f, 0.7f, 1.0f, 2.5f, 0.3f, 1.5f, 0.5f };
    static const float f1[15] = { 0.75f, 0.625f, 0.875f, 0.75f, 0.625f, 0.75f, 0.5f, 0.625f, 0.875f, 0.75f, 0.625f, 0.875f, 0.75f, 0.5f, 0.625f };
    static const float s2[5] = { 0.3f, 0.8f, 1.5f, 2.5f, 4.0f };
    static const float s3[3] = { 0.5f, 1.5f, 3.0f };
    static const float s4[3] = { 0.5f, 1.5f, 3.0f };
    static const float s5[5] = { 0.0f, 0.2f, 0.5f, 1.0f, 1.5f };
    static const float s6[3] = { 0.3f, 1.0f, 2.0f };
    int nrec = 0;
    float dec_factor = 0.9375f;
    uint8_t dec[81];
#define SR_PUT(cw_, st_, ix_, nd_, r_) do { if (nrec < max_rec) { sr_rec* q = rec + nrec; q->cw = cw_; q->stage = st_; q->idx = ix_; q->needed = nd_; \
        q->ok = (r_).ok; q->iters = (r_).iters; q->rep_t = (r_).rep_t; q->rep_p = (r_).rep_p; } ++nrec; } while (0)
    for (int cw = 0; cw < 4; ++cw) {
        float b[RO_CW_BITS];
        for (int i = 0; i < RO_CW_BITS; ++i) b[i] = llr[table[cw * RO_CW_BITS + i]];
        sr_result r, rf[5];
        int have[5] = { 0, 0, 0, 0, 0 }, used[5] = { 0, 0, 0, 0, 0 };
        int attempts = 1;
        const int first_idx = dec_factor == 0.9375f ? 0 : 1;
        int ok = sr_decode(&code, b, max_iter, dec_factor, dec, &r);
        int iters = r.iters;
        SR_PUT(cw, 0, first_idx, 1, r);
        if (first_idx == 1) { rf[1] = r; have[1] = 1; }
        if (!ok) {
            uint32_t h = 0;
            for (int j = 0; j < 16; ++j) { uint32_t u; memcpy(&u, &b[j], 4); h ^= u + 0x9e3779b9u + (h << 6) + (h >> 2); }
            for (int t = 0; t < 4 && !ok; ++t) {
                attempts++;
                if (!have[t + 1]) { sr_decode(&code, b, max_iter, f0[t], dec, &rf[t + 1]); have[t + 1] = 1; }
                used[t + 1] = 1;
                if (rf[t + 1].ok) { ok = 1; iters = rf[t + 1].iters; }
            }
            dec_factor = 0.9375f;
            if (!ok) {
                float pert[RO_CW_BITS];
                ro_mt rng;
                int a = 0, won = 0;
                for (int phase = 1; phase <= 6; ++phase) {
                    const int cnt = (phase == 1) ? 15 : (phase == 2) ? 5 : (phase == 5) ? 5 : 3;
                    for (int t = 0; t < cnt; ++t, ++a) {
                        float sigma, fac = dec_factor;
                        uint32_t seed;
                        switch (phase) {
                            case 1: fac = f1[t]; sigma = s1[t]; seed = h + (uint32_t)(t * 997 + t * 31); break;
                            case 2: fac = (t % 2 == 0) ? 0.625f : 0.875f; sigma = s2[t]; seed = h + (uint32_t)((t + 15) * 997 + 12345); break;
                            case 3: sigma = s3[t]; seed = h + (uint32_t)((t + 20) * 997 + 54321); break;
                            case 4: sigma = s4[t]; seed = h + (uint32_t)((t + 23) * 997 + 99999); break;
                            case 5: sigma = s5[t]; seed = h + (uint32_t)((t + 26) * 997 + 33333); break;
                            default: sigma = s6[t]; seed = h + (uint32_t)((t + 31) * 997 + 77777); break;
                        }
                        /* phases 3-6 decode at the factor phases 1-2 leave behind (0.875), whichever attempt comes first */
                        if (phase >= 3) fac = 0.875f;
                        if (won && !all) continue;
                        ro_mt_seed(&rng, seed);
                        ro_normal nd = { 0, 0 };
                        for (int i = 0; i < RO_CW_BITS; ++i) {
                            float v = b[i];
                            switch (phase) {
                                case 1: v += ro_normal_draw(&nd, &rng, 0.0f, sigma); break;
                                case 2: v = v < 10.0f ? v : 10.0f; v = v > -10.0f ? v : -10.0f; v += ro_normal_draw(&nd, &rng, 0.0f, sigma); break;
                                case 3: v = v * 0.5f + ro_normal_draw(&nd, &rng, 0.0f, sigma); break;
                                case 4: v = v < 6.0f ? v : 6.0f; v = v > -6.0f ? v : -6.0f; v += ro_normal_draw(&nd, &rng, 0.0f, sigma); break;
                                case 5: v = (v >= 0) ? 1.0f : -1.0f; v += ro_normal_draw(&nd, &rng, 0.0f, sigma); break;
                                default: v = v * 0.25f + ro_normal_draw(&nd, &rng, 0.0f, sigma); break;
                            }
                            pert[i] = v;
                        }
                        sr_result ra;
                        uint8_t d2[81];
                        sr_decode(&code, pert, max_iter, fac, d2, &ra);
                        SR_PUT(cw, 2, a, won ? 0 : 1, ra);
                        if (!won) {
                            attempts++;
                            if (ra.ok) { won = 1; ok = 1; iters = ra.iters; }
                        }
                    }
                }
                dec_factor = 0.875f;   /* phases 1 and 2 leave it there; an attempt that wins inside them does too */
            }
        }
        for (int t = 1; t <= 4; ++t) {
            if (!have[t] && all) { sr_decode(&code, b, max_iter, f0[t - 1], dec, &rf[t]); have[t] = 1; }
            if (have[t]) SR_PUT(cw, 1, t, used[t], rf[t]);
        }
        ok_out[cw] = (uint8_t)ok; iters_out[cw] = iters; attempts_out[cw] = attempts;
    }
#undef SR_PUT
    return nrec;
}
