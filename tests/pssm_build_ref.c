/* pssm_build_ref.c — scalar statement of "Building a PSSM" (DESIGN.md): counts, position-based sequence weights and weighted
 * counts of a master sequence's aligned hits, lambda, and the conversion into an int8 PSSM.  TEST INFRASTRUCTURE ONLY.
 * Written from the definition, one alignment column at a time; it shares no code with the library. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t score, status, q_begin, q_end, s_begin, s_end, columns, identities, mismatches, gap_opens, gap_columns, cigar_len;
    int64_t cigar_offset;
} hit_record;   /* the layout of sw_align_result */

/* Robinson & Robinson background, per mille, order ARNDCQEGHILKMFPSTWYV */
static const double BG[20] = {78.05, 51.29, 44.87, 53.64, 19.25, 42.64, 62.95, 73.77, 21.99, 51.42,
                              90.19, 57.44, 22.43, 38.56, 52.03, 71.20, 58.41, 13.30, 32.16, 64.41};

/* has[h * qlen + i] = residue code (0..19) sequence h has at query position i, or -1.  Sequence n is the master. */
static int8_t* residues(const int8_t* query, int32_t qlen, int32_t n, const int8_t* chars, const uint64_t* offsets,
                        const int32_t* lengths, const hit_record* res, const uint32_t* cigar, const uint8_t* include,
                        int32_t* used) {
    int8_t* has = (int8_t*)malloc((size_t)(n + 1) * (size_t)qlen);
    if (!has) return NULL;
    memset(has, -1, (size_t)(n + 1) * (size_t)qlen);
    *used = 0;
    for (int32_t h = 0; h < n; h++) {
        if (include && !include[h]) continue;
        if (res[h].status != 0 || res[h].cigar_len <= 0) continue;
        ++*used;
        const int8_t* s = chars + (offsets[h] - offsets[0]);
        int64_t qi = res[h].q_begin, sj = res[h].s_begin;
        for (int32_t w = 0; w < res[h].cigar_len; w++) {
            const uint32_t word = cigar[res[h].cigar_offset + w];
            const uint32_t op = word & 15u;
            for (uint32_t c = 0; c < (word >> 4); c++) {
                if (op == 7 || op == 8) {
                    if (qi >= 0 && qi < qlen && sj >= 0 && sj < lengths[h] && s[sj] >= 0 && s[sj] < 20)
                        has[(size_t)h * qlen + qi] = s[sj];
                    qi++;
                    sj++;
                } else if (op == 1) {
                    qi++;
                } else if (op == 2) {
                    sj++;
                }
            }
        }
    }
    if (query)
        for (int32_t i = 0; i < qlen; i++)
            if (query[i] >= 0 && query[i] < 20) has[(size_t)n * qlen + i] = query[i];
    return has;
}

/* -> 0, or -1 when out of memory.  counts: qlen x 20 uint32; weights: n + 1 uint64; wcounts: qlen x 20 uint64 */
int pbr_accumulate(const int8_t* query, int32_t qlen, int32_t n, const int8_t* chars, const uint64_t* offsets,
                   const int32_t* lengths, const hit_record* res, const uint32_t* cigar, const uint8_t* include,
                   uint32_t* counts, uint64_t* weights, uint64_t* wcounts, int32_t* used) {
    int8_t* has = residues(query, qlen, n, chars, offsets, lengths, res, cigar, include, used);
    if (!has) return -1;
    memset(counts, 0, sizeof(uint32_t) * 20 * (size_t)qlen);
    memset(wcounts, 0, sizeof(uint64_t) * 20 * (size_t)qlen);
    memset(weights, 0, sizeof(uint64_t) * ((size_t)n + 1));
    for (int32_t h = 0; h <= n; h++)
        for (int32_t i = 0; i < qlen; i++)
            if (has[(size_t)h * qlen + i] >= 0) counts[(size_t)i * 20 + has[(size_t)h * qlen + i]]++;
    for (int32_t h = 0; h <= n; h++)
        for (int32_t i = 0; i < qlen; i++) {
            const int a = has[(size_t)h * qlen + i];
            if (a < 0) continue;
            uint64_t k = 0;
            for (int b = 0; b < 20; b++) k += counts[(size_t)i * 20 + b] > 0;
            weights[h] += (((uint64_t)1) << 32) / (k * (uint64_t)counts[(size_t)i * 20 + a]);
        }
    for (int32_t h = 0; h <= n; h++)
        for (int32_t i = 0; i < qlen; i++)
            if (has[(size_t)h * qlen + i] >= 0) wcounts[(size_t)i * 20 + has[(size_t)h * qlen + i]] += weights[h];
    free(has);
    return 0;
}

static double excess(const int8_t* t21, double lambda) {
    double sum = 0;
    for (int a = 0; a < 20; a++)
        for (int b = 0; b < 20; b++) sum += (BG[a] / 1000.0) * (BG[b] / 1000.0) * exp(lambda * t21[a * 21 + b]);
    return sum - 1.0;
}

/* the positive root of sum p_a p_b exp(lambda s_ab) = 1 by bisection on [1e-3, 2]; NaN when the ends do not bracket it */
double pbr_lambda(const int8_t* t21) {
    double lo = 1e-3, hi = 2.0;
    if (!(excess(t21, lo) < 0) || !(excess(t21, hi) > 0)) return NAN;
    while (1) {
        const double mid = lo + (hi - lo) / 2;
        if (!(mid > lo && mid < hi)) break;
        if (excess(t21, mid) > 0) hi = mid;
        else lo = mid;
    }
    return lo;
}

/* raw: qlen x 20 doubles; pssm: qlen x 21 int8.  -> 0; -1: beta not positive; -2: a column-20 entry that is not negative */
int pbr_convert(const int8_t* t21, const int8_t* master, int32_t qlen, const uint32_t* counts, const uint64_t* wcounts,
                double beta, int8_t* pssm, double* raw, double* lambda_out) {
    if (!(beta > 0)) return -1;
    const double lambda = pbr_lambda(t21);
    *lambda_out = lambda;
    for (int32_t i = 0; i < qlen; i++) {
        const int m = master[i] >= 0 && master[i] < 20 ? master[i] : 20;
        if (t21[m * 21 + 20] >= 0) return -2;
        pssm[(size_t)i * 21 + 20] = t21[m * 21 + 20];
        uint64_t total = 0;
        int k = 0;
        for (int a = 0; a < 20; a++) {
            total += wcounts[(size_t)i * 20 + a];
            if (counts[(size_t)i * 20 + a]) k++;
        }
        if (total == 0) {
            for (int a = 0; a < 20; a++) {
                pssm[(size_t)i * 21 + a] = t21[m * 21 + a];
                raw[(size_t)i * 20 + a] = t21[m * 21 + a];
            }
            continue;
        }
        const double alpha = k - 1;
        for (int a = 0; a < 20; a++) {
            const double pa = BG[a] / 1000.0;
            const double fa = (double)wcounts[(size_t)i * 20 + a] / (double)total;
            double g = 0;
            for (int b = 0; b < 20; b++) {
                const double pb = BG[b] / 1000.0;
                const double fb = (double)wcounts[(size_t)i * 20 + b] / (double)total;
                const double qab = pa * pb * exp(lambda * t21[a * 21 + b]);
                g += fb * qab / pb;
            }
            const double q = (alpha * fa + beta * g) / (alpha + beta);
            const double r = log(q / pa) / lambda;
            raw[(size_t)i * 20 + a] = r;
            double v = r < 0 ? -floor(-r + 0.5) : floor(r + 0.5);   /* nearest, halves away from zero */
            if (v > 127) v = 127;
            if (v < -128) v = -128;
            pssm[(size_t)i * 21 + a] = (int8_t)v;
        }
    }
    return 0;
}
