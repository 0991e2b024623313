/* cudasw4_amd_msa_select.h — selection of the rows of the query-anchored alignment (cudasw4_amd_msa.h): coverage, identity to
 * the query and a diversity filter.
 *
 * An extension.  Rows, res(h), ident(g, h) and similar_P(g, h) are those of cudasw4_amd_msa.h; the master is row
 * n, the hits are rows 0 .. n - 1 in rank order.  similar_P(g, h) iff res(h) > 0 and 100 * ident(g, h) >= P * res(h).
 *
 *     pairs(h)  = #{i : row_h[i] <= 20}                 (aligned columns, "other" codes included)
 *     covered   : 100 * pairs(h) >= C * qlen            C = 0 .. 100, 0: no test
 *     close     : 100 * ident(master, h) >= Q * res(h)  Q = 0 .. 100, 0: no test; Q > 0 needs a master (query != NULL)
 *     depth[i]  = #{kept rows r, master included : row_r[i] < 20}
 *     needed(h) = D == 0, or some i has row_h[i] < 20 and depth[i] < D       D >= 0
 *     ladder    = P_0 < P_1 < ... < P_{T-1},  1 <= T <= 16,  each in 1 .. 100
 *
 * State of every row (one byte), decided in this order:
 *   1. the master is kept (SW_MSA_STATE_KEPT) when res(master) > 0, and its residues count into depth;
 *   2. a hit with res == 0 (which includes every hit that takes no part) has SW_MSA_STATE_NONE;
 *   3. every other hit that is not covered has SW_MSA_STATE_COVERAGE;
 *   4. otherwise a hit that is not close has SW_MSA_STATE_QUERY_IDENTITY;
 *   5. otherwise the hit is a candidate;
 *   6. for t = 0 .. T - 1, and within a rung for the candidates in rank order: a candidate h is KEPT iff needed(h) under the
 *      depth of that moment and no row g kept so far — in an earlier rung or earlier in this one, the master included,
 *      whatever its rank — has similar_{P_t}(g, h); a kept hit adds its residues to depth at once;
 *   7. whoever is still a candidate after the last rung has SW_MSA_STATE_THINNED.
 * depth only grows, so a candidate that is once not needed never is again.  With D = 0, C = Q = 0 and the ladder {P},
 * state == SW_MSA_STATE_KEPT is exactly `keep` of sw_msa_filter at P.
 *
 * Everything is integer arithmetic: the outputs do not depend on any order of execution. */
#ifndef CUDASW4_AMD_MSA_SELECT_H
#define CUDASW4_AMD_MSA_SELECT_H

#include "cudasw4_amd_msa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SW_MSA_SELECT_MAX_HITS (1 << 14)   /* the levels of all ordered pairs are kept in scratch: (n + 1)^2 bytes */
#define SW_MSA_SELECT_MAX_LADDER 16

#define SW_MSA_STATE_NONE 0
#define SW_MSA_STATE_KEPT 1
#define SW_MSA_STATE_COVERAGE 2
#define SW_MSA_STATE_QUERY_IDENTITY 3
#define SW_MSA_STATE_THINNED 4

/* All pointers are DEVICE pointers unless marked HOST.  The call is asynchronous on `stream` and writes every byte of every
 * output itself.  n == 0 is legal (the master alone).
 *   SW_ERR_INVALID: sw_msa_filter's argument errors: qlen, n < 0, null residues, n > 0 with a null hit buffer; a null
 *                   state / counts; min_coverage or min_query_identity outside 0..100; min_query_identity > 0 with a null
 *                   query; diff < 0; n_ladder outside 1..16 or a null ladder; a rung outside 1..100 or not strictly
 *                   ascending; n > SW_MSA_SELECT_MAX_HITS.  Nothing is launched.
 *   SW_ERR_TEMP:    temp_bytes below what *temp_bytes_needed reports
 * temp == NULL: *temp_bytes_needed is written (when the pointer is given) and nothing is launched.  The need depends on
 * qlen, n, n_ladder and which optional outputs are asked for, on nothing else. */
typedef struct sw_msa_select_args {
    const int8_t* query;         /* master codes, qlen; NULL: the master row is all NONE */
    int32_t qlen;
    int32_t n;                   /* hits, in rank order */
    const int8_t* chars;         /* as in sw_pssm_accumulate_args */
    const uint64_t* offsets;
    const int32_t* lengths;
    const sw_align_result* results;
    const uint32_t* cigar;
    const uint8_t* include;      /* n, or NULL */
    int32_t min_coverage;        /* C */
    int32_t min_query_identity;  /* Q */
    int32_t diff;                /* D */
    const int32_t* ladder;       /* HOST: n_ladder rungs */
    int32_t n_ladder;            /* T */
    uint8_t* state;              /* out: n + 1, entry n the master's */
    int32_t* residues;           /* out: n + 1 */
    int32_t* counts;             /* out: 4 — kept hits, below coverage, below query identity, thinned (the master is in none) */
    int32_t* depth;              /* out, optional: qlen */
    uint8_t* rows;               /* out, optional: (n + 1) x qlen, row n = master */
    uint8_t* levels;             /* out, optional: (n + 1) x (n + 1), [h][g] = #{t : similar_{P_t}(g, h)} for g != h, 0 on the
                                    diagonal (tests and small n) */
    void* temp;
    size_t temp_bytes;
    size_t* temp_bytes_needed;   /* HOST, optional */
    void* const* phase_events;   /* HOST, optional: 4 hipEvent_t recorded on `stream`: before the rows stage, before the levels
                                    stage, before the select stage and after it */
    void* stream;
} sw_msa_select_args;

int sw_msa_select(sw_ctx* ctx, const sw_msa_select_args* a);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_MSA_SELECT_H */
