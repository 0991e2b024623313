/* cudasw4_amd_msa.h — the query-anchored multiple alignment of a query's aligned hits, and its redundancy filter.
 *
 * An extension.  The inputs are those of sw_pssm_accumulate (cudasw4_amd_pssm.h): the master codes, the n
 * hits IN RANK ORDER with their subjects, the records and CIGAR words sw_align_hits / sw_align_hits_pssm wrote, and an
 * optional include byte per hit.  A hit takes part under the rule of sw_pssm_accumulate: include byte non-zero (or no
 * include array), status SW_ALIGN_OK and cigar_len > 0.
 *
 * Rows.  Row h (qlen bytes) holds per query position i
 *     a (0..19)     an '=' or 'X' column pairs i with the subject code a < 20
 *     20            an '=' or 'X' column pairs i with a subject code >= 20 (or a negative one)
 *     SW_MSA_GAP    i lies in [q_begin, q_end) and an 'I' run covers it (a query residue against a gap)
 *     SW_MSA_NONE   everything else: i outside [q_begin, q_end), a hit that takes no part, a position no run covers
 * 'D' runs own no column.  The master is row n: query[i] if 0 <= query[i] < 20, else 20; query == NULL: all NONE.
 * Positions are checked against qlen and the subject's length before they are used: a pair column whose query position
 * lies outside [0, qlen) is dropped, one whose subject position lies outside the subject leaves NONE.  A record with a
 * negative q_begin or s_begin is no alignment: its whole row is NONE.
 *
 * Counts.  res(h) = #{i : row_h[i] < 20};  ident(g, h) = #{i : row_g[i] == row_h[i] and row_h[i] < 20}.
 * Redundancy.  For P in 1..100, similar(g, h) iff res(h) > 0 and 100 * ident(g, h) >= P * res(h) (64-bit integers): a
 * fragment is redundant to the full-length row that contains it, not the other way round.
 * Greedy keep.  Order: the master, then the hits 0, 1, ..., n - 1.  The master is kept when res > 0.  A hit with res > 0 is
 * kept iff no KEPT earlier row g has similar(g, h), else it is purged.  A hit with res == 0 (which includes every hit
 * that takes no part) has keep 0 and is not counted as purged.  P == 0: no filter, keep = (res > 0), purged = 0.
 * Greedy is not the transitive closure: with B redundant to A and C to B but not to A, C is kept.
 *
 * Everything is integer arithmetic: the outputs do not depend on any order of execution. */
#ifndef CUDASW4_AMD_MSA_H
#define CUDASW4_AMD_MSA_H

#include "cudasw4_amd_pssm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SW_MSA_GAP 21
#define SW_MSA_NONE 22
#define SW_MSA_MAX_HITS (1 << 15)

/* All pointers are DEVICE pointers unless marked HOST.  The call is asynchronous on `stream` and zeroes its outputs
 * itself.  n == 0 is legal (the master alone).
 *   SW_ERR_INVALID: qlen < 1, qlen > SW_PSSM_MAX_QUERY_LEN, n < 0, n > SW_MSA_MAX_HITS, max_identity outside 0..100, a null
 *                   residues / keep / purged, n > 0 with a null chars / offsets / lengths / results / cigar
 *   SW_ERR_TEMP:    temp_bytes below what *temp_bytes_needed reports
 * temp == NULL: *temp_bytes_needed is written (when the pointer is given) and nothing is launched.  The need depends on
 * qlen, n, max_identity and whether pair_ident is asked for, on nothing else. */
typedef struct sw_msa_args {
    const int8_t* query;         /* master codes, qlen; NULL: the master row is all NONE */
    int32_t qlen;
    int32_t n;                   /* hits, in rank order */
    const int8_t* chars;         /* as in sw_pssm_accumulate_args */
    const uint64_t* offsets;
    const int32_t* lengths;
    const sw_align_result* results;
    const uint32_t* cigar;
    const uint8_t* include;      /* n, or NULL */
    int32_t max_identity;        /* P: 0 (no filter) or 1..100 */
    uint8_t* rows;               /* out, optional: (n + 1) x qlen, row n = master */
    int32_t* residues;           /* out: n + 1 */
    uint8_t* keep;               /* out: n + 1 */
    int32_t* purged;             /* out: 1 */
    uint32_t* pair_ident;        /* out, optional: (n + 1) x (n + 1), [h][g] = ident(g, h) for every g that precedes h in the
                                    greedy order (g == n, the master, precedes every hit), 0 elsewhere (tests and small n) */
    void* temp;
    size_t temp_bytes;
    size_t* temp_bytes_needed;   /* HOST, optional */
    void* const* phase_events;   /* HOST, optional: 4 hipEvent_t recorded on `stream`: before the rows stage, before the pair
                                    stage, before the greedy stage and after it */
    void* stream;
} sw_msa_args;

int sw_msa_filter(sw_ctx* ctx, const sw_msa_args* a);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_MSA_H */
