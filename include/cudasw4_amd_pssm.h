/* cudasw4_amd_pssm.h — profile search: a position-specific scoring matrix (PSSM) as the query of libcudasw4_amd.so.
 *
 * An extension (the reference scores residue strings only).  A PSSM query of qlen positions is qlen x 21 int8 scores:
 * row i = query position i, column c = dbdata subject code c (0..19 = ARNDCQEGHILKMFPSTWYV, 20 = "other" and the
 * padding of the dbdata layout).  It takes the place of the pair (sw_set_matrix, sw_set_query): where a letter query
 * scores position i against subject letter c with matrix[query[i]][c], a PSSM query scores it with pssm[i][c].
 * Everything else — recurrence, gap model, overflow and re-score rules, top-K, result layout — is that of a letter
 * query, and every scan path of cudasw4_amd.h / cudasw4_amd_engine.h serves both.  A PSSM whose row i is the table row
 * of letter i of a string reproduces that string's scores bit for bit.
 */
#ifndef CUDASW4_AMD_PSSM_H
#define CUDASW4_AMD_PSSM_H

#include "cudasw4_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SW_PSSM_COLUMNS 21
/* longest PSSM query (the device form takes 32 bytes per position) */
#define SW_PSSM_MAX_QUERY_LEN (1 << 22)

/* Install a PSSM as the context's query (HOST pointer, row-major qlen x SW_PSSM_COLUMNS int8).
 *   CONTRACT: column 20 of every row must be negative (padding has to neutralise itself: the condition sw_set_matrix
 *   imposes on a table); otherwise any int8 value is allowed.  The rows that pad the query to the kernels' tile are
 *   the library's business.
 * Staging is that of sw_set_query: the scores are copied into a pinned buffer of the context (the caller's buffer is
 * free again on return), the upload is enqueued on `stream` behind the scans of the previous query, and the call does
 * not wait for the GPU.  Needs no sw_set_matrix.  From here on EVERY scan entry point scores with the PSSM —
 * sw_scan_partition, sw_rescore_overflow[_stat], sw_scan_batch with everything it launches (bulk and side launches, row
 * pipelines, windows, the re-score service), and the planning calls (sw_plan_launch, sw_scan_temp_bytes,
 * sw_query_length) describe it — until the next sw_set_query (back to letters) or sw_set_query_pssm.  Bounds that a
 * letter query derives from the largest entry of the substitution table (the int32 kind served in fp32 lanes, the
 * overlap of windows) are derived from the largest entry of the PSSM.
 * sw_align_hits is not affected: it takes its query as an argument and scores with the context's matrix.  The hits of a
 * PSSM query are aligned with sw_align_hits_pssm below, which takes the PSSM as an argument in the same way. */
int sw_set_query_pssm(sw_ctx* ctx, const int8_t* pssm_host, int32_t qlen, void* stream);

/* 1 when the context's current query is a PSSM, 0 for a letter query or none. */
int sw_query_is_pssm(const sw_ctx* ctx);

/* sw_align_hits with a PSSM as the query.  pssm: DEVICE, a->qlen x SW_PSSM_COLUMNS int8 row-major (NOT the context's current
 * query).  a->query: DEVICE consensus codes, one per position, or NULL (argmax consensus).  Needs no sw_set_matrix.
 * Everything else in sw_align_args, the statuses, scratch rule, chunking and phase events are those of sw_align_hits.
 *   Score: pssm[i][s_j] takes the place of matrix[query[i]][s_j] in all three passes (subject codes above 20 count as
 *   20); the tie rules of the end, the start and the traceback are unchanged.
 *   Identity: an aligned pair at query position i is SW_CIGAR_EQ (and counted in `identities`) when the subject code is
 *   below 20 and equals the consensus code of position i, else SW_CIGAR_X.  Consensus codes of 20 and above are identical
 *   to nothing.  Without a consensus, position i has the lowest code c < 20 with the largest pssm[i][c].
 *   CONTRACT: column 20 of every row negative, as for the PSSM of a scan; the rows are read as they are. */
int sw_align_hits_pssm(sw_ctx* ctx, const sw_align_args* a, const int8_t* pssm);

/* Building a PSSM: the weighted residue counts of a query's aligned hits ("Building a PSSM").  The n hits are
 * what sw_align_hits / sw_align_hits_pssm wrote for them (results, CIGAR words) and their subjects; the master sequence
 * `query` is one more sequence, index n, with residue query[i] at every position i where query[i] < 20.
 *   A hit takes part when its include byte is non-zero (include == NULL: every hit), its status is SW_ALIGN_OK and its
 *   cigar_len > 0.  It has residue a at query position i when a '=' or 'X' column of its CIGAR pairs position i with the
 *   subject code a < 20; 'I' and 'D' columns and subject codes of 20 and above contribute nothing.
 *   counts[i][a]  (uint32, qlen x 20) = sequences (master included) that have residue a at i; k_i = the a with counts > 0
 *   weights[h]    (uint64, n + 1)     = sum over the (i, a) of sequence h of floor(2^32 / (k_i * counts[i][a])): position-based
 *                                       sequence weights (Henikoff & Henikoff 1994) in fixed point; 0 for a hit that takes no part
 *   wcounts[i][a] (uint64, qlen x 20) = sum of weights[h] over the sequences h that have a at i
 *   used          (int32)             = hits that took part
 * Integer arithmetic throughout: the result does not depend on any order of summation.  All pointers are DEVICE pointers;
 * query may be NULL (no master row), include may be NULL.  The call zeroes its outputs itself and is asynchronous on
 * `stream`.  n == 0 is legal (the master alone).  SW_ERR_INVALID: qlen < 1, qlen > SW_PSSM_MAX_QUERY_LEN, n < 0, a null
 * output, or n > 0 with a null chars / offsets / lengths / results / cigar; counts must be 16-byte aligned. */
typedef struct sw_pssm_accumulate_args {
    const int8_t* query;         /* master codes, qlen; NULL: no master row */
    int32_t qlen;
    int32_t n;                   /* hits */
    const int8_t* chars;         /* the subjects, as in sw_align_args */
    const uint64_t* offsets;     /* n + 1 */
    const int32_t* lengths;      /* n */
    const sw_align_result* results;   /* n, as the aligner wrote them; cigar_offset is honoured */
    const uint32_t* cigar;
    const uint8_t* include;      /* n, or NULL */
    uint32_t* counts;            /* out: qlen x 20 */
    uint64_t* weights;           /* out: n + 1, entry n is the master's */
    uint64_t* wcounts;           /* out: qlen x 20 */
    int32_t* used;               /* out */
    void* const* phase_events;   /* HOST, optional: 3 hipEvent_t recorded on `stream` before the memsets and the counting
                                    launch, between the two launches and after the weighting launch */
    void* stream;
} sw_pssm_accumulate_args;

int sw_pssm_accumulate(sw_ctx* ctx, const sw_pssm_accumulate_args* a);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_PSSM_H */
