/* cudasw4_amd_hsps.h — hit alignment with up to N non-overlapping local alignments per (query, subject) pair
 * (Waterman-Eggert; what BLAST calls -max_hsps).  An extension of sw_align_hits / sw_align_hits_pssm.
 *
 * For one pair the alignments are numbered k = 0 .. max_hsps - 1.  U_k is the set of cells (i, j) that are aligned pairs
 * ('=' or 'X' columns) of alignments 0 .. k-1; U_0 is empty.  Alignment k is what the four steps of sw_align_hits give
 * when the substitution score of every cell of U_k is minus infinity in all three passes: only the diagonal move INTO a
 * used cell is unavailable, gaps may run through it, so a later alignment may cross an earlier one but never shares a pair
 * with it.  Tie rules and traceback preferences are those of sw_align_hits.  Hence S_0 >= S_1 >= ..., the pair sets of one
 * hit's alignments are disjoint, each CIGAR rescored with the plain scores gives its S_k, and every alignment begins and
 * ends with an aligned pair that scores above 0.
 *
 * Layout: a->results holds n * max_hsps records and a->cigar_offsets n * max_hsps + 1 entries; slot (i, k) has index
 * i * max_hsps + k in both, and the cigar_offset of a record is its slot's offset.  Every record is written.
 *   slot 0    exactly the record of sw_align_hits for the pair (a->expected_scores and SW_ALIGN_SCORE_MISMATCH included; a
 *             subject over max_subject_len keeps cigar_offset 0); min_score does not apply to it.
 *   slot k>0  S_k < min_score: slot k and all behind it are SW_ALIGN_EMPTY (score 0, coordinates -1, no CIGAR);
 *             behind an SW_ALIGN_EMPTY slot every slot is SW_ALIGN_EMPTY;
 *             behind a slot that is SW_ALIGN_NO_TRACE, SW_ALIGN_SCORE_MISMATCH or SW_ALIGN_BAD_LENGTH every slot is
 *             SW_ALIGN_NOT_COMPUTED (score 0, coordinates -1, cigar_len 0): the pairs of an alignment that was not traced
 *             are unknown, so nothing behind it is defined.  A CIGAR slot too small for alignment k gives slot k
 *             SW_ALIGN_NO_TRACE like a rectangle over a->trace_bytes.
 * SW_ERR_INVALID, before anything is launched: max_hsps outside 1 .. SW_MAX_HSPS; min_score < 1; SW_ALIGN_COORDS_ONLY or a
 * non-NULL a->phase_events with max_hsps > 1.
 * Scratch: the sizing call (a->temp == NULL) reports, per pair, the scratch of sw_align_hits plus (max_hsps - 1) * qlen int32
 * (the used pairs: the subject column each earlier alignment pairs with a query row).  With less scratch the pairs run in
 * chunks; all rounds of a pair run inside its chunk.  Within a chunk the launches are round-major and phase-major.
 * max_hsps == 1 is sw_align_hits / sw_align_hits_pssm: the same launches, records and CIGAR words, byte for byte. */
#ifndef CUDASW4_AMD_HSPS_H
#define CUDASW4_AMD_HSPS_H

#include "cudasw4_amd_pssm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SW_MAX_HSPS 16
#define SW_ALIGN_NOT_COMPUTED 5   /* sw_align_result::status: behind an alignment that has no traceback */

typedef struct sw_hsp_args {
    int32_t max_hsps;    /* 1 .. SW_MAX_HSPS alignments per pair */
    int32_t min_score;   /* >= 1: alignments k >= 1 that score less are not reported */
} sw_hsp_args;

int sw_align_hsps(sw_ctx* ctx, const sw_align_args* a, const sw_hsp_args* h);
/* pssm and a->query as in sw_align_hits_pssm; a used cell vetoes pssm[i][s_j] in the same way */
int sw_align_hsps_pssm(sw_ctx* ctx, const sw_align_args* a, const sw_hsp_args* h, const int8_t* pssm);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_HSPS_H */
