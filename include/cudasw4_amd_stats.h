/* cudasw4_amd_stats.h — search statistics: the device side of Z-scores and E-values.
 *
 * An extension (the reference reports raw scores only).  The statistics are the regression-scaled ones of FASTA / SSEARCH
 * (Pearson 1998): the scores of unrelated subjects are regressed on ln(subject length), a score becomes a Z-score and the
 * Z-score an extreme-value probability.  All the fit needs is a small integer table — a 2-D histogram of (length bin, score)
 * over every subject of a scan — and that table is what this header's one entry point computes, from the score array a scan
 * leaves on the device.  The fit itself is host code (libcudasw4_host.so: swdrv_stats_from_histogram).
 */
#ifndef CUDASW4_AMD_STATS_H
#define CUDASW4_AMD_STATS_H

#include "cudasw4_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SW_STATS_LBINS 64    /* half-octave length bins: SW_MAX_SUBJECT_LEN = 2^28 reaches bin 56 */
#define SW_STATS_SBINS 256   /* scores 0 .. 254, and 255 = "255 or more" */

/* Add the n subjects (scores[i], lengths[i]) to the table.
 *   length bin of a true length L >= 2: e = floor(log2 L), bin = 2 e + ((L >> (e - 1)) & 1); L <= 1: bin 0
 *   score >= 0:  hist[bin][min(score, 255)] += 1 (uint32, SW_STATS_LBINS x SW_STATS_SBINS, row-major) and
 *                sumlen[bin] += max(L, 0) (uint64, SW_STATS_LBINS)
 *   score <  0 (the -1 of padding, the -2 of a failed pipeline stage; also NaN): *skipped += 1, nothing else
 * Scores are the integer-valued floats the scans write.  The call ADDS into its outputs — the caller zeroes them — so the
 * calls over batches, lanes, shards and GPUs sum to the table of the whole; integer arithmetic throughout: the table does
 * not depend on any order.  All pointers are DEVICE pointers; scores and lengths need 4-byte alignment only (any
 * `scores + k` is legal), sumlen 8-byte alignment.  Asynchronous on `stream`; n == 0 is a no-op.
 * SW_ERR_INVALID: null context, n < 0, or n > 0 with a null pointer. */
int sw_score_histogram(sw_ctx* ctx, const float* scores, const int32_t* lengths, int64_t n, uint32_t* hist, uint64_t* sumlen,
                       uint32_t* skipped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_STATS_H */
