/* cudasw4_amd_rank.h — ranking by E-value: the device side.
 *
 * An extension (the reference ranks by raw score).  Under the statistics of DESIGN.md §12 a subject's E-value falls as its
 * Z-score rises, so the list "by E-value" is the list of the largest Z-scores.  sw_zscore_keys turns the scores a scan left
 * on the device into float Z-score keys, sw_topk (cudasw4_amd.h) selects over them with the identity as its ids, and
 * sw_gather_hits turns the positions it chose back into raw scores and ids.  The fit the keys need is host code
 * (libcudasw4_host.so: swdrv_stats_from_histogram), and so is the final order of the few candidates (swdrv_rank_order).
 */
#ifndef CUDASW4_AMD_RANK_H
#define CUDASW4_AMD_RANK_H

#include "cudasw4_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the key of a subject that was not scored (score < 0: the -1 of padding, the -2 of a failed pipeline stage; also NaN):
 * below every real key */
#define SW_RANK_KEY_NONE (-3.0e38f)
/* real keys are clamped to +-SW_RANK_KEY_LIMIT, so a key is never infinite (Z-scores of that size do not occur) */
#define SW_RANK_KEY_LIMIT (2.9e38f)

/* keys[i] of the n subjects (scores[i], lengths[i]) under the fit (a, b1, sd > 0):
 *   scores[i] >= 0:  z = (scores[i] - a - b1 ln(max(lengths[i], 1))) / sd in double precision, keys[i] = (float) z
 *   otherwise:       keys[i] = SW_RANK_KEY_NONE
 * positions (may be NULL): positions[i] = i — the `ids` of a sw_topk over the keys, which then returns positions.
 * *count (uint64) is INCREASED by the number of subjects with scores[i] >= 0 and z >= z_min, compared in double precision
 * before the rounding to float; the caller zeroes it, and the calls over shards and GPUs sum.  z_min = -DBL_MAX counts every
 * scored subject.
 * All pointers are DEVICE pointers; scores, lengths, keys and positions need 4-byte alignment only (any `scores + k`,
 * `lengths + j`, `keys + m` is legal), count 8-byte alignment.  Asynchronous on `stream`; n == 0 is a no-op.
 * SW_ERR_INVALID, and nothing is launched: null context, sd <= 0, a, b1, sd or z_min not finite, n < 0, n >= 2^31, or n > 0
 * with a null scores, lengths, keys or count. */
int sw_zscore_keys(sw_ctx* ctx, const float* scores, const int32_t* lengths, int64_t n, double a, double b1, double sd,
                   double z_min, float* keys, int32_t* positions, unsigned long long* count, void* stream);

/* out_scores[j] = scores[positions[j]], out_ids[j] = ids[positions[j]] for the k positions a sw_topk over keys chose; a
 * position of -1 (its padding when n < k) gives (-1, -1).  Positions index scores and ids; all pointers are DEVICE pointers.
 * Asynchronous on `stream`; k == 0 is a no-op.  SW_ERR_INVALID: null context, k < 0, or k > 0 with a null pointer. */
int sw_gather_hits(sw_ctx* ctx, const int32_t* positions, int k, const float* scores, const int32_t* ids, float* out_scores,
                   int32_t* out_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_RANK_H */
