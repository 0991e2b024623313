/* cudasw4_amd_shuffle.h — shuffled subjects: the device side of the search statistics calibrated on permuted subjects
 * (what FASTA / SSEARCH offer as -z 11 .. and PRSS does).
 *
 * An extension (the reference reports raw scores only).  A subject whose residues are permuted keeps its length and its
 * composition and loses its homology to anything, so the scores of a query against shuffled subjects are scores of
 * unrelated subjects whatever the database holds.  This header's one entry point writes replicas of a block of subjects
 * with every subject permuted; the scans (sw_scan_partition), the table (sw_score_histogram, cudasw4_amd_stats.h) and the
 * fit (libcudasw4_host.so: swdrv_stats_from_histogram) are the existing ones.
 *
 * The permutation is a function of (seed, subject key, replica, true length) alone — no state, no order:
 *   mix32(x):  x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16          (uint32)
 *   k = mix32(mix32(mix32(mix32(seed) ^ lo32(id)) ^ hi32(id)) ^ replica)
 *   L >= 2:  h = max(1, (bit_length(L - 1) + 1) / 2), mask = 2^h - 1;  one Feistel pass on c:  l = c >> h, r = c & mask;
 *            for rd = 0 .. 3:  f = mix32(r ^ k ^ (rd * 0x9e3779b9)) & mask, (l, r) = (r, l ^ f);  c = (l << h) | r
 *            pi(i): c = i, the pass repeated until c < L (cycle walking);  out[i] = in[pi(i)]
 *   L <= 1:  a copy
 * The pass is a bijection of [0, 2^(2h)) and 2^(2h) < 4 L, so pi is a bijection of [0, L) and a walk takes fewer than four
 * passes on average.
 */
#ifndef CUDASW4_AMD_SHUFFLE_H
#define CUDASW4_AMD_SHUFFLE_H

#include "cudasw4_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Write replicas first_replica .. first_replica + replicas - 1 of the n subjects (chars, offsets, lengths: dbdata layout, as
 * for sw_scan_partition; offsets[i] - offsets[0] = byte offset of subject i in `chars`, offsets[n] ends the block) to `out`:
 * replica r of the call (0-based) starts at out + r * replica_stride and has the layout of the input — the same offsets,
 * subject i permuted with the key of (seed, keys[i], first_replica + r), every padding byte code 20.  Every byte of the
 * block is written in every replica; the bytes between a replica's end and the next replica's start are not touched.
 *   keys            DEVICE int64[n], or NULL: the position i
 *   lengths         true lengths; a length over the subject's padded size counts as that size
 *   replica_stride  a multiple of 4, at least offsets[n] - offsets[0]
 * All pointers are DEVICE pointers; `chars` points at the first subject of the range and `offsets` at its offset, so a
 * sub-range of a database is legal; out is 4-byte aligned and must not overlap chars.  The two ends of the block are read
 * back first (the call waits for what `stream` holds so far); the shuffle itself is asynchronous on `stream`.  n == 0 or
 * replicas == 0 is a no-op.
 * SW_ERR_INVALID: null context, negative n / replicas / first_replica, a replica_stride that is no multiple of 4; with work
 * to do, a null chars / offsets / lengths / out, a misaligned pointer, a replica_stride smaller than the block. */
int sw_shuffle_subjects(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, const int64_t* keys,
                        int32_t n, uint32_t seed, int32_t first_replica, int32_t replicas, int8_t* out, size_t replica_stride,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_SHUFFLE_H */
