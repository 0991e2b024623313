/* cudasw4_amd_mask.h — low-complexity masking of the subjects on the device (what MMseqs2 and DIAMOND do to
 * their targets by default and FASTA / SSEARCH honour from pseg).
 *
 * An extension (the reference scans the subjects as they are).  A subject with a low-complexity tract — poly-Q, an S/G/A-rich
 * linker, a two- or three-letter repeat — scores high against every query that holds a similar tract, whatever their
 * descent; neither the regression on ln(length) nor the calibration on shuffled subjects models that, because shuffling keeps
 * the composition.  This header's one entry point replaces such tracts by code 20 (X), which scores like an unknown residue.
 *
 * The rule (integers only; the kernel, the host library — swh::mask_subject — and the tests' numpy statement agree bit for
 * bit).  Parameters: a window W, 4 <= W <= 32, and two sums with 1 <= extend_sum <= trigger_sum.
 *   U[n] = round(1024 log2 n), n = 1 .. 32, U[0] = 0: SW_MASK_U_TABLE below, literals; nothing calls log2 at run time
 *   for a subject of true length L (a negative length counts as 0, one over the subject's padded size as that size):
 *   1. window i covers positions [i, i + W), 0 <= i <= L - W (L < W: no window)
 *   2. S_i = sum over the codes a < 20 of n_a U[n_a], n_a = positions of the window with code a.  Codes >= 20 count for
 *      nothing: every such position is a letter of its own.  With no such code in the window its Shannon entropy is
 *      log2 W - S_i / (1024 W) bits
 *   3. lo(i) = S_i >= extend_sum, trig(i) = S_i >= trigger_sum
 *   4. a run is a maximal interval [a, b] of window starts with lo true throughout
 *   5. if any window of the run has trig, positions [a, b + W) are masked: they get code 20
 * These are the trigger and the extension stage of SEG (Wootton & Federhen 1993) on a fixed window; SEG's third stage, which
 * trims a segment to its least probable sub-segment, is not part of the rule, so a masked segment reaches up to W - 1
 * residues into each flank.  Masking is idempotent (a masked position can only lower the n_a of the windows over it), and the
 * result of a subject depends on that subject alone.
 *
 * Bits to sums: threshold(W, K) = max(1, ceil(1024 W (log2 W - K))), in double precision, once, on the host
 * (libcudasw4_host.so: swdrv_mask_threshold).  W = 12 with K = 1.9 / 2.2 bits gives 20705 / 17019.
 */
#ifndef CUDASW4_AMD_MASK_H
#define CUDASW4_AMD_MASK_H

#include "cudasw4_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SW_MASK_MIN_WINDOW 4
#define SW_MASK_MAX_WINDOW 32
#define SW_MASK_CODE 20
/* U[0 .. 32] */
#define SW_MASK_U_TABLE                                                                                                        \
    0, 0, 1024, 1623, 2048, 2378, 2647, 2875, 3072, 3246, 3402, 3542, 3671, 3789, 3899, 4001, 4096, 4186, 4270, 4350, 4426,   \
        4498, 4566, 4632, 4695, 4755, 4813, 4869, 4923, 4975, 5025, 5073, 5120

typedef struct sw_mask_params {
    int32_t window;
    int32_t trigger_sum;
    int32_t extend_sum;
} sw_mask_params;

/* Mask the n subjects (chars, offsets, lengths: dbdata layout, the contract of sw_shuffle_subjects: offsets[i] - offsets[0] =
 * byte offset of subject i in `chars`, offsets[n] ends the block, every subject starts on a multiple of 4 bytes; `chars`
 * points at the first subject of the range and `offsets` at its offset, so a sub-range of a database is legal).  All pointers
 * are DEVICE pointers.
 *   out      == chars: in place; only dwords that hold a masked position are written.
 *            An `out` that does not overlap the block gets the whole block: the masked copy, padding bytes as they are; the
 *            bytes behind the block are not touched.  A partial overlap is SW_ERR_INVALID.
 *   temp     scratch, 8-byte aligned.  temp == NULL: only *temp_bytes_needed is written — the scratch that takes all n
 *            subjects in one go (24 bytes per 64 bytes of the block) — and nothing is launched.  With less the call works
 *            through ranges of whole subjects that fit (and reads the offsets back to find them); scratch that cannot hold
 *            the longest subject is SW_ERR_INVALID, and the message names the need.  temp_bytes_needed may be NULL otherwise.
 *   counts   NULL, or DEVICE uint64[2] the call ADDS to: [0] positions covered by masked segments, [1] subjects with at
 *            least one segment.
 * The two ends of the block are read back first (the call waits for what `stream` holds so far); the masking itself is
 * asynchronous on `stream`: per range three launches in stream order (flags, resolve, apply), which is also what makes the
 * in-place form safe.  n == 0 is a no-op.
 * SW_ERR_INVALID: null context or params, n < 0, a window outside 4 .. 32, sums out of order or below 1; with work to do, a
 * null chars / offsets / lengths / out, a misaligned pointer (chars, out, lengths: 4 bytes; offsets, temp, counts: 8). */
int sw_mask_subjects(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t n,
                     const sw_mask_params* p, int8_t* out, void* temp, size_t temp_bytes, size_t* temp_bytes_needed,
                     unsigned long long* counts, void* stream);

/* Measurement (tools/mask_bench.py): sw_mask_subjects with four events (hipEvent_t, created by the caller with timing on)
 * recorded on `stream` before the flags, the resolve and the apply launch and behind the last one.  The scratch must take
 * the block in one go (SW_ERR_INVALID otherwise): one range, three launches. */
int sw_mask_subjects_phases(sw_ctx* ctx, const int8_t* chars, const uint64_t* offsets, const int32_t* lengths, int32_t n,
                            const sw_mask_params* p, int8_t* out, void* temp, size_t temp_bytes, unsigned long long* counts,
                            void* stream, void* const* phase_events);

#ifdef __cplusplus
}
#endif
#endif /* CUDASW4_AMD_MASK_H */
