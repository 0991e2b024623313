/* cudasw4_amd_driver.h — C ABI of libcudasw4_host.so: the C++ host driver (DB sharding over the GPUs
 * of a node, residency / batch streaming, partition walk, overflow re-score, per-GPU top-K, host merge)
 * for embedding and tests.  It mirrors the public surface of the reference's class CudaSW4
 * (cudasw4.cuh:496-839) the way `align` uses it (main.cu:157-259):
 *
 *   swdrv_create       CudaSW4::CudaSW4(deviceIds, numTop, blosumType, KernelTypeConfig, MemoryConfig, verbose)
 *   swdrv_open_db      loadDB(prefix) + setDatabase            (dbdata.cpp:207-222, cudasw4.cuh:552-568)
 *   swdrv_pseudo_db    loadPseudoDB(num, length) + setDatabase (dbdata.hpp:222-272)
 *   swdrv_upload       prefetchDBToGpus                        (cudasw4.cuh:651-696)
 *   swdrv_scan         scan(query, length) -> ScanResult       (cudasw4.cuh:698-765)
 *
 * All calls return 0 on success, -1 on error (text from swdrv_last_error()).  Scores are computed only by
 * libcudasw4_amd.so; there is no CPU path.
 */
#ifndef CUDASW4_AMD_DRIVER_H
#define CUDASW4_AMD_DRIVER_H

#include <stddef.h>
#include <stdint.h>

#include "cudasw4_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct swdrv swdrv;

const char* swdrv_last_error(void);

/* devices/ndev: HIP device ids; ndev = 0 -> all visible devices.
 * matrix: 45 | 50 | 62 | 80 (the 21-letter tables) or 4525 | 5025 | 6225 | 8025 (the full 25-letter tables: the query
 * is then encoded with 25 letters, the DB stays the 21-code dbdata alphabet, see include/cudasw4_amd.h).  kinds: SW_KIND_* for single / many_small / many_large / overflow.
 * max_gpu_mem = 0 -> unlimited. */
int swdrv_create(const int* devices, int ndev, int num_top, int matrix,
                 int kind_single, int kind_many_small, int kind_many_large, int kind_overflow,
                 size_t max_gpu_mem, size_t max_batch_bytes, size_t max_batch_sequences, size_t max_temp_bytes,
                 int gop, int gex, int verbose, swdrv** out);
int swdrv_destroy(swdrv* d);

int swdrv_open_db(swdrv* d, const char* prefix, int prefetch);
int swdrv_pseudo_db(swdrv* d, size_t num, int32_t length);
/* DB from arrays already in dbdata layout (ascending length, every subject padded to a multiple of 4 with code 20);
 * the arrays are copied.  Subject i gets the header "S". */
int swdrv_db_from_arrays(swdrv* d, const int8_t* chars, size_t nchars, const uint64_t* offsets, const int32_t* lengths, size_t n);
/* One process per GPU: this driver scans shards rank*ngpu .. rank*ngpu+ngpu-1 of world*ngpu char-balanced shards of
 * every length partition (partitionDBAmongstGpus over all GPUs of the job, cudasw4.cuh:928-1004); reported ids stay
 * global (+ id_base).  Call before swdrv_open_db / swdrv_pseudo_db / swdrv_db_from_arrays. */
int swdrv_set_shard(swdrv* d, int rank, int world, int64_t id_base);
int swdrv_upload(swdrv* d);
int64_t swdrv_num_sequences(swdrv* d);
int swdrv_num_gpus(swdrv* d);
int swdrv_set_num_top(swdrv* d, int num_top);

/* query: residue letters (not encoded).  scores/ids: capacity `cap`; *nres = number of results written.
 * *num_overflows: subjects whose exact score reached the packed kind's limit (2048 / 25000) — the reference's "num
 * overflows" (main.cu:243-245); swdrv_last_rescored: how many subjects the last scan re-scored in 32 bits (>= that). */
int swdrv_scan(swdrv* d, const char* query, int32_t qlen, int32_t* scores, int64_t* ids, int cap,
               int* nres, int* num_overflows, double* seconds, double* gcups);
int swdrv_last_rescored(swdrv* d);

/* The same scan in two halves (SearchDriver::submit / collect): swdrv_scan_submit enqueues everything the query needs on
 * every GPU and returns without waiting; swdrv_scan_collect waits for the OLDEST submitted query and returns its merged
 * results.  At most two queries may be in flight, so a caller that knows its next query (align reads whole query files,
 * main.cu:157-259) submits it before collecting the current one and the GPUs never idle between queries.  Results are
 * the same as swdrv_scan's. */
int swdrv_scan_submit(swdrv* d, const char* query, int32_t qlen);
int swdrv_scan_collect(swdrv* d, int32_t* scores, int64_t* ids, int cap, int* nres, int* num_overflows, double* seconds,
                       double* gcups);
int swdrv_in_flight(swdrv* d);

/* Profile search (an extension; include/cudasw4_amd_pssm.h): the query is a position-specific scoring matrix, qlen x 21
 * int8, row i = query position i, column c = dbdata subject code c (0..19 = ARNDCQEGHILKMFPSTWYV, 20 = other / padding:
 * negative in every row).  The driver's matrix is not used; its gap scores, shards, residency, streaming and merge are, and
 * the results have the layout of swdrv_scan's.  swdrv_scan_submit_pssm pairs with swdrv_scan_collect, so a PSSM query and
 * a letter query can be in flight together.  The hits of a PSSM query are aligned with swdrv_align_hits_pssm. */
int swdrv_scan_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, int32_t* scores, int64_t* ids, int cap,
                    int* nres, int* num_overflows, double* seconds, double* gcups);
int swdrv_scan_submit_pssm(swdrv* d, const int8_t* pssm, int32_t qlen);

/* ---- measurement / verification hooks (bench.py, tests) ----
 * Kernel events: HIP events around every DP launch on the stream it runs on.  take: 15 doubles per launch
 * (gpu index, kind, part_id, query length, subjects, cells, padded subject bytes, milliseconds, begin ms, end ms — these
 * two on the device clock since recording was switched on: launches on different streams overlap, the union of the
 * intervals is the time the DP kernels kept the GPU busy — and the kernel instantiation: kind computed in, rows per lane,
 * query stripes, lanes per group; last: 1 for an overflow re-score launch, whose cells / bytes are 0 — the length of
 * its list is only known on the device); returns the number of launches recorded since the last call
 * (may exceed cap), -1 on error. */
int swdrv_record_kernel_events(swdrv* d, int on);
int swdrv_take_kernel_events(swdrv* d, double* out, int cap);
int swdrv_shard_info(swdrv* d, int gpu, int64_t* num_local, int64_t* residues, int64_t* chars, int* resident);
/* hybrid residency (cudasw4.cuh:1044-1046,1087-1144): padded subject bytes of the GPU's shard that stay in device memory
 * (== chars when the shard is resident, 0 when all of it is streamed); -1 on error */
int64_t swdrv_cached_chars(swdrv* d, int gpu);
/* subject bytes copied host -> device by scans since swdrv_create (the one-time upload of resident / cached chars is
 * not counted): the bus traffic of streamed shards */
int64_t swdrv_streamed_bytes(swdrv* d);
/* every score of the last scan on GPU `gpu` (shard order) and the global id of every position (the
 * CUDASW_DEBUG_CHECK_CORRECTNESS view, cudasw4.cuh:728-756); num_local entries each */
int swdrv_last_scores(swdrv* d, int gpu, float* scores, int64_t* ids);
/* last streamed scan: (gpu index, begin ms, end ms) per batch, device clock relative to that GPU's scan start */
int swdrv_batch_intervals(swdrv* d, float* out, int cap);
/* last scan: (begin s, end s) per GPU on the host clock, relative to the scan's start */
int swdrv_gpu_spans(swdrv* d, double* out, int cap);
/* The launch planner (no GPU needed): runs of a length-sorted subject list, largest partition first;
 * 5 int64 per run (kind, part_id, begin, end, max length); returns the number of runs, -1 on error. */
int swdrv_plan_runs(const int32_t* sorted_lengths, size_t n, int kind_single, int kind_many_small, int kind_many_large,
                    int64_t* out, int cap);
/* the same; latency_mode != 0: the plan of the driver's latency mode (swdrv_latency_scans) — partition 34 keeps a launch
 * of its own whatever its size */
int swdrv_plan_runs_mode(const int32_t* sorted_lengths, size_t n, int kind_single, int kind_many_small, int kind_many_large,
                         int latency_mode, int64_t* out, int cap);

/* partitionDBAmongstGpus (cudasw4.cuh:928-1004) on raw arrays (no GPU needed): out[(rank*36 + partition)*2 + {0,1}] =
 * begin / end of the subject range of `rank` in `partition`. */
int swdrv_shard_ranges(const int32_t* sorted_lengths, const uint64_t* offsets, size_t n, int world, int64_t* out);

/* The residency decision of one GPU's shard (no GPU needed; GpuWorkingSet + assignBatchesToGpuMem + computeDbCopyPlan,
 * cudasw4.cuh:317-392,1087-1144,1177-1277): local_offsets[n + 1] = byte offsets of the shard's subjects in ascending
 * length, max_len its longest subject, free_mem what the device has free, the limits as in swdrv_create (0 = default).
 * -> *cache_begin: subjects [cache_begin, n) keep their chars in device memory (0: the shard is resident), *cache_bytes
 * their bytes, *batch_bytes the batch size of the streamed rest, batches[2 i], [2 i + 1] = begin / end of streamed batch
 * i; *temp_per_stream (may be NULL): what each of the 4 stripe-border scratch buffers of a GPU (work, second work, two
 * auxiliary streams) may grow to, so that cached chars + 3 staging buffers + 4 scratch buffers + 24 bytes per subject fit
 * the limit (from 4.3 GiB up; below that the 256 MiB floor per buffer wins); returns the number of batches (may exceed
 * cap), -1 on error.  allow_cache = 0: all-or-nothing residency. */
int swdrv_plan_residency(const uint64_t* local_offsets, size_t n, int32_t max_len, size_t max_gpu_mem, size_t max_batch_bytes,
                         size_t max_batch_sequences, size_t max_temp_bytes, size_t free_mem, int allow_cache,
                         int64_t* cache_begin, int64_t* cache_bytes, int64_t* batch_bytes, int64_t* batches, int cap,
                         int64_t* temp_per_stream);

/* long subjects scanned as overlapping windows (exact for short queries, include/cudasw4_amd.h: sw_window_overlap): side
 * launches that did so and windows scanned since swdrv_create */
int swdrv_window_stats(swdrv* d, int64_t* launches, int64_t* windows);
/* re-score service launches (include/cudasw4_amd.h: sw_rescore_service) since swdrv_create: the bulk launch's overflow list
 * re-scored while it was being filled.  CUDASW4_AMD_RESCORE_SERVICE=0|1 forces the service off / on; by default it runs
 * while recent scans re-scored anything. */
int64_t swdrv_service_launches(swdrv* d);
/* side launches of the longest subjects (partitions 34 / 35) that ran as pipelines of one-wave stages over many compute
 * units (sw_scan_rows_pipelined) since swdrv_create: taken when the one-wave-per-subject launch would be what the scan
 * waits for (shards of a real DB, short queries) */
int64_t swdrv_pipeline_launches(swdrv* d);
/* 1: the start handshake (sw_probe_handshake) holds on every GPU of the driver — side launches, re-score service and tail
 * hand-over are in use; 0: the driver fell back to plain stream order (a profiler that serialises kernels, ...) */
int swdrv_handshake_active(swdrv* d);
/* queries a caller with a query file should keep pending once a query of this length has been submitted: 1, or 2 where the tail
 * hand-over applies (up to SearchDriver::kMaxInFlight = 4 may be pending; more than two was measured and is slower) */
int swdrv_preferred_in_flight(swdrv* d, int32_t query_length);
/* scans planned in LATENCY MODE since swdrv_create: partition 34 (1281 ... 8000 residues) on wave-wide groups beside the
 * bulk launch instead of inside it, when the whole launch is short against the walk of its longest subject on 16 lanes
 * (small shards of real DBs).  CUDASW4_AMD_LATENCY_MODE=never|always overrides the estimate. */
int64_t swdrv_latency_scans(swdrv* d);
/* Tail hand-over between two queries in flight (include/cudasw4_amd.h: sw_set_dry_signal): a query submitted with
 * swdrv_submit while the one before is still pending runs on a second lane of the GPU (context, work stream, score arrays)
 * and its bulk launch starts when the earlier one's work counter runs dry, filling the slots its last round leaves idle —
 * on resident shards of a few rounds of workgroups (what each of N GPUs gets from a small DB) and for queries that are
 * scanned in a few milliseconds; results are those of swdrv_scan.  Returns the queries gated that way since swdrv_create.  CUDASW4_AMD_TAIL_OVERLAP=0 turns the hand-over
 * off, =1 lifts the shard-size rule. */
int64_t swdrv_tail_overlaps(swdrv* d);
/* 1 when the hand-over applies — the loaded DB's shards are small (at most 20 rounds of workgroups: 491 520 subjects on 256 CUs), or a query of
 * query_length residues (0: not considered) is scanned in a few milliseconds (<= 8 ms at 10 TCUPS: short queries, whatever
 * the DB) —: a caller with its next query at hand should then swdrv_submit it before it collects the current one (`align`
 * and bench.py do) */
int swdrv_prefers_two_in_flight(swdrv* d, int32_t query_length);

/* NUMA placement: the node of the gpu-th GPU's PCI function (-1: unknown) and its HIP device ordinal.  In-process
 * multi-GPU drivers run each GPU's worker thread on that node themselves; a one-process-per-GPU caller binds its own
 * thread with swdrv_bind_to_numa_node (0: bound; -1: unknown node or none of its CPUs allowed, affinity unchanged). */
int swdrv_numa_node(swdrv* d, int gpu);
int swdrv_device_of(swdrv* d, int gpu);
int swdrv_device_numa_node(int device);   /* the same for a HIP device ordinal, before any driver exists */
int swdrv_bind_to_numa_node(int node);

/* header / length of a subject by global id (getReferenceHeader / getReferenceLength) */
int32_t swdrv_reference_length(swdrv* d, int64_t id);
int swdrv_reference_header(swdrv* d, int64_t id, char* buf, int cap);

/* Hit alignment (an extension: the reference is score-only): coordinates, counts and CIGAR of the n hits `ids` / `scores`
 * of a scan of `query` (residue letters, the query the hits were scanned with), computed with sw_align_hits on the first GPU
 * of the driver, with a context and a stream of its own.  Call after the scan's collect; the scan's matrix and gap scores
 * apply.  results[i].cigar_offset indexes `cigar`, where the hits' CIGARs lie back to back (qlen + length of every hit words
 * always suffice; cigar_cap is checked).  A hit whose recomputed score differs from its scan score is an error.  The trace
 * budget of one pair follows max_temp_bytes: pairs whose rectangle is over it get SW_ALIGN_NO_TRACE (coordinates only). */
int swdrv_align_hits(swdrv* d, const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, int n,
                     sw_align_result* results, uint32_t* cigar, int64_t cigar_cap);
/* The same for the hits of a PSSM query (sw_align_hits_pssm, include/cudasw4_amd_pssm.h).  pssm: the qlen x 21 int8 scores the
 * hits were scanned with (host).  consensus: qlen residue letters that identities and the CIGAR's '=' / 'X' are counted
 * against (a non-standard letter, '*' or '-' is identical to nothing), or NULL: the best-scoring standard residue of
 * every row, the first of equals.  Gap scores, trace budget, outputs and errors as above; the driver's matrix is not used. */
int swdrv_align_hits_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                          const int32_t* scores, int n, sw_align_result* results, uint32_t* cigar, int64_t cigar_cap);
/* Up to max_hsps (1 .. 16) non-overlapping local alignments per hit (sw_align_hsps / sw_align_hsps_pssm,
 * include/cudasw4_amd_hsps.h).  results: n * max_hsps records, slot (i, k) at i * max_hsps + k: slot 0 is the
 * record of the calls above; alignments k >= 1 that score below min_score (>= 1) are not reported (SW_ALIGN_EMPTY from there
 * on); behind a slot without traceback the slots are SW_ALIGN_NOT_COMPUTED (5).  cigar: the CIGARs of all slots back to
 * back (max_hsps * (qlen + length) words per hit always suffice).  Everything else as above; the used pairs of a hit take
 * (max_hsps - 1) * qlen * 4 bytes of its share of max_temp_bytes. */
int swdrv_align_hsps(swdrv* d, const char* query, int32_t qlen, const int64_t* ids, const int32_t* scores, int n, int max_hsps,
                     int min_score, sw_align_result* results, uint32_t* cigar, int64_t cigar_cap);
int swdrv_align_hsps_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, const char* consensus, const int64_t* ids,
                          const int32_t* scores, int n, int max_hsps, int min_score, sw_align_result* results, uint32_t* cigar,
                          int64_t cigar_cap);

/* Building a PSSM from a query's aligned hits (an extension; DESIGN.md, "Building a PSSM"): the step between two rounds of
 * an iterated profile search.
 *
 * The conversion alone (pure host code, no GPU needed): residue counts and weighted counts, as sw_pssm_accumulate of
 * include/cudasw4_amd_pssm.h defines them, into the qlen x 21 int8 PSSM every scan takes.  matrix: as for the driver's
 * constructor; a 25-letter matrix stands for the 21-letter table of the same name.  master_codes: dbdata codes of the
 * master sequence (20 and above: not a standard residue).  counts (uint32) and wcounts (uint64): qlen x 20.
 * pseudocount: beta > 0.  raw_out (optional): qlen x 20 doubles, the scores before rounding (rows without counts: the
 * table's entries).  lambda_out (optional): the matrix's ungapped lambda under the Robinson & Robinson background.
 * Column 20 of row i is table[min(master_codes[i], 20)][20]; a table where that is not negative is refused. */
int swdrv_pssm_from_counts(int matrix, const int8_t* master_codes, int32_t qlen, const uint32_t* counts,
                           const uint64_t* wcounts, double pseudocount, int8_t* pssm_out, double* raw_out, double* lambda_out);

typedef struct swdrv_pssm_info {
    int32_t used;          /* hits that took part */
    int32_t below_score;   /* left out: scan score below min_score */
    int32_t no_trace;      /* left out: SW_ALIGN_NO_TRACE (no CIGAR within the trace budget) */
    int32_t copies;        /* left out: a copy of the master (the whole query, all columns identical) */
    double lambda;
    uint8_t* included;     /* in: NULL, or n bytes that receive 1 for every hit that took part and 0 for the others */
} swdrv_pssm_info;

/* The whole step: align the n hits `ids` / `scores` of a scan of the master — with its letters when pssm is NULL, else
 * with `pssm` (qlen x 21 int8, the PSSM the hits were scanned with; the master's letters are the consensus) —, apply the
 * inclusion rule, accumulate on the device (sw_pssm_accumulate, on the subjects, results and CIGARs the aligner left
 * there) and convert.  A hit is left out, in this order, when its score is below min_score, when it has no CIGAR within
 * the trace budget, or when it is a copy of the master (q_begin == 0, q_end == qlen, identities == columns == qlen); hits of
 * score 0 have no alignment and take no part either.  pssm_out: qlen x 21 int8; info_out: optional. */
int swdrv_build_pssm(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                     const int32_t* scores, int n, int32_t min_score, double pseudocount, int8_t* pssm_out,
                     swdrv_pssm_info* info_out);

/* swdrv_build_pssm with the redundancy filter of sw_msa_filter (include/cudasw4_amd_msa.h) between the
 * inclusion rule and the weighting: purge_identity P in 1 .. 100 leaves out every hit that is at least P per cent identical
 * (over its own aligned residues) to the master or to an earlier hit that went in; 0: swdrv_build_pssm.  purged_out
 * (optional): how many hits that cost; info_out->used and ->included do not count them. */
int swdrv_build_pssm_purged(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                            const int32_t* scores, int n, int32_t min_score, double pseudocount, int purge_identity,
                            int8_t* pssm_out, swdrv_pssm_info* info_out, int32_t* purged_out);

/* The query-anchored multiple alignment of the n hits `ids` / `scores` of a scan of the master: the hits
 * are aligned as swdrv_align_hits does (pssm non-NULL: as swdrv_align_hits_pssm, the master's letters being the consensus),
 * and sw_msa_filter runs on what the aligner left on the device.  max_identity: 0 (no filter) or 1 .. 100.
 * Outputs, each optional: results / cigar as swdrv_align_hits writes them; rows ((n + 1) x qlen bytes, row n the master:
 * residue codes 0 .. 19, 20 other, 21 gap, 22 none), residues (n + 1), keep (n + 1), purged (1).  out_path non-NULL: the
 * kept hits are written there as swdrv_write_msa writes them, with the DB's headers and letters and `query_header`. */
int swdrv_hit_msa(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                  const int32_t* scores, int n, int max_identity, const char* query_header, const char* out_path, int format,
                  sw_align_result* results, uint32_t* cigar, int64_t cigar_cap, uint8_t* rows, int32_t* residues, uint8_t* keep,
                  int32_t* purged);

/* swdrv_hit_msa with the selection of include/cudasw4_amd_msa_select.h in place of the greedy filter:
 * min_coverage and min_query_identity in 0 .. 100 (0: no test), diff >= 0, ladder: n_ladder (1 .. 16) strictly ascending
 * rungs in 1 .. 100; at most SW_MSA_SELECT_MAX_HITS hits.  Outputs, each optional: results / cigar / rows / residues as
 * swdrv_hit_msa; state (n + 1 bytes: 0 none, 1 kept, 2 below coverage, 3 below query identity, 4 thinned), depth (qlen),
 * counts (4: kept hits, below coverage, below query identity, thinned).  out_path: the hits with state 1 are written. */
int swdrv_hit_msa_select(swdrv* d, const char* master_letters, int32_t qlen, const int8_t* pssm, const int64_t* ids,
                         const int32_t* scores, int n, int min_coverage, int min_query_identity, int diff, const int32_t* ladder,
                         int n_ladder, const char* query_header, const char* out_path, int format, sw_align_result* results,
                         uint32_t* cigar, int64_t cigar_cap, uint8_t* rows, int32_t* residues, uint8_t* state, int32_t* depth,
                         int32_t* counts);

/* The writer alone (no GPU): '>' + query_header and the master's letters, then for every hit with keep[h] != 0 (keep NULL:
 * every hit) that is SW_ALIGN_OK with a CIGAR, in the given order, '>' + headers[h] and one line: '-' before q_begin; along
 * the CIGAR the subject's letter in upper case for '=' / 'X', '-' per 'I' column, the subject's letters in lower case for
 * 'D' (format 1, FASTA: none); '-' up to the master's length.  format 0: A3M.  results[h].cigar_offset indexes `cigar`. */
int swdrv_write_msa(const char* path, int format, const char* master_letters, const char* query_header, int n,
                    const char* const* headers, const char* const* subject_letters, const sw_align_result* results,
                    const uint32_t* cigar, const uint8_t* keep);

/* The 20 standard columns of a qlen x 21 PSSM as an NCBI ASCII PSSM file (what `align --outPssm` writes and `align --pssm`
 * reads; column 20 is not part of the format).  consensus: qlen residue letters, NUL-terminated.  No GPU needed. */
int swdrv_write_pssm_ascii(const char* path, const int8_t* pssm, int32_t qlen, const char* consensus);

/* Search statistics (an extension; DESIGN.md §12, include/cudasw4_amd_stats.h): Z-scores and E-values by the regression of
 * FASTA / SSEARCH (Pearson 1998), fitted per query on the scan's own scores.
 *
 * The table: hist (uint32, 64 x 256, row-major) counts the subjects by (length bin, min(score, 255)); sumlen (uint64, 64)
 * sums the true lengths per length bin; subjects with a negative score are in neither.  Length bins are half octaves:
 * swdrv_length_bin.  Tables add: the table of several shards, ranks or GPUs is the sum of theirs.
 *
 * The fit (double precision, sums in ascending (bin, score) order): a bin with row sum n_b > 0 has x_b = ln(sumlen_b / n_b);
 * N = all cells summed; the cells (b, s) with n_b > 0 and 1 <= s <= 254 are eligible (0: no alignment; 255: censored).
 * Starting from all eligible cells, at most 10 times: over the included cells, weighted by their counts, n, the sums of x, s,
 * x^2, x s; b1 = (n Sxs - Sx Ss) / (n Sxx - Sx^2), or 0 when that denominator is 0 or fewer than two bins are included;
 * a = (Ss - b1 Sx) / n; var = sum w (s - a - b1 x_b)^2 / (n - 2); sd = sqrt(var); the next set is the eligible cells with
 * |s - a - b1 x_b| / sd <= 5; stop when the set repeats.  n < 100 or var <= 0 at any point: SWDRV_STATS_NO_FIT.
 *
 * Per hit of score S and true length L: z = (S - a - b1 ln L) / sd, P = 1 - exp(-exp(-(pi / sqrt 6) z - 0.5772156649015329)),
 * E = N P.  Under SWDRV_STATS_NO_FIT every z is 0 and every E is -1. */
#define SWDRV_STATS_OK 0
#define SWDRV_STATS_NO_FIT 1   /* (SW_STATS_NO_FIT of DESIGN.md §12) */
typedef struct swdrv_stats {
    double a, b1, sd;      /* expected score of an unrelated subject of length L: a + b1 ln L; sd of the residuals */
    int64_t n_included;    /* subjects the last regression ran over */
    int64_t N;             /* subjects scored: every cell of the table */
    int32_t rounds;        /* regressions computed */
    int32_t status;        /* SWDRV_STATS_* */
} swdrv_stats;

/* on != 0: every query submitted from now on also leaves its table (one launch of sw_score_histogram per GPU on the final
 * scores, right before the top-K).  Off (the default) nothing is allocated, launched or copied.  Not with queries in flight. */
int swdrv_set_statistics(swdrv* d, int on);
/* fit and table of the query collected last (out, hist — 64 x 256 — and sumlen — 64 — may each be NULL); an error when that
 * query was scanned with the statistics off.  A driver made with swdrv_set_shard sees its shard's table only. */
int swdrv_last_statistics(swdrv* d, swdrv_stats* out, uint32_t* hist, uint64_t* sumlen);
/* the fit alone (no GPU needed) */
int swdrv_stats_from_histogram(const uint32_t* hist, const uint64_t* sumlen, swdrv_stats* out);
/* z[i] and e[i] (each may be NULL) of n hits (no GPU needed); lengths below 1 count as 1 */
int swdrv_evalues(const swdrv_stats* stats, const int32_t* scores, const int32_t* lengths, int n, double* z, double* e);
/* half-octave length bin: L >= 2: 2 e + ((L >> (e - 1)) & 1) with e = floor(log2 L); L <= 1: 0 */
int swdrv_length_bin(int32_t length);

/* Ranking by E-value (an extension; DESIGN.md §13, include/cudasw4_amd_rank.h).  The list of a scan is the top-K by raw
 * score; under the statistics above a long subject collects b1 ln L more points than a short one by chance alone, so the
 * list by E-value — by Z-score, descending — is another one.  SWDRV_RANK_EVALUE switches the statistics on and makes every
 * query submitted from now on return the num_top subjects of largest Z-score (ties: ascending id): the scan and its table as
 * before; then, once the table is fitted, on every GPU Z-score keys of all its scores (sw_zscore_keys), sw_topk over the keys
 * and the gather of the raw scores and ids (sw_gather_hits); the GPUs' candidates are ordered on the host in double precision
 * (swdrv_rank_order).  Selection on the device runs on float keys: two subjects may change places, or trade the last place,
 * only when their Z-scores differ by less than 1e-6 max(1, |z|).  Results keep raw scores and global ids, so swdrv_align_hits,
 * swdrv_build_pssm and swdrv_evalues take them unchanged.  Where the scan allows no fit the list is the raw-score list.
 * max_evalue > 0: the subjects of the whole DB with score >= 0 and E <= max_evalue are counted as well (swdrv_last_ranking);
 * <= 0: no threshold.  Under SWDRV_RANK_EVALUE ONE query may be in flight: a second swdrv_scan_submit is an error.
 * SWDRV_RANK_SCORE (the default): the raw-score list; nothing is allocated, launched or copied beyond what the statistics
 * setting asks for (it stays as it is).  Not with queries in flight. */
#define SWDRV_RANK_SCORE 0
#define SWDRV_RANK_EVALUE 1
int swdrv_set_ranking(swdrv* d, int mode, double max_evalue);
/* of the query collected last: *count = subjects at or under the threshold, summed over the GPUs (-1: no threshold, no fit, or
 * ranked by score); *z_min = the Z-score the threshold stands for (-infinity when max_evalue >= N; 0 when count is -1).
 * Either pointer may be NULL. */
int swdrv_last_ranking(swdrv* d, int64_t* count, double* z_min);
/* The Z-score at which the E-value of a DB of N scored subjects equals X (no GPU needed): for 0 < X < N,
 * z_min = -(ln(-ln1p(-X / N)) + 0.5772156649015329) sqrt(6) / pi; X >= N: -infinity; X <= 0: +infinity; N <= 0 or NaN: NaN. */
double swdrv_zscore_for_evalue(int64_t N, double X);
/* out_order[0 .. n): the indices of n hits by Z-score under `stats` (double precision, as swdrv_evalues computes it)
 * descending, equal Z-scores by ascending id (no GPU needed): the host merge.  Under SWDRV_STATS_NO_FIT: by raw score
 * descending, then ascending id. */
int swdrv_rank_order(const swdrv_stats* stats, const int32_t* scores, const int32_t* lengths, const int64_t* ids, int n,
                     int32_t* out_order);

/* Statistics calibrated on shuffled subjects (an extension; DESIGN.md §15, include/cudasw4_amd_shuffle.h): what FASTA /
 * SSEARCH offer as -z 11 .. and PRSS does.  The fit above assumes that almost every subject is unrelated to the query; a
 * database dominated by one family breaks that, and a database of fewer than 100 usable scores allows no fit at all.  Here the
 * query is scored against a SAMPLE of the database whose subjects' residues are permuted on the device — length and
 * composition kept, homology destroyed — and the same fit is made on those scores:
 *   sample    M = min(n, max_subjects) subjects of the n the driver opened (whatever its shard or GPUs), ids
 *             ((2 j + 1) n) / (2 M) for j = 0 .. M - 1: ascending, distinct, length-stratified in a sorted database
 *   replicas  R = shuffles (1 .. 64), or with shuffles = 0 ceil(2000 / M) clamped to [1, 64]
 *   shuffle   subject `id` (within the opened database, without id_base) in replica r by the permutation of
 *             (seed, id, r, true length): include/cudasw4_amd_shuffle.h
 *   scores    exact (SW_KIND_I32), with the driver's matrix — or the PSSM — and gap scores, on the driver's first GPU
 *   table     the M R scores and true lengths through sw_score_histogram; the fit is swdrv_stats_from_histogram of it
 * The calibrated statistics of a scan are that fit's a, b1, sd, rounds and status with N TAKEN FROM THE SCAN'S TABLE: the
 * caller sets out->N (which these calls leave at M R) before swdrv_evalues.  The calibration depends on the query and the
 * database only, so it may run before the scan is collected.  max_subjects >= 1.  out, hist (64 x 256), sumlen (64),
 * subjects (M) and replicas (R) may each be NULL.  Where R replicas of the sample exceed max_temp_bytes they go through in
 * chunks; the sample stays on the device between calls with the same (database, max_subjects, shuffles, seed). */
int swdrv_calibrate_shuffled(swdrv* d, const char* query, int32_t qlen, int32_t max_subjects, int32_t shuffles, uint32_t seed,
                             swdrv_stats* out, uint32_t* hist, uint64_t* sumlen, int32_t* subjects, int32_t* replicas);
int swdrv_calibrate_shuffled_pssm(swdrv* d, const int8_t* pssm, int32_t qlen, int32_t max_subjects, int32_t shuffles, uint32_t seed,
                                  swdrv_stats* out, uint32_t* hist, uint64_t* sumlen, int32_t* subjects, int32_t* replicas);
/* Under SWDRV_RANK_EVALUE: the fit of the NEXT collected query — its status, a, b1 and sd, with N from that query's own
 * table — in place of the fit of the table (fit == NULL: back to that).  Set while nothing is in flight; the collect clears it. */
int swdrv_set_rank_fit(swdrv* d, const swdrv_stats* fit);
/* The rules alone (no GPU needed).  swdrv_shuffle_sample: out_ids (may be NULL) receives the M ids, returns M;
 * swdrv_shuffle_replicas: returns R; swdrv_shuffle_permutation: out[i] (L entries) = the position residue i of the shuffled
 * subject is taken from.  -1 on error. */
int swdrv_shuffle_sample(int64_t n, int64_t max_subjects, int64_t* out_ids);
int swdrv_shuffle_replicas(int64_t M, int32_t shuffles);
int swdrv_shuffle_permutation(int32_t L, uint32_t seed, int64_t id, int32_t replica, int32_t* out);

/* Low-complexity masking of the subjects (an extension; DESIGN.md §16, include/cudasw4_amd_mask.h: the rule): what MMseqs2
 * and DIAMOND do to their targets by default.  With masking on, every copy of subject chars that reaches a GPU — the resident
 * or cached part once behind its upload, every streamed batch once behind each of its copies — is masked in place on the
 * device before anything scans it; hit alignment, HSPs, PSSM building and the shuffled calibration see the same masked
 * subjects (a masked column is an X op and code 20 in the counts), while the reference letters the driver reports stay raw.
 * Call before the database is opened, like swdrv_set_shard: afterwards it fails.  window 4 .. 32; the entropies in bits,
 * trigger_bits <= extend_bits; on = 0: off, and nothing is computed. */
int swdrv_set_subject_masking(swdrv* d, int on, int32_t window, double trigger_bits, double extend_bits);
/* The most recent complete pass over the DB, summed over the GPUs — the resident part's upload plus the streamed batches of
 * the query collected last: positions covered by masked segments, subjects with a segment, true residues passed.  Zeros
 * before any pass. */
int swdrv_masking_counts(swdrv* d, uint64_t* positions, uint64_t* subjects, uint64_t* residues_seen);
/* The rule alone (no GPU needed).  swdrv_mask_threshold: max(1, ceil(1024 W (log2 W - bits))).  swdrv_mask_subject: out[0 ..
 * length) = the masked codes (out may be codes), returns the positions the segments cover, -1 for parameters out of range. */
int32_t swdrv_mask_threshold(int32_t window, double bits);
int64_t swdrv_mask_subject(const int8_t* codes, int32_t length, int32_t window, int32_t trigger_sum, int32_t extend_sum, int8_t* out);

/* ---- input helpers (no GPU needed): what `align` does to its inputs before the scan ---- */

/* ConvertAA_20 (convert.cuh:6-34): letters -> codes 0..20 */
void swdrv_encode(const char* letters, int8_t* codes, size_t n);
/* the pseudo-DB subject (dbdata.hpp:222-272): `length` codes from std::mt19937(seed) + uniform_int_distribution<>(0,19) */
void swdrv_pseudo_sequence(int32_t length, int seed, int8_t* codes);
/* 21 x 21 substitution matrix (types.hpp:29-270); matrix = 45 | 50 | 62 | 80; returns 0 or -1 */
int swdrv_matrix(int matrix, int8_t* out441);
/* 25 x 25 table (types.hpp:205-396), letter order ARNDCQEGHILKMFPSTWYVBJZX*, and its query encoder (anything else -> X) */
int swdrv_matrix25(int matrix, int8_t* out625);
void swdrv_encode25(const char* letters, int8_t* codes, size_t n);
/* FASTA / FASTQ (.gz) reader (kseqpp/kseqpp.hpp:54-118): open -> next* -> close.  next returns 1 while there is a
 * record; the header / sequence pointers stay valid until the following call. */
typedef struct swdrv_reader swdrv_reader;
int swdrv_reader_open(const char* path, swdrv_reader** out);
int swdrv_reader_next(swdrv_reader* r, const char** header, size_t* header_len, const char** sequence, size_t* sequence_len);
void swdrv_reader_close(swdrv_reader* r);

#ifdef __cplusplus
}
#endif
#endif
