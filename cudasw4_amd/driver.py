"""ctypes binding of include/cudasw4_amd_driver.h (libcudasw4_host.so): the C++ host driver.

Plumbing only — the library drives libcudasw4_amd.so; there is no CPU path.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CUDASW4_AMD_HOST_LIB: another build of the same C ABI (tests/host/fake_gpu: the real driver on a two-device fake runtime)
LIB_PATH = os.environ.get("CUDASW4_AMD_HOST_LIB") or os.path.join(_HERE, "lib", "libcudasw4_host.so")
MAKEDB = os.path.join(_HERE, "lib", "makedb")
ALIGN = os.path.join(_HERE, "lib", "align")

EXPORTS = ["swdrv_last_error", "swdrv_create", "swdrv_destroy", "swdrv_open_db", "swdrv_pseudo_db", "swdrv_upload",
           "swdrv_num_sequences", "swdrv_num_gpus", "swdrv_set_num_top", "swdrv_scan", "swdrv_reference_length",
           "swdrv_reference_header", "swdrv_encode", "swdrv_pseudo_sequence", "swdrv_matrix", "swdrv_reader_open",
           "swdrv_reader_next", "swdrv_reader_close", "swdrv_db_from_arrays", "swdrv_set_shard",
           "swdrv_record_kernel_events", "swdrv_take_kernel_events", "swdrv_shard_info", "swdrv_last_scores",
           "swdrv_batch_intervals", "swdrv_gpu_spans", "swdrv_plan_runs", "swdrv_shard_ranges", "swdrv_matrix25",
           "swdrv_encode25", "swdrv_last_rescored", "swdrv_scan_submit", "swdrv_scan_collect", "swdrv_in_flight",
           "swdrv_cached_chars", "swdrv_streamed_bytes", "swdrv_plan_residency", "swdrv_numa_node", "swdrv_device_of",
           "swdrv_bind_to_numa_node", "swdrv_device_numa_node", "swdrv_window_stats", "swdrv_service_launches",
           "swdrv_tail_overlaps", "swdrv_prefers_two_in_flight", "swdrv_pipeline_launches", "swdrv_handshake_active", "swdrv_preferred_in_flight",
           "swdrv_latency_scans", "swdrv_plan_runs_mode", "swdrv_align_hits", "swdrv_scan_pssm", "swdrv_scan_submit_pssm",
           "swdrv_align_hits_pssm", "swdrv_align_hsps", "swdrv_align_hsps_pssm", "swdrv_pssm_from_counts", "swdrv_build_pssm", "swdrv_write_pssm_ascii",
           "swdrv_build_pssm_purged", "swdrv_hit_msa", "swdrv_hit_msa_select", "swdrv_write_msa",
           "swdrv_set_statistics", "swdrv_last_statistics", "swdrv_stats_from_histogram", "swdrv_evalues", "swdrv_length_bin",
           "swdrv_set_ranking", "swdrv_last_ranking", "swdrv_zscore_for_evalue", "swdrv_rank_order",
           "swdrv_calibrate_shuffled", "swdrv_calibrate_shuffled_pssm", "swdrv_set_rank_fit", "swdrv_shuffle_sample",
           "swdrv_shuffle_replicas", "swdrv_shuffle_permutation",
           "swdrv_set_subject_masking", "swdrv_masking_counts", "swdrv_mask_threshold", "swdrv_mask_subject"]


class DriverError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libcudasw4_host.so is not built: run __graft_entry__.build()")
    # PyTorch wheels bundle their own HIP runtime.  If this library pulled in the system's libamdhip64 first, a later
    # `import torch` would bring a second runtime into the process and find no GPU: load torch's first when it is there.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32
    L.swdrv_last_error.restype = ctypes.c_char_p
    L.swdrv_create.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.c_int, sz, sz, sz, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.POINTER(vp)]
    L.swdrv_destroy.argtypes = [vp]
    L.swdrv_open_db.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
    L.swdrv_pseudo_db.argtypes = [vp, sz, i32]
    L.swdrv_upload.argtypes = [vp]
    L.swdrv_num_sequences.restype = ctypes.c_int64
    L.swdrv_num_sequences.argtypes = [vp]
    L.swdrv_num_gpus.argtypes = [vp]
    L.swdrv_set_num_top.argtypes = [vp, ctypes.c_int]
    L.swdrv_scan.argtypes = [vp, ctypes.c_char_p, i32, vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                             ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double),
                             ctypes.POINTER(ctypes.c_double)]
    L.swdrv_scan_submit.argtypes = [vp, ctypes.c_char_p, i32]
    L.swdrv_scan_collect.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.swdrv_in_flight.argtypes = [vp]
    L.swdrv_cached_chars.restype = ctypes.c_int64
    L.swdrv_cached_chars.argtypes = [vp, ctypes.c_int]
    L.swdrv_streamed_bytes.restype = ctypes.c_int64
    L.swdrv_streamed_bytes.argtypes = [vp]
    L.swdrv_plan_residency.argtypes = [vp, sz, i32, sz, sz, sz, sz, sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), vp, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_int64)]
    L.swdrv_reference_length.restype = i32
    L.swdrv_reference_length.argtypes = [vp, ctypes.c_int64]
    L.swdrv_reference_header.argtypes = [vp, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int]
    L.swdrv_encode.argtypes = [ctypes.c_char_p, vp, sz]
    L.swdrv_pseudo_sequence.argtypes = [i32, ctypes.c_int, vp]
    L.swdrv_matrix.argtypes = [ctypes.c_int, vp]
    L.swdrv_reader_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.swdrv_reader_next.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz),
                                    ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz)]
    L.swdrv_reader_close.argtypes = [vp]
    i64 = ctypes.c_int64
    L.swdrv_db_from_arrays.argtypes = [vp, vp, sz, vp, vp, sz]
    L.swdrv_set_shard.argtypes = [vp, ctypes.c_int, ctypes.c_int, i64]
    L.swdrv_record_kernel_events.argtypes = [vp, ctypes.c_int]
    L.swdrv_take_kernel_events.argtypes = [vp, vp, ctypes.c_int]
    L.swdrv_shard_info.argtypes = [vp, ctypes.c_int, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64),
                                   ctypes.POINTER(ctypes.c_int)]
    L.swdrv_last_scores.argtypes = [vp, ctypes.c_int, vp, vp]
    L.swdrv_batch_intervals.argtypes = [vp, vp, ctypes.c_int]
    L.swdrv_gpu_spans.argtypes = [vp, vp, ctypes.c_int]
    L.swdrv_plan_runs.argtypes = [vp, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int]
    L.swdrv_plan_runs_mode.argtypes = [vp, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int]
    L.swdrv_shard_ranges.argtypes = [vp, vp, sz, ctypes.c_int, vp]
    L.swdrv_matrix25.argtypes = [ctypes.c_int, vp]
    L.swdrv_last_rescored.argtypes = [vp]
    L.swdrv_numa_node.argtypes = [vp, ctypes.c_int]
    L.swdrv_service_launches.restype = ctypes.c_int64
    L.swdrv_service_launches.argtypes = [vp]
    L.swdrv_latency_scans.restype = ctypes.c_int64
    L.swdrv_latency_scans.argtypes = [vp]
    L.swdrv_pipeline_launches.restype = ctypes.c_int64
    L.swdrv_pipeline_launches.argtypes = [vp]
    L.swdrv_preferred_in_flight.restype = ctypes.c_int
    L.swdrv_preferred_in_flight.argtypes = [vp, ctypes.c_int32]
    L.swdrv_handshake_active.restype = ctypes.c_int
    L.swdrv_handshake_active.argtypes = [vp]
    L.swdrv_tail_overlaps.restype = ctypes.c_int64
    L.swdrv_tail_overlaps.argtypes = [vp]
    L.swdrv_prefers_two_in_flight.argtypes = [vp, ctypes.c_int32]
    L.swdrv_window_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.swdrv_device_of.argtypes = [vp, ctypes.c_int]
    L.swdrv_bind_to_numa_node.argtypes = [ctypes.c_int]
    L.swdrv_device_numa_node.argtypes = [ctypes.c_int]
    L.swdrv_encode25.argtypes = [ctypes.c_char_p, vp, sz]
    return L


lib = _load()


def _align_fn():
    """swdrv_align_hits, bound on first use: _load() also serves builds of this C ABI without it (tests/host/fake_gpu)"""
    f = lib.swdrv_align_hits
    if f.argtypes is None:
        vp = ctypes.c_void_p
        f.argtypes = [vp, ctypes.c_char_p, ctypes.c_int32, vp, vp, ctypes.c_int, vp, vp, ctypes.c_int64]
    return f


def _align_pssm_fn():
    """swdrv_align_hits_pssm, bound on first use (like swdrv_align_hits: not in every build of this C ABI)"""
    f = lib.swdrv_align_hits_pssm
    if f.argtypes is None:
        vp = ctypes.c_void_p
        f.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_char_p, vp, vp, ctypes.c_int, vp, vp, ctypes.c_int64]
    return f


def _align_hsps_fns():
    """swdrv_align_hsps / swdrv_align_hsps_pssm, bound on first use (like swdrv_align_hits: not in every build of this C ABI)"""
    f, g = lib.swdrv_align_hsps, lib.swdrv_align_hsps_pssm
    if f.argtypes is None:
        vp, i = ctypes.c_void_p, ctypes.c_int
        f.argtypes = [vp, ctypes.c_char_p, ctypes.c_int32, vp, vp, i, i, i, vp, vp, ctypes.c_int64]
        g.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_char_p, vp, vp, i, i, i, vp, vp, ctypes.c_int64]
    return f, g


def _hsp_lists(res, cigar, n, max_hsps):
    """the n * max_hsps slots of swdrv_align_hsps as one list per hit: slot 0 whatever it is, then the slots that are OK.
    -> [[(record, CIGAR string)]]"""
    from . import capi
    out = []
    for i in range(n):
        hit = []
        for k in range(max_hsps):
            r = res[i * max_hsps + k]
            if k and int(r["status"]) != capi.ALIGN_OK:
                break
            hit.append((r, capi.cigar_string(cigar[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])])))
        out.append(hit)
    return out


def _check_hsps(max_hsps, min_score):
    from . import capi
    if not 1 <= int(max_hsps) <= capi.MAX_HSPS:
        raise ValueError("max_hsps must lie in [1, %d]" % capi.MAX_HSPS)
    if max_hsps > 1 and min_score is None:
        raise ValueError("max_hsps > 1 needs min_score: the least score of a further alignment")
    if min_score is not None and int(min_score) < 1:
        raise ValueError("min_score must be at least 1")


def _pssm_fns():
    """swdrv_scan_pssm / swdrv_scan_submit_pssm, bound on first use (like swdrv_align_hits: not in every build of this C ABI)"""
    scan, submit = lib.swdrv_scan_pssm, lib.swdrv_scan_submit_pssm
    if scan.argtypes is None:
        vp = ctypes.c_void_p
        scan.argtypes = [vp, vp, ctypes.c_int32, vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                         ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        submit.argtypes = [vp, vp, ctypes.c_int32]
    return scan, submit


class _PssmInfo(ctypes.Structure):
    _fields_ = [("used", ctypes.c_int32), ("below_score", ctypes.c_int32), ("no_trace", ctypes.c_int32),
                ("copies", ctypes.c_int32), ("lambda_", ctypes.c_double), ("included", ctypes.c_void_p)]


def _build_fns():
    """swdrv_pssm_from_counts / swdrv_build_pssm / swdrv_write_pssm_ascii, bound on first use (like swdrv_align_hits: not in
    every build of this C ABI)"""
    fc, bp, wr = lib.swdrv_pssm_from_counts, lib.swdrv_build_pssm, lib.swdrv_write_pssm_ascii
    if fc.argtypes is None:
        vp = ctypes.c_void_p
        fc.argtypes = [ctypes.c_int, vp, ctypes.c_int32, vp, vp, ctypes.c_double, vp, vp, ctypes.POINTER(ctypes.c_double)]
        bp.argtypes = [vp, ctypes.c_char_p, ctypes.c_int32, vp, vp, vp, ctypes.c_int, ctypes.c_int32, ctypes.c_double, vp,
                       ctypes.POINTER(_PssmInfo)]
        wr.argtypes = [ctypes.c_char_p, vp, ctypes.c_int32, ctypes.c_char_p]
    return fc, bp, wr


def _msa_fns():
    """swdrv_build_pssm_purged / swdrv_hit_msa / swdrv_write_msa, bound on first use (like swdrv_align_hits: not in every build
    of this C ABI)"""
    bp, hm, wr = lib.swdrv_build_pssm_purged, lib.swdrv_hit_msa, lib.swdrv_write_msa
    if bp.argtypes is None:
        vp, i, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
        bp.argtypes = [vp, cp, ctypes.c_int32, vp, vp, vp, i, ctypes.c_int32, ctypes.c_double, i, vp, ctypes.POINTER(_PssmInfo),
                       ctypes.POINTER(ctypes.c_int32)]
        hm.argtypes = [vp, cp, ctypes.c_int32, vp, vp, vp, i, i, cp, cp, i, vp, vp, ctypes.c_int64, vp, vp, vp,
                       ctypes.POINTER(ctypes.c_int32)]
        wr.argtypes = [cp, i, cp, cp, i, ctypes.POINTER(cp), ctypes.POINTER(cp), vp, vp, vp]
    return bp, hm, wr


def _msa_select_fn():
    """swdrv_hit_msa_select, bound on first use"""
    f = lib.swdrv_hit_msa_select
    if f.argtypes is None:
        vp, i, cp, i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int32
        f.argtypes = [vp, cp, i32, vp, vp, vp, i, i, i, i, vp, i, cp, cp, i, vp, vp, ctypes.c_int64, vp, vp, vp, vp, vp]
    return f


MSA_FORMATS = {"a3m": 0, "fasta": 1}


def write_msa(path, fmt, master_letters, query_header, headers, subject_letters, results, cigar, keep=None):
    """swdrv_write_msa: the A3M (fmt 'a3m') or FASTA ('fasta') file `align --outMsa` writes, from alignments the caller has:
    results (capi.align_result_dtype() records whose cigar_offset index the uint32 words `cigar`), the hits' headers and RAW
    letters, keep (one byte per hit, None: every hit).  No GPU needed."""
    from . import capi
    n = len(headers)
    res = np.ascontiguousarray(results, dtype=capi.align_result_dtype())
    cig = np.ascontiguousarray(cigar, dtype=np.uint32)
    k = np.ascontiguousarray(keep, dtype=np.uint8) if keep is not None else None
    enc = lambda t: t if isinstance(t, bytes) else t.encode()
    hs = (ctypes.c_char_p * max(n, 1))(*[enc(h) for h in headers])
    ss = (ctypes.c_char_p * max(n, 1))(*[enc(x) for x in subject_letters])
    _check(_msa_fns()[2](enc(path), MSA_FORMATS[fmt], enc(master_letters), enc(query_header), n, hs, ss, res.ctypes.data,
                         cig.ctypes.data, k.ctypes.data if k is not None else None))


STATS_OK, STATS_NO_FIT = 0, 1
STATS_LBINS, STATS_SBINS = 64, 256


class _Stats(ctypes.Structure):
    _fields_ = [("a", ctypes.c_double), ("b1", ctypes.c_double), ("sd", ctypes.c_double), ("n_included", ctypes.c_int64),
                ("N", ctypes.c_int64), ("rounds", ctypes.c_int32), ("status", ctypes.c_int32)]


def _stats_fns():
    """swdrv_set_statistics / swdrv_last_statistics / swdrv_stats_from_histogram / swdrv_evalues / swdrv_length_bin, bound on
    first use (like swdrv_align_hits: not in every build of this C ABI)"""
    on, last, fit, ev, lb = (lib.swdrv_set_statistics, lib.swdrv_last_statistics, lib.swdrv_stats_from_histogram,
                             lib.swdrv_evalues, lib.swdrv_length_bin)
    if on.argtypes is None:
        vp = ctypes.c_void_p
        on.argtypes = [vp, ctypes.c_int]
        last.argtypes = [vp, ctypes.POINTER(_Stats), vp, vp]
        fit.argtypes = [vp, vp, ctypes.POINTER(_Stats)]
        ev.argtypes = [ctypes.POINTER(_Stats), vp, vp, ctypes.c_int, vp, vp]
        lb.argtypes = [ctypes.c_int32]
    return on, last, fit, ev, lb


def _stats_dict(s):
    return {"a": s.a, "b1": s.b1, "sd": s.sd, "n_included": int(s.n_included), "N": int(s.N), "rounds": int(s.rounds),
            "status": int(s.status)}


def _stats_struct(stats):
    return _Stats(float(stats["a"]), float(stats["b1"]), float(stats["sd"]), int(stats["n_included"]), int(stats["N"]),
                  int(stats["rounds"]), int(stats["status"]))


SHUFFLE_DEFAULT_SUBJECTS, SHUFFLE_MAX_REPLICAS = 10000, 64


def _shuffle_fns():
    """swdrv_calibrate_shuffled / swdrv_calibrate_shuffled_pssm / swdrv_set_rank_fit / swdrv_shuffle_sample /
    swdrv_shuffle_replicas / swdrv_shuffle_permutation, bound on first use (not in every build of this C ABI)"""
    cal, calp, setfit, sample, reps, perm = (lib.swdrv_calibrate_shuffled, lib.swdrv_calibrate_shuffled_pssm, lib.swdrv_set_rank_fit,
                                            lib.swdrv_shuffle_sample, lib.swdrv_shuffle_replicas, lib.swdrv_shuffle_permutation)
    if cal.argtypes is None:
        vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
        cal.argtypes = [vp, ctypes.c_char_p, i32, i32, i32, u32, ctypes.POINTER(_Stats), vp, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        calp.argtypes = [vp, vp, i32, i32, i32, u32, ctypes.POINTER(_Stats), vp, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        setfit.argtypes = [vp, ctypes.POINTER(_Stats)]
        sample.argtypes = [i64, i64, vp]
        reps.argtypes = [i64, i32]
        perm.argtypes = [i32, u32, i64, i32, vp]
    return cal, calp, setfit, sample, reps, perm


def _mask_fns():
    """swdrv_set_subject_masking / swdrv_masking_counts / swdrv_mask_threshold / swdrv_mask_subject, bound on first use (not in
    every build of this C ABI)"""
    seton, counts, thr, one = (lib.swdrv_set_subject_masking, lib.swdrv_masking_counts, lib.swdrv_mask_threshold,
                               lib.swdrv_mask_subject)
    if seton.argtypes is None:
        vp, i32, u64p = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)
        seton.argtypes = [vp, ctypes.c_int, i32, ctypes.c_double, ctypes.c_double]
        counts.argtypes = [vp, u64p, u64p, u64p]
        thr.argtypes = [i32, ctypes.c_double]
        thr.restype = i32
        one.argtypes = [vp, i32, i32, i32, i32, vp]
        one.restype = ctypes.c_int64
    return seton, counts, thr, one


RANK_SCORE, RANK_EVALUE = 0, 1


def _rank_fns():
    """swdrv_set_ranking / swdrv_last_ranking / swdrv_zscore_for_evalue / swdrv_rank_order, bound on first use (like
    swdrv_align_hits: not in every build of this C ABI)"""
    setr, last, zfor, order = lib.swdrv_set_ranking, lib.swdrv_last_ranking, lib.swdrv_zscore_for_evalue, lib.swdrv_rank_order
    if setr.argtypes is None:
        vp = ctypes.c_void_p
        setr.argtypes = [vp, ctypes.c_int, ctypes.c_double]
        last.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
        zfor.argtypes = [ctypes.c_int64, ctypes.c_double]
        zfor.restype = ctypes.c_double
        order.argtypes = [ctypes.POINTER(_Stats), vp, vp, vp, ctypes.c_int, vp]
    return setr, last, zfor, order


def zscore_for_evalue(N, evalue):
    """swdrv_zscore_for_evalue (no GPU needed): the Z-score at which the E-value of a DB of N scored subjects equals `evalue`
    (-inf for evalue >= N)."""
    return float(_rank_fns()[2](int(N), float(evalue)))


def rank_order(stats, scores, lengths, ids):
    """swdrv_rank_order (no GPU needed): the indices of the hits by Z-score under `stats` (a fit dict) descending, equal
    Z-scores by ascending id -> int32 array."""
    sc = np.ascontiguousarray(scores, dtype=np.int32)
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    ii = np.ascontiguousarray(ids, dtype=np.int64)
    if not len(sc) == len(ln) == len(ii):
        raise ValueError("scores, lengths and ids must have one length")
    out = np.zeros(len(sc), dtype=np.int32)
    c = _stats_struct(stats)
    _check(_rank_fns()[3](ctypes.byref(c), sc.ctypes.data, ln.ctypes.data, ii.ctypes.data, len(sc), out.ctypes.data))
    return out


def pssm_from_counts(master_codes, counts, wcounts, matrix=62, pseudocount=10.0, with_raw=False):
    """swdrv_pssm_from_counts (no GPU needed): residue counts (qlen x 20, uint32) and weighted counts (qlen x 20, uint64) of a
    master sequence's aligned hits -> ((qlen, 21) int8 PSSM, lambda), or (PSSM, lambda, raw (qlen, 20) float64 scores)."""
    m = np.ascontiguousarray(master_codes, dtype=np.int8)
    qlen = len(m)
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    w = np.ascontiguousarray(wcounts, dtype=np.uint64)
    if qlen < 1 or c.size != qlen * 20 or w.size != qlen * 20:
        raise ValueError("counts and wcounts must be (qlen, 20) arrays for a master of qlen >= 1 codes")
    out = np.zeros((qlen, 21), dtype=np.int8)
    raw = np.zeros((qlen, 20), dtype=np.float64)
    lam = ctypes.c_double()
    _check(_build_fns()[0](int(matrix), m.ctypes.data, qlen, c.ctypes.data, w.ctypes.data, float(pseudocount), out.ctypes.data,
                           raw.ctypes.data, ctypes.byref(lam)))
    return (out, lam.value, raw) if with_raw else (out, lam.value)


def write_pssm_ascii(path, pssm, consensus):
    """The C++ writer of NCBI ASCII PSSMs (what `align --outPssm` writes; the layout of pssm.write_ascii)."""
    from . import pssm as _pssm
    m = _pssm.as_pssm(pssm)
    if isinstance(consensus, str):
        consensus = consensus.encode()
    _check(_build_fns()[2](str(path).encode(), m.ctypes.data, m.shape[0], consensus))


# ---- input helpers of the host library (what `align` does to its inputs; no GPU needed) ----

def encode(letters) -> np.ndarray:
    """ConvertAA_20: residue letters -> int8 codes 0..20."""
    if isinstance(letters, str):
        letters = letters.encode()
    out = np.empty(len(letters), dtype=np.int8)
    lib.swdrv_encode(letters, out.ctypes.data, len(letters))
    return out


def pseudo_sequence(length, seed=42) -> np.ndarray:
    """The pseudo-DB subject (one mt19937(seed) sequence), as codes."""
    out = np.empty(length, dtype=np.int8)
    lib.swdrv_pseudo_sequence(length, seed, out.ctypes.data)
    return out


def matrix(which=62) -> np.ndarray:
    out = np.empty(441, dtype=np.int8)
    if lib.swdrv_matrix(which, out.ctypes.data) != 0:
        raise ValueError("unknown matrix %r" % which)
    return out


def matrix25(which=62) -> np.ndarray:
    """The full 25 x 25 table, letter order ARNDCQEGHILKMFPSTWYVBJZX*."""
    out = np.empty(625, dtype=np.int8)
    if lib.swdrv_matrix25(which, out.ctypes.data) != 0:
        raise ValueError("unknown matrix %r" % which)
    return out


def encode25(letters) -> np.ndarray:
    """Query letters -> codes 0..24 for the 25-letter tables (anything else -> X)."""
    if isinstance(letters, str):
        letters = letters.encode()
    out = np.empty(len(letters), dtype=np.int8)
    lib.swdrv_encode25(letters, out.ctypes.data, len(letters))
    return out


def read_sequences(path):
    """FASTA / FASTQ (.gz) -> (headers, sequences as bytes), parsed like the reference's kseq reader."""
    h = ctypes.c_void_p()
    _check(lib.swdrv_reader_open(path.encode(), ctypes.byref(h)))
    headers, seqs = [], []
    hp, sp = ctypes.c_char_p(), ctypes.c_char_p()
    hl, sl = ctypes.c_size_t(), ctypes.c_size_t()
    try:
        while lib.swdrv_reader_next(h, ctypes.byref(hp), ctypes.byref(hl), ctypes.byref(sp), ctypes.byref(sl)):
            headers.append(ctypes.string_at(hp, hl.value).decode())
            seqs.append(ctypes.string_at(sp, sl.value))
    finally:
        lib.swdrv_reader_close(h)
    return headers, seqs


def device_numa_node(device):
    """NUMA node of HIP device `device` (its PCI function's numa_node attribute; -1: unknown)."""
    return int(lib.swdrv_device_numa_node(int(device)))


def bind_to_numa_node(node):
    """Run the calling thread (and the threads it starts) on the CPUs of `node` that the process may use -> True if bound."""
    return lib.swdrv_bind_to_numa_node(int(node)) == 0


def _check(rc):
    if rc != 0:
        raise DriverError(lib.swdrv_last_error().decode())


def plan_runs(sorted_lengths, kind_single, kind_many_small, kind_many_large, latency_mode=False):
    """The launch planner of the C++ driver (plan_launch_runs; no GPU needed): runs of a length-sorted subject list,
    largest partition first -> list of dicts (kind, part_id, begin, end, maxlen).  latency_mode: the plan of small shards
    of real DBs (partition 34 keeps a launch of its own whatever its size)."""
    l = np.ascontiguousarray(sorted_lengths, dtype=np.int32)
    out = np.zeros(36 * 5, dtype=np.int64)
    n = lib.swdrv_plan_runs_mode(l.ctypes.data, len(l), kind_single, kind_many_small, kind_many_large, int(bool(latency_mode)),
                                 out.ctypes.data, 36)
    if n < 0:
        raise DriverError(lib.swdrv_last_error().decode())
    return [{"kind": int(out[5 * i]), "part_id": int(out[5 * i + 1]), "begin": int(out[5 * i + 2]),
             "end": int(out[5 * i + 3]), "maxlen": int(out[5 * i + 4])} for i in range(n)]


def shard_ranges(offsets, sorted_lengths, world):
    """partitionDBAmongstGpus as the C++ driver does it (shard_database; no GPU needed):
    ranges[rank][partition] = (begin, end)."""
    l = np.ascontiguousarray(sorted_lengths, dtype=np.int32)
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.zeros(world * 36 * 2, dtype=np.int64)
    _check(lib.swdrv_shard_ranges(l.ctypes.data, o.ctypes.data, len(l), world, out.ctypes.data))
    out = out.reshape(world, 36, 2)
    return [[(int(b), int(e)) for b, e in out[r]] for r in range(world)]


def plan_residency(local_offsets, max_len, max_gpu_mem=0, max_batch_bytes=0, max_batch_sequences=0, max_temp_bytes=0,
                   free_mem=288 << 30, allow_cache=True):
    """The C++ driver's residency decision for one GPU's shard (plan_residency; no GPU needed) -> dict: cache_begin (the
    subjects from there on stay in device memory), cache_bytes, batch_bytes, batches = [(begin, end), ...] of the rest,
    temp_per_stream (cap of each of the 4 stripe-border scratch buffers)."""
    o = np.ascontiguousarray(local_offsets, dtype=np.uint64)
    n = len(o) - 1
    cap = max(n, 1)
    out = np.zeros(2 * cap, dtype=np.int64)
    cb, cby, bb, tps = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    nb = lib.swdrv_plan_residency(o.ctypes.data, n, int(max_len), max_gpu_mem, max_batch_bytes, max_batch_sequences,
                                  max_temp_bytes, free_mem, int(allow_cache), ctypes.byref(cb), ctypes.byref(cby),
                                  ctypes.byref(bb), out.ctypes.data, cap, ctypes.byref(tps))
    if nb < 0:
        raise DriverError(lib.swdrv_last_error().decode())
    return {"cache_begin": cb.value, "cache_bytes": cby.value, "batch_bytes": bb.value, "temp_per_stream": tps.value,
            "batches": [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(nb)]}


class Driver:
    """SearchDriver (C++) == the reference's CudaSW4 as `align` uses it."""

    def __init__(self, devices=None, num_top=10, matrix=62, kinds=(0, 0, 3, 3), max_gpu_mem=0, max_batch_bytes=0,
                 max_batch_sequences=0, max_temp_bytes=0, gop=-11, gex=-1, verbose=False):
        h = ctypes.c_void_p()
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            n = len(devices)
        else:
            arr, n = None, 0
        _check(lib.swdrv_create(arr, n, num_top, matrix, kinds[0], kinds[1], kinds[2], kinds[3], max_gpu_mem,
                                max_batch_bytes, max_batch_sequences, max_temp_bytes, gop, gex, int(verbose),
                                ctypes.byref(h)))
        self.handle = h
        self.num_top = num_top
        self.statistics = False
        self.statistics_mode = "scan"
        self._shuffle = (None, SHUFFLE_DEFAULT_SUBJECTS, 1)   # shuffles, max_subjects, seed of mode "shuffled"
        self._calibrations = []                                # of the queries in flight, oldest first (mode "shuffled")
        self.ranking = "score"
        self.max_evalue = None

    def set_ranking(self, by="score", max_evalue=None):
        """Ranking of the result lists.  "evalue": statistics on, and every scan from now on returns the num_top
        subjects of smallest E-value (largest Z-score; ties: ascending id) — "scores" and "ids" stay raw scores and global ids,
        "zscores" and "evalues" stay aligned with them, so align_hits, build_pssm and iterate take the list as it is.  With
        max_evalue the dicts also carry "n_significant": the subjects of the whole DB with E <= max_evalue (-1 where the scan
        allows no fit; the list is then the raw-score list).  One query in flight.  "score": the raw-score lists again (the
        statistics stay as they are).  Not with queries in flight."""
        if by not in ("score", "evalue"):
            raise ValueError("ranking must be 'score' or 'evalue', not %r" % (by,))
        if by == "score" and max_evalue is not None:
            raise ValueError("max_evalue belongs to ranking by 'evalue'")
        x = float(max_evalue) if max_evalue is not None else 0.0
        if max_evalue is not None and not x > 0:
            raise ValueError("max_evalue must be positive")
        _check(_rank_fns()[0](self.handle, RANK_EVALUE if by == "evalue" else RANK_SCORE, x))
        self.ranking = by
        self.max_evalue = x if max_evalue is not None else None
        if by == "evalue":
            self.statistics = True

    def last_ranking(self):
        """(count, z_min) of the query collected last (swdrv_last_ranking): the subjects at or under the E-value threshold over
        all GPUs (-1: no threshold, no fit, or ranked by score) and the Z-score the threshold stands for."""
        c, z = ctypes.c_int64(), ctypes.c_double()
        _check(_rank_fns()[1](self.handle, ctypes.byref(c), ctypes.byref(z)))
        return int(c.value), float(z.value)

    def set_statistics(self, on=True, mode="scan", shuffles=None, max_subjects=SHUFFLE_DEFAULT_SUBJECTS, seed=1):
        """Search statistics: from now on every scan also histograms its scores on the GPU, and the dicts of
        scan / scan_pssm / collect carry "zscores" and "evalues" (float64, aligned with "scores") and "stats" (the fit: a, b1,
        sd, n_included, N, rounds, status, mode; plus the table: hist, sumlen).  Not with queries in flight.
        mode "shuffled" (DESIGN.md §15): the fit is made on the scores of the query against a sample of at most max_subjects
        subjects of the DB, each permuted `shuffles` times (None: ceil(2000 / sample) clamped to [1, 64]) under `seed` — every
        query is calibrated (calibrate()) when it is submitted; "stats" then holds that fit with N from the scan's table, the
        calibration's hist and sumlen, and "subjects" / "replicas"; under set_ranking("evalue") the list is ranked by it."""
        if mode not in ("scan", "shuffled"):
            raise ValueError("statistics mode must be 'scan' or 'shuffled', not %r" % (mode,))
        if shuffles is not None and not 1 <= int(shuffles) <= SHUFFLE_MAX_REPLICAS:
            raise ValueError("shuffles must lie in [1, %d]" % SHUFFLE_MAX_REPLICAS)
        if int(max_subjects) < 1:
            raise ValueError("max_subjects must be at least 1")
        if not on and self.ranking == "evalue":
            raise ValueError("ranking by E-value needs the statistics: set_ranking('score') first")
        if self._calibrations:
            raise DriverError("set_statistics with queries in flight: collect() them first")
        _check(_stats_fns()[0](self.handle, int(bool(on))))
        self.statistics = bool(on)
        self.statistics_mode = mode if on else "scan"
        self._shuffle = (None if shuffles is None else int(shuffles), int(max_subjects), int(seed) & 0xFFFFFFFF)

    def calibrate(self, query_or_pssm, shuffles=None, max_subjects=None, seed=None):
        """The shuffled calibration of one query (swdrv_calibrate_shuffled): residue letters (str / bytes) or a
        PSSM ((qlen, 21) int8).  -> the fit dict (a, b1, sd, n_included, N = subjects x replicas, rounds, status) with the
        calibration's table (hist, sumlen), "subjects" and "replicas".  Depends on the query and the DB only: it may run
        while a scan is in flight.  The parameters default to those of set_statistics."""
        sh, ms, sd = self._shuffle
        sh = sh if shuffles is None else int(shuffles)
        ms = ms if max_subjects is None else int(max_subjects)
        sd = sd if seed is None else int(seed) & 0xFFFFFFFF
        s, m, r = _Stats(), ctypes.c_int32(), ctypes.c_int32()
        hist = np.zeros((STATS_LBINS, STATS_SBINS), dtype=np.uint32)
        sumlen = np.zeros(STATS_LBINS, dtype=np.uint64)
        tail = (ms, sh or 0, sd, ctypes.byref(s), hist.ctypes.data, sumlen.ctypes.data, ctypes.byref(m), ctypes.byref(r))
        if isinstance(query_or_pssm, (str, bytes)):
            q = query_or_pssm.encode() if isinstance(query_or_pssm, str) else query_or_pssm
            _check(_shuffle_fns()[0](self.handle, q, len(q), *tail))
        else:
            from . import pssm as _pssm
            p = _pssm.as_pssm(query_or_pssm)
            _check(_shuffle_fns()[1](self.handle, p.ctypes.data, p.shape[0], *tail))
        out = _stats_dict(s)
        out.update(hist=hist, sumlen=sumlen, subjects=int(m.value), replicas=int(r.value), mode="shuffled")
        return out

    def _calibrate_for_submit(self, query_or_pssm):
        """mode "shuffled": the calibration of a query about to be submitted, queued for its collect; under E-value ranking it
        is also the fit the driver ranks that query by"""
        if not (self.statistics and self.statistics_mode == "shuffled"):
            return
        cal = self.calibrate(query_or_pssm)
        if self.ranking == "evalue":
            c = _stats_struct(cal)
            _check(_shuffle_fns()[2](self.handle, ctypes.byref(c)))
        self._calibrations.append(cal)

    def _checked(self, rc, submitted):
        """_check for the calls that submit or collect a query: a failed call takes its query's calibration with it
        (submitted: the newest one; else the oldest)"""
        if rc != 0 and self._calibrations:
            self._calibrations.pop(-1 if submitted else 0)
        _check(rc)

    def last_statistics(self):
        """Fit and table of the query collected last (swdrv_last_statistics) -> the "stats" dict of its result."""
        s = _Stats()
        hist = np.zeros((STATS_LBINS, STATS_SBINS), dtype=np.uint32)
        sumlen = np.zeros(STATS_LBINS, dtype=np.uint64)
        _check(_stats_fns()[1](self.handle, ctypes.byref(s), hist.ctypes.data, sumlen.ctypes.data))
        out = _stats_dict(s)
        out["hist"], out["sumlen"] = hist, sumlen
        return out

    def _with_statistics(self, result):
        if not self.statistics:
            return result
        st = self.last_statistics()
        st["mode"] = "scan"
        if self.statistics_mode == "shuffled":   # the calibration's fit and table, N from the scan's own table
            cal = self._calibrations.pop(0)
            cal["N"] = st["N"]
            st = cal
        ids = result["ids"]
        lengths = np.array([self.reference_length(int(i)) for i in ids], dtype=np.int32)
        z = np.zeros(len(ids), dtype=np.float64)
        e = np.zeros(len(ids), dtype=np.float64)
        sc = np.ascontiguousarray(result["scores"], dtype=np.int32)
        c = _stats_struct(st)
        _check(_stats_fns()[3](ctypes.byref(c), sc.ctypes.data, lengths.ctypes.data, len(ids), z.ctypes.data, e.ctypes.data))
        result["zscores"], result["evalues"], result["stats"] = z, e, st
        if self.ranking == "evalue" and self.max_evalue is not None:
            result["n_significant"] = self.last_ranking()[0]
        return result

    def close(self):
        if self.handle:
            lib.swdrv_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def open_db(self, prefix, prefetch=False):
        _check(lib.swdrv_open_db(self.handle, prefix.encode(), int(prefetch)))

    def pseudo_db(self, num, length):
        _check(lib.swdrv_pseudo_db(self.handle, num, length))

    def db_from_arrays(self, chars, offsets, lengths):
        """DB from numpy arrays in dbdata layout (sorted by ascending length); the driver copies them."""
        c = np.ascontiguousarray(chars, dtype=np.int8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        l = np.ascontiguousarray(lengths, dtype=np.int32)
        _check(lib.swdrv_db_from_arrays(self.handle, c.ctypes.data, len(c), o.ctypes.data, l.ctypes.data, len(l)))

    def set_shard(self, rank, world, id_base=0):
        """One process per GPU: take shard `rank` of `world` (call before loading the DB)."""
        _check(lib.swdrv_set_shard(self.handle, rank, world, id_base))

    def set_subject_masking(self, on=True, window=12, trigger_bits=1.9, extend_bits=2.2):
        """Low-complexity masking of the subjects on the GPU (cudasw4_amd.mask states the rule): every copy of
        subject chars that reaches a GPU is masked before it is scanned, and align_hits / align_hsps / build_pssm / calibrate
        see the same masked subjects.  Call before loading the DB, like set_shard: afterwards it raises."""
        _check(_mask_fns()[0](self.handle, int(bool(on)), int(window), float(trigger_bits), float(extend_bits)))

    def masking_counts(self):
        """The most recent complete pass over the DB, summed over the GPUs (swdrv_masking_counts) -> dict(positions, subjects,
        residues_seen): the resident part's upload plus the streamed batches of the query collected last."""
        p, sj, r = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(_mask_fns()[1](self.handle, ctypes.byref(p), ctypes.byref(sj), ctypes.byref(r)))
        return {"positions": int(p.value), "subjects": int(sj.value), "residues_seen": int(r.value)}

    def upload(self):
        _check(lib.swdrv_upload(self.handle))

    def record_kernel_events(self, on=True):
        _check(lib.swdrv_record_kernel_events(self.handle, int(on)))

    def take_kernel_events(self):
        """-> list of dicts (gpu, kind, part_id, qlen, subjects, cells, chars, ms, t0_ms, t1_ms, eff_kind, rows,
        nstripes, lanes, rescore), HIP-event timed launches; t0/t1: begin and end on the device clock since recording was
        switched on; the last four name the kernel instantiation."""
        cap = 16384
        while True:
            buf = np.zeros(cap * 15, dtype=np.float64)
            n = lib.swdrv_take_kernel_events(self.handle, buf.ctypes.data, cap)
            if n < 0:
                raise DriverError(lib.swdrv_last_error().decode())
            if n <= cap:
                break
            raise DriverError("more than %d kernel events between two takes" % cap)
        keys = ("gpu", "kind", "part_id", "qlen", "subjects", "cells", "chars", "ms", "t0_ms", "t1_ms", "eff_kind", "rows",
                "nstripes", "lanes", "rescore")
        floats = ("cells", "chars", "ms", "t0_ms", "t1_ms")
        return [dict(zip(keys, (float(v) if k in floats else int(v) for k, v in zip(keys, buf[15 * i:15 * i + 15]))))
                for i in range(n)]

    def shard_info(self, gpu=0):
        i64 = ctypes.c_int64
        n, r, c, res = i64(), i64(), i64(), ctypes.c_int()
        _check(lib.swdrv_shard_info(self.handle, gpu, ctypes.byref(n), ctypes.byref(r), ctypes.byref(c), ctypes.byref(res)))
        return {"subjects": n.value, "residues": r.value, "chars": c.value, "resident": bool(res.value),
                "cached_chars": int(lib.swdrv_cached_chars(self.handle, gpu))}

    def window_stats(self):
        """(side launches that scanned long subjects as overlapping windows, windows scanned) since the driver was created."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        _check(lib.swdrv_window_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def service_launches(self):
        """Re-score service launches since the driver was created."""
        return int(lib.swdrv_service_launches(self.handle))

    def prefers_two_in_flight(self, query_length=0):
        """True when the tail hand-over applies (small resident shards, or a query of query_length residues that is scanned
        in a few milliseconds): use scan_many / submit + collect."""
        return bool(lib.swdrv_prefers_two_in_flight(self.handle, int(query_length)))

    def latency_scans(self):
        """Scans planned in latency mode (swdrv_latency_scans)."""
        return int(lib.swdrv_latency_scans(self.handle))

    def handshake_active(self):
        """True when the start handshake passed its probe (swdrv_handshake_active)."""
        return int(lib.swdrv_handshake_active(self.handle)) == 1

    def pipeline_launches(self):
        """Side launches of the longest subjects that ran as pipelines of one-wave stages over many CUs (swdrv_pipeline_launches)."""
        return int(lib.swdrv_pipeline_launches(self.handle))

    def tail_overlaps(self):
        """Queries whose bulk launch was gated on the dry signal of the query before (swdrv_tail_overlaps)."""
        return int(lib.swdrv_tail_overlaps(self.handle))

    def numa_node(self, gpu=0):
        """NUMA node of the GPU's PCI function (-1: unknown)."""
        return int(lib.swdrv_numa_node(self.handle, gpu))

    def device_of(self, gpu=0):
        return int(lib.swdrv_device_of(self.handle, gpu))

    def streamed_bytes(self):
        """Subject bytes copied host -> device by scans since the driver was created (all GPUs)."""
        return int(lib.swdrv_streamed_bytes(self.handle))

    def last_scores(self, gpu=0):
        """Every score of the last scan on one GPU and the global id of each position."""
        n = self.shard_info(gpu)["subjects"]
        s = np.zeros(max(n, 1), dtype=np.float32)
        i = np.zeros(max(n, 1), dtype=np.int64)
        _check(lib.swdrv_last_scores(self.handle, gpu, s.ctypes.data, i.ctypes.data))
        return s[:n].astype(np.int32), i[:n]

    def all_scores(self):
        """Scores of the last scan for every subject of this driver's shards, indexed by global id -> (ids, scores)."""
        ids, sc = [], []
        for g in range(self.num_gpus()):
            s, i = self.last_scores(g)
            ids.append(i)
            sc.append(s)
        return np.concatenate(ids), np.concatenate(sc)

    def batch_intervals(self):
        buf = np.zeros(3 * 65536, dtype=np.float32)
        n = lib.swdrv_batch_intervals(self.handle, buf.ctypes.data, 65536)
        if n < 0:
            raise DriverError(lib.swdrv_last_error().decode())
        n = min(n, 65536)
        return [(int(buf[3 * i]), float(buf[3 * i + 1]), float(buf[3 * i + 2])) for i in range(n)]

    def gpu_spans(self):
        buf = np.zeros(2 * 64, dtype=np.float64)
        n = lib.swdrv_gpu_spans(self.handle, buf.ctypes.data, 64)
        if n < 0:
            raise DriverError(lib.swdrv_last_error().decode())
        return [(float(buf[2 * i]), float(buf[2 * i + 1])) for i in range(n)]

    def num_sequences(self):
        return int(lib.swdrv_num_sequences(self.handle))

    def num_gpus(self):
        return int(lib.swdrv_num_gpus(self.handle))

    def set_num_top(self, k):
        lib.swdrv_set_num_top(self.handle, k)
        self.num_top = k

    def scan(self, query_letters):
        if isinstance(query_letters, str):
            query_letters = query_letters.encode()
        self._calibrate_for_submit(query_letters)
        cap = max(self.num_top, 1)
        scores = np.zeros(cap, dtype=np.int32)
        ids = np.zeros(cap, dtype=np.int64)
        nres, novf = ctypes.c_int(), ctypes.c_int()
        sec, gcups = ctypes.c_double(), ctypes.c_double()
        self._checked(lib.swdrv_scan(self.handle, query_letters, len(query_letters), scores.ctypes.data, ids.ctypes.data, cap,
                                     ctypes.byref(nres), ctypes.byref(novf), ctypes.byref(sec), ctypes.byref(gcups)), True)
        n = nres.value
        return self._with_statistics({"scores": scores[:n].copy(), "ids": ids[:n].copy(), "num_overflows": novf.value,
                                      "num_rescored": int(lib.swdrv_last_rescored(self.handle)),
                                      "seconds": sec.value, "gcups": gcups.value})

    def scan_pssm(self, pssm):
        """scan() with a position-specific scoring matrix as the query: (qlen, 21) int8, row i = query position i, column c =
        subject code c, column 20 negative (cudasw4_amd.pssm).  Same result dict as scan()."""
        from . import pssm as _pssm
        m = _pssm.as_pssm(pssm)
        self._calibrate_for_submit(m)
        cap = max(self.num_top, 1)
        scores = np.zeros(cap, dtype=np.int32)
        ids = np.zeros(cap, dtype=np.int64)
        nres, novf = ctypes.c_int(), ctypes.c_int()
        sec, gcups = ctypes.c_double(), ctypes.c_double()
        self._checked(_pssm_fns()[0](self.handle, m.ctypes.data, m.shape[0], scores.ctypes.data, ids.ctypes.data, cap,
                                     ctypes.byref(nres), ctypes.byref(novf), ctypes.byref(sec), ctypes.byref(gcups)), True)
        n = nres.value
        return self._with_statistics({"scores": scores[:n].copy(), "ids": ids[:n].copy(), "num_overflows": novf.value,
                                      "num_rescored": int(lib.swdrv_last_rescored(self.handle)),
                                      "seconds": sec.value, "gcups": gcups.value})

    def submit_pssm(self, pssm):
        """submit() with a PSSM query; collect() returns its results.  May be in flight together with a letter query."""
        from . import pssm as _pssm
        m = _pssm.as_pssm(pssm)
        self._calibrate_for_submit(m)
        self._checked(_pssm_fns()[1](self.handle, m.ctypes.data, m.shape[0]), True)

    def submit(self, query_letters):
        """First half of scan(): enqueue the query on every GPU without waiting (at most two in flight)."""
        if isinstance(query_letters, str):
            query_letters = query_letters.encode()
        self._calibrate_for_submit(query_letters)
        self._checked(lib.swdrv_scan_submit(self.handle, query_letters, len(query_letters)), True)

    def collect(self):
        """Second half of scan(): the merged results of the oldest submitted query."""
        cap = max(self.num_top, 1)
        scores = np.zeros(cap, dtype=np.int32)
        ids = np.zeros(cap, dtype=np.int64)
        nres, novf = ctypes.c_int(), ctypes.c_int()
        sec, gcups = ctypes.c_double(), ctypes.c_double()
        self._checked(lib.swdrv_scan_collect(self.handle, scores.ctypes.data, ids.ctypes.data, cap, ctypes.byref(nres),
                                             ctypes.byref(novf), ctypes.byref(sec), ctypes.byref(gcups)), False)
        n = nres.value
        return self._with_statistics({"scores": scores[:n].copy(), "ids": ids[:n].copy(), "num_overflows": novf.value,
                                      "num_rescored": int(lib.swdrv_last_rescored(self.handle)),
                                      "seconds": sec.value, "gcups": gcups.value})

    def scan_many(self, queries):
        """Every query of a list, pipelined: the next query is submitted before the current one is collected, so the
        GPUs stay busy across query boundaries (what `align` does with a query file).  -> list of result dicts."""
        out = []
        for q in queries:
            self.submit(q)
            while lib.swdrv_in_flight(self.handle) >= max(2, int(lib.swdrv_preferred_in_flight(self.handle, len(q)))):
                out.append(self.collect())
        while lib.swdrv_in_flight(self.handle) > 0:
            out.append(self.collect())
        return out

    def scan_stream(self, queries):
        """Every query of a list the way `align` processes a query file (align_main.cpp: processQueryFile): one query at a
        time like the reference, except where the driver says the tail hand-over applies to the query just submitted (a
        small resident shard, or a query that is scanned in a few milliseconds) — then the next query is submitted before
        that one is collected.  -> list of result dicts, in the order of the queries."""
        out = []
        for q in queries:
            self.submit(q)
            limit = int(lib.swdrv_preferred_in_flight(self.handle, len(q)))
            while lib.swdrv_in_flight(self.handle) >= limit:
                out.append(self.collect())
        while lib.swdrv_in_flight(self.handle) > 0:
            out.append(self.collect())
        return out

    def align_hits(self, query_letters, result, max_hsps=1, min_score=None):
        """Coordinates, counts and CIGAR of the hits of a scan/collect result of `query_letters` (swdrv_align_hits).
        -> (structured array of capi.align_result_dtype(), list of CIGAR strings, "*" where there is none)
        max_hsps > 1 (swdrv_align_hsps; min_score is then required): up to that many non-overlapping alignments per hit, the
        further ones scoring at least min_score.  -> one list per hit of (record, CIGAR string): the hit's first alignment
        (whatever its status), then its further alignments, best first."""
        from . import capi
        _check_hsps(max_hsps, min_score)
        if isinstance(query_letters, str):
            query_letters = query_letters.encode()
        ids = np.ascontiguousarray(result["ids"], dtype=np.int64)
        scores = np.ascontiguousarray(result["scores"], dtype=np.int32)
        n = len(ids)
        if max_hsps > 1:
            res = np.zeros(n * max_hsps, dtype=capi.align_result_dtype())
            cap = max_hsps * sum(len(query_letters) + self.reference_length(int(i)) for i in ids)
            cigar = np.zeros(max(cap, 1), dtype=np.uint32)
            _check(_align_hsps_fns()[0](self.handle, query_letters, len(query_letters), ids.ctypes.data, scores.ctypes.data, n,
                                        max_hsps, min_score, res.ctypes.data, cigar.ctypes.data, cap))
            return _hsp_lists(res, cigar, n, max_hsps)
        res = np.zeros(n, dtype=capi.align_result_dtype())
        cap = sum(len(query_letters) + self.reference_length(int(i)) for i in ids)
        cigar = np.zeros(max(cap, 1), dtype=np.uint32)
        _check(_align_fn()(self.handle, query_letters, len(query_letters), ids.ctypes.data, scores.ctypes.data, n,
                           res.ctypes.data, cigar.ctypes.data, cap))
        cigars = [capi.cigar_string(cigar[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])]) for r in res]
        return res, cigars

    def align_hits_pssm(self, pssm, result, consensus=None, max_hsps=1, min_score=None):
        """align_hits for the hits of a scan_pssm / submit_pssm result of `pssm` (swdrv_align_hits_pssm).  consensus: one
        residue letter per position, which identities and '=' / 'X' are counted against (a non-standard letter is identical
        to nothing); None: the best-scoring standard residue of every row (pssm.consensus_of).  Returns what align_hits returns,
        with max_hsps > 1 (swdrv_align_hsps_pssm) its lists."""
        from . import capi, pssm as _pssm
        _check_hsps(max_hsps, min_score)
        m = _pssm.as_pssm(pssm)
        qlen = m.shape[0]
        if consensus is not None:
            if isinstance(consensus, str):
                consensus = consensus.encode()
            if len(consensus) != qlen:
                raise ValueError("consensus has %d residues, the PSSM %d rows" % (len(consensus), qlen))
        ids = np.ascontiguousarray(result["ids"], dtype=np.int64)
        scores = np.ascontiguousarray(result["scores"], dtype=np.int32)
        n = len(ids)
        if max_hsps > 1:
            res = np.zeros(n * max_hsps, dtype=capi.align_result_dtype())
            cap = max_hsps * sum(qlen + self.reference_length(int(i)) for i in ids)
            cigar = np.zeros(max(cap, 1), dtype=np.uint32)
            _check(_align_hsps_fns()[1](self.handle, m.ctypes.data, qlen, consensus, ids.ctypes.data, scores.ctypes.data, n,
                                        max_hsps, min_score, res.ctypes.data, cigar.ctypes.data, cap))
            return _hsp_lists(res, cigar, n, max_hsps)
        res = np.zeros(n, dtype=capi.align_result_dtype())
        cap = sum(qlen + self.reference_length(int(i)) for i in ids)
        cigar = np.zeros(max(cap, 1), dtype=np.uint32)
        _check(_align_pssm_fn()(self.handle, m.ctypes.data, qlen, consensus, ids.ctypes.data, scores.ctypes.data, n,
                                res.ctypes.data, cigar.ctypes.data, cap))
        cigars = [capi.cigar_string(cigar[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])]) for r in res]
        return res, cigars

    def hit_msa(self, query_letters, result, max_identity=None, pssm=None, consensus=None, fmt="a3m", query_header="query",
                min_coverage=None, min_query_identity=None, diff=None, ladder=None):
        """The query-anchored multiple alignment of the hits of `result` (swdrv_hit_msa): the hits are aligned as
        align_hits aligns them — with `pssm` given as align_hits_pssm does, `query_letters` (or `consensus`) being the master —
        and the rows, residue counts and the greedy redundancy filter are computed on the GPU from what the aligner left there.
        max_identity: None (no filter) or 1 .. 100.
        -> dict: rows ((n + 1, qlen) uint8, row n the master; 0..19 residue, 20 other, 21 gap, 22 none), residues (n + 1),
        keep (n + 1), purged, a3m (the text `align --outMsa` writes for the kept hits), results, cigars
        With any of min_coverage (1 .. 100), min_query_identity (1 .. 100), diff (>= 1) or ladder (strictly ascending rungs)
        the rows go through the selection of DESIGN.md §18 instead (swdrv_hit_msa_select): the ladder defaults to {max_identity}
        and without max_identity to {100} under coverage / query identity alone (only a hit whose every residue repeats a kept
        row is thinned), under diff to 20, 30, ... below max_identity (default 90) and then that.  The dict then also has
        state (n + 1), depth (qlen), counts (kept hits, below coverage, below query identity, thinned) and ladder (the rungs
        that were used); keep is state == 1 and purged counts the thinned hits."""
        import tempfile
        from . import capi, pssm as _pssm
        master = consensus if consensus is not None else query_letters
        if isinstance(master, str):
            master = master.encode()
        qlen = len(master)
        P = 0 if max_identity is None else int(max_identity)
        if max_identity is not None and not 1 <= P <= 100:
            raise ValueError("max_identity must lie in [1, 100]")
        scored_with = None
        if pssm is not None:
            scored_with = _pssm.as_pssm(pssm)
            if scored_with.shape[0] != qlen:
                raise ValueError("the master has %d residues, the PSSM %d rows" % (qlen, scored_with.shape[0]))
        ids = np.ascontiguousarray(result["ids"], dtype=np.int64)
        scores = np.ascontiguousarray(result["scores"], dtype=np.int32)
        n = len(ids)
        res = np.zeros(max(n, 1), dtype=capi.align_result_dtype())
        cap = sum(qlen + self.reference_length(int(i)) for i in ids)
        cigar = np.zeros(max(cap, 1), dtype=np.uint32)
        rows = np.zeros((n + 1, max(qlen, 1)), dtype=np.uint8)
        residues = np.zeros(n + 1, dtype=np.int32)
        keep = np.zeros(n + 1, dtype=np.uint8)
        purged = ctypes.c_int32(0)
        selecting = any(v is not None for v in (min_coverage, min_query_identity, diff, ladder))
        if selecting:
            from . import msa as _msa
            C = 0 if min_coverage is None else int(min_coverage)
            Q = 0 if min_query_identity is None else int(min_query_identity)
            D = 0 if diff is None else int(diff)
            if (min_coverage is not None and not 1 <= C <= 100) or (min_query_identity is not None and not 1 <= Q <= 100):
                raise ValueError("min_coverage and min_query_identity must lie in [1, 100]")
            if diff is not None and D < 1:
                raise ValueError("diff must be at least 1")
            if ladder is not None:
                if max_identity is not None:
                    raise ValueError("ladder and max_identity cannot be combined: the ladder's last rung is the cut")
                rungs = _msa.check_ladder(ladder)
            elif diff is not None:
                rungs = _msa.default_ladder(P if max_identity is not None else 90)
            else:   # coverage / query identity alone: max_identity, or the weakest cut the selection has
                rungs = [P if max_identity is not None else 100]
            state = np.zeros(n + 1, dtype=np.uint8)
            depth = np.zeros(qlen, dtype=np.int32)
            counts = np.zeros(4, dtype=np.int32)
            lad = np.array(rungs, dtype=np.int32)
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "hits." + fmt)
                _check(_msa_select_fn()(self.handle, master, qlen, scored_with.ctypes.data if scored_with is not None else None,
                                        ids.ctypes.data, scores.ctypes.data, n, C, Q, D, lad.ctypes.data, len(lad),
                                        query_header.encode(), path.encode(), MSA_FORMATS[fmt], res.ctypes.data, cigar.ctypes.data,
                                        cap, rows.ctypes.data, residues.ctypes.data, state.ctypes.data, depth.ctypes.data,
                                        counts.ctypes.data))
                with open(path) as f:
                    text = f.read()
            res = res[:n]
            cigars = [capi.cigar_string(cigar[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])]) for r in res]
            return {"rows": rows, "residues": residues, "keep": (state == 1).astype(np.uint8), "purged": int(counts[3]), "a3m": text,
                    "results": res, "cigars": cigars, "state": state, "depth": depth, "counts": counts.tolist(), "ladder": rungs}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "hits." + fmt)
            _check(_msa_fns()[1](self.handle, master, qlen, scored_with.ctypes.data if scored_with is not None else None,
                                 ids.ctypes.data, scores.ctypes.data, n, P, query_header.encode(), path.encode(), MSA_FORMATS[fmt],
                                 res.ctypes.data, cigar.ctypes.data, cap, rows.ctypes.data, residues.ctypes.data, keep.ctypes.data,
                                 ctypes.byref(purged)))
            with open(path) as f:
                text = f.read()
        res = res[:n]
        cigars = [capi.cigar_string(cigar[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])]) for r in res]
        return {"rows": rows, "residues": residues, "keep": keep, "purged": int(purged.value), "a3m": text, "results": res,
                "cigars": cigars}

    def build_pssm(self, query_letters, result, pssm=None, min_score=0, pseudocount=10.0, max_evalue=None, purge_identity=None):
        """One step of an iterated search (swdrv_build_pssm): the hits of `result` — a scan of `query_letters`, or with
        `pssm` given a scan_pssm of it, `query_letters` being the master sequence — aligned, filtered (score >= min_score,
        with a CIGAR, not a copy of the master), accumulated on the GPU and converted.
        max_evalue: in place of the min_score test a hit takes part when its E-value under the fit of `result`'s own scan is
        at most max_evalue (`result` must come from a scan with set_statistics(True); under NO_FIT no hit takes part); the
        other rules are unchanged, and info's below_score counts the hits the E-value left out.
        purge_identity: None, or P in 1 .. 100 (swdrv_build_pssm_purged): the hits that pass those rules go through the greedy
        redundancy filter of hit_msa in rank order, and those at least P per cent identical to the master or to an earlier
        hit that went in are left out before the weighting; info["purged"] counts them.
        -> ((qlen, 21) int8 PSSM, info dict: used, below_score, no_trace, copies, lambda, included = ids that took part)"""
        from . import pssm as _pssm
        if purge_identity is not None and not 1 <= int(purge_identity) <= 100:
            raise ValueError("purge_identity must lie in [1, 100]")
        if max_evalue is not None:
            if "evalues" not in result:
                raise ValueError("max_evalue needs a result with E-values: set_statistics(True) before the scan")
            ev = np.asarray(result["evalues"])
            keep = (ev >= 0) & (ev <= float(max_evalue))
            kept = {"ids": np.asarray(result["ids"])[keep], "scores": np.asarray(result["scores"])[keep]}
            built, info = self.build_pssm(query_letters, kept, pssm=pssm, min_score=0, pseudocount=pseudocount,
                                          purge_identity=purge_identity)
            info["below_score"] += int(len(keep) - keep.sum())
            return built, info
        if isinstance(query_letters, str):
            query_letters = query_letters.encode()
        qlen = len(query_letters)
        scored_with = None
        if pssm is not None:
            scored_with = _pssm.as_pssm(pssm)
            if scored_with.shape[0] != qlen:
                raise ValueError("the master has %d residues, the PSSM %d rows" % (qlen, scored_with.shape[0]))
        ids = np.ascontiguousarray(result["ids"], dtype=np.int64)
        scores = np.ascontiguousarray(result["scores"], dtype=np.int32)
        n = len(ids)
        out = np.zeros((max(qlen, 1), 21), dtype=np.int8)
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        info = _PssmInfo(included=flags.ctypes.data)
        purged = ctypes.c_int32(0)
        if purge_identity is None:
            _check(_build_fns()[1](self.handle, query_letters, qlen, scored_with.ctypes.data if scored_with is not None else None,
                                   ids.ctypes.data, scores.ctypes.data, n, int(min_score), float(pseudocount), out.ctypes.data,
                                   ctypes.byref(info)))
        else:
            _check(_msa_fns()[0](self.handle, query_letters, qlen, scored_with.ctypes.data if scored_with is not None else None,
                                 ids.ctypes.data, scores.ctypes.data, n, int(min_score), float(pseudocount), int(purge_identity),
                                 out.ctypes.data, ctypes.byref(info), ctypes.byref(purged)))
        built = {"used": info.used, "below_score": info.below_score, "no_trace": info.no_trace, "copies": info.copies,
                 "lambda": info.lambda_, "included": [int(i) for i, f in zip(ids, flags[:n]) if f]}
        if purge_identity is not None:
            built["purged"] = int(purged.value)
        return out[:qlen], built

    def iterate(self, query_letters, rounds, min_score=0, pseudocount=10.0, max_evalue=None, purge_identity=None):
        """Iterated profile search: round 1 scans with the letters; every round builds a PSSM from its reported hits
        (build_pssm), and round r + 1 scans with the one of round r.  Stops after `rounds` rounds, or when a round includes
        the ids the round before included (then the last info has converged = True).  max_evalue: hits go in by their
        E-value under each round's own fit instead of by min_score (needs set_statistics(True)).  purge_identity: build_pssm's,
        in every round.
        -> (result of the last round, PSSM built from it, list of the rounds' info dicts)"""
        if rounds < 1:
            raise ValueError("rounds must be at least 1")
        if max_evalue is not None and not self.statistics:
            raise ValueError("max_evalue needs set_statistics(True)")
        result = self.scan(query_letters)
        scoring, infos = None, []
        while True:
            built, info = self.build_pssm(query_letters, result, pssm=scoring, min_score=min_score, pseudocount=pseudocount,
                                          max_evalue=max_evalue, purge_identity=purge_identity)
            info["converged"] = bool(infos) and sorted(info["included"]) == sorted(infos[-1]["included"])
            infos.append(info)
            if len(infos) >= rounds or info["converged"]:
                return result, built, infos
            scoring = built
            result = self.scan_pssm(scoring)

    def reference_length(self, i):
        return int(lib.swdrv_reference_length(self.handle, i))

    def reference_header(self, i):
        buf = ctypes.create_string_buffer(4096)
        lib.swdrv_reference_header(self.handle, i, buf, 4096)
        return buf.value.decode()
