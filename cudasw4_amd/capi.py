"""ctypes binding of the C ABI in include/cudasw4_amd.h (libcudasw4_amd.so).

This is plumbing: every compute call goes to the HIP library.  There is no Python or CPU fallback —
if the shared library is missing the import of this module raises, and without a GPU
`Context()` raises `SwError` (SW_ERR_NO_DEVICE).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CUDASW4_AMD_LIB", os.path.join(_HERE, "lib", "libcudasw4_amd.so"))  # env override: A/B builds

KIND_F16X2, KIND_I16X2, KIND_I32, KIND_F32 = 0, 1, 2, 3
KIND_NAMES = {"half2": KIND_F16X2, "f16x2": KIND_F16X2, "dpxs16": KIND_I16X2, "i16x2": KIND_I16X2,
              "dpxs32": KIND_I32, "i32": KIND_I32, "float": KIND_F32, "f32": KIND_F32}
MAX_ACC = {KIND_F16X2: 2048, KIND_I16X2: 25000}

SW_OK = 0
ERR_NAMES = {-1: "SW_ERR_INVALID", -2: "SW_ERR_HIP", -3: "SW_ERR_NO_QUERY", -4: "SW_ERR_NO_MATRIX",
             -5: "SW_ERR_TEMP", -6: "SW_ERR_NO_DEVICE"}

# every symbol include/cudasw4_amd.h (the boundary) and include/cudasw4_amd_engine.h (the batch engine's building blocks) declare
EXPORTS = ["sw_batch_create", "sw_batch_destroy", "sw_scan_batch", "sw_batch_join", "sw_batch_side_events", "sw_batch_feedback",
           "sw_batch_handshake_active", "sw_batch_stats", "sw_batch_signal_state", "sw_batch_open_gates", "sw_batch_reset",
           "sw_batch_test_lose_side_launch", "sw_query_length", "sw_batch_describe_plan",
           "sw_version", "sw_last_error", "sw_device_count", "sw_ctx_create", "sw_ctx_destroy", "sw_set_matrix",
           "sw_set_query", "sw_scan_temp_bytes", "sw_scan_partition", "sw_rescore_overflow", "sw_rescore_overflow_stat",
           "sw_topk_temp_bytes",
           "sw_topk", "sw_plan_query", "sw_check_letter_codes", "sw_plan_launch", "sw_set_start_signal",
           "sw_window_overlap", "sw_reduce_windows", "sw_rescore_service", "sw_rescore_overflow_claim",
           "sw_rescore_service_temp_bytes", "sw_streams_run_concurrently", "sw_set_dry_signal", "sw_set_dirty_counter", "sw_set_grid_reserve",
           "sw_set_long16_min", "sw_scan_rows_pipelined",
           "sw_scan_rows_pipelined_temp_bytes", "sw_probe_handshake", "sw_launch_vgpr_slot",
           "sw_set_rows_pipeline_slot", "sw_packed_launch_falls_back", "sw_scan_partition_counted", "sw_rescore_overflow_pipelined", "sw_rescore_overflow_pipelined_temp_bytes", "sw_measure_valu_rate",
           "sw_align_hits"]
# ... and include/cudasw4_amd_pssm.h (profile search: a position-specific scoring matrix as the query)
PSSM_EXPORTS = ["sw_set_query_pssm", "sw_query_is_pssm", "sw_align_hits_pssm", "sw_pssm_accumulate"]
# ... and include/cudasw4_amd_stats.h (search statistics: the (length bin, score) histogram of a scan's scores)
STATS_EXPORTS = ["sw_score_histogram"]
STATS_LBINS, STATS_SBINS = 64, 256
# ... and include/cudasw4_amd_rank.h (ranking by E-value: Z-score keys for sw_topk, and the gather behind it)
RANK_EXPORTS = ["sw_zscore_keys", "sw_gather_hits"]
RANK_KEY_NONE = -3.0e38   # as float32: the key of a subject that was not scored
# ... and include/cudasw4_amd_hsps.h (hit alignment: up to MAX_HSPS non-overlapping local alignments per hit)
HSPS_EXPORTS = ["sw_align_hsps", "sw_align_hsps_pssm"]
MAX_HSPS = 16
# ... and include/cudasw4_amd_shuffle.h (statistics calibrated on shuffled subjects: replicas of a block, every subject permuted)
SHUFFLE_EXPORTS = ["sw_shuffle_subjects"]
# ... and include/cudasw4_amd_mask.h (low-complexity masking of the subjects on the device)
MASK_EXPORTS = ["sw_mask_subjects", "sw_mask_subjects_phases"]
# ... and include/cudasw4_amd_msa.h (the query-anchored MSA of a query's hits and its redundancy filter)
MSA_EXPORTS = ["sw_msa_filter"]
MSA_GAP, MSA_NONE, MSA_MAX_HITS = 21, 22, 1 << 15
# ... and include/cudasw4_amd_msa_select.h (coverage, identity to the query and the diversity selection over those rows)
MSA_SELECT_EXPORTS = ["sw_msa_select"]
MSA_SELECT_MAX_HITS, MSA_SELECT_MAX_LADDER = 1 << 14, 16
MSA_STATE_NONE, MSA_STATE_KEPT, MSA_STATE_COVERAGE, MSA_STATE_QUERY_IDENTITY, MSA_STATE_THINNED = 0, 1, 2, 3, 4


# sw_align_hits (include/cudasw4_amd.h): result records, statuses, flags, CIGAR op codes
ALIGN_OK, ALIGN_EMPTY, ALIGN_NO_TRACE, ALIGN_SCORE_MISMATCH, ALIGN_BAD_LENGTH = 0, 1, 2, 3, 4
ALIGN_NOT_COMPUTED = 5   # sw_align_hsps: behind an alignment that has no traceback
ALIGN_COORDS_ONLY = 1
CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}
ALIGN_RESULT_FIELDS = ["score", "status", "q_begin", "q_end", "s_begin", "s_end", "columns", "identities", "mismatches",
                       "gap_opens", "gap_columns", "cigar_len"]


def align_result_dtype():
    import numpy as np
    return np.dtype([(f, np.int32) for f in ALIGN_RESULT_FIELDS] + [("cigar_offset", np.int64)])


def align_trace_bytes(rows, cols):
    """trace budget one pair needs for a rectangle of rows x cols cells (sw_align_args::trace_bytes)"""
    return (rows + 511) // 512 * (cols + 63) * 256


def cigar_string(words):
    return "".join("%d%s" % (int(w) >> 4, CIGAR_OPS[int(w) & 15]) for w in words) or "*"


class _AlignArgs(ctypes.Structure):
    _fields_ = [("query", ctypes.c_void_p), ("qlen", ctypes.c_int32), ("n", ctypes.c_int32),
                ("chars", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("lengths", ctypes.c_void_p),
                ("max_subject_len", ctypes.c_int32), ("gop", ctypes.c_int), ("gex", ctypes.c_int),
                ("expected_scores", ctypes.c_void_p), ("results", ctypes.c_void_p), ("cigar", ctypes.c_void_p),
                ("cigar_offsets", ctypes.c_void_p), ("flags", ctypes.c_int), ("trace_bytes", ctypes.c_size_t),
                ("temp", ctypes.c_void_p), ("temp_bytes", ctypes.c_size_t),
                ("temp_bytes_needed", ctypes.POINTER(ctypes.c_size_t)), ("phase_events", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


class _HspArgs(ctypes.Structure):
    _fields_ = [("max_hsps", ctypes.c_int32), ("min_score", ctypes.c_int32)]


class _MaskParams(ctypes.Structure):
    _fields_ = [("window", ctypes.c_int32), ("trigger_sum", ctypes.c_int32), ("extend_sum", ctypes.c_int32)]


class SwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "SW_ERR"), code, msg))
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libcudasw4_amd.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C cudasw4_amd/csrc`): %s" % LIB_PATH)
    # PyTorch wheels bundle their own HIP runtime.  If this library pulled in the system's libamdhip64 first, a later
    # `import torch` would bring a second runtime into the process and find no GPU: load torch's first when it is there.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    L.sw_version.restype = ctypes.c_char_p
    L.sw_last_error.restype = ctypes.c_char_p
    L.sw_device_count.restype = ctypes.c_int
    L.sw_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.sw_ctx_destroy.argtypes = [vp]
    L.sw_set_matrix.argtypes = [vp, vp, ctypes.c_int]
    L.sw_set_query.argtypes = [vp, vp, i32, vp]
    L.sw_scan_temp_bytes.restype = sz
    L.sw_scan_temp_bytes.argtypes = [vp, ctypes.c_int, ctypes.c_int, i32, i32]
    L.sw_scan_partition.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, i32, i32, i32, ctypes.c_int,
                                    ctypes.c_int, vp, vp, i64, vp, vp, ctypes.c_int, vp, sz, vp]
    L.sw_rescore_overflow.argtypes = [vp, ctypes.c_int, vp, vp, i32, vp, vp, vp, i32, ctypes.c_int, ctypes.c_int,
                                      vp, vp, i64, vp, sz, vp]
    L.sw_rescore_overflow_stat.argtypes = [vp, ctypes.c_int, vp, vp, i32, vp, vp, vp, i32, ctypes.c_int, ctypes.c_int,
                                           vp, vp, i64, vp, sz, i32, vp, vp]
    L.sw_topk_temp_bytes.restype = sz
    L.sw_topk_temp_bytes.argtypes = [i64, ctypes.c_int]
    L.sw_topk.argtypes = [vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, sz, vp]
    L.sw_plan_query.argtypes = [ctypes.c_int, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.sw_check_letter_codes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.sw_set_start_signal.argtypes = [vp, vp]
    L.sw_probe_handshake.argtypes = [vp, vp, vp, vp]
    L.sw_rescore_overflow_claim.argtypes = [vp, ctypes.c_int, vp, vp, i32, vp, vp, vp, i32, ctypes.c_int, ctypes.c_int, vp, vp, i64, vp, sz, i32, vp, vp]
    L.sw_rescore_overflow_pipelined_temp_bytes.restype = sz
    L.sw_rescore_overflow_pipelined_temp_bytes.argtypes = [vp, i32]
    L.sw_rescore_overflow_pipelined.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, i32, ctypes.c_int, ctypes.c_int, vp, vp, i64, vp, i32, vp, vp, sz, vp]
    L.sw_measure_valu_rate.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.sw_launch_vgpr_slot.argtypes = [vp, ctypes.c_int, ctypes.c_int, i32, i32]
    L.sw_set_rows_pipeline_slot.argtypes = [vp, ctypes.c_int]
    L.sw_set_dry_signal.argtypes = [vp, vp, ctypes.c_uint32]
    L.sw_set_grid_reserve.argtypes = [vp, i32]
    L.sw_set_long16_min.argtypes = [vp, i32]
    L.sw_scan_rows_pipelined_temp_bytes.restype = sz
    L.sw_scan_rows_pipelined_temp_bytes.argtypes = [vp, i32, i32]
    L.sw_scan_rows_pipelined.argtypes = [vp, vp, vp, vp, i32, i32, i32, ctypes.c_int, ctypes.c_int, vp, vp, i64, vp, vp, vp, i32, vp, sz, vp]
    L.sw_window_overlap.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.sw_window_overlap.restype = i32
    L.sw_reduce_windows.argtypes = [vp, vp, vp, vp, i32, vp, vp, ctypes.c_int64, vp]
    L.sw_plan_launch.argtypes = [vp, ctypes.c_int, ctypes.c_int, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32),
                                 ctypes.POINTER(i32), ctypes.POINTER(i32)]
    if hasattr(L, "sw_align_hits"):   # (CUDASW4_AMD_LIB may name an older build)
        L.sw_align_hits.argtypes = [vp, ctypes.POINTER(_AlignArgs)]
    if hasattr(L, "sw_set_query_pssm"):
        L.sw_set_query_pssm.argtypes = [vp, vp, i32, vp]
        L.sw_query_is_pssm.argtypes = [vp]
    if hasattr(L, "sw_score_histogram"):
        L.sw_score_histogram.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp]
    if hasattr(L, "sw_zscore_keys"):
        dbl = ctypes.c_double
        L.sw_zscore_keys.argtypes = [vp, vp, vp, i64, dbl, dbl, dbl, dbl, vp, vp, vp, vp]
        L.sw_gather_hits.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
    if hasattr(L, "sw_shuffle_subjects"):
        L.sw_shuffle_subjects.argtypes = [vp, vp, vp, vp, vp, i32, ctypes.c_uint32, i32, i32, vp, sz, vp]
    if hasattr(L, "sw_mask_subjects"):
        L.sw_mask_subjects.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(_MaskParams), vp, vp, sz, ctypes.POINTER(sz), vp, vp]
        L.sw_mask_subjects_phases.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(_MaskParams), vp, vp, sz, vp, vp, ctypes.POINTER(vp)]
    return L


lib = _load()


def check(rc):
    if rc != SW_OK:
        raise SwError(rc, lib.sw_last_error().decode())


def version():
    return lib.sw_version().decode()


def device_count():
    return int(lib.sw_device_count())


def plan_query(kind, qlen):
    r, s = ctypes.c_int32(), ctypes.c_int32()
    check(lib.sw_plan_query(kind, qlen, ctypes.byref(r), ctypes.byref(s)))
    return r.value, s.value


class Context:
    """One per GPU (sw_ctx).  Pointers are passed as integers (tensor.data_ptr())."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        check(lib.sw_ctx_create(device, ctypes.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            lib.sw_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_matrix(self, m21):
        import numpy as np
        m = np.ascontiguousarray(m21, dtype=np.int8).reshape(-1)
        dim = int(round(len(m) ** 0.5))
        check(lib.sw_set_matrix(self.handle, m.ctypes.data, dim))

    def set_query(self, codes, stream=0):
        import numpy as np
        q = np.ascontiguousarray(codes, dtype=np.int8)
        check(lib.sw_set_query(self.handle, q.ctypes.data, len(q), stream))

    def set_query_pssm(self, pssm, stream=0):
        """Install a position-specific scoring matrix (qlen x 21 int8, column 20 negative) as the query: every scan scores
        position i against subject code c with pssm[i][c] until the next set_query / set_query_pssm (cudasw4_amd_pssm.h)."""
        from . import pssm as _pssm
        if not hasattr(lib, "sw_set_query_pssm"):
            raise SwError(-1, "this build of libcudasw4_amd.so has no sw_set_query_pssm")
        m = _pssm.as_pssm(pssm)
        check(lib.sw_set_query_pssm(self.handle, m.ctypes.data, m.shape[0], stream))

    def query_is_pssm(self):
        return bool(lib.sw_query_is_pssm(self.handle))

    def scan_temp_bytes(self, kind, part_id, n, max_subject_len):
        return int(lib.sw_scan_temp_bytes(self.handle, kind, part_id, n, max_subject_len))

    def scan_partition(self, kind, part_id, chars, offsets, lengths, first_pos, n, max_subject_len, gop, gex,
                       scores, ids, id_offset=0, ovf_pos=0, ovf_count=0, ovf_check=0, temp=0, temp_bytes=0, stream=0):
        check(lib.sw_scan_partition(self.handle, kind, part_id, chars, offsets, lengths, first_pos, n, max_subject_len,
                                    gop, gex, scores, ids, id_offset, ovf_pos, ovf_count, ovf_check, temp, temp_bytes,
                                    stream))

    def measure_valu_rate(self, mix, millis=50):
        """-> (lane-instructions per second the device issues of that instruction mix, shader clock in Hz seen by the waves)"""
        r, hz = ctypes.c_double(), ctypes.c_double()
        check(lib.sw_measure_valu_rate(self.handle, mix, millis, ctypes.byref(r), ctypes.byref(hz)))
        return r.value, hz.value

    def launch_vgpr_slot(self, kind, part_id, n, max_subject_len):
        return int(lib.sw_launch_vgpr_slot(self.handle, kind, part_id, n, max_subject_len))

    def set_rows_pipeline_slot(self, vgprs):
        check(lib.sw_set_rows_pipeline_slot(self.handle, vgprs))

    def scan_rows_pipelined_temp_bytes(self, n, max_subject_len):
        return int(lib.sw_scan_rows_pipelined_temp_bytes(self.handle, n, max_subject_len))

    def scan_rows_pipelined(self, chars, offsets, lengths, first_pos, n, max_subject_len, gop, gex, scores, ids, id_offset=0,
                            fail_count=0, temp=0, temp_bytes=0, stream=0, over_limit_count=0, over_limit_count2=0, packed_limit=0):
        """Very long subjects as pipelines of one-wave stages across many CUs (sw_scan_rows_pipelined)."""
        check(lib.sw_scan_rows_pipelined(self.handle, chars, offsets, lengths, first_pos, n, max_subject_len, gop, gex, scores,
                                         ids, id_offset, fail_count, over_limit_count, over_limit_count2, packed_limit, temp,
                                         temp_bytes, stream))

    def rescore_overflow_pipelined_temp_bytes(self, max_subject_len):
        return int(lib.sw_rescore_overflow_pipelined_temp_bytes(self.handle, max_subject_len))

    def rescore_overflow_pipelined(self, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, min_subject_len,
                                   gop, gex, scores, ids, id_offset, fail_count, packed_limit, true_count, temp, temp_bytes, stream=0):
        check(lib.sw_rescore_overflow_pipelined(self.handle, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len,
                                                min_subject_len, gop, gex, scores, ids, id_offset, fail_count, packed_limit,
                                                true_count, temp, temp_bytes, stream))

    def rescore_overflow_claim(self, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, gop, gex,
                               scores, ids, id_offset, temp, temp_bytes, packed_limit, true_count, stream=0):
        check(lib.sw_rescore_overflow_claim(self.handle, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths,
                                            max_subject_len, gop, gex, scores, ids, id_offset, temp, temp_bytes, packed_limit,
                                            true_count, stream))

    def rescore_overflow(self, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, gop, gex,
                         scores, ids, id_offset=0, temp=0, temp_bytes=0, stream=0):
        check(lib.sw_rescore_overflow(self.handle, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths,
                                      max_subject_len, gop, gex, scores, ids, id_offset, temp, temp_bytes, stream))

    def rescore_overflow_stat(self, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths, max_subject_len, gop, gex,
                              scores, ids, id_offset, temp, temp_bytes, packed_limit, true_count, stream=0):
        check(lib.sw_rescore_overflow_stat(self.handle, kind, ovf_pos, ovf_count, max_count, chars, offsets, lengths,
                                           max_subject_len, gop, gex, scores, ids, id_offset, temp, temp_bytes,
                                           packed_limit, true_count, stream))

    def plan_launch(self, kind, part_id, n, max_subject_len):
        """-> (kind computed in, rows per lane, query stripes, lanes per group) of the launch sw_scan_partition
        (part_id >= 0) or sw_rescore_overflow (part_id = -1) would make for the current query."""
        k, r, s, l = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib.sw_plan_launch(self.handle, kind, part_id, n, max_subject_len, ctypes.byref(k), ctypes.byref(r),
                                 ctypes.byref(s), ctypes.byref(l)))
        return k.value, r.value, s.value, l.value

    def check_letter_codes(self, chars, n, bad_flag, stream=0):
        check(lib.sw_check_letter_codes(self.handle, chars, n, bad_flag, stream))

    def topk(self, scores, ids, n, k, out_scores, out_ids, temp, temp_bytes, stream=0):
        check(lib.sw_topk(self.handle, scores, ids, n, k, out_scores, out_ids, temp, temp_bytes, stream))


def align_hits(ctx, query, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, results, cigar=0, cigar_offsets=0,
               expected_scores=0, flags=0, trace_bytes=0, temp=0, temp_bytes=0, stream=0, phase_events=None):
    """sw_align_hits.  ctx: a Context (None: a NULL context); buffers are device pointers as integers.
    With temp == 0 nothing is launched and the scratch all n pairs need in one chunk is returned.
    phase_events: 4 hipEvent_t handles (integers, e.g. torch.cuda.Event(enable_timing=True).cuda_event) or None."""
    need = ctypes.c_size_t(0)
    ev = (ctypes.c_void_p * 4)(*phase_events) if phase_events is not None else None
    a = _AlignArgs(query, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, expected_scores, results, cigar,
                   cigar_offsets, flags, trace_bytes, temp, temp_bytes, ctypes.pointer(need),
                   ctypes.cast(ev, ctypes.c_void_p) if ev is not None else None, stream)
    check(lib.sw_align_hits(ctx.handle if ctx is not None else None, ctypes.byref(a)))
    return int(need.value)


def align_hits_pssm(ctx, pssm, consensus, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, results, cigar=0,
                    cigar_offsets=0, expected_scores=0, flags=0, trace_bytes=0, temp=0, temp_bytes=0, stream=0, phase_events=None):
    """sw_align_hits_pssm: align_hits with a PSSM as the query.  pssm: device pointer to qlen x 21 int8 (row-major);
    consensus: device pointer to qlen codes, or 0 (the best-scoring standard residue of every row).  The other arguments
    and the return value are those of align_hits."""
    if not hasattr(lib, "sw_align_hits_pssm"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_align_hits_pssm")
    f = lib.sw_align_hits_pssm
    if f.argtypes is None:   # bound on first use (CUDASW4_AMD_LIB may name an older build)
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlignArgs), ctypes.c_void_p]
    need = ctypes.c_size_t(0)
    ev = (ctypes.c_void_p * 4)(*phase_events) if phase_events is not None else None
    a = _AlignArgs(consensus or None, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, expected_scores, results, cigar,
                   cigar_offsets, flags, trace_bytes, temp, temp_bytes, ctypes.pointer(need),
                   ctypes.cast(ev, ctypes.c_void_p) if ev is not None else None, stream)
    check(f(ctx.handle if ctx is not None else None, ctypes.byref(a), pssm or None))
    return int(need.value)


def _align_args(query, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, results, cigar, cigar_offsets, expected_scores,
                flags, trace_bytes, temp, temp_bytes, stream, phase_events):
    """-> (sw_align_args, the size_t it reports the scratch in, what has to stay alive during the call)"""
    need = ctypes.c_size_t(0)
    ev = (ctypes.c_void_p * 4)(*phase_events) if phase_events is not None else None
    a = _AlignArgs(query or None, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, expected_scores, results, cigar,
                   cigar_offsets, flags, trace_bytes, temp, temp_bytes, ctypes.pointer(need),
                   ctypes.cast(ev, ctypes.c_void_p) if ev is not None else None, stream)
    return a, need, ev


def align_hsps(ctx, query, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, results, cigar=0, cigar_offsets=0,
               max_hsps=1, min_score=1, expected_scores=0, flags=0, trace_bytes=0, temp=0, temp_bytes=0, stream=0,
               phase_events=None):
    """sw_align_hsps (include/cudasw4_amd_hsps.h): align_hits with up to max_hsps non-overlapping alignments per pair.
    results: n * max_hsps records, cigar_offsets: n * max_hsps + 1 entries, slot (i, k) at i * max_hsps + k; alignments
    k >= 1 that score less than min_score are not reported.  The other arguments and the return value are align_hits'."""
    if not hasattr(lib, "sw_align_hsps"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_align_hsps")
    f = lib.sw_align_hsps
    if f.argtypes is None:   # bound on first use (CUDASW4_AMD_LIB may name an older build)
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlignArgs), ctypes.POINTER(_HspArgs)]
    a, need, _keep = _align_args(query, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, results, cigar, cigar_offsets,
                                 expected_scores, flags, trace_bytes, temp, temp_bytes, stream, phase_events)
    h = _HspArgs(max_hsps, min_score)
    check(f(ctx.handle if ctx is not None else None, ctypes.byref(a), ctypes.byref(h)))
    return int(need.value)


def align_hsps_pssm(ctx, pssm, consensus, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, results, cigar=0,
                    cigar_offsets=0, max_hsps=1, min_score=1, expected_scores=0, flags=0, trace_bytes=0, temp=0, temp_bytes=0,
                    stream=0, phase_events=None):
    """sw_align_hsps_pssm: align_hsps with a PSSM as the query (pssm, consensus: as align_hits_pssm)."""
    if not hasattr(lib, "sw_align_hsps_pssm"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_align_hsps_pssm")
    f = lib.sw_align_hsps_pssm
    if f.argtypes is None:
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlignArgs), ctypes.POINTER(_HspArgs), ctypes.c_void_p]
    a, need, _keep = _align_args(consensus, qlen, n, chars, offsets, lengths, max_subject_len, gop, gex, results, cigar,
                                 cigar_offsets, expected_scores, flags, trace_bytes, temp, temp_bytes, stream, phase_events)
    h = _HspArgs(max_hsps, min_score)
    check(f(ctx.handle if ctx is not None else None, ctypes.byref(a), ctypes.byref(h), pssm or None))
    return int(need.value)


class _PssmAccumulateArgs(ctypes.Structure):
    _fields_ = [("query", ctypes.c_void_p), ("qlen", ctypes.c_int32), ("n", ctypes.c_int32), ("chars", ctypes.c_void_p),
                ("offsets", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("results", ctypes.c_void_p),
                ("cigar", ctypes.c_void_p), ("include", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("weights", ctypes.c_void_p), ("wcounts", ctypes.c_void_p), ("used", ctypes.c_void_p),
                ("phase_events", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


def pssm_accumulate(ctx, query, qlen, n, chars, offsets, lengths, results, cigar, include, counts, weights, wcounts, used,
                    stream=0, phase_events=None):
    """sw_pssm_accumulate (include/cudasw4_amd_pssm.h): residue counts (uint32, qlen x 20), sequence weights (uint64, n + 1,
    the master last) and weighted counts (uint64, qlen x 20) of the n hits sw_align_hits / sw_align_hits_pssm aligned, plus
    the master `query`.  Every buffer is a device pointer as an integer; query and include may be 0.  Asynchronous on
    `stream`.  phase_events: 3 hipEvent_t handles (before, between and after the two launches) or None."""
    if not hasattr(lib, "sw_pssm_accumulate"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_pssm_accumulate")
    f = lib.sw_pssm_accumulate
    if f.argtypes is None:   # bound on first use (CUDASW4_AMD_LIB may name an older build)
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_PssmAccumulateArgs)]
    ev = (ctypes.c_void_p * 3)(*phase_events) if phase_events is not None else None
    a = _PssmAccumulateArgs(query or None, qlen, n, chars or None, offsets or None, lengths or None, results or None,
                            cigar or None, include or None, counts or None, weights or None, wcounts or None, used or None,
                            ctypes.cast(ev, ctypes.c_void_p) if ev is not None else None, stream or None)
    check(f(ctx.handle if ctx is not None else None, ctypes.byref(a)))


class _MsaArgs(ctypes.Structure):
    _fields_ = [("query", ctypes.c_void_p), ("qlen", ctypes.c_int32), ("n", ctypes.c_int32), ("chars", ctypes.c_void_p),
                ("offsets", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("results", ctypes.c_void_p),
                ("cigar", ctypes.c_void_p), ("include", ctypes.c_void_p), ("max_identity", ctypes.c_int32),
                ("rows", ctypes.c_void_p), ("residues", ctypes.c_void_p), ("keep", ctypes.c_void_p), ("purged", ctypes.c_void_p),
                ("pair_ident", ctypes.c_void_p), ("temp", ctypes.c_void_p), ("temp_bytes", ctypes.c_size_t),
                ("temp_bytes_needed", ctypes.POINTER(ctypes.c_size_t)), ("phase_events", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


def msa_filter(ctx, query, qlen, n, chars, offsets, lengths, results, cigar, include, max_identity, residues, keep, purged,
               rows=0, pair_ident=0, temp=0, temp_bytes=0, stream=0, phase_events=None):
    """sw_msa_filter (include/cudasw4_amd_msa.h): the rows of the query-anchored alignment of the n hits sw_align_hits /
    sw_align_hits_pssm aligned (uint8, (n + 1) x qlen, the master last; optional), their residue counts (int32, n + 1), the
    greedy redundancy filter at max_identity per cent (keep: uint8, n + 1; purged: int32, 1; 0 = no filter) and, for tests,
    the pairwise identity counts (uint32, (n + 1) x (n + 1)).  Every buffer is a device pointer as an integer; query, include,
    rows and pair_ident may be 0.  Asynchronous on `stream`.  phase_events: 4 hipEvent_t handles or None.
    -> the temp bytes the call needs; with temp == 0 nothing is launched."""
    if not hasattr(lib, "sw_msa_filter"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_msa_filter")
    f = lib.sw_msa_filter
    if f.argtypes is None:   # bound on first use (CUDASW4_AMD_LIB may name an older build)
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_MsaArgs)]
    ev = (ctypes.c_void_p * 4)(*phase_events) if phase_events is not None else None
    need = ctypes.c_size_t(0)
    a = _MsaArgs(query or None, qlen, n, chars or None, offsets or None, lengths or None, results or None, cigar or None,
                 include or None, max_identity, rows or None, residues or None, keep or None, purged or None, pair_ident or None,
                 temp or None, temp_bytes, ctypes.pointer(need), ctypes.cast(ev, ctypes.c_void_p) if ev is not None else None,
                 stream or None)
    check(f(ctx.handle if ctx is not None else None, ctypes.byref(a)))
    return int(need.value)


class _MsaSelectArgs(ctypes.Structure):
    _fields_ = [("query", ctypes.c_void_p), ("qlen", ctypes.c_int32), ("n", ctypes.c_int32), ("chars", ctypes.c_void_p),
                ("offsets", ctypes.c_void_p), ("lengths", ctypes.c_void_p), ("results", ctypes.c_void_p),
                ("cigar", ctypes.c_void_p), ("include", ctypes.c_void_p), ("min_coverage", ctypes.c_int32),
                ("min_query_identity", ctypes.c_int32), ("diff", ctypes.c_int32), ("ladder", ctypes.POINTER(ctypes.c_int32)),
                ("n_ladder", ctypes.c_int32), ("state", ctypes.c_void_p), ("residues", ctypes.c_void_p),
                ("counts", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("levels", ctypes.c_void_p),
                ("temp", ctypes.c_void_p), ("temp_bytes", ctypes.c_size_t),
                ("temp_bytes_needed", ctypes.POINTER(ctypes.c_size_t)), ("phase_events", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


def msa_select(ctx, query, qlen, n, chars, offsets, lengths, results, cigar, include, min_coverage, min_query_identity, diff,
               ladder, state, residues, counts, depth=0, rows=0, levels=0, temp=0, temp_bytes=0, stream=0, phase_events=None):
    """sw_msa_select (include/cudasw4_amd_msa_select.h): the state of every row of the query-anchored alignment (uint8, n + 1:
    0 none, 1 kept, 2 below min_coverage, 3 below min_query_identity, 4 thinned) under the diversity selection `diff` over the
    identity `ladder` (a host sequence of 1 .. 16 strictly ascending rungs in 1 .. 100), the residue counts (int32, n + 1),
    counts (int32, 4: kept hits, below coverage, below query identity, thinned) and optionally depth (int32, qlen), rows
    (uint8, (n + 1) x qlen) and, for tests, levels (uint8, (n + 1) x (n + 1)).  Every buffer is a device pointer as an
    integer; query, include, depth, rows and levels may be 0.  Asynchronous on `stream`.  phase_events: 4 hipEvent_t handles
    or None.  -> the temp bytes the call needs; with temp == 0 nothing is launched."""
    if not hasattr(lib, "sw_msa_select"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_msa_select")
    f = lib.sw_msa_select
    if f.argtypes is None:   # bound on first use (CUDASW4_AMD_LIB may name an older build)
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_MsaSelectArgs)]
    ev = (ctypes.c_void_p * 4)(*phase_events) if phase_events is not None else None
    rungs = [int(x) for x in ladder] if ladder is not None else []
    lad = (ctypes.c_int32 * max(len(rungs), 1))(*rungs)
    need = ctypes.c_size_t(0)
    a = _MsaSelectArgs(query or None, qlen, n, chars or None, offsets or None, lengths or None, results or None, cigar or None,
                       include or None, min_coverage, min_query_identity, diff,
                       ctypes.cast(lad, ctypes.POINTER(ctypes.c_int32)) if ladder is not None else None, len(rungs),
                       state or None, residues or None, counts or None, depth or None, rows or None, levels or None,
                       temp or None, temp_bytes, ctypes.pointer(need),
                       ctypes.cast(ev, ctypes.c_void_p) if ev is not None else None, stream or None)
    check(f(ctx.handle if ctx is not None else None, ctypes.byref(a)))
    return int(need.value)


def score_histogram(ctx, scores, lengths, n, hist, sumlen, skipped, stream=0):
    """sw_score_histogram (include/cudasw4_amd_stats.h): ADD the n subjects (scores float32, lengths int32) to hist (uint32,
    64 x 256: [length bin][min(score, 255)]), sumlen (uint64, 64) and skipped (uint32, 1: negative scores, binned nowhere).
    Every buffer is a device pointer as an integer; the caller zeroes the outputs.  Asynchronous on `stream`."""
    if not hasattr(lib, "sw_score_histogram"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_score_histogram")
    check(lib.sw_score_histogram(ctx.handle if ctx is not None else None, scores or None, lengths or None, n, hist or None,
                                 sumlen or None, skipped or None, stream or None))


def zscore_keys(ctx, scores, lengths, n, a, b1, sd, z_min, keys, positions=0, count=0, stream=0):
    """sw_zscore_keys (include/cudasw4_amd_rank.h): keys[i] = float32 of the Z-score (scores[i] - a - b1 ln max(lengths[i], 1)) / sd
    for scores[i] >= 0, RANK_KEY_NONE otherwise; positions[i] = i when positions is given; *count (uint64) is INCREASED by the
    subjects with scores[i] >= 0 and z >= z_min (no threshold: -sys.float_info.max).  Every buffer is a device pointer as an
    integer; the caller zeroes count.  Asynchronous on `stream`."""
    if not hasattr(lib, "sw_zscore_keys"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_zscore_keys")
    check(lib.sw_zscore_keys(ctx.handle if ctx is not None else None, scores or None, lengths or None, n, a, b1, sd, z_min,
                             keys or None, positions or None, count or None, stream or None))


def gather_hits(ctx, positions, k, scores, ids, out_scores, out_ids, stream=0):
    """sw_gather_hits (include/cudasw4_amd_rank.h): out_scores[j], out_ids[j] = scores[p], ids[p] for p = positions[j], the k
    positions a sw_topk over keys chose; p = -1 gives (-1, -1).  Device pointers as integers; asynchronous on `stream`."""
    if not hasattr(lib, "sw_gather_hits"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_gather_hits")
    check(lib.sw_gather_hits(ctx.handle if ctx is not None else None, positions or None, k, scores or None, ids or None,
                             out_scores or None, out_ids or None, stream or None))


def shuffle_subjects(ctx, chars, offsets, lengths, n, seed, out, replica_stride, keys=0, first_replica=0, replicas=1, stream=0):
    """sw_shuffle_subjects (include/cudasw4_amd_shuffle.h): replicas first_replica .. first_replica + replicas - 1 of the n
    subjects (chars, offsets, lengths: dbdata layout) to out, replica r of the call at out + r * replica_stride, subject i
    permuted with the key of (seed, keys[i] or the position i, first_replica + r), padding bytes code 20.  Every buffer is a
    device pointer as an integer.  Asynchronous on `stream` behind a read-back of the block's two ends."""
    if not hasattr(lib, "sw_shuffle_subjects"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_shuffle_subjects")
    check(lib.sw_shuffle_subjects(ctx.handle if ctx is not None else None, chars or None, offsets or None, lengths or None,
                                  keys or None, n, seed & 0xFFFFFFFF, first_replica, replicas, out or None, replica_stride,
                                  stream or None))


def mask_subjects(ctx, chars, offsets, lengths, n, window, trigger_sum, extend_sum, out, temp=0, temp_bytes=0, counts=0, stream=0):
    """sw_mask_subjects (include/cudasw4_amd_mask.h): the n subjects (chars, offsets, lengths: dbdata layout) with their
    low-complexity segments replaced by code 20, to out (== chars: in place; otherwise the whole block is written).  temp:
    scratch of temp_bytes bytes (mask_subjects_temp_bytes holds all n subjects in one go; with less the call works through
    ranges of whole subjects); counts (uint64[2]) is INCREASED by the covered positions and the subjects with a segment.
    Every buffer is a device pointer as an integer.  Asynchronous on `stream` behind a read-back of the block's two ends."""
    if not hasattr(lib, "sw_mask_subjects"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_mask_subjects")
    p = _MaskParams(window, trigger_sum, extend_sum)
    check(lib.sw_mask_subjects(ctx.handle if ctx is not None else None, chars or None, offsets or None, lengths or None, n,
                               ctypes.byref(p), out or None, temp or None, temp_bytes, None, counts or None, stream or None))


def mask_subjects_phases(ctx, chars, offsets, lengths, n, window, trigger_sum, extend_sum, out, temp, temp_bytes, events, counts=0,
                         stream=0):
    """sw_mask_subjects_phases: mask_subjects with four HIP events (handles as integers) recorded before the flags, the resolve
    and the apply launch and behind the last one; the scratch must take the block in one go."""
    p = _MaskParams(window, trigger_sum, extend_sum)
    ev = (ctypes.c_void_p * 4)(*[int(e) for e in events])
    check(lib.sw_mask_subjects_phases(ctx.handle if ctx is not None else None, chars or None, offsets or None, lengths or None, n,
                                      ctypes.byref(p), out or None, temp or None, temp_bytes, counts or None, stream or None, ev))


def mask_subjects_temp_bytes(ctx, offsets, n, window=12, trigger_sum=20705, extend_sum=17019, stream=0):
    """the scratch sw_mask_subjects needs to take the n subjects behind `offsets` (device) in one go; nothing is launched"""
    if not hasattr(lib, "sw_mask_subjects"):
        raise SwError(-1, "this build of libcudasw4_amd.so has no sw_mask_subjects")
    p = _MaskParams(window, trigger_sum, extend_sum)
    need = ctypes.c_size_t(0)
    check(lib.sw_mask_subjects(ctx.handle if ctx is not None else None, None, offsets or None, None, n, ctypes.byref(p), None,
                               None, 0, ctypes.byref(need), None, stream or None))
    return int(need.value)


def topk_temp_bytes(n, k):
    return int(lib.sw_topk_temp_bytes(n, k))
