"""One call of sw_align_hits / sw_align_hits_pssm through the C ABI for a case of tests/align_cases.py, with every argument
of sw_align_args open to the caller, and the field-for-field comparison with the scalar references.  Shared by
tests/test_gpu_align_edges.py and tests/fuzz_gpu.py (import only where there is a GPU)."""
import numpy as np

import align_cases as C
import align_ref as A
import oracle_lib as O

SENTINEL = 0x5EA15EA1   # what the CIGAR buffer holds where nothing was written
RESULT_FILL = 0x7B      # ... and every byte of the result records


class Call:
    """res: the result records; words: the CIGAR of every pair; need: the scratch the sizing call reported; cigar: the whole
    CIGAR buffer with one guard word behind the last slot; coff: the slots' offsets"""


def run(torch, capi, ctx, case, subjects, gop, gex, trace=None, caps=None, temp_bytes=None, expected=None, flags=0, max_len=None,
        stream=None, offset_base=0, first=0, db=None):
    """subjects: dbdata code arrays (or db = (chars, offsets, lengths) as they are).  trace: sw_align_args::trace_bytes
    (default: what the largest whole matrix needs); caps: CIGAR slot sizes in words (default qlen + length); temp_bytes:
    default the reported need; max_len: max_subject_len (default the longest subject); stream: a torch stream;
    offset_base: added to every offset (only offsets[i] - offsets[0] counts); first: pass the arrays from pair `first` on."""
    chars, offsets, lengths = db if db is not None else O.make_db(subjects)
    n = len(lengths)
    qlen = case.qlen
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    caps = (qlen + lengths.astype(np.int64)) if caps is None else np.asarray(caps, dtype=np.int64)
    coff = np.zeros(n + 1, dtype=np.int64)
    coff[1:] = np.cumsum(caps)
    offs = (offsets.astype(np.uint64) + np.uint64(offset_base)).view(np.int64)
    dch, doff, dlen, dcoff = dev(chars), dev(offs), dev(lengths), dev(coff)
    dt = capi.align_result_dtype()
    dres = torch.full((max(n, 1) * dt.itemsize,), RESULT_FILL, dtype=torch.uint8, device="cuda")
    dcig = torch.from_numpy(np.full(int(coff[-1]) + 1, SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    dexp = dev(np.asarray(expected, dtype=np.int32)) if expected is not None else None
    if trace is None:
        trace = max([C.trace_bytes(qlen, int(L)) for L in lengths] or [0])
    if max_len is None:
        max_len = int(lengths.max()) if n else 0
    k = first
    skip = int(offsets[k] - offsets[0]) if n else 0
    args = (n - k, dch.data_ptr() + skip, doff.data_ptr() + 8 * k, dlen.data_ptr() + 4 * k, max_len, gop, gex,
            dres.data_ptr() + k * dt.itemsize, dcig.data_ptr(), dcoff.data_ptr() + 8 * k)
    kw = dict(expected_scores=dexp.data_ptr() + 4 * k if dexp is not None else 0, flags=flags, trace_bytes=trace)
    if case.is_pssm:
        dp = dev(np.ascontiguousarray(case.pssm, dtype=np.int8).reshape(-1))
        dc = dev(np.ascontiguousarray(case.consensus, dtype=np.int8)) if case.consensus is not None else None
        call = lambda **more: capi.align_hits_pssm(ctx, dp.data_ptr(), dc.data_ptr() if dc is not None else 0, qlen, *args, **kw, **more)
    else:
        ctx.set_matrix(case.table)
        dq = dev(np.ascontiguousarray(case.q, dtype=np.int8))
        call = lambda **more: capi.align_hits(ctx, dq.data_ptr(), qlen, *args, **kw, **more)
    out = Call()
    out.need = call()
    temp = torch.empty(max(temp_bytes if temp_bytes is not None else out.need, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # the uploads are done whatever stream the kernels run on
    call(temp=temp.data_ptr(), temp_bytes=temp.numel(), stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out.raw = dres.cpu().numpy().tobytes()
    out.res = np.frombuffer(out.raw, dtype=dt)[:n].copy()
    out.cigar = dcig.cpu().numpy().view(np.uint32).copy()
    out.coff = coff
    out.words = [out.cigar[int(coff[i]):int(coff[i]) + max(0, min(int(r["cigar_len"]), int(caps[i])))].copy() if i >= k else None
                 for i, r in enumerate(out.res)]
    return out


def compare(res, words, want, where=()):
    """field for field and CIGAR word for word; want: [(fields, words)].  -> None, or what differs first"""
    for k, (r, w) in enumerate(want):
        got = {f: int(res[k][f]) for f in A.FIELDS}
        if got != r:
            return "pair %d: got %r want %r %r" % (k, got, r, where)
        if words[k].tolist() != w.tolist():
            return "pair %d: CIGAR %s want %s %r" % (k, A.cigar_string(words[k]), A.cigar_string(w), where)
    return None


def unused_words_untouched(call, want):
    """every word of the CIGAR buffer outside the CIGARs of the OK pairs still holds the sentinel, the guard word behind
    the last slot included.  (A pair that ran out of its own slot may have written inside that slot, nowhere else.)"""
    for k, (r, w) in enumerate(want):
        lo, hi = int(call.coff[k]), int(call.coff[k + 1])
        if r["status"] == A.OK:
            lo += r["cigar_len"]
        elif r["status"] == A.NO_TRACE:
            continue
        if not (call.cigar[lo:hi] == SENTINEL).all():
            return "slot %d" % k
    return None if call.cigar[-1] == SENTINEL else "guard word"
