"""One call of sw_align_hsps / sw_align_hsps_pssm through the C ABI for a case of tests/hsp_cases.py, and the comparison with
the scalar reference hsp_ref, slot for slot.  Shared by tests/test_gpu_hsp.py and tests/test_gpu_hsp_soak.py (import only
where there is a GPU)."""
import numpy as np

import align_abi as AB
import align_cases as C
import hsp_cases as HC
import hsp_ref as H
import oracle_lib as O

SENTINEL, RESULT_FILL = AB.SENTINEL, AB.RESULT_FILL


class Call:
    """res: the n * max_hsps records; words: the CIGAR of every slot; need: the scratch the sizing call reported; cigar: the
    whole CIGAR buffer with one guard word behind the last slot; coff: the slots' offsets; raw: the records' bytes"""


def used_bytes(qlen, max_hsps):
    return (4 * (max_hsps - 1) * qlen + 255) // 256 * 256


def run(torch, capi, ctx, case, subjects, gop, gex, max_hsps, min_score, trace=None, caps=None, temp_bytes=None, expected=None,
        max_len=None, plain=False):
    """subjects: dbdata code arrays.  trace: sw_align_args::trace_bytes (default: the largest whole matrix); caps: CIGAR slot
    sizes in words, n * max_hsps (default qlen + length each); temp_bytes: default the reported need; max_len:
    max_subject_len (default the longest subject).  plain: call sw_align_hits / sw_align_hits_pssm instead (max_hsps == 1)."""
    chars, offsets, lengths = O.make_db(subjects)
    n, qlen = len(lengths), case.qlen
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if caps is None:
        caps = np.repeat(qlen + lengths.astype(np.int64), max_hsps)
    caps = np.asarray(caps, dtype=np.int64)
    assert caps.shape == (n * max_hsps,)
    coff = np.zeros(n * max_hsps + 1, dtype=np.int64)
    coff[1:] = np.cumsum(caps)
    dch, doff, dlen, dcoff = dev(chars), dev(offsets.view(np.int64)), dev(lengths), dev(coff)
    dt = capi.align_result_dtype()
    dres = torch.full((max(n * max_hsps, 1) * dt.itemsize,), RESULT_FILL, dtype=torch.uint8, device="cuda")
    dcig = torch.from_numpy(np.full(int(coff[-1]) + 1, SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    dexp = dev(np.asarray(expected, dtype=np.int32)) if expected is not None else None
    if trace is None:
        trace = max([C.trace_bytes(qlen, int(L)) for L in lengths] or [0])
    if max_len is None:
        max_len = int(lengths.max()) if n else 0
    args = (n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), max_len, gop, gex, dres.data_ptr(), dcig.data_ptr(), dcoff.data_ptr())
    kw = dict(expected_scores=dexp.data_ptr() if dexp is not None else 0, trace_bytes=trace)
    if not plain:
        kw.update(max_hsps=max_hsps, min_score=min_score)
    if case.is_pssm:
        dp = dev(np.ascontiguousarray(case.pssm, dtype=np.int8).reshape(-1))
        dc = dev(np.ascontiguousarray(case.consensus, dtype=np.int8)) if case.consensus is not None else None
        f = capi.align_hits_pssm if plain else capi.align_hsps_pssm
        call = lambda **more: f(ctx, dp.data_ptr(), dc.data_ptr() if dc is not None else 0, qlen, *args, **kw, **more)
    else:
        ctx.set_matrix(case.table)
        dq = dev(np.ascontiguousarray(case.q, dtype=np.int8))
        f = capi.align_hits if plain else capi.align_hsps
        call = lambda **more: f(ctx, dq.data_ptr(), qlen, *args, **kw, **more)
    out = Call()
    out.need = call()
    temp = torch.empty(max(temp_bytes if temp_bytes is not None else out.need, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call(temp=temp.data_ptr(), temp_bytes=temp.numel())
    torch.cuda.synchronize()
    out.raw = dres.cpu().numpy().tobytes()
    out.res = np.frombuffer(out.raw, dtype=dt)[:n * max_hsps].copy()
    out.cigar = dcig.cpu().numpy().view(np.uint32).copy()
    out.coff = coff
    out.words = [out.cigar[int(coff[i]):int(coff[i]) + max(0, min(int(r["cigar_len"]), int(caps[i])))].copy()
                 for i, r in enumerate(out.res)]
    return out


def want_of(case, subjects, gop, gex, max_hsps, min_score, trace=None, caps=None, expected=None, max_len=None):
    """hsp_ref's slots of every subject, flat in the order of the records: [(fields, words)]"""
    want = []
    for i, s in enumerate(subjects):
        kw = {}
        if trace is not None:
            kw["trace_bytes"] = trace
        if caps is not None:
            kw["caps"] = np.asarray(caps[i * max_hsps:(i + 1) * max_hsps], dtype=np.int32)
        if expected is not None:
            kw["expected"] = int(expected[i])
        if max_len is not None:
            kw["max_subject_len"] = max_len
        want += HC.reference(case, s, gop, gex, max_hsps, min_score, **kw)
    return want


def check(call, want, where=()):
    """records field for field, CIGARs word for word, every record's cigar_offset its slot's, the unused words of the CIGAR
    buffer and its guard word untouched.  -> None, or what is wrong first"""
    bad = AB.compare(call.res, call.words, want, where)
    if bad:
        return bad.replace("pair", "slot")
    for k, (r, _) in enumerate(want):
        if r["status"] != H.BAD_LENGTH and int(call.res[k]["cigar_offset"]) != int(call.coff[k]):
            return "slot %d: cigar_offset %d, not %d %r" % (k, int(call.res[k]["cigar_offset"]), int(call.coff[k]), where)
    bad = AB.unused_words_untouched(call, want)
    return None if bad is None else "%s not untouched %r" % (bad, where)
