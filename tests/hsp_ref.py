"""ctypes access to tests/hsp_ref.c, the scalar full-matrix reference of sw_align_hsps / sw_align_hsps_pssm.
TEST INFRASTRUCTURE ONLY.

Compiled on demand into tests/host/_build/ (git-ignored), like align_ref."""
import ctypes
import os
import subprocess

import numpy as np

from align_ref import EMPTY, FIELDS, NO_TRACE, OK, OPS, SCORE_MISMATCH, cigar_string  # noqa: F401  (the same records)

BAD_LENGTH, NOT_COMPUTED = 4, 5

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hsp_ref.c")
BUILD = os.path.join(HERE, "host", "_build")
SO = os.path.join(BUILD, "libhsp_ref.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            os.makedirs(BUILD, exist_ok=True)
            tmp = SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-shared", SRC, "-o", tmp])
            os.replace(tmp, SO)
        L = ctypes.CDLL(SO)
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.hsr_align.restype = ctypes.c_int
        L.hsr_align.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, ctypes.c_int64, vp, vp, vp]
        _lib = L
    return _lib


def align(q, s, m=None, pssm=None, gop=-11, gex=-1, max_hsps=1, min_score=1, expected=None, trace_bytes=None, caps=None,
          max_subject_len=None):
    """Letters: q = query codes, m = (rows x 21) int8.  PSSM form: pssm = (qlen x 21) int8, q = consensus codes or None.
    s: dbdata subject codes.  caps: CIGAR slot sizes in words, one per alignment (default qlen + len(s) each).
    -> [(dict of FIELDS, CIGAR as a uint32 array)] of max_hsps slots"""
    s = np.ascontiguousarray(s, dtype=np.int8)
    assert (m is None) != (pssm is None)
    if m is not None:
        q = np.ascontiguousarray(q, dtype=np.int8)
        m = np.ascontiguousarray(m, dtype=np.int8).reshape(-1)
        qlen = len(q)
        assert m.size % 21 == 0 and (qlen == 0 or int(q.max()) < m.size // 21) and (len(s) == 0 or int(s.max()) <= 20)
    else:
        pssm = np.ascontiguousarray(pssm, dtype=np.int8)
        assert pssm.ndim == 2 and pssm.shape[1] == 21
        qlen = pssm.shape[0]
        assert len(s) == 0 or int(s.min()) >= 0
        if q is not None:
            q = np.ascontiguousarray(q, dtype=np.int8)
            assert q.shape == (qlen,)
    caps = np.full(max_hsps, qlen + len(s), dtype=np.int32) if caps is None else np.ascontiguousarray(caps, dtype=np.int32)
    assert caps.shape == (max_hsps,)
    out = np.zeros((max_hsps, len(FIELDS)), dtype=np.int32)
    cig = np.zeros(max(int(caps.sum()), 1), dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = lib().hsr_align(ptr(q), ptr(m), ptr(pssm), qlen, s.ctypes.data, len(s), gop, gex, max_hsps, min_score,
                         len(s) if max_subject_len is None else max_subject_len, -1 if expected is None else expected,
                         -1 if trace_bytes is None else trace_bytes, caps.ctypes.data, out.ctypes.data, cig.ctypes.data)
    if rc != 0:
        raise MemoryError("hsp_ref failed")
    slots, off = [], 0
    for k in range(max_hsps):
        r = dict(zip(FIELDS, (int(x) for x in out[k])))
        slots.append((r, cig[off:off + r["cigar_len"]].copy()))
        off += int(caps[k])
    return slots


def pairs(r, words):
    """the aligned pairs (query row, subject column) of one alignment"""
    i, j, out = r["q_begin"], r["s_begin"], []
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        for _ in range(n):
            if op in (7, 8):
                out.append((i, j))
                i += 1
                j += 1
            elif op == 1:
                i += 1
            else:
                j += 1
    assert i == r["q_end"] and j == r["s_end"], (i, j, r)
    return out
