"""ctypes access to tests/pssm_align_ref.c, the scalar full-matrix reference of sw_align_hits_pssm.  TEST INFRASTRUCTURE ONLY.

Compiled on demand into tests/host/_build/ (git-ignored), like align_ref."""
import ctypes
import os
import subprocess

import numpy as np

from align_ref import EMPTY, FIELDS, NO_TRACE, OK, OPS, SCORE_MISMATCH, cigar_string  # noqa: F401  (the same records)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pssm_align_ref.c")
BUILD = os.path.join(HERE, "host", "_build")
SO = os.path.join(BUILD, "libpssm_align_ref.so")

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
        L.par_align.restype = ctypes.c_int
        L.par_align.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_int32]
        _lib = L
    return _lib


def _pssm(p):
    p = np.ascontiguousarray(p, dtype=np.int8)
    assert p.ndim == 2 and p.shape[1] == 21 and p.shape[0] >= 1, p.shape
    return p


def align(pssm, s, consensus=None, gop=-11, gex=-1, coords_only=False, cigar_cap=None):
    """pssm: (qlen, 21) int8; s: dbdata subject codes (above 20: scored as 20); consensus: one code per position, or None
    (the lowest code < 20 with the largest score of the row).
    -> (dict of FIELDS, CIGAR as a uint32 array of len << 4 | op words)"""
    p = _pssm(pssm)
    raw = np.ascontiguousarray(s, dtype=np.int8)
    assert len(raw) == 0 or int(raw.min()) >= 0
    s = np.minimum(raw, 20).astype(np.int8)   # (codes of 20 and above are identical to nothing either way)
    cons = None
    if consensus is not None:
        cons = np.ascontiguousarray(consensus, dtype=np.int8)
        assert cons.shape == (p.shape[0],)
    cap = p.shape[0] + len(s) if cigar_cap is None else cigar_cap
    out = np.zeros(len(FIELDS), dtype=np.int32)
    cig = np.zeros(max(cap, 1), dtype=np.uint32)
    rc = lib().par_align(p.ctypes.data, cons.ctypes.data if cons is not None else None, p.shape[0], s.ctypes.data, len(s),
                         gop, gex, int(coords_only), out.ctypes.data, cig.ctypes.data, cap)
    if rc != 0:
        raise MemoryError("pssm_align_ref failed")
    r = dict(zip(FIELDS, (int(x) for x in out)))
    return r, cig[:r["cigar_len"]].copy()


def rescore(pssm, s, gop, gex, r, words):
    """score of the alignment the CIGAR describes (q_begin / s_begin of r), with the same gap model"""
    p = _pssm(pssm)
    i, j, total = r["q_begin"], r["s_begin"], 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op in (7, 8):
            for _ in range(n):
                total += int(p[i, min(int(s[j]), 20)])
                i += 1
                j += 1
        else:
            total += gop + (n - 1) * max(gop, gex)   # (gop > gex: the recurrence opens anew in every column of the run)
            if op == 1:
                i += n
            else:
                j += n
    assert i == r["q_end"] and j == r["s_end"], (i, j, r)
    return total


def column_scores(pssm, s, r, words):
    """substitution score of the first and the last column (None when that column is a gap)"""
    p = _pssm(pssm)
    first = int(words[0]) & 15
    last = int(words[-1]) & 15
    f = int(p[r["q_begin"], min(int(s[r["s_begin"]]), 20)]) if first in (7, 8) else None
    l_ = int(p[r["q_end"] - 1, min(int(s[r["s_end"] - 1]), 20)]) if last in (7, 8) else None
    return f, l_


def recount(pssm, s, consensus, r, words):
    """(identities, mismatches, the CIGAR with '=' / 'X' decided anew) of an alignment's pairs against `consensus` codes"""
    i, j, ids, mis = r["q_begin"], r["s_begin"], 0, 0
    ops = []
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        for _ in range(n):
            if op in (7, 8):
                same = int(s[j]) < 20 and int(s[j]) == int(consensus[i])
                ids += same
                mis += not same
                ops.append(7 if same else 8)
                i += 1
                j += 1
            else:
                ops.append(op)
                i += op == 1
                j += op == 2
    runs = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return ids, mis, [n << 4 | op for n, op in runs]
