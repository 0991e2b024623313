"""ctypes access to tests/align_ref.c, the scalar full-matrix reference of sw_align_hits.  TEST INFRASTRUCTURE ONLY.

Compiled on demand into tests/host/_build/ (git-ignored), like oracle_lib.build_oracle."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "align_ref.c")
BUILD = os.path.join(HERE, "host", "_build")
SO = os.path.join(BUILD, "libalign_ref.so")

FIELDS = ["score", "status", "q_begin", "q_end", "s_begin", "s_end", "columns", "identities", "mismatches", "gap_opens",
          "gap_columns", "cigar_len"]
OK, EMPTY, NO_TRACE, SCORE_MISMATCH = 0, 1, 2, 3
OPS = {1: "I", 2: "D", 7: "=", 8: "X"}

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
        L.alr_align.restype = ctypes.c_int
        L.alr_align.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_int32]
        _lib = L
    return _lib


def align(q, s, m, gop=-11, gex=-1, coords_only=False, cigar_cap=None):
    """q: query codes, s: dbdata subject codes, m: (rows x 21) int8 (one row per query code).
    -> (dict of FIELDS, CIGAR as a uint32 array of len << 4 | op words)"""
    q = np.ascontiguousarray(q, dtype=np.int8)
    s = np.ascontiguousarray(s, dtype=np.int8)
    m = np.ascontiguousarray(m, dtype=np.int8).reshape(-1)
    assert m.size % 21 == 0 and (len(q) == 0 or int(q.max()) < m.size // 21) and (len(s) == 0 or int(s.max()) <= 20)
    cap = len(q) + len(s) if cigar_cap is None else cigar_cap
    out = np.zeros(len(FIELDS), dtype=np.int32)
    cig = np.zeros(max(cap, 1), dtype=np.uint32)
    rc = lib().alr_align(q.ctypes.data, len(q), s.ctypes.data, len(s), m.ctypes.data, gop, gex, int(coords_only),
                         out.ctypes.data, cig.ctypes.data, cap)
    if rc != 0:
        raise MemoryError("align_ref failed")
    r = dict(zip(FIELDS, (int(x) for x in out)))
    return r, cig[:r["cigar_len"]].copy()


def cigar_string(words):
    return "".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in words)


def rescore(q, s, m, gop, gex, r, words):
    """score of the alignment the CIGAR describes (q_begin / s_begin of r), with the same gap model"""
    m = np.asarray(m, dtype=np.int8).reshape(-1, 21)
    i, j, total = r["q_begin"], r["s_begin"], 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op in (7, 8):
            for _ in range(n):
                total += int(m[q[i], s[j]])
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


def column_scores(q, s, m, r, words):
    """substitution score of the first and the last column (None when that column is a gap)"""
    m = np.asarray(m, dtype=np.int8).reshape(-1, 21)
    first = int(words[0]) & 15
    last = int(words[-1]) & 15
    f = int(m[q[r["q_begin"]], s[r["s_begin"]]]) if first in (7, 8) else None
    l_ = int(m[q[r["q_end"] - 1], s[r["s_end"] - 1]]) if last in (7, 8) else None
    return f, l_
