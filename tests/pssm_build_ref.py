"""ctypes access to tests/pssm_build_ref.c, the scalar reference of PSSM building (counts, weights, weighted counts, lambda,
conversion), and the inclusion rule in Python.  TEST INFRASTRUCTURE ONLY.

Compiled on demand into tests/host/_build/ (git-ignored), like pssm_align_ref."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pssm_build_ref.c")
BUILD = os.path.join(HERE, "host", "_build")
SO = os.path.join(BUILD, "libpssm_build_ref.so")

FIELDS = ["score", "status", "q_begin", "q_end", "s_begin", "s_end", "columns", "identities", "mismatches", "gap_opens",
          "gap_columns", "cigar_len"]
RECORD = np.dtype([(f, np.int32) for f in FIELDS] + [("cigar_offset", np.int64)])   # the layout of sw_align_result
OK, EMPTY, NO_TRACE = 0, 1, 2
OPS = {"I": 1, "D": 2, "=": 7, "X": 8}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            os.makedirs(BUILD, exist_ok=True)
            tmp = SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-shared", SRC, "-o", tmp, "-lm"])
            os.replace(tmp, SO)
        L = ctypes.CDLL(SO)
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.pbr_accumulate.restype = ctypes.c_int
        L.pbr_accumulate.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.pbr_lambda.restype = ctypes.c_double
        L.pbr_lambda.argtypes = [vp]
        L.pbr_convert.restype = ctypes.c_int
        L.pbr_convert.argtypes = [vp, vp, i32, vp, vp, ctypes.c_double, vp, vp, ctypes.POINTER(ctypes.c_double)]
        _lib = L
    return _lib


def _table(t21):
    t = np.ascontiguousarray(t21, dtype=np.int8).reshape(-1)
    assert t.size == 441
    return t


def accumulate(query, qlen, chars, offsets, lengths, results, cigar, include=None):
    """query: master codes or None; results: RECORD array (n); cigar: uint32 words the records' cigar_offset index.
    -> (counts (qlen, 20) uint32, weights (n + 1) uint64, wcounts (qlen, 20) uint64, used)"""
    n = len(results)
    q = np.ascontiguousarray(query, dtype=np.int8) if query is not None else None
    assert q is None or len(q) == qlen
    chars = np.ascontiguousarray(chars, dtype=np.int8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    res = np.ascontiguousarray(results, dtype=RECORD)
    cig = np.ascontiguousarray(cigar, dtype=np.uint32)
    inc = np.ascontiguousarray(include, dtype=np.uint8) if include is not None else None
    counts = np.zeros((qlen, 20), dtype=np.uint32)
    weights = np.zeros(n + 1, dtype=np.uint64)
    wcounts = np.zeros((qlen, 20), dtype=np.uint64)
    used = ctypes.c_int32()
    rc = lib().pbr_accumulate(q.ctypes.data if q is not None else None, qlen, n, chars.ctypes.data, offsets.ctypes.data,
                              lengths.ctypes.data, res.ctypes.data, cig.ctypes.data, inc.ctypes.data if inc is not None else None,
                              counts.ctypes.data, weights.ctypes.data, wcounts.ctypes.data, ctypes.byref(used))
    if rc != 0:
        raise MemoryError("pssm_build_ref failed")
    return counts, weights, wcounts, used.value


def lam(t21):
    return float(lib().pbr_lambda(_table(t21).ctypes.data))


def convert(t21, master, counts, wcounts, beta=10.0):
    """-> (pssm (qlen, 21) int8, raw (qlen, 20) float64, lambda); ValueError for beta <= 0 or a non-negative column-20 entry"""
    t = _table(t21)
    m = np.ascontiguousarray(master, dtype=np.int8)
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    w = np.ascontiguousarray(wcounts, dtype=np.uint64)
    qlen = len(m)
    assert c.size == qlen * 20 and w.size == qlen * 20
    pssm = np.zeros((qlen, 21), dtype=np.int8)
    raw = np.zeros((qlen, 20), dtype=np.float64)
    lam_ = ctypes.c_double()
    rc = lib().pbr_convert(t.ctypes.data, m.ctypes.data, qlen, c.ctypes.data, w.ctypes.data, float(beta), pssm.ctypes.data,
                           raw.ctypes.data, ctypes.byref(lam_))
    if rc != 0:
        raise ValueError("pssm_build_ref: beta must be positive" if rc == -1 else "pssm_build_ref: column 20 must be negative")
    return pssm, raw, lam_.value


def words(text):
    """"3=1X2I" -> CIGAR words (len << 4 | op)"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) << 4 | OPS[ch])
            num = ""
    return np.array(out, dtype=np.uint32)


def inclusion(results, scores, qlen, min_score):
    """The host rule, in its order: below min_score; no trace; a copy of the master; else in when it has an alignment.
    -> (include bytes, dict of the counts left out)"""
    inc = np.zeros(len(results), dtype=np.uint8)
    out = {"below_score": 0, "no_trace": 0, "copies": 0}
    for h, r in enumerate(results):
        if int(scores[h]) < min_score:
            out["below_score"] += 1
        elif int(r["status"]) == NO_TRACE:
            out["no_trace"] += 1
        elif (int(r["status"]) == OK and int(r["q_begin"]) == 0 and int(r["q_end"]) == qlen
              and int(r["identities"]) == qlen and int(r["columns"]) == qlen):
            out["copies"] += 1
        elif int(r["status"]) == OK and int(r["cigar_len"]) > 0:
            inc[h] = 1
    return inc, out


def random_alignments(rng, qlen, n, master=None):
    """n random subjects with random, self-consistent alignments against a query of qlen positions (no DP involved: the
    counts only depend on what the records say).  -> (chars, offsets, lengths, RECORD array, cigar words)"""
    subjects, recs, cig = [], [], []
    for _ in range(n):
        qb = int(rng.integers(0, qlen))
        qe = int(rng.integers(qb + 1, qlen + 1))
        sb = int(rng.integers(0, 7))
        ops, i = [], qb
        while i < qe:
            r = rng.random()
            if r < 0.08 and ops and i + 1 < qe:
                ops.append("I")
                i += 1
            elif r < 0.16 and ops:
                ops.append("D")
            else:
                ops.append("=" if rng.random() < 0.6 else "X")
                i += 1
        while ops[-1] == "D":   # (an alignment does not end in a gap)
            ops.pop()
        slen_al = sum(o != "I" for o in ops)
        s = rng.integers(0, 21, sb + slen_al + int(rng.integers(0, 5))).astype(np.int8)
        if master is not None:   # '=' columns carry the master's residue where it is a standard one
            i, j = qb, sb
            for o in ops:
                if o in "=X":
                    if o == "=" and master[i] < 20:
                        s[j] = master[i]
                    i += 1
                    j += 1
                elif o == "I":
                    i += 1
                else:
                    j += 1
        runs = []
        for o in ops:
            if runs and runs[-1][1] == o:
                runs[-1][0] += 1
            else:
                runs.append([1, o])
        rec = np.zeros((), dtype=RECORD)
        rec["score"], rec["status"] = 10, OK
        rec["q_begin"], rec["q_end"], rec["s_begin"], rec["s_end"] = qb, qe, sb, sb + slen_al
        rec["columns"] = len(ops)
        rec["cigar_len"] = len(runs)
        rec["cigar_offset"] = len(cig)
        cig += [k << 4 | OPS[o] for k, o in runs]
        subjects.append(s)
        recs.append(rec)
    lengths = np.array([len(s) for s in subjects], dtype=np.int32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum((lengths.astype(np.int64) + 3) // 4 * 4)
    chars = np.full(int(offsets[-1]), 20, dtype=np.int8)
    for k, s in enumerate(subjects):
        chars[int(offsets[k]):int(offsets[k]) + len(s)] = s
    return chars, offsets, lengths, np.array(recs, dtype=RECORD), np.array(cig, dtype=np.uint32)
