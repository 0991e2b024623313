"""ctypes wrapper of tests/pssm_ref.c (compiled on demand into tests/host/_build/): the scalar reference of profile search."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pssm_ref.c")
BUILD = os.path.join(HERE, "host", "_build")
SO = os.path.join(BUILD, "libpssm_ref.so")

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
        L.pr_score.restype = i32
        L.pr_score.argtypes = [vp, i32, vp, i32, ctypes.c_int, ctypes.c_int]
        L.pr_scan.restype = None
        L.pr_scan.argtypes = [vp, i32, vp, vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, vp]
        _lib = L
    return _lib


def _pssm(p):
    p = np.ascontiguousarray(p, dtype=np.int8)
    assert p.ndim == 2 and p.shape[1] == 21, p.shape
    return p


def score(pssm, subject, gop=-11, gex=-1) -> int:
    p = _pssm(pssm)
    s = np.ascontiguousarray(subject, dtype=np.int8)
    return int(lib().pr_score(p.ctypes.data, p.shape[0], s.ctypes.data, len(s), gop, gex))


def scan(pssm, chars, offsets, lengths, gop=-11, gex=-1) -> np.ndarray:
    p = _pssm(pssm)
    chars = np.ascontiguousarray(chars, dtype=np.int8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    out = np.empty(len(lengths), dtype=np.int32)
    lib().pr_scan(p.ctypes.data, p.shape[0], chars.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(lengths), gop, gex,
                  out.ctypes.data)
    return out
