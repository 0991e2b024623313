"""Search statistics: Z-scores and E-values by the regression of FASTA / SSEARCH on a scan's own scores.

Thin wrappers over the host library (include/cudasw4_amd_driver.h); no GPU needed.  The table they work on is what
`Driver.set_statistics(True)` makes a scan leave: hist[length bin][min(score, 255)] (uint32, 64 x 256) and the summed
true lengths per length bin, sumlen (uint64, 64).  Tables add: sum those of several shards or ranks, then fit.
"""
import ctypes

import numpy as np

from . import driver as _driver

OK, NO_FIT = _driver.STATS_OK, _driver.STATS_NO_FIT
LBINS, SBINS = _driver.STATS_LBINS, _driver.STATS_SBINS


def length_bin(length):
    """Half-octave length bin of a true subject length (swdrv_length_bin)."""
    return int(_driver._stats_fns()[4](int(length)))


def from_histogram(hist, sumlen):
    """The fit (swdrv_stats_from_histogram) -> dict: a, b1, sd, n_included, N, rounds, status (OK or NO_FIT)."""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    s = np.ascontiguousarray(sumlen, dtype=np.uint64)
    if h.size != LBINS * SBINS or s.size != LBINS:
        raise ValueError("hist must hold %d x %d counts and sumlen %d sums" % (LBINS, SBINS, LBINS))
    out = _driver._Stats()
    _driver._check(_driver._stats_fns()[2](h.ctypes.data, s.ctypes.data, ctypes.byref(out)))
    return _driver._stats_dict(out)


def evalues(stats, scores, lengths):
    """(Z-scores, E-values) of hits of the given scores and true subject lengths under a fit (swdrv_evalues): float64 arrays;
    under NO_FIT all 0 and all -1."""
    sc = np.ascontiguousarray(scores, dtype=np.int32)
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    if sc.shape != ln.shape or sc.ndim != 1:
        raise ValueError("scores and lengths must be 1-D arrays of one size")
    z = np.zeros(len(sc), dtype=np.float64)
    e = np.zeros(len(sc), dtype=np.float64)
    st = _driver._stats_struct(stats)
    _driver._check(_driver._stats_fns()[3](ctypes.byref(st), sc.ctypes.data, ln.ctypes.data, len(sc), z.ctypes.data, e.ctypes.data))
    return z, e


# ---- statistics calibrated on shuffled subjects: the rules, without a GPU ----

def shuffle_sample(n, max_subjects=_driver.SHUFFLE_DEFAULT_SUBJECTS):
    """The sampled subject ids of a DB of n sequences (swdrv_shuffle_sample): ((2 j + 1) n) / (2 M) for j = 0 .. M - 1 with
    M = min(n, max_subjects) -> int64 array, ascending and distinct."""
    m = min(int(n), int(max_subjects))
    out = np.zeros(max(m, 0), dtype=np.int64)
    got = _driver._shuffle_fns()[3](int(n), int(max_subjects), out.ctypes.data)
    if got < 0:
        _driver._check(got)
    return out[:got]


def shuffle_replicas(subjects, shuffles=None):
    """Replicas of a sample of `subjects` (swdrv_shuffle_replicas): `shuffles` (1 .. 64) when given, else
    ceil(2000 / subjects) clamped to [1, 64]."""
    if shuffles is not None and not 1 <= int(shuffles) <= _driver.SHUFFLE_MAX_REPLICAS:
        raise ValueError("shuffles must lie in [1, %d]" % _driver.SHUFFLE_MAX_REPLICAS)
    got = _driver._shuffle_fns()[4](int(subjects), int(shuffles or 0))
    if got < 0:
        _driver._check(got)
    return int(got)


def shuffle_permutation(length, seed, subject_id, replica=0):
    """pi of a subject of true length `length` under (seed, subject_id, replica) (swdrv_shuffle_permutation): residue i of
    the shuffled subject is residue pi[i] of the original -> int32 array."""
    out = np.zeros(max(int(length), 0), dtype=np.int32)
    _driver._check(_driver._shuffle_fns()[5](int(length), int(seed) & 0xFFFFFFFF, int(subject_id), int(replica), out.ctypes.data))
    return out
