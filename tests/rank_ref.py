"""Independent numpy restatement of the ranking by E-value.  Never calls the library: the tests compare the
kernels, the host library, the driver and the command line against this file."""
import numpy as np

import stats_ref as R

KEY_NONE = np.float32(-3.0e38)


def zscores(stats, scores, lengths):
    """double z of every subject (stats_ref.evalues' z); the fit must have status OK"""
    assert stats["status"] == R.OK and stats["sd"] > 0
    return R.evalues(stats, scores, lengths)[0]


def keys(stats, scores, lengths):
    """float32 keys: (float) z for score >= 0, KEY_NONE for the others"""
    scores = np.asarray(scores, dtype=np.float64)
    z = zscores(stats, np.maximum(scores, 0), lengths)
    return np.where(scores >= 0, z.astype(np.float32), KEY_NONE).astype(np.float32)


def tol(z):
    """two subjects may change places only when their double z differ by less than this"""
    return 1e-6 * np.maximum(1.0, np.abs(z))


def z_min(N, X):
    """the Z-score at which E = N P(z) equals X; X >= N: -inf"""
    if X >= N:
        return -np.inf
    return float(-(np.log(-np.log1p(-X / N)) + R.EULER_GAMMA) * np.sqrt(6.0) / np.pi)


def count(stats, scores, lengths, X):
    """subjects with score >= 0 and z >= z_min(X), compared in double precision"""
    scores = np.asarray(scores)
    z = zscores(stats, scores, lengths)
    return int(((scores >= 0) & (z >= z_min(stats["N"], X))).sum())


def min_distance_to(z, value):
    """smallest |z - value| over tol(z): below 1 a count may differ by the device's log"""
    return float((np.abs(z - value) / tol(z)).min()) if np.isfinite(value) else np.inf


def order(z, ids):
    """indices by z descending, ties by ascending id"""
    return np.lexsort((np.asarray(ids), -np.asarray(z, dtype=np.float64)))


def ranked(stats, scores, lengths, k):
    """-> (ids, z of them): the k subjects of largest double z, ties by ascending id; ids are positions in the arrays.
    Under NO_FIT: the raw-score list."""
    scores = np.asarray(scores)
    if stats["status"] != R.OK:
        idx = np.lexsort((np.arange(len(scores)), -scores.astype(np.int64)))[:k]
        return idx, np.zeros(len(idx))
    z = zscores(stats, scores, lengths)
    idx = order(z, np.arange(len(scores)))[:k]
    return idx, z[idx]


def boundary_gap(stats, scores, lengths, k):
    """smallest difference between DISTINCT z on the two sides of the k-th place, over tol: at 1 or above, the set of the
    list is exact whatever the float keys do"""
    z = np.sort(zscores(stats, scores, lengths))[::-1]
    inside, outside = z[:k], z[k:]
    if not len(inside) or not len(outside):
        return np.inf
    # of all pairs (inside, outside) with different z the closest is one of two: the largest outside value with the smallest
    # inside value above it, or the smallest inside value with the largest outside value below it
    lo, hi_out = inside[-1], outside[0]
    gaps = [np.inf]
    above, below = inside[inside > hi_out], outside[outside < lo]
    if len(above):
        gaps.append((above.min() - hi_out) / tol(hi_out))
    if len(below):
        gaps.append((lo - below.max()) / tol(lo))
    return float(min(gaps))


def same_up_to_close_swaps(got_ids, want_ids, z_of):
    """got is want, up to exchanges of subjects whose double z differ by less than tol: equal as sets, and at every place
    the two lists' z agree within tol"""
    got_ids, want_ids = list(map(int, got_ids)), list(map(int, want_ids))
    if sorted(got_ids) != sorted(want_ids):
        return False
    zg = np.array([z_of[i] for i in got_ids])
    zw = np.array([z_of[i] for i in want_ids])
    return bool((np.abs(zg - zw) < tol(zw)).all() or got_ids == want_ids)
