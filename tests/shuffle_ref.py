"""Independent numpy restatement of the shuffled-subject calibration: the key, the permutation, the block
shuffle, the sample and replica rules, and a calibration that scans the shuffled block with the CPU oracle.  Never calls
the library: the tests compare the kernel, the host library and the command line against this file."""
import numpy as np

import stats_ref as R

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9
OTHER = 20
DEFAULT_MAX_SUBJECTS = 10000


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def key(seed, subject_id, replica):
    subject_id = int(subject_id) & 0xFFFFFFFFFFFFFFFF
    return mix32(mix32(mix32(mix32(int(seed)) ^ (subject_id & M32)) ^ (subject_id >> 32)) ^ (int(replica) & M32))


def _mix32_np(x):
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def half_bits(length):
    return max(1, ((int(length) - 1).bit_length() + 1) // 2)


def _pass(c, k, h):
    mask = np.uint64((1 << h) - 1)
    l, r = c >> np.uint64(h), c & mask
    for rd in range(4):
        f = _mix32_np(r ^ np.uint64(k) ^ np.uint64((rd * GOLDEN) & M32)) & mask
        l, r = r, l ^ f
    return (l << np.uint64(h)) | r


def permutation(length, seed, subject_id, replica, with_passes=False):
    """pi of a subject of true length `length`: out[i] = in[pi[i]] -> int64 array (and the largest number of passes)."""
    length = int(length)
    if length <= 1:
        p = np.arange(max(length, 0), dtype=np.int64)
        return (p, 0) if with_passes else p
    k, h = key(seed, subject_id, replica), half_bits(length)
    c = _pass(np.arange(length, dtype=np.uint64), k, h)
    passes = 1
    while True:
        out = np.nonzero(c >= np.uint64(length))[0]
        if len(out) == 0:
            break
        c[out] = _pass(c[out], k, h)
        passes += 1
    p = c.astype(np.int64)
    return (p, passes) if with_passes else p


def shuffle_block(chars, offsets, lengths, seed, keys=None, first_replica=0, replicas=1, first=0, n=None):
    """Replicas [first_replica, first_replica + replicas) of subjects [first, first + n) -> int8 [replicas][block bytes]:
    the layout of the input (offsets relative to offsets[first]), every padding byte code 20.  keys: the subjects' ids
    (None: the position within the range)."""
    chars = np.asarray(chars, dtype=np.int8)
    off = np.asarray(offsets).astype(np.int64)
    n = len(lengths) - first if n is None else n
    base = int(off[first])
    out = np.full((replicas, int(off[first + n]) - base), OTHER, dtype=np.int8)
    for j in range(n):
        i = first + j
        length, b = int(lengths[i]), int(off[i])
        sid = j if keys is None else int(keys[j])
        for r in range(replicas):
            out[r, b - base:b - base + max(length, 0)] = chars[b + permutation(length, seed, sid, first_replica + r)]
    return out


def sample_ids(n, max_subjects=DEFAULT_MAX_SUBJECTS):
    m = min(int(n), int(max_subjects))
    return np.array([((2 * j + 1) * int(n)) // (2 * m) for j in range(m)], dtype=np.int64)


def replicas_for(m, shuffles=None):
    if shuffles is not None:
        return int(shuffles)
    return min(64, max(1, -(-2000 // max(int(m), 1))))


def gather(chars, offsets, lengths, ids):
    """the subjects `ids` as a block in dbdata layout"""
    off = np.asarray(offsets).astype(np.int64)
    ls = np.asarray(lengths, dtype=np.int32)[ids]
    padded = (ls.astype(np.int64) + 3) // 4 * 4
    o = np.zeros(len(ids) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(padded)
    c = np.full(int(o[-1]), OTHER, dtype=np.int8)
    for j, i in enumerate(ids):
        c[int(o[j]):int(o[j]) + int(ls[j])] = chars[int(off[i]):int(off[i]) + int(ls[j])]
    return c, o, ls


def calibrate(scan_fn, chars, offsets, lengths, seed, max_subjects=DEFAULT_MAX_SUBJECTS, shuffles=None):
    """scan_fn(chars, offsets, lengths) -> scores.  -> (hist, sumlen, fit, M, R): the table of the M x R shuffled sample
    and its fit (N is the shuffled table's: the caller takes N from the real scan)."""
    ids = sample_ids(len(lengths), max_subjects)
    c, o, ls = gather(chars, offsets, lengths, ids)
    reps = replicas_for(len(ids), shuffles)
    hist = np.zeros((R.LBINS, R.SBINS), dtype=np.uint32)
    sumlen = np.zeros(R.LBINS, dtype=np.uint64)
    blocks = shuffle_block(c, o, ls, seed, keys=ids, replicas=reps)
    for r in range(reps):
        h, s, skipped = R.histogram(np.asarray(scan_fn(blocks[r], o, ls)).astype(np.int64), ls)
        assert skipped == 0
        hist += h
        sumlen += s
    return hist, sumlen, R.fit(hist, sumlen), len(ids), reps


def calibrated(fit, n_scan):
    """the calibrated statistics of a scan: the shuffled fit with N from the real scan's table"""
    out = dict(fit)
    out["N"] = int(n_scan)
    return out
