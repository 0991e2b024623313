"""The numpy restatement of the subject-masking rule (include/cudasw4_amd_mask.h): what the device kernels
(sw_mask_subjects) and the host library (swdrv_mask_subject) are held against, bit for bit.  Integers only."""
import math

import numpy as np

# U[n] = round(1024 log2 n), n = 1 .. 32; U[0] = 0 — literals, as in the header
U = [0, 0, 1024, 1623, 2048, 2378, 2647, 2875, 3072, 3246, 3402, 3542, 3671, 3789, 3899, 4001, 4096, 4186, 4270, 4350, 4426,
     4498, 4566, 4632, 4695, 4755, 4813, 4869, 4923, 4975, 5025, 5073, 5120]
MIN_WINDOW, MAX_WINDOW = 4, 32
MASK_CODE = 20
DEFAULT_WINDOW, DEFAULT_TRIGGER_BITS, DEFAULT_EXTEND_BITS = 12, 1.9, 2.2


def threshold(window, bits):
    return max(1, int(math.ceil(1024.0 * window * (math.log2(window) - bits))))


DEFAULTS = (DEFAULT_WINDOW, threshold(DEFAULT_WINDOW, DEFAULT_TRIGGER_BITS), threshold(DEFAULT_WINDOW, DEFAULT_EXTEND_BITS))


def window_sums(codes, window):
    """S_i for every window start i = 0 .. L - W (empty for L < W)"""
    c = np.asarray(codes).astype(np.int8).view(np.uint8)
    L = len(c)
    if L < window:
        return np.zeros(0, dtype=np.int64)
    nU = np.arange(MAX_WINDOW + 1, dtype=np.int64) * np.asarray(U, dtype=np.int64)
    S = np.zeros(L - window + 1, dtype=np.int64)
    for a in range(20):
        cs = np.concatenate([[0], np.cumsum(c == a)])
        S += nU[cs[window:] - cs[:-window]]
    return S


def segments(codes, window, trigger_sum, extend_sum):
    """[(first, last + 1)] of the masked segments of one subject, ascending"""
    assert MIN_WINDOW <= window <= MAX_WINDOW and 1 <= extend_sum <= trigger_sum
    S = window_sums(codes, window)
    if len(S) == 0:
        return []
    lo = S >= extend_sum
    trig = S >= trigger_sum
    edges = np.diff(np.concatenate([[0], lo.astype(np.int8), [0]]))
    starts, ends = np.nonzero(edges == 1)[0], np.nonzero(edges == -1)[0]   # runs [a, b + 1)
    tcs = np.concatenate([[0], np.cumsum(trig)])
    return [(int(a), int(b) - 1 + window) for a, b in zip(starts, ends) if tcs[b] > tcs[a]]


def mask_subject(codes, window=DEFAULTS[0], trigger_sum=DEFAULTS[1], extend_sum=DEFAULTS[2], with_count=False):
    out = np.array(codes, dtype=np.int8, copy=True)
    covered = np.zeros(len(out), dtype=bool)   # (the segments of two runs less than W apart overlap: a position counts once)
    for a, b in segments(out, window, trigger_sum, extend_sum):
        covered[a:b] = True
    out[covered] = MASK_CODE
    return (out, int(covered.sum())) if with_count else out


def true_lengths(offsets, lengths):
    padded = np.diff(np.asarray(offsets).astype(np.int64))
    return np.minimum(np.maximum(np.asarray(lengths).astype(np.int64), 0), padded)


def mask_block(chars, offsets, lengths, window=DEFAULTS[0], trigger_sum=DEFAULTS[1], extend_sum=DEFAULTS[2], first=0, n=None):
    """The subjects first .. first + n - 1 of a block in dbdata layout -> (the bytes of that range with the masked positions
    set to code 20 and everything else as it is, positions covered, subjects with a segment)"""
    n = len(lengths) - first if n is None else n
    base = int(offsets[first])
    out = np.array(chars[base:int(offsets[first + n])], dtype=np.int8, copy=True)
    tl = true_lengths(offsets, lengths)
    positions = subjects = 0
    for i in range(first, first + n):
        o = int(offsets[i]) - base
        masked, covered = mask_subject(out[o:o + int(tl[i])], window, trigger_sum, extend_sum, with_count=True)
        out[o:o + int(tl[i])] = masked
        positions += covered
        subjects += covered > 0
    return out, positions, subjects
