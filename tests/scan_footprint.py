"""The arena and the case DBs of the scan-launch footprint tests (test_gpu_scan_footprint.py, test_scan_footprint_cpu.py).

The arena is ONE uint8 array filled with a canary byte.  Every buffer a launch may write is a slice of it, between guard
zones that are at least as large as anything the launch could ask for (the caller states the sizes; guards_hold checks the
rule), so a kernel that writes too far changes a canary inside the same allocation: a failed assertion, never a fault.  The
class works on a numpy array (the CPU test) and on a torch device tensor alike: it only slices, assigns and compares.

The case DBs are built here, without a device, so that the CPU test can check that they are what the GPU test takes them
for: batches, the places of the short and the empty subjects, the planted copy, the subjects beyond an under-reported bound."""
import numpy as np

import oracle_lib as O

CANARIES = (0xA5, 0x3C)   # two, on different cases: a kernel that stores the canary's own value cannot hide behind both
SENTINEL = -7             # scores (as float), ids and list entries nobody may write
PART16, PART64 = 33, 34   # a partition of 16-lane groups; the long partition (wave-wide groups for a few subjects)
ALIGN = 256


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class Arena:
    """specs: (name, bytes, guard) in the order of the layout; `guard` bytes of canary lie in front of and behind the buffer
    at least (neighbours share the larger of their two wishes).  Every buffer starts at a multiple of 256 bytes; what
    follows a buffer's last byte directly is canary."""

    def __init__(self, specs, canary, alloc):
        self.canary = int(canary)
        self.names = [name for name, _, _ in specs]
        self.off, self.size = {}, {}
        end, wish = 0, 0
        for name, nbytes, guard in specs:
            start = -(-(end + max(wish, guard)) // ALIGN) * ALIGN
            self.off[name], self.size[name] = start, int(nbytes)
            end, wish = start + int(nbytes), guard
        self.total = end + wish
        self.buf = alloc(self.total)
        self.fill()

    def fill(self):
        self.buf[:] = self.canary

    def slice(self, name, nbytes=None):
        o = self.off[name]
        return self.buf[o:o + (self.size[name] if nbytes is None else nbytes)]

    def guard_sizes(self, name):
        """(bytes of canary in front of the buffer, bytes behind it)"""
        i = self.names.index(name)
        before = self.off[name] - (self.off[self.names[i - 1]] + self.size[self.names[i - 1]] if i else 0)
        after = (self.off[self.names[i + 1]] if i + 1 < len(self.names) else self.total) - (self.off[name] + self.size[name])
        return before, after

    def guards_hold(self, wishes):
        """wishes: name -> bytes every guard of that buffer must have at least"""
        return all(min(self.guard_sizes(name)) >= w for name, w in wishes.items())

    def check(self, used=None):
        """-> one line per guard zone that no longer holds the canary (empty: all intact).  used: name -> the bytes of that
        buffer the launch was offered; the guard then begins right behind them.  Offsets are relative to the END of the
        buffer in front of the zone (0 = the first byte behind it) and, negative, to the START of the buffer behind it."""
        used = used or {}
        out = []
        start, prev = 0, None
        for name in self.names + [None]:
            stop = self.off[name] if name is not None else self.total
            zone = self.buf[start:stop]
            if stop > start and bool((zone != self.canary).any()):
                idx = np.flatnonzero(_host(zone != self.canary))
                first, last = int(idx[0]), int(idx[-1])
                out.append("%d bytes changed between %s and %s: first %d, last %d behind the end of %s (%d .. %d before the start of %s)"
                           % (len(idx), prev or "the arena's start", name or "the arena's end", first, last, prev or "nothing",
                              first - (stop - start), last - (stop - start), name or "nothing"))
            if name is not None:
                start, prev = self.off[name] + min(self.size[name], used.get(name, self.size[name])), name
        return out

    def high_water(self, name):
        """one past the last byte of the buffer that is not the canary (0: untouched)"""
        idx = np.flatnonzero(_host(self.slice(name) != self.canary))
        return int(idx[-1]) + 1 if len(idx) else 0


def numpy_alloc(nbytes):
    return np.empty(nbytes, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------- scratch sizes
def region_bytes(columns, lanes=16):
    """scratch of one workgroup for walks of that many columns (sw_api.hip: border_capacity, border_bytes_per_wg): per group
    blocks of 2 * lanes positions, 8 bytes each, and on 16-lane groups 4 bytes of address stream per position"""
    steps = (columns + lanes - 1 + 3) // 4 * 4
    lcap = (steps + 15) // 16 * 16 + 16
    blocks = (lcap + 2 * lanes - 1) // (2 * lanes) + 3
    return (256 // lanes) * blocks * 2 * lanes * (12 if lanes == 16 else 8)


CHAIN_MAXIMA_BYTES = 16 * 7 * 16 * 4   # per workgroup: 16 groups x (kChainMax - 1) pairs x 16 lanes


def chain_bytes(maxlen, c):
    """... for chains of c pairs: the virtual subject (every pair but the last in whole quads, four separator columns each)
    and the per-pair maxima"""
    if c == 1:
        return region_bytes(maxlen)
    pair = max(12, (maxlen + 3) // 4 * 4)
    return region_bytes((c - 1) * (pair + 4) + maxlen) + CHAIN_MAXIMA_BYTES


# ------------------------------------------------------------------------------------------------------------------ cases
def query(qlen):
    return np.random.default_rng(7000 + qlen).integers(0, 20, qlen).astype(np.int8)


def mutated(rng, seg, every):
    s = np.array(seg, dtype=np.int8)
    s[::every] = rng.integers(0, 20, len(s[::every]))
    return s


def index(batch, group, half):
    return 32 * batch + 2 * group + half


class Case:
    """A DB of N subjects of which a launch scans [first_pos, first_pos + n); the letters of the range are the last ones of
    `chars` (the subjects in front of the range first, then those behind it, then the range: offsets[i] - offsets[0] is
    where subject i starts, as the header asks, and nothing else).  No slack behind the last letter word."""

    def __init__(self, name, seqs, first_pos, n, part, bound=None):
        self.name, self.seqs, self.first_pos, self.n, self.part, self.bound = name, seqs, first_pos, n, part, bound
        self.N = len(seqs)
        assert 0 < first_pos and first_pos + n < self.N
        order = list(range(first_pos)) + list(range(first_pos + n, self.N)) + list(range(first_pos, first_pos + n))
        self.lengths = np.array([len(s) for s in seqs], dtype=np.int32)
        padded = (self.lengths.astype(np.int64) + 3) // 4 * 4
        self.offsets = np.zeros(self.N + 1, dtype=np.uint64)
        at = 0
        for i in order:
            self.offsets[i] = at
            at += int(padded[i])
        self.offsets[self.N] = at
        self.chars = np.full(at, 20, dtype=np.int8)
        for i, s in enumerate(seqs):
            self.chars[int(self.offsets[i]):int(self.offsets[i]) + len(s)] = s
        self.maxlen = int(self.lengths[first_pos:first_pos + n].max())
        self._expect = {}

    @property
    def range(self):
        return slice(self.first_pos, self.first_pos + self.n)

    def expect(self, q, gaps=(-11, -1), bound=None):
        """oracle scores of all N subjects, each cut at `bound` rounded up to a whole letter word where it is longer"""
        key = (q.tobytes(), gaps, bound)
        if key not in self._expect:
            cut = None if bound is None else (bound + 3) // 4 * 4
            chars, offsets, lengths = O.make_db([s[:cut] for s in self.seqs])
            self._expect[key] = O.scan(q, chars, offsets, lengths, gop=gaps[0], gex=gaps[1], simd=True)
        return self._expect[key]


def _tails(rng, q, seqs, bound):
    """a piece of the query across or behind `bound` in every subject that is clearly longer: cutting it there changes its score"""
    for i, s in enumerate(seqs):
        if len(s) > bound + 24:
            n = int(rng.integers(40, 61))
            at_q = int(rng.integers(0, len(q) - n + 1))
            at = int(rng.integers(min(bound - n // 2, len(s) - n), len(s) - n + 1))
            s[at:at + n] = mutated(rng, q[at_q:at_q + n], 6)


HEAD, TAIL = 5, 3   # subjects in front of and behind the scanned range


def _wrap(rng, seqs):
    head = [rng.integers(0, 20, int(l)).astype(np.int8) for l in rng.integers(50, 90, HEAD)]
    tail = [rng.integers(0, 20, int(l)).astype(np.int8) for l in rng.integers(50, 90, TAIL)]
    return head + seqs + tail


RAGGED_N, RAGGED_BOUND = 339, 400
PLANTED = index(6, 5, 0)                                # the near copy of the query's first 590 residues
SHORT_PAIRS = {(9, 3): (0, 3), (8, 3): (1, 2), (9, 2): (2, 0), (8, 1): (3, 1)}   # (batch, group) -> lengths of its two subjects
EMPTY_PAIRS = [(9, g) for g in range(8, 12)]           # a whole wave of empty pairs in the middle of the first chain of C = 4
_cases = {}


def ragged(qlen, planted=True, last_mult4=False):
    """case (a): 339 subjects of 330 .. 600 residues in the range — eleven batches, the last one of nineteen subjects (nine
    pairs, one single subject, six empty groups).  Batch B is handed out as number 10 - B: batches 10, 9, 8, 7 are the first
    chain of C = 4.  Lengths 0 .. 3 and empty pairs in batches 9 and 8, one near copy of the query's first 590 residues
    beyond the fp16 limit (planted), a piece of the query behind residue 400 of every longer subject (for launches that
    report 400 as the longest subject)."""
    key = ("ragged", qlen, planted, last_mult4)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(31000 + qlen)
    q = query(qlen) if qlen >= 590 else rng.integers(0, 20, 850).astype(np.int8)
    lens = rng.integers(330, 601, RAGGED_N)
    lens[lens % 4 == 0] += 1
    lens[lens > 600] = 599
    lens[7] = 600                                       # the longest subject the case promises
    seqs = [rng.integers(0, 20, int(l)).astype(np.int8) for l in lens]
    _tails(rng, q, seqs, RAGGED_BOUND)
    for (batch, group), (la, lb) in SHORT_PAIRS.items():
        seqs[index(batch, group, 0)] = rng.integers(0, 20, la).astype(np.int8)
        seqs[index(batch, group, 1)] = rng.integers(0, 20, lb).astype(np.int8)
    for group in range(4, 8):                           # a wave of subjects of at most three residues
        seqs[index(8, group, 0)] = rng.integers(0, 20, group % 4).astype(np.int8)
        seqs[index(8, group, 1)] = rng.integers(0, 20, (group + 1) % 4).astype(np.int8)
    for batch, group in EMPTY_PAIRS:
        seqs[index(batch, group, 0)] = np.zeros(0, dtype=np.int8)
        seqs[index(batch, group, 1)] = np.zeros(0, dtype=np.int8)
    if planted:
        seqs[PLANTED] = np.concatenate([mutated(rng, q[:590], 11), rng.integers(0, 20, 7).astype(np.int8)])
    if last_mult4:                                      # the canary then follows the last LETTER directly, no padding byte between
        seqs[RAGGED_N - 1] = seqs[RAGGED_N - 1][:len(seqs[RAGGED_N - 1]) // 4 * 4]
    _cases[key] = Case("ragged", _wrap(rng, seqs), HEAD, RAGGED_N, PART16, RAGGED_BOUND)
    return _cases[key]


def dirtier():
    """the launch that leaves its scratch behind for another (stale scratch): 200 subjects of 600 .. 900 residues, longer
    than any 16-lane case's, for a query of three stripes"""
    if "dirtier" not in _cases:
        rng = np.random.default_rng(32000)
        q = query(1530)
        seqs = [rng.integers(0, 20, int(l)).astype(np.int8) for l in rng.integers(600, 901, 200)]
        seqs[17][100:400] = mutated(rng, q[200:500], 5)
        _cases["dirtier"] = Case("dirtier", _wrap(rng, seqs), HEAD, 200, PART16)
    return _cases["dirtier"]


def streamed(qlen, hi):
    """case (c): 330 subjects of 40 .. hi residues, ascending (the streamed kernels take a batch's last subject for its
    longest), every third with a piece of the query, one with an exact copy of 300 (or hi) residues: near the fp16 limit,
    so that the overflow list is written and the subject streamed behind it is flagged with it"""
    key = ("streamed", qlen, hi)
    if key not in _cases:
        rng = np.random.default_rng(33000 + qlen + hi)
        q = query(qlen)
        lens = np.sort(rng.integers(40, hi + 1, 330))
        lens[-1] = hi
        seqs = [rng.integers(0, 20, int(l)).astype(np.int8) for l in lens]
        for k in range(0, 330, 3):
            n = int(rng.integers(20, len(seqs[k]) + 1))
            at_q = int(rng.integers(0, qlen - n + 1))
            at = int(rng.integers(0, len(seqs[k]) - n + 1))
            seqs[k][at:at + n] = mutated(rng, q[at_q:at_q + n], 4 + k % 3)
        seqs[300][:] = q[100:100 + len(seqs[300])]
        _cases[key] = Case("streamed", _wrap(rng, seqs), HEAD, 330, PART16, bound=(hi * 2 // 3) // 4 * 4)
    return _cases[key]


WIDE_LENGTHS = (1281, 1300, 1350, 1390, 1400, 1450, 1550, 1650, 1700)
WIDE_BOUND = 1400


def wide(qlen):
    """case (e): nine subjects of 1281 .. 1700 residues for the wave-wide groups of partition 34; one carries 500 mutated
    residues of the query, the ones beyond 1400 a piece of it behind residue 1400"""
    key = ("wide", qlen)
    if key not in _cases:
        rng = np.random.default_rng(34000 + qlen)
        q = query(qlen)
        seqs = [rng.integers(0, 20, l).astype(np.int8) for l in WIDE_LENGTHS]
        seqs[2][300:800] = mutated(rng, q[100:600], 5)
        _tails(rng, q, seqs, WIDE_BOUND)
        head = [rng.integers(0, 20, 1290).astype(np.int8) for _ in range(2)]
        tail = [rng.integers(0, 20, 1290).astype(np.int8) for _ in range(2)]
        _cases[key] = Case("wide", head + seqs + tail, 2, len(WIDE_LENGTHS), PART64, WIDE_BOUND)
    return _cases[key]


LIST_CAPACITY, LIST_LONG = 64, 60


def listed(qlen, count):
    """case (f): a DB of 120 subjects of 100 .. 700 residues and one of 8200, and a re-score list of `count` positions
    scattered over it: the subject beyond 8000 first, then the DB's first and its last subject.  The entries behind the
    count name subject 1, which is not in the list: a kernel that read them would score it.
    -> (case, positions[LIST_CAPACITY])"""
    key = ("listed", qlen)
    if key not in _cases:
        rng = np.random.default_rng(35000 + qlen)
        q = query(qlen)
        seqs = [rng.integers(0, 20, int(l)).astype(np.int8) for l in rng.integers(100, 701, 120)]
        seqs[LIST_LONG] = rng.integers(0, 20, 8200).astype(np.int8)
        seqs[LIST_LONG][4000:4600] = mutated(rng, q[50:650], 4)
        seqs[33][20:90] = mutated(rng, q[700:770], 5)
        c = Case("listed", seqs, 1, 118, -1)     # (no range: the list addresses all N subjects)
        c.order = [LIST_LONG, 0, 119] + [int(i) for i in rng.permutation(120) if i not in (LIST_LONG, 0, 119, 1)]
        _cases[key] = c
    c = _cases[key]
    pos = np.full(LIST_CAPACITY, 1, dtype=np.int32)
    pos[:count] = c.order[:count]
    return c, pos
