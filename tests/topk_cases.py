"""Inputs and references for the top-K tests (tests/test_topk_cases_cpu.py, tests/test_gpu_topk.py).  numpy only: no GPU, no torch.

sw_topk (cudasw4_amd/csrc/sw_topk.hip) returns the k best scores in descending order, equal scores in input
(position) order, padded with (-1.0, -1) from index n on.  It has three implementations behind one entry point:

  small   k <= 32 and n > k: topk_small_partial_kernel (every workgroup walks chunks of 2 048 scores with its k best keys in
          LDS; small_merge extracts a chunk's maxima one by one) and topk_small_final_kernel (the same over the workgroups' lists)
  select  six radix-select passes over the 64-bit key (score bits, ~position), a compaction, then topk_rank_emit_kernel
          (k <= 1024) or a hipCUB sort of the winners
  sort    a full hipCUB sort; also taken when k >= n

`reference` is the plain restatement of the result, `walk_model` a restatement of the small path's chunk walk (of chunks and
insertions, not of threads) that tells where in the best list every insertion lands, and the families below are inputs aimed
at one kernel line each.  -0.0 and NaN are left out of every family: the device orders scores by their bits, the reference
by their values, and the two agree for every other float.
"""
from collections import namedtuple

import numpy as np

CHUNK = 2048          # kSmallChunk: scores per chunk of the small path (256 threads x 8)
SMALL_K = 32          # kSmallK: the small path's largest k
SMALL_MAX_GRID = 1024  # kSmallMaxGrid


# ---------------------------------------------------------------- reference

def reference(scores_f32, k):
    """-> (scores float32[k], positions int64[k]): the first min(k, n) entries of the input ordered by (score descending,
    position ascending), compared as float64, then (-1.0, -1) padding.  Independent of the oracle's swo_topk."""
    s = np.asarray(scores_f32, dtype=np.float32)
    n = len(s)
    k = int(k)
    out_s = np.full(max(k, 0), -1.0, dtype=np.float32)
    out_i = np.full(max(k, 0), -1, dtype=np.int64)
    m = min(k, n)
    if m <= 0:
        return out_s, out_i
    s64 = s.astype(np.float64)
    if m < n:
        kth = np.partition(s64, n - m)[n - m]                  # value of the m-th best
        above = np.flatnonzero(s64 > kth)
        ties = np.flatnonzero(s64 == kth)[:m - len(above)]     # flatnonzero is in position order
        cand = np.concatenate([above, ties])
    else:
        cand = np.arange(n)
    order = np.lexsort((cand, -s64[cand]))                     # last key is the primary one
    cand = cand[order]
    assert len(cand) == m
    out_s[:m] = s[cand]
    out_i[:m] = cand
    return out_s, out_i


def k_for_position(scores_f32, p):
    """the k whose k-th best element (reference order) is the one at position p"""
    s = np.asarray(scores_f32, dtype=np.float64)
    return int((s > s[p]).sum() + (s[:p + 1] == s[p]).sum())


def small_grid(n, num_cus):
    """workgroups of topk_small_partial_kernel (sw_topk.hip: small_grid)"""
    nchunks = (n + CHUNK - 1) // CHUNK
    return max(1, min(nchunks, SMALL_MAX_GRID, max(1, num_cus) * 4))


# ---------------------------------------------------------------- the chunk walk of the small path

Walk = namedtuple("Walk", "partial final partial_chunks final_chunks lists final_list")
Walk.__doc__ = """partial[b]: insertions of workgroup b that landed at index k-1 and were followed by another non-skipped chunk of
that workgroup; final: the same for the final kernel (it has no skip test: every chunk after the landing counts);
partial_chunks[b] / final_chunks: one (chunk, insertions, of which at k-1) per chunk that was not skipped;
lists[b] / final_list: the best lists as (score, position) pairs, None where a list was never filled that far."""

_LOWEST = (-np.inf, np.inf)   # stands for the kernels' key 0: below every real (score, position)


def _beats(s, p, ts, tp):
    """elementwise (s, p) above (ts, tp) in the order (score descending, position ascending)"""
    return (s > ts) | ((s == ts) & (p < tp))


def _merge_chunk(best, s, p, k):
    """small_merge: the chunk's maxima one at a time until one fails to enter (at most k rounds).  best: descending list of
    (score, position), changed in place.  -> (insertions, insertions that landed at index k-1)"""
    ts, tp = best[k - 1]
    enter = np.flatnonzero(_beats(s, p, ts, tp))      # the k-th best only rises: nothing else can ever enter
    if len(enter) == 0:
        return 0, 0
    enter = enter[np.lexsort((p[enter], -s[enter]))]
    inserted = at_kth = 0
    for j in enter[:k]:
        m = (float(s[j]), int(p[j]))
        ts, tp = best[k - 1]
        if not (m[0] > ts or (m[0] == ts and m[1] < tp)):
            break
        i = k - 1                                     # the sorted insertion of thread 0
        while i > 0 and (best[i - 1][0] < m[0] or (best[i - 1][0] == m[0] and best[i - 1][1] > m[1])):
            best[i] = best[i - 1]
            i -= 1
        best[i] = m
        inserted += 1
        at_kth += i == k - 1
    return inserted, at_kth


def _counted(chunks):
    """landings at k-1 in every recorded chunk but the last one"""
    return sum(c[2] for c in chunks[:-1])


def walk_model(scores, k, grid):
    """The chunk walk of topk_small_partial_kernel launched with `grid` workgroups and of topk_small_final_kernel over
    their grid*k candidates.  Workgroup b visits chunks b, b+grid, ... of 2 048 elements; a chunk is skipped when nothing
    in it beats the workgroup's k-th best, otherwise its maxima are merged one at a time until one fails to enter."""
    s = np.asarray(scores, dtype=np.float64)
    n = len(s)
    pos = np.arange(n, dtype=np.int64)
    nchunks = (n + CHUNK - 1) // CHUNK
    partial, partial_chunks, lists = [], [], []
    for b in range(grid):
        best = [_LOWEST] * k
        rec = []
        for c in range(b, nchunks, grid):
            lo, hi = c * CHUNK, min(n, (c + 1) * CHUNK)
            ins, kth = _merge_chunk(best, s[lo:hi], pos[lo:hi], k)
            if ins:
                rec.append((c, ins, kth))
        partial.append(_counted(rec))
        partial_chunks.append(rec)
        lists.append(best)
    # the final kernel: candidate b*k + j is entry j of workgroup b's list; unfilled entries (key 0) never enter
    cs = np.array([e[0] for l in lists for e in l], dtype=np.float64)
    cp = np.array([e[1] if e[1] != np.inf else -1 for l in lists for e in l], dtype=np.int64)
    real = cp >= 0
    best = [_LOWEST] * k
    rec = []
    nfinal = (grid * k + CHUNK - 1) // CHUNK
    for c in range(nfinal):
        sl = slice(c * CHUNK, min(grid * k, (c + 1) * CHUNK))
        keep = real[sl]
        ins, kth = _merge_chunk(best, cs[sl][keep], cp[sl][keep], k)
        rec.append((c, ins, kth))                     # no skip test here: small_merge runs on every chunk
    return Walk(partial, _counted(rec), partial_chunks, rec, [[e if e != _LOWEST else None for e in l] for l in lists],
                [e if e != _LOWEST else None for e in best])


# ---------------------------------------------------------------- input families: (n, k, seed) -> float32 scores

def ascending(n, k=0, seed=0):
    # small_merge, the break test `m <= kth`: every chunk replaces the whole list, its last round (k-1) lands at k-1 —
    # the insertion a late wave could see when the k-th best was read after the reduction.  The final kernel sees the
    # workgroups' lists in ascending order and does the same.
    assert n < 1 << 24
    return np.arange(n, dtype=np.float32)


def ascending_stairs(w):
    # as ascending, with runs of w equal scores (w no multiple of 2 048): ties run across chunk and workgroup borders, so
    # the ~position half of topk_key decides which of a run enters and where small_merge's `best[i - 1] < m` stops.
    assert w % CHUNK != 0

    def make(n, k=0, seed=0):
        assert n // w < 1 << 24
        return (np.arange(n, dtype=np.int64) // w).astype(np.float32)
    make.__name__ = "ascending_stairs_%d" % w
    return make


def descending(n, k=0, seed=0):
    # topk_small_partial_kernel, `above = above || key[e] > thr` and the __syncthreads_or skip: nothing enters after the
    # first chunk of a workgroup.
    assert n < 1 << 24
    return np.arange(n - 1, -1, -1, dtype=np.float32)


NEWCOMER_GAP = 1 << 20


def single_newcomer(n, k, seed=0):
    # small_merge in a chunk whose ONE newcomer barely enters: anchors 2G ... kG at positions 1 ... k-1, element 2048*c
    # holds G + c, everything else is noise below G.  In workgroup 0 every later chunk has exactly one element that enters;
    # it lands at k-1 and the next round's maximum fails the break test.
    G = NEWCOMER_GAP
    assert 1 <= k <= SMALL_K and n >= k and (n + CHUNK - 1) // CHUNK + G < 1 << 24
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1000, n).astype(np.float32)
    s[0::CHUNK] = G + np.arange((n + CHUNK - 1) // CHUNK)
    s[1:k] = G * np.arange(2, k + 1)
    return s


def all_equal(n, k=0, seed=0):
    # topk_hist_kernel passes 3-5 (the ~position digits) and topk_pick: the k-th element lies inside one tie group that is
    # the whole input, so the position digits alone decide it.
    return np.full(n, 7.0, dtype=np.float32)


def two_levels(count_hi, lo=3.0, hi=5.0):
    # count_hi seeded positions hold `hi`, all others `lo`.  k < count_hi: the k-th lies among the hi ties; k == count_hi:
    # topk_pick's `remaining == h[b]` takes the whole bin (skip_rest, no position passes); k > count_hi: the position passes
    # run among the lo ties.  topk_compact_kernel's `(key & decided) >= prefix` must keep exactly k.
    def make(n, k=0, seed=0):
        s = np.full(n, lo, dtype=np.float32)
        s[np.random.default_rng(seed).choice(n, min(count_hi, n), replace=False)] = hi
        return s
    make.__name__ = "two_levels_%d" % count_hi
    return make


def mostly_unscored(n, k, seed=0):
    # topk_key on negative floats (`u ^= 0xffffffff`): the scan pre-fills with -1, a failed pipeline marks subjects -2.
    # Fewer than k positive scores, so the k-th best is one of the -1 ties and the -2 entries must stay out.
    rng = np.random.default_rng(seed)
    s = np.full(n, -1.0, dtype=np.float32)
    where = rng.choice(n, min(n, 8), replace=False)
    npos = min(5, max(k - 1, 0), len(where))
    s[where[:npos]] = rng.integers(1, 500, npos)
    s[where[npos:npos + 3]] = -2.0
    return s


MIXED_PALETTE = np.array([-1e9, -46662.0, -16777218.0, -2.5, -1.0, -0.5, -1e-30, 0.0, 1e-30, 0.25, 0.5, 1.0, 1.5, 2047.0, 2048.0,
                          46662.0, 46662.5, 16777216.0, 16777218.0, 33554436.0, 1e9, 999999936.0], dtype=np.float32)


def mixed_floats(n, k=0, seed=0):
    # topk_key's transform over the whole float range and its inverse in the emit kernels: negative, zero, fractional and
    # large values (46 662; above 2^24; up to 1e9) with duplicates, and random floats of every magnitude between them.
    rng = np.random.default_rng(seed)
    s = MIXED_PALETTE[rng.integers(0, len(MIXED_PALETTE), n)].copy()
    some = rng.random(n) < 0.3
    s[some] = (rng.standard_normal(int(some.sum())) * 10.0 ** rng.integers(-3, 9, int(some.sum()))).astype(np.float32)
    s[s == 0] = 0.0                                   # (no -0.0: see the module docstring)
    return s


STAIRS = (1000, CHUNK * 3 + 7)
FAMILIES = {f.__name__: f for f in (ascending, ascending_stairs(STAIRS[0]), ascending_stairs(STAIRS[1]), descending, single_newcomer,
                                    all_equal, two_levels(5000), mostly_unscored, mixed_floats)}

# the select's digit borders: the k-th element at these positions of a tie group (the 10-bit low digit of ~position; the top
# position digit, shift 21), in an input of BORDER_N scores; k comes from k_for_position
BORDER_N = (1 << 21) + 3000
BORDER_POSITIONS = (1023, 1024, 1025, (1 << 21) - 1, 1 << 21, (1 << 21) + 1)
BORDER_SEED = 21
