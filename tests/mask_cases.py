"""Inputs of the subject-masking tests (test_mask_cpu.py, test_gpu_mask.py): seeded, generated, nothing committed as data."""
import functools

import numpy as np

import mask_ref as MR
import oracle_lib as O
from cudasw4_amd import synthdb

BLOCK_LENGTHS = [0, 1, 3, 4, 11, 12, 13, 23, 24, 25, 63, 64, 65, 75, 76, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097, 70001]
# (window, trigger_sum, extend_sum): the defaults; the smallest window, where only a homopolymer triggers and one repeated
# letter extends; the widest window at 3.0 / 3.5 bits
PARAM_SETS = [(12, 20705, 17019), (4, 4 * MR.U[4], 2048), (32, MR.threshold(32, 3.0), MR.threshold(32, 3.5))]
# unbounded runs: any window with one repeated letter is lo, only a homopolymer window triggers
RUN_WINDOW = 12
RUN_PARAMS = (RUN_WINDOW, RUN_WINDOW * MR.U[RUN_WINDOW], 2048)
LONGEST_TILE = 1024   # bytes of the largest piece a workgroup of the masking kernels takes


def structured_subject(rng, length):
    """Background and low-complexity segments of random lengths 1 .. 40 in turn; a low-complexity segment draws from one to
    three letters with skewed weights; about 1 % of the positions are code 20."""
    out = np.empty(length, dtype=np.int8)
    pos, low = 0, bool(rng.integers(0, 2))
    while pos < length:
        k = min(int(rng.integers(1, 41)), length - pos)
        if low:
            m = int(rng.integers(1, 4))
            letters = rng.choice(20, size=m, replace=False)
            w = np.array([0.7, 0.2, 0.1][:m])
            out[pos:pos + k] = letters[rng.choice(m, size=k, p=w / w.sum())]
        else:
            out[pos:pos + k] = rng.integers(0, 20, k)
        pos += k
        low = not low
    out[rng.random(length) < 0.01] = 20
    return out


def _block(seqs):
    chars, offsets, lengths = O.make_db(seqs)
    return {"chars": np.asarray(chars, dtype=np.int8), "offsets": np.asarray(offsets, dtype=np.uint64),
            "lengths": np.asarray(lengths, dtype=np.int32)}


@functools.lru_cache(maxsize=None)
def structured_block(seed=3):
    rng = np.random.default_rng(seed)
    return _block([structured_subject(rng, l) for l in BLOCK_LENGTHS])


@functools.lru_cache(maxsize=None)
def run_block():
    """Four subjects for RUN_PARAMS.  Six letters leave no window of 12 without a repeat, so all of a subject is one run of lo
    windows except where 12 distinct letters are planted; a planted homopolymer 12-mer is the only trigger.
      0  70 001 residues, the trigger at the far right end, the distinct window at 3000: masked from behind it to the end
      1  the mirror image: the trigger at the far left, the distinct window 3000 before the end
      2  one letter throughout (5000): masked whole
      3  no trigger (5000): untouched although all of it is lo
    A window that overlaps the planted one by seven letters or more may have no repeat either, so the run ends within 12
    positions of the planted window: "bounds" holds, per subject, the inclusive ranges of the one segment's first position
    and of the position behind its last (None: no segment)."""
    rng = np.random.default_rng(17)
    W, L = RUN_WINDOW, 70001
    distinct = np.arange(6, 6 + W, dtype=np.int8)

    def six(n):
        return rng.integers(0, 6, n).astype(np.int8)

    right = six(L)
    right[3000:3000 + W] = distinct
    right[L - W:] = 2
    left = six(L)
    left[L - 3000 - W:L - 3000] = distinct
    left[:W] = 4
    b = _block([right, left, np.full(5000, 9, dtype=np.int8), six(5000)])
    # (a chance homopolymer 12-mer of six letters: 6^-11 per window)
    d = L - 3000 - W
    b["bounds"] = [((3001, 3012), (L, L)), ((0, 0), (d, d + W - 1)), ((0, 0), (5000, 5000)), None]
    return b


def cases():
    """(name, codes) of single subjects for the CPU tests"""
    rng = np.random.default_rng(23)
    out = [("structured%d" % l, structured_subject(rng, l)) for l in BLOCK_LENGTHS if l <= 4097]
    out.append(("polyQ", np.full(40, 5, dtype=np.int8)))
    out.append(("two-letter repeat", np.tile(np.array([15, 7], dtype=np.int8), 30)))
    out.append(("all X", np.full(50, 20, dtype=np.int8)))
    out.append(("codes above 20", (rng.integers(0, 3, 80) + 21).astype(np.int8)))
    rb = run_block()
    for i in (2, 3):
        o = int(rb["offsets"][i])
        out.append(("run%d" % i, rb["chars"][o:o + int(rb["lengths"][i])]))
    return out


# ---- the end-to-end fixture: decoys with a low-complexity tract against relatives of the query's core ------------------------

TRACT_CODES, TRACT_WEIGHTS = (15, 7, 0), (0.6, 0.25, 0.15)   # S, G, A
N_DECOYS, N_RELATIVES, N_BACKGROUND = 150, 12, 300
LETTERS = "ARNDCQEGHILKMFPSTWYV"


def _tract(rng, n):
    return np.asarray(TRACT_CODES, dtype=np.int8)[rng.choice(3, size=n, p=TRACT_WEIGHTS)]


@functools.lru_cache(maxsize=None)
def fixture(seed=11):
    """A 240-residue query with a 40-residue S/G/A tract at 100 .. 139; 150 random decoys with a 60-residue tract of the same
    letters, 12 relatives of the query's other 200 residues at identity 0.30, 300 random background subjects; the DB ascends
    by length.  -> dict(query, letters, chars, offsets, lengths, kind ('D' / 'R' / 'B' per subject))"""
    rng = np.random.default_rng(seed)
    comp = synthdb.SPROT_COMPOSITION
    core = synthdb._residues(rng, 200, comp)
    query = np.concatenate([core[:100], _tract(rng, 40), core[100:]]).astype(np.int8)
    subjects = []
    for _ in range(N_RELATIVES):
        subjects.append(("R", synthdb.mutate(rng, core, 0.30, 0.01, comp)))
    for _ in range(N_DECOYS):
        body = synthdb._residues(rng, int(rng.integers(100, 400)), comp)
        at = int(rng.integers(0, len(body) + 1))
        subjects.append(("D", np.concatenate([body[:at], _tract(rng, 60), body[at:]]).astype(np.int8)))
    for _ in range(N_BACKGROUND):
        subjects.append(("B", synthdb._residues(rng, int(rng.integers(50, 601)), comp)))
    order = sorted(range(len(subjects)), key=lambda i: (len(subjects[i][1]), i))
    b = _block([subjects[i][1] for i in order])
    b["kind"] = np.array([subjects[i][0] for i in order])
    b["query"] = query
    b["letters"] = "".join(LETTERS[c] for c in query)
    return b
