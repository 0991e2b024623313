"""Case generators of the hit-alignment tests (sw_align_hits, sw_align_hits_pssm).  TEST INFRASTRUCTURE ONLY: numpy and the
scalar references (align_ref, pssm_align_ref), no GPU.

Two kinds of cases:

  planted(...)             one pair whose optimal local alignment is known before any DP runs: an exact copy of r query rows
                           (or of the consensus of r PSSM rows) inside subject flanks of code 20, with at most one gap.  The
                           rectangle fixes the dimensions of the kernel's passes: the trace pass runs over r x c, the reverse
                           pass over q_end x s_end.  tests/test_align_cases_cpu.py holds every planted case of the GPU tests
                           to its intended coordinates under the reference alone.
  random_align_case(rng)   one query and 1..12 subjects with random scoring, budgets and scratch sizes, and the results the
                           C ABI has to report for them (tests/fuzz_gpu.py --features align).

Why a planted rectangle is the optimum.  Every subject residue of the copy meets its own row, whose score is the largest of
its column (a BLOSUM self-score; the favoured entry of a PSSM row), so no alignment scores more than the sum over the copy;
the flanks (code 20) and the query rows outside the rectangle (code 20 / rows without a positive entry) score negative
against everything, so nothing extends it, no other row ties with its end, and a PSSM row outside it cannot favour a residue
of the copy more than that residue's own row does.  With a gap, each half beside it scores
more than the gap costs, so bridging beats either half."""
import numpy as np

import align_ref as A
import oracle_lib as O
import pssm_align_ref as PA

# rows and cols at which dp_pass (sw_align_kernel.hpp) changes its path: 8 rows per lane, 64 lanes, 512 rows per stripe,
# a last stripe of fewer than 64 lanes, the 64-step blocks of the look-ahead
BORDERS = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 519, 520, 1023, 1024, 1025, 1030]
REVERSE_COLS = [1, 64, 65, 128, 129]
GAP3 = 3

# the gap scores tests/fuzz_gpu.py draws for the scan (one entry doubled on purpose: the default is drawn twice as often) ...
FUZZ_GAPS = [(-11, -1), (-11, -1), (-13, -2), (-10, -1), (-5, -5), (-20, -3), (-1, -1), (-40, -12), (-3, -12), (-100, -30)]
# ... and what only the alignment entry points take
ALIGN_GAPS = FUZZ_GAPS + [(0, 0), (-5, -5), (-2, -5), (-65536, -65536), (-65536, -1)]

STRONG = [17, 4, 8, 18, 14]   # W C H Y P: the largest self-scores of the BLOSUM tables


def trace_bytes(rows, cols):
    """sw_align_args::trace_bytes of a rows x cols rectangle (include/cudasw4_amd.h; capi.align_trace_bytes)"""
    return (rows + 511) // 512 * (cols + 63) * 256


def slot_bytes(max_subject_len, trace):
    """scratch of one pair: the stripe border and the trace, each rounded up to 256 bytes"""
    return (8 * (max_subject_len + 1) + 255) // 256 * 256 + (trace + 255) // 256 * 256


def random_pssm(rng, qlen):
    """as tests/test_gpu_pssm_align.py: scores -9 .. 3, one favoured residue per row (5 .. 12), column 20 negative"""
    p = rng.integers(-9, 4, (qlen, 21)).astype(np.int8)
    p[np.arange(qlen), rng.integers(0, 20, qlen)] = rng.integers(5, 13, qlen)
    p[:, 20] = -1 - rng.integers(0, 4, qlen)
    return p


def consensus_codes(p):
    return np.argmax(np.asarray(p)[:, :20], axis=1).astype(np.int8)


def matrix_rows(which, full25):
    """-> (table as sw_set_matrix takes it, rows x 21 int8 as the references take it)"""
    if not full25:
        m = O.blosum21(which)
        return m, m
    from cudasw4_amd import driver
    t = np.asarray(driver.matrix25(which), dtype=np.int8)
    return t, np.ascontiguousarray(t.reshape(25, 25)[:, list(range(20)) + [23]])


class Case:
    """one query (letters: q + table / mref; PSSM: pssm + consensus or None) and its subjects"""

    def __init__(self, **kw):
        self.q = self.pssm = self.consensus = self.table = self.mref = None
        self.__dict__.update(kw)
        self._ref = {}

    @property
    def is_pssm(self):
        return self.pssm is not None

    @property
    def qlen(self):
        return len(self.pssm) if self.is_pssm else len(self.q)

    def query_key(self):
        """cases with one key can share a call"""
        if self.is_pssm:
            return ("pssm", self.pssm.tobytes(), None if self.consensus is None else np.asarray(self.consensus).tobytes())
        return ("letters", np.asarray(self.q).tobytes(), np.asarray(self.table).tobytes())

    def reference(self, s, gop, gex):
        """(fields, CIGAR words) of the scalar reference for subject s, computed once per (subject, gap scores)"""
        s = np.minimum(np.asarray(s, dtype=np.int8).view(np.uint8), 20).astype(np.int8)   # what the kernels read
        key = (s.tobytes(), gop, gex)
        if key not in self._ref:
            if self.is_pssm:
                self._ref[key] = PA.align(self.pssm, s, self.consensus, gop, gex)
            else:
                self._ref[key] = A.align(self.q, s, self.mref, gop, gex)
        return self._ref[key]

    def rescore(self, s, gop, gex, r, words):
        s = np.minimum(np.asarray(s, dtype=np.int8).view(np.uint8), 20).astype(np.int8)
        if self.is_pssm:
            return PA.rescore(self.pssm, s, gop, gex, r, words)
        return A.rescore(self.q, s, self.mref, gop, gex, r, words)


# ---- planted rectangles ------------------------------------------------------------------------------------------------

def _gap_cost(glen, gaps):
    return max(-(gop + (glen - 1) * max(gop, gex)) for gop, gex in gaps)


def planted(rng, r, c, q_begin, s_begin, gap=None, form="letters", gaps=((-11, -1), (-5, -5)), q_tail=9, s_tail=6, which=62,
            touch=None):
    """One pair whose alignment is the rectangle of r rows and c cols at (q_begin, s_begin).

    gap: None, or (side, length, at): side "I" = a run of `length` query rows without a subject residue, starting at row
    `at` of the rectangle (c = r - length); side "D" = `length` subject residues without a query row, starting at column
    `at` (c = r + length).  form: "letters" (BLOSUM `which`, 21 letters) or "pssm".  gaps: the gap scores the case must hold
    under.  touch: a subject code to put right before and right after the copy in place of code 20 (with q_begin = 0 and
    q_tail = 0 the query has no row that could meet it: the row the kernel pads the query with must not either).
    -> Case with .subject and .coords = (q_begin, q_end, s_begin, s_end)"""
    side, glen, at = gap if gap else (None, 0, 0)
    assert side in (None, "I", "D") and r >= 1 and c == r - (glen if side == "I" else 0) + (glen if side == "D" else 0) and c >= 1
    qlen = q_begin + r + q_tail
    if form == "letters":
        table, mref = matrix_rows(which, False)
        m = np.asarray(mref).reshape(21, 21)
        codes = rng.integers(0, 20, qlen).astype(np.int8)
        codes[:q_begin] = 20
        codes[q_begin + r:] = 20
        own = lambda lo, hi: int(sum(int(m[a, a]) for a in codes[lo:hi]))
    else:
        p = random_pssm(rng, qlen)
        p[:q_begin] = rng.integers(-9, 0, (q_begin, 21))
        p[q_begin + r:] = rng.integers(-9, 0, (q_tail, 21))
        codes = consensus_codes(p)
        own = lambda lo, hi: int(sum(int(p[i, codes[i]]) for i in range(lo, hi)))

    def strengthen(lo, hi, phase):
        for k, i in enumerate(range(lo, hi)):
            if form == "letters":
                codes[i] = STRONG[(k + phase) % len(STRONG)]
            else:
                p[i, codes[i]] = 12

    rows = np.arange(q_begin, q_begin + r)
    if side is None:
        copy = codes[rows]
    else:
        cost = _gap_cost(glen, gaps)
        first = (q_begin, q_begin + at)                                       # query rows of the two halves
        second = (q_begin + at + (glen if side == "I" else 0), q_begin + r)
        assert first[1] > first[0] and second[1] > second[0], "a gap lies between two halves"
        weak = False
        for phase, (lo, hi) in enumerate((first, second)):
            if own(lo, hi) <= cost:
                strengthen(lo, hi, phase)
                weak = True
            assert own(lo, hi) > cost, (r, c, gap, own(lo, hi), cost)
        if side == "I":
            # the rows of the run: random letters (a letter never scores more than the column's own); tiny halves, and
            # every PSSM (a row may favour a residue more than that residue's own row does): negative against everything
            if form != "letters":
                p[first[1]:second[0]] = rng.integers(-9, 0, (glen, 21))
                codes = consensus_codes(p)
            elif weak:
                codes[first[1]:second[0]] = 20
            copy = np.concatenate([codes[first[0]:first[1]], codes[second[0]:second[1]]])
        else:
            # the residues of the run: random, where each half outscores the gap even without its `glen` rows next to the run
            # (those could slide onto the run's residues instead of bridging it); else code 20
            far = own(first[0], max(first[0], first[1] - glen)) > cost and own(min(second[1], second[0] + glen), second[1]) > cost
            extra = rng.integers(0, 20, glen).astype(np.int8) if far and not weak else np.full(glen, 20, dtype=np.int8)
            copy = np.concatenate([codes[first[0]:first[1]], extra, codes[second[0]:second[1]]])
    assert len(copy) == c
    flank = lambda n: np.full(n, 20, dtype=np.int8)
    subject = np.concatenate([flank(s_begin), copy, flank(s_tail)]).astype(np.int8)
    if touch is not None:
        assert q_begin == 0 and q_tail == 0 and s_begin >= 1 and s_tail >= 1
        subject[s_begin - 1] = subject[s_begin + c] = touch
    coords = (q_begin, q_begin + r, s_begin, s_begin + c)
    if form == "letters":
        return Case(q=codes, table=table, mref=mref, subject=subject, coords=coords, gap=gap, rows=r, cols=c, form=form)
    return Case(pssm=p, consensus=None, subject=subject, coords=coords, gap=gap, rows=r, cols=c, form=form)


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dimension_cases(form):
    """(a), first set: per border value d a square d x d at (3, 11), and d x (d - 3), (d - 3) x d with one gap in the middle:
    the trace pass on the border, the reverse pass (3 + d) x (11 + d).  d = 1, 2 have no room for a gap of 3 and two halves:
    squares only."""
    def make():
        rng = np.random.default_rng([7001, int(form == "pssm")])
        out = []
        for d in BORDERS:
            out.append(planted(rng, d, d, 3, 11, form=form))
            if d - GAP3 >= 2:
                at = (d - GAP3) // 2
                out.append(planted(rng, d, d - GAP3, 3, 11, gap=("I", GAP3, at), form=form))
                out.append(planted(rng, d - GAP3, d, 3, 11, gap=("D", GAP3, at), form=form))
        return out
    return _once(("dimension", form), make)


def reverse_cases(form):
    """(a), second set: the reverse pass with d rows and d' cols (q_end = d, s_end = d'), d from the border list and d' on
    and beside the multiples of 64; the rectangle is the square of m = min(d, d', 40) that ends there.  The cases of one d
    and one m share their query (the rows before the rectangle must be filler, so the query follows m)."""
    def make():
        out = []
        for d in BORDERS:
            bases = {}
            for dc in REVERSE_COLS:
                m = min(d, dc, 40)
                if m not in bases:
                    bases[m] = planted(np.random.default_rng([7002, int(form == "pssm"), d, m]), m, m, d - m, 0, form=form)
                kw = dict(bases[m].__dict__)
                kw.pop("_ref")
                kw.update(subject=np.concatenate([np.full(dc - m, 20, np.int8), bases[m].subject]), coords=(d - m, d, dc - m, dc))
                out.append(Case(**kw))
        return out
    return _once(("reverse", form), make)


SEAM_GAPS = [(-11, -1), (-1, 0)]
SEAMS = [("I", 5, 510), ("I", 70, 480), ("D", 5, 62), ("D", 130, 60)]


def seam_cases(form):
    """(b): a rectangle of 1100 rows with one gap at a seam of dp_pass: an I run across the stripe border at row 512 (5 long
    from row 510; 70 long from row 480, longer than a 64-step block), a D run across the 64-step blocks (5 long from column
    62; 130 long from column 60, across two of them)"""
    def make():
        rng = np.random.default_rng([7003, int(form == "pssm")])
        out = []
        for side, glen, at in SEAMS:
            c = 1100 - glen if side == "I" else 1100 + glen
            out.append(planted(rng, 1100, c, 0, 5, gap=(side, glen, at), form=form, gaps=SEAM_GAPS))
        return out
    return _once(("seam", form), make)


CORNER_ROWS = [7, 8, 9, 64, 65, 512, 513, 1024]


def corner_cases(form):
    """the rectangle is the whole query (no row before, none after) and the subject holds an alanine (code 0, the code
    dp_pass scores its padding rows with) right before and right after the copy: a padding row that took part in the argmax
    of the local or of the reverse pass would lengthen the alignment"""
    def make():
        rng = np.random.default_rng([7004, int(form == "pssm")])
        return [planted(rng, d, d, 0, 11, form=form, q_tail=0, touch=0) for d in CORNER_ROWS]
    return _once(("corner", form), make)


def planted_sets(form):
    """every planted case of tests/test_gpu_align_edges.py with the gap scores it runs under"""
    return [("dimension", dimension_cases(form), [(-11, -1), (-5, -5)]),
            ("reverse", reverse_cases(form), [(-11, -1), (-5, -5)]),
            ("seam", seam_cases(form), SEAM_GAPS),
            ("corner", corner_cases(form), [(-11, -1), (-5, -5)])]


# ---- randomised cases ------------------------------------------------------------------------------------------------------

PAIR_CELLS = 4_000_000
CASE_CELLS = 40_000_000


def mutated_relative(rng, codes, L):
    """a subject of length L that holds a copy of `codes` with substitutions, insertions and deletions in random flanks"""
    copy = []
    for ch in codes:
        x = rng.random()
        if x < 0.04:
            continue
        if x < 0.08:
            copy.extend(rng.integers(0, 20, int(rng.integers(1, 12))).tolist())
        copy.append(int(rng.integers(0, 20)) if x > 0.85 else int(ch))
    copy = np.array(copy[:L], dtype=np.int8)
    s = rng.integers(0, 20, L).astype(np.int8)
    at = int(rng.integers(0, L - len(copy) + 1))
    s[at:at + len(copy)] = copy
    return s


def _draw_subject(rng, codes, qlen, cap):
    """codes: standard residues of the query rows (the consensus of a PSSM).  cap: longest subject the cell budget allows"""
    kind = ["planted", "planted", "relative", "relative", "repeat", "low", "empty", "random"][int(rng.integers(0, 8))]
    if kind == "planted":
        fits = [d for d in BORDERS if d <= qlen]
        r = int(rng.choice(fits))
        q_begin = int(rng.integers(0, qlen - r + 1))
        rows = codes[q_begin:q_begin + r]
        pick = int(rng.integers(0, 3))
        if pick == 1 and r >= 12:      # an I run
            glen = int(rng.integers(1, min(r - 8, 80)))
            at = int(rng.integers(4, r - glen - 3))
            rows = np.concatenate([rows[:at], rows[at + glen:]])
        elif pick == 2 and r >= 8:     # a D run
            glen = int(rng.integers(1, 140))
            at = int(rng.integers(4, r - 3))
            rows = np.concatenate([rows[:at], rng.integers(0, 20, glen).astype(np.int8), rows[at:]])
        s_begin = int(rng.choice([0, 1, 11, 60, 64])) if rng.integers(0, 2) else int(rng.choice(BORDERS)) % 200
        s = np.concatenate([np.full(s_begin, 20, np.int8), rows, np.full(int(rng.integers(0, 9)), 20, np.int8)])
    elif kind == "relative":
        lo = int(rng.integers(0, qlen))
        piece = codes[lo:lo + int(rng.integers(1, qlen - lo + 1))]
        L = len(piece) + int(rng.integers(0, 300)) if rng.integers(0, 4) else int(rng.integers(len(piece), max(len(piece) + 1, cap)))
        s = mutated_relative(rng, piece, max(L, 1))
    elif kind == "repeat":
        unit = codes[:int(rng.integers(1, 7))] if rng.integers(0, 2) else rng.integers(0, 20, int(rng.integers(1, 7))).astype(np.int8)
        s = np.tile(unit, int(rng.integers(2, 80)))
    elif kind == "low":
        s = rng.choice(rng.choice(20, 3, replace=False).astype(np.int8), int(rng.integers(3, 500)))
    elif kind == "empty":
        s = np.full(int(rng.integers(1, 90)), 20, dtype=np.int8)
    else:
        L = int(rng.integers(1, 700)) if rng.integers(0, 3) else int(rng.integers(1, max(2, cap)))
        s = rng.integers(0, 21, L).astype(np.int8)
    return kind, np.ascontiguousarray(s[:max(1, cap)], dtype=np.int8)


def under_budgets(full, trace=None, caps=None, expected=None):
    """what sw_align_hits reports for pairs whose reference results under ample budgets are `full` [(fields, words)]: a wrong
    expected score gives SCORE_MISMATCH (score and coordinates stay), a rectangle over the trace budget or a CIGAR longer than
    its slot gives NO_TRACE (exact coordinates); neither has counts or a CIGAR"""
    want = []
    for k, (r, w) in enumerate(full):
        r = dict(r)
        if expected is not None and expected[k] != r["score"]:
            r.update(status=A.SCORE_MISMATCH)
        if r["status"] == A.OK:
            over = trace is not None and trace_bytes(r["q_end"] - r["q_begin"], r["s_end"] - r["s_begin"]) > trace
            if over or (caps is not None and r["cigar_len"] > caps[k]):
                r.update(status=A.NO_TRACE)
        if r["status"] != A.OK:
            r.update(columns=0, identities=0, mismatches=0, gap_opens=0, gap_columns=0, cigar_len=0)
            w = w[:0]
        want.append((r, w))
    return want


def tie_cases(form):
    """-> [(Case, subjects)]: queries made of a repeated unit (period 5: ties inside a lane's 8 rows; 24: between lanes; 520:
    between stripes) against one unit, two units and a mutated run of units, and a three-letter low-complexity pair: many end
    cells, start cells and traceback branches of one score.  Not planted: the reference says which one the rules pick."""
    rng = np.random.default_rng([7005, int(form == "pssm")])
    out = []
    for period, copies in ((5, 30), (24, 46), (520, 3)):
        unit = rng.integers(0, 20, period).astype(np.int8)
        codes = np.tile(unit, copies)
        flank = lambda n: np.full(n, 20, dtype=np.int8)
        subjects = [np.concatenate([flank(3), unit, flank(2)]), np.concatenate([unit, unit]), np.tile(unit, copies)[: 1500],
                    mutated_relative(rng, np.tile(unit, min(copies, 12)), 12 * period + 40)]
        if form == "letters":
            table, mref = matrix_rows(62, False)
            out.append((Case(q=codes, table=table, mref=mref, form=form), subjects))
        else:
            unit_rows = random_pssm(rng, period)
            unit_rows[np.arange(period), unit] = 12
            p = np.tile(unit_rows, (copies, 1))
            out.append((Case(pssm=p, consensus=None, form=form), subjects))
    low = rng.choice(np.array([0, 9, 10], dtype=np.int8), 700)
    subjects = [rng.choice(np.array([0, 9, 10], dtype=np.int8), int(n)) for n in (40, 300, 900)] + [low[100:400].copy()]
    if form == "letters":
        table, mref = matrix_rows(62, False)
        out.append((Case(q=low, table=table, mref=mref, form=form), subjects))
    else:
        p = np.full((700, 21), -2, dtype=np.int8)
        p[np.arange(700), low] = 4
        p[:, [0, 9, 10]] = np.maximum(p[:, [0, 9, 10]], 1)   # three letters, two scores: ties wherever two paths meet
        p[:, 20] = -1
        out.append((Case(pssm=p, consensus=None, form=form), subjects))
    return out


def random_align_case(rng):
    """One randomised call of sw_align_hits / sw_align_hits_pssm and what it has to report.  -> Case with
    form, which, gop, gex, subjects, kinds; trace (sw_align_args::trace_bytes), caps (CIGAR slot sizes in words), temp_slots
    (None: the whole need, else the number of pair slots the scratch holds), expected (None or the list handed in as
    expected_scores); full (the reference's (fields, words) per pair, ample budgets) and want (the same under the case's
    budgets and expected scores: what the C ABI reports)."""
    form = ["letters21", "letters25", "pssm", "pssm_cons"][int(rng.integers(0, 4))]
    which = int(rng.choice([45, 50, 62, 80]))
    gop, gex = ALIGN_GAPS[int(rng.integers(0, len(ALIGN_GAPS)))]
    qlen = int(rng.choice(BORDERS)) + int(rng.integers(0, 3)) * int(rng.integers(0, 40)) if rng.integers(0, 2) else int(rng.integers(1, 1400))
    if form.startswith("letters"):
        full25 = form == "letters25"
        table, mref = matrix_rows(which, full25)
        q = rng.integers(0, 25 if full25 else 21, qlen).astype(np.int8)
        style = int(rng.integers(0, 5))
        if style == 0:     # a tandem repeat inside the query: end and start ties
            unit = rng.integers(0, 20, int(rng.integers(1, 7))).astype(np.int8)
            lo = int(rng.integers(0, qlen))
            rep = np.tile(unit, 40)[:qlen - lo]
            q[lo:lo + len(rep)] = rep
        elif style == 1:   # low complexity: traceback ties
            q = rng.choice(rng.choice(20, 3, replace=False).astype(np.int8), qlen)
        case = Case(q=np.ascontiguousarray(q, dtype=np.int8), table=table, mref=mref)
        codes = np.minimum(case.q, 19).astype(np.int8)
    else:
        p = random_pssm(rng, qlen)
        if rng.integers(0, 4) == 0:
            rows = rng.choice(qlen, max(2, qlen // 10), replace=qlen < 2)
            p[rows[::2], rng.integers(0, 20, len(rows[::2]))] = 127
            p[rows[1::2], rng.integers(0, 20, len(rows[1::2]))] = -128
        codes = consensus_codes(p)
        cons = None
        if form == "pssm_cons":
            cons = codes.copy()
            cons[rng.random(qlen) < 0.1] = 20     # "other": identical to nothing
            cons[rng.random(qlen) < 0.05] = 24
            cons[rng.random(qlen) < 0.1] = rng.integers(0, 20)
        case = Case(pssm=p, consensus=cons)
    # the references' int32 sentinel (-10^9) stays below every real value while (rows + cols) * 65536 < 10^9
    cap = min(PAIR_CELLS // qlen, 9600, 15000 - qlen)
    subjects, kinds, cells = [], [], 0
    for _ in range(int(rng.integers(1, 13))):
        kind, s = _draw_subject(rng, codes, qlen, cap)
        if cells + qlen * len(s) > CASE_CELLS:
            break
        cells += qlen * len(s)
        subjects.append(s)
        kinds.append(kind)
    if not subjects:
        subjects, kinds = [codes[:cap].copy()], ["planted"]
    n = len(subjects)
    full = [case.reference(s, gop, gex) for s in subjects]
    ok = [k for k in range(n) if full[k][0]["status"] == A.OK]
    need = lambda k: trace_bytes(full[k][0]["q_end"] - full[k][0]["q_begin"], full[k][0]["s_end"] - full[k][0]["s_begin"])
    trace = max(trace_bytes(qlen, len(s)) for s in subjects)
    tmode = int(rng.choice([0, 0, 1, 2])) if ok else 0
    if tmode:
        trace = need(ok[int(rng.integers(0, len(ok)))]) - (256 if tmode == 2 else 0)
    caps = []
    for k, s in enumerate(subjects):
        cm = int(rng.choice([0, 0, 1, 2]))
        nw = full[k][0]["cigar_len"]
        caps.append(qlen + len(s) if cm == 0 or nw == 0 else nw - (cm == 2))
    temp_slots = None if rng.integers(0, 2) else int(rng.integers(1, n + 1))
    expected = None
    emode = int(rng.integers(0, 3))
    if emode:
        expected = [f[0]["score"] for f in full]
        if emode == 2:
            expected[int(rng.integers(0, n))] += int(rng.choice([-1, 1, 100]))
    want = under_budgets(full, trace, caps, expected)
    case.__dict__.update(form=form, which=which, gop=gop, gex=gex, subjects=subjects, kinds=kinds, trace=trace, caps=caps,
                         temp_slots=temp_slots, expected=expected, full=full, want=want, cells=cells)
    return case
