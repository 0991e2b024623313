"""GPU: sw_align_hits and sw_align_hits_pssm at the shapes of their passes, not of their inputs, and at the edges of their
arguments; both forms, through the C ABI, field for field and CIGAR word for word against tests/align_ref.c and
tests/pssm_align_ref.c.

The cases are planted (tests/align_cases.py): the alignment rectangle is known before any DP runs, so the trace pass
(rows x cols) and the reverse pass (q_end x s_end) of dp_pass (sw_align_kernel.hpp) sit on the borders the kernel has:
8 rows per lane, 512 rows per stripe, a last stripe of fewer than 64 lanes, the 64-step blocks of the look-ahead, the byte
shift of the PSSM tile reload.  tests/test_align_cases_cpu.py proves on the CPU that every planted case hits its rectangle.

A planted query is filler outside its rectangle, so a query belongs to its case (the reverse-pass set shares one between
the cases of a border value): the cases of a set are one call per query, not one call per set.  A call is a few hundred
microseconds of kernels.

Run times on the MI355X are in the docstrings of the test functions."""
import numpy as np
import pytest

import align_abi as AB
import align_cases as C
import align_ref as A
import gpu_util as G
import oracle_lib as O

pytestmark = pytest.mark.gpu

FORMS = ["letters", "pssm"]


@pytest.fixture(scope="module")
def env():
    torch, capi, _ = G.gpu_modules()
    ctx = capi.Context(0)
    yield torch, capi, ctx
    ctx.close()


def run(env, case, subjects, gop, gex, **kw):
    torch, capi, ctx = env
    return AB.run(torch, capi, ctx, case, subjects, gop, gex, **kw)


def reference(case, subjects, gop, gex):
    return [case.reference(s, gop, gex) for s in subjects]


def check(env, case, subjects, gop, gex, where=(), **kw):
    """one call with ample budgets against the reference -> the call"""
    call = run(env, case, subjects, gop, gex, **kw)
    want = reference(case, subjects, gop, gex)
    bad = AB.compare(call.res, call.words, want, where)
    assert bad is None, bad
    assert AB.unused_words_untouched(call, want) is None
    return call


def test_trace_budget_formula(env):
    _, capi, _ = env
    for rows, cols in ((1, 1), (512, 1), (513, 64), (1030, 1233), (40000, 35213)):
        assert C.trace_bytes(rows, cols) == capi.align_trace_bytes(rows, cols)


# ---- a. pass dimensions ------------------------------------------------------------------------------------------------

def groups_by_query(cases):
    groups = {}
    for c in cases:
        groups.setdefault(c.query_key(), []).append(c)
    return list(groups.values())


@pytest.mark.parametrize("name", ["dimension", "reverse", "corner"])
@pytest.mark.parametrize("form", FORMS)
def test_pass_dimensions(env, form, name):
    """dimension: per border value d a planted d x d, d x (d - 3) and (d - 3) x d at (3, 11): the trace pass on the border,
    the reverse pass (3 + d) x (11 + d).  reverse: the reverse pass d x d' for d' = 1, 64, 65, 128, 129.  corner: the
    rectangle is the whole query and an alanine touches the copy on both sides (the padding rows of the last lane score as
    code 0: they must not take part in an argmax).  Under -11/-1 and -5/-5.
    MI355X: 0.45 s (dimension), 0.07 s (reverse), 0.04 s (corner) per form."""
    cases, gaps = next((cs, gs) for n, cs, gs in C.planted_sets(form) if n == name)
    for gop, gex in gaps:
        for group in groups_by_query(cases):
            subjects = [c.subject for c in group]
            call = check(env, group[0], subjects, gop, gex, where=(form, name, gop, gex, [c.coords for c in group]))
            for c, r in zip(group, call.res):   # (what test_align_cases_cpu.py holds the reference to)
                assert (int(r["q_begin"]), int(r["q_end"]), int(r["s_begin"]), int(r["s_end"])) == c.coords


# ---- b. gaps at the seams --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_gaps_at_the_seams(env, form):
    """1100 rows; an I run of 5 from row 510 and of 70 from row 480 (across the stripe border at 512; longer than a 64-step
    block), a D run of 5 from column 62 and of 130 from column 60 (across the look-ahead blocks); under -11/-1 and -1/0.
    MI355X: 0.1 s per form."""
    for gop, gex in C.SEAM_GAPS:
        for c in C.seam_cases(form):
            want, words = c.reference(c.subject, gop, gex)
            side, glen, at = c.gap
            text = A.cigar_string(words)
            assert "%d%s" % (glen, side) in text and want["gap_opens"] == 1, text
            if side == "I":   # (the run's first and last row lie on both sides of the border)
                assert text.startswith("%d=" % at) and at < 512 <= at + glen
            check(env, c, [c.subject], gop, gex, where=(form, c.gap, gop, gex))


# ---- c. the clamp of the global passes -----------------------------------------------------------------------------------

def clamp_pairs(form, rng):
    """(case, subject) x 2: a query of 600 with its rows 500 .. 579 copied to 8900 .. 8979 of a subject of 9000, and a query of
    1100 (a reverse pass of two stripes) with rows 1000 .. 1079 copied there"""
    out = []
    for qlen, lo in ((600, 500), (1100, 1000)):
        if form == "letters":
            q = rng.integers(0, 20, qlen).astype(np.int8)
            case = C.Case(q=q, table=O.blosum21(62), mref=O.blosum21(62))
            codes = q
        else:
            p = C.random_pssm(rng, qlen)
            case = C.Case(pssm=p, consensus=None)
            codes = C.consensus_codes(p)
        s = rng.integers(0, 20, 9000).astype(np.int8)
        s[8900:8980] = codes[lo:lo + 80]
        out.append((case, s, lo))
    return out


@pytest.mark.parametrize("form", FORMS)
def test_floor_clamp_of_the_global_passes(env, form):
    """Gap scores -65536/-65536 and -65536/-1 (the documented bound): the reverse pass has about 8980 columns, and with
    gex = -65536 edge(n) = gop + (n - 1) * gex passes kFloor = -2^29 after 8192 of them, so the far end of its first row, and
    every cell that takes its value from there, sits on the clamp.
    The references compute in int32 with the sentinel -10^9 for "no gap yet"; every real value stays above it while
    (rows + cols) * 65536 < 10^9, and (1100 + 9000) * 65536 = 6.6 * 10^8.
    MI355X: 0.2 s per form."""
    rng = np.random.default_rng(29 + (form == "pssm"))
    assert (1100 + 9000) * 65536 < 10**9
    for case, s, lo in clamp_pairs(form, rng):
        for gop, gex in ((-65536, -65536), (-65536, -1)):
            want, words = case.reference(s, gop, gex)
            assert want["status"] == A.OK and want["q_begin"] <= lo and want["q_end"] >= lo + 80 and want["s_end"] >= 8980
            assert want["gap_opens"] == 0
            if gex == -65536:   # the last columns of the reverse pass's first row, and all they lead to, are clamped
                assert gop + (want["s_end"] - 1) * gex < -(1 << 29)
            check(env, case, [s], gop, gex, where=(form, case.qlen, gop, gex))


# ---- d. argument edges -----------------------------------------------------------------------------------------------------

def relatives_case(form, rng, qlen, n, lo, hi):
    if form == "letters":
        q = rng.integers(0, 20, qlen).astype(np.int8)
        case = C.Case(q=q, table=O.blosum21(62), mref=O.blosum21(62))
        codes = q
    else:
        p = C.random_pssm(rng, qlen)
        case = C.Case(pssm=p, consensus=None)
        codes = C.consensus_codes(p)
    return case, G.relatives(rng, codes, n, lo, hi)


@pytest.mark.parametrize("form", FORMS)
def test_argument_edges(env, form):
    """MI355X: 0.01 s per form."""
    torch, capi, ctx = env
    rng = np.random.default_rng(41 + (form == "pssm"))
    case, subjects = relatives_case(form, rng, 200, 7, 200, 500)
    whole = check(env, case, subjects, -11, -1)

    def code_of(**kw):
        with pytest.raises(capi.SwError) as e:
            run(env, case, subjects, **kw)
        return e.value.code

    # gap scores: -65536 is the bound (test_floor_clamp_of_the_global_passes runs at it), one below is refused
    assert code_of(gop=-65537, gex=-1) == -1 and code_of(gop=-11, gex=-65537) == -1
    assert code_of(gop=1, gex=-1) == -1 and code_of(gop=-11, gex=1) == -1
    check(env, case, subjects[:2], -65536, -65536)
    # an unknown flag bit
    assert code_of(gop=-11, gex=-1, flags=2) == -1 and code_of(gop=-11, gex=-1, flags=capi.ALIGN_COORDS_ONLY | 4) == -1
    # a query of 2^20 + 1 (refused before any buffer is looked at: the pointers of the 200-residue query are never read)
    dq = torch.zeros(8, dtype=torch.int8, device="cuda")
    with pytest.raises(capi.SwError) as e:
        if case.is_pssm:
            capi.align_hits_pssm(ctx, dq.data_ptr(), 0, (1 << 20) + 1, 1, dq.data_ptr(), dq.data_ptr(), dq.data_ptr(), 4, -11, -1,
                                 dq.data_ptr(), dq.data_ptr(), dq.data_ptr(), trace_bytes=256)
        else:
            capi.align_hits(ctx, dq.data_ptr(), (1 << 20) + 1, 1, dq.data_ptr(), dq.data_ptr(), dq.data_ptr(), 4, -11, -1,
                            dq.data_ptr(), dq.data_ptr(), dq.data_ptr(), trace_bytes=256)
    assert e.value.code == -1
    # n = 0 with a temp: SW_OK, nothing written
    empty = run(env, case, [], -11, -1, temp_bytes=4096)
    assert empty.raw == bytes([AB.RESULT_FILL]) * len(empty.raw) and (empty.cigar == AB.SENTINEL).all()
    # max_subject_len below two of the seven lengths: those two are BAD_LENGTH, the others as before, less scratch asked for
    lengths = sorted(len(s) for s in subjects)
    bound = lengths[4]
    assert lengths[4] < lengths[5]
    tb = max(C.trace_bytes(case.qlen, L) for L in lengths)
    short = run(env, case, subjects, -11, -1, max_len=bound, trace=tb)
    assert short.need == 7 * C.slot_bytes(bound, tb) < whole.need == 7 * C.slot_bytes(lengths[-1], tb)
    bad = [k for k, s in enumerate(subjects) if len(s) > bound]
    assert len(bad) == 2
    for k in range(7):
        if k in bad:
            want = dict(score=0, status=capi.ALIGN_BAD_LENGTH, q_begin=-1, q_end=-1, s_begin=-1, s_end=-1, columns=0, identities=0,
                        mismatches=0, gap_opens=0, gap_columns=0, cigar_len=0)
            assert {f: int(short.res[k][f]) for f in A.FIELDS} == want
        else:
            assert short.res[k].tobytes() == whole.res[k].tobytes() and short.words[k].tolist() == whole.words[k].tolist()


# ---- e. slices and pointers ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_slices_streams_and_stray_codes(env, form):
    """MI355X: 0.03 s per form."""
    torch, capi, ctx = env
    rng = np.random.default_rng(53 + (form == "pssm"))
    case, subjects = relatives_case(form, rng, 300, 9, 250, 700)
    whole = check(env, case, subjects, -11, -1)
    # offsets that do not start at 0: only offsets[i] - offsets[0] counts
    moved = run(env, case, subjects, -11, -1, offset_base=4096)
    assert moved.res.tobytes() == whole.res.tobytes() and moved.cigar.tolist() == whole.cigar.tolist()
    # the tail of the arrays from pair 3 on: chars + offsets[3], offsets + 3, lengths + 3, n - 3, results + 3, cigar_offsets + 3
    tail = run(env, case, subjects, -11, -1, first=3)
    assert tail.res[3:].tobytes() == whole.res[3:].tobytes()
    assert all(a.tolist() == b.tolist() for a, b in zip(tail.words[3:], whole.words[3:]))
    dt = capi.align_result_dtype()
    assert tail.raw[:3 * dt.itemsize] == bytes([AB.RESULT_FILL]) * (3 * dt.itemsize)       # pairs 0 .. 2: not touched
    assert (tail.cigar[:int(tail.coff[3])] == AB.SENTINEL).all()
    # a stream of the caller's
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    streamed = run(env, case, subjects, -11, -1, stream=side)
    assert streamed.res.tobytes() == whole.res.tobytes() and streamed.cigar.tolist() == whole.cigar.tolist()
    # subject bytes that are no dbdata code (21 .. 24, and negative ones) count as code 20
    chars, offsets, lengths = O.make_db(subjects)
    stray = chars.copy()
    for k in (2, 6):
        at = int(offsets[k]) + rng.choice(int(lengths[k]), max(1, int(lengths[k]) // 20), replace=False)
        stray[at] = rng.choice(np.array([21, 22, 23, 24, -1, -1, -128], dtype=np.int8), len(at))
    assert (stray != chars).sum() >= 20
    cleaned = [np.where((s < 0) | (s > 20), 20, s).astype(np.int8)
               for s in (stray[int(offsets[k]):int(offsets[k]) + int(lengths[k])] for k in range(9))]
    got = run(env, case, None, -11, -1, db=(stray, offsets, lengths))
    want = reference(case, cleaned, -11, -1)
    bad = AB.compare(got.res, got.words, want, (form, "stray codes"))
    assert bad is None, bad
    assert want[2][0]["mismatches"] > whole.res[2]["mismatches"]   # (they landed inside the alignment)


# ---- f. exact budgets ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_exact_budgets(env, form):
    """MI355X: 0.04 s per form."""
    rng = np.random.default_rng(67 + (form == "pssm"))
    case, rel = relatives_case(form, rng, 700, 4, 600, 1500)
    empty = np.full(40, 20, dtype=np.int8)
    subjects = [rel[0], rel[1], empty, rel[2], rel[3]]
    full = reference(case, subjects, -11, -1)
    assert [f[0]["status"] for f in full] == [A.OK, A.OK, A.EMPTY, A.OK, A.OK]
    need = [C.trace_bytes(f[0]["q_end"] - f[0]["q_begin"], f[0]["s_end"] - f[0]["s_begin"]) if f[0]["status"] == A.OK else 0 for f in full]
    # the trace budget: exactly what pair 1's rectangle needs, and one 256-byte step less
    for trace in (need[1], need[1] - 256):
        call = run(env, case, subjects, -11, -1, trace=trace)
        want = C.under_budgets(full, trace=trace)
        bad = AB.compare(call.res, call.words, want, (form, "trace", trace))
        assert bad is None, bad
        assert want[1][0]["status"] == (A.OK if trace == need[1] else A.NO_TRACE)
        assert AB.unused_words_untouched(call, want) is None
    r = call.res[1]   # under the budget: exact coordinates, no counts
    assert [int(r[f]) for f in ("score", "q_begin", "q_end", "s_begin", "s_end")] == \
           [full[1][0][f] for f in ("score", "q_begin", "q_end", "s_begin", "s_end")]
    assert [int(r[f]) for f in ("columns", "identities", "mismatches", "gap_opens", "gap_columns", "cigar_len")] == [0] * 6
    # CIGAR slots: pairs 1 (the empty pair's slot follows it) and 4 (the guard word follows it) get exactly their words ...
    caps = [case.qlen + len(s) for s in subjects]
    caps[1], caps[4] = full[1][0]["cigar_len"], full[4][0]["cigar_len"]
    assert min(caps[1], caps[4]) >= 3
    call = run(env, case, subjects, -11, -1, caps=caps)
    bad = AB.compare(call.res, call.words, full, (form, "exact slots"))
    assert bad is None, bad
    assert AB.unused_words_untouched(call, full) is None
    # ... and one word less: NO_TRACE, and no word outside their own slots is touched
    caps[1] -= 1
    caps[4] -= 1
    call = run(env, case, subjects, -11, -1, caps=caps)
    want = C.under_budgets(full, caps=caps)
    assert [w[0]["status"] for w in want] == [A.OK, A.NO_TRACE, A.EMPTY, A.OK, A.NO_TRACE]
    bad = AB.compare(call.res, call.words, want, (form, "short slots"))
    assert bad is None, bad
    assert AB.unused_words_untouched(call, want) is None
    assert (call.cigar[int(call.coff[2]):int(call.coff[3])] == AB.SENTINEL).all() and call.cigar[-1] == AB.SENTINEL


# ---- g. ties -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_ties(env, form):
    """Repeats of period 5, 24 and 520 and a three-letter pair: end cells, start cells and traceback branches of one score,
    inside a lane, between lanes and between stripes; under affine, linear (-5/-5), inverted (-2/-5) and free (0/0) gaps.
    What picks among them (`better`, open before extend, diagonal before E before F) changes no score, only which optimum.
    MI355X: 0.5 s per form."""
    for case, subjects in C.tie_cases(form):
        for gop, gex in ((-11, -1), (-5, -5), (-2, -5), (0, 0)):
            check(env, case, subjects, gop, gex, where=(form, case.qlen, gop, gex))
