"""CPU: the planted cases of tests/test_gpu_align_edges.py (tests/align_cases.py) do what they are meant to do under the
scalar references alone: every one reports status OK and exactly the intended coordinates, so q_end - q_begin and
s_end - s_begin are the intended rows and cols of the trace pass and q_end, s_end those of the reverse pass.  This is a
condition on the generators, not a measurement: a case that misses is a bug of align_cases.py.  Also: the letter and the
PSSM reference agree on the pssm.from_sequence forms of the planted letter cases, the reference's CIGAR re-scores to its
score, and the randomised case generator keeps its budgets."""
import numpy as np
import pytest

import align_cases as C
import align_ref as A
import pssm_align_ref as PA

FORMS = ["letters", "pssm"]
SETS = ["dimension", "reverse", "seam", "corner"]


def cases_of(form, name):
    return next((cases, gaps) for n, cases, gaps in C.planted_sets(form) if n == name)


def test_the_planted_sets_cover_the_border_list():
    for form in FORMS:
        dim, _ = cases_of(form, "dimension")
        squares = [c for c in dim if c.gap is None]
        assert [c.rows for c in squares] == C.BORDERS and all(c.rows == c.cols and c.coords[0] == 3 and c.coords[2] == 11 for c in squares)
        with_gap = [d for d in C.BORDERS if d - C.GAP3 >= 2]
        assert with_gap == C.BORDERS[2:]   # 1 and 2 leave no room for a gap of 3 between two halves
        assert [(c.rows, c.cols) for c in dim if c.gap and c.gap[0] == "I"] == [(d, d - 3) for d in with_gap]
        assert [(c.rows, c.cols) for c in dim if c.gap and c.gap[0] == "D"] == [(d - 3, d) for d in with_gap]
        rev, _ = cases_of(form, "reverse")
        assert [(c.coords[1], c.coords[3]) for c in rev] == [(d, dc) for d in C.BORDERS for dc in C.REVERSE_COLS]
        seam, gaps = cases_of(form, "seam")
        corner, _ = cases_of(form, "corner")
        assert all(c.coords[0] == 0 and c.coords[1] == c.qlen and c.subject[10] == 0 and c.subject[11 + c.cols] == 0 for c in corner)
        assert [c.gap for c in seam] == C.SEAMS and all(c.rows == 1100 for c in seam) and gaps == [(-11, -1), (-1, 0)]


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("form", FORMS)
def test_every_planted_case_hits_its_coordinates(form, name):
    cases, gaps = cases_of(form, name)
    for gop, gex in gaps:
        for k, c in enumerate(cases):
            r, words = c.reference(c.subject, gop, gex)
            got = (r["q_begin"], r["q_end"], r["s_begin"], r["s_end"])
            assert r["status"] == A.OK and got == c.coords, (form, name, k, gop, gex, c.rows, c.cols, c.gap, got, c.coords)
            assert r["q_end"] - r["q_begin"] == c.rows and r["s_end"] - r["s_begin"] == c.cols
            assert c.rescore(c.subject, gop, gex, r, words) == r["score"]
            text = A.cigar_string(words)
            if c.gap is None:
                assert text == "%d=" % c.rows, (form, name, k, text)
            elif gop < gex:   # the planted run, and nothing else but identities (gop == gex: a split run costs the same)
                assert "%d%s" % (c.gap[1], c.gap[0]) in text and r["gap_opens"] == 1 and r["gap_columns"] == c.gap[1], (k, text)
                assert r["mismatches"] == 0 and r["identities"] == min(c.rows, c.cols)


@pytest.mark.parametrize("name", SETS)
def test_letter_and_pssm_reference_agree_on_the_planted_letter_cases(name):
    from cudasw4_amd import pssm
    cases, gaps = cases_of("letters", name)
    for gop, gex in gaps:
        for k, c in enumerate(cases):
            want, wcig = c.reference(c.subject, gop, gex)
            got, gcig = PA.align(pssm.from_sequence(c.q, c.table), c.subject, c.q, gop, gex)
            assert got == want and gcig.tolist() == wcig.tolist(), (name, k, gop, gex)


def test_random_cases_keep_their_budgets_and_say_what_to_expect():
    rng = np.random.default_rng(5)
    forms, statuses, kinds = set(), set(), set()
    for _ in range(25):
        c = C.random_align_case(np.random.default_rng(int(rng.integers(0, 2**31))))
        n = len(c.subjects)
        assert 1 <= n <= 12 and c.cells <= C.CASE_CELLS and all(c.qlen * len(s) <= C.PAIR_CELLS for s in c.subjects)
        assert (c.qlen + max(len(s) for s in c.subjects)) * 65536 < 10**9   # the references' sentinel stays out of reach
        assert (c.gop, c.gex) in C.ALIGN_GAPS and len(c.caps) == len(c.want) == len(c.full) == n
        forms.add(c.form)
        kinds.update(c.kinds)
        for k, ((r, w), (fr, fw)) in enumerate(zip(c.want, c.full)):
            statuses.add(r["status"])
            assert [r[f] for f in ("score", "q_begin", "q_end", "s_begin", "s_end")] == \
                   [fr[f] for f in ("score", "q_begin", "q_end", "s_begin", "s_end")]
            if r["status"] == A.OK:
                assert w.tolist() == fw.tolist() and len(w) <= c.caps[k] and c.rescore(c.subjects[k], c.gop, c.gex, r, w) == r["score"]
                assert C.trace_bytes(r["q_end"] - r["q_begin"], r["s_end"] - r["s_begin"]) <= c.trace
            else:
                assert len(w) == 0 and r["cigar_len"] == 0 and r["columns"] == 0
    assert forms == {"letters21", "letters25", "pssm", "pssm_cons"}
    assert statuses == {A.OK, A.EMPTY, A.NO_TRACE, A.SCORE_MISMATCH}
    assert kinds == {"planted", "relative", "repeat", "low", "empty", "random"}
