"""GPU: sw_align_hsps / sw_align_hsps_pssm (up to N non-overlapping local alignments per hit) against the scalar reference
tests/hsp_ref.c: every slot field for field, every CIGAR word for word, the unused words of the CIGAR buffer untouched;
through the C ABI, the host driver (Driver.align_hits(max_hsps=...)) and `align --maxHsps`."""
import os
import subprocess

import numpy as np
import pytest

import gpu_util as G
import hsp_abi as HA
import hsp_cases as HC
import hsp_ref as H
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    torch, capi, _ = G.gpu_modules()
    ctx = capi.Context(0)
    yield torch, capi, ctx
    ctx.close()


def run_and_check(env, case, subjects, max_hsps, min_score, gop=-11, gex=-1, where=(), **kw):
    """one call against hsp_ref and the properties of its alignments.  -> (call, want)"""
    call = HA.run(*env, case, subjects, gop, gex, max_hsps, min_score, **kw)
    want = HA.want_of(case, subjects, gop, gex, max_hsps, min_score, trace=kw.get("trace"), caps=kw.get("caps"),
                      expected=kw.get("expected"), max_len=kw.get("max_len"))
    bad = HA.check(call, want, where)
    assert bad is None, bad
    for i, s in enumerate(subjects):
        bad = HC.check_properties(case, s, gop, gex, want[i * max_hsps:(i + 1) * max_hsps])
        assert bad is None, (bad, where, i)
    return call, want


def statuses(want):
    return [r["status"] for r, _ in want]


# ---- the cases of the issue, letters and both PSSM forms ------------------------------------------------------------------

@pytest.mark.parametrize("form", HC.FORMS)
def test_three_exact_copies(env, form):
    """three alignments of one score, smallest subject end first; the fourth slot depends on min_score"""
    q, s = HC.three_copies(np.random.default_rng(24))
    case = HC.make_case(q, form)
    call, want = run_and_check(env, case, [s], 4, 1, where=(form, "min_score 1"))
    S0 = want[0][0]["score"]
    assert [r["score"] for r, _ in want[:3]] == [S0] * 3 and [r["s_begin"] for r, _ in want[:3]] == [10, 44, 78]
    assert [H.cigar_string(w) for _, w in want[:3]] == ["24="] * 3
    assert want[3][0]["status"] == H.OK and 0 < want[3][0]["score"] < S0
    call, want = run_and_check(env, case, [s], 4, S0, where=(form, "min_score S0"))
    assert statuses(want) == [H.OK] * 3 + [H.EMPTY] and [r["s_begin"] for r, _ in want[:3]] == [10, 44, 78]
    assert [int(call.res[3][f]) for f in ("score", "q_begin", "q_end", "s_begin", "s_end", "cigar_len")] == [0, -1, -1, -1, -1, 0]


@pytest.mark.parametrize("form", HC.FORMS)
def test_crossing_alignments(env, form):
    """query A B against subject B A, and two tandem repeats against three: later alignments lie above, below and across
    the earlier ones"""
    rng = np.random.default_rng(31)
    q, s = HC.swapped_domains(rng)
    _, want = run_and_check(env, HC.make_case(q, form), [s], 4, 1, where=(form, "swapped"))
    (a, _), (b, _) = want[0], want[1]
    assert a["status"] == b["status"] == H.OK
    assert (a["q_begin"] < b["q_begin"]) != (a["s_begin"] < b["s_begin"])      # the two domains, in the other order
    for gop, gex in ((-11, -1), (-5, -5)):
        q, s = HC.tandem(rng)
        _, want = run_and_check(env, HC.make_case(q, form), [s], 5, 1, gop, gex, where=(form, "tandem", gop, gex))
        assert statuses(want)[:4] == [H.OK] * 4


@pytest.mark.parametrize("form", HC.FORMS[:2])
@pytest.mark.parametrize("qlen", [8, 9, 511, 512, 513, 520])
def test_used_pairs_at_the_borders(env, form, qlen):
    """used pairs in a lane's first and last row, in lane 0 and lane 63, in column 0 and the last column, across rows
    511 / 512, seen by the reverse and the trace pass at other lane offsets than by the local pass"""
    rng = np.random.default_rng(qlen)
    q = rng.integers(0, 20, qlen).astype(np.int8)
    subjects = HC.border_subjects(rng, q)
    _, want = run_and_check(env, HC.make_case(q, form), subjects, 4, 1, where=(form, qlen))
    first = [want[4 * i][0] for i in range(len(subjects))]
    assert all(r["status"] == H.OK for r, _ in want)
    # begins and ends that are no multiples of 8, behind which further rounds run
    assert any(r["q_begin"] % 8 for r, _ in want[0:3]) and any(r["q_end"] % 8 for r, _ in want[0:3])
    assert (first[1]["q_begin"], first[1]["q_end"]) == (0, qlen)
    rows0 = {i for r, w in want[0:4] for i, _ in H.pairs(r, w)}
    cols0 = {j for r, w in want[0:4] for _, j in H.pairs(r, w)}
    assert {0, qlen - 1} <= rows0 and {0, len(subjects[0]) - 1} <= cols0
    if qlen > 512:
        assert all(r["q_begin"] <= 511 and r["q_end"] >= 513 for r, _ in want[8:10])     # across rows 511 / 512


@pytest.mark.parametrize("form", HC.FORMS[:2])
def test_three_stripe_query(env, form):
    q, s = HC.three_stripes(np.random.default_rng(1100))
    _, want = run_and_check(env, HC.make_case(q, form), [s], 3, 1, where=(form,))
    assert statuses(want) == [H.OK] * 3
    assert sorted(r["q_begin"] >= 1024 for r, _ in want[:2]) == [False, True]     # one hit inside the last stripe only


def test_pssm_forms_give_the_letter_records(env):
    """the PSSM of a letter query with the letters as the consensus gives the letter form's bytes; a built PSSM runs with and
    without a caller consensus"""
    rng = np.random.default_rng(77)
    q, s = HC.tandem(rng, unit=41, nq=3, ns=4)
    subjects = [s, HC.three_copies(rng, 30)[1]]
    a = HA.run(*env, HC.make_case(q, "letters"), subjects, -11, -1, 4, 1)
    b = HA.run(*env, HC.make_case(q, "pssm"), subjects, -11, -1, 4, 1)
    assert a.raw == b.raw and a.cigar.tolist() == b.cigar.tolist()
    import align_cases as C
    p = C.random_pssm(rng, 130)
    cons = C.consensus_codes(p)
    sub = [np.concatenate([HC.spacer(rng), cons[5:90], HC.spacer(rng), HC.mutated(rng, cons[20:120]), HC.spacer(rng), cons[60:128]])]
    other = cons.copy()
    other[::3] = (other[::3] + 1) % 20
    for consensus in (None, cons, other):
        run_and_check(env, C.Case(pssm=p, consensus=consensus), sub, 4, 1, where=("built", consensus is None))


@pytest.mark.parametrize("form", HC.FORMS[:2])
def test_max_hsps_1_is_the_plain_call(env, form):
    rng = np.random.default_rng(5)
    q = rng.integers(0, 20, 530).astype(np.int8)
    subjects = HC.border_subjects(rng, q) + [np.full(30, 20, dtype=np.int8)]
    case = HC.make_case(q, form)
    a = HA.run(*env, case, subjects, -11, -1, 1, 1, plain=True)
    for min_score in (1, 10 ** 6):     # min_score does not apply to slot 0
        b = HA.run(*env, case, subjects, -11, -1, 1, min_score)
        assert a.raw == b.raw and a.cigar.tolist() == b.cigar.tolist() and a.need == b.need
    bad = HA.check(b, HA.want_of(case, subjects, -11, -1, 1, 1))
    assert bad is None, bad


# ---- statuses ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def status_case():
    rng = np.random.default_rng(91)
    q = rng.integers(0, 20, 140).astype(np.int8)
    big = np.concatenate([HC.spacer(rng), q[10:130], HC.spacer(rng), HC.mutated(rng, q, 0.1), HC.spacer(rng)])   # slot 1 is larger than slot 0
    empty = np.full(50, 20, dtype=np.int8)
    return HC.make_case(q, "letters"), [big, empty, np.concatenate([q[:60], HC.spacer(rng), q[:60]])]


def test_trace_budgets(env, status_case):
    """A budget too small for slot 0 gives NO_TRACE, NOT_COMPUTED, ...; one that holds slot 0's rectangle but not slot 1's
    gives OK, NO_TRACE, NOT_COMPUTED.  "Too small" is one 256-byte step: a rectangle's need is a multiple of 256 bytes and
    sw_align_args::trace_bytes is rounded up to one (as in sw_align_hits), so a budget a single word short is the same budget."""
    import align_cases as C
    case, subjects = status_case
    full = HA.want_of(case, subjects, -11, -1, 3, 1)
    need = [C.trace_bytes(r["q_end"] - r["q_begin"], r["s_end"] - r["s_begin"]) for r, _ in full[:2]]
    assert need[0] < need[1]
    # one 256-byte step (a step of the budget's arithmetic) under slot 0's rectangle
    _, want = run_and_check(env, case, subjects[:1], 3, 1, trace=need[0] - 256, where="under slot 0")
    assert statuses(want) == [H.NO_TRACE, H.NOT_COMPUTED, H.NOT_COMPUTED]
    # enough for slot 0's rectangle, not for slot 1's
    call, want = run_and_check(env, case, subjects[:1], 3, 1, trace=need[1] - 256, where="under slot 1")
    assert statuses(want) == [H.OK, H.NO_TRACE, H.NOT_COMPUTED]
    assert [int(call.res[2][f]) for f in ("score", "q_begin", "q_end", "s_begin", "s_end", "cigar_len")] == [0, -1, -1, -1, -1, 0]
    _, want = run_and_check(env, case, subjects[:1], 3, 1, trace=need[1], where="exact")
    assert statuses(want) == [H.OK] * 3
    # the documented rounding: trace_bytes counts in steps of 256 bytes, so one word less than slot 0's need is slot 0's need
    call = HA.run(*env, case, subjects[:1], -11, -1, 3, 1, trace=need[0] - 4)
    exact = HA.run(*env, case, subjects[:1], -11, -1, 3, 1, trace=need[0])
    assert int(call.res[0]["status"]) == H.OK and call.raw == exact.raw and call.need == exact.need


def test_cigar_slot_too_small(env, status_case):
    case, subjects = status_case
    full = HA.want_of(case, subjects, -11, -1, 3, 1)
    caps = np.repeat([case.qlen + len(s) for s in subjects], 3)
    caps[0], caps[1] = full[0][0]["cigar_len"], full[1][0]["cigar_len"] - 1     # slot 0 exactly, slot 1 one word short
    caps[6] = 0
    assert full[1][0]["cigar_len"] >= 3
    _, want = run_and_check(env, case, subjects, 3, 1, caps=caps, where="caps")
    assert statuses(want)[:3] == [H.OK, H.NO_TRACE, H.NOT_COMPUTED] and statuses(want)[6:] == [H.NO_TRACE, H.NOT_COMPUTED, H.NOT_COMPUTED]


def test_expected_scores_empty_pairs_and_long_subjects(env, status_case):
    case, subjects = status_case
    full = HA.want_of(case, subjects, -11, -1, 3, 1)
    exp = [full[0][0]["score"] + 1, 0, full[6][0]["score"]]
    call, want = run_and_check(env, case, subjects, 3, 1, expected=exp, where="expected")
    assert statuses(want) == [H.SCORE_MISMATCH, H.NOT_COMPUTED, H.NOT_COMPUTED] + [H.EMPTY] * 3 + [H.OK] * 3
    assert int(call.res[0]["q_begin"]) == full[0][0]["q_begin"] and int(call.res[0]["score"]) == full[0][0]["score"]
    # a subject over max_subject_len
    bound = len(subjects[2])
    assert len(subjects[0]) > bound >= len(subjects[1])
    _, want = run_and_check(env, case, subjects, 3, 1, max_len=bound, where="max_len")
    assert statuses(want)[:3] == [H.BAD_LENGTH, H.NOT_COMPUTED, H.NOT_COMPUTED] and statuses(want)[6:] == [H.OK] * 3


def test_no_pairs_and_chunks(env, status_case):
    torch, capi, ctx = env
    case, subjects = status_case
    call = HA.run(*env, case, [], -11, -1, 3, 1)
    assert call.need == 0 and set(call.raw) == {HA.RESULT_FILL} and call.cigar.tolist() == [HA.SENTINEL]
    # scratch for one pair only: the call runs in chunks and gives the one-chunk result
    import align_cases as C
    one, want = run_and_check(env, case, subjects, 3, 1, where="one chunk")
    trace = max(C.trace_bytes(case.qlen, len(s)) for s in subjects)
    slot = C.slot_bytes(max(len(s) for s in subjects), trace) + HA.used_bytes(case.qlen, 3)
    assert one.need == 3 * slot
    chunked = HA.run(*env, case, subjects, -11, -1, 3, 1, temp_bytes=slot + 100)
    assert chunked.raw == one.raw and chunked.cigar.tolist() == one.cigar.tolist()
    with pytest.raises(capi.SwError) as e:
        HA.run(*env, case, subjects, -11, -1, 3, 1, temp_bytes=slot - 1)
    assert e.value.code == -5


def test_refused_arguments(env, status_case):
    torch, capi, ctx = env
    case, subjects = status_case
    for kw, word in ((dict(max_hsps=0), "max_hsps"), (dict(max_hsps=17), "max_hsps"), (dict(max_hsps=2, min_score=0), "min_score"),
                     (dict(max_hsps=2, flags=capi.ALIGN_COORDS_ONLY), "SW_ALIGN_COORDS_ONLY"),
                     (dict(max_hsps=2, phase_events=[0, 0, 0, 0]), "phase_events")):
        with pytest.raises(capi.SwError) as e:
            capi.align_hsps(ctx, 0, 10, 1, 0, 0, 0, 100, -11, -1, 0, **kw)
        assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))


# ---- the host driver and the command line --------------------------------------------------------------------------------------

LETTERS = "ARNDCQEGHILKMFPSTWYV"
GOLDEN_DB = os.path.join(O.GOLDEN_DIR, "allqueries_db", "aq")
FASTA = os.path.join(O.GOLDEN_DIR, "allqueries.fasta")
MIN_SCORE = 25


@pytest.fixture(scope="module")
def planted_db():
    """two queries and a small DB: random subjects, and for every query subjects with several copies of pieces of it"""
    rng = np.random.default_rng(404)
    queries = [rng.integers(0, 20, n).astype(np.int8) for n in (90, 530)]
    seqs = [rng.integers(0, 20, int(n)).astype(np.int8) for n in rng.integers(40, 500, 300)]
    for q in queries:
        for _ in range(6):
            a = int(rng.integers(0, len(q) - 40))
            b = int(rng.integers(a + 30, len(q) + 1))
            seqs.append(np.concatenate([HC.spacer(rng, 12), q[a:b], HC.spacer(rng, 20), HC.mutated(rng, q[a:b]), HC.spacer(rng, 7),
                                        HC.mutated(rng, q, 0.2)]))
    seqs.sort(key=len)
    return queries, seqs, O.make_db(seqs)


@pytest.mark.parametrize("mode", ["resident", "streamed"])
def test_driver_align_hits_with_max_hsps(planted_db, mode):
    from cudasw4_amd import capi, driver
    queries, seqs, db = planted_db
    kw = dict(max_gpu_mem=1, max_batch_bytes=200_000) if mode == "streamed" else {}
    d = driver.Driver(devices=[0], num_top=8, kinds=(0, 0, 3, 3), **kw)
    d.db_from_arrays(*db)
    d.upload()
    try:
        for q in queries:
            letters = "".join(LETTERS[c] for c in q)
            r = d.scan(letters)
            plain, plain_cigars = d.align_hits(letters, r)
            lists = d.align_hits(letters, r, max_hsps=3, min_score=MIN_SCORE)
            assert len(lists) == len(r["ids"]) == 8
            case, several = HC.make_case(q), 0
            for k, hit in enumerate(lists):
                want = HC.reference(case, seqs[int(r["ids"][k])], -11, -1, 3, MIN_SCORE)
                want = want[:1] + [x for x in want[1:] if x[0]["status"] == H.OK]
                assert [{f: int(rec[f]) for f in H.FIELDS} for rec, _ in hit] == [x[0] for x in want], (mode, k)
                assert [c for _, c in hit] == [H.cigar_string(x[1]) or "*" for x in want]
                assert hit[0][0].tobytes()[:48] == plain[k].tobytes()[:48] and hit[0][1] == plain_cigars[k]
                several += len(hit) > 1
            assert several >= 4
            one, one_cigars = d.align_hits(letters, r, max_hsps=1)
            assert one.tobytes() == plain.tobytes() and one_cigars == plain_cigars
        # the PSSM form of the last query gives the same lists
        from cudasw4_amd import pssm
        p = pssm.from_sequence(queries[-1], O.blosum21(62))
        rp = d.scan_pssm(p)
        assert rp["ids"].tolist() == r["ids"].tolist()
        plists = d.align_hits_pssm(p, rp, consensus=letters, max_hsps=3, min_score=MIN_SCORE)
        assert [[(rec.tobytes()[:48], c) for rec, c in hit] for hit in plists] == [[(rec.tobytes()[:48], c) for rec, c in hit] for hit in lists]
    finally:
        d.close()


def run_align(tmp_path, name, *extra):
    """`align` for the first three golden queries (144, 189 and 222 residues) against the golden DB -> the output file's text"""
    from cudasw4_amd import driver
    headers, letters = O.read_fasta(FASTA)
    fasta, of = str(tmp_path / "three.fasta"), str(tmp_path / name)
    with open(fasta, "w") as f:
        for h, l in list(zip(headers, letters))[:3]:
            f.write(">%s\n%s\n" % (h, l.decode()))
    p = subprocess.run([driver.ALIGN, "--query", fasta, "--db", GOLDEN_DB, "--top", "3", "--of", of] + list(extra),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return open(of).read()


def test_align_cli_tsv_with_max_hsps(tmp_path):
    _, letters = O.read_fasta(FASTA)
    flags = ["--tsv", "--alignments", "--maxHsps", "3", "--hspMinScore", str(MIN_SCORE)]
    for evalues in (False, True):
        lines = run_align(tmp_path, "hsps.tsv", *(flags + (["--evalues"] if evalues else []))).splitlines()
        head = lines[0].split("\t")
        assert head[8:17] == ["Query begin", "Query end", "Reference begin", "Reference end", "Alignment length", "Identities",
                              "Gap opens", "CIGAR", "HSP"] and head[17:] == (["Z-score", "E-value"] if evalues else [])
        rows = [l.split("\t") for l in lines[1:]]
        firsts = [r for r in rows if r[16] == "1"]
        assert len(firsts) == 3 * 3
        further, at = 0, 0
        while at < len(rows):
            first = rows[at]
            case = HC.make_case(O.encode(letters[int(first[0])]))
            want = HC.reference(case, O.encode(letters[int(first[7])]), -11, -1, 3, MIN_SCORE)
            want = want[:1] + [x for x in want[1:] if x[0]["status"] == H.OK]
            for k, (r, w) in enumerate(want):
                row = rows[at + k]
                assert row[:4] == first[:4] and row[5:8] == first[5:8] and int(row[16]) == k + 1, (at, k, row)
                assert [int(x) for x in [row[4]] + row[8:15]] == [r["score"], r["q_begin"] + 1, r["q_end"], r["s_begin"] + 1, r["s_end"],
                                                                 r["columns"], r["identities"], r["gap_opens"]], (at, k, row)
                assert row[15] == (H.cigar_string(w) or "*")
                if evalues:      # 20 subjects allow no fit: no statistics for any alignment
                    assert row[17:] == ["*", "*"]
            further += len(want) - 1
            at += len(want)
        assert further >= 5


def test_align_cli_plain_and_max_hsps_1(tmp_path):
    base = run_align(tmp_path, "base.tsv", "--alignments", "--tsv")
    assert run_align(tmp_path, "one.tsv", "--alignments", "--tsv", "--maxHsps", "1") == base and base.count("\n") == 1 + 3 * 3   # byte for byte
    base = run_align(tmp_path, "base.out", "--alignments")
    lines = run_align(tmp_path, "plain.out", "--alignments", "--maxHsps", "3", "--hspMinScore", str(MIN_SCORE)).splitlines()
    extra = [l for l in lines if l.startswith("Alignment ") and "." in l.split()[1][:-1]]
    assert [l for l in lines if l not in extra] == base.splitlines() and len(extra) >= 5
    _, letters = O.read_fasta(FASTA)
    query, result = -1, None
    for l in lines:
        if l.startswith("Query "):
            query = int(l.split(",")[0].split()[1])
        elif l.startswith("Result "):
            result = l
        elif l in extra:
            i, k = (int(x) for x in l.split()[1][:-1].split("."))
            assert result.startswith("Result %d." % i)
            ref = int(result.rsplit("referenceId ", 1)[1])
            r, w = HC.reference(HC.make_case(O.encode(letters[query])), O.encode(letters[ref]), -11, -1, 3, MIN_SCORE)[k - 1]
            assert l == "Alignment %d.%d. Score %d. Query %d-%d. Reference %d-%d. Length %d. Identities %d. Gap opens %d. CIGAR %s" % (
                i, k, r["score"], r["q_begin"] + 1, r["q_end"], r["s_begin"] + 1, r["s_end"], r["columns"], r["identities"],
                r["gap_opens"], H.cigar_string(w))


def test_align_cli_pssm_queries_and_iterations(tmp_path):
    """--pssmAlignments --maxHsps for a --pssm query (the PSSM of golden query 1 with its letters as the residue column) against
    hsp_ref's PSSM form, and --iterations with --maxHsps: the first alignments are the ones printed without --maxHsps"""
    from cudasw4_amd import pssm
    _, letters = O.read_fasta(FASTA)
    f = str(tmp_path / "q1.pssm")
    pssm.write_ascii(f, pssm.from_sequence(O.encode(letters[1]), O.blosum21(62)), consensus=letters[1].decode())
    hsps = ["--maxHsps", "3", "--hspMinScore", str(MIN_SCORE)]
    rows = lambda text: [l.split("\t") for l in text.splitlines()[1:]]
    b = rows(run_align(tmp_path, "pssm.tsv", "--tsv", "--pssmAlignments", "--pssm", f, *hsps))
    import align_cases as C
    p, cons = pssm.read_ascii(f)                 # (column 20 is the reader's -1, not the table's score against "other")
    case = C.Case(pssm=p, consensus=O.encode(cons.encode()))
    assert len(b) > 3 * 3 + 3
    at = [r[2] for r in b].index(b[-1][2])       # inputs are processed in the order given: the query file, then the PSSM
    assert at >= 3 * 3 and b[at - 1][0] == "2"
    for result in range(3):      # the PSSM is query 0 of its own "file": three results with their further alignments
        first = b[at]
        assert (first[0], int(first[1]), int(first[3])) == ("0", len(letters[1]), result)
        want = HC.reference(case, O.encode(letters[int(first[7])]), -11, -1, 3, MIN_SCORE)
        want = want[:1] + [x for x in want[1:] if x[0]["status"] == H.OK]
        for k, (r, w) in enumerate(want):
            row = b[at + k]
            assert [int(x) for x in [row[4]] + row[8:15] + [row[16]]] == [r["score"], r["q_begin"] + 1, r["q_end"], r["s_begin"] + 1,
                                                                         r["s_end"], r["columns"], r["identities"], r["gap_opens"], k + 1]
            assert row[15] == (H.cigar_string(w) or "*") and row[:4] == first[:4]
        at += len(want)
    assert at == len(b)
    one = rows(run_align(tmp_path, "it1.tsv", "--tsv", "--alignments", "--iterations", "2", "--inclusionScore", "40"))
    more = rows(run_align(tmp_path, "it3.tsv", "--tsv", "--alignments", "--iterations", "2", "--inclusionScore", "40", *hsps))
    assert [r[:16] for r in more if r[16] == "1"] == one and len(more) > len(one)
    for r in more:      # further alignments: not above the first one's score, in the result's own lines
        if r[16] != "1":
            first = [x for x in more if x[:4] == r[:4] and x[16] == "1"][0]
            assert MIN_SCORE <= int(r[4]) <= int(first[4]) and r[5:8] == first[5:8]


# ---- E-values of further alignments, on a DB that allows a fit -------------------------------------------------------------------

@pytest.fixture(scope="module")
def fitted_db(tmp_path_factory):
    """a Swiss-Prot-like DB of 3000 subjects as dbdata files, golden query 2 (222 residues), and its scan with the statistics on"""
    from cudasw4_amd import driver, synthdb
    tmp = tmp_path_factory.mktemp("fitted")
    chars, offsets, lengths = synthdb.sprot_like(n=3000, max_len=8000)
    lut = np.frombuffer(LETTERS.encode() + b"X", dtype=np.uint8)
    fasta, prefix, qfile = str(tmp / "db.fa"), str(tmp / "sp"), str(tmp / "q.fa")
    with open(fasta, "w") as f:
        for i in range(len(lengths)):
            o = int(offsets[i])
            f.write(">s%d\n%s\n" % (i, lut[chars[o:o + int(lengths[i])]].tobytes().decode()))
    p = subprocess.run([driver.MAKEDB, fasta, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    _, letters = O.read_fasta(FASTA)
    with open(qfile, "w") as f:
        f.write(">query\n%s\n" % letters[2].decode())
    d = driver.Driver(devices=[0], num_top=10)
    d.open_db(prefix)
    d.set_statistics(True)
    r = d.scan(letters[2].decode())
    reflen = {int(i): d.reference_length(int(i)) for i in r["ids"]}
    d.close()
    assert r["stats"]["status"] == driver.STATS_OK
    return dict(prefix=prefix, qfile=qfile, scan=r, reflen=reflen, tmp=tmp)


def test_align_cli_evalues_of_further_alignments(fitted_db):
    """TSV and plain output with --maxHsps 3 --evalues where the scan allows a fit: the first line of a result carries the
    result's Z-score and E-value, every further line the query's fit applied to ITS score and the subject's length"""
    from cudasw4_amd import driver, stats
    r, st = fitted_db["scan"], fitted_db["scan"]["stats"]
    text = lambda score, length: tuple(f % v[0] for f, v in zip(("%.2f", "%.3g"), stats.evalues(st, [score], [length])))

    def run(name, *extra):
        of = str(fitted_db["tmp"] / name)
        p = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", fitted_db["qfile"], "--db", fitted_db["prefix"],
                            "--top", "10", "--of", of, "--alignments", "--maxHsps", "3", "--hspMinScore", "20", "--evalues"] + list(extra),
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        return open(of).read().splitlines()

    lines = run("e.tsv", "--tsv")
    assert lines[0].split("\t")[16:] == ["HSP", "Z-score", "E-value"]
    rows = [l.split("\t") for l in lines[1:]]
    firsts = [x for x in rows if x[16] == "1"]
    assert [int(x[4]) for x in firsts] == r["scores"].tolist() and [int(x[7]) for x in firsts] == r["ids"].tolist()
    assert [x[17] for x in firsts] == ["%.2f" % z for z in r["zscores"]] and [x[18] for x in firsts] == ["%.3g" % e for e in r["evalues"]]
    further = [x for x in rows if x[16] != "1"]
    assert len(further) >= 5
    differ = 0
    for x in further:
        first = [y for y in firsts if y[3] == x[3]][0]
        assert (x[17], x[18]) == text(int(x[4]), fitted_db["reflen"][int(x[7])]), x
        assert int(x[4]) <= int(first[4]) and int(x[5]) == fitted_db["reflen"][int(x[7])]
        if int(x[4]) < int(first[4]):     # its own score, not the result's: a lower Z-score and a larger E-value
            assert float(x[17]) < float(first[17]) and float(x[18]) > float(first[18]) and (x[17], x[18]) != (first[17], first[18])
            differ += 1
    assert differ >= 5
    # plain output: the same values on the Alignment i.k lines, the result's own on the Result lines
    plain = run("e.txt")
    extra = [l for l in plain if l.startswith("Alignment ") and "." in l.split()[1][:-1]]
    assert len(extra) == len(further)
    for l, x in zip(extra, further):
        assert l.startswith("Alignment %s.%s. Score %s. " % (x[3], x[16], x[4])) and l.endswith(" Z-score: %s E-value: %s" % (x[17], x[18])), (l, x)
    results = [l for l in plain if l.startswith("Result ")]
    assert [l.rsplit(" Z-score: ", 1)[1] for l in results] == ["%s E-value: %s" % (y[17], y[18]) for y in firsts]


def test_align_cli_out_pssm_is_built_from_the_first_alignments(fitted_db):
    """--outPssm with --maxHsps 3: the builder reads the first alignments the aligner left on the device among the 3 slots of
    every hit (HitAligner::resident()), so the PSSM written is byte for byte the one written without --maxHsps"""
    from cudasw4_amd import driver
    out = {}
    for name, extra in (("plain", []), ("hsps", ["--maxHsps", "3", "--hspMinScore", "20"])):
        prefix = str(fitted_db["tmp"] / ("built_" + name))
        p = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", fitted_db["qfile"], "--db", fitted_db["prefix"],
                            "--top", "40", "--tsv", "--of", prefix + ".tsv", "--alignments", "--iterations", "2", "--inclusionScore", "60",
                            "--outPssm", prefix] + extra, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        out[name] = (open(prefix + ".0.pssm").read(), [l.split("\t") for l in open(prefix + ".tsv").read().splitlines()[1:]])
    assert out["hsps"][0] == out["plain"][0] and len(out["plain"][0].splitlines()) > 222
    assert [x[:16] for x in out["hsps"][1] if x[16] == "1"] == out["plain"][1] and len(out["hsps"][1]) > len(out["plain"][1])
