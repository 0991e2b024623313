"""GPU: sw_align_hits_pssm (coordinates, counts and CIGAR of the hits of a PSSM query) against the scalar reference
tests/pssm_align_ref.c, field for field; through the C ABI, the host driver (Driver.align_hits_pssm) and
`align --pssmAlignments`."""
import os
import subprocess

import numpy as np
import pytest

import align_ref as A
import gpu_util as G
import oracle_lib as O
import pssm_align_ref as PA

pytestmark = pytest.mark.gpu

GAPS = [(-11, -1), (-5, -5)]
QLENS = [1, 2, 8, 9, 63, 64, 65, 511, 512, 513, 1030]


@pytest.fixture(scope="module")
def env():
    torch, capi, _ = G.gpu_modules()
    ctx = capi.Context(0)   # (no sw_set_matrix: the PSSM form needs none)
    yield torch, capi, ctx
    ctx.close()


def random_pssm(rng, qlen):
    """position-specific scores with a negative mean (-9 .. 3) and one favoured residue per row (5 .. 12), so that
    alignments stay local; column 20 negative"""
    p = rng.integers(-9, 4, (qlen, 21)).astype(np.int8)
    p[np.arange(qlen), rng.integers(0, 20, qlen)] = rng.integers(5, 13, qlen)
    p[:, 20] = -1 - rng.integers(0, 4, qlen)
    return p


def codes_of_consensus(p):
    return np.argmax(np.asarray(p)[:, :20], axis=1).astype(np.int8)


def gpu_align(env, subjects, gop, gex, pssm=None, consensus=None, query=None, table=None, expected=None, trace_bytes=None,
              flags=0, temp_bytes=None):
    """pssm (+ consensus codes or None): sw_align_hits_pssm; query + table: sw_align_hits.
    -> (structured results, list of CIGAR word arrays)"""
    torch, capi, ctx = env
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    chars, offsets, lengths = O.make_db(subjects)
    n = len(subjects)
    qlen = len(pssm) if pssm is not None else len(query)
    coff = np.zeros(n + 1, dtype=np.int64)
    coff[1:] = np.cumsum(qlen + lengths.astype(np.int64))
    dch, doff, dlen, dcoff = dev(chars), dev(offsets.view(np.int64)), dev(lengths), dev(coff)
    dt = capi.align_result_dtype()
    dres = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda")
    dcig = torch.zeros(max(int(coff[-1]), 1), dtype=torch.int32, device="cuda")
    dexp = dev(np.asarray(expected, dtype=np.int32)) if expected is not None else None
    tb = trace_bytes if trace_bytes is not None else max(capi.align_trace_bytes(qlen, int(L)) for L in lengths)
    maxlen = int(lengths.max())
    kw = dict(expected_scores=dexp.data_ptr() if dexp is not None else 0, flags=flags, trace_bytes=tb)
    if pssm is not None:
        dp = dev(np.ascontiguousarray(pssm, dtype=np.int8).reshape(-1))
        dc = dev(np.ascontiguousarray(consensus, dtype=np.int8)) if consensus is not None else None

        def call(**more):
            return capi.align_hits_pssm(ctx, dp.data_ptr(), dc.data_ptr() if dc is not None else 0, qlen, n, dch.data_ptr(),
                                        doff.data_ptr(), dlen.data_ptr(), maxlen, gop, gex, dres.data_ptr(), dcig.data_ptr(),
                                        dcoff.data_ptr(), **kw, **more)
    else:
        ctx.set_matrix(table)
        dq = dev(np.ascontiguousarray(query, dtype=np.int8))

        def call(**more):
            return capi.align_hits(ctx, dq.data_ptr(), qlen, n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(), maxlen, gop,
                                   gex, dres.data_ptr(), dcig.data_ptr(), dcoff.data_ptr(), **kw, **more)
    need = call()
    temp = torch.empty(temp_bytes or need, dtype=torch.uint8, device="cuda")
    call(temp=temp.data_ptr(), temp_bytes=temp.numel())
    torch.cuda.synchronize()
    res = np.frombuffer(dres.cpu().numpy().tobytes(), dtype=dt).copy()
    cig = dcig.cpu().numpy().view(np.uint32)
    words = [cig[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])].copy() for r in res]
    return res, words, need


def check_against_reference(p, cons, subjects, res, words, gop, gex, coords_only=False, trace_bytes=None):
    from cudasw4_amd import capi
    for k, s in enumerate(subjects):
        want, wcig = PA.align(p, s, cons, gop, gex, coords_only=coords_only)
        if trace_bytes is not None and want["status"] == A.OK and not coords_only:
            if capi.align_trace_bytes(want["q_end"] - want["q_begin"], want["s_end"] - want["s_begin"]) > trace_bytes:
                want = dict(want, status=A.NO_TRACE, columns=0, identities=0, mismatches=0, gap_opens=0, gap_columns=0,
                            cigar_len=0)
                wcig = wcig[:0]
        got = {f: int(res[k][f]) for f in A.FIELDS}
        assert got == want, (k, len(p), len(s), gop, gex, got, want)
        assert words[k].tolist() == wcig.tolist(), (k, A.cigar_string(words[k]), A.cigar_string(wcig))


def shape_subjects(rng, cons):
    """lengths 1, 2, 3, 17, 64, 65, 500; two relatives of the whole consensus and one of an infix that starts and ends off
    the multiples of 8, so that the reverse and the trace pass see rows that do not line up with the tile"""
    qlen = len(cons)
    subjects = [rng.integers(0, 21, int(L)).astype(np.int8) for L in (1, 2, 3, 17, 64, 65, 500)]
    subjects += G.relatives(rng, cons, 2, max(qlen, 2), qlen + 300)
    lo = min(3, qlen - 1)
    hi = max(lo + 1, qlen - 5 if (qlen - 5) % 8 else qlen - 6)
    assert qlen < 16 or (lo % 8 and hi % 8)
    infix = cons[lo:hi]
    other = lambda n: np.full(n, 20, dtype=np.int8)   # flanks that no row scores above zero: the alignment is the infix
    subjects += [np.concatenate([other(11), infix, other(6)])]
    return subjects


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("qlen", QLENS)
def test_pair_shapes(env, qlen, gaps):
    gop, gex = gaps
    rng = np.random.default_rng(1000 * qlen - gop)
    p = random_pssm(rng, qlen)
    cons = codes_of_consensus(p)
    subjects = shape_subjects(rng, cons)
    res, words, _ = gpu_align(env, subjects, gop, gex, pssm=p)
    check_against_reference(p, None, subjects, res, words, gop, gex)
    if qlen >= 8:   # (the inputs do what they are meant to: the infix's rows start and end off the tile's rows of 8)
        want = PA.align(p, subjects[-1], None, gop, gex)[0]
        assert want["status"] == A.OK and want["q_begin"] % 8 != 0 and want["q_end"] % 8 != 0, want


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("qlen", [300, 513])
def test_from_sequence_equals_the_letter_form(env, qlen, full):
    from cudasw4_amd import driver, pssm
    rng = np.random.default_rng(qlen + full)
    if full:
        table, alpha = driver.matrix25(62), 25
    else:
        table, alpha = O.blosum21(62), 21
    q = rng.integers(0, alpha, qlen).astype(np.int8)
    if full:
        q[::7] = 24
    subjects = G.relatives(rng, np.minimum(q, 19).astype(np.int8), 4, qlen, qlen + 300)
    subjects += [rng.integers(0, 21, 600).astype(np.int8), np.full(30, 20, dtype=np.int8), q[40:200].copy() % 21]
    for gop, gex in GAPS:
        letter, lw, need_l = gpu_align(env, subjects, gop, gex, query=q, table=table)
        prof, pw, need_p = gpu_align(env, subjects, gop, gex, pssm=pssm.from_sequence(q, table), consensus=q)
        assert prof.tobytes() == letter.tobytes() and need_p == need_l
        assert all(a.tolist() == b.tolist() for a, b in zip(pw, lw))
        assert (letter["status"] == A.OK).sum() >= 5


def test_position_specificity(env):
    """two halves with one consensus and different rows: no table indexed by a letter gives these alignments"""
    rng = np.random.default_rng(8)
    half = 150
    cons = rng.integers(0, 20, half).astype(np.int8)
    sharp = np.full((half, 21), -6, dtype=np.int8)
    sharp[np.arange(half), cons] = 11
    flat = np.full((half, 21), -1, dtype=np.int8)
    flat[np.arange(half), cons] = 2
    p = np.concatenate([sharp, flat])
    p[:, 20] = -1
    full = np.concatenate([cons, cons])
    subjects = G.relatives(rng, full, 3, 2 * half, 2 * half + 200) + G.relatives(rng, cons, 2, half, half + 100)
    res, words, _ = gpu_align(env, subjects, -11, -1, pssm=p, consensus=full)
    check_against_reference(p, full, subjects, res, words, -11, -1)
    # the same subjects under a PSSM whose rows depend on the consensus letter alone (what a table gives) align differently
    table_like = np.concatenate([sharp, sharp])
    res2, words2, _ = gpu_align(env, subjects, -11, -1, pssm=table_like, consensus=full)
    check_against_reference(table_like, full, subjects, res2, words2, -11, -1)
    coords = lambda r: [(int(x["q_begin"]), int(x["q_end"]), int(x["s_begin"]), int(x["s_end"])) for x in r]
    assert coords(res2) != coords(res) and res2["score"].tolist() != res["score"].tolist()


@pytest.mark.parametrize("supplied", [False, True])
def test_extreme_entries(env, supplied):
    rng = np.random.default_rng(12 + supplied)
    qlen = 530
    p = random_pssm(rng, qlen)
    rows = rng.choice(qlen, 60, replace=False)
    p[rows[:30], rng.integers(0, 20, 30)] = 127
    p[rows[30:], rng.integers(0, 20, 30)] = -128
    p[rows[10:20], rng.integers(0, 20, 10)] = -128
    cons = codes_of_consensus(p)
    given = None
    if supplied:
        given = cons.copy()
        given[::5] = 20          # "other": identical to nothing
        given[1::11] = 24
    subjects = G.relatives(rng, cons, 4, qlen, qlen + 200) + [rng.integers(0, 21, 300).astype(np.int8)]
    res, words, _ = gpu_align(env, subjects, -11, -1, pssm=p, consensus=given)
    check_against_reference(p, given, subjects, res, words, -11, -1)
    assert int(res["score"].max()) > 127 * 10


def test_statuses_and_chunks(env):
    from cudasw4_amd import capi
    rng = np.random.default_rng(5)
    qlen = 600
    p = random_pssm(rng, qlen)
    cons = codes_of_consensus(p)
    subjects = G.relatives(rng, cons, 5, 600, 2000) + [np.full(50, 20, dtype=np.int8)] + G.relatives(rng, cons[:100], 1, 100, 150)
    ref = [PA.align(p, s, None, -11, -1)[0] for s in subjects]
    assert ref[5]["status"] == A.EMPTY and all(r["status"] == A.OK for i, r in enumerate(ref) if i != 5)
    # a budget that fits the smallest rectangle only: exact coordinates, no CIGAR, for the others
    small = capi.align_trace_bytes(ref[6]["q_end"] - ref[6]["q_begin"], ref[6]["s_end"] - ref[6]["s_begin"])
    res, words, _ = gpu_align(env, subjects, -11, -1, pssm=p, trace_bytes=small)
    check_against_reference(p, None, subjects, res, words, -11, -1, trace_bytes=small)
    assert [int(r["status"]) for r in res] == [A.NO_TRACE] * 5 + [A.EMPTY, A.OK]
    # coordinates only
    res, words, _ = gpu_align(env, subjects, -11, -1, pssm=p, flags=capi.ALIGN_COORDS_ONLY)
    check_against_reference(p, None, subjects, res, words, -11, -1, coords_only=True)
    # expected scores: one wrong entry flags that pair only
    exp = [r["score"] for r in ref]
    exp[2] += 1
    res, words, _ = gpu_align(env, subjects, -11, -1, pssm=p, expected=exp)
    assert [int(r["status"]) for r in res] == [0, 0, A.SCORE_MISMATCH, 0, 0, A.EMPTY, 0]
    assert res[2]["score"] == ref[2]["score"] and res[2]["q_begin"] == ref[2]["q_begin"] and res[2]["cigar_len"] == 0
    # chunks of two pairs of the seven: identical results
    whole, fw, need = gpu_align(env, subjects, -11, -1, pssm=p)
    tb = max(capi.align_trace_bytes(qlen, len(s)) for s in subjects)
    slot = (8 * (max(len(s) for s in subjects) + 1) + 255) // 256 * 256 + (tb + 255) // 256 * 256
    assert need == 7 * slot
    res, words, _ = gpu_align(env, subjects, -11, -1, pssm=p, temp_bytes=2 * slot + 100)
    assert res.tobytes() == whole.tobytes() and all(a.tolist() == b.tolist() for a, b in zip(words, fw))
    with pytest.raises(capi.SwError) as e:
        gpu_align(env, subjects[:1], -11, -1, pssm=p, temp_bytes=16)
    assert e.value.code == -5


# ---- the host driver ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synth():
    """a few thousand Swiss-Prot-like background sequences with seeded relatives of two PSSMs' consensus"""
    from cudasw4_amd import synthdb
    rng = np.random.default_rng(21)
    pssms = [random_pssm(rng, 140), random_pssm(rng, 700)]
    lengths = synthdb.sprot_like_lengths(3000, seed=8, max_len=3000)
    bg = synthdb.random_db(lengths, seed=9, composition=synthdb.SPROT_COMPOSITION)
    seqs = [bg[0][int(bg[1][i]):int(bg[1][i]) + int(bg[2][i])] for i in range(len(lengths))]
    for p in pssms:
        cons = codes_of_consensus(p)
        seqs += G.relatives(rng, cons, 12, len(cons), len(cons) + 400)
        seqs += G.relatives(rng, cons[len(cons) // 3:], 4, len(cons), len(cons) + 100)
    seqs.sort(key=len)
    return pssms, seqs, O.make_db(seqs)


def driver_alignments(synth, devices=(0,), **kw):
    from cudasw4_amd import driver, pssm
    pssms, seqs, db = synth
    d = driver.Driver(devices=list(devices), num_top=12, kinds=(0, 0, 3, 3), **kw)
    d.db_from_arrays(*db)
    d.upload()
    out = []
    for k, p in enumerate(pssms):
        r = d.scan_pssm(p)
        # (align_hits_pssm hands the scan's scores to the kernels as expected_scores: a disagreement raises)
        cons = pssm.consensus_of(p) if k else None
        res, cig = d.align_hits_pssm(p, r, consensus=cons)
        out.append((r["scores"].tolist(), r["ids"].tolist(), res.tobytes(), cig))
    d.close()
    return out


def test_driver_align_hits_pssm(synth):
    from cudasw4_amd import capi
    pssms, seqs, db = synth
    base = driver_alignments(synth)
    dt = capi.align_result_dtype()
    for k, (scores, ids, raw, cigars) in enumerate(base):
        res = np.frombuffer(raw, dtype=dt)
        assert len(res) == 12 and res["score"].tolist() == scores
        cons = codes_of_consensus(pssms[k]) if k else None
        for i in range(12):
            want, wcig = PA.align(pssms[k], seqs[ids[i]], cons, -11, -1)
            assert {f: int(res[i][f]) for f in A.FIELDS} == want, (k, i)
            assert cigars[i] == (A.cigar_string(wcig) or "*")
    assert driver_alignments(synth, devices=[0] * 8) == base
    assert driver_alignments(synth, max_gpu_mem=1, max_batch_bytes=200_000) == base


def test_driver_consensus_letters(synth):
    """non-standard consensus letters are identical to nothing; a scan score that is not the alignment's raises"""
    from cudasw4_amd import driver, pssm
    pssms, seqs, db = synth
    p = pssms[0]
    d = driver.Driver(devices=[0], num_top=3, kinds=(0, 0, 3, 3))
    d.db_from_arrays(*db)
    d.upload()
    r = d.scan_pssm(p)
    letters = list(pssm.consensus_of(p))
    m = len(letters[::4])
    letters[::4] = list(("X*-B" * m)[:m])
    letters = "".join(letters)
    res, cig = d.align_hits_pssm(p, r, consensus=letters)
    codes = O.encode(letters)
    for i in range(3):
        want, wcig = PA.align(p, seqs[int(r["ids"][i])], codes, -11, -1)
        assert {f: int(res[i][f]) for f in A.FIELDS} == want and cig[i] == A.cigar_string(wcig)
    bad = dict(r, scores=r["scores"] + 1)
    with pytest.raises(driver.DriverError):
        d.align_hits_pssm(p, bad)
    with pytest.raises(ValueError):
        d.align_hits_pssm(p, r, consensus=letters[:-1])
    d.close()


# ---- the command line --------------------------------------------------------------------------------------------------

def test_align_cli_pssm_alignments(tmp_path):
    from cudasw4_amd import driver, pssm
    rng = np.random.default_rng(31)
    p = random_pssm(rng, 210)
    p[:, 20] = pssm.OTHER_SCORE
    cons = list(pssm.consensus_of(p))
    cons[5], cons[60] = "X", "-"
    cons = "".join(cons)
    f = str(tmp_path / "fam.pssm")
    pssm.write_ascii(f, p, consensus=cons)
    prefix = os.path.join(O.GOLDEN_DIR, "allqueries_db", "aq")
    fasta = os.path.join(O.GOLDEN_DIR, "allqueries.fasta")

    def run(args, of):
        r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN] + args + ["--db", prefix, "--top", "3", "--of", of],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(of).read().splitlines()

    both = run(["--pssm", f, "--query", fasta, "--pssmAlignments", "--tsv"], str(tmp_path / "both.tsv"))
    letters = run(["--query", fasta, "--alignments", "--tsv"], str(tmp_path / "letters.tsv"))
    assert both[0] == letters[0] and both[0].split("\t")[8:] == ["Query begin", "Query end", "Reference begin", "Reference end",
                                                                  "Alignment length", "Identities", "Gap opens", "CIGAR"]
    assert both[4:] == letters[1:]           # letter queries: byte for byte the rows of --alignments
    d = driver.Driver(devices=[0], num_top=3)
    d.open_db(prefix)
    r = d.scan_pssm(p)
    res, cig = d.align_hits_pssm(p, r, consensus=cons)
    d.close()
    rows = [l.split("\t") for l in both[1:4]]
    assert all(len(x) == 16 and x[2] == "fam.pssm" for x in rows)
    for i, x in enumerate(rows):
        assert int(x[4]) == int(r["scores"][i]) == int(res[i]["score"]) and int(x[7]) == int(r["ids"][i])
        assert [int(v) for v in x[8:15]] == [int(res[i]["q_begin"]) + 1, int(res[i]["q_end"]), int(res[i]["s_begin"]) + 1,
                                             int(res[i]["s_end"]), int(res[i]["columns"]), int(res[i]["identities"]),
                                             int(res[i]["gap_opens"])]
        assert x[15] == cig[i]
    # plain mode: one "Alignment" line per result, for the PSSM as for the letters
    plain = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--pssm", f, "--db", prefix, "--top", "3", "--pssmAlignments"],
                           capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    al = [l for l in plain.stdout.splitlines() if l.startswith("Alignment ")]
    assert len(al) == 3 and al[0].endswith("CIGAR " + cig[0]) and ". Identities %d." % int(res[0]["identities"]) in al[0]
