"""GPU: sw_pssm_accumulate fed with what sw_align_hits / sw_align_hits_pssm really wrote — counts, weights, weighted counts and
`used` bit for bit against the scalar reference tests/pssm_build_ref.c —, then Driver.build_pssm, Driver.iterate and
`align --iterations` against the same chain computed on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import align_ref as A
import gpu_util as G
import oracle_lib as O
import pssm_align_ref as PA
import pssm_build_cases as C
import pssm_build_ref as R
import pssm_ref as PR

pytestmark = pytest.mark.gpu

CASES = C.cases()


@pytest.fixture(scope="module")
def env():
    torch, capi, _ = G.gpu_modules()
    ctx = capi.Context(0)
    ctx.set_matrix(O.blosum21(62))
    yield torch, capi, ctx
    ctx.close()


def gpu_chain(env, q, subjects, gop=-11, gex=-1, pssm=None, include=None, with_master=True, trace_bytes=None, shuffle=None):
    """align the subjects against q (letters; with `pssm`: sw_align_hits_pssm with q as the consensus), accumulate on what the
    aligner left in device memory -> (records, CIGAR buffer, (counts, weights, wcounts, used)), all downloaded.
    shuffle: a Generator — the CIGARs are moved to shuffled slots of a new buffer behind a gap, and the records' cigar_offset
    follow, before the accumulation."""
    torch, capi, ctx = env
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, qlen = len(subjects), len(q)
    dq = dev(np.ascontiguousarray(q, dtype=np.int8))
    dt = capi.align_result_dtype()
    assert dt == R.RECORD
    if n:
        chars, offsets, lengths = O.make_db(subjects)
        coff = np.zeros(n + 1, dtype=np.int64)
        coff[1:] = np.cumsum(qlen + lengths.astype(np.int64))
        dch, doff, dlen, dcoff = dev(chars), dev(offsets.view(np.int64)), dev(lengths), dev(coff)
        dres = torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda")
        dcig = torch.zeros(int(coff[-1]), dtype=torch.int32, device="cuda")
        tb = trace_bytes if trace_bytes is not None else max(capi.align_trace_bytes(qlen, int(L)) for L in lengths)
        kw = dict(trace_bytes=tb)
        if pssm is not None:
            dp = dev(np.ascontiguousarray(pssm, dtype=np.int8).reshape(-1))
            call = lambda **more: capi.align_hits_pssm(ctx, dp.data_ptr(), dq.data_ptr(), qlen, n, dch.data_ptr(), doff.data_ptr(),
                                                       dlen.data_ptr(), int(lengths.max()), gop, gex, dres.data_ptr(),
                                                       dcig.data_ptr(), dcoff.data_ptr(), **kw, **more)
        else:
            call = lambda **more: capi.align_hits(ctx, dq.data_ptr(), qlen, n, dch.data_ptr(), doff.data_ptr(), dlen.data_ptr(),
                                                  int(lengths.max()), gop, gex, dres.data_ptr(), dcig.data_ptr(), dcoff.data_ptr(),
                                                  **kw, **more)
        temp = torch.empty(call(), dtype=torch.uint8, device="cuda")
        call(temp=temp.data_ptr(), temp_bytes=temp.numel())
        torch.cuda.synchronize()
        if shuffle is not None:
            res = np.frombuffer(dres.cpu().numpy().tobytes(), dtype=dt).copy()
            old = dcig.cpu().numpy().view(np.uint32)
            new = np.full(len(old) + 1000, 0xFFFFFFFF, dtype=np.uint32)   # (a stray word would be a run of 2^28 columns)
            at = 777
            for k in shuffle.permutation(n):
                a, m = int(res[k]["cigar_offset"]), int(res[k]["cigar_len"])
                new[at:at + m] = old[a:a + m]
                res[k]["cigar_offset"] = at
                at += m + int(shuffle.integers(0, 3))
            dres = dev(np.frombuffer(res.tobytes(), dtype=np.uint8).copy())
            dcig = dev(new.view(np.int32))
    else:
        chars, offsets, lengths = np.zeros(4, np.int8), np.zeros(1, np.uint64), np.zeros(0, np.int32)
        dch = doff = dlen = dres = dcig = None
    ptr = lambda t: t.data_ptr() if t is not None else 0
    dinc = dev(np.ascontiguousarray(include, dtype=np.uint8)) if include is not None else None
    # outputs start as garbage: the call zeroes them itself
    dcounts = torch.full((qlen * 20,), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    dweights = torch.full((n + 1,), -3, dtype=torch.int64, device="cuda")
    dwcounts = torch.full((qlen * 20,), -5, dtype=torch.int64, device="cuda")
    dused = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    capi.pssm_accumulate(ctx, dq.data_ptr() if with_master else 0, qlen, n, ptr(dch), ptr(doff), ptr(dlen), ptr(dres), ptr(dcig),
                         ptr(dinc), dcounts.data_ptr(), dweights.data_ptr(), dwcounts.data_ptr(), dused.data_ptr())
    torch.cuda.synchronize()
    res = np.frombuffer(dres.cpu().numpy().tobytes(), dtype=dt).copy() if n else np.zeros(0, dtype=dt)
    cig = dcig.cpu().numpy().view(np.uint32) if n else np.zeros(1, dtype=np.uint32)
    got = (dcounts.cpu().numpy().view(np.uint32).reshape(qlen, 20), dweights.cpu().numpy().view(np.uint64),
           dwcounts.cpu().numpy().view(np.uint64).reshape(qlen, 20), int(dused.item()))
    return res, cig, got, (chars, offsets, lengths)


def assert_equals_reference(q, res, cig, got, db, include=None, with_master=True):
    want = R.accumulate(q if with_master else None, len(q), db[0], db[1], db[2], res, cig, include)
    assert got[3] == want[3], (got[3], want[3])
    assert got[0].tobytes() == want[0].tobytes(), np.argwhere(got[0] != want[0])[:5]
    assert got[1].tobytes() == want[1].tobytes(), np.argwhere(got[1] != want[1])[:5]
    assert got[2].tobytes() == want[2].tobytes(), np.argwhere(got[2] != want[2])[:5]
    return want


def words_of(res, cig):
    return [cig[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])] for r in res]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_planted_shapes(env, case):
    q = case["q"]
    res, cig, got, db = gpu_chain(env, q, case["subjects"], case["gop"], case["gex"])
    assert case["holds"](res, words_of(res, cig))   # (the aligner wrote what the case is there for)
    want = assert_equals_reference(q, res, cig, got, db)
    assert want[3] == int(((res["status"] == 0) & (res["cigar_len"] > 0)).sum())
    if case["name"] == "copies300":
        assert int(got[0].max()) == 301 and (got[0][4:70].max(axis=1) == 301).all()


def test_include_master_and_empty_lists(env):
    case = next(c for c in CASES if c["name"] == "qlen65")
    q, subjects = case["q"], case["subjects"]
    n = len(subjects)
    full = gpu_chain(env, q, subjects)
    assert_equals_reference(q, *full)
    # a zero include byte; all zero; include == NULL is every hit
    for inc in ([1, 0, 1, 1, 0, 1], [0] * n, [1] * n):
        res, cig, got, db = gpu_chain(env, q, subjects, include=inc)
        want = assert_equals_reference(q, res, cig, got, db, include=inc)
        assert want[3] == sum(inc) and [int(w) == 0 for w in got[1][:n]] == [not b for b in inc]
    assert gpu_chain(env, q, subjects, include=[1] * n)[2][2].tobytes() == full[2][2].tobytes()
    # query == NULL: no master row, its weight stays 0
    res, cig, got, db = gpu_chain(env, q, subjects, with_master=False)
    assert_equals_reference(q, res, cig, got, db, with_master=False)
    assert int(got[1][n]) == 0 and int(got[0].sum()) < int(full[2][0].sum())
    # n == 0: the master alone; n == 0 without a master: zeros
    res, cig, got, db = gpu_chain(env, q, [])
    assert_equals_reference(q, res, cig, got, db)
    assert got[3] == 0 and int(got[0].sum()) == len(q) and got[1].tolist() == [len(q) << 32]
    res, cig, got, db = gpu_chain(env, q, [], with_master=False)
    assert got[3] == 0 and not got[0].any() and not got[2].any() and got[1].tolist() == [0]
    # n == 1
    res, cig, got, db = gpu_chain(env, q, subjects[2:3])
    assert_equals_reference(q, res, cig, got, db)


def test_no_trace_and_shuffled_slots(env):
    torch, capi, ctx = env
    case = next(c for c in CASES if c["name"] == "qlen600")
    q, subjects = case["q"], case["subjects"]
    # a trace budget that only the 70-column fragment fits: the others have coordinates and no CIGAR, and take no part
    small = capi.align_trace_bytes(70, 70)
    res, cig, got, db = gpu_chain(env, q, subjects, trace_bytes=small)
    assert int(res[1]["status"]) == R.OK and (res["status"] == R.NO_TRACE).sum() >= 5
    want = assert_equals_reference(q, res, cig, got, db)
    assert want[3] == int((res["status"] == R.OK).sum()) and int(got[1][0]) == 0
    # CIGARs in shuffled slots behind a gap: cigar_offset is what locates them
    res, cig, got, db = gpu_chain(env, q, subjects, shuffle=np.random.default_rng(3))
    assert int(res["cigar_offset"].min()) == 777 and sorted(res["cigar_offset"].tolist()) != res["cigar_offset"].tolist()
    assert_equals_reference(q, res, cig, got, db)
    plain = gpu_chain(env, q, subjects)
    assert got[0].tobytes() == plain[2][0].tobytes() and got[2].tobytes() == plain[2][2].tobytes()


def test_argument_checks(env):
    torch, capi, ctx = env
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda").data_ptr()
    ok = dict(query=buf, qlen=10, n=0, chars=0, offsets=0, lengths=0, results=0, cigar=0, include=0, counts=buf, weights=buf,
              wcounts=buf, used=buf)
    capi.pssm_accumulate(ctx, **ok)
    for bad in (dict(qlen=0), dict(qlen=(1 << 22) + 1), dict(n=-1), dict(counts=0), dict(weights=0), dict(wcounts=0), dict(used=0),
                dict(n=2), dict(n=2, chars=buf, offsets=buf, lengths=buf, results=buf), dict(counts=buf + 4)):
        with pytest.raises(capi.SwError) as e:
            capi.pssm_accumulate(ctx, **dict(ok, **bad))
        assert e.value.code == -1, bad
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["qlen64", "qlen600", "runs129", "other_codes"])
def test_pssm_form(env, name):
    """the same with sw_align_hits_pssm output: a from_sequence PSSM scores like the letters, the master is the consensus"""
    from cudasw4_amd import pssm
    case = next(c for c in CASES if c["name"] == name)
    q = case["q"]
    p = pssm.from_sequence(q, O.blosum21(62))
    res, cig, got, db = gpu_chain(env, q, case["subjects"], pssm=p)
    assert case["holds"](res, words_of(res, cig))
    assert_equals_reference(q, res, cig, got, db)
    letters = gpu_chain(env, q, case["subjects"])
    assert res.tobytes() == letters[0].tobytes() and got[2].tobytes() == letters[2][2].tobytes()


# ---- the host driver ---------------------------------------------------------------------------------------------------

TOP, MIN_SCORE = 50, 85


def build_family():
    """about 2 000 short background subjects, a planted family of a 120-residue query (close and remote relatives, so that
    later rounds find more than the first), a self-copy of the query and relatives too weak for MIN_SCORE"""
    from cudasw4_amd import synthdb
    rng = np.random.default_rng(77)
    q = rng.integers(0, 20, 120).astype(np.int8)
    lengths = rng.integers(30, 200, 2000)
    bg = synthdb.random_db(lengths, seed=5, composition=synthdb.SPROT_COMPOSITION)
    seqs = [bg[0][int(bg[1][i]):int(bg[1][i]) + int(bg[2][i])] for i in range(len(lengths))]

    def relative(rate, lo=0, hi=120):
        copy = [int(rng.integers(0, 20)) if rng.random() < rate else int(c) for c in q[lo:hi]]
        if hi - lo > 40:
            del copy[20:23]
            copy[50:50] = rng.integers(0, 20, 4).tolist()
        return np.concatenate([rng.integers(0, 20, int(rng.integers(0, 30))).astype(np.int8), np.array(copy, dtype=np.int8),
                               rng.integers(0, 20, int(rng.integers(0, 30))).astype(np.int8)])
    seqs += [relative(r) for r in (0.2, 0.3, 0.35, 0.4, 0.45, 0.5, 0.5, 0.55, 0.6, 0.6, 0.65, 0.65, 0.7, 0.7)]
    seqs += [relative(0.3, 30, 48), relative(0.2, 70, 84)]     # weak: in the top list, below MIN_SCORE
    seqs += [q.copy()]                                          # the query itself
    seqs.sort(key=len)
    return q, seqs, O.make_db(seqs)


@pytest.fixture(scope="module")
def family():
    return build_family()


def letters_of(codes):
    return "".join("ARNDCQEGHILKMFPSTWYV"[c] for c in codes)


def make_driver(family, upload=True, **kw):
    from cudasw4_amd import driver
    d = driver.Driver(devices=[0], num_top=TOP, kinds=(0, 0, 3, 3), **kw)
    d.db_from_arrays(*family[2])
    if upload:
        d.upload()
    return d


def reference_build(q, seqs, ids, scores, res, cigars, min_score, beta=10.0):
    """the reference chain behind an alignment: inclusion rule, accumulation, conversion"""
    subjects = [seqs[int(i)] for i in ids]
    chars, offsets, lengths = O.make_db(subjects)
    rec = np.zeros(len(ids), dtype=R.RECORD)
    words, at = [], 0
    for k in range(len(ids)):
        for f in R.FIELDS:
            rec[k][f] = res[k][f]
        w = cigars[k]
        rec[k]["cigar_offset"] = at
        at += len(w)
        words.append(np.asarray(w, dtype=np.uint32))
    cig = np.concatenate(words + [np.zeros(1, dtype=np.uint32)])
    inc, left = R.inclusion(rec, scores, len(q), min_score)
    counts, weights, wcounts, used = R.accumulate(q, len(q), chars, offsets, lengths, rec, cig, inc)
    p, _, lam = R.convert(O.blosum21(62), q, counts, wcounts, beta)
    return p, dict(left, used=used, included=[int(i) for i, b in zip(ids, inc) if b], **{"lambda": lam})


def cpu_round(q, family, scoring):
    """one round on the CPU: scan (letters: the oracle; a PSSM: pssm_ref), top list, alignments by the scalar aligners"""
    _, seqs, (chars, offsets, lengths) = family
    if scoring is None:
        all_scores = O.scan(q, chars, offsets, lengths)
    else:
        all_scores = PR.scan(scoring, chars, offsets, lengths)
    scores, ids = O.topk(all_scores, TOP)
    res, cigars = [], []
    for i in ids:
        if scoring is None:
            r, w = A.align(q, seqs[int(i)], O.blosum21(62))
        else:
            r, w = PA.align(scoring, seqs[int(i)], q)
        res.append(r)
        cigars.append(w)
    return scores, ids, res, cigars


def test_driver_build_pssm(family):
    from cudasw4_amd import pssm
    q, seqs, db = family
    letters = letters_of(q)
    d = make_driver(family)
    result = d.scan(letters)
    res, cigar_text = d.align_hits(letters, result)
    want, winfo = reference_build(q, seqs, result["ids"], result["scores"], res, [R.words(c) if c != "*" else [] for c in cigar_text],
                                  MIN_SCORE)
    got, info = d.build_pssm(letters, result, min_score=MIN_SCORE)
    assert got.tolist() == want.tolist()
    assert {k: info[k] for k in ("used", "below_score", "no_trace", "copies")} == {k: winfo[k] for k in ("used", "below_score", "no_trace", "copies")}
    assert info["included"] == winfo["included"] and abs(info["lambda"] - winfo["lambda"]) < 1e-12
    # the planted DB reaches every branch of the rule but NO_TRACE (which the next call forces)
    assert info["copies"] == 1 and info["below_score"] >= 2 and info["used"] >= 10 and info["no_trace"] == 0
    assert int(result["scores"][0]) == O.score(q, q) and got.tolist() != pssm.from_sequence(q, O.blosum21(62)).tolist()
    assert (got[:, 20] == pssm.from_sequence(q, O.blosum21(62))[:, 20]).all()
    # another pseudocount, and the PSSM form: hits of a scan with the built PSSM, aligned with it
    got5, _ = d.build_pssm(letters, result, min_score=MIN_SCORE, pseudocount=2.5)
    assert got5.tolist() == reference_build(q, seqs, result["ids"], result["scores"], res,
                                            [R.words(c) if c != "*" else [] for c in cigar_text], MIN_SCORE, 2.5)[0].tolist()
    r2 = d.scan_pssm(got)
    res2, cig2 = d.align_hits_pssm(got, r2, consensus=letters)
    want2, winfo2 = reference_build(q, seqs, r2["ids"], r2["scores"], res2, [R.words(c) if c != "*" else [] for c in cig2], MIN_SCORE)
    got2, info2 = d.build_pssm(letters, r2, pssm=got, min_score=MIN_SCORE)
    assert got2.tolist() == want2.tolist() and info2["included"] == winfo2["included"] and info2["copies"] == winfo2["copies"]
    # no hit at all, and no hit above the score: the query's own rows
    empty = dict(ids=np.zeros(0, dtype=np.int64), scores=np.zeros(0, dtype=np.int32))
    for r, ms in ((empty, 0), (result, 10 ** 6)):
        p0, i0 = d.build_pssm(letters, r, min_score=ms)
        assert p0.tolist() == pssm.from_sequence(q, O.blosum21(62)).tolist() and i0["used"] == 0
    assert i0["below_score"] == TOP
    with pytest.raises(ValueError):
        d.build_pssm(letters, result, pssm=got[:-1], min_score=MIN_SCORE)
    d.close()
    # a trace budget that fits no pair: every hit above the score is counted as left out for want of a trace
    # (this driver only aligns: the hits come from the scan above)
    d = make_driver(family, upload=False, max_temp_bytes=4096)
    p0, i0 = d.build_pssm(letters, result, min_score=MIN_SCORE)
    assert i0["no_trace"] == TOP - i0["below_score"] > 0 and i0["used"] == 0 and i0["copies"] == 0
    assert p0.tolist() == pssm.from_sequence(q, O.blosum21(62)).tolist()
    d.close()


def test_driver_iterate(family):
    from cudasw4_amd import pssm
    q, seqs, db = family
    letters = letters_of(q)
    d = make_driver(family)
    result, built, infos = d.iterate(letters, 3, MIN_SCORE)
    # the same chain on the CPU
    scoring, winfos = None, []
    for _ in range(3):
        scores, ids, res, cigars = cpu_round(q, family, scoring)
        want, winfo = reference_build(q, seqs, ids, scores, res, cigars, MIN_SCORE)
        winfos.append(winfo)
        if len(winfos) > 1 and sorted(winfos[-1]["included"]) == sorted(winfos[-2]["included"]):
            break
        scoring = want
    assert len(infos) == len(winfos) >= 2
    assert result["scores"].tolist() == scores.tolist() and result["ids"].tolist() == ids.tolist()
    assert built.tolist() == want.tolist()
    for a, b in zip(infos, winfos):
        assert a["included"] == b["included"] and (a["used"], a["below_score"], a["copies"], a["no_trace"]) == \
            (b["used"], b["below_score"], b["copies"], b["no_trace"])
    assert infos[1]["included"] != infos[0]["included"]   # (the profile found something the letters had not)
    # one round is the scan and one build
    r1, b1, i1 = d.iterate(letters, 1, MIN_SCORE)
    assert r1["ids"].tolist() == d.scan(letters)["ids"].tolist() and len(i1) == 1 and not i1[0]["converged"]
    # an inclusion score above every hit: nothing goes in, round 2 repeats round 1 and the loop stops as converged
    top_score = int(r1["scores"][0])
    r, b, i = d.iterate(letters, 5, top_score + 1)
    assert len(i) == 2 and i[1]["converged"] and not i[0]["converged"] and i[1]["included"] == []
    assert b.tolist() == pssm.from_sequence(q, O.blosum21(62)).tolist() and r["scores"].tolist() == r1["scores"].tolist()
    d.close()


# ---- the command line --------------------------------------------------------------------------------------------------

def test_align_iterations(family, tmp_path):
    from cudasw4_amd import driver, pssm
    q, seqs, db = family
    letters = letters_of(q)
    fasta = str(tmp_path / "db.fa")
    with open(fasta, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">s%d\n%s\n" % (i, letters_of(np.minimum(s, 19))))
    prefix = str(tmp_path / "fam")
    p = subprocess.run([driver.MAKEDB, fasta, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    qfile = str(tmp_path / "q.fa")
    with open(qfile, "w") as f:
        f.write(">query one\n%s\n" % letters)

    def run(args, of):
        r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", qfile, "--db", prefix, "--top", str(TOP), "--of", of]
                           + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(of).read(), r.stdout

    d = driver.Driver(devices=[0], num_top=TOP)
    d.open_db(prefix)
    result, built, infos = d.iterate(letters, 3, MIN_SCORE)
    first = d.scan(letters)
    d.close()
    out_prefix = str(tmp_path / "P")
    tsv, stdout = run(["--iterations", "3", "--inclusionScore", str(MIN_SCORE), "--tsv", "--outPssm", out_prefix, "--verbose"],
                      str(tmp_path / "it.tsv"))
    rows = [l.split("\t") for l in tsv.splitlines()[1:]]
    assert [int(x[4]) for x in rows] == result["scores"].tolist() and [int(x[7]) for x in rows] == result["ids"].tolist()
    back, cons = pssm.read_ascii(out_prefix + ".0.pssm")
    assert back[:, :20].tolist() == built[:, :20].tolist() and cons == letters
    per_round = [l for l in stdout.splitlines() if l.startswith("Query 0 round ")]
    assert len(per_round) == len(infos)
    for line, info in zip(per_round, infos):
        assert " %d in the PSSM, %d below the inclusion score, %d without a trace, %d copies" % (
            info["used"], info["below_score"], info["no_trace"], info["copies"]) in line
    assert ("converged" in per_round[-1]) == (infos[-1]["converged"] and len(infos) < 3)
    # an inclusion score nothing reaches: stops after round 2 and says so; the results are round 1's
    tsv_c, stdout_c = run(["--iterations", "4", "--inclusionScore", "100000", "--tsv", "--verbose"], str(tmp_path / "c.tsv"))
    assert len([l for l in stdout_c.splitlines() if l.startswith("Query 0 round ")]) == 2 and ", converged" in stdout_c
    # the alignment columns of the last round are against that round's scoring
    tsv_a, _ = run(["--iterations", "2", "--inclusionScore", str(MIN_SCORE), "--tsv", "--alignments"], str(tmp_path / "a.tsv"))
    d = driver.Driver(devices=[0], num_top=TOP)
    d.open_db(prefix)
    p1, _ = d.build_pssm(letters, first, min_score=MIN_SCORE)
    r2 = d.scan_pssm(p1)
    res2, cig2 = d.align_hits_pssm(p1, r2, consensus=letters)
    d.close()
    rows_a = [l.split("\t") for l in tsv_a.splitlines()[1:]]
    assert [int(x[4]) for x in rows_a] == r2["scores"].tolist() and [x[15] for x in rows_a] == cig2
    assert [int(x[13]) for x in rows_a] == res2["identities"].tolist()
    # unchanged outputs: without the new flags, and with --iterations 1, what a scan prints
    plain, out_plain = run([], str(tmp_path / "plain.txt"))
    one, out_one = run(["--iterations", "1"], str(tmp_path / "one.txt"))
    assert one == plain and out_one.replace("one.txt", "plain.txt") == out_plain
    assert "iterations:" not in out_plain and "inclusionScore" not in out_plain and tsv_c.splitlines()[1:] == run(["--tsv"], str(tmp_path / "p.tsv"))[0].splitlines()[1:]
    lines = plain.splitlines()
    assert lines[0].startswith("Query 0, header") and len(lines) == 1 + TOP
    assert [int(l.split("Score: ")[1].split(".")[0]) for l in lines[1:]] == first["scores"].tolist()
    assert [int(l.rsplit("referenceId ", 1)[1]) for l in lines[1:]] == first["ids"].tolist()
