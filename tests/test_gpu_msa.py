"""GPU: sw_msa_filter (rows, residue counts, pairwise identity, greedy keep, purged) against tests/msa_ref.py on inputs built
directly in numpy — random subjects, random valid CIGARs, consistent records —, then the host driver and `align --outMsa`."""
import numpy as np
import pytest

import gpu_util as G
import msa_ref as M

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def env():
    torch, capi, _ = G.gpu_modules()
    ctx = capi.Context(0)
    yield torch, capi, ctx
    ctx.close()


def run_filter(env, case, P, include=None, with_query=True, with_rows=True, with_ident=True):
    """sw_msa_filter on the case's arrays -> dict like msa_ref.msa_filter's.  Every output starts as garbage (the call zeroes
    what it does not write) and `rows` sits between guard bytes, which must survive."""
    torch, capi, ctx = env
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, qlen = case["n"], case["qlen"]
    assert capi.align_result_dtype() == M.RECORD
    dq = dev(case["query"]) if with_query else None
    if n:
        dch, doff, dlen = dev(case["chars"]), dev(case["offsets"].view(np.int64)), dev(case["lengths"])
        dres = dev(np.frombuffer(case["results"].tobytes(), dtype=np.uint8).copy())
        dcig = dev(case["cigar"].view(np.int32))
    else:
        dch = doff = dlen = dres = dcig = None
    dinc = dev(np.ascontiguousarray(include, dtype=np.uint8)) if include is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else 0
    drows = torch.full((GUARD + (n + 1) * qlen + GUARD,), 0xA7, dtype=torch.uint8, device="cuda") if with_rows else None
    dresid = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    dkeep = torch.full((n + 1 + GUARD,), 0x5C, dtype=torch.uint8, device="cuda")
    dpurged = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    dident = torch.full(((n + 1) * (n + 1),), 0x3B3B3B3, dtype=torch.int32, device="cuda") if with_ident else None
    args = dict(query=ptr(dq), qlen=qlen, n=n, chars=ptr(dch), offsets=ptr(doff), lengths=ptr(dlen), results=ptr(dres),
                cigar=ptr(dcig), include=ptr(dinc), max_identity=P, residues=dresid.data_ptr(), keep=dkeep.data_ptr(),
                purged=dpurged.data_ptr(), rows=drows.data_ptr() + GUARD if with_rows else 0, pair_ident=ptr(dident))
    need = capi.msa_filter(ctx, **args)
    assert need > 0
    temp = torch.full((need,), 0xEE, dtype=torch.uint8, device="cuda")
    assert capi.msa_filter(ctx, temp=temp.data_ptr(), temp_bytes=need, **args) == need
    torch.cuda.synchronize()
    out = dict(residues=dresid.cpu().numpy(), keep=dkeep.cpu().numpy()[:n + 1], purged=int(dpurged.item()))
    assert (dkeep.cpu().numpy()[n + 1:] == 0x5C).all()
    if with_rows:
        raw = drows.cpu().numpy()
        assert (raw[:GUARD] == 0xA7).all() and (raw[-GUARD:] == 0xA7).all()
        out["rows"] = raw[GUARD:-GUARD].reshape(n + 1, qlen)
    if with_ident:
        out["pair_ident"] = dident.cpu().numpy().view(np.uint32).reshape(n + 1, n + 1)
    return out


def assert_equal(got, want):
    if "rows" in got:
        assert got["rows"].tobytes() == want["rows"].tobytes(), np.argwhere(got["rows"] != want["rows"])[:5]
    assert got["residues"].tolist() == want["residues"].tolist()
    if "pair_ident" in got and want.get("pair_ident") is not None:
        assert got["pair_ident"].tobytes() == want["pair_ident"].tobytes(), np.argwhere(got["pair_ident"] != want["pair_ident"])[:5]
    assert got["keep"].tolist() == want["keep"].tolist(), np.flatnonzero(got["keep"] != want["keep"])[:10]
    assert got["purged"] == want["purged"]


def reference(case, P, include=None, with_query=True, onehot=False):
    rows = M.build_rows(case["query"] if with_query else None, case["qlen"], case["chars"], case["offsets"], case["lengths"],
                        case["results"], case["cigar"], include)
    idents = M.pair_ident_onehot(rows) if onehot else M.pair_ident(rows)
    keep, purged = M.greedy(rows, P, idents)
    return dict(rows=rows, residues=M.residues(rows), keep=keep, purged=purged, pair_ident=idents)


@pytest.mark.parametrize("qlen", [1, 31, 32, 33, 63, 64, 65, 700])
def test_shapes_against_reference(env, qlen):
    """every qlen of the list against every n of the list; P, the include bytes and the master alternate over the n"""
    rng = np.random.default_rng(1000 + qlen)
    for k, n in enumerate([0, 1, 2, 63, 64, 65, 200]):
        # families of near-copies so that every P purges something; hits that take no part; subject codes 20
        case = M.random_case(rng, qlen, n, max_runs=12 if qlen < 700 else 40, families=3, copy_rate=0.04)
        P = [0, 1, 94, 100][(k + qlen) % 4]
        include = (rng.random(n) < 0.8).astype(np.uint8) if k % 2 else None
        with_query = k % 3 != 2
        got = run_filter(env, case, P, include, with_query)
        want = reference(case, P, include, with_query)
        assert_equal(got, want)
        if n >= 63:
            assert (want["rows"][:n] == 20).any() and (want["rows"][:n] == M.GAP).any() or qlen == 1
            assert (case["results"]["status"] != 0).any() and (case["results"]["cigar_len"] == 0).any()
        if not with_query:
            assert (got["rows"][n] == M.NONE).all() and got["keep"][n] == 0


@pytest.mark.parametrize("P", [0, 1, 94, 100])
def test_every_threshold_and_long_cigars(env, P):
    """CIGARs of more than 64 and of more than 128 runs (the walker's blocks of 64 run words), at every P"""
    rng = np.random.default_rng(77 + P)
    case = M.random_case(rng, 700, 65, max_runs=200, families=2, copy_rate=0.02)
    runs = case["results"]["cigar_len"]
    assert (runs > 128).any() and ((runs > 64) & (runs <= 128)).any() and (runs == 0).any()
    got = run_filter(env, case, P)
    want = reference(case, P)
    assert_equal(got, want)
    if P in (1, 94):
        assert want["purged"] > 0
    if P == 0:
        assert want["purged"] == 0 and got["keep"].tolist() == (want["residues"] > 0).astype(int).tolist()
    # the optional outputs are optional
    lean = run_filter(env, case, P, with_rows=False, with_ident=False)
    assert lean["keep"].tolist() == got["keep"].tolist() and lean["purged"] == got["purged"]
    assert lean["residues"].tolist() == got["residues"].tolist()


def planted(qlen, rows_codes, other=None):
    """hits whose aligned residues are given: one '=' run over the whole query each"""
    n = len(rows_codes)
    recs = np.zeros(n, dtype=M.RECORD)
    subjects, words = [], []
    for h, codes in enumerate(rows_codes):
        codes = np.asarray(codes, dtype=np.int8)
        subjects.append(codes)
        recs[h]["q_begin"], recs[h]["q_end"], recs[h]["s_end"] = 0, len(codes), len(codes)
        recs[h]["cigar_len"], recs[h]["cigar_offset"] = 1, h
        words.append(len(codes) << 4 | M.OP_EQ)
    lengths = np.array([len(s) for s in subjects], dtype=np.int32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    return dict(query=np.full(qlen, 20, dtype=np.int8), qlen=qlen, n=n, chars=np.concatenate(subjects + [np.zeros(4, np.int8)]),
                offsets=offsets, lengths=lengths, results=recs, cigar=np.array(words + [0], dtype=np.uint32))


def test_copies_are_purged(env):
    rng = np.random.default_rng(5)
    one = rng.integers(0, 20, 90).astype(np.int8)
    case = planted(90, [one] * 300)
    got = run_filter(env, case, 94)
    assert got["keep"].tolist() == [1] + [0] * 299 + [0] and got["purged"] == 299   # (the master here is all 'X': no residue)
    assert_equal(got, reference(case, 94))
    assert run_filter(env, case, 0, with_ident=False)["keep"].tolist() == [1] * 300 + [0]


def test_greedy_is_not_transitive(env):
    """B is redundant to A, C to B but not to A: B is purged, so C is kept"""
    a = np.zeros(100, dtype=np.int8)
    b = a.copy()
    b[:8] = 1          # 92 % of A
    c = b.copy()
    c[8:16] = 2        # 92 % of B, 84 % of A
    case = planted(100, [a, b, c])
    got = run_filter(env, case, 90)
    assert got["pair_ident"][1, 0] == 92 and got["pair_ident"][2, 1] == 92 and got["pair_ident"][2, 0] == 84
    assert got["keep"].tolist() == [1, 0, 1, 0] and got["purged"] == 1
    assert_equal(got, reference(case, 90))
    # the fragment asymmetry: a fragment is redundant to the full-length row, not the other way round
    case = planted(100, [a[:40], a])
    got = run_filter(env, case, 90)
    assert got["keep"].tolist() == [1, 1, 0] and got["purged"] == 0
    case = planted(100, [a, a[:40]])
    got = run_filter(env, case, 90)
    assert got["keep"].tolist() == [1, 0, 0] and got["purged"] == 1


def test_foreign_cigar_leaves_none(env):
    """CIGARs whose positions exceed qlen or the subject: nothing is written outside rows (run_filter's guard bytes), pair
    columns off the subject and 'I' columns beyond q_end are NONE"""
    rng = np.random.default_rng(9)
    qlen = 70
    case = M.random_case(rng, qlen, 6, no_part_rate=0.0)
    recs, cig = case["results"], case["cigar"].copy()
    words = np.array([50 << 4 | M.OP_EQ, 3 << 4 | M.OP_D, 30 << 4 | M.OP_I, 4000 << 4 | M.OP_X, (1 << 27) << 4 | M.OP_EQ,
                      (1 << 27) << 4 | M.OP_D, 9 << 4 | M.OP_X], dtype=np.uint32)
    at = len(cig)
    case["cigar"] = np.concatenate([cig, words, np.zeros(2, dtype=np.uint32)])
    for h, (qb, qe, sb) in enumerate([(0, qlen, 0), (40, 60, 2), (69, 70, 0), (5, 400, int(case["lengths"][3]) - 3), (-1, 10, 0),
                                      (3, 20, -2)]):
        recs[h]["q_begin"], recs[h]["q_end"], recs[h]["s_begin"] = qb, qe, sb
        recs[h]["cigar_offset"], recs[h]["cigar_len"] = at, len(words)
    got = run_filter(env, case, 94)
    want = reference(case, 94)
    assert_equal(got, want)
    rows = got["rows"]
    assert (rows[4] == M.NONE).all() and (rows[5] == M.NONE).all()            # negative begins: no alignment
    assert (rows[0][int(case["lengths"][0]):50] == M.NONE).all() or case["lengths"][0] >= 50
    assert (rows[1][60:] != M.GAP).all() and (rows[3] == M.NONE).sum() > 0


def test_temp_contract_and_argument_checks(env):
    torch, capi, ctx = env
    buf = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    b = buf.data_ptr()
    ok = dict(query=b, qlen=10, n=0, chars=0, offsets=0, lengths=0, results=0, cigar=0, include=0, max_identity=94, residues=b,
              keep=b + 64, purged=b + 128)
    need = capi.msa_filter(ctx, **ok)            # temp == NULL: reports, launches nothing
    assert need > 0 and int(buf.sum().item()) == 0
    assert capi.msa_filter(ctx, **dict(ok, max_identity=0)) <= need
    with pytest.raises(capi.SwError) as e:
        capi.msa_filter(ctx, temp=b + 4096, temp_bytes=need - 1, **ok)
    assert e.value.code == -5
    capi.msa_filter(ctx, temp=b + 4096, temp_bytes=need, **ok)
    for bad in (dict(qlen=0), dict(qlen=(1 << 22) + 1), dict(n=-1), dict(n=(1 << 15) + 1), dict(max_identity=-1),
                dict(max_identity=101), dict(residues=0), dict(keep=0), dict(purged=0), dict(n=2),
                dict(n=2, chars=b, offsets=b, lengths=b, results=b)):
        with pytest.raises(capi.SwError) as e:
            capi.msa_filter(ctx, temp=b + 4096, temp_bytes=1 << 18, **dict(ok, **bad))
        assert e.value.code == -1, bad
    torch.cuda.synchronize()


def test_several_tiles_against_onehot_products(env):
    """n = 600, qlen = 700, families of near-copies: ten tiles of 64 rows, 22 words; the reference's identity counts come
    from one-hot matrix products"""
    rng = np.random.default_rng(2024)
    case = M.random_case(rng, 700, 600, max_runs=30, families=8, copy_rate=0.03, no_part_rate=0.05)
    got = run_filter(env, case, 94)
    want = reference(case, 94, onehot=True)
    assert_equal(got, want)
    assert 50 < want["purged"] < 590 and int(want["keep"].sum()) > 8
    # the same keep without the identity output (the kernel without its test store) and at P = 60
    assert run_filter(env, case, 94, with_rows=False, with_ident=False)["keep"].tolist() == want["keep"].tolist()
    want60 = M.greedy(want["rows"], 60, want["pair_ident"])
    got60 = run_filter(env, case, 60, with_rows=False, with_ident=False)
    assert got60["keep"].tolist() == want60[0].tolist() and got60["purged"] == want60[1]


# ---- the host driver and the command line -------------------------------------------------------------------------------

TOP, MIN_SCORE = 40, 70
LETTERS = "ARNDCQEGHILKMFPSTWYV"


def letters_of(codes):
    return "".join(LETTERS[c] for c in codes)


@pytest.fixture(scope="module")
def small_db(tmp_path_factory):
    """a 150-residue query; a dozen relatives with substitutions and indels, three of them near-copies (98 %) of a fourth;
    the query itself; 300 random subjects.  Header "s<k> ..." names seqs[k] (makedb orders the DB by length itself)."""
    import subprocess
    from cudasw4_amd import driver
    rng = np.random.default_rng(4242)
    q = rng.integers(0, 20, 150).astype(np.int8)

    def mutate(src, rate, indels=True):
        out = [int(rng.integers(0, 20)) if rng.random() < rate else int(c) for c in src]
        if indels:
            del out[40:43]
            out[90:90] = rng.integers(0, 20, 4).tolist()
        return np.array(out, dtype=np.int8)

    def flank(core):
        return np.concatenate([rng.integers(0, 20, int(rng.integers(0, 25))).astype(np.int8), core,
                               rng.integers(0, 20, int(rng.integers(0, 25))).astype(np.int8)])
    parent = mutate(q, 0.2)
    seqs = [flank(parent)] + [flank(mutate(parent, 0.02, indels=False)) for _ in range(3)]
    seqs += [flank(mutate(q, r)) for r in (0.15, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.5)]
    seqs += [flank(mutate(q[30:110], 0.2, indels=False)), q.copy()]
    seqs += [rng.integers(0, 20, int(L)).astype(np.int8) for L in rng.integers(50, 250, 300)]
    tmp = tmp_path_factory.mktemp("family")
    fasta = str(tmp / "db.fa")
    with open(fasta, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">s%d some description %d\n%s\n" % (i, len(s), letters_of(s)))
    prefix = str(tmp / "fam")
    p = subprocess.run([driver.MAKEDB, fasta, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    qfile = str(tmp / "q.fa")
    with open(qfile, "w") as f:
        f.write(">query one\n%s\n" % letters_of(q))
    return dict(q=q, letters=letters_of(q), seqs=seqs, prefix=prefix, qfile=qfile, tmp=tmp)


def host_arrays(subjects, ids, res, cigar_text):
    """the C ABI's arrays for msa_ref from what Driver.align_hits returned; subjects: the hits' codes in rank order"""
    rec = np.zeros(len(ids), dtype=M.RECORD)
    words, at = [], 0
    for k in range(len(ids)):
        for f in M.FIELDS:
            rec[k][f] = res[k][f]
        w = M.cigar_words(cigar_text[k]) if cigar_text[k] != "*" else np.zeros(0, dtype=np.uint32)
        rec[k]["cigar_offset"] = at
        at += len(w)
        words.append(w)
    lengths = np.array([len(s) for s in subjects], dtype=np.int32)
    offsets = np.zeros(len(ids) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    return np.concatenate(subjects + [np.zeros(4, np.int8)]), offsets, lengths, rec, np.concatenate(words + [np.zeros(1, np.uint32)])


def run_align(db, args, of):
    import subprocess
    from cudasw4_amd import driver
    r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", db["qfile"], "--db", db["prefix"], "--top", str(TOP),
                        "--of", of] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(of).read(), r.stdout


def test_driver_and_command_line(small_db):
    import pssm_build_ref as R
    import oracle_lib as O
    from cudasw4_amd import driver
    db = small_db
    q, letters, seqs, tmp = db["q"], db["letters"], db["seqs"], db["tmp"]
    d = driver.Driver(devices=[0], num_top=TOP)
    d.open_db(db["prefix"])
    result = d.scan(letters)
    ids = result["ids"]
    subjects = [seqs[int(d.reference_header(int(i)).split()[0][1:])] for i in ids]
    assert all(d.reference_length(int(i)) == len(s) for i, s in zip(ids, subjects))
    res, cigar_text = d.align_hits(letters, result)
    assert (res["status"] != 2).all() and (res["status"] == 0).sum() >= 30      # no hit of the fixture is without a trace
    chars, offsets, lengths, rec, cig = host_arrays(subjects, ids, res, cigar_text)

    # Driver.hit_msa = the reference applied to Driver.align_hits' output
    got = d.hit_msa(letters, result, max_identity=90, query_header="query one")
    want = M.msa_filter(q, len(q), chars, offsets, lengths, rec, cig, None, 90)
    assert got["cigars"] == cigar_text and got["results"].tobytes() == res.tobytes()
    assert got["rows"].tobytes() == want["rows"].tobytes() and got["residues"].tolist() == want["residues"].tolist()
    assert got["keep"].tolist() == want["keep"].tolist() and got["purged"] == want["purged"]
    # the three near-copies and the query's own copy go, their parent and the other relatives stay
    assert want["purged"] >= 4 and int(want["keep"][:len(ids)].sum()) >= 20 and want["keep"][len(ids)] == 1
    unfiltered = d.hit_msa(letters, result)
    assert unfiltered["purged"] == 0 and unfiltered["keep"].tolist() == (want["residues"] > 0).astype(int).tolist()
    assert unfiltered["rows"].tobytes() == want["rows"].tobytes()

    # the A3M's match columns are the device rows
    lines = got["a3m"].splitlines()
    kept = [k for k in range(len(ids)) if got["keep"][k]]
    assert lines[0] == ">query one" and lines[1] == letters and len(lines) == 2 + 2 * len(kept)
    for at, k in enumerate(kept):
        assert lines[2 + 2 * at] == ">" + d.reference_header(int(ids[k]))
        match = [c for c in lines[3 + 2 * at] if c == "-" or c.isupper()]
        assert match == [LETTERS[v] if v < 20 else "X" if v == 20 else "-" for v in got["rows"][k]], k
        w = M.cigar_words(cigar_text[k])
        assert lines[3 + 2 * at] == M.a3m_line(len(q), letters_of(subjects[k]), rec[k], w)
    assert any(c.islower() for l in lines[3::2] for c in l)
    fasta = d.hit_msa(letters, result, max_identity=90, fmt="fasta")["a3m"].splitlines()
    assert all(len(l) == len(q) for l in fasta[1::2]) and len(fasta) == len(lines)

    # --purgeIdentity: `used` drops by `purged`, and the PSSM is the reference's on the kept set
    plain, info = d.build_pssm(letters, result, min_score=MIN_SCORE)
    built, pinfo = d.build_pssm(letters, result, min_score=MIN_SCORE, purge_identity=94)
    assert "purged" not in info and pinfo["purged"] >= 3 and pinfo["used"] == info["used"] - pinfo["purged"]
    inc, _ = R.inclusion(rec, result["scores"], len(q), MIN_SCORE)
    keep94 = M.msa_filter(q, len(q), chars, offsets, lengths, rec, cig, inc, 94)
    assert keep94["purged"] == pinfo["purged"]
    inc2 = (np.asarray(inc, dtype=np.uint8) & keep94["keep"][:len(ids)]).astype(np.uint8)
    counts, weights, wcounts, used = R.accumulate(q, len(q), chars, offsets, lengths, rec, cig, inc2)
    assert used == pinfo["used"] and pinfo["included"] == [int(i) for i, b in zip(ids, inc2) if b]
    assert built.tolist() == R.convert(O.blosum21(62), q, counts, wcounts, 10.0)[0].tolist() and built.tolist() != plain.tolist()
    _, _, infos = d.iterate(letters, 2, MIN_SCORE, purge_identity=94)
    assert infos[0]["purged"] == pinfo["purged"] and infos[0]["included"] == pinfo["included"]
    d.close()

    # align --outMsa PREFIX --msaMaxIdentity 90 writes exactly the kept hits
    prefix = str(tmp / "M")
    _, stdout = run_align(db, ["--outMsa", prefix, "--msaMaxIdentity", "90", "--verbose"], str(tmp / "m.txt"))
    assert open(prefix + ".0.a3m").read() == got["a3m"]
    assert "msa: %d of %d results written, %d purged, 0 without a trace\n" % (len(kept), TOP, got["purged"]) in stdout
    run_align(db, ["--outMsa", prefix, "--msaFormat", "fasta"], str(tmp / "m2.txt"))
    every = open(prefix + ".0.fasta").read().splitlines()
    assert len(every) == 2 + 2 * int(unfiltered["keep"][:len(ids)].sum()) and all(len(l) == len(q) for l in every[1::2])
    # --purgeIdentity in the rounds' verbose line
    _, stdout = run_align(db, ["--iterations", "2", "--inclusionScore", str(MIN_SCORE), "--purgeIdentity", "94", "--verbose"],
                          str(tmp / "p.txt"))
    first = [l for l in stdout.splitlines() if l.startswith("Query 0 round 1:")][0]
    assert " %d in the PSSM," % pinfo["used"] in first and ", %d purged as redundant, lambda" % pinfo["purged"] in first


def test_outputs_without_the_flags_are_unchanged(small_db):
    """the result columns of a run with --outMsa equal those of the same command line without it, and without the new flags
    nothing of the feature shows in stdout"""
    db, tmp = small_db, small_db["tmp"]
    for extra in ([], ["--tsv", "--alignments"], ["--iterations", "2", "--inclusionScore", str(MIN_SCORE), "--tsv", "--verbose"]):
        plain, out_plain = run_align(db, extra, str(tmp / "a.out"))
        with_msa, out_msa = run_align(db, extra + ["--outMsa", str(tmp / "U")], str(tmp / "a.out"))
        assert plain == with_msa and len(plain.splitlines()) >= TOP
        assert "msa" not in out_plain.lower() and "purged" not in out_plain and "outMsa: " in out_msa
        if "--verbose" in extra:   # (timings differ from run to run: the rounds' lines)
            strip = lambda text: [l for l in text.splitlines() if l.startswith("Query 0 round ")]
            assert len(strip(out_plain)) == 2
        else:
            strip = lambda text: [l for l in text.splitlines() if not l.startswith("outMsa: ")]
        assert strip(out_msa) == strip(out_plain)


def test_pssm_query_and_rounds_write_their_last_alignment(small_db):
    """--pssm FILE --outMsa: the file's residue column is the first row and the results are aligned against the PSSM; with
    --iterations the rows are the last round's, aligned with that round's scoring"""
    from cudasw4_amd import driver
    db, tmp = small_db, small_db["tmp"]
    letters = db["letters"]
    d = driver.Driver(devices=[0], num_top=TOP)
    d.open_db(db["prefix"])
    first = d.scan(letters)
    p1, _ = d.build_pssm(letters, first, min_score=MIN_SCORE)
    r2 = d.scan_pssm(p1)
    want = d.hit_msa(letters, r2, max_identity=90, pssm=p1)
    d.close()
    assert want["purged"] >= 3 and (want["results"]["status"] != 2).all()
    pfile = str(tmp / "round1.pssm")
    driver.write_pssm_ascii(pfile, p1, letters)
    import subprocess
    prefix = str(tmp / "Q")
    r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--pssm", pfile, "--db", db["prefix"], "--top", str(TOP), "--of",
                        str(tmp / "q.out"), "--outMsa", prefix, "--msaMaxIdentity", "90"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = open(prefix + ".0.a3m").read().splitlines()
    assert got[0].startswith(">") and got[1:] == want["a3m"].splitlines()[1:]
    # two rounds from the letters: round 2 scans with p1, and its results are aligned against p1
    prefix = str(tmp / "R")
    run_align(db, ["--iterations", "2", "--inclusionScore", str(MIN_SCORE), "--outMsa", prefix, "--msaMaxIdentity", "90"],
              str(tmp / "r.out"))
    assert open(prefix + ".0.a3m").read() == want["a3m"].replace(">query\n", ">query one\n", 1)
