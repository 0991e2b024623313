"""Search statistics on the GPU: the histogram kernel against numpy on bare arrays, the driver's score tap in
every scan mode, the degenerate pseudo DB, and `align`'s flags."""
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import stats_ref as R
from test_stats_cpu import _test1_lengths, check_calibration, z_close

pytestmark = pytest.mark.gpu

QUERIES = (2, 12)
TOP = 20


# ---- the kernel: capi.score_histogram on arrays --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hist_runner():
    import torch
    from cudasw4_amd import capi
    ctx = capi.Context(0)

    def run(pieces, score_shift=0, length_shift=0):
        """pieces: list of (scores, lengths) added into ONE table by one call each; the device arrays start `shift`
        elements behind a 256-byte boundary -> (hist, sumlen, skipped)"""
        hist = torch.zeros(R.LBINS * R.SBINS, dtype=torch.int32, device="cuda:0")
        sumlen = torch.zeros(R.LBINS, dtype=torch.int64, device="cuda:0")
        skipped = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        keep = []
        for scores, lengths in pieces:
            n = len(scores)
            s = torch.zeros(n + 8, dtype=torch.float32, device="cuda:0")
            l = torch.zeros(n + 8, dtype=torch.int32, device="cuda:0")
            s[score_shift:score_shift + n] = torch.from_numpy(np.asarray(scores, dtype=np.float32)).to("cuda:0")
            l[length_shift:length_shift + n] = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).to("cuda:0")
            keep += [s, l]
            capi.score_histogram(ctx, s.data_ptr() + 4 * score_shift, l.data_ptr() + 4 * length_shift, n, hist.data_ptr(),
                                 sumlen.data_ptr(), skipped.data_ptr())
        torch.cuda.synchronize()
        return (hist.cpu().numpy().view(np.uint32).reshape(R.LBINS, R.SBINS), sumlen.cpu().numpy().view(np.uint64),
                int(skipped.cpu().numpy().view(np.uint32)[0]))

    yield run
    ctx.close()


def _mixed(n, seed=5):
    rng = np.random.default_rng(seed)
    pool = np.array(_test1_lengths(), dtype=np.int64)
    lengths = pool[np.arange(n) % len(pool)].astype(np.int32)
    special = np.array([0, 1, 37, 254, 255, 256, 10 ** 6, -1, -2], dtype=np.float32)
    scores = rng.integers(0, 121, n).astype(np.float32)
    where = rng.random(n) < 0.3
    scores[where] = special[rng.integers(0, len(special), int(where.sum()))]
    return scores, lengths


def _same(got, scores, lengths):
    hist, sumlen, skipped = R.histogram(scores, lengths)
    assert got[2] == skipped
    assert np.array_equal(got[0], hist)
    assert np.array_equal(got[1], sumlen)


def test_histogram_kernel(hist_runner):
    # n = 0: a no-op (nothing is read or written)
    got = hist_runner([(np.zeros(0), np.zeros(0))])
    assert got[0].sum() == 0 and got[1].sum() == 0 and got[2] == 0
    for scores, lengths in (([41.0], [290]), ([-1.0], [290])):
        _same(hist_runner([(scores, lengths)]), np.array(scores), np.array(lengths))
    scores, lengths = _mixed(70001)
    assert (scores < 0).sum() > 1000 and (scores > 255).sum() > 1000
    _same(hist_runner([(scores, lengths)]), scores, lengths)
    # every lane of every wave on ONE word
    n = 300000
    got = hist_runner([(np.full(n, 41.0), np.full(n, 290))])
    assert int(got[0][R.length_bin(290), 41]) == n and int(got[0].sum()) == n and int(got[1][R.length_bin(290)]) == 290 * n
    _same(got, np.full(n, 41.0), np.full(n, 290))


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_histogram_kernel_unaligned(hist_runner, shift):
    scores, lengths = _mixed(70001, seed=6)
    for n in (70001 - 4 + shift, shift, 4 + shift):        # n = shift mod 4, also with an empty middle
        s, l = scores[:n], lengths[:n]
        _same(hist_runner([(s, l)], shift, shift), s, l)
        _same(hist_runner([(s, l)], shift, (shift + 1) % 4), s, l)    # the lengths aligned differently from the scores
        _same(hist_runner([(s, l)], 0, shift), s, l)


def test_histogram_kernel_adds(hist_runner):
    scores, lengths = _mixed(70001, seed=7)
    whole = hist_runner([(scores, lengths)])
    halves = hist_runner([(scores[:35000], lengths[:35000]), (scores[35000:], lengths[35000:])])
    assert np.array_equal(whole[0], halves[0]) and np.array_equal(whole[1], halves[1]) and whole[2] == halves[2]
    _same(halves, scores, lengths)


# ---- the driver -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_db():
    """sprot_like(3000) and the oracle's scores for the two queries: computed once, shared, never changed."""
    from cudasw4_amd import synthdb
    chars, offsets, lengths, family = synthdb.sprot_like(n=3000, max_len=8000, return_family_ids=True)
    _, letters = O.read_fasta(O.GOLDEN_DIR + "/allqueries.fasta")
    _, qs = O.load_queries()
    nonfamily = np.ones(len(lengths), dtype=bool)
    nonfamily[np.asarray(family, dtype=np.int64)] = False
    want = {}
    for qi in QUERIES:
        sc = O.scan(qs[qi], chars, offsets, lengths, simd=True).astype(np.int64)
        hist, sumlen, _ = R.histogram(sc, lengths)
        want[qi] = {"scores": sc, "hist": hist, "sumlen": sumlen, "fit": R.fit(hist, sumlen), "self": O.score(qs[qi], qs[qi])}
    return {"db": (chars, offsets, lengths), "lengths": np.asarray(lengths), "nonfamily": nonfamily, "letters": letters,
            "codes": qs, "want": want}


def _driver(small_db, **kw):
    from cudasw4_amd import driver
    kw.setdefault("devices", [0])
    d = driver.Driver(num_top=TOP, **kw)
    d.db_from_arrays(*small_db["db"])
    return d


def _check_result(small_db, qi, r):
    w = small_db["want"][qi]
    st = r["stats"]
    assert np.array_equal(st["hist"], w["hist"]) and np.array_equal(st["sumlen"], w["sumlen"]) and st["N"] == len(small_db["lengths"])
    es, ei = O.topk(w["scores"], TOP)
    assert r["scores"].tolist() == es.tolist() and r["ids"].tolist() == ei.tolist()
    for k in ("n_included", "rounds", "status"):
        assert st[k] == w["fit"][k]
    rz, re_ = R.evalues(w["fit"], r["scores"], small_db["lengths"][r["ids"]])
    assert np.allclose(r["evalues"], re_, rtol=1e-9, atol=0.0)
    assert z_close(r["zscores"], rz, w["fit"], r["scores"], small_db["lengths"][r["ids"]])
    assert r["zscores"].dtype == np.float64 and r["evalues"].dtype == np.float64 and len(r["evalues"]) == len(r["scores"])


@pytest.mark.parametrize("config", ["one", "three", "streamed"])
def test_driver_statistics(small_db, config):
    from cudasw4_amd import stats
    kw = {"one": {}, "three": dict(devices=[0, 0, 0]), "streamed": dict(max_gpu_mem=1, max_batch_bytes=200_000)}[config]
    d = _driver(small_db, **kw)
    if config == "streamed":
        assert not d.shard_info(0)["resident"]
    if config == "one":   # statistics off: what a scan returned before, and no table
        off = {qi: d.scan(small_db["letters"][qi]) for qi in QUERIES}
        for r in off.values():
            assert sorted(r) == ["gcups", "ids", "num_overflows", "num_rescored", "scores", "seconds"]
        with pytest.raises(Exception):
            d.last_statistics()
    d.set_statistics(True)
    for qi in QUERIES:
        r = d.scan(small_db["letters"][qi])
        _check_result(small_db, qi, r)
        # the table is that of every score the scan left, and the calibration holds on the GPU's scores
        ids, sc = d.all_scores()
        allsc = np.zeros(len(ids), dtype=np.int64)
        allsc[ids] = sc
        assert np.array_equal(allsc, small_db["want"][qi]["scores"])
        hist, sumlen, skipped = R.histogram(allsc, small_db["lengths"])
        assert skipped == 0 and np.array_equal(r["stats"]["hist"], hist) and np.array_equal(r["stats"]["sumlen"], sumlen)
        last = d.last_statistics()
        assert np.array_equal(last["hist"], hist) and last["a"] == r["stats"]["a"]
        if config == "one":
            fit = {k: v for k, v in r["stats"].items() if k not in ("hist", "sumlen")}
            _, e = stats.evalues(fit, allsc, small_db["lengths"])
            check_calibration(e, allsc, small_db["lengths"], small_db["nonfamily"], small_db["want"][qi]["self"], fit, stats.evalues)
            assert r["scores"].tolist() == off[qi]["scores"].tolist() and r["ids"].tolist() == off[qi]["ids"].tolist()
    if config == "one":
        d.set_statistics(False)
        assert "stats" not in d.scan(small_db["letters"][QUERIES[0]])
    d.close()


def test_driver_statistics_in_flight_and_pssm(small_db):
    from cudasw4_amd import pssm
    d = _driver(small_db)
    d.set_statistics(True)
    a, b = QUERIES
    d.submit(small_db["letters"][a])
    d.submit(small_db["letters"][b])
    with pytest.raises(Exception):
        d.set_statistics(False)      # not with queries in flight
    _check_result(small_db, a, d.collect())
    _check_result(small_db, b, d.collect())
    for qi in QUERIES:
        _check_result(small_db, qi, d.scan_pssm(pssm.from_sequence(small_db["codes"][qi], O.blosum21(62))))
    d.close()


def test_pseudo_db_has_no_fit():
    from cudasw4_amd import driver, stats
    d = driver.Driver(devices=[0], num_top=10)
    d.pseudo_db(2000, 512)
    d.set_statistics(True)
    _, letters = O.read_fasta(O.GOLDEN_DIR + "/allqueries.fasta")
    r = d.scan(letters[2])
    assert r["stats"]["status"] == stats.NO_FIT and r["stats"]["N"] == 2000
    assert r["evalues"].tolist() == [-1.0] * 10 and r["zscores"].tolist() == [0.0] * 10
    assert int(r["stats"]["hist"].sum()) == 2000 and int((r["stats"]["hist"] > 0).sum()) == 1
    d.close()


# ---- the command line -----------------------------------------------------------------------------------------------------

LETTERS = "ARNDCQEGHILKMFPSTWYV"


def test_align_evalues(small_db, tmp_path):
    from cudasw4_amd import driver
    chars, offsets, lengths = small_db["db"]
    fasta = str(tmp_path / "db.fa")
    lut = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    with open(fasta, "w") as f:
        for i in range(len(lengths)):   # the header carries the subject's position in the synthetic DB
            o = int(offsets[i])
            f.write(">s%d\n%s\n" % (i, lut[chars[o:o + int(lengths[i])]].tobytes().decode()))
    prefix = str(tmp_path / "sp")
    p = subprocess.run([driver.MAKEDB, fasta, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    qi = 12
    letters = small_db["letters"][qi]
    letters = letters.decode() if isinstance(letters, bytes) else letters
    qfile = str(tmp_path / "q.fa")
    with open(qfile, "w") as f:
        f.write(">query\n%s\n" % letters)

    def run(args, of, ok=True):
        r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", qfile, "--db", prefix, "--top", str(TOP), "--of", of]
                           + args, capture_output=True, text=True)
        if ok:
            assert r.returncode == 0, r.stderr[-2000:]
        return (open(of).read() if ok else ""), r

    d = driver.Driver(devices=[0], num_top=TOP)
    d.open_db(prefix)
    d.set_statistics(True)
    first = d.scan(letters)
    result, built, infos = d.iterate(letters, 2, max_evalue=1e-3)
    origin = {int(i): int(d.reference_header(int(i))[1:]) for i in first["ids"]}
    d.close()
    # the fit does not depend on the order makedb gave the subjects
    assert first["scores"].tolist() == O.topk(small_db["want"][qi]["scores"], TOP)[0].tolist()
    assert first["stats"]["n_included"] == small_db["want"][qi]["fit"]["n_included"]

    tsv, r = run(["--tsv", "--evalues", "--verbose"], str(tmp_path / "e.tsv"))
    lines = tsv.splitlines()
    assert lines[0].split("\t")[-2:] == ["Z-score", "E-value"] and len(lines) == 1 + TOP
    rows = [l.split("\t") for l in lines[1:]]
    assert [int(x[4]) for x in rows] == first["scores"].tolist() and [int(x[7]) for x in rows] == first["ids"].tolist()
    assert [x[-2] for x in rows] == ["%.2f" % z for z in first["zscores"]]
    assert [x[-1] for x in rows] == ["%.3g" % e for e in first["evalues"]]
    st = first["stats"]
    assert "statistics: N %d fitted on %d a " % (st["N"], st["n_included"]) in r.stdout and " rounds %d" % st["rounds"] in r.stdout
    # plain output carries the two values on the result line
    plain, _ = run(["--evalues"], str(tmp_path / "e.txt"))
    assert plain.splitlines()[1].endswith("referenceId %d Z-score: %.2f E-value: %.3g" % (first["ids"][0], first["zscores"][0], first["evalues"][0]))
    # --maxEvalue: only the results with E <= X, none of them outside the families
    tsv_m, _ = run(["--tsv", "--maxEvalue", "1e-3"], str(tmp_path / "m.tsv"))
    rows_m = [l.split("\t") for l in tsv_m.splitlines()[1:]]
    passing = [int(i) for i, e in zip(first["ids"], first["evalues"]) if e <= 1e-3]
    assert [int(x[7]) for x in rows_m] == passing and 0 < len(passing)
    assert not any(small_db["nonfamily"][origin[i]] for i in passing)
    assert tsv_m.splitlines()[0] == lines[0]
    # --inclusionEvalue: round 1 includes the results with E <= X that are neither the query's copy nor without a trace
    _, r_it = run(["--tsv", "--iterations", "2", "--inclusionEvalue", "1e-3", "--verbose"], str(tmp_path / "it.tsv"))
    per_round = [l for l in r_it.stdout.splitlines() if l.startswith("Query 0 round ")]
    assert len(per_round) == len(infos) == 2
    for line, info in zip(per_round, infos):
        assert " %d in the PSSM, %d above the inclusion E-value, %d without a trace, %d copies" % (
            info["used"], info["below_score"], info["no_trace"], info["copies"]) in line
    i0 = infos[0]
    assert set(i0["included"]) <= set(passing) and i0["used"] == len(passing) - i0["copies"] - i0["no_trace"]
    assert i0["below_score"] == TOP - len(passing) and i0["used"] == len(i0["included"]) > 0
    tsv_it = open(str(tmp_path / "it.tsv")).read()
    rows_it = [l.split("\t") for l in tsv_it.splitlines()[1:]]
    assert [int(x[4]) for x in rows_it] == result["scores"].tolist() and [int(x[7]) for x in rows_it] == result["ids"].tolist()
    # both inclusion rules at once: refused
    _, r_bad = run(["--iterations", "2", "--inclusionScore", "50", "--inclusionEvalue", "1e-3"], str(tmp_path / "bad.tsv"), ok=False)
    assert r_bad.returncode != 0 and "--inclusionEvalue" in r_bad.stderr
    # without the new flags: what a scan printed before
    tsv_p, r_p = run(["--tsv"], str(tmp_path / "p.tsv"))
    assert [l.split("\t") for l in tsv_p.splitlines()] == [x.split("\t")[:-2] for x in lines] and "statistics" not in r_p.stdout
