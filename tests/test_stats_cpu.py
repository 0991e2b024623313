"""Search statistics without a GPU: the host library's length bins, fit and E-values against the numpy
restatement in stats_ref.py, the calibration of the E-values on a small Swiss-Prot-like DB scored by the CPU oracle, and
degenerate tables."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import stats_ref as R

QUERIES = (0, 2, 7, 12, 19)


def _test1_lengths():
    ls = [1, 2, 3]
    for k in range(2, 29):
        ls += [2 ** k - 1, 2 ** k, 2 ** k + 2 ** (k - 1) - 1, 2 ** k + 2 ** (k - 1)]
    return ls


def test_length_bin_matches_reference():
    from cudasw4_amd import stats
    ls = _test1_lengths() + np.random.default_rng(11).integers(1, 2 ** 28 + 1, 10000).tolist()
    got = [stats.length_bin(l) for l in ls]
    assert got == [R.length_bin(l) for l in ls]
    assert got == R.length_bins(ls).tolist()      # (the vectorised form the other tests histogram with)
    assert stats.length_bin(2 ** 28) == 56 and stats.length_bin(1) == 0 and stats.length_bin(0) == 0 and stats.length_bin(-5) == 0
    assert [stats.length_bin(l) for l in (2, 3, 4, 5, 6, 7, 8)] == [2, 3, 4, 4, 5, 5, 6]


@pytest.fixture(scope="module")
def scored():
    """sprot_like(3000) scored by the CPU oracle for the five queries: computed once, shared, never changed."""
    from cudasw4_amd import synthdb
    chars, offsets, lengths, family = synthdb.sprot_like(n=3000, max_len=8000, return_family_ids=True)
    _, qs = O.load_queries()
    nonfamily = np.ones(len(lengths), dtype=bool)
    nonfamily[np.asarray(family, dtype=np.int64)] = False
    out = {}
    for qi in QUERIES:
        sc = O.scan(qs[qi], chars, offsets, lengths, simd=True).astype(np.int64)
        hist, sumlen, skipped = R.histogram(sc, lengths)
        assert skipped == 0 and int(hist.sum()) == len(lengths)
        out[qi] = {"scores": sc, "hist": hist, "sumlen": sumlen, "self": O.score(qs[qi], qs[qi])}
    return {"lengths": np.asarray(lengths), "nonfamily": nonfamily, "q": out}


def _close(a, b):
    return np.allclose(a, b, rtol=1e-9, atol=0.0)


def z_close(z, rz, st, scores, lengths):
    """A Z-score is the DIFFERENCE S - a - b1 ln L over sd and passes through zero, where no relative bound on the result
    can hold (the library's compiler may fuse the multiply-add, numpy does not): 1e-9 relative to its operands instead."""
    scale = (np.abs(np.asarray(scores, dtype=np.float64)) + abs(st["a"]) + abs(st["b1"]) * np.log(np.maximum(lengths, 1))) / st["sd"]
    return bool((np.abs(z - rz) <= 1e-9 * scale).all())


def test_fit_and_evalues_match_reference(scored):
    from cudasw4_amd import stats
    for qi, d in scored["q"].items():
        ref = R.fit(d["hist"], d["sumlen"])
        got = stats.from_histogram(d["hist"], d["sumlen"])
        print(qi, got)
        assert ref["status"] == R.OK
        for k in ("n_included", "rounds", "status", "N"):
            assert got[k] == ref[k], (qi, k, got, ref)
        for k in ("a", "b1", "sd"):
            assert abs(got[k] - ref[k]) <= 1e-9 * abs(ref[k]), (qi, k, got, ref)
        z, e = stats.evalues(got, d["scores"], scored["lengths"])
        rz, re_ = R.evalues(ref, d["scores"], scored["lengths"])
        assert _close(e, re_), qi
        assert z_close(z, rz, ref, d["scores"], scored["lengths"]), qi


def check_calibration(e, scores, lengths, nonfamily, self_score, stats_dict, evalues_fn):
    """The conditions of DESIGN.md §12 on one query's E-values over the whole DB."""
    assert not (e[nonfamily] <= 1e-3).any(), np.sort(e[nonfamily])[:5]
    assert int((e[nonfamily] <= 10).sum()) <= 40
    # the DB holds the query itself (cut at the DB's longest length where it is longer): the best-scoring subject
    top = int(np.argmax(scores))
    assert scores[top] >= 0.9 * self_score
    assert e[top] < 1e-30
    for length in (30, 290, 8000):
        _, es = evalues_fn(stats_dict, np.arange(0, 400), np.full(400, length))
        assert (np.diff(es) <= 0).all()


def test_calibration(scored):
    from cudasw4_amd import stats
    for qi, d in scored["q"].items():
        st = stats.from_histogram(d["hist"], d["sumlen"])
        _, e = stats.evalues(st, d["scores"], scored["lengths"])
        print(qi, "E<=10:", int((e[scored["nonfamily"]] <= 10).sum()), "min nonfamily E:", e[scored["nonfamily"]].min())
        check_calibration(e, d["scores"], scored["lengths"], scored["nonfamily"], d["self"], st, stats.evalues)


def _table(entries):
    """entries: (length, score, count)"""
    hist = np.zeros((R.LBINS, R.SBINS), dtype=np.uint32)
    sumlen = np.zeros(R.LBINS, dtype=np.uint64)
    for length, score, count in entries:
        b = R.length_bin(length)
        hist[b, min(score, 255)] += count
        sumlen[b] += np.uint64(length * count)
    return hist, sumlen


def test_degenerate_tables():
    from cudasw4_amd import stats

    def both(entries):
        hist, sumlen = _table(entries)
        got, ref = stats.from_histogram(hist, sumlen), R.fit(hist, sumlen)
        assert got["status"] == ref["status"] and got["N"] == ref["N"] and got["rounds"] == ref["rounds"], (got, ref)
        return got

    st = both([])
    assert st["status"] == stats.NO_FIT and st["N"] == 0
    z, e = stats.evalues(st, [50, 0], [300, 20])
    assert z.tolist() == [0.0, 0.0] and e.tolist() == [-1.0, -1.0]
    # one populated bin, varied scores: no slope, but a fit
    st = both([(300, s, 10) for s in range(30, 50)])
    assert st["status"] == stats.OK and st["b1"] == 0.0 and abs(st["a"] - 39.5) < 1e-12 and st["sd"] > 0 and st["n_included"] == 200
    # every subject the same score (the pseudo DB: one sequence many times): var = 0
    st = both([(512, 41, 2000)])
    assert st["status"] == stats.NO_FIT and st["N"] == 2000
    # 99 eligible entries are too few, 100 are enough
    few = [(100, 30, 25), (100, 32, 25), (1000, 40, 25), (1000, 43, 24)]
    st = both(few + [(1000, 0, 500), (1000, 255, 500)])
    assert st["status"] == stats.NO_FIT and st["n_included"] == 99 and st["N"] == 1099
    st = both(few + [(1000, 43, 1)])
    assert st["status"] == stats.OK and st["n_included"] == 100 and st["b1"] > 0
    # only "no alignment" and censored scores
    st = both([(100, 0, 5000), (1000, 255, 5000), (3000, 300, 10)])
    assert st["status"] == stats.NO_FIT and st["n_included"] == 0 and st["N"] == 10010


def test_stats_header_symbols_are_exported():
    import ctypes
    import re
    from cudasw4_amd import capi, driver
    text = open(os.path.join(O.ROOT, "include", "cudasw4_amd_stats.h")).read()
    declared = set(re.findall(r"^[a-z_0-9 *]*\b(sw_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(capi.STATS_EXPORTS) == {"sw_score_histogram"} and not (declared & set(capi.EXPORTS))
    assert '#include "cudasw4_amd.h"' in text and "sw_score_histogram" not in open(os.path.join(O.ROOT, "include", "cudasw4_amd.h")).read()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "sw_score_histogram")
    assert "#define SW_STATS_LBINS %d" % R.LBINS in text and "#define SW_STATS_SBINS %d" % R.SBINS in text
    with pytest.raises(capi.SwError):   # a null context needs no GPU to be refused
        capi.score_histogram(None, 0, 0, 1, 0, 0, 0)
    # the host driver without its kernel library's tap: the driver sources name no new entry point of the kernel library
    for name in ("search_driver.cpp", "driver_capi.cpp"):
        assert "sw_score_histogram" not in open(os.path.join(O.ROOT, "cudasw4_amd", "csrc", "host", name)).read()
    assert driver.STATS_LBINS == R.LBINS and driver.STATS_SBINS == R.SBINS


def test_align_refuses_both_inclusion_rules(golden_dir):
    from cudasw4_amd import driver
    fasta = os.path.join(golden_dir, "allqueries.fasta")
    prefix = os.path.join(golden_dir, "allqueries_db", "aq")
    out = subprocess.run([driver.ALIGN, "--query", fasta, "--db", prefix, "--iterations", "2", "--inclusionScore", "50",
                          "--inclusionEvalue", "1e-3"], capture_output=True, text=True)
    assert out.returncode != 0 and "--inclusionEvalue" in out.stderr and "No GPU found" not in out.stderr
    out = subprocess.run([driver.ALIGN, "--help"], capture_output=True, text=True)
    for flag in ("--evalues", "--maxEvalue", "--inclusionEvalue"):
        assert flag in out.stdout, flag
    assert "there are no E-values" not in out.stdout
    # the option dump names the new flags only when they are used
    out = subprocess.run([driver.ALIGN, "--query", "q.fa", "--db", "x"], capture_output=True, text=True)
    for word in ("evalues", "maxEvalue", "inclusionEvalue"):
        assert word not in out.stdout, word
