"""Statistics calibrated on shuffled subjects without a GPU: the host library's permutation, sample and
replica rules against the numpy restatement in shuffle_ref.py; what the calibration is for — a family-dominated and a
small database, scored by the CPU oracle; its agreement with the scan's own fit where that one is sound; the command line's
argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import shuffle_cases as C
import shuffle_ref as SR
import stats_ref as R

PERM_LENGTHS = list(range(0, 301)) + [511, 512, 513, 1023, 1024, 1025, 4096, 4097, 35213, 70001]


def test_permutation_matches_reference_and_is_a_bijection():
    from cudasw4_amd import stats
    worst = 0
    for k, length in enumerate(PERM_LENGTHS):
        seed, sid, rep = 2024 + k % 3, (k * 7919) if k % 2 else (1 << 33) + k, k % 5
        ref, passes = SR.permutation(length, seed, sid, rep, with_passes=True)
        worst = max(worst, passes)
        got = stats.shuffle_permutation(length, seed, sid, rep)
        assert got.dtype == np.int32 and got.tolist() == ref.tolist(), length
        assert np.array_equal(np.sort(ref), np.arange(length)), length
    print("most passes of a walk:", worst)
    assert worst < 64
    # the key: every one of seed, both halves of the id and the replica matters
    base = stats.shuffle_permutation(300, 1, 5, 0).tolist()
    for other in ((2, 5, 0), (1, 6, 0), (1, 5 + (1 << 32), 0), (1, 5, 1)):
        assert stats.shuffle_permutation(300, *other).tolist() != base, other
    assert SR.mix32(0) == 0 and SR.mix32(1) == 0x514E28B7   # (the finaliser of MurmurHash3)
    assert [SR.half_bits(l) for l in (2, 3, 4, 5, 16, 17, 256, 257, 70001)] == [1, 1, 1, 2, 2, 3, 4, 5, 9]


def test_shuffled_block_keeps_composition_and_pads_with_code_20():
    rng = np.random.default_rng(3)
    seqs = [rng.integers(0, 21, l, dtype=np.int8) for l in (0, 1, 2, 3, 5, 64, 65, 301, 1023)]
    chars, offsets, lengths = O.make_db(seqs)
    keys = np.arange(len(seqs), dtype=np.int64) * 1000003 + (1 << 32)
    out = SR.shuffle_block(chars, offsets, lengths, 2024, keys=keys, replicas=3)
    assert out.shape == (3, len(chars))
    moved = 0
    for r in range(3):
        for i, s in enumerate(seqs):
            b, e = int(offsets[i]), int(offsets[i + 1])
            got = out[r, b:b + len(s)]
            assert np.array_equal(np.bincount(got, minlength=21), np.bincount(s, minlength=21)), (r, i)
            assert (out[r, b + len(s):e] == SR.OTHER).all(), (r, i)
            pi = SR.permutation(len(s), 2024, keys[i], r)
            assert np.array_equal(got, s[pi])
            moved += int((pi != np.arange(len(s))).sum())
    assert moved > 0.9 * 3 * sum(len(s) for s in seqs)
    assert not np.array_equal(out[0], out[1]) and np.array_equal(chars, O.make_db(seqs)[0])   # the input is unchanged
    # keys None: the position within the range; a sub-range has offsets relative to its first subject
    sub = SR.shuffle_block(chars, offsets, lengths, 7, first=4, n=3)
    whole = SR.shuffle_block(*O.make_db(seqs[4:7]), 7)
    assert np.array_equal(sub, whole)


def test_sample_and_replica_rules():
    from cudasw4_amd import stats
    for n, m in ((7, 10), (10, 10), (11, 10), (10 ** 7, 10 ** 4), (12345, 1), (1, 1), (0, 5), (3000, 10000)):
        got, ref = stats.shuffle_sample(n, m), SR.sample_ids(n, m)
        assert got.dtype == np.int64 and got.tolist() == ref.tolist(), (n, m)
        assert len(got) == min(n, m)
        if len(got):
            assert (np.diff(got) > 0).all() and got[0] >= 0 and got[-1] < n, (n, m)
        if n <= m:
            assert got.tolist() == list(range(n))
    assert stats.shuffle_sample(11, 10).tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]
    assert stats.shuffle_sample(12345, 1).tolist() == [6172]
    assert stats.shuffle_sample(10 ** 7, 10 ** 4)[:3].tolist() == [500, 1500, 2500]
    # the default rule and its two clamps; a given number is taken as it is
    for m, want in ((1, 64), (31, 64), (32, 63), (63, 32), (600, 4), (1000, 2), (1999, 2), (2000, 1), (2001, 1), (10 ** 7, 1)):
        assert stats.shuffle_replicas(m) == want == SR.replicas_for(m), m
    assert stats.shuffle_replicas(5, 1) == 1 and stats.shuffle_replicas(10 ** 6, 64) == 64 == SR.replicas_for(10 ** 6, 64)
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            stats.shuffle_replicas(100, bad)
    from cudasw4_amd import driver
    with pytest.raises(driver.DriverError):
        stats.shuffle_sample(10, 0)


def test_family_dominated_database():
    c = C.case("family")
    rel, scan, cal = c["relative"], c["scan_fit"], c["cal_fit"]
    assert len(rel) == 600 and int(rel.sum()) == 240
    print("relatives score", c["scores"][rel].min(), "...", c["scores"][rel].max(), "unrelated at most", c["scores"][~rel].max())
    print("scan fit", scan)
    print("calibrated", c["stats"])
    # the scan's own fit is the family's: nothing is significant
    _, e = R.evalues(scan, c["scores"], c["lengths"])
    assert scan["status"] == R.OK and scan["sd"] > 20
    assert not (e[rel] <= 1).any()
    # the calibrated fit is that of unrelated subjects
    assert cal["status"] == R.OK and cal["N"] == 2400 and c["stats"]["N"] == 600
    assert 4 <= cal["sd"] <= 5.5
    print("largest E of a relative", c["e"][rel].max(), "smallest E of an unrelated subject", c["e"][~rel].min())
    assert (c["e"][rel] <= 1e-3).all()
    assert not (c["e"][~rel] <= 1).any()


def test_small_database():
    c = C.case("small")
    rel, scan, cal = c["relative"], c["scan_fit"], c["cal_fit"]
    assert len(rel) == 63 and int(rel.sum()) == 3
    print("scan fit", scan)
    print("calibrated", c["stats"])
    assert scan["status"] == R.NO_FIT
    assert cal["status"] == R.OK and cal["N"] == 63 * 32 and c["stats"]["N"] == 63
    print("largest E of a relative", c["e"][rel].max(), "smallest E of an unrelated subject", c["e"][~rel].min())
    assert (c["e"][rel] <= 1e-3).all()
    assert not (c["e"][~rel] <= 1).any()
    # the host library's fit of the reference's table is the reference's fit
    from cudasw4_amd import stats
    got = stats.from_histogram(c["cal_hist"], c["cal_sumlen"])
    for k in ("n_included", "rounds", "status", "N"):
        assert got[k] == cal[k], k
    for k in ("a", "b1", "sd"):
        assert abs(got[k] - cal[k]) <= 1e-9 * abs(cal[k]), k


def test_agrees_with_the_scan_fit_on_a_database_of_unrelated_subjects():
    """sprot_like(3000), one shuffle per subject: the two regression lines within 1.0 score units at L = 100 and L = 1600
    (measured: 0.4), sd within 10 % (measured: 4.5 %)."""
    from cudasw4_amd import synthdb
    chars, offsets, lengths = synthdb.sprot_like(n=3000, max_len=8000)
    _, qs = O.load_queries()
    for qi in (2, 12):
        q = qs[qi]
        sc = O.scan(q, chars, offsets, lengths, simd=True).astype(np.int64)
        scan = R.fit(*R.histogram(sc, lengths)[:2])
        _, _, cal, m, reps = SR.calibrate(lambda c, o, l: O.scan(q, c, o, l, simd=True), chars, offsets, lengths, C.SHUFFLE_SEED,
                                          shuffles=1)
        assert (m, reps) == (3000, 1) and scan["status"] == cal["status"] == R.OK
        for length in (100, 1600):
            d = abs((scan["a"] + scan["b1"] * np.log(length)) - (cal["a"] + cal["b1"] * np.log(length)))
            print(qi, "L", length, "lines differ by", d)
            assert d <= 1.0, (qi, length, scan, cal)
        print(qi, "sd", scan["sd"], cal["sd"])
        assert abs(scan["sd"] - cal["sd"]) <= 0.10 * scan["sd"], (qi, scan, cal)
        stats = SR.calibrated(cal, scan["N"])
        for x in (1e-3,):
            counts = [int((R.evalues(st, sc, lengths)[1] <= x).sum()) for st in (scan, stats)]
            print(qi, "subjects at E <=", x, counts)
            assert counts[0] == counts[1]


def test_shuffle_header_symbols_are_exported():
    import ctypes
    from cudasw4_amd import capi, driver
    text = open(os.path.join(O.ROOT, "include", "cudasw4_amd_shuffle.h")).read()
    declared = set(re.findall(r"^[a-z_0-9 *]*\b(sw_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(capi.SHUFFLE_EXPORTS) == {"sw_shuffle_subjects"}
    assert not (declared & (set(capi.EXPORTS) | set(capi.PSSM_EXPORTS) | set(capi.STATS_EXPORTS) | set(capi.RANK_EXPORTS) | set(capi.HSPS_EXPORTS)))
    assert "sw_shuffle_subjects" not in open(os.path.join(O.ROOT, "include", "cudasw4_amd.h")).read()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "sw_shuffle_subjects")
    with pytest.raises(capi.SwError) as e:   # a null context needs no GPU to be refused
        capi.shuffle_subjects(None, 0, 0, 0, 1, 1, 0, 0)
    assert e.value.code == -1
    host = ctypes.CDLL(driver.LIB_PATH)
    for name in ("swdrv_calibrate_shuffled", "swdrv_calibrate_shuffled_pssm", "swdrv_set_rank_fit", "swdrv_shuffle_sample",
                 "swdrv_shuffle_replicas", "swdrv_shuffle_permutation"):
        assert name in driver.EXPORTS and hasattr(host, name), name
    # the files of the fake-runtime build name neither the kernel nor the calibrator
    for name in ("search_driver.cpp", "driver_capi.cpp"):
        body = open(os.path.join(O.ROOT, "cudasw4_amd", "csrc", "host", name)).read()
        assert "sw_shuffle_subjects" not in body and "shuffle_stats.hpp" not in body, name
    assert hasattr(driver.Driver, "calibrate")


def test_align_refuses_malformed_shuffle_flags(golden_dir):
    from cudasw4_amd import driver
    fasta = os.path.join(golden_dir, "allqueries.fasta")
    prefix = os.path.join(golden_dir, "allqueries_db", "aq")
    base = [driver.ALIGN, "--query", fasta, "--db", prefix]
    cases = [
        (["--statistics", "permuted"], "--statistics"),
        (["--statistics", "shuffled", "--shuffles", "0"], "--shuffles"),
        (["--statistics", "shuffled", "--shuffles", "65"], "--shuffles"),
        (["--statistics", "shuffled", "--shuffleSubjects", "0"], "--shuffleSubjects"),
        (["--shuffles", "4"], "--statistics shuffled"),
        (["--shuffleSubjects", "100"], "--statistics shuffled"),
        (["--shuffleSeed", "7"], "--statistics shuffled"),
        (["--statistics", "scan", "--shuffles", "4"], "--statistics shuffled"),
        (["--statistics", "shuffled", "--interactive"], "--interactive"),
    ]
    for extra, word in cases:
        out = subprocess.run(base + extra, capture_output=True, text=True)
        assert out.returncode != 0 and word in out.stderr and "No GPU found" not in out.stderr, (extra, out.stderr)
    out = subprocess.run([driver.ALIGN, "--help"], capture_output=True, text=True)
    for flag in ("--statistics scan|shuffled", "--shuffles", "--shuffleSubjects", "--shuffleSeed"):
        assert flag in out.stdout, flag
    # the option dump names the new flags only when they are used
    out = subprocess.run(base[:1] + ["--query", "q.fa", "--db", "x"], capture_output=True, text=True)
    for word in ("statistics", "shuffle"):
        assert word not in out.stdout, word
    out = subprocess.run(base[:1] + ["--query", "q.fa", "--db", "x", "--statistics", "shuffled", "--shuffles", "4"], capture_output=True, text=True)
    assert "statistics: shuffled" in out.stdout and "shuffles: 4" in out.stdout and "evalues: 1" in out.stdout
