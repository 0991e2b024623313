"""Ranking by E-value without a GPU: the conditions the GPU tests rely on (checked on the oracle's scores),
the threshold's Z-score and the host merge against rank_ref.py, the exported symbols, and `align`'s flag."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rank_cases as C
import rank_ref as K
import stats_ref as R

HOST = os.path.join(O.ROOT, "cudasw4_amd", "csrc", "host")


def test_reference_inputs():
    """What test_gpu_rank.py takes for granted of sprot_like(3000): the Z list is not the raw-score list; no two distinct z
    straddle the k-th place within tol (so the list is exact as a set); no z lies within tol of z_min(10) (so the count is)."""
    db = C.small_db()
    least = {9: 1, 4: 5}
    for qi, k in C.CASES:
        w = db["want"][qi]
        assert w["fit"]["status"] == R.OK
        _, raw_ids = O.topk(w["scores"], k)
        differ = len(set(w["ranked_ids"].tolist()) - set(raw_ids.tolist()))
        gap = K.boundary_gap(w["fit"], w["scores"], db["lengths"], k)
        zs = np.sort(w["z"])[::-1]
        near = K.min_distance_to(w["z"], w["z_min"])
        print("query %d k %d: %d subjects of the Z list not in the raw-score list, z gap at the boundary %.4g (%.3g tol), "
              "closest z to z_min(10) = %.6g: %.3g tol, count %d" % (qi, k, differ, zs[k - 1] - zs[k], gap, w["z_min"], near, w["count"]))
        assert differ >= least[qi]
        assert gap >= 1.0
        assert near >= 1.0
        assert 0 < w["count"] < len(db["lengths"])


def test_zscore_for_evalue_inverts_the_evalue():
    from cudasw4_amd import driver
    for N in (100, 3000, 570000, 10 ** 9):
        st = {"a": 0.0, "b1": 0.0, "sd": 1.0, "N": N, "status": R.OK}
        xs = np.concatenate([10.0 ** np.arange(-30, 1), np.array([0.5, 3.0, 10.0, N / 7.0, N / 2.0])])
        xs = xs[xs <= N / 2.0]
        for x in xs:
            z = driver.zscore_for_evalue(N, float(x))
            assert np.isfinite(z)
            assert abs(z - K.z_min(N, float(x))) <= 1e-12 * max(1.0, abs(z))
            _, e = R.evalues(st, np.array([z]), np.array([1]))     # (a = b1 = 0, sd = 1: the score IS the z)
            assert abs(e[0] - x) <= 1e-9 * x, (N, x, e[0])
        for x in (N, N + 0.5, 10.0 * N, np.inf):
            assert driver.zscore_for_evalue(N, float(x)) == -np.inf
        assert driver.zscore_for_evalue(N, 0.0) == np.inf and driver.zscore_for_evalue(N, -1.0) == np.inf
        assert np.isnan(driver.zscore_for_evalue(N, np.nan))
    assert np.isnan(driver.zscore_for_evalue(0, 1.0))


def test_rank_order_matches_lexsort():
    from cudasw4_amd import driver, stats
    rng = np.random.default_rng(17)
    st = {"a": 21.5, "b1": 4.75, "sd": 5.25, "n_included": 5000, "N": 6000, "rounds": 3, "status": R.OK}
    for n in (0, 1, 2, 7, 200, 5000):
        scores = rng.integers(0, 300, n).astype(np.int32)
        lengths = rng.integers(1, 9000, n).astype(np.int32)
        ids = rng.permutation(10 * n + 5)[:n].astype(np.int64)
        # planted exact ties: runs of equal (score, length) — equal double z — under distinct ids
        for start in range(0, n - 4, 37):
            scores[start:start + 4] = scores[start]
            lengths[start:start + 4] = lengths[start]
        got = driver.rank_order(st, scores, lengths, ids)
        z = K.zscores(st, scores, lengths)
        want = K.order(z, ids)
        assert got.tolist() == want.tolist(), n
        if n >= 200:
            assert (np.diff(z[got]) == 0).sum() >= 3 * ((n - 4) // 37)     # (the ties are there)
            lz, _ = stats.evalues(st, scores, lengths)
            assert np.array_equal(np.lexsort((ids, -lz)), got)            # the library's own z gives the same order
    # without a fit: the order of a score-ranked list
    nofit = dict(st, status=R.NO_FIT, sd=0.0)
    scores = rng.integers(0, 40, 500).astype(np.int32)
    ids = rng.permutation(500).astype(np.int64)
    got = driver.rank_order(nofit, scores, np.full(500, 100, np.int32), ids)
    assert got.tolist() == np.lexsort((ids, -scores.astype(np.int64))).tolist()
    with pytest.raises(ValueError):
        driver.rank_order(st, [1, 2], [3], [4, 5])


def test_rank_symbols_are_declared_and_exported():
    from cudasw4_amd import capi, driver
    text = open(os.path.join(O.ROOT, "include", "cudasw4_amd_rank.h")).read()
    declared = set(re.findall(r"^[a-z_0-9 *]*\b(sw_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(capi.RANK_EXPORTS) == {"sw_zscore_keys", "sw_gather_hits"}
    assert not (declared & (set(capi.EXPORTS) | set(capi.STATS_EXPORTS) | set(capi.PSSM_EXPORTS)))
    assert '#include "cudasw4_amd.h"' in text and "#define SW_RANK_KEY_NONE (-3.0e38f)" in text
    assert np.float32(capi.RANK_KEY_NONE) == K.KEY_NONE
    for other in ("cudasw4_amd.h", "cudasw4_amd_stats.h", "cudasw4_amd_engine.h", "cudasw4_amd_pssm.h"):
        body = open(os.path.join(O.ROOT, "include", other)).read()
        assert "sw_zscore_keys" not in body and "sw_gather_hits" not in body, other
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    # the driver's C ABI
    header = open(os.path.join(O.ROOT, "include", "cudasw4_amd_driver.h")).read()
    assert set(re.findall(r"\b(swdrv_[a-z_0-9]+)\s*\(", header)) == set(driver.EXPORTS)
    host = ctypes.CDLL(driver.LIB_PATH)
    for name in ("swdrv_set_ranking", "swdrv_last_ranking", "swdrv_zscore_for_evalue", "swdrv_rank_order"):
        assert name in driver.EXPORTS and hasattr(host, name), name
    assert "#define SWDRV_RANK_SCORE %d" % driver.RANK_SCORE in header and "#define SWDRV_RANK_EVALUE %d" % driver.RANK_EVALUE in header
    # the driver reaches the two kernels through function pointers: the files of the fake-runtime build name neither
    for name in ("search_driver.cpp", "driver_capi.cpp"):
        body = open(os.path.join(HOST, name)).read()
        assert "sw_zscore_keys" not in body and "sw_gather_hits" not in body and "cudasw4_amd_rank.h" not in body, name
    assert hasattr(driver.Driver, "set_ranking") and hasattr(driver.Driver, "last_ranking")


def test_null_context_is_refused_without_a_gpu():
    from cudasw4_amd import capi
    with pytest.raises(capi.SwError) as e:
        capi.zscore_keys(None, 4096, 4096, 1, 0.0, 1.0, 1.0, 0.0, 4096, 4096, 4096)
    assert e.value.code == -1 and "sw_zscore_keys" in str(e.value)
    with pytest.raises(capi.SwError) as e:
        capi.gather_hits(None, 4096, 1, 4096, 4096, 4096, 4096)
    assert e.value.code == -1 and "sw_gather_hits" in str(e.value)


def test_align_rank_by_flag(golden_dir):
    from cudasw4_amd import driver
    fasta = os.path.join(golden_dir, "allqueries.fasta")
    prefix = os.path.join(golden_dir, "allqueries_db", "aq")
    # an unknown value is refused before any device is opened
    out = subprocess.run([driver.ALIGN, "--query", fasta, "--db", prefix, "--rankBy", "length"], capture_output=True, text=True)
    assert out.returncode != 0 and "--rankBy" in out.stderr and "length" in out.stderr and "No GPU found" not in out.stderr
    assert "rankBy: length" in out.stdout
    out = subprocess.run([driver.ALIGN, "--help"], capture_output=True, text=True)
    assert "--rankBy score|evalue" in out.stdout
    # the option dump names the flag only when it is used; evalue implies --evalues
    out = subprocess.run([driver.ALIGN, "--query", "q.fa", "--db", "x"], capture_output=True, text=True)
    assert "rankBy" not in out.stdout and "evalues" not in out.stdout
    out = subprocess.run([driver.ALIGN, "--query", "q.fa", "--db", "x", "--rankBy", "evalue"], capture_output=True, text=True)
    assert "rankBy: evalue" in out.stdout and "evalues: 1" in out.stdout and "maxEvalue" not in out.stdout
    out = subprocess.run([driver.ALIGN, "--query", "q.fa", "--db", "x", "--rankBy", "score"], capture_output=True, text=True)
    assert "rankBy: score" in out.stdout and "evalues" not in out.stdout
    # not with --interactive (refused before any device is opened)
    out = subprocess.run([driver.ALIGN, "--db", prefix, "--interactive", "--rankBy", "evalue"], capture_output=True, text=True,
                         stdin=subprocess.DEVNULL)
    assert out.returncode != 0 and "--interactive" in out.stderr and "No GPU found" not in out.stderr


def test_python_set_ranking_checks_its_arguments():
    """(the checks that need no driver handle)"""
    from cudasw4_amd import driver
    d = driver.Driver.__new__(driver.Driver)
    d.handle, d.ranking, d.max_evalue, d.statistics = None, "score", None, False
    for bad in (dict(by="length"), dict(by="score", max_evalue=1.0), dict(by="evalue", max_evalue=0.0), dict(by="evalue", max_evalue=-3)):
        with pytest.raises(ValueError):
            d.set_ranking(**bad)
