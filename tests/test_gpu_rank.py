"""Ranking by E-value on the GPU: the key and gather kernels on bare arrays, keys -> sw_topk -> gather on the
oracle's scores, the driver in every scan mode against rank_ref.py, its refusals and its fallback, alignment and PSSM building
on a ranked list, and `align --rankBy`."""
import subprocess
import sys

import numpy as np
import pytest

import align_ref as A
import oracle_lib as O
import rank_cases as C
import rank_ref as K
import stats_ref as R
from test_stats_cpu import z_close

pytestmark = pytest.mark.gpu

NS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099)
SCORES = np.array([-2, -1, 0, 1, 254, 255, 30000], dtype=np.float32)
LENGTHS = np.array([0, 1, 2, 3, 2 ** 28], dtype=np.int32)
FIT = {"a": 11.25, "b1": 4.875, "sd": 5.0625, "N": 570000, "n_included": 560000, "rounds": 3, "status": R.OK}
Z_MIN = 2.0
NO_THRESHOLD = -sys.float_info.max
PAD = 8
SENTINEL = 7777.0


def _inputs(n):
    """every (score, length) pair of the two lists from n = 35 on (7 and 5 are coprime), shorter ones start elsewhere"""
    i = np.arange(n)
    return SCORES[(i + n) % len(SCORES)], LENGTHS[(i + 2 * n) % len(LENGTHS)]


def _expected(scores, lengths, z_min=Z_MIN):
    z = K.zscores(FIT, np.maximum(scores, 0).astype(np.float64), lengths)
    real = scores >= 0
    return K.keys(FIT, scores, lengths), real, int((real & (z >= z_min)).sum()), z


def _check_keys(got, scores, lengths):
    want, real, _, _ = _expected(scores, lengths)
    assert np.array_equal(got[~real].view(np.uint32), np.full(int((~real).sum()), K.KEY_NONE).view(np.uint32))   # bit-exact
    assert (np.abs(got[real].astype(np.float64) - want[real].astype(np.float64)) <= np.spacing(np.abs(want[real])).astype(np.float64)).all()
    assert np.isfinite(got).all()


@pytest.fixture(scope="module")
def gpu():
    import torch
    from cudasw4_amd import capi
    ctx = capi.Context(0)
    yield torch, capi, ctx
    ctx.close()


def test_inputs_keep_clear_of_the_threshold():
    """the count is exact only where no z lies within tol of z_min: true of every (score, length) pair of the kernel tests"""
    s, l = _inputs(35)
    _, real, _, z = _expected(s, l)
    assert len(set(zip(s.tolist(), l.tolist()))) == 35
    assert K.min_distance_to(z[real], Z_MIN) >= 1.0
    assert 0 < int((real & (z >= Z_MIN)).sum()) < int(real.sum())


def test_zscore_keys_kernel(gpu):
    torch, capi, ctx = gpu
    dev = "cuda:0"
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    for n in NS:
        scores, lengths = _inputs(n)
        want_keys, real, want_count, _ = _expected(scores, lengths)
        # the inputs at every element shift behind a 256-byte boundary
        s_at, l_at = [], []
        for shift in range(4):
            s = torch.zeros(n + PAD, dtype=torch.float32, device=dev)
            l = torch.zeros(n + PAD, dtype=torch.int32, device=dev)
            s[shift:shift + n] = torch.from_numpy(scores).to(dev)
            l[shift:shift + n] = torch.from_numpy(lengths).to(dev)
            s_at.append(s)
            l_at.append(l)
        for ss in range(4):
            for ls in range(4):
                for ks in range(4):
                    keys = torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device=dev)
                    pos = torch.full((n + PAD,), -7, dtype=torch.int32, device=dev)
                    ps = (ks + ss) % 4          # the positions aligned differently from the keys, too
                    count.zero_()
                    capi.zscore_keys(ctx, s_at[ss].data_ptr() + 4 * ss, l_at[ls].data_ptr() + 4 * ls, n, FIT["a"], FIT["b1"], FIT["sd"],
                                     Z_MIN, keys.data_ptr() + 4 * ks, pos.data_ptr() + 4 * ps, count.data_ptr())
                    k, p = keys.cpu().numpy(), pos.cpu().numpy()
                    where = (n, ss, ls, ks)
                    assert int(count.cpu()[0]) == want_count, where
                    _check_keys(k[ks:ks + n], scores, lengths)
                    assert np.array_equal(p[ps:ps + n], np.arange(n, dtype=np.int32)), where
                    # nothing outside the n entries was written
                    assert (k[:ks] == SENTINEL).all() and (k[ks + n:] == SENTINEL).all(), where
                    assert (p[:ps] == -7).all() and (p[ps + n:] == -7).all(), where


def test_zscore_keys_adds_and_takes_no_positions(gpu):
    torch, capi, ctx = gpu
    dev = "cuda:0"
    rng = np.random.default_rng(3)
    n = 70001
    scores = rng.integers(-2, 400, n).astype(np.float32)
    lengths = rng.integers(1, 36000, n).astype(np.int32)
    _, real, want_count, z = _expected(scores, lengths)
    assert K.min_distance_to(z[real], Z_MIN) >= 1.0
    s, l = torch.from_numpy(scores).to(dev), torch.from_numpy(lengths).to(dev)
    keys = torch.zeros(n, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    args = (ctx, s.data_ptr(), l.data_ptr(), n, FIT["a"], FIT["b1"], FIT["sd"])
    capi.zscore_keys(*args, Z_MIN, keys.data_ptr(), 0, count.data_ptr())       # positions = NULL
    assert int(count.cpu()[0]) == want_count
    capi.zscore_keys(*args, Z_MIN, keys.data_ptr(), 0, count.data_ptr())       # two calls add
    assert int(count.cpu()[0]) == 2 * want_count
    _check_keys(keys.cpu().numpy(), scores, lengths)
    count.zero_()
    capi.zscore_keys(*args, NO_THRESHOLD, keys.data_ptr(), 0, count.data_ptr())   # no threshold: every scored subject
    assert int(count.cpu()[0]) == int(real.sum())


def test_zscore_keys_count_worst_case(gpu):
    """300 000 equal entries, all above z_min: every lane of every wave counts"""
    torch, capi, ctx = gpu
    dev = "cuda:0"
    n = 300000
    s = torch.full((n,), 90.0, dtype=torch.float32, device=dev)
    l = torch.full((n,), 290, dtype=torch.int32, device=dev)
    keys = torch.zeros(n, dtype=torch.float32, device=dev)
    pos = torch.zeros(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    z = K.zscores(FIT, np.array([90.0]), np.array([290]))[0]
    assert z > Z_MIN + 1
    capi.zscore_keys(ctx, s.data_ptr(), l.data_ptr(), n, FIT["a"], FIT["b1"], FIT["sd"], Z_MIN, keys.data_ptr(), pos.data_ptr(),
                     count.data_ptr())
    assert int(count.cpu()[0]) == n
    k = keys.cpu().numpy()
    assert (k == k[0]).all() and abs(float(k[0]) - float(np.float32(z))) <= float(np.spacing(np.float32(z)))
    assert np.array_equal(pos.cpu().numpy(), np.arange(n, dtype=np.int32))


def test_zscore_keys_argument_edges(gpu):
    torch, capi, ctx = gpu
    dev = "cuda:0"
    n = 100
    s = torch.full((n,), 50.0, dtype=torch.float32, device=dev)
    l = torch.full((n,), 300, dtype=torch.int32, device=dev)
    keys = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    pos = torch.full((n,), -7, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    good = dict(scores=s.data_ptr(), lengths=l.data_ptr(), n=n, a=FIT["a"], b1=FIT["b1"], sd=FIT["sd"], z_min=Z_MIN, keys=keys.data_ptr(),
                positions=pos.data_ptr(), count=count.data_ptr())
    nan, inf = float("nan"), float("inf")
    refused = [dict(sd=0.0), dict(sd=-1.0), dict(sd=nan), dict(sd=inf), dict(a=nan), dict(a=inf), dict(b1=nan), dict(b1=-inf),
               dict(z_min=nan), dict(z_min=-inf), dict(z_min=inf), dict(n=-1), dict(n=2 ** 31), dict(n=2 ** 40),
               dict(scores=0), dict(lengths=0), dict(keys=0), dict(count=0),
               dict(scores=s.data_ptr() + 2), dict(lengths=l.data_ptr() + 1), dict(keys=keys.data_ptr() + 2),
               dict(positions=pos.data_ptr() + 3), dict(count=count.data_ptr() + 4)]
    for change in refused:
        with pytest.raises(capi.SwError) as e:
            capi.zscore_keys(ctx, **dict(good, **change))
        assert e.value.code == -1, change
    torch.cuda.synchronize()
    # nothing was launched
    assert (keys.cpu().numpy() == SENTINEL).all() and (pos.cpu().numpy() == -7).all() and count.cpu().tolist() == [0, 0]
    # n = 0 is a no-op, also with null pointers; the good arguments pass
    capi.zscore_keys(ctx, **dict(good, n=0, scores=0, lengths=0, keys=0, positions=0, count=0))
    capi.zscore_keys(ctx, **good)
    assert count.cpu().tolist() == [n, 0] and (keys.cpu().numpy() != SENTINEL).all()


def test_gather_hits(gpu):
    torch, capi, ctx = gpu
    dev = "cuda:0"
    n = 1000
    scores = np.arange(n, dtype=np.float32) * 3 + 1
    ids = (np.arange(n, dtype=np.int32) * 7 + 11)
    s, i = torch.from_numpy(scores).to(dev), torch.from_numpy(ids).to(dev)
    positions = np.array([5, -1, 0, n - 1, -1, 5] + list(range(300, 600)), dtype=np.int32)     # (more than one workgroup)
    k = len(positions)
    p = torch.from_numpy(positions).to(dev)
    out_s = torch.full((k + 2,), SENTINEL, dtype=torch.float32, device=dev)
    out_i = torch.full((k + 2,), -7, dtype=torch.int32, device=dev)
    capi.gather_hits(ctx, p.data_ptr(), k, s.data_ptr(), i.data_ptr(), out_s.data_ptr(), out_i.data_ptr())
    gs, gi = out_s.cpu().numpy(), out_i.cpu().numpy()
    assert np.array_equal(gs[:k], np.where(positions >= 0, scores[positions], -1.0).astype(np.float32))
    assert np.array_equal(gi[:k], np.where(positions >= 0, ids[positions], -1).astype(np.int32))
    assert (gs[k:] == SENTINEL).all() and (gi[k:] == -7).all()
    capi.gather_hits(ctx, 0, 0, 0, 0, 0, 0)       # k = 0: a no-op
    for change in (dict(k=-1), dict(positions=0), dict(scores=0), dict(ids=0), dict(out_scores=0), dict(out_ids=0)):
        args = dict(positions=p.data_ptr(), k=k, scores=s.data_ptr(), ids=i.data_ptr(), out_scores=out_s.data_ptr(), out_ids=out_i.data_ptr())
        with pytest.raises(capi.SwError):
            capi.gather_hits(ctx, **dict(args, **change))


@pytest.fixture(scope="module")
def small_db():
    return C.small_db()


@pytest.mark.parametrize("case", C.CASES)
def test_keys_topk_gather(gpu, small_db, case):
    """the device chain of a ranked query, on the oracle's scores: the reference list as a set, its order up to swaps of
    subjects within tol"""
    torch, capi, ctx = gpu
    dev = "cuda:0"
    qi, k = case
    w = small_db["want"][qi]
    n = len(w["scores"])
    fit = w["fit"]
    s = torch.from_numpy(w["scores"].astype(np.float32)).to(dev)
    l = torch.from_numpy(small_db["lengths"].astype(np.int32)).to(dev)
    ids = torch.from_numpy((np.arange(n, dtype=np.int32) + 100000)).to(dev)      # (ids are not positions)
    keys = torch.zeros(n, dtype=torch.float32, device=dev)
    pos = torch.zeros(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    capi.zscore_keys(ctx, s.data_ptr(), l.data_ptr(), n, fit["a"], fit["b1"], fit["sd"], w["z_min"], keys.data_ptr(), pos.data_ptr(),
                     count.data_ptr())
    assert int(count.cpu()[0]) == w["count"]
    tb = capi.topk_temp_bytes(n, k)
    temp = torch.zeros(max(tb, 8), dtype=torch.uint8, device=dev)
    top_key = torch.zeros(k, dtype=torch.float32, device=dev)
    top_pos = torch.zeros(k, dtype=torch.int32, device=dev)
    ctx.topk(keys.data_ptr(), pos.data_ptr(), n, k, top_key.data_ptr(), top_pos.data_ptr(), temp.data_ptr(), tb)
    out_s = torch.zeros(k, dtype=torch.float32, device=dev)
    out_i = torch.zeros(k, dtype=torch.int32, device=dev)
    capi.gather_hits(ctx, top_pos.data_ptr(), k, s.data_ptr(), ids.data_ptr(), out_s.data_ptr(), out_i.data_ptr())
    got_pos = top_pos.cpu().numpy()
    assert sorted(got_pos.tolist()) == sorted(w["ranked_ids"].tolist())
    assert K.same_up_to_close_swaps(got_pos, w["ranked_ids"], w["z"])
    assert np.array_equal(out_s.cpu().numpy(), w["scores"][got_pos].astype(np.float32))
    assert np.array_equal(out_i.cpu().numpy(), got_pos + 100000)
    assert np.array_equal(top_key.cpu().numpy(), keys.cpu().numpy()[got_pos])


# ---- the driver -------------------------------------------------------------------------------------------------------------

def _driver(small_db, k, **kw):
    from cudasw4_amd import driver
    kw.setdefault("devices", [0])
    d = driver.Driver(num_top=k, **kw)
    d.db_from_arrays(*small_db["db"])
    return d


def _check_ranked(small_db, qi, r):
    w = small_db["want"][qi]
    lengths = small_db["lengths"]
    st = r["stats"]
    assert np.array_equal(st["hist"], w["hist"]) and np.array_equal(st["sumlen"], w["sumlen"]) and st["N"] == len(lengths)
    for key in ("n_included", "rounds", "status"):
        assert st[key] == w["fit"][key]
    # the reference's ranked list: exact as a set (test_rank_cpu.py checks the boundary gaps), the order up to close swaps
    assert sorted(r["ids"].tolist()) == sorted(w["ranked_ids"].tolist())
    assert K.same_up_to_close_swaps(r["ids"], w["ranked_ids"], w["z"])
    assert r["scores"].tolist() == w["scores"][r["ids"]].tolist()          # raw scores of those ids
    rz, re_ = R.evalues(w["fit"], r["scores"], lengths[r["ids"]])
    assert np.allclose(r["evalues"], re_, rtol=1e-9, atol=0.0)
    assert z_close(r["zscores"], rz, w["fit"], r["scores"], lengths[r["ids"]])
    assert r["zscores"].dtype == np.float64 and len(r["evalues"]) == len(r["scores"]) == w["k"]
    assert (np.diff(r["zscores"]) <= 0).all() and (np.diff(r["evalues"]) >= 0).all()
    assert r["n_significant"] == w["count"]


@pytest.mark.parametrize("config", ["one", "three", "streamed"])
def test_driver_ranking(small_db, config):
    from cudasw4_amd import pssm
    kw = {"one": {}, "three": dict(devices=[0, 0, 0]), "streamed": dict(max_gpu_mem=1, max_batch_bytes=200_000)}[config]
    d = _driver(small_db, 10, **kw)
    if config == "streamed":
        assert not d.shard_info(0)["resident"]
    for qi, k in C.CASES:
        letters = small_db["letters"][qi]
        w = small_db["want"][qi]
        d.set_num_top(k)
        before = d.scan(letters)
        es, ei = O.topk(w["scores"], k)
        assert before["scores"].tolist() == es.tolist() and before["ids"].tolist() == ei.tolist()
        assert sorted(before) == ["gcups", "ids", "num_overflows", "num_rescored", "scores", "seconds"]
        assert d.last_ranking()[0] == -1
        d.set_ranking("evalue", max_evalue=C.MAX_EVALUE)
        r = d.scan(letters)
        _check_ranked(small_db, qi, r)
        count, z_min = d.last_ranking()
        assert count == w["count"] and abs(z_min - w["z_min"]) <= 1e-12 * abs(w["z_min"])
        # a list the raw-score path cannot produce
        assert set(r["ids"].tolist()) != set(before["ids"].tolist())
        assert len(set(r["ids"].tolist()) - set(before["ids"].tolist())) >= (1 if k == 10 else 5)
        if qi == 4:     # a PSSM query takes the same path (the PSSM of the letters scores like the letters)
            _check_ranked(small_db, qi, d.scan_pssm(pssm.from_sequence(small_db["codes"][qi], O.blosum21(62))))
            d.submit(letters)
            _check_ranked(small_db, qi, d.collect())
        # no threshold: the same list, no count
        d.set_ranking("evalue")
        r0 = d.scan(letters)
        assert r0["ids"].tolist() == r["ids"].tolist() and "n_significant" not in r0 and d.last_ranking()[0] == -1
        # back to raw scores: what the driver returned before
        d.set_ranking("score")
        again = d.scan(letters)
        assert again["ids"].tolist() == before["ids"].tolist() and again["scores"].tolist() == before["scores"].tolist()
        assert "stats" in again and "n_significant" not in again      # (the statistics stay as they are)
        d.set_statistics(False)
        assert sorted(d.scan(letters)) == sorted(before)
    d.close()


def test_refusals_under_evalue_ranking(small_db):
    from cudasw4_amd import driver
    qi, k = C.CASES[0]
    letters = small_db["letters"][qi]
    d = _driver(small_db, k)
    d.set_ranking("evalue", max_evalue=C.MAX_EVALUE)
    d.submit(letters)
    with pytest.raises(driver.DriverError) as e:
        d.submit(letters)                       # one query in flight
    assert "one query in flight" in str(e.value)
    with pytest.raises(driver.DriverError):
        d.set_ranking("score")                  # not with a query in flight
    with pytest.raises(driver.DriverError):
        d.set_ranking("evalue")
    _check_ranked(small_db, qi, d.collect())    # the refused calls left the pending query alone
    with pytest.raises(ValueError):
        d.set_statistics(False)
    with pytest.raises(ValueError):
        d.set_ranking("zscore")
    d.set_ranking("score")
    d.submit(letters)
    d.submit(letters)                           # by raw score two may be in flight, as before
    a, b = d.collect(), d.collect()
    assert a["ids"].tolist() == b["ids"].tolist() == O.topk(small_db["want"][qi]["scores"], k)[1].tolist()
    d.close()


def test_pseudo_db_falls_back_to_the_score_list():
    from cudasw4_amd import driver, stats
    _, letters = O.read_fasta(O.GOLDEN_DIR + "/allqueries.fasta")
    d = driver.Driver(devices=[0], num_top=10)
    d.pseudo_db(2000, 512)
    before = d.scan(letters[2])
    d.set_ranking("evalue", max_evalue=C.MAX_EVALUE)
    r = d.scan(letters[2])
    assert r["stats"]["status"] == stats.NO_FIT
    assert r["ids"].tolist() == before["ids"].tolist() and r["scores"].tolist() == before["scores"].tolist()
    assert r["n_significant"] == -1 and d.last_ranking()[0] == -1
    assert r["evalues"].tolist() == [-1.0] * 10 and r["zscores"].tolist() == [0.0] * 10
    d.close()


def test_alignment_and_pssm_on_a_ranked_list(small_db):
    """align_hits and build_pssm(max_evalue=) take a ranked result as it is, and agree with the CPU chain on the same ids"""
    from test_gpu_pssm_build import reference_build
    import pssm_build_ref as PB
    qi, k = C.CASES[1]
    letters = small_db["letters"][qi]
    q = small_db["codes"][qi]
    chars, offsets, lengths = small_db["db"]
    seqs = {int(i): chars[int(offsets[i]):int(offsets[i]) + int(lengths[i])] for i in small_db["want"][qi]["ranked_ids"]}
    d = _driver(small_db, k)
    d.set_ranking("evalue", max_evalue=C.MAX_EVALUE)
    r = d.scan(letters)
    _check_ranked(small_db, qi, r)
    res, cigars = d.align_hits(letters, r)
    for j, i in enumerate(r["ids"]):
        want, words = A.align(q, seqs[int(i)], O.blosum21(62))
        for f in A.FIELDS:
            assert int(res[j][f]) == want[f], (j, int(i), f)
        assert cigars[j] == (A.cigar_string(words) or "*")
        assert int(res[j]["score"]) == int(r["scores"][j])
    x = 1e-3
    keep = (r["evalues"] >= 0) & (r["evalues"] <= x)
    assert 0 < int(keep.sum()) < k
    want, winfo = reference_build(q, seqs, r["ids"][keep], r["scores"][keep], res[keep],
                                  [PB.words(c) if c != "*" else [] for c, kp in zip(cigars, keep) if kp], 0)
    got, info = d.build_pssm(letters, r, max_evalue=x)
    assert got.tolist() == want.tolist() and info["included"] == winfo["included"]
    assert info["used"] == winfo["used"] > 0 and info["below_score"] == k - int(keep.sum())
    d.close()


# ---- the command line -----------------------------------------------------------------------------------------------------

LETTERS = "ARNDCQEGHILKMFPSTWYV"


def test_align_rank_by(small_db, tmp_path):
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
    qi, k = C.CASES[1]
    w = small_db["want"][qi]
    letters = small_db["letters"][qi]
    letters = letters.decode() if isinstance(letters, bytes) else letters
    qfile = str(tmp_path / "q.fa")
    with open(qfile, "w") as f:
        f.write(">query\n%s\n" % letters)

    def run(args, of):
        r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", qfile, "--db", prefix, "--top", str(k), "--of", of]
                           + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(of).read(), r

    d = driver.Driver(devices=[0], num_top=k)
    d.open_db(prefix)
    d.set_ranking("evalue", max_evalue=C.MAX_EVALUE)
    ranked = d.scan(letters)
    origin = [int(d.reference_header(int(i))[1:]) for i in ranked["ids"]]
    d.close()
    # the list does not depend on the order makedb gave the subjects (ties aside: none at these places)
    assert sorted(origin) == sorted(w["ranked_ids"].tolist()) and ranked["n_significant"] == w["count"]

    tsv, r = run(["--tsv", "--rankBy", "evalue", "--verbose"], str(tmp_path / "e.tsv"))
    lines = tsv.splitlines()
    assert lines[0].split("\t")[-2:] == ["Z-score", "E-value"] and len(lines) == 1 + k
    rows = [l.split("\t") for l in lines[1:]]
    assert [int(x[7]) for x in rows] == ranked["ids"].tolist() and [int(x[4]) for x in rows] == ranked["scores"].tolist()
    assert [x[-2] for x in rows] == ["%.2f" % z for z in ranked["zscores"]]
    assert "significant:" not in r.stdout and "rankBy: evalue" in r.stdout
    # --maxEvalue: the results of the ranked list with E <= X, and the count over the whole DB
    tsv_m, r_m = run(["--tsv", "--rankBy", "evalue", "--maxEvalue", "10", "--verbose"], str(tmp_path / "m.tsv"))
    passing = [int(i) for i, e in zip(ranked["ids"], ranked["evalues"]) if e <= 10]
    assert [int(l.split("\t")[7]) for l in tsv_m.splitlines()[1:]] == passing
    assert "significant: %d subjects at E <= 10 (%d reported)" % (w["count"], len(passing)) in r_m.stdout.splitlines()
    assert len(passing) == min(w["count"], k)       # the ranked list holds the significant subjects first
    # without the flag: byte for byte what --rankBy score prints, and what the raw-score list is
    tsv_p, r_p = run(["--tsv"], str(tmp_path / "p.tsv"))
    tsv_s, r_s = run(["--tsv", "--rankBy", "score"], str(tmp_path / "s.tsv"))
    assert tsv_p.encode() == tsv_s.encode() and "rankBy" not in r_p.stdout and "statistics" not in r_p.stdout
    assert [int(l.split("\t")[4]) for l in tsv_p.splitlines()[1:]] == O.topk(w["scores"], k)[0].tolist()
    assert [l.split("\t")[7] for l in tsv_p.splitlines()[1:]] != [x[7] for x in rows]
