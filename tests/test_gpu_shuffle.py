"""Statistics calibrated on shuffled subjects on the GPU: the shuffle kernel bit for bit against the numpy
restatement (shuffle_ref.py), the host library's calibration on the family-dominated and the small database
(shuffle_cases.py) against the reference's table and fit, the pseudo DB, and `align --statistics shuffled`."""
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import shuffle_cases as C
import shuffle_ref as SR
import stats_ref as R
from test_stats_cpu import z_close

pytestmark = pytest.mark.gpu

BLOCK_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 70001]
FILL = 77   # what the output buffer holds before a call: no code of the alphabet


# ---- the kernel: capi.shuffle_subjects on arrays ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def block():
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, 21, l, dtype=np.int8) for l in BLOCK_LENGTHS]
    chars, offsets, lengths = O.make_db(seqs)
    keys = (np.arange(len(seqs), dtype=np.int64) * 2654435761 + (1 << 32) + 3)
    assert int(keys.max()) > 1 << 32
    return {"chars": np.asarray(chars, dtype=np.int8), "offsets": np.asarray(offsets, dtype=np.uint64),
            "lengths": np.asarray(lengths, dtype=np.int32), "keys": keys}


@pytest.fixture(scope="module")
def shuffler():
    import torch
    from cudasw4_amd import capi
    ctx = capi.Context(0)

    def run(chars, offsets, lengths, seed, keys=None, first_replica=0, replicas=1, stride=None, first=0, n=None):
        """-> (int8 [replicas][stride] as the device holds it after the call, the input chars as the device holds them)"""
        dev = "cuda:0"
        n = len(lengths) - first if n is None else n
        nbytes = int(offsets[first + n]) - int(offsets[first])
        stride = nbytes if stride is None else stride
        c = torch.from_numpy(chars.view(np.uint8).copy()).to(dev)
        o = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        l = torch.from_numpy(lengths.copy()).to(dev)
        k = torch.from_numpy(np.asarray(keys, dtype=np.int64).copy()).to(dev) if keys is not None else None
        out = torch.full((max(replicas * stride, 4),), FILL, dtype=torch.uint8, device=dev)
        capi.shuffle_subjects(ctx, c.data_ptr() + int(offsets[first]), o.data_ptr() + 8 * first, l.data_ptr() + 4 * first, n, seed,
                              out.data_ptr(), stride, keys=k.data_ptr() if k is not None else 0, first_replica=first_replica,
                              replicas=replicas)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.int8)[:replicas * stride].reshape(replicas, stride) if stride else np.zeros((replicas, 0), np.int8)
        return got, c.cpu().numpy().view(np.int8)

    yield run, ctx
    ctx.close()


def test_kernel_matches_reference(block, shuffler):
    run, _ = shuffler
    b = block
    for keys in (None, b["keys"]):
        got, chars_after = run(b["chars"], b["offsets"], b["lengths"], 2024, keys=keys, first_replica=2, replicas=2)
        ref = SR.shuffle_block(b["chars"], b["offsets"], b["lengths"], 2024, keys=keys, first_replica=2, replicas=2)
        assert got.shape == ref.shape and np.array_equal(got, ref), np.nonzero(got != ref)
        assert np.array_equal(chars_after, b["chars"])   # the input is unchanged
    # every byte was written, and the subjects were shuffled at all
    assert not (got == FILL).any() and (got[0] != b["chars"]).mean() > 0.5


def test_kernel_from_the_middle_of_a_block(block, shuffler):
    run, _ = shuffler
    b = block
    assert int(b["offsets"][7]) != 0
    for keys in (None, b["keys"][7:19]):
        got, _ = run(b["chars"], b["offsets"], b["lengths"], 9, keys=keys, replicas=2, first=7, n=12)
        ref = SR.shuffle_block(b["chars"], b["offsets"], b["lengths"], 9, keys=keys, replicas=2, first=7, n=12)
        assert got.shape == ref.shape and np.array_equal(got, ref)


def test_kernel_replica_ranges_and_stride(block, shuffler):
    run, _ = shuffler
    b = block
    nbytes = int(b["offsets"][-1])
    whole, _ = run(b["chars"], b["offsets"], b["lengths"], 31, keys=b["keys"], first_replica=0, replicas=3)
    one, _ = run(b["chars"], b["offsets"], b["lengths"], 31, keys=b["keys"], first_replica=0, replicas=1)
    two, _ = run(b["chars"], b["offsets"], b["lengths"], 31, keys=b["keys"], first_replica=1, replicas=2)
    assert np.array_equal(whole, np.concatenate([one, two]))
    assert not np.array_equal(whole[0], whole[1]) and not np.array_equal(whole[1], whole[2])
    # a stride larger than the block: the gap keeps what it held
    wide, _ = run(b["chars"], b["offsets"], b["lengths"], 31, keys=b["keys"], replicas=3, stride=nbytes + 260)
    assert np.array_equal(wide[:, :nbytes], whole) and (wide[:, nbytes:] == FILL).all()


def test_kernel_refuses_invalid_arguments(block, shuffler):
    import torch
    from cudasw4_amd import capi
    _, ctx = shuffler
    b = block
    n, nbytes = len(b["lengths"]), int(b["offsets"][-1])
    c = torch.from_numpy(b["chars"].view(np.uint8).copy()).to("cuda:0")
    o = torch.from_numpy(b["offsets"].view(np.int64).copy()).to("cuda:0")
    l = torch.from_numpy(b["lengths"].copy()).to("cuda:0")
    out = torch.full((nbytes + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    good = dict(ctx=ctx, chars=c.data_ptr(), offsets=o.data_ptr(), lengths=l.data_ptr(), n=n, seed=1, out=out.data_ptr(),
                replica_stride=nbytes)
    bad = [dict(ctx=None), dict(chars=0), dict(offsets=0), dict(lengths=0), dict(out=0), dict(n=-1), dict(replicas=-1),
           dict(first_replica=-1), dict(replica_stride=nbytes - 4), dict(replica_stride=nbytes + 2), dict(out=out.data_ptr() + 1)]
    for change in bad:
        with pytest.raises(capi.SwError) as e:
            capi.shuffle_subjects(**{**good, **change})
        assert e.value.code == -1, change
    # n = 0 and replicas = 0: nothing is read or written
    capi.shuffle_subjects(**{**good, "n": 0})
    capi.shuffle_subjects(**{**good, "replicas": 0})
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


def test_kernel_many_short_subjects_in_one_call(shuffler):
    run, _ = shuffler
    rng = np.random.default_rng(8)
    chars, offsets, lengths = O.make_db([rng.integers(0, 20, 30, dtype=np.int8) for _ in range(3000)])
    chars, offsets, lengths = np.asarray(chars, np.int8), np.asarray(offsets, np.uint64), np.asarray(lengths, np.int32)
    got, _ = run(chars, offsets, lengths, 4, replicas=2)
    assert np.array_equal(got, SR.shuffle_block(chars, offsets, lengths, 4, replicas=2))


# ---- the host library: Driver.calibrate -----------------------------------------------------------------------------------

def _driver(c, **kw):
    from cudasw4_amd import driver
    kw.setdefault("devices", [0])
    kw.setdefault("num_top", 20)
    d = driver.Driver(**kw)
    d.db_from_arrays(c["chars"], c["offsets"], c["lengths"])
    return d


def _same_fit(got, ref):
    for k in ("n_included", "rounds", "status", "N"):
        assert got[k] == ref[k], (k, got, ref)
    for k in ("a", "b1", "sd"):
        assert abs(got[k] - ref[k]) <= 1e-9 * abs(ref[k]), (k, got, ref)


@pytest.mark.parametrize("name", ["family", "small"])
def test_calibrate_matches_reference(name):
    from cudasw4_amd import pssm, stats
    c = C.case(name)
    d = _driver(c)
    cal = d.calibrate(c["letters"], shuffles=c["shuffles"], seed=C.SHUFFLE_SEED)
    assert (cal["subjects"], cal["replicas"]) == (len(c["lengths"]), c["shuffles"])
    assert np.array_equal(cal["hist"], c["cal_hist"]) and np.array_equal(cal["sumlen"], c["cal_sumlen"])
    _same_fit(cal, c["cal_fit"])
    # the outcomes of test_shuffle_cpu.py, with the library's numbers
    st = dict(cal, N=len(c["lengths"]))
    z, e = stats.evalues(st, c["scores"], c["lengths"])
    assert z_close(z, c["z"], c["stats"], c["scores"], c["lengths"]) and np.allclose(e, c["e"], rtol=1e-6, atol=0.0)
    rel = c["relative"]
    assert 4 <= cal["sd"] <= 5.5 and (e[rel] <= 1e-3).all() and not (e[~rel] <= 1).any()
    # twice the same; the PSSM that restates the query gives the letter form's table; another seed another table
    again = d.calibrate(c["letters"], shuffles=c["shuffles"], seed=C.SHUFFLE_SEED)
    assert np.array_equal(again["hist"], cal["hist"]) and np.array_equal(again["sumlen"], cal["sumlen"])
    prof = d.calibrate(pssm.from_sequence(c["letters"], O.blosum21(62)), shuffles=c["shuffles"], seed=C.SHUFFLE_SEED)
    assert np.array_equal(prof["hist"], cal["hist"]) and np.array_equal(prof["sumlen"], cal["sumlen"])
    other = d.calibrate(c["letters"], shuffles=c["shuffles"], seed=C.SHUFFLE_SEED + 1)
    assert not np.array_equal(other["hist"], cal["hist"]) and int(other["hist"].sum()) == int(cal["hist"].sum())
    d.close()
    if name == "family":
        # replicas forced into chunks: two of the four fit the scratch limit
        nbytes = int(c["offsets"][-1])
        limit = (2 * nbytes + 4096) // 256 * 256
        assert 2 * ((nbytes + 255) // 256 * 256) <= limit < 3 * nbytes
        d = _driver(c, max_temp_bytes=limit)
        chunked = d.calibrate(c["letters"], shuffles=4, seed=C.SHUFFLE_SEED)
        assert np.array_equal(chunked["hist"], cal["hist"]) and np.array_equal(chunked["sumlen"], cal["sumlen"])
        d.close()


def test_driver_results_under_shuffled_statistics():
    c = C.case("family")
    rel = c["relative"]
    d = _driver(c)
    d.set_statistics(True, mode="shuffled", shuffles=4, seed=C.SHUFFLE_SEED)
    r = d.scan(c["letters"])
    top = O.topk(c["scores"], 20)
    assert r["scores"].tolist() == top[0].tolist() and r["ids"].tolist() == top[1].tolist()
    assert r["stats"]["mode"] == "shuffled" and r["stats"]["N"] == 600 and np.array_equal(r["stats"]["hist"], c["cal_hist"])
    assert z_close(r["zscores"], c["z"][r["ids"]], c["stats"], r["scores"], c["lengths"][r["ids"]])
    assert np.allclose(r["evalues"], c["e"][r["ids"]], rtol=1e-6, atol=0.0)
    # ranked by the calibrated E-value: the reference's order over the whole DB
    d.set_ranking("evalue", max_evalue=1e-3)
    ranked = d.scan(c["letters"])
    order = np.lexsort((np.arange(len(c["z"])), -c["z"]))[:20]
    assert ranked["ids"].tolist() == order.tolist() and ranked["scores"].tolist() == c["scores"][order].tolist()
    assert ranked["n_significant"] == int((c["e"] <= 1e-3).sum()) == int(rel.sum())
    # back to the scan's own fit: the family's, nothing significant
    d.set_ranking("score")
    d.set_statistics(True)
    plain = d.scan(c["letters"])
    assert plain["stats"]["mode"] == "scan" and abs(plain["stats"]["sd"] - c["scan_fit"]["sd"]) <= 1e-9 * c["scan_fit"]["sd"]
    assert not (plain["evalues"] <= 1).any()
    d.close()


def test_pseudo_db_is_calibrated():
    from cudasw4_amd import driver, stats
    d = driver.Driver(devices=[0], num_top=10)
    d.pseudo_db(2000, 300)
    _, letters = O.read_fasta(O.GOLDEN_DIR + "/allqueries.fasta")
    d.set_statistics(True)
    assert d.scan(letters[2])["stats"]["status"] == stats.NO_FIT
    d.set_statistics(True, mode="shuffled")
    r = d.scan(letters[2])
    st = r["stats"]
    assert st["status"] == stats.OK and st["b1"] == 0.0 and st["sd"] > 0 and st["N"] == 2000
    assert (st["subjects"], st["replicas"]) == (2000, 1) and int((st["hist"].sum(axis=1) > 0).sum()) == 1
    assert (r["evalues"] > 0).all() and len(set(r["scores"].tolist())) == 1
    d.close()


# ---- the command line -----------------------------------------------------------------------------------------------------

LETTERS = "ARNDCQEGHILKMFPSTWYV"


def test_align_statistics_shuffled(tmp_path):
    from cudasw4_amd import driver
    c = C.case("family")
    chars, offsets, lengths = c["chars"], c["offsets"], c["lengths"]
    fasta = str(tmp_path / "db.fa")
    lut = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    with open(fasta, "w") as f:
        for i in range(len(lengths)):   # the header carries the subject's position in shuffle_cases' DB
            o = int(offsets[i])
            f.write(">s%d\n%s\n" % (i, lut[chars[o:o + int(lengths[i])]].tobytes().decode()))
    prefix = str(tmp_path / "fam")
    p = subprocess.run([driver.MAKEDB, fasta, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    letters = c["letters"].decode() if isinstance(c["letters"], bytes) else c["letters"]
    qfile = str(tmp_path / "q.fa")
    with open(qfile, "w") as f:
        f.write(">query\n%s\n" % letters)
    top = 300

    def run(args, of):
        r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", qfile, "--db", prefix, "--top", str(top), "--of", of]
                           + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(of, "rb").read(), r

    # the reference on the DB in the order makedb gave it (the subject key is the id within the opened DB)
    d = driver.Driver(devices=[0], num_top=top)
    d.open_db(prefix)
    origin = np.array([int(d.reference_header(i)[1:]) for i in range(len(lengths))])
    d.close()
    seqs = [chars[int(offsets[i]):int(offsets[i]) + int(lengths[i])] for i in origin]
    mc, mo, ml = O.make_db(seqs)
    scores = c["scores"][origin]
    q = c["query"]
    _, _, cfit, m, reps = SR.calibrate(lambda a, b, l: O.scan(q, a, b, l, simd=True), mc, mo, ml, C.SHUFFLE_SEED, shuffles=4)
    st = SR.calibrated(cfit, len(ml))
    z, e = R.evalues(st, scores, ml)
    rel = c["relative"][origin]

    shuffled = ["--statistics", "shuffled", "--shuffles", "4", "--shuffleSeed", str(C.SHUFFLE_SEED)]
    tsv, r = run(["--tsv", "--verbose"] + shuffled, str(tmp_path / "s.tsv"))
    rows = [l.split("\t") for l in tsv.decode().splitlines()[1:]]
    ids = [int(x[7]) for x in rows]
    want = O.topk(scores, top)
    assert [int(x[4]) for x in rows] == want[0].tolist() and ids == want[1].tolist()
    assert [x[-2] for x in rows] == ["%.2f" % v for v in z[ids]] and [x[-1] for x in rows] == ["%.3g" % v for v in e[ids]]
    assert "statistics: shuffled 600 subjects x 4, N 600 fitted on %d a " % cfit["n_included"] in r.stdout
    assert " rounds %d" % cfit["rounds"] in r.stdout
    # --maxEvalue: exactly the relatives of the top list
    tsv_m, _ = run(["--tsv", "--maxEvalue", "1e-3"] + shuffled, str(tmp_path / "m.tsv"))
    ids_m = [int(l.split("\t")[7]) for l in tsv_m.decode().splitlines()[1:]]
    assert ids_m == [i for i in ids if rel[i]] and len(ids_m) == 240
    # --rankBy evalue: the reference's order
    tsv_r, _ = run(["--tsv", "--rankBy", "evalue"] + shuffled, str(tmp_path / "r.tsv"))
    ids_r = [int(l.split("\t")[7]) for l in tsv_r.decode().splitlines()[1:]]
    assert ids_r == np.lexsort((np.arange(len(z)), -z))[:top].tolist()
    # --iterations with --inclusionEvalue: under the scan's own fit no relative is admitted, under the calibrated one they are,
    # and the second round's PSSM is calibrated as well
    admitted = {}
    for name, flags in (("scan", []), ("shuffled", shuffled)):
        _, r_it = run(["--tsv", "--iterations", "2", "--inclusionEvalue", "1e-3", "--verbose"] + flags, str(tmp_path / "it.tsv"))
        rounds = [l for l in r_it.stdout.splitlines() if l.startswith("Query 0 round ")]
        admitted[name] = [int(re.search(r"(\d+) results, (\d+) in the PSSM", l).group(2)) for l in rounds]
    assert admitted["scan"] == [0] or admitted["scan"] == [0, 0], admitted
    assert len(admitted["shuffled"]) == 2 and min(admitted["shuffled"]) > 100, admitted
    # without the flag, and with --statistics scan: the same bytes, in both output forms
    for args in (["--tsv", "--evalues"], []):
        a, ra = run(args, str(tmp_path / "a.out"))
        b, rb = run(args + ["--statistics", "scan"], str(tmp_path / "b.out"))
        assert a == b and len(a) > 0
        assert [l for l in ra.stdout.splitlines() if l.startswith("statistics")] == []
        assert [l for l in rb.stdout.splitlines() if l.startswith("statistics")] == ["statistics: scan"]
