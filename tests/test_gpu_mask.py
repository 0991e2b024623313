"""GPU: low-complexity masking of the subjects — the kernels (capi.mask_subjects) against the numpy statement
of the rule byte for byte, the driver's residency modes against the CPU oracle over the masked database, hit alignment and the
shuffled calibration on masked subjects, and the command line.  Every comparison is exact."""
import re
import subprocess

import numpy as np
import pytest

import align_ref as AR
import mask_cases as MC
import mask_ref as MR
import oracle_lib as O
import shuffle_ref as SR

pytestmark = pytest.mark.gpu

FILL = 77   # what an output buffer holds before a call: no code of the alphabet
TAIL = 64   # bytes behind the block that must keep it


# ---- the kernels: capi.mask_subjects on arrays ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def masker():
    import torch
    from cudasw4_amd import capi
    ctx = capi.Context(0)
    dev = "cuda:0"

    def run(block, params, in_place=False, first=0, n=None, temp_bytes=None, counts=None, chars_dev=None):
        """-> (the range's bytes after the call, the bytes behind them, the input as the device holds it after the call,
        counts as a list); chars_dev: a device copy of the whole block to work on (in place)"""
        chars, offsets, lengths = block["chars"], block["offsets"], block["lengths"]
        n = len(lengths) - first if n is None else n
        base, nbytes = int(offsets[first]), int(offsets[first + n]) - int(offsets[first])
        c = chars_dev if chars_dev is not None else torch.from_numpy(chars.view(np.uint8).copy()).to(dev)
        o = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        l = torch.from_numpy(lengths.copy()).to(dev)
        out = None if in_place else torch.full((nbytes + TAIL,), FILL, dtype=torch.uint8, device=dev)
        need = capi.mask_subjects_temp_bytes(ctx, o.data_ptr() + 8 * first, n, *params)
        assert need == (nbytes + 63) // 64 * 24
        tb = need if temp_bytes is None else temp_bytes
        temp = torch.zeros(max(tb, 8) // 8 + 1, dtype=torch.int64, device=dev)
        cnt = torch.tensor(counts if counts is not None else [0, 0], dtype=torch.int64, device=dev)
        capi.mask_subjects(ctx, c.data_ptr() + base, o.data_ptr() + 8 * first, l.data_ptr() + 4 * first, n, *params,
                           out=c.data_ptr() + base if in_place else out.data_ptr(), temp=temp.data_ptr(), temp_bytes=tb,
                           counts=cnt.data_ptr())
        torch.cuda.synchronize()
        after = c.cpu().numpy().view(np.int8)
        if in_place:
            return after[base:base + nbytes], None, after, cnt.cpu().tolist()
        got = out.cpu().numpy().view(np.int8)
        return got[:nbytes], got[nbytes:], after, cnt.cpu().tolist()

    yield run, ctx
    ctx.close()


@pytest.fixture(scope="module")
def structured():
    """the structured block and, per parameter set, the reference's (bytes, positions, subjects): computed once"""
    b = MC.structured_block()
    return b, {p: MR.mask_block(b["chars"], b["offsets"], b["lengths"], *p) for p in MC.PARAM_SETS}


@pytest.mark.parametrize("params", MC.PARAM_SETS, ids=lambda p: "w%d" % p[0])
def test_kernel_matches_reference(structured, masker, params):
    run, _ = masker
    b, refs = structured
    ref, positions, subjects = refs[params]
    assert positions > 1000 and subjects >= 10 and (b["chars"] == 20).sum() > 100
    got, tail, after, counts = run(b, params)
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]
    assert (tail == FILL).all() and np.array_equal(after, b["chars"])   # nothing behind the block, the input unchanged
    assert counts == [positions, subjects]
    got, _, after, counts = run(b, params, in_place=True)
    assert np.array_equal(got, ref) and np.array_equal(after, ref) and counts == [positions, subjects]


def test_kernel_from_the_middle_of_a_block(structured, masker):
    run, _ = masker
    b, _ = structured
    assert int(b["offsets"][7]) != 0
    for params in MC.PARAM_SETS:
        ref, positions, subjects = MR.mask_block(b["chars"], b["offsets"], b["lengths"], *params, first=7, n=12)
        got, tail, _, counts = run(b, params, first=7, n=12)
        assert np.array_equal(got, ref) and (tail == FILL).all() and counts == [positions, subjects]
        # in place: the subjects around the range keep their bytes
        got, _, after, _ = run(b, params, in_place=True, first=7, n=12)
        lo, hi = int(b["offsets"][7]), int(b["offsets"][19])
        assert np.array_equal(got, ref) and np.array_equal(after[:lo], b["chars"][:lo]) and np.array_equal(after[hi:], b["chars"][hi:])


def test_unbounded_runs(masker):
    run, _ = masker
    b = MC.run_block()
    ref, positions, subjects = MR.mask_block(b["chars"], b["offsets"], b["lengths"], *MC.RUN_PARAMS)
    assert subjects == 3
    for in_place in (False, True):
        got, _, _, counts = run(b, MC.RUN_PARAMS, in_place=in_place)
        assert np.array_equal(got, ref) and counts == [positions, subjects]
    for i, bounds in enumerate(b["bounds"]):
        o, L = int(b["offsets"][i]), int(b["lengths"][i])
        m = np.nonzero(got[o:o + L] == 20)[0]
        if bounds is None:
            assert len(m) == 0 and np.array_equal(got[o:o + L], b["chars"][o:o + L])
            continue
        (a0, a1), (e0, e1) = bounds
        assert a0 <= m[0] <= a1 and e0 <= m[-1] + 1 <= e1 and len(m) == m[-1] + 1 - m[0]   # one stretch, from / to the planted window
        assert len(m) > 4 * MC.LONGEST_TILE                                                 # ... which crosses tiles


def test_small_scratch_works_in_ranges(structured, masker):
    from cudasw4_amd import capi
    run, _ = masker
    b, refs = structured
    params = MC.PARAM_SETS[0]
    ref, positions, subjects = refs[params]
    longest = int(np.diff(b["offsets"].astype(np.int64)).max())
    need = (longest + 63) // 64 * 24            # of the longest subject alone
    assert need < (int(b["offsets"][-1]) + 63) // 64 * 24
    for in_place in (False, True):
        got, tail, _, counts = run(b, params, in_place=in_place, temp_bytes=need)
        assert np.array_equal(got, ref) and counts == [positions, subjects]
    # many short subjects through a scratch of one bitmap word per flag: ranges of at most 64 bytes
    rng = np.random.default_rng(8)
    short = MC._block([MC.structured_subject(rng, int(l)) for l in rng.integers(0, 61, 300)])
    sref, spos, ssub = MR.mask_block(short["chars"], short["offsets"], short["lengths"], *MC.PARAM_SETS[1])
    got, _, _, counts = run(short, MC.PARAM_SETS[1], temp_bytes=24)
    assert np.array_equal(got, sref) and counts == [spos, ssub] and ssub > 20
    with pytest.raises(capi.SwError) as e:
        run(b, params, temp_bytes=need - 1)
    assert e.value.code == -1 and str(need) in str(e.value)


def test_idempotent_and_counts_accumulate(structured, masker):
    import torch
    run, _ = masker
    b, refs = structured
    params = MC.PARAM_SETS[0]
    ref, positions, subjects = refs[params]
    c = torch.from_numpy(b["chars"].view(np.uint8).copy()).to("cuda:0")
    _, _, after, counts = run(b, params, in_place=True, chars_dev=c, counts=[5, 7])
    assert np.array_equal(after, ref) and counts == [5 + positions, 7 + subjects]
    _, _, again, counts = run(b, params, in_place=True, chars_dev=c, counts=counts)
    assert np.array_equal(again, ref) and counts == [5 + positions, 7 + subjects]   # a second pass finds no segment
    # out of place, twice into the same counts
    _, _, _, counts = run(b, params, counts=[0, 0])
    _, _, _, counts = run(b, params, counts=counts)
    assert counts == [2 * positions, 2 * subjects]


def test_kernel_refuses_invalid_arguments(structured, masker):
    import torch
    from cudasw4_amd import capi
    _, ctx = masker
    b, _ = structured
    n, nbytes = len(b["lengths"]), int(b["offsets"][-1])
    c = torch.from_numpy(np.concatenate([b["chars"], b["chars"]]).view(np.uint8).copy()).to("cuda:0")
    o = torch.from_numpy(b["offsets"].view(np.int64).copy()).to("cuda:0")
    l = torch.from_numpy(b["lengths"].copy()).to("cuda:0")
    out = torch.full((nbytes + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    need = capi.mask_subjects_temp_bytes(ctx, o.data_ptr(), n)
    temp = torch.zeros(need // 8 + 2, dtype=torch.int64, device="cuda:0")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    before = c.clone()
    good = dict(ctx=ctx, chars=c.data_ptr(), offsets=o.data_ptr(), lengths=l.data_ptr(), n=n, window=12, trigger_sum=20705,
                extend_sum=17019, out=out.data_ptr(), temp=temp.data_ptr(), temp_bytes=need, counts=cnt.data_ptr())
    bad = [dict(ctx=None), dict(chars=0), dict(offsets=0), dict(lengths=0), dict(out=0), dict(n=-1), dict(window=3), dict(window=33),
           dict(trigger_sum=17018), dict(extend_sum=0), dict(trigger_sum=0, extend_sum=0), dict(out=out.data_ptr() + 1),
           dict(chars=c.data_ptr() + 2), dict(offsets=o.data_ptr() + 4), dict(lengths=l.data_ptr() + 2), dict(temp=temp.data_ptr() + 4),
           dict(counts=cnt.data_ptr() + 4),
           # partial overlaps of out and chars, from either side
           dict(out=c.data_ptr() + 64), dict(out=c.data_ptr() + nbytes - 4), dict(chars=c.data_ptr() + 128, out=c.data_ptr())]
    for change in bad:
        with pytest.raises(capi.SwError) as e:
            capi.mask_subjects(**{**good, **change})
        assert e.value.code == -1, change
    capi.mask_subjects(**{**good, "n": 0})   # nothing is read or written
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((c == before).all()) and cnt.cpu().tolist() == [0, 0, 0]
    # an out that starts where the block ends does not overlap it
    capi.mask_subjects(**{**good, "out": c.data_ptr() + nbytes})
    torch.cuda.synchronize()
    ref = MR.mask_block(b["chars"], b["offsets"], b["lengths"])[0]
    assert np.array_equal(c.cpu().numpy().view(np.int8), np.concatenate([b["chars"], ref]))


def test_phase_events_variant(structured, masker):
    """sw_mask_subjects_phases (what tools/mask_bench.py times): the same bytes and counts, four events recorded in order, and a
    refusal where the scratch would need more than one range"""
    import torch
    from cudasw4_amd import capi
    _, ctx = masker
    b, refs = structured
    params = MC.PARAM_SETS[0]
    ref, positions, subjects = refs[params]
    n, nbytes = len(b["lengths"]), int(b["offsets"][-1])
    c = torch.from_numpy(b["chars"].view(np.uint8).copy()).to("cuda:0")
    o = torch.from_numpy(b["offsets"].view(np.int64).copy()).to("cuda:0")
    l = torch.from_numpy(b["lengths"].copy()).to("cuda:0")
    out = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda:0")
    need = capi.mask_subjects_temp_bytes(ctx, o.data_ptr(), n, *params)
    temp = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda:0")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in evs:
        e.record()
    torch.cuda.synchronize()
    args = (ctx, c.data_ptr(), o.data_ptr(), l.data_ptr(), n, *params)
    capi.mask_subjects_phases(*args, out=out.data_ptr(), temp=temp.data_ptr(), temp_bytes=need, events=[int(e.cuda_event) for e in evs],
                              counts=cnt.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int8), ref) and cnt.cpu().tolist() == [positions, subjects]
    assert all(evs[i].elapsed_time(evs[i + 1]) >= 0 for i in range(3))
    with pytest.raises(capi.SwError) as e:
        capi.mask_subjects_phases(*args, out=out.data_ptr(), temp=temp.data_ptr(), temp_bytes=need - 8, events=[int(x.cuda_event) for x in evs])
    assert e.value.code == -1


# ---- the driver ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx():
    """the end-to-end fixture with the reference's masked DB and the oracle's scores over the raw and the masked chars"""
    f = dict(MC.fixture())
    f["masked"], f["positions"], f["subjects"] = MR.mask_block(f["chars"], f["offsets"], f["lengths"])
    f["raw_scores"] = O.scan(f["query"], f["chars"], f["offsets"], f["lengths"], simd=True)
    f["masked_scores"] = O.scan(f["query"], f["masked"], f["offsets"], f["lengths"], simd=True)
    f["residues"] = int(f["lengths"].astype(np.int64).sum())
    return f


def _driver(f, masking=True, **kw):
    from cudasw4_amd import driver
    kw.setdefault("devices", [0])
    kw.setdefault("num_top", 12)
    d = driver.Driver(kinds=(0, 0, 3, 3), **kw)
    if masking:
        d.set_subject_masking()
    d.db_from_arrays(f["chars"], f["offsets"], f["lengths"])
    return d


def _all_scores(d):
    ids, sc = d.all_scores()
    got = np.empty(len(sc), dtype=np.int32)
    got[ids] = sc.astype(np.int32)
    return got


CONFIGS = {"resident": {}, "streamed": dict(max_gpu_mem=1, max_batch_bytes=20000),
           "hybrid": dict(max_gpu_mem=144000, max_batch_bytes=8000), "three shards": dict(devices=[0, 0, 0]),
           "three shards streamed": dict(devices=[0, 0, 0], max_gpu_mem=1, max_batch_bytes=8000)}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_driver_scans_the_masked_database(fx, config):
    d = _driver(fx, **CONFIGS[config])
    assert d.masking_counts() == {"positions": 0, "subjects": 0, "residues_seen": 0}
    infos = [d.shard_info(g) for g in range(d.num_gpus())]
    if config == "resident" or config == "three shards":
        assert all(i["cached_chars"] == i["chars"] for i in infos)   # (the upload itself comes with the first scan)
    elif config == "hybrid":
        assert all(0 < i["cached_chars"] < i["chars"] for i in infos), infos
    else:
        assert all(i["cached_chars"] == 0 and not i["resident"] for i in infos)
    want = {"positions": fx["positions"], "subjects": fx["subjects"], "residues_seen": fx["residues"]}
    for scan in range(3):   # (a streamed scan stages the first batch of the next one ahead: masked once, by the scan that uses it)
        r = d.scan(fx["letters"])
        assert np.array_equal(_all_scores(d), fx["masked_scores"]), (config, scan)
        assert d.masking_counts() == want, (config, scan)
        if config in ("streamed", "hybrid"):
            assert len(d.batch_intervals()) >= 3
        es, ei = O.topk(fx["masked_scores"], 12)
        assert r["scores"].tolist() == es.tolist() and r["ids"].tolist() == ei.tolist()
        assert (fx["kind"][r["ids"]] == "R").all()
    d.close()


def test_driver_without_masking_and_late_switch(fx):
    from cudasw4_amd import driver
    d = _driver(fx, masking=False)
    r = d.scan(fx["letters"])
    assert np.array_equal(_all_scores(d), fx["raw_scores"])
    assert (fx["kind"][r["ids"]] == "D").sum() >= 4
    assert d.masking_counts() == {"positions": 0, "subjects": 0, "residues_seen": 0}
    with pytest.raises(driver.DriverError):
        d.set_subject_masking()           # the database is loaded
    d.close()
    d = driver.Driver(devices=[0])
    for bad in (dict(window=3), dict(window=33), dict(trigger_bits=2.3, extend_bits=2.2)):
        with pytest.raises(driver.DriverError):
            d.set_subject_masking(**bad)
    d.close()


def test_other_parameters_through_the_driver(fx):
    from cudasw4_amd import mask
    W, K1, K2 = 16, 2.2, 2.6
    params = (W, mask.threshold(W, K1), mask.threshold(W, K2))
    ref, positions, subjects = MR.mask_block(fx["chars"], fx["offsets"], fx["lengths"], *params)
    from cudasw4_amd import driver
    d = driver.Driver(devices=[0], num_top=12, kinds=(0, 0, 3, 3), max_gpu_mem=1, max_batch_bytes=30000)
    d.set_subject_masking(True, W, K1, K2)
    d.db_from_arrays(fx["chars"], fx["offsets"], fx["lengths"])
    d.scan(fx["letters"])
    assert np.array_equal(_all_scores(d), O.scan(fx["query"], ref, fx["offsets"], fx["lengths"], simd=True))
    assert d.masking_counts() == {"positions": positions, "subjects": subjects, "residues_seen": fx["residues"]}
    assert positions != fx["positions"]
    d.close()


def _cigar_words(text):
    ops = {"I": 1, "D": 2, "=": 7, "X": 8}
    return [(int(n) << 4) | ops[op] for n, op in re.findall(r"(\d+)([IDX=])", text)]


def _subject(f, chars, i):
    o = int(f["offsets"][i])
    return chars[o:o + int(f["lengths"][i])]


def test_alignment_and_calibration_see_the_masked_subjects(fx):
    from cudasw4_amd import capi, driver
    m = O.blosum21(62)
    d = _driver(fx)
    r = d.scan(fx["letters"])
    # the relatives, and the best decoys with their masked scores: sw_align_hits refuses a pair whose score differs from the
    # scan's, so every OK holds the host statement of the rule against the device's
    decoys = np.nonzero(fx["kind"] == "D")[0]
    decoys = decoys[np.argsort(-fx["masked_scores"][decoys], kind="stable")[:6]]
    hits = {"ids": np.concatenate([r["ids"], decoys]).astype(np.int64),
            "scores": np.concatenate([r["scores"], fx["masked_scores"][decoys]]).astype(np.int32)}
    recs, cigars = d.align_hits(fx["letters"], hits)
    assert (recs["status"] == capi.ALIGN_OK).all() and (recs["score"] == hits["scores"]).all()
    for rec, cigar, i in zip(recs, cigars, hits["ids"]):
        assert AR.rescore(fx["query"], _subject(fx, fx["masked"], int(i)), m, -11, -1, rec, _cigar_words(cigar)) == rec["score"]
    # a decoy's raw score is not its masked score: with the raw one the pair is refused
    worst = int(decoys[0])
    assert fx["raw_scores"][worst] > fx["masked_scores"][worst]
    raw = {"ids": np.array([worst], dtype=np.int64), "scores": fx["raw_scores"][[worst]].astype(np.int32)}
    with pytest.raises(driver.DriverError):
        d.align_hits(fx["letters"], raw)
    # several alignments per hit
    lists = d.align_hits(fx["letters"], r, max_hsps=2, min_score=25)
    assert len(lists) == len(r["ids"])
    for hsps, i, sc in zip(lists, r["ids"], r["scores"]):
        assert 1 <= len(hsps) <= 2 and hsps[0][0]["status"] == capi.ALIGN_OK and hsps[0][0]["score"] == sc
        for rec, cigar in hsps:
            assert AR.rescore(fx["query"], _subject(fx, fx["masked"], int(i)), m, -11, -1, rec, _cigar_words(cigar)) == rec["score"]
    # the reference letters stay raw
    assert d.reference_length(int(decoys[0])) == int(fx["lengths"][decoys[0]])
    # the shuffled calibration: its sample is the host-masked subjects
    d.set_statistics(True, mode="shuffled", shuffles=2, seed=5)
    rs = d.scan(fx["letters"])
    hist, sumlen, fit, M, reps = SR.calibrate(lambda a, b, l: O.scan(fx["query"], a, b, l, simd=True), fx["masked"], fx["offsets"],
                                              fx["lengths"], 5, shuffles=2)
    assert rs["stats"]["mode"] == "shuffled" and (rs["stats"]["subjects"], rs["stats"]["replicas"]) == (M, reps)
    assert np.array_equal(rs["stats"]["hist"], hist) and np.array_equal(rs["stats"]["sumlen"], sumlen)
    raw_hist = SR.calibrate(lambda a, b, l: O.scan(fx["query"], a, b, l, simd=True), fx["chars"], fx["offsets"], fx["lengths"], 5, shuffles=2)[0]
    assert not np.array_equal(hist, raw_hist)
    d.close()


# ---- the command line ----------------------------------------------------------------------------------------------------------

def test_align_mask_subjects(fx, tmp_path):
    from cudasw4_amd import driver
    chars, offsets, lengths = fx["chars"], fx["offsets"], fx["lengths"]
    lut = np.frombuffer(MC.LETTERS.encode(), dtype=np.uint8)
    fasta = str(tmp_path / "db.fa")
    with open(fasta, "w") as f:
        for i in range(len(lengths)):   # the header carries the subject's kind and its position in the fixture
            f.write(">%s%d\n%s\n" % (fx["kind"][i], i, lut[_subject(fx, chars, i)].tobytes().decode()))
    prefix = str(tmp_path / "fx")
    p = subprocess.run([driver.MAKEDB, fasta, prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    qfile = str(tmp_path / "q.fa")
    with open(qfile, "w") as f:
        f.write(">query\n%s\n" % fx["letters"])

    def run(args, name, env=None):
        of = str(tmp_path / name)
        r = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", qfile, "--db", prefix, "--top", "12", "--of", of] + args,
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(of).read(), r

    def rows(tsv):
        return [l.split("\t") for l in tsv.splitlines()[1:]]

    def kinds(tsv):
        return [re.search(r"\b([DRB])\d+\b", l).group(1) for l in tsv.splitlines()[1:]]

    plain, r0 = run(["--tsv"], "plain.tsv")
    def masking_lines(r):   # of the option dump and of --verbose
        return [l for l in r.stdout.splitlines() if l.startswith(("mask", "subject masking"))]

    assert kinds(plain).count("D") >= 4 and masking_lines(r0) == []
    assert sorted(int(x[4]) for x in rows(plain)) == sorted(O.topk(fx["raw_scores"], 12)[0].tolist())
    masked, r1 = run(["--tsv", "--maskSubjects", "--verbose"], "masked.tsv")
    assert kinds(masked) == ["R"] * 12
    assert [int(x[4]) for x in rows(masked)] == O.topk(fx["masked_scores"], 12)[0].tolist()
    line = "subject masking: window 12 trigger 1.9 extend 2.2: %d of %d residues in %d of %d subjects" % (
        fx["positions"], fx["residues"], fx["subjects"], len(lengths))
    assert line in r1.stdout.splitlines(), [l for l in r1.stdout.splitlines() if "mask" in l]
    assert masking_lines(r1) == ["maskSubjects: 1", line]
    # streamed, with other parameters
    ref16 = MR.mask_block(chars, offsets, lengths, 16, MR.threshold(16, 2.2), MR.threshold(16, 2.6))
    _, r2 = run(["--tsv", "--maskSubjects", "--maskWindow", "16", "--maskTrigger", "2.2", "--maskExtend", "2.6", "--verbose",
                 "--maxGpuMem", "1", "--maxBatchBytes", "30000"], "w16.tsv")
    assert "subject masking: window 16 trigger 2.2 extend 2.6: %d of %d residues in %d of %d subjects" % (
        ref16[1], fx["residues"], ref16[2], len(lengths)) in r2.stdout.splitlines()
    # alignments of masked subjects (the score check of every aligned hit passes), also in the plain form
    al, _ = run(["--tsv", "--maskSubjects", "--alignments"], "al.tsv")
    assert kinds(al) == ["R"] * 12 and all(re.fullmatch(r"(\d+[IDX=])+", x[-1]) for x in rows(al))
    run(["--tsv", "--maskSubjects", "--statistics", "shuffled", "--rankBy", "evalue"], "sh.tsv")
    # without the flag: the same output, field by field, as a run with no library override in the environment
    import os
    env = {k: v for k, v in os.environ.items() if k != "CUDASW4_AMD_LIB"}
    for args, name in ((["--tsv", "--alignments"], "b.tsv"), ([], "c.txt")):
        a, ra = run(args, "x-" + name)
        b, rb = run(args, "y-" + name, env=env)
        assert a == b and len(a) > 0
        assert [l.split("\t") for l in a.splitlines()] == [l.split("\t") for l in b.splitlines()]
        assert masking_lines(ra) == [] and masking_lines(rb) == []
