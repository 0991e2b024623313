"""GPU: the C++ host driver (libcudasw4_host.so) and the align command line, end to end."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

GOLDEN_DB = os.path.join(O.GOLDEN_DIR, "allqueries_db", "aq")
FASTA = os.path.join(O.GOLDEN_DIR, "allqueries.fasta")


def expected_top(row, k):
    s, i = O.topk(np.asarray(row, dtype=np.int32), k)
    return s.tolist(), i.tolist()


@pytest.mark.parametrize("kinds", [(0, 0, 3, 3), (1, 1, 2, 2), (2, 1, 2, 2), (3, 0, 3, 3)])
def test_driver_allvsall_resident(kinds):
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    _, seqs = O.read_fasta(FASTA)
    d = driver.Driver(devices=[0], num_top=20, kinds=kinds)
    d.open_db(GOLDEN_DB)
    d.upload()
    assert d.num_sequences() == 20 and d.num_gpus() == 1
    for qi, q in enumerate(seqs):
        r = d.scan(q)
        es, ei = expected_top(g["allvsall"][qi], 20)
        assert r["scores"].tolist() == es, (kinds, qi)
        assert r["ids"].tolist() == ei
        if kinds[0] in (0, 1):  # the reference's statistic: subjects whose score reaches the packed kind's limit
            limit = 2048 if kinds[0] == 0 else 25000
            assert r["num_overflows"] == sum(1 for x in g["allvsall"][qi] if x >= limit), (kinds, qi)
            assert r["num_overflows"] <= r["num_rescored"] <= sum(1 for x in g["allvsall"][qi] if x >= limit // 4)
        else:
            assert r["num_overflows"] == 0 or kinds[1] in (0, 1)
    assert d.reference_length(19) == 5478 and "LGB1_VICFA" in d.reference_header(0)


def test_driver_streamed_batches_and_two_shards_on_one_gpu():
    """--maxGpuMem below the DB size forces the batch-streaming path; devices=[0,0] runs two shards
    (the multi-GPU code path: per-partition char-balanced ranges, local->global ids, host merge)."""
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    _, seqs = O.read_fasta(FASTA)
    for devices, kwargs in (([0], dict(max_gpu_mem=1, max_batch_bytes=6000)), ([0, 0], {}), ([0, 0, 0], dict(max_gpu_mem=1, max_batch_bytes=3000))):
        d = driver.Driver(devices=devices, num_top=7, kinds=(0, 0, 3, 3), **kwargs)
        d.open_db(GOLDEN_DB)
        assert d.num_gpus() == len(devices)
        for qi in (0, 4, 13, 19):
            r = d.scan(seqs[qi])
            es, ei = expected_top(g["allvsall"][qi], 7)
            assert r["scores"].tolist() == es, (devices, qi)
            assert r["ids"].tolist() == ei
            assert r["num_overflows"] == sum(1 for x in g["allvsall"][qi] if x >= 2048), (devices, qi)
            assert r["num_rescored"] >= r["num_overflows"]
        d.close()


def test_streamed_driver_switches_databases_between_scans():
    """A streamed scan leaves the first batch of the NEXT scan in a staging buffer (the buffers rotate across scans) and
    keeps long-subject launches running next to the following batches.  One driver, batch counts of 1, 2, 3, 4 and 7
    (every rotation phase of the three buffers), several scans each, then ANOTHER DB on the same driver: nothing staged
    for the old DB may be used for the new one.  Every score against the oracle."""
    from cudasw4_amd import driver
    rng = np.random.default_rng(77)
    letters = b"ARNDCQEGHILKMFPSTWYV"

    def make(n, lo, hi, giants):
        lens = np.sort(np.concatenate([rng.integers(lo, hi, n), np.array(giants, dtype=np.int64)])).astype(np.int64)
        return O.make_db([rng.integers(0, 20, int(l)).astype(np.int8) for l in lens])

    dbs = [make(300, 20, 400, [1500, 9000]), make(200, 100, 900, [2000]), make(500, 1, 60, [])]
    queries = [rng.integers(0, 20, ql).astype(np.int8) for ql in (40, 300, 900)]
    for batch_bytes in (1 << 30, 40000, 26000, 20000, 11000):
        d = driver.Driver(devices=[0], num_top=5, kinds=(0, 0, 3, 3), max_gpu_mem=1, max_batch_bytes=batch_bytes)
        for chars, offsets, lengths in dbs + dbs[:1]:
            d.db_from_arrays(chars, offsets, lengths)
            assert not d.shard_info(0)["resident"]
            for q in queries:
                expect = O.scan(q, chars, offsets, lengths, simd=True)
                for _ in range(2):
                    r = d.scan(bytes(letters[c] for c in q))
                    ids, sc = d.all_scores()
                    got = np.empty_like(sc)
                    got[ids] = sc
                    np.testing.assert_array_equal(got.astype(np.int32), expect, err_msg="batch bytes %d" % batch_bytes)
                    es, ei = O.topk(expect, 5)
                    assert r["scores"].tolist() == es.tolist() and r["ids"].tolist() == ei.tolist()
        d.close()


def test_driver_pseudo_db():
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    _, seqs = O.read_fasta(FASTA)
    d = driver.Driver(devices=[0], num_top=3, kinds=(1, 1, 2, 2))
    d.pseudo_db(5001, 256)
    d.upload()
    for qi in (0, 10, 19):
        r = d.scan(seqs[qi])
        assert r["scores"].tolist() == [g["pseudo"]["256"][qi]] * 3 and r["ids"].tolist() == [0, 1, 2]
        assert r["gcups"] > 0


def test_driver_random_db_from_makedb(tmp_path):
    """makedb -> align path on a ragged random DB, all partitions incl. > 8000, vs the oracle."""
    from cudasw4_amd import driver
    rng = np.random.default_rng(17)
    letters = "ARNDCQEGHILKMFPSTWYVX"
    lens = list(rng.integers(1, 400, 900)) + list(rng.integers(400, 2500, 60)) + [8100, 9000]
    recs = []
    for i, L in enumerate(lens):
        recs.append(">seq%d\n%s\n" % (i, "".join(letters[int(c)] for c in rng.integers(0, 21, int(L)))))
    fasta = str(tmp_path / "db.fa")
    open(fasta, "w").write("".join(recs))
    prefix = str(tmp_path / "db")
    subprocess.check_call([driver.MAKEDB, fasta, prefix], stdout=subprocess.DEVNULL)
    chars = np.fromfile(prefix + "0chars", dtype=np.int8)
    offsets = np.fromfile(prefix + "0offsets", dtype=np.uint64)
    lengths = np.fromfile(prefix + "0lengths", dtype=np.int32)
    q = "".join(letters[int(c)] for c in rng.integers(0, 20, 700))
    expect = O.scan(O.encode(q), chars, offsets, lengths, simd=True)
    es, ei = O.topk(expect, 50)
    for kinds in ((0, 0, 3, 3), (1, 1, 2, 2)):
        for devices in ([0], [0, 0]):
            d = driver.Driver(devices=devices, num_top=50, kinds=kinds)
            d.open_db(prefix)
            r = d.scan(q)
            assert r["scores"].tolist() == es.tolist() and r["ids"].tolist() == ei.tolist(), (kinds, devices)
            d.close()


@pytest.mark.parametrize("kinds", [(0, 0, 3, 3), (1, 1, 2, 2)])
def test_long_subjects_as_windows_for_short_queries(kinds, monkeypatch):
    """Exact windowing (include/cudasw4_amd.h: sw_window_overlap): for a short query the giants of a DB
    are cut into overlapping windows that are scanned as independent subjects, and a subject's score is the maximum over
    its windows.  Every score must equal the unsplit scan's and the oracle's — in particular for alignments that straddle
    a window boundary: the query itself, and the query with a 150-residue insertion in its middle, are planted right
    across the first boundaries of several giants."""
    from cudasw4_amd import driver
    rng = np.random.default_rng(314)
    _, letters = O.read_fasta(FASTA)
    alphabet = b"ARNDCQEGHILKMFPSTWYV"
    short_q = [letters[0][:48], letters[0], letters[3][:300]]          # 48, 144 and 300 residues
    long_q = letters[9]                                                  # 1000 residues: W = 12 001, only the longest giant is cut
    seqs = [bytes(rng.choice(list(alphabet), int(l)).astype(np.uint8)) for l in rng.integers(30, 1200, 1500)]
    giants = []
    for gi, l in enumerate((8100, 9000, 12000, 17000, 23000, 29000, 35000)):
        s = bytearray(rng.choice(list(alphabet), l).astype(np.uint8).tobytes())
        q = short_q[gi % 3]
        # window stride for these queries: max(W rounded to 4, 2048); plant across the first two boundaries
        W = len(q) + len(q) * 11 + 1
        C = max((W + 3) // 4 * 4, 2048)
        at = C - len(q) // 2
        s[at:at + len(q)] = q
        gapped = q[:len(q) // 2] + bytes(rng.choice(list(alphabet), 150).astype(np.uint8)) + q[len(q) // 2:]
        at2 = 2 * C - len(q) // 2 - 40
        if at2 + len(gapped) < l:
            s[at2:at2 + len(gapped)] = gapped
        giants.append(bytes(s))
    db_seqs = sorted(seqs + giants, key=len)
    enc = [O.encode(x) for x in db_seqs]
    chars, offsets, lengths = O.make_db(enc)
    results = {}
    for windows in (True, False):
        # "always": also where the engine's time estimate would not bother; "0": never
        monkeypatch.setenv("CUDASW4_AMD_WINDOWS", "always" if windows else "0")
        d = driver.Driver(devices=[0], num_top=10, kinds=kinds)
        d.db_from_arrays(chars, offsets, lengths)
        d.upload()
        out = []
        for q in short_q + [long_q]:
            r = d.scan(q)
            sc, ids = d.last_scores(0)
            out.append((sc.copy(), r["scores"].tolist(), r["ids"].tolist()))
        launches, nwin = d.window_stats()
        results[windows] = (out, launches, nwin)
        d.close()
    (with_w, launches, nwin), (without, l0, n0) = results[True], results[False]
    assert l0 == 0 and n0 == 0
    assert launches == 4 and nwin > 4 * len(giants)          # every query cut at least the longest giant
    for qi, q in enumerate(short_q + [long_q]):
        expect = O.scan(O.encode(q), chars, offsets, lengths, simd=True)
        assert (with_w[qi][0] == expect).all(), (qi, np.nonzero(with_w[qi][0] != expect)[0][:5])
        assert (without[qi][0] == expect).all()
        assert with_w[qi][1:] == without[qi][1:]
    # the planted alignments are what the top of the lists is made of: they were found across the boundaries
    assert with_w[1][1][0] >= 700 and with_w[0][1][0] >= 230


@pytest.mark.parametrize("kinds", [(0, 0, 3, 3), (1, 1, 2, 2)])
def test_rescore_service_beside_the_bulk_launch(kinds, monkeypatch):
    """The bulk launch's overflow list is re-scored WHILE it is filled (include/cudasw4_amd.h: sw_rescore_service): a few
    workgroups started beside the packed launch poll the list, the ordinary re-score launch takes what they have not
    taken, entries are claimed by compare-and-swap.  Same DB — relatives of the queries among 20 000 unrelated sequences,
    so that hundreds of subjects overflow in fp16 and some in int16 — with the service forced on, forced off, and left to
    the driver's feedback: every score equals the oracle, the re-score counts agree, nothing is scored twice or lost."""
    from cudasw4_amd import driver, synthdb
    rng = np.random.default_rng(99)
    _, letters = O.read_fasta(FASTA)
    queries = [letters[5], letters[11], letters[16]]          # 567, 2005 and 4548 residues
    fam = synthdb.family_members([O.encode(q) for q in queries], seed=7, min_size=60, max_size=60)
    lengths = synthdb.sprot_like_lengths(20000, seed=8, max_len=6000)
    bg = synthdb.random_db(lengths, seed=9, composition=synthdb.SPROT_COMPOSITION)
    seqs = [bg[0][int(bg[1][i]):int(bg[1][i]) + int(bg[2][i])] for i in range(len(lengths))] + list(fam)
    seqs.sort(key=len)
    chars, offsets, lens = O.make_db(seqs)
    expect = [O.scan(O.encode(q), chars, offsets, lens, simd=True) for q in queries]
    limit = 2048 if kinds[0] == 0 else 25000
    runs = {}
    for mode in ("1", "0", None):
        if mode is None:
            monkeypatch.delenv("CUDASW4_AMD_RESCORE_SERVICE", raising=False)
        else:
            monkeypatch.setenv("CUDASW4_AMD_RESCORE_SERVICE", mode)
        d = driver.Driver(devices=[0], num_top=20, kinds=kinds)
        d.db_from_arrays(chars, offsets, lens)
        d.upload()
        out = []
        for rep in range(2):
            for qi, q in enumerate(queries):
                r = d.scan(q)
                sc, _ = d.last_scores(0)
                assert (sc == expect[qi]).all(), (mode, qi, np.nonzero(sc != expect[qi])[0][:5])
                assert r["num_overflows"] == int((expect[qi] >= limit).sum()) and r["num_rescored"] >= r["num_overflows"]
                out.append((r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"], r["num_rescored"]))
        runs[mode] = (out, d.service_launches())
        d.close()
    assert runs["1"][0] == runs["0"][0] == runs[None][0]
    assert runs["1"][1] == 6 and runs["0"][1] == 0 and runs[None][1] >= 3      # feedback: on while scans re-score
    assert sum(o[3] for o in runs["1"][0]) > (100 if kinds[0] == 0 else 0)


@pytest.mark.parametrize("kinds", [(0, 0, 3, 3), (1, 1, 2, 2), (3, 0, 3, 3)])
def test_tail_hand_over_between_two_queries_in_flight(kinds, monkeypatch):
    """A query submitted while the one before is still running takes the GPU's other lane (context, work stream, score
    arrays) and its bulk launch is gated on the dry signal of the earlier one (include/cudasw4_amd.h: sw_set_dry_signal).
    Same DB as the service test (relatives of the queries: overflow lists, re-scores, a side launch for the long
    subjects), queries of 48 ... 4548 residues submitted two at a time: every score of every query equals the oracle, top
    lists and counters equal those of one query at a time, and every query but the first was gated."""
    from cudasw4_amd import driver, synthdb
    _, letters = O.read_fasta(FASTA)
    queries = [letters[5], letters[11][:48], letters[11], letters[1], letters[16], letters[8]]
    fam = synthdb.family_members([O.encode(q) for q in queries if len(q) > 400], seed=7, min_size=40, max_size=40)
    lengths = synthdb.sprot_like_lengths(20000, seed=18, max_len=9000)
    bg = synthdb.random_db(lengths, seed=19, composition=synthdb.SPROT_COMPOSITION)
    seqs = [bg[0][int(bg[1][i]):int(bg[1][i]) + int(bg[2][i])] for i in range(len(lengths))] + list(fam)
    seqs.sort(key=len)
    chars, offsets, lens = O.make_db(seqs)
    expect = [O.scan(O.encode(q), chars, offsets, lens, simd=True) for q in queries]
    runs = {}
    for mode in ("serial", "lanes", "off"):
        monkeypatch.delenv("CUDASW4_AMD_TAIL_OVERLAP", raising=False)
        if mode == "off":
            monkeypatch.setenv("CUDASW4_AMD_TAIL_OVERLAP", "0")
        d = driver.Driver(devices=[0], num_top=20, kinds=kinds)
        d.db_from_arrays(chars, offsets, lens)
        d.upload()
        out = []
        order = list(range(len(queries))) * 2
        if mode == "serial":
            for qi in order:
                r = d.scan(queries[qi])
                out.append((r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"], r["num_rescored"]))
        else:
            d.submit(queries[order[0]])
            for n, qi in enumerate(order):
                if n + 1 < len(order):
                    d.submit(queries[order[n + 1]])
                r = d.collect()
                if mode == "lanes":  # (on one lane the next query is already overwriting the score array)
                    sc, _ = d.last_scores(0)     # of the query just collected, while the next one runs on the other lane
                    assert (sc == expect[qi]).all(), (mode, n, qi, np.nonzero(sc != expect[qi])[0][:5])
                out.append((r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"], r["num_rescored"]))
        runs[mode] = (out, d.tail_overlaps())
        d.close()
    assert runs["serial"][0] == runs["lanes"][0] == runs["off"][0]
    assert runs["serial"][1] == 0 and runs["off"][1] == 0 and runs["lanes"][1] == 2 * len(queries) - 1
    if kinds[0] != 3:
        assert sum(o[3] for o in runs["lanes"][0]) > 0


def test_handshake_is_probed_and_falls_back_under_a_serialising_profiler(monkeypatch):
    """the bulk launch waits (hipStreamWaitValue32) for a value only device code raises.  The driver probes that
    pattern once at construction (sw_probe_handshake, bounded) and runs without start handshake, re-score service and tail
    hand-over where it does not hold or where the environment says kernels are serialised (rocprofv3 --pmc exports
    ROCPROF_COUNTER_COLLECTION): same results, no service launch, no gated query, no hang."""
    from cudasw4_amd import driver, synthdb
    _, letters = O.read_fasta(FASTA)
    queries = [letters[5], letters[11]]
    fam = synthdb.family_members([O.encode(q) for q in queries], seed=7, min_size=30, max_size=30)
    lengths = synthdb.sprot_like_lengths(12000, seed=18, max_len=9000)
    bg = synthdb.random_db(lengths, seed=19, composition=synthdb.SPROT_COMPOSITION)
    seqs = [bg[0][int(bg[1][i]):int(bg[1][i]) + int(bg[2][i])] for i in range(len(lengths))] + list(fam)
    seqs.sort(key=len)
    chars, offsets, lens = O.make_db(seqs)
    expect = [O.scan(O.encode(q), chars, offsets, lens, simd=True) for q in queries]
    seen = {}
    for mode in ("plain", "profiler"):
        monkeypatch.delenv("ROCPROF_COUNTER_COLLECTION", raising=False)
        if mode == "profiler":
            monkeypatch.setenv("ROCPROF_COUNTER_COLLECTION", "1")
        d = driver.Driver(devices=[0], num_top=20, kinds=(0, 0, 3, 3))
        assert d.handshake_active() == (mode == "plain")
        d.db_from_arrays(chars, offsets, lens)
        d.upload()
        out = []
        d.submit(queries[0])
        for n in range(4):
            if n + 1 < 4:
                d.submit(queries[(n + 1) % 2])
            r = d.collect()
            out.append((r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"]))
        for qi, q in enumerate(queries):
            d.scan(q)
            sc, _ = d.last_scores(0)
            assert (sc == expect[qi]).all(), (mode, qi)
        seen[mode] = (out, d.service_launches(), d.tail_overlaps())
        d.close()
    assert seen["plain"][0] == seen["profiler"][0]
    assert seen["profiler"][1:] == (0, 0) and seen["plain"][1] > 0


@pytest.mark.parametrize("kinds", [(1, 1, 2, 2), (0, 0, 3, 3)])
def test_pipelined_giants_forced_off_on_and_by_the_estimate(kinds, monkeypatch):
    """Small shards of real DBs: the longest subjects of partitions 34 / 35 as pipelines of one-wave stages
    (sw_scan_rows_pipelined, chosen inside sw_scan_batch), forced off (CUDASW4_AMD_PIPELINES=0), forced on (=always) and left
    to the engine's walk-time estimate: every score of every query equals the oracle each way, the counter says which path ran."""
    from cudasw4_amd import driver, synthdb
    rng = np.random.default_rng(5)
    _, letters = O.read_fasta(FASTA)
    queries = [letters[11][:60], letters[5], letters[11]]      # 60, 567 and 2005 residues
    fam = synthdb.family_members([O.encode(q) for q in queries[1:]], seed=3, min_size=30, max_size=30)
    lens = np.concatenate([synthdb.sprot_like_lengths(6000, seed=28, max_len=1200), rng.integers(1281, 7900, 700),
                           np.array([8001, 9500, 15000, 26000, 40960])])
    bg = synthdb.random_db(np.sort(lens).astype(np.int32), seed=29, composition=synthdb.SPROT_COMPOSITION)
    seqs = [bg[0][int(bg[1][i]):int(bg[1][i]) + int(bg[2][i])] for i in range(len(lens))] + list(fam)
    seqs.sort(key=len)
    chars, offsets, lengths = O.make_db(seqs)
    expect = [O.scan(O.encode(q), chars, offsets, lengths, simd=True) for q in queries]
    seen = {}
    for pipes in ("0", "always", None):
        if pipes is None:
            monkeypatch.delenv("CUDASW4_AMD_PIPELINES", raising=False)
        else:
            monkeypatch.setenv("CUDASW4_AMD_PIPELINES", pipes)
        d = driver.Driver(devices=[0], num_top=15, kinds=kinds)
        d.db_from_arrays(chars, offsets, lengths)
        d.upload()
        tops = []
        for qi, q in enumerate(queries):
            r = d.scan(q)
            sc, _ = d.last_scores(0)
            assert (sc == expect[qi]).all(), (pipes, qi, np.nonzero(sc != expect[qi])[0][:5], lengths[np.nonzero(sc != expect[qi])[0][:5]])
            tops.append((r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"]))
        seen[pipes] = (tops, d.pipeline_launches())
        d.close()
    assert len({str(v[0]) for v in seen.values()}) == 1
    assert seen["0"][1] == 0
    # "always": every subject of partition 35 and the longest of partition 34, for every query whose giants are not cut into
    # windows instead (the 60- and the 567-residue query: the span bound cuts them)
    assert seen["always"][1] >= 1
    # this DB is a "small shard" and the estimates say so: its longest subjects run pipelined
    assert seen[None][1] >= 1


@pytest.mark.parametrize("kinds", [(1, 1, 2, 2), (0, 0, 3, 3), (3, 0, 3, 3)])
def test_very_short_queries_on_quads_with_partition_34_split_off(kinds, monkeypatch):
    """Round 5: queries up to 96 residues run the bulk of the DB on 4-lane groups (DPP quads), and below such a launch
    partition 34 keeps a launch of its own (a long subject's walk on quads would bound the launch).  Forced on for this
    small DB (the built-in rule wants 12 batches per CU), forced off, and with the split extended to 8-lane bulk
    launches: every score equals the oracle, the kernel events say which shapes ran."""
    from cudasw4_amd import driver, synthdb
    rng = np.random.default_rng(15)
    lens = np.concatenate([synthdb.sprot_like_lengths(5000, seed=31, max_len=1280), rng.integers(1281, 6000, 1500), np.array([9000, 20000])])
    chars, offsets, lengths = synthdb.random_db(np.sort(lens).astype(np.int32), seed=32, composition=synthdb.SPROT_COMPOSITION)
    alphabet = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
    queries = [alphabet[rng.integers(0, 20, n)].tobytes().decode() for n in (7, 48, 95, 96, 97, 130)]
    expect = [O.scan(O.encode(q), chars, offsets, lengths, simd=True) for q in queries]
    shapes = {}
    for mode, env in (("quads", {"CUDASW4_AMD_LANES4_MAX_Q": "96"}), ("off", {"CUDASW4_AMD_LANES4_MAX_Q": "0"}),
                      ("split8", {"CUDASW4_AMD_LANES4_MAX_Q": "96", "CUDASW4_AMD_SPLIT34_MAX_LANES": "8"})):
        for k in ("CUDASW4_AMD_LANES4_MAX_Q", "CUDASW4_AMD_SPLIT34_MAX_LANES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = driver.Driver(devices=[0], num_top=10, kinds=kinds)
        d.db_from_arrays(chars, offsets, lengths)
        d.upload()
        d.record_kernel_events(True)
        for qi, q in enumerate(queries):
            r = d.scan(q)
            sc, _ = d.last_scores(0)
            assert (sc == expect[qi]).all(), (mode, len(q), np.nonzero(sc != expect[qi])[0][:5])
            assert (r["scores"].tolist(), r["ids"].tolist()) == expected_top(expect[qi], 10)
            ev = [e for e in d.take_kernel_events() if not e["rescore"]]
            shapes[(mode, len(q))] = sorted({(e["part_id"], e["lanes"]) for e in ev})
        d.close()
    # (the float configuration scores partition 34 in another kind than the partitions below it: a launch of its own
    # whatever the query, which the planner labels 33 from 512 subjects up — the shape rules of the bulk)
    same_kind = kinds[0] == kinds[1]
    for n in (7, 48, 95, 96):
        assert (33, 4) in shapes[("quads", n)], shapes[("quads", n)]
        if same_kind:
            assert (34, 16) in shapes[("quads", n)], shapes[("quads", n)]
        assert all(l != 4 for _, l in shapes[("off", n)]), shapes[("off", n)]
    # beyond the limit: 8-lane groups, partition 34 merged into their launch unless the split is asked for
    for n in (97, 130):
        assert (33, 8) in shapes[("quads", n)], shapes[("quads", n)]
        if same_kind:
            assert all(p != 34 or l == 64 for p, l in shapes[("quads", n)]), shapes[("quads", n)]
            assert (33, 8) in shapes[("split8", n)] and (34, 16) in shapes[("split8", n)], shapes[("split8", n)]


@pytest.mark.parametrize("dpx", [False, True])
def test_documented_binding_runs_on_the_gpu(dpx):
    """VERDICT r3 test gap (ii): the reference-side binding of INTEGRATION.md section 2 — the verbatim code block, compiled
    against the reference's own headers where they lie (tests/boundary/Makefile; the binary travels to the GPU box) — EXECUTED:
    contexts, matrix, query, the partition walk, overflow re-score and top-K on real device buffers holding the reference's
    all-vs-all DB; every score and the top-5 equal the golden values generated from the reference's own DP."""
    exe = os.path.join(O.ROOT, "oracle", "_ref", "boundary", "binding_gpu")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/boundary/binding_gpu is built only where the reference tree exists (__graft_entry__.build())")
    g = O.golden("ref_scores.json")
    for qi in (2, 9, 16, 19):
        p = subprocess.run([exe, GOLDEN_DB, str(qi)] + (["DPX"] if dpx else []), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "binding ok" in p.stdout, p.stderr[-2000:]
        lines = {l.split()[0]: l.split()[1:] for l in p.stdout.splitlines() if l.split()}
        scores = [int(x) for x in lines["SCORES"]]
        assert scores == g["allvsall"][qi], (qi, scores)
        es, ei = expected_top(g["allvsall"][qi], 5)
        assert [tuple(map(int, t.split(":"))) for t in lines["TOP"]] == list(zip(es, ei))
        limit = 25000 if dpx else 2048
        assert int(lines["OVERFLOWS"][0]) >= sum(1 for v in g["allvsall"][qi] if v >= limit)


def test_align_cli_tsv_and_plain(tmp_path):
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    headers, seqs = O.read_fasta(FASTA)
    of = str(tmp_path / "out.tsv")
    p = subprocess.run([driver.ALIGN, "--query", FASTA, "--db", GOLDEN_DB, "--top", "3", "--tsv", "--of", of, "--verbose",
                        "--uploadFull", "--prefetchDBFile", "--printLengthPartitions"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "Processing query file" in p.stdout and "Total time:" in p.stdout and "GCUPS" in p.stdout
    assert "Processing query 19 ... Done. Scan time:" in p.stdout
    lines = open(of).read().splitlines()
    assert lines[0].split("\t") == ["Query number", "Query length", "Query header", "Result number", "Result score",
                                    "Reference length", "Reference header", "Reference ID in DB"]
    rows = [l.split("\t") for l in lines[1:]]
    assert len(rows) == 20 * 3
    for qi in range(20):
        es, ei = expected_top(g["allvsall"][qi], 3)
        for k in range(3):
            row = rows[qi * 3 + k]
            assert int(row[0]) == qi and int(row[1]) == len(seqs[qi]) and row[2] == headers[qi] and int(row[3]) == k
            assert int(row[4]) == es[k] and int(row[7]) == ei[k] and int(row[5]) == len(seqs[ei[k]]) and row[6] == headers[ei[k]]
    # plain output, dpx kernels, pseudo db
    p = subprocess.run([driver.ALIGN, "--query", FASTA, "--pseudodb", "2000", "128", "--top", "2", "--dpx"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    exp = g["pseudo"]["128"]
    for qi in range(20):
        assert "Query %d, header%s, length %d, num overflows 0" % (qi, headers[qi], len(seqs[qi])) in p.stdout
    assert "Result 0. Score: %d. Length: 128. Header H. referenceId 0" % exp[0] in p.stdout
    assert "Result 1. Score: %d. Length: 128. Header H. referenceId 1" % exp[19] in p.stdout


def test_align_ref_compat_switch(tmp_path):
    """`align --refCompat`: the reference binary parses --gop / --gex and the per-matrix default gap
    scores but always runs -11 / -1 (options.cpp:179-194 never reach the kernels, cudasw4.cuh:539-550), so for --mat
    blosum45|50|80 this build's default output (per-matrix gaps applied) differs from the reference's.  With the switch
    the output is the reference's: equal to the oracle at -11 / -1 on the selected matrix, whatever gap options are
    given; without it the per-matrix defaults apply (and give other scores)."""
    from cudasw4_amd import driver
    headers, seqs = O.read_fasta(FASTA)
    queries = [O.encode(q) for q in seqs]
    chars, offsets, lengths = O.make_db(queries)

    def run(extra):
        of = str(tmp_path / "o.tsv")
        p = subprocess.run(["timeout", "-k", "10", "240", driver.ALIGN, "--query", FASTA, "--db", GOLDEN_DB, "--top", "20", "--tsv", "--of", of] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        rows = [l.split("\t") for l in open(of).read().splitlines()[1:]]
        sc = np.zeros((20, 20), dtype=np.int64)
        for r in rows:
            sc[int(r[0]), int(r[7])] = int(r[4])
        return sc, p.stdout

    def printed_gaps(out):
        """the gap scores of a run's options dump"""
        opts = dict(l.split(": ", 1) for l in out.splitlines() if l.startswith(("gop: ", "gex: ")))
        return int(opts["gop"]), int(opts["gex"])

    def oracle(mat, gop, gex):
        return np.array([O.scan(q, chars, offsets, lengths, m21=O.blosum21(mat), gop=gop, gex=gex, simd=True) for q in queries])

    for mat in (45, 80):
        want = np.array([O.scan(q, chars, offsets, lengths, m21=O.blosum21(mat), gop=-11, gex=-1, simd=True) for q in queries])
        compat, out = run(["--mat", "blosum%d" % mat, "--refCompat"])
        assert (compat == want).all() and "refCompat: gap scores applied are -11 / -1" in out
        compat2, _ = run(["--mat", "blosum%d" % mat, "--refCompat", "--gop", "-5", "--gex", "-3"])
        assert (compat2 == want).all()
        native, out = run(["--mat", "blosum%d" % mat])
        assert "refCompat" not in out and (native != want).any()
        # ... and what it prints without the switch are the scores under the gap scores it says it applies
        gop, gex = printed_gaps(out)
        assert (gop, gex) != (-11, -1) and "blosum: blosum%d" % mat in out
        assert (native == oracle(mat, gop, gex)).all(), (mat, gop, gex, np.argwhere(native != oracle(mat, gop, gex))[:5])
    # explicit gap scores reach the scan
    explicit, out = run(["--gop", "-5", "--gex", "-3"])
    assert printed_gaps(out) == (-5, -3) and "refCompat" not in out
    assert (explicit == oracle(62, -5, -3)).all(), np.argwhere(explicit != oracle(62, -5, -3))[:5]
    # the environment switch does the same
    env = dict(os.environ, CUDASW4_AMD_REF_COMPAT="1")
    of = str(tmp_path / "e.tsv")
    p = subprocess.run([driver.ALIGN, "--query", FASTA, "--db", GOLDEN_DB, "--top", "1", "--tsv", "--of", of, "--mat", "blosum50"],
                       capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "refCompat: gap scores applied are -11 / -1" in p.stdout


def test_align_cli_hybrid_residency_and_pipelined_queries(monkeypatch):
    """`align --maxGpuMem` below the DB size: the verbose output says how much of the shard stays cached in device memory
    (the reference prints "N out of M DB batches will be cached in gpu memory", cudasw4.cuh:1044-1046), the results are
    the golden ones — also with the next query submitted before the current one is collected (CUDASW4_AMD_PIPELINE=1),
    whose output keeps the reference's order and format."""
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    headers, seqs = O.read_fasta(FASTA)
    outputs = []
    for pipe in ("0", "1"):
        monkeypatch.setenv("CUDASW4_AMD_PIPELINE", pipe)
        p = subprocess.run([driver.ALIGN, "--query", FASTA, "--db", GOLDEN_DB, "--top", "2", "--verbose",
                            "--maxGpuMem", "40683", "--maxBatchBytes", "3000"], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        m = [l for l in p.stdout.splitlines() if "chars cached in gpu memory" in l]
        assert len(m) == 1, p.stdout[:2000]
        cached, streamed = int(m[0].split(" chars cached")[0].split()[-1]), int(m[0].split(" streamed in ")[0].split()[-1])
        assert 0 < cached < 41780 and cached + streamed == 41780
        for qi in range(20):
            es, ei = expected_top(g["allvsall"][qi], 2)
            assert "Query %d, header%s, length %d, num overflows %d" % (
                qi, headers[qi], len(seqs[qi]), sum(1 for x in g["allvsall"][qi] if x >= 2048)) in p.stdout
            assert "Result 0. Score: %d. Length: %d. Header %s. referenceId %d" % (es[0], len(seqs[ei[0]]), headers[ei[0]], ei[0]) in p.stdout
        order = [int(l.split()[2]) for l in p.stdout.splitlines() if l.startswith("Processing query ") and "file" not in l]
        assert order == list(range(20))
        outputs.append([l for l in p.stdout.splitlines() if l.startswith("Result ") or l.startswith("Query ")])
    assert outputs[0] == outputs[1]


def test_align_interactive_mode(tmp_path):
    """main.cu:336-424: 's <sequence>' (multi-line until an empty line), 'f <file>', 'exit'."""
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    headers, seqs = O.read_fasta(FASTA)
    q3 = seqs[3].decode()
    script = "s %s\n%s\n\nf %s\nbogus\nexit\n" % (q3[:100], q3[100:], FASTA)
    of = str(tmp_path / "out.txt")
    p = subprocess.run([driver.ALIGN, "--db", GOLDEN_DB, "--interactive", "--top", "2", "--of", of],
                       input=script, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "Interactive mode ready" in p.stdout and "Unrecognized command: bogus" in p.stdout
    assert p.stdout.count("Waiting for command...") >= 3
    out = open(of).read().splitlines()
    es, ei = expected_top(g["allvsall"][3], 2)
    assert out[0] == "Result 0. Score: %d. Length: %d. Header %s. referenceId %d" % (es[0], len(seqs[ei[0]]), headers[ei[0]], ei[0])
    assert out[1].startswith("Result 1. Score: %d." % es[1])
    # the 'f' command prints the same two-line blocks for all 20 queries
    assert len(out) == 2 + 20 * 2
    es19, ei19 = expected_top(g["allvsall"][19], 2)
    assert out[-2].startswith("Result 0. Score: %d." % es19[0]) and out[-2].endswith("referenceId %d" % ei19[0])


def test_driver_and_align_with_full_25_letter_matrix(tmp_path):
    """`--mat blosum62_25` / matrix=6225: the query is encoded with 25 letters (B, J, Z, X, * distinct), the DB stays in
    the dbdata alphabet; C++ driver and align CLI vs the oracle."""
    from cudasw4_amd import driver
    rng = np.random.default_rng(8)
    chars = np.fromfile(GOLDEN_DB + "0chars", dtype=np.int8)
    offsets = np.fromfile(GOLDEN_DB + "0offsets", dtype=np.uint64)
    lengths = np.fromfile(GOLDEN_DB + "0lengths", dtype=np.int32)
    _, seqs = O.read_fasta(FASTA)
    q = bytearray(seqs[7])
    for pos, letter in zip(rng.choice(len(q), 40, replace=False), b"BJZX*" * 8):
        q[pos] = letter
    q = bytes(q)
    m = driver.matrix25(62).reshape(25, 25)[:, list(range(20)) + [23]]
    expect = O.scan(driver.encode25(q), chars, offsets, lengths, m21=np.ascontiguousarray(m))
    assert (expect != O.scan(O.encode(q), chars, offsets, lengths)).any()  # the full table does change scores
    es, ei = O.topk(expect, 6)
    d = driver.Driver(devices=[0], num_top=6, matrix=6225, kinds=(1, 1, 2, 2))
    d.open_db(GOLDEN_DB)
    r = d.scan(q)
    assert r["scores"].tolist() == es.tolist() and r["ids"].tolist() == ei.tolist()
    d.close()
    fa = str(tmp_path / "q.fa")
    open(fa, "wb").write(b">q\n" + q + b"\n")
    p = subprocess.run([driver.ALIGN, "--query", fa, "--db", GOLDEN_DB, "--top", "2", "--mat", "blosum62_25"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "blosum: blosum62_25" in p.stdout and "Result 0. Score: %d." % es[0] in p.stdout and "Result 1. Score: %d." % es[1] in p.stdout


def test_align_with_the_vector_loader_fallback():
    """`align` when the DB files cannot be memory-mapped (forced here): loadDBWithVectors path (main.cu:180-191),
    same hits; with --maxGpuMem 1 the shard streams from the in-memory copy."""
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    env = dict(os.environ, CUDASW4_AMD_DB_NO_MMAP="1")
    for extra in ([], ["--maxGpuMem", "1", "--maxBatchBytes", "5000"]):
        p = subprocess.run([driver.ALIGN, "--query", FASTA, "--db", GOLDEN_DB, "--top", "1", "--verbose"] + extra,
                           capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr
        assert "Failed to map db files. Using fallback db." in p.stdout
        for qi in (0, 9, 19):
            es, ei = expected_top(g["allvsall"][qi], 1)
            assert "Result 0. Score: %d." % es[0] in p.stdout


def test_more_than_4_gib_of_subject_chars_resident_and_streamed():
    """Offsets beyond 2^32: a pseudo DB of 8.5 million subjects x 512 residues (4.35 GB of chars) through the C++ driver,
    resident and above a 2 GiB memory limit (part cached, the rest streamed); every score equals the reference's golden score, ids are global."""
    from cudasw4_amd import driver
    g = O.golden("ref_scores.json")
    _, seqs = O.read_fasta(FASTA)
    n = 8_500_000
    for kw in ({}, dict(max_gpu_mem=2 << 30, max_batch_bytes=1 << 30)):
        d = driver.Driver(devices=[0], num_top=5, kinds=(0, 0, 3, 3), **kw)
        d.pseudo_db(n, 512)
        if not kw:
            d.upload()
        assert d.shard_info(0)["resident"] == (not kw) and d.shard_info(0)["chars"] == n * 512 > 2**32
        for qi in (0, 3):
            r = d.scan(seqs[qi])
            assert r["scores"].tolist() == [g["pseudo"]["512"][qi]] * 5 and r["ids"].tolist() == [0, 1, 2, 3, 4]
            sc, ids = d.last_scores(0)
            assert len(sc) == n and int(sc.min()) == int(sc.max()) == g["pseudo"]["512"][qi]
            assert int(ids[-1]) == n - 1 and int(ids[n // 2]) == n // 2
        d.close()
