"""GPU: the C++ host driver (sw_scan_batch behind driver.Driver) under non-default substitution matrices and gap scores.

The engine's decisions that depend on the scoring — the window span (include/cudasw4_amd_engine.h: sw_window_overlap), the
pipelines (gop <= gex), the packed kinds' fallback to 32 bits (fp16 with |gex| > 12), the frame period behind the early
overflow flags, the re-score service — are reached here through the driver the way `align --mat ... --gop ... --gex ...`
reaches them: one synthetic DB, every score of every subject, the top-10, the overflow statistic, hit alignments and PSSM
queries against the CPU references, for every scoring of SCORINGS under every engine mode.

The builders (inputs(), scoring(), oracle_scan(), ...) use no GPU: tests/test_driver_scoring_inputs_cpu.py asserts with the
oracle alone that the inputs reach what the tests below claim."""
import functools
import os
import subprocess

import numpy as np
import pytest

import align_ref as A
import oracle_lib as O

pytestmark = pytest.mark.gpu

FASTA = os.path.join(O.GOLDEN_DIR, "allqueries.fasta")

# name -> (matrix, gop, gex); None: that matrix's default gap scores, read from the product (default_gaps)
SCORINGS = {
    "blosum45": (45, None, None),
    "blosum50": (50, None, None),
    "blosum80": (80, None, None),
    "b62_5_5": (62, -5, -5),
    "b62_2_5": (62, -2, -5),        # gop > gex: no pipelines
    "b62_20_0": (62, -20, 0),       # a gap column may cost nothing: no window span
    "b62_40_13": (62, -40, -13),    # fp16 launches fall back to fp32 (|gex| > 12)
    "b6225_13_2": (6225, -13, -2),  # the 25-letter table
}
NAMES = list(SCORINGS)
KINDS = [(0, 0, 3, 3), (1, 1, 2, 2)]
MODES = {"asis": {}, "windows": {"CUDASW4_AMD_WINDOWS": "always"}, "pipelines": {"CUDASW4_AMD_PIPELINES": "always"},
         "service": {"CUDASW4_AMD_RESCORE_SERVICE": "1"}}
ENGINE_VARS = ["CUDASW4_AMD_WINDOWS", "CUDASW4_AMD_PIPELINES", "CUDASW4_AMD_RESCORE_SERVICE"]


# ---- the scorings ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def default_gaps(mat):
    """the product's default gap scores of a matrix: `align` prints its options before it opens a device or any input"""
    from cudasw4_amd import driver
    p = subprocess.run(["timeout", "-k", "10", "60", driver.ALIGN, "--mat", "blosum%d" % mat, "--query", FASTA, "--db",
                        os.path.join(O.GOLDEN_DIR, "no_such_db")], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    got = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(": ")
        if k in ("gop", "gex", "blosum"):
            got[k] = v
    assert got.get("blosum") == "blosum%d" % mat, p.stdout[-500:]
    return int(got["gop"]), int(got["gex"])


def scoring(name):
    mat, gop, gex = SCORINGS[name]
    if gop is None:
        gop, gex = default_gaps(mat)
    return mat, gop, gex


@functools.lru_cache(maxsize=None)
def oracle_matrix(mat):
    """rows = query codes, 21 columns = dbdata subject codes (a 25-letter table scores subject code 20 with its X column)"""
    if mat > 100:
        from cudasw4_amd import driver
        m = driver.matrix25(mat // 100).reshape(25, 25)[:, list(range(20)) + [23]]
        return np.ascontiguousarray(m)
    return O.blosum21(mat).reshape(21, 21)


def window_stride(qlen, m, gop, gex):
    """(C, W4) of the documented span formula: an alignment with a positive score spans fewer than W = Q + Q * max(M) /
    min(|gop|, |gex|) + 1 subject columns; windows start every C = max(W rounded up to 4, 2048) columns and overlap by W4.
    None: a gap column may cost nothing, there is no span."""
    cost = min(-gop, -gex)
    if cost <= 0:
        return None
    w4 = (qlen + qlen * int(np.max(m)) // cost + 1 + 3) // 4 * 4
    return max(w4, 2048), w4


# ---- the inputs --------------------------------------------------------------------------------------------------------

def mutated(rng, codes, identity, indel):
    s = np.where(rng.random(len(codes)) < identity, codes, rng.integers(0, 20, len(codes))).astype(np.int8)
    if indel and len(s) >= 30:
        a, b = len(s) // 3, 2 * len(s) // 3
        s = np.concatenate([s[:a], s[a + 3:b], rng.integers(0, 20, 5).astype(np.int8), s[b:]])
    return s


@functools.lru_cache(maxsize=None)
def inputs():
    """-> dict: queries (letters, ascending length; the last one is for the int16 configuration only), seqs (codes, sorted by
    length), db = (chars, offsets, lengths), pssms.  Seeded; the same arrays for every test of the session."""
    import test_gpu_pssm as TP
    from cudasw4_amd import pssm as P
    rng = np.random.default_rng(20261018)
    _, gold = O.read_fasta(FASTA)
    queries = [gold[5][:48], gold[0], gold[3][:300], gold[9], gold[11], gold[19]]
    assert [len(q) for q in queries] == [48, 144, 300, 1000, 2005, 5478]
    qcodes = [O.encode(q) for q in queries]
    pssms = [TP.random_pssm(rng, 120), TP.random_pssm(rng, 900, extremes=True)]

    def background(n, other=False):
        s = rng.integers(0, 20, int(n)).astype(np.int8)
        if other:
            s[rng.random(len(s)) < 0.02] = 20
        return s

    bulk = [background(n, other=(i % 7 == 0)) for i, n in enumerate(rng.integers(20, 1201, 600))]
    bulk += [background(n) for n in (1100, 1150, 1180, 1200) * 3]          # room for the longer plants
    p34 = [background(n) for n in rng.integers(1300, 5400, 24)] + [background(n) for n in (5600, 5700, 5750, 5800, 5850, 5900, 5950, 6000)]
    giants = [background(n) for n in (8100, 12000, 20000, 35000)]

    # window-boundary plants of the two shortest queries: the query across the first boundary, the query with a 150-residue
    # insertion across the second one, for the boundaries of every scoring (giant 0: 48 residues, giant 1: 144 residues)
    reserved = 0
    for gi, q in enumerate(qcodes[:2]):
        spots = set()
        for name in NAMES:
            mat, gop, gex = scoring(name)
            cw = window_stride(len(q), oracle_matrix(mat), gop, gex)
            if cw:
                spots.add(cw[0])
        gapped = np.concatenate([q[:len(q) // 2], rng.integers(0, 20, 150).astype(np.int8), q[len(q) // 2:]])
        taken = []
        for C in sorted(spots):
            for at, piece in ((C - len(q) // 2, q), (2 * C - len(q) // 2 - 40, gapped)):
                assert at + len(piece) < len(giants[gi]) and all(at >= e or at + len(piece) <= b for b, e in taken), (gi, C, at)
                giants[gi][at:at + len(piece)] = piece
                taken.append((at, at + len(piece)))
                reserved = max(reserved, at + len(piece))

    # relatives of every query at graded identity, in the bulk, in partition 34 and in the giants (one plant per bulk /
    # partition-34 subject; a query longer than its subject is planted as a piece of it)
    free_bulk = sorted(range(len(bulk)), key=lambda i: len(bulk[i]))
    free_p34 = sorted(range(len(p34)), key=lambda i: len(p34[i]))
    cursor = [reserved + 100] * len(giants)

    def plant(pool, free, rel):
        fits = [i for i in free if len(pool[i]) >= len(rel) + 8]
        i = fits[int(rng.integers(0, min(len(fits), 6)))] if fits else free[-1]
        free.remove(i)
        piece = rel[:len(pool[i]) - 8]
        at = int(rng.integers(0, len(pool[i]) - len(piece) + 1))
        pool[i][at:at + len(piece)] = piece

    for qi, q in enumerate(qcodes):
        for ident, indel in ((1.0, True), (0.9, False), (0.9, True), (0.7, False), (0.7, True), (0.5, False)):
            plant(bulk, free_bulk, mutated(rng, q, ident, indel))
        for ident, indel in ((1.0, True), (0.9, False), (0.7, True), (0.5, False)):
            plant(p34, free_p34, mutated(rng, q, ident, indel))
        for k, (ident, indel) in enumerate(((1.0, False), (0.9, True), (0.7, False), (0.5, False))):
            if qi < 2 and ident == 1.0:
                continue        # (the exact copies of the two shortest queries are the window plants)
            g = (qi + k) % len(giants)
            rel = mutated(rng, q, ident, indel)
            if cursor[g] + len(rel) + 50 < len(giants[g]):
                giants[g][cursor[g]:cursor[g] + len(rel)] = rel
                cursor[g] += len(rel) + 50
    # the int16 configuration's long query: pieces of it at the same identities, so that partition 34 has scores on both
    # sides of 12 500 as well as the copy beyond 25 000
    big = qcodes[-1]
    for lo, hi, ident in ((0, 2800, 1.0), (1500, 4700, 0.9), (800, 5000, 0.7), (2000, 5400, 0.9)):
        plant(p34, free_p34, mutated(rng, big[lo:hi], ident, False))
    # relatives of the PSSMs' consensus
    code = {c: i for i, c in enumerate(P.LETTERS)}
    for p in pssms:
        cons = np.array([code[c] for c in P.consensus_of(p)], dtype=np.int8)
        for ident, indel in ((1.0, False), (0.9, True), (0.7, False)):
            plant(bulk, free_bulk, mutated(rng, cons, ident, indel))
        plant(p34, free_p34, mutated(rng, cons, 0.9, True))

    seqs = [np.zeros(0, np.int8), background(1)] + bulk + p34 + giants
    seqs.sort(key=len)
    return {"queries": queries, "seqs": seqs, "db": O.make_db(seqs), "pssms": pssms}


def query_letters(name, qi):
    """the query as the driver takes it: for the 25-letter table some residues become B, J, Z, X and * (distinct rows there)"""
    q = inputs()["queries"][qi]
    if scoring(name)[0] > 100:
        b = bytearray(q)
        for k, pos in enumerate(range(5, len(b), 37)):
            b[pos] = b"BJZX*"[k % 5]
        q = bytes(b)
    return q


def query_codes(name, qi):
    q = query_letters(name, qi)
    if scoring(name)[0] > 100:
        from cudasw4_amd import driver
        return driver.encode25(q)
    return O.encode(q)


@functools.lru_cache(maxsize=None)
def oracle_scan(name, qi):
    mat, gop, gex = scoring(name)
    chars, offsets, lengths = inputs()["db"]
    # (the lock-step int16 oracle indexes 21 query rows: the 25-letter table takes the scalar one)
    out = O.scan(query_codes(name, qi), chars, offsets, lengths, m21=oracle_matrix(mat), gop=gop, gex=gex, simd=mat < 100)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_scan_pssm(name, pi):
    import pssm_ref as PR
    _, gop, gex = scoring(name)
    out = PR.scan(inputs()["pssms"][pi], *inputs()["db"], gop=gop, gex=gex)
    out.setflags(write=False)
    return out


def packed_limits(kinds):
    """per subject: the limit of the packed kind its partition runs in (2^30: a 32-bit kind, nothing overflows)"""
    lens = inputs()["db"][2]
    kind = np.where(lens <= 1280, kinds[0], np.where(lens <= 8000, kinds[1], kinds[2]))
    return np.where(kind == 0, 2048, np.where(kind == 1, 25000, 2**30))


def queries_of(kinds):
    return range(6 if kinds[0] == 1 else 5)


# ---- the driver --------------------------------------------------------------------------------------------------------

def make_driver(name, kinds, monkeypatch, env=None, devices=(0,), num_top=10, upload=True, **kw):
    from cudasw4_amd import driver
    for v in ENGINE_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)     # (read when the driver creates its engines)
    mat, gop, gex = scoring(name)
    d = driver.Driver(devices=list(devices), num_top=num_top, matrix=mat, gop=gop, gex=gex, kinds=kinds, **kw)
    d.db_from_arrays(*inputs()["db"])
    if upload:
        d.upload()
    return d


def scores_by_id(d):
    ids, sc = d.all_scores()
    got = np.full(len(sc), -99, dtype=np.int32)
    got[ids] = sc
    return got


def check_scan(d, r, expect, where):
    got = scores_by_id(d)
    bad = np.nonzero(got != expect)[0]
    assert len(bad) == 0, (where, len(bad), bad[:5], got[bad[:5]], expect[bad[:5]], inputs()["db"][2][bad[:5]])
    es, ei = O.topk(expect, 10)
    assert r["scores"].tolist() == es.tolist() and r["ids"].tolist() == ei.tolist(), where


# a. every score, the top-10 and the statistics; b. which engine path ran

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kinds", KINDS, ids=["fp16", "int16"])
@pytest.mark.parametrize("name", NAMES)
def test_scores_top10_statistics_and_engine_paths(name, kinds, mode, monkeypatch):
    mat, gop, gex = scoring(name)
    d = make_driver(name, kinds, monkeypatch, MODES[mode])
    limits = packed_limits(kinds)
    for qi in queries_of(kinds):
        expect = oracle_scan(name, qi)
        r = d.scan(query_letters(name, qi))
        print(name, kinds, mode, "query", qi, "overflows", r["num_overflows"], "rescored", r["num_rescored"], "top", int(r["scores"][0]))
        check_scan(d, r, expect, (name, kinds, mode, qi))
        want = int((expect >= limits).sum())
        assert r["num_overflows"] == want, (name, kinds, mode, qi, r["num_overflows"], want)
        assert r["num_rescored"] >= r["num_overflows"], (name, kinds, mode, qi, r["num_rescored"], want)
    launches, nwin = d.window_stats()
    pipes, services, handshake = d.pipeline_launches(), d.service_launches(), d.handshake_active()
    d.close()
    print(name, kinds, mode, "windows", (launches, nwin), "pipelines", pipes, "service", services)
    longest = int(inputs()["db"][2][-1])
    if min(-gop, -gex) == 0:
        assert (launches, nwin) == (0, 0)
    elif mode == "windows":
        # the two shortest queries' span cuts the longest giant whatever the scoring of this grid
        C, W4 = window_stride(48, oracle_matrix(mat), gop, gex)
        assert longest > C + W4 and launches > 0 and nwin > launches
    if gop > gex:
        assert pipes == 0
    elif mode == "pipelines":
        assert pipes > 0
    if mode == "service" and handshake:
        # fp16 with |gex| > 12: the bulk run is served by fp32, there is no list a service could take from
        fallback = kinds[0] == 0 and -gex > 12
        assert (services == 0) if fallback else (services > 0)


# c. hit alignment under the driver's scoring

@pytest.mark.parametrize("name", NAMES)
def test_align_hits_use_the_drivers_scoring(name, monkeypatch):
    mat, gop, gex = scoring(name)
    m = oracle_matrix(mat)
    seqs = inputs()["seqs"]
    d = make_driver(name, (0, 0, 3, 3), monkeypatch)
    for qi in (1, 3):
        q = query_letters(name, qi)
        codes = query_codes(name, qi)
        r = d.scan(q)
        check_scan(d, r, oracle_scan(name, qi), (name, qi))
        res, cigars = d.align_hits(q, r)
        assert len(res) == 10
        for k in range(10):
            s = seqs[int(r["ids"][k])]
            want, wcig = A.align(codes, s, m, gop, gex)
            assert {f: int(res[k][f]) for f in A.FIELDS} == want, (name, qi, k)
            assert cigars[k] == (A.cigar_string(wcig) or "*"), (name, qi, k)
            assert want["status"] == A.OK and A.rescore(codes, s, m, gop, gex, want, wcig) == want["score"] == int(r["scores"][k])
    d.close()


# d. PSSM queries under the driver's gap scores

@pytest.mark.parametrize("name", NAMES)
def test_pssm_queries_use_the_drivers_gap_scores(name, monkeypatch):
    import pssm_align_ref as PA
    _, gop, gex = scoring(name)
    seqs = inputs()["seqs"]
    d = make_driver(name, (0, 0, 3, 3), monkeypatch)
    for pi, p in enumerate(inputs()["pssms"]):
        r = d.scan_pssm(p)
        check_scan(d, r, oracle_scan_pssm(name, pi), (name, "pssm", pi))
        res, cigars = d.align_hits_pssm(p, r)
        for k in range(10):
            want, wcig = PA.align(p, seqs[int(r["ids"][k])], None, gop, gex)
            assert {f: int(res[k][f]) for f in A.FIELDS} == want, (name, pi, k)
            assert cigars[k] == (A.cigar_string(wcig) or "*"), (name, pi, k)
    d.close()


# e. shards and streaming

@pytest.mark.parametrize("streamed", [False, True], ids=["resident", "streamed"])
def test_three_shards_resident_and_streamed(streamed, monkeypatch):
    name = "blosum45"
    kw = dict(max_gpu_mem=1, max_batch_bytes=32 << 10) if streamed else {}
    d = make_driver(name, (0, 0, 3, 3), monkeypatch, devices=[0] * 3, upload=not streamed, **kw)
    assert d.num_gpus() == 3 and all(d.shard_info(g)["resident"] == (not streamed) for g in range(3))
    limits = packed_limits((0, 0, 3, 3))
    for qi in range(5):
        expect = oracle_scan(name, qi)
        r = d.scan(query_letters(name, qi))
        check_scan(d, r, expect, (name, streamed, qi))
        assert r["num_overflows"] == int((expect >= limits).sum()) and r["num_rescored"] >= r["num_overflows"]
    d.close()


# f. two queries in flight

@pytest.mark.parametrize("kinds", KINDS, ids=["fp16", "int16"])
def test_two_queries_in_flight(kinds, monkeypatch):
    name = "b62_5_5"
    d = make_driver(name, kinds, monkeypatch)
    qs = [query_letters(name, qi) for qi in queries_of(kinds)]
    single = []
    for qi, q in enumerate(qs):
        r = d.scan(q)
        check_scan(d, r, oracle_scan(name, qi), (name, kinds, qi))
        single.append((r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"]))
    many = d.scan_many(qs + qs)
    assert [(r["scores"].tolist(), r["ids"].tolist(), r["num_overflows"]) for r in many] == single + single
    d.close()
