"""GPU: profile search — a position-specific scoring matrix (PSSM) as the query (include/cudasw4_amd_pssm.h), through the C
ABI (sw_set_query_pssm + the launcher-level scan) and, where marked D, through the C++ host driver (sw_scan_batch).

References: for a PSSM made of table rows (pssm.from_sequence) the letter query's own scores, bit for bit; for random PSSMs
the scalar reference tests/pssm_ref.c.  The runs under the library's test hooks are child processes (the hooks are read at
context creation), each under its own time limit:  python tests/test_gpu_pssm.py child  prints one JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = O.ROOT
pytestmark = pytest.mark.gpu


# ---- helpers -----------------------------------------------------------------------------------------------------------

def cabi_scan(searcher, query=None, pssm=None):
    """One scan of the Python launcher-level searcher (sw_scan_partition + sw_rescore_overflow per run) with a letter query
    or with a PSSM installed by sw_set_query_pssm in its place -> (all scores in DB order, overflow count)."""
    ctx = searcher.ctx
    if pssm is not None:
        ctx.set_query = lambda codes, stream=0: type(ctx).set_query_pssm(ctx, pssm, stream)
        try:
            res = searcher.scan(np.zeros(len(pssm), dtype=np.int8))
        finally:
            del ctx.set_query
        assert ctx.query_is_pssm()
    else:
        res = searcher.scan(query)
        assert not ctx.query_is_pssm()
    return searcher.all_scores(), res.num_overflows


def golden_db():
    _, qs = O.load_queries()
    order = np.argsort([len(q) for q in qs], kind="stable")
    chars, offsets, lengths = O.make_db([qs[i] for i in order])
    return qs, chars, offsets, lengths


def pick_queries(qs):
    """golden queries for 8- and 16-lane groups, one and many stripes, and the longest (4-lane groups: no golden query is
    short enough — the C-ABI test takes the first 90 residues of one)"""
    by_len = sorted(range(len(qs)), key=lambda i: len(qs[i]))
    def first(lo, hi):
        return next(i for i in by_len if lo <= len(qs[i]) <= hi)
    picks = [first(1, 160), first(161, 256), first(300, 760), first(800, 3000), by_len[-1]]
    assert len(set(picks)) == 5
    return picks


def synthetic_db(rng, pssms, n_bulk=260):
    """seeded subjects of length 0, 1, a bulk of 30..700, partition 34 (1300..3000) and one above 8000, with near-copies of
    every PSSM's consensus planted in subjects of all three classes"""
    from cudasw4_amd import pssm as P
    seqs = [np.zeros(0, np.int8), rng.integers(0, 20, 1).astype(np.int8)]
    seqs += [rng.integers(0, 21, int(n)).astype(np.int8) for n in rng.integers(30, 700, n_bulk)]
    seqs += [rng.integers(0, 20, int(n)).astype(np.int8) for n in rng.integers(1300, 3000, 24)]
    seqs += [rng.integers(0, 20, 8500).astype(np.int8), rng.integers(0, 20, 9100).astype(np.int8)]
    code = {c: i for i, c in enumerate(P.LETTERS)}
    for p in pssms:
        cons = np.array([code[c] for c in P.consensus_of(p)], dtype=np.int8)
        for ident in (1.0, 0.9, 0.7):
            copy = np.where(rng.random(len(cons)) < ident, cons, rng.integers(0, 20, len(cons))).astype(np.int8)
            if ident < 1.0:   # an indel in the middle
                copy = np.concatenate([copy[:len(copy) // 2], rng.integers(0, 20, 3).astype(np.int8), copy[len(copy) // 2 + 2:]])
            for flank in (10, 1400, 8200):
                seqs.append(np.concatenate([rng.integers(0, 20, flank).astype(np.int8), copy, rng.integers(0, 20, flank // 2 + 5).astype(np.int8)]))
    seqs.sort(key=len)
    return seqs, O.make_db(seqs)


def random_pssm(rng, n, lo=-12, hi=14, extremes=False):
    p = rng.integers(lo, hi + 1, (n, 21)).astype(np.int8)
    if extremes:
        rows = rng.choice(n, max(2, n // 10), replace=False)
        p[rows[::2], rng.integers(0, 20, len(rows[::2]))] = 127
        p[rows[1::2], rng.integers(0, 20, len(rows[1::2]))] = -128
    p[:, 20] = -1 - rng.integers(0, 5, n)
    return p


# ---- a. equivalence with the letter query --------------------------------------------------------------------------

def test_pssm_of_table_rows_equals_the_letter_query_cabi(monkeypatch):
    import gpu_util as G
    from cudasw4_amd import pssm as P
    torch, capi, search = G.gpu_modules()
    qs, chars, offsets, lengths = golden_db()
    db = search.DeviceDB.from_arrays(chars, offsets, lengths, device=0)
    m = O.blosum21(62)
    overflows = 0
    lanes_seen = set()
    monkeypatch.setenv("CUDASW4_AMD_LANES4_MAX_Q", "96")   # (read at context creation: 4-lane groups whatever the DB's size)
    queries = [qs[qi] for qi in pick_queries(qs)] + [qs[0][:90]]
    for name, kt in G.kinds_configs(search, capi).items():
        s = search.Searcher(device=0, num_top=0, matrix=m, kernel_types=kt)
        s.set_database(db)
        for q in queries:
            want, wovf = cabi_scan(s, query=q)
            plan_q = s.ctx.plan_launch(kt.single_pass, 10, 1000, 300)
            got, govf = cabi_scan(s, pssm=P.from_sequence(q, m))
            assert s.ctx.plan_launch(kt.single_pass, 10, 1000, 300) == plan_q     # the planning calls describe the PSSM query alike
            lanes_seen.add(plan_q[3])
            assert got.tolist() == want.tolist(), (name, len(q))
            assert govf == wovf, (name, len(q), govf, wovf)
            overflows += wovf
    assert {4, 8, 16} <= lanes_seen, lanes_seen
    assert overflows > 0   # the packed configurations met their limits on the way


@pytest.mark.parametrize("kinds", [(0, 0, 3, 3), (1, 1, 2, 2)])
def test_pssm_of_table_rows_equals_the_letter_query_driver(kinds):
    from cudasw4_amd import driver, pssm as P
    import torch
    assert torch.cuda.is_available()
    qs, chars, offsets, lengths = golden_db()
    _, letters = O.read_fasta(os.path.join(O.GOLDEN_DIR, "allqueries.fasta"))
    d = driver.Driver(devices=[0], num_top=10, kinds=kinds)
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    m = driver.matrix(62)
    for qi in pick_queries(qs):
        a = d.scan(letters[qi])
        ia, sa = d.all_scores()
        b = d.scan_pssm(P.from_sequence(driver.encode(letters[qi]), m))
        ib, sb = d.all_scores()
        assert sa[np.argsort(ia)].tolist() == sb[np.argsort(ib)].tolist(), qi
        assert a["scores"].tolist() == b["scores"].tolist() and a["ids"].tolist() == b["ids"].tolist()
        assert a["num_overflows"] == b["num_overflows"] and a["num_rescored"] == b["num_rescored"], qi
    d.close()


def test_pssm_of_a_25_letter_table_equals_the_letter_query():
    from cudasw4_amd import driver, pssm as P
    qs, chars, offsets, lengths = golden_db()
    _, letters = O.read_fasta(os.path.join(O.GOLDEN_DIR, "allqueries.fasta"))
    q = bytearray(letters[pick_queries(qs)[2]])
    for at, ch in ((3, b"B"), (40, b"Z"), (41, b"X"), (100, b"B"), (101, b"*"), (150, b"J")):
        q[at:at + 1] = ch
    q = bytes(q)
    d = driver.Driver(devices=[0], num_top=10, matrix=6225, kinds=(0, 0, 3, 3))
    d.db_from_arrays(chars, offsets, lengths)
    a = d.scan(q)
    ia, sa = d.all_scores()
    p = P.from_sequence(driver.encode25(q), driver.matrix25(62))
    assert p.tolist() == P.from_sequence(q, driver.matrix25(62)).tolist()
    b = d.scan_pssm(p)
    ib, sb = d.all_scores()
    assert sa[np.argsort(ia)].tolist() == sb[np.argsort(ib)].tolist()
    assert a["scores"].tolist() == b["scores"].tolist() and a["ids"].tolist() == b["ids"].tolist()
    d.close()


# ---- b. random PSSMs against the scalar reference, under every hook ----------------------------------------------------

def child_main():
    """one process = one setting of the hooks: random PSSMs on the synthetic DB through the C ABI and the driver"""
    import gpu_util as G
    import pssm_ref as PR
    from cudasw4_amd import driver
    torch, capi, search = G.gpu_modules()
    rng = np.random.default_rng(20260)
    pssms = [random_pssm(rng, 61), random_pssm(rng, 300), random_pssm(rng, 230, extremes=True), random_pssm(rng, 2200)]
    seqs, (chars, offsets, lengths) = synthetic_db(rng, pssms)
    db = search.DeviceDB.from_arrays(chars, offsets, lengths, device=0)
    out = {"subjects": len(seqs), "longest": int(lengths.max()), "mismatch": [], "overflows": {}, "best": []}
    refs = [PR.scan(p, chars, offsets, lengths) for p in pssms]
    out["best"] = [int(r.max()) for r in refs]
    for name, kt in G.kinds_configs(search, capi).items():
        s = search.Searcher(device=0, num_top=0, kernel_types=kt)   # no sw_set_matrix: a PSSM query needs none
        s.set_database(db)
        for pi, p in enumerate(pssms):
            got, novf = cabi_scan(s, pssm=p)
            if got.tolist() != refs[pi].tolist():
                bad = np.nonzero(got != refs[pi])[0]
                out["mismatch"].append(["cabi", name, pi, int(len(bad)), int(bad[0]), int(got[bad[0]]), int(refs[pi][bad[0]]), int(lengths[bad[0]])])
            out["overflows"]["cabi/%s/%d" % (name, pi)] = int(novf)
    for kinds in ((0, 0, 3, 3), (1, 1, 2, 2), (3, 0, 3, 3)):
        d = driver.Driver(devices=[0], num_top=10, kinds=kinds)
        d.db_from_arrays(chars, offsets, lengths)
        d.upload()
        for pi, p in enumerate(pssms):
            r = d.scan_pssm(p)
            ids, sc = d.all_scores()
            got = sc[np.argsort(ids)]
            if got.tolist() != refs[pi].tolist():
                bad = np.nonzero(got != refs[pi])[0]
                out["mismatch"].append(["driver", list(kinds), pi, int(len(bad)), int(bad[0]), int(got[bad[0]]), int(refs[pi][bad[0]]), int(lengths[bad[0]])])
            es, ei = O.topk(refs[pi], 10)
            if r["scores"].tolist() != es.tolist() or r["ids"].tolist() != ei.tolist():
                out["mismatch"].append(["driver-top", list(kinds), pi])
            out["overflows"]["driver/%s/%d" % ("".join(map(str, kinds)), pi)] = int(r["num_overflows"])
        out["pipelines"] = out.get("pipelines", 0) + int(d.pipeline_launches())
        w = d.window_stats()
        out["window_launches"] = out.get("window_launches", 0) + int(w[0])
        out["windows"] = out.get("windows", 0) + int(w[1])
        d.close()
    print("PSSM_CHILD " + json.dumps(out))


HOOKS = [{}, {"CUDASW4_AMD_PIPELINES": "always"}, {"CUDASW4_AMD_WINDOWS": "always"}, {"CUDASW4_AMD_STREAM": "1"},
         {"CUDASW4_AMD_NO_OFFS": "1"}, {"CUDASW4_AMD_I32_NATIVE": "1"}]


@pytest.mark.parametrize("hook", HOOKS, ids=lambda h: "+".join("%s=%s" % kv for kv in h.items()) or "default")
def test_random_pssms_equal_the_scalar_reference(hook):
    env = dict(os.environ, **hook)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True,
                         env=env, cwd=ROOT)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    line = [l for l in run.stdout.splitlines() if l.startswith("PSSM_CHILD ")][-1]
    out = json.loads(line[len("PSSM_CHILD "):])
    print(hook, out)
    assert out["mismatch"] == [], out["mismatch"]
    assert out["longest"] > 8000 and out["best"][1] >= 2048 and out["best"][3] >= 25000, out["best"]
    # the re-score paths ran: the planted copies pass the fp16 limit with the 300-position PSSM, the int16 limit with the long one
    ov = out["overflows"]
    assert ov["driver/0033/1"] > 0 and ov["driver/1122/3"] > 0, ov
    if hook.get("CUDASW4_AMD_NO_OFFS") == "1":
        # this hook sends every packed launch of the launcher-level C ABI to its 32-bit kind (include/cudasw4_amd.h: nothing to
        # flag, nothing to re-score there); the driver counts exact scores at or above the limit either way (asserted above)
        assert ov["cabi/half2+float/1"] == 0 and ov["cabi/dpxs16+dpxs32/3"] == 0, ov
    else:
        assert ov["cabi/half2+float/1"] > 0 and ov["cabi/dpxs16+dpxs32/3"] > 0, ov
    if hook.get("CUDASW4_AMD_PIPELINES") == "always":
        assert out["pipelines"] > 0, out
    if hook.get("CUDASW4_AMD_WINDOWS") == "always":
        assert out["window_launches"] > 0 and out["windows"] > 0, out


# ---- c. one context, queries of both forms in turn -------------------------------------------------------------------

def test_switching_between_letters_and_pssms_in_one_context():
    import gpu_util as G
    import pssm_ref as PR
    torch, capi, search = G.gpu_modules()
    qs, chars, offsets, lengths = golden_db()
    db = search.DeviceDB.from_arrays(chars, offsets, lengths, device=0)
    rng = np.random.default_rng(3)
    q = qs[pick_queries(qs)[1]]
    p1 = random_pssm(rng, len(q))
    p2 = random_pssm(rng, len(q), lo=-3, hi=120)          # same length, a much larger top entry: the bounds must follow
    for name, kt in G.kinds_configs(search, capi).items():
        s = search.Searcher(device=0, num_top=0, matrix=O.blosum21(62), kernel_types=kt)
        s.set_database(db)
        want_q = O.scan(q, chars, offsets, lengths, simd=True)
        assert cabi_scan(s, query=q)[0].tolist() == want_q.tolist(), name
        assert cabi_scan(s, pssm=p1)[0].tolist() == PR.scan(p1, chars, offsets, lengths).tolist(), name
        assert cabi_scan(s, pssm=p2)[0].tolist() == PR.scan(p2, chars, offsets, lengths).tolist(), name
        assert cabi_scan(s, query=q)[0].tolist() == want_q.tolist(), name
        assert cabi_scan(s, pssm=p1)[0].tolist() == PR.scan(p1, chars, offsets, lengths).tolist(), name


# ---- d. driver: shards, streaming, two queries in flight --------------------------------------------------------------

@pytest.mark.parametrize("shards", [1, 8])
@pytest.mark.parametrize("streamed", [False, True])
def test_driver_top10_on_shards_resident_and_streamed(shards, streamed):
    import pssm_ref as PR
    from cudasw4_amd import driver
    rng = np.random.default_rng(77)
    pssms = [random_pssm(rng, 120), random_pssm(rng, 900)]
    seqs, (chars, offsets, lengths) = synthetic_db(rng, pssms, n_bulk=400)
    # (a limit of one byte leaves no shard anything to keep in device memory, however small the shard: every batch is streamed)
    kw = dict(max_gpu_mem=1, max_batch_bytes=32 << 10) if streamed else {}
    d = driver.Driver(devices=[0] * shards, num_top=10, kinds=(0, 0, 3, 3), **kw)
    d.db_from_arrays(chars, offsets, lengths)
    if streamed:
        infos = [d.shard_info(g) for g in range(shards)]
        assert all(not i["resident"] and i["cached_chars"] == 0 for i in infos), infos
    for p in pssms:
        r = d.scan_pssm(p)
        es, ei = O.topk(PR.scan(p, chars, offsets, lengths), 10)
        assert r["scores"].tolist() == es.tolist() and r["ids"].tolist() == ei.tolist(), (shards, streamed, len(p))
    if streamed:
        assert d.streamed_bytes() >= len(pssms) * sum(i["chars"] for i in infos)   # every query moved every shard's chars
    d.close()


def test_pssm_query_in_flight_beside_a_letter_query():
    import pssm_ref as PR
    from cudasw4_amd import driver
    qs, chars, offsets, lengths = golden_db()
    _, letters = O.read_fasta(os.path.join(O.GOLDEN_DIR, "allqueries.fasta"))
    rng = np.random.default_rng(9)
    p = random_pssm(rng, 333)
    qi = pick_queries(qs)[2]
    d = driver.Driver(devices=[0], num_top=10, kinds=(0, 0, 3, 3))
    d.db_from_arrays(chars, offsets, lengths)
    d.upload()
    want_q = O.topk(O.scan(qs[qi], chars, offsets, lengths, simd=True), 10)
    want_p = O.topk(PR.scan(p, chars, offsets, lengths), 10)
    for first_pssm in (False, True):
        if first_pssm:
            d.submit_pssm(p)
            d.submit(letters[qi])
        else:
            d.submit(letters[qi])
            d.submit_pssm(p)
        a, b = d.collect(), d.collect()
        rq, rp = (b, a) if first_pssm else (a, b)
        assert rq["scores"].tolist() == want_q[0].tolist() and rq["ids"].tolist() == want_q[1].tolist()
        assert rp["scores"].tolist() == want_p[0].tolist() and rp["ids"].tolist() == want_p[1].tolist()
    d.close()


# ---- e. the command line ---------------------------------------------------------------------------------------------

def test_align_pssm_option(tmp_path):
    import pssm_ref as PR
    from cudasw4_amd import pssm as P
    qs, chars, offsets, lengths = golden_db()
    rng = np.random.default_rng(31)
    p = random_pssm(rng, 210)
    p[:, 20] = P.OTHER_SCORE
    f = str(tmp_path / "fam.pssm")
    P.write_ascii(f, p, percentages=True, footer=True)
    align = os.path.join(ROOT, "cudasw4_amd", "lib", "align")
    prefix = os.path.join(O.GOLDEN_DIR, "allqueries_db", "aq")
    fasta = os.path.join(O.GOLDEN_DIR, "allqueries.fasta")

    def rows(args):
        of = str(tmp_path / "out.tsv")
        run = subprocess.run(["timeout", "-k", "10", "240", align] + args + ["--db", prefix, "--top", "10", "--tsv", "--of", of], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        lines = open(of).read().splitlines()
        return [l.split("\t") for l in lines[1:]]

    # the DB on disk in its own order: reference list by the lengths / ids the tool reports
    from cudasw4_amd import driver
    d = driver.Driver(devices=[0], num_top=10)
    d.open_db(prefix)
    want = d.scan_pssm(p)
    d.close()
    assert sorted(want["scores"].tolist(), reverse=True) == O.topk(PR.scan(p, chars, offsets, lengths), 10)[0].tolist()
    got = rows(["--pssm", f])
    assert len(got) == 10 and all(r[0] == "0" and r[1] == "210" and r[2] == "fam.pssm" for r in got)
    assert [int(r[4]) for r in got] == want["scores"].tolist() and [int(r[7]) for r in got] == want["ids"].tolist()
    # twice, and mixed with a query file: input order is kept
    mixed = rows(["--pssm", f, "--query", fasta, "--pssm", f])
    nq = len(qs)
    assert len(mixed) == 10 * (nq + 2)
    assert [r[2] for r in mixed[:10]] == ["fam.pssm"] * 10 and [r[2] for r in mixed[-10:]] == ["fam.pssm"] * 10
    assert all(r[2] != "fam.pssm" for r in mixed[10:-10])
    assert [r[3:] for r in mixed[:10]] == [r[3:] for r in got] == [r[3:] for r in mixed[-10:]]
    plain = rows(["--query", fasta])
    assert [r for r in mixed[10:-10]] == plain


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "child":
    sys.path.insert(0, ROOT)
    child_main()
