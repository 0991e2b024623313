"""CPU: the MSA definition on hand-worked rows (tests/msa_ref.py), cudasw4_amd/msa.py against that reference, the host
writer (swdrv_write_msa) against expected A3M / FASTA text, and the refusals of the new `align` flags — no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import msa_ref as M

N = M.NONE


def row(text):
    """'AAC-.': letters = codes by position in ARNDCQEGHILKMFPSTWYV, 'x' = 20, '-' = GAP, '.' = NONE"""
    table = {c: i for i, c in enumerate("ARNDCQEGHILKMFPSTWYV")}
    table.update({"x": 20, "-": M.GAP, ".": M.NONE})
    return np.array([table[c] for c in text], dtype=np.uint8)


def test_threshold_edge():
    """res = 50: 47 identities are 94 % (100 * 47 = 4700 >= 94 * 50), 46 are not"""
    master = row("." * 60)
    a = row("A" * 50 + "." * 10)
    for same, redundant in ((47, True), (46, False)):
        b = row("A" * same + "C" * (50 - same) + "-" * 4 + "x" * 3 + "." * 3)
        rows = np.stack([a, b, master])
        assert M.residues(rows).tolist() == [50, 50, 0]
        assert M.ident(a, b) == same
        keep, purged = M.greedy(rows, 94)
        assert keep.tolist() == [1, 0 if redundant else 1, 0] and purged == int(redundant)
        assert M.similar(same, 50, 94) == redundant
    # GAP, NONE and code 20 never count, on either side
    assert M.ident(row("-.xA"), row("-.xA")) == 1 and M.residues(np.stack([row("-.xA")])).tolist() == [1]


def test_fragment_asymmetry_and_master():
    full = row("ARNDCQEGHI")
    frag = row("...DCQE...")
    rows = np.stack([full, frag, row("." * 10)])
    assert M.greedy(rows, 90)[0].tolist() == [1, 0, 0] and M.greedy(rows, 90)[1] == 1
    rows = np.stack([frag, full, row("." * 10)])
    assert M.greedy(rows, 90)[0].tolist() == [1, 1, 0] and M.greedy(rows, 90)[1] == 0
    # the master goes first: a hit that repeats it is purged, a master without residues purges nothing
    rows = np.stack([full, frag, full])
    assert M.greedy(rows, 90) [0].tolist() == [0, 0, 1] and M.greedy(rows, 90)[1] == 2
    rows = np.stack([full, row("." * 10), row("x" * 10)])
    assert M.greedy(rows, 90)[0].tolist() == [1, 0, 0] and M.greedy(rows, 90)[1] == 0
    # P = 0: no filter
    rows = np.stack([full, full, row("-" * 10), full])
    assert M.greedy(rows, 0)[0].tolist() == [1, 1, 0, 1] and M.greedy(rows, 0)[1] == 0
    assert M.greedy(rows, 100)[0].tolist() == [0, 0, 0, 1] and M.greedy(rows, 100)[1] == 2


def test_non_transitive_chain():
    a = row("A" * 100)
    b = row("R" * 8 + "A" * 92)
    c = row("R" * 8 + "N" * 8 + "A" * 84)
    rows = np.stack([a, b, c, row("." * 100)])
    assert M.ident(a, b) == 92 and M.ident(b, c) == 92 and M.ident(a, c) == 84
    keep, purged = M.greedy(rows, 90)
    assert keep.tolist() == [1, 0, 1, 0] and purged == 1   # B goes, so C — redundant to B alone — stays
    assert M.pair_ident(rows)[2].tolist() == [84, 92, 0, 0] and (M.pair_ident(rows) == M.pair_ident_onehot(rows)).all()


def test_rows_from_a_hand_worked_cigar():
    # query positions 2..9 of 12: 3=, 2I, 1D, 2X (subject code 20 in it), then 1=
    rec = np.zeros(1, dtype=M.RECORD)
    rec[0]["q_begin"], rec[0]["q_end"], rec[0]["s_begin"], rec[0]["cigar_len"] = 2, 10, 1, 5
    subject = np.array([9, 0, 1, 2, 7, 20, 3, 4, 9], dtype=np.int8)
    words = M.cigar_words("3=2I1D2X1=")
    got = M.build_rows(np.arange(12, dtype=np.int8), 12, subject, np.array([0, 9], dtype=np.uint64), np.array([9], dtype=np.int32),
                       rec, words)
    assert got[0].tolist() == [N, N, 0, 1, 2, 21, 21, 20, 3, 4, N, N] and got[1].tolist() == list(range(12))
    rec[0]["status"] = 2
    assert (M.build_rows(None, 12, subject, [0, 9], [9], rec, words) == N).all()


def as_lists(case):
    n = case["n"]
    subjects = [case["chars"][int(case["offsets"][h]):int(case["offsets"][h]) + int(case["lengths"][h])] for h in range(n)]
    cigars = [case["cigar"][int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["cigar_len"])] for r in case["results"]]
    return subjects, cigars


@pytest.mark.parametrize("qlen,n", [(1, 3), (33, 40), (64, 65), (150, 90)])
def test_python_module_against_reference(qlen, n):
    from cudasw4_amd import msa
    assert (msa.GAP, msa.NONE) == (M.GAP, M.NONE)
    rng = np.random.default_rng(qlen * 7 + n)
    case = M.random_case(rng, qlen, n, max_runs=80 if qlen > 100 else 10, families=3, copy_rate=0.04)
    subjects, cigars = as_lists(case)
    include = (rng.random(n) < 0.8).astype(np.uint8)
    for inc, query in ((None, case["query"]), (include, case["query"]), (None, None)):
        want = M.msa_filter(query, qlen, case["chars"], case["offsets"], case["lengths"], case["results"], case["cigar"], inc, 94)
        rows = msa.rows_from_alignments(query if query is not None else qlen, subjects, case["results"], cigars, inc)
        assert rows.tobytes() == want["rows"].tobytes()
        idents = msa.pair_identity(rows)
        assert idents.tobytes() == want["pair_ident"].tobytes()
        for P in (0, 1, 60, 94, 100):
            keep, purged = msa.greedy_keep(rows, P, idents)
            wk, wp = M.greedy(want["rows"], P, want["pair_ident"])
            assert keep.tolist() == wk.tolist() and purged == wp, P
    strings = ["".join("%d%s" % (int(w) >> 4, {1: "I", 2: "D", 7: "=", 8: "X"}[int(w) & 15]) for w in c) or "*" for c in cigars]
    assert msa.rows_from_alignments(case["query"], subjects, case["results"], strings).tobytes() == \
        M.build_rows(case["query"], qlen, case["chars"], case["offsets"], case["lengths"], case["results"], case["cigar"]).tobytes()
    with pytest.raises(ValueError):
        msa.greedy_keep(rows, 101)


# ---- the writer (swdrv_write_msa; no GPU) -----------------------------------------------------------------------------------

def writer_case():
    """master of 14 residues; hit 0: a D run, an I run, an X letter in the subject, starts at query position 0; hit 1: an I
    run right behind a D run, starts at position 3 and ends before the master does; hit 2 has no trace; hit 3 is purged"""
    master = "MKTAYIAKQRQISF"
    subjects = ["ggMKTXYIcdAKRQISFtt", "wwAYLAKqqQRyy", "MKTAYIAKQRQISF", "MKTAYIAKQRQISF"]
    cigars = ["3=1X2=2D2=1I1=4=", "2=1X2=2D1I2=", "*", "14="]
    starts = [(0, 14, 2), (3, 11, 2), (0, 0, 0), (0, 14, 0)]
    res = np.zeros(4, dtype=M.RECORD)
    words, at = [], 0
    for h, (c, (qb, qe, sb)) in enumerate(zip(cigars, starts)):
        w = M.cigar_words(c) if c != "*" else np.zeros(0, dtype=np.uint32)
        res[h]["q_begin"], res[h]["q_end"], res[h]["s_begin"] = qb, qe, sb
        res[h]["status"] = 0 if len(w) else 2
        res[h]["cigar_len"], res[h]["cigar_offset"] = len(w), at
        words.append(w)
        at += len(w)
    cigar = np.concatenate(words + [np.zeros(1, dtype=np.uint32)])
    headers = ["sp|P1|ONE first hit", "two", "three no trace", "four purged"]
    keep = np.array([1, 1, 1, 0], dtype=np.uint8)
    return master, subjects, cigars, res, cigar, headers, keep


A3M = """>my query 1
MKTAYIAKQRQISF
>sp|P1|ONE first hit
MKTXYIcdAK-RQISF
>two
---AYLAKqq-QR---
"""
FASTA = A3M.replace("cd", "").replace("qq", "")


def columns(line):
    return sum(1 for c in line if c == "-" or c.isupper())


def test_writer_against_expected_text(tmp_path):
    from cudasw4_amd import driver, msa
    master, subjects, cigars, res, cigar, headers, keep = writer_case()
    for fmt, want in (("a3m", A3M), ("fasta", FASTA)):
        path = str(tmp_path / ("out." + fmt))
        driver.write_msa(path, fmt, master, "my query 1", headers, subjects, res, cigar, keep)
        text = open(path).read()
        assert text == want
        lines = text.splitlines()
        assert all(columns(l) == len(master) for l in lines[1::2]) and len(lines) == 6
        if fmt == "fasta":
            assert all(len(l) == len(master) for l in lines[1::2])
        # the Python formatter and the reference's line writer say the same
        assert msa.format_a3m(master, "my query 1", headers, subjects, res, cigars, keep, fmt) == want
        for h in (0, 1):
            w = cigar[int(res[h]["cigar_offset"]):int(res[h]["cigar_offset"]) + int(res[h]["cigar_len"])]
            assert M.a3m_line(len(master), subjects[h], res[h], w, fasta=fmt == "fasta") == lines[3 + 2 * h]
    # keep == None: every hit with a trace; the DB's gap character for its "other" code is written as X / x
    path = str(tmp_path / "all.a3m")
    subjects[3] = "MKT-YIAKQRQISF"
    driver.write_msa(path, "a3m", master, "q", headers, subjects, res, cigar, None)
    lines = open(path).read().splitlines()
    assert len(lines) == 8 and lines[6] == ">four purged" and lines[7] == "MKTXYIAKQRQISF"
    # the match columns of a line are the residues of the hit's row
    rows = M.build_rows(None, len(master), np.concatenate([driver.encode(s) for s in subjects]),
                        np.cumsum([0] + [len(s) for s in subjects]).astype(np.uint64), np.array([len(s) for s in subjects], np.int32),
                        res, cigar)
    upper = [c for c in lines[3] if c == "-" or c.isupper()]
    assert [("ARNDCQEGHILKMFPSTWYV" + "X")[v] if v <= 20 else "-" for v in rows[0]] == upper
    with pytest.raises(driver.DriverError):
        driver.write_msa(str(tmp_path / "no" / "dir.a3m"), "a3m", master, "q", headers, subjects, res, cigar, None)
    bad = res.copy()
    bad[3]["q_begin"] = 5     # 5 + 14 query columns: more than the master has
    with pytest.raises(driver.DriverError):
        driver.write_msa(path, "a3m", master, "q", headers, subjects, bad, cigar, None)


# ---- the command line: refusals before any device is opened -----------------------------------------------------------------

@pytest.mark.parametrize("args,message", [
    (["--outMsa", "P", "--msaMaxIdentity", "0"], "--msaMaxIdentity must be an integer in 1 .. 100"),
    (["--outMsa", "P", "--msaMaxIdentity", "101"], "--msaMaxIdentity must be an integer in 1 .. 100"),
    (["--outMsa", "P", "--msaMaxIdentity", "9x"], "--msaMaxIdentity must be an integer in 1 .. 100"),
    (["--outMsa", "P", "--msaFormat", "stockholm"], "--msaFormat must be a3m or fasta"),
    (["--msaFormat", "fasta"], "need --outMsa"),
    (["--msaMaxIdentity", "90"], "need --outMsa"),
    (["--purgeIdentity", "94"], "--purgeIdentity needs --iterations above 1 or --outPssm"),
    (["--purgeIdentity", "94.5", "--iterations", "2", "--inclusionScore", "50"], "--purgeIdentity must be an integer in 1 .. 100"),
    (["--purgeIdentity", "0", "--outPssm", "P", "--inclusionScore", "50"], "--purgeIdentity must be an integer in 1 .. 100"),
    (["--outMsa", "P", "--interactive"], "cannot be combined with --interactive"),
    (["--purgeIdentity", "94", "--iterations", "2", "--inclusionScore", "50", "--interactive"], "cannot be combined with --interactive"),
    (["--outMsa", "P", "--top", "0"], "--outMsa needs --top of at least 1"),
])
def test_align_refuses_before_any_device(args, message, tmp_path):
    from cudasw4_amd import driver
    q = tmp_path / "q.fa"
    q.write_text(">q\nMKTAYIAKQRQISF\n")
    # a DB prefix that does not exist: a run that got as far as opening it would say so instead
    r = subprocess.run([driver.ALIGN, "--query", str(q), "--db", str(tmp_path / "nodb")] + args, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and message in r.stderr, (r.returncode, r.stderr[-500:])
    assert "No GPU found" not in r.stderr and "nodb" not in r.stderr
    assert not list(tmp_path.glob("P.*"))


def test_help_and_option_dump(tmp_path):
    from cudasw4_amd import driver
    text = subprocess.run([driver.ALIGN, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--outMsa PREFIX", "--msaFormat a3m|fasta", "--msaMaxIdentity P", "--purgeIdentity P"):
        assert flag in text
    q = tmp_path / "q.fa"
    q.write_text(">q\nMKTAYIAKQRQISF\n")
    r = subprocess.run([driver.ALIGN, "--query", str(q), "--db", str(tmp_path / "nodb"), "--outMsa", "P", "--msaFormat", "xx",
                        "--msaMaxIdentity", "90"], capture_output=True, text=True, timeout=60)
    assert "outMsa: P\nmsaFormat: xx\nmsaMaxIdentity: 90\n" in r.stdout
    r = subprocess.run([driver.ALIGN, "--query", str(q), "--db", str(tmp_path / "nodb"), "--msaFormat", "a3m"], capture_output=True,
                       text=True, timeout=60)
    assert "outMsa" not in r.stdout and "purgeIdentity" not in r.stdout
