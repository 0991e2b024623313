"""CPU: building a PSSM from aligned hits — the host conversion (swdrv_pssm_from_counts / pssm.from_counts) against the scalar
reference tests/pssm_build_ref.c and against values worked out by hand, the C++ ASCII writer, and the new flags of `align`.
No GPU involved."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pssm_build_ref as R

ROOT = O.ROOT
LIBDIR = os.path.join(ROOT, "cudasw4_amd", "lib")
ALIGN = os.path.join(LIBDIR, "align")
MATRICES = [45, 50, 62, 80]
LAMBDA = {45: 0.229091, 50: 0.231827, 62: 0.317606, 80: 0.342969}
F = 1 << 32


def master_only(codes):
    """counts / weighted counts of a master without hits, from the reference"""
    z = np.zeros(0, dtype=R.RECORD)
    return R.accumulate(codes, len(codes), np.zeros(4, np.int8), np.zeros(1, np.uint64), np.zeros(0, np.int32), z,
                        np.zeros(1, np.uint32))


@pytest.mark.parametrize("which", MATRICES)
def test_lambda_check_values(which):
    from cudasw4_amd import pssm
    assert abs(R.lam(O.blosum21(which)) - LAMBDA[which]) < 1e-6
    c, _, w, _ = master_only(np.array([0], dtype=np.int8))
    _, lam = pssm.from_counts("A", c, w, matrix=which)
    assert abs(lam - LAMBDA[which]) < 1e-6
    _, lam25 = pssm.from_counts("A", c, w, matrix=which * 100 + 25)   # a _25 matrix: the 21-letter table of the same name
    assert lam25 == lam


def test_half_a_half_s_row():
    from cudasw4_amd import pssm
    counts = np.zeros((1, 20), dtype=np.uint32)
    wcounts = np.zeros((1, 20), dtype=np.uint64)
    counts[0, [0, 15]] = 1           # A and S: k = 2, alpha = 1
    wcounts[0, [0, 15]] = 12345678   # f = 1/2 A + 1/2 S
    want = [3.271, -1.300, -0.456, -1.144, -0.761, -0.761]
    _, raw, _ = R.convert(O.blosum21(62), [0], counts, wcounts, 10.0)
    assert np.abs(raw[0, :6] - want).max() < 1e-3, raw[0, :6]
    p, _, praw = pssm.from_counts([0], counts, wcounts, matrix=62, pseudocount=10.0, with_raw=True)
    assert np.abs(praw[0, :6] - want).max() < 1e-3, praw[0, :6]
    assert p[0, :6].tolist() == [3, -1, 0, -1, -1, -1]


@pytest.mark.parametrize("which", MATRICES)
def test_no_hits_is_from_sequence(which):
    from cudasw4_amd import driver, pssm
    letters = "ARNDCQEGHILKMFPSTWYV" + "XAXB*ZJU" + "MKV"
    codes = driver.encode(letters)
    assert (codes[:20] == np.arange(20)).all() and (codes[[20, 22, 23, 24, 25, 26, 27]] == 20).all()
    c, wt, w, used = master_only(codes)
    assert used == 0 and int(c.sum()) == int((codes < 20).sum()) and wt.tolist() == [F * int((codes < 20).sum())]
    table = O.blosum21(which)
    want = pssm.from_sequence(letters, table)
    got, lam, raw = pssm.from_counts(letters, c, w, matrix=which, with_raw=True)
    assert got.dtype == np.int8 and got.shape == (len(letters), 21)
    assert got.tolist() == want.tolist()
    assert (got[:, 20] == table.reshape(21, 21)[np.minimum(codes, 20), 20]).all() and (got[:, 20] < 0).all()
    assert np.abs(raw - want[:, :20]).max() < 1e-12   # alpha = 0, f a unit vector: raw = s
    ref, rraw, _ = R.convert(table, codes, c, w)
    assert ref.tolist() == want.tolist() and np.abs(rraw - want[:, :20]).max() < 1e-12
    # the same under the 25-letter matrix of that name, and with codes in place of letters
    assert pssm.from_counts(codes, c, w, matrix=which * 100 + 25)[0].tolist() == want.tolist()


def test_worked_example():
    """master ACDE; hit 1 = "ACN" aligned 2=1X from query position 0; hit 2 = "SCE", from its second letter, aligned 1=1I1=
    from query position 1.  Position 0: A A; 1: C C C; 2: D N; 3: E E."""
    from cudasw4_amd import pssm
    master = O.encode("ACDE")
    subjects = [O.encode("ACN"), O.encode("SCE")]
    chars, offsets, lengths = O.make_db(subjects)
    res = np.zeros(2, dtype=R.RECORD)
    cig = np.concatenate([R.words("2=1X"), R.words("1=1I1=")])
    res[0] = (20, R.OK, 0, 3, 0, 3, 3, 2, 1, 0, 0, 2, 0)
    res[1] = (9, R.OK, 1, 4, 1, 3, 3, 2, 0, 1, 1, 3, 2)
    counts, weights, wcounts, used = R.accumulate(master, 4, chars, offsets, lengths, res, cig)
    A, C, D, E, N = 0, 4, 3, 6, 2
    want_c = np.zeros((4, 20), dtype=np.uint32)
    want_c[0, A], want_c[1, C], want_c[2, D], want_c[2, N], want_c[3, E] = 2, 3, 1, 1, 2
    assert used == 2 and counts.tolist() == want_c.tolist()
    # k = 1, 1, 2, 1: the terms are 2^32 / (1 * 2), 2^32 / (1 * 3), 2^32 / (2 * 1), 2^32 / (1 * 2)
    t0, t1, t2, t3 = 2147483648, 1431655765, 2147483648, 2147483648
    w1, w2, wm = t0 + t1 + t2, t1 + t3, t0 + t1 + t2 + t3
    assert (w1, w2, wm) == (5726623061, 3579139413, 7874106709)
    assert weights.tolist() == [w1, w2, wm]
    want_w = np.zeros((4, 20), dtype=np.uint64)
    want_w[0, A], want_w[1, C], want_w[2, D], want_w[2, N], want_w[3, E] = wm + w1, wm + w1 + w2, wm, w1, wm + w2
    assert wcounts.tolist() == want_w.tolist()
    assert int(want_w[1, C]) == 17179869183 and int(want_w[0, A]) == 13600729770
    # a zero include byte takes hit 2 out; without a master row the hits stand alone
    c2, wt2, _, used2 = R.accumulate(master, 4, chars, offsets, lengths, res, cig, include=[1, 0])
    assert used2 == 1 and int(c2[1, C]) == 2 and int(wt2[1]) == 0 and int(c2[3, E]) == 1
    c3, wt3, _, _ = R.accumulate(None, 4, chars, offsets, lengths, res, cig)
    assert int(c3[0, A]) == 1 and int(wt3[2]) == 0 and int(c3[2, D]) == 0
    # position 2 of the PSSM: D and N observed (alpha = 1), the others from the pseudocounts alone; conserved C stays high
    p, lam, raw = pssm.from_counts(master, counts, wcounts, matrix=62, with_raw=True)
    ref, rraw, _ = R.convert(O.blosum21(62), master, counts, wcounts)
    assert p.tolist() == ref.tolist() and np.abs(raw - rraw).max() < 1e-9
    assert p[1, C] == 9 and p[2, D] > p[2, A] and p[2, N] > p[2, A]
    assert p[0].tolist() == O.blosum21(62).reshape(21, 21)[A].tolist()   # one residue observed: alpha = 0, the table's row


CASES = [(which, seed) for which in MATRICES for seed in (1, 2, 3)]


@pytest.mark.parametrize("which,seed", CASES)
def test_conversion_against_reference(which, seed):
    """Counts and weighted counts of random alignments (made by the reference): raw scores within 1e-9, and every int8 entry
    equal — no entry of any case lies within 1e-6 of a half-integer, which the test asserts, so nothing is excused."""
    from cudasw4_amd import pssm
    rng = np.random.default_rng(1000 * which + seed)
    qlen = int(rng.integers(40, 120))
    master = rng.integers(0, 21, qlen).astype(np.int8)
    master[rng.integers(0, qlen, 3)] = 20
    n = int(rng.integers(1, 40))
    chars, offsets, lengths, res, cig = R.random_alignments(rng, qlen, n, master)
    include = (rng.random(n) < 0.8).astype(np.uint8)
    counts, weights, wcounts, used = R.accumulate(master, qlen, chars, offsets, lengths, res, cig, include)
    assert used == int(include.sum()) and int(counts.max()) >= 2
    beta = [10.0, 3.5, 25.0][seed - 1]
    want, wraw, wlam = R.convert(O.blosum21(which), master, counts, wcounts, beta)
    got, lam, raw = pssm.from_counts(master, counts, wcounts, matrix=which, pseudocount=beta, with_raw=True)
    assert abs(lam - wlam) < 1e-12
    assert np.abs(raw - wraw).max() < 1e-9
    frac = np.abs(np.abs(wraw) % 1.0 - 0.5)
    assert frac.min() > 1e-6, (which, seed, float(frac.min()))
    assert got.tolist() == want.tolist()
    assert (np.abs(got[:, :20] - wraw) <= 0.5 + 1e-9).all()   # (rounded to nearest)


def test_rows_without_counts_refusals_and_clamping():
    from cudasw4_amd import driver, pssm
    table = O.blosum21(62).reshape(21, 21)
    master = np.array([3, 20, 7, 11], dtype=np.int8)
    counts = np.zeros((4, 20), dtype=np.uint32)
    wcounts = np.zeros((4, 20), dtype=np.uint64)
    counts[2, [7, 9]] = [5, 1]
    wcounts[2, [7, 9]] = [5 * F, F // 3]
    p, _, raw = pssm.from_counts(master, counts, wcounts, with_raw=True)
    ref, rraw, _ = R.convert(table, master, counts, wcounts)
    assert p.tolist() == ref.tolist() and np.abs(raw - rraw).max() < 1e-9
    for i in (0, 1, 3):   # T_i == 0: the table's row of the master's letter (row 20 for a non-standard one)
        assert p[i].tolist() == table[master[i]].tolist()
    assert p[2].tolist() != table[7].tolist() and p[2, 20] == table[7, 20]
    for beta in (0.0, -1.0, float("nan")):
        with pytest.raises(driver.DriverError):
            pssm.from_counts(master, counts, wcounts, pseudocount=beta)
        if beta == beta:
            with pytest.raises(ValueError):
                R.convert(table, master, counts, wcounts, beta)
    with pytest.raises(driver.DriverError):
        pssm.from_counts(master, counts, wcounts, matrix=63)
    with pytest.raises(ValueError):
        pssm.from_counts(master, counts[:3], wcounts)
    # Clamping.  With a vanishing pseudocount an unobserved residue of a row with two observed ones (alpha = 1) has
    # Q = beta g / (1 + beta), far below exp(-128 lambda): the entry is -128, not a wrapped value.
    p, _, raw = pssm.from_counts(master, counts, wcounts, pseudocount=1e-40, with_raw=True)
    ref, rraw, _ = R.convert(table, master, counts, wcounts, 1e-40)
    unobserved = [a for a in range(20) if a not in (7, 9)]
    assert (raw[2, unobserved] < -200).all() and (p[2, unobserved] == -128).all() and ref.tolist() == p.tolist()
    assert p[2, 7] > 0
    # The upper clamp cannot be reached from any counts: Q <= max(f, g) <= max(1, p_a exp(lambda s_max)), so
    # raw <= max(ln(1 / p_a) / lambda, s_max) < 19 for the four tables (p_W = 0.0133, lambda >= 0.229).  The largest raw a
    # single observed residue gives, beta -> 0 with alpha = 1: ln(f / p) / lambda.
    counts[2, :] = 0
    wcounts[2, :] = 0
    counts[2, [17, 9]] = [1, 1]
    wcounts[2, [17, 9]] = [F * 1000, 1]
    p, _, raw = pssm.from_counts(master, counts, wcounts, pseudocount=1e-40, with_raw=True)
    assert 13 < raw[2, 17] < 19 and p[2, 17] == round(raw[2, 17]) and int(p.max()) < 127


def test_ascii_writer_round_trip(tmp_path):
    from cudasw4_amd import driver, pssm
    rng = np.random.default_rng(4)
    p = rng.integers(-128, 128, (37, 21)).astype(np.int8)
    p[:, 20] = -3
    p[0, :4] = [-128, 127, 0, -1]
    cons = "".join(rng.choice(list(pssm.LETTERS + "X*-"), 37))
    f = str(tmp_path / "w.pssm")
    driver.write_pssm_ascii(f, p, cons)
    back, bcons = pssm.read_ascii(f)
    assert back[:, :20].tolist() == p[:, :20].tolist() and bcons == cons and (back[:, 20] == pssm.OTHER_SCORE).all()
    g = str(tmp_path / "py.pssm")
    pssm.write_ascii(g, p, consensus=cons)
    assert open(f).read() == open(g).read()
    # align's reader takes it: the run gets past the file and fails on the device or on the DB, not on a line of the file
    out = subprocess.run([ALIGN, "--pssm", f, "--db", str(tmp_path / "nodb")], capture_output=True, text=True)
    assert out.returncode != 0 and "w.pssm:" not in out.stderr
    assert "No GPU found" in out.stderr or "nodb" in out.stderr, out.stderr
    with pytest.raises(driver.DriverError):
        driver.write_pssm_ascii(f, p, cons[:-1])


def test_align_flags(tmp_path, golden_dir):
    fasta = os.path.join(golden_dir, "allqueries.fasta")
    prefix = os.path.join(golden_dir, "allqueries_db", "aq")
    # --iterations above 1 without --inclusionScore: refused on the command line, before any device is opened
    out = subprocess.run([ALIGN, "--query", fasta, "--db", prefix, "--iterations", "2"], capture_output=True, text=True)
    assert out.returncode != 0 and "--inclusionScore" in out.stderr and "E-values" in out.stderr and "raw score" in out.stderr
    assert "No GPU found" not in out.stderr
    assert "iterations: 2" in out.stdout
    out = subprocess.run([ALIGN, "--query", fasta, "--db", prefix, "--outPssm", str(tmp_path / "p")], capture_output=True, text=True)
    assert out.returncode != 0 and "--inclusionScore" in out.stderr and "No GPU found" not in out.stderr
    for bad in (["--iterations", "0"], ["--iterations", "2", "--inclusionScore", "50", "--pseudocount", "0"],
                ["--iterations", "2", "--inclusionScore", "50", "--interactive"]):
        out = subprocess.run([ALIGN, "--query", fasta, "--db", prefix] + bad, capture_output=True, text=True)
        assert out.returncode != 0 and "No GPU found" not in out.stderr and out.stderr.startswith("align: "), out.stderr
    out = subprocess.run([ALIGN, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--iterations", "--inclusionScore", "--pseudocount", "--outPssm"):
        assert flag in out.stdout, flag
    # the option dump names the new flags only when they are used
    out = subprocess.run([ALIGN, "--query", "q.fa", "--db", "x"], capture_output=True, text=True)
    for word in ("iterations", "inclusionScore", "pseudocount", "outPssm"):
        assert word not in out.stdout
    out = subprocess.run([ALIGN, "--query", "q.fa", "--db", "x", "--iterations", "3", "--inclusionScore", "40", "--pseudocount", "5",
                          "--outPssm", "pre"], capture_output=True, text=True)
    for line in ("iterations: 3", "inclusionScore: 40", "pseudocount: 5", "outPssm: pre"):
        assert line in out.stdout


def test_accumulate_is_declared_exported_and_checks_its_arguments():
    from cudasw4_amd import capi, driver
    header = open(os.path.join(ROOT, "include", "cudasw4_amd_pssm.h")).read()
    assert "int sw_pssm_accumulate(sw_ctx* ctx, const sw_pssm_accumulate_args* a);" in header
    assert "sw_pssm_accumulate" in capi.PSSM_EXPORTS and "sw_pssm_accumulate" not in capi.EXPORTS
    assert hasattr(ctypes.CDLL(os.path.join(LIBDIR, "libcudasw4_amd.so")), "sw_pssm_accumulate")
    for name in ("swdrv_pssm_from_counts", "swdrv_build_pssm", "swdrv_write_pssm_ascii"):
        assert name in driver.EXPORTS and hasattr(ctypes.CDLL(os.path.join(LIBDIR, "libcudasw4_host.so")), name)
    with pytest.raises(capi.SwError) as e:   # a null context needs no GPU to be refused
        capi.pssm_accumulate(None, 0, 10, 0, 0, 0, 0, 0, 0, 0, 4096, 4096, 4096, 4096)
    assert e.value.code == -1
    assert capi.lib.sw_pssm_accumulate(None, None) == -1
    # the host files of the fake-runtime build do not reach the new code
    for name in ("search_driver.cpp", "driver_capi.cpp"):
        text = open(os.path.join(ROOT, "cudasw4_amd", "csrc", "host", name)).read()
        assert "pssm_build" not in text and "sw_pssm_accumulate" not in text
