"""CPU: profile search (a position-specific scoring matrix as the query) — everything that needs no GPU: the scalar
reference tests/pssm_ref.c pinned to the project's oracle, the NCBI ASCII reader / writer (Python and `align --pssm`),
the exported symbols of include/cudasw4_amd_pssm.h and the command line."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pssm_ref as PR

ROOT = O.ROOT
LIBDIR = os.path.join(ROOT, "cudasw4_amd", "lib")
ALIGN = os.path.join(LIBDIR, "align")


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(os.path.join(LIBDIR, "libcudasw4_amd.so")) and os.path.exists(ALIGN)
            and os.path.exists(os.path.join(LIBDIR, "libcudasw4_host.so"))):
        import __graft_entry__ as g
        g.build()
    return LIBDIR


# ---- 1. the reference of the reference ------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [45, 50, 62, 80])
def test_pssm_ref_with_from_sequence_equals_the_oracle(which):
    from cudasw4_amd import pssm
    m = O.blosum21(which)
    rng = np.random.default_rng(1000 + which)
    lengths = [1, 2, 3, 15, 16, 17, 64, 255, 700]
    for gop, gex in ((-11, -1), (-10, -2), (-5, -5), (-20, -3), (0, 0)):
        for _ in range(12):
            ql = int(rng.choice(lengths)) if rng.random() < 0.5 else int(rng.integers(1, 701))
            sl = int(rng.choice(lengths)) if rng.random() < 0.5 else int(rng.integers(1, 701))
            q = rng.integers(0, 21, ql).astype(np.int8)
            s = rng.integers(0, 21, sl).astype(np.int8)
            if rng.random() < 0.5 and sl >= 8:   # a related pair: long gapped alignments, not only noise
                k = min(ql, sl)
                s[:k] = np.where(rng.random(k) < 0.8, q[:k], s[:k])
            p = pssm.from_sequence(q, m)
            assert p.shape == (ql, 21) and p.dtype == np.int8
            assert PR.score(p, s, gop, gex) == O.score(q, s, m, gop, gex), (which, gop, gex, ql, sl)


def test_pssm_ref_scan_walks_the_dbdata_layout():
    from cudasw4_amd import pssm
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, 21, int(n)).astype(np.int8) for n in (0, 1, 5, 33, 120, 121)]
    chars, offsets, lengths = O.make_db(seqs)
    q = rng.integers(0, 20, 77).astype(np.int8)
    p = pssm.from_sequence(q, O.blosum21(62))
    got = PR.scan(p, chars, offsets, lengths)
    assert got.tolist() == O.scan(q, chars, offsets, lengths).tolist()
    assert got[0] == 0
    # genuinely position-specific: two rows that no single letter could have
    p2 = p.copy()
    p2[3, :20] = -128
    p2[4, :20] = 127
    assert PR.scan(p2, chars, offsets, lengths).tolist() == [PR.score(p2, s) for s in seqs]
    assert PR.score(p2, seqs[3]) >= 127


def test_from_sequence_forms():
    from cudasw4_amd import pssm
    m = O.blosum21(62)
    a = pssm.from_sequence("ARNDX", m)
    b = pssm.from_sequence(O.encode("ARNDX"), m)
    assert a.tolist() == b.tolist() and (a[:, 20] < 0).all()
    assert a[0].tolist() == m.reshape(21, 21)[0].tolist()
    tabs = O.golden("ref_tables.json") if os.path.exists(os.path.join(O.GOLDEN_DIR, "ref_tables.json")) else None
    m25 = np.arange(625, dtype=np.int64).reshape(25, 25) % 11 - 8   # any table with a negative X column
    m25[:, 23] = -1
    p = pssm.from_sequence("ABZX*", m25.astype(np.int8))
    assert p.shape == (5, 21) and p[1, :20].tolist() == m25[20, :20].tolist() and p[1, 20] == m25[20, 23]
    assert tabs is None or isinstance(tabs, (dict, list))
    with pytest.raises(ValueError):
        pssm.from_sequence([21], m)
    with pytest.raises(ValueError):
        pssm.as_pssm(np.zeros((4, 21), dtype=np.int8))       # column 20 not negative
    with pytest.raises(ValueError):
        pssm.as_pssm(np.zeros((4, 20), dtype=np.int8))


# ---- 2. ASCII reader / writer ------------------------------------------------------------------------------------------

def _random_pssm(rng, n, lo=-12, hi=14):
    p = rng.integers(lo, hi + 1, (n, 21)).astype(np.int8)
    p[:, 20] = -1
    return p


@pytest.mark.parametrize("percentages,footer", [(False, False), (True, True), (True, False), (False, True)])
def test_ascii_round_trip(tmp_path, percentages, footer):
    from cudasw4_amd import pssm
    rng = np.random.default_rng(7)
    p = _random_pssm(rng, 57)
    p[5, 3], p[6, 4] = 127, -128
    cons = "".join(pssm.LETTERS[int(i)] for i in rng.integers(0, 20, 57))
    path = str(tmp_path / "a.pssm")
    pssm.write_ascii(path, p, cons, percentages=percentages, footer=footer)
    back, c2 = pssm.read_ascii(path)
    assert back.dtype == np.int8 and back.tolist() == p.tolist() and c2 == cons
    assert (back[:, 20] == pssm.OTHER_SCORE).all()
    pssm.write_ascii(path, p)   # consensus derived
    assert pssm.read_ascii(path)[1] == pssm.consensus_of(p)


def _psiblast_text(rows, header=True, cols=None):
    head = "           A  R  N  D  C  Q  E  G  H  I  L  K  M  F  P  S  T  W  Y  V   A   R   N   D   C   Q   E   G   H   I   L   K   M   F   P   S   T   W   Y   V\n"
    out = ["\n", "Last position-specific scoring matrix computed, weighted observed percentages rounded down, information per position, and relative weight of gapless real matches to pseudocounts\n"]
    if header:
        out.append(head)
    for idx, res, sc in rows:
        out.append("%5d %s  %s   %s  0.37 0.12\n" % (idx, res, " ".join("%2d" % v for v in sc), " ".join("%3d" % 0 for _ in range(20))))
    out += ["\n", "                      K         Lambda\n", "Standard Ungapped    0.1340     0.3170\n", "1 X gapped 0.04 0.26\n"]
    return "".join(out)


MALFORMED = {
    "missing_header": lambda good: (_psiblast_text(good, header=False), 3),
    "wrong_columns": lambda good: (_psiblast_text(good).replace(" 0.37 0.12", " 0.37", 1), 4),
    "nineteen_scores": lambda good: ("           A  R  N  D  C  Q  E  G  H  I  L  K  M  F  P  S  T  W  Y  V\n    1 M  " + " ".join(["1"] * 19) + "\n", 2),
    "not_consecutive": lambda good: (_psiblast_text([good[0], (3,) + good[1][1:]]), 5),
    "out_of_int8": lambda good: (_psiblast_text([good[0], (2, "A", [128] + [0] * 19)]), 5),
    "wrong_header_order": lambda good: (_psiblast_text(good).replace("A  R  N  D", "R  A  N  D", 1), 3),
}


@pytest.fixture(scope="module")
def good_rows():
    rng = np.random.default_rng(11)
    return [(i + 1, "ARNDCQ"[i % 6], rng.integers(-9, 12, 20).tolist()) for i in range(9)]


def test_reader_takes_psiblast_layout_and_stops_at_the_footer(tmp_path, good_rows):
    from cudasw4_amd import pssm
    path = str(tmp_path / "psi.pssm")
    open(path, "w").write(_psiblast_text(good_rows))
    p, cons = pssm.read_ascii(path)
    assert p[:, :20].tolist() == [r[2] for r in good_rows] and cons == "".join(r[1] for r in good_rows)


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_files_name_file_and_line(tmp_path, built, good_rows, case):
    from cudasw4_amd import pssm
    text, line = MALFORMED[case](good_rows)
    path = str(tmp_path / (case + ".pssm"))
    open(path, "w").write(text)
    with pytest.raises(pssm.PssmFormatError) as ei:
        pssm.read_ascii(path)
    assert "%s:%d:" % (path, line) in str(ei.value), str(ei.value)
    # `align` validates PSSM files before it opens a device: the same verdict on a machine without a GPU
    out = subprocess.run([ALIGN, "--pssm", path, "--db", str(tmp_path / "nodb")], capture_output=True, text=True)
    assert out.returncode != 0
    assert "%s:%d:" % (path, line) in out.stderr, out.stderr


# ---- 3. symbols, command line ---------------------------------------------------------------------------------------

def test_pssm_header_symbols_are_exported(built):
    from cudasw4_amd import capi, driver
    text = open(os.path.join(ROOT, "include", "cudasw4_amd_pssm.h")).read()
    declared = set(re.findall(r"^[a-z_0-9 *]*\b(sw_[a-z_0-9]+)\s*\(", text, re.M))
    assert declared == set(capi.PSSM_EXPORTS) and "sw_set_query_pssm" in declared
    assert '#include "cudasw4_amd.h"' in text
    assert not (declared & set(capi.EXPORTS))
    lib = ctypes.CDLL(os.path.join(built, "libcudasw4_amd.so"))
    for name in declared:
        assert hasattr(lib, name), name
    host = ctypes.CDLL(os.path.join(built, "libcudasw4_host.so"))
    for name in ("swdrv_scan_pssm", "swdrv_scan_submit_pssm"):
        assert hasattr(host, name) and name in driver.EXPORTS
    assert hasattr(capi.Context, "set_query_pssm") and hasattr(driver.Driver, "scan_pssm") and hasattr(driver.Driver, "submit_pssm")


def test_set_query_pssm_checks_its_arguments_without_a_gpu(built):
    lib = ctypes.CDLL(os.path.join(built, "libcudasw4_amd.so"))
    lib.sw_set_query_pssm.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.sw_last_error.restype = ctypes.c_char_p
    p = np.full((3, 21), -1, dtype=np.int8)
    assert lib.sw_set_query_pssm(None, p.ctypes.data, 3, None) == -1      # SW_ERR_INVALID: null context
    lib.sw_query_is_pssm.argtypes = [ctypes.c_void_p]
    assert lib.sw_query_is_pssm(None) == 0


def test_align_command_line(tmp_path, built, good_rows):
    out = subprocess.run([ALIGN, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--pssm" in out.stdout
    good = str(tmp_path / "good.pssm")
    open(good, "w").write(_psiblast_text(good_rows))
    # refused with a message, before any device is looked for
    out = subprocess.run([ALIGN, "--pssm", good, "--alignments", "--db", "x"], capture_output=True, text=True)
    assert out.returncode != 0 and "--pssm" in out.stderr and "--alignments" in out.stderr
    # a --pssm is a query: no "Query is missing"; listed in the options
    out = subprocess.run([ALIGN, "--pssm", good, "--db", str(tmp_path / "nodb")], capture_output=True, text=True)
    assert "Query is missing" not in out.stdout and "pssmFile 0 : " + good in out.stdout
    import torch
    if not torch.cuda.is_available():
        assert out.returncode != 0 and "No GPU found" in out.stderr
    # a missing file is an error of its own
    out = subprocess.run([ALIGN, "--pssm", str(tmp_path / "absent.pssm"), "--db", "x"], capture_output=True, text=True)
    assert out.returncode != 0 and "absent.pssm" in out.stderr
    # without --pssm nothing changes: no pssm line among the options
    out = subprocess.run([ALIGN, "--query", "q.fa", "--db", "x"], capture_output=True, text=True)
    assert "pssmFile" not in out.stdout
