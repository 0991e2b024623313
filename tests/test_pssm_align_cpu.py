"""CPU: the reference of hit alignment for PSSM queries (tests/pssm_align_ref.c) pinned to the letter reference
(tests/align_ref.c) and to the PSSM scan reference (tests/pssm_ref.c), and the new entry points of the C ABI, the driver's
C ABI, the Python bindings and `align` (sw_align_hits_pssm, swdrv_align_hits_pssm, --pssmAlignments)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as A
import gpu_util as G
import oracle_lib as O
import pssm_align_ref as PA
import pssm_ref as PR

ROOT = O.ROOT
LIBDIR = os.path.join(ROOT, "cudasw4_amd", "lib")
GAPS = [(-11, -1), (-5, -5)]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(LIBDIR, "libcudasw4_host.so")):
        import __graft_entry__ as g
        g.build()
    return LIBDIR


def matrix25_as_rows(which=62):
    from cudasw4_amd import driver
    m = np.asarray(driver.matrix25(which), dtype=np.int8).reshape(25, 25)
    return np.ascontiguousarray(m[:, list(range(20)) + [23]])


def random_pssm(rng, qlen, extremes=True):
    """position-specific scores in about [-8, 12], column 20 = -1, and a few rows that reach the ends of int8"""
    p = rng.integers(-8, 13, (qlen, 21)).astype(np.int8)
    if extremes:
        for i in rng.integers(0, qlen, max(1, qlen // 16)):
            p[i, rng.integers(0, 20, 3)] = (127, -128, -127)
    p[:, 20] = -1
    return p


def subjects_for(rng, cons, qlen):
    out = [rng.integers(0, 21, int(rng.integers(1, 150))).astype(np.int8)]
    out += G.relatives(rng, np.minimum(cons, 19).astype(np.int8), 2, max(qlen, 2), qlen + 150)
    return out


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("gaps", GAPS)
def test_from_sequence_reproduces_the_letter_reference(built, full, gaps):
    from cudasw4_amd import pssm
    gop, gex = gaps
    rng = np.random.default_rng(300 + 7 * full - gop)
    if full:
        from cudasw4_amd import driver
        table, mref, alpha = driver.matrix25(62), matrix25_as_rows(), 25
    else:
        table = mref = O.blosum21(62)
        alpha = 21
    for k in range(25):
        q = rng.integers(0, alpha, int(rng.integers(1, 120))).astype(np.int8)
        p = pssm.from_sequence(q, table)
        auto = np.array([pssm.LETTERS.index(c) for c in pssm.consensus_of(p)], dtype=np.int8)
        for s in subjects_for(rng, q, len(q)):
            want, wcig = A.align(q, s, mref, gop, gex)
            # consensus = q: every field and every CIGAR word
            got, cig = PA.align(p, s, q, gop, gex)
            assert got == want and cig.tolist() == wcig.tolist(), (k, full, got, want)
            # no consensus: the same alignment; '=' / 'X' and their counts against consensus_of
            got, cig = PA.align(p, s, None, gop, gex)
            same = [f for f in A.FIELDS if f not in ("identities", "mismatches", "cigar_len")]
            assert [got[f] for f in same] == [want[f] for f in same]
            if want["status"] == A.OK:
                ids, mis, words = PA.recount(p, s, auto, want, wcig)
                assert (got["identities"], got["mismatches"], cig.tolist()) == (ids, mis, words)
                assert ids + mis == want["identities"] + want["mismatches"]


@pytest.mark.parametrize("gaps", GAPS)
def test_position_specific_pssms(built, gaps):
    gop, gex = gaps
    rng = np.random.default_rng(41 - gop)
    seen = 0
    for k in range(40):
        qlen = int(rng.integers(1, 140))
        p = random_pssm(rng, qlen)
        cons = np.argmax(p[:, :20], axis=1).astype(np.int8)
        for s in subjects_for(rng, cons, qlen):
            r, words = PA.align(p, s, None, gop, gex)
            assert r["score"] == PR.score(p, s, gop, gex), (k, gop, gex)
            if r["score"] == 0:
                assert r["status"] == A.EMPTY and r["q_begin"] == -1 and r["s_end"] == -1 and len(words) == 0
                continue
            seen += 1
            assert r["status"] == A.OK
            assert PA.rescore(p, s, gop, gex, r, words) == r["score"]
            first, last = PA.column_scores(p, s, r, words)
            assert first is not None and first > 0 and last is not None and last > 0, A.cigar_string(words)
            assert r["columns"] == sum(int(w) >> 4 for w in words)
            assert r["identities"] + r["mismatches"] + r["gap_columns"] == r["columns"]
            ids, mis, again = PA.recount(p, s, cons, r, words)
            assert (r["identities"], r["mismatches"], words.tolist()) == (ids, mis, again)
            c, cw = PA.align(p, s, None, gop, gex, coords_only=True)
            assert [c[f] for f in ("score", "q_begin", "q_end", "s_begin", "s_end")] == \
                   [r[f] for f in ("score", "q_begin", "q_end", "s_begin", "s_end")] and len(cw) == 0
    assert seen > 60


def test_consensus_rules():
    """codes of 20 and above are identical to nothing; without a consensus the first maximum of the row counts"""
    p = np.full((4, 21), -4, dtype=np.int8)
    for i, c in enumerate((3, 5, 7, 9)):
        p[i, c] = 6
    p[1, 2] = 6          # row 1: codes 2 and 5 tie, the lower one is the consensus
    p[:, 20] = -1
    s = np.array([3, 5, 7, 9], dtype=np.int8)
    r, w = PA.align(p, s, None, -6, -1)
    assert (r["score"], A.cigar_string(w), r["identities"], r["mismatches"]) == (24, "1=1X2=", 3, 1)
    r, w = PA.align(p, s, [3, 5, 20, 9], -6, -1)
    assert (A.cigar_string(w), r["identities"], r["mismatches"]) == ("2=1X1=", 3, 1)
    r, w = PA.align(p, np.array([3, 2, 7, 9], dtype=np.int8), None, -6, -1)
    assert (r["score"], A.cigar_string(w)) == (24, "4=")


def test_capi_declares_and_exports_align_hits_pssm(built):
    from cudasw4_amd import capi
    header = open(os.path.join(ROOT, "include", "cudasw4_amd_pssm.h")).read()
    assert re.search(r"^int sw_align_hits_pssm\(sw_ctx\* ctx, const sw_align_args\* a, const int8_t\* pssm\);", header, re.M)
    assert "sw_align_hits_pssm" in capi.PSSM_EXPORTS and "sw_align_hits_pssm" not in capi.EXPORTS
    assert "sw_align_hits_pssm" not in open(os.path.join(ROOT, "include", "cudasw4_amd.h")).read()
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libcudasw4_amd.so"))
    assert hasattr(lib, "sw_align_hits_pssm")
    # argument checks need no GPU: a null context, null args, a null PSSM
    with pytest.raises(capi.SwError) as e:
        capi.align_hits_pssm(None, 4096, 0, 10, 1, 0, 0, 0, 100, -11, -1, 0)
    assert e.value.code == -1
    assert capi.lib.sw_align_hits_pssm(None, None, None) == -1
    args = capi._AlignArgs()
    assert capi.lib.sw_align_hits_pssm(None, ctypes.byref(args), None) == -1


def test_driver_exports_align_hits_pssm(built):
    from cudasw4_amd import driver
    header = open(os.path.join(ROOT, "include", "cudasw4_amd_driver.h")).read()
    assert "swdrv_align_hits_pssm(" in header and "swdrv_align_hits_pssm" in driver.EXPORTS
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libcudasw4_host.so"))
    assert hasattr(lib, "swdrv_align_hits_pssm")
    assert hasattr(driver.Driver, "align_hits_pssm")
    lib.swdrv_align_hits_pssm.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + \
                                         [ctypes.c_void_p] * 2 + [ctypes.c_int64]
    assert lib.swdrv_align_hits_pssm(None, None, 0, None, None, None, 0, None, None, 0) == -1


def test_fake_linked_driver_has_no_pssm_alignment_symbol(built):
    """tests/host/fake_gpu links driver_capi.cpp + search_driver.cpp against a fake C ABI without sw_align_hits_pssm"""
    fake = os.path.join(ROOT, "tests", "host", "_build", "libfake_driver.so")
    if not os.path.exists(fake):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "host", "fake_gpu")], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(fake)
    assert not hasattr(lib, "swdrv_align_hits_pssm")


def test_align_command_line(tmp_path, built):
    from cudasw4_amd import pssm
    align = os.path.join(LIBDIR, "align")
    out = subprocess.run([align, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--pssmAlignments" in out.stdout
    rng = np.random.default_rng(3)
    good = str(tmp_path / "good.pssm")
    pssm.write_ascii(good, random_pssm(rng, 30, extremes=False))
    nodb = str(tmp_path / "nodb")
    # with the new flag a --pssm gets past option checking, with or without --alignments beside it: what fails is the DB / GPU
    for extra in (["--pssmAlignments"], ["--pssmAlignments", "--alignments"]):
        out = subprocess.run([align, "--pssm", good, "--db", nodb] + extra, capture_output=True, text=True)
        assert out.returncode != 0 and "cannot be combined" not in out.stderr
        assert "pssmAlignments: 1" in out.stdout and "pssmFile 0 : " + good in out.stdout
        assert "No GPU found" in out.stderr or "nodb" in out.stderr, out.stderr
    # without it the refusal stands and names the flag that lifts it
    out = subprocess.run([align, "--pssm", good, "--alignments", "--db", nodb], capture_output=True, text=True)
    assert out.returncode != 0 and all(w in out.stderr for w in ("--pssm", "--alignments", "--pssmAlignments"))
    # the option dump of other command lines does not change
    out = subprocess.run([align, "--query", "q.fa", "--db", "x"], capture_output=True, text=True)
    assert "pssmAlignments" not in out.stdout
