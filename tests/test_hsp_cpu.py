"""CPU: the reference of several alignments per hit (tests/hsp_ref.c) against the single-alignment references, an
independent numpy DP and the properties of its definition; and the new entry points of the C ABI, the driver's C ABI, the
Python bindings and `align` (sw_align_hsps, swdrv_align_hsps, --maxHsps / --hspMinScore)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import align_cases as C
import gpu_util as G
import hsp_cases as HC
import hsp_ref as H
import oracle_lib as O

ROOT = O.ROOT
LIBDIR = os.path.join(ROOT, "cudasw4_amd", "lib")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(LIBDIR, "libcudasw4_host.so")):
        import __graft_entry__ as g
        g.build()
    return LIBDIR


# ---- max_hsps = 1 is align_ref / pssm_align_ref -------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["letters", "pssm"])
def test_one_alignment_is_the_plain_reference_on_tie_cases(form):
    for case, subjects in C.tie_cases(form):
        for gop, gex in ((-11, -1), (-5, -5), (-2, -5), (0, 0)):
            for s in subjects:
                want = case.reference(s, gop, gex)
                (r, w), = HC.reference(case, s, gop, gex, 1, 1)
                assert r == want[0] and w.tolist() == want[1].tolist(), (form, gop, gex, len(s))


def test_one_alignment_is_the_plain_reference_on_random_cases():
    """align_cases.random_align_case: both letter tables, PSSMs with and without a consensus, with the case's trace budget,
    CIGAR slots and expected scores"""
    rng = np.random.default_rng(2024)
    seen = set()
    for _ in range(30):
        case = C.random_align_case(rng)
        seen.add(case.form)
        for k, s in enumerate(case.subjects):
            (r, w), = HC.reference(case, s, case.gop, case.gex, 1, 1, trace_bytes=case.trace, caps=[case.caps[k]],
                                   expected=None if case.expected is None else case.expected[k])
            assert r == case.want[k][0] and w.tolist() == case.want[k][1].tolist(), (case.form, k, r, case.want[k][0])
    assert seen == {"letters21", "letters25", "pssm", "pssm_cons"}


# ---- an independent DP with an explicit forbidden set -------------------------------------------------------------------------

def local_score_numpy(scores, s, gop, gex, forbidden):
    """best local score of Gotoh's recurrence, written cell by cell: scores (qlen x 21), the diagonal move into a cell of
    `forbidden` does not exist"""
    qlen, slen = scores.shape[0], len(s)
    NEG = -10 ** 9
    Hm = np.zeros((qlen + 1, slen + 1), dtype=np.int64)
    E = np.full((qlen + 1, slen + 1), NEG, dtype=np.int64)
    F = np.full((qlen + 1, slen + 1), NEG, dtype=np.int64)
    best = 0
    for i in range(1, qlen + 1):
        for j in range(1, slen + 1):
            E[i, j] = max(E[i, j - 1] + gex, Hm[i, j - 1] + gop)
            F[i, j] = max(F[i - 1, j] + gex, Hm[i - 1, j] + gop)
            h = max(0, E[i, j], F[i, j])
            if (i - 1, j - 1) not in forbidden:
                h = max(h, Hm[i - 1, j - 1] + int(scores[i - 1, s[j - 1]]))
            Hm[i, j] = h
            best = max(best, h)
    return int(best)


@pytest.mark.parametrize("form", ["letters", "pssm"])
def test_scores_against_a_numpy_dp_with_a_forbidden_set(form):
    rng = np.random.default_rng(12 + (form == "pssm"))
    for trial in range(12):
        qlen = int(rng.integers(3, 13))
        q = rng.integers(0, 20, qlen).astype(np.int8)
        s = np.concatenate([HC.spacer(rng, int(rng.integers(0, 5))), q[: int(rng.integers(2, qlen + 1))], HC.spacer(rng, 3),
                            HC.mutated(rng, q, 0.2), q[int(rng.integers(0, qlen - 1)):]])[:40]
        gop, gex = [(-11, -1), (-5, -5), (-3, -1)][trial % 3]
        case = HC.make_case(q, form)
        slots = HC.reference(case, s, gop, gex, 5, 1)
        assert HC.check_properties(case, s, gop, gex, slots) is None
        forbidden, sc = set(), HC.plain_scores(case)
        for k, (r, w) in enumerate(slots):
            assert r["score"] == local_score_numpy(sc, s, gop, gex, forbidden), (form, trial, k)
            if r["status"] != H.OK:
                assert r["status"] == H.EMPTY and all(x[0]["status"] == H.EMPTY for x in slots[k:])
                break
            forbidden |= set(H.pairs(r, w))


# ---- the four properties on related pairs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("scoring", [(62, -11, -1), (50, -13, -2)])
@pytest.mark.parametrize("form", ["letters", "pssm-argmax"])
def test_properties_on_random_related_pairs(form, scoring):
    which, gop, gex = scoring
    rng = np.random.default_rng(which + (form != "letters"))
    for _ in range(25):
        q = rng.integers(0, 20, int(rng.integers(5, 160))).astype(np.int8)
        case = HC.make_case(q, form, which)
        for s in G.relatives(rng, q, 1, len(q) + 1, 2 * len(q) + 60) + [np.concatenate([q, HC.mutated(rng, q), q[::-1], q[len(q) // 2:]])]:
            for min_score in (1, 30):
                slots = HC.reference(case, s, gop, gex, 6, min_score)
                bad = HC.check_properties(case, s, gop, gex, slots)
                assert bad is None, (bad, form, scoring, len(q), len(s))
                st = [r["status"] for r, _ in slots]
                n_ok = st.index(H.EMPTY) if H.EMPTY in st else len(st)
                assert st == [H.OK] * n_ok + [H.EMPTY] * (len(st) - n_ok)
                assert all(r["score"] >= min_score for r, _ in slots[1:n_ok])
                assert all(r["score"] == 0 and r["q_begin"] == r["s_end"] == -1 and len(w) == 0 for r, w in slots[n_ok:])
            # fewer slots: a prefix of the same list
            assert [(r, w.tolist()) for r, w in HC.reference(case, s, gop, gex, 2, 1)] == \
                   [(r, w.tolist()) for r, w in HC.reference(case, s, gop, gex, 6, 1)[:2]]


def test_statuses_behind_a_slot_without_traceback():
    rng = np.random.default_rng(3)
    q, s = HC.three_copies(rng)
    case = HC.make_case(q)
    full = HC.reference(case, s, -11, -1, 3, 1)
    st = lambda slots: [r["status"] for r, _ in slots]
    assert st(full) == [H.OK] * 3
    assert st(HC.reference(case, s, -11, -1, 3, 1, caps=[1, 0, 50])) == [H.OK, H.NO_TRACE, H.NOT_COMPUTED]
    assert st(HC.reference(case, s, -11, -1, 3, 1, expected=full[0][0]["score"] + 1)) == [H.SCORE_MISMATCH, H.NOT_COMPUTED, H.NOT_COMPUTED]
    assert st(HC.reference(case, s, -11, -1, 3, 1, max_subject_len=len(s) - 1)) == [H.BAD_LENGTH, H.NOT_COMPUTED, H.NOT_COMPUTED]
    assert st(HC.reference(case, s, -11, -1, 3, 1, trace_bytes=C.trace_bytes(24, 24) - 256)) == [H.NO_TRACE, H.NOT_COMPUTED, H.NOT_COMPUTED]
    assert st(HC.reference(case, np.full(9, 20, dtype=np.int8), -11, -1, 3, 1)) == [H.EMPTY] * 3
    r = HC.reference(case, s, -11, -1, 3, 1, caps=[1, 0, 50])[2][0]
    assert (r["score"], r["q_begin"], r["q_end"], r["s_begin"], r["s_end"], r["cigar_len"]) == (0, -1, -1, -1, -1, 0)


# ---- the C ABI, the bindings and the command line ----------------------------------------------------------------------------

def test_header_symbols_are_declared_and_exported(built):
    from cudasw4_amd import capi, driver
    header = open(os.path.join(ROOT, "include", "cudasw4_amd_hsps.h")).read()
    declared = set(re.findall(r"^int (sw_[a-z_0-9]+)\(", header, re.M))
    assert declared == set(capi.HSPS_EXPORTS) == {"sw_align_hsps", "sw_align_hsps_pssm"}
    assert not (declared & (set(capi.EXPORTS) | set(capi.PSSM_EXPORTS) | set(capi.STATS_EXPORTS) | set(capi.RANK_EXPORTS)))
    assert '#include "cudasw4_amd_pssm.h"' in header
    assert re.search(r"#define SW_MAX_HSPS 16\b", header) and re.search(r"#define SW_ALIGN_NOT_COMPUTED 5\b", header)
    assert capi.MAX_HSPS == 16 and capi.ALIGN_NOT_COMPUTED == 5 == H.NOT_COMPUTED
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libcudasw4_amd.so"))
    assert all(hasattr(lib, name) for name in declared)
    assert hasattr(capi, "align_hsps") and hasattr(capi, "align_hsps_pssm")
    dheader = open(os.path.join(ROOT, "include", "cudasw4_amd_driver.h")).read()
    host = ctypes.CDLL(os.path.join(LIBDIR, "libcudasw4_host.so"))
    for name in ("swdrv_align_hsps", "swdrv_align_hsps_pssm"):
        assert name + "(" in dheader and name in driver.EXPORTS and hasattr(host, name)
    import inspect
    for f in (driver.Driver.align_hits, driver.Driver.align_hits_pssm):
        p = inspect.signature(f).parameters
        assert p["max_hsps"].default == 1 and p["min_score"].default is None


def test_fake_linked_driver_has_no_hsp_symbol(built):
    """tests/host/fake_gpu links driver_capi.cpp + search_driver.cpp against a fake C ABI without the aligner"""
    fake = os.path.join(ROOT, "tests", "host", "_build", "libfake_driver.so")
    if not os.path.exists(fake):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "host", "fake_gpu")], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(fake)
    assert not hasattr(lib, "swdrv_align_hsps") and not hasattr(lib, "swdrv_align_hsps_pssm")


def test_struct_sizes_match_the_header(built, tmp_path):
    from cudasw4_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n' % os.path.join(ROOT, "include", "cudasw4_amd_hsps.h")
                   + 'printf("%zu %zu %zu %zu %zu\\n", sizeof(sw_hsp_args), offsetof(sw_hsp_args, max_hsps), offsetof(sw_hsp_args, min_score), '
                     'sizeof(sw_align_args), sizeof(sw_align_result));\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out == [ctypes.sizeof(capi._HspArgs), capi._HspArgs.max_hsps.offset, capi._HspArgs.min_score.offset,
                   ctypes.sizeof(capi._AlignArgs), capi.align_result_dtype().itemsize]
    assert out[:3] == [8, 0, 4]


def test_argument_checks_that_need_no_device(built):
    from cudasw4_amd import capi
    cases = [(dict(max_hsps=0), "max_hsps"), (dict(max_hsps=17), "max_hsps"), (dict(max_hsps=-1), "max_hsps"),
             (dict(max_hsps=2, min_score=0), "min_score"), (dict(max_hsps=1, min_score=-5), "min_score"),
             (dict(max_hsps=2, flags=capi.ALIGN_COORDS_ONLY), "SW_ALIGN_COORDS_ONLY"),
             (dict(max_hsps=16, phase_events=[0, 0, 0, 0]), "phase_events"), (dict(max_hsps=2), "null argument")]
    for f, lead in ((capi.align_hsps, (None, 0)), (capi.align_hsps_pssm, (None, 0, 0))):
        for kw, word in cases:
            with pytest.raises(capi.SwError) as e:
                f(*lead, 10, 1, 0, 0, 0, 100, -11, -1, 0, **kw)
            assert e.value.code == -1 and word in str(e.value) and f.__name__.replace("align", "sw_align") in str(e.value), (kw, str(e.value))
    assert capi.lib.sw_align_hsps(None, None, None) == -1 and capi.lib.sw_align_hsps_pssm(None, None, None, None) == -1


def test_driver_argument_checks():
    from cudasw4_amd import driver
    d = object.__new__(driver.Driver)     # the checks come before the handle is touched
    for kw, word in ((dict(max_hsps=0), "max_hsps"), (dict(max_hsps=17, min_score=5), "max_hsps"), (dict(max_hsps=2), "min_score"),
                     (dict(max_hsps=2, min_score=0), "min_score")):
        with pytest.raises(ValueError, match=word):
            driver.Driver.align_hits(d, "ACDE", dict(ids=[], scores=[]), **kw)
        with pytest.raises(ValueError, match=word):
            driver.Driver.align_hits_pssm(d, np.full((4, 21), -1, dtype=np.int8), dict(ids=[], scores=[]), **kw)


def run_align(*args):
    return subprocess.run([os.path.join(LIBDIR, "align"), "--query", "no_such_file.fa", "--db", "no_such_db"] + list(args),
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_fire_before_any_device(built):
    for args, words in ((["--maxHsps", "3", "--hspMinScore", "20"], ["--maxHsps", "--alignments", "--pssmAlignments"]),
                        (["--hspMinScore", "20"], ["--hspMinScore", "--alignments"]),
                        (["--alignments", "--maxHsps", "0", "--hspMinScore", "20"], ["--maxHsps", "1 .. 16"]),
                        (["--alignments", "--maxHsps", "17", "--hspMinScore", "20"], ["--maxHsps", "1 .. 16"]),
                        (["--pssmAlignments", "--maxHsps", "2"], ["--maxHsps", "--hspMinScore"]),
                        (["--alignments", "--maxHsps", "2", "--hspMinScore", "0"], ["--hspMinScore", "at least 1"])):
        p = run_align(*args)
        assert p.returncode == 1 and p.stderr.startswith("align: "), (args, p.stderr)
        assert all(w in p.stderr for w in words) and "GPU" not in p.stderr, (args, p.stderr)
    # --maxHsps 1 needs no --hspMinScore: it gets as far as opening a device or the DB
    p = run_align("--alignments", "--maxHsps", "1")
    assert "--maxHsps" not in p.stderr and "--hspMinScore" not in p.stderr
    assert "--maxHsps" in subprocess.run([os.path.join(LIBDIR, "align"), "--help"], capture_output=True, text=True).stdout
