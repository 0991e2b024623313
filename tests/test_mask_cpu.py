"""CPU: the subject-masking rule — the numpy statement (mask_ref.py) against its definition, the host
library against the numpy statement, the conditions on the defaults and on the end-to-end fixture, and the command line."""
import math
import subprocess

import numpy as np
import pytest

import mask_cases as MC
import mask_ref as MR
import oracle_lib as O
from cudasw4_amd import driver, mask, synthdb

ALL_PARAMS = MC.PARAM_SETS + [MC.RUN_PARAMS]
CASES = MC.cases()


def test_table_and_thresholds():
    assert MR.U[0] == 0 and MR.U[1:] == [int(round(1024 * math.log2(n))) for n in range(1, 33)]
    assert MR.threshold(12, 1.9) == 20705 and MR.threshold(12, 2.2) == 17019
    assert MR.DEFAULTS == (mask.DEFAULT_WINDOW, mask.threshold(12, mask.DEFAULT_TRIGGER_BITS), mask.threshold(12, mask.DEFAULT_EXTEND_BITS))
    # the header's literals are the reference's
    header = open(O.ROOT + "/include/cudasw4_amd_mask.h").read()
    body = header[header.index("#define SW_MASK_U_TABLE"):].split("typedef")[0].replace("\\", " ").replace("#define SW_MASK_U_TABLE", "")
    assert [int(x) for x in body.replace(",", " ").split()] == MR.U
    # with no code >= 20 in the window the sum is the entropy, to the rounding of U
    rng = np.random.default_rng(1)
    for W in (4, 12, 32):
        c = rng.integers(0, 4, 200).astype(np.int8)
        S = MR.window_sums(c, W)
        for i in (0, 57, len(S) - 1):
            n = np.bincount(c[i:i + W], minlength=20)
            h = -sum(k / W * math.log2(k / W) for k in n if k)
            assert abs((math.log2(W) - S[i] / (1024.0 * W)) - h) <= 0.5 / 1024 + 1e-9   # (every U[n] is off by at most a half, and the n_a add up to W)


def test_host_threshold_matches_reference():
    for W in range(4, 33):
        for K in (0.0, 0.5, 1.0, 1.9, 2.0, 2.2, 2.5, 3.0, 3.3, 4.0, 5.0, 6.0):
            assert mask.threshold(W, K) == MR.threshold(W, K), (W, K)
    assert mask.threshold(4, 2.0) == 1 and mask.threshold(32, 5.0) == 1 and mask.threshold(16, 7.5) == 1
    with pytest.raises(ValueError):
        mask.threshold(3, 1.0)


@pytest.mark.parametrize("params", ALL_PARAMS, ids=lambda p: "w%d" % p[0] + "-%d-%d" % p[1:])
def test_host_library_matches_reference(params):
    W, T, E = params
    some = 0
    for name, codes in CASES:
        got, n = mask.mask_subject(codes, W, trigger_sum=T, extend_sum=E, with_count=True)
        ref, rn = MR.mask_subject(codes, W, T, E, with_count=True)
        assert np.array_equal(got, ref) and n == rn, name
        covered = _covered(codes, W, T, E)
        assert rn == int(covered.sum()) and np.array_equal(ref != codes, covered & (codes != 20)), name
        some += rn > 0
        # idempotence, in both statements
        assert np.array_equal(MR.mask_subject(ref, W, T, E), ref), name
        assert np.array_equal(mask.mask_subject(got, W, trigger_sum=T, extend_sum=E), got), name
        if len(codes) < W:
            assert np.array_equal(ref, codes), name
    assert some >= 5


def _covered(codes, W, T, E):
    m = np.zeros(len(codes), dtype=bool)
    for a, b in MR.segments(codes, W, T, E):
        m[a:b] = True
    return m


def test_bits_interface_and_errors():
    codes = dict(CASES)["structured1025"]
    assert np.array_equal(mask.mask_subject(codes), MR.mask_subject(codes))
    assert np.array_equal(mask.mask_subject(codes, 16, 2.0, 2.4), MR.mask_subject(codes, 16, MR.threshold(16, 2.0), MR.threshold(16, 2.4)))
    for bad in (dict(window=3), dict(window=33), dict(trigger_sum=10, extend_sum=11), dict(trigger_sum=5, extend_sum=0)):
        with pytest.raises(ValueError):
            mask.mask_subject(codes, **bad)


def test_unbounded_runs_in_the_reference():
    b = MC.run_block()
    for i, bounds in enumerate(b["bounds"]):
        o = int(b["offsets"][i])
        seg = MR.segments(b["chars"][o:o + int(b["lengths"][i])], *MC.RUN_PARAMS)
        if bounds is None:
            assert seg == []
            continue
        assert len(seg) == 1
        (a0, a1), (e0, e1) = bounds
        assert a0 <= seg[0][0] <= a1 and e0 <= seg[0][1] <= e1, (i, seg)
        assert seg[0][1] - seg[0][0] > 4 * MC.LONGEST_TILE


def test_poly_q_tract_is_masked_with_short_flanks():
    rng = np.random.default_rng(4)
    W = MR.DEFAULT_WINDOW
    codes = rng.integers(0, 20, 200).astype(np.int8)
    codes[90:110] = 5   # Q
    for out in (MR.mask_subject(codes), mask.mask_subject(codes)):
        m = np.nonzero(out != codes)[0]
        assert (out[90:110] == 20).all()
        assert 90 - (W - 1) <= m.min() and m.max() <= 109 + (W - 1)


def test_defaults_spare_random_sequences():
    """A condition on the defaults: under 0.5 % of the residues of 400 random subjects at Swiss-Prot composition (0.15 % were
    measured when the defaults were chosen; 2.2 / 2.5 bits without SEG's trimming stage mask 2.2 %)."""
    rng = np.random.default_rng(3)
    total = masked = 0
    for _ in range(400):
        c = synthdb._residues(rng, int(rng.integers(50, 601)), synthdb.SPROT_COMPOSITION)
        total += len(c)
        masked += int((MR.mask_subject(c) != c).sum())
    assert masked < 0.005 * total, (masked, total)


def test_fixture_meets_its_conditions():
    """The end-to-end fixture under the CPU oracle, so that the GPU test cannot pass on a degenerate fixture."""
    f = MC.fixture()
    kind = f["kind"]
    assert ((kind == "D").sum(), (kind == "R").sum(), (kind == "B").sum()) == (MC.N_DECOYS, MC.N_RELATIVES, MC.N_BACKGROUND)
    assert (np.diff(f["lengths"]) >= 0).all() and len(f["query"]) == 240
    raw = O.scan(f["query"], f["chars"], f["offsets"], f["lengths"], simd=True)
    masked_chars, positions, subjects = MR.mask_block(f["chars"], f["offsets"], f["lengths"])
    msk = O.scan(f["query"], masked_chars, f["offsets"], f["lengths"], simd=True)
    assert (kind[O.topk(raw, 12)[1]] == "D").sum() >= 4
    assert (kind[O.topk(msk, 12)[1]] == "R").all()
    weakest = msk[kind == "R"].min()
    assert msk[kind == "D"].max() < weakest and msk[kind == "B"].max() < weakest
    assert (msk[kind == "R"] >= 0.8 * raw[kind == "R"]).all()
    assert subjects >= MC.N_DECOYS and positions >= 50 * MC.N_DECOYS


def test_align_refuses_malformed_masking_flags():
    def run(*flags):
        return subprocess.run([driver.ALIGN, "--query", "q.fa", "--db", "nowhere"] + list(flags), capture_output=True, text=True)

    for flags, what in ((("--maskWindow", "8"), "need --maskSubjects"), (("--maskTrigger", "1.5"), "need --maskSubjects"),
                        (("--maskExtend", "2.0"), "need --maskSubjects"),
                        (("--maskSubjects", "--maskWindow", "3"), "--maskWindow must lie in 4 .. 32"),
                        (("--maskSubjects", "--maskWindow", "33"), "--maskWindow must lie in 4 .. 32"),
                        (("--maskSubjects", "--maskWindow", "twelve"), "--maskWindow needs a number"),
                        (("--maskSubjects", "--maskWindow", "12.5"), "--maskWindow needs a number"),
                        (("--maskSubjects", "--maskTrigger", "2.3"), "--maskTrigger must not be above --maskExtend"),
                        (("--maskSubjects", "--maskTrigger", "x"), "--maskTrigger needs a number"),
                        (("--maskSubjects", "--maskExtend", "2.2bits"), "--maskExtend needs a number"),
                        (("--maskSubjects", "--maskExtend", "nan"), "--maskExtend needs a number")):
        r = run(*flags)
        assert r.returncode == 1 and what in r.stderr and "No GPU" not in r.stderr, (flags, r.stderr)
    # the option dump names the flags only when they were given
    r = run("--maskSubjects", "--maskWindow", "16")
    assert "maskSubjects: 1\n" in r.stdout and "maskWindow: 16\n" in r.stdout and "maskTrigger" not in r.stdout
    assert "mask" not in run().stdout
    h = subprocess.run([driver.ALIGN, "--help"], capture_output=True, text=True).stdout
    assert "Subject masking" in h and all(x in h for x in ("--maskSubjects", "--maskWindow", "--maskTrigger", "--maskExtend"))
