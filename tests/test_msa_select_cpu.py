"""CPU: the selection of MSA rows on hand-worked rows (tests/msa_select_ref.py), cudasw4_amd/msa.py against
that reference, a guard that the shared case set exercises every state and rung, and the refusals of the new `align` flags
— no device."""
import subprocess

import numpy as np
import pytest

import msa_ref as M
import msa_select_ref as R

N = M.NONE


def worked_example():
    """qlen 20, the master all code 0; B (second): codes 1 at 0-9, then 0 0 0 0 2 2 2 2 2 2; A (first): NONE at 0-9, then B's"""
    master = np.zeros(20, dtype=np.uint8)
    b = np.array([1] * 10 + [0, 0, 0, 0, 2, 2, 2, 2, 2, 2], dtype=np.uint8)
    a = b.copy()
    a[:10] = N
    return np.stack([a, b, master])


def test_worked_example():
    rows = worked_example()
    # rung 40: A is 40 % identical to the master (skipped), B 20 % (kept); rung 100: A's ten residues all repeat B's
    trace = []
    state, depth, counts = R.select(rows, D=10, ladder=(40, 100), trace=trace)
    assert state.tolist() == [4, 1, 1] and depth.tolist() == [2] * 20 and counts == [1, 0, 0, 1] and trace == [(0, 1)]
    # (comparing A only with higher-ranked kept rows would keep it: nothing ranks above A but the master)
    assert not M.similar(M.ident(rows[2], rows[0]), 10, 100) and M.similar(M.ident(rows[1], rows[0]), 10, 100)
    state, depth, counts = R.select(rows, D=10, ladder=(100,))
    assert state.tolist() == [1, 1, 1] and depth.tolist() == [2] * 10 + [3] * 10 and counts == [2, 0, 0, 0]
    assert R.select(rows, C=60, ladder=(100,))[0].tolist() == [2, 1, 1]
    assert R.select(rows, Q=30, ladder=(100,))[0].tolist() == [1, 3, 1]
    assert R.levels(rows, (40, 100)).tolist() == [[0, 2, 1], [1, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize("P", [1, 50, 94, 100])
def test_no_diff_is_the_greedy_filter(P):
    for seed, (qlen, n) in enumerate([(33, 40), (64, 65), (150, 90)]):
        case = M.random_case(np.random.default_rng(100 * P + seed), qlen, n, families=3, copy_rate=0.06)
        rows = R.case_rows(case)
        keep, purged = M.greedy(rows, P)
        state, _, counts = R.select(rows, ladder=(P,))
        assert (state == 1).astype(int).tolist() == keep.tolist()
        assert counts == [int(keep[:n].sum()), 0, 0, purged] and purged > 0


def test_threshold_edges():
    # coverage, qlen 50: 25 aligned columns pass C = 50 (codes 20 and gaps: a code 20 is an aligned column, a gap is not)
    master = np.full(50, N, dtype=np.uint8)
    for aligned, passes in ((25, True), (24, False)):
        row = np.array([3] * (aligned - 2) + [20, 20] + [M.GAP] * 5 + [N] * (45 - aligned), dtype=np.uint8)
        assert R.pairs(row) == aligned
        assert R.select(np.stack([row, master]), C=50)[0].tolist() == [1 if passes else 2, 0]
    # query identity, res 50: 10 identities with the master pass Q = 20, 9 do not
    master = np.zeros(60, dtype=np.uint8)
    for same, passes in ((10, True), (9, False)):
        row = np.array([0] * same + [5] * (50 - same) + [20] * 4 + [M.GAP] * 3 + [N] * 3, dtype=np.uint8)
        rows = np.stack([row, master])
        assert M.residues(rows).tolist() == [50, 60] and M.ident(master, row) == same
        state, _, counts = R.select(rows, Q=20)
        assert state.tolist() == [1 if passes else 3, 1] and counts == [int(passes), 0, int(not passes), 0]
    # Q is tested behind C, and a hit without residues is neither
    row = np.array([5] * 10 + [N] * 50, dtype=np.uint8)
    empty = np.array([20] * 40 + [N] * 20, dtype=np.uint8)
    assert R.select(np.stack([row, empty, master]), C=50, Q=20)[0].tolist() == [2, 0, 1]


def guard_runs():
    for qlen, n, f in R.GUARD_CASES:
        for seed in R.GUARD_SEEDS:
            rows = R.case_rows(R.guard_case(qlen, n, f, seed))
            yield rows, R.ident_matrix(rows)


def test_not_needed_is_permanent_and_a_deep_D_never_thins_for_need():
    p = R.GUARD_PARAMS
    for rows, idents in guard_runs():
        n = len(rows) - 1
        state, depth, _ = R.select(rows, idents=idents, **p)
        # re-testing every thinned row after the last rung changes nothing: it is still not needed, or still similar to a
        # kept row at the last rung
        res = M.residues(rows)
        kept = [g for g in range(n + 1) if state[g] == 1]
        for h in np.flatnonzero(state == 4):
            blocked = any(M.similar(idents[h, g], res[h], p["ladder"][-1]) for g in kept)
            assert blocked or not R.needed(rows[h], depth, p["D"])
        # D >= n + 1: every candidate is needed at every moment, so the states are those of D = 0
        deep = R.select(rows, idents=idents, **dict(p, D=n + 1))
        flat = R.select(rows, idents=idents, **dict(p, D=0))
        assert deep[0].tolist() == flat[0].tolist() and deep[1].tolist() == flat[1].tolist() and int(depth.max()) <= n + 1


def test_the_case_set_is_not_vacuous():
    """asserted on the reference alone: every state occurs, rows are kept in at least three rungs, and a row is kept after a
    lower-ranked one"""
    states, rungs, after = set(), set(), False
    for rows, idents in guard_runs():
        trace = []
        state, _, _ = R.select(rows, idents=idents, trace=trace, **R.GUARD_PARAMS)
        states |= set(state.tolist())
        rungs |= {t for t, _ in trace}
        order = [h for _, h in trace]
        after = after or any(later < earlier for earlier, later in zip(order, order[1:]))
    assert states == {0, 1, 2, 3, 4} and len(rungs) >= 3 and after


def test_python_module_against_reference():
    from cudasw4_amd import msa
    assert msa.default_ladder() == [20, 30, 40, 50, 60, 70, 80, 90] and msa.default_ladder(35) == [20, 30, 35] and msa.default_ladder(20) == [20]
    variants = [R.GUARD_PARAMS, dict(C=0, Q=0, D=0, ladder=(94,)), dict(C=0, Q=0, D=1, ladder=(50, 100)),
                dict(C=60, Q=30, D=1000, ladder=tuple(range(10, 90, 5)))]
    for rows, idents in guard_runs():
        for p in variants:
            want = R.select(rows, idents=idents, **p)
            got = msa.select_rows(rows, p["C"], p["Q"], p["D"], p["ladder"])
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2] == want[2], p
    rows = worked_example()
    assert msa.select_rows(rows, diff=10, ladder=(40, 100))[0].tolist() == [4, 1, 1]
    rows[2] = N    # no master
    assert msa.select_rows(rows, diff=10, ladder=(40, 100))[0].tolist() == R.select(rows, D=10, ladder=(40, 100))[0].tolist() == [1, 1, 0]
    for bad in (dict(min_coverage=101), dict(min_query_identity=-1), dict(diff=-1), dict(ladder=()), dict(ladder=(50, 50)),
                dict(ladder=(0,)), dict(ladder=(101,)), dict(ladder=tuple(range(1, 18)))):
        with pytest.raises(ValueError):
            msa.select_rows(rows, **bad)


def test_c_abi_is_declared():
    import os
    import re
    from cudasw4_amd import capi, driver
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "cudasw4_amd_msa_select.h")).read()
    declared = set(re.findall(r"\b(sw_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.MSA_SELECT_EXPORTS) == {"sw_msa_select"} and "sw_msa_select" not in capi.EXPORTS
    assert "SW_MSA_SELECT_MAX_HITS (1 << 14)" in header and capi.MSA_SELECT_MAX_HITS == 1 << 14
    import ctypes
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "sw_msa_select")
    assert "swdrv_hit_msa_select" in driver.EXPORTS


# ---- the command line: refusals before any device is opened -----------------------------------------------------------------

PERCENT = " must be an integer in 1 .. 100"
NEED = "--msaMinCoverage / --msaMinQueryIdentity / --msaDiff / --msaDiffLadder need --outMsa"
LADDER = "--msaDiffLadder must be 1 .. 16 strictly ascending integers in 1 .. 100"


@pytest.mark.parametrize("args,message", [
    (["--outMsa", "P", "--msaMinCoverage", "0"], "--msaMinCoverage" + PERCENT),
    (["--outMsa", "P", "--msaMinCoverage", "101"], "--msaMinCoverage" + PERCENT),
    (["--outMsa", "P", "--msaMinCoverage", "5x"], "--msaMinCoverage" + PERCENT),
    (["--outMsa", "P", "--msaMinQueryIdentity", "0"], "--msaMinQueryIdentity" + PERCENT),
    (["--outMsa", "P", "--msaMinQueryIdentity", "100.5"], "--msaMinQueryIdentity" + PERCENT),
    (["--outMsa", "P", "--msaDiff", "0"], "--msaDiff must be an integer of at least 1"),
    (["--outMsa", "P", "--msaDiff", "-3"], "--msaDiff must be an integer of at least 1"),
    (["--outMsa", "P", "--msaDiff", "many"], "--msaDiff must be an integer of at least 1"),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "20,20"], LADDER),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "40,30"], LADDER),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "0,30"], LADDER),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "30,101"], LADDER),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "30,,40"], LADDER),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "30,4o"], LADDER),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", ""], LADDER),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", ",".join(str(p) for p in range(1, 18))], LADDER),
    (["--outMsa", "P", "--msaDiffLadder", "30,40"], "--msaDiffLadder needs --msaDiff"),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "30,40", "--msaMaxIdentity", "90"],
     "--msaDiffLadder cannot be combined with --msaMaxIdentity"),
    (["--msaMinCoverage", "50"], NEED),
    (["--msaMinQueryIdentity", "20"], NEED),
    (["--msaDiff", "5"], NEED),
    (["--msaDiff", "5", "--msaDiffLadder", "30,40"], NEED),
    (["--outMsa", "P", "--msaMinCoverage", "50", "--top", "16385"], "take --top up to 16384"),
    (["--outMsa", "P", "--msaDiff", "5", "--top", "20000"], "take --top up to 16384"),
    (["--outMsa", "P", "--msaMinCoverage", "50", "--interactive"], "cannot be combined with --interactive"),
    (["--outMsa", "P", "--msaMinQueryIdentity", "50", "--interactive"], "cannot be combined with --interactive"),
    (["--outMsa", "P", "--msaDiff", "5", "--msaDiffLadder", "30,40", "--interactive"], "cannot be combined with --interactive"),
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
    for flag in ("--msaMinCoverage C", "--msaMinQueryIdentity Q", "--msaDiff D", "--msaDiffLadder p0,p1,..."):
        assert flag in text
    q = tmp_path / "q.fa"
    q.write_text(">q\nMKTAYIAKQRQISF\n")
    base = [driver.ALIGN, "--query", str(q), "--db", str(tmp_path / "nodb"), "--outMsa", "P"]
    r = subprocess.run(base + ["--msaMinCoverage", "50", "--msaMinQueryIdentity", "2x", "--msaDiff", "7", "--msaDiffLadder", "30,60"],
                       capture_output=True, text=True, timeout=60)
    assert "msaMinCoverage: 50\nmsaMinQueryIdentity: 2x\nmsaDiff: 7\nmsaDiffLadder: 30,60\n" in r.stdout
    r = subprocess.run(base + ["--msaDiff", "7"], capture_output=True, text=True, timeout=60)
    assert "msaDiff: 7\n" in r.stdout and "msaDiffLadder" not in r.stdout and "msaMinCoverage" not in r.stdout
    r = subprocess.run(base + ["--msaMaxIdentity", "90"], capture_output=True, text=True, timeout=60)
    assert "outMsa: P\n" in r.stdout and "msaDiff" not in r.stdout and "msaMin" not in r.stdout
