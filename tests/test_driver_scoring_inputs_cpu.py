"""CPU: the inputs of tests/test_gpu_driver_scoring.py reach what those tests claim — asserted with the oracle alone, for
every scoring: scores on both sides of the packed kinds' limits and inside the room below them in which the kernels flag
early (1536 below 2048, 12 500 below 25 000), and best hits of the two shortest queries that straddle a window boundary of
a giant subject.  If a condition fails here, the inputs are what has to change."""
import numpy as np
import pytest

import align_ref as A
import oracle_lib as O
import test_gpu_driver_scoring as S

pytestmark = []     # (the module imported above is marked gpu; this one runs everywhere)


def test_db_shape():
    lens = S.inputs()["db"][2]
    assert (np.diff(lens) >= 0).all() and lens[0] == 0 and lens[1] == 1
    assert 550 <= int(((lens >= 20) & (lens <= 1280)).sum()) <= 700
    assert 25 <= int(((lens > 1280) & (lens <= 8000)).sum()) <= 40
    assert lens[-4:].tolist() == [8100, 12000, 20000, 35000]
    assert any((s == 20).any() for s in S.inputs()["seqs"] if len(s) <= 1280)
    assert [len(q) for q in S.inputs()["queries"]] == [48, 144, 300, 1000, 2005, 5478]


def test_default_gaps_come_from_the_product():
    assert S.default_gaps(62) == (-11, -1)
    for mat in (45, 50, 80):
        gop, gex = S.default_gaps(mat)
        assert gop < gex < 0


@pytest.mark.parametrize("name", S.NAMES)
def test_scores_on_both_sides_of_the_packed_limits(name):
    lens = S.inputs()["db"][2]
    packed = lens <= 8000
    # fp16 configuration: its five queries
    near = over = 0
    for qi in range(5):
        e = S.oracle_scan(name, qi)[packed]
        near += int(((e >= 2048 - 1536) & (e < 2048)).sum())
        over += int((e >= 2048).sum())
    assert near >= 5 and over >= 5, (name, near, over)
    # int16 configuration: the long query
    e = S.oracle_scan(name, 5)[packed]
    assert int((e >= 25000).sum()) >= 1 and int(((e >= 12500) & (e < 25000)).sum()) >= 3, (name, np.sort(e)[-8:])


@pytest.mark.parametrize("name", S.NAMES)
def test_best_hits_of_the_shortest_queries_straddle_a_window_boundary(name):
    mat, gop, gex = S.scoring(name)
    m = S.oracle_matrix(mat)
    lens = S.inputs()["db"][2]
    for qi in (0, 1):
        expect = S.oracle_scan(name, qi)
        best = int(O.topk(expect, 1)[1][0])
        assert lens[best] > 8000, (name, qi, best, int(lens[best]))
        codes = S.query_codes(name, qi)
        cw = S.window_stride(len(codes), m, gop, gex)
        if cw is None:
            assert min(-gop, -gex) == 0 and name == "b62_20_0"      # the documented span formula has cost 0: no windows
            continue
        C, W4 = cw
        assert lens[best] > C + W4       # the engine cuts this subject
        r, _ = A.align(codes, S.inputs()["seqs"][best], m, gop, gex)
        assert r["status"] == A.OK and r["score"] == int(expect[best])
        assert any(r["s_begin"] < k * C < r["s_end"] for k in (1, 2)), (name, qi, C, r)


def test_the_scoring_grid_reaches_the_scoring_dependent_decisions():
    by = {n: S.scoring(n) for n in S.NAMES}
    assert any(gop > gex for _, gop, gex in by.values())                      # no pipelines
    assert any(min(-gop, -gex) == 0 for _, gop, gex in by.values())           # no window span
    assert any(-gex > 12 for _, gop, gex in by.values())                      # fp16 falls back to fp32
    assert {-gex for _, gop, gex in by.values()} >= {1, 2, 5}                 # fp16 frame periods 1024, 512 and 128
    assert len({m for m, _, _ in by.values()}) == 5
