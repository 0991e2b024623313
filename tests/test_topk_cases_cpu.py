"""The top-K case file checked on its own (no GPU): `reference` against the oracle's top-K, the input families against what
their comments claim (through `walk_model`, the chunk walk of the small path), and the k of the select's digit-border cases.
These are conditions, not measurements: an input that misses its condition is a bug in tests/topk_cases.py."""
import numpy as np
import pytest

import oracle_lib as O
import topk_cases as T


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("family", sorted(T.FAMILIES))
def test_reference_equals_oracle_topk_on_integer_inputs(family, k):
    n = 20_000
    s = np.trunc(T.FAMILIES[family](n, k, 11))       # (mixed_floats: its integer parts, up to 1e9)
    assert s.dtype == np.float32 and np.all(s == s.astype(np.int32))
    rs, ri = T.reference(s, k)
    es, ei = O.topk(s.astype(np.int32), k)
    assert rs.tolist() == es.tolist() and ri.tolist() == ei.tolist()


def test_reference_pads_and_handles_empty_input():
    s = np.array([3, 9, 3, -1, 9], dtype=np.float32)
    rs, ri = T.reference(s, 8)
    assert rs.dtype == np.float32 and ri.dtype == np.int64
    assert rs.tolist() == [9, 9, 3, 3, -1, -1, -1, -1] and ri.tolist() == [1, 4, 0, 2, 3, -1, -1, -1]
    es, ei = O.topk(s.astype(np.int32), 8)
    assert rs.tolist() == es.tolist() and ri.tolist() == ei.tolist()
    rs, ri = T.reference(np.zeros(0, np.float32), 5)
    assert rs.tolist() == [-1.0] * 5 and ri.tolist() == [-1] * 5
    # fractional and huge values order as floats, ties by position
    s = np.array([0.5, -0.5, 1e9, 0.25, 0.5, -1e9, 16777218.0], dtype=np.float32)
    assert T.reference(s, 7)[1].tolist() == [2, 6, 0, 4, 3, 1, 5]


def test_walk_model_final_list_is_the_reference():
    """the model walks the chunks as the kernels do, so its final list must be the top-K itself"""
    for family, n, k, grid in (("mixed_floats", 30_000, 10, 4), ("two_levels_5000", 50_000, 32, 64), ("mostly_unscored", 9_000, 7, 1),
                               ("ascending_stairs_1000", 70_001, 31, 9), ("single_newcomer", 40_000, 2, 3)):
        s = T.FAMILIES[family](n, k, 3)
        w = T.walk_model(s, k, grid)
        rs, ri = T.reference(s, k)
        assert [e[1] for e in w.final_list] == ri.tolist() and [e[0] for e in w.final_list] == rs.tolist(), family


# grid -> n: full chunks only, the last one in the last workgroup, so that the workgroups' lists ascend with the workgroup
# index; 1 and 64 with many chunks per workgroup, 1 024 with two (4 M scores: what the model walks in about a second)
WALK_SIZES = {1: T.CHUNK * 150, 64: T.CHUNK * 64 * 5, 1024: T.CHUNK * 1024 * 2}


@pytest.mark.parametrize("grid,k", [(1, 1), (1, 2), (1, 10), (1, 32), (64, 1), (64, 10), (64, 31), (64, 32), (1024, 10)])
@pytest.mark.parametrize("family", ["ascending", "ascending_stairs_1000", "ascending_stairs_%d" % (T.CHUNK * 3 + 7)])
def test_ascending_inputs_land_at_the_kth_place_in_every_workgroup(family, grid, k):
    n = WALK_SIZES[grid] - 7
    s = T.FAMILIES[family](n, k, 0)
    w = T.walk_model(s, k, grid)
    nchunks = (n + T.CHUNK - 1) // T.CHUNK
    for b in range(grid):
        visited = len(range(b, nchunks, grid))
        assert visited >= 2                           # (the sizes above are chosen so)
        assert w.partial[b] >= 1, (family, grid, k, b, w.partial_chunks[b])
    if family == "ascending":                         # every chunk replaces the whole list: its last round lands at k-1
        assert all(c[1] == k and c[2] == 1 for rec in w.partial_chunks for c in rec)
        assert all(len(rec) == len(range(b, nchunks, grid)) for b, rec in enumerate(w.partial_chunks))
    if grid * k > T.CHUNK:
        assert w.final >= 1, (family, grid, k, w.final_chunks)
    assert [e[1] for e in w.final_list] == T.reference(s, k)[1].tolist()


@pytest.mark.parametrize("g", [1, 6])
def test_ascending_at_the_small_size_of_the_gpu_test(g):
    """n = 2048*5 + 1 is six chunks, and small_grid never launches more workgroups than chunks: with one workgroup every
    chunk but the last is a counted landing, with six there is none (the size allows no more)"""
    n, k = T.CHUNK * 5 + 1, 10
    w = T.walk_model(T.ascending(n), k, g)
    assert w.partial == ([5] if g == 1 else [0] * 6)
    assert [len(rec) for rec in w.partial_chunks] == ([6] if g == 1 else [1] * 6)


@pytest.mark.parametrize("grid", [1, 64, 1024])
def test_descending_enters_only_in_the_first_chunk(grid):
    n, k = T.CHUNK * 64 * 3 + 5, 10
    g = min(grid, (n + T.CHUNK - 1) // T.CHUNK)
    w = T.walk_model(T.descending(n), k, g)
    assert all(len(rec) == 1 and rec[0][0] == b for b, rec in enumerate(w.partial_chunks)) and sum(w.partial) == 0


@pytest.mark.parametrize("grid,n,k", [(1, T.CHUNK * 100 + 5, k) for k in (1, 2, 10, 32)] + [(64, T.CHUNK * 64 * 4 + 5, k) for k in (1, 2, 10, 32)]
                         + [(1024, T.CHUNK * 1024 * 2 + 5, 10)])   # (the 4 M-score walk: one k)
def test_single_newcomer_lands_once_per_later_chunk_of_workgroup_0(grid, n, k):
    s = T.single_newcomer(n, k, 5)
    w = T.walk_model(s, k, grid)
    nchunks = (n + T.CHUNK - 1) // T.CHUNK
    mine = list(range(0, nchunks, grid))
    rec = w.partial_chunks[0]
    assert [c[0] for c in rec] == mine and len(mine) >= 3
    assert rec[0][1:] == (k, 1)                       # the anchors and element 0 fill the list
    assert all(c[1:] == (1, 1) for c in rec[1:])      # every later chunk: one element enters, at k-1
    assert w.partial[0] == len(mine) - 1              # every landing but the last chunk's is followed by another chunk
    assert [e[1] for e in w.final_list] == T.reference(s, k)[1].tolist()


def test_small_grid_formula():
    assert T.small_grid(1, 256) == 1 and T.small_grid(T.CHUNK * 5 + 1, 256) == 6
    assert T.small_grid(T.CHUNK * 1024 * 3 + 5, 256) == 1024 and T.small_grid(T.CHUNK * 1024 * 3 + 5, 304) == 1024
    assert T.small_grid(T.CHUNK * 1024 * 3 + 5, 64) == 256 and T.small_grid(0, 256) == 1


# ---- the select's digit borders (topk_cases.BORDER_*: tests/test_gpu_topk.py runs the same list)

@pytest.mark.parametrize("family", ["all_equal", "two_levels_5000"])
def test_digit_border_cases_put_the_kth_element_where_they_say(family):
    s = T.FAMILIES[family](T.BORDER_N, 0, T.BORDER_SEED)
    for p in T.BORDER_POSITIONS:
        k = T.k_for_position(s, p)
        rs, ri = T.reference(s, k)
        assert ri[k - 1] == p and rs[k - 1] == s[p]
        assert (s == s[p]).sum() > 1000               # ... inside a large tie group
        if family == "all_equal":
            assert k == p + 1
    if family == "two_levels_5000":
        assert (s == 5.0).sum() == 5000 and s[T.reference(s, 5000)[1]].min() == 5.0 and T.reference(s, 5001)[0][-1] == 3.0
