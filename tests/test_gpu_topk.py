"""GPU: sw_topk's three paths (small, select, sort) and its unforced dispatch against tests/topk_cases.py's plain reference,
compared exactly — float equality on scores, integer equality on ids, over all k entries — on inputs aimed at the places
where the kernels can go wrong: the landing orders of small_merge (every chunk replacing the whole best list, a single
newcomer that barely enters), the (n, k) thresholds between the paths, the select's digit borders inside tie groups,
negative and non-integer scores, the argument checks, and the C++ driver's per-shard top-K with ties across shard borders.
tests/test_topk_cases_cpu.py checks, without a GPU, that the inputs do what their names say."""
import numpy as np
import pytest

import oracle_lib as O
import topk_cases as T
from gpu_util import gpu_modules

pytestmark = pytest.mark.gpu

ID_BASE = 1000            # ids need not equal positions
PATHS = ("small", "select", "sort", None)   # None: CUDASW4_AMD_TOPK unset, the product's own dispatch


def reaches(path, n, k):
    """does a call forced to `path` run that path?  (a forced small with k > 32 or n <= k, a forced select with k >= n,
    silently take another one)"""
    if path == "small":
        return k <= T.SMALL_K and n > k
    if path == "select":
        return n > k
    return True


def set_path(monkeypatch, path):
    if path is None:
        monkeypatch.delenv("CUDASW4_AMD_TOPK", raising=False)
    else:
        monkeypatch.setenv("CUDASW4_AMD_TOPK", path)   # read by sw_topk on every call


class Device:
    """scores on the device with ids arange(n) + ID_BASE, and one temp buffer for every k asked of it"""

    def __init__(self, scores):
        torch, self.capi, _ = gpu_modules()
        self.torch = torch
        self.scores = np.ascontiguousarray(scores, dtype=np.float32)
        self.n = len(self.scores)
        self.d_s = torch.from_numpy(self.scores).cuda() if self.n else None
        self.d_i = torch.arange(ID_BASE, ID_BASE + self.n, dtype=torch.int32, device="cuda") if self.n else None
        self.temp = None

    def run(self, ctx, k, stream=0, temp=None):
        torch, capi = self.torch, self.capi
        tb = capi.topk_temp_bytes(self.n, k)
        if temp is None:
            if self.temp is None or self.temp.numel() < tb:
                self.temp = torch.empty(max(tb, 1), dtype=torch.uint8, device="cuda")
            temp = self.temp
        out_s = torch.full((k,), -7.0, dtype=torch.float32, device="cuda")
        out_i = torch.full((k,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.topk(self.d_s.data_ptr() if self.n else 0, self.d_i.data_ptr() if self.n else 0, self.n, k, out_s.data_ptr(),
                 out_i.data_ptr(), temp.data_ptr(), temp.numel(), stream)
        torch.cuda.synchronize()
        return out_s.cpu().numpy(), out_i.cpu().numpy().astype(np.int64)

    def expect(self, k):
        rs, ri = T.reference(self.scores, k)
        return rs, np.where(ri >= 0, ri + ID_BASE, -1)

    def check(self, ctx, monkeypatch, k, paths=PATHS, what=""):
        es, ei = self.expect(k)
        ran = 0
        for path in paths:
            if not reaches(path, self.n, k):
                continue
            set_path(monkeypatch, path)
            gs, gi = self.run(ctx, k)
            bad = np.flatnonzero((gs != es) | (gi != ei))
            assert len(bad) == 0, "%s n=%d k=%d path=%s: %d entries differ, first at %d: got (%r, %d), expected (%r, %d)" % (
                what, self.n, k, path, len(bad), bad[0], gs[bad[0]], gi[bad[0]], es[bad[0]], ei[bad[0]])
            ran += 1
        return ran


@pytest.fixture(scope="module")
def ctx():
    torch, capi, _ = gpu_modules()
    c = capi.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()


# ---------------------------------------------------------------- landing orders of small_merge

LANDING_FAMILIES = ("ascending", "ascending_stairs_%d" % T.STAIRS[0], "ascending_stairs_%d" % T.STAIRS[1], "descending", "single_newcomer")


@pytest.mark.parametrize("k", [1, 2, 10, 31, 32])
@pytest.mark.parametrize("n", [T.CHUNK * 1024 * 3 + 5, T.CHUNK * 5 + 1])   # three chunks per workgroup at the largest grid; six chunks
@pytest.mark.parametrize("family", LANDING_FAMILIES)
def test_landing_orders(ctx, monkeypatch, family, n, k):
    """Inputs under which small_merge's rounds keep inserting after the first chunks: ascending orders replace the whole
    best list in every chunk of both kernels (the last round lands at k-1), the single newcomer lands at k-1 in every
    later chunk of workgroup 0, the descending order exercises the skip test.  The other paths get the same inputs."""
    dev = Device(T.FAMILIES[family](n, k, 7))
    assert dev.check(ctx, monkeypatch, k, what=family) == 4


# ---------------------------------------------------------------- thresholds between the paths

THRESHOLDS = ([(k + 1, k) for k in (1, 32, 33)] + [(k, k) for k in (1, 32, 33)] + [(n, 10) for n in (2047, 2048, 2049, 4097)]
              + [(n, k) for n in ((1 << 17) - 1, 1 << 17) for k in (33, n // 8, n // 8 + 1)]
              + [(300_000, k) for k in (1023, 1024, 1025)]       # topk_rank_emit_kernel -> hipCUB sort of the winners
              + [(5, 9), (40, 64), (33, 1030)])                  # k > n: (-1.0, -1) from index n on


@pytest.mark.parametrize("n,k", THRESHOLDS)
def test_path_thresholds(ctx, monkeypatch, n, k):
    """(n, k) on both sides of every switch in sw_topk and use_select — k = 32 | 33, n = k | k + 1, the chunk size, n = 2^17,
    k*8 = n, k = 1024 | 1025 — unforced and forced to every path the pair can reach."""
    rng = np.random.default_rng(n * 31 + k)
    inputs = {"two_levels": T.two_levels(max(1, n // 3))(n, k, n + k), "random": rng.integers(0, 50, n).astype(np.float32)}
    for name, s in inputs.items():
        dev = Device(s)
        ran = dev.check(ctx, monkeypatch, k, what=name)
        assert ran == 2 + (n > k) + (k <= T.SMALL_K and n > k)
        if k > n:
            gs, gi = dev.run(ctx, k)
            assert gs[n:].tolist() == [-1.0] * (k - n) and gi[n:].tolist() == [-1] * (k - n)


def test_empty_input_is_all_padding(ctx, monkeypatch):
    """n = 0 with k = 5: null inputs and a null temp buffer are allowed, the result is padding"""
    torch, capi, _ = gpu_modules()
    for path in PATHS:
        set_path(monkeypatch, path)
        assert capi.topk_temp_bytes(0, 5) == 0
        out_s = torch.full((5,), -7.0, dtype=torch.float32, device="cuda")
        out_i = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        ctx.topk(0, 0, 0, 5, out_s.data_ptr(), out_i.data_ptr(), 0, 0, 0)
        torch.cuda.synchronize()
        assert out_s.tolist() == [-1.0] * 5 and out_i.tolist() == [-1] * 5, path


# ---------------------------------------------------------------- the select's digit borders

@pytest.mark.parametrize("p", T.BORDER_POSITIONS)
@pytest.mark.parametrize("family", ["all_equal", "two_levels_5000"])
def test_select_digit_borders(ctx, monkeypatch, family, p):
    """The k-th element inside a tie group, at a position on either side of a border of the select's position digits
    (the low 10-bit digit; the top digit at 2^21): the three position passes decide it."""
    s = T.FAMILIES[family](T.BORDER_N, 0, T.BORDER_SEED)
    k = T.k_for_position(s, p)
    dev = Device(s)
    assert dev.expect(k)[1][k - 1] == p + ID_BASE
    paths = ("select", "sort") if k > 1024 else ("select", "sort", None)
    assert dev.check(ctx, monkeypatch, k, paths=paths, what=family) == len(paths)


@pytest.mark.parametrize("count_hi,lo,hi", [(5000, 3.0, 5.0), (5000, 1000.0, 1001.0), (500, 3.0, 5.0), (20, 3.0, 5.0)])
def test_select_takes_exactly_the_whole_tie_bin(ctx, monkeypatch, count_hi, lo, hi):
    """k = count_hi takes the upper level's bin whole (topk_pick sets skip_rest: no position passes; with 1000 | 1001 only at
    the second score digit), k - 1 stops inside it, k + 1 goes on into the lower level's ties."""
    dev = Device(T.two_levels(count_hi, lo, hi)(T.BORDER_N, 0, 5))
    for k in (count_hi - 1, count_hi, count_hi + 1):
        paths = ("select", "sort") if k > 1024 else PATHS
        assert dev.check(ctx, monkeypatch, k, paths=paths) == len(paths) - (k > T.SMALL_K and k <= 1024)


# ---------------------------------------------------------------- values

@pytest.mark.parametrize("n", [700, 200_000])
@pytest.mark.parametrize("family", ["mostly_unscored", "mixed_floats"])
def test_values(ctx, monkeypatch, family, n):
    """negative ties at the k-th place (the scan's -1 pre-fill, -2 marks) and floats of every sign and size: the key
    transform must order all of them and the emit kernels must give back the same bits"""
    for k in (10, 32, 100):
        dev = Device(T.FAMILIES[family](n, k, 13))
        assert dev.check(ctx, monkeypatch, k, what=family) == (4 if k <= T.SMALL_K else 3)


# ---------------------------------------------------------------- arguments

def untouched(out_s, out_i):
    return bool((out_s == -7).all()) and bool((out_i == -7).all())


def test_refused_and_empty_calls_launch_nothing(ctx, monkeypatch):
    torch, capi, _ = gpu_modules()
    n = 5000
    dev = Device(np.arange(n, dtype=np.float32))
    tb = capi.topk_temp_bytes(n, 10)
    temp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    out_s = torch.full((10,), -7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((10,), -7, dtype=torch.int32, device="cuda")
    args = (dev.d_s.data_ptr(), dev.d_i.data_ptr())
    outs = (out_s.data_ptr(), out_i.data_ptr())
    for path in PATHS:
        set_path(monkeypatch, path)
        for k in (0, -3):                                   # nothing asked for: returns at once
            ctx.topk(*args, n, k, *outs, temp.data_ptr(), tb, 0)
        with pytest.raises(capi.SwError):                    # more results than an int32 position can name
            ctx.topk(*args, 1 << 31, 10, *outs, temp.data_ptr(), tb, 0)
        with pytest.raises(capi.SwError):
            ctx.topk(*args, -1, 10, *outs, temp.data_ptr(), tb, 0)
        for o in ((0, outs[1]), (outs[0], 0), (0, 0)):       # null outputs
            with pytest.raises(capi.SwError):
                ctx.topk(*args, n, 10, *o, temp.data_ptr(), tb, 0)
        with pytest.raises(capi.SwError):                    # null inputs with n > 0
            ctx.topk(0, 0, n, 10, *outs, temp.data_ptr(), tb, 0)
        with pytest.raises(capi.SwError) as e:               # null temp
            ctx.topk(*args, n, 10, *outs, 0, tb, 0)
        assert e.value.code == -5, path
        torch.cuda.synchronize()
        assert untouched(out_s, out_i), path


def test_temp_buffer_one_byte_short(ctx, monkeypatch):
    """Every path refuses (SW_ERR_TEMP, -5) a buffer one byte short of what IT needs and works in one of exactly that
    size.  small: grid*k*8 with small_grid's grid; sort: sw_topk_temp_bytes(n, k) where the sort's layout is the largest
    of the three it covers (large n, small k); select: sw_topk_temp_bytes(k + 1, k), its layout being the largest there
    (large k: four arrays of k and the sort scratch of 64-bit keys, against two arrays of k + 1)."""
    torch, capi, _ = gpu_modules()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = []
    for n, k in ((T.CHUNK * 5 + 1, 10), (T.CHUNK * 2000, 32), (T.CHUNK * 1024 * 3 + 5, 31)):
        cases.append(("small", n, k, T.small_grid(n, cus) * k * 8))
    cases.append(("sort", 200_000, 10, capi.topk_temp_bytes(200_000, 10)))
    cases.append(("select", 200_000, 20_000, capi.topk_temp_bytes(20_001, 20_000)))
    assert capi.topk_temp_bytes(200_000, 10) > capi.topk_temp_bytes(201, 10) == T.SMALL_MAX_GRID * T.SMALL_K * 8
    assert capi.topk_temp_bytes(20_001, 20_000) > T.SMALL_MAX_GRID * T.SMALL_K * 8
    rng = np.random.default_rng(2)
    for path, n, k, need in cases:
        set_path(monkeypatch, path)
        dev = Device(rng.integers(0, 1000, n).astype(np.float32))
        es, ei = dev.expect(k)
        out_s = torch.full((k,), -7.0, dtype=torch.float32, device="cuda")
        out_i = torch.full((k,), -7, dtype=torch.int32, device="cuda")
        short = torch.empty(need, dtype=torch.uint8, device="cuda")
        with pytest.raises(capi.SwError) as e:
            ctx.topk(dev.d_s.data_ptr(), dev.d_i.data_ptr(), n, k, out_s.data_ptr(), out_i.data_ptr(), short.data_ptr(), need - 1, 0)
        assert e.value.code == -5, (path, n, k)
        torch.cuda.synchronize()
        assert untouched(out_s, out_i), (path, n, k)
        gs, gi = dev.run(ctx, k, temp=short)                 # exactly what the path needs
        assert np.array_equal(gs, es) and np.array_equal(gi, ei), (path, n, k)


def test_other_stream_gives_the_same_list(ctx, monkeypatch):
    torch, capi, _ = gpu_modules()
    stream = torch.cuda.Stream()
    for n, k in ((T.CHUNK * 40 + 3, 10), (200_000, 100), (3000, 3000)):
        dev = Device(T.mixed_floats(n, k, 4))
        es, ei = dev.expect(k)
        for path in PATHS:
            if not reaches(path, n, k):
                continue
            set_path(monkeypatch, path)
            a = dev.run(ctx, k)
            b = dev.run(ctx, k, stream=stream.cuda_stream)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (n, k, path)
            assert np.array_equal(b[0], es) and np.array_equal(b[1], ei), (n, k, path)


def test_back_to_back_calls_share_one_temp_buffer(ctx, monkeypatch):
    """the first call (larger n and k) leaves candidates, select state and sort scratch in the buffer: none of it may
    show in the second"""
    torch, capi, _ = gpu_modules()
    rng = np.random.default_rng(8)
    big = Device(rng.integers(0, 100_000, 300_000).astype(np.float32))
    small = Device(rng.integers(0, 30, 5000).astype(np.float32))      # lower scores than anything the first call left behind
    temp = torch.empty(max(capi.topk_temp_bytes(big.n, 1000), capi.topk_temp_bytes(small.n, 10)), dtype=torch.uint8, device="cuda")
    for first_path, first_k in (("select", 1000), ("sort", 1000), ("small", 32)):
        for path in PATHS:
            set_path(monkeypatch, first_path)
            gs, gi = big.run(ctx, first_k, temp=temp)
            es, ei = big.expect(first_k)
            assert np.array_equal(gs, es) and np.array_equal(gi, ei), first_path
            set_path(monkeypatch, path)
            gs, gi = small.run(ctx, 10, temp=temp)
            es, ei = small.expect(10)
            assert np.array_equal(gs, es) and np.array_equal(gi, ei), (first_path, path)


# ---------------------------------------------------------------- through the C++ driver

def test_driver_shards_with_ties_across_borders_and_the_kth_place():
    """Eight shards of one GPU over ~600 short subjects with many exact duplicates: every shard runs its own sw_topk (with
    num_top above its subject count: the n == k sort path) and the host merges the lists.  Expected: the oracle's scores
    ordered by (score descending, id ascending), truncated to min(k, n_total)."""
    from cudasw4_amd import driver
    rng = np.random.default_rng(23)
    alphabet = b"ARNDCQEGHILKMFPSTWYV"
    families = [rng.integers(0, 20, int(l)).astype(np.int8) for l in (64, 64, 80, 80, 80, 96, 96, 48, 48, 110)]
    copies = (90, 70, 50, 40, 30, 20, 10, 5, 3, 2)
    seqs = [f for f, c in zip(families, copies) for _ in range(c)]
    seqs += [rng.integers(0, 20, int(l)).astype(np.int8) for l in rng.integers(30, 120, 280)]
    seqs.sort(key=len)                                     # (stable: the copies of a family stay together)
    chars, offsets, lengths = O.make_db(seqs)
    n_total = len(seqs)
    query = families[0]                                    # 90 subjects tie at the top, family 1 (same length) lies among them
    expect = O.scan(query, chars, offsets, lengths, simd=True)
    d = driver.Driver(devices=[0] * 8, num_top=10, kinds=(0, 0, 3, 3))
    d.db_from_arrays(chars, offsets, lengths)
    assert d.num_gpus() == 8 and d.num_sequences() == n_total
    letters = bytes(alphabet[c] for c in query)
    first = True
    for k in (33, 1, n_total + 5, 10, n_total, 32):
        d.set_num_top(k)
        r = d.scan(letters)
        es, ei = T.reference(expect.astype(np.float32), k)
        m = min(k, n_total)
        assert len(r["scores"]) == m, k
        assert r["scores"].tolist() == es[:m].astype(np.int64).tolist(), k
        assert r["ids"].tolist() == ei[:m].tolist(), k
        if first:                                          # the input does what the docstring says
            first = False
            shard_of = np.empty(n_total, dtype=np.int64)
            sizes = []
            for g in range(8):
                _, ids = d.last_scores(g)
                shard_of[ids] = g
                sizes.append(len(ids))
            assert sum(sizes) == n_total and all(0 < x < n_total for x in sizes)     # n_total and n_total + 5 exceed every shard
            top = np.flatnonzero(expect == expect.max())
            assert len(top) >= 90 and len(set(shard_of[top].tolist())) >= 2          # the top tie group straddles shard borders
            ranked = T.reference(expect.astype(np.float32), n_total)[0]
            assert all(ranked[kk - 1] == ranked[kk] for kk in (1, 10, 32, 33))       # ... and every k-th place
    d.close()
