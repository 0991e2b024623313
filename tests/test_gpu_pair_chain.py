"""GPU: pair chains of the packed multi-stripe sw_scan_kernel on 16-lane groups (sw_dp_kernel.hpp: "Pair chains").

A workgroup claims up to C batches at once (CUDASW4_AMD_CHAIN) and each of its groups walks its C pairs of subjects as one
virtual subject per stripe: pair k, four separator columns, pair k + 1.  The lanes are handed over in four blocks of four at
quad boundaries: their maxima become pair k's, their state that of a fresh subject.  What can go wrong lies at the borders:
state leaking through a reset (a homolog right before an unrelated subject), a pair's maxima (kept in the scratch between the
stripes), ragged and empty subjects inside a chain (a pair takes at least twelve columns), groups without a subject B or
without any subject, the last claim's shorter chain, the frame lowering falling between the resets of one border (subjects of
504 residues: asserted below), and subjects that reach the fp16 limit at every place of a chain.

Every case runs with C = 1, 2, 3 and 4 and CUDASW4_AMD_CHAIN_ALL=1, which lifts the rule that only launches with more than
C x grid batches left chain; test_chains_then_single_claims runs the rule itself, with the default C.  The subjects the packed kernel flags are re-scored in 32 bits as the callers do; the scores
must then equal the CPU oracle's, and so each other's for every C."""
import numpy as np
import pytest

import oracle_lib as O
from gpu_util import gpu_modules

pytestmark = pytest.mark.gpu

PART = 33           # a partition of 16-lane groups
CHAINS = (1, 2, 3, 4)     # 3 is the default
GAPS = [(-11, -1), (-12, -5)]    # as tests/test_gpu_uniform_frame.py
# query length -> (rows per lane, stripes): 850 = two stripes of 27 rows (three waves per SIMD), 1500 = two of 47 rows (two
# waves; the last row's class is not 0)
QUERIES = {850: (27, 2), 1500: (47, 2)}


def _index(batch, group, half):
    return 32 * batch + 2 * group + half


def _mutated(rng, seg, every):
    s = seg.copy()
    s[::every] = rng.integers(0, 20, len(s[::every]))
    return s


def _uniform(rng, q, length):
    """257 subjects of one length: nine batches (the last claim of C = 2 and of C = 4 takes one), the last batch one subject
    (fifteen groups without any, one without a subject B).  Every third subject carries a mutated piece of the query."""
    seqs = []
    for k in range(257):
        s = rng.integers(0, 20, length).astype(np.int8)
        if k % 3 == 0:
            n = int(rng.integers(40, 200))
            at_q = int(rng.integers(0, len(q) - n + 1))
            at = int(rng.integers(0, length - n + 1))
            s[at:at + n] = _mutated(rng, q[at_q:at_q + n], 4 + k % 3)
        seqs.append(s)
    return seqs


def _ragged(rng, q):
    """339 subjects: eleven batches (the last claim takes C - 1 = 3 of them with C = 4, one with C = 2), the last batch nine
    pairs, a single subject and six empty groups.  Batch B is handed out as number 10 - B: batches 10, 9, 8, 7 are the first
    chain of C = 4, batches 6, 5, 4, 3 the second one."""
    n = 339
    lens = rng.integers(330, 600, n)
    lens[lens % 4 == 0] += 1                       # no multiples of 4 among the ordinary ones
    seqs = [rng.integers(0, 20, int(l)).astype(np.int8) for l in lens]

    def put(batch, group, half, s):
        seqs[_index(batch, group, half)] = np.asarray(s, dtype=np.int8)

    # lengths 0 .. 3 inside a chain, next to ordinary subjects (batches 9 and 8: the middle of the first chain of C = 4)
    for batch, group, (la, lb) in ((9, 3, (0, 3)), (8, 3, (1, 2)), (9, 2, (2, 0)), (8, 1, (3, 1))):
        put(batch, group, 0, rng.integers(0, 20, la))
        put(batch, group, 1, rng.integers(0, 20, lb))
    # a whole wave (groups 4 .. 7) of subjects of at most three residues, and one (groups 8 .. 11) of empty ones: pairs that
    # take the minimum of twelve columns
    for group in range(4, 8):
        put(8, group, 0, rng.integers(0, 20, group % 4))
        put(8, group, 1, rng.integers(0, 20, (group + 1) % 4))
    for group in range(8, 12):
        put(9, group, 0, [])
        put(9, group, 1, [])
    # homologs directly BEFORE unrelated subjects of the same group: batch 6 opens the chain of batches 6, 5 (C = 2) and
    # 6, 5, 4, 3 (C = 4); the subjects of the same groups in batch 5 (and 4) stay random
    put(6, 2, 0, _mutated(rng, q[100:250], 7))                      # a moderate hit
    put(6, 2, 1, np.concatenate([rng.integers(0, 20, 80), _mutated(rng, q[300:700], 9), rng.integers(0, 20, 57)]))
    # subjects that reach the fp16 limit (near copies of 590 residues of the query), first, in the middle and last in a chain
    big = lambda: np.concatenate([_mutated(rng, q[:590], 11), rng.integers(0, 20, 7)])   # noqa: E731
    put(6, 5, 0, big())      # first (C = 2 and C = 4)
    put(5, 6, 1, big())      # the middle of C = 4, the end of C = 2
    put(3, 7, 0, big())      # last
    put(10, 0, 1, big())     # first pair of the launch's first chain, in the partial batch
    return seqs


def _tail(rng, q):
    """615 subjects, twenty batches, for ONE workgroup (CUDASW4_AMD_GRID_CAP=1): more than sixteen batches per workgroup, so the
    launcher chains, and the kernel's tail rule makes the first claims chains and the last ones single batches.  Ragged
    lengths, an odd count, a homolog before unrelated subjects and near copies beyond the fp16 limit in a chain and in a
    single claim (batch B is handed out as number 19 - B)."""
    lens = rng.integers(330, 600, 615)
    seqs = [rng.integers(0, 20, int(l)).astype(np.int8) for l in lens]
    big = lambda: np.concatenate([_mutated(rng, q[:590], 11), rng.integers(0, 20, 7)])   # noqa: E731
    seqs[_index(19, 1, 0)] = _mutated(rng, q[100:250], 7)     # first pair of the first chain
    seqs[_index(18, 3, 1)] = big()                            # inside a chain
    seqs[_index(12, 9, 0)] = big()
    seqs[_index(1, 4, 0)] = big()                             # a single claim near the end (C = 3: batches 1 and 0)
    seqs[_index(0, 4, 1)] = _mutated(rng, q[300:500], 6)
    seqs[_index(17, 6, 0)] = np.zeros(0, dtype=np.int8)
    seqs[_index(16, 6, 1)] = rng.integers(0, 20, 3).astype(np.int8)
    return seqs


BUILDERS = {"uniform512": lambda rng, q: _uniform(rng, q, 512), "uniform504": lambda rng, q: _uniform(rng, q, 504), "ragged": _ragged}
ALL_BUILDERS = dict(BUILDERS, tail=_tail)
_cache = {}


def _case(name, qlen):
    """DB and oracle scores of a case, computed once for every kind, gap setting and chain length"""
    key = (name, qlen)
    if key not in _cache:
        rng = np.random.default_rng(len(name) * 1000 + qlen)
        q = rng.integers(0, 20, qlen).astype(np.int8)
        seqs = ALL_BUILDERS[name](rng, q)
        chars, offsets, lengths = O.make_db(seqs)
        expect = {g: O.scan(q, chars, offsets, lengths, gop=g[0], gex=g[1], simd=True) for g in GAPS}
        _cache[key] = (q, chars, offsets, lengths, expect)
    return _cache[key]


def _region_bytes(columns):
    """scratch bytes of one workgroup of 16-lane groups for walks of that many columns: 16 groups x blocks x 96 words"""
    steps = (columns + 15 + 3) // 4 * 4
    lcap = (steps + 15) // 16 * 16 + 16
    blocks = (lcap + 31) // 32 + 3
    return 16 * blocks * 96 * 4


def _chain_bytes(maxlen, c):
    """... for chains of c pairs: the virtual subject (every pair but the last in whole quads, four separator columns each),
    and seven words of maxima per lane"""
    if c == 1:
        return _region_bytes(maxlen)
    pair = max(12, (maxlen + 3) // 4 * 4)
    return _region_bytes((c - 1) * (pair + 4) + maxlen) + 16 * 7 * 16 * 4


def _period(kind_name, gex):
    """the uniform frame's period in steps (sw_api.hip: offs_possible, capped by the level table): the frame is lowered behind
    every step whose global anti-diagonal 16 * stripe + step + 1 is a multiple of it"""
    a = -gex
    room = 1536 if kind_name == "f16x2" else 12500
    k = 1 << 21
    while k >= 64 and a * (k + 3 * 16 + 16) > room:
        k >>= 1
    if kind_name == "i16x2":
        k = min(k, 2048)
    return min(k, 256)


def _lowering_meets_a_border(length, c, stripes, period):
    """uniform subjects: does a lowering fall behind the separator quad of a border of the chain or behind one of the three
    quads between its four resets (quads E / 4 ... E / 4 + 3, E the virtual column behind the pair)?"""
    pair = max(12, (length + 3) // 4 * 4)
    for k in range(c - 1):
        end = k * (pair + 4) + pair
        for s in range(stripes):
            for quad in range(end // 4, end // 4 + 4):
                if (16 * s + 4 * quad + 4) % period == 0:
                    return True
    return False


def _upload(torch, chars, offsets, lengths):
    """(the subjects' order is the case's, not ascending by length: uploaded as they are, with slack behind the letters so
    that 4-byte letter loads never leave the allocation)"""
    d_chars = torch.full((len(chars) + 32,), 20, dtype=torch.int8, device="cuda")
    d_chars[:len(chars)].copy_(torch.from_numpy(chars))
    return d_chars, torch.from_numpy(offsets.view(np.int64).copy()).cuda(), torch.from_numpy(lengths.copy()).cuda()


def _scan(torch, capi, ctx, kind, dev, n, maxlen, gop, gex, expect, temp, what):
    """one packed launch and the 32-bit re-score of what it flagged -> (final scores, flagged positions)"""
    d_chars, d_offsets, d_lengths = dev
    scores = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    ids = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ovf_pos = torch.zeros(n, dtype=torch.int32, device="cuda")
    ovf_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.scan_partition(kind, PART, d_chars.data_ptr(), d_offsets.data_ptr(), d_lengths.data_ptr(), 0, n, maxlen,
                       gop, gex, scores.data_ptr(), ids.data_ptr(), 0, ovf_pos.data_ptr(), ovf_cnt.data_ptr(), 1,
                       temp.data_ptr(), temp.numel(), 0)
    torch.cuda.synchronize()
    nflag = int(ovf_cnt.item())
    flagged = np.sort(ovf_pos.cpu().numpy()[:nflag])
    packed = scores.cpu().numpy().astype(np.int32)
    print("%s: %d of %d flagged, highest score %d" % (what, nflag, n, expect.max()))
    # flagged only near the kind's limit (the bound of tests/test_gpu_address_stream.py), each subject once
    limit = 2048 if kind == capi.KIND_F16X2 else 25000
    assert len(np.unique(flagged)) == nflag
    assert (expect[flagged] >= limit - (-gex) * (2048 + 2 * 64 + 12)).all(), (what, flagged, expect[flagged])
    ok = np.ones(n, dtype=bool)
    ok[flagged] = False
    np.testing.assert_array_equal(packed[ok], expect[ok], err_msg="packed scores, " + what)
    if nflag:
        rtemp = torch.empty(max(16, ctx.scan_temp_bytes(capi.KIND_I32, -1, nflag, maxlen)), dtype=torch.uint8, device="cuda")
        ctx.rescore_overflow(capi.KIND_I32, ovf_pos.data_ptr(), ovf_cnt.data_ptr(), nflag, d_chars.data_ptr(), d_offsets.data_ptr(),
                             d_lengths.data_ptr(), maxlen, gop, gex, scores.data_ptr(), ids.data_ptr(), 0, rtemp.data_ptr(), rtemp.numel(), 0)
        torch.cuda.synchronize()
    got = scores.cpu().numpy().astype(np.int32)
    np.testing.assert_array_equal(got, expect, err_msg=what)
    np.testing.assert_array_equal(ids.cpu().numpy(), np.arange(n))
    return got, flagged


@pytest.mark.parametrize("name", sorted(BUILDERS))
@pytest.mark.parametrize("qlen", sorted(QUERIES))
@pytest.mark.parametrize("kind_name", ["f16x2", "i16x2"])
@pytest.mark.parametrize("gop,gex", GAPS)
def test_pair_chain_scores(monkeypatch, name, qlen, kind_name, gop, gex):
    torch, capi, search = gpu_modules()
    kind = capi.KIND_F16X2 if kind_name == "f16x2" else capi.KIND_I16X2
    q, chars, offsets, lengths, expects = _case(name, qlen)
    expect = expects[(gop, gex)]
    n, maxlen = len(lengths), int(lengths.max())
    nbatches = (n + 31) // 32
    assert maxlen > 320       # longer than what multi-stripe queries stream: sw_scan_kernel
    if name == "ragged":
        assert (expect >= 2048).sum() >= 4     # the planted near copies are beyond the fp16 limit
        # the unrelated subjects behind the homologs of batch 6, group 2
        assert expect[_index(6, 2, 0)] > 300 and expect[_index(6, 2, 1)] > 900
        assert max(expect[_index(5, 2, 0)], expect[_index(5, 2, 1)], expect[_index(4, 2, 0)], expect[_index(4, 2, 1)]) < 150
    monkeypatch.setenv("CUDASW4_AMD_CHAIN_ALL", "1")
    dev = _upload(torch, chars, offsets, lengths)
    results = {}
    for c in CHAINS:
        if name == "uniform504" and c > 1:
            # the frame is lowered between the resets of the first border: behind quad 127, whose top resets lanes 0 .. 3
            assert _lowering_meets_a_border(504, c, QUERIES[qlen][1], _period(kind_name, gex)), (c, _period(kind_name, gex))
        monkeypatch.setenv("CUDASW4_AMD_CHAIN", str(c))
        ctx = capi.Context(0)
        ctx.set_matrix(O.blosum21(62))
        ctx.set_query(q)
        assert ctx.plan_launch(kind, PART, n, maxlen)[1:] == QUERIES[qlen] + (16,), ctx.plan_launch(kind, PART, n, maxlen)
        need = ctx.scan_temp_bytes(kind, PART, n, maxlen)
        # one workgroup per batch here; the scratch is at least the chain's (it also covers the launch's 32-bit fallback)
        assert need >= nbatches * _chain_bytes(maxlen, c), (c, need, nbatches, _chain_bytes(maxlen, c))
        if c == 1:
            assert need % _region_bytes(maxlen) == 0, (need, _region_bytes(maxlen))
        temp = torch.zeros(need, dtype=torch.uint8, device="cuda")
        results[c] = _scan(torch, capi, ctx, kind, dev, n, maxlen, gop, gex, expect, temp,
                           "case %s qlen %d %s gap (%d, %d) C = %d" % (name, qlen, kind_name, gop, gex, c))
        if c > 1:
            # the launch did chain: the lanes' per-pair maxima lie behind the eleven (nine) workgroups' regions
            region = _chain_bytes(maxlen, c) - 16 * 7 * 16 * 4
            assert bool(temp[nbatches * region:nbatches * _chain_bytes(maxlen, c)].any()), "no chain was walked"
        ctx.close()
    for c in CHAINS[1:]:
        np.testing.assert_array_equal(results[c][0], results[1][0], err_msg="C = %d against C = 1" % c)
        # the early flags are a pair's own (its columns, its place in the frame): the same subjects for every C here
        np.testing.assert_array_equal(results[c][1], results[1][1], err_msg="flagged, C = %d against C = 1" % c)


@pytest.mark.parametrize("qlen", sorted(QUERIES))
@pytest.mark.parametrize("kind_name", ["f16x2", "i16x2"])
def test_chains_then_single_claims(monkeypatch, qlen, kind_name):
    """The launch as it ships: no CUDASW4_AMD_CHAIN_ALL, the default chain length.  One workgroup (CUDASW4_AMD_GRID_CAP=1) and
    twenty batches: the launcher chains (more than sixteen batches per workgroup), and by the kernel's tail rule the first six
    claims are chains of three — while more than three batches remain — and the last two single batches.  Against the
    oracle and against CUDASW4_AMD_CHAIN=1."""
    torch, capi, search = gpu_modules()
    kind = capi.KIND_F16X2 if kind_name == "f16x2" else capi.KIND_I16X2
    gop, gex = GAPS[0]
    q, chars, offsets, lengths, expects = _case("tail", qlen)
    expect = expects[(gop, gex)]
    n, maxlen = len(lengths), int(lengths.max())
    nbatches = (n + 31) // 32
    assert nbatches == 20 and maxlen > 320 and (expect >= 2048).sum() >= 3
    monkeypatch.delenv("CUDASW4_AMD_CHAIN_ALL", raising=False)
    monkeypatch.setenv("CUDASW4_AMD_GRID_CAP", "1")
    dev = _upload(torch, chars, offsets, lengths)
    results = {}
    for c in (None, 1):
        if c is None:
            monkeypatch.delenv("CUDASW4_AMD_CHAIN", raising=False)
        else:
            monkeypatch.setenv("CUDASW4_AMD_CHAIN", str(c))
        ctx = capi.Context(0)
        ctx.set_matrix(O.blosum21(62))
        ctx.set_query(q)
        assert ctx.plan_launch(kind, PART, n, maxlen)[1:] == QUERIES[qlen] + (16,)
        need = ctx.scan_temp_bytes(kind, PART, n, maxlen)
        assert need >= _chain_bytes(maxlen, 3 if c is None else 1), (c, need)     # one workgroup
        temp = torch.zeros(need, dtype=torch.uint8, device="cuda")
        results[c] = _scan(torch, capi, ctx, kind, dev, n, maxlen, gop, gex, expect, temp,
                           "case tail qlen %d %s C = %s" % (qlen, kind_name, "default" if c is None else c))
        if c is None:
            region = _chain_bytes(maxlen, 3) - 16 * 7 * 16 * 4
            assert bool(temp[region:_chain_bytes(maxlen, 3)].any()), "the default launch walked no chain"
        ctx.close()
    np.testing.assert_array_equal(results[None][0], results[1][0])
    np.testing.assert_array_equal(results[None][1], results[1][1])
