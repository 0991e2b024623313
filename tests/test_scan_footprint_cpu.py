"""The arena helper and the case DBs of tests/test_gpu_scan_footprint.py, checked without a device: the helper sees a single
changed byte wherever it lies and names its offset, its guards obey the size rule, and the DBs are what the GPU cases take
them for (batches, the short and the empty subjects, the planted copy, the subjects beyond an under-reported bound)."""
import numpy as np
import pytest

import oracle_lib as O
import scan_footprint as F

SPECS = [("chars", 1001, 256), ("temp", 5000, 7000), ("scores", 400, 400), ("ids", 400, 400), ("ovf_count", 4, 64)]


def _arena(canary=F.CANARIES[0]):
    return F.Arena(SPECS, canary, F.numpy_alloc)


def test_layout_alignment_and_guard_rule():
    a = _arena()
    for name, nbytes, guard in SPECS:
        assert a.off[name] % 256 == 0 and a.size[name] == nbytes
        assert min(a.guard_sizes(name)) >= guard, name
    # neighbours share the larger wish; the last guard reaches the arena's end
    assert a.guard_sizes("chars")[1] >= 7000 and a.guard_sizes("scores")[0] >= 7000
    assert a.off["ovf_count"] + 4 + 64 == a.total == len(a.buf)
    # the rule of the GPU test, given a need function: every guard of temp holds the largest scratch the case could ask for
    need = lambda maxlen, c, grid: grid * F.chain_bytes(maxlen, c)   # noqa: E731
    big = need(600, 8, 11)
    b = F.Arena([("chars", 1000, 256), ("temp", need(400, 1, 11), big), ("scores", 400, 400)], 0xA5, F.numpy_alloc)
    assert b.guards_hold({"temp": big, "scores": 400, "chars": 256})
    assert not b.guards_hold({"temp": big + 1})
    assert not F.Arena([("temp", 100, 50)], 0xA5, F.numpy_alloc).guards_hold({"temp": 51})


@pytest.mark.parametrize("canary", F.CANARIES)
def test_untouched_arena_passes_and_buffers_may_change(canary):
    a = _arena(canary)
    assert a.check() == []
    for name in a.names:
        a.slice(name)[:] = 0x11
    assert a.check() == []
    assert a.high_water("temp") == 5000
    a.fill()
    assert a.high_water("temp") == 0
    a.slice("temp")[10:20] = 0
    assert a.high_water("temp") == 20


@pytest.mark.parametrize("canary", F.CANARIES)
@pytest.mark.parametrize("where", ["directly before", "directly behind", "far end of the guard behind", "far end of the guard before",
                                   "first byte of the arena", "last byte of the arena"])
def test_a_single_changed_byte_is_found_with_its_offset(canary, where):
    a = _arena(canary)
    start, end = a.off["temp"], a.off["temp"] + a.size["temp"]
    before, behind = a.guard_sizes("temp")
    at, names, first, neg = {
        "directly before": (start - 1, ("chars", "temp"), before - 1, -1),
        "directly behind": (end, ("temp", "scores"), 0, -behind),
        "far end of the guard behind": (a.off["scores"] - 1, ("temp", "scores"), behind - 1, -1),
        "far end of the guard before": (a.off["chars"] + a.size["chars"], ("chars", "temp"), 0, -before),
        "first byte of the arena": (0, ("the arena's start", "chars"), 0, -a.off["chars"]),
        "last byte of the arena": (a.total - 1, ("ovf_count", "the arena's end"), 63, -1),
    }[where]
    a.buf[at] ^= 0x01
    report = a.check()
    assert len(report) == 1, report
    assert report[0].startswith("1 bytes changed between %s and %s: first %d, last %d behind" % (names[0], names[1], first, first)), report
    assert "(%d .. %d before" % (neg, neg) in report[0], report


def test_a_smaller_offer_moves_the_guard_to_its_end():
    a = _arena()
    a.slice("temp")[:] = 0
    a.fill()
    a.slice("temp")[:3000] = 0
    assert a.check(used={"temp": 3000}) == []
    a.slice("temp")[3000] = 0
    report = a.check(used={"temp": 3000})
    assert len(report) == 1 and "first 0, last 0 behind the end of temp" in report[0], report
    assert a.check() == []            # at full size that byte is the buffer's own
    a.slice("temp")[4999] = 0
    a.slice("temp")[3007] = 0
    assert "3 bytes changed between temp and scores: first 0, last 1999 behind" in a.check(used={"temp": 3000})[0]


def test_region_sizes_are_the_launchers():
    """region_bytes / chain_bytes restate sw_api.hip's border_bytes_per_wg / chain_bytes_per_wg: against the recorded plan table
    (tests/golden/launch_plan_table.npz: sw_scan_temp_bytes of a 1000-residue query, fp32, one subject = one workgroup)"""
    import plan_table_grid as G
    t = np.load(G.DATA)
    qi, ki, ni = G.QLENS.index(1000), G.KINDS.index(3), G.NS.index(1)
    for msl in (64, 320, 1024, 1280):
        assert int(t["default/temp"][0, qi, ki, G.PARTS.index(33), ni, G.MSLS.index(msl)]) == F.region_bytes(msl), msl
    for msl in (1281, 8000):
        assert int(t["default/temp"][0, qi, ki, G.PARTS.index(34), ni, G.MSLS.index(msl)]) == F.region_bytes(msl, 64), msl


@pytest.mark.parametrize("qlen", [850, 1500])
def test_ragged_case_is_what_the_table_claims(qlen):
    c = F.ragged(qlen, last_mult4=qlen == 1500)
    q = F.query(qlen)
    assert c.n == 339 and (c.n + 31) // 32 == 11 and c.n - 10 * 32 == 19     # eleven batches, the last one partial
    assert c.first_pos > 0 and c.first_pos + c.n < c.N
    L = c.lengths[c.range]
    assert c.maxlen == 600 and L[7] == 600
    ordinary = L[L > 3]
    assert ordinary.min() >= 330 and len(ordinary) == 339 - 8 - 8 - 8
    for (batch, group), (la, lb) in F.SHORT_PAIRS.items():
        assert (L[F.index(batch, group, 0)], L[F.index(batch, group, 1)]) == (la, lb)
    assert sorted(int(L[F.index(b, g, h)]) for (b, g) in F.SHORT_PAIRS for h in (0, 1)) == [0, 0, 1, 1, 2, 2, 3, 3]
    for batch, group in F.EMPTY_PAIRS:       # empty pairs inside the first chain of C = 3, 4 and 8 (batches 10 .. 7 at least)
        assert L[F.index(batch, group, 0)] == 0 and L[F.index(batch, group, 1)] == 0 and 7 <= batch < 10
    # dbdata layout: every subject padded to a multiple of 4 with code 20, the range's letters last, nothing behind them
    pad = (c.lengths.astype(np.int64) + 3) // 4 * 4
    assert len(c.chars) == pad.sum() and int(c.offsets[0]) == 0 == int(c.offsets.min())
    last = c.first_pos + c.n - 1
    assert int(c.offsets[last]) + pad[last] == len(c.chars)
    assert (c.lengths[last] % 4 == 0) == (qlen == 1500)
    for i in range(c.N):
        o, l = int(c.offsets[i]), int(c.lengths[i])
        assert (c.chars[o:o + l] == c.seqs[i]).all() and (c.chars[o + l:o + pad[i]] == 20).all()
    spans = sorted((int(c.offsets[i]), int(c.offsets[i]) + int(pad[i])) for i in range(c.N) if pad[i])
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    # the planted copy is beyond the fp16 limit; nothing else comes inside the flag margin below it (limit - 1536)
    e = c.expect(q)[c.range]
    assert e[F.PLANTED] >= 2048
    others = np.delete(e, F.PLANTED)
    assert others.max() < 2048 - 1536, others.max()
    # a launch that reports 400 for the longest subject
    over = L > (c.bound + 3) // 4 * 4
    assert over.sum() >= 20 and (~over).sum() >= 20
    cut = c.expect(q, bound=c.bound)[c.range]
    assert (cut[~over] == e[~over]).all()
    assert (cut[over] != e[over]).sum() * 2 >= over.sum(), ((cut[over] != e[over]).sum(), over.sum())
    assert (cut <= e).all()


def test_streamed_wide_and_listed_cases():
    for hi, bound in ((300, 200), (190, 124)):
        c = F.streamed(850, hi)
        L = c.lengths[c.range]
        assert c.n == 330 and (np.diff(L) >= 0).all() and L.min() >= 40 and L.max() == hi == c.maxlen and c.bound == bound
        assert c.expect(F.query(850))[c.range].max() >= 2048 - 1536      # the overflow list is written
        over = L > c.bound
        assert over.sum() >= 20 and (~over).sum() >= 20
    c = F.wide(850)
    L = c.lengths[c.range]
    assert tuple(L) == F.WIDE_LENGTHS and L.min() == 1281 and c.maxlen == 1700 and c.part == 34
    over = L > c.bound
    assert over.sum() >= 3 and (~over).sum() >= 3                   # (nine subjects in all)
    e, cut = c.expect(F.query(850))[c.range], c.expect(F.query(850), bound=c.bound)[c.range]
    assert (cut[~over] == e[~over]).all() and (cut[over] != e[over]).sum() * 2 >= over.sum()
    for count in (0, 1, 37):
        c, pos = F.listed(850, count)
        assert len(pos) == F.LIST_CAPACITY == 64 and len(set(pos[:count])) == count and (pos[count:] == 1).all() and 1 not in pos[:count]
        if count:
            assert pos[0] == F.LIST_LONG and c.lengths[pos[0]] > 8000
        if count > 2:
            assert 0 in pos[:count] and c.N - 1 in pos[:count] and np.ptp(pos[:count]) == c.N - 1
    d = F.dirtier()
    assert d.lengths[d.range].min() >= 600 and d.maxlen > 600 and len(O.blosum21(62)) == 441
