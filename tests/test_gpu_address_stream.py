"""GPU: the address stream of the packed multi-stripe sw_scan_kernel on 16-lane groups (sw_dp_kernel.hpp: stream_region_words,
dp_step<ADDR>).

A group writes one word per subject column behind its border array once per subject pair — the two letters' profile-row
offsets — and lane l reads the word of column t - l at step t of every stripe, instead of passing the letters along the
group.  What can go wrong lies at the stream's edges: the padding words before column 0 and behind each subject's own end
(pairs of different lengths, a last group without a subject B, empty subjects), the four-column words a lane writes (lengths
around every multiple of 4, 16, 32 and 64), the walk over several stripes and over the border blocks, and the size of the
scratch region that now holds 12 instead of 8 bytes per column.  Both packed kinds, gap scores (-11, -1) and (-12, -5): every
score the kernel did not flag must equal the oracle's, and only near the kind's limit may it flag.

Random residues with short planted copies of query segments (across the stripe borders too): the scores stay far below
the 16-bit limits, so no subject should be left out; a case fails when more than a tenth of its subjects are."""
import numpy as np
import pytest

import oracle_lib as O
from gpu_util import gpu_modules

pytestmark = pytest.mark.gpu

# subject lengths around every boundary of the stream (a lane writes four columns at a time, sixteen lanes a round; border
# blocks are 32 steps), and empty subjects
EDGES = [0, 0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]


def _subjects(rng, q, lens, stripe_rows):
    """random subjects in the given order; every third one that has room carries a mutated copy of at most 40 residues of
    the query, every other of those cut from across a stripe border"""
    seqs = []
    for k, l in enumerate(lens):
        s = rng.integers(0, 20, int(l)).astype(np.int8)
        if k % 3 == 0 and l >= 12:
            n = int(min(l, 40))
            if (k // 3) % 2 == 0 and stripe_rows + n // 2 <= len(q):
                at_q = stripe_rows * int(rng.integers(1, len(q) // stripe_rows + 1)) - n // 2   # straddles a stripe border
                at_q = min(at_q, len(q) - n)
            else:
                at_q = int(rng.integers(0, len(q) - n + 1))
            emb = q[at_q:at_q + n].copy()
            emb[::4] = rng.integers(0, 20, len(emb[::4]))
            at = int(rng.integers(0, l - n + 1))
            s[at:at + n] = emb
        seqs.append(s)
    return seqs


def _lens(name, rng):
    if name == "edges":          # every edge length, an odd count: the last group has no subject B
        return np.sort(np.concatenate([EDGES, rng.integers(130, 420, 28), [450]]))            # 47 subjects
    if name == "bimodal32":      # exactly 32 subjects; 15 short + 17 long: one pair's lengths differ by more than 64
        return np.sort(np.concatenate([rng.integers(20, 70, 15), rng.integers(330, 420, 17)]))
    if name == "steps33":        # 33 subjects (a full batch and a single subject); neighbours differ by exactly 1
        return np.concatenate([np.arange(97, 129), [400]])
    if name == "few7":           # one partial batch, odd
        return np.sort(np.concatenate([[0, 2, 18, 66, 131, 200], [345]]))
    raise KeyError(name)


# (case, query length, CUDASW4_AMD_TWO_WAVE_PENALTY, expected rows per lane, stripes): 850 residues = 2 stripes of 27 rows,
# 1700 = 4 stripes of 27 rows, or 3 stripes of 36 rows (a two-wave kernel) with the planner's penalty off
CASES = [("edges", 850, None, 27, 2), ("bimodal32", 1700, None, 27, 4), ("steps33", 1700, "1", 36, 3), ("few7", 850, None, 27, 2),
         ("edges", 1700, None, 27, 4)]
PART = 33   # a partition of 16-lane groups

_cache = {}


def _case(name, qlen, rows):
    """DB and oracle scores of a case, computed once for both gap settings' tests"""
    key = (name, qlen)
    if key not in _cache:
        rng = np.random.default_rng(len(name) * 1000 + qlen)
        q = rng.integers(0, 20, qlen).astype(np.int8)
        seqs = _subjects(rng, q, _lens(name, rng), 16 * rows)
        chars, offsets, lengths = O.make_db(seqs)
        expect = {g: O.scan(q, chars, offsets, lengths, gop=g[0], gex=g[1], simd=True) for g in ((-11, -1), (-12, -5))}
        _cache[key] = (q, chars, offsets, lengths, expect)
    return _cache[key]


def _region_bytes(maxlen):
    """scratch bytes of one workgroup of 16-lane groups: 16 groups x blocks x (64 border + 32 stream words)"""
    steps = (maxlen + 15 + 3) // 4 * 4
    lcap = (steps + 15) // 16 * 16 + 16
    blocks = (lcap + 31) // 32 + 3
    return 16 * blocks * 96 * 4


@pytest.mark.parametrize("name,qlen,penalty,rows,stripes", CASES)
@pytest.mark.parametrize("gop,gex", [(-11, -1), (-12, -5)])
def test_address_stream_scores(monkeypatch, name, qlen, penalty, rows, stripes, gop, gex):
    torch, capi, search = gpu_modules()
    if penalty is not None:
        monkeypatch.setenv("CUDASW4_AMD_TWO_WAVE_PENALTY", penalty)
    q, chars, offsets, lengths, expects = _case(name, qlen, rows)
    expect = expects[(gop, gex)]
    assert expect.max() < 400, expect.max()    # far below the fp16 limit: nothing should be flagged
    ctx = capi.Context(0)
    ctx.set_matrix(O.blosum21(62))
    db = search.DeviceDB.from_arrays(chars, offsets, lengths, device=0)
    n = len(lengths)
    maxlen = int(lengths.max())
    assert maxlen > 320   # longer than what multi-stripe queries stream: sw_scan_kernel, one pair per group at a time
    scores = torch.empty(n, dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ovf_pos = torch.zeros(n, dtype=torch.int32, device="cuda")
    ovf_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.set_query(q)
    for kind in (capi.KIND_F16X2, capi.KIND_I16X2):
        assert ctx.plan_launch(kind, PART, n, maxlen)[1:] == (rows, stripes, 16), ctx.plan_launch(kind, PART, n, maxlen)
        need = ctx.scan_temp_bytes(kind, PART, n, maxlen)
        # the scratch holds the border array and the address stream of every group: 12 bytes per column
        assert need >= (n + 31) // 32 * _region_bytes(maxlen) and need % _region_bytes(maxlen) == 0, (need, _region_bytes(maxlen))
        temp = torch.empty(need, dtype=torch.uint8, device="cuda")
        scores.fill_(-1.0)
        ovf_cnt.zero_()
        ctx.scan_partition(kind, PART, db.chars.data_ptr(), db.offsets.data_ptr(), db.lengths.data_ptr(), 0, n, maxlen,
                           gop, gex, scores.data_ptr(), ids.data_ptr(), 0, ovf_pos.data_ptr(), ovf_cnt.data_ptr(), 1,
                           temp.data_ptr(), temp.numel(), 0)
        torch.cuda.synchronize()
        got = scores.cpu().numpy().astype(np.int32)
        flagged = ovf_pos.cpu().numpy()[: int(ovf_cnt.item())]
        print("case %s qlen %d kind %d gap (%d, %d): %d of %d flagged, highest score %d" % (name, qlen, kind, gop, gex, len(flagged), n, expect.max()))
        ok = np.ones(n, dtype=bool)
        ok[flagged] = False                      # flagged subjects are re-scored in 32 bits by the caller
        # flagged only near the kind's limit: score + the larger of the uniform frame's highest zero level and the column
        # frame's bound, a * (K + 2 lanes + 4 + P) with its period K <= 2048
        limit = 2048 if kind == capi.KIND_F16X2 else 25000
        assert (expect[flagged] >= limit - (-gex) * (2048 + 2 * 64 + 12)).all(), (kind, flagged, expect[flagged])
        assert 10 * len(flagged) <= n, (kind, len(flagged), n)
        np.testing.assert_array_equal(got[ok], expect[ok], err_msg="case %s kind %d qlen %d gex %d" % (name, kind, qlen, gex))
        np.testing.assert_array_equal(ids.cpu().numpy(), np.arange(n))


@pytest.mark.parametrize("shrink", [1, 3])
def test_streamed_rounds_in_the_larger_region(shrink):
    """Short subjects of a multi-stripe query run the streamed kernels, whose rounds hold as many columns as the scratch gives
    the grid (scan_common: the `cols` loop): with the scratch sw_scan_temp_bytes asks for, and with a third of it — shorter
    rounds in regions of the new size — every score equals the oracle's."""
    torch, capi, search = gpu_modules()
    rng = np.random.default_rng(77)
    q = rng.integers(0, 20, 850).astype(np.int8)
    lens = np.sort(np.concatenate([EDGES, rng.integers(20, 190, 46)]))
    chars, offsets, lengths = O.make_db(_subjects(rng, q, lens, 16 * 27))
    expect = O.scan(q, chars, offsets, lengths, simd=True)
    ctx = capi.Context(0)
    ctx.set_matrix(O.blosum21(62))
    db = search.DeviceDB.from_arrays(chars, offsets, lengths, device=0)
    n, maxlen = len(lengths), int(lengths.max())
    scores = torch.empty(n, dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ovf_pos = torch.zeros(n, dtype=torch.int32, device="cuda")
    ovf_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.set_query(q)
    for kind in (capi.KIND_F16X2, capi.KIND_I16X2):
        need = ctx.scan_temp_bytes(kind, PART, n, maxlen)
        assert need > (n + 31) // 32 * _region_bytes(maxlen)     # sized for rounds of several subjects, not for the longest one
        temp = torch.empty(need // shrink, dtype=torch.uint8, device="cuda")
        scores.fill_(-1.0)
        ovf_cnt.zero_()
        ctx.scan_partition(kind, PART, db.chars.data_ptr(), db.offsets.data_ptr(), db.lengths.data_ptr(), 0, n, maxlen,
                           -11, -1, scores.data_ptr(), ids.data_ptr(), 0, ovf_pos.data_ptr(), ovf_cnt.data_ptr(), 1,
                           temp.data_ptr(), temp.numel(), 0)
        torch.cuda.synchronize()
        got = scores.cpu().numpy().astype(np.int32)
        flagged = ovf_pos.cpu().numpy()[: int(ovf_cnt.item())]
        ok = np.ones(n, dtype=bool)
        ok[flagged] = False
        limit = 2048 if kind == capi.KIND_F16X2 else 25000
        assert (expect[flagged] >= limit - (2048 + 2 * 64 + 12)).all(), (kind, flagged, expect[flagged])
        assert 10 * len(flagged) <= n, (kind, len(flagged), n)
        np.testing.assert_array_equal(got[ok], expect[ok], err_msg="kind %d shrink %d" % (kind, shrink))
