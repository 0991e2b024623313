"""GPU: the uniform frame of the packed sw_scan_kernel (sw_dp_kernel.hpp; restated in tests/test_uniform_frame_cpu.py).

The frame is lowered by a*K after every K-th step of the global anti-diagonal t + LANES*stripe, K <= 256: subjects longer
than K lower mid-subject, several stripes shift the lowering step against the border blocks (2*LANES steps each), so that
some lowerings fall inside a block and some on its last quad.  Both packed kinds, 16-lane multi-stripe launches (the
single-stripe 16-lane launches run the streamed kernels), 64-lane groups (single- and multi-stripe), 8- and 4-lane groups,
gap extensions of 1 and 5, homologs with large scores: every score must equal the oracle's."""
import numpy as np
import pytest

import oracle_lib as O
from gpu_util import gpu_modules

pytestmark = pytest.mark.gpu


def _db(rng, q, lens):
    seqs = [rng.integers(0, 20, int(l)).astype(np.int8) for l in np.sort(lens)]
    for k in range(3, len(seqs), 7):   # mutated copies of the query inside long subjects
        emb = q[: len(seqs[k])].copy()
        emb[:: 5 + k % 4] = rng.integers(0, 20, len(emb[:: 5 + k % 4]))
        at = int(rng.integers(0, len(seqs[k]) - len(emb) + 1))
        seqs[k][at:at + len(emb)] = emb
    return seqs


# (lanes, partition, query length, subject lengths): 16 lanes with several stripes, 64 lanes with one and with several,
# 8 and 4 lanes (single-stripe shapes) forced through the environment
CASES = [(16, 33, 1000, (300, 1300)), (16, 33, 1700, (200, 900)), (64, 34, 300, (1281, 2200)), (64, 34, 2100, (1281, 1800)),
         (8, 33, 200, (100, 1200)), (4, 33, 90, (100, 1200))]


@pytest.mark.parametrize("lanes,part_id,qlen,lens", CASES)
@pytest.mark.parametrize("gop,gex", [(-11, -1), (-12, -5)])
def test_uniform_frame_scores(monkeypatch, lanes, part_id, qlen, lens, gop, gex):
    torch, capi, search = gpu_modules()
    monkeypatch.setenv("CUDASW4_AMD_LANES4_MAX_Q", "1000000" if lanes == 4 else "0")
    monkeypatch.setenv("CUDASW4_AMD_LANES8_MAX_Q", "1000000" if lanes == 8 else "0")
    monkeypatch.setenv("CUDASW4_AMD_LANES4_MAX_SUBJECT", "100000")
    rng = np.random.default_rng(lanes * 7 + qlen + abs(gex))
    q = rng.integers(0, 20, qlen).astype(np.int8)
    seqs = _db(rng, q, rng.integers(lens[0], lens[1], 40))
    chars, offsets, lengths = O.make_db(seqs)
    expect = O.scan(q, chars, offsets, lengths, gop=gop, gex=gex, simd=True)
    ctx = capi.Context(0)
    ctx.set_matrix(O.blosum21(62))
    db = search.DeviceDB.from_arrays(chars, offsets, lengths, device=0)
    n = len(seqs)
    maxlen = int(lengths.max())
    scores = torch.empty(n, dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ovf_pos = torch.zeros(n, dtype=torch.int32, device="cuda")
    ovf_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.set_query(q)
    for kind in (capi.KIND_F16X2, capi.KIND_I16X2):
        assert ctx.plan_launch(kind, part_id, n, maxlen)[3] == lanes, (kind, lanes)
        need = ctx.scan_temp_bytes(kind, part_id, n, maxlen)
        temp = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        scores.fill_(-1.0)
        ovf_cnt.zero_()
        ctx.scan_partition(kind, part_id, db.chars.data_ptr(), db.offsets.data_ptr(), db.lengths.data_ptr(), 0, n, maxlen,
                           gop, gex, scores.data_ptr(), ids.data_ptr(), 0, ovf_pos.data_ptr(), ovf_cnt.data_ptr(), 1,
                           temp.data_ptr(), temp.numel(), 0)
        torch.cuda.synchronize()
        got = scores.cpu().numpy().astype(np.int32)
        flagged = ovf_pos.cpu().numpy()[: int(ovf_cnt.item())]
        ok = np.ones(n, dtype=bool)
        ok[flagged] = False                      # flagged subjects are re-scored in 32 bits by the caller
        # flagged only near the kind's limit: score + the larger of the uniform frame's highest zero level and the column
        # frame's bound, a * (K + 2 lanes + 4 + P) with its period K <= 2048
        limit = 2048 if kind == capi.KIND_F16X2 else 25000
        assert (expect[flagged] >= limit - (-gex) * (2048 + 2 * 64 + 12)).all(), (kind, flagged, expect[flagged])
        assert ok.sum() >= n // 2
        np.testing.assert_array_equal(got[ok], expect[ok], err_msg="kind %d lanes %d qlen %d gex %d" % (kind, lanes, qlen, gex))
