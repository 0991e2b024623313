"""GPU: what the launcher-level scan ABI (include/cudasw4_amd.h) promises about memory, on an arena with guard zones.

  P1  a launch stays inside the temp_bytes it was given (sw_scan_temp_bytes), and inside its output arrays;
  P2  a smaller temp buffer gives the same results down to one pair's scratch for one workgroup; below that SW_ERR_TEMP,
      and nothing is touched;
  P3  the scratch is plain scratch: whatever it held before — zeros, NaN patterns, large finite values, what another
      launch left there — the results are the same;
  P4  an under-reported max_subject_len is memory-safe and cuts longer subjects at the bound (rounded up to a whole letter
      word: sw_dp_kernel.hpp, load_pair).

Every buffer a launch may write (temp, scores, ids, ovf_pos, ovf_count) is a slice of ONE device tensor filled with a canary
byte (scan_footprint.Arena).  The guards around temp are as large as the scratch of the same launch with the true longest
subject, the case's longest chains and no grid cap, and the dirtying launch's of P3: a kernel that ignored the offer, the
clamps or the bound altogether would still write inside the allocation, so a defect is a changed canary, not a fault.  The
subject letters live in the arena too, the scanned range last, canary bytes directly behind the last letter word.

Cases (scan_footprint.py; the CPU oracle is the reference, the flagged subjects are re-scored in 32 bits as callers do):
  a  packed multi-stripe sw_scan_kernel, 16-lane groups, address stream, chains of 1, 3, 4 and 8 pairs (CUDASW4_AMD_CHAIN_ALL)
  b  the same with three stripes        c  the streamed rounds (sw_stream_kernel.hpp), one workgroup, rounds of 2, 4, 16 slots
  d  the 32-bit kinds, two and three stripes      e  wave-wide groups (partition 34), all four kinds
  f  re-score lists (sw_rescore_overflow[_stat])  g  single-stripe queries: no scratch at all, temp NULL or of 0 bytes

Streamed launches (c) flag a subject also for the score of the subject streamed right before it, and from a score that
depends on its place in the round, so between launches whose rounds differ (P2) only the final scores are compared, and
`one`, the scratch of one pair for one workgroup, is read with CUDASW4_AMD_STREAM=1 as well: a round of several slots is
not one pair."""
import os

import numpy as np
import pytest

import oracle_lib as O
import scan_footprint as F
from gpu_util import gpu_modules

pytestmark = pytest.mark.gpu

KIND = {"f16x2": 0, "i16x2": 1, "i32": 2, "f32": 3}
LIMIT = {0: 2048, 1: 25000}
MARGIN = {0: 1536, 1: 2100}          # include/cudasw4_amd.h: no flagged subject scores below limit - margin with gex = -1
PREFILLS = (0x00, 0xFF, 0x7C, 0x7B)  # zeros; fp16 NaN; 0x7C7C: fp16 NaN, a large biased int16; 0x7B7B: fp16 61248, a large int16
S = F.SENTINEL


def _scenarios():
    sc = {}

    def add(name, **kw):
        kw.setdefault("gaps", (-11, -1))
        sc[name] = kw

    for kind in ("f16x2", "i16x2"):
        for qlen, rows in ((850, 27), (1500, 47)):
            for c in (1, 3, 4, 8):
                add("a-%s-q%d-c%d" % (kind, qlen, c), case=("ragged", qlen), qlen=qlen, kind=kind, chain=c,
                    env=dict(CHAIN=c, CHAIN_ALL=1), plan=(KIND[kind], rows, 2, 16))
        add("b-%s-q1530-c3" % kind, case=("ragged", 1530), qlen=1530, kind=kind, chain=3, env=dict(CHAIN=3, CHAIN_ALL=1),
            plan=(KIND[kind], 32, 3, 16))
        for slots in (2, 4, 16):
            add("c-%s-s%d" % (kind, slots), case=("streamed", 850, 300 if kind == "f16x2" else 190), qlen=850, kind=kind,
                env=dict(STREAM=slots, GRID_CAP=1), plan=(KIND[kind], 27, 2, 16), streamed=True)
        add("e-%s" % kind, case=("wide", 1500), qlen=1500, kind=kind, env={}, plan=(KIND[kind], 12, 2, 64))
    add("a-f16x2-q850-c3-gap12_5", case=("ragged", 850), qlen=850, kind="f16x2", chain=3, env=dict(CHAIN=3, CHAIN_ALL=1),
        plan=(0, 27, 2, 16), gaps=(-12, -5))
    add("d-f32-q850", case=("ragged-plain", 850), qlen=850, kind="f32", env={}, plan=(3, 27, 2, 16))
    add("d-f32-q1300", case=("ragged-plain", 1300), qlen=1300, kind="f32", env={}, plan=(3, 28, 3, 16))
    add("d-i32-q850", case=("ragged-plain", 850), qlen=850, kind="i32", env={}, plan=(3, 27, 2, 16))     # int32 in fp32 lanes
    add("d-i32native-q850", case=("ragged-plain", 850), qlen=850, kind="i32", env=dict(I32_NATIVE=1), plan=(2, 27, 2, 16))
    add("d-i32native-q1600", case=("ragged-plain", 1600), qlen=1600, kind="i32", env=dict(I32_NATIVE=1), plan=(2, 34, 3, 16))
    add("e-f32", case=("wide", 850), qlen=850, kind="f32", env={}, plan=(3, 7, 2, 64))
    add("e-i32native", case=("wide", 850), qlen=850, kind="i32", env=dict(I32_NATIVE=1), plan=(2, 7, 2, 64))
    return sc


SCENARIOS = _scenarios()


def _case(spec):
    if spec[0] == "ragged":
        return F.ragged(spec[1], last_mult4=spec[1] == 1500)
    if spec[0] == "ragged-plain":
        return F.ragged(spec[1], planted=False)
    if spec[0] == "streamed":
        return F.streamed(spec[1], spec[2])
    return F.wide(spec[1])


class Rig:
    """the modules, and contexts by (query, environment): the tuning variables are read when a context is created"""

    def __init__(self, monkeypatch):
        self.torch, self.capi, _ = gpu_modules()
        self.device = "cuda"
        self.mp = monkeypatch
        self.ctxs = {}

    def context(self, q, env):
        key = (q.tobytes(), tuple(sorted(env.items())))
        if key not in self.ctxs:
            for name in list(os.environ):
                if name.startswith("CUDASW4_AMD_") and name != "CUDASW4_AMD_LIB":
                    self.mp.delenv(name)
            for name, value in env.items():
                self.mp.setenv("CUDASW4_AMD_" + name, str(value))
            ctx = self.capi.Context(0)
            ctx.set_matrix(O.blosum21(62))
            ctx.set_query(q)
            self.ctxs[key] = ctx
        return self.ctxs[key]

    def to_device(self, array):
        return self.torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def close(self):
        for ctx in self.ctxs.values():
            ctx.close()


@pytest.fixture
def rig(monkeypatch):
    r = Rig(monkeypatch)
    yield r
    r.close()


class Bench:
    """a case on the device: its letters and everything a launch writes inside one arena"""

    def __init__(self, rig, case, canary, temp_bytes, guard, list_capacity=None):
        torch = rig.torch
        self.rig, self.case = rig, case
        N, cap = case.N, list_capacity or case.N
        nchars = len(case.chars)
        specs = [("chars", nchars, 256), ("chars_slack", nchars + 64, 256), ("temp", temp_bytes, max(guard, 256)),
                 ("scores", 4 * N, 4 * N), ("ids", 4 * N, 4 * N), ("ovf_pos", 4 * cap, 4 * cap), ("ovf_count", 4, 256), ("stat", 4, 256)]
        self.arena = F.Arena(specs, canary, lambda n: torch.empty(n, dtype=torch.uint8, device=rig.device))
        assert self.arena.buf.data_ptr() % 256 == 0 and self.arena.off["temp"] % 256 == 0
        assert self.arena.guards_hold({"temp": guard, "scores": 4 * N, "ids": 4 * N, "ovf_pos": 4 * cap, "ovf_count": 4})
        self.d_chars = rig.to_device(case.chars.view(np.uint8))
        self.offsets = rig.to_device(case.offsets.view(np.int64))
        self.lengths = rig.to_device(case.lengths)
        self.list = None      # (positions, count) of a re-score list

    def ptr(self, name):
        return self.arena.buf.data_ptr() + self.arena.off[name]

    def typed(self, name, dtype):
        return self.arena.slice(name).view(dtype)

    def host(self, name, dtype):
        return self.arena.slice(name).cpu().numpy().view(dtype)

    def reset(self, keep_temp=False):
        torch, a = self.rig.torch, self.arena
        kept = a.slice("temp").clone() if keep_temp else None
        a.fill()
        if kept is not None:
            a.slice("temp").copy_(kept)
        n = len(self.d_chars)
        a.slice("chars").copy_(self.d_chars)
        a.slice("chars_slack")[:n].copy_(self.d_chars)
        a.slice("chars_slack")[n:] = 20
        self.typed("scores", torch.float32)[:] = float(S)
        self.typed("ids", torch.int32)[:] = S
        self.typed("ovf_pos", torch.int32)[:] = S
        self.typed("ovf_count", torch.int32)[:] = 0
        self.typed("stat", torch.int32)[:] = 5
        if self.list is not None:
            self.typed("ovf_pos", torch.int32).copy_(self.rig.to_device(self.list[0]))
            self.typed("ovf_count", torch.int32)[:] = self.list[1]

    def intact(self, offer, what):
        self.rig.torch.cuda.synchronize()     # (a defect has changed a canary by now, inside the arena)
        report = self.arena.check(used={"temp": offer})
        assert not report, "%s, %d of %d temp bytes offered: %s" % (what, offer, self.arena.size["temp"], "; ".join(report))


def _scan(b, ctx, kind, offer, what, bound=None, gaps=(-11, -1), prefill=None, keep_temp=False, chars="chars", temp_null=False,
          id_offset=0, streamed=False):
    """one launch over the case's range with `offer` bytes of scratch, the guards, the sentinels, and the 32-bit re-score of
    what it flagged -> (final scores of the range, sorted flagged positions)"""
    torch, capi, case = b.rig.torch, b.rig.capi, b.case
    first, n = case.first_pos, case.n
    maxlen = case.maxlen if bound is None else bound
    b.reset(keep_temp)
    if prefill is not None:
        b.arena.slice("temp", offer)[:] = prefill
    ctx.scan_partition(kind, case.part, b.ptr(chars), b.offsets.data_ptr(), b.lengths.data_ptr(), first, n, maxlen, gaps[0], gaps[1],
                       b.ptr("scores"), b.ptr("ids"), id_offset, b.ptr("ovf_pos"), b.ptr("ovf_count"), 1,
                       0 if temp_null else b.ptr("temp"), offer, 0)
    b.intact(offer, what)
    count = int(b.host("ovf_count", np.int32)[0])
    pos = b.host("ovf_pos", np.int32)
    assert 0 <= count <= n, (what, count)
    flagged = np.sort(pos[:count])
    assert (pos[count:] == S).all(), (what, "list entries behind the count were written")
    assert len(np.unique(flagged)) == count and (count == 0 or (flagged[0] >= first and flagged[-1] < first + n)), (what, flagged)
    packed, ids = b.host("scores", np.float32), b.host("ids", np.int32)
    for arr in (packed, ids):
        assert (arr[:first] == S).all() and (arr[first + n:] == S).all(), (what, "entries outside the range were written")
    np.testing.assert_array_equal(ids[first:first + n], id_offset + np.arange(first, first + n), err_msg=what + ": ids")
    assert (packed[flagged] == S).all(), (what, "a flagged subject's score was written")
    expect = case.expect(b.q, gaps, bound)
    if kind in LIMIT:
        ok = np.ones(case.N, dtype=bool)
        ok[flagged] = False
        np.testing.assert_array_equal(packed[case.range][ok[case.range]], expect[case.range][ok[case.range]], err_msg=what + ": packed scores")
        if gaps[1] == -1:
            near = expect[flagged] >= LIMIT[kind] - MARGIN[kind]
            if streamed:
                # ... or the subject streamed through the lanes right before it (the same place of the next batch) reached the
                # jump of the zero levels, or was itself listed for that reason (what it left in the lanes is not known to be low)
                for i in np.argsort(-flagged):
                    before = flagged[i] + 32
                    if not near[i] and before < first + n:
                        near[i] = expect[before] >= (512 if kind == 0 else 2048) - 4 or bool(near[flagged == before].any())
            assert near.all(), (what, "flagged far below the limit", flagged[~near], expect[flagged[~near]])
        else:
            assert (expect[flagged] >= LIMIT[kind] - (-gaps[1]) * (2048 + 2 * 64 + 12)).all(), (what, flagged)   # (as test_gpu_pair_chain.py)
    else:
        assert count == 0 or kind in LIMIT
    if count:
        rtemp = torch.empty(max(16, ctx.scan_temp_bytes(capi.KIND_I32, -1, count, maxlen)), dtype=torch.uint8, device=b.rig.device)
        ctx.rescore_overflow(capi.KIND_I32, b.ptr("ovf_pos"), b.ptr("ovf_count"), count, b.ptr(chars), b.offsets.data_ptr(),
                             b.lengths.data_ptr(), maxlen, gaps[0], gaps[1], b.ptr("scores"), b.ptr("ids"), id_offset,
                             rtemp.data_ptr(), rtemp.numel(), 0)
        b.intact(offer, what + ", re-score")
    final = b.host("scores", np.float32)[case.range].astype(np.int32)
    np.testing.assert_array_equal(final, expect[case.range], err_msg=what)   # all n subjects
    return final, flagged


def _open(rig, name, canary, extra_guard=0, bound=None):
    """the scenario's context, case and arena: temp as large as the launch's need, guards as the module docstring says"""
    sc = SCENARIOS[name]
    case, q, kind = _case(sc["case"]), F.query(sc["qlen"]), KIND[sc["kind"]]
    ctx = rig.context(q, sc["env"])
    assert ctx.plan_launch(kind, case.part, case.n, case.maxlen) == sc["plan"], (name, ctx.plan_launch(kind, case.part, case.n, case.maxlen))
    need = ctx.scan_temp_bytes(kind, case.part, case.n, case.maxlen)
    assert need > 0
    free = {k: v for k, v in sc["env"].items() if k != "GRID_CAP"}
    if "chain" in sc:
        free["CHAIN"] = 8
    guard = max(need, rig.context(q, free).scan_temp_bytes(kind, case.part, case.n, case.maxlen), extra_guard)
    if sc.get("streamed"):
        # the streamed plan: the scratch holds a round's columns, more than the longest subject's
        assert need > rig.context(q, dict(sc["env"], STREAM=1)).scan_temp_bytes(kind, case.part, case.n, case.maxlen)
    b = Bench(rig, case, canary, need if bound is None else ctx.scan_temp_bytes(kind, case.part, case.n, bound), guard)
    b.q = q
    return sc, case, q, kind, ctx, need, b


def _canary(name):
    return F.CANARIES[sum(name.encode()) % 2]


# ------------------------------------------------------------------------------------------------------------------ P1
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_p1_footprint_at_full_size(rig, name):
    sc, case, q, kind, ctx, need, b = _open(rig, name, _canary(name))
    id_offset = 1000 if _canary(name) == F.CANARIES[1] else 0
    final, flagged = _scan(b, ctx, kind, need, name, gaps=sc["gaps"], id_offset=id_offset, streamed=sc.get("streamed", False))
    mark = b.arena.high_water("temp")    # (the re-score has its own scratch: this is the scan's)
    print("%s: need %d bytes, last byte written %d, %d flagged" % (name, need, mark, len(flagged)))
    assert 0 < mark <= need
    if kind == KIND["f16x2"] and sc["case"][0] in ("ragged", "streamed"):
        assert len(flagged) >= 1, "the overflow list was not written"
    # the same DB followed by 64 bytes of code 20 instead of the canary: nothing behind the last letter word is looked at
    again, flagged2 = _scan(b, ctx, kind, need, name + ", slack behind the letters", gaps=sc["gaps"], id_offset=id_offset,
                            chars="chars_slack", streamed=sc.get("streamed", False))
    np.testing.assert_array_equal(again, final)
    np.testing.assert_array_equal(flagged2, flagged)
    if sc.get("chain", 1) > 1:
        # the launch did chain: the per-pair maxima behind the eleven workgroups' regions were written
        c = sc["chain"]
        assert need >= 11 * F.chain_bytes(600, c), (need, F.chain_bytes(600, c))
        maxima = b.arena.slice("temp")[11 * (F.chain_bytes(600, c) - F.CHAIN_MAXIMA_BYTES):]
        assert bool((maxima != b.arena.canary).any()), "no chain was walked"


# ------------------------------------------------------------------------------------------------------------------ P2
P2_CASES = ["a-f16x2-q850-c4", "a-i16x2-q1500-c4", "a-i16x2-q850-c3", "b-f16x2-q1530-c3", "c-f16x2-s4", "c-i16x2-s16",
            "d-f32-q1300", "d-i32native-q850", "e-f16x2", "e-i16x2", "e-f32", "e-i32native"]


@pytest.mark.parametrize("name", P2_CASES)
def test_p2_smaller_offers(rig, name):
    sc, case, q, kind, ctx, need, b = _open(rig, name, _canary(name + "p2"))
    torch, capi = rig.torch, rig.capi
    streamed = sc.get("streamed", False)
    one_env = dict(sc["env"], GRID_CAP=1, CHAIN=1)
    if streamed:
        one_env["STREAM"] = 1
    one = rig.context(q, one_env).scan_temp_bytes(kind, case.part, case.n, case.maxlen)
    assert one == F.region_bytes(case.maxlen, sc["plan"][3]) and one + 1 < need // 2, (one, need)
    ref, ref_flagged = _scan(b, ctx, kind, need, name, streamed=streamed)
    offers = [need // 2] + ([need // 10] if need // 10 >= one else []) + [one + 1, one]
    for offer in offers:
        final, flagged = _scan(b, ctx, kind, offer, "%s, offer %d" % (name, offer), streamed=streamed)
        np.testing.assert_array_equal(final, ref)
        if not streamed:
            np.testing.assert_array_equal(flagged, ref_flagged)
        if name == "a-f16x2-q850-c4" and offer == one:
            # the clamp: no chain is walked — where the full-size launch keeps its per-pair maxima nothing was written
            # (those bytes lie behind the offer: guard bytes, as intact() has checked; said once more for the region itself)
            lo = 11 * (F.chain_bytes(600, 4) - F.CHAIN_MAXIMA_BYTES)
            assert bool((b.arena.slice("temp")[lo:] == b.arena.canary).all()) and b.arena.high_water("temp") <= one
    if name == "a-f16x2-q850-c4":
        _scan(b, ctx, kind, need, name + ", full size again")
        lo = 11 * (F.chain_bytes(600, 4) - F.CHAIN_MAXIMA_BYTES)
        assert need >= 11 * F.chain_bytes(600, 4) and bool((b.arena.slice("temp")[lo:] != b.arena.canary).any())
    # one byte less than one pair's scratch for one workgroup: SW_ERR_TEMP, and nothing at all is touched
    b.reset()
    before = b.arena.buf.clone()
    with pytest.raises(capi.SwError) as err:
        ctx.scan_partition(kind, case.part, b.ptr("chars"), b.offsets.data_ptr(), b.lengths.data_ptr(), case.first_pos, case.n,
                           case.maxlen, -11, -1, b.ptr("scores"), b.ptr("ids"), 0, b.ptr("ovf_pos"), b.ptr("ovf_count"), 1,
                           b.ptr("temp"), one - 1, 0)
    assert err.value.code == -5
    torch.cuda.synchronize()
    assert torch.equal(b.arena.buf, before)


# ------------------------------------------------------------------------------------------------------------------ P3
P3_CASES = ["a-f16x2-q850-c3", "a-i16x2-q1500-c8", "a-f16x2-q1500-c1", "b-i16x2-q1530-c3", "c-f16x2-s4", "c-i16x2-s2",
            "d-f32-q850", "d-i32native-q1600", "e-f16x2", "e-i16x2", "e-f32", "e-i32native"]


def _dirty(rig, b, offer_max, like_kind):
    """another launch on the same scratch: a query of three stripes, subjects of 600 .. 900 residues, the other packed kind"""
    torch, capi = rig.torch, rig.capi
    d, dq = F.dirtier(), F.query(1530)
    dkind = 1 if like_kind == 0 else 0
    dctx = rig.context(dq, {})
    assert dctx.plan_launch(dkind, d.part, d.n, d.maxlen) == (dkind, 32, 3, 16)
    offer = min(offer_max, dctx.scan_temp_bytes(dkind, d.part, d.n, d.maxlen))
    dev = [rig.to_device(x) for x in (np.concatenate([d.chars, np.full(64, 20, np.int8)]), d.offsets.view(np.int64), d.lengths)]
    scores = torch.full((d.N,), -1.0, dtype=torch.float32, device=rig.device)
    ids = torch.full((d.N,), -1, dtype=torch.int32, device=rig.device)
    ovf = torch.zeros(d.N + 1, dtype=torch.int32, device=rig.device)
    dctx.scan_partition(dkind, d.part, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d.first_pos, d.n, d.maxlen, -11, -1,
                        scores.data_ptr(), ids.data_ptr(), 0, ovf[1:].data_ptr(), ovf.data_ptr(), 1, b.ptr("temp"), offer, 0)
    b.intact(offer, "the dirtying launch")
    flagged = ovf[1:1 + int(ovf[0])].cpu().numpy()
    ok = np.ones(d.N, dtype=bool)
    ok[: d.first_pos] = ok[d.first_pos + d.n:] = False
    ok[flagged] = False
    np.testing.assert_array_equal(scores.cpu().numpy()[ok], d.expect(dq)[ok], err_msg="the dirtying launch")
    assert b.arena.high_water("temp") > 0


def _dirty_need(rig, kind):
    d = F.dirtier()
    return rig.context(F.query(1530), {}).scan_temp_bytes(1 if kind == 0 else 0, d.part, d.n, d.maxlen)


@pytest.mark.parametrize("name", P3_CASES)
def test_p3_stale_scratch(rig, name):
    kind = KIND[SCENARIOS[name]["kind"]]
    sc, case, q, kind, ctx, need, b = _open(rig, name, _canary(name + "p3"), extra_guard=_dirty_need(rig, kind))
    streamed = sc.get("streamed", False)
    runs = [_scan(b, ctx, kind, need, "%s, scratch of 0x%02X" % (name, fill), prefill=fill, streamed=streamed) for fill in PREFILLS]
    b.reset()
    _dirty(rig, b, need, kind)
    runs.append(_scan(b, ctx, kind, need, name + ", scratch as another launch left it", keep_temp=True, streamed=streamed))
    for final, flagged in runs[1:]:     # (each equals the oracle already: _scan)
        np.testing.assert_array_equal(final, runs[0][0])
        np.testing.assert_array_equal(flagged, runs[0][1])


# ------------------------------------------------------------------------------------------------------------------ P4
P4_CASES = [("a-f16x2-q850-c1", 400), ("a-i16x2-q1500-c1", 400), ("a-f16x2-q850-c1", 401), ("a-f16x2-q850-c3", 400), ("a-i16x2-q1500-c3", 400),
            ("d-f32-q850", 400), ("d-i32native-q1600", 400), ("c-f16x2-s4", 200),
            ("e-f16x2", 1400), ("e-i16x2", 1400), ("e-f32", 1400), ("e-i32native", 1400)]


@pytest.mark.parametrize("name,bound", P4_CASES)
def test_p4_under_reported_bound_cuts_at_the_bound(rig, name, bound):
    """the scratch is sized for `bound`, the arena's guards for the true longest subject; a subject no longer than the bound
    scores exactly, a longer one what the oracle gives for its first `bound` residues (rounded up to a whole letter word) —
    in a launch that walks chains of pairs too: a pair is placed by its cut length, its chain neighbours keep their scores"""
    sc, case, q, kind, ctx, need, b = _open(rig, name, _canary(name + "p4"), bound=bound)
    assert bound < case.maxlen and (bound == 401 or bound == case.bound)
    offer = ctx.scan_temp_bytes(kind, case.part, case.n, bound)
    streamed = sc.get("streamed", False)     # (a streamed launch's scratch holds a round's columns whatever the bound)
    assert 0 < offer <= need and (streamed or offer < need) and b.arena.size["temp"] == offer and min(b.arena.guard_sizes("temp")) >= need
    over = case.lengths[case.range] > (bound + 3) // 4 * 4
    full, cut = case.expect(q)[case.range], case.expect(q, bound=bound)[case.range]
    # the cut is visible: it changes the score of at least half of the longer subjects (the streamed DB's pieces of the
    # query lie anywhere in a subject: at least three)
    changed = int((cut[over] != full[over]).sum())
    assert over.sum() >= 3 and changed >= (3 if streamed else (over.sum() + 1) // 2) and (cut[~over] == full[~over]).all()
    _scan(b, ctx, kind, offer, "%s, bound %d" % (name, bound), bound=bound, streamed=streamed)   # (asserts the cut scores)


# ------------------------------------------------------------------------------------------------------------------ (f)
def _rescore(b, ctx, kind, count, what, stat=False, prefill=None, keep_temp=False, id_offset=0):
    torch, capi, case = b.rig.torch, b.rig.capi, b.case
    need = b.arena.size["temp"]
    b.reset(keep_temp)
    if prefill is not None:
        b.arena.slice("temp")[:] = prefill
    args = (kind, b.ptr("ovf_pos"), b.ptr("ovf_count"), F.LIST_CAPACITY, b.ptr("chars"), b.offsets.data_ptr(), b.lengths.data_ptr(),
            case.maxlen, -11, -1, b.ptr("scores"), b.ptr("ids"), id_offset, b.ptr("temp"), need)
    if stat:
        ctx.rescore_overflow_stat(*args, 300, b.ptr("stat"), 0)
    else:
        ctx.rescore_overflow(*args, 0)
    b.intact(need, what)
    pos = b.list[0][:count]
    expect = case.expect(b.q)
    want_scores, want_ids = np.full(case.N, S, dtype=np.int64), np.full(case.N, S, dtype=np.int64)
    want_scores[pos], want_ids[pos] = expect[pos], id_offset + pos
    np.testing.assert_array_equal(b.host("scores", np.float32).astype(np.int64), want_scores, err_msg=what)
    np.testing.assert_array_equal(b.host("ids", np.int32), want_ids, err_msg=what)
    np.testing.assert_array_equal(b.host("ovf_pos", np.int32), b.list[0], err_msg=what + ": the list")
    assert int(b.host("ovf_count", np.int32)[0]) == count
    assert int(b.host("stat", np.int32)[0]) == 5 + (int((expect[pos] >= 300).sum()) if stat else 0), what
    return b.host("scores", np.float32)


@pytest.mark.parametrize("kind_name,env", [("f32", {}), ("i32", dict(I32_NATIVE=1))])
@pytest.mark.parametrize("count", [0, 1, 37])
def test_rescore_lists_footprint_and_stale_scratch(rig, kind_name, env, count):
    kind, q = KIND[kind_name], F.query(850)
    case, pos = F.listed(850, count)
    ctx = rig.context(q, env)
    assert case.maxlen == 8200 and ctx.plan_launch(kind, -1, F.LIST_CAPACITY, case.maxlen) == (kind, 7, 2, 64)
    need = ctx.scan_temp_bytes(kind, -1, F.LIST_CAPACITY, case.maxlen)
    assert need == (F.LIST_CAPACITY // 4) * F.region_bytes(case.maxlen, 64)
    b = Bench(rig, case, _canary(kind_name + str(count)), need, max(need, _dirty_need(rig, 0)), list_capacity=F.LIST_CAPACITY)
    b.q, b.list = q, (pos, count)
    if count:
        assert (case.expect(q)[pos[:count]] >= 300).sum() >= 1
    ref = _rescore(b, ctx, kind, count, "list of %d, %s" % (count, kind_name), id_offset=1000 * (count == 37))
    print("list of %d, %s: need %d bytes, last byte written %d" % (count, kind_name, need, b.arena.high_water("temp")))
    for fill in PREFILLS:
        got = _rescore(b, ctx, kind, count, "list of %d, %s, _stat, scratch of 0x%02X" % (count, kind_name, fill), stat=True, prefill=fill,
                       id_offset=1000 * (count == 37))
        np.testing.assert_array_equal(got, ref)
    b.reset()
    _dirty(rig, b, need, 0)
    got = _rescore(b, ctx, kind, count, "list of %d, %s, scratch as another launch left it" % (count, kind_name), keep_temp=True,
                   id_offset=1000 * (count == 37))
    np.testing.assert_array_equal(got, ref)


# ------------------------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("lanes,qlen,env", [(8, 200, dict(LANES8_MAX_Q=256, LANES4_MAX_Q=0)), (4, 100, dict(LANES4_MAX_Q=128))])
@pytest.mark.parametrize("temp_null", [True, False])
def test_single_stripe_queries_touch_no_scratch(rig, lanes, qlen, env, temp_null):
    case, q, kind = F.ragged(200, planted=False), F.query(qlen), KIND["f16x2"]
    ctx = rig.context(q, env)
    assert ctx.plan_launch(kind, case.part, case.n, case.maxlen) == (kind, 25, 1, lanes)
    assert ctx.scan_temp_bytes(kind, case.part, case.n, case.maxlen) == 0
    # (guards as large as the scratch of a two-stripe query on this DB)
    b = Bench(rig, case, F.CANARIES[lanes == 4], 0, rig.context(F.query(850), {}).scan_temp_bytes(kind, case.part, case.n, case.maxlen))
    b.q = q
    assert b.arena.size["temp"] == 0
    _scan(b, ctx, kind, 0, "%d-lane groups, temp %s" % (lanes, "NULL" if temp_null else "of 0 bytes inside the arena"), temp_null=temp_null,
          id_offset=77)
